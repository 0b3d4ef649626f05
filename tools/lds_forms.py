"""Static census of the LDS instruction forms of one kernel, from a unit's -S output:
the count of each ds_* form, how many of the two-address forms (ds_read2_b64,
ds_write2_b64, ...) address adjacent elements (offset1 = offset0 + 1: one contiguous
piece the compiler could not prove aligned), and the LDS-array cycles the forms add up
to by the per-form costs below (wave64, conflict-free).  Static counts: a loop body
counts once, so this says what the kernel is made of, not what a wave executes.

    python tools/lds_forms.py unit.s [kernel-substring] [--cycles form=N ...]

The costs are the LDS cycles per wave-instruction of the MI355X (reads: two 32-lane
groups for 4- and 8-byte reads, four 16-lane groups for 16-byte reads, a two-address
read as two accesses of four groups each; stores: the transfer of their address and
data registers, 2 cycles per dword and more for the 16-byte ones, which exceeds their
array cycles); tools/lds_read_forms_check.hip
measures the three 16-byte read forms on the box, and --cycles overrides an entry.
"""
import re
import sys
from collections import Counter

# LDS-array cycles per wave-instruction; a form not listed counts DEFAULT
CYCLES = {
    "ds_read_b32": 2, "ds_read_b64": 2, "ds_read_b96": 8, "ds_read_b128": 4,
    "ds_read2_b32": 4, "ds_read2_b64": 8, "ds_read2st64_b32": 4, "ds_read2st64_b64": 8,
    "ds_read_u8": 2, "ds_read_i8": 2, "ds_read_u16": 2, "ds_read_i16": 2,
    "ds_write_b8": 4, "ds_write_b16": 4, "ds_write_b32": 4, "ds_write_b64": 6,
    "ds_write_b96": 10, "ds_write_b128": 13, "ds_write2_b32": 6, "ds_write2_b64": 13,
    "ds_write2st64_b32": 6, "ds_write2st64_b64": 13,
    "ds_bpermute_b32": 2, "ds_permute_b32": 2, "ds_swizzle_b32": 2,
}
DEFAULT = 2
TWO = re.compile(r"^ds_(read|write)2(st64)?_b(32|64)$")
OFF0 = re.compile(r"offset0:(\d+)")
OFF1 = re.compile(r"offset1:(\d+)")


def kernel_body(lines, pat):
    """The instruction lines of the first kernel whose mangled name holds `pat`."""
    start = next(i for i, ln in enumerate(lines) if ln.startswith("_Z") and ":" in ln and pat in ln.split(":")[0])
    end = next(i for i in range(start + 1, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    return lines[start].split(":")[0], [ln.strip() for ln in lines[start + 1:end]]


def is_adjacent(ln):
    """A two-address form whose offsets are neighbours (a missing offset is 0)."""
    m0, m1 = OFF0.search(ln), OFF1.search(ln)
    return (int(m1.group(1)) if m1 else 0) - (int(m0.group(1)) if m0 else 0) == 1


def census(body):
    """(Counter of ds_* forms, Counter of adjacent two-address forms) of instruction lines."""
    forms, adjacent = Counter(), Counter()
    for ln in body:
        if not ln.startswith("ds_"):
            continue
        op = ln.split()[0]
        forms[op] += 1
        if TWO.match(op) and is_adjacent(ln):
            adjacent[op] += 1
    return forms, adjacent


def array_cycles(forms, cycles=CYCLES):
    return sum(n * cycles.get(op, DEFAULT) for op, n in forms.items())


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--") and "=" not in a]
    cycles = dict(CYCLES)
    for kv in (a for a in sys.argv[1:] if "=" in a):      # the form=N entries behind --cycles
        k, v = kv.split("=")
        cycles[k] = float(v)
    path = args[0]
    pat = args[1] if len(args) > 1 else "k_mpc_step"
    name, body = kernel_body(open(path).read().split("\n"), pat)
    insts = sum(1 for ln in body if ln and not ln.startswith((";", ".")) and not ln.endswith(":"))
    forms, adjacent = census(body)
    total = array_cycles(forms, cycles)
    print(f"{name}: {insts} instructions, {sum(forms.values())} LDS")
    print(f"{'form':22s} {'count':>6s} {'adjacent':>9s} {'cyc each':>9s} {'cycles':>8s} {'share':>6s}")
    for op, n in sorted(forms.items(), key=lambda kv: -kv[1] * cycles.get(kv[0], DEFAULT)):
        c = cycles.get(op, DEFAULT)
        adj = f"{adjacent[op]:9d}" if TWO.match(op) else f"{'':9s}"
        print(f"{op:22s} {n:6d} {adj} {c:9g} {n * c:8g} {100.0 * n * c / max(total, 1):5.1f}%")
    print(f"{'LDS-array cycles':22s} {'':6s} {'':9s} {'':9s} {total:8g}")


if __name__ == "__main__":
    main()
