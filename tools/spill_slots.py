#!/usr/bin/env python3
"""Static recount of SGPR-spill traffic in a device assembly file (hipcc -S output).

    ASM_DIR=dir bash tools/asm_digest.sh ntm_n20      # writes dir/ntm_n20.s
    python tools/spill_slots.py dir/ntm_n20.s [--kernel SUBSTR] [--top N]

Per kernel: the static VALU count, v_readlane_b32 in all and from the VGPRs the
allocator spills SGPRs into (the assembly marks them "SGPR spill to VGPR lane"),
v_writelane_b32 into them, the number of lanes (slots) in use, the resources from
the compiler's metadata, and the slot histogram: lanes grouped into the runs that
are restored together (consecutive lanes with equal restore counts), most restored
first.  A restore site is one v_readlane_b32 of a lane; a tuple of eight dwords
restored whole shows as one run of eight lanes.  CPU only.
"""
import argparse
import collections
import re
import sys

KERNEL = re.compile(r"^(_Z\w+):\s*; @")
END = re.compile(r"^\.Lfunc_end\d+:")
SPILLREG = re.compile(r"implicit-def: \$vgpr(\d+) : SGPR spill to VGPR lane")
RDL = re.compile(r"^\s+v_readlane_b32 (s\d+|vcc_lo|vcc_hi|exec_lo|exec_hi|m0), v(\d+), (\S+)")
WRL = re.compile(r"^\s+v_writelane_b32 v(\d+), (\S+), (\S+)")
META = re.compile(r"^; (codeLenInByte|NumVgprs|NumSgprs|ScratchSize|Occupancy)\s*[:=]\s*(\d+)")
SPILLCNT = re.compile(r"^\s+\.(sgpr|vgpr)_spill_count:\s+(\d+)")
NAME = re.compile(r"^\s+\.name:\s+(\S+)")


def parse(path):
    kernels, cur, last = [], None, None
    spill_counts, name = {}, None
    for line in open(path):
        m = KERNEL.match(line)
        if m:
            cur = dict(name=m.group(1), valu=0, rdl=0, spill=set(), reads=[], writes=[], meta={})
            kernels.append(cur)
            last = cur
            continue
        if cur is not None:
            if END.match(line):
                cur = None
                continue
            m = SPILLREG.search(line)
            if m:
                cur["spill"].add(int(m.group(1)))
                continue
            s = line.lstrip()
            if s.startswith("v_"):
                cur["valu"] += 1
                m = RDL.match(line)
                if m:
                    cur["rdl"] += 1
                    cur["reads"].append((int(m.group(2)), m.group(3)))
                    continue
                m = WRL.match(line)
                if m:
                    cur["writes"].append((int(m.group(1)), m.group(3)))
            continue
        m = META.match(line)
        if m and last is not None and m.group(1) not in last["meta"]:
            last["meta"][m.group(1)] = int(m.group(2))
            continue
        m = NAME.match(line)
        if m:   # in a kernel's metadata map .name stands ahead of the two spill counts
            name = m.group(1)
            continue
        m = SPILLCNT.match(line)
        if m and name:
            spill_counts.setdefault(name, {})[m.group(1)] = int(m.group(2))
    for k in kernels:
        k["meta"].update({f"{a}_spill": b for a, b in spill_counts.get(k["name"], {}).items()})
    return kernels


def runs(hist):
    """[(vgpr, first lane, last lane, restores per lane)], consecutive lanes with equal counts merged."""
    out = []
    for (v, lane), n in sorted(hist.items()):
        if out and out[-1][0] == v and out[-1][2] == lane - 1 and out[-1][3] == n:
            out[-1][2] = lane
        else:
            out.append([v, lane, lane, n])
    return out


def report(k, top):
    sp = k["spill"]
    rd = collections.Counter((v, int(l)) for v, l in k["reads"] if v in sp and l.isdigit())
    wr = [(v, l) for v, l in k["writes"] if v in sp]
    slots = {(v, int(l)) for v, l in wr if l.isdigit()} | set(rd)
    nrd = sum(rd.values())
    print(k["name"])
    m = k["meta"]
    print("  resources: " + ", ".join(f"{a} {m[a]}" for a in
          ("NumVgprs", "vgpr_spill", "sgpr_spill", "ScratchSize", "codeLenInByte", "Occupancy") if a in m))
    print(f"  static VALU {k['valu']}, v_readlane_b32 {k['rdl']}, from the spill VGPRs "
          f"({', '.join('v%d' % v for v in sorted(sp)) or 'none'}) {nrd} "
          f"({100.0 * nrd / max(k['valu'], 1):.1f}% of VALU), v_writelane_b32 into them {len(wr)}, slots {len(slots)}")
    rr = sorted(runs(rd), key=lambda r: -(r[3] * (r[2] - r[1] + 1)))
    print("  slot histogram (lanes restored together; restores = sites x lanes):")
    for v, a, b, n in rr[:top]:
        lanes = f"{a}" if a == b else f"{a}-{b}"
        print(f"    v{v} lanes {lanes:7s} {n:3d} sites x {b - a + 1} = {n * (b - a + 1)}")
    if len(rr) > top:
        print(f"    ... {len(rr) - top} more runs, {sum(r[3] * (r[2] - r[1] + 1) for r in rr[top:])} restores")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="", help="only kernels whose mangled name contains this")
    ap.add_argument("--top", type=int, default=12, help="runs of the histogram to print")
    a = ap.parse_args()
    ks = [k for k in parse(a.asm) if a.kernel in k["name"]]
    if not ks:
        sys.exit("no kernel matched")
    for k in ks:
        report(k, a.top)


if __name__ == "__main__":
    main()
