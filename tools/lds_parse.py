"""Reduce the LDS passes of tools/prof_lds.sh (lds1 + lds2 counter CSVs) to the last
k_mpc_step dispatch and write lds_<tag>.json: the LDS pipe's share of a CU's cycles
next to the VALU's share of a SIMD's, and the bank-conflict share of the LDS cycles.

Units.  SQ_WAVE_CYCLES, SQ_WAIT_* and SQ_ACTIVE_INST_* count quad-cycles per wave;
SQ_LDS_IDX_ACTIVE and SQ_LDS_BANK_CONFLICT count LDS-array cycles.  A wave lives
SQ_WAVE_CYCLES x 4 cycles; with `wpc` waves resident per CU the CU is busy for the
waves' summed life over wpc, so
    LDS-array cycles per CU cycle = wpc x SQ_LDS_IDX_ACTIVE / (4 SQ_WAVE_CYCLES)
    VALU busy share of a SIMD     = (wpc / 4) x SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES
(both per wave or per launch: the ratio is the same).  Both assume full residency for
the whole launch, which the tail of the last waves falls short of by a few percent.
"""
import collections
import csv
import json
import sys
from pathlib import Path

outdir, tag = Path(sys.argv[1]), sys.argv[2]
wpc = int(sys.argv[3]) if len(sys.argv) > 3 else 16      # the slim far N = 20 kernels: 16 waves per CU


def last_step(path):
    d = collections.defaultdict(lambda: collections.defaultdict(float))
    for r in csv.DictReader(open(path)):
        if "k_mpc_step" not in r["Kernel_Name"]:
            continue
        d[int(r["Dispatch_Id"])][r["Counter_Name"]] += float(r["Counter_Value"])
    return d[max(d)] if d else {}


def ratio(a, b):
    return a / b if b else None


c = {}
for f in sorted(outdir.rglob("lds*_counter_collection.csv")):
    c.update(last_step(f))
waves = c.get("SQ_WAVES", 0.0)
wc = c.get("SQ_WAVE_CYCLES", 0.0)
idx = c.get("SQ_LDS_IDX_ACTIVE", 0.0)
lds_share = ratio(wpc * idx, 4.0 * wc)
valu_share = ratio(wpc / 4.0 * c.get("SQ_ACTIVE_INST_VALU", 0.0), wc)
res = {
    "round": tag,
    "kernel": "k_mpc_step<64,20>",
    "counters_per_launch": dict(sorted(c.items())),
    "per_wave": {k: v / waves for k, v in sorted(c.items()) if waves and k != "SQ_WAVES"},
    "derived": {
        "waves_per_cu": wpc,
        "lds_array_cycles_per_cu_cycle": lds_share,
        "lds_inst_active_per_cu_cycle": ratio(wpc * c.get("SQ_ACTIVE_INST_LDS", 0.0), wc),
        "lds_array_cycles_per_lds_inst": ratio(idx, c.get("SQ_INSTS_LDS", 0.0)),
        "bank_conflict_share_of_lds_array_cycles": ratio(c.get("SQ_LDS_BANK_CONFLICT", 0.0), idx),
        "lds_issue_stall_frac_of_wave_cycles": ratio(c.get("SQ_WAIT_INST_LDS", 0.0), wc),
        "simd_valu_busy_estimate": valu_share,
        "lds_share_over_valu_share": ratio(lds_share, valu_share) if lds_share is not None else None,
    },
    "note": "separate --pmc passes over one bench step at B=1e5, N=20; shares assume full residency "
            "(waves_per_cu) for the whole launch.",
}
(outdir / f"lds_{tag}.json").write_text(json.dumps(res, indent=1) + "\n")
print(json.dumps(res["derived"], indent=1))
