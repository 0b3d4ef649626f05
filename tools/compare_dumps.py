#!/usr/bin/env python3
"""Byte comparison of two `bench.py --dump-outputs` directories and of the two runs'
`solver` entries (the record format of profiles/r07_ab/bitwise.txt).  Diagnostic only.

    python tools/compare_dumps.py <tag> <dirA> <dirB> <a.json> <b.json> [<tag> ...]

Prints one line per array and per solver entry, then ALL IDENTICAL or DIFFERENT
(exit status 1)."""
import json
import sys
from pathlib import Path

import numpy as np

bad = 0
args = sys.argv[1:]
assert args and len(args) % 5 == 0, __doc__
for tag, da, db, ja, jb in (args[i:i + 5] for i in range(0, len(args), 5)):
    names = sorted(p.name for p in Path(da).glob("*.npy"))
    if names != sorted(p.name for p in Path(db).glob("*.npy")) or not names:
        print(f"{tag} file lists differ: {names} / {sorted(p.name for p in Path(db).glob('*.npy'))}")
        bad += 1
        continue
    for n in names:
        a, b = np.load(Path(da) / n), np.load(Path(db) / n)
        same = a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
        note = "array-equal (bytes)"
        if not same:
            bad += 1
            note = "DIFFERENT"
            if a.shape == b.shape:
                ne = (a != b) & ~(np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a != b
                cols = np.unique(np.nonzero(np.atleast_2d(ne))[-1])
                note += f": {int(ne.sum())} entries unequal as numbers in {cols.size} scenarios (first {cols[:5].tolist()})"
                if a.dtype.kind == "f" and not ne.any():
                    note += "; equal as numbers (signed zeros or NaN payloads)"
        print(f"{tag} {n} shape {a.shape} {note}")
    sa, sb = (json.loads(Path(p).read_text().strip().splitlines()[-1])["solver"] for p in (ja, jb))
    if sa == sb:
        print(f"{tag} solver entries identical: {json.dumps(sa)}")
    else:
        bad += 1
        print(f"{tag} solver entries DIFFERENT: {json.dumps(sa)} / {json.dumps(sb)}")
print("DIFFERENT" if bad else "ALL IDENTICAL")
sys.exit(1 if bad else 0)
