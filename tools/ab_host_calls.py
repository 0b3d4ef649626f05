#!/usr/bin/env python
"""Host cost per call of the Python binding, this tree's ntm_mpc against another tree's (a
refactor of ntm_mpc/api.py against its parent commit) on the same library, on one box.
At N = 10, mode 0, B = 1 (BASELINE config 1) a launch is so short that the time the binding
spends marshalling is inside what bench.py measures around ctl.step.

    python tools/ab_host_calls.py ab --parent PARENT_TREE [--calls 2000] [--repeats 5] [--out FILE.json]
    python tools/ab_host_calls.py measure [--root TREE] [--calls 2000]

`measure` times, in one process, `calls` calls each of step (out= and active_ws= as bench.py
passes them), step_est and run_from(k_sim=1) between two synchronisations with perf_counter
(after 200 untimed calls) and prints microseconds per call as one JSON line; --root names the
tree whose package is imported.  `ab` runs `measure` in fresh processes, PARENT_TREE and this
tree alternating, `repeats` times each, both on this tree's library (NTM_MPC_LIB), and
prints one JSON object: every repeat, each side's median and spread (max - min), and per
entry whether the change's median exceeds the parent's by no more than the parent's spread.
"""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path
from statistics import median

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("step", "step_est", "run_from")


def measure(root, calls):
    for p in (str(root), str(Path(root) / "mpc-ntm-control_amd")):
        sys.path.insert(0, p)
    import torch
    from ntm_mpc import Config, Estimator, NtmMpc, scenarios_x0
    ctl = NtmMpc(device=0)
    cfg = Config(N=10, mode=0)
    est = Estimator(False, 0.5, 0.0, 0.0)
    x = ctl.tensor(scenarios_x0(0, 1))
    d_hat, x_hat = ctl.tensor([[0.0], [0.0]]), x.clone()
    rho, U_old = ctl.initial_state(x, cfg)
    ws = ctl.new_active_ws(1, cfg)
    outs = [None, None]

    def step(i):
        outs[i & 1] = ctl.step(x, rho, U_old, cfg, out=outs[i & 1], active_ws=ws)

    run = {"step": step, "step_est": lambda i: ctl.step_est(x, rho, U_old, d_hat, x_hat, est, cfg, active_ws=ws),
           "run_from": lambda i: ctl.run_from(x, rho, U_old, ws, 1, cfg)}
    us = {}
    for name in ENTRIES:
        for i in range(200):
            run[name](i)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(calls):
            run[name](i)
        torch.cuda.synchronize()
        us[name] = (time.perf_counter() - t) / calls * 1e6
    ctl.close()
    return us


def ab(parent, calls, repeats):
    env = dict(os.environ, NTM_MPC_LIB=os.environ.get("NTM_MPC_LIB", str(ROOT / "mpc-ntm-control_amd" / "lib" /
                                                                        "libntm_mpc.so")))
    runs = {"parent": [], "change": []}
    for _ in range(repeats):
        for side, root in (("parent", parent), ("change", ROOT)):
            p = subprocess.run([sys.executable, __file__, "measure", "--root", str(root), "--calls", str(calls)],
                               env=env, capture_output=True, text=True, timeout=300)
            if p.returncode:
                raise SystemExit(f"{side}: measure failed ({p.returncode})\n{p.stderr}")
            runs[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
    res = {"calls": calls, "repeats": repeats, "N": 10, "mode": 0, "batch": 1,
           "library": os.path.relpath(env["NTM_MPC_LIB"], ROOT), "us_per_call": runs, "median": {}, "spread": {}, "within_parent_spread": {}}
    for name in ENTRIES:
        v = {s: [r[name] for r in runs[s]] for s in runs}
        res["median"][name] = {s: median(v[s]) for s in v}
        res["spread"][name] = {s: max(v[s]) - min(v[s]) for s in v}
        res["within_parent_spread"][name] = (res["median"][name]["change"] - res["median"][name]["parent"]
                                             <= res["spread"][name]["parent"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=("measure", "ab"))
    ap.add_argument("--root", default=str(ROOT))
    ap.add_argument("--parent", default=None)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.cmd == "measure":
        print(json.dumps(measure(a.root, a.calls)))
        return 0
    if not a.parent:
        ap.error("ab needs --parent")
    line = json.dumps(ab(a.parent, a.calls, a.repeats))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
