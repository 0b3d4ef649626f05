#!/usr/bin/env python
"""Cost of the observer entry point: ntm_mpc_step_obs with the degenerate options
(nominal_model = 0, gain = 0, d_hat = 0: the same step) against ntm_mpc_step_dual, the
other runtime-N sibling, on one box.  The project's A/B protocol: the closed loop
through the step entry point, W untimed steps then K timed ones (device events around
each launch), R alternating runs of each side from the same initial states.

    python tools/ab_step_obs.py [--batch 100000] [--N 20] [--mode 2] [--steps 20] [--warmup 5]
                                [--runs 3] [--out FILE.json]

Prints one JSON object: ms per step-batch of every run, each side's mean and spread
(max - min over its runs), the difference of the means, and whether the last timed
step's U, x_next and exit flags of the two sides are bit-identical.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "mpc-ntm-control_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def one_run(ctl, cfg, x0, K, W, side):
    import numpy as np
    import torch
    from ntm_mpc import Observer
    B = x0.shape[1]
    rho, U_old = ctl.initial_state(x0, cfg)
    ws = ctl.new_active_ws(B, cfg)
    d = ctl.tensor(np.zeros((2, B)))
    obs = Observer(nominal_model=False, gain=0.0)

    def step(x):
        if side == "obs":
            return ctl.step_obs(x, rho, U_old, d, obs, cfg, active_ws=ws)
        return ctl.step_dual(x, rho, U_old, cfg, active_ws=ws)

    x = x0
    for _ in range(W):
        x = step(x)["x_next"]
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(K)]
    torch.cuda.synchronize()
    for i in range(K):
        ev[i][0].record()
        out = step(x)
        ev[i][1].record()
        x = out["x_next"]
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev) / K, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--mode", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ntm_mpc import Config, NtmMpc, scenarios_x0
    ctl = NtmMpc(device=0)
    cfg = Config(N=a.N, mode=a.mode)
    x0 = ctl.tensor(scenarios_x0(0, a.batch))
    ms = {"dual": [], "obs": []}
    last = {}
    one_run(ctl, cfg, x0, 2, 1, "dual")                          # untimed: module load, buffers
    one_run(ctl, cfg, x0, 2, 1, "obs")
    for _ in range(a.runs):
        for side in ("dual", "obs"):
            t, out = one_run(ctl, cfg, x0, a.steps, a.warmup, side)
            ms[side].append(t)
            last[side] = out
    same = all(bool(torch.equal(last["dual"][k], last["obs"][k])) for k in ("U", "x_next", "exitflag", "inner_iters"))
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    res = {"batch": a.batch, "N": a.N, "mode": a.mode, "steps": a.steps, "warmup": a.warmup,
           "ms_per_step": ms, "mean": mean, "spread": {k: max(v) - min(v) for k, v in ms.items()},
           "obs_minus_dual_ms": mean["obs"] - mean["dual"], "obs_over_dual": mean["obs"] / mean["dual"],
           "last_step_bitwise_equal": same}
    ctl.close()
    line = json.dumps(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
