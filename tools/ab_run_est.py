#!/usr/bin/env python
"""Cost of the output-feedback closed loop: ntm_mpc_run_est with the degenerate options
(sigma_y = 0, kappa = 0, equal gains, xhat0 = NULL: the same loop) against
ntm_mpc_run_obs of the same library, on one box.  Both keep the whole loop in one
launch, so a window of steps is the difference of two launches: ms per step-batch over
steps W+1 .. W+K = (t(k_sim = W + K) - t(k_sim = W)) / K, device events around each
launch, every output array written (preallocated once), R alternating runs of each side
from the same initial states.

    python tools/ab_run_est.py [--batch 100000] [--N 20] [--mode 2] [--steps 20] [--warmup 5]
                               [--runs 3] [--out FILE.json]

Prints one JSON object: ms per step-batch of every run, each side's mean and spread
(max - min over its runs), the difference of the means, and whether the last step's
outputs (x, u, U, w_pred, d_hat, flags, iteration counts) of the two sides are
bit-identical, with x_hat equal to x.
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "mpc-ntm-control_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

KEYS = ("xk", "uk", "Uk", "wpred", "dk", "exitflag", "inner_iters")


def buffers(ctl, N, B, k):
    import torch
    i32 = dict(dtype=torch.int32)
    return {"xk": ctl._empty(2 * (k + 1), B), "uk": ctl._empty(k, B), "Uk": ctl._empty(N * k, B),
            "wpred": ctl._empty((N + 1) * k, B), "dk": ctl._empty(2 * (k + 1), B), "xhk": ctl._empty(2 * (k + 1), B),
            "yk": ctl._empty(2 * k, B), "exitflag": ctl._empty(k, B, **i32), "inner_iters": ctl._empty(k, B, **i32)}


def launch(ctl, cfg, x0, k, side, o, gain):
    from ntm_mpc import Estimator, Observer
    from ntm_mpc.api import _ptr
    B = x0.shape[1]
    head = (ctl._ctx, C.byref(ctl.physics.to_c()), C.byref(cfg.to_c()))
    if side == "obs":
        rc = ctl.lib.ntm_mpc_run_obs_device(*head, C.byref(Observer(False, gain).to_c()), B, k, _ptr(x0), None,
                                            _ptr(o["xk"]), _ptr(o["uk"]), _ptr(o["Uk"]), _ptr(o["wpred"]),
                                            _ptr(o["dk"]), _ptr(o["exitflag"]), _ptr(o["inner_iters"]), ctl._stream())
    else:
        rc = ctl.lib.ntm_mpc_run_est_device(*head, C.byref(Estimator(False, gain, 0.0, 0.0).to_c()), B, k, _ptr(x0),
                                            None, None, _ptr(o["xk"]), _ptr(o["uk"]), _ptr(o["Uk"]), _ptr(o["wpred"]),
                                            _ptr(o["dk"]), _ptr(o["xhk"]), _ptr(o["yk"]), _ptr(o["exitflag"]),
                                            _ptr(o["inner_iters"]), ctl._stream())
    ctl._raise(rc, "run_" + side)


def timed(ctl, cfg, x0, k, side, o, gain):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    launch(ctl, cfg, x0, k, side, o, gain)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--mode", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--gain", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ntm_mpc import Config, NtmMpc, scenarios_x0
    ctl = NtmMpc(device=0)
    cfg = Config(N=a.N, mode=a.mode)
    x0 = ctl.tensor(scenarios_x0(0, a.batch))
    W, K = a.warmup, a.steps
    short = {s: buffers(ctl, a.N, a.batch, W) for s in ("obs", "est")}
    full = {s: buffers(ctl, a.N, a.batch, W + K) for s in ("obs", "est")}
    for side in ("obs", "est"):                                   # untimed: module load
        launch(ctl, cfg, x0, 1, side, full[side], a.gain)
    torch.cuda.synchronize()
    ms = {"obs": [], "est": []}
    raw = {"obs": [], "est": []}
    for _ in range(a.runs):
        for side in ("obs", "est"):
            t_w = timed(ctl, cfg, x0, W, side, short[side], a.gain)
            t_f = timed(ctl, cfg, x0, W + K, side, full[side], a.gain)
            raw[side].append([t_w, t_f])
            ms[side].append((t_f - t_w) / K)
    same = all(bool(torch.equal(full["obs"][k], full["est"][k])) for k in KEYS)
    same = same and bool(torch.equal(full["est"]["xhk"], full["est"]["xk"]))
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    res = {"batch": a.batch, "N": a.N, "mode": a.mode, "steps": K, "warmup": W, "gain": a.gain,
           "launch_ms_warmup_and_full": raw, "ms_per_step": ms, "mean": mean,
           "spread": {k: max(v) - min(v) for k, v in ms.items()},
           "est_minus_obs_ms": mean["est"] - mean["obs"], "est_over_obs": mean["est"] / mean["obs"],
           "outputs_bitwise_equal": same}
    ctl.close()
    line = json.dumps(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
