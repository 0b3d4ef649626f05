#!/usr/bin/env python
"""Cost of the actuator dead time in the closed loop: ntm_mpc_run_dly at several delays
against ntm_mpc_run_est of the same library, on one box.  Every side keeps the whole loop
in one launch, so a window of steps is the difference of two launches: ms per step-batch
over steps W+1 .. W+K = (t(k_sim = W + K) - t(k_sim = W)) / K, device events around each
launch, every output array written (preallocated once), R alternating runs of each side
from the same initial states (degenerate estimator options, a zero queue, predict = 1; a
delay written "3n" runs with predict = 0).

    python tools/ab_run_dly.py [--batch 100000] [--N 20] [--mode 2] [--steps 20] [--warmup 5]
                               [--runs 3] [--delays 0,3,3n,8] [--out FILE.json]

Prints one JSON object: ms per step-batch of every run, each side's mean and spread (max -
min over its runs), each delay's difference to run_est, each side's mean LPV iterations per
step and fraction of optimal QPs over the timed window (the sides follow different
trajectories), and whether run_dly at d = 0 gave run_est's outputs bit for bit.
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

KEYS = ("xk", "uk", "Uk", "wpred", "dk", "xhk", "yk", "exitflag", "inner_iters")


def buffers(ctl, N, B, k):
    import torch
    i32 = dict(dtype=torch.int32)
    return {"xk": ctl._empty(2 * (k + 1), B), "uk": ctl._empty(k, B), "Uk": ctl._empty(N * k, B),
            "wpred": ctl._empty((N + 1) * k, B), "dk": ctl._empty(2 * (k + 1), B), "xhk": ctl._empty(2 * (k + 1), B),
            "yk": ctl._empty(2 * k, B), "uak": ctl._empty(k, B), "xpk": ctl._empty(2 * k, B),
            "exitflag": ctl._empty(k, B, **i32), "inner_iters": ctl._empty(k, B, **i32)}


def launch(ctl, cfg, x0, k, side, o, gain):
    from ntm_mpc import Delay, Estimator
    from ntm_mpc.api import _ptr
    B = x0.shape[1]
    head = (ctl._ctx, C.byref(ctl.physics.to_c()), C.byref(cfg.to_c()), C.byref(Estimator(False, gain, 0.0, 0.0).to_c()))
    if side == "est":
        rc = ctl.lib.ntm_mpc_run_est_device(*head, B, k, _ptr(x0), None, None, _ptr(o["xk"]), _ptr(o["uk"]),
                                            _ptr(o["Uk"]), _ptr(o["wpred"]), _ptr(o["dk"]), _ptr(o["xhk"]),
                                            _ptr(o["yk"]), _ptr(o["exitflag"]), _ptr(o["inner_iters"]), ctl._stream())
    else:
        dly = Delay(int(side[1:].rstrip("n")), not side.endswith("n"))
        rc = ctl.lib.ntm_mpc_run_dly_device(*head, C.byref(dly.to_c()), B, k, _ptr(x0), None, None, None, _ptr(o["xk"]), _ptr(o["uk"]), _ptr(o["Uk"]), _ptr(o["wpred"]),
                                            _ptr(o["dk"]), _ptr(o["xhk"]), _ptr(o["yk"]), _ptr(o["uak"]),
                                            _ptr(o["xpk"]), _ptr(o["exitflag"]), _ptr(o["inner_iters"]), ctl._stream())
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
    ap.add_argument("--delays", default="0,3,3n,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ntm_mpc import Config, NtmMpc, scenarios_x0
    ctl = NtmMpc(device=0)
    cfg = Config(N=a.N, mode=a.mode)
    x0 = ctl.tensor(scenarios_x0(0, a.batch))
    W, K = a.warmup, a.steps
    sides = ["est"] + ["d" + d for d in a.delays.split(",")]
    short = {s: buffers(ctl, a.N, a.batch, W) for s in sides}
    full = {s: buffers(ctl, a.N, a.batch, W + K) for s in sides}
    for side in sides:                                            # untimed: module load
        launch(ctl, cfg, x0, 1, side, full[side], a.gain)
    torch.cuda.synchronize()
    ms = {s: [] for s in sides}
    raw = {s: [] for s in sides}
    for _ in range(a.runs):
        for side in sides:
            t_w = timed(ctl, cfg, x0, W, side, short[side], a.gain)
            t_f = timed(ctl, cfg, x0, W + K, side, full[side], a.gain)
            raw[side].append([t_w, t_f])
            ms[side].append((t_f - t_w) / K)
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    res = {"batch": a.batch, "N": a.N, "mode": a.mode, "steps": K, "warmup": W, "gain": a.gain,
           "launch_ms_warmup_and_full": raw, "ms_per_step": ms, "mean": mean,
           "spread": {k: max(v) - min(v) for k, v in ms.items()},
           "minus_est_ms": {s: mean[s] - mean["est"] for s in sides if s != "est"},
           "window_optimal_fraction": {s: float((full[s]["exitflag"][W:] == 1).double().mean()) for s in sides},
           "window_mean_inner_iters": {s: float(full[s]["inner_iters"][W:].double().mean()) for s in sides}}
    if "d0" in full:
        res["d0_outputs_bitwise_equal_to_run_est"] = all(bool(torch.equal(full["est"][k], full["d0"][k])) for k in KEYS)
    ctl.close()
    line = json.dumps(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
