#!/usr/bin/env python
"""Cost of the resumable closed loop: ntm_mpc_run_from in one call and as 4 x 5 steps
against ntm_mpc_run of the same library and ntm_mpc_run of a library built from the parent
commit (--parent-lib), on one box, in one process, alternating.

    python tools/ab_run_from.py --parent-lib PATH/libntm_mpc.so [--batch 100000] [--N 20]
                                [--mode 2] [--steps 20] [--warmup 5] [--chunks 4] [--runs 3]
                                [--out FILE.json]

ms per step-batch over steps W+1 .. W+K, device events around the launches, every output
array written (preallocated once), R alternating runs of each side from the same x0:
  run, run_parent   (t(k_sim = W + K) - t(k_sim = W)) / K, as tools/ab_run_est.py;
  from_1            W steps by run_from (untimed), then one timed run_from(K) / K;
  from_chunks       W steps by run_from (untimed), then --chunks timed run_from(K / chunks)
                    calls, one pair of events around all of them, / K;
  from_diff         run_from from the init state measured as run is: (t(W + K) - t(W)) / K,
                    the kernel's rate per step with each call's fixed cost subtracted away.
The two run_from sides pay their state traffic (4N doubles + 2(N+1) ints in and out per
scenario per call) inside the timed window; run's window subtracts its set-up away.

Prints one JSON object: every run's figure, each side's mean and spread (max - min), the
differences to the parent's run, the largest same-build spread and 3x it (the project's
threshold for a difference that counts), and whether the four sides' outputs over the
window are bit-identical.
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

KEYS = ("xk", "uk", "Uk", "wpred", "exitflag", "inner_iters")


def buffers(ctl, N, B, k):
    import torch
    i32 = dict(dtype=torch.int32)
    return {"xk": ctl._empty(2 * (k + 1), B), "uk": ctl._empty(k, B), "Uk": ctl._empty(N * k, B),
            "wpred": ctl._empty((N + 1) * k, B), "exitflag": ctl._empty(k, B, **i32),
            "inner_iters": ctl._empty(k, B, **i32)}


class ParentLib:
    """ntm_mpc_run_device of another build of the library, on a context of its own."""

    def __init__(self, path, device):
        from ntm_mpc import _lib as L
        self.lib = C.CDLL(str(path))
        for name in ("ntm_ctx_create", "ntm_ctx_destroy", "ntm_last_error", "ntm_mpc_run_device"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = L.EXPORTS[name]
        self.ctx = C.c_void_p()
        assert self.lib.ntm_ctx_create(C.byref(self.ctx), device) == 0

    def close(self):
        self.lib.ntm_ctx_destroy(self.ctx)


def run(lib, ctx, ctl, cfg, x0, k, o):
    from ntm_mpc.api import _ptr
    rc = lib.ntm_mpc_run_device(ctx, C.byref(ctl.physics.to_c()), C.byref(cfg.to_c()), x0.shape[1], k, _ptr(x0),
                                *[_ptr(o[key]) for key in KEYS], ctl._stream())
    assert rc == 0, lib.ntm_last_error(ctx)


def run_from(ctl, cfg, state, k, o):
    from ntm_mpc.api import _ptr
    rc = ctl.lib.ntm_mpc_run_from_device(ctl._ctx, C.byref(ctl.physics.to_c()), C.byref(cfg.to_c()), state[0].shape[1],
                                         k, *[_ptr(t) for t in state], *[_ptr(o[key]) for key in KEYS], ctl._stream())
    ctl._raise(rc, "ntm_mpc_run_from_device")


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--mode", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ntm_mpc import Config, NtmMpc, scenarios_x0
    W, K, B = a.warmup, a.steps, a.batch
    assert K % a.chunks == 0, "--steps must be a multiple of --chunks"
    kc = K // a.chunks
    ctl = NtmMpc(device=0)
    par = ParentLib(a.parent_lib, 0)
    cfg = Config(N=a.N, mode=a.mode)
    x0 = ctl.tensor(scenarios_x0(0, B))
    short, full = buffers(ctl, a.N, B, W), {s: buffers(ctl, a.N, B, W + K) for s in ("run", "run_parent")}
    warm, one = buffers(ctl, a.N, B, W), buffers(ctl, a.N, B, K)
    parts = [buffers(ctl, a.N, B, kc) for _ in range(a.chunks)]
    libs = {"run": (ctl.lib, ctl._ctx), "run_parent": (par.lib, par.ctx)}

    def init_state():
        x = x0.clone()
        rho, Uo = ctl.initial_state(x, cfg)
        return [x, rho, Uo, ctl.new_active_ws(B, cfg)]

    def fresh_state():
        state = init_state()
        run_from(ctl, cfg, state, W, warm)
        return state

    for side in libs:                                             # untimed: module load
        run(*libs[side], ctl, cfg, x0, 1, full[side])
    run_from(ctl, cfg, fresh_state(), 1, one)
    torch.cuda.synchronize()
    full_from = buffers(ctl, a.N, B, W + K)
    sides = ("run", "from_1", "from_chunks", "from_diff", "run_parent")
    ms = {s: [] for s in sides}
    for _ in range(a.runs):
        for side in sides:
            if side in libs:
                t_w = timed(lambda: run(*libs[side], ctl, cfg, x0, W, short))
                t_f = timed(lambda: run(*libs[side], ctl, cfg, x0, W + K, full[side]))
                ms[side].append((t_f - t_w) / K)
            elif side == "from_diff":
                sw, sf = init_state(), init_state()
                t_w = timed(lambda: run_from(ctl, cfg, sw, W, short))
                t_f = timed(lambda: run_from(ctl, cfg, sf, W + K, full_from))
                ms[side].append((t_f - t_w) / K)
            elif side == "from_1":
                st1 = fresh_state()
                ms[side].append(timed(lambda: run_from(ctl, cfg, st1, K, one)) / K)
            else:
                stc = fresh_state()
                ms[side].append(timed(lambda: [run_from(ctl, cfg, stc, kc, o) for o in parts]) / K)
    # the window's outputs: steps W+1 .. W+K of the two runs, the one call, the chunks in a row
    def window(o, key):
        per = {"xk": 2, "uk": 1, "Uk": a.N, "wpred": a.N + 1, "exitflag": 1, "inner_iters": 1}[key]
        return o[key][per * W:]
    cat = {k: torch.cat([parts[0][k]] + [p[k][2:] if k == "xk" else p[k] for p in parts[1:]]) for k in KEYS}
    same = {"run_vs_parent": all(bool(torch.equal(full["run"][k], full["run_parent"][k])) for k in KEYS),
            "from_1_vs_run": all(bool(torch.equal(one[k], window(full["run"], k))) for k in KEYS),
            "chunks_vs_from_1": all(bool(torch.equal(cat[k], one[k])) for k in KEYS),
            "final_state": all(bool(torch.equal(p, q)) for p, q in zip(st1, stc))}
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    res = {"batch": B, "N": a.N, "mode": a.mode, "steps": K, "warmup": W, "chunks": a.chunks,
           "state_bytes_per_call": B * (4 * a.N * 8 + 2 * (a.N + 1) * 4 + 2 * 8) * 2,
           "ms_per_step": ms, "mean": mean, "spread": spread,
           "minus_parent_ms": {k: mean[k] - mean["run_parent"] for k in sides if k != "run_parent"},
           "largest_spread_ms": max(spread.values()), "threshold_3x_spread_ms": 3 * max(spread.values()),
           "outputs_bitwise_equal": same}
    ctl.close()
    par.close()
    line = json.dumps(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
