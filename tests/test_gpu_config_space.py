"""GPU parity off the benchmark points, part 1: the generic kernels over the
horizon range, lane groups that share a wave, and the C-ABI's pointer contract.

The parity suite of test_gpu_parity.py sits on the three benchmark horizons
(N = 10, 20, 50).  Here the runtime-N kernels k_mpc_step<16,0> / <64,0> and
k_mpc_run<16,0> / <64,0> run at the horizons where their code changes path
(N = 16 | 17: lanes per scenario; 32 | 33: the last all-LDS size and the
shift_first switch; 49, 51, 63, 64 around the compiled N = 50 and at the
maximum), four scenarios per wave are compared with the oracle in part-filled
waves and with different fates side by side, and the step / run entry points
are called with 8-byte-aligned and with NULL output pointers.

Tolerances are test_gpu_parity's own (U_TOL, X_TOL, RUN_TOL).  CPU
preconditions: the NumPy and the C oracle, teacher-forced over
3 steps x 8 scenarios, take the same path in 24 of 24 scenario-steps and differ
by <= 4.4e-14 umax at (N, mode) = (5,3), (12,3), (16,2), (16,3), (17,3), (24,3),
(33,2); the C oracle returns exit flag 1 for every scenario of the sweep.
Part 2 (off-default physics / configuration, infeasibility) is
test_gpu_config_space_offdefault.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import cbind
from oracle import ntm_oracle as O
from test_gpu_parity import DEV, H, RUN_TOL, T, U_TOL, X_TOL, _assert_run_close, _teacher_forced, cfgs

pytestmark = pytest.mark.gpu

XSCALE = np.array([0.15, 2000 * np.pi])[:, None]
STEP_KEYS = ("U", "x_pred", "x_next", "exitflag", "inner_iters")
RUN_KEYS = ("xk", "uk", "Uk", "wpred", "exitflag", "inner_iters")


def generic_name(N):
    return f"k_mpc_step<P={16 if N <= 16 else 64},NN=0,lds>"


# ---------------------------------------------------------------- 1. horizon sweep
SWEEP = [(2, 2, False), (5, 3, False), (11, 1, False), (15, 2, True), (16, 2, False), (16, 3, True), (16, 1, True),
         (17, 2, False), (17, 3, True), (21, 2, True), (31, 1, False), (32, 3, True), (33, 2, False), (33, 3, True),
         (49, 2, False), (51, 3, True), (63, 1, False), (64, 3, False), (64, 1, True)]


@pytest.mark.parametrize("N,mode,warm", SWEEP)
def test_sweep_step_teacher_forced(ctl, N, mode, warm):
    """Three teacher-forced steps on the runtime-N kernels.  B = 21 up to N = 16
    leaves the last wave of four 16-lane groups part filled.

    (N, mode) = (49, 2) found a shortfall of the runtime-N kernels: 1.206e-10 umax at
    step 2, scenario 5, entries 18 and 19, where the LPV loop 2-cycles and the device
    certified a set that left U_18 free 2.8e-10 of the largest input outside umin,
    inside the certificate's 1e-9 primal tolerance.  Those kernels now hold the
    certificate's input-bound rows to 1e-12 (StructRows::bound_tol)."""
    B = 21 if N <= 16 else (8 if N <= 33 else 6)
    assert ctl.step_kernel_name(B, cfgs(N, mode)[0]) == generic_name(N)
    res = _teacher_forced(ctl, N, mode, warm, k_sim=3, B=B)
    assert all((r["exitflag"] == 1).all() for r in res["refs"])      # the oracle solves every scenario


@pytest.mark.parametrize("N,mode,B", [(5, 2, 9), (12, 1, 9), (16, 3, 9), (17, 2, 6), (33, 3, 6), (64, 2, 6)])
def test_sweep_run_closed_loop(ctl, N, mode, B):
    """k_mpc_run<16,0> / <64,0> against the C oracle's closed loop, free-running."""
    k_sim = 6
    cfg, ocfg = cfgs(N, mode)
    assert ctl.step_kernel_name(B, cfg) == generic_name(N)
    x0 = O.scenario_x0(np.arange(B)).T
    ref = cbind.run(x0, ocfg, k_sim)
    out = ctl.run(T(x0), k_sim, cfg)
    _assert_run_close(out, ref, cfg, k_sim, tol=RUN_TOL, x0=x0, ocfg=ocfg)


# ---------------------------------------------------------------- 2. lane groups sharing a wave
P16 = [3, 10, 16]           # k_mpc_step<16,0>, <16,10> and <16,0> with every lane of the group in use


def p16_name(N):
    return f"k_mpc_step<P=16,NN={10 if N == 10 else 0},lds>"


def _one_step(ctl, x, cfg, ocfg):
    rho, Uo = cbind.initial_state(x, ocfg)
    return ctl.step(T(x), T(rho), T(Uo), cfg), rho, Uo


def _close_to_oracle(out, ref, cfg, sel):
    """U, x_pred and x_next of the scenarios ``sel`` against the oracle; returns (dU / umax, dx)."""
    N = cfg.N
    du = np.max(np.abs(H(out["U"]) - ref["U"])[:, sel], initial=0.0) / cfg.umax
    xs = np.tile(XSCALE, (N + 1, 1))
    dx = max(np.max((np.abs(H(out["x_pred"]) - ref["x_pred"]) / xs)[:, sel], initial=0.0),
             np.max((np.abs(H(out["x_next"]) - ref["x_next"]) / XSCALE)[:, sel], initial=0.0))
    return du, dx


@pytest.mark.parametrize("B", [1, 2, 3, 5, 7])
@pytest.mark.parametrize("N", P16)
def test_p16_ragged_batches(ctl, N, B):
    """Part-filled waves of 16-lane groups (the retired groups return at once)."""
    cfg, ocfg = cfgs(N, 2)
    assert ctl.step_kernel_name(B, cfg) == p16_name(N)
    x = O.scenario_x0(np.arange(B)).T
    out, rho, Uo = _one_step(ctl, x, cfg, ocfg)
    ref = cbind.step(x, rho, Uo, ocfg)
    du, dx = _close_to_oracle(out, ref, cfg, np.arange(B))
    print(f"N={N} B={B}: max |U - U_oracle| / umax = {du:.2e}, states {dx:.2e}")
    np.testing.assert_array_equal(H(out["exitflag"]), ref["exitflag"])
    np.testing.assert_array_equal(H(out["inner_iters"]), ref["inner_iters"])
    assert du <= U_TOL and dx <= X_TOL, (du, dx)


@pytest.mark.parametrize("N", P16)
def test_p16_composition_invariance(ctl, N):
    """include/ntm_mpc.h: within one build a scenario's results do not depend on the
    batch around it.  13 scenarios as one batch, reversed, and as sub-batches of
    1, 2, 3 and 7: the step and the closed loop agree bit for bit per scenario."""
    B, k_sim = 13, 3
    cfg, ocfg = cfgs(N, 2)
    x = O.scenario_x0(np.arange(B)).T

    def both(ids):
        xs = np.ascontiguousarray(x[:, ids])
        st, _, _ = _one_step(ctl, xs, cfg, ocfg)
        return st, ctl.run(T(xs), k_sim, cfg)

    whole = both(np.arange(B))
    rev = both(np.arange(B)[::-1])
    parts, at = [], 0
    for n in (1, 2, 3, 7):
        parts.append(both(np.arange(at, at + n)))
        at += n
    for i, keys in ((0, STEP_KEYS), (1, RUN_KEYS)):
        for k in keys:
            assert torch.equal(rev[i][k].flip(-1), whole[i][k]), (k, "reversed")
            assert torch.equal(torch.cat([p[i][k] for p in parts], dim=-1), whole[i][k]), (k, "sub-batches")


@pytest.mark.parametrize("N", P16)
def test_p16_mixed_fates_in_one_wave(ctl, N):
    """Groups of one wave with different fates: a non-finite state (-7), two kinds of
    infeasible x_0 (-2) and healthy scenarios that run 2 to 10 LPV iterations."""
    cfg, ocfg = cfgs(N, 2)
    x = O.scenario_x0(np.arange(7)).T.copy()
    x[1, 1] = np.nan
    x[0, 2] = 0.05                              # below xmin[0]
    x[:, 5] = O.REFERENCE_X0
    good = np.array([0, 3, 4, 6])
    out, rho, Uo = _one_step(ctl, x, cfg, ocfg)
    ref = cbind.step(x, rho, Uo, ocfg)
    np.testing.assert_array_equal(ref["exitflag"], [1, -7, -2, 1, 1, -2, 1])
    fl, U = H(out["exitflag"]), H(out["U"])
    np.testing.assert_array_equal(fl, ref["exitflag"])
    assert (U[:, fl != 1] == 0).all()
    du, dx = _close_to_oracle(out, ref, cfg, good)
    print(f"N={N} mixed fates: max |U - U_oracle| / umax = {du:.2e}, states {dx:.2e}")
    np.testing.assert_array_equal(H(out["inner_iters"])[good], ref["inner_iters"][good])
    assert du <= U_TOL and dx <= X_TOL, (du, dx)
    alone, _, _ = _one_step(ctl, np.ascontiguousarray(x[:, good]), cfg, ocfg)
    for k in STEP_KEYS:
        assert torch.equal(alone[k], out[k][..., torch.as_tensor(good, device=DEV)]), k


# ---------------------------------------------------------------- 5. the C-ABI's pointer contract
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _flat(a, pad):
    """(E, B) host data as the ABI's flat scenario-major device array, ``pad`` doubles
    into a larger allocation (pad = 1: 8-byte but not 16-byte aligned)."""
    a = np.ascontiguousarray(np.asarray(a).T).reshape(-1)
    buf = torch.empty(a.size + 2, dtype=torch.float64, device=DEV)
    t = buf[pad:pad + a.size]
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 8 * pad
    return t


@pytest.mark.parametrize("N,build", [(6, "lds"), (20, "lds1"), (20, "far"), (50, "far")])
def test_step_8_byte_aligned_pointers(ctl, N, build):
    """Caller arrays that are only 8-byte aligned (store_record's one-double path at an
    even N, x_next's two-lane path) give the results of the 16-byte aligned call."""
    B = 9
    cfg, ocfg = cfgs(N, 2)
    x = O.scenario_x0(np.arange(B)).T
    rho, Uo = cbind.initial_state(x, ocfg)
    sizes = {"U": N, "x_pred": 2 * (N + 1), "x_next": 2}
    if build == "far":
        ctl.set_small_batch(0)
    try:
        assert ctl.step_build(B, cfg) == build
        got = []
        for pad in (0, 1):
            io = {"x": _flat(x, pad), "rho": _flat(rho, pad), "Uo": _flat(Uo, pad)}
            io.update({k: _flat(np.full((e, B), np.nan), pad) for k, e in sizes.items()})
            fl, it = (torch.full((B,), -99, dtype=torch.int32, device=DEV) for _ in range(2))
            rc = ctl.lib.ntm_mpc_step_ws_device(ctl._ctx, C.byref(ctl.physics.to_c()), C.byref(cfg.to_c()), B,
                                                _p(io["x"]), _p(io["rho"]), _p(io["Uo"]), _p(io["U"]),
                                                _p(io["x_pred"]), _p(io["x_next"]), _p(fl), _p(it), None,
                                                ctl._stream())
            assert rc == 0, rc
            torch.cuda.synchronize()
            got.append({**{k: io[k].clone() for k in ("rho", "Uo", *sizes)}, "exitflag": fl, "inner_iters": it})
    finally:
        ctl.set_small_batch(-1)
    for k in got[0]:
        assert torch.equal(got[0][k], got[1][k]), k
    assert (got[1]["exitflag"] == 1).all() and not torch.isnan(got[1]["x_next"]).any()


@pytest.mark.parametrize("N", [6, 20])
def test_run_null_outputs(ctl, N):
    """ntm_mpc_run_device with each output pointer NULL in turn, and with all but uk
    NULL: the outputs that remain are those of the full call, bit for bit; the same
    once through ntm_mpc_run with host pointers."""
    B, k_sim = 7, 3
    cfg, _ = cfgs(N, 2)
    x0 = O.scenario_x0(np.arange(B)).T
    full = ctl.run(T(x0), k_sim, cfg)
    xd = _flat(x0, 0)

    def call(skip):
        outs = {k: torch.empty_like(full[k].T.contiguous().reshape(-1)) for k in RUN_KEYS}
        args = [None if k in skip else _p(outs[k]) for k in RUN_KEYS]
        rc = ctl.lib.ntm_mpc_run_device(ctl._ctx, C.byref(ctl.physics.to_c()), C.byref(cfg.to_c()), B, k_sim, _p(xd),
                                        *args, ctl._stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        for k in RUN_KEYS:
            if k not in skip:
                assert torch.equal(outs[k], full[k].T.contiguous().reshape(-1)), (k, skip)

    for k in RUN_KEYS:
        call({k})
    call(set(RUN_KEYS) - {"uk"})
    if N == 20:
        xh = np.ascontiguousarray(x0.T)
        uk = np.empty(B * k_sim)
        fl = np.empty(B * k_sim, np.int32)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))              # noqa: E731
        rc = ctl.lib.ntm_mpc_run(ctl._ctx, C.byref(ctl.physics.to_c()), C.byref(cfg.to_c()), B, k_sim, dp(xh), None,
                                 dp(uk), None, None, fl.ctypes.data_as(C.POINTER(C.c_int32)), None)
        assert rc == 0, rc
        np.testing.assert_array_equal(uk, H(full["uk"]).T.reshape(-1))
        np.testing.assert_array_equal(fl, H(full["exitflag"]).T.reshape(-1))
