"""GPU tests of output feedback: measurement noise and the filtered state estimate
(ntm_mpc_step_est / ntm_mpc_run_est, include/ntm_mpc.h) through the C-ABI, against the
observer entry points (the degenerate case, bit for bit) and against the composed oracle
reference of tests/estimator_ref.py (itself checked on the CPU by
tests/test_estimator_ref.py).

Tolerances are those of tests/test_gpu_parity.py: teacher-forced steps U_TOL = 1e-10
umax on U and X_TOL = 1e-9 on the states (x_pred, x_next, y, x_hat and d_hat, in the
state's scale); free-running closed loops RUN_TOL = 5e-8.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import estimator_ref as E
import mismatch_ref as M
from oracle import ntm_oracle as O

from test_estimator_ref import (GAIN, GEN, KAPPA, PROP_BOUND, PROP_GAIN, PROP_GEN, PROP_STEPS, SIGMA_Y,
                                rejection_ratio, x0_of, xhat0_of)
from test_gpu_mismatch import XS, _generic_horizons, _obs
from test_gpu_parity import RUN_TOL, U_TOL, X_TOL, H, T, cfgs
from test_gpu_scenarios import dev_gen

pytestmark = pytest.mark.gpu

STEP_KEYS = ("U", "x_pred", "x_next", "y", "exitflag", "inner_iters")


def _est(nominal=True, gain=GAIN, kappa=KAPPA, sigma_y=SIGMA_Y):
    from ntm_mpc import Estimator
    return Estimator(nominal_model=nominal, gain=gain, kappa=kappa, sigma_y=sigma_y)


def _d0(B):
    return np.ascontiguousarray(np.stack([1e-5 * np.cos(np.arange(B)), 0.3 * np.sin(np.arange(B))]))


# ------------------------------------------------------------ the degenerate case
@pytest.mark.parametrize("with_spreads", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_degenerate_options_are_the_observer_step(ctl, mode, with_spreads):
    """sigma_y = 0, kappa = 0, equal gains 0.5, x_hat == x, a non-zero d_hat: step_est is
    step_obs bit for bit (U, x_pred, x_next, rho, U_old, the carried active sets, d_hat,
    exit flags, iteration counts), x_hat and y come out equal to x_next; two steps, the
    second from the first's outputs, at one horizon per lane width."""
    B = 24
    gen = GEN if with_spreads else dataclasses.replace(GEN, jbs_spread=0.0, wdep_spread=0.0)
    try:
        for N in _generic_horizons(ctl):
            cfg, _ = cfgs(N, mode)
            x = T(x0_of(B))
            ctl.set_scenarios(None)
            rho0, uo0 = ctl.initial_state(x, cfg)
            ra, ua, wa, da = rho0.clone(), uo0.clone(), ctl.new_active_ws(B, cfg), T(_d0(B))
            rb, ub, wb, db = rho0.clone(), uo0.clone(), ctl.new_active_ws(B, cfg), T(_d0(B))
            xa = xb = x
            hb = x.clone()
            for k in range(2):
                ctl.set_scenarios(dev_gen(gen, k0=k))
                a = ctl.step_obs(xa, ra, ua, da, _obs(True, 0.5), cfg, active_ws=wa)
                b = ctl.step_est(xb, rb, ub, db, hb, _est(True, (0.5, 0.5), 0.0, 0.0), cfg, active_ws=wb)
                for key in ("U", "x_pred", "x_next", "exitflag", "inner_iters"):
                    assert torch.equal(a[key], b[key]), (N, k, key)
                assert torch.equal(ra, rb) and torch.equal(ua, ub) and torch.equal(wa, wb), (N, k)
                assert torch.equal(da, db) and b["d_hat"] is db, (N, k)
                assert torch.equal(hb, b["x_next"]) and torch.equal(b["y"], b["x_next"]), (N, k)
                assert b["x_hat"] is hb
                xa, xb = a["x_next"], b["x_next"]
    finally:
        ctl.set_scenarios(None)


@pytest.mark.parametrize("mode", [1, 2])
def test_degenerate_run_is_the_observer_run(ctl, mode):
    """run_est with the degenerate options is run_obs bit for bit, dk included, and
    xhk == xk, yk == xk's columns 1..; with xhat0 = NULL and with xhat0 = x0."""
    B, k_sim = 24, 4
    d0 = T(_d0(B))
    ctl.set_scenarios(dev_gen(GEN))
    try:
        for N in _generic_horizons(ctl):
            cfg, _ = cfgs(N, mode)
            x0 = T(x0_of(B))
            a = ctl.run_obs(x0, _obs(True, 0.5), k_sim, cfg, d0=d0)
            for xh0 in (None, x0.clone()):
                b = ctl.run_est(x0, _est(True, (0.5, 0.5), 0.0, 0.0), k_sim, cfg, d0=d0, xhat0=xh0)
                for key in a:
                    assert torch.equal(a[key], b[key]), (N, key)
                assert torch.equal(b["xhk"], b["xk"]) and torch.equal(b["yk"], b["xk"][2:]), N
    finally:
        ctl.set_scenarios(None)


# ------------------------------------------------------------ teacher-forced parity
def _teacher_forced(ctl, N, mode):
    """Six teacher-forced steps of the common inputs at (N, mode): the worst figures, the
    number of scenario-steps on the reference's path, and the total."""
    B, k_sim = 16, 6
    cfg, ocfg = cfgs(N, mode)
    x = x0_of(B)
    xh = xhat0_of(x)
    rho, Uo = M.initial_state(xh, ocfg, GEN, nominal=True)
    d = np.zeros((2, B))
    keys = ("U", "x_pred", "x_next", "y", "x_hat", "d_hat", "rho", "U_old")
    worst = {"U": 0.0, "x_pred": 0.0, "x_next": 0.0, "y": 0.0, "x_hat": 0.0, "d_hat": 0.0}
    same_n = 0
    try:
        for k in range(k_sim):
            g = dataclasses.replace(GEN, k0=k)
            ctl.set_scenarios(dev_gen(g))
            ref = E.step(x, xh, rho, Uo, d, ocfg, g, True, GAIN, KAPPA, SIGMA_Y)
            tr, tu, td, th = T(rho), T(Uo), T(d), T(xh)
            out = ctl.step_est(T(x), tr, tu, td, th, _est(), cfg)
            assert (H(out["exitflag"]) == ref["exitflag"]).all(), k
            assert (ref["exitflag"] == 1).all(), k
            gi = H(out["inner_iters"])
            same = gi == ref["inner_iters"]
            same_n += int(same.sum())
            cmp = {key: np.array(ref[key], copy=True) for key in keys}
            for i_g in np.unique(gi[~same]):
                rp = E.step(x, xh, rho, Uo, d, dataclasses.replace(ocfg, i_sim=int(i_g), epsilon=-1.0), g, True, GAIN,
                            KAPPA, SIGMA_Y)
                sel = ~same & (gi == i_g)
                for key in cmp:
                    cmp[key][:, sel] = rp[key][:, sel]
            got = {"U": H(out["U"]), "x_pred": H(out["x_pred"]), "x_next": H(out["x_next"]), "y": H(out["y"]),
                   "x_hat": H(th), "d_hat": H(td)}
            worst["U"] = max(worst["U"], np.max(np.abs(got["U"] - cmp["U"])) / cfg.umax)
            xp = np.abs(got["x_pred"] - cmp["x_pred"]).reshape(N + 1, 2, B) / XS[None]
            worst["x_pred"] = max(worst["x_pred"], np.max(xp))
            for key in ("x_next", "y", "x_hat", "d_hat"):
                worst[key] = max(worst[key], np.max(np.abs(got[key] - cmp[key]) / XS))
            assert out["d_hat"] is td and out["x_hat"] is th
            np.testing.assert_allclose(H(tr)[:, same], ref["rho"][:, same], rtol=1e-9, atol=0)
            assert np.any(xh != x, axis=0).all() and np.all(got["y"] != got["x_next"])
            x, xh, rho, Uo, d = ref["x_next"], ref["x_hat"], ref["rho"], ref["U_old"], ref["d_hat"]
    finally:
        ctl.set_scenarios(None)
    print(f"N={N} mode {mode}: " + ", ".join(f"{k_} {v:.2e}" for k_, v in worst.items())
          + f", same path {same_n} of {B * k_sim}")
    return worst, same_n, B * k_sim


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_step_est_teacher_forced(ctl, mode):
    """The common inputs (nominal model, every plant its own plasma and disturbance, noisy
    measurement, x_hat != x): each step both sides get identical (x, x_hat, rho, U_old,
    d_hat).  One horizon per lane width in modes 1 and 2, and (20, 3).  A scenario whose
    LPV loop stopped at another inner iteration is compared along the GPU's path
    (test_gpu_parity's rule: at least 90% of the scenarios on the same path)."""
    for N in ([20] if mode == 3 else _generic_horizons(ctl)):
        worst, same_n, total = _teacher_forced(ctl, N, mode)
        assert worst["U"] <= U_TOL, (N, worst)
        for key in ("x_pred", "x_next", "y", "x_hat", "d_hat"):
            assert worst[key] <= X_TOL, (N, key, worst)
        assert same_n >= 0.9 * total, (N, same_n)


# ------------------------------------------------------------ the closed loop
def _run_gpu(ctl, cfg, x0, k_sim, gen, est, d0=None, xhat0=None):
    ctl.set_scenarios(dev_gen(gen))
    try:
        out = ctl.run_est(T(x0), est, k_sim, cfg, d0=None if d0 is None else T(d0),
                          xhat0=None if xhat0 is None else T(xhat0))
        return {k: H(v) for k, v in out.items()}
    finally:
        ctl.set_scenarios(None)


def test_run_est_free_running(ctl):
    """ntm_mpc_run_est against the composed reference, free-running (RUN_TOL), N = 20,
    mode 2, 20 steps; xhk, dk and yk included; column 0 of xhk / dk are the inputs; at most
    10% of the scenarios replayed along the GPU's iteration counts."""
    N, B, k_sim = 20, 16, 20
    cfg, ocfg = cfgs(N, 2)
    x0 = x0_of(B)
    xh0, d0 = xhat0_of(x0), _d0(B)
    g = _run_gpu(ctl, cfg, x0, k_sim, GEN, _est(), d0, xh0)
    kw = dict(nominal=True, gain=GAIN, kappa=KAPPA, sigma_y=SIGMA_Y, d0=d0, xhat0=xh0)
    ref = E.run(x0, ocfg, k_sim, GEN, **kw)
    div = (g["inner_iters"] != ref["inner_iters"]).any(axis=0)
    if div.any():
        rp = E.run(x0, ocfg, k_sim, GEN, iters=g["inner_iters"], **kw)
        for k in ref:
            ref[k][:, div] = rp[k][:, div]
    ndiv = int(div.sum())
    assert ndiv <= 0.1 * B, ndiv
    xs, ys = np.tile(XS[:, 0], k_sim + 1)[:, None], np.tile(XS[:, 0], k_sim)[:, None]
    figs = {"uk": np.max(np.abs(g["uk"] - ref["uk"])) / cfg.umax, "Uk": np.max(np.abs(g["Uk"] - ref["Uk"])) / cfg.umax,
            "xk": np.max(np.abs(g["xk"] - ref["xk"]) / xs), "wpred": np.max(np.abs(g["wpred"] - ref["wpred"])) / 0.15,
            "dk": np.max(np.abs(g["dk"] - ref["dk"]) / xs), "xhk": np.max(np.abs(g["xhk"] - ref["xhk"]) / xs),
            "yk": np.max(np.abs(g["yk"] - ref["yk"]) / ys)}
    print("run_est N=20 mode 2, 20 steps: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()) + f", replayed {ndiv}")
    for k, v in figs.items():
        assert v <= RUN_TOL, (k, v)
    assert (g["exitflag"] == ref["exitflag"]).all() and (ref["exitflag"] == 1).all()
    np.testing.assert_array_equal(g["dk"][:2], d0)
    np.testing.assert_array_equal(g["xhk"][:2], xh0)
    np.testing.assert_array_equal(g["xk"][:2], x0)
    assert np.all(g["xhk"][2:] != g["xk"][2:]) and np.all(g["xhk"][2:] != g["yk"])


# ------------------------------------------------------------ the measurement noise
def test_measurement_noise_is_the_samplers(ctl):
    """y is x_next + sigma_y n of the host sampler, exactly: the sigma_y are powers of two,
    so the product is exact and the sum is one rounding whether or not it is fused.  Step
    (k0 = 3, first_id = 5) and run; a zero sigma_y leaves that component's y at x_next."""
    from ntm_mpc import meas_sample
    N, B, k_sim = 12, 13, 3
    cfg, _ = cfgs(N, 2)
    x0 = x0_of(B, 5)
    gen = dataclasses.replace(GEN, first_id=5, k0=3)
    for sy in (SIGMA_Y, (SIGMA_Y[0], 0.0), (0.0, SIGMA_Y[1])):
        g = _run_gpu(ctl, cfg, x0, k_sim, gen, _est(sigma_y=sy), xhat0=xhat0_of(x0))
        for k in range(k_sim):
            n = meas_sample(dev_gen(gen), B, gen.k0 + k).T        # (2, B)
            xn = g["xk"][2 * (k + 1):2 * (k + 2)]
            np.testing.assert_array_equal(g["yk"][2 * k:2 * (k + 1)], xn + np.array(sy)[:, None] * n)
            for i in range(2):
                assert np.all((g["yk"][2 * k + i] == xn[i]) == (sy[i] == 0.0))
    ctl.set_scenarios(None)
    rho, uo = ctl.initial_state(T(xhat0_of(x0)), cfg)
    ctl.set_scenarios(dev_gen(gen))
    try:
        out = ctl.step_est(T(x0), rho, uo, T(np.zeros((2, B))), T(xhat0_of(x0)), _est(), cfg)
        n = meas_sample(dev_gen(gen), B, gen.k0).T
        np.testing.assert_array_equal(H(out["y"]), H(out["x_next"]) + np.array(SIGMA_Y)[:, None] * n)
    finally:
        ctl.set_scenarios(None)


# ------------------------------------------------------------ lane groups
def _step_all(ctl, cfg, x, xh, d, rho, uo, first_id, est=None, gen=GEN):
    """One step_est of the columns given (global ids first_id ..): every output, host arrays."""
    ctl.set_scenarios(dev_gen(gen, first_id=first_id, k0=1))
    tr, tu, td, th = T(rho), T(uo), T(d), T(xh)
    ws = ctl.new_active_ws(x.shape[1], cfg)
    out = ctl.step_est(T(x), tr, tu, td, th, est or _est(), cfg, active_ws=ws)
    r = {k: H(out[k]) for k in STEP_KEYS}
    r.update(rho=H(tr), U_old=H(tu), d_hat=H(td), x_hat=H(th), ws=H(ws))
    return r


SPLIT = ((0, 1), (1, 6), (6, 13))
QUIET = dataclasses.replace(GEN, sigma_w=0.0, jbs_spread=0.0, wdep_spread=0.0)


def test_lane_groups_are_independent(ctl):
    """13 scenarios whole and as 1 + 5 + 7 (first_id offsets) give the same results bit for
    bit, step and run, at one horizon per lane width: at fewer than 64 lanes per scenario
    the three carried values live in the lanes of a shared wave.  Reversed too: a column's
    global id is first_id + its index, so the reversed batch runs with nothing that
    depends on the id (no spreads, sigma_w = sigma_y = 0; the filter and the estimate still
    run, x_hat != x) and must be the reversed results of the same batch in order."""
    B, k_sim = 13, 3
    x = x0_of(B)
    xh, d = xhat0_of(x), _d0(B)
    e0, r = _est(sigma_y=0.0), slice(None, None, -1)
    try:
        for N in _generic_horizons(ctl):
            cfg, _ = cfgs(N, 2)
            ctl.set_scenarios(None)
            rho_t, uo_t = ctl.initial_state(T(xh), cfg)
            rho, uo = H(rho_t), H(uo_t)
            whole = _step_all(ctl, cfg, x, xh, d, rho, uo, 0)
            parts = [_step_all(ctl, cfg, x[:, lo:hi], xh[:, lo:hi], d[:, lo:hi], rho[:, lo:hi], uo[:, lo:hi], lo)
                     for lo, hi in SPLIT]
            for k in whole:
                np.testing.assert_array_equal(whole[k], np.concatenate([p[k] for p in parts], axis=-1), err_msg=k)
            assert np.all(whole["y"] != whole["x_next"]) and np.all(whole["x_hat"] != whole["y"])
            fwd = _step_all(ctl, cfg, x, xh, d, rho, uo, 0, e0, QUIET)
            bwd = _step_all(ctl, cfg, x[:, r], xh[:, r], d[:, r], rho[:, r], uo[:, r], 0, e0, QUIET)
            for k in fwd:
                np.testing.assert_array_equal(fwd[k], bwd[k][..., r], err_msg=k)
            full = _run_gpu(ctl, cfg, x, k_sim, GEN, _est(), d, xh)
            runs = [_run_gpu(ctl, cfg, x[:, lo:hi], k_sim, dataclasses.replace(GEN, first_id=lo), _est(),
                             d[:, lo:hi], xh[:, lo:hi]) for lo, hi in SPLIT]
            for k in full:
                np.testing.assert_array_equal(full[k], np.concatenate([p[k] for p in runs], axis=1), err_msg=k)
            fwd = _run_gpu(ctl, cfg, x, k_sim, QUIET, e0, d, xh)
            bwd = _run_gpu(ctl, cfg, x[:, r], k_sim, QUIET, e0, d[:, r], xh[:, r])
            for k in fwd:
                np.testing.assert_array_equal(fwd[k], bwd[k][:, r], err_msg=k)
            assert np.any(fwd["xhk"][2:] != fwd["xk"][2:], axis=0).all()
    finally:
        ctl.set_scenarios(None)


@pytest.mark.parametrize("N", [6, 20])
def test_nan_estimate_stays_in_its_lanes(ctl, N):
    """One scenario with a NaN x_hat among healthy ones: exit flag -7 and U = 0, its d_hat
    kept and x_hat = y; its neighbours are bit-identical to the batch without it."""
    B, bad = 13, 6
    cfg, _ = cfgs(N, 2)
    x = x0_of(B)
    xh, d = xhat0_of(x), _d0(B)
    try:
        ctl.set_scenarios(None)
        rho_t, uo_t = ctl.initial_state(T(xh), cfg)
        rho, uo = H(rho_t), H(uo_t)
        good = _step_all(ctl, cfg, x, xh, d, rho, uo, 0)
        xb = xh.copy()
        xb[0, bad] = np.nan
        got = _step_all(ctl, cfg, x, xb, d, rho, uo, 0)
    finally:
        ctl.set_scenarios(None)
    assert (good["exitflag"] == 1).all()
    assert got["exitflag"][bad] == -7 and np.all(got["U"][:, bad] == 0.0)
    np.testing.assert_array_equal(got["d_hat"][:, bad], d[:, bad])
    np.testing.assert_array_equal(got["x_hat"][:, bad], got["y"][:, bad])
    assert np.all(np.isfinite(got["y"][:, bad])) and np.all(got["y"][:, bad] != got["x_next"][:, bad])
    others = np.arange(B) != bad
    for k in good:
        np.testing.assert_array_equal(got[k][..., others], good[k][..., others], err_msg=k)


def test_run_est_is_shard_invariant(ctl):
    """Two halves run with first_id offsets reproduce the one-batch results bit for bit,
    step and run."""
    N, B, k_sim = 20, 16, 6
    cfg, _ = cfgs(N, 2)
    x0 = x0_of(B)
    xh0, d0 = xhat0_of(x0), _d0(B)
    full = _run_gpu(ctl, cfg, x0, k_sim, GEN, _est(), d0, xh0)
    parts = [_run_gpu(ctl, cfg, x0[:, lo:hi], k_sim, dataclasses.replace(GEN, first_id=lo), _est(), d0[:, lo:hi],
                      xh0[:, lo:hi]) for lo, hi in ((0, 8), (8, 16))]
    for k in full:
        np.testing.assert_array_equal(full[k], np.concatenate([p[k] for p in parts], axis=1), err_msg=k)
    try:
        ctl.set_scenarios(None)
        rho_t, uo_t = ctl.initial_state(T(xh0), cfg)
        rho, uo = H(rho_t), H(uo_t)
        whole = _step_all(ctl, cfg, x0, xh0, d0, rho, uo, 0)
        halves = [_step_all(ctl, cfg, x0[:, lo:hi], xh0[:, lo:hi], d0[:, lo:hi], rho[:, lo:hi], uo[:, lo:hi], lo)
                  for lo, hi in ((0, 8), (8, 16))]
    finally:
        ctl.set_scenarios(None)
    for k in whole:
        np.testing.assert_array_equal(whole[k], np.concatenate([p[k] for p in halves], axis=-1), err_msg=k)


# ------------------------------------------------------------ the property
def test_filter_rejects_measurement_noise_on_the_gpu(ctl):
    """test_estimator_ref's noise-rejection property through run_est, the same inputs and
    the same 0.8 bound (N = 20, mode 2, 30 steps, statistics from step 6 on)."""
    N, B = 20, 16
    cfg, _ = cfgs(N, 2)
    x0 = x0_of(B)
    xh0 = xhat0_of(x0)
    h_f = _run_gpu(ctl, cfg, x0, PROP_STEPS, PROP_GEN, _est(True, PROP_GAIN, (0.5, 0.5), SIGMA_Y), xhat0=xh0)
    h_0 = _run_gpu(ctl, cfg, x0, PROP_STEPS, PROP_GEN, _est(True, PROP_GAIN, 0.0, SIGMA_Y), xhat0=xh0)
    assert (h_f["exitflag"] == 1).all() and (h_0["exitflag"] == 1).all()
    ratio, rms0 = rejection_ratio(h_f, h_0)
    print(f"GPU N={N}: ratio w {ratio[0]:.3f}, omega {ratio[1]:.3f}; rms at kappa = 0: {rms0[0]:.3e} m, "
          f"{rms0[1]:.3e} rad/s")
    np.testing.assert_array_equal(h_0["xhk"][2:], h_0["yk"])
    assert np.all(ratio <= PROP_BOUND), ratio


# ------------------------------------------------------------ validation
def test_estimator_arguments_validated(ctl):
    from ntm_mpc import Config, NtmLibraryError
    from ntm_mpc._lib import NtmEstimator
    from ntm_mpc.api import _ptr
    N, B = 6, 4
    cfg = Config(N=N, mode=2)
    x = ctl.tensor(x0_of(B))                                     # the ABI's layout: the raw calls stage nothing
    ctl.set_scenarios(None)
    rho, uo = ctl.initial_state(x, cfg)
    d, xh = ctl.tensor(np.zeros((2, B))), ctl.tensor(x0_of(B))
    d2 = C.c_double * 2

    def est_c(gain=(0.5, 0.5), kappa=(0.5, 0.5), sy=(0.0, 0.0), reserved=0):
        return C.byref(NtmEstimator(1, reserved, d2(*gain), d2(*kappa), d2(*sy)))

    def raw_step(est, d_ptr, h_ptr, c=cfg):
        o = {"U": ctl._empty(N, B), "xp": ctl._empty(2 * (N + 1), B), "xn": ctl._empty(2, B),
             "fl": ctl._empty(B, dtype=torch.int32), "it": ctl._empty(B, dtype=torch.int32)}
        return ctl.lib.ntm_mpc_step_est_device(ctl._ctx, C.byref(ctl.physics.to_c()), C.byref(c.to_c()), est, B,
                                               _ptr(x), _ptr(rho.clone()), _ptr(uo.clone()), d_ptr, h_ptr,
                                               _ptr(o["U"]), _ptr(o["xp"]), _ptr(o["xn"]), None, _ptr(o["fl"]),
                                               _ptr(o["it"]), None, ctl._stream())

    def raw_run(est, c=cfg):
        return ctl.lib.ntm_mpc_run_est_device(ctl._ctx, C.byref(ctl.physics.to_c()), C.byref(c.to_c()), est, B, 2,
                                              _ptr(x), None, None, None, None, None, None, None, None, None, None,
                                              None, ctl._stream())

    nan, inf = float("nan"), float("inf")
    try:
        for bad in (-0.1, 1.5, nan, inf):
            for i in range(2):
                v = (bad, 0.5) if i == 0 else (0.5, bad)
                for kw in ({"gain": v}, {"kappa": v}):
                    assert raw_step(est_c(**kw), _ptr(d), _ptr(xh)) == -1, kw
                    assert raw_run(est_c(**kw)) == -1, kw
            with pytest.raises(NtmLibraryError, match=r"\(-1\)"):
                ctl.step_est(x, rho.clone(), uo.clone(), d, xh, _est(True, bad, 0.5, 0.0), cfg)
            with pytest.raises(NtmLibraryError, match=r"\(-1\)"):
                ctl.run_est(x, _est(True, 0.5, bad, 0.0), 2, cfg)
        ctl.set_scenarios(dev_gen(QUIET))
        for bad in (-1e-3, nan, inf):                            # sigma_y, a generator attached
            for sy in ((bad, 0.0), (0.0, bad)):
                assert raw_step(est_c(sy=sy), _ptr(d), _ptr(xh)) == -1, sy
                assert raw_run(est_c(sy=sy)) == -1, sy
        # a generator with all-zero sigmas and spreads is enough for the seed
        assert raw_step(est_c(sy=SIGMA_Y), _ptr(d.clone()), _ptr(xh.clone())) == 0
        assert raw_run(est_c(sy=SIGMA_Y)) == 0
        ctl.set_scenarios(None)                                  # sigma_y != 0 and no generator: no seed
        for sy in ((1e-3, 0.0), (0.0, 1.0)):
            assert raw_step(est_c(sy=sy), _ptr(d), _ptr(xh)) == -1, sy
            assert raw_run(est_c(sy=sy)) == -1, sy
        with pytest.raises(NtmLibraryError, match=r"\(-1\)"):
            ctl.run_est(x, _est(), 2, cfg)
        ok = est_c()
        assert raw_step(est_c(reserved=1), _ptr(d), _ptr(xh)) == -1 and raw_run(est_c(reserved=1)) == -1
        assert raw_step(None, _ptr(d), _ptr(xh)) == -1 and raw_run(None) == -1       # NULL est
        assert raw_step(ok, None, _ptr(xh)) == -1                                    # NULL d_hat
        assert raw_step(ok, _ptr(d), None) == -1                                     # NULL x_hat
        for flags in (O.LITERAL_PHI_RIGHTMUL, O.LITERAL_GAMMA_INDEX, O.LITERAL_PLANT_NO_C):
            c = dataclasses.replace(cfg, flags=flags)
            assert raw_step(ok, _ptr(d), _ptr(xh), c) == -4 and raw_run(ok, c) == -4, flags
            with pytest.raises(NtmLibraryError, match=r"\(-4\)"):
                ctl.step_est(x, rho.clone(), uo.clone(), d, xh, _est(sigma_y=0.0), c)
        torch.cuda.synchronize()
        assert torch.equal(d, torch.zeros_like(d)) and torch.equal(xh, ctl.tensor(x0_of(B)))   # no refused call wrote
        # the context works afterwards, and NTM_RHO1_SQUARED is allowed
        for c in (cfg, dataclasses.replace(cfg, flags=O.RHO1_SQUARED)):
            assert raw_step(ok, _ptr(d.clone()), _ptr(xh.clone()), c) == 0 and raw_run(ok, c) == 0
            r2, u2 = ctl.initial_state(x, c)
            out = ctl.step_est(x, r2, u2, T(np.zeros((2, B))), T(x0_of(B)), _est(sigma_y=0.0), c)
            assert (H(out["exitflag"]) == 1).all()
    finally:
        ctl.set_scenarios(None)


# ------------------------------------------------------------ host paths
def test_host_entry_points_match_device(ctl):
    N, B, k_sim = 20, 9, 3
    cfg, _ = cfgs(N, 2)
    x = x0_of(B)
    xh0, d0 = xhat0_of(x), _d0(B)
    est = _est()
    ctl.set_scenarios(None)
    rho0, uo0 = ctl.initial_state_host(xh0, cfg)
    ctl.set_scenarios(dev_gen(GEN, first_id=3, k0=2))
    try:
        rh, uh, dh, hh = rho0.copy(order="K"), uo0.copy(order="K"), d0.copy(order="K"), xh0.copy(order="K")
        wh = -np.ones((2 * (N + 1), B), np.int32)
        h = ctl.step_est_host(x, rh, uh, dh, hh, est, cfg, active_ws=wh)
        rd, ud, dd, hd, wd = T(rho0), T(uo0), T(d0), T(xh0), ctl.new_active_ws(B, cfg)
        g = ctl.step_est(T(x), rd, ud, dd, hd, est, cfg, active_ws=wd)
        for k in STEP_KEYS + ("d_hat", "x_hat"):
            np.testing.assert_array_equal(h[k], H(g[k]), err_msg=k)
        for a, b in ((rh, rd), (uh, ud), (dh, dd), (hh, hd), (wh, wd)):
            np.testing.assert_array_equal(a, H(b))
        assert np.any(dh != d0) and np.all(hh != xh0) and np.all(h["y"] != h["x_next"])
        for d_init, h_init in ((d0, xh0), (None, None)):
            hr = ctl.run_est_host(x, est, k_sim, cfg, d0=d_init, xhat0=h_init)
            gr = ctl.run_est(T(x), est, k_sim, cfg, d0=None if d_init is None else T(d_init),
                             xhat0=None if h_init is None else T(h_init))
            for k in gr:
                np.testing.assert_array_equal(hr[k], H(gr[k]), err_msg=k)
        np.testing.assert_array_equal(hr["xhk"][:2], x)            # xhat0 = NULL: the initial estimate is x0
    finally:
        ctl.set_scenarios(None)
