"""GPU tests of plant-model mismatch and the offset-free disturbance estimate
(ntm_mpc_step_obs / ntm_mpc_run_obs, include/ntm_mpc.h) through the C-ABI, against the
composed oracle reference of tests/mismatch_ref.py (itself checked on the CPU by
tests/test_mismatch_ref.py).

Tolerances are those of tests/test_gpu_parity.py: teacher-forced steps U_TOL = 1e-10
umax on U and X_TOL = 1e-9 on the states (and on d_hat, in the state's scale);
free-running closed loops RUN_TOL = 5e-8.
"""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

import mismatch_ref as M
from oracle import ntm_oracle as O

from test_gpu_parity import RUN_TOL, U_TOL, X_TOL, H, T, cfgs
from test_gpu_scenarios import GEN, dev_gen

pytestmark = pytest.mark.gpu

XS = np.array([0.15, 2000 * math.pi])[:, None]                 # |w|, |omega| magnitudes


def _obs(nominal=False, gain=0.0):
    from ntm_mpc import Observer
    return Observer(nominal_model=nominal, gain=gain)


def _x0(B, first=0):
    return np.ascontiguousarray(O.scenario_x0(np.arange(first, first + B)).T)


def _generic_horizons(ctl):
    """One horizon per lane width the runtime-N kernels are launched with here."""
    by_lanes = {}
    for N in (6, 12, 20, 24, 40):
        lanes, nn = C.c_int32(), C.c_int32()
        assert ctl.lib.ntm_step_launch_info(N, C.byref(lanes), C.byref(nn)) == 0
        by_lanes.setdefault(lanes.value, N)
    assert set(by_lanes) <= {16, 32, 64} and len(by_lanes) >= 2, by_lanes
    return sorted(by_lanes.values())


# ------------------------------------------------------------ the degenerate case
@pytest.mark.parametrize("with_gen", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_degenerate_options_are_todays_step(ctl, mode, with_gen):
    """nominal_model = 0, gain = 0, d_hat = 0: step_obs is step_dual bit for bit (U, x_pred,
    x_next, rho, U_old, the carried active sets, exit flags, iteration counts), two
    steps, the second from the first's outputs, at one horizon per lane width."""
    B = 24
    try:
        for N in _generic_horizons(ctl):
            cfg, _ = cfgs(N, mode)
            x = T(_x0(B))
            ctl.set_scenarios(dev_gen(GEN) if with_gen else None)
            rho0, uo0 = ctl.initial_state(x, cfg)
            ra, ua, wa = rho0.clone(), uo0.clone(), ctl.new_active_ws(B, cfg)
            rb, ub, wb = rho0.clone(), uo0.clone(), ctl.new_active_ws(B, cfg)
            xa = xb = x
            for k in range(2):
                if with_gen:
                    ctl.set_scenarios(dev_gen(GEN, k0=k))
                d = T(np.zeros((2, B)))
                a = ctl.step_dual(xa, ra, ua, cfg, active_ws=wa)
                b = ctl.step_obs(xb, rb, ub, d, _obs(False, 0.0), cfg, active_ws=wb)
                for key in ("U", "x_pred", "x_next", "exitflag", "inner_iters"):
                    assert torch.equal(a[key], b[key]), (N, k, key)
                assert torch.equal(ra, rb) and torch.equal(ua, ub) and torch.equal(wa, wb), (N, k)
                assert torch.equal(b["d_hat"], torch.zeros_like(d)), (N, k)
                xa, xb = a["x_next"], b["x_next"]
    finally:
        ctl.set_scenarios(None)


# ------------------------------------------------------------ teacher-forced parity
@pytest.mark.parametrize("N,mode", [(6, 1), (20, 2)])
def test_step_obs_teacher_forced(ctl, N, mode):
    """Nominal model, every plant its own plasma and disturbance, gain 0.5: each step both
    sides get identical (x_k, rho, U_old, d_hat).  A scenario whose LPV loop stopped at
    another inner iteration is compared along the GPU's path (test_gpu_parity's rule:
    at least 90% of the scenarios on the same path)."""
    B, k_sim, gain = 16, 6, 0.5
    cfg, ocfg = cfgs(N, mode)
    x = _x0(B)
    rho, Uo = M.initial_state(x, ocfg, GEN, nominal=True)
    d = np.zeros((2, B))
    worst = worst_x = worst_d = 0.0
    same_n = 0
    try:
        for k in range(k_sim):
            g = dataclasses.replace(GEN, k0=k)
            ctl.set_scenarios(dev_gen(g))
            ref = M.step(x, rho, Uo, d, ocfg, g, nominal=True, gain=gain)
            tr, tu, td = T(rho), T(Uo), T(d)
            out = ctl.step_obs(T(x), tr, tu, td, _obs(True, gain), cfg)
            assert (H(out["exitflag"]) == ref["exitflag"]).all(), k
            gi = H(out["inner_iters"])
            same = gi == ref["inner_iters"]
            same_n += int(same.sum())
            cmp = {key: np.array(ref[key], copy=True) for key in ("U", "x_pred", "x_next", "d_hat", "rho", "U_old")}
            for i_g in np.unique(gi[~same]):
                rp = M.step(x, rho, Uo, d, dataclasses.replace(ocfg, i_sim=int(i_g), epsilon=-1.0), g, nominal=True,
                            gain=gain)
                sel = ~same & (gi == i_g)
                for key in cmp:
                    cmp[key][:, sel] = rp[key][:, sel]
            worst = max(worst, np.max(np.abs(H(out["U"]) - cmp["U"])) / cfg.umax)
            xp = np.abs(H(out["x_pred"]) - cmp["x_pred"]).reshape(N + 1, 2, B) / XS[None]
            worst_x = max(worst_x, np.max(np.abs(H(out["x_next"]) - cmp["x_next"]) / XS), np.max(xp))
            worst_d = max(worst_d, np.max(np.abs(H(td) - cmp["d_hat"]) / XS))
            assert out["d_hat"] is td
            np.testing.assert_allclose(H(tr)[:, same], ref["rho"][:, same], rtol=1e-9, atol=0)
            if k:
                assert np.all(d[0] != 0.0)
            x, rho, Uo, d = ref["x_next"], ref["rho"], ref["U_old"], ref["d_hat"]
    finally:
        ctl.set_scenarios(None)
    print(f"N={N} mode {mode}: U {worst:.2e} of umax, states {worst_x:.2e}, d_hat {worst_d:.2e}, "
          f"same path {same_n} of {B * k_sim}")
    assert worst <= U_TOL, worst
    assert worst_x <= X_TOL, worst_x
    assert worst_d <= X_TOL, worst_d
    assert same_n >= 0.9 * B * k_sim, same_n


# ------------------------------------------------------------ the closed loop
def _run_pair(ctl, cfg, ocfg, x0, k_sim, gen, nominal, gain, d0=None):
    ctl.set_scenarios(dev_gen(gen))
    try:
        out = ctl.run_obs(T(x0), _obs(nominal, gain), k_sim, cfg, d0=None if d0 is None else T(d0))
    finally:
        ctl.set_scenarios(None)
    g = {k: H(v) for k, v in out.items()}
    ref = M.run(x0, ocfg, k_sim, gen, nominal=nominal, gain=gain, d0=d0)
    div = (g["inner_iters"] != ref["inner_iters"]).any(axis=0)
    if div.any():                                              # along the GPU's path (test_gpu_parity's rule)
        rp = M.run(x0, ocfg, k_sim, gen, nominal=nominal, gain=gain, d0=d0, iters=g["inner_iters"])
        for k in ref:
            ref[k][:, div] = rp[k][:, div]
    return out, g, ref, int(div.sum())


def test_run_obs_free_running(ctl):
    """ntm_mpc_run_obs against the composed reference, free-running (RUN_TOL), dk included;
    column 0 of dk is d0."""
    N, B, k_sim = 20, 16, 20
    cfg, ocfg = cfgs(N, 2)
    x0 = _x0(B)
    d0 = np.ascontiguousarray(np.stack([1e-5 * np.cos(np.arange(B)), 0.3 * np.sin(np.arange(B))]))
    out, g, ref, ndiv = _run_pair(ctl, cfg, ocfg, x0, k_sim, GEN, True, 0.5, d0)
    assert ndiv <= 0.1 * B, ndiv
    xs = np.tile(XS[:, 0], k_sim + 1)[:, None]
    figs = {"uk": np.max(np.abs(g["uk"] - ref["uk"])) / cfg.umax, "Uk": np.max(np.abs(g["Uk"] - ref["Uk"])) / cfg.umax,
            "xk": np.max(np.abs(g["xk"] - ref["xk"]) / xs), "wpred": np.max(np.abs(g["wpred"] - ref["wpred"])) / 0.15,
            "dk": np.max(np.abs(g["dk"] - ref["dk"]) / xs)}
    print("run_obs N=20 mode 2, 20 steps: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()) + f", replayed {ndiv}")
    for k, v in figs.items():
        assert v <= RUN_TOL, (k, v)
    assert (g["exitflag"] == ref["exitflag"]).all()
    np.testing.assert_array_equal(g["dk"][:2], d0)
    np.testing.assert_array_equal(g["xk"][:2], x0)
    assert np.max(np.abs(g["dk"][2:4] - d0)) > 0                # the estimate moved


def test_run_obs_null_d0_is_zeros(ctl):
    N, B, k_sim = 20, 16, 4
    cfg, _ = cfgs(N, 2)
    x0 = T(_x0(B))
    ctl.set_scenarios(dev_gen(GEN))
    try:
        a = ctl.run_obs(x0, _obs(True, 0.5), k_sim, cfg, d0=None)
        b = ctl.run_obs(x0, _obs(True, 0.5), k_sim, cfg, d0=T(np.zeros((2, B))))
    finally:
        ctl.set_scenarios(None)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["dk"][:2], torch.zeros_like(a["dk"][:2]))


# ------------------------------------------------------------ the physical property
def test_estimate_removes_the_offset(ctl):
    """A wrong j_BS is an error in C1 alone.  Nominal model, plants with a 10% j_BS
    spread, no noise, N = 20, mode 2, 40 steps.  At gain 1 the estimate is the C1
    difference (1e-12: the oracle holds 1e-17, the margin is the GPU's summation order
    in x_next, about an ulp of w each), d_hat[1] stays zero, and the last step's one-step
    prediction of w is the plant's (1e-12).  At gain 0 the scenario with the largest
    mismatch keeps a prediction error of at least 1e-5 (the oracle: 1.7e-4).  An
    estimate added to the plant, or left out of the lift, fails this."""
    N, B, k_sim = 20, 8, 40
    cfg, ocfg = cfgs(N, 2)
    gen = O.ScenarioGen(jbs_spread=0.1)
    x0 = T(_x0(B))
    dC1 = np.array([O.C_vec(O.scenario_physics(O.Physics(), gen, s), ocfg.Ts)[0] - O.C_vec(O.Physics(), ocfg.Ts)[0]
                    for s in range(B)])
    ctl.set_scenarios(dev_gen(gen))
    try:
        one = {k: H(v) for k, v in ctl.run_obs(x0, _obs(True, 1.0), k_sim, cfg).items()}
        zero = {k: H(v) for k, v in ctl.run_obs(x0, _obs(True, 0.0), k_sim, cfg).items()}
    finally:
        ctl.set_scenarios(None)
    assert (one["exitflag"] == 1).all() and (zero["exitflag"] == 1).all()

    def pred_err(h):                                            # |x_pred(1) - x_next| in w, last step
        return np.abs(h["wpred"][(k_sim - 1) * (N + 1) + 1] - h["xk"][2 * k_sim])

    e_d = np.max(np.abs(one["dk"][-2] - dC1))
    print(f"gain 1: |d_hat[0] - dC1| {e_d:.2e}, |d_hat[1]| {np.max(np.abs(one['dk'][1::2])):.2e}, prediction error "
          f"{pred_err(one).max():.2e}; gain 0: prediction error {pred_err(zero)[np.argmax(np.abs(dC1))]:.2e}")
    assert e_d <= 1e-12, e_d
    assert np.max(np.abs(one["dk"][1::2])) <= 1e-9
    assert pred_err(one).max() <= 1e-12, pred_err(one)
    assert np.all(zero["dk"] == 0.0)
    assert pred_err(zero)[np.argmax(np.abs(dC1))] >= 1e-5, pred_err(zero)


# ------------------------------------------------------------ independence
def test_run_obs_is_shard_invariant(ctl):
    """Shards with first_id offsets reproduce the one-batch run_obs bit for bit."""
    N, B, k_sim = 20, 16, 6
    cfg, _ = cfgs(N, 2)
    x0 = _x0(B)
    d0 = np.ascontiguousarray(np.stack([1e-5 * np.cos(np.arange(B)), 0.3 * np.sin(np.arange(B))]))
    obs = _obs(True, 0.5)
    try:
        ctl.set_scenarios(dev_gen(GEN, first_id=0))
        full = ctl.run_obs(T(x0), obs, k_sim, cfg, d0=T(d0))
        parts = []
        for lo, hi in ((0, 5), (5, 16)):
            ctl.set_scenarios(dev_gen(GEN, first_id=lo))
            parts.append(ctl.run_obs(T(x0[:, lo:hi]), obs, k_sim, cfg, d0=T(d0[:, lo:hi])))
    finally:
        ctl.set_scenarios(None)
    for k in full:
        assert torch.equal(full[k], torch.cat([parts[0][k], parts[1][k]], dim=1)), k


def test_nominal_model_without_generator_changes_nothing(ctl):
    N, B, k_sim = 20, 16, 5
    cfg, _ = cfgs(N, 2)
    x0 = T(_x0(B))
    ctl.set_scenarios(None)
    a = ctl.run_obs(x0, _obs(True, 0.5), k_sim, cfg)
    b = ctl.run_obs(x0, _obs(False, 0.5), k_sim, cfg)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    rho, uo = ctl.initial_state(x0, cfg)
    outs = []
    for nominal in (True, False):
        d = T(np.zeros((2, B)))
        outs.append((ctl.step_obs(x0, rho.clone(), uo.clone(), d, _obs(nominal, 0.5), cfg), d))
    for k in ("U", "x_pred", "x_next", "exitflag", "inner_iters", "d_hat"):
        assert torch.equal(outs[0][0][k], outs[1][0][k]), k


# ------------------------------------------------------------ validation
def test_observer_arguments_validated(ctl):
    from ntm_mpc import Config, NtmLibraryError
    from ntm_mpc._lib import NtmObserver
    from ntm_mpc.api import _ptr
    N, B = 6, 4
    cfg = Config(N=N, mode=2)
    x = ctl.tensor(_x0(B))                                       # the ABI's layout: the raw calls stage nothing
    rho, uo = ctl.initial_state(x, cfg)
    d = ctl.tensor(np.zeros((2, B)))

    def raw_step(obs, d_ptr, c=cfg):
        o = {"U": ctl._empty(N, B), "xp": ctl._empty(2 * (N + 1), B), "xn": ctl._empty(2, B),
             "fl": ctl._empty(B, dtype=torch.int32), "it": ctl._empty(B, dtype=torch.int32)}
        return ctl.lib.ntm_mpc_step_obs_device(ctl._ctx, C.byref(ctl.physics.to_c()), C.byref(c.to_c()), obs, B,
                                               _ptr(x), _ptr(rho.clone()), _ptr(uo.clone()), d_ptr, _ptr(o["U"]),
                                               _ptr(o["xp"]), _ptr(o["xn"]), _ptr(o["fl"]), _ptr(o["it"]), None,
                                               ctl._stream())

    def raw_run(obs, c=cfg):
        return ctl.lib.ntm_mpc_run_obs_device(ctl._ctx, C.byref(ctl.physics.to_c()), C.byref(c.to_c()), obs, B, 2,
                                              _ptr(x), None, None, None, None, None, None, None, None, ctl._stream())

    ok = C.byref(NtmObserver(0, 0, 0.5))
    for gain in (-0.1, 1.5, float("nan"), float("inf")):
        assert raw_step(C.byref(NtmObserver(1, 0, gain)), _ptr(d)) == -1, gain
        assert raw_run(C.byref(NtmObserver(1, 0, gain))) == -1, gain
        with pytest.raises(NtmLibraryError, match=r"\(-1\)"):
            ctl.step_obs(x, rho.clone(), uo.clone(), d, _obs(True, gain), cfg)
        with pytest.raises(NtmLibraryError, match=r"\(-1\)"):
            ctl.run_obs(x, _obs(True, gain), 2, cfg)
    assert raw_step(C.byref(NtmObserver(0, 1, 0.5)), _ptr(d)) == -1           # reserved
    assert raw_run(C.byref(NtmObserver(0, 1, 0.5))) == -1
    assert raw_step(None, _ptr(d)) == -1 and raw_run(None) == -1              # NULL obs
    assert raw_step(ok, None) == -1                                            # NULL d_hat
    for flags in (O.LITERAL_PHI_RIGHTMUL, O.LITERAL_GAMMA_INDEX, O.LITERAL_PLANT_NO_C):
        c = dataclasses.replace(cfg, flags=flags)
        assert raw_step(ok, _ptr(d), c) == -4 and raw_run(ok, c) == -4, flags
        with pytest.raises(NtmLibraryError, match=r"\(-4\)"):
            ctl.step_obs(x, rho.clone(), uo.clone(), d, _obs(False, 0.5), c)
    torch.cuda.synchronize()
    assert torch.equal(d, torch.zeros_like(d))                                 # no refused call touched it
    # the context works afterwards, and NTM_RHO1_SQUARED is allowed
    for c in (cfg, dataclasses.replace(cfg, flags=O.RHO1_SQUARED)):
        assert raw_step(ok, _ptr(d), c) == 0 and raw_run(ok, c) == 0
        r2, u2 = ctl.initial_state(x, c)
        out = ctl.step_obs(x, r2, u2, T(np.zeros((2, B))), _obs(False, 0.5), c)
        assert (H(out["exitflag"]) == 1).all()


# ------------------------------------------------------------ host paths
def test_host_entry_points_match_device(ctl):
    N, B, k_sim = 20, 9, 3
    cfg, _ = cfgs(N, 2)
    x = _x0(B)
    d0 = np.ascontiguousarray(np.stack([1e-5 * np.cos(np.arange(B)), 0.3 * np.sin(np.arange(B))]))
    obs = _obs(True, 0.5)
    ctl.set_scenarios(None)
    rho0, uo0 = ctl.initial_state_host(x, cfg)
    ctl.set_scenarios(dev_gen(GEN, first_id=3, k0=2))
    try:
        rh, uh, dh, wh = rho0.copy(order="K"), uo0.copy(order="K"), d0.copy(order="K"), -np.ones((2 * (N + 1), B), np.int32)
        h = ctl.step_obs_host(x, rh, uh, dh, obs, cfg, active_ws=wh)
        rd, ud, dd, wd = T(rho0), T(uo0), T(d0), ctl.new_active_ws(B, cfg)
        g = ctl.step_obs(T(x), rd, ud, dd, obs, cfg, active_ws=wd)
        for k in ("U", "x_pred", "x_next", "exitflag", "inner_iters", "d_hat"):
            np.testing.assert_array_equal(h[k], H(g[k]), err_msg=k)
        for a, b in ((rh, rd), (uh, ud), (dh, dd), (wh, wd)):
            np.testing.assert_array_equal(a, H(b))
        assert np.any(dh != d0)
        for d_init in (d0, None):
            hr = ctl.run_obs_host(x, obs, k_sim, cfg, d0=d_init)
            gr = ctl.run_obs(T(x), obs, k_sim, cfg, d0=None if d_init is None else T(d_init))
            for k in gr:
                np.testing.assert_array_equal(hr[k], H(gr[k]), err_msg=k)
    finally:
        ctl.set_scenarios(None)
