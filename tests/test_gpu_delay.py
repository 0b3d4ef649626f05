"""GPU tests of the actuator dead time (ntm_mpc_step_dly / ntm_mpc_run_dly /
ntm_mpc_run_dly_from, include/ntm_mpc.h) through the C-ABI: against the estimator entry
points (steps = 0, bit for bit), against the composed oracle reference of
tests/delay_ref.py (itself checked on the CPU by tests/test_delay_ref.py), and against
themselves (chunks, shards, lane groups).

Tolerances are those of tests/test_gpu_parity.py: teacher-forced steps U_TOL = 1e-10 umax
on U and X_TOL = 1e-9 on the states (in the state's scale); free-running closed loops
RUN_TOL = 5e-8.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import delay_ref as D
import mismatch_ref as M
from oracle import ntm_oracle as O

from test_delay_ref import EXACT_DELAYS, EXACT_STEPS, q0_of
from test_estimator_ref import GAIN, GEN, KAPPA, SIGMA_Y, x0_of, xhat0_of
from test_gpu_mismatch import XS, _generic_horizons
from test_gpu_parity import RUN_TOL, U_TOL, X_TOL, H, T, cfgs
from test_gpu_scenarios import dev_gen

pytestmark = pytest.mark.gpu

STEP_KEYS = ("U", "x_pred", "x_next", "y", "x_plan", "u_applied", "exitflag", "inner_iters")
STATE = ("x", "rho", "U_old", "active_ws", "d_hat", "x_hat", "u_queue")
NOISY = dict(nominal=True, gain=GAIN, kappa=KAPPA, sigma_y=SIGMA_Y)


def _est(nominal=True, gain=GAIN, kappa=KAPPA, sigma_y=SIGMA_Y):
    from ntm_mpc import Estimator
    return Estimator(nominal_model=nominal, gain=gain, kappa=kappa, sigma_y=sigma_y)


def _dly(steps, predict=True):
    from ntm_mpc import Delay
    return Delay(steps=steps, predict=predict)


def _d0(B):
    return np.ascontiguousarray(np.stack([1e-5 * np.cos(np.arange(B)), 0.3 * np.sin(np.arange(B))]))


def _queues(steps, B):
    """Per-scenario-distinct queues inside the input range: no two entries alike."""
    j, s = np.arange(steps)[:, None], np.arange(B)[None, :]
    return np.ascontiguousarray(2e5 + 1.1e5 * j + 7e3 * s + 3e2 * j * s)


def _start(ctl, cfg, x0, xh0, d0, q0):
    """[x, rho, U_old, active_ws, d_hat, x_hat, u_queue] of a loop's first call: rho of the
    nominal model at xhat0 (no generator attached), no candidates."""
    ctl.set_scenarios(None)
    xh = ctl.tensor(xh0)
    rho, uo = ctl.initial_state(xh, cfg)
    return [ctl.tensor(x0), rho, uo, ctl.new_active_ws(x0.shape[1], cfg), ctl.tensor(d0), xh,
            None if q0 is None else ctl.tensor(q0)]


def _cat(hs):
    out = {}
    for k in hs[0]:
        if k in ("xk", "dk", "xhk"):
            out[k] = torch.cat([hs[0][k]] + [h[k][2:] for h in hs[1:]])
        else:
            out[k] = torch.cat([h[k] for h in hs])
    return out


def _chunked(ctl, cfg, state, gen, chunks, est, dly):
    hs, done = [], 0
    for n in chunks:
        ctl.set_scenarios(dev_gen(gen, k0=gen.k0 + done))
        hs.append(ctl.run_dly_from(*state, est, dly, n, cfg))
        done += n
    return _cat(hs)


# ------------------------------------------------------------ 1. the degenerate case
@pytest.mark.parametrize("mode", [1, 2])
def test_zero_delay_is_the_estimator_step(ctl, mode):
    """steps = 0, either predict: step_dly is step_est bit for bit on every output and every
    carried value; two steps, the second from the first's outputs, one horizon per lane
    width; the plan state is x_hat and the applied input U[0]."""
    B = 24
    x0 = x0_of(B)
    try:
        for N in _generic_horizons(ctl):
            cfg, _ = cfgs(N, mode)
            for predict in (True, False):
                sa = _start(ctl, cfg, x0, xhat0_of(x0), _d0(B), None)
                sb = _start(ctl, cfg, x0, xhat0_of(x0), _d0(B), None)
                xa, xb = sa[0], sb[0]
                for k in range(2):
                    ctl.set_scenarios(dev_gen(GEN, k0=k))
                    h_in = sb[5].clone()
                    a = ctl.step_est(xa, sa[1], sa[2], sa[4], sa[5], _est(), cfg, active_ws=sa[3])
                    b = ctl.step_dly(xb, sb[1], sb[2], sb[4], sb[5], None, _est(), _dly(0, predict), cfg,
                                     active_ws=sb[3])
                    for key in ("U", "x_pred", "x_next", "y", "exitflag", "inner_iters"):
                        assert torch.equal(a[key], b[key]), (N, predict, k, key)
                    for i in (1, 2, 3, 4, 5):
                        assert torch.equal(sa[i], sb[i]), (N, predict, k, STATE[i])
                    assert torch.equal(b["x_plan"], h_in) and torch.equal(b["u_applied"], b["U"][0]), (N, predict, k)
                    assert b["d_hat"] is sb[4] and b["x_hat"] is sb[5] and b["u_queue"] is None
                    assert (H(b["exitflag"]) == 1).all()
                    xa, xb = a["x_next"], b["x_next"]
    finally:
        ctl.set_scenarios(None)


@pytest.mark.parametrize("mode", [1, 2])
def test_zero_delay_is_the_estimator_run(ctl, mode):
    """steps = 0: run_dly is run_est and run_dly_from is run_est_from bit for bit, 4 steps,
    histories and carried state; uak == uk and xpk is xhk's columns 0 .. k_sim-1."""
    B, k_sim = 24, 4
    x0 = x0_of(B)
    xh0, d0 = xhat0_of(x0), _d0(B)
    try:
        for N in _generic_horizons(ctl):
            cfg, _ = cfgs(N, mode)
            ctl.set_scenarios(dev_gen(GEN))
            a = ctl.run_est(T(x0), _est(), k_sim, cfg, d0=T(d0), xhat0=T(xh0))
            sa = _start(ctl, cfg, x0, xh0, d0, None)[:6]
            ctl.set_scenarios(dev_gen(GEN))
            af = ctl.run_est_from(*sa, _est(), k_sim, cfg)
            for predict in (True, False):
                b = ctl.run_dly(T(x0), _est(), _dly(0, predict), k_sim, cfg, d0=T(d0), xhat0=T(xh0))
                sb = _start(ctl, cfg, x0, xh0, d0, None)
                ctl.set_scenarios(dev_gen(GEN))
                bf = ctl.run_dly_from(*sb, _est(), _dly(0, predict), k_sim, cfg)
                for got, ref in ((b, a), (bf, af)):
                    for key in ref:
                        assert torch.equal(ref[key], got[key]), (N, predict, key)
                    assert torch.equal(got["uak"], got["uk"]) and torch.equal(got["xpk"], got["xhk"][:-2])
                for i in range(6):
                    assert torch.equal(sa[i], sb[i]), (N, predict, STATE[i])
            assert (H(a["exitflag"]) == 1).all()
    finally:
        ctl.set_scenarios(None)


# ------------------------------------------------------------ 2. teacher-forced parity
def _teacher_forced(ctl, N, mode):
    """Six teacher-forced steps of the common noisy inputs at (N, mode), d = 2 from q0: the
    worst figures, the number of scenario-steps on the reference's path, and the total."""
    B, k_sim, steps = 16, 6, 2
    cfg, ocfg = cfgs(N, mode)
    x = x0_of(B)
    xh = xhat0_of(x)
    rho, Uo = M.initial_state(xh, ocfg, GEN, nominal=True)
    d, q = np.zeros((2, B)), q0_of(B)
    keys = ("U", "x_pred", "x_next", "y", "x_hat", "d_hat", "x_plan", "rho", "U_old")
    worst = {k_: 0.0 for k_ in ("U", "x_pred", "x_next", "y", "x_hat", "d_hat", "x_plan", "q_new")}
    same_n = 0
    try:
        for k in range(k_sim):
            g = dataclasses.replace(GEN, k0=k)
            ctl.set_scenarios(dev_gen(g))
            ref = D.step(x, xh, rho, Uo, d, q, ocfg, g, predict=True, **NOISY)
            tr, tu, td, th, tq = T(rho), T(Uo), T(d), T(xh), T(q)
            out = ctl.step_dly(T(x), tr, tu, td, th, tq, _est(), _dly(steps), cfg)
            assert (H(out["exitflag"]) == ref["exitflag"]).all(), k
            assert (ref["exitflag"] == 1).all(), k
            gi = H(out["inner_iters"])
            same = gi == ref["inner_iters"]
            same_n += int(same.sum())
            cmp = {key: np.array(ref[key], copy=True) for key in keys}
            for i_g in np.unique(gi[~same]):
                rp = D.step(x, xh, rho, Uo, d, q, dataclasses.replace(ocfg, i_sim=int(i_g), epsilon=-1.0), g,
                            predict=True, **NOISY)
                sel = ~same & (gi == i_g)
                for key in cmp:
                    cmp[key][:, sel] = rp[key][:, sel]
            got = {"U": H(out["U"]), "x_pred": H(out["x_pred"]), "x_next": H(out["x_next"]), "y": H(out["y"]),
                   "x_plan": H(out["x_plan"]), "x_hat": H(th), "d_hat": H(td)}
            worst["U"] = max(worst["U"], np.max(np.abs(got["U"] - cmp["U"])) / cfg.umax)
            xp = np.abs(got["x_pred"] - cmp["x_pred"]).reshape(N + 1, 2, B) / XS[None]
            worst["x_pred"] = max(worst["x_pred"], np.max(xp))
            for key in ("x_next", "y", "x_hat", "d_hat", "x_plan"):
                worst[key] = max(worst[key], np.max(np.abs(got[key] - cmp[key]) / XS))
            gq = H(tq)
            np.testing.assert_array_equal(gq[:-1], q[1:])                      # shifted entries: exact
            worst["q_new"] = max(worst["q_new"], np.max(np.abs(gq[-1] - cmp["U"][0])) / cfg.umax)
            np.testing.assert_array_equal(gq[-1], got["U"][0])
            np.testing.assert_array_equal(H(out["u_applied"]), q[0])
            assert out["d_hat"] is td and out["x_hat"] is th and out["u_queue"] is tq
            assert np.any(got["x_plan"] != xh, axis=0).all()
            x, xh, rho, Uo, d, q = (ref["x_next"], ref["x_hat"], ref["rho"], ref["U_old"], ref["d_hat"],
                                    ref["u_queue"])
    finally:
        ctl.set_scenarios(None)
    print(f"N={N} mode {mode} d={steps}: " + ", ".join(f"{k_} {v:.2e}" for k_, v in worst.items())
          + f", same path {same_n} of {B * k_sim}")
    return worst, same_n, B * k_sim


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_step_dly_teacher_forced(ctl, mode):
    """d = 2 from q0, the common noisy inputs: each step both sides get identical (x, x_hat,
    rho, U_old, d_hat, queue).  One horizon per lane width in modes 1 and 2, and (20, 3).
    A scenario whose LPV loop stopped at another inner iteration is compared along the
    GPU's path (test_gpu_parity's rule: at least 90% of the scenarios on the same path)."""
    for N in ([20] if mode == 3 else _generic_horizons(ctl)):
        worst, same_n, total = _teacher_forced(ctl, N, mode)
        assert worst["U"] <= U_TOL and worst["q_new"] <= U_TOL, (N, worst)
        for key in ("x_plan", "x_pred", "x_next", "y", "x_hat", "d_hat"):
            assert worst[key] <= X_TOL, (N, key, worst)
        assert same_n >= 0.9 * total, (N, same_n)


# ------------------------------------------------------------ 3. the closed loop
def _run_gpu(ctl, cfg, x0, k_sim, gen, est, dly, d0=None, xhat0=None, uq0=None):
    ctl.set_scenarios(None if gen is None else dev_gen(gen))
    try:
        out = ctl.run_dly(T(x0), est, dly, k_sim, cfg, d0=None if d0 is None else T(d0),
                          xhat0=None if xhat0 is None else T(xhat0), uq0=None if uq0 is None else T(uq0))
        return {k: H(v) for k, v in out.items()}
    finally:
        ctl.set_scenarios(None)


def test_run_dly_free_running(ctl):
    """ntm_mpc_run_dly against the composed reference, free-running (RUN_TOL), N = 20, mode
    2, d = 2 from q0, 12 steps: uak, xpk, xhk, dk, yk (and uk, Uk, xk, wpred); at most 10%
    of the scenarios replayed along the GPU's iteration counts.  The applied inputs are the
    initial queue, then the commands d steps late, bit for bit; a NULL uq0 is a zero queue."""
    N, B, k_sim, steps = 20, 16, 12, 2
    cfg, ocfg = cfgs(N, 2)
    x0 = x0_of(B)
    xh0, d0, q0 = xhat0_of(x0), _d0(B), q0_of(B)
    g = _run_gpu(ctl, cfg, x0, k_sim, GEN, _est(), _dly(steps), d0, xh0, q0)
    kw = dict(d0=d0, xhat0=xh0, uq0=q0, **NOISY)
    ref = D.run(x0, ocfg, k_sim, steps, GEN, **kw)
    ref.pop("u_queue")
    div = (g["inner_iters"] != ref["inner_iters"]).any(axis=0)
    if div.any():
        rp = D.run(x0, ocfg, k_sim, steps, GEN, iters=g["inner_iters"], **kw)
        for k in ref:
            ref[k][:, div] = rp[k][:, div]
    ndiv = int(div.sum())
    assert ndiv <= 0.1 * B, ndiv
    xs, ys = np.tile(XS[:, 0], k_sim + 1)[:, None], np.tile(XS[:, 0], k_sim)[:, None]
    figs = {"uk": np.max(np.abs(g["uk"] - ref["uk"])) / cfg.umax, "Uk": np.max(np.abs(g["Uk"] - ref["Uk"])) / cfg.umax,
            "uak": np.max(np.abs(g["uak"] - ref["uak"])) / cfg.umax,
            "xk": np.max(np.abs(g["xk"] - ref["xk"]) / xs), "wpred": np.max(np.abs(g["wpred"] - ref["wpred"])) / 0.15,
            "dk": np.max(np.abs(g["dk"] - ref["dk"]) / xs), "xhk": np.max(np.abs(g["xhk"] - ref["xhk"]) / xs),
            "yk": np.max(np.abs(g["yk"] - ref["yk"]) / ys), "xpk": np.max(np.abs(g["xpk"] - ref["xpk"]) / ys)}
    print(f"run_dly N=20 mode 2 d={steps}, {k_sim} steps: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items())
          + f", replayed {ndiv}")
    for k, v in figs.items():
        assert v <= RUN_TOL, (k, v)
    assert (g["exitflag"] == ref["exitflag"]).all() and (ref["exitflag"] == 1).all()
    np.testing.assert_array_equal(g["uak"][steps:], g["uk"][:-steps])
    np.testing.assert_array_equal(g["uak"][:steps], q0)
    np.testing.assert_array_equal(g["xhk"][:2], xh0)
    assert np.any(g["xpk"] != g["xhk"][:-2], axis=0).all()
    zero = _run_gpu(ctl, cfg, x0, 4, GEN, _est(), _dly(steps), d0, xh0, np.zeros((steps, B)))
    null = _run_gpu(ctl, cfg, x0, 4, GEN, _est(), _dly(steps), d0, xh0, None)
    for k in zero:
        np.testing.assert_array_equal(zero[k], null[k], err_msg=k)
    assert np.all(null["uak"][:steps] == 0.0)
    np.testing.assert_array_equal(null["uak"][steps:], null["uk"][:-steps])


# ------------------------------------------------------------ 4. the plan is exact where the model is the plant
@pytest.mark.parametrize("steps", EXACT_DELAYS)
@pytest.mark.parametrize("N,mode", [(20, 2), (6, 1)])
def test_plan_state_is_the_future_state(ctl, N, mode, steps):
    """test_delay_ref's exactness property through run_dly (no generator, no noise, x_hat0 =
    x0, gains and kappa 0, zero queue, 12 steps): the plan state of step k is the state d
    steps later to X_TOL in the state's scale (the two call sites may be fused differently
    on the device, so bits are not demanded; whether they agree is printed).  predict = 0
    plans from x_hat, bit for bit."""
    B, k_sim = 16, EXACT_STEPS
    cfg, _ = cfgs(N, mode)
    x0 = x0_of(B)
    e0 = _est(True, 0.0, 0.0, 0.0)
    g = _run_gpu(ctl, cfg, x0, k_sim, None, e0, _dly(steps))
    assert (g["exitflag"] == 1).all()
    np.testing.assert_array_equal(g["xhk"], g["xk"])
    n = k_sim - steps
    got, want = g["xpk"][:2 * (n + 1)], g["xk"][2 * steps:]
    err = np.max(np.abs(got - want) / np.tile(XS[:, 0], n + 1)[:, None])
    print(f"N={N} mode {mode} d={steps}: max |x_plan[k] - x[k+d]| = {err:.2e} (scaled), bitwise: "
          f"{np.array_equal(got, want)}")
    assert err <= X_TOL, err
    np.testing.assert_array_equal(g["uak"][steps:], g["uk"][:-steps])
    assert np.all(g["uak"][:steps] == 0.0)
    h = _run_gpu(ctl, cfg, x0, k_sim, None, e0, _dly(steps, False))
    np.testing.assert_array_equal(h["xpk"], h["xhk"][:-2])
    assert np.any(h["uk"] != g["uk"])


# ------------------------------------------------------------ 5. chunks
@pytest.mark.parametrize("N", [6, 20])
def test_chunks_are_bit_identical(ctl, N):
    """run_dly_from(5) == run_dly_from(2) then (3), d = 3, mode 2: every history and the
    carried state, queue included; both equal run_dly from the same start; zero steps
    change nothing; and the state after two steps, continued by three step_dly calls,
    agrees with the second chunk (flags equal, values to RUN_TOL)."""
    B, steps, mode = 16, 3, 2
    cfg, _ = cfgs(N, mode)
    x0 = x0_of(B)
    xh0, d0, q0 = xhat0_of(x0), _d0(B), _queues(steps, B)
    gen = dataclasses.replace(GEN, k0=2)
    est, dly = _est(), _dly(steps)
    try:
        s1 = _start(ctl, cfg, x0, xh0, d0, q0)
        one = _chunked(ctl, cfg, s1, gen, [5], est, dly)
        s2 = _start(ctl, cfg, x0, xh0, d0, q0)
        first = _chunked(ctl, cfg, s2, gen, [2], est, dly)
        mid = [t.clone() for t in s2]
        before = [t.clone() for t in s2]
        ctl.set_scenarios(dev_gen(gen, k0=gen.k0 + 2))
        none = ctl.run_dly_from(*s2, est, dly, 0, cfg)
        for a, b, name in zip(s2, before, STATE):
            assert torch.equal(a, b), name
        assert torch.equal(none["xk"], s2[0]) and none["uak"].shape == (0, B) and none["xpk"].shape == (0, B)
        second = _chunked(ctl, cfg, s2, dataclasses.replace(gen, k0=gen.k0 + 2), [3], est, dly)
        two = _cat([first, second])
        for k in one:
            assert torch.equal(one[k], two[k]), k
        for a, b, name in zip(s1, s2, STATE):
            assert torch.equal(a, b), name
        assert torch.equal(s1[6], one["uk"][-steps:]) and torch.equal(s1[0], one["xk"][-2:])
        ctl.set_scenarios(dev_gen(gen))
        whole = ctl.run_dly(T(x0), est, dly, 5, cfg, d0=T(d0), xhat0=T(xh0), uq0=T(q0))
        for k in one:
            assert torch.equal(one[k], whole[k]), k
        assert (H(one["exitflag"]) == 1).all()
        assert torch.equal(one["uak"][:steps], ctl.tensor(q0)) and torch.equal(one["uak"][steps:], one["uk"][:-steps])
        # mid-loop: three single steps from the carried state
        x = mid[0]
        worst = 0.0
        sec = {k: H(v) for k, v in second.items()}
        for k in range(3):
            ctl.set_scenarios(dev_gen(gen, k0=gen.k0 + 2 + k))
            o = ctl.step_dly(x, mid[1], mid[2], mid[4], mid[5], mid[6], est, dly, cfg, active_ws=mid[3])
            np.testing.assert_array_equal(H(o["exitflag"]), sec["exitflag"][k])
            figs = (np.max(np.abs(H(o["U"]) - sec["Uk"][k * N:(k + 1) * N])) / cfg.umax,
                    np.max(np.abs(H(o["u_applied"]) - sec["uak"][k])) / cfg.umax,
                    np.max(np.abs(H(o["x_next"]) - sec["xk"][2 * (k + 1):2 * (k + 2)]) / XS),
                    np.max(np.abs(H(o["x_plan"]) - sec["xpk"][2 * k:2 * (k + 1)]) / XS),
                    np.max(np.abs(H(o["y"]) - sec["yk"][2 * k:2 * (k + 1)]) / XS),
                    np.max(np.abs(H(mid[5]) - sec["xhk"][2 * (k + 1):2 * (k + 2)]) / XS),
                    np.max(np.abs(H(mid[4]) - sec["dk"][2 * (k + 1):2 * (k + 2)]) / XS))
            worst = max(worst, *figs)
            x = o["x_next"]
        print(f"N={N}: three step_dly calls against run_dly_from(3): worst {worst:.2e}")
        assert worst <= RUN_TOL, worst
        assert np.max(np.abs(H(mid[6]) - H(s2[6]))) / cfg.umax <= RUN_TOL
    finally:
        ctl.set_scenarios(None)


# ------------------------------------------------------------ 6. lane groups and shards
def _step_all(ctl, cfg, x, xh, d, q, rho, uo, first_id, dly, gen=GEN):
    """One step_dly of the columns given (global ids first_id ..): every output, host arrays."""
    ctl.set_scenarios(dev_gen(gen, first_id=first_id, k0=1))
    tr, tu, td, th, tq = T(rho), T(uo), T(d), T(xh), T(q)
    ws = ctl.new_active_ws(x.shape[1], cfg)
    out = ctl.step_dly(T(x), tr, tu, td, th, tq, _est(), dly, cfg, active_ws=ws)
    r = {k: H(out[k]) for k in STEP_KEYS}
    r.update(rho=H(tr), U_old=H(tu), d_hat=H(td), x_hat=H(th), u_queue=H(tq), ws=H(ws))
    return r


SPLIT = ((0, 1), (1, 6), (6, 13))


def test_lane_groups_and_shards(ctl):
    """13 scenarios with per-scenario-distinct queues, d = 3, whole and as 1 + 5 + 7
    (first_id offsets): the same bits, step and run, at one horizon per lane width (at fewer
    than 64 lanes per scenario the queues of neighbouring scenarios share a wave).  One
    scenario with a NaN queue entry: flag -7 and U = 0, its neighbours bit-identical to the
    batch without it."""
    B, k_sim, steps, bad = 13, 4, 3, 6
    x = x0_of(B)
    xh, d, q = xhat0_of(x), _d0(B), _queues(steps, B)
    dly = _dly(steps)
    try:
        for N in _generic_horizons(ctl):
            cfg, _ = cfgs(N, 2)
            ctl.set_scenarios(None)
            rho_t, uo_t = ctl.initial_state(T(xh), cfg)
            rho, uo = H(rho_t), H(uo_t)
            whole = _step_all(ctl, cfg, x, xh, d, q, rho, uo, 0, dly)
            parts = [_step_all(ctl, cfg, x[:, lo:hi], xh[:, lo:hi], d[:, lo:hi], q[:, lo:hi], rho[:, lo:hi],
                               uo[:, lo:hi], lo, dly) for lo, hi in SPLIT]
            for k in whole:
                np.testing.assert_array_equal(whole[k], np.concatenate([p[k] for p in parts], axis=-1), err_msg=k)
            assert (whole["exitflag"] == 1).all()
            np.testing.assert_array_equal(whole["u_applied"], q[0])
            np.testing.assert_array_equal(whole["u_queue"][:-1], q[1:])
            np.testing.assert_array_equal(whole["u_queue"][-1], whole["U"][0])
            full = _run_gpu(ctl, cfg, x, k_sim, GEN, _est(), dly, d, xh, q)
            runs = [_run_gpu(ctl, cfg, x[:, lo:hi], k_sim, dataclasses.replace(GEN, first_id=lo), _est(), dly,
                             d[:, lo:hi], xh[:, lo:hi], q[:, lo:hi]) for lo, hi in SPLIT]
            for k in full:
                np.testing.assert_array_equal(full[k], np.concatenate([p[k] for p in runs], axis=1), err_msg=k)
            np.testing.assert_array_equal(full["uak"][:steps], q)
            np.testing.assert_array_equal(full["uak"][steps:], full["uk"][:-steps])
            qb = q.copy()
            qb[1, bad] = np.nan
            got = _step_all(ctl, cfg, x, xh, d, qb, rho, uo, 0, dly)
            assert got["exitflag"][bad] == -7 and np.all(got["U"][:, bad] == 0.0), N
            assert np.any(np.isnan(got["x_plan"][:, bad])) and got["u_applied"][bad] == q[0, bad]
            others = np.arange(B) != bad
            for k in whole:
                np.testing.assert_array_equal(got[k][..., others], whole[k][..., others], err_msg=k)
    finally:
        ctl.set_scenarios(None)


# ------------------------------------------------------------ 7. validation, host paths
def test_delay_arguments_validated(ctl):
    from ntm_mpc import Config, NtmLibraryError
    from ntm_mpc._lib import NtmDelay
    from ntm_mpc.api import _ptr
    N, B, k_sim = 6, 4, 2
    cfg = Config(N=N, mode=2)
    x = ctl.tensor(x0_of(B))                                     # the ABI's layout: the raw calls stage nothing
    ctl.set_scenarios(None)
    rho, uo = ctl.initial_state(x, cfg)
    d, xh = ctl.tensor(np.zeros((2, B))), ctl.tensor(x0_of(B))
    ws = ctl.new_active_ws(B, cfg)
    q = ctl.tensor(np.full((8, B), 1e5))                         # room for every legal delay
    est = C.byref(_est(sigma_y=0.0).to_c())
    phys = C.byref(ctl.physics.to_c())

    def dly_c(steps=2, predict=1):
        return C.byref(NtmDelay(steps, predict))

    o = {"U": ctl._empty(N, B), "xp": ctl._empty(2 * (N + 1), B), "xn": ctl._empty(2, B), "z": ctl._empty(2, B),
         "ua": ctl._empty(B), "fl": ctl._empty(B, dtype=torch.int32), "it": ctl._empty(B, dtype=torch.int32),
         "uak": ctl._empty(k_sim, B), "xpk": ctl._empty(2 * k_sim, B)}

    def raw_step(dly, q_ptr, c=cfg, x_plan=None, u_app=None):
        st = [rho.clone(), uo.clone(), d.clone(), xh.clone()]        # alive for the call: no block is handed out twice
        return ctl.lib.ntm_mpc_step_dly_device(ctl._ctx, phys, C.byref(c.to_c()), est, dly, B, _ptr(x),
                                               *[_ptr(t) for t in st], q_ptr, _ptr(o["U"]), _ptr(o["xp"]),
                                               _ptr(o["xn"]), None, x_plan, u_app, _ptr(o["fl"]), _ptr(o["it"]), None,
                                               ctl._stream())

    def raw_run(dly, q_ptr, c=cfg, uak=None, xpk=None):
        return ctl.lib.ntm_mpc_run_dly_device(ctl._ctx, phys, C.byref(c.to_c()), est, dly, B, k_sim, _ptr(x), None, None,
                                              q_ptr, None, None, None, None, None, None, None, uak, xpk, None, None,
                                              ctl._stream())

    def raw_from(dly, q_ptr, c=cfg, uak=None, xpk=None):
        st = [x.clone(), rho.clone(), uo.clone(), ws.clone(), d.clone(), xh.clone()]
        return ctl.lib.ntm_mpc_run_dly_from_device(ctl._ctx, phys, C.byref(c.to_c()), est, dly, B, k_sim,
                                                   *[_ptr(t) for t in st], q_ptr, None, None, None, None, None, None,
                                                   None, uak, xpk, None, None, ctl._stream())

    try:
        qc = q.clone()
        qp = _ptr(qc)
        for raw in (raw_step, raw_run, raw_from):
            assert raw(None, qp) == -1, raw.__name__                              # NULL delay
            for steps in (-1, 9, 1 << 20):
                assert raw(dly_c(steps), qp) == -1, (raw.__name__, steps)
            for predict in (-1, 2):
                assert raw(dly_c(2, predict), qp) == -1, (raw.__name__, predict)
                assert raw(dly_c(0, predict), None) == -1, (raw.__name__, predict)
            for flags in (O.LITERAL_PHI_RIGHTMUL, O.LITERAL_GAMMA_INDEX, O.LITERAL_PLANT_NO_C):
                assert raw(dly_c(), qp, dataclasses.replace(cfg, flags=flags)) == -4, (raw.__name__, flags)
            assert raw(dly_c(), qp, dataclasses.replace(cfg, flags=O.RHO1_SQUARED)) == 0, raw.__name__
            assert raw(dly_c(0), None) == 0 and raw(dly_c(8), qp) == 0, raw.__name__
        # a NULL queue with steps > 0: zeros for run_dly's uq0, refused where it is carried
        assert raw_step(dly_c(), None) == -1 and raw_from(dly_c(), None) == -1 and raw_run(dly_c(), None) == 0
        # a queue that overlaps another argument
        qq = q.clone()
        assert raw_step(dly_c(2), _ptr(qq), x_plan=_ptr(qq)) == -1
        assert raw_step(dly_c(2), _ptr(qq), u_app=C.c_void_p(qq.data_ptr() + 8)) == -1
        assert raw_step(dly_c(2), _ptr(o["U"])) == -1
        assert raw_run(dly_c(2), _ptr(qq), uak=_ptr(qq)) == -1 and raw_run(dly_c(2), _ptr(x)) == -1
        assert raw_from(dly_c(2), _ptr(qq), xpk=C.c_void_p(qq.data_ptr() + 2 * B * 8 - 8)) == -1
        assert raw_from(dly_c(2), _ptr(qq), xpk=C.c_void_p(qq.data_ptr() + 2 * B * 8)) == 0     # adjacent: fine
        assert raw_step(dly_c(2), _ptr(qq), x_plan=_ptr(o["z"]), u_app=_ptr(o["ua"])) == 0
        torch.cuda.synchronize()
        with pytest.raises(NtmLibraryError, match=r"\(-1\)"):
            ctl.step_dly(x, rho.clone(), uo.clone(), d.clone(), xh.clone(), ctl.tensor(np.zeros((9, B))),
                         _est(sigma_y=0.0), _dly(9), cfg)
        with pytest.raises(NtmLibraryError, match=r"\(-1\)"):
            ctl.run_dly(x, _est(sigma_y=0.0), _dly(9), k_sim, cfg)
        with pytest.raises(ValueError):                                           # a queue of the wrong length
            ctl.run_dly(x, _est(sigma_y=0.0), _dly(3), k_sim, cfg, uq0=ctl.tensor(np.zeros((2, B))))
        out = ctl.run_dly(x, _est(sigma_y=0.0), _dly(8), k_sim, cfg)
        assert (H(out["exitflag"]) == 1).all() and np.all(H(out["uak"]) == 0.0)
    finally:
        ctl.set_scenarios(None)


def test_host_entry_points_match_device(ctl):
    N, B, k_sim, steps = 20, 9, 3, 3
    cfg, _ = cfgs(N, 2)
    x = x0_of(B)
    xh0, d0, q0 = xhat0_of(x), _d0(B), _queues(steps, B)
    est, dly = _est(), _dly(steps)
    ctl.set_scenarios(None)
    rho0, uo0 = ctl.initial_state_host(xh0, cfg)
    ctl.set_scenarios(dev_gen(GEN, first_id=3, k0=2))
    cp = lambda a: a.copy(order="K")                                              # noqa: E731
    try:
        rh, uh, dh, hh, qh = cp(rho0), cp(uo0), cp(d0), cp(xh0), cp(q0)
        wh = -np.ones((2 * (N + 1), B), np.int32)
        h = ctl.step_dly_host(x, rh, uh, dh, hh, qh, est, dly, cfg, active_ws=wh)
        rd, ud, dd, hd, qd, wd = T(rho0), T(uo0), T(d0), T(xh0), T(q0), ctl.new_active_ws(B, cfg)
        g = ctl.step_dly(T(x), rd, ud, dd, hd, qd, est, dly, cfg, active_ws=wd)
        for k in STEP_KEYS + ("d_hat", "x_hat", "u_queue"):
            np.testing.assert_array_equal(h[k], H(g[k]), err_msg=k)
        for a, b in ((rh, rd), (uh, ud), (dh, dd), (hh, hd), (qh, qd), (wh, wd)):
            np.testing.assert_array_equal(a, H(b))
        np.testing.assert_array_equal(qh[:-1], q0[1:])
        np.testing.assert_array_equal(h["u_applied"], q0[0])
        for q_init in (q0, None):
            hr = ctl.run_dly_host(x, est, dly, k_sim, cfg, d0=d0, xhat0=xh0, uq0=q_init)
            gr = ctl.run_dly(T(x), est, dly, k_sim, cfg, d0=T(d0), xhat0=T(xh0),
                             uq0=None if q_init is None else T(q_init))
            for k in gr:
                np.testing.assert_array_equal(hr[k], H(gr[k]), err_msg=k)
        assert np.all(hr["uak"] == 0.0)                                           # k_sim == steps, a zero queue
        sh = [cp(x), cp(rho0), cp(uo0), -np.ones((2 * (N + 1), B), np.int32), cp(d0), cp(xh0), cp(q0)]
        sd = [T(x), T(rho0), T(uo0), ctl.new_active_ws(B, cfg), T(d0), T(xh0), T(q0)]
        hf = ctl.run_dly_from_host(*sh, est, dly, k_sim, cfg)
        gf = ctl.run_dly_from(*sd, est, dly, k_sim, cfg)
        for k in gf:
            np.testing.assert_array_equal(hf[k], H(gf[k]), err_msg=k)
        for a, b, name in zip(sh, sd, STATE):
            np.testing.assert_array_equal(a, H(b), err_msg=name)
        np.testing.assert_array_equal(sh[6], hf["uk"])                            # the last d commands
        # steps = 0 through the host path, with and without a queue array
        e0 = ctl.step_est_host(x, cp(rho0), cp(uo0), cp(d0), cp(xh0), est, cfg)
        for q_arg in (None, np.zeros((0, B))):
            z0 = ctl.step_dly_host(x, cp(rho0), cp(uo0), cp(d0), cp(xh0), q_arg, est, _dly(0), cfg)
            for k in ("U", "x_pred", "x_next", "y", "d_hat", "x_hat", "exitflag", "inner_iters"):
                np.testing.assert_array_equal(z0[k], e0[k], err_msg=k)
    finally:
        ctl.set_scenarios(None)
