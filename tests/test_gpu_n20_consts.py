"""The problem constants of the N = 20 far kernels (csrc/ntm_n20.hip): the unit is compiled
without input-rate rows (rate_rows in csrc/ntm_ws.h), so the rate arms of the row
provider and of polish_compact, and with them every restore of `du`, are folded out,
while r, eps and the state bounds xmin / xmax are read where they were.

The tests run the three kernels of the unit (the step kernel, its scenario-generator
instantiation and the closed-loop kernel), far build forced at a small batch, against the
C oracle with constants that are neither the defaults nor symmetric, so that a swapped
parity index or a wrong field cannot pass, and check that mode 3 at N = 20 still takes
the runtime-N kernels (the launchers of the far unit refuse it)."""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import pytest
import torch

from oracle import cbind
from oracle import ntm_oracle as O
from test_gpu_parity import DEV, H, RUN_TOL, T, U_TOL, X_TOL, _assert_run_close, _teacher_forced, cfgs

pytestmark = pytest.mark.gpu

FAR_NAME = "k_mpc_step<P=64,NN=20,far>"
N = 20
W2PI = 2 * math.pi
# Two sets of constants, chosen with the oracle alone (cbind.step on scenarios 0..63 of the
# seeded set, mode 2, first step; a predicted state "touches" a bound when it sits within
# 1e-9 of it, relative):
#   LOW   the reference omega below omega's lower bound: every scenario optimal, 20 of 64
#         plans touch w's lower bound, 4 w's upper one, 5 omega's lower one;
#   HIGH  the reference omega above omega's upper bound: 62 optimal and 2 infeasible,
#         50 plans touch w's upper bound, 20 omega's upper one.
# Between them each of xmin[0], xmin[1], xmax[0], xmax[1] is an active row's right-hand
# side somewhere, and xmin[0] != xmin[1], xmax[0] != xmax[1], r[0] != r[1] in both.
LOW = dict(xmin=(0.065, 790 * W2PI), xmax=(0.145, 1500 * W2PI), r=(0.02, 600 * W2PI))
HIGH = dict(xmin=(0.065, 700 * W2PI), xmax=(0.145, 1210 * W2PI), r=(0.02, 1300 * W2PI))
CONSTS = {"low": LOW, "high": HIGH}
# Mode 0 has no rows, so nothing bounds its plans, and it is comparable to 1e-10 umax only
# at the reference's own operating point (x0 = [0; 2000 pi] with the default r, where every
# iteration's plan stays below 0.02 umax).  Anywhere else the LPV loop passes through plans of
# 1e4 - 1e10 umax (one ulp of such a U is 1e-12 - 1e-6 umax, fed back through rho(x)), and
# the reference's two restatements disagree with each other there: with r = (0.09 m,
# 900 * 2 pi) and x0 = r the NumPy and the C oracle end 0.11 umax apart; with r = (0.001 m,
# 900 * 2 pi) from the reference's x0 an intermediate plan reaches 6e9 umax.  So mode 0
# keeps the default r (whose two entries differ) and the reference's x0, as every teacher-
# forced test of the suite does; the state bounds, which mode 0 does not read, stay the
# non-default ones.
R_MODE0 = (0.0, 1000 * W2PI)
# plasma spread and w disturbance, as tests/test_gpu_scenarios.py sets them
GEN = O.ScenarioGen(seed=20241220, first_id=0, k0=0, sigma_w=1e-3, sigma_omega=0.0, jbs_spread=0.1,
                    wdep_spread=0.1)


def _force_far(ctl, B, cfg):
    ctl.set_small_batch(0)
    assert ctl.step_build(B, cfg) == "far"
    assert ctl.step_kernel_name(B, cfg) == FAR_NAME


def _step_against_oracle(ctl, cfg, ocfg, x, rho, Uo, gen=None):
    """One teacher-forced step, compared as tests/test_gpu_parity.py::_teacher_forced_loop
    compares it: exit flags exact; U / umax and the states (relative to |w| ~ 0.15 m and
    |omega| ~ 2000 pi) against the oracle for the scenarios whose LPV loop stopped at the
    oracle's inner iteration, and for the others against the oracle re-run along the
    kernel's path (its inner-iteration count, no early stop).  With these constants the
    loop stops between 2 and 10 iterations on sum |U - U_old| < 1e-14, a bitwise fixed
    point that two roundings reach an iteration apart for up to a third of the scenarios,
    so the share on the oracle's path is printed, not bounded; every scenario is compared
    on one path or the other.  Returns the worst U and state figures and the oracle's step."""
    from ntm_mpc import ScenarioGen
    B = x.shape[1]
    xscale = np.array([0.15, 2000 * math.pi])[:, None]
    if gen is not None:
        ctl.set_scenarios(ScenarioGen(**dataclasses.asdict(gen)))
    try:
        ref = cbind.step(x, rho, Uo, ocfg, gen=gen)
        out = ctl.step(T(x), T(rho), T(Uo), cfg)
        fl, gi, U, xn = H(out["exitflag"]), H(out["inner_iters"]), H(out["U"]), H(out["x_next"])
        xp = H(out["x_pred"]).reshape(N + 1, 2, B).transpose(1, 0, 2)
    finally:
        if gen is not None:
            ctl.set_scenarios(None)
    np.testing.assert_array_equal(fl, ref["exitflag"])
    same = gi == ref["inner_iters"]
    worst_u = np.zeros(B)
    worst_x = np.zeros(B)
    for i_g in np.unique(gi):
        sel = np.where(gi == i_g)[0]
        on_path = same[sel]
        rp = ref
        if not on_path.all():
            rp = cbind.step(x, rho, Uo, dataclasses.replace(ocfg, i_sim=int(i_g), epsilon=-1.0), gen=gen)
        for r_, idx in ((ref, sel[on_path]), (rp, sel[~on_path])):
            if idx.size == 0:
                continue
            xr = r_["x_pred"].reshape(N + 1, 2, B).transpose(1, 0, 2)
            worst_u[idx] = np.max(np.abs(U[:, idx] - r_["U"][:, idx]), axis=0) / cfg.umax
            worst_x[idx] = np.maximum(np.max(np.abs(xp[:, :, idx] - xr[:, :, idx]) / xscale[:, :, None], axis=(0, 1)),
                                      np.max(np.abs(xn[:, idx] - r_["x_next"][:, idx]) / xscale, axis=0))
    print(f"N={N} mode {cfg.mode} B={B}: max |U - U_oracle| / umax = {worst_u.max():.2e}, states {worst_x.max():.2e}, "
          f"on the oracle's path {int(same.sum())} of {B}")
    assert np.isfinite(U).all() and worst_u.max() <= U_TOL, worst_u
    assert worst_x.max() <= X_TOL, worst_x
    return {"worst": float(worst_u.max()), "worst_x": float(worst_x.max()), "ref": ref}


def _touches(ref, kw, B):
    """Per parity c, the scenarios whose oracle plan holds a predicted state of stage 2 or
    later (a row with two or more non-zeros: a general row) on a bound of component c."""
    xp = ref["x_pred"].reshape(N + 1, 2, B)
    out = []
    for c in (0, 1):
        lo = np.abs(xp[2:, c, :] - kw["xmin"][c]) <= 1e-9 * kw["xmin"][c]
        hi = np.abs(xp[2:, c, :] - kw["xmax"][c]) <= 1e-9 * kw["xmax"][c]
        out.append((lo.any(0), hi.any(0)))
    return out


@pytest.mark.parametrize("consts", ["low", "high"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_far_step_teacher_forced_asymmetric_constants(ctl, mode, consts):
    """B = 64, N = 20 on the far build, one teacher-forced step against the C oracle: U within
    1e-10 umax, the next and the predicted states within 1e-9, exit flags exact.  Mode 2,
    with the solver counters on: the oracle's own plans hold states on bounds of both
    parities (w and omega), and the kernel's final sets of exactly those scenarios hold
    general state rows."""
    kw = CONSTS[consts] if mode else dict(CONSTS[consts], r=R_MODE0)
    B = 64
    cfg, ocfg = cfgs(N, mode, **kw)
    x = O.scenario_x0(np.arange(B)).T if mode else np.tile(O.REFERENCE_X0[:, None], (1, B))
    rho, Uo = cbind.initial_state(x, ocfg)
    stats = torch.zeros((6, B), dtype=torch.int32, device=DEV)
    try:
        _force_far(ctl, B, cfg)
        ctl.set_stats(stats)
        res = _step_against_oracle(ctl, cfg, ocfg, x, rho, Uo)
        st = H(stats).astype(np.int64)
    finally:
        ctl.set_stats(None)
        ctl.set_small_batch(-1)
    if mode != 2:
        return
    ref = res["ref"]
    optimal = ref["exitflag"] == 1
    (w_lo, w_hi), (om_lo, om_hi) = _touches(ref, kw, B)
    print(f"oracle plans on a bound: w {int(w_lo.sum())} / {int(w_hi.sum())}, omega {int(om_lo.sum())} / {int(om_hi.sum())}; "
          f"general rows per scenario {st[3].tolist()}")
    # the reference alone: both parities, and the bounds named above for this set
    assert (w_hi & optimal).any() and ((om_lo if consts == "low" else om_hi) & optimal).any()
    if consts == "low":
        assert (w_lo & optimal).any()
    # the kernel's counters: the last QP's set of each such scenario holds general state rows
    both = (w_lo | w_hi | om_lo | om_hi) & optimal
    assert (st[0][both] > 0).all() and (st[3][both] > 0).all(), (st[0], st[3])


def test_far_step_state_bounds_at_x0(ctl):
    """The x_0 rows are constant rows (feasible_const / the scaling pass's folded test read
    xmin and xmax directly): x0 on each state bound, inside the 1e-9 tolerance of a constant
    row and 1e-6 outside it, on both components; the exit flags equal the oracle's, which
    hold both an optimal and an infeasible scenario."""
    kw = LOW
    cfg, ocfg = cfgs(N, 2, **kw)
    (w0, om0), (w1, om1) = kw["xmin"], kw["xmax"]
    wm, omm = 0.1, 1000 * W2PI
    x = np.array([[w0, omm], [w0 - 5e-10, omm], [w0 - 1e-6, omm], [w1, omm], [w1 + 1e-6, omm],
                  [wm, om0], [wm, om0 * (1 - 1e-6)], [wm, om1], [wm, om1 * (1 + 1e-6)], [wm, omm]]).T
    B = x.shape[1]
    rho, Uo = cbind.initial_state(x, ocfg)
    ref = cbind.step(x, rho, Uo, ocfg)
    try:
        _force_far(ctl, B, cfg)
        out = ctl.step(T(x), T(rho), T(Uo), cfg)
        fl = H(out["exitflag"])
    finally:
        ctl.set_small_batch(-1)
    print(f"exit flags {fl.tolist()}, oracle {ref['exitflag'].tolist()}")
    assert (ref["exitflag"][[2, 4, 6, 8]] == -2).all() and (ref["exitflag"] == 1).any()
    np.testing.assert_array_equal(fl, ref["exitflag"])


def test_far_step_with_generator(ctl):
    """One far-forced step at B = 8 with the scenario generator on (the GEN = true
    instantiation of the step kernel), asymmetric constants."""
    B = 8
    cfg, ocfg = cfgs(N, 2, **LOW)
    x = O.scenario_x0(np.arange(B)).T
    rho, Uo = cbind.initial_state_gen(x, ocfg, GEN)
    try:
        _force_far(ctl, B, cfg)
        _step_against_oracle(ctl, cfg, ocfg, x, rho, Uo, gen=GEN)
    finally:
        ctl.set_small_batch(-1)


def test_far_run_closed_loop(ctl):
    """B = 8, three closed-loop steps at N = 20, mode 2 through run (k_mpc_run) on the far
    build against the oracle, asymmetric constants, at the closed-loop tests' tolerance."""
    B, k_sim = 8, 3
    cfg, ocfg = cfgs(N, 2, **LOW)
    x0 = O.scenario_x0(np.arange(B)).T
    ref = cbind.run(x0, ocfg, k_sim)
    try:
        _force_far(ctl, B, cfg)
        out = ctl.run(T(x0), k_sim, cfg)
    finally:
        ctl.set_small_batch(-1)
    _assert_run_close(out, ref, cfg, k_sim, tol=RUN_TOL, x0=x0, ocfg=ocfg)


def test_rate_rows_at_n20_keep_the_runtime_n_kernel(ctl):
    """N = 20 mode 3 never reaches the far unit: with the far build forced the step still
    names the runtime-N kernel and its all-LDS build class as before, and one teacher-forced
    step at B = 8 matches the oracle."""
    B = 8
    cfg = cfgs(N, 3)[0]
    ctl.set_small_batch(0)
    try:
        assert ",NN=0," in ctl.step_kernel_name(B, cfg) and ",NN=0," in ctl.step_kernel_name(100_000, cfg)
        assert ctl.step_build(B, cfg) == "lds" and ctl.step_build(100_000, cfg) == "lds"
        res = _teacher_forced(ctl, N, 3, False, k_sim=1, B=B)
    finally:
        ctl.set_small_batch(-1)
    assert res["worst"] <= U_TOL and res["worst_div"] <= U_TOL and res["worst_x"] <= X_TOL, res
