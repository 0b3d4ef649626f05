"""The V-space input box of the slim far N = 20 kernels (csrc/ntm_ws.h: WS::kBox).  The scaling
pass writes vlo = umin / D and vhi = umax / D once per QP into the 2N doubles of the lift's
a11 / a21, which are dead from the end of the lift's recursion to the next lift;
StructRows::check reads them where it divided twice per call.  (polish_compact still divides
uf / D_l once per re-solve: taking a bound-fixed variable's value from vlo / vhi measured
inside the run-to-run spread and was not kept)

The kernels of the unit (the step kernel, its scenario-generator instantiation, run,
run_from), far build forced at B = 8, against the C oracle at the tolerances
tests/test_gpu_n20_cert_passes.py uses for the same comparisons, exit flags exact.  Inputs,
chosen with the oracle alone (cbind.step / cbind.run on ids 0..7 of the seeded set):

  umin = 1e5, umax = 1.2e6 (neither the defaults nor symmetric, so lo != -hi).  Mode 2, first
      step: the plans of ids 0, 3, 5 hold inputs on both bounds (8 / 12, 9 / 11, 1 / 19 of 20),
      ids 4 and 7 one and two on the upper one, ids 1, 2, 6 all 20 on the lower one; the second
      and third closed-loop steps keep ids 0, 3, 5 on both.  Mode 1: at least 19 of the 20
      variables of every plan on a bound (ids 0, 3, 5 on both).  Ids 0, 3, 5 run 6 to 10 LPV
      iterations a step, so their QPs from the third on are certified candidates.
  next to a w bound (the construction of test_gpu_n20_cert_passes.py, with umin = -1e5, umax =
      7.5e5): id 3 (omega = 900 * 2 pi) holds w on its lower bound from stage 1 on, so the
      stage-1 w row, a single non-zero, fixes u_0 at 1.879e5 (between the bounds: a fixed
      variable whose V-space value is neither vlo nor vhi), while u_18 and u_19 sit on umax
      in the same plan.

Each property is asserted from the oracle's plan and from what the kernels return (inputs
exactly on a bound, the solver counters, the multipliers of step_dual), so a batch that does
not hold the case fails instead of passing empty."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from oracle import cbind
from oracle import ntm_oracle as O
from test_gpu_n20_consts import LOW, _force_far, _step_against_oracle
from test_gpu_parity import DEV, H, RUN_TOL, T, U_TOL, X_TOL, _assert_run_close, _teacher_forced_loop, cfgs

pytestmark = pytest.mark.gpu

N, B = 20, 8
W2PI = 2 * math.pi
BOX = dict(umin=1e5, umax=1.2e6)
IDS_BOTH = (0, 3, 5)                                     # plans with inputs on both bounds
# plasma spread and w disturbance, as tests/test_gpu_scenarios.py sets them
GEN = O.ScenarioGen(seed=20241220, first_id=0, k0=0, sigma_w=1e-3, sigma_omega=0.0, jbs_spread=0.1,
                    wdep_spread=0.1)


def _on_bounds(U, kw):
    """Per scenario, the number of inputs exactly on umin and exactly on umax."""
    return (U == kw["umin"]).sum(0), (U == kw["umax"]).sum(0)


@pytest.mark.parametrize("mode", [1, 2])
def test_far_step_asymmetric_input_bounds(ctl, mode):
    """Two teacher-forced steps at B = 8 on the far build, umin != -umax.  The oracle's plans
    and the kernel's hold inputs exactly on the lower bound and exactly on the upper one, in
    one plan for ids 0, 3, 5; in mode 1 at least N - 1 inputs of every plan sit on a bound;
    the solver counters show QPs in every scenario and candidate re-solves in those three."""
    cfg, ocfg = cfgs(N, mode, **BOX)
    x = O.scenario_x0(np.arange(B)).T
    rho, Uo = cbind.initial_state(x, ocfg)
    stats = torch.zeros((6, B), dtype=torch.int32, device=DEV)
    try:
        _force_far(ctl, B, cfg)
        ctl.set_stats(stats)
        for k in range(2):
            stats.zero_()
            xk, rk, uk = T(x), T(rho), T(Uo)
            res = _teacher_forced_loop(ctl, N, mode, False, 1, None, cfg, ocfg, B, x, rho, Uo)
            assert res["worst"] <= U_TOL and res["worst_div"] <= U_TOL and res["worst_x"] <= X_TOL, res
            st = H(stats).astype(np.int64)
            ref = res["refs"][-1]
            assert (ref["exitflag"] == 1).all(), ref["exitflag"]
            out = ctl.step(xk, rk, uk, cfg)
            U = H(out["U"])
            (rlo, rhi), (glo, ghi) = _on_bounds(ref["U"], BOX), _on_bounds(U, BOX)
            print(f"mode {mode} step {k}: oracle on umin {rlo.tolist()} umax {rhi.tolist()}, kernel {glo.tolist()} {ghi.tolist()}, "
                  f"QPs {st[0].tolist()}, candidates {st[4].tolist()}")
            for s in IDS_BOTH:
                assert rlo[s] > 0 and rhi[s] > 0, (s, rlo, rhi)
            np.testing.assert_array_equal(glo, rlo)
            np.testing.assert_array_equal(ghi, rhi)
            if mode == 1:
                assert (rlo + rhi >= N - 1).all(), (rlo, rhi)
            assert (st[0] > 0).all() and (st[4][list(IDS_BOTH)] > 0).all(), (st[0], st[4])
            x, rho, Uo = ref["x_next"], ref["rho"], ref["U_old"]
    finally:
        ctl.set_stats(None)
        ctl.set_small_batch(-1)


def test_far_step_single_entry_row_next_to_bound_fixed_inputs(ctl):
    """x0 within 1e-9 of w's lower bound: in id 3's plan the stage-1 w row (one non-zero)
    fixes u_0 strictly between the input bounds while u_18 and u_19 sit on umax; one
    teacher-forced step against the oracle.  The multipliers of the same QP (step_dual) are
    positive on the stage-1 w row and on the two upper-bound rows."""
    kw = dict(LOW, umin=-1e5, umax=7.5e5)
    cfg, ocfg = cfgs(N, 2, **kw)
    (w0, _), (w1, _) = LOW["xmin"], LOW["xmax"]
    omm = 1000 * W2PI
    x = np.array([[w0 + 5e-10, omm], [w0 + 1e-10, omm], [w0, omm], [w0 + 5e-10, 900 * W2PI], [w1 - 5e-10, omm],
                  [0.1, omm]]).T
    Bc, s = x.shape[1], 3
    rho, Uo = cbind.initial_state(x, ocfg)
    try:
        _force_far(ctl, Bc, cfg)
        res = _step_against_oracle(ctl, cfg, ocfg, x, rho, Uo)
        out = ctl.step(T(x), T(rho), T(Uo), cfg)
        U = H(out["U"])
        dual = ctl.step_dual(T(x), T(rho), T(Uo), cfg)
        lam, dflag = H(dual["lambda"]), H(dual["exitflag"])
    finally:
        ctl.set_small_batch(-1)
    ref = res["ref"]
    assert (ref["exitflag"] == 1).all(), ref["exitflag"]
    w_stage1 = ref["x_pred"].reshape(N + 1, 2, Bc)[1, 0, :]
    assert abs(w_stage1[s] - w0) <= 1e-9 * w0, w_stage1
    for Us in (ref["U"][:, s], U[:, s]):
        assert kw["umin"] < Us[0] < kw["umax"], Us
        assert Us[18] == kw["umax"] and Us[19] == kw["umax"], Us
    (rlo, rhi), (glo, ghi) = _on_bounds(ref["U"], kw), _on_bounds(U, kw)
    print(f"oracle on umin {rlo.tolist()} umax {rhi.tolist()}, kernel {glo.tolist()} {ghi.tolist()}")
    np.testing.assert_array_equal(glo, rlo)
    np.testing.assert_array_equal(ghi, rhi)
    assert (rlo[4:] > 0).all(), rlo                       # ids 4, 5: inputs on the lower bound
    # row ids (getWLc): 6 j + 1 = u_j <= umax, 6 i + 2 = w_i >= w_min (stage i < N)
    assert dflag[s] == 1
    print(f"multipliers of id {s}: stage-1 w row {lam[8, s]:.3e}, upper bounds {lam[6 * 18 + 1, s]:.3e} {lam[6 * 19 + 1, s]:.3e}")
    assert lam[8, s] > 0 and lam[6 * 18 + 1, s] > 0 and lam[6 * 19 + 1, s] > 0, lam[:, s]


def test_far_step_with_generator(ctl):
    """One far-forced step at B = 8 with the scenario generator on (the GEN = true
    instantiation of the step kernel), umin != -umax."""
    cfg, ocfg = cfgs(N, 2, **BOX)
    x = O.scenario_x0(np.arange(B)).T
    rho, Uo = cbind.initial_state_gen(x, ocfg, GEN)
    try:
        _force_far(ctl, B, cfg)
        res = _step_against_oracle(ctl, cfg, ocfg, x, rho, Uo, gen=GEN)
    finally:
        ctl.set_small_batch(-1)
    lo, hi = _on_bounds(res["ref"]["U"], BOX)
    assert (lo > 0).any() and (hi > 0).any(), (lo, hi)


def test_far_run_and_run_from_cross_the_lift(ctl):
    """Two closed-loop steps through run (k_mpc_run) against the oracle at the closed-loop
    tolerance, and the same two as run_from of one step each (a state hand-over between them),
    bit for bit run's: the second step's lift rewrites a11 / a21 over the first step's box.
    The second step's plans, the oracle's and the kernels', hold inputs on both bounds."""
    k_sim = 2
    cfg, ocfg = cfgs(N, 2, **BOX)
    x0 = O.scenario_x0(np.arange(B)).T
    ref = cbind.run(x0, ocfg, k_sim)
    stats = torch.zeros((6, B), dtype=torch.int32, device=DEV)
    try:
        _force_far(ctl, B, cfg)
        ctl.set_stats(stats)
        out = ctl.run(T(x0), k_sim, cfg)
        st = H(stats).astype(np.int64)
        x = T(x0)
        rho, uo = ctl.initial_state(x, cfg)
        ws = ctl.new_active_ws(B, cfg)
        parts = [{k: H(v).copy() for k, v in ctl.run_from(x, rho, uo, ws, 1, cfg).items()} for _ in range(k_sim)]
    finally:
        ctl.set_stats(None)
        ctl.set_small_batch(-1)
    _assert_run_close(out, ref, cfg, k_sim, tol=RUN_TOL, x0=x0, ocfg=ocfg)
    assert (ref["exitflag"] == 1).all(), ref["exitflag"]
    Uk, rUk = H(out["Uk"]).reshape(k_sim, N, B), ref["Uk"].reshape(k_sim, N, B)
    for k in range(k_sim):
        (rlo, rhi), (glo, ghi) = _on_bounds(rUk[k], BOX), _on_bounds(Uk[k], BOX)
        print(f"step {k}: oracle on umin {rlo.tolist()} umax {rhi.tolist()}, run {glo.tolist()} {ghi.tolist()}")
        for s in IDS_BOTH:
            assert rlo[s] > 0 and rhi[s] > 0, (k, s, rlo, rhi)
        np.testing.assert_array_equal(glo, rlo)
        np.testing.assert_array_equal(ghi, rhi)
    assert (st[0] > 0).all() and (st[4][list(IDS_BOTH)] > 0).all(), (st[0], st[4])
    for k, part in enumerate(parts):
        np.testing.assert_array_equal(part["Uk"], H(out["Uk"])[N * k:N * (k + 1)])
        np.testing.assert_array_equal(part["uk"], H(out["uk"])[k:k + 1])
        np.testing.assert_array_equal(part["exitflag"], H(out["exitflag"])[k:k + 1])
        np.testing.assert_array_equal(part["xk"], H(out["xk"])[2 * k:2 * k + 4])
