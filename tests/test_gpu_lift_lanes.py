"""The lane-masked lift recursion of the N = 20 far kernels (csrc/ntm_lanes.h:
lift_chunk_lanes; csrc/ntm_lift.h: lift_chunk_at under lift_phase's slim branch): stage i of
Gamma's columns and of the free response runs with EXEC narrowed to the lanes
that advance at that stage, where it used to compute on every lane and select.

The stand-alone check compares the lift with the select form bit for bit over
the whole packed Gamma, e and the words around them.  The kernel tests run the
three kernels that share the lift (the step kernel, its scenario-generator
instantiation and the closed-loop kernel), far build forced at a small batch,
against the C oracle at the step and closed-loop tests' tolerances."""
from __future__ import annotations

import math

import numpy as np
import pytest

from checkprog import build_and_run
from oracle import cbind
from oracle import ntm_oracle as O
from test_gpu_parity import H, RUN_TOL, T, U_TOL, X_TOL, _assert_run_close, _teacher_forced, cfgs

pytestmark = pytest.mark.gpu

FAR_NAME = "k_mpc_step<P=64,NN=20,far>"
# plasma spread and w disturbance, as tests/test_gpu_scenarios.py sets them
GEN = O.ScenarioGen(seed=20241220, first_id=0, k0=0, sigma_w=1e-3, sigma_omega=0.0, jbs_spread=0.1,
                    wdep_spread=0.1)


def test_lift_lanes_check(tmp_path):
    """tools/lift_lanes_check.hip: one 64-lane block; the product's lift against the
    select form on random finite coefficients, with an infinity and a NaN in a11 / a21 /
    b of a middle stage and of stage 0 and a NaN x_k (the columns the value cannot reach
    unchanged), the chunk helpers under the kernel's entry EXEC, all 64 lanes on and an
    irregular subset (lanes above N and lanes off on entry write nothing), EXEC after the
    helpers; one PASS line."""
    build_and_run("lift_lanes_check", tmp_path, "-O3")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_far_step_two_teacher_forced_steps(ctl, mode):
    """B = 5, N = 20 on the far build: two teacher-forced steps against the C oracle,
    U within 1e-10 umax, the next and the predicted states within 1e-9, exit flags
    exact (mode 3 at N = 20 runs the generic kernels)."""
    ctl.set_small_batch(0)
    try:
        assert ctl.step_kernel_name(5, cfgs(20, mode)[0]) == FAR_NAME
        res = _teacher_forced(ctl, 20, mode, False, k_sim=2, B=5)
    finally:
        ctl.set_small_batch(-1)
    assert res["worst"] <= U_TOL and res["worst_div"] <= U_TOL and res["worst_x"] <= X_TOL, res


def test_far_step_with_generator(ctl):
    """One far-forced step at B = 5 with the scenario generator on: the GEN = true
    instantiation, whose C1 and b coefficient are each scenario's own."""
    ctl.set_small_batch(0)
    try:
        assert ctl.step_kernel_name(5, cfgs(20, 2)[0]) == FAR_NAME
        res = _teacher_forced(ctl, 20, 2, False, k_sim=1, B=5, gen=GEN)
    finally:
        ctl.set_small_batch(-1)
    assert res["worst"] <= U_TOL and res["worst_div"] <= U_TOL and res["worst_x"] <= X_TOL, res


def test_far_run_closed_loop(ctl):
    """B = 5, three closed-loop steps at N = 20, mode 2 through run (k_mpc_run) on the
    far build against the oracle, at the closed-loop tests' tolerance."""
    B, k_sim = 5, 3
    cfg, ocfg = cfgs(20, 2)
    x0 = O.scenario_x0(np.arange(B)).T
    ref = cbind.run(x0, ocfg, k_sim)
    ctl.set_small_batch(0)
    try:
        out = ctl.run(T(x0), k_sim, cfg)
    finally:
        ctl.set_small_batch(-1)
    _assert_run_close(out, ref, cfg, k_sim, tol=RUN_TOL, x0=x0, ocfg=ocfg)


def test_far_step_prediction_reads_the_lift(ctl):
    """x_pred of a certified plan is e + Gamma U from the lift's own LDS: one far-forced
    step in mode 2, every scenario optimal and on the oracle's path, the predicted states
    against the oracle's within 1e-9 of |w| ~ 0.15 m and |omega| ~ 2000 pi."""
    B, N = 5, 20
    cfg, ocfg = cfgs(N, 2)
    x = O.scenario_x0(np.arange(B)).T
    rho, Uo = cbind.initial_state(x, ocfg)
    ref = cbind.step(x, rho, Uo, ocfg)
    ctl.set_small_batch(0)
    try:
        assert ctl.step_kernel_name(B, cfg) == FAR_NAME
        out = ctl.step(T(x), T(rho), T(Uo), cfg)
        fl, it, xp = H(out["exitflag"]), H(out["inner_iters"]), H(out["x_pred"])
    finally:
        ctl.set_small_batch(-1)
    np.testing.assert_array_equal(fl, ref["exitflag"])
    assert (fl == 1).all()
    np.testing.assert_array_equal(it, ref["inner_iters"])
    xscale = np.array([0.15, 2000 * math.pi])[:, None, None]
    xg = xp.reshape(N + 1, 2, B).transpose(1, 0, 2)
    xr = ref["x_pred"].reshape(N + 1, 2, B).transpose(1, 0, 2)
    d = float(np.max(np.abs(xg - xr) / xscale))
    print(f"far build, x_pred against the oracle: {d:.2e}")
    assert np.isfinite(xg).all() and d <= X_TOL, d
