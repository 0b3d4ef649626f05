"""The lane-masked triangular Gamma passes of the N = 20 far kernel (csrc/ntm_lanes.h, ntm_dots.h):
the row dots (fmac5_lanes_from / fmac5x2_lanes_from under gamma_row_dot /
gamma_row_dot2), the certificate's gradient (fadd5_lanes_upto under dot_rows2) and
the scaling pass's column pass (fadd5x2_class_lanes_upto, with its non-finite flag).

The stand-alone check compares every helper with the select form it replaces bit
for bit, the column helpers under partial entry EXEC too; the kernel tests run the
far build, forced at a small batch, through all of these passes against the C oracle
at the step tests' tolerance with the exit flags exact."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from checkprog import build_and_run
from oracle import cbind
from oracle import ntm_oracle as O
from test_gpu_parity import H, T, U_TOL, X_TOL, _teacher_forced, cfgs

pytestmark = pytest.mark.gpu

FAR_NAME = "k_mpc_step<P=64,NN=20,far>"


def test_masked_dot_check(tmp_path):
    """tools/masked_dot_check.hip: one 64-lane block, the row and the column helpers
    against the select form on random finite data over the whole packed Gamma,
    accumulators through -0.0, entry EXEC with the lanes >= 40 off and with an irregular
    pattern off (off lanes write nothing, keep their sums, set no non-finite bit), EXEC
    after the helper, non-finite data; one PASS line."""
    build_and_run("masked_dot_check", tmp_path, "-O3")


def test_far_build_two_teacher_forced_steps(ctl):
    """B = 5, N = 20, mode 2 on the far build: two teacher-forced steps against the C
    oracle, U within 1e-10 umax, exit flags exact."""
    ctl.set_small_batch(0)
    try:
        assert ctl.step_kernel_name(5, cfgs(20, 2)[0]) == FAR_NAME
        res = _teacher_forced(ctl, 20, 2, False, k_sim=2, B=5)
    finally:
        ctl.set_small_batch(-1)
    assert res["worst"] <= U_TOL and res["worst_div"] <= U_TOL and res["worst_x"] <= X_TOL, res


def test_far_build_mixed_fates(ctl):
    """One batch on the far build holding a NaN x_k (exit flag -7), the infeasible
    reference x_0 (-2) and healthy scenarios: flags exact, the failed scenarios' U zero,
    the healthy ones at the oracle's optimum."""
    cfg, ocfg = cfgs(20, 2)
    x = O.scenario_x0(np.arange(7)).T.copy()
    x[1, 1] = np.nan
    x[:, 4] = O.REFERENCE_X0
    good = np.array([0, 2, 3, 5, 6])
    rho, Uo = cbind.initial_state(x, ocfg)
    ref = cbind.step(x, rho, Uo, ocfg)
    np.testing.assert_array_equal(ref["exitflag"], [1, -7, 1, 1, -2, 1, 1])
    ctl.set_small_batch(0)
    try:
        assert ctl.step_kernel_name(7, cfg) == FAR_NAME
        out = ctl.step(T(x), T(rho), T(Uo), cfg)
        fl, U, xn = H(out["exitflag"]), H(out["U"]), H(out["x_next"])
    finally:
        ctl.set_small_batch(-1)
    np.testing.assert_array_equal(fl, ref["exitflag"])
    assert (U[:, fl != 1] == 0).all()
    du = np.max(np.abs(U - ref["U"])[:, good]) / cfg.umax
    dx = np.max((np.abs(xn - ref["x_next"]) / np.array([0.15, 2000 * np.pi])[:, None])[:, good])
    print(f"far build, mixed fates: max |U - U_oracle| / umax = {du:.2e}, next state {dx:.2e}")
    np.testing.assert_array_equal(H(out["inner_iters"])[good], ref["inner_iters"][good])
    assert du <= U_TOL and dx <= X_TOL, (du, dx)
