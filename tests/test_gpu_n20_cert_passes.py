"""The lane-masked row pass of the N = 20 far kernels' scaling pass (csrc/ntm_lanes.h:
rownorm5_lanes_from, under row_norm_lanes of csrc/ntm_gram.h): the norms of the scaled state
rows, each row's last non-zero column and the count of its non-zeros, unrolled over the
columns in chunks of five with EXEC narrowed to the rows a column reaches, where the loop
form computed every term on every lane and selected.

The stand-alone check compares the helper with the loop form bit for bit.  The kernel tests
run the three kernels that share it (the step kernel, its scenario-generator instantiation
and the closed-loop kernel), far build forced at a small batch, against the C oracle at the
step and closed-loop tests' tolerances.  What the pass writes (irn[r], rinfo[r]) reaches the
result through the general state rows of an active set, so the batch must hold sets with
six and more of them, square sets (k = 0) and sets with a spare column (k = 1); one more
case starts next to a w bound, where the stage-1 w row (a single non-zero) is active next
to its constant omega row."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from checkprog import build_and_run
from oracle import cbind
from oracle import ntm_oracle as O
from test_gpu_n20_consts import LOW, _force_far, _step_against_oracle
from test_gpu_parity import DEV, H, RUN_TOL, T, U_TOL, X_TOL, _assert_run_close, _teacher_forced, _teacher_forced_loop, cfgs

pytestmark = pytest.mark.gpu

FAR_NAME = "k_mpc_step<P=64,NN=20,far>"
N, B = 20, 8
W2PI = 2 * math.pi
# The scenarios are ids 0..7 of the seeded set (O.scenario_x0).  The oracle's own optimal
# sets over their first two steps in mode 2 (O.qp_solve's active rows of each QP of the LPV
# loop, the general ones being those with two or more non-zeros):
#   general rows, 6 and more per QP over a step: ids 1, 4 (13 and 0 alternating: 6.5) and
#       7 (13-14 and 4-5: 8.9 and 9.3);
#   every QP of a step with 20 active rows (k = 0): ids 1, 4 and 6;
#   QPs with 19 (k = 1): id 0 (19.5 per QP at its first step) and id 3 (every other QP of
#       its second step).
IDS_GENERAL = (1, 4, 7)
IDS_SQUARE = (1, 4, 6)
IDS_SPARE = (0, 3)
# plasma spread and w disturbance, as tests/test_gpu_scenarios.py sets them
GEN = O.ScenarioGen(seed=20241220, first_id=0, k0=0, sigma_w=1e-3, sigma_omega=0.0, jbs_spread=0.1,
                    wdep_spread=0.1)


def test_cert_passes_check(tmp_path):
    """tools/cert_passes_check.hip: one 64-lane block per case; the row pass against the loop
    form: rows with no, one and several non-zeros placed first, last and in the middle,
    exact zeros and -0.0, an infinity and a NaN inside and outside a row's range, a non-finite
    D_j, sums seeded on entry, four entry EXECs (full, the lanes >= 2N off, two irregular
    patterns); a lane off on entry holds a sentinel in s, last and cnt before the branch
    and must hold the same bits after it has reconverged; one PASS line."""
    build_and_run("cert_passes_check", tmp_path, "-O3")


@pytest.mark.parametrize("mode", [1, 2])
def test_far_step_two_teacher_forced_steps(ctl, mode):
    """B = 8, N = 20 on the far build: two teacher-forced steps against the C oracle, U
    within 1e-10 umax, the next and the predicted states within 1e-9, exit flags exact.
    Mode 2 with the solver counters on, one step at a time: the batch must hold a
    scenario-step with six or more general rows per QP, one with more than N - 1 active
    rows per QP (a k = 0 set) and one with fewer than N (a k >= 1 set), on the scenarios
    named above."""
    cfg, ocfg = cfgs(N, mode)
    x = O.scenario_x0(np.arange(B)).T
    rho, Uo = cbind.initial_state(x, ocfg)
    stats = torch.zeros((6, B), dtype=torch.int32, device=DEV)
    per_step = []
    ctl.set_small_batch(0)
    try:
        assert ctl.step_kernel_name(B, cfg) == FAR_NAME
        ctl.set_stats(stats)
        for k in range(2):
            stats.zero_()
            res = _teacher_forced_loop(ctl, N, mode, False, 1, None, cfg, ocfg, B, x, rho, Uo)
            assert res["worst"] <= U_TOL and res["worst_div"] <= U_TOL and res["worst_x"] <= X_TOL, res
            per_step.append(H(stats).astype(np.int64))
            ref = res["refs"][-1]
            x, rho, Uo = ref["x_next"], ref["rho"], ref["U_old"]
    finally:
        ctl.set_stats(None)
        ctl.set_small_batch(-1)
    if mode != 2:
        return
    general, square, spare = set(), set(), set()
    for k, st in enumerate(per_step):
        qps, act, gen = st[0], st[2], st[3]
        print(f"step {k}: QPs {qps.tolist()}, active rows {act.tolist()}, general rows {gen.tolist()}")
        assert (qps > 0).all()
        general |= {s for s in range(B) if gen[s] >= 6 * qps[s]}
        square |= {s for s in range(B) if act[s] > (N - 1) * qps[s]}
        spare |= {s for s in range(B) if act[s] < N * qps[s]}
    assert set(IDS_GENERAL) <= general, general
    assert set(IDS_SQUARE) <= square, square
    assert set(IDS_SPARE) <= spare, spare


def test_far_step_next_to_a_w_bound(ctl):
    """x0 within 1e-9 of w's lower bound (5e-10, 1e-10 and 0 above it, at two omega), one at
    its upper bound and one in the interior, the reference below the lower bound: in the
    oracle's plan of the first four the stage-1 w sits on the bound, so the row with a single
    non-zero (rinfo's single-entry form) is active next to its constant omega row; one
    teacher-forced step against the oracle, every scenario optimal and compared."""
    cfg, ocfg = cfgs(N, 2, **LOW)
    (w0, _), (w1, _) = LOW["xmin"], LOW["xmax"]
    omm = 1000 * W2PI
    x = np.array([[w0 + 5e-10, omm], [w0 + 1e-10, omm], [w0, omm], [w0 + 5e-10, 900 * W2PI], [w1 - 5e-10, omm],
                  [0.1, omm]]).T
    rho, Uo = cbind.initial_state(x, ocfg)
    try:
        _force_far(ctl, x.shape[1], cfg)
        res = _step_against_oracle(ctl, cfg, ocfg, x, rho, Uo)
    finally:
        ctl.set_small_batch(-1)
    ref = res["ref"]
    assert (ref["exitflag"] == 1).all(), ref["exitflag"]
    w_stage1 = ref["x_pred"].reshape(N + 1, 2, x.shape[1])[1, 0, :]
    assert (np.abs(w_stage1[:4] - w0) <= 1e-9 * w0).all() and (w_stage1[4:] - w0 > 1e-3).all(), w_stage1


def test_far_step_with_generator(ctl):
    """One far-forced step at B = 8 with the scenario generator on: the GEN = true
    instantiation of the step kernel."""
    ctl.set_small_batch(0)
    try:
        assert ctl.step_kernel_name(B, cfgs(N, 2)[0]) == FAR_NAME
        res = _teacher_forced(ctl, N, 2, False, k_sim=1, B=B, gen=GEN)
    finally:
        ctl.set_small_batch(-1)
    assert res["worst"] <= U_TOL and res["worst_div"] <= U_TOL and res["worst_x"] <= X_TOL, res


def test_far_run_closed_loop(ctl):
    """B = 8, three closed-loop steps at N = 20, mode 2 through run (k_mpc_run) on the far
    build against the oracle, at the closed-loop tests' tolerance."""
    k_sim = 3
    cfg, ocfg = cfgs(N, 2)
    x0 = O.scenario_x0(np.arange(B)).T
    ref = cbind.run(x0, ocfg, k_sim)
    ctl.set_small_batch(0)
    try:
        out = ctl.run(T(x0), k_sim, cfg)
    finally:
        ctl.set_small_batch(-1)
    _assert_run_close(out, ref, cfg, k_sim, tol=RUN_TOL, x0=x0, ocfg=ocfg)
