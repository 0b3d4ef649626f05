"""The lane-masked triangular substitutions of the N = 20 far kernels' echelon re-solve
(csrc/ntm_lanes.h: fsub_lanes / bsub_lanes; under polish_compact, csrc/ntm_device.h): the forward
substitution E V = h (with E Z = -e_c when k = 1) and the certificate's back
substitution E' mu = grad run unrolled in batches of five steps with EXEC narrowed
to the lanes a step touches, where they used to compute on every lane and select.

The stand-alone check compares the helpers with the loop form bit for bit.  The
kernel tests run the three kernels that share them (the step kernel, its scenario-
generator instantiation and the closed-loop kernel), far build forced at a small
batch, against the C oracle at the step and closed-loop tests' tolerances, on
scenarios whose optimal sets reach the new code: triangular systems of six rows
and more (a second batch of steps), square sets (k = 0, one right-hand side) and
sets with a spare column (k = 1, two)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from checkprog import build_and_run
from oracle import cbind
from oracle import ntm_oracle as O
from test_gpu_parity import DEV, H, RUN_TOL, T, U_TOL, X_TOL, _assert_run_close, _teacher_forced, _teacher_forced_loop, cfgs

pytestmark = pytest.mark.gpu

FAR_NAME = "k_mpc_step<P=64,NN=20,far>"
N, B = 20, 8
# The scenarios are ids 0..7 of the seeded set (O.scenario_x0).  The oracle's own optimal
# sets over their first two steps in mode 2 (O.qp_solve's active rows of each QP of the
# LPV loop, the general ones being those with two or more non-zeros):
#   general rows, 6 and more per QP over a step: ids 1, 4 (13 and 0 alternating: 6.5) and
#       7 (13-14 and 4-5: 8.9 and 9.3), id 0 at its second step (12 and 0);
#   every QP of a step with 20 active rows (k = 0): ids 1, 4 and 6, id 7 at its first step;
#   QPs with 19 (k = 1): id 0 (19.5 per QP at its first step), id 3 (19 rows, 7 of them
#       general, every other QP of its second step), id 7 at its second step (19, 5).
IDS_GENERAL = (1, 4, 7)
IDS_SQUARE = (1, 4, 6)
IDS_SPARE = (0, 3)
# plasma spread and w disturbance, as tests/test_gpu_scenarios.py sets them
GEN = O.ScenarioGen(seed=20241220, first_id=0, k0=0, sigma_w=1e-3, sigma_omega=0.0, jbs_spread=0.1,
                    wdep_spread=0.1)


def test_echelon_sub_check(tmp_path):
    """tools/echelon_sub_check.hip: one 64-lane block per case; the helpers against the loop
    form for every n = 0..20 and nc = -1..n, random lower-triangular E with exact zeros,
    -0.0 right-hand sides, an infinity and a NaN in h, in an element and in a diagonal
    reciprocal, three entry EXECs, a signalling NaN past the triangle; one PASS line."""
    build_and_run("echelon_sub_check", tmp_path, "-O3")


@pytest.mark.parametrize("mode", [1, 2])
def test_far_step_two_teacher_forced_steps(ctl, mode):
    """B = 8, N = 20 on the far build: two teacher-forced steps against the C oracle, U
    within 1e-10 umax, the next and the predicted states within 1e-9, exit flags exact.
    Mode 2 with the solver counters on, one step at a time: the batch must hold a
    scenario-step with six or more general rows per QP, one with more than N - 1 active
    rows per QP (a k = 0 set occurred) and one with fewer than N (a k >= 1 set occurred),
    on the scenarios named above."""
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


@pytest.mark.parametrize("small_batch", [-1, 0])
def test_rate_rows_at_n20_run_on_the_generic_kernels(ctl, small_batch):
    """N = 20 with input-rate rows (mode 3) takes the runtime-N kernels at every batch size,
    never an N = 20 specialisation: those kernels rely on it (polish_compact's echelon
    paths at N = 20 hold no collision handling for rate rows).  The name query needs a
    context, hence a device."""
    ctl.set_small_batch(small_batch)
    try:
        names = {ctl.step_kernel_name(b, cfgs(N, 3)[0]) for b in (1, B, 100_000)}
    finally:
        ctl.set_small_batch(-1)
    assert names and all(",NN=0," in n for n in names), names


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
