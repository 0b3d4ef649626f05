"""The aligned pair reads of the N = 20 far kernels (csrc/ntm_lanes.h: ld_pair, ld5; the
slim far N = 20 layout of csrc/ntm_ws.h, WS::kPair): the doubles [2i], [2i+1] of e, xp,
Phi, irn, the re-solve's scratch at Vb / Uf and of Gamma's columns, and the five-entry
chunks of U, d, dr, a11 and a21, are read as 16-byte aligned ds_read_b128 where the compiler
had paired them as ds_read2_b64, and uu moved to the head of the vector block so that
every one of those vectors starts on 16 bytes.

Loads only, so the results are the parent's bit for bit (the byte comparison of the
benchmark's outputs is recorded in profiles/r15_lds/bitwise.txt); these tests hold the three
kernels of the unit (the step kernel, its scenario-generator instantiation and the
closed-loop kernel), far build forced at small batches, against the C oracle at the suite's
1e-10 umax with the exit flags exact.  The pair reads sit in the scaling pass, the lift, the
certificate's y and gradient, the k = 1 line search and the rollout, so the inputs must reach
square echelon sets (k = 0), sets with a spare column (k = 1) and a set re-solved by the
bordered elimination (the polish of a Goldfarb-Idnani run).  The kernel's own counters say
which were reached (include/ntm_mpc.h, ntm_ctx_set_stats: per scenario the QPs, GI
iterations, active rows and general rows of the final sets, re-solve attempts, GI runs): a
QP's final set with N active rows is square, one with N - 1 has a spare column (the
oracle's own final sets at these inputs hold 19 or 20 rows, never fewer), and a GI run ends
in the bordered re-solve of its set."""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import pytest
import torch

from checkprog import build_and_run
from oracle import cbind
from oracle import ntm_oracle as O
from test_gpu_parity import DEV, H, RUN_TOL, T, U_TOL, X_TOL, _assert_run_close, cfgs

pytestmark = pytest.mark.gpu

FAR_NAME = "k_mpc_step<P=64,NN=20,far>"
N = 20
W2PI = 2 * math.pi
# Non-default, unequal state bounds and reference (tests/test_gpu_n20_consts.py's LOW set: the
# reference omega below omega's lower bound, so plans touch w's lower and upper bound and
# omega's lower one; xmin[0] != xmin[1], xmax[0] != xmax[1], r[0] != r[1])
LOW = dict(xmin=(0.065, 790 * W2PI), xmax=(0.145, 1500 * W2PI), r=(0.02, 600 * W2PI))
CONSTS = {"default": {}, "low": LOW}
# plasma spread and w disturbance, as tests/test_gpu_scenarios.py sets them
GEN = O.ScenarioGen(seed=20241220, first_id=0, k0=0, sigma_w=1e-3, sigma_omega=0.0, jbs_spread=0.1,
                    wdep_spread=0.1)


def _force_far(ctl, B, cfg):
    ctl.set_small_batch(0)
    assert ctl.step_build(B, cfg) == "far"
    assert ctl.step_kernel_name(B, cfg) == FAR_NAME


def _step_against_oracle(ctl, cfg, ocfg, x, rho, Uo, gen=None):
    """One teacher-forced step (as tests/test_gpu_n20_consts.py compares it): exit flags exact;
    U / umax and the states (relative to |w| ~ 0.15 m and |omega| ~ 2000 pi) against the
    oracle for the scenarios whose LPV loop stopped at the oracle's inner iteration, and for
    the others against the oracle re-run along the kernel's path (its inner-iteration count,
    no early stop).  Returns the oracle's step."""
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
          f"on the oracle's path {int(same.sum())} of {B}, exit flags {fl.tolist()}")
    assert np.isfinite(U).all() and worst_u.max() <= U_TOL, worst_u
    assert worst_x.max() <= X_TOL, worst_x
    return ref


def _three_steps(ctl, cfg, ocfg, x, gen=None, stats=None):
    """Three steps along the oracle's closed loop (each step starts from the oracle's next
    state, rho and U_old), each compared; returns the counters of each step."""
    B = x.shape[1]
    rho, Uo = cbind.initial_state(x, ocfg) if gen is None else cbind.initial_state_gen(x, ocfg, gen)
    per_step = []
    try:
        _force_far(ctl, B, cfg)
        if stats is not None:
            ctl.set_stats(stats)
        for k in range(3):
            if stats is not None:
                stats.zero_()
            g = None if gen is None else dataclasses.replace(gen, k0=gen.k0 + k)
            ref = _step_against_oracle(ctl, cfg, ocfg, x, rho, Uo, gen=g)
            if stats is not None:
                per_step.append(H(stats).astype(np.int64))
            x, rho, Uo = ref["x_next"], ref["rho"], ref["U_old"]
    finally:
        if stats is not None:
            ctl.set_stats(None)
        ctl.set_small_batch(-1)
    return per_step


def test_lds_read_forms_check(tmp_path):
    """tools/lds_read_forms_check.hip: one ds_read2_b64 offset1:1, two ds_read_b64 and one
    aligned ds_read_b128 return the same 16 bytes per lane, pairs at four offsets, every lane
    on and under two partial EXEC masks (a lane that is off writes nothing); it also prints
    the cycles per pair of each form in the kernel's shape (16 waves per CU).  One PASS line."""
    build_and_run("lds_read_forms_check", tmp_path, "-O3")


@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("consts", ["default", "low"])
def test_far_step_three_steps(ctl, consts, mode, B):
    """Scenarios 0..B-1 of the seeded set on the far build, three steps along the oracle's
    closed loop, each within 1e-10 umax / 1e-9 of the oracle with the exit flags exact.  Mode 2
    at the default operating point with the counters on: the three steps hold a scenario-step
    whose QPs all end on square sets (k = 0), one with a spare-column set (k = 1), and a GI
    run (whose set the bordered elimination re-solves)."""
    cfg, ocfg = cfgs(N, mode, **CONSTS[consts])
    x = O.scenario_x0(np.arange(B)).T
    counted = mode == 2 and consts == "default"
    stats = torch.zeros((6, B), dtype=torch.int32, device=DEV) if counted else None
    per_step = _three_steps(ctl, cfg, ocfg, x, stats=stats)
    if not counted:
        return
    square = spare = gi_runs = 0
    for k, st in enumerate(per_step):
        qps, act, tries, runs = st[0], st[2], st[4], st[5]
        print(f"step {k}: QPs {qps.tolist()}, active rows {act.tolist()}, re-solve attempts {tries.tolist()}, "
              f"GI runs {runs.tolist()}")
        assert (qps > 0).all()
        square += int((act == N * qps).sum())
        spare += int(((act < N * qps) & (act >= (N - 1) * qps)).sum())
        gi_runs += int(runs.sum())
    # the oracle's own final sets: scenario 1 holds 20 rows in every QP of every step, scenario 0
    # alternates 20 and 19 over its first step (and scenario 2, in the B = 3 batch too)
    assert square > 0 and spare > 0 and gi_runs > 0, (square, spare, gi_runs)


def test_far_step_next_to_a_w_bound(ctl):
    """Start states within 1e-9 of w's lower bound (5e-10 and 1e-10 above it, and 5e-10 above
    it at another omega), non-default bounds: in the oracle's plan the stage-1 w sits on the
    bound; three steps along the oracle's closed loop, every scenario optimal."""
    cfg, ocfg = cfgs(N, 2, **LOW)
    w0 = LOW["xmin"][0]
    omm = 1000 * W2PI
    x = np.array([[w0 + 5e-10, omm], [w0 + 1e-10, omm], [w0 + 5e-10, 900 * W2PI]]).T
    rho, Uo = cbind.initial_state(x, ocfg)
    ref = cbind.step(x, rho, Uo, ocfg)
    assert (ref["exitflag"] == 1).all(), ref["exitflag"]
    w_stage1 = ref["x_pred"].reshape(N + 1, 2, x.shape[1])[1, 0, :]
    assert (np.abs(w_stage1 - w0) <= 1e-9 * w0).all(), w_stage1
    _three_steps(ctl, cfg, ocfg, x)


@pytest.mark.parametrize("B", [3, 8])
def test_far_step_with_generator(ctl, B):
    """The GEN = true instantiation of the step kernel (plasma spread and w disturbance),
    non-default bounds: three steps along the oracle's closed loop."""
    cfg, ocfg = cfgs(N, 2, **LOW)
    _three_steps(ctl, cfg, ocfg, O.scenario_x0(np.arange(B)).T, gen=GEN)


@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("mode", [1, 2])
def test_far_run_closed_loop(ctl, mode, B):
    """Three closed-loop steps through run (k_mpc_run) on the far build against the oracle, at
    the closed-loop tests' tolerance; mode 2 with the non-default bounds."""
    k_sim = 3
    cfg, ocfg = cfgs(N, mode, **(LOW if mode == 2 else {}))
    x0 = O.scenario_x0(np.arange(B)).T
    ref = cbind.run(x0, ocfg, k_sim)
    try:
        _force_far(ctl, B, cfg)
        out = ctl.run(T(x0), k_sim, cfg)
    finally:
        ctl.set_small_batch(-1)
    _assert_run_close(out, ref, cfg, k_sim, tol=RUN_TOL, x0=x0, ocfg=ocfg)
