"""CPU checks of tests/resume_ref.py, the reference the GPU tests of the resumable closed
loops (tests/test_gpu_run_from.py) are held to: with a constant schedule the composition
is the oracle's own closed loop bit for bit, a chunked composition is the unchunked one,
and the umax-halving schedule the GPU tests use is feasible and really binds.
"""
import dataclasses

import numpy as np
import pytest

import estimator_ref as E
import resume_ref as R
from oracle import cbind
from oracle import ntm_oracle as O

B, K = 9, 5
GEN = O.ScenarioGen(seed=20241220, first_id=0, k0=2, sigma_w=1e-3, sigma_omega=0.0, jbs_spread=0.1, wdep_spread=0.1)


def x0_of(n=B):
    return np.ascontiguousarray(O.scenario_x0(np.arange(n)).T)


@pytest.mark.parametrize("N,mode", [(20, 2), (20, 1), (10, 2)])
@pytest.mark.parametrize("gen", [None, GEN], ids=["nominal", "gen"])
def test_constant_schedule_is_the_oracle_run(N, mode, gen):
    cfg = O.Config(N=N, mode=mode)
    x0 = x0_of()
    ref = cbind.run(x0, cfg, K, gen=gen)
    h, _ = R.run(x0, K, R.constant(cfg, gen))
    for k in ref:
        np.testing.assert_array_equal(h[k], ref[k], err_msg=k)
    assert np.all(ref["exitflag"] == 1)


def test_chunks_compose():
    cfg = O.Config(N=20, mode=2)
    x0 = x0_of()
    sched = R.constant(cfg, GEN)
    h, st = R.run(x0, K, sched)
    rho, Uo = cbind.initial_state_gen(x0, cfg, GEN)
    h1, s1 = R.run_from(x0, rho, Uo, 2, sched)
    h2, s2 = R.run_from(*s1, 3, sched, k_first=2)
    np.testing.assert_array_equal(np.vstack([h1["uk"], h2["uk"]]), h["uk"])
    np.testing.assert_array_equal(np.vstack([h1["xk"], h2["xk"][2:]]), h["xk"])
    for a, b in zip(s2, st):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("N", [20, 10])
def test_umax_halving_is_feasible_and_binds(N):
    """umax halves after step 2 (steps 2, 3, 4 run with the new bound): every flag stays 1
    and more than half of the applied inputs after the change sit on the new bound."""
    cfg = O.Config(N=N, mode=2)
    half = dataclasses.replace(cfg, umax=cfg.umax / 2)
    h, _ = R.run(x0_of(), K, R.switch_at(2, (cfg, None), (half, None)))
    assert np.all(h["exitflag"] == 1)
    late = h["uk"][2:]
    assert np.all(late <= half.umax * (1 + 1e-12))
    on_bound = np.abs(late - half.umax) <= 1e-9 * cfg.umax
    assert 2 * on_bound.sum() >= late.size, on_bound.sum()
    assert np.any(h["uk"][:2] > half.umax)          # the old bound was in use before


def test_est_constant_schedule_is_estimator_ref_run():
    cfg = O.Config(N=6, mode=1)
    x0 = x0_of(4)
    opts = dict(nominal=True, gain=(0.5, 0.2), kappa=(0.5, 0.25), sigma_y=(2.0 ** -10, 16.0))
    ref = E.run(x0, cfg, 3, GEN, **opts)
    rho, Uo = E.M.initial_state(x0, cfg, GEN, True, None)
    h, _ = R.run_est_from(x0, x0, rho, Uo, np.zeros((2, 4)), 3, lambda k: (cfg, GEN, opts))
    for k in ref:
        np.testing.assert_array_equal(h[k], ref[k], err_msg=k)
