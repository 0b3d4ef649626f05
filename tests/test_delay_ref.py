"""CPU checks of tests/delay_ref.py, the reference the GPU dead-time tests
(tests/test_gpu_delay.py) are held to: its degenerate case against tests/estimator_ref.py,
the exit flags of the inputs the GPU tests use, the queue's bookkeeping, and the exactness
of the delay-compensating plan where the model is the plant.
"""
import numpy as np
import pytest

import delay_ref as D
import estimator_ref as E
from oracle import ntm_oracle as O

from test_estimator_ref import GAIN, GEN, KAPPA, SIGMA_Y, x0_of, xhat0_of

NOISY = dict(nominal=True, gain=GAIN, kappa=KAPPA, sigma_y=SIGMA_Y)
# the exactness property's inputs: the model is the plant, the estimate is the state
EXACT = dict(nominal=True, gain=0.0, kappa=0.0, sigma_y=0.0)
EXACT_CASES = [(6, 1), (12, 2), (20, 2), (20, 3), (24, 2)]
EXACT_DELAYS = (1, 3, 8)
EXACT_STEPS = 12


def q0_of(B):
    """The initial queue of the d = 2 cases: q0[j, s] = (5e5, 1.5e6)[j] (1 + 0.1 cos s)."""
    return np.ascontiguousarray(np.array([5e5, 1.5e6])[:, None] * (1.0 + 0.1 * np.cos(np.arange(B)))[None, :])


def check_queue_bookkeeping(h, steps, uq0):
    """uak[k + d] == uk[k] exactly, the first d applied inputs are the initial queue, and
    the queue left over holds the last d commands."""
    k_sim = h["uk"].shape[0]
    np.testing.assert_array_equal(h["uak"][steps:], h["uk"][:k_sim - steps])
    np.testing.assert_array_equal(h["uak"][:steps], uq0[:k_sim])
    if "u_queue" in h and k_sim >= steps:
        np.testing.assert_array_equal(h["u_queue"], h["uk"][k_sim - steps:])


@pytest.mark.parametrize("route", ["c", "numpy"])
@pytest.mark.parametrize("gen", [GEN, None])
def test_zero_delay_is_estimator_ref_bitwise(gen, route):
    """steps = 0, both predict values: run is estimator_ref.run bit for bit on every key it
    has, the plan state is x_hat and the applied input the command; with x_hat0 = x0 (where
    estimator_ref takes the solve's own plant step) and with x_hat0 != x0."""
    B, k_sim, cfg = 6, 4, O.Config(N=6, mode=2)
    x0 = x0_of(B)
    sy = SIGMA_Y if gen is not None else 0.0
    for xh0 in (None, xhat0_of(x0)):
        ref = E.run(x0, cfg, k_sim, gen, nominal=True, gain=GAIN, kappa=KAPPA, sigma_y=sy, xhat0=xh0, route=route)
        for predict in (True, False):
            h = D.run(x0, cfg, k_sim, 0, gen, nominal=True, gain=GAIN, kappa=KAPPA, sigma_y=sy, xhat0=xh0,
                      predict=predict, route=route)
            for key in ref:
                np.testing.assert_array_equal(h[key], ref[key], err_msg=key)
            np.testing.assert_array_equal(h["uak"], h["uk"])
            np.testing.assert_array_equal(h["xpk"], h["xhk"][:-2])


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("N", [6, 12, 20, 24, 40])
def test_exit_flags_noisy_d2_teacher_forced_inputs(N, mode):
    """ids 0..15, the common noisy inputs, d = 2 from q0, 6 steps: every QP is optimal, so
    the GPU tests compare plans, not failures."""
    cfg, x0 = O.Config(N=N, mode=mode), x0_of(16)
    q0 = q0_of(16)
    h = D.run(x0, cfg, 6, 2, GEN, xhat0=xhat0_of(x0), uq0=q0, **NOISY)
    assert (h["exitflag"] == 1).all(), np.argwhere(h["exitflag"] != 1)
    check_queue_bookkeeping(h, 2, q0)
    assert np.any(h["xpk"] != h["xhk"][:-2], axis=0).all()


@pytest.mark.parametrize("mode", [2, 3])
def test_exit_flags_noisy_d2_free_running_inputs(mode):
    """N = 20, d = 2 from q0, 12 steps."""
    cfg, x0 = O.Config(N=20, mode=mode), x0_of(16)
    q0 = q0_of(16)
    h = D.run(x0, cfg, 12, 2, GEN, xhat0=xhat0_of(x0), uq0=q0, **NOISY)
    assert (h["exitflag"] == 1).all(), np.argwhere(h["exitflag"] != 1)
    check_queue_bookkeeping(h, 2, q0)


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("N,mode", [(6, 1), (6, 2), (12, 2), (20, 2), (20, 3)])
def test_exit_flags_noisy_zero_queue(N, mode, steps):
    """The common noisy inputs from a zero queue (power off until the first command
    arrives), d in {1, 3}, 12 steps."""
    cfg, x0 = O.Config(N=N, mode=mode), x0_of(16)
    h = D.run(x0, cfg, 12, steps, GEN, xhat0=xhat0_of(x0), **NOISY)
    assert (h["exitflag"] == 1).all(), np.argwhere(h["exitflag"] != 1)
    check_queue_bookkeeping(h, steps, np.zeros((steps, 16)))


@pytest.mark.parametrize("steps", EXACT_DELAYS)
@pytest.mark.parametrize("N,mode", EXACT_CASES)
def test_plan_state_is_the_future_state_exactly(N, mode, steps):
    """No generator, no noise, x_hat0 = x0, gains and kappa 0: the model is the plant and
    the estimate is the state, so the plan state of step k is the state the plant reaches
    d steps later, xk's column k + d, bit for bit (the same O.plant_step calls on the same
    values).  Every QP is optimal.  With predict = 0 the plan state is x_hat."""
    cfg, x0 = O.Config(N=N, mode=mode), x0_of(16)
    h = D.run(x0, cfg, EXACT_STEPS, steps, None, **EXACT)
    assert (h["exitflag"] == 1).all(), np.argwhere(h["exitflag"] != 1)
    np.testing.assert_array_equal(h["xhk"], h["xk"])
    n = EXACT_STEPS - steps
    err = np.max(np.abs(h["xpk"][:2 * (n + 1)] - h["xk"][2 * steps:]))
    print(f"N={N} mode {mode} d={steps}: max |x_plan[k] - x[k+d]| = {err}")
    np.testing.assert_array_equal(h["xpk"][:2 * (n + 1)], h["xk"][2 * steps:])
    check_queue_bookkeeping(h, steps, np.zeros((steps, 16)))
    h0 = D.run(x0, cfg, EXACT_STEPS, steps, None, predict=False, **EXACT)
    np.testing.assert_array_equal(h0["xpk"], h0["xhk"][:-2])
    assert np.any(h0["uk"] != h["uk"])


def test_nan_queue_entry_makes_the_plan_state_non_finite():
    """A non-finite queue entry reaches the controller as a non-finite state (under
    predict): the reference's flag is -7 and U = 0, as for a NaN x_hat."""
    cfg, x0 = O.Config(N=6, mode=2), x0_of(2)
    q = np.zeros((3, 2))
    q[1, 1] = np.nan
    import mismatch_ref as M
    rho, Uo = M.initial_state(x0, cfg, None, True)
    r = D.step(x0, x0, rho, Uo, np.zeros((2, 2)), q, cfg, None, **EXACT)
    assert r["exitflag"][0] == 1 and r["exitflag"][1] == -7
    assert np.all(r["U"][:, 1] == 0.0) and np.all(np.isnan(r["x_plan"][:, 1]))
    assert r["u_applied"][1] == 0.0 and np.isnan(r["u_queue"][0, 1]) and r["u_queue"][2, 1] == 0.0
