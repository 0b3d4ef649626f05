"""CPU checks of tests/estimator_ref.py, the reference the GPU output-feedback tests
(tests/test_gpu_estimator.py) are held to: its degenerate case against
tests/mismatch_ref.py, its two routes against each other, the exit flags of the inputs
the GPU tests use, and the filter's noise rejection at the oracle level.
"""
import dataclasses

import numpy as np
import pytest

import estimator_ref as E
import mismatch_ref as M
from oracle import ntm_oracle as O

GEN = O.ScenarioGen(seed=20241220, first_id=0, k0=0, sigma_w=1e-3, sigma_omega=0.0, jbs_spread=0.1,
                    wdep_spread=0.1)
SIGMA_Y = (2.0 ** -10, 16.0)
KAPPA = (0.5, 0.25)
GAIN = (0.5, 0.2)
# the noise-rejection property's inputs (the issue's): a quiet plant, a slow d_hat
PROP_GEN = dataclasses.replace(GEN, sigma_w=2.0 ** -13)
PROP_GAIN = (0.1, 0.1)
PROP_STEPS, PROP_FROM, PROP_BOUND = 30, 6, 0.8


def x0_of(B, first=0):
    return np.ascontiguousarray(O.scenario_x0(np.arange(first, first + B)).T)


def xhat0_of(x0):
    s = np.arange(x0.shape[1])
    return np.ascontiguousarray(x0 + np.stack([1e-3 * np.cos(s), 10.0 * np.sin(s)]))


def rejection_ratio(h_f, h_0, k_from=PROP_FROM):
    """rms(x_hat - x) with the filter over the same without it (kappa = 0), per component,
    over every scenario and the steps from k_from on (columns k_from + 1 .. of xhk / xk)."""
    def rms(h):
        e = (h["xhk"] - h["xk"])[2 * (k_from + 1):]
        return np.array([np.sqrt(np.mean(e[i::2] ** 2)) for i in range(2)])
    return rms(h_f) / rms(h_0), rms(h_0)


@pytest.mark.parametrize("route", ["c", "numpy"])
@pytest.mark.parametrize("gen", [GEN, None])
def test_degenerate_reference_is_mismatch_ref_bitwise(gen, route):
    """sigma_y = 0, kappa = 0, equal gains, x_hat0 = x0: run is mismatch_ref.run bit for bit,
    x_hat is the state and y is x_next."""
    B, k_sim, cfg = 6, 4, O.Config(N=6, mode=2)
    x0 = x0_of(B)
    d0 = np.ascontiguousarray(np.stack([1e-5 * np.cos(np.arange(B)), 0.3 * np.sin(np.arange(B))]))
    ref = M.run(x0, cfg, k_sim, gen, nominal=True, gain=0.5, d0=d0, route=route)
    for xh0 in (None, x0):
        h = E.run(x0, cfg, k_sim, gen, nominal=True, gain=(0.5, 0.5), kappa=0.0, sigma_y=0.0, d0=d0, xhat0=xh0,
                  route=route)
        for key in ref:
            np.testing.assert_array_equal(h[key], ref[key], err_msg=key)
        np.testing.assert_array_equal(h["xhk"], h["xk"])
        np.testing.assert_array_equal(h["yk"], h["xk"][2:])


@pytest.mark.parametrize("N,mode", [(6, 1), (10, 2)])
def test_routes_agree(N, mode):
    """The NumPy route and the C route, identical inputs every step (x_hat and d_hat
    included): 1e-13 umax on U, equal flags and iteration counts (the bound
    test_mismatch_ref.test_routes_agree holds)."""
    B, cfg = 8, O.Config(N=N, mode=mode)
    x = x0_of(B)
    xh = xhat0_of(x)
    rho, Uo = M.initial_state(xh, cfg, GEN, nominal=True)
    d = np.zeros((2, B))
    worst = 0.0
    for k in range(4):
        g = dataclasses.replace(GEN, k0=k)
        a = E.step(x, xh, rho, Uo, d, cfg, g, True, GAIN, KAPPA, SIGMA_Y, route="numpy")
        b = E.step(x, xh, rho, Uo, d, cfg, g, True, GAIN, KAPPA, SIGMA_Y, route="c")
        np.testing.assert_array_equal(a["exitflag"], b["exitflag"])
        np.testing.assert_array_equal(a["inner_iters"], b["inner_iters"])
        worst = max(worst, np.max(np.abs(a["U"] - b["U"])) / cfg.umax)
        for key in ("x_next", "y", "x_hat", "d_hat"):
            np.testing.assert_allclose(a[key][0], b[key][0], rtol=0, atol=1e-13, err_msg=key)
            np.testing.assert_allclose(a[key][1], b[key][1], rtol=0, atol=1e-9, err_msg=key)
        assert np.all(a["y"] != a["x_next"]) and np.all(a["x_hat"] != a["y"])
        x, xh, rho, Uo, d = b["x_next"], b["x_hat"], b["rho"], b["U_old"], b["d_hat"]
    print(f"N={N} mode {mode}: max |U_numpy - U_c| / umax = {worst:.2e}")
    assert worst <= 1e-13, worst


@pytest.mark.parametrize("N,mode", [(6, 1), (6, 2), (12, 2), (20, 1), (20, 2), (20, 3), (24, 2)])
def test_exit_flags_of_the_gpu_tests_inputs(N, mode):
    """ids 0..15, the common inputs, 20 free-running steps: every QP is optimal, so the GPU
    tests compare plans, not failures."""
    cfg, x0 = O.Config(N=N, mode=mode), x0_of(16)
    h = E.run(x0, cfg, 20, GEN, nominal=True, gain=GAIN, kappa=KAPPA, sigma_y=SIGMA_Y, xhat0=xhat0_of(x0))
    assert (h["exitflag"] == 1).all(), np.argwhere(h["exitflag"] != 1)


def test_exit_flags_of_the_teacher_forced_long_horizon():
    """(40, 2) is used for the 6 teacher-forced steps only (one -2 in 320 scenario-steps
    over 20 free-running steps): its flags over those 6 steps."""
    cfg, x0 = O.Config(N=40, mode=2), x0_of(16)
    h = E.run(x0, cfg, 6, GEN, nominal=True, gain=GAIN, kappa=KAPPA, sigma_y=SIGMA_Y, xhat0=xhat0_of(x0))
    assert (h["exitflag"] == 1).all(), np.argwhere(h["exitflag"] != 1)


@pytest.mark.parametrize("N", [10, 20])
def test_filter_rejects_measurement_noise(N):
    """sigma_w = 2^-13, sigma_y = (2^-10, 16), gain 0.1, mode 2, 30 steps, statistics from
    step 6 on: rms(x_hat - x) at kappa = 0.5 over the same at kappa = 0 is at most 0.8 in
    both components (0.626 / 0.627 at N = 10 and 0.629 / 0.627 at N = 20 measured on this
    reference; at kappa = 0 the error is the noise itself, 1.03e-3 m and 16.5 rad/s).  The
    margin up to 0.8 covers other ids; the GPU follows the same realisations."""
    cfg, x0 = O.Config(N=N, mode=2), x0_of(16)
    kw = dict(nominal=True, gain=PROP_GAIN, sigma_y=SIGMA_Y, xhat0=xhat0_of(x0))
    h_f = E.run(x0, cfg, PROP_STEPS, PROP_GEN, kappa=(0.5, 0.5), **kw)
    h_0 = E.run(x0, cfg, PROP_STEPS, PROP_GEN, kappa=0.0, **kw)
    assert (h_f["exitflag"] == 1).all() and (h_0["exitflag"] == 1).all()
    ratio, rms0 = rejection_ratio(h_f, h_0)
    print(f"N={N}: ratio w {ratio[0]:.3f}, omega {ratio[1]:.3f}; rms at kappa = 0: {rms0[0]:.3e} m, {rms0[1]:.3e} rad/s")
    np.testing.assert_array_equal(h_0["xhk"][2:], h_0["yk"])       # kappa = 0: the estimate is the measurement
    assert np.all(ratio <= PROP_BOUND), ratio
