"""CPU checks of tests/mismatch_ref.py, the reference the GPU observer tests
(tests/test_gpu_mismatch.py) are held to: its two routes against each other and
against the C oracle, the offset-free property at the oracle level, and the exit flags
of the inputs the GPU tests use.
"""
import dataclasses

import numpy as np
import pytest

import mismatch_ref as M
from oracle import cbind
from oracle import ntm_oracle as O

GEN = O.ScenarioGen(seed=20241220, first_id=0, k0=0, sigma_w=1e-3, sigma_omega=0.0, jbs_spread=0.1,
                    wdep_spread=0.1)


def _x0(B, first=0):
    return np.ascontiguousarray(O.scenario_x0(np.arange(first, first + B)).T)


@pytest.mark.parametrize("N,mode", [(6, 1), (10, 2)])
@pytest.mark.parametrize("gen", [GEN, None])
def test_route_c_degenerate_is_the_c_oracle_bitwise(N, mode, gen):
    """d_hat = 0, nominal_model = 0, any gain-0 step: route (b) is cbind.step(..., gen=gen)."""
    B, cfg = 8, O.Config(N=N, mode=mode)
    x = _x0(B)
    rho, Uo = cbind.initial_state(x, cfg) if gen is None else cbind.initial_state_gen(x, cfg, gen)
    for k in range(4):
        g = None if gen is None else dataclasses.replace(gen, k0=k)
        ref = cbind.step(x, rho, Uo, cfg, gen=g)
        out = M.step(x, rho, Uo, np.zeros((2, B)), cfg, g, nominal=False, gain=0.0, route="c")
        for key in ("U", "x_pred", "x_next", "rho", "U_old", "exitflag", "inner_iters"):
            np.testing.assert_array_equal(out[key], ref[key], err_msg=f"{key} step {k}")
        np.testing.assert_array_equal(out["d_hat"], 0.0)
        x, rho, Uo = ref["x_next"], ref["rho"], ref["U_old"]


@pytest.mark.parametrize("N,mode", [(6, 1), (10, 2)])
def test_routes_agree(N, mode):
    """The NumPy route and the C route, identical inputs every step (d_hat included):
    1e-13 umax on U, the bound the two oracle restatements hold to each other."""
    B, cfg = 8, O.Config(N=N, mode=mode)
    x = _x0(B)
    rho, Uo = M.initial_state(x, cfg, GEN, nominal=True)
    d = np.zeros((2, B))
    worst = 0.0
    for k in range(4):
        g = dataclasses.replace(GEN, k0=k)
        a = M.step(x, rho, Uo, d, cfg, g, nominal=True, gain=0.5, route="numpy")
        b = M.step(x, rho, Uo, d, cfg, g, nominal=True, gain=0.5, route="c")
        np.testing.assert_array_equal(a["exitflag"], b["exitflag"])
        same = a["inner_iters"] == b["inner_iters"]
        assert same.all(), (k, a["inner_iters"], b["inner_iters"])
        worst = max(worst, np.max(np.abs(a["U"] - b["U"])) / cfg.umax)
        np.testing.assert_allclose(a["x_next"][0], b["x_next"][0], rtol=0, atol=1e-13)
        np.testing.assert_allclose(a["d_hat"][0], b["d_hat"][0], rtol=0, atol=1e-13)
        np.testing.assert_allclose(a["d_hat"][1], b["d_hat"][1], rtol=0, atol=1e-9)
        if k:
            assert np.all(d[0] != 0.0)                       # the estimate did enter the solve
        x, rho, Uo, d = b["x_next"], b["rho"], b["U_old"], b["d_hat"]
    print(f"N={N} mode {mode}: max |U_numpy - U_c| / umax = {worst:.2e}")
    assert worst <= 1e-13, worst


def test_offset_free_at_the_oracle_level():
    """A wrong j_BS is an error in C1 alone: at gain 1 the estimate is that error after
    one step and stays it.  N = 10, 8 scenarios, 40 steps, no noise, nominal model."""
    B, k_sim, cfg = 8, 40, O.Config(N=10, mode=2)
    gen = O.ScenarioGen(jbs_spread=0.1)
    x0 = _x0(B)
    h = M.run(x0, cfg, k_sim, gen, nominal=True, gain=1.0)
    assert (h["exitflag"] == 1).all()
    dC1 = np.array([O.C_vec(O.scenario_physics(O.Physics(), gen, s), cfg.Ts)[0] - O.C_vec(O.Physics(), cfg.Ts)[0]
                    for s in range(B)])
    assert np.max(np.abs(dC1)) > 1e-5                        # there is a mismatch to find
    err = np.max(np.abs(h["dk"][-2] - dC1))
    print(f"max |d_hat[0] - dC1| after {k_sim} steps = {err:.2e}, dC1 in [{dC1.min():.2e}, {dC1.max():.2e}]")
    assert err <= 1e-15, err
    assert np.all(h["dk"][1::2] == 0.0)
    # gain 0 leaves the estimate at its input
    h0 = M.run(x0, cfg, 3, gen, nominal=True, gain=0.0)
    assert np.all(h0["dk"] == 0.0)


@pytest.mark.parametrize("N", [6, 10, 20])
@pytest.mark.parametrize("mode", [1, 2])
def test_exit_flags_of_the_gpu_tests_inputs(N, mode):
    """ids 0..15, spreads 0.1 / 0.1, sigma_w in {0, 1e-3}, gains 0, 0.5, 1, 12 steps,
    nominal model: every QP is optimal, so the GPU tests compare plans, not failures."""
    cfg, x0 = O.Config(N=N, mode=mode), _x0(16)
    for sw in (0.0, 1e-3):
        gen = dataclasses.replace(GEN, sigma_w=sw)
        for gain in (0.0, 0.5, 1.0):
            h = M.run(x0, cfg, 12, gen, nominal=True, gain=gain)
            assert (h["exitflag"] == 1).all(), (sw, gain)
