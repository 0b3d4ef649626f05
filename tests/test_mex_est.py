"""The MEX gateway's 'step_est' and 'run_est' (measurement noise and the filtered state
estimate, ntm_mpc_step_est / ntm_mpc_run_est): every output is bitwise what the ctypes
host path (NtmMpc.step_est_host / run_est_host) returns; the estimator goes in as a
struct, d_hat, x_hat and y (dk, xhk and yk) are the extra outputs.  The argument errors
need no GPU.
"""
import numpy as np
import pytest

from test_mex_gateway import Mex, MexError, _skip_if_variant, mex  # noqa: F401  (mex: the module's shim fixture)

GEN = {"seed": 20241220.0, "first_id": 3.0, "k0": 2.0, "sigma_w": 1e-3, "jbs_spread": 0.1, "wdep_spread": 0.1}
MEST = {"nominal_model": 1.0, "gain": np.array([0.5, 0.2]), "kappa": np.array([0.5, 0.25]),
        "sigma_y": np.array([2.0 ** -10, 16.0])}


def test_mex_est_rejects_bad_arguments(mex):                     # noqa: F811
    B, N = 3, 4
    x, rho, uo, d = np.ones((2, B)), np.ones((3 * N, B)), np.ones((N, B)), np.zeros((2, B))
    cfg = {"N": 4.0}
    for args in (("step_est", x, rho, uo, d, x), ("step_est", x, rho, uo, d, x, 3.0, cfg),
                 ("step_est", x, rho, uo, d, np.zeros((3, B)), MEST, cfg),
                 ("step_est", x, rho, uo, np.zeros((2, B + 1)), x, MEST, cfg),
                 ("step_est", x, rho, uo, d, x, {"gain": np.ones(3)}, cfg), ("run_est", x, 5.0),
                 ("run_est", x, 5.0, 1.0, cfg), ("run_est", x, 0.0, MEST, cfg),
                 ("run_est", x, 5.0, {"sigma_y": np.ones(3)}, cfg),
                 ("run_est", x, 5.0, MEST, cfg, np.zeros((2, B + 1))),
                 ("run_est", x, 5.0, MEST, cfg, d, np.zeros((3, B)))):
        with pytest.raises(MexError) as e:
            mex(*args)
        assert e.value.ident == "ntm:arg", args[0]


@pytest.mark.gpu
@pytest.mark.parametrize("N,mode", [(20, 2), (6, 1)])
def test_mex_est_commands_match_ctypes(mex, ctl, N, mode):      # noqa: F811
    import torch
    from ntm_mpc import Config, Estimator, ScenarioGen, scenarios_x0
    _skip_if_variant()
    B, k_sim = 7, 3
    mcfg, cfg = {"N": float(N), "mode": float(mode)}, Config(N=N, mode=mode)
    est = Estimator(nominal_model=True, gain=(0.5, 0.2), kappa=(0.5, 0.25), sigma_y=(2.0 ** -10, 16.0))
    x = np.ascontiguousarray(scenarios_x0(0, B))
    s = np.arange(B)
    xh0 = np.ascontiguousarray(x + np.stack([1e-3 * np.cos(s), 10.0 * np.sin(s)]))
    d0 = np.ascontiguousarray(np.stack([1e-5 * np.cos(s), 0.3 * np.sin(s)]))
    ws0 = -np.ones((2 * (N + 1), B), np.int32)
    rho0, uo0 = ctl.initial_state_host(xh0, cfg)                 # nominal model: before the generator
    rho_m, uo_m = mex("init", xh0, mcfg, nout=2)
    np.testing.assert_array_equal(rho_m, rho0)
    gen = ScenarioGen(seed=20241220, first_id=3, k0=2, sigma_w=1e-3, jbs_spread=0.1, wdep_spread=0.1)
    mex("scenarios", GEN, nout=0)
    ctl.set_scenarios(gen)
    try:
        outs = mex("step_est", x, rho_m, uo_m, d0, xh0, MEST, mcfg, ws0.copy(), nout=11)
        rh, uh, dh, hh, wh = (rho0.copy(order="K"), uo0.copy(order="K"), d0.copy(order="K"), xh0.copy(order="K"),
                              ws0.copy())
        h = ctl.step_est_host(x, rh, uh, dh, hh, est, cfg, active_ws=wh)
        U, xp, xn, fl, it, rho_o, uo_o, ws_o, d_o, h_o, y_o = outs
        for a, b in ((U, h["U"]), (xp, h["x_pred"]), (xn, h["x_next"]), (rho_o, rh), (uo_o, uh), (ws_o, wh),
                     (d_o, dh), (h_o, hh), (y_o, h["y"])):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(fl[0], h["exitflag"])
        np.testing.assert_array_equal(it[0], h["inner_iters"])
        assert np.any(d_o != d0) and np.all(h_o != xh0) and np.all(y_o != xn)
        # without ws and with fewer outputs: the same step from an empty workspace
        U5 = mex("step_est", x, rho_m, uo_m, d0, xh0, MEST, mcfg, nout=5)
        np.testing.assert_array_equal(U5[0], U)
        # a scalar field sets both components, a missing one is 0
        y1 = mex("step_est", x, rho_m, uo_m, d0, xh0, {"nominal_model": 1.0, "gain": 0.5}, mcfg, nout=11)
        h1 = ctl.step_est_host(x, rho0.copy(order="K"), uo0.copy(order="K"), d0.copy(order="K"), xh0.copy(order="K"),
                               Estimator(nominal_model=True, gain=0.5), cfg)
        for i, k in ((0, "U"), (8, "d_hat"), (9, "x_hat"), (10, "y")):
            np.testing.assert_array_equal(y1[i], h1[k], err_msg=k)
        np.testing.assert_array_equal(y1[10], y1[2])             # sigma_y = 0: y is x_next
        empty = np.zeros((0, 0))
        for extra, d_init, h_init in (((d0, xh0), d0, xh0), ((), None, None), ((empty, xh0), None, xh0)):
            ro = mex("run_est", x, float(k_sim), MEST, mcfg, *extra, nout=9)
            hr = ctl.run_est_host(x, est, k_sim, cfg, d0=d_init, xhat0=h_init)
            for a, k in zip(ro, ("xk", "uk", "Uk", "wpred", "exitflag", "inner_iters", "dk", "xhk", "yk")):
                np.testing.assert_array_equal(a, hr[k], err_msg=k)
            assert np.all(ro[7][2:] != ro[0][2:]) and np.all(ro[8] != ro[0][2:])
    finally:
        ctl.set_scenarios(None)
        mex("scenarios", np.zeros((0, 0)), nout=0)
    mex("close", nout=0)
    torch.cuda.synchronize()
