"""The MEX gateway's 'step_dly', 'run_dly' and 'run_dly_from' (actuator dead time,
ntm_mpc_step_dly / ntm_mpc_run_dly / ntm_mpc_run_dly_from): every output is bitwise what
the ctypes host path (NtmMpc.step_dly_host / run_dly_host / run_dly_from_host) returns; the
delay goes in as a struct after the estimator, the queue after x_hat.  The argument errors
need no GPU.
"""
import numpy as np
import pytest

from test_mex_est import GEN, MEST
from test_mex_gateway import Mex, MexError, _skip_if_variant, mex  # noqa: F401  (mex: the module's shim fixture)

MDLY = {"steps": 3.0, "predict": 1.0}


def test_mex_dly_rejects_bad_arguments(mex):                     # noqa: F811
    B, N = 3, 4
    x, rho, uo, d = np.ones((2, B)), np.ones((3 * N, B)), np.ones((N, B)), np.zeros((2, B))
    q, ws = np.zeros((3, B)), -np.ones((2 * (N + 1), B), np.int32)
    cfg = {"N": 4.0}
    for args in (("step_dly", x, rho, uo, d, x, q, MEST), ("step_dly", x, rho, uo, d, x, q, MEST, 3.0, cfg),
                 ("step_dly", x, rho, uo, d, x, q, 3.0, MDLY, cfg),
                 ("step_dly", x, rho, uo, d, x, np.zeros((2, B)), MEST, MDLY, cfg),
                 ("step_dly", x, rho, uo, d, x, np.zeros((3, B + 1)), MEST, MDLY, cfg),
                 ("step_dly", x, rho, uo, d, x, np.zeros((0, 0)), MEST, MDLY, cfg),
                 ("step_dly", x, rho, uo, d, x, q, MEST, {"steps": 9.0}, cfg),
                 ("step_dly", x, rho, uo, d, x, q, MEST, {"steps": -1.0}, cfg),
                 ("step_dly", x, rho, uo, d, x, q, MEST, MDLY, cfg, np.ones((2 * (N + 1), B))),
                 ("run_dly", x, 5.0, MEST), ("run_dly", x, 5.0, MEST, 1.0, cfg), ("run_dly", x, 0.0, MEST, MDLY, cfg),
                 ("run_dly", x, 5.0, MEST, MDLY, cfg, d, x, np.zeros((2, B))),
                 ("run_dly", x, 5.0, MEST, {"steps": 9.0}, cfg),
                 ("run_dly_from", x, rho, uo, ws, d, x, q, 2.0, MEST),
                 ("run_dly_from", x, rho, uo, ws, d, x, np.zeros((4, B)), 2.0, MEST, MDLY, cfg),
                 ("run_dly_from", x, rho, uo, ws, d, x, q, -1.0, MEST, MDLY, cfg),
                 ("run_dly_from", x, rho, uo, ws.astype(np.float64), d, x, q, 2.0, MEST, MDLY, cfg)):
        with pytest.raises(MexError) as e:
            mex(*args)
        assert e.value.ident == "ntm:arg", args[0]


@pytest.mark.gpu
@pytest.mark.parametrize("N,mode", [(20, 2), (6, 1)])
def test_mex_dly_commands_match_ctypes(mex, ctl, N, mode):      # noqa: F811
    import torch
    from ntm_mpc import Config, Delay, Estimator, ScenarioGen, scenarios_x0
    _skip_if_variant()
    B, k_sim, steps = 7, 4, 3
    mcfg, cfg = {"N": float(N), "mode": float(mode)}, Config(N=N, mode=mode)
    est = Estimator(nominal_model=True, gain=(0.5, 0.2), kappa=(0.5, 0.25), sigma_y=(2.0 ** -10, 16.0))
    dly = Delay(steps=steps)
    x = np.ascontiguousarray(scenarios_x0(0, B))
    s = np.arange(B)
    xh0 = np.ascontiguousarray(x + np.stack([1e-3 * np.cos(s), 10.0 * np.sin(s)]))
    d0 = np.ascontiguousarray(np.stack([1e-5 * np.cos(s), 0.3 * np.sin(s)]))
    q0 = np.ascontiguousarray(2e5 + 1.1e5 * np.arange(steps)[:, None] + 7e3 * s[None, :])
    ws0 = -np.ones((2 * (N + 1), B), np.int32)
    cp = lambda a: a.copy(order="K")                             # noqa: E731
    rho0, uo0 = ctl.initial_state_host(xh0, cfg)                 # nominal model: before the generator
    rho_m, uo_m = mex("init", xh0, mcfg, nout=2)
    np.testing.assert_array_equal(rho_m, rho0)
    gen = ScenarioGen(seed=20241220, first_id=3, k0=2, sigma_w=1e-3, jbs_spread=0.1, wdep_spread=0.1)
    mex("scenarios", GEN, nout=0)
    ctl.set_scenarios(gen)
    try:
        outs = mex("step_dly", x, rho_m, uo_m, d0, xh0, q0, MEST, MDLY, mcfg, ws0.copy(), nout=14)
        rh, uh, dh, hh, qh, wh = cp(rho0), cp(uo0), cp(d0), cp(xh0), cp(q0), ws0.copy()
        h = ctl.step_dly_host(x, rh, uh, dh, hh, qh, est, dly, cfg, active_ws=wh)
        U, xp, xn, fl, it, rho_o, uo_o, ws_o, d_o, h_o, y_o, q_o, z_o, ua_o = outs
        for a, b in ((U, h["U"]), (xp, h["x_pred"]), (xn, h["x_next"]), (rho_o, rh), (uo_o, uh), (ws_o, wh),
                     (d_o, dh), (h_o, hh), (y_o, h["y"]), (q_o, qh), (z_o, h["x_plan"])):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(fl[0], h["exitflag"])
        np.testing.assert_array_equal(it[0], h["inner_iters"])
        np.testing.assert_array_equal(ua_o[0], h["u_applied"])
        np.testing.assert_array_equal(ua_o[0], q0[0])
        np.testing.assert_array_equal(q_o[:-1], q0[1:])
        np.testing.assert_array_equal(q_o[-1], U[0])
        assert np.any(z_o != xh0, axis=0).all()
        # without ws and with fewer outputs: the same step from an empty workspace
        U5 = mex("step_dly", x, rho_m, uo_m, d0, xh0, q0, MEST, MDLY, mcfg, nout=5)
        np.testing.assert_array_equal(U5[0], U)
        # steps = 0 with [] for the queue is 'step_est'; a missing predict is 1
        e11 = mex("step_est", x, rho_m, uo_m, d0, xh0, MEST, mcfg, nout=11)
        z14 = mex("step_dly", x, rho_m, uo_m, d0, xh0, np.zeros((0, 0)), MEST, {"steps": 0.0}, mcfg, nout=14)
        for a, b in zip(e11, z14[:11]):
            np.testing.assert_array_equal(a, b)
        assert z14[11].shape == (0, B)
        np.testing.assert_array_equal(z14[12], xh0)
        p14 = mex("step_dly", x, rho_m, uo_m, d0, xh0, q0, MEST, {"steps": float(steps)}, mcfg, nout=14)
        np.testing.assert_array_equal(p14[12], z_o)
        n14 = mex("step_dly", x, rho_m, uo_m, d0, xh0, q0, MEST, {"steps": float(steps), "predict": 0.0}, mcfg, nout=14)
        np.testing.assert_array_equal(n14[12], xh0)
        empty = np.zeros((0, 0))
        names = ("xk", "uk", "Uk", "wpred", "exitflag", "inner_iters", "dk", "xhk", "yk", "uak", "xpk")
        for extra, d_init, h_init, q_init in (((d0, xh0, q0), d0, xh0, q0), ((), None, None, None),
                                              ((empty, xh0, empty), None, xh0, None)):
            ro = mex("run_dly", x, float(k_sim), MEST, MDLY, mcfg, *extra, nout=11)
            hr = ctl.run_dly_host(x, est, dly, k_sim, cfg, d0=d_init, xhat0=h_init, uq0=q_init)
            for a, k in zip(ro, names):
                np.testing.assert_array_equal(a, hr[k], err_msg=k)
            np.testing.assert_array_equal(ro[9][steps:], ro[1][:-steps])
            np.testing.assert_array_equal(ro[9][:steps], np.zeros((steps, B)) if q_init is None else q_init)
        fo = mex("run_dly_from", x, rho_m, uo_m, ws0.copy(), d0, xh0, q0, float(k_sim), MEST, MDLY, mcfg, nout=18)
        sh = [cp(x), cp(rho0), cp(uo0), ws0.copy(), cp(d0), cp(xh0), cp(q0)]
        hf = ctl.run_dly_from_host(*sh, est, dly, k_sim, cfg)
        for a, k in zip(fo[:11], names):
            np.testing.assert_array_equal(a, hf[k], err_msg=k)
        for a, b in zip(fo[11:], sh):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(fo[17], fo[1][-steps:])
        z0 = mex("run_dly_from", x, rho_m, uo_m, ws0.copy(), d0, xh0, q0, 0.0, MEST, MDLY, mcfg, nout=18)
        for a, b in zip(z0[11:], (x, rho0, uo0, ws0, d0, xh0, q0)):
            np.testing.assert_array_equal(a, b)
    finally:
        ctl.set_scenarios(None)
        mex("scenarios", np.zeros((0, 0)), nout=0)
    mex("close", nout=0)
    torch.cuda.synchronize()
