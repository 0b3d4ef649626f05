"""The MEX gateway's 'step_obs' and 'run_obs' (plant-model mismatch and the disturbance
estimate, ntm_mpc_step_obs / ntm_mpc_run_obs): every output is bitwise what the ctypes
host path (NtmMpc.step_obs_host / run_obs_host) returns; the observer goes in as a
struct, d_hat and dk are the extra outputs.  The argument errors need no GPU.
"""
import numpy as np
import pytest

from test_mex_gateway import Mex, MexError, _skip_if_variant, mex  # noqa: F401  (mex: the module's shim fixture)

GEN = {"seed": 20241220.0, "first_id": 3.0, "k0": 2.0, "sigma_w": 1e-3, "jbs_spread": 0.1, "wdep_spread": 0.1}


def test_mex_obs_rejects_bad_arguments(mex):                     # noqa: F811
    B, N = 3, 4
    x, rho, uo, d = np.ones((2, B)), np.ones((3 * N, B)), np.ones((N, B)), np.zeros((2, B))
    cfg, obs = {"N": 4.0}, {"nominal_model": 1.0, "gain": 0.5}
    for args in (("step_obs", x, rho, uo, d), ("step_obs", x, rho, uo, d, 3.0, cfg),
                 ("step_obs", x, rho, uo, np.zeros((3, B)), obs, cfg), ("run_obs", x, 5.0),
                 ("run_obs", x, 5.0, 1.0, cfg), ("run_obs", x, 0.0, obs, cfg),
                 ("run_obs", x, 5.0, obs, cfg, np.zeros((2, B + 1)))):
        with pytest.raises(MexError) as e:
            mex(*args)
        assert e.value.ident == "ntm:arg", args[0]


@pytest.mark.gpu
@pytest.mark.parametrize("N,mode", [(20, 2), (6, 1)])
def test_mex_obs_commands_match_ctypes(mex, ctl, N, mode):      # noqa: F811
    import torch
    from ntm_mpc import Config, Observer, ScenarioGen, scenarios_x0
    _skip_if_variant()
    B, k_sim = 7, 3
    mcfg, cfg = {"N": float(N), "mode": float(mode)}, Config(N=N, mode=mode)
    mobs, obs = {"nominal_model": 1.0, "gain": 0.5}, Observer(nominal_model=True, gain=0.5)
    x = np.ascontiguousarray(scenarios_x0(0, B))
    d0 = np.ascontiguousarray(np.stack([1e-5 * np.cos(np.arange(B)), 0.3 * np.sin(np.arange(B))]))
    ws0 = -np.ones((2 * (N + 1), B), np.int32)
    rho0, uo0 = ctl.initial_state_host(x, cfg)                   # nominal model: before the generator
    rho_m, uo_m = mex("init", x, mcfg, nout=2)
    np.testing.assert_array_equal(rho_m, rho0)
    gen = ScenarioGen(seed=20241220, first_id=3, k0=2, sigma_w=1e-3, jbs_spread=0.1, wdep_spread=0.1)
    mex("scenarios", GEN, nout=0)
    ctl.set_scenarios(gen)
    try:
        outs = mex("step_obs", x, rho_m, uo_m, d0, mobs, mcfg, ws0.copy(), nout=9)
        rh, uh, dh, wh = rho0.copy(order="K"), uo0.copy(order="K"), d0.copy(order="K"), ws0.copy()
        h = ctl.step_obs_host(x, rh, uh, dh, obs, cfg, active_ws=wh)
        U, xp, xn, fl, it, rho_o, uo_o, ws_o, d_o = outs
        for a, b in ((U, h["U"]), (xp, h["x_pred"]), (xn, h["x_next"]), (rho_o, rh), (uo_o, uh), (ws_o, wh),
                     (d_o, dh)):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(fl[0], h["exitflag"])
        np.testing.assert_array_equal(it[0], h["inner_iters"])
        assert np.any(d_o != d0)
        # without ws and with fewer outputs: the same step from an empty workspace
        U5 = mex("step_obs", x, rho_m, uo_m, d0, mobs, mcfg, nout=5)
        np.testing.assert_array_equal(U5[0], U)
        for d_init in (d0, None):
            extra = () if d_init is None else (d_init,)
            ro = mex("run_obs", x, float(k_sim), mobs, mcfg, *extra, nout=7)
            hr = ctl.run_obs_host(x, obs, k_sim, cfg, d0=d_init)
            for a, k in zip(ro, ("xk", "uk", "Uk", "wpred", "exitflag", "inner_iters", "dk")):
                np.testing.assert_array_equal(a, hr[k], err_msg=k)
            assert np.any(ro[6][2:] != 0.0)
    finally:
        ctl.set_scenarios(None)
        mex("scenarios", np.zeros((0, 0)), nout=0)
    mex("close", nout=0)
    torch.cuda.synchronize()
