"""The MEX gateway's 'run_from' and 'run_est_from' (the resumable closed loops,
ntm_mpc_run_from / ntm_mpc_run_est_from): every output is bitwise what the ctypes host
path (NtmMpc.run_from_host / run_est_from_host) returns; the state arrays go in and come
back as the extra outputs, chunk after chunk.  The argument errors need no GPU.
"""
import numpy as np
import pytest

from test_mex_gateway import Mex, MexError, _skip_if_variant, mex  # noqa: F401  (mex: the module's shim fixture)

GEN = {"seed": 20241220.0, "first_id": 3.0, "k0": 2.0, "sigma_w": 1e-3, "jbs_spread": 0.1, "wdep_spread": 0.1}
MEST = {"nominal_model": 1.0, "gain": np.array([0.5, 0.2]), "kappa": np.array([0.5, 0.25]),
        "sigma_y": np.array([2.0 ** -10, 16.0])}
HIST = ("xk", "uk", "Uk", "wpred", "exitflag", "inner_iters")


def test_mex_run_from_rejects_bad_arguments(mex):                # noqa: F811
    B, N = 3, 4
    x, rho, uo, d = np.ones((2, B)), np.ones((3 * N, B)), np.ones((N, B)), np.zeros((2, B))
    ws = -np.ones((2 * (N + 1), B), np.int32)
    cfg = {"N": 4.0}
    for args in (("run_from", x, rho, uo, ws), ("run_from", x, rho, uo, ws.astype(np.float64), 2.0, cfg),
                 ("run_from", x, rho, uo, ws[:-1], 2.0, cfg), ("run_from", x, rho, uo, ws, -1.0, cfg),
                 ("run_from", x, rho, uo, ws, cfg, cfg), ("run_from", np.ones((3, B)), rho, uo, ws, 2.0, cfg),
                 ("run_from", x, rho[:-1], uo, ws, 2.0, cfg), ("run_from", x, rho, np.ones((N, B + 1)), ws, 2.0, cfg),
                 ("run_est_from", x, rho, uo, ws, d, x, 2.0), ("run_est_from", x, rho, uo, ws, d, x, 2.0, 1.0, cfg),
                 ("run_est_from", x, rho, uo, ws, d, x, -2.0, MEST, cfg),
                 ("run_est_from", x, rho, uo, ws, np.zeros((3, B)), x, 2.0, MEST, cfg),
                 ("run_est_from", x, rho, uo, ws, d, np.zeros((2, B + 1)), 2.0, MEST, cfg),
                 ("run_est_from", x, rho, uo, ws.astype(np.float64), d, x, 2.0, MEST, cfg),
                 ("run_est_from", x, rho, uo, ws, d, x, 2.0, {"kappa": np.ones(3)}, cfg)):
        with pytest.raises(MexError) as e:
            mex(*args)
        assert e.value.ident == "ntm:arg", args


@pytest.mark.gpu
@pytest.mark.parametrize("N,mode", [(20, 2), (6, 1)])
def test_mex_run_from_commands_match_ctypes(mex, ctl, N, mode):  # noqa: F811
    import torch
    from ntm_mpc import Config, Estimator, ScenarioGen, scenarios_x0
    _skip_if_variant()
    B = 7
    mcfg, cfg = {"N": float(N), "mode": float(mode)}, Config(N=N, mode=mode)
    est = Estimator(nominal_model=True, gain=(0.5, 0.2), kappa=(0.5, 0.25), sigma_y=(2.0 ** -10, 16.0))
    x0 = np.ascontiguousarray(scenarios_x0(0, B))
    s = np.arange(B)
    xh0 = np.ascontiguousarray(x0 + np.stack([1e-3 * np.cos(s), 10.0 * np.sin(s)]))
    ws0 = -np.ones((2 * (N + 1), B), np.int32)
    gen = ScenarioGen(seed=20241220, first_id=3, k0=2, sigma_w=1e-3, jbs_spread=0.1, wdep_spread=0.1)
    try:
        # run_from: the scenarios' own plasma, so init runs with the generator attached
        mex("scenarios", GEN, nout=0)
        ctl.set_scenarios(gen)
        rho_m, uo_m = mex("init", x0, mcfg, nout=2)
        rho_h, uo_h = ctl.initial_state_host(x0, cfg)
        np.testing.assert_array_equal(rho_m, rho_h)
        sm = [x0, rho_m, uo_m, ws0.copy()]
        sh = [np.asfortranarray(a.copy()) for a in (x0, rho_h, uo_h, ws0)]
        for n, k0 in ((2, 2), (1, 4)):
            mex("scenarios", dict(GEN, k0=float(k0)), nout=0)
            ctl.set_scenarios(ScenarioGen(**{**gen.__dict__, "k0": k0}))
            outs = mex("run_from", *sm, float(n), mcfg, nout=10)
            h = ctl.run_from_host(*sh, n, cfg)
            for a, k in zip(outs[:6], HIST):
                np.testing.assert_array_equal(a, h[k], err_msg=k)
            sm = outs[6:]
            for a, b in zip(sm, sh):
                np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(sm[0], outs[0][-2:])
            assert sm[3].dtype == np.int32 and np.any(sm[3] >= 0)
        assert np.array_equal(mex("run_from", *sm, 1.0, mcfg, nout=1)[0][:2], sm[0])     # fewer outputs
        # run_est_from: the nominal model, so init runs before the generator is attached
        mex("scenarios", np.zeros((0, 0)), nout=0)
        ctl.set_scenarios(None)
        rho_m, uo_m = mex("init", xh0, mcfg, nout=2)
        rho_h, uo_h = ctl.initial_state_host(xh0, cfg)
        d0 = np.zeros((2, B))
        sm = [x0, rho_m, uo_m, ws0.copy(), d0, xh0]
        sh = [np.asfortranarray(a.copy()) for a in (x0, rho_h, uo_h, ws0, d0, xh0)]
        for n, k0 in ((2, 2), (1, 4)):
            mex("scenarios", dict(GEN, k0=float(k0)), nout=0)
            ctl.set_scenarios(ScenarioGen(**{**gen.__dict__, "k0": k0}))
            outs = mex("run_est_from", *sm, float(n), MEST, mcfg, nout=15)
            h = ctl.run_est_from_host(*sh, est, n, cfg)
            for a, k in zip(outs[:9], HIST + ("dk", "xhk", "yk")):
                np.testing.assert_array_equal(a, h[k], err_msg=k)
            sm = outs[9:]
            for a, b in zip(sm, sh):
                np.testing.assert_array_equal(a, b)
            assert np.all(sm[5] != sm[0]) and np.any(sm[4] != 0.0)
    finally:
        ctl.set_scenarios(None)
        mex("scenarios", np.zeros((0, 0)), nout=0)
    mex("close", nout=0)
    torch.cuda.synchronize()
