"""The MEX gateway's 'step' with the multipliers: outputs 9 and 10 (lambda, rho_qp)
come from ntm_mpc_step_dual and are bitwise what the ctypes host path
(NtmMpc.step_dual_host) returns; asked for eight outputs or fewer, 'step' is what it
was (ntm_mpc_step_ws), bit for bit.  The outputs follow the existing eight (rho, Uold
and ws are outputs 6-8 already), so no caller's output list changes meaning.
"""
import numpy as np
import pytest

from test_mex_gateway import Mex, _skip_if_variant, mex  # noqa: F401  (mex: the module's shim fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,mode", [(20, 2), (6, 3)])
def test_mex_step_with_multipliers(mex, ctl, N, mode):          # noqa: F811
    import torch
    from ntm_mpc import Config, scenarios_x0
    _skip_if_variant()
    B = 7
    mcfg = {"N": float(N), "mode": float(mode)}
    cfg = Config(N=N, mode=mode)
    x = np.ascontiguousarray(scenarios_x0(0, B))
    rho0, uo0 = ctl.initial_state_host(x, cfg)
    ws0 = -np.ones((2 * (N + 1), B), np.int32)
    # ten outputs: the dual step
    outs = mex("step", x, rho0.copy(order="K"), uo0.copy(order="K"), mcfg, ws0.copy(), nout=10)
    rho_h, uo_h, ws_h = rho0.copy(order="K"), uo0.copy(order="K"), ws0.copy()
    h = ctl.step_dual_host(x, rho_h, uo_h, cfg, active_ws=ws_h)
    U, xp, xn, fl, it, rho_m, uo_m, ws_m, lam, rq = outs
    assert lam.shape == (cfg.m, B) and rq.shape == (3 * N, B)
    for a, b in ((U, h["U"]), (xp, h["x_pred"]), (xn, h["x_next"]), (rho_m, rho_h), (uo_m, uo_h), (ws_m, ws_h),
                 (lam, h["lambda"]), (rq, h["rho_qp"])):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(fl[0], h["exitflag"])
    np.testing.assert_array_equal(it[0], h["inner_iters"])
    assert np.any(lam > 0.0)
    # five and eight outputs: the step as it was
    for nout in (5, 8):
        outs = mex("step", x, rho0.copy(order="K"), uo0.copy(order="K"), mcfg, ws0.copy(), nout=nout)
        rho_h, uo_h, ws_h = rho0.copy(order="K"), uo0.copy(order="K"), ws0.copy()
        h = ctl.step_host(x, rho_h, uo_h, cfg, active_ws=ws_h)
        for a, k in zip(outs[:3], ("U", "x_pred", "x_next")):
            np.testing.assert_array_equal(a, h[k], err_msg=k)
        np.testing.assert_array_equal(outs[3][0], h["exitflag"])
        np.testing.assert_array_equal(outs[4][0], h["inner_iters"])
        if nout == 8:
            for a, b in zip(outs[5:], (rho_h, uo_h, ws_h)):
                np.testing.assert_array_equal(a, b)
    mex("close", nout=0)
    torch.cuda.synchronize()
