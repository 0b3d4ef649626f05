"""The argument errors of the MEX gateway's twelve commands, text for text: too few arguments
give the command's usage line, a first array of the wrong shape the shape message, a
workspace that is not int32 the ws message.  The strings are those the gateway gave before
its commands shared their helpers; MATLAB scripts match on them.  No GPU: every error here is
raised before the library is called.
"""
import numpy as np
import pytest

from test_mex_est import MEST
from test_mex_gateway import MexError, mex  # noqa: F401  (mex: the module's shim fixture)

B, N = 3, 4
X, RHO, UO, D2, Q = np.ones((2, B)), np.ones((3 * N, B)), np.ones((N, B)), np.zeros((2, B)), np.zeros((3, B))
WS = -np.ones((2 * (N + 1), B), np.int32)
CFG, OBS, MDLY = {"N": float(N)}, {"nominal_model": 1.0, "gain": 0.5}, {"steps": 3.0, "predict": 1.0}
X3, WSBAD = np.ones((3, B)), np.ones((2 * (N + 1), B))            # a wrong first array; a double workspace
WS_TEXT = "ws must be an int32 10-by-3 array"

# command: (usage, too few arguments, the first array's name, full arguments, index of ws or None)
COMMANDS = {
    "step": ("usage: ntm_mpc_mex('step', x_k, rho, Uold[, cfg[, ws]])", (X, RHO), "x_k", (X, RHO, UO, CFG, WS), 4),
    "init": ("usage: ntm_mpc_mex('init', x0[, cfg])", (), "x0", (X, CFG), None),
    "run": ("usage: ntm_mpc_mex('run', x0, k_sim[, cfg])", (X,), "x0", (X, 5.0, CFG), None),
    "step_obs": ("usage: ntm_mpc_mex('step_obs', x_k, rho, Uold, d_hat, obs[, cfg[, ws]])", (X, RHO, UO, D2), "x_k",
                 (X, RHO, UO, D2, OBS, CFG, WS), 6),
    "run_obs": ("usage: ntm_mpc_mex('run_obs', x0, k_sim, obs[, cfg[, d0]])", (X, 5.0), "x0", (X, 5.0, OBS, CFG), None),
    "step_est": ("usage: ntm_mpc_mex('step_est', x_k, rho, Uold, d_hat, x_hat, est[, cfg[, ws]])", (X, RHO, UO, D2, X),
                 "x_k", (X, RHO, UO, D2, X, MEST, CFG, WS), 7),
    "run_est": ("usage: ntm_mpc_mex('run_est', x0, k_sim, est[, cfg[, d0[, xhat0]]])", (X, 5.0), "x0",
                (X, 5.0, MEST, CFG), None),
    "run_from": ("usage: ntm_mpc_mex('run_from', x, rho, Uold, ws, k_sim[, cfg])", (X, RHO, UO, WS), "x",
                 (X, RHO, UO, WS, 2.0, CFG), 3),
    "run_est_from": ("usage: ntm_mpc_mex('run_est_from', x, rho, Uold, ws, d_hat, x_hat, k_sim, est[, cfg])",
                     (X, RHO, UO, WS, D2, X, 2.0), "x", (X, RHO, UO, WS, D2, X, 2.0, MEST, CFG), 3),
    "step_dly": ("usage: ntm_mpc_mex('step_dly', x_k, rho, Uold, d_hat, x_hat, u_queue, est, dly[, cfg[, ws]])",
                 (X, RHO, UO, D2, X, Q, MEST), "x_k", (X, RHO, UO, D2, X, Q, MEST, MDLY, CFG, WS), 9),
    "run_dly": ("usage: ntm_mpc_mex('run_dly', x0, k_sim, est, dly[, cfg[, d0[, xhat0[, uq0]]]])", (X, 5.0, MEST), "x0",
                (X, 5.0, MEST, MDLY, CFG), None),
    "run_dly_from": ("usage: ntm_mpc_mex('run_dly_from', x, rho, Uold, ws, d_hat, x_hat, u_queue, k_sim, est, dly[, cfg])",
                     (X, RHO, UO, WS, D2, X, Q, 2.0, MEST), "x", (X, RHO, UO, WS, D2, X, Q, 2.0, MEST, MDLY, CFG), 3),
}


def raised(mex, *args):                                           # noqa: F811
    with pytest.raises(MexError) as e:
        mex(*args)
    return str(e.value)


@pytest.mark.parametrize("cmd", list(COMMANDS))
def test_mex_command_argument_errors(mex, cmd):                   # noqa: F811
    usage, few, first, full, ws_at = COMMANDS[cmd]
    assert raised(mex, cmd, *few) == "ntm:arg: " + usage
    assert raised(mex, cmd, X3, *full[1:]) == f"ntm:arg: {first} must be a real 2-by-{B} double array"
    if ws_at is not None:
        bad = list(full)
        bad[ws_at] = WSBAD
        assert raised(mex, cmd, *bad) == "ntm:arg: " + WS_TEXT
        bad[ws_at] = WS[:-1]                                      # int32, one row short
        assert raised(mex, cmd, *bad) == "ntm:arg: " + WS_TEXT
