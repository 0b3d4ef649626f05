"""Reference restatement of the resumable closed loops (ntm_mpc_run_from /
ntm_mpc_run_est_from, include/ntm_mpc.h): the loop composed step by step from the C
oracle's step (oracle/cbind.step) or from tests/estimator_ref.step, with the
configuration and the generator taken from a per-step schedule.  TEST INFRASTRUCTURE ONLY.

``schedule(k) -> (cfg, gen)`` gives step k's configuration and generator; the generator's
``k0`` it returns is the base, step k runs at time index ``gen.k0 + k`` as ntm_mpc_run
does.  ``constant(cfg, gen)`` is the schedule of an ordinary run.  The carried state is
(x, rho, U_old) (the oracle has no warm-start sets: they are a hint that never changes a
result beyond the solver's tolerance).
"""
from __future__ import annotations

import dataclasses

import numpy as np

import estimator_ref as E
from oracle import cbind


def constant(cfg, gen=None):
    return lambda k: (cfg, gen)


def switch_at(k_switch: int, before, after):
    """Schedule that returns ``before`` (a (cfg, gen) pair) for k < k_switch, else ``after``."""
    return lambda k: before if k < k_switch else after


def _at(gen, k):
    return None if gen is None else dataclasses.replace(gen, k0=gen.k0 + k)


def _histories(N, B, k_sim, est=False):
    h = {"xk": np.zeros((2 * (k_sim + 1), B)), "uk": np.zeros((k_sim, B)), "Uk": np.zeros((N * k_sim, B)),
         "wpred": np.zeros(((N + 1) * k_sim, B)), "exitflag": np.zeros((k_sim, B), np.int32),
         "inner_iters": np.zeros((k_sim, B), np.int32)}
    if est:
        h.update(dk=np.zeros((2 * (k_sim + 1), B)), xhk=np.zeros((2 * (k_sim + 1), B)), yk=np.zeros((2 * k_sim, B)))
    return h


def _record(h, k, N, r):
    h["uk"][k] = r["U"][0]
    h["Uk"][k * N:(k + 1) * N] = r["U"]
    h["wpred"][k * (N + 1):(k + 1) * (N + 1)] = r["x_pred"][0::2]
    h["exitflag"][k], h["inner_iters"][k] = r["exitflag"], r["inner_iters"]


def run_from(x, rho, U_old, k_sim: int, schedule, k_first: int = 0):
    """Steps k_first .. k_first + k_sim - 1 of the scheduled loop from the state (x, rho,
    U_old) ((E, B) arrays, not modified).  Returns (histories in ntm_mpc_run's layout,
    (x, rho, U_old) after the last step)."""
    x, rho, U_old = (np.array(a, dtype=float) for a in (x, rho, U_old))
    N, B = U_old.shape
    h = _histories(N, B, k_sim)
    h["xk"][:2] = x
    for k in range(k_sim):
        cfg, gen = schedule(k_first + k)
        assert cfg.N == N, "the horizon cannot change between steps"
        r = cbind.step(x, rho, U_old, cfg, gen=_at(gen, k_first + k))
        _record(h, k, N, r)
        x, rho, U_old = r["x_next"], r["rho"], r["U_old"]
        h["xk"][2 * (k + 1):2 * (k + 2)] = x
    return h, (x, rho, U_old)


def run(x0, k_sim: int, schedule):
    """The scheduled loop from x0: the initial state is the oracle's for step 0's (cfg, gen)."""
    cfg, gen = schedule(0)
    rho, U_old = cbind.initial_state_gen(np.ascontiguousarray(x0, dtype=float), cfg, gen)
    return run_from(x0, rho, U_old, k_sim, schedule)


def run_est_from(x, x_hat, rho, U_old, d_hat, k_sim: int, schedule, k_first: int = 0, route="c", phys=None):
    """The estimator loop: ``schedule(k) -> (cfg, gen, est)`` with est a dict of
    estimator_ref.step's options (nominal, gain, kappa, sigma_y).  Returns (histories in
    ntm_mpc_run_est's layout, (x, x_hat, rho, U_old, d_hat) after the last step)."""
    x, xh, rho, U_old, d = (np.array(a, dtype=float) for a in (x, x_hat, rho, U_old, d_hat))
    N, B = U_old.shape
    h = _histories(N, B, k_sim, est=True)
    h["xk"][:2], h["dk"][:2], h["xhk"][:2] = x, d, xh
    for k in range(k_sim):
        cfg, gen, est = schedule(k_first + k)
        assert cfg.N == N, "the horizon cannot change between steps"
        r = E.step(x, xh, rho, U_old, d, cfg, _at(gen, k_first + k), est.get("nominal", False), est.get("gain", 0.0),
                   est.get("kappa", 0.0), est.get("sigma_y", 0.0), route, phys)
        _record(h, k, N, r)
        x, xh, rho, U_old, d = r["x_next"], r["x_hat"], r["rho"], r["U_old"], r["d_hat"]
        h["xk"][2 * (k + 1):2 * (k + 2)] = x
        h["dk"][2 * (k + 1):2 * (k + 2)] = d
        h["xhk"][2 * (k + 1):2 * (k + 2)] = xh
        h["yk"][2 * k:2 * (k + 1)] = r["y"]
    return h, (x, xh, rho, U_old, d)
