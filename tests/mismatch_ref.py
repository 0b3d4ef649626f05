"""Reference restatement of the observer step (ntm_mpc_step_obs / ntm_mpc_run_obs,
include/ntm_mpc.h): plant-model mismatch and the offset-free disturbance estimate,
composed from the oracle's own functions.  TEST INFRASTRUCTURE ONLY.

One step, per scenario (global id ``gen.first_id + s``, time index ``gen.k0``):
  model  k_m = the nominal physics (nominal_model) or the scenario's, C + d_hat;
  plant  k_p = the scenario's physics; x_next = plant step + disturbance;
  e      = x_next - (k_m's one-step map without d_hat, no disturbance);
  d_hat <- fma(gain, e - d_hat, d_hat)   (one rounding; kept where e is not finite).

Two routes give the model's solve:
  (a) "numpy": O.mpc_step with O.C_vec returning C(model) + d_hat while it runs (the
      lift and the rollout read the offset through that function alone);
  (b) "c":     the C oracle, one scenario per cbind.step call, on an equivalent
      physics: j_BS (1 + d0/C1) and omega0 + d1 tau_E0/Ts (j_BS enters C1 only, omega0
      C2 only), so its C is C(model) + d_hat to a rounding of C.
The plant step and the innovation are the NumPy oracle's (O.plant_step, O.disturbance)
on both routes, with one exception: where the plant's physics IS route (b)'s
equivalent physics (no mismatch, d_hat = 0) the C oracle's own plant step and
disturbance are taken, so that route (b) is then cbind.step(..., gen=gen) bit for bit.
"""
from __future__ import annotations

import contextlib
import dataclasses
from fractions import Fraction

import numpy as np

from oracle import cbind
from oracle import ntm_oracle as O


def plant_physics(phys: O.Physics, gen, sid: int) -> O.Physics:
    return phys if gen is None else O.scenario_physics(phys, gen, sid)


def model_physics(phys: O.Physics, gen, sid: int, nominal: bool) -> O.Physics:
    return phys if nominal else plant_physics(phys, gen, sid)


def equivalent_physics(pm: O.Physics, cfg: O.Config, d) -> O.Physics:
    """The physics whose C_vec is C_vec(pm) + d (to a rounding): route (b)."""
    c = O.C_vec(pm, cfg.Ts)
    return dataclasses.replace(pm, j_BS=pm.j_BS * (1.0 + float(d[0]) / c[0]),
                               omega0=pm.omega0 + float(d[1]) * pm.tau_E0 / cfg.Ts)


def fma(a: float, b: float, c: float) -> float:
    """a b + c with one rounding (exact rational arithmetic, one float()), as O.gen_factor."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def update(gain: float, e, d):
    """d_hat <- fma(gain, e - d_hat, d_hat) per component; a non-finite e keeps d_hat."""
    return np.array([fma(gain, float(e[i]) - float(d[i]), d[i]) if np.isfinite(e[i]) else float(d[i])
                     for i in range(2)])


@contextlib.contextmanager
def _offset(d):
    """While active, O.C_vec returns C + d: the model's offset carries the estimate."""
    orig = O.C_vec
    O.C_vec = lambda phys, Ts: orig(phys, Ts) + np.asarray(d, dtype=float)
    try:
        yield
    finally:
        O.C_vec = orig


def _add_dist(xn, dist):
    return np.array([xn[0] + dist[0] if dist[0] != 0.0 else xn[0],
                     xn[1] + dist[1] if dist[1] != 0.0 else xn[1]])


def step_one(x, rho, Uo, d, cfg: O.Config, phys: O.Physics, gen, s: int, nominal: bool, gain: float, route: str):
    """One scenario (column s of the batch): x (2), rho (3N, record layout), Uo (N), d (2)."""
    N = cfg.N
    sid = 0 if gen is None else gen.first_id + s
    k = 0 if gen is None else gen.k0
    pm, pp = model_physics(phys, gen, sid, nominal), plant_physics(phys, gen, sid)
    dist = np.zeros(2) if gen is None else O.disturbance(gen, sid, k)
    xn = None
    if route == "numpy":
        with _offset(d):
            r = O.mpc_step(x, rho.reshape(N, 3).T, Uo, pm, cfg)
        out = {"U": r["U"], "x_pred": r["xpred"].T.reshape(-1), "rho": r["Rho"].T.reshape(-1), "U_old": r["Uold"],
               "exitflag": r["exitflag"], "inner_iters": r["inner_iters"]}
    else:
        pe = equivalent_physics(pm, cfg, d)
        same = pe == pp
        g1 = None
        if same and gen is not None:    # the C oracle's own plant step and disturbance
            g1 = dataclasses.replace(gen, first_id=sid, jbs_spread=0.0, wdep_spread=0.0)
        r = cbind.step(x.reshape(2, 1), rho.reshape(-1, 1), Uo.reshape(-1, 1), cfg, ph=pe, gen=g1)
        out = {"U": r["U"][:, 0], "x_pred": r["x_pred"][:, 0], "rho": r["rho"][:, 0], "U_old": r["U_old"][:, 0],
               "exitflag": int(r["exitflag"][0]), "inner_iters": int(r["inner_iters"][0])}
        if same:
            xn = r["x_next"][:, 0]
    if xn is None:
        xn = _add_dist(O.plant_step(x, out["U"][0], pp, cfg), dist)
    e = xn - O.plant_step(x, out["U"][0], pm, cfg)
    out["x_next"] = xn
    out["d_hat"] = update(gain, e, d)
    return out


def step(x, rho, Uo, d_hat, cfg: O.Config, gen=None, nominal=False, gain=0.0, route="c", phys=None):
    """Batched observer step on (E, B) arrays (cbind.step's layout); inputs are not modified."""
    phys = phys or O.Physics()
    B, N = x.shape[1], cfg.N
    out = {"U": np.zeros((N, B)), "x_pred": np.zeros((2 * (N + 1), B)), "x_next": np.zeros((2, B)),
           "rho": np.zeros((3 * N, B)), "U_old": np.zeros((N, B)), "d_hat": np.zeros((2, B)),
           "exitflag": np.zeros(B, np.int32), "inner_iters": np.zeros(B, np.int32)}
    for s in range(B):
        r = step_one(np.array(x[:, s]), np.array(rho[:, s]), np.array(Uo[:, s]), np.array(d_hat[:, s]), cfg, phys,
                     gen, s, nominal, gain, route)
        for k_, v in r.items():
            if out[k_].ndim == 2:
                out[k_][:, s] = v
            else:
                out[k_][s] = v
    return out


def initial_state(x0, cfg: O.Config, gen=None, nominal=False, phys=None):
    """rho (3N, B) = repmat(rho(x0)) of the MODEL, U_old = +inf."""
    phys = phys or O.Physics()
    B = x0.shape[1]
    rho = np.zeros((3 * cfg.N, B))
    for s in range(B):
        pm = model_physics(phys, gen, 0 if gen is None else gen.first_id + s, nominal)
        rho[:, s] = np.tile(O.rho_all(x0[:, s], pm, cfg), cfg.N)
    return rho, np.full((cfg.N, B), np.inf)


def run(x0, cfg: O.Config, k_sim: int, gen=None, nominal=False, gain=0.0, d0=None, route="c", phys=None,
        iters=None):
    """The composed closed loop, ntm_mpc_run_obs's layout: xk, uk, Uk, wpred, dk, exitflag,
    inner_iters.  ``iters`` (k_sim, B): run step k of scenario s for exactly iters[k, s]
    LPV iterations (the replay along another implementation's path)."""
    B, N = x0.shape[1], cfg.N
    x = np.array(x0, dtype=float)
    d = np.zeros((2, B)) if d0 is None else np.array(d0, dtype=float)
    rho, Uo = initial_state(x, cfg, gen, nominal, phys)
    h = {"xk": np.zeros((2 * (k_sim + 1), B)), "uk": np.zeros((k_sim, B)), "Uk": np.zeros((N * k_sim, B)),
         "wpred": np.zeros(((N + 1) * k_sim, B)), "dk": np.zeros((2 * (k_sim + 1), B)),
         "exitflag": np.zeros((k_sim, B), np.int32), "inner_iters": np.zeros((k_sim, B), np.int32)}
    h["xk"][:2], h["dk"][:2] = x, d
    for k in range(k_sim):
        g = None if gen is None else dataclasses.replace(gen, k0=gen.k0 + k)
        if iters is None:
            r = step(x, rho, Uo, d, cfg, g, nominal, gain, route, phys)
        else:
            r = None
            for i_g in np.unique(iters[k]):
                rp = step(x, rho, Uo, d, dataclasses.replace(cfg, i_sim=int(i_g), epsilon=-1.0), g, nominal, gain,
                          route, phys)
                if r is None:
                    r = rp
                sel = iters[k] == i_g
                for k_ in r:
                    r[k_][..., sel] = rp[k_][..., sel]
        h["uk"][k] = r["U"][0]
        h["Uk"][k * N:(k + 1) * N] = r["U"]
        h["wpred"][k * (N + 1):(k + 1) * (N + 1)] = r["x_pred"][0::2]
        h["exitflag"][k], h["inner_iters"][k] = r["exitflag"], r["inner_iters"]
        x, rho, Uo, d = r["x_next"], r["rho"], r["U_old"], r["d_hat"]
        h["xk"][2 * (k + 1):2 * (k + 2)] = x
        h["dk"][2 * (k + 1):2 * (k + 2)] = d
    return h
