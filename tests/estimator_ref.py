"""Reference restatement of the output-feedback step (ntm_mpc_step_est / ntm_mpc_run_est,
include/ntm_mpc.h): measurement noise and a fixed-gain state filter next to the
disturbance estimate, composed from tests/mismatch_ref.py and the oracle's own
functions.  TEST INFRASTRUCTURE ONLY.

One step, per scenario (global id ``gen.first_id + s``, time index ``gen.k0``); three
values are carried: the plant's state x, the estimate x_hat and d_hat:
  controller: mismatch_ref.step_one's solve (model k_m, C + d_hat) FROM x_hat;
  plant  x_next = O.plant_step(x, U[0], k_p) + O.disturbance;
  y_i    = x_next_i + sigma_y[i] O.gen_normal(seed, sid, k, 2 + i)   (skipped at sigma_y[i] == 0);
  m      = O.plant_step(x_hat, U[0], k_m)                 (no d_hat, no disturbance);
  iota_i = (y_i - m_i) - d_hat_i                          (the old d_hat);
  d_hat_i <- fma(gain[i], (y_i - m_i) - d_hat_i, d_hat_i) (kept where y_i - m_i is not finite);
  x_hat_i <- fma(-kappa[i], iota_i, y_i)                  (y_i where iota_i is not finite).
Where x_hat is x bit for bit, x_next is mismatch_ref.step_one's own (its plant step from
the state it solved from), so the degenerate options reproduce mismatch_ref bit for bit on
either route.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import mismatch_ref as M
from oracle import ntm_oracle as O


def _pair(v):
    a = np.broadcast_to(np.asarray(v, dtype=float), (2,))
    return float(a[0]), float(a[1])


def meas_noise(gen, sid: int, k: int, sigma_y):
    """sigma_y[i] n(seed, sid, k, 2 + i); exactly 0.0 where sigma_y[i] == 0 (no draw)."""
    sy = _pair(sigma_y)
    return np.array([sy[i] * O.gen_normal(gen.seed, sid, k, 2 + i) if sy[i] != 0.0 else 0.0 for i in range(2)])


def step_one(x, xh, rho, Uo, d, cfg: O.Config, phys: O.Physics, gen, s: int, nominal: bool, gain, kappa, sigma_y,
             route: str):
    """One scenario (column s of the batch): x, xh, d (2), rho (3N, record layout), Uo (N)."""
    gain, kappa, sy = _pair(gain), _pair(kappa), _pair(sigma_y)
    sid = 0 if gen is None else gen.first_id + s
    k = 0 if gen is None else gen.k0
    pm, pp = M.model_physics(phys, gen, sid, nominal), M.plant_physics(phys, gen, sid)
    r = M.step_one(xh, rho, Uo, d, cfg, phys, gen, s, nominal, 0.0, route)
    out = {k_: r[k_] for k_ in ("U", "x_pred", "rho", "U_old", "exitflag", "inner_iters")}
    u0 = out["U"][0]
    if np.array_equal(x, xh):
        xn = np.array(r["x_next"], dtype=float)
    else:
        dist = np.zeros(2) if gen is None else O.disturbance(gen, sid, k)
        xn = M._add_dist(O.plant_step(x, u0, pp, cfg), dist)
    if sy[0] != 0.0 or sy[1] != 0.0:
        assert gen is not None, "sigma_y != 0 needs a generator (its seed)"
        nz = meas_noise(gen, sid, k, sy)
        y = np.array([xn[i] + nz[i] if sy[i] != 0.0 else xn[i] for i in range(2)])
    else:
        y = np.array(xn)
    m = O.plant_step(xh, u0, pm, cfg)
    dn, xhn = np.zeros(2), np.zeros(2)
    for i in range(2):
        e = float(y[i]) - float(m[i])
        iota = e - float(d[i])
        dn[i] = M.fma(gain[i], e - float(d[i]), d[i]) if np.isfinite(e) else float(d[i])
        xhn[i] = M.fma(-kappa[i], iota, y[i]) if np.isfinite(iota) else float(y[i])
    out.update(x_next=xn, y=y, d_hat=dn, x_hat=xhn)
    return out


def step(x, xh, rho, Uo, d_hat, cfg: O.Config, gen=None, nominal=False, gain=0.0, kappa=0.0, sigma_y=0.0, route="c",
         phys=None):
    """Batched estimator step on (E, B) arrays (cbind.step's layout); inputs are not modified."""
    phys = phys or O.Physics()
    B, N = x.shape[1], cfg.N
    out = {"U": np.zeros((N, B)), "x_pred": np.zeros((2 * (N + 1), B)), "x_next": np.zeros((2, B)),
           "y": np.zeros((2, B)), "x_hat": np.zeros((2, B)), "rho": np.zeros((3 * N, B)), "U_old": np.zeros((N, B)),
           "d_hat": np.zeros((2, B)), "exitflag": np.zeros(B, np.int32), "inner_iters": np.zeros(B, np.int32)}
    for s in range(B):
        r = step_one(np.array(x[:, s]), np.array(xh[:, s]), np.array(rho[:, s]), np.array(Uo[:, s]),
                     np.array(d_hat[:, s]), cfg, phys, gen, s, nominal, gain, kappa, sigma_y, route)
        for k_, v in r.items():
            if out[k_].ndim == 2:
                out[k_][:, s] = v
            else:
                out[k_][s] = v
    return out


def run(x0, cfg: O.Config, k_sim: int, gen=None, nominal=False, gain=0.0, kappa=0.0, sigma_y=0.0, d0=None,
        xhat0=None, route="c", phys=None, iters=None):
    """The composed closed loop, ntm_mpc_run_est's layout: mismatch_ref.run's keys plus xhk
    (2(k_sim+1), B; column 0 the initial estimate) and yk (2 k_sim, B).  The initial rho is
    the model's at xhat0.  ``iters`` (k_sim, B): run step k of scenario s for exactly
    iters[k, s] LPV iterations (the replay along another implementation's path)."""
    B, N = x0.shape[1], cfg.N
    x = np.array(x0, dtype=float)
    xh = np.array(x0 if xhat0 is None else xhat0, dtype=float)
    d = np.zeros((2, B)) if d0 is None else np.array(d0, dtype=float)
    rho, Uo = M.initial_state(xh, cfg, gen, nominal, phys)
    h = {"xk": np.zeros((2 * (k_sim + 1), B)), "uk": np.zeros((k_sim, B)), "Uk": np.zeros((N * k_sim, B)),
         "wpred": np.zeros(((N + 1) * k_sim, B)), "dk": np.zeros((2 * (k_sim + 1), B)),
         "xhk": np.zeros((2 * (k_sim + 1), B)), "yk": np.zeros((2 * k_sim, B)),
         "exitflag": np.zeros((k_sim, B), np.int32), "inner_iters": np.zeros((k_sim, B), np.int32)}
    h["xk"][:2], h["dk"][:2], h["xhk"][:2] = x, d, xh
    for k in range(k_sim):
        g = None if gen is None else dataclasses.replace(gen, k0=gen.k0 + k)
        if iters is None:
            r = step(x, xh, rho, Uo, d, cfg, g, nominal, gain, kappa, sigma_y, route, phys)
        else:
            r = None
            for i_g in np.unique(iters[k]):
                rp = step(x, xh, rho, Uo, d, dataclasses.replace(cfg, i_sim=int(i_g), epsilon=-1.0), g, nominal,
                          gain, kappa, sigma_y, route, phys)
                if r is None:
                    r = rp
                sel = iters[k] == i_g
                for k_ in r:
                    r[k_][..., sel] = rp[k_][..., sel]
        h["uk"][k] = r["U"][0]
        h["Uk"][k * N:(k + 1) * N] = r["U"]
        h["wpred"][k * (N + 1):(k + 1) * (N + 1)] = r["x_pred"][0::2]
        h["exitflag"][k], h["inner_iters"][k] = r["exitflag"], r["inner_iters"]
        x, xh, rho, Uo, d = r["x_next"], r["x_hat"], r["rho"], r["U_old"], r["d_hat"]
        h["xk"][2 * (k + 1):2 * (k + 2)] = x
        h["dk"][2 * (k + 1):2 * (k + 2)] = d
        h["xhk"][2 * (k + 1):2 * (k + 2)] = xh
        h["yk"][2 * k:2 * (k + 1)] = r["y"]
    return h
