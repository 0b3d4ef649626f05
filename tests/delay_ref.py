"""Reference restatement of the actuator dead time (ntm_mpc_step_dly / ntm_mpc_run_dly,
include/ntm_mpc.h): delayed inputs and the delay-compensating plan, composed from
tests/estimator_ref.py, tests/mismatch_ref.py and the oracle's own functions.  TEST
INFRASTRUCTURE ONLY.

One step, per scenario; four values are carried: x, x_hat, d_hat and the queue q[steps] of
pending inputs, oldest first:
  plan   z = x_hat; with predict, z <- O.plant_step(z, q[j], k_m) under
         mismatch_ref._offset(d_hat) (the model WITH d_hat, no disturbance), j = 0 .. steps-1;
  controller: mismatch_ref.step_one's solve (model k_m, C + d_hat) FROM z; u_cmd = U[0];
  u_app  = q[0] if steps > 0 else u_cmd;
  plant, y, m, d_hat, x_hat: estimator_ref.step_one's expressions with u_app for U[0];
  queue  q <- (q[1:], u_cmd).
With steps = 0 this is estimator_ref.step_one bit for bit: z is x_hat, u_app is U[0], and
where x_hat is x the plant step is the solve's own, as there.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import estimator_ref as E
import mismatch_ref as M
from oracle import ntm_oracle as O


def plan_state(xh, q, d, pm: O.Physics, cfg: O.Config, predict: bool):
    """x_hat carried over the queued inputs by the model with C + d_hat."""
    z = np.array(xh, dtype=float)
    if predict:
        with M._offset(d):
            for u in q:
                z = np.asarray(O.plant_step(z, float(u), pm, cfg), dtype=float)
    return z


def step_one(x, xh, rho, Uo, d, q, cfg: O.Config, phys: O.Physics, gen, s: int, nominal: bool, gain, kappa, sigma_y,
             predict: bool, route: str):
    """One scenario (column s of the batch): x, xh, d (2), rho (3N), Uo (N), q (steps)."""
    gain, kappa, sy = E._pair(gain), E._pair(kappa), E._pair(sigma_y)
    steps = len(q)
    sid = 0 if gen is None else gen.first_id + s
    k = 0 if gen is None else gen.k0
    pm, pp = M.model_physics(phys, gen, sid, nominal), M.plant_physics(phys, gen, sid)
    z = plan_state(xh, q, d, pm, cfg, predict)
    r = M.step_one(z, rho, Uo, d, cfg, phys, gen, s, nominal, 0.0, route)
    out = {k_: r[k_] for k_ in ("U", "x_pred", "rho", "U_old", "exitflag", "inner_iters")}
    u_cmd = out["U"][0]
    u_app = float(q[0]) if steps > 0 else u_cmd
    if steps == 0 and np.array_equal(x, xh):
        xn = np.array(r["x_next"], dtype=float)
    else:
        dist = np.zeros(2) if gen is None else O.disturbance(gen, sid, k)
        xn = M._add_dist(O.plant_step(x, u_app, pp, cfg), dist)
    if sy[0] != 0.0 or sy[1] != 0.0:
        assert gen is not None, "sigma_y != 0 needs a generator (its seed)"
        nz = E.meas_noise(gen, sid, k, sy)
        y = np.array([xn[i] + nz[i] if sy[i] != 0.0 else xn[i] for i in range(2)])
    else:
        y = np.array(xn)
    m = O.plant_step(xh, u_app, pm, cfg)
    dn, xhn = np.zeros(2), np.zeros(2)
    for i in range(2):
        e = float(y[i]) - float(m[i])
        iota = e - float(d[i])
        dn[i] = M.fma(gain[i], e - float(d[i]), d[i]) if np.isfinite(e) else float(d[i])
        xhn[i] = M.fma(-kappa[i], iota, y[i]) if np.isfinite(iota) else float(y[i])
    qn = np.concatenate([np.asarray(q[1:], dtype=float), [u_cmd]]) if steps > 0 else np.zeros(0)
    out.update(x_next=xn, y=y, d_hat=dn, x_hat=xhn, x_plan=z, u_applied=u_app, u_queue=qn)
    return out


def step(x, xh, rho, Uo, d_hat, q, cfg: O.Config, gen=None, nominal=False, gain=0.0, kappa=0.0, sigma_y=0.0,
         predict=True, route="c", phys=None):
    """Batched step on (E, B) arrays (cbind.step's layout), q (steps, B); inputs are not modified."""
    phys = phys or O.Physics()
    B, N, steps = x.shape[1], cfg.N, q.shape[0]
    out = {"U": np.zeros((N, B)), "x_pred": np.zeros((2 * (N + 1), B)), "x_next": np.zeros((2, B)),
           "y": np.zeros((2, B)), "x_hat": np.zeros((2, B)), "rho": np.zeros((3 * N, B)), "U_old": np.zeros((N, B)),
           "d_hat": np.zeros((2, B)), "x_plan": np.zeros((2, B)), "u_applied": np.zeros(B),
           "u_queue": np.zeros((steps, B)), "exitflag": np.zeros(B, np.int32), "inner_iters": np.zeros(B, np.int32)}
    for s in range(B):
        r = step_one(np.array(x[:, s]), np.array(xh[:, s]), np.array(rho[:, s]), np.array(Uo[:, s]),
                     np.array(d_hat[:, s]), np.array(q[:, s]), cfg, phys, gen, s, nominal, gain, kappa, sigma_y,
                     predict, route)
        for k_, v in r.items():
            if out[k_].ndim == 2:
                out[k_][:, s] = v
            else:
                out[k_][s] = v
    return out


def run(x0, cfg: O.Config, k_sim: int, steps: int, gen=None, nominal=False, gain=0.0, kappa=0.0, sigma_y=0.0,
        d0=None, xhat0=None, uq0=None, predict=True, route="c", phys=None, iters=None):
    """The composed closed loop, ntm_mpc_run_dly's layout: estimator_ref.run's keys plus uak
    (k_sim, B), the applied input, and xpk (2 k_sim, B), the plan state.  The initial rho is
    the model's at xhat0; uq0 None: zeros.  ``iters`` as estimator_ref.run."""
    B, N = x0.shape[1], cfg.N
    x = np.array(x0, dtype=float)
    xh = np.array(x0 if xhat0 is None else xhat0, dtype=float)
    d = np.zeros((2, B)) if d0 is None else np.array(d0, dtype=float)
    q = np.zeros((steps, B)) if uq0 is None else np.array(uq0, dtype=float)
    assert q.shape == (steps, B)
    rho, Uo = M.initial_state(xh, cfg, gen, nominal, phys)
    h = {"xk": np.zeros((2 * (k_sim + 1), B)), "uk": np.zeros((k_sim, B)), "Uk": np.zeros((N * k_sim, B)),
         "wpred": np.zeros(((N + 1) * k_sim, B)), "dk": np.zeros((2 * (k_sim + 1), B)),
         "xhk": np.zeros((2 * (k_sim + 1), B)), "yk": np.zeros((2 * k_sim, B)), "uak": np.zeros((k_sim, B)),
         "xpk": np.zeros((2 * k_sim, B)), "exitflag": np.zeros((k_sim, B), np.int32),
         "inner_iters": np.zeros((k_sim, B), np.int32)}
    h["xk"][:2], h["dk"][:2], h["xhk"][:2] = x, d, xh
    for k in range(k_sim):
        g = None if gen is None else dataclasses.replace(gen, k0=gen.k0 + k)
        if iters is None:
            r = step(x, xh, rho, Uo, d, q, cfg, g, nominal, gain, kappa, sigma_y, predict, route, phys)
        else:
            r = None
            for i_g in np.unique(iters[k]):
                rp = step(x, xh, rho, Uo, d, q, dataclasses.replace(cfg, i_sim=int(i_g), epsilon=-1.0), g, nominal,
                          gain, kappa, sigma_y, predict, route, phys)
                if r is None:
                    r = rp
                sel = iters[k] == i_g
                for k_ in r:
                    r[k_][..., sel] = rp[k_][..., sel]
        h["uk"][k] = r["U"][0]
        h["uak"][k] = r["u_applied"]
        h["Uk"][k * N:(k + 1) * N] = r["U"]
        h["wpred"][k * (N + 1):(k + 1) * (N + 1)] = r["x_pred"][0::2]
        h["xpk"][2 * k:2 * (k + 1)] = r["x_plan"]
        h["exitflag"][k], h["inner_iters"][k] = r["exitflag"], r["inner_iters"]
        x, xh, rho, Uo, d, q = r["x_next"], r["x_hat"], r["rho"], r["U_old"], r["d_hat"], r["u_queue"]
        h["xk"][2 * (k + 1):2 * (k + 2)] = x
        h["dk"][2 * (k + 1):2 * (k + 2)] = d
        h["xhk"][2 * (k + 1):2 * (k + 2)] = xh
        h["yk"][2 * k:2 * (k + 1)] = r["y"]
    h["u_queue"] = q
    return h
