"""The four KKT measures of include/ntm_mpc.h (ntm_qp_kkt_device /
ntm_mpc_kkt_device), restated in NumPy on explicit QP data

    min 1/2 U'GU + F'U   s.t.  Lin U <= b,   Lagrangian + lam'(Lin U - b), lam >= 0.

With d_j = 1/sqrt(G_jj) (1 where G_jj <= 0), V = U/d, vmax = max(1, max|V|),
rn_i = |Lin_i o d|_2 (a constant row has rn_i = 0: 1 is used there),
mu_i = lam_i rn_i and mumax = max(1, max|mu|):

    [0] stationarity     max_j |(GU + F + Lin'lam)_j d_j| / max(1, max_j |F_j d_j|)
    [1] primal           max(0, max_i v_i), v_i = (Lin_i U - b_i)/(rn_i vmax);
                         v_i = -b_i on constant rows
    [2] dual             max(0, max_i -mu_i) / mumax
    [3] complementarity  max_i |mu_i (Lin_i U - b_i)/rn_i| / (mumax vmax), ordinary rows

the solver's own units, so its certificate tolerance 1e-9 is the bound the tests
use (KKT_TOL).  With m = 0 only [0] is non-zero.

This is a plain helper module (no fixtures, no tests).
"""
from __future__ import annotations

import numpy as np

KKT_TOL = 1e-9          # the device certificate's tolerance (StructRows / DenseRows check, multiplier test)


def scaling(G):
    """d_j = 1/sqrt(G_jj), 1 where G_jj <= 0 (the solver's Jacobi scaling)."""
    g = np.diag(G)
    pos = g > 0.0
    return np.where(pos, 1.0 / np.sqrt(np.where(pos, g, 1.0)), 1.0)


def row_norms(G, Lin):
    """rn_i = |Lin_i o d|_2 (0 for a constant row)."""
    return np.linalg.norm(Lin * scaling(G)[None, :], axis=1)


def to_mu(G, Lin, lam):
    """Multipliers in the solver's units: mu_i = lam_i rn_i (rn_i = 1 on constant rows)."""
    rn = row_norms(G, Lin)
    return np.asarray(lam) * np.where(rn > 0.0, rn, 1.0)


def measures(G, F, Lin, b, U, lam):
    """(4,) array of the measures above for one QP."""
    G, F, U = np.asarray(G, float), np.asarray(F, float), np.asarray(U, float)
    d = scaling(G)
    fmax = max(1.0, float(np.max(np.abs(F * d))))
    m = 0 if Lin is None else np.asarray(Lin).shape[0]
    if m == 0:
        return np.array([float(np.max(np.abs((G @ U + F) * d))) / fmax, 0.0, 0.0, 0.0])
    Lin, b, lam = np.asarray(Lin, float), np.asarray(b, float), np.asarray(lam, float)
    vmax = max(1.0, float(np.max(np.abs(U / d))))
    rn = np.linalg.norm(Lin * d[None, :], axis=1)
    const = ~(rn > 0.0)
    rn1 = np.where(const, 1.0, rn)
    res = Lin @ U - b
    mu = lam * rn1
    mumax = max(1.0, float(np.max(np.abs(mu))))
    stat = float(np.max(np.abs((G @ U + F + Lin.T @ lam) * d))) / fmax
    prim = max(0.0, float(np.max(np.where(const, -b, res / (rn1 * vmax)))))
    dual = max(0.0, float(np.max(-mu))) / mumax
    comp = float(np.max(np.where(const, 0.0, np.abs(mu * (res / rn1))))) / (mumax * vmax)
    return np.array([stat, prim, dual, comp])


def planted_lambda(p):
    """The planted multipliers of a tests/qp_planted.py problem scattered over its m
    rows: each planted tight row (p.Lt, p.lam) is matched to its index by
    (Lin_i, b_i).  Returns (lam (m,), unique): ``unique`` is False when some planted
    row matches more than one row of the problem (the match then takes the first)."""
    lam = np.zeros(p.m)
    bt = p.Lt @ p.Ustar
    unique = True
    for row, bi, li in zip(p.Lt, bt, p.lam):
        hit = np.flatnonzero(np.all(p.Lin == row[None, :], axis=1) & (p.b == bi))
        assert hit.size >= 1, p.family
        unique = unique and hit.size == 1
        lam[hit[0]] += li
    return lam, unique


UNIQUE_FAMILIES = ("plain", "vertex", "rowscale", "gscale", "bigm")        # the multipliers are unique
DEGENERATE_FAMILIES = ("dup", "weak", "eq", "dep", "vertex_dup")          # only the measures are defined
