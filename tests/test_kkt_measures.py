"""tests/kkt_measures.py (the NumPy restatement of the KKT audit's four measures)
on the planted problems of tests/qp_planted.py, and the NumPy oracle's multipliers
as the precondition of the GPU bounds (tests/test_gpu_qp_dual.py): the reference
keeps those bounds with orders to spare.

Measured here (NumPy oracle, family_batch(N) at the twelve GPU horizons):
measures of the oracle's (U, lambda) <= 1.4e-15; its multipliers against the
planted ones (the five families where they are unique) <= 5.2e-14 of
max(1, max mu*) in mu units; the largest multiplier times (1 + 1e-3) reads
4.04e-6 in the stationarity measure; the largest entry of U moved by
1e-6 max(1, |U|) reads 1.57e-7 (the figure the issue quotes as 1.6e-7).
"""
import numpy as np
import pytest

import kkt_measures as K
import qp_planted as Q
from oracle import ntm_oracle as O


def _feasible(N):
    return [p for p in Q.family_batch(N) if p.flag == Q.FLAG_OK]


@pytest.mark.parametrize("N", Q.HORIZONS_GPU)
def test_planted_pair_measures_are_exact_zeros(N):
    """(U*, lambda*) is the KKT point by construction, in small integers times
    powers of two: every product and sum of the measures is exact, so all four
    are 0.0, not merely small.  In the five unique families each planted row
    matches exactly one row of the problem by (Lin_i, b_i)."""
    for p in _feasible(N):
        lam, unique = K.planted_lambda(p)
        if p.family in K.UNIQUE_FAMILIES:
            assert unique, (N, p.family)
        k = K.measures(p.G, p.F, p.Lin, p.b, p.Ustar, lam)
        assert np.all(k == 0.0), (N, p.family, k)


def test_no_rows_only_stationarity():
    p = Q.make("plain", 8, np.random.default_rng(5), k=0)
    k = K.measures(p.G, p.F, None, None, p.Ustar, None)
    assert np.all(k == 0.0), k
    k = K.measures(p.G, p.F, None, None, p.Ustar + 1.0, None)
    assert k[0] > 0.0 and np.all(k[1:] == 0.0), k


def test_each_measure_sees_its_own_defect():
    p = [q for q in _feasible(8) if q.family == "plain"][0]
    lam, _ = K.planted_lambda(p)
    i = int(np.argmax(lam))
    free = int(np.flatnonzero((p.b - p.Lin @ p.Ustar > 0) & np.any(p.Lin != 0, axis=1))[0])
    l2 = lam.copy(); l2[i] = -lam[i]                          # a negative multiplier
    assert K.measures(p.G, p.F, p.Lin, p.b, p.Ustar, l2)[2] > 0.1
    l3 = lam.copy(); l3[free] = 1.0                           # a multiplier on a slack row
    k3 = K.measures(p.G, p.F, p.Lin, p.b, p.Ustar, l3)
    assert k3[3] > 1e-3 and k3[2] == 0.0
    b2 = p.b.copy(); b2[free] = p.Lin[free] @ p.Ustar - 1.0   # a violated row
    k4 = K.measures(p.G, p.F, p.Lin, b2, p.Ustar, lam)
    assert k4[1] > 1e-3 and k4[0] == 0.0
    zero = int(np.flatnonzero(~np.any(p.Lin != 0, axis=1))[0])
    b3 = p.b.copy(); b3[zero] = -0.25                         # a violated constant row: the absolute test
    assert K.measures(p.G, p.F, p.Lin, b3, p.Ustar, lam)[1] == 0.25


def test_oracle_multipliers_and_sensitivity_figures():
    """The reference's own error and the sensitivity of the measures (module
    docstring): what the GPU bounds 1e-10 (multipliers) and 1e-9 (measures) rest on."""
    worst_k = worst_mu = 0.0
    see_lam = see_u = np.inf
    for N in Q.HORIZONS_GPU:
        for p in _feasible(N):
            U, flag, info = O.qp_solve(p.G, p.F, p.Lin, p.b)
            assert flag == 1
            lam = np.zeros(p.m)
            a = np.array(info["active"], dtype=int)
            if len(a):
                lam[a] = info["multipliers"]
            worst_k = max(worst_k, float(K.measures(p.G, p.F, p.Lin, p.b, U, lam).max()))
            if p.family in K.UNIQUE_FAMILIES:
                mus = K.to_mu(p.G, p.Lin, K.planted_lambda(p)[0])
                worst_mu = max(worst_mu, float(np.max(np.abs(K.to_mu(p.G, p.Lin, lam) - mus)) / max(1.0, mus.max())))
            if len(a):
                l2 = lam.copy()
                l2[a[np.argmax(lam[a])]] *= 1 + 1e-3
                see_lam = min(see_lam, float(K.measures(p.G, p.F, p.Lin, p.b, U, l2)[0]))
                U2 = U.copy()
                j = int(np.argmax(np.abs(U)))
                U2[j] += 1e-6 * max(1.0, abs(U[j]))
                see_u = min(see_u, float(K.measures(p.G, p.F, p.Lin, p.b, U2, lam).max()))
    print(f"oracle: measures {worst_k:.2e}, mu error {worst_mu:.2e}; sensitivity: lambda (1 + 1e-3) {see_lam:.2e}, "
          f"U 1e-6 {see_u:.2e}")
    assert worst_k <= 1.4e-15
    assert worst_mu <= 5.2e-14
    assert see_lam >= 4.0e-6
    assert see_u >= 1.5e-7          # measured 1.57e-7
