"""Multipliers and objective of the dense QP entry (ntm_qp_dual_device) and the
dense KKT audit (ntm_qp_kkt_device) against optima planted by construction
(tests/qp_planted.py) and the certified fixtures.

The references are exact: planted integer multipliers, and for the audit the
NumPy restatement tests/kkt_measures.py.  Bounds: U_TOL = 1e-10 (the project's QP
bound) for U and, in mu units relative to max(1, max mu*), for the multipliers of
the five families where they are unique; KKT_TOL = 1e-9 (the device certificate's
own tolerance) for the four measures where the multipliers are not unique;
1e-12 (1/2 |U|'|G||U| + |F|'|U|) for fval (fp64 summation of <= N^2 + N = 4160
terms).  tests/test_kkt_measures.py holds the NumPy oracle to 5.2e-14 and 1.4e-15
on the same problems.
"""
import numpy as np
import pytest
import torch

import kkt_measures as K
import qp_planted as Q
from pathlib import Path

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
_CACHE = {}


def _np(ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def _solve_dual(ctl, ps):
    """(U, fval, flag, its, lam, kkt) of a batch: quadprog_dual, then the device
    audit of its own output."""
    args = [ctl.tensor(a) for a in Q.pack(ps)]
    U, fval, flag, its, lam = ctl.quadprog_dual(*args)
    kkt = ctl.kkt(*args, U, lam)
    return _np((U, fval, flag, its, lam, kkt))


def _family(ctl, N):
    if N not in _CACHE:
        ps = Q.family_batch(N)
        _CACHE[N] = (ps, _solve_dual(ctl, ps))
    return _CACHE[N]


def _check_dual(ps, U, fval, flag, lam, kkt, tag):
    """Per scenario: flag, U, multipliers (unique families) or measures (degenerate
    ones), fval, exact zeros where the flag is not 1, the device audit <= 1e-9."""
    wmu = wk = wf = wd = 0.0
    for i, p in enumerate(ps):
        assert flag[i] == p.flag, (tag, i, p.family, int(flag[i]))
        if p.flag != Q.FLAG_OK:
            assert np.all(U[:, i] == 0.0) and np.all(lam[:, i] == 0.0) and fval[i] == 0.0, (tag, i, p.family)
            continue
        assert p.err(U[:, i]) <= Q.U_TOL, (tag, i, p.family, p.err(U[:, i]))
        if p.family in K.UNIQUE_FAMILIES:
            mus = K.to_mu(p.G, p.Lin, K.planted_lambda(p)[0])
            e = float(np.max(np.abs(K.to_mu(p.G, p.Lin, lam[:, i]) - mus)) / max(1.0, mus.max()))
            wmu = max(wmu, e)
            assert e <= Q.U_TOL, (tag, i, p.family, e)
        else:
            k = K.measures(p.G, p.F, p.Lin, p.b, U[:, i], lam[:, i])
            wk = max(wk, float(k.max()))
            assert np.all(k <= K.KKT_TOL), (tag, i, p.family, k)
        u = U[:, i]
        ref = 0.5 * u @ p.G @ u + p.F @ u
        bound = 1e-12 * (0.5 * np.abs(u) @ np.abs(p.G) @ np.abs(u) + np.abs(p.F) @ np.abs(u))
        wf = max(wf, abs(fval[i] - ref) / bound if bound > 0 else 0.0)
        assert abs(fval[i] - ref) <= bound, (tag, i, p.family, fval[i], ref)
        wd = max(wd, float(kkt[:, i].max()))
        assert np.all(kkt[:, i] <= K.KKT_TOL), (tag, i, p.family, kkt[:, i])
    print(f"{tag}: mu error {wmu:.1e}, degenerate families' measures {wk:.1e}, fval error / bound {wf:.1e}, "
          f"device audit {wd:.1e}")


@pytest.mark.parametrize("N", Q.HORIZONS_GPU)
def test_planted_multipliers_and_objective(ctl, N):
    """family_batch(N): B = 25, m = 8N + 4 (at N = 64 the LDS limit), two constant
    rows per scenario.  U, exitflag and iters are ntm_qp_device's bit for bit."""
    ps, (U, fval, flag, its, lam, kkt) = _family(ctl, N)
    assert lam.shape == (8 * N + 4, len(ps))
    _check_dual(ps, U, fval, flag, lam, kkt, f"k_qp_dual N={N}")
    U0, flag0, its0 = _np(ctl.quadprog(*[ctl.tensor(a) for a in Q.pack(ps)]))
    assert np.array_equal(_bits(U), _bits(U0)) and np.array_equal(flag, flag0) and np.array_equal(its, its0)


@pytest.mark.parametrize("N", [3, 16, 17])
@pytest.mark.parametrize("batch", ["mixed_fates", "bad_hessians"])
def test_other_fates_export_zeros(ctl, N, batch):
    """Scenarios that end infeasible or non-finite beside healthy ones (four per
    wave at N <= 16): lambda exactly 0 and fval 0 wherever the flag is not 1, the
    neighbours meet every bound, and the whole output is bitwise the same with the
    batch reversed."""
    ps = getattr(Q, batch)(N)
    U, fval, flag, its, lam, kkt = _solve_dual(ctl, ps)
    _check_dual(ps, U, fval, flag, lam, kkt, f"k_qp_dual {batch} N={N}")
    U2, fval2, flag2, its2, lam2, kkt2 = _solve_dual(ctl, ps[::-1])
    for a, b in ((U, U2), (lam, lam2), (kkt, kkt2)):
        assert np.array_equal(_bits(a), _bits(b[:, ::-1]))
    for a, b in ((fval, fval2), (flag, flag2), (its, its2)):
        assert np.array_equal(_bits(a), _bits(b[::-1]))


def test_no_rows(ctl):
    """m = 0: no lambda, fval at the unconstrained minimiser, only the
    stationarity measure is non-zero."""
    ps = [Q.make("plain", N, np.random.default_rng(70 + i), k=0, m=0) for i, N in enumerate((8, 8, 8))]
    Gb, Fb, _, _ = Q.pack(ps)
    G, F = ctl.tensor(Gb), ctl.tensor(Fb)
    U, fval, flag, its, lam = ctl.quadprog_dual(G, F, None, None)
    kkt = ctl.kkt(G, F, None, None, U, None)
    U, fval, flag, lam, kkt = _np((U, fval, flag, lam, kkt))
    assert lam.shape == (0, 3) and np.all(flag == 1)
    for i, p in enumerate(ps):
        assert p.err(U[:, i]) <= Q.U_TOL
        u = U[:, i]
        bound = 1e-12 * (0.5 * np.abs(u) @ np.abs(p.G) @ np.abs(u) + np.abs(p.F) @ np.abs(u))
        assert abs(fval[i] - (0.5 * u @ p.G @ u + p.F @ u)) <= bound
        assert kkt[0, i] <= K.KKT_TOL and np.all(kkt[1:, i] == 0.0)


# ---------------------------------------------------------------- the audit kernel itself

def _planted_pairs(ps):
    Us = np.stack([p.Ustar for p in ps], axis=1)
    lam = np.stack([K.planted_lambda(p)[0] if p.flag == Q.FLAG_OK else np.zeros(p.m) for p in ps], axis=1)
    return Us, lam


@pytest.mark.parametrize("N", Q.HORIZONS_GPU)
def test_audit_of_planted_pairs(ctl, N):
    """On (U*, lambda*) of the five unique families ntm_qp_kkt_device returns exactly
    [0, 0, 0, 0]: every product and sum is of small integers times powers of two.
    With the largest planted multiplier times (1 + 2^-10) the stationarity measure
    is >= 1e-6 and agrees with the NumPy measure to 1e-9 relative (both are fp64
    sums of the same <= 580 terms)."""
    ps = Q.family_batch(N)
    args = [ctl.tensor(a) for a in Q.pack(ps)]
    Us, lam = _planted_pairs(ps)
    kkt, = _np((ctl.kkt(*args, ctl.tensor(Us), ctl.tensor(lam)),))
    l2 = lam.copy()
    l2[np.argmax(lam, axis=0), np.arange(len(ps))] *= 1 + 2.0 ** -10
    kk2, = _np((ctl.kkt(*args, ctl.tensor(Us), ctl.tensor(l2)),))
    worst = 0.0
    for i, p in enumerate(ps):
        if p.family not in K.UNIQUE_FAMILIES:
            continue
        assert np.all(kkt[:, i] == 0.0), (N, i, p.family, kkt[:, i])
        ref = K.measures(p.G, p.F, p.Lin, p.b, Us[:, i], l2[:, i])
        assert kk2[0, i] >= 1e-6 and ref[0] >= 1e-6, (N, i, p.family, kk2[:, i], ref)
        worst = max(worst, abs(kk2[0, i] - ref[0]) / ref[0])
        assert abs(kk2[0, i] - ref[0]) <= 1e-9 * ref[0], (N, i, p.family, kk2[0, i], ref[0])
        assert np.allclose(kk2[1:, i], ref[1:], rtol=1e-9, atol=0.0), (N, i, p.family, kk2[:, i], ref)
    print(f"k_qp_kkt N={N}: perturbed stationarity, device against NumPy {worst:.1e} relative")


@pytest.mark.parametrize("N", [8, 17])
def test_audit_nan_stays_in_its_scenario(ctl, N):
    """A NaN in U or in lambda gives NaN for that scenario alone (four scenarios
    share a wave at N = 8)."""
    ps = [p for p in Q.family_batch(N) if p.family in K.UNIQUE_FAMILIES]
    args = [ctl.tensor(a) for a in Q.pack(ps)]
    Us, lam = _planted_pairs(ps)
    Us[N // 2, 1] = np.nan
    lam[3, 2] = np.nan
    lam[int(np.argmax(lam[:, 5])), 5] = np.inf
    kkt, = _np((ctl.kkt(*args, ctl.tensor(Us), ctl.tensor(lam)),))
    for i in range(len(ps)):
        if i in (1, 2, 5):
            assert np.all(np.isnan(kkt[:, i])), (i, kkt[:, i])
        else:
            assert np.all(kkt[:, i] == 0.0), (i, kkt[:, i])


@pytest.mark.parametrize("name", ["qp_m1_N20", "qp_m2_N20", "qp_m3_N20", "qp_m2_N50", "qp_m3_N50", "qp_m2_N10"])
def test_audit_of_certified_fixtures(ctl, name):
    """The MPC-structured QPs of the golden fixtures (cond(G) 1e9-1e11): U against
    the 50-digit optimum, and both audits of the solver's (U, lambda) <= 1e-9."""
    d = np.load(GOLD / f"{name}.npz")
    n = d["G"].shape[0]
    Gb = np.stack([d["G"][i].reshape(-1, order="F") for i in range(n)], axis=1)
    Lb = np.stack([d["Lin"][i].reshape(-1, order="F") for i in range(n)], axis=1)
    args = [ctl.tensor(a) for a in (Gb, d["F"].T, Lb, d["b"].T)]
    U, fval, flag, its, lam = ctl.quadprog_dual(*args)
    kkt = ctl.kkt(*args, U, lam)
    U, flag, lam, kkt = _np((U, flag, lam, kkt))
    np.testing.assert_array_equal(flag, d["exitflag"])
    assert np.max(np.abs(U - d["U_exact"].T)) <= 1e-10 * 2e6
    ref = np.stack([K.measures(d["G"][i], d["F"][i], d["Lin"][i], d["b"][i], U[:, i], lam[:, i]) for i in range(n)],
                   axis=1)
    print(f"{name}: device audit {kkt.max(axis=1)}, NumPy measures {ref.max(axis=1)}")
    assert np.all(kkt <= K.KKT_TOL), kkt.max(axis=1)
    assert np.all(ref <= K.KKT_TOL), ref.max(axis=1)
