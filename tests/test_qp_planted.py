"""Both CPU oracles against optima planted by construction (tests/qp_planted.py).

The reference of every other QP test is a restatement of the solver's own
method; here it is the integer U* each problem was built from, exact in fp64.
This file pins the generator (its KKT conditions hold exactly) and is the
standing proof that the oracles sit inside the project's bound on every
family, degenerate active sets included:

    max |(U - U*) s| <= 1e-10 max(1, max |U* s|),   flag 1    (feasible)
    flag -2 and U = 0                                          (infeasible)
    flag -7 and U = 0                                          (non-finite data, G not PD)
"""
import numpy as np
import pytest

import qp_planted as Q
from oracle import cbind
from oracle import ntm_oracle as O

DRAWS = 3


def _solve_both(p):
    Up, fp, _ = O.qp_solve(p.G, p.F, p.Lin, p.b)
    Uc, fc, its = cbind.qp(p.G, p.F, p.Lin, p.b)
    return (Up, fp), (Uc, fc), its


@pytest.mark.parametrize("N", Q.HORIZONS_CPU)
@pytest.mark.parametrize("family", Q.FAMILIES)
def test_oracles_find_planted_optimum(family, N):
    if family == "infeas3" and N < 2:
        with pytest.raises(ValueError):          # the family does not exist at N = 1
            Q.make(family, N, np.random.default_rng(0))
        return
    worst = 0.0
    for draw in range(DRAWS):
        p = Q.make(family, N, np.random.default_rng(Q.seed_of(family, N, draw)), nzero=draw)
        (Up, fp), (Uc, fc), its = _solve_both(p)
        assert fp == p.flag and fc == p.flag, (draw, fp, fc)
        if p.flag == Q.FLAG_OK:
            ntight = Q.check_kkt(p)
            if family in ("weak", "vertex_dup"):
                assert ntight > N
            if family in ("vertex", "vertex_dup", "bigm"):
                assert np.linalg.cond(p.LA) <= 10.0
            if family == "bigm":
                assert p.m == 8 * N + 4
            ep, ec = p.err(Up), p.err(Uc)
            worst = max(worst, ep, ec)
            assert ep <= Q.U_TOL and ec <= Q.U_TOL, (draw, ep, ec)
            assert p.min_iters <= its <= 10 * (N + p.m) + 50, (draw, its)
        else:
            assert np.all(Up == 0.0) and np.all(Uc == 0.0)
    print(f"{family} N={N}: worst oracle error {worst:.2e}")


def test_vertex_rows_are_well_conditioned():
    """Family 6's matrix: strictly diagonally dominant at every horizon, so the
    planted vertex is as well determined as the bound assumes."""
    for N in Q.HORIZONS_GPU:
        for seed in range(20):
            M = Q.vertex_matrix(np.random.default_rng(seed), N)
            assert np.linalg.matrix_rank(M) == N
            assert np.linalg.cond(M) <= 10.0, (N, seed)


def test_batch_pads_to_a_common_m():
    for N in (1, 2, 17):
        ps = Q.batch(N, draws=2, nzero=2)
        assert len(ps) == 2 * len(Q.families_for(N))
        assert {p.m for p in ps} == {8 * N + 4}
        assert {p.family for p in ps} == set(Q.families_for(N))
        for p in ps:
            assert int(np.sum(~p.Lin.any(axis=1) & (p.b == 1.0))) >= 2
            if p.flag == Q.FLAG_OK:
                Q.check_kkt(p)
        Gb, Fb, Lb, bb = Q.pack(ps)
        assert Gb.shape == (N * N, len(ps)) and Lb.shape == ((8 * N + 4) * N, len(ps))
        np.testing.assert_array_equal(Lb[:, 3].reshape(N, -1).T, ps[3].Lin)


@pytest.mark.parametrize("N", [3, 16, 20])
@pytest.mark.parametrize("kind", Q.NONFINITE_KINDS + Q.BAD_G_KINDS)
def test_oracles_nonfinite_contract(kind, N):
    """NaN or +-Inf anywhere in G, F, Lin, b, and a G that is zero, indefinite or
    singular PSD: flag -7 and U = 0 from both oracles."""
    p = Q.spoil(Q.make("plain", N, np.random.default_rng(5 + N), nzero=1), kind)
    (Up, fp), (Uc, fc), _ = _solve_both(p)
    assert fp == fc == Q.FLAG_NONFINITE, (fp, fc)
    assert np.all(Up == 0.0) and np.all(Uc == 0.0)


def _oracles_agree_with(ps):
    for i, p in enumerate(ps):
        (Up, fp), (Uc, fc), _ = _solve_both(p)
        assert fp == fc == p.flag, (i, p.family, fp, fc, p.flag)
        if p.flag == Q.FLAG_OK:
            assert p.err(Up) <= Q.U_TOL and p.err(Uc) <= Q.U_TOL, (i, p.family, p.err(Up), p.err(Uc))
        else:
            assert np.all(Up == 0.0) and np.all(Uc == 0.0), (i, p.family)


@pytest.mark.parametrize("N", Q.HORIZONS_GPU)
def test_oracles_on_the_gpu_batches(N):
    """The batches tests/test_gpu_qp_planted.py sends to the device (every family
    padded to m = 8N + 4, with constant rows): the flags and optima it expects
    are the ones both oracles give."""
    _oracles_agree_with(Q.family_batch(N))


@pytest.mark.parametrize("N", [3, 8, 16, 17, 20])
def test_oracles_on_the_mixed_fate_batches(N):
    _oracles_agree_with(Q.mixed_fates(N) + Q.bad_hessians(N))


@pytest.mark.parametrize("N", [3, 16, 20, 33])
def test_oracles_on_scalings_beyond_fp32(N):
    """Power-of-two scalings far outside fp32's range change nothing in fp64."""
    ps = Q.beyond_fp32(N)
    for p in ps:
        Q.check_kkt(p)
    assert np.float32(ps[0].G[0, 0]) == np.inf
    act = ps[1].Lt
    assert np.all(act.astype(np.float32) == 0.0) and np.any(act != 0.0)
    _oracles_agree_with(ps)
