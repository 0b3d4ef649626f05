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


def test_drop_families_keep_every_earlier_seed():
    """The drop families sit behind the twelve in seed_of's order and outside
    FAMILIES: no seed, batch or recorded figure of the earlier families moved."""
    assert Q.FAMILIES == ("plain", "dup", "weak", "eq", "dep", "vertex", "vertex_dup", "rowscale", "gscale", "bigm",
                          "infeas2", "infeas3")
    assert [Q.seed_of(f, 7, 1) for f in ("plain", "bigm", "infeas2", "infeas3")] == \
        [7064, 9000027 + 7064, 10000030 + 7064, 11000033 + 7064]
    assert Q.seed_of("drop", 7, 1) == 12000036 + 7064 and Q.seed_of("dropdep", 7, 1) == 13000039 + 7064
    assert Q.families_for(1, drops=True) == Q.families_for(1) and "drop" not in Q.families_for(8)
    assert Q.families_for(8, drops=True) == Q.families_for(8) + Q.DROP_FAMILIES
    assert len(Q.family_batch(2)) == 25
    for f in Q.DROP_FAMILIES:
        with pytest.raises(ValueError):            # N = 1 cannot drop: the families do not exist there
            Q.make_drop(f, 1, 0)


@pytest.mark.parametrize("N", [n for n in Q.HORIZONS_CPU if n >= 2])
def test_oracles_on_the_drop_batches(N):
    """drop_batch(N), the batch tests/test_gpu_qp_drops.py sends to the device.  The
    construction holds exactly and only the k planted rows are tight at U*; the
    counting copy of the oracle's loop (held to the oracle's own U, flag, set and
    count inside make_drop) dropped >= 2 rows on every drop problem and met >= 1
    dependent row and dropped >= 1 on every dropdep problem, on the problem as
    stated and on its Jacobi-scaled form (the units the C oracle and the device
    pick rows in); both oracles end inside the bound.  Recorded here: N = 2 ... 64,
    2 to 17 drops per problem on either path, the C oracle's iteration count equal
    to the scaled path's on every problem (printed, not asserted: ties may round
    differently), largest |data| 1390, both oracles
    within 1e-17 of U* (their exact re-solve on the final set leaves no more)."""
    ps = Q.drop_batch(N)
    assert [p.family for p in ps] == ["drop", "dropdep"] * 2 + ["plain"] + ["drop", "dropdep"] * 2
    assert len({p.m for p in ps}) == 1 and ps[0].m <= 8 * N + 4
    worst = big = 0.0
    cdrops = []
    for i, p in enumerate(ps):
        k = p.LA.shape[0]
        assert Q.check_kkt(p) == k and np.all(p.lam > 0.0) and np.linalg.matrix_rank(p.LA) == k
        assert int(np.sum(~p.Lin.any(axis=1) & (p.b == 1.0))) >= 2
        big = max(big, np.abs(p.G).max(), np.abs(p.F).max(), np.abs(p.b).max())
        if p.family != "plain":
            c = p.path
            assert p.min_iters == k                    # of any path; this oracle's took k + 2 drops
            assert c["iterations"] == c["adds"] + c["drops"] == k + 2 * c["drops"], (i, c)
            assert c["candidate"] < Q.DROP_SEARCH_CAP
            if p.family == "drop":
                assert c["drops"] >= 2 and c["scaled_drops"] >= 2, (i, c)
            else:
                assert c["deps"] >= 1 and c["drops"] >= 1 and c["scaled_deps"] >= 1 and c["scaled_drops"] >= 1, (i, c)
        (Up, fp), (Uc, fc), its = _solve_both(p)
        assert fp == fc == Q.FLAG_OK, (i, p.family, fp, fc)
        ep, ec = p.err(Up), p.err(Uc)
        worst = max(worst, ep, ec)
        assert ep <= Q.U_TOL and ec <= Q.U_TOL, (i, p.family, ep, ec)
        assert p.min_iters <= its <= 10 * (N + p.m) + 50 and (its - k) % 2 == 0, (i, p.family, its)
        if p.path:
            cdrops.append((its - k) // 2)
    assert big < 2.0 ** 20                         # every product of two entries is exact in fp64
    paths = [p.path for p in ps if p.path]
    if N >= 8:                                     # drops whose Givens sweep leaves rotated columns behind
        assert sum(c["scaled_deep"] > 0 for c in paths) >= 4, [c["scaled_deep"] for c in paths]
    print(f"drop batch N={N} m={ps[0].m}: drops {[c['drops'] for c in paths]}, dependent {[c['deps'] for c in paths]}; "
          f"scaled {[c['scaled_drops'] for c in paths]}, {[c['scaled_deps'] for c in paths]}; the C oracle's drops "
          f"{cdrops}; candidates {[c['candidate'] for c in paths]}; largest |data| {big:.0f}, "
          f"worst oracle error {worst:.1e}")


def test_drop_search_is_deterministic_and_loud():
    """The same (family, N, draw) gives the same problem, whatever was drawn
    before; a criterion nothing meets raises, it never hands back an unchecked
    candidate."""
    a, b = Q.make_drop("dropdep", 8, 1, nzero=1), Q.make_drop("dropdep", 8, 1, nzero=1)
    assert np.array_equal(a.Lin, b.Lin) and np.array_equal(a.F, b.F) and a.path == b.path
    with pytest.raises(RuntimeError):
        Q.make_drop("drop", 2, 0, min_drops=10 ** 6)


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
