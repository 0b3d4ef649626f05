"""The stand-alone QP entry points (ntm_qp_device / ntm_qp_mixed_device: k_qp and
k_qp_mixed over DenseRows) against optima planted by construction.

No solver is the reference here: every problem of tests/qp_planted.py is built
backwards from an integer U*, exact in fp64 (tests/test_qp_planted.py holds both
CPU oracles to the same answers).  What is checked, per scenario:

    feasible     flag 1 and max |(U - U*) s| <= 1e-10 max(1, max |U* s|)
    infeasible   flag -2 and U == 0 exactly
    non-finite   flag -7 and U == 0 exactly (NaN / Inf in G, F, Lin, b; G not PD)

at the horizons where k_qp changes path (N <= 16: four scenarios per wave,
N >= 17: one; N <= 32: explicit T = R^-1, N >= 33: back substitution), at the
largest row count (m = 8N + 4, at N = 64 the LDS limit), on degenerate active
sets (duplicated, opposed, dependent and weakly active rows, full vertices),
and with different fates inside one wave.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import qp_planted as Q

pytestmark = pytest.mark.gpu

NTM_E_UNSUPPORTED = -4      # include/ntm_mpc.h


def _solve(ctl, ps, mixed=False):
    args = [ctl.tensor(a) for a in Q.pack(ps)]
    out = ctl.quadprog_mixed(*args) if mixed else ctl.quadprog(*args)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check(ps, U, flag, its=None, tag=""):
    """Flags, planted optima, exact zeros, iteration bounds; prints the worst
    error per family (of the bound's quantity) and returns it."""
    worst = {}
    for i, p in enumerate(ps):
        assert flag[i] == p.flag, (tag, i, p.family, int(flag[i]), p.flag)
        if p.flag == Q.FLAG_OK:
            e = p.err(U[:, i])
            worst[p.family] = max(worst.get(p.family, 0.0), e)
            assert e <= Q.U_TOL, (tag, i, p.family, e)
            if its is not None:
                assert its[i] >= p.min_iters, (tag, i, p.family, int(its[i]), p.min_iters)
        else:
            assert np.all(U[:, i] == 0.0), (tag, i, p.family, U[:, i])
        if its is not None:
            assert 0 <= its[i] <= 10 * (p.N + p.m) + 50, (tag, i, p.family, int(its[i]))
    print(f"{tag}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    return worst


@pytest.mark.parametrize("N", Q.HORIZONS_GPU)
def test_every_family_at_edge_horizons(ctl, N):
    ps = Q.family_batch(N)
    U, flag, its = _solve(ctl, ps)
    _check(ps, U, flag, its, tag=f"k_qp N={N} m={ps[0].m} B={len(ps)}")


@pytest.mark.parametrize("N", [16, 33, 50, 64])
def test_most_rows_at_the_lds_edge(ctl, N):
    """m = 8N + 4, the most rows ntm_qp_device takes: four scenarios per wave with
    more than 64 KiB of dynamic LDS at N = 16, ~159.4 KB of the 160 KiB at
    N = 64.  NtmMpc.quadprog raises unless the call returns NTM_OK."""
    ps = Q.batch(N, draws=5, nzero=0, families=("bigm",), first_draw=10)
    assert {p.m for p in ps} == {8 * N + 4}
    U, flag, its = _solve(ctl, ps)
    _check(ps, U, flag, its, tag=f"k_qp bigm N={N}")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


@pytest.mark.parametrize("N", [8, 16, 17])
def test_mixed_fates_in_one_wave(ctl, N):
    """Four scenarios share a wave of k_qp<16> (N = 8, 16; one per wave at N = 17,
    for contrast) and end differently; every group collective has to stay inside
    its 16 lanes.  Reordering the batch changes who shares a wave: each
    scenario's U, flag and iteration count must not change by a bit
    (include/ntm_mpc.h: results do not depend on the batch around a scenario)."""
    ps = Q.mixed_fates(N)
    B = len(ps)
    for g in range(B // 4):
        assert {p.flag for p in ps[4 * g:4 * g + 4]} == {1, -2, -7}
    U, flag, its = _solve(ctl, ps)
    _check(ps, U, flag, its, tag=f"k_qp mixed fates N={N}")
    for name, order in (("reversed", list(range(B))[::-1]), ("rotated", [(i + 1) % B for i in range(B)])):
        U2, flag2, its2 = _solve(ctl, [ps[j] for j in order])
        for pos, j in enumerate(order):
            assert flag2[pos] == flag[j] and its2[pos] == its[j], (name, j, ps[j].family)
            assert np.array_equal(_bits(U2[:, pos]), _bits(U[:, j])), (name, j, ps[j].family)


@pytest.mark.parametrize("N", [3, 16, 20])
def test_hessian_not_positive_definite(ctl, N):
    """G zero, diag(1, -1, 1, ...) or singular PSD: flag -7 and U = 0, as both
    oracles return; the feasible neighbours in the same wave stay exact."""
    ps = Q.bad_hessians(N)
    assert [p.flag for p in ps] == [1, -7, 1, -7, -7, 1, 1]
    U, flag, its = _solve(ctl, ps)
    _check(ps, U, flag, its, tag=f"k_qp bad G N={N}")


@pytest.mark.parametrize("N", [3, 16, 20, 33, 50])
def test_mixed_precision_entry_point(ctl, N):
    """ntm_qp_mixed_device on the batches of test_every_family_at_edge_horizons:
    the fp64 result meets the same flags and bound whether the fp32 stage's
    (possibly different, degenerate) active set certified or fp64 fell back;
    exactly one of info bit 0 (certified) / bit 1 (fallback) is set on every
    optimal scenario, bit 2 (fp32 not optimal) implies bit 1; U32 is finite.

    Recorded on an MI355X: 0 of the 21 feasible scenarios took the fallback at
    every N, and the fp32 stage was optimal on all of them (worst U32 error
    5e-7 at N = 3 to 5e-6 at N = 50): the data are small integers, exact in
    fp32 too, so the fp32 stage meets the same problem.  Not asserted; the
    fallback paths themselves are test_mixed_precision_falls_back_beyond_fp32.
    """
    ps = Q.family_batch(N)
    U, U32, flag, info, _ = _solve(ctl, ps, mixed=True)
    _check(ps, U, flag, tag=f"k_qp_mixed N={N}")
    ok = np.array([p.flag == Q.FLAG_OK for p in ps])
    assert np.all(((info[ok] & 1) != 0) ^ ((info[ok] & 2) != 0)), info[ok]
    assert np.all(((info & 4) == 0) | ((info & 2) != 0)), info
    assert np.all(np.isfinite(U32[:, ok]))
    e32 = max(p.err(U32[:, i]) for i, p in enumerate(ps) if p.flag == Q.FLAG_OK)
    print(f"k_qp_mixed N={N}: fallback {int(np.sum((info[ok] & 2) != 0))} of {int(ok.sum())}, "
          f"fp32 not optimal {int(np.sum((info[ok] & 4) != 0))}, worst fp32 error {e32:.1e}")


@pytest.mark.parametrize("N", [3, 16, 20, 33])
def test_mixed_precision_falls_back_beyond_fp32(ctl, N):
    """Problems the fp32 stage cannot see (qp_planted.beyond_fp32): G overflows
    fp32 (stage non-finite: info bits 1 and 2) or the active rows round to zero
    (stage optimal on another problem, its set does not certify: bit 1 alone).
    The fp64 fallback must return the planted optimum, U32 must be defined
    (finite) all the same, and the plain neighbour certifies (bit 0).  k_qp
    takes the same batch: power-of-two scalings change nothing in fp64."""
    ps = Q.beyond_fp32(N)
    U, flag, its = _solve(ctl, ps)
    _check(ps, U, flag, its, tag=f"k_qp beyond fp32 N={N}")
    U, U32, flag, info, _ = _solve(ctl, ps, mixed=True)
    _check(ps, U, flag, tag=f"k_qp_mixed beyond fp32 N={N}")
    print(f"k_qp_mixed beyond fp32 N={N}: info {info.tolist()}")
    assert info.tolist() == [6, 2, 1, 6, 2], info
    assert np.all(np.isfinite(U32)), U32


def test_mixed_precision_lds_limit(ctl):
    """N = 64, m = 516: the fp64 workspace (~159 KB) and the fp32 one
    (GI32::bytes, ~55 KB) do not fit 160 KiB together: NTM_E_UNSUPPORTED with a
    message, nothing launched, and the context goes on working.  N = 50,
    m = 8N + 2 (config 5's shape, ~136 KB) fits."""
    ps = Q.batch(64, draws=3, nzero=0, families=("bigm",))
    N, m, B = 64, 516, len(ps)
    G, F, Lin, b = (ctl.tensor(a) for a in Q.pack(ps))
    U, U32 = ctl.tensor(np.full((N, B), 7.0)), ctl.tensor(np.full((N, B), 7.0))
    fl, info, it = (torch.full((B,), 99, dtype=torch.int32, device=U.device) for _ in range(3))
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    rc = ctl.lib.ntm_qp_mixed_device(ctl._ctx, B, N, m, p(G), p(F), p(Lin), p(b), p(U), p(U32), p(fl), p(info),
                                     p(it), None)
    torch.cuda.synchronize()
    assert rc == NTM_E_UNSUPPORTED, rc
    assert len(ctl.lib.ntm_last_error(ctl._ctx)) > 0
    assert torch.all(U == 7.0) and torch.all(fl == 99)          # outputs untouched
    # the same problems through the fp64 entry point, which takes this shape
    Uq, flag, its = _solve(ctl, ps)
    _check(ps, Uq, flag, its, tag="k_qp after the refused mixed call")
    ps50 = Q.batch(50, draws=3, nzero=2, families=("bigm", "vertex_dup", "weak"), m=8 * 50 + 2)
    Um, U32m, flagm, infom, _ = _solve(ctl, ps50, mixed=True)
    _check(ps50, Um, flagm, tag="k_qp_mixed N=50 m=402")
    assert np.all(np.isfinite(U32m))
