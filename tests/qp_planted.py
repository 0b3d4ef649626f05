"""QPs built backwards from their answer, in small integers.

    min 1/2 U'GU + F'U   s.t.  Lin U <= b

Every problem here is made from its optimum: G = A'A + I with integer A, an
integer U*, integer rows tight at U* with integer multipliers lam >= 0, integer
rows with integer slack, and F = -G U* - L_A' lam.  G is SPD, so the KKT
conditions are sufficient and U* is the unique primal optimum however
degenerate the multipliers are; every number (and every power-of-two scaling
of it) is exact in fp64, so nothing is solved to obtain the reference.

Families (``FAMILIES``; ``make(family, N, rng)``):

    plain       k in [1, N/2] independent active rows, lam in {1, 2, 3}
    dup         plain + an exact copy and a 4x copy of every active row (lam = 0)
    weak        plain + N+2 more tight rows with lam = 0 (more than N rows tight)
    eq          plain + the negative of every active row (each pair an equality)
    dep         plain with k >= 2 + the row L_A[0] + L_A[1], lam = 2
                (N = 1: k = 1 and the row L_A[0] + L_A[0])
    vertex      k = N rows of diag(+-3) + tridiag{-1, 0, 1}, row-permuted, lam > 0
    vertex_dup  vertex + 2x copies of half of its rows (rounded up), lam = 1
    rowscale    plain, each active row and its b times 2^e, e in [-20, 20]
    gscale      plain, then G <- SGS, F <- SF, Lin <- Lin S, U* <- U*/S with
                S = diag(2^e), e in [-12, 12]; errors are measured in the scaled
                units (``Planted.s``)
    bigm        k in [1, N] rows of vertex's matrix, inactive rows up to m = 8N+4
    infeas2     plain + r.U <= -1 and -r.U <= -1                  -> flag -2
    infeas3     plain + U_0 <= 0, U_1 <= 0, -U_0 - U_1 <= -1      -> flag -2 (N >= 2)

This is a plain helper module (no fixtures, no tests).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

U_TOL = 1e-10           # the project's QP bound (tests/test_gpu_parity.py)
FLAG_OK, FLAG_INFEASIBLE, FLAG_NONFINITE = 1, -2, -7

FEASIBLE = ("plain", "dup", "weak", "eq", "dep", "vertex", "vertex_dup", "rowscale", "gscale", "bigm")
INFEASIBLE = ("infeas2", "infeas3")
FAMILIES = FEASIBLE + INFEASIBLE

HORIZONS_CPU = (1, 2, 3, 8, 16, 17, 32, 33, 64)
HORIZONS_GPU = (1, 2, 3, 8, 15, 16, 17, 20, 32, 33, 50, 64)


def families_for(N: int):
    """Every family that exists at horizon N (infeas3 needs two variables)."""
    return tuple(f for f in FAMILIES if not (f == "infeas3" and N < 2))


@dataclass
class Planted:
    family: str
    G: np.ndarray            # (N, N)
    F: np.ndarray            # (N,)
    Lin: np.ndarray          # (m, N)
    b: np.ndarray            # (m,)
    Ustar: np.ndarray        # (N,) the planted optimum (zeros where flag != 1: D16)
    flag: int                # expected exit flag
    s: np.ndarray            # (N,) units of the error: max |(U - U*) s|
    n_core: int              # rows that are not inactive filler (tight, conflicting)
    min_iters: int           # active rows with lam > 0 (plain and vertex; else 0)
    LA: np.ndarray = field(default=None, repr=False)   # the rows with lam > 0 as drawn (unscaled)
    Lt: np.ndarray = field(default=None, repr=False)   # every row planted tight at U*, in the final units
    lam: np.ndarray = field(default=None, repr=False)  # their multipliers (>= 0)

    @property
    def N(self):
        return self.G.shape[0]

    @property
    def m(self):
        return self.Lin.shape[0]

    def err(self, U) -> float:
        """max |(U - U*) s| / max(1, max |U* s|): the quantity U_TOL bounds."""
        return float(np.max(np.abs((np.asarray(U) - self.Ustar) * self.s))
                     / max(1.0, float(np.max(np.abs(self.Ustar * self.s)))))


def _ints(rng, lo, hi, size):
    return rng.integers(lo, hi + 1, size=size).astype(np.float64)


def _nonzero_rows(rng, n, N):
    L = _ints(rng, -3, 3, (n, N))
    for i in range(n):
        while not L[i].any():
            L[i] = _ints(rng, -3, 3, N)
    return L


def _independent_rows(rng, k, N):
    while True:
        L = _nonzero_rows(rng, k, N)
        if np.linalg.matrix_rank(L) == k:
            return L


def vertex_matrix(rng, N):
    """diag(+-3) + a tridiagonal of {-1, 0, 1}: strictly diagonally dominant, so
    the N rows are independent and well conditioned (cond < 3.5 measured);
    rows permuted."""
    M = np.diag(rng.choice([-3.0, 3.0], size=N))
    if N > 1:
        M += np.diag(_ints(rng, -1, 1, N - 1), 1) + np.diag(_ints(rng, -1, 1, N - 1), -1)
    return M[rng.permutation(N)]


def make(family: str, N: int, rng, m: int | None = None, nzero: int = 0, k: int | None = None,
         rexp: int | None = None, gexp: int | None = None) -> Planted:
    """One planted QP.  ``m``: total rows (filled with inactive rows; default the
    core rows + N + 3, bigm: 8N + 4); ``nzero`` of them are all-zero rows with
    b = 1 (legal constant rows); ``k``: the number of active rows of a plain
    problem instead of a drawn one (0: inactive rows only); ``rexp``: rowscale
    with every active row times 2^-rexp; ``gexp``: gscale with S_j = 2^+-gexp and
    S_0 = 2^gexp (see beyond_fp32)."""
    if family not in FAMILIES:
        raise ValueError(family)
    if family == "infeas3" and N < 2:
        raise ValueError("infeas3 needs N >= 2")
    A = _ints(rng, -2, 2, (N + 2, N))
    G = A.T @ A + np.eye(N)
    Us = _ints(rng, -3, 3, N)
    s = np.ones(N)

    # ---- rows tight at U* (L, lam), b = L U*
    if family in ("vertex", "vertex_dup"):
        LA = vertex_matrix(rng, N)
    elif family == "bigm":
        LA = vertex_matrix(rng, N)[:int(rng.integers(1, N + 1))]
    elif k is not None:
        if family != "plain" or not 0 <= k <= N:
            raise ValueError("k is for plain problems, 0 <= k <= N")
        LA = _independent_rows(rng, k, N) if k else np.zeros((0, N))
    else:
        kmin = 2 if (family == "dep" and N >= 2) else 1
        LA = _independent_rows(rng, int(rng.integers(kmin, max(kmin, N // 2) + 1)), N)
    k = LA.shape[0]
    lamA = _ints(rng, 1, 3, k)
    L, lam = LA.copy(), lamA.copy()
    if family == "dup":
        L = np.vstack([L, LA, 4.0 * LA])
        lam = np.concatenate([lam, np.zeros(2 * k)])
    elif family == "weak":
        L = np.vstack([L, _nonzero_rows(rng, N + 2, N)])
        lam = np.concatenate([lam, np.zeros(N + 2)])
    elif family == "eq":
        L = np.vstack([L, -LA])
        lam = np.concatenate([lam, np.zeros(k)])
    elif family == "dep":
        L = np.vstack([L, LA[0] + LA[min(1, k - 1)]])
        lam = np.concatenate([lam, [2.0]])
    elif family == "vertex_dup":
        h = (N + 1) // 2
        L = np.vstack([L, 2.0 * LA[:h]])
        lam = np.concatenate([lam, np.ones(h)])
    bt = L @ Us
    F = -G @ Us - L.T @ lam
    if family == "rowscale":
        # the multiplier scales by 1/sc: F is unchanged
        sc = 2.0 ** (_ints(rng, -20, 20, k) if rexp is None else np.full(k, -float(rexp)))
        L, bt, lam = L * sc[:, None], bt * sc, lam / sc
    Lt = L.copy()
    flag = FLAG_OK
    # ---- conflicting rows (nothing planted: the expected answer is flag -2, U = 0)
    if family == "infeas2":
        r = _nonzero_rows(rng, 1, N)[0]
        L, bt = np.vstack([L, r, -r]), np.concatenate([bt, [-1.0, -1.0]])
        flag = FLAG_INFEASIBLE
    elif family == "infeas3":
        e = np.zeros((3, N))
        e[0, 0], e[1, 1], e[2, 0], e[2, 1] = 1.0, 1.0, -1.0, -1.0
        L, bt = np.vstack([L, e]), np.concatenate([bt, [0.0, 0.0, -1.0]])
        flag = FLAG_INFEASIBLE
    n_core = L.shape[0]
    # ---- inactive rows, constant rows, permutation
    if m is None:
        m = 8 * N + 4 if family == "bigm" else n_core + N + 3 + nzero
    n_in = m - n_core - nzero
    if n_in < 0:
        raise ValueError(f"{family}, N = {N}: m = {m} < {n_core} core rows + {nzero} zero rows")
    Li = _ints(rng, -3, 3, (n_in, N))
    bi = Li @ Us + _ints(rng, 1, 3, n_in)
    Lin = np.vstack([L, Li, np.zeros((nzero, N))])
    b = np.concatenate([bt, bi, np.ones(nzero)])
    perm = rng.permutation(m)
    Lin, b = Lin[perm], b[perm]
    if family == "gscale":
        S = 2.0 ** (_ints(rng, -12, 12, N) if gexp is None else rng.choice([-float(gexp), float(gexp)], size=N))
        if gexp is not None:
            S[0] = 2.0 ** gexp
        G, F, Lin, Us, s = G * S[:, None] * S[None, :], F * S, Lin * S[None, :], Us / S, S
        Lt = Lt * S[None, :]
    if flag != FLAG_OK:
        Us = np.zeros(N)
    return Planted(family, G, F, Lin, b, Us, flag, s, n_core,
                   k if family in ("plain", "vertex") else 0, LA, Lt, lam)


def seed_of(family: str, N: int, draw: int) -> int:
    return 1000003 * FAMILIES.index(family) + 1009 * N + draw


def batch(N: int, draws: int = 1, nzero: int = 2, families=None, m: int | None = None, first_draw: int = 0):
    """``draws`` problems of every family that exists at N, padded to a common m
    (default: the largest problem's, which is 8N + 4 when bigm is among them)
    with inactive rows and ``nzero`` constant rows each."""
    fams = families_for(N) if families is None else tuple(families)
    jobs = [(f, d) for d in range(first_draw, first_draw + draws) for f in fams]
    if m is None:
        sizes = [make(f, N, np.random.default_rng(seed_of(f, N, d))) for f, d in jobs]
        m = max(p.m if p.family == "bigm" else p.n_core + nzero + 3 for p in sizes)
    return [make(f, N, np.random.default_rng(seed_of(f, N, d)), m=m, nzero=nzero) for f, d in jobs]


def family_batch(N: int):
    """Two draws of every family plus one more problem: B = 25 (23 at N = 1), not
    a multiple of the four scenarios a wave of k_qp holds at N <= 16; common
    m = 8N + 4 (bigm's), two all-zero rows with b = 1 in every scenario."""
    ps = batch(N, draws=2, nzero=2)
    ps.append(make("plain", N, np.random.default_rng(seed_of("plain", N, 2)), m=ps[0].m, nzero=2))
    assert len(ps) % 4 != 0 and {p.m for p in ps} == {8 * N + 4}
    assert {p.family for p in ps} == set(families_for(N))
    return ps


def pack(problems):
    """(G (N*N, B), F (N, B), Lin (m*N, B), b (m, B)): column-major per scenario,
    one column per scenario (the layout NtmMpc.quadprog takes)."""
    Gb = np.stack([p.G.reshape(-1, order="F") for p in problems], axis=1)
    Lb = np.stack([p.Lin.reshape(-1, order="F") for p in problems], axis=1)
    return Gb, np.stack([p.F for p in problems], axis=1), Lb, np.stack([p.b for p in problems], axis=1)


def check_kkt(p: Planted):
    """The construction itself, exactly (every product and sum below is one of
    small integers times powers of two, so fp64 evaluates it without rounding):
    U* is feasible, the planted rows are tight, their multipliers are >= 0 and
    G U* + F + Lt' lam = 0.  Returns the number of rows tight at U*."""
    assert p.flag == FLAG_OK
    r = p.b - p.Lin @ p.Ustar
    assert np.all(r >= 0.0), r.min()
    assert np.all(p.lam >= 0.0)
    assert np.all(p.G @ p.Ustar + p.F + p.Lt.T @ p.lam == 0.0)
    tight = p.Lin[r == 0.0]
    for row in p.Lt:                                   # each planted row is among the tight ones
        assert np.any(np.all(tight == row[None, :], axis=1))
    return int(np.sum(r == 0.0))


# ---- inputs with no optimum: the non-finite contract (flag -7, U = 0)

NONFINITE_KINDS = ("nan_G", "nan_F", "nan_Lin", "nan_b", "inf_b", "neginf_Lin", "inf_G", "inf_F")
BAD_G_KINDS = ("zero_G", "indefinite_G", "singular_G")


def spoil(p: Planted, kind: str) -> Planted:
    """A copy of a feasible problem with one entry made non-finite, or with G
    replaced by a matrix that is not positive definite: zero, diag(1, -1, 1, 1,
    ...) (N >= 2), or the identity with a [[1, 1], [1, 1]] block (singular PSD,
    N >= 2).  Expected: flag -7 and U = 0."""
    G, F, Lin, b = p.G.copy(), p.F.copy(), p.Lin.copy(), p.b.copy()
    N, m = p.N, p.m
    if kind == "nan_G":
        G[N - 1, N // 2] = G[N // 2, N - 1] = np.nan
    elif kind == "inf_G":
        G[0, 0] = np.inf
    elif kind == "nan_F":
        F[N - 1] = np.nan
    elif kind == "inf_F":
        F[0] = -np.inf
    elif kind == "nan_Lin":
        Lin[m - 1, N - 1] = np.nan
    elif kind == "neginf_Lin":
        Lin[0, 0] = -np.inf
    elif kind == "nan_b":
        b[m // 2] = np.nan
    elif kind == "inf_b":
        b[m - 1] = np.inf
    elif kind == "zero_G":
        G[:] = 0.0
    elif kind == "indefinite_G":
        G = np.eye(N)
        G[1, 1] = -1.0
    elif kind == "singular_G":
        G = np.eye(N)
        G[N - 2:, N - 2:] = 1.0
    else:
        raise ValueError(kind)
    return Planted(kind, G, F, Lin, b, np.zeros(N), FLAG_NONFINITE, np.ones(N), p.n_core, 0, None)


# ---- batches whose scenarios end differently (k_qp packs four per wave at N <= 16)

def _mk(family, N, draw, **kw):
    return make(family, N, np.random.default_rng(seed_of(family, N, 100 + draw)), m=N + 6, nzero=2, **kw)


def mixed_fates(N: int):
    """14 scenarios with a common m = N + 6, ordered so that every aligned group
    of four holds all three fates (optimal after many or few adds or none,
    infeasible after one or two adds, non-finite in G, F, Lin or b)."""
    return [_mk("vertex", N, 0), spoil(_mk("plain", N, 20), "nan_G"), _mk("infeas2", N, 0), _mk("plain", N, 0, k=1),
            spoil(_mk("plain", N, 21), "nan_F"), _mk("infeas3", N, 0), _mk("plain", N, 1, k=0),
            spoil(_mk("plain", N, 22), "nan_Lin"),
            _mk("plain", N, 2, k=1), spoil(_mk("plain", N, 23), "nan_b"), _mk("infeas2", N, 1),
            spoil(_mk("plain", N, 24), "inf_b"),
            _mk("vertex", N, 1), _mk("infeas3", N, 1)]


def bad_hessians(N: int):
    """7 scenarios, m = N + 6: G zero, indefinite and singular PSD between
    feasible neighbours."""
    return [_mk("plain", N, 30), spoil(_mk("plain", N, 31), "zero_G"), _mk("plain", N, 32, k=1),
            spoil(_mk("plain", N, 33), "indefinite_G"),
            spoil(_mk("vertex", N, 34), "singular_G"), _mk("vertex", N, 35), _mk("plain", N, 36)]


def beyond_fp32(N: int):
    """5 scenarios, m = N + 6, that fp64 solves exactly as it solves their
    unscaled twins (power-of-two scalings) and fp32 cannot see: gscale with
    S_j = 2^+-70 (G_00 = int * 2^140 overflows fp32: its stage ends non-finite)
    and rowscale with every active row times 2^-160 (the rows and their b
    round to zero in fp32: its stage solves the problem without them, so its
    active set cannot certify).  Either way ntm_qp_mixed_device has to fall
    back to fp64."""
    return [_mk("gscale", N, 40, gexp=70), _mk("rowscale", N, 41, rexp=160), _mk("plain", N, 42),
            _mk("gscale", N, 43, gexp=70), _mk("rowscale", N, 44, rexp=160)]
