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

Families that make Goldfarb-Idnani take rows back (``DROP_FAMILIES``;
``make_drop(family, N, draw)``, N >= 2; none of the twelve above ever drops a row
or meets a dependent one on its way to flag 1):

    drop        plain with lam in [20, 40] (the unconstrained minimiser lies far
                from U*) + 2N+3 near rows with slack 1 or 2 at U*: many are
                violated on the way, added and dropped again.  Kept only if the
                counting copy of the oracle's loop (``gi_counted``) ends with
                flag 1 after >= 2 drops
    dropdep     drop + three pairs L_A[j] + c, -c with slack 1 each, whose sum is
                an active row: with both in the set that row is dependent (a
                dual-only step and a drop).  Kept only if flag 1 after >= 1
                dependent event and >= 1 drop

Both criteria are asked of two paths: the problem as stated (the NumPy oracle's)
and its Jacobi-scaled form (``jacobi_scaled``: the units in which the C oracle
and the device pick the most violated row).

This is a plain helper module (no fixtures, no tests).
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np

from oracle import ntm_oracle as O

U_TOL = 1e-10           # the project's QP bound (tests/test_gpu_parity.py)
FLAG_OK, FLAG_INFEASIBLE, FLAG_NONFINITE = 1, -2, -7

FEASIBLE = ("plain", "dup", "weak", "eq", "dep", "vertex", "vertex_dup", "rowscale", "gscale", "bigm")
INFEASIBLE = ("infeas2", "infeas3")
FAMILIES = FEASIBLE + INFEASIBLE
# Feasible too, but kept out of FAMILIES: batch(), family_batch() and every seed of
# the twelve above (seed_of's family index) stay what they were.
DROP_FAMILIES = ("drop", "dropdep")
_SEED_ORDER = FAMILIES + DROP_FAMILIES

HORIZONS_CPU = (1, 2, 3, 8, 16, 17, 32, 33, 64)
HORIZONS_GPU = (1, 2, 3, 8, 15, 16, 17, 20, 32, 33, 50, 64)


def families_for(N: int, drops: bool = False):
    """Every family that exists at horizon N (infeas3 needs two variables);
    ``drops``: the drop families as well (N >= 2: at N = 1 the most violated row is
    the final one, nothing is ever dropped)."""
    fams = tuple(f for f in FAMILIES if not (f == "infeas3" and N < 2))
    return fams + (DROP_FAMILIES if drops and N >= 2 else ())


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
    path: dict = field(default=None, repr=False)       # drop families: gi_counted's adds, drops, deps

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
    return 1000003 * _SEED_ORDER.index(family) + 1009 * N + draw


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


# ---- problems on which Goldfarb-Idnani drops rows and meets dependent ones

def gi_counted(G, F, Lin, b):
    """O.qp_dual_active_set's loop, statement for statement, with three counters.
    Returns (U, flag, active rows, multipliers, iterations, counts) with counts =
    {"adds", "drops", "deps", "deep"}: full steps that add the picked row, rows taken
    out (after a partial step or a dual-only one), dual-only steps (the picked row
    depends on the active ones: t2 = inf), and drops from position l of q active
    rows with q - l >= 3 (two or more Givens rotations: only then does a rotated
    column other than the discarded last one stay behind, which needs N >= 3 and
    at N = 3 a full set).  iterations = adds + drops and
    adds - drops = len(active) whenever it returns; make_drop holds it to the
    oracle's own result on every problem it accepts."""
    n, m = G.shape[0], Lin.shape[0]
    max_iter = 10 * (n + m) + 50
    cnt = {"adds": 0, "drops": 0, "deps": 0, "deep": 0}
    assert np.all(np.isfinite(G)) and np.all(np.isfinite(F)) and np.all(np.isfinite(Lin)) and np.all(np.isfinite(b))
    Nc, bc = -Lin, -b
    nonzero = np.any(Nc != 0.0, axis=1)
    if np.any((~nonzero) & (bc > O.CONST_ROW_TOL)):
        return np.zeros(n), O.EXIT_INFEASIBLE, [], np.zeros(0), 0, cnt
    nrm = np.linalg.norm(Nc, axis=1)
    J = np.linalg.inv(np.linalg.cholesky(G)).T
    U = -(J @ (J.T @ F))
    R = np.zeros((n, n))
    act: list[int] = []
    u = np.zeros(0)
    it = 0
    while True:
        s = Nc @ U - bc
        viol = np.where(nonzero, s / np.where(nrm > 0, nrm, 1.0), np.inf)
        if act:
            viol[act] = np.inf
        p = int(np.argmin(viol))
        if viol[p] == np.inf or s[p] >= -1e-12 * max(nrm[p] * np.max(np.abs(U), initial=1.0), abs(bc[p])):
            return U, O.EXIT_OK, act, u, it, cnt
        up = np.append(u, 0.0)
        while True:
            it += 1
            if it > max_iter:
                return U, O.EXIT_MAXIT, act, up[:len(act)], it, cnt
            q = len(act)
            d = J.T @ Nc[p]
            z = J[:, q:] @ d[q:]
            r = np.linalg.solve(np.triu(R[:q, :q]), d[:q]) if q else np.zeros(0)
            t1, l = math.inf, -1
            for j in range(q):
                if r[j] > 0.0:
                    tj = up[j] / r[j]
                    if tj < t1:
                        t1, l = tj, j
            zn = float(d[q:] @ d[q:])
            sp = float(Nc[p] @ U - bc[p])
            t2 = math.inf if zn <= 1e-300 or math.sqrt(zn) <= O.GI_DEP_TOL * np.linalg.norm(d) else -sp / zn
            t = min(t1, t2)
            if t == math.inf:
                return np.zeros(n), O.EXIT_INFEASIBLE, act, up[:q], it, cnt
            if t2 == math.inf:
                cnt["deps"] += 1
                cnt["drops"] += 1
                cnt["deep"] += q - l >= 3
                up[:q] = np.maximum(0.0, up[:q] - t * r)
                up[q] += t
                J, R = O._drop(J, R, q, l)
                act.pop(l)
                up = np.delete(up, l)
                continue
            U = U + t * z
            up[:q] = np.maximum(0.0, up[:q] - t * r)
            up[q] += t
            if t == t2:
                cnt["adds"] += 1
                J, R = O._add(J, R, q, d)
                act.append(p)
                u = up
                break
            cnt["drops"] += 1
            cnt["deep"] += q - l >= 3
            J, R = O._drop(J, R, q, l)
            act.pop(l)
            up = np.delete(up, l)


N_NEAR_PAIRS = 3
DROP_SEARCH_CAP = 400


def drop_rows(N: int) -> int:
    """The most core rows a drop-family problem has: N/2 active, 2N+3 near, the pairs."""
    return max(1, N // 2) + 2 * N + 3 + 2 * N_NEAR_PAIRS


def _drop_candidate(family, N, rng, m, nzero):
    """One draw of a drop-family problem, as yet unchecked.  min_iters = k holds on
    any path; k + 2 drops is the NumPy oracle's count alone (the C oracle and the
    device pick rows in Jacobi-scaled units and solve some of these in k)."""
    A = _ints(rng, -2, 2, (N + 2, N))
    G = A.T @ A + np.eye(N)
    Us = _ints(rng, -3, 3, N)
    LA = _independent_rows(rng, int(rng.integers(1, max(1, N // 2) + 1)), N)
    k = LA.shape[0]
    lam = _ints(rng, 20, 40, k)
    F = -G @ Us - LA.T @ lam
    near = _nonzero_rows(rng, 2 * N + 3, N)
    L = np.vstack([LA, near])
    bt = np.concatenate([LA @ Us, near @ Us + _ints(rng, 1, 2, near.shape[0])])
    if family == "dropdep":
        for _ in range(N_NEAR_PAIRS):
            j = int(rng.integers(0, k))
            while True:
                c = _nonzero_rows(rng, 1, N)[0]
                if (LA[j] + c).any():
                    break
            pair = np.vstack([LA[j] + c, -c])
            L, bt = np.vstack([L, pair]), np.concatenate([bt, pair @ Us + 1.0])
    n_core = L.shape[0]
    n_in = m - n_core - nzero
    if n_in < 0:
        raise ValueError(f"{family}, N = {N}: m = {m} < {n_core} core rows + {nzero} zero rows")
    Li = _ints(rng, -3, 3, (n_in, N))
    Lin = np.vstack([L, Li, np.zeros((nzero, N))])
    b = np.concatenate([bt, Li @ Us + _ints(rng, 1, 3, n_in), np.ones(nzero)])
    perm = rng.permutation(m)
    return Planted(family, G, F, Lin[perm], b[perm], Us, FLAG_OK, np.ones(N), n_core, k, LA, LA.copy(), lam)


def jacobi_scaled(p: Planted):
    """(G, F, Lin, b) of p in the units the device and the C oracle pick rows in:
    V = U/d with d_j = 1/sqrt(G_jj), every ordinary row divided by |Lin_i o d|_2.
    The same problem, but rounded, and Goldfarb-Idnani's most violated row is
    another one: its path differs from the unscaled statement's."""
    d = 1.0 / np.sqrt(np.diag(p.G))
    Ls = p.Lin * d[None, :]
    rn = np.linalg.norm(Ls, axis=1)
    rn = np.where(rn > 0.0, rn, 1.0)
    return p.G * d[:, None] * d[None, :], p.F * d, Ls / rn[:, None], p.b / rn


def make_drop(family: str, N: int, draw: int, m: int | None = None, nzero: int = 0, min_drops: int | None = None):
    """The first candidate of (family, N, draw) that gi_counted solves with flag 1
    on the path the family is about: ``min_drops`` drops (default 2 for drop, 1 for
    dropdep) and, for dropdep, one dependent event; both as stated (the NumPy
    oracle's path, exact data) and Jacobi-scaled (the path of the device's
    units: at N = 2 the two have little in common).  Candidate c is drawn from the
    seed (seed_of(family, N, draw), c), c < DROP_SEARCH_CAP; the whole problem,
    filler rows and permutation included, is what is tried, since the filler rows
    have small slack too and steer the path.  Running out of candidates raises."""
    if family not in DROP_FAMILIES:
        raise ValueError(family)
    if N < 2:
        raise ValueError("the drop families need N >= 2")
    if m is None:
        m = drop_rows(N) + 3 + nzero
    if min_drops is None:
        min_drops = 2 if family == "drop" else 1
    def meets(flag, cnt):
        return flag == FLAG_OK and cnt["drops"] >= min_drops and (family != "dropdep" or cnt["deps"] >= 1)

    for c in range(DROP_SEARCH_CAP):
        p = _drop_candidate(family, N, np.random.default_rng([seed_of(family, N, draw), c]), m, nzero)
        U, flag, act, u, it, cnt = gi_counted(p.G, p.F, p.Lin, p.b)
        if not meets(flag, cnt):
            continue
        _, flags, _, _, _, cnts = gi_counted(*jacobi_scaled(p))
        if not meets(flags, cnts):
            continue
        Uo, fo, acto, uo, ito = O.qp_dual_active_set(p.G, p.F, p.Lin, p.b)
        assert fo == flag and ito == it and list(acto) == list(act), (family, N, draw, c)
        assert np.array_equal(Uo, U) and np.array_equal(uo, u), (family, N, draw, c)
        assert it == cnt["adds"] + cnt["drops"] and cnt["adds"] - cnt["drops"] == len(act), (family, N, draw, c, cnt)
        p.path = dict(cnt, candidate=c, iterations=it, scaled_drops=cnts["drops"], scaled_deps=cnts["deps"],
                      scaled_deep=cnts["deep"])
        return p
    raise RuntimeError(f"{family}, N = {N}, draw {draw}: no accepted problem in {DROP_SEARCH_CAP} candidates")


@functools.lru_cache(maxsize=None)
def _drop_batch(N: int):
    m = drop_rows(N) + 3 + 2
    ps = []
    for d in range(4):
        ps += [make_drop("drop", N, d, m=m, nzero=2), make_drop("dropdep", N, d, m=m, nzero=2)]
    ps.insert(4, make("plain", N, np.random.default_rng(seed_of("plain", N, 3)), m=m, nzero=2))
    assert len(ps) % 4 != 0 and {p.m for p in ps} == {m} and m <= 8 * N + 4
    return tuple(ps)


def drop_batch(N: int):
    """Four drop and four dropdep problems, alternating, with one plain neighbour in
    the middle: B = 9 (not a multiple of the four scenarios a wave of k_qp holds at
    N <= 16, and every wave mixes long and short add/drop sequences), common
    m = drop_rows(N) + 5, two all-zero rows with b = 1 in every scenario.  Built
    once per horizon; the problems are shared, leave them unchanged."""
    return list(_drop_batch(N))


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
