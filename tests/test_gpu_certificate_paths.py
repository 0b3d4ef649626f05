"""The certified re-solve's predicate collectives and exact-division shortcuts
(polish_compact in csrc/ntm_device.h, gany / gall / gargmin in csrc/ntm_collectives.h): the
stand-alone collectives check, the drop
position of a dual-infeasible candidate against the NumPy oracle's multipliers, a
candidate set holding a single-entry state row (the one case that still takes
the IEEE division for a fixed variable's multiplier), and the rejected
candidates, whose exit flags and fallback results must stay what
test_gpu_parity.py documents.

Tolerance: max |U_gpu - U_oracle| / umax <= 1e-10, the step tests' bound
(test_gpu_parity.py).
"""

import numpy as np
import pytest
import torch

from checkprog import build_and_run
from oracle import cbind
from oracle import ntm_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U_TOL = 1e-10


def T(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def H(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def cfgs(N, mode):
    from ntm_mpc import Config
    return Config(N=N, mode=mode), O.Config(N=N, mode=mode)


def test_collectives_check(tmp_path):
    """tools/collectives_check.hip: gany / gall and the payload-free gargmin against
    the DPP forms, P = 16, 32 and 64, one PASS line."""
    build_and_run("collectives_check", tmp_path, "-O2")


def _workspace(N, B, sets):
    ws = np.full((2 * (N + 1), B), -1, dtype=np.int32)
    for s, rows in enumerate(sets):
        ws[:len(rows), s] = rows
        ws[N, s] = len(rows)
    return torch.tensor(ws, dtype=torch.int32, device=DEV)


# (N, small_batch): the far N = 20 build forced at a small batch, the all-LDS one a
# small batch takes by default, and the N = 50 build
BUILDS = [(20, 0), (20, -1), (50, -1)]


@pytest.mark.parametrize("N,small_batch", [(20, 0), (10, -1)])
def test_single_entry_state_row_candidate(ctl, N, small_batch):
    """Scenario 0's candidate holds the w row of x_1 (one non-zero: it fixes u_0 with
    |hv| != 1, so the multiplier takes the division) next to input-bound rows;
    scenario 1's holds bound rows only (the +-res shortcut).  At N = 10 both sit in
    one wave.  Either way the step returns the oracle's optimum."""
    B = 2
    cfg, ocfg = cfgs(N, 2)
    x = O.scenario_x0(np.arange(B)).T
    rho, Uo = cbind.initial_state(x, ocfg)
    ref = cbind.step(x, rho, Uo, ocfg)
    bounds = [6 * j + 1 for j in range(1, min(N, 8))]
    ws = _workspace(N, B, [bounds + [10], bounds])          # id 10: w_1 <= w_max
    ctl.set_small_batch(small_batch)
    try:
        out = ctl.step(T(x), T(rho), T(Uo), cfg, active_ws=ws)
        U, fl = H(out["U"]), H(out["exitflag"])
    finally:
        ctl.set_small_batch(-1)
    err = np.max(np.abs(U - ref["U"])) / cfg.umax
    print(f"N={N} small_batch={small_batch}: flags {fl}, max |U - U_oracle| / umax = {err:.3e}")
    np.testing.assert_array_equal(fl, ref["exitflag"])
    assert err <= U_TOL


@pytest.mark.parametrize("N,small_batch", BUILDS)
def test_rejected_candidates_unchanged(ctl, N, small_batch):
    """Two rows fixing one variable, a set holding a constant row, and a non-finite
    x_k: the first two candidates are rejected (same flags and optimum as with no
    workspace, and the oracle's optimum), the third scenario leaves with -7."""
    B = 3
    cfg, ocfg = cfgs(N, 2)
    x = O.scenario_x0(np.arange(B)).T.copy()
    x[1, 2] = np.nan
    rho, Uo = cbind.initial_state(x, ocfg)
    ref = cbind.step(x[:, :2].copy(), rho[:, :2].copy(), Uo[:, :2].copy(), ocfg)
    bounds = [6 * j + 1 for j in range(1, 8)]
    ws = _workspace(N, B, [bounds + [6 * 3],                 # u_3 at both of its bounds
                           bounds + [2],                      # an x_0 row: constant
                           bounds])
    ctl.set_small_batch(small_batch)
    try:
        plain = ctl.step(T(x), T(rho), T(Uo), cfg)
        Up, fp = H(plain["U"]), H(plain["exitflag"])
        out = ctl.step(T(x), T(rho), T(Uo), cfg, active_ws=ws)
        U, fl = H(out["U"]), H(out["exitflag"])
    finally:
        ctl.set_small_batch(-1)
    err = np.max(np.abs(U[:, :2] - ref["U"])) / cfg.umax
    print(f"N={N} small_batch={small_batch}: flags {fl} (no workspace {fp}), max |U - U_oracle| / umax = {err:.3e}")
    np.testing.assert_array_equal(fl, [1, 1, -7])
    np.testing.assert_array_equal(fl, fp)
    np.testing.assert_array_equal(fl[:2], ref["exitflag"])
    assert np.max(np.abs(U[:, :2] - Up[:, :2])) <= U_TOL * cfg.umax
    assert err <= U_TOL


# ---------------------------------------------------------------- drop position
# Scenario ids (ntm_scenarios_x0 / O.scenario_x0) whose first QP (i_sim = 1, rho of
# x_0) certifies a set with room for three more rows: found on the CPU with the NumPy
# oracle among ids 0..599 (most first QPs hold N rows).  The added rows are drawn on
# the CPU from the oracle's own set with a fixed seed.
DROP_IDS = {20: [18, 31, 52, 89, 93, 94, 100, 136, 162, 182, 192, 200, 246, 262, 300, 343, 412, 437, 456, 463, 497,
                 505, 510, 516],
            10: [52, 100, 246, 300, 437, 522, 563]}
DROP_SEED = 20241220
ARGMIN_GAP = 1e-6


def _scaled_qp(x0, ocfg):
    """The first QP of a step from rho(x_0), scaled as qp_solve scales it."""
    ph = O.Physics()
    Phi, Gam, Lam = O.lift(O.initial_rho(x0, ph, ocfg), ph, ocfg)
    G, F = O.cost(Phi, Gam, Lam, x0, ocfg)
    Lin, b = O.constraints(Phi, Gam, Lam, x0, ocfg)
    Dv = O.jacobi_scale(G)
    Ls = Lin * Dv[None, :]
    rn = np.linalg.norm(Ls, axis=1)
    rn = np.where(rn > 0.0, rn, 1.0)
    return dict(G=G, F=F, Lin=Lin, b=b, Dv=Dv, Gs=G * Dv[:, None] * Dv[None, :], Ns=-(Ls / rn[:, None]),
                bcs=-(b / rn), Fs=F * Dv)


def _multipliers(q, act, monkeypatch):
    """polish_active_set on `act`: ({row id: multiplier}, certified), the multipliers
    formed as _polish_certify forms them from the re-solve it is handed."""
    cap = {}
    orig = O._polish_certify

    def spy(Gs, Fs, Ns, bcs, act_, Lin, Dv, S, fixed, Ufix, V, mu):
        cap.update(S=list(S), V=V, mu=np.asarray(mu, dtype=float))
        return orig(Gs, Fs, Ns, bcs, act_, Lin, Dv, S, fixed, Ufix, V, mu)

    with monkeypatch.context() as m:
        m.setattr(O, "_polish_certify", spy)
        _, _, ok = O.polish_active_set(q["Gs"], q["Fs"], q["Ns"], q["bcs"], list(act), q["Lin"], q["b"], q["Dv"])
    if not cap:
        return None, False
    S, mu, V = cap["S"], cap["mu"], cap["V"]
    res = q["Gs"] @ V + q["Fs"] - (q["Ns"][S].T @ mu if S else 0.0)
    mult = {}
    for a in act:
        if a in S:
            mult[a] = mu[S.index(a)]
        else:
            j = np.flatnonzero(q["Lin"][a])[0]
            mult[a] = res[j] / q["Ns"][a, j]
    return mult, ok


def _predict_drops(q, cand, monkeypatch):
    """Drop the most negative multiplier until the set is dual feasible.  Returns the
    number of drops, or None if an argmin is decided by a relative gap < ARGMIN_GAP
    or the sequence does not end in a set the oracle certifies."""
    act, drops = list(cand), 0
    while True:
        mult, ok = _multipliers(q, act, monkeypatch)
        if mult is None:
            return None
        v = np.array([mult[a] for a in act])
        if not np.all(np.isfinite(v)):
            return None
        if not v.min() < -O.POLISH_DUAL_TOL * max(1.0, np.max(np.abs(v))):
            return drops if ok else None
        o = np.argsort(v)
        if len(v) > 1 and v[o[1]] - v[o[0]] < ARGMIN_GAP * max(abs(v[o[0]]), abs(v[o[1]])):
            return None
        act.pop(int(o[0]))
        drops += 1


@pytest.mark.parametrize("N,small_batch", [(20, 0), (10, -1)])
def test_drop_position_against_oracle(ctl, monkeypatch, N, small_batch):
    """A certified set plus k in {1, 2, 3} inactive input-bound rows, in slot 0: the
    kernel must drop exactly the rows the oracle's multipliers name (most negative
    first), one verification per drop plus the certifying one (stats row 4), and end
    on the first step's U bit for bit.  N = 20: the far build, B = 24.  N = 10: four
    scenarios per wave, B = 7, so the last wave is ragged and its groups drop
    different numbers of rows."""
    from ntm_mpc import Config
    ids = np.array(DROP_IDS[N])
    B = len(ids)
    cfg, ocfg = Config(N=N, mode=2, i_sim=1), O.Config(N=N, mode=2, i_sim=1)
    X = O.scenario_x0(ids)
    x = X.T
    rho, Uo = cbind.initial_state(x, ocfg)
    # CPU: each scenario's QP, the oracle's set, the added rows (fixed by seed)
    rng = np.random.default_rng(DROP_SEED + N)
    qps, adds = [], []
    for s in range(B):
        q = _scaled_qp(X[s], ocfg)
        _, flag, info = O.qp_solve(q["G"], q["F"], q["Lin"], q["b"])
        assert flag == 1
        fixedv = {int(np.flatnonzero(q["Lin"][a])[0]) for a in info["active"] if np.count_nonzero(q["Lin"][a]) == 1}
        freev = [j for j in range(N) if j not in fixedv]
        js = rng.choice(freev, size=1 + s % 3, replace=False)
        qps.append(q)
        adds.append([int(6 * j + rng.integers(0, 2)) for j in js])       # u_j >= umin or u_j <= umax
    ctl.set_small_batch(small_batch)
    try:
        ws = ctl.new_active_ws(B, cfg)
        first = ctl.step(T(x), T(rho), T(Uo), cfg, active_ws=ws)
        U1, f1, ws1 = H(first["U"]), H(first["exitflag"]), H(ws)
        cands = []
        for s in range(B):
            n = int(ws1[N, s])
            assert 0 <= n <= N - 3, f"scenario {ids[s]}: first step left {n} rows in slot 0"
            cands.append([int(a) for a in ws1[:n, s]] + adds[s])
        stats = torch.zeros((6, B), dtype=torch.int32, device=DEV)
        ctl.set_stats(stats)
        try:
            second = ctl.step(T(x), T(rho), T(Uo), cfg, active_ws=_workspace(N, B, cands))
            U2, f2, st = H(second["U"]), H(second["exitflag"]), H(stats)
        finally:
            ctl.set_stats(None)
    finally:
        ctl.set_small_batch(-1)
    np.testing.assert_array_equal(f1, np.ones(B, dtype=f1.dtype))
    kept = 0
    for s in range(B):
        clash = len(set(cands[s])) != len(cands[s])
        drops = None if clash else _predict_drops(qps[s], cands[s], monkeypatch)
        print(f"N={N} id {ids[s]}: set {len(cands[s]) - len(adds[s])} rows + {adds[s]}: predicted drops {drops}, "
              f"verifications {st[4, s]}, flag {f2[s]}, U bitwise {np.array_equal(U1[:, s], U2[:, s])}")
        if drops is None:
            continue
        kept += 1
        assert f2[s] == 1
        assert np.array_equal(U1[:, s], U2[:, s]), f"scenario {ids[s]}: U differs from the first step's"
        assert st[4, s] == drops + 1, f"scenario {ids[s]}: {st[4, s]} verifications, predicted {drops + 1}"
    print(f"N={N}: {kept} of {B} crafted cases kept")
    assert kept >= 0.75 * B
