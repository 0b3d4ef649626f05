"""Multipliers from the fused MPC step (ntm_mpc_step_dual) and the structured KKT
audit (ntm_mpc_kkt_device).

Every check rebuilds the step's last QP on the host from the step's own outputs
``rho_qp`` and ``x_k`` with the library's cost / getWLc entries (b = c + W x_k,
rate rows appended in NumPy) and measures (U, lambda) with tests/kkt_measures.py;
the device audit rebuilds the same QP inside its kernel and must agree.  Bounds:
KKT_TOL = 1e-9, the device certificate's own tolerance, for every measure and for
the multipliers against the 50-digit ones of the fixtures (a multiplier below it
is indistinguishable from zero to the device, so a weakly active row may differ);
1e-10 umax for U.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

import kkt_measures as K
from oracle import ntm_oracle as O

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
U_TOL = 1e-10

# Structured audit against the dense NumPy measure after the largest multiplier is
# scaled by (1 + 2^-10) (both read >= 1e-6 there).  The two sides sum Gamma' Om Gamma U
# in different orders over data of condition 1e9-1e11, so the figure is measured,
# not derived: worst relative difference on an MI355X 2.63e-12 (N = 20, mode 2; 1.4e-13
# to 2.6e-12 over the shapes and modes below); the bound is 100 x that, never looser
# than 1e-3.
AGREE_MEASURED = 2.7e-12
AGREE_TOL = min(1e-3, 100 * AGREE_MEASURED)


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def host_qp(ctl, cfg, rho_qp, x):
    """The QP of (rho_qp, x_k) per scenario, from the library's own function-level
    entries: lists of G (N, N), F (N,), Lin (m, N), b (m,)."""
    N, B = cfg.N, x.shape[1]
    rq, xk = ctl.tensor(rho_qp), ctl.tensor(x)
    G, F = (_np(t) for t in ctl.cost(rq, xk, cfg))
    out = []
    if cfg.mode >= 2:
        m = 6 * N + 4
        W, L, c = (_np(t) for t in ctl.getWLc(rq, cfg))
    for s in range(B):
        if cfg.mode == 0:
            Lin, b = np.zeros((0, N)), np.zeros(0)
        elif cfg.mode == 1:
            Lin = np.vstack([-np.eye(N), np.eye(N)])
            b = np.concatenate([np.full(N, -cfg.umin), np.full(N, cfg.umax)])
        else:
            Lin = L[:, s].reshape(m, N, order="F")
            b = c[:, s] + W[:, s].reshape(m, 2, order="F") @ x[:, s]
            if cfg.mode == 3:
                Lin = np.vstack([Lin, O.rate_rows(N)])
                b = np.concatenate([b, np.full(2 * (N - 1), cfg.du_max)])
        out.append((G[:, s].reshape(N, N, order="F"), F[:, s], Lin, b))
    return out


def _T(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


@pytest.mark.parametrize("name", ["qp_ss_m2_N20", "qp_ss_m3_N50"])
def test_fixture_multipliers_through_step_dual(ctl, name):
    """The closed loop's steady-state QPs (40 per fixture) through step_dual with
    i_sim = 1 and the carried set as the workspace: flags 1, U within 1e-10 umax of
    the 50-digit optimum, rho_qp bitwise the input rho, and lambda over all rows
    against the fixture's 50-digit multipliers scattered on their active rows, in
    mu units: <= 1e-9 max(1, mumax)."""
    from ntm_mpc import Config
    d = np.load(GOLD / f"{name}.npz")
    N, mode, n = int(d["N"]), int(d["mode"]), d["x"].shape[0]
    cfg = Config(N=N, mode=mode, i_sim=1)
    ws = np.full((2 * (N + 1), n), -1, np.int32)
    ws[:N + 1] = d["cand"].T
    out = ctl.step_dual(_T(d["x"].T), _T(d["rho"].T), _T(d["U_old"].T), cfg, active_ws=_T(ws, torch.int32))
    np.testing.assert_array_equal(_np(out["exitflag"]), 1)
    U, lam, rq = _np(out["U"]), _np(out["lambda"]), _np(out["rho_qp"])
    err = np.max(np.abs(U - d["U_exact"].T)) / cfg.umax
    assert err <= U_TOL, err
    assert np.array_equal(_bits(rq), _bits(d["rho"].T))
    assert lam.shape == (cfg.m, n)
    worst = mumax = 0.0
    qps = host_qp(ctl, cfg, rq, np.ascontiguousarray(d["x"].T))
    for s, (G, F, Lin, b) in enumerate(qps):
        ref = np.zeros(cfg.m)
        q = int(d["act"][s, N])
        ref[d["act"][s, :q]] = d["lam"][s, :q]
        mu, mur = K.to_mu(G, Lin, lam[:, s]), K.to_mu(G, Lin, ref)
        e = float(np.max(np.abs(mu - mur)) / max(1.0, np.max(np.abs(mur))))
        worst, mumax = max(worst, e), max(mumax, float(np.max(np.abs(mur))))
        assert e <= K.KKT_TOL, (name, s, e)
    kd = _np(ctl.step_kkt(_T(d["x"].T), out["rho_qp"], out["U"], out["lambda"], cfg))
    print(f"{name}: |U - U_exact| {err:.2e} umax, multipliers {worst:.2e} of max(1, mumax), mumax {mumax:.2e}, "
          f"device audit {kd.max(axis=1)}")
    assert np.all(kd <= K.KKT_TOL), kd.max(axis=1)


def _audit(ctl, cfg, x, out, tag):
    """NumPy measures and the device audit of a step_dual result (<= 1e-9 where the
    flag is 1), then their agreement after a deliberate change of lambda.  Returns
    the worst relative difference of the two."""
    U, lam, rq, flag = _np(out["U"]), _np(out["lambda"]), _np(out["rho_qp"]), _np(out["exitflag"])
    qps = host_qp(ctl, cfg, rq, x)
    kd = _np(ctl.step_kkt(_T(x), out["rho_qp"], out["U"], out["lambda"], cfg))
    l2 = lam.copy()
    for s, (G, F, Lin, b) in enumerate(qps):
        if flag[s] != 1:
            assert np.all(lam[:, s] == 0.0), (tag, s)
            continue
        kn = K.measures(G, F, Lin, b, U[:, s], lam[:, s])
        assert np.all(kn <= K.KKT_TOL), (tag, s, "NumPy", kn)
        assert np.all(kd[:, s] <= K.KKT_TOL), (tag, s, "device", kd[:, s])
        if cfg.m:
            l2[int(np.argmax(K.to_mu(G, Lin, lam[:, s]))), s] *= 1 + 2.0 ** -10
    k2 = _np(ctl.step_kkt(_T(x), out["rho_qp"], out["U"], _T(l2), cfg))
    worst = 0.0
    for s, (G, F, Lin, b) in enumerate(qps):
        if flag[s] != 1 or not np.any(l2[:, s] != lam[:, s]):
            continue
        ref = K.measures(G, F, Lin, b, U[:, s], l2[:, s])
        for e in range(4):
            if ref[e] >= 1e-6:
                assert k2[e, s] >= 1e-6, (tag, s, e, k2[:, s], ref)
                r = abs(k2[e, s] - ref[e]) / ref[e]
                worst = max(worst, r)
                assert r <= AGREE_TOL, (tag, s, e, k2[:, s], ref)
            else:
                assert abs(k2[e, s] - ref[e]) <= K.KKT_TOL + AGREE_TOL * ref[e], (tag, s, e, k2[:, s], ref)
    return worst


SHAPES = [(N, B, mode) for N, B in ((3, 21), (16, 21), (17, 9), (20, 9), (33, 9)) for mode in (1, 2, 3)] + [(64, 3, 3)]


@pytest.mark.parametrize("N,B,mode", SHAPES)
def test_two_steps_every_lane_shape(ctl, N, B, mode):
    """Two teacher-forced steps of the full LPV loop from scenarios_x0: P = 16
    (N = 3, 16; B = 21: four scenarios per wave, the last wave part-filled), P = 64
    (N = 17, 20, 33; B = 9) and the largest workspace (N = 64, mode 3, 8N + 2 rows).
    Each step runs step() and step_dual() on the same inputs; step()'s outputs
    drive the next step."""
    from ntm_mpc import Config, scenarios_x0
    cfg = Config(N=N, mode=mode)
    x = np.ascontiguousarray(scenarios_x0(0, B))
    rho, uo = ctl.initial_state(_T(x), cfg)
    worst = 0.0
    for k in range(2):
        rho_d, uo_d = rho.clone(), uo.clone()
        ref = ctl.step(_T(x), rho, uo, cfg)
        out = ctl.step_dual(_T(x), rho_d, uo_d, cfg)
        fl, fr = _np(out["exitflag"]), _np(ref["exitflag"])
        np.testing.assert_array_equal(fl, fr)
        same = _np(out["inner_iters"]) == _np(ref["inner_iters"])
        assert same.mean() >= (0.6 if mode == 3 else 0.9), (k, same.mean())
        du = np.max(np.abs(_np(out["U"]) - _np(ref["U"])), axis=0) / cfg.umax
        xn, xr = _np(out["x_next"]), _np(ref["x_next"])
        dx = np.max(np.abs(xn - xr) / np.abs(xr), axis=0)
        assert np.all(du[same] <= U_TOL), (k, du)
        assert np.all(dx[same] <= 1e-9), (k, dx)
        worst = max(worst, _audit(ctl, cfg, x, out, f"N={N} mode={mode} step {k}"))
        x = np.ascontiguousarray(xr)
    print(f"N={N} B={B} mode={mode}: structured audit against dense NumPy after the change of lambda, worst "
          f"relative difference {worst:.2e}")


@pytest.mark.parametrize("mode", [2, 3])
def test_reference_x0_among_healthy_scenarios(ctl, mode):
    """The reference's x0 (w = 0, NTM_MPC_Sim.m:34) violates w >= 0.06: flag -2,
    U = 0, lambda = 0 for that scenario; its neighbours (same wave at N = 8) are
    bitwise what they are without it."""
    from ntm_mpc import Config, scenarios_x0
    N, B = 8, 6
    cfg = Config(N=N, mode=mode)
    x = np.ascontiguousarray(scenarios_x0(0, B))
    x2 = x.copy()
    x2[:, 2] = O.REFERENCE_X0
    outs = []
    for xs in (x, x2):
        rho, uo = ctl.initial_state(_T(xs), cfg)
        o = ctl.step_dual(_T(xs), rho, uo, cfg)
        outs.append({k: _np(v) for k, v in o.items()})
    a, b = outs
    assert b["exitflag"][2] == -2 and np.all(b["U"][:, 2] == 0.0) and np.all(b["lambda"][:, 2] == 0.0)
    keep = [0, 1, 3, 4, 5]
    assert np.all(b["exitflag"][keep] == 1)
    for k in ("U", "lambda", "rho_qp", "x_next"):
        assert np.array_equal(_bits(a[k][:, keep]), _bits(b[k][:, keep])), k


@pytest.mark.parametrize("N,mode", [(8, 2), (20, 3)])
def test_lambda_does_not_depend_on_the_batch(ctl, N, mode):
    """13 scenarios whole against 1 + 2 + 3 + 7: lambda, U and rho_qp bitwise."""
    from ntm_mpc import Config, scenarios_x0
    cfg = Config(N=N, mode=mode)
    x = np.ascontiguousarray(scenarios_x0(0, 13))

    def run(xs):
        rho, uo = ctl.initial_state(_T(xs), cfg)
        o = ctl.step_dual(_T(xs), rho, uo, cfg)
        return {k: _np(o[k]) for k in ("U", "lambda", "rho_qp")}

    whole = run(x)
    assert np.any(whole["lambda"] > 0.0)
    at = 0
    for n in (1, 2, 3, 7):
        part = run(np.ascontiguousarray(x[:, at:at + n]))
        for k, v in part.items():
            assert np.array_equal(_bits(v), _bits(whole[k][:, at:at + n])), (k, at, n)
        at += n


def test_full_size_batch_once(ctl):
    """B = 1e5, N = 20, mode 2: one step_dual from the benchmark's initial state,
    then step_kkt.  Every scenario with flag 1 has all four measures <= 1e-9 and
    every other one lambda = 0.  The worst measure and both kernels' times are
    printed, not asserted."""
    from ntm_mpc import Config, scenarios_x0
    B, N = 100_000, 20
    cfg = Config(N=N, mode=2)
    x = _T(scenarios_x0(0, B))
    rho, uo = ctl.initial_state(x, cfg)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    out = ctl.step_dual(x, rho, uo, cfg)
    ev[1].record()
    kkt = ctl.step_kkt(x, out["rho_qp"], out["U"], out["lambda"], cfg)
    ev[2].record()
    torch.cuda.synchronize()
    ok = out["exitflag"] == 1
    worst = kkt[:, ok].max(dim=1).values.cpu().numpy()
    print(f"B=1e5 N=20 mode 2: flag 1 on {int(ok.sum())} of {B}; worst measures {worst}; step_dual "
          f"{ev[0].elapsed_time(ev[1]):.2f} ms, step_kkt {ev[1].elapsed_time(ev[2]):.2f} ms (first launches)")
    assert int(ok.sum()) > 0.9 * B
    assert bool(torch.all(kkt[:, ok] <= K.KKT_TOL)), worst
    assert bool(torch.all(out["lambda"][:, ~ok] == 0.0))
