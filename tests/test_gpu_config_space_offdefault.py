"""GPU parity off the benchmark points, part 2: off-default physics and
configuration, and exit flag -2 on every build (part 1: test_gpu_config_space.py).

Every other GPU test runs the default ntm_physics and, but for N, mode, Q, r, Ru
and flags, the default ntm_config; umin = 0 in particular hides sign errors in
the lower input bound.  Here every build runs a combined off-default set
(PH2 / CFG2, whose constraints bind: the tests assert so from the oracle's
output), each field is changed on its own at N = 20 (each moves U or x_next by
>= 0.13 of full scale in the oracle, nine orders above the tolerance), and the
infeasible outcomes are pinned: the D22 edge of the x_0 rows, and a tightened
omega bound whose LPV loops alternate feasible and infeasible QPs (the
Goldfarb-Idnani infeasibility exit, the U = 0 reset, the warm-start slots after
an infeasible QP, the constant omega row of x_1).

Tolerances are test_gpu_parity's own.  CPU preconditions: the two
oracles agree to 4.4e-14 umax on the same path with PH2 / CFG2 at (N, mode) =
(12,2), (12,3), (20,2), (20,3), (24,3); the final flags and iteration counts of
the tightened-bound batch do not change when xmax[1] is scaled by 1 +- 1e-6, on
either of the two steps, at any of the builds below."""
import contextlib
import math

import numpy as np
import pytest

from oracle import cbind
from oracle import ntm_oracle as O
from test_gpu_parity import H, RUN_TOL, T, U_TOL, X_TOL, _assert_run_close, _teacher_forced, cfgs

pytestmark = pytest.mark.gpu

TP = 2 * math.pi
XSCALE = np.array([0.15, 2000 * math.pi])[:, None]
PH2 = dict(j_BS=80e3, w_dep=0.03, eta_CD=0.8, tau_r=250.0, tau_E=3.0, w_sat=0.30, w_marg=0.025, tau_w=0.2,
           omega0=TP * 400)
CFG2 = dict(Ts=0.08, xmin=(0.065, 150 * TP), xmax=(0.16, 4000 * TP), umin=2e5, umax=1.5e6, r=(0.08, 900 * TP),
            du_max=3e5)


@pytest.fixture(scope="module")
def pctl():
    """A controller of this module's own, whose physics the tests set."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ntm_mpc import NtmMpc
    c = NtmMpc()
    yield c
    c.close()


@contextlib.contextmanager
def physics_of(pctl, **kw):
    """pctl with ntm_mpc.Physics(**kw); yields the matching O.Physics."""
    from ntm_mpc import Physics
    pctl.physics = Physics(**kw)
    try:
        yield O.Physics(**kw)
    finally:
        pctl.physics = Physics()


@contextlib.contextmanager
def build_of(ctl, build):
    """Force the N = 20 build "lds1" (the default at these batch sizes), "lds" or "far";
    None leaves the dispatch alone.  The batch limits are restored on exit."""
    try:
        if build == "lds":
            ctl.set_one_wave_batch(0)
        elif build == "far":
            ctl.set_small_batch(0)
        yield
    finally:
        ctl.set_one_wave_batch(-1)
        ctl.set_small_batch(-1)


def kernel_name(N, mode, build):
    """The dispatch target of (N, mode) at the reference's Q and Ru = 0."""
    if N == 20 and mode != 3:
        return "k_mpc_step<P=64,NN=20," + {"lds1": "lds> (one-wave budget)", "lds": "lds>", "far": "far>"}[build]
    if N == 50:
        return "k_mpc_step<P=64,NN=50,far>"              # ntm_n50 (modes 0-2) or ntm_n50m3 (mode 3)
    return f"k_mpc_step<P={16 if N <= 16 else 64},NN={10 if N == 10 else 0},lds>"


def assert_build(ctl, B, cfg, build):
    assert ctl.step_kernel_name(B, cfg) == kernel_name(cfg.N, cfg.mode, build)
    if build in ("lds1", "lds", "far"):
        assert ctl.step_build(B, cfg) == build


# ---------------------------------------------------------------- 3. function level with PH2 / CFG2
def _states(B, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.03, 0.2, B), rng.uniform(0.4, 1.6, B) * 900 * TP])


def _rho2(N, B, seed, ph, ocfg):
    xs = _states(B * N, seed).reshape(2, B, N)
    return np.stack([np.concatenate([O.rho_all(xs[:, s, i], ph, ocfg) for i in range(N)]) for s in range(B)], axis=1)


def test_offdefault_rho_AB(pctl):
    B = 300
    cfg, ocfg = cfgs(20, 2, **CFG2)
    x = _states(B, 1)
    with physics_of(pctl, **PH2) as ph:
        ref = np.stack([O.rho_all(x[:, s], ph, ocfg) for s in range(B)], axis=1)
        np.testing.assert_allclose(H(pctl.rho(T(x), cfg)), ref, rtol=1e-14, atol=0)
        A, Bv = (H(t) for t in pctl.AB(T(ref), cfg))
        for s in range(0, B, 3):
            np.testing.assert_allclose(A[:, s].reshape(2, 2, order="F"), O.A_mat(ref[0, s], ref[1, s], ph, ocfg.Ts),
                                       rtol=1e-14, atol=0)
            np.testing.assert_allclose(Bv[:, s], O.B_mat(ref[2, s], ph, ocfg.Ts), rtol=1e-14, atol=0)
        # the off-default constants reach the result: the default ones are far away
        d = np.stack([O.rho_all(x[:, s], O.Physics(), ocfg) for s in range(B)], axis=1)
        assert np.max(np.abs(d - ref) / np.abs(ref)) > 1e-2


@pytest.mark.parametrize("N", [7, 20])
def test_offdefault_lift_cost_getwlc(pctl, N):
    """Phi, Gamma, Lambda (1e-13), G, F (1e-12 of the largest entry) and getWLc's W, L, c
    (1e-13) with PH2 / CFG2 against the NumPy oracle."""
    B = 11
    cfg, ocfg = cfgs(N, 2, **CFG2)
    m = 6 * N + 4
    with physics_of(pctl, **PH2) as ph:
        rho = _rho2(N, B, 3, ph, ocfg)
        x = _states(B, 4)
        Phi, Gam, Lam = (H(t) for t in pctl.lift(T(rho), cfg))
        G, F = (H(t) for t in pctl.cost(T(rho), T(x), cfg))
        W, L, c = (H(t) for t in pctl.getWLc(T(rho), cfg))
    worst = 0.0
    for s in range(B):
        P_, G_, L_ = O.lift(rho[:, s].reshape(N, 3).T, ph, ocfg)
        np.testing.assert_allclose(Phi[:, s].reshape(2 * N, 2, order="F"), P_, rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(Gam[:, s].reshape(2 * N, N, order="F"), G_, rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(Lam[:, s], L_, rtol=1e-13, atol=1e-300)
        Gr, Fr = O.cost(P_, G_, L_, x[:, s], ocfg)
        eg = np.max(np.abs(G[:, s].reshape(N, N, order="F") - Gr)) / np.max(np.abs(Gr))
        ef = np.max(np.abs(F[:, s] - Fr)) / np.max(np.abs(Fr))
        worst = max(worst, eg, ef)
        assert eg <= 1e-12 and ef <= 1e-12, (s, eg, ef)
        Wr, Lr, cr = O.getWLc(ocfg.xmax, ocfg.xmin, ocfg.umax, ocfg.umin, G_, P_, L_)
        np.testing.assert_allclose(W[:, s].reshape(m, 2, order="F"), Wr, rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(L[:, s].reshape(m, N, order="F"), Lr, rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(c[:, s], cr, rtol=1e-13, atol=1e-12)
    print(f"N={N} PH2/CFG2: G, F within {worst:.2e} of the largest entry")


# ---------------------------------------------------------------- 3. steps and loops with PH2 / CFG2
def _binding(refs, ocfg):
    """From the oracle's output: plan entries at umin, at umax, and scenario-steps with
    a predicted island width on one of its bounds (an active w row)."""
    U = np.concatenate([r["U"] for r in refs], axis=1)
    w = np.concatenate([r["x_pred"][2::2] for r in refs], axis=1)             # w of x^_1..x^_N
    at_w = (np.abs(w - ocfg.xmin[0]) < 1e-7) | (np.abs(w - ocfg.xmax[0]) < 1e-7)
    return (int((np.abs(U - ocfg.umin) < 1e-6 * ocfg.umax).sum()), int((np.abs(U - ocfg.umax) < 1e-6 * ocfg.umax).sum()),
            int(at_w.any(axis=0).sum()))


STEP2 = [(4, 2, False, None), (10, 2, True, None), (10, 3, False, None), (12, 3, True, None), (20, 2, False, "lds1"),
         (20, 2, True, "lds"), (20, 2, True, "far"), (20, 1, False, "far"), (20, 3, False, None), (24, 2, True, None),
         (50, 2, False, "far"), (50, 3, True, "far")]


@pytest.mark.parametrize("N,mode,warm,build", STEP2)
def test_offdefault_step_every_build(pctl, N, mode, warm, build):
    """Teacher-forced steps with PH2 / CFG2 on every dispatch target.  The oracle's
    plans sit on umin and on umax in every case, and from N = 20 on (modes 2, 3) a
    w row is active as well, so no case passes with nothing binding."""
    B, k_sim = (8, 3) if N == 50 else (16, 4)
    cfg, ocfg = cfgs(N, mode, **CFG2)
    with physics_of(pctl, **PH2) as ph, build_of(pctl, build):
        assert_build(pctl, B, cfg, build)
        res = _teacher_forced(pctl, N, mode, warm, k_sim=k_sim, B=B, physics=ph, **CFG2)
    assert all((r["exitflag"] == 1).all() for r in res["refs"])
    n_lo, n_hi, n_w = _binding(res["refs"], ocfg)
    print(f"N={N} mode {mode}: {n_lo} plan entries at umin, {n_hi} at umax, {n_w} scenario-steps with a w row active")
    assert n_lo > 0 and n_hi > 0
    if N >= 20 and mode >= 2:
        assert n_w > 0


@pytest.mark.parametrize("N,mode,B,build", [(10, 1, 16, None), (20, 2, 16, "far"), (50, 3, 8, "far")])
def test_offdefault_run_closed_loop(pctl, N, mode, B, build):
    k_sim = 10
    cfg, ocfg = cfgs(N, mode, **CFG2)
    x0 = O.scenario_x0(np.arange(B)).T
    with physics_of(pctl, **PH2) as ph, build_of(pctl, build):
        assert_build(pctl, B, cfg, build)
        ref = cbind.run(x0, ocfg, k_sim, ph=ph)
        out = pctl.run(T(x0), k_sim, cfg)
        _assert_run_close(out, ref, cfg, k_sim, tol=RUN_TOL, x0=x0, ocfg=ocfg, physics=ph)


# ---------------------------------------------------------------- 3. one field at a time
CFG_VARIANTS = [dict(umin=2e5), dict(umax=1.5e6), dict(xmin=(0.065, 150 * TP)), dict(xmax=(0.16, 4000 * TP)),
                dict(Ts=0.08), dict(r=(0.08, 900 * TP)), dict(epsilon=1.0, i_sim=6), dict(i_sim=3),
                dict(mode=3, du_max=3e5)]
PH_VARIANTS = [dict(j_BS=80e3), dict(w_dep=0.03), dict(tau_r=250.0), dict(eta_CD=0.8), dict(w_sat=0.30, w_marg=0.025),
               dict(tau_E=3.0, tau_E0=3.0), dict(Lq=0.8, B_pol=1.0), dict(tau_A0=2.5e-6, tau_w=0.2, omega0=TP * 400),
               dict(m=3.0), dict(Cw=1.2), dict(rs=1.6, a=1.9), dict(mu0=1.3e-6)]


def _vid(v):
    return "-".join(v)


@pytest.mark.parametrize("build", ["lds1", "far"])
@pytest.mark.parametrize("var", CFG_VARIANTS, ids=_vid)
def test_one_config_field(ctl, var, build):
    """N = 20, mode 2 (but for the du_max variant, which needs the rate rows and so
    runs on the generic kernel), one ntm_config field off its default."""
    kw = dict(var)
    mode = kw.pop("mode", 2)
    cfg, _ = cfgs(20, mode, **kw)
    with build_of(ctl, build):
        assert_build(ctl, 8, cfg, None if mode == 3 else build)
        res = _teacher_forced(ctl, 20, mode, False, k_sim=2, B=8, **kw)
    assert all((r["exitflag"] == 1).all() for r in res["refs"])


@pytest.mark.parametrize("build", ["lds1", "far"])
@pytest.mark.parametrize("var", PH_VARIANTS, ids=_vid)
def test_one_physics_field(pctl, var, build):
    """N = 20, mode 2, one group of ntm_physics constants off its default."""
    cfg, _ = cfgs(20, 2)
    with physics_of(pctl, **var) as ph, build_of(pctl, build):
        assert_build(pctl, 8, cfg, build)
        res = _teacher_forced(pctl, 20, 2, False, k_sim=2, B=8, physics=ph)
    assert all((r["exitflag"] == 1).all() for r in res["refs"])


# ---------------------------------------------------------------- 4. exit flag -2 on every build
BUILDS = [(6, 2, None), (10, 2, None), (16, 2, None), (20, 2, "lds1"), (20, 2, "lds"), (20, 2, "far"), (20, 3, None),
          (33, 2, None), (50, 2, "far"), (50, 3, "far")]
X0_EDGE = np.array([[0.15, 0.15 + 5e-10, 0.15 + 2e-9, 0.06 - 5e-10, 0.06 - 2e-9, 0.0605, 0.1499], [1000 * TP] * 7])
X_TIGHT = np.array([[0.10, 0.09, 0.12, 0.08, 0.10, 0.10, 0.1499, 0.11],
                    np.array([1000.0, 1000, 995, 990, 960, 900, 1000, 700]) * TP])
XMAX_TIGHT = (0.15, 1010 * TP)


def _check_step(out, ref, cfg, exact_iters=True):
    """Flags (and LPV iterations) equal the oracle's; U == 0 exactly where the flag is
    -2; U, x_pred and x_next within tolerance where it is 1.  Returns (dU / umax, dx)."""
    N = cfg.N
    fl, U = H(out["exitflag"]), H(out["U"])
    np.testing.assert_array_equal(fl, ref["exitflag"])
    if exact_iters:
        np.testing.assert_array_equal(H(out["inner_iters"]), ref["inner_iters"])
    assert (U[:, fl == -2] == 0).all() and (ref["U"][:, fl == -2] == 0).all()
    ok = fl == 1
    du = np.max(np.abs(U - ref["U"])[:, ok], initial=0.0) / cfg.umax
    dx = max(np.max((np.abs(H(out["x_pred"]) - ref["x_pred"]) / np.tile(XSCALE, (N + 1, 1)))[:, ok], initial=0.0),
             np.max((np.abs(H(out["x_next"]) - ref["x_next"]) / XSCALE)[:, ok], initial=0.0))
    assert du <= U_TOL and dx <= X_TOL, (du, dx)
    return du, dx


@pytest.mark.parametrize("N,mode,build", BUILDS + [(10, 1, None), (20, 1, "far"), (50, 1, "far")])
def test_x0_edge_of_feasibility(ctl, N, mode, build):
    """D22 on the x_0 rows: an x_0 up to 1e-9 outside [xmin, xmax] is feasible, 2e-9
    outside is not; box mode has no state rows and solves them all."""
    cfg, ocfg = cfgs(N, mode)
    x = X0_EDGE
    rho, Uo = cbind.initial_state(x, ocfg)
    ref = cbind.step(x, rho, Uo, ocfg)
    np.testing.assert_array_equal(ref["exitflag"], [1] * 7 if mode == 1 else [1, 1, -2, 1, -2, 1, 1])
    with build_of(ctl, build):
        assert_build(ctl, 7, cfg, build)
        out = ctl.step(T(x), T(rho), T(Uo), cfg)
        du, dx = _check_step(out, ref, cfg)
    print(f"N={N} mode {mode} x_0 edge: max |U - U_oracle| / umax = {du:.2e}, states {dx:.2e}")


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("N,mode,build", BUILDS)
def test_tightened_omega_bound(ctl, N, mode, build, warm):
    """xmax[1] = 1010 * 2 pi: LPV loops that alternate feasible and infeasible QPs
    (U reset to 0 between them), some ending on flag 1 after 3-5 infeasible QPs,
    some on -2, and scenario 6 stopping at the constant omega row of x_1; two
    teacher-forced steps, with and without the carried workspace."""
    cfg, ocfg = cfgs(N, mode, xmax=XMAX_TIGHT)
    x = X_TIGHT
    rho, Uo = cbind.initial_state(x, ocfg)
    ws = ctl.new_active_ws(8, cfg) if warm else None
    worst = (0.0, 0.0)
    with build_of(ctl, build):
        assert_build(ctl, 8, cfg, build)
        for k in range(2):
            ref = cbind.step(x, rho, Uo, ocfg)
            if k == 0 and N >= 16:
                np.testing.assert_array_equal(ref["exitflag"], [-2, -2, 1, 1 if N <= 20 else -2, -2, -2, -2, 1])
                np.testing.assert_array_equal(ref["inner_iters"], [10] * 6 + [2, 10])
            out = ctl.step(T(x), T(rho), T(Uo), cfg, active_ws=ws)
            worst = tuple(max(a, b) for a, b in zip(worst, _check_step(out, ref, cfg)))
            x, rho, Uo = ref["x_next"], ref["rho"], ref["U_old"]
    print(f"N={N} mode {mode} tightened omega bound: max |U - U_oracle| / umax = {worst[0]:.2e}, states {worst[1]:.2e}")
