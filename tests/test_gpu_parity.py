"""GPU parity tests: every row of SURVEY.md §8(a) through the C-ABI against the
CPU oracle, on seeded inputs.

Tolerances (fp64 everywhere; north_star asks <= 1e-10 relative on U):
  * rho / A / B / Phi / Gamma / Lambda / getWLc: 1e-13 relative (few-ulp work)
  * G, F: 1e-12 relative to the largest entry of the same matrix
  * QP / one MPC step (teacher-forced: identical inputs to the GPU and the
    oracle every step): max |U_gpu - U_oracle| / umax <= 1e-10
  * free-running closed loop: RUN_TOL = 5e-8 (rounding is amplified by the
    closed loop; unconstrained mode 0 1e-6 of umax, its minimisers
    being unbounded); the 256-scenario loops of test_gpu_parity_wide.py bound
    each scenario by max(RUN_TOL, 10 x the loop's own sensitivity)
"""
import dataclasses
import math

import numpy as np
import pytest
import torch

from oracle import cbind
from oracle import ntm_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U_TOL = 1e-10
# mode 3 (BASELINE config 5, input-rate rows: an extension, not in the reference):
# the same 1e-10.  The oracle's final value comes from an accurate long-double KKT
# solve on its active set (oracle accurate_resolve / orc_accurate),
# within ~1e-16 umax of a 30-digit solve; its fp64 re-solve alone sat up to
# ~6e-9 umax off when the rate rows leave G~_FF nearly singular
U_TOL_RATE = 1e-10
# predicted / next states, relative to |w| ~ 0.15 m and |omega| ~ 2000 pi: 1e-9
X_TOL, X_TOL_RATE = 1e-9, 1e-9
# free-running closed loops against the C oracle over 20 steps: the loop feeds each
# step's rounding back through rho(x) (per-step errors of ~1e-12 umax grow to
# 1e-9 - 1e-8 by step 20: measured 1.2e-9 to 3.3e-9 in modes 2 and 3, N = 20 and
# 50, and 1.03e-8 in mode 1 on the far build), so the bound is 5e-8, 20x tighter
# than round 3's 1e-6 (whose oracle sat ~1e-9 off the exact optimum itself)
RUN_TOL = 5e-8


def T(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def H(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def cfgs(N, mode, **kw):
    from ntm_mpc import Config
    return Config(N=N, mode=mode, **kw), O.Config(N=N, mode=mode, **kw)


def random_states(B, seed=1):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.02, 0.2, B)
    om = rng.uniform(0.5, 1.5, B) * 2000 * math.pi
    return np.stack([w, om])


def random_rho(N, B, seed=2):
    ph = O.Physics()
    cfg = O.Config(N=N)
    xs = random_states(B * N, seed).reshape(2, B, N)
    rho = np.zeros((3 * N, B))
    for s in range(B):
        for i in range(N):
            rho[3 * i:3 * i + 3, s] = O.rho_all(xs[:, s, i], ph, cfg)
    return rho


# ---------------------------------------------------------------- a1-a5
def test_rho_matches_oracle(ctl):
    B = 1000
    x = random_states(B)
    _, ocfg = cfgs(20, 2)
    got = H(ctl.rho(T(x)))
    ref = np.stack([O.rho_all(x[:, s], O.Physics(), ocfg) for s in range(B)], axis=1)
    np.testing.assert_allclose(got, ref, rtol=1e-14, atol=0)


def test_AB_match_oracle(ctl):
    B = 500
    x = random_states(B, 3)
    ph = O.Physics()
    _, ocfg = cfgs(20, 2)
    rho = np.stack([O.rho_all(x[:, s], ph, ocfg) for s in range(B)], axis=1)
    A, Bv = ctl.AB(T(rho))
    A, Bv = H(A), H(Bv)
    for s in range(0, B, 7):
        Aref = O.A_mat(rho[0, s], rho[1, s], ph, 0.1)
        np.testing.assert_allclose(A[:, s].reshape(2, 2, order="F"), Aref, rtol=1e-14, atol=0)
        np.testing.assert_allclose(Bv[:, s], O.B_mat(rho[2, s], ph, 0.1), rtol=1e-14, atol=0)


# ---------------------------------------------------------------- a8
@pytest.mark.parametrize("N", [1, 3, 10, 20, 50])
def test_lift_matches_oracle(ctl, N):
    B = 33
    cfg, ocfg = cfgs(N, 2)
    rho = random_rho(N, B)
    Phi, Gam, Lam = (H(t) for t in ctl.lift(T(rho), cfg))
    for s in range(B):
        P_, G_, L_ = O.lift(rho[:, s].reshape(N, 3).T, O.Physics(), ocfg)
        np.testing.assert_allclose(Phi[:, s].reshape(2 * N, 2, order="F"), P_, rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(Gam[:, s].reshape(2 * N, N, order="F"), G_, rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(Lam[:, s], L_, rtol=1e-13, atol=1e-300)


# ---------------------------------------------------------------- a9
@pytest.mark.parametrize("N,Ru", [(3, 0.0), (20, 0.0), (50, 0.0), (20, 1e-10), (3, 1e-9)])
def test_cost_matches_oracle(ctl, N, Ru):
    """G and F of NTM_MPC_Sim.m:120-121 (+ 2 Ru I with an input weight, ABI v5)."""
    B = 17
    cfg, ocfg = cfgs(N, 2, Ru=Ru)
    rho = random_rho(N, B, 5)
    x = random_states(B, 6)
    G, F = (H(t) for t in ctl.cost(T(rho), T(x), cfg))
    for s in range(B):
        P_, G_, L_ = O.lift(rho[:, s].reshape(N, 3).T, O.Physics(), ocfg)
        Gr, Fr = O.cost(P_, G_, L_, x[:, s], ocfg)
        Gs = G[:, s].reshape(N, N, order="F")
        assert np.max(np.abs(Gs - Gr)) <= 1e-12 * np.max(np.abs(Gr))
        assert np.max(np.abs(F[:, s] - Fr)) <= 1e-12 * np.max(np.abs(Fr))


# ---------------------------------------------------------------- a10
@pytest.mark.parametrize("N", [1, 4, 20])
def test_getwlc_matches_oracle(ctl, N):
    B = 9
    cfg, ocfg = cfgs(N, 2)
    m = 6 * N + 4
    rho = random_rho(N, B, 7)
    W, L, c = (H(t) for t in ctl.getWLc(T(rho), cfg))
    for s in range(B):
        P_, G_, L_ = O.lift(rho[:, s].reshape(N, 3).T, O.Physics(), ocfg)
        Wr, Lr, cr = O.getWLc(ocfg.xmax, ocfg.xmin, ocfg.umax, ocfg.umin, G_, P_, L_)
        np.testing.assert_allclose(W[:, s].reshape(m, 2, order="F"), Wr, rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(L[:, s].reshape(m, N, order="F"), Lr, rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(c[:, s], cr, rtol=1e-13, atol=1e-12)


# ---------------------------------------------------------------- a11
def _qp_batch(N, mode, B, seed):
    """Realistic QPs: states and schedules along oracle closed-loop trajectories."""
    _, ocfg = cfgs(N, mode)
    ph = O.Physics()
    x0 = O.scenario_x0(np.arange(seed, seed + B))
    if mode == O.MODE_NONE:
        # BASELINE config 1 uses the reference x0 (NTM_MPC_Sim.m:34); from the
        # synthetic states the unconstrained LQ is singular
        x0 = np.tile(O.REFERENCE_X0, (B, 1))
        x0[:, 1] *= 1.0 + 1e-3 * np.arange(B)
    Gs, Fs, Ls, bs = [], [], [], []
    for s in range(B):
        xk = x0[s]
        Rho = O.initial_rho(xk, ph, ocfg)
        U = np.zeros(N)
        for it in range(1 + (s % 3)):
            Phi, Gam, Lam = O.lift(Rho, ph, ocfg)
            G, F = O.cost(Phi, Gam, Lam, xk, ocfg)
            Lin, b = O.constraints(Phi, Gam, Lam, xk, ocfg)
            U, _, _ = O.qp_solve(G, F, Lin, b)
            _, Rho = O.rollout(xk, Rho, U, ph, ocfg)
        Phi, Gam, Lam = O.lift(Rho, ph, ocfg)
        G, F = O.cost(Phi, Gam, Lam, xk, ocfg)
        Lin, b = O.constraints(Phi, Gam, Lam, xk, ocfg)
        Gs.append(G), Fs.append(F), Ls.append(Lin), bs.append(b)
    return Gs, Fs, Ls, bs


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_quadprog_matches_oracle(ctl, mode):
    N, B = 20, 24
    Gs, Fs, Ls, bs = _qp_batch(N, mode, B, 100)
    m = Ls[0].shape[0]
    Gb = np.stack([g.reshape(-1, order="F") for g in Gs], axis=1)
    Fb = np.stack(Fs, axis=1)
    Lb = np.stack([l_.reshape(-1, order="F") for l_ in Ls], axis=1) if m else None
    bb = np.stack(bs, axis=1) if m else None
    U, flag, its = ctl.quadprog(T(Gb), T(Fb), T(Lb) if m else None, T(bb) if m else None)
    U, flag = H(U), H(flag)
    for s in range(B):
        Ur, fr, _ = cbind.qp(Gs[s], Fs[s], Ls[s] if m else None, bs[s] if m else None)
        assert flag[s] == fr
        scale = max(2e6, np.max(np.abs(Ur)))       # mode 0 minimisers are unbounded (~1e11)
        tol = U_TOL_RATE if mode == 3 else U_TOL
        assert np.max(np.abs(U[:, s] - Ur)) / scale <= tol, (s, np.max(np.abs(U[:, s] - Ur)))


# ---------------------------------------------------------------- a7, a12, a13: one MPC step
@pytest.mark.parametrize("N,mode,warm", [(10, 0, False), (20, 1, False), (20, 2, False), (3, 2, False),
                                         (50, 2, False), (50, 1, False), (20, 2, True), (20, 1, True),
                                         (50, 2, True), (20, 3, False), (20, 3, True), (4, 3, False),
                                         (50, 3, True), (1, 2, False), (1, 1, True), (64, 2, True)])
def test_step_teacher_forced(ctl, N, mode, warm):
    _teacher_forced(ctl, N, mode, warm)


# Non-identity stage weights: the reference's Omega = blkdiag(Q, ..., Q) (NTM_MPC_Sim.m:59,
# 67-70) with a coupled symmetric positive-definite Q (row-major 2x2), so the per-stage
# Om products of the device (free response, certificate gradient, Gram terms) are
# exercised off the diagonal; another reference state r as well
@pytest.mark.parametrize("N,mode,warm", [(20, 2, True), (20, 1, False), (50, 2, False), (3, 2, False), (50, 3, True)])
def test_step_teacher_forced_weighted(ctl, N, mode, warm):
    _teacher_forced(ctl, N, mode, warm, k_sim=6 if N < 50 else 4, Q=(2.0e4, 3.0, 3.0, 2.0e-2),
                    r=(0.09, 900 * 2 * math.pi))


# Input weight R_u (ABI v5; SURVEY §2.1 D17 "Q, R_u exposed in config"; the reference's
# cost has none, NTM_MPC_Sim.m:59,72-73): G = 2 Gamma' Om Gamma + 2 Ru I on both sides
# (oracle cost / orc_cost).  The weights span the range where the plan moves (oracle,
# first step, 32 scenarios at N = 20 mode 2: Ru = 1e-11 moves U by 2e-4 umax, 1e-10 by
# 2e-3, 1e-9 by 0.70, i.e. the input cost takes over from the bang-bang plan); the
# smallest eigenvalue of the Ru = 0 Hessian is 3.9e-17.  The launches
# run on the generic kernels (the host dispatch), in every mode.
@pytest.mark.parametrize("N,mode,warm,Ru", [(20, 2, True, 1e-10), (20, 2, False, 1e-9), (20, 1, False, 1e-9),
                                            (50, 3, True, 1e-10), (3, 2, False, 1e-9), (10, 2, False, 1e-11),
                                            (20, 3, True, 1e-9)])
def test_step_teacher_forced_input_weight(ctl, N, mode, warm, Ru):
    _teacher_forced(ctl, N, mode, warm, Ru=Ru)


def test_input_weight_changes_the_plan_and_dispatch(ctl):
    """Ru != 0 is not a no-op (the plans move by far more than the parity tolerance),
    runs on the generic kernel, and Ru = 0 stays on the specialised one."""
    from ntm_mpc import Config
    assert ctl.step_kernel_name(100_000, Config(N=20, mode=2, Ru=1e-10)) == "k_mpc_step<P=64,NN=0,lds>"
    assert ctl.step_kernel_name(100_000, Config(N=20, mode=2, Ru=0.0)) == "k_mpc_step<P=64,NN=20,far>"
    B = 32
    x = O.scenario_x0(np.arange(B)).T
    outs = []
    for Ru in (0.0, 1e-10):
        cfg, ocfg = cfgs(20, 2, Ru=Ru)
        rho, Uo = cbind.initial_state(x, ocfg)
        outs.append(H(ctl.step(T(x), T(rho), T(Uo), cfg)["U"]))
    assert np.max(np.abs(outs[1] - outs[0])) / 2e6 > 1e-4


def test_run_closed_loop_input_weight(ctl):
    """ntm_mpc_run with Ru > 0 against the C oracle's closed loop (free-running, RUN_TOL)."""
    B, k_sim = 32, 20
    cfg, ocfg = cfgs(20, 2, Ru=1e-10)
    x0 = O.scenario_x0(np.arange(B)).T
    ref = cbind.run(x0, ocfg, k_sim)
    out = ctl.run(T(x0), k_sim, cfg)
    _assert_run_close(out, ref, cfg, k_sim, tol=RUN_TOL, x0=x0, ocfg=ocfg)


# N = 20 has two builds (ntm_ctx_set_small_batch): batches up to 8 x the compute
# units (2048 on an MI355X) run on the all-LDS 2-wave build, which is what the
# small batches of these tests reach by default; larger ones on the far-workspace
# (slim) 4-wave build (GI's factors in HBM), forced here.  The full-size tests
# (test_full_size_batch_properties) run the far build at B = 1e5 by default.
@pytest.mark.parametrize("N,mode,warm", [(20, 1, False), (20, 2, False), (20, 2, True), (20, 3, True)])
def test_step_teacher_forced_far_build(ctl, N, mode, warm):
    ctl.set_small_batch(0)
    try:
        _teacher_forced(ctl, N, mode, warm)
    finally:
        ctl.set_small_batch(-1)


@pytest.mark.parametrize("mode", [1, 2])
def test_run_closed_loop_far_build(ctl, mode):
    B, k_sim = 32, 20
    cfg, ocfg = cfgs(20, mode)
    x0 = O.scenario_x0(np.arange(B)).T
    ref = cbind.run(x0, ocfg, k_sim)
    ctl.set_small_batch(0)
    try:
        out = ctl.run(T(x0), k_sim, cfg)
    finally:
        ctl.set_small_batch(-1)
    _assert_run_close(out, ref, cfg, k_sim, tol=RUN_TOL, x0=x0, ocfg=ocfg)


def test_step_layout_by_batch(ctl):
    """ntm_ctx_step_layout reports the build ntm_ctx_set_small_batch selects."""
    from ntm_mpc import Config
    c20, c50, c10 = Config(N=20, mode=2), Config(N=50, mode=2), Config(N=10, mode=2)
    # the all-LDS build takes up to 8 scenarios per compute unit (2048 on an MI355X's 256)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert ctl.step_layout(4 * cus, c20) == "lds" and ctl.step_layout(8 * cus, c20) == "lds"
    assert ctl.step_layout(8 * cus + 1, c20) == "far" and ctl.step_layout(100_000, c20) == "far"
    assert ctl.step_layout(100_000, c50) == "far" and ctl.step_layout(1, c50) == "far"
    assert ctl.step_layout(100_000, c10) == "lds"
    # the literal D4/D6 switches run on the generic (all-LDS) kernel at any batch size
    lit = Config(N=20, mode=2, flags=1)
    assert ctl.step_layout(100_000, lit) == "lds" and ctl.step_kernel_name(100_000, lit) == "k_mpc_step<P=64,NN=0,lds>"
    assert ctl.step_kernel_name(100_000, c20) == "k_mpc_step<P=64,NN=20,far>"
    # N = 20 with input-rate rows runs on the generic kernel too (its collision paths
    # and refined bordered re-solve keep mode 3 within 1e-10)
    assert ctl.step_kernel_name(100_000, Config(N=20, mode=3)) == "k_mpc_step<P=64,NN=0,lds>"
    assert ctl.step_kernel_name(100_000, Config(N=50, mode=3)) == "k_mpc_step<P=64,NN=50,far>"
    # a weighted stage cost: only the horizons compiled with Om = I (N <= 32) go generic;
    # the N = 50 kernel carries a general Om
    qw = dict(Q=(2.0e4, 3.0, 3.0, 2.0e-2))
    assert ctl.step_kernel_name(100_000, Config(N=50, mode=2, **qw)) == "k_mpc_step<P=64,NN=50,far>"
    assert ctl.step_kernel_name(100_000, Config(N=20, mode=2, **qw)) == "k_mpc_step<P=64,NN=0,lds>"
    ctl.set_small_batch(0)
    try:
        assert ctl.step_layout(1, c20) == "far"
        ctl.set_small_batch(1 << 40)
        assert ctl.step_layout(100_000, c20) == "lds"
    finally:
        ctl.set_small_batch(-1)


def test_small_batch_builds_agree(ctl):
    """The two N = 20 builds on the same inputs: same flags and inner iterations,
    U to 1e-12 umax (same arithmetic in different register allocations; the
    bitwise stopping rule could still part them by an iteration, which these
    seeded inputs do not)."""
    B = 256
    cfg, ocfg = cfgs(20, 2)
    x = O.scenario_x0(np.arange(B)).T
    rho, Uo = cbind.initial_state(x, ocfg)
    outs = []
    for lim in (-1, 0):
        ctl.set_small_batch(lim)
        try:
            outs.append(ctl.step(T(x), T(rho), T(Uo), cfg))
        finally:
            ctl.set_small_batch(-1)
    a, b = outs
    assert (H(a["exitflag"]) == H(b["exitflag"])).all()
    assert (H(a["inner_iters"]) == H(b["inner_iters"])).all()
    assert np.max(np.abs(H(a["U"]) - H(b["U"]))) / cfg.umax <= 1e-12


def test_one_wave_build_bitwise(ctl):
    """The all-LDS N = 20 build with the one-wave register budget (batches of at
    most 4 per CU, ntm_ctx_set_one_wave_batch) is the same arithmetic as the
    two-wave one: step and closed loop agree bit for bit; the builds are chosen
    by batch size (one wave up to 4 per CU, two up to 8 per CU, far above)."""
    B = 64
    cfg, ocfg = cfgs(20, 2)
    # thresholds per compute unit (1024 and 2048 scenarios on an MI355X's 256)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert ctl.step_build(4 * cus, cfg) == "lds1" and ctl.step_build(4 * cus + 1, cfg) == "lds"
    assert ctl.step_build(8 * cus, cfg) == "lds" and ctl.step_build(8 * cus + 1, cfg) == "far"
    assert ctl.step_build(100_000, cfg) == "far"
    assert "(one-wave budget)" in ctl.step_kernel_name(4 * cus, cfg)
    x = O.scenario_x0(np.arange(B)).T
    rho, Uo = cbind.initial_state(x, ocfg)
    outs, runs = [], []
    for lim in (-1, 0):
        ctl.set_one_wave_batch(lim)
        try:
            assert ctl.step_build(B, cfg) == ("lds1" if lim < 0 else "lds")
            outs.append(ctl.step(T(x), T(rho), T(Uo), cfg))
            runs.append(ctl.run(T(x), 6, cfg))
        finally:
            ctl.set_one_wave_batch(-1)
    for k in ("U", "x_pred", "x_next", "exitflag", "inner_iters"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    for k in ("uk", "Uk", "xk", "wpred", "exitflag", "inner_iters"):
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_sharded_far_total_is_bitwise(ctl):
    """A batch that takes the far build on one GPU (8192 > 2048 scenarios),
    sharded into all-LDS-size shards of 1024 with dist.pin_layout, reproduces
    the one-GPU batch bit for bit over two closed-loop steps."""
    import ntm_mpc
    from ntm_mpc.dist import pin_layout, shard_range
    total, world = 8192, 8
    cfg, _ = cfgs(20, 2)
    x0 = ntm_mpc.scenarios_x0(0, total)

    def two_steps(x):
        x = T(x)
        rho, uo = ctl.initial_state(x, cfg)
        ws = ctl.new_active_ws(x.shape[1], cfg)
        outs = []
        for _ in range(2):
            o = ctl.step(x, rho, uo, cfg, active_ws=ws)
            outs.append({k: H(o[k]).copy() for k in ("U", "x_next", "exitflag", "inner_iters")})
            x = o["x_next"].clone()
        return outs

    assert ctl.step_layout(total, cfg) == "far" and ctl.step_layout(total // world, cfg) == "lds"
    whole = two_steps(x0)
    try:
        assert pin_layout(ctl, total, cfg) == "far"
        parts = [two_steps(x0[:, f:f + c]) for f, c in (shard_range(total, world, r) for r in range(world))]
    finally:
        ctl.set_small_batch(-1)
    for k in range(2):
        for key in whole[k]:
            np.testing.assert_array_equal(np.concatenate([p[k][key] for p in parts], axis=-1), whole[k][key],
                                          err_msg=f"step {k} {key}")


def _teacher_forced(ctl, N, mode, warm, k_sim=None, gen=None, B=None, physics=None, x=None, **kw):
    """Each step, the GPU and the oracle get identical (x_k, rho, U_old); with
    warm=True the GPU also carries its active-set workspace from step to step
    (ntm_mpc_step_ws_device), which must not change the answer.

    The LPV loop stops on sum|U - Uold| < 1e-14 (NTM_MPC_Sim.m:123, D14), i.e. on
    a bitwise fixed point, so GPU and CPU rounding may stop it one iteration
    apart.  In modes 0-2 the loop is contractive and every scenario still
    agrees; with input-rate rows (mode 3) the loop can 2-cycle between active
    sets, and a scenario whose path diverged (different inner-iteration count,
    DESIGN.md §3) legitimately ends elsewhere: there the scenarios that took
    the same path are compared directly (>= 90% of them must have), and the
    others against the oracle re-run along the GPU's path (the GPU's
    inner-iteration count, no early stop), to the same tolerance.

    ``gen`` (oracle ScenarioGen): each scenario runs its own plasma and step k's
    plant step adds its disturbance at time index k, on both sides.

    ``B`` and ``k_sim`` override the batch size and the number of steps (defaults by
    horizon: 48 x 12 below N = 50, 48 x 4 at 50, 16 x 3 above); ``x`` (2, B) the
    initial states (default: the seeded scenarios); ``physics`` (an O.Physics) is
    the oracle's side of a controller ``ctl`` built with the matching
    ntm_mpc.Physics.  Returns the measured figures (worst U / umax on the same
    path and along the GPU's path, the same-path share)."""
    B0, ks = (48, 12) if N < 50 else ((48, 4) if N == 50 else (16, 3))
    B = B0 if B is None else B
    k_sim = ks if k_sim is None else k_sim
    cfg, ocfg = cfgs(N, mode, **kw)
    if x is None:
        x = O.scenario_x0(np.arange(B)).T if mode else np.tile(O.REFERENCE_X0[:, None], (1, B))
    assert x.shape == (2, B)
    if gen is None:
        rho, Uo = cbind.initial_state(x, ocfg, ph=physics)
    else:
        rho, Uo = cbind.initial_state_gen(x, ocfg, gen, ph=physics)
    try:
        return _teacher_forced_loop(ctl, N, mode, warm, k_sim, gen, cfg, ocfg, B, x, rho, Uo, physics)
    finally:
        if gen is not None:
            ctl.set_scenarios(None)


def _teacher_forced_loop(ctl, N, mode, warm, k_sim, gen, cfg, ocfg, B, x, rho, Uo, physics=None):
    from ntm_mpc import ScenarioGen
    ws = ctl.new_active_ws(B, cfg) if warm else None
    worst, worst_div, worst_x, same_iters, n, refs = 0.0, 0.0, 0.0, 0, 0, []
    xscale = np.array([0.15, 2000 * math.pi])[:, None]      # |w|, |omega| magnitudes
    for k in range(k_sim):
        ogen = None if gen is None else dataclasses.replace(gen, k0=k)
        if gen is not None:
            ctl.set_scenarios(ScenarioGen(**dataclasses.asdict(ogen)))
        ref = cbind.step(x, rho, Uo, ocfg, ph=physics, gen=ogen)
        refs.append(ref)
        tr, tu = T(rho), T(Uo)
        out = ctl.step(T(x), tr, tu, cfg, active_ws=ws)
        assert (H(out["exitflag"]) == ref["exitflag"]).all(), k
        same = H(out["inner_iters"]) == ref["inner_iters"]
        same_iters += int(same.sum())
        n += x.shape[1]
        cmp = same if mode == 3 else np.ones_like(same)
        worst = max(worst, np.max(np.abs(H(out["U"]) - ref["U"])[:, cmp], initial=0.0) / cfg.umax)
        gi = H(out["inner_iters"])
        xn = H(out["x_next"])
        xtol = X_TOL_RATE if mode == 3 else X_TOL
        xp = H(out["x_pred"]).reshape(N + 1, 2, -1).transpose(1, 0, 2)
        for i_g in np.unique(gi[~same]):
            # a path that stopped at another inner iteration: the oracle re-run along
            # the GPU's path gives the U, the rollout (x_pred: the last iteration's
            # rho, still moving when U has converged) and the plant step to compare
            # (the whole batch is re-run so each scenario keeps its generator id)
            sel = np.where(~same & (gi == i_g))[0]
            pcfg = dataclasses.replace(ocfg, i_sim=int(i_g), epsilon=-1.0)
            rp = cbind.step(x, rho, Uo, pcfg, ph=physics, gen=ogen)
            worst_div = max(worst_div, np.max(np.abs(H(out["U"])[:, sel] - rp["U"][:, sel])) / cfg.umax)
            xq = rp["x_pred"].reshape(N + 1, 2, -1).transpose(1, 0, 2)[:, :, sel]
            assert np.max(np.abs(xp[:, :, sel] - xq) / xscale[:, :, None]) <= xtol
        xr = ref["x_pred"].reshape(N + 1, 2, -1).transpose(1, 0, 2)
        worst_x = max(worst_x, np.max(np.abs(xn - ref["x_next"])[:, cmp] / xscale, initial=0.0),
                      np.max(np.abs(xp - xr)[:, :, same] / xscale[:, :, None], initial=0.0))
        assert np.max(np.abs(xn - ref["x_next"])[:, cmp] / xscale, initial=0.0) <= xtol
        assert np.max(np.abs(xp - xr)[:, :, same] / xscale[:, :, None], initial=0.0) <= xtol
        x, rho, Uo = ref["x_next"], ref["rho"], ref["U_old"]
    tol = U_TOL_RATE if mode == 3 else U_TOL
    print(f"N={N} mode {mode} B={B} x {k_sim} steps: max |U - U_oracle| / umax = {worst:.2e} (same path), "
          f"{worst_div:.2e} (along the GPU's path), states {worst_x:.2e}, same path {same_iters} of {n}")
    assert worst <= tol, worst
    assert worst_div <= tol, worst_div
    # the fraction of scenarios that stop at the same inner iteration is a property
    # of two exact solvers' rounding at the bitwise stopping rule: the two CPU
    # restatements themselves agree on 69% of the mode-3 steps at N = 4
    # (tests/test_oracle_c.py), the diverged ones are bounded by worst_div above
    assert same_iters >= (0.6 if mode == 3 else 0.9) * n, (same_iters, n)
    return {"worst": worst, "worst_div": worst_div, "worst_x": worst_x, "same": same_iters, "n": n, "refs": refs}


@pytest.mark.parametrize("N", [4, 20])
def test_rate_qps_match_oracle(ctl, N):
    """Mode 3's QPs themselves (not the LPV path): every QP the oracle meets
    along its trajectory, solved through ntm_qp_device, matches the oracle."""
    B, k_sim = 16, 6
    _, ocfg = cfgs(N, 3)
    ph = O.Physics()
    x = O.scenario_x0(np.arange(B)).T.copy()
    rho, Uo = cbind.initial_state(x, ocfg)
    Gs, Fs, Ls, bs = [], [], [], []
    for k in range(k_sim):
        for s in range(B):
            Rho = rho[:, s].reshape(N, 3).T
            Phi, Gam, Lam = O.lift(Rho, ph, ocfg)
            G, F = O.cost(Phi, Gam, Lam, x[:, s], ocfg)
            Lin, b = O.constraints(Phi, Gam, Lam, x[:, s], ocfg)
            Gs.append(G), Fs.append(F), Ls.append(Lin), bs.append(b)
        ref = cbind.step(x, rho, Uo, ocfg)
        x, rho, Uo = ref["x_next"], ref["rho"], ref["U_old"]
    Gb = np.stack([g.reshape(-1, order="F") for g in Gs], axis=1)
    Lb = np.stack([l_.reshape(-1, order="F") for l_ in Ls], axis=1)
    U, flag, _ = ctl.quadprog(T(Gb), T(np.stack(Fs, axis=1)), T(Lb), T(np.stack(bs, axis=1)))
    U, flag = H(U), H(flag)
    for i in range(len(Gs)):
        Ur, fr, _ = cbind.qp(Gs[i], Fs[i], Ls[i], bs[i])
        assert flag[i] == fr
        assert np.max(np.abs(U[:, i] - Ur)) / 2e6 <= U_TOL_RATE, i


@pytest.mark.parametrize("N,m", [(3, 40), (2, 60), (20, 200)])
def test_quadprog_many_dense_rows(ctl, N, m):
    """quadprog with more rows than the MPC step ever has (m > 8N+4): the
    active-row flags are sized from m, so none lands on the row norms.
    Random strictly convex QPs with feasible random rows, vs the oracle."""
    B = 24
    rng = np.random.default_rng(11 + N)
    Gs, Fs, Ls, bs = [], [], [], []
    for _ in range(B):
        A = rng.standard_normal((N + 2, N))
        Gs.append(A.T @ A + 0.1 * np.eye(N))
        Fs.append(rng.standard_normal(N) * 10)
        Lin = rng.standard_normal((m, N))
        xf = rng.standard_normal(N)
        Ls.append(Lin)
        bs.append(Lin @ xf + rng.uniform(0.0, 1.0, m))
    Gb = np.stack([g.reshape(-1, order="F") for g in Gs], axis=1)
    Lb = np.stack([l_.reshape(-1, order="F") for l_ in Ls], axis=1)
    U, flag, _ = ctl.quadprog(T(Gb), T(np.stack(Fs, axis=1)), T(Lb), T(np.stack(bs, axis=1)))
    U, flag = H(U), H(flag)
    for s in range(B):
        Ur, fr, _ = cbind.qp(Gs[s], Fs[s], Ls[s], bs[s])
        assert flag[s] == fr == 1, (s, flag[s], fr)
        assert np.max(np.abs(U[:, s] - Ur)) <= 1e-10 * max(1.0, np.max(np.abs(Ur))), s


def test_quadprog_null_rows_rejected(ctl):
    """m > 0 with a NULL Lin or b is an API error (NTM_E_INVALID), not a fault."""
    import ctypes as C
    N, m, B = 3, 4, 2
    G = T(np.tile(np.eye(N).reshape(-1, 1), (1, B)))
    F = T(np.ones((N, B)))
    Lb = T(np.ones((m * N, B)))
    U = torch.empty(N * B, dtype=torch.float64, device=DEV)
    fl = torch.empty(B, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    for lin, b in ((None, None), (p(Lb), None), (None, p(F))):
        rc = ctl.lib.ntm_qp_device(ctl._ctx, B, N, m, p(G), p(F), lin, b, p(U), p(fl), None, None)
        assert rc == -1, rc
    torch.cuda.synchronize()


def test_context_on_another_device_keeps_callers_device():
    """A context made for device d runs its work on d (host-buffer entry points
    included) and leaves the caller's current device unchanged."""
    from ntm_mpc import Config, NtmMpc
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    torch.cuda.set_device(0)
    c1 = NtmMpc(device=1)
    cfg = Config(N=20, mode=2)
    x0 = np.ascontiguousarray(O.scenario_x0(np.arange(8)).T)
    rho, uo = c1.initial_state_host(x0, cfg)
    out = c1.step_host(x0, rho, uo, cfg)
    assert torch.cuda.current_device() == 0
    ref = cbind.step(x0, *cbind.initial_state(x0, O.Config(N=20, mode=2)), O.Config(N=20, mode=2))
    assert np.max(np.abs(out["U"] - ref["U"])) / cfg.umax <= U_TOL
    c1.close()


def test_step_reference_x0_infeasible(ctl):
    """Known answer D15: x0 = [0; 2000 pi] (NTM_MPC_Sim.m:34) violates w >= 0.06
    (:40) -> quadprog exitflag -2 and U = 0 (D16), every scenario."""
    N, B = 3, 5
    cfg, ocfg = cfgs(N, 2)
    x = np.tile(O.REFERENCE_X0[:, None], (1, B))
    rho, Uo = cbind.initial_state(x, ocfg)
    out = ctl.step(T(x), T(rho), T(Uo), cfg)
    assert (H(out["exitflag"]) == -2).all()
    assert (H(out["U"]) == 0).all()


def test_quadprog_constant_row_tolerance(ctl):
    """D22: a constant row (Lin_i = 0) is violated only beyond 1e-9, as in both
    oracles (tests/test_oracle.py::test_constant_row_tolerance)."""
    bs = [-7e-18, -0.9e-9, -1e-6]
    B = len(bs)
    G = np.tile(np.eye(3).reshape(9, 1), (1, B))
    F = np.tile(np.array([1.0, -2.0, 0.5])[:, None], (1, B))
    Lin = np.tile(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]).reshape(-1, order="F")[:, None], (1, B))
    b = np.array([[b0, 10.0] for b0 in bs]).T
    U, flag, _ = ctl.quadprog(T(G), T(F), T(Lin), T(b))
    np.testing.assert_array_equal(H(flag), [1, 1, -2])
    np.testing.assert_allclose(H(U)[:, :2], -F[:, :2], atol=1e-15)


def test_step_nonfinite_flag(ctl):
    N = 20
    cfg, ocfg = cfgs(N, 2)
    x = O.scenario_x0(np.arange(4)).T.copy()
    x[1, 2] = np.nan
    rho, Uo = cbind.initial_state(x, ocfg)
    out = ctl.step(T(x), T(rho), T(Uo), cfg)
    fl = H(out["exitflag"])
    assert fl[2] == -7 and (fl[[0, 1, 3]] == 1).all()


@pytest.mark.parametrize("B", [1, 3, 65])
def test_step_ragged_batches(ctl, B):
    N = 20
    cfg, ocfg = cfgs(N, 2)
    x = O.scenario_x0(np.arange(B)).T
    rho, Uo = cbind.initial_state(x, ocfg)
    ref = cbind.step(x, rho, Uo, ocfg)
    out = ctl.step(T(x), T(rho), T(Uo), cfg)
    assert np.max(np.abs(H(out["U"]) - ref["U"])) / 2e6 <= U_TOL


# ---------------------------------------------------------------- closed loop
@pytest.mark.parametrize("N,mode", [(10, 0), (20, 1), (20, 2), (20, 3), (50, 2), (50, 3)])
def test_run_closed_loop(ctl, N, mode):
    """ntm_mpc_run (NTM_MPC_Sim.m:80-131) against the C oracle's closed loop: every
    workspace output north_star names, the applied inputs uk, the plans Uk
    (:106), the states xk and the predicted island width wpred (x_pred's w row,
    :110-117), free-running (rounding amplified by the loop: RUN_TOL = 5e-8 in
    modes 1-3, 1e-6 in mode 0)."""
    B, k_sim = 32, 20
    cfg, ocfg = cfgs(N, mode)
    x0 = O.scenario_x0(np.arange(B)).T if mode else np.tile(O.REFERENCE_X0[:, None], (1, B))
    ref = cbind.run(x0, ocfg, k_sim)
    out = ctl.run(T(x0), k_sim, cfg)
    # mode 0: the unconstrained minimisers reach ~1e11 (reference x0), so 1e-10 of
    # umax would ask for 1e-15 relative; the round-3 1e-6 stays
    _assert_run_close(out, ref, cfg, k_sim, tol=RUN_TOL if mode else 1e-6, x0=x0, ocfg=ocfg)


def _replay_along(x0s, ocfg, iters, gen, sid, physics=None):
    """The C oracle's closed loop for one scenario (global id ``sid`` of ``gen``)
    along a given path: step k runs exactly iters[k] LPV iterations (no early
    stop), so a scenario whose bitwise stopping rule (NTM_MPC_Sim.m:123-125)
    fired at another iteration on the GPU is checked on the GPU's own path.
    Returns the histories in ntm_mpc_run's layout (one column)."""
    N, K = ocfg.N, len(iters)
    g0 = None if gen is None else dataclasses.replace(gen, first_id=gen.first_id + sid)
    x = np.ascontiguousarray(x0s.reshape(2, 1))
    if g0 is None:
        rho, Uo = cbind.initial_state(x, ocfg, ph=physics)
    else:
        rho, Uo = cbind.initial_state_gen(x, ocfg, g0, ph=physics)
    h = {"xk": np.zeros((2 * (K + 1), 1)), "uk": np.zeros((K, 1)), "Uk": np.zeros((N * K, 1)),
         "wpred": np.zeros(((N + 1) * K, 1)), "exitflag": np.zeros((K, 1), np.int32),
         "inner_iters": np.zeros((K, 1), np.int32)}
    h["xk"][:2] = x
    for k in range(K):
        pc = dataclasses.replace(ocfg, i_sim=int(iters[k]), epsilon=-1.0)
        r = cbind.step(x, rho, Uo, pc, ph=physics,
                       gen=None if g0 is None else dataclasses.replace(g0, k0=g0.k0 + k))
        h["uk"][k] = r["U"][0]
        h["Uk"][k * N:(k + 1) * N] = r["U"]
        h["wpred"][k * (N + 1):(k + 1) * (N + 1)] = r["x_pred"][0::2]
        h["exitflag"][k], h["inner_iters"][k] = r["exitflag"], r["inner_iters"]
        x, rho, Uo = r["x_next"], r["rho"], r["U_old"]
        h["xk"][2 * (k + 1):2 * (k + 2)] = x
    return h


def _assert_run_close(out, ref, cfg, k_sim, tol=1e-6, x0=None, ocfg=None, gen=None, physics=None):
    """Closed-loop histories of the GPU against the C oracle's.  Mode 3 (rate rows)
    with ``x0``/``ocfg``: the LPV loop's bitwise stopping rule can fire at another
    iteration on the two sides, after which the plans part; such a
    scenario (at most 40% of them) is compared with the oracle replayed along the
    GPU's iteration counts instead (_replay_along)."""
    N = cfg.N
    g = {k: H(out[k]) for k in ("uk", "Uk", "xk", "wpred", "exitflag", "inner_iters")}
    if cfg.mode == 3 and x0 is not None:
        div = np.where(((g["inner_iters"] != ref["inner_iters"]) | (g["exitflag"] != ref["exitflag"])).any(axis=0))[0]
        print(f"N={N} mode 3: {len(div)} of {x0.shape[1]} scenarios replayed along the GPU's iteration counts")
        assert len(div) <= 0.4 * x0.shape[1], len(div)
        ref = {k: np.array(v, copy=True) for k, v in ref.items()}
        for s in div:
            rp = _replay_along(x0[:, s], ocfg, g["inner_iters"][:, s], gen, int(s), physics)
            for k in ref:
                ref[k][:, s] = rp[k][:, 0]
    du = np.max(np.abs(g["uk"] - ref["uk"])) / cfg.umax
    assert du <= tol, du
    dU = np.max(np.abs(g["Uk"] - ref["Uk"])) / cfg.umax
    assert dU <= tol, dU
    xscale = np.tile(np.array([0.15, 2000 * math.pi]), k_sim + 1)[:, None]
    assert np.max(np.abs(g["xk"] - ref["xk"]) / xscale) <= tol
    dw = np.max(np.abs(g["wpred"] - ref["wpred"])) / 0.15
    print(f"N={N} mode {cfg.mode} closed loop, {k_sim} steps: uk {du:.2e}, Uk {dU:.2e} (of umax), "
          f"xk {np.max(np.abs(g['xk'] - ref['xk']) / xscale):.2e}, wpred {dw:.2e}")
    assert dw <= tol, dw
    assert g["wpred"].shape == ((N + 1) * k_sim, ref["wpred"].shape[1])
    assert (g["exitflag"] == ref["exitflag"]).mean() > 0.99


def test_step_matches_run_first_step(ctl):
    """ntm_mpc_run's first step == ntm_mpc_step from the same initial state.

    The two are separate kernels built from the same device phases; the compiler
    may contract a*b+c into FMAs differently in each, so they agree to rounding
    (same exit flags and inner iterations, U and x_next to 1e-12 relative), not
    necessarily bit for bit."""
    N, B = 20, 16
    cfg, ocfg = cfgs(N, 2)
    x0 = O.scenario_x0(np.arange(B)).T
    rho, Uo = ctl.initial_state(T(x0), cfg)
    st = ctl.step(T(x0), rho, Uo, cfg)
    rn = ctl.run(T(x0), 1, cfg)
    assert torch.equal(st["exitflag"], rn["exitflag"][0])
    assert torch.equal(st["inner_iters"], rn["inner_iters"][0])
    assert torch.max(torch.abs(st["U"][0] - rn["uk"][0])).item() <= 1e-12 * cfg.umax
    xs = torch.tensor([[0.15], [2000 * math.pi]], dtype=torch.float64, device=DEV)
    assert torch.max(torch.abs(st["x_next"] - rn["xk"][2:4]) / xs).item() <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("small_batch", [-1, 0])
def test_host_buffer_entry_points_match_device(ctl, small_batch):
    """ntm_mpc_step / ntm_mpc_run with host arrays (the MEX boundary) give
    bit-identical results to the device-pointer entry points.  small_batch = 0
    forces the far-workspace build, whose per-context HBM block the two entry
    points share across streams (the context's own and the caller's): the
    launches must be ordered on it, or the results drift run to run."""
    ctl.set_small_batch(small_batch)
    try:
        _host_vs_device(ctl)
    finally:
        ctl.set_small_batch(-1)


def _host_vs_device(ctl):
    N, B = 20, 40
    cfg, ocfg = cfgs(N, 2)
    x0 = np.ascontiguousarray(O.scenario_x0(np.arange(B)).T)
    rho, Uo = ctl.initial_state(T(x0), cfg)
    rho_h, uo_h = ctl.initial_state_host(x0, cfg)
    np.testing.assert_array_equal(rho_h, H(rho))
    assert np.all(np.isinf(uo_h)) and np.all(uo_h > 0)
    r_or, u_or = cbind.initial_state(x0, ocfg)
    np.testing.assert_allclose(rho_h, r_or, rtol=1e-15)
    for _ in range(3):
        dv = ctl.step(T(x0), rho, Uo, cfg)
        hs = ctl.step_host(x0, rho_h, uo_h, cfg)
        for k in ("U", "x_pred", "x_next", "exitflag", "inner_iters"):
            np.testing.assert_array_equal(hs[k], H(dv[k]), err_msg=k)
        np.testing.assert_array_equal(rho_h, H(rho))
        np.testing.assert_array_equal(uo_h, H(Uo))
        x0 = np.ascontiguousarray(hs["x_next"])
    rd = ctl.run(T(x0), 3, cfg)
    rh = ctl.run_host(x0, 3, cfg)
    for k in rd:
        np.testing.assert_array_equal(rh[k], H(rd[k]), err_msg=k)


def test_step_garbage_workspace_is_ignored(ctl):
    """A caller-supplied warm-start workspace that is not a valid active set
    (ids out of range, repeats, counts > N) is ignored, never trusted: same
    flags and the same optimum as with no workspace."""
    N, B = 20, 64
    cfg, _ = cfgs(N, 2)
    x = T(O.scenario_x0(np.arange(B)).T)
    rng = np.random.default_rng(7)
    junk = rng.integers(-5, 400, size=(2 * (N + 1), B)).astype(np.int32)
    junk[N, :B // 2] = rng.integers(-3, 3 * N, size=B // 2)          # counts, many invalid
    junk[2 * N + 1, :] = N
    junk[0:4, 10] = 7                                                 # repeats
    junk[N, 10] = 4
    rho0, uo0 = ctl.initial_state(x, cfg)
    ref = ctl.step(x, rho0.clone(), uo0.clone(), cfg)
    out = ctl.step(x, rho0.clone(), uo0.clone(), cfg, active_ws=T(junk).to(torch.int32))
    assert torch.equal(out["exitflag"], ref["exitflag"])
    assert torch.max(torch.abs(out["U"] - ref["U"])).item() <= U_TOL * cfg.umax


def test_step_constant_rows_in_workspace_are_rejected(ctl):
    """A carried set holding a constant row (an x_0 row, getWLc rows 2..5, or the
    omega row of x_1, which B does not reach) is rejected, never solved with a
    garbage normal: same flags and optimum as with no workspace."""
    N, B = 20, 64
    cfg, _ = cfgs(N, 2)
    x = T(O.scenario_x0(np.arange(B)).T)
    ws = np.full((2 * (N + 1), B), -1, dtype=np.int32)
    for s in range(B):                        # slot 0: u-bound rows plus one constant row
        rows = [6 * j + 1 for j in range(1, 8)] + [2 + (s % 4) if s % 5 else 9]
        ws[:len(rows), s] = rows
        ws[N, s] = len(rows)
    rho0, uo0 = ctl.initial_state(x, cfg)
    ref = ctl.step(x, rho0.clone(), uo0.clone(), cfg)
    out = ctl.step(x, rho0.clone(), uo0.clone(), cfg, active_ws=T(ws).to(torch.int32))
    assert torch.equal(out["exitflag"], ref["exitflag"])
    assert torch.max(torch.abs(out["U"] - ref["U"])).item() <= U_TOL * cfg.umax


def test_closed_loop_bitwise_deterministic(ctl):
    """Two identical closed loops of the bench (B = 40000 scenarios, carried
    workspace, 10 steps) agree bit for bit: no result depends on LDS a launch
    did not write (a stale read of rinfo[-1] once made 5-50 scenarios differ)."""
    N, B, K = 20, 40000, 10
    cfg, _ = cfgs(N, 2)

    def loop():
        x = T(O.scenario_x0(np.arange(B)).T)
        rho, uo = ctl.initial_state(x, cfg)
        ws = ctl.new_active_ws(B, cfg)
        Us = []
        for _ in range(K):
            out = ctl.step(x, rho, uo, cfg, active_ws=ws)
            Us.append(out["U"].clone())
            x = out["x_next"].clone()
        return torch.stack(Us), rho.clone(), ws.clone()

    a, b = loop(), loop()
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_step_workspace_roundtrip_host(ctl):
    """ntm_mpc_step_ws (host buffers) == ntm_mpc_step_ws_device, workspace included."""
    N, B = 20, 32
    cfg, _ = cfgs(N, 2)
    x0 = np.ascontiguousarray(O.scenario_x0(np.arange(B)).T)
    rho, uo = ctl.initial_state(T(x0), cfg)
    ws = ctl.new_active_ws(B, cfg)
    rh, uh = H(rho).copy(), H(uo).copy()
    wh = np.full((2 * (N + 1), B), -1, np.int32)
    for _ in range(3):
        dv = ctl.step(T(x0), rho, uo, cfg, active_ws=ws)
        hs = ctl.step_host(x0, rh, uh, cfg, active_ws=wh)
        np.testing.assert_array_equal(hs["U"], H(dv["U"]))
        np.testing.assert_array_equal(wh, H(ws))
        x0 = np.ascontiguousarray(hs["x_next"])
    assert (wh[N] >= 0).all()                                          # slots hold active sets


def test_empty_batch_and_invalid_arguments(ctl):
    """B = 0 is a no-op; out-of-range N, an unknown mode, a non-finite du_max or
    a negative or non-finite Ru are API errors (NTM_E_INVALID with a message), not
    solver outcomes."""
    from ntm_mpc import NtmLibraryError
    N = 20
    cfg, _ = cfgs(N, 2)
    x = torch.empty(2, 0, dtype=torch.float64, device=DEV)
    rho, uo = ctl.initial_state(x, cfg)
    out = ctl.step(x, rho, uo, cfg)
    assert out["U"].shape == (N, 0) and out["exitflag"].shape == (0,)
    x1 = T(O.scenario_x0(np.arange(2)).T)
    for bad in (dict(N=0), dict(N=65), dict(mode=4), dict(mode=3, du_max=float("nan")), dict(Ru=-1e-10),
                dict(Ru=float("nan")), dict(Ru=float("inf"))):
        c = cfgs(bad.pop("N", N), bad.pop("mode", 2), **bad)[0]
        with pytest.raises(NtmLibraryError):
            r, u = ctl.initial_state(x1, c)
            ctl.step(x1, r, u, c)


@pytest.mark.parametrize("N,mode", [(20, 2), (50, 3)])
def test_full_size_batch_properties(ctl, N, mode):
    """BASELINE configs 3 (N = 20, full getWLc rows) and 5 (N = 50, + rate rows)
    at full size (B = 1e5), one step with the carried workspace, checked by
    size-independent properties:
      * every scenario is solved (exitflag 1) and its plan is feasible: U within
        [umin, umax] and the predicted states x^_1..x^_N within [xmin, xmax]
        (the getWLc rows), to 1e-9 relative;
      * a seeded sample of 64 scenarios matches the oracle (teacher-forced);
      * batch-composition invariance: the same 64 scenarios run as their own
        batch (on the same build) give bit-identical outputs (no cross-scenario
        coupling)."""
    import ntm_mpc
    B = 100_000
    cfg, ocfg = cfgs(N, mode)
    x = ntm_mpc.device_tensor(ntm_mpc.scenarios_x0(0, B))
    rho, uo = ctl.initial_state(x, cfg)
    ws = ctl.new_active_ws(B, cfg)
    out = ctl.step(x, rho, uo, cfg, active_ws=ws)             # step 1 fills the workspace
    x2, rho2, uo2, ws2 = out["x_next"].clone(), rho.clone(), uo.clone(), ws.clone()
    rho_in, uo_in = rho2.clone(), uo2.clone()
    out = ctl.step(x2, rho2, uo2, cfg, active_ws=ws2)        # the measured step
    flags = H(out["exitflag"])
    assert (flags == 1).all()
    U = H(out["U"])
    assert U.min() >= cfg.umin - 1e-9 * cfg.umax and U.max() <= cfg.umax * (1 + 1e-9)
    xp = H(out["x_pred"]).reshape(N + 1, 2, B)[1:]            # x^_1..x^_N
    for c in range(2):
        span = cfg.xmax[c] - cfg.xmin[c]
        assert xp[:, c].min() >= cfg.xmin[c] - 1e-9 * span and xp[:, c].max() <= cfg.xmax[c] + 1e-9 * span
    if mode == 3:                                             # rate rows |U_i - U_{i-1}| <= du_max
        assert np.max(np.abs(np.diff(U, axis=0))) <= cfg.du_max * (1 + 1e-9)
    ids = np.sort(np.random.default_rng(5).choice(B, 64, replace=False))
    xs, rs, us = H(x2)[:, ids], H(rho_in)[:, ids], H(uo_in)[:, ids]
    ref = cbind.step(np.ascontiguousarray(xs), np.ascontiguousarray(rs), np.ascontiguousarray(us), ocfg)
    same = H(out["inner_iters"])[ids] == ref["inner_iters"]
    assert same.mean() >= 0.9
    assert np.max(np.abs(U[:, ids] - ref["U"])[:, same]) / cfg.umax <= (U_TOL_RATE if mode == 3 else U_TOL)
    # the sub-batch takes the build the full batch took (the library picks the
    # N = 20 build by batch size, ntm_ctx_set_small_batch; bit for bit holds within a build)
    ctl.set_small_batch((1 << 62) if ctl.step_layout(B, cfg) == "lds" else 0)
    try:
        sub = ctl.step(T(xs), T(rs), T(us), cfg, active_ws=ws[:, ids].contiguous())
    finally:
        ctl.set_small_batch(-1)
    for k in ("U", "x_pred", "x_next", "exitflag", "inner_iters"):
        np.testing.assert_array_equal(H(sub[k]), H(out[k])[..., ids], err_msg=k)


def _collision_kind(Lin, act, N):
    """The long-horizon 'one collision' shapes: exactly one general row
    does not own the last free column it ends in (another row ends there too),
    with k = n_F - n_S = 0 (one free column where no row ends: kind 1) or k = 1
    (two such columns: kind 2); 0 for any other set."""
    nz = [np.nonzero(np.abs(Lin[r]) > 0)[0] for r in act]
    fixed = {int(c[0]) for c in nz if len(c) == 1}
    free = [j for j in range(N) if j not in fixed]
    gen = [c for c in nz if len(c) > 1]
    k = len(free) - len(gen)
    if k not in (0, 1) or not gen:
        return 0
    last = [max(j for j in c if j not in fixed) if any(j not in fixed for j in c) else -1 for c in gen]
    holes = [j for j in free if j not in last]
    if -1 in last or len(holes) != k + 1 or len(set(last)) != len(gen) - 1:
        return 0
    return 1 + k


def test_long_horizon_sets_vs_exact_kkt(ctl):
    """the N=50 re-solve paths (echelon k = 0 / 1, the one-collision
    echelon sets of config 5 with k = 0 and k = 1, the bordered elimination) checked against an exact
    (30-digit) KKT solve of the SAME active set the device certified.  One QP per
    launch (i_sim = 1) so the QP's data are the launch inputs; the device's
    active set is read back from its warm-start workspace.  The exact solve must
    certify the set (primal feasible, multipliers >= 0) and the device's U must
    match it to 1e-10 * umax; at least one set of each one-collision kind must be among them."""
    N, B, steps = 50, 16, 6
    cfg, ocfg = cfgs(N, 3, i_sim=1)
    ph = O.Physics()
    x = O.scenario_x0(np.arange(B)).T
    rho, Uo = cbind.initial_state(x, ocfg)
    ws = ctl.new_active_ws(B, cfg)
    n_coll = [0, 0, 0]
    n_checked = 0
    worst = 0.0
    for k in range(steps):
        tr, tu = T(rho), T(Uo)
        out = ctl.step(T(x), tr, tu, cfg, active_ws=ws)
        U, flag, wsh = H(out["U"]), H(out["exitflag"]), H(ws)
        for s in range(B):
            if flag[s] != 1:
                continue
            q = int(wsh[N, s])                              # slot 0: the launch's one QP
            act = [int(v) for v in wsh[:q, s]]
            Rho = rho[:, s].reshape(N, 3).T
            Phi, Gam, Lam = O.lift(Rho, ph, ocfg)
            G, F = O.cost(Phi, Gam, Lam, x[:, s], ocfg)
            Lin, b = O.constraints(Phi, Gam, Lam, x[:, s], ocfg)
            kind = _collision_kind(Lin, act, N)
            if k >= 2 and n_checked >= 12 and (kind == 0 or (kind == 1 and n_coll[1] >= 6)):
                continue                                    # keep the mpmath work bounded
            Ue, lam, cert = O.kkt_polish(G, F, Lin, b, act, dps=30)
            assert cert["max_violation"] <= 1e-9, (k, s, cert)
            assert cert["min_multiplier"] >= -1e-9 * max(1.0, np.max(np.abs(lam))), (k, s, cert)
            worst = max(worst, np.max(np.abs(U[:, s] - Ue)) / cfg.umax)
            n_checked += 1
            n_coll[kind] += 1
        x, rho, Uo = H(out["x_next"]), H(tr), H(tu)         # the device's own closed loop
    print(f"N=50 mode 3: {n_checked} sets checked, {n_coll[1]} one-collision (k = 0), {n_coll[2]} one-collision "
          f"(k = 1), max |U - U_exact| / umax = {worst:.2e}")
    assert n_checked >= 8 and n_coll[1] >= 1 and n_coll[2] >= 1, n_coll
    assert worst <= 1e-10, worst
