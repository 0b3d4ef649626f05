"""GPU tests of the resumable closed loops (ntm_mpc_run_from / ntm_mpc_run_est_from): the
fused closed-loop kernels with the controller state (x, rho, U_old, the two warm-start
sets; d_hat and x_hat for the estimator) carried in and out.

Tolerances are DESIGN.md §3's: free-running closed loops RUN_TOL = 5e-8 of umax on the
inputs and of the state's scale (0.15 m, 2000 pi rad/s) on the states; two kernels built
from the same phases agree on one step to 1e-12 relative (test_step_matches_run_first_step).
Chunk invariance is exact (torch.equal).
"""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

import resume_ref as R
from oracle import cbind
from oracle import ntm_oracle as O

pytestmark = pytest.mark.gpu

B, K = 9, 5
RUN_TOL = 5e-8
XS = np.array([0.15, 2000 * math.pi])
OGEN = O.ScenarioGen(seed=20241220, first_id=0, k0=2, sigma_w=1e-3, sigma_omega=0.0, jbs_spread=0.1, wdep_spread=0.1)
HIST = ("xk", "uk", "Uk", "wpred", "exitflag", "inner_iters")
EST_HIST = HIST + ("dk", "xhk", "yk")


def H(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def x0_of(n=B):
    return np.ascontiguousarray(O.scenario_x0(np.arange(n)).T)


def dev_gen(g, **kw):
    from ntm_mpc import ScenarioGen
    return None if g is None else ScenarioGen(**{**dataclasses.asdict(g), **kw})


def cfgs(N, mode, **kw):
    from ntm_mpc import Config
    return Config(N=N, mode=mode, **kw), O.Config(N=N, mode=mode, **kw)


def init_state(ctl, cfg, x0, gen):
    """[x, rho, U_old, active_ws] of a loop's first call: ntm_mpc_init's state, no candidates."""
    ctl.set_scenarios(dev_gen(gen))
    x = ctl.tensor(x0)
    rho, Uo = ctl.initial_state(x, cfg)
    return [x, rho, Uo, ctl.new_active_ws(x0.shape[1], cfg)]


def cat(hs):
    """Histories of consecutive chunks as one loop's: xk-like keys share a column."""
    out = {}
    for k in hs[0]:
        if k in ("xk", "dk", "xhk"):
            out[k] = torch.cat([hs[0][k]] + [h[k][2:] for h in hs[1:]])
        else:
            out[k] = torch.cat([h[k] for h in hs])
    return out


def chunked(ctl, cfgs_per_chunk, state, gen, chunks, est=None, after_chunk=None):
    """run_from (run_est_from with ``est``: one per chunk) over ``chunks`` steps each, the
    generator's k0 advanced by the steps done; ``state`` is updated in place."""
    hs, done = [], 0
    for i, n in enumerate(chunks):
        ctl.set_scenarios(dev_gen(gen, k0=gen.k0 + done) if gen is not None else None)
        if est is None:
            hs.append(ctl.run_from(*state, n, cfgs_per_chunk[i]))
        else:
            hs.append(ctl.run_est_from(*state, est[i], n, cfgs_per_chunk[i]))
        done += n
        if after_chunk:
            after_chunk(i)
    return cat(hs)


@pytest.fixture
def builds(ctl):
    """Restores the context's build thresholds, generator and counters after a test."""
    yield ctl
    ctl.set_small_batch(-1)
    ctl.set_one_wave_batch(-1)
    ctl.set_scenarios(None)
    ctl.set_stats(None)


def select(ctl, build):
    ctl.set_small_batch(0 if build == "far" else -1)
    ctl.set_one_wave_batch(0 if build == "lds" else -1)


# (id, N, mode, config extras, N = 20 build selection, step_build, step_kernel_name)
BUILDS = [
    ("n20-far", 20, 2, {}, "far", "far", "k_mpc_step<P=64,NN=20,far>"),
    ("n20-lds", 20, 2, {}, "lds", "lds", "k_mpc_step<P=64,NN=20,lds>"),
    ("n20-lds1", 20, 2, {}, "lds1", "lds1", "k_mpc_step<P=64,NN=20,lds> (one-wave budget)"),
    ("n50-m2", 50, 2, {}, None, "far", "k_mpc_step<P=64,NN=50,far>"),
    ("n50-m3", 50, 3, {}, None, "far", "k_mpc_step<P=64,NN=50,far>"),
    ("n10", 10, 2, {}, None, "lds", "k_mpc_step<P=16,NN=10,lds>"),
    ("n20-m3-generic", 20, 3, {}, None, "lds", "k_mpc_step<P=64,NN=0,lds>"),
    ("n6-m1-generic", 6, 1, {}, None, "lds", "k_mpc_step<P=16,NN=0,lds>"),
    ("n20-Ru-generic", 20, 2, {"Ru": 1e-9}, None, "lds", "k_mpc_step<P=64,NN=0,lds>"),
]


def _assert_same(a, b, keys, what):
    for k in keys:
        assert torch.equal(a[k], b[k]), (what, k)


# ------------------------------------------------------------ 1. chunk invariance
@pytest.mark.parametrize("case", BUILDS, ids=[c[0] for c in BUILDS])
def test_chunks_are_bit_identical(builds, case):
    """run_from(5) == run_from(2) then run_from(3) on every history, on the final x, rho,
    U_old and active_ws and on the stats counters, on the build the case names; the second
    chunk verifies carried candidates (stats row 4 > 0)."""
    ctl = builds
    _, N, mode, kw, sel, build, name = case
    cfg, _ = cfgs(N, mode, **kw)
    select(ctl, sel)
    assert ctl.step_build(B, cfg) == build and ctl.step_kernel_name(B, cfg) == name
    x0 = x0_of()
    st1 = torch.zeros(6, B, dtype=torch.int32, device="cuda")
    ctl.set_stats(st1)
    s1 = init_state(ctl, cfg, x0, OGEN)
    one = chunked(ctl, [cfg], s1, OGEN, [K])
    st2 = torch.zeros(6, B, dtype=torch.int32, device="cuda")
    ctl.set_stats(st2)
    s2 = init_state(ctl, cfg, x0, OGEN)
    snap = {}
    two = chunked(ctl, [cfg, cfg], s2, OGEN, [2, 3], after_chunk=lambda i: snap.setdefault(i, st2.clone()))
    _assert_same(one, two, HIST, case[0])
    for a, b, k in zip(s1, s2, ("x", "rho", "U_old", "active_ws")):
        assert torch.equal(a, b), (case[0], k)
    assert torch.equal(s1[0], one["xk"][-2:])
    assert torch.equal(st1, st2)
    assert int((st2[4] - snap[0][4]).sum()) > 0


def test_five_single_steps_on_the_far_build(builds):
    ctl = builds
    cfg, _ = cfgs(20, 2)
    select(ctl, "far")
    assert ctl.step_build(B, cfg) == "far"
    s1, s2 = init_state(ctl, cfg, x0_of(), OGEN), init_state(ctl, cfg, x0_of(), OGEN)
    one = chunked(ctl, [cfg], s1, OGEN, [K])
    five = chunked(ctl, [cfg] * K, s2, OGEN, [1] * K)
    _assert_same(one, five, HIST, "1+1+1+1+1")
    for a, b in zip(s1, s2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("sel", ["far", "lds1"])
def test_zero_steps_change_nothing(builds, sel):
    ctl = builds
    cfg, _ = cfgs(20, 2)
    select(ctl, sel)
    state = init_state(ctl, cfg, x0_of(), OGEN)
    chunked(ctl, [cfg], state, OGEN, [2])
    state[3][0, 0] = 77                       # not a valid set: must come back untouched, too
    before = [t.clone() for t in state]
    out = ctl.run_from(*state, 0, cfg)
    for a, b in zip(state, before):
        assert torch.equal(a, b)
    assert torch.equal(out["xk"], state[0]) and out["uk"].shape == (0, B)


# ------------------------------------------------------------ 2. against the oracle
def _closeness(g, ref, umax, k_sim):
    xs = np.tile(XS, k_sim + 1)[:, None]
    return {"uk": np.max(np.abs(g["uk"] - ref["uk"])) / umax, "Uk": np.max(np.abs(g["Uk"] - ref["Uk"])) / umax,
            "xk": np.max(np.abs(g["xk"] - ref["xk"]) / xs), "wpred": np.max(np.abs(g["wpred"] - ref["wpred"])) / 0.15}


def _assert_close(out, ref, umax, k_sim, what, tol=RUN_TOL):
    g = {k: H(out[k]) for k in HIST}
    figs = _closeness(g, ref, umax, k_sim)
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    for k, v in figs.items():
        assert v <= tol, (what, k, v)
    np.testing.assert_array_equal(g["exitflag"], ref["exitflag"])
    return g


ORACLE = [(10, None), (20, "far"), (20, "lds"), (50, None)]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("N,sel", ORACLE, ids=[f"N{n}-{s}" for n, s in ORACLE])
def test_run_from_init_matches_the_oracle(builds, N, sel, mode):
    """run_from from ntm_mpc_init's state against the C oracle's closed loop (generator
    attached), RUN_TOL; mandatory for the far N = 20 build."""
    ctl = builds
    cfg, ocfg = cfgs(N, mode)
    select(ctl, sel)
    if sel:
        assert ctl.step_build(B, cfg) == sel
    x0 = x0_of()
    ref = cbind.run(x0, ocfg, K, gen=OGEN)
    state = init_state(ctl, cfg, x0, OGEN)
    out = chunked(ctl, [cfg], state, OGEN, [K])
    _assert_close(out, ref, cfg.umax, K, f"run_from N={N} mode {mode} {sel}")
    assert np.all(ref["exitflag"] == 1)


# ------------------------------------------------------------ 3. against run
@pytest.mark.parametrize("sel", ["far", "lds", "lds1"])
def test_run_from_matches_run(builds, sel):
    """First step: flags and iteration counts equal, uk and xk to 1e-12 relative (two
    kernels from the same phases).  Whether five steps are bit-identical is printed."""
    ctl = builds
    cfg, _ = cfgs(20, 2)
    select(ctl, sel)
    x0 = x0_of()
    state = init_state(ctl, cfg, x0, OGEN)
    a = ctl.run(ctl.tensor(x0), K, cfg)
    b = ctl.run_from(*state, K, cfg)
    assert torch.equal(a["exitflag"][0], b["exitflag"][0]) and torch.equal(a["inner_iters"][0], b["inner_iters"][0])
    assert torch.max(torch.abs(a["uk"][0] - b["uk"][0])).item() <= 1e-12 * cfg.umax
    xs = torch.tensor(XS[:, None], dtype=torch.float64, device="cuda")
    assert torch.max(torch.abs(a["xk"][:4] - b["xk"][:4]) / xs.repeat(2, 1)).item() <= 1e-12
    same = {k: bool(torch.equal(a[k], b[k])) for k in HIST}
    print(f"run vs run_from, N=20 mode 2 {sel}, {K} steps bit-identical: {all(same.values())} {same}")


# ------------------------------------------------------------ 4. interop with step_ws
def test_state_continues_in_step_ws(builds):
    """The state out of run_from(2), continued by three step() calls with the carried
    workspace, against run_from(3) from the same state: flags and iteration counts equal,
    values to RUN_TOL."""
    ctl = builds
    cfg, _ = cfgs(20, 2)
    select(ctl, "far")
    state = init_state(ctl, cfg, x0_of(), OGEN)
    chunked(ctl, [cfg], state, OGEN, [2])
    sa = [t.clone() for t in state]
    og3 = dataclasses.replace(OGEN, k0=OGEN.k0 + 2)
    ref = chunked(ctl, [cfg], sa, og3, [3])
    x, rho, Uo, ws = (t.clone() for t in state)
    for k in range(3):
        ctl.set_scenarios(dev_gen(og3, k0=og3.k0 + k))
        r = ctl.step(x, rho, Uo, cfg, active_ws=ws)
        assert torch.equal(r["exitflag"], ref["exitflag"][k]) and torch.equal(r["inner_iters"], ref["inner_iters"][k])
        assert torch.max(torch.abs(r["U"] - ref["Uk"][k * 20:(k + 1) * 20])).item() <= RUN_TOL * cfg.umax
        x = r["x_next"]
        xs = torch.tensor(XS[:, None], dtype=torch.float64, device="cuda")
        assert torch.max(torch.abs(x - ref["xk"][2 * k + 2:2 * k + 4]) / xs).item() <= RUN_TOL


# ------------------------------------------------------------ 5. the feature in use
@pytest.mark.parametrize("N,sel", [(20, "far"), (20, "lds"), (10, None)])
def test_umax_halves_during_the_loop(builds, N, sel):
    """umax halves after step 2 (the nominal plant): against resume_ref at RUN_TOL, every
    flag 1, and at least half of the applied inputs after the change on the new bound."""
    ctl = builds
    cfg, ocfg = cfgs(N, 2)
    half, ohalf = dataclasses.replace(cfg, umax=cfg.umax / 2), dataclasses.replace(ocfg, umax=ocfg.umax / 2)
    select(ctl, sel)
    x0 = x0_of()
    ref, _ = R.run(x0, K, R.switch_at(2, (ocfg, None), (ohalf, None)))
    state = init_state(ctl, cfg, x0, None)
    out = chunked(ctl, [cfg, half], state, None, [2, 3])
    g = _assert_close(out, ref, cfg.umax, K, f"umax halving N={N} {sel}")
    assert np.all(g["exitflag"] == 1)
    late = g["uk"][2:]
    on_bound = np.abs(late - half.umax) <= 1e-9 * cfg.umax
    print(f"on the new bound: {on_bound.sum()} of {late.size}")
    assert 2 * on_bound.sum() >= late.size


# ------------------------------------------------------------ 6. run_est_from
GAIN, KAPPA, SIGMA_Y = (0.5, 0.2), (0.5, 0.25), (2.0 ** -10, 16.0)


def _est(**kw):
    from ntm_mpc import Estimator
    return Estimator(**{**dict(nominal_model=True, gain=GAIN, kappa=KAPPA, sigma_y=SIGMA_Y), **kw})


def init_est_state(ctl, cfg, x0, xh0=None, d0=None):
    """The estimator loop's first state under nominal_model: init with no generator, from x_hat."""
    n = x0.shape[1]
    ctl.set_scenarios(None)
    xh = ctl.tensor(x0 if xh0 is None else xh0)
    rho, Uo = ctl.initial_state(xh, cfg)
    d = ctl.tensor(np.zeros((2, n)) if d0 is None else d0)
    return [ctl.tensor(x0), rho, Uo, ctl.new_active_ws(n, cfg), d, xh]


@pytest.mark.parametrize("N,mode", [(20, 2), (6, 1)])
def test_est_chunks_are_bit_identical_and_match_run_est(builds, N, mode):
    ctl = builds
    cfg, _ = cfgs(N, mode)
    x0 = x0_of()
    xh0 = x0 + np.stack([1e-3 * np.cos(np.arange(B)), 10.0 * np.sin(np.arange(B))])
    s1, s2 = init_est_state(ctl, cfg, x0, xh0), init_est_state(ctl, cfg, x0, xh0)
    one = chunked(ctl, [cfg], s1, OGEN, [K], est=[_est()])
    two = chunked(ctl, [cfg] * 2, s2, OGEN, [2, 3], est=[_est()] * 2)
    _assert_same(one, two, EST_HIST, f"est N={N}")
    for a, b, k in zip(s1, s2, ("x", "rho", "U_old", "active_ws", "d_hat", "x_hat")):
        assert torch.equal(a, b), k
    assert torch.equal(s1[4], one["dk"][-2:]) and torch.equal(s1[5], one["xhk"][-2:])
    ctl.set_scenarios(dev_gen(OGEN))
    ref = ctl.run_est(ctl.tensor(x0), _est(), K, cfg, xhat0=ctl.tensor(xh0))
    xs, ys = np.tile(XS, K + 1)[:, None], np.tile(XS, K)[:, None]
    g, r = {k: H(one[k]) for k in EST_HIST}, {k: H(ref[k]) for k in EST_HIST}
    figs = _closeness(g, r, cfg.umax, K)
    figs.update(dk=np.max(np.abs(g["dk"] - r["dk"]) / xs), xhk=np.max(np.abs(g["xhk"] - r["xhk"]) / xs),
                yk=np.max(np.abs(g["yk"] - r["yk"]) / ys))
    print(f"run_est_from vs run_est N={N}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    for k, v in figs.items():
        assert v <= RUN_TOL, (k, v)
    np.testing.assert_array_equal(g["exitflag"], r["exitflag"])


@pytest.mark.parametrize("N,mode", [(20, 2), (6, 1)])
def test_degenerate_est_continues_run_obs(builds, N, mode):
    """sigma_y = 0, kappa = 0, equal gains, x_hat == x: run_obs(5) == run_est_from 2 + 3."""
    from ntm_mpc import Observer
    ctl = builds
    cfg, _ = cfgs(N, mode)
    x0 = x0_of()
    ctl.set_scenarios(dev_gen(OGEN))
    a = ctl.run_obs(ctl.tensor(x0), Observer(nominal_model=True, gain=0.5), K, cfg)
    state = init_est_state(ctl, cfg, x0)
    e = _est(gain=(0.5, 0.5), kappa=0.0, sigma_y=0.0)
    b = chunked(ctl, [cfg] * 2, state, OGEN, [2, 3], est=[e, e])
    _assert_same(a, b, HIST + ("dk",), f"obs N={N}")
    assert torch.equal(b["xhk"], b["xk"])


def test_sigma_y_switched_on_during_the_loop(builds):
    """sigma_y from 0 to its values at step 2, against resume_ref, RUN_TOL."""
    ctl = builds
    N = 6
    cfg, ocfg = cfgs(N, 1)
    x0 = x0_of()
    quiet = dict(nominal=True, gain=GAIN, kappa=KAPPA, sigma_y=0.0)
    noisy = dict(quiet, sigma_y=SIGMA_Y)
    rho, Uo = cbind.initial_state(x0, ocfg)
    ref, _ = R.run_est_from(x0, x0, rho, Uo, np.zeros((2, B)), K,
                            lambda k: (ocfg, OGEN, quiet if k < 2 else noisy))
    state = init_est_state(ctl, cfg, x0)
    out = chunked(ctl, [cfg] * 2, state, OGEN, [2, 3], est=[_est(sigma_y=0.0), _est()])
    g = {k: H(out[k]) for k in EST_HIST}
    xs, ys = np.tile(XS, K + 1)[:, None], np.tile(XS, K)[:, None]
    figs = _closeness(g, ref, cfg.umax, K)
    figs.update(dk=np.max(np.abs(g["dk"] - ref["dk"]) / xs), xhk=np.max(np.abs(g["xhk"] - ref["xhk"]) / xs),
                yk=np.max(np.abs(g["yk"] - ref["yk"]) / ys))
    print("sigma_y switch: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    for k, v in figs.items():
        assert v <= RUN_TOL, (k, v)
    np.testing.assert_array_equal(g["exitflag"], ref["exitflag"])
    assert np.array_equal(g["yk"][:4], g["xk"][2:6]) and np.all(g["yk"][4:] != g["xk"][6:])


# ------------------------------------------------------------ 7. arguments, host entry points
def test_arguments_are_validated(builds):
    ctl = builds
    cfg, _ = cfgs(20, 2)
    state = init_state(ctl, cfg, x0_of(), None)
    ph = C.byref(ctl.physics.to_c())
    ptr = [C.c_void_p(t.data_ptr()) for t in state]

    def raw(c=cfg, k=1, p=ptr):
        return ctl.lib.ntm_mpc_run_from_device(ctl._ctx, ph, C.byref(c.to_c()), B, k, *p, *([None] * 6), None)
    for i in range(4):
        assert raw(p=[None if j == i else q for j, q in enumerate(ptr)]) == -1
    assert raw(k=-1) == -1
    assert raw(c=dataclasses.replace(cfg, N=0)) == -1 and raw(c=dataclasses.replace(cfg, N=65)) == -1
    es = init_est_state(ctl, cfg, x0_of())
    eptr = [C.c_void_p(t.data_ptr()) for t in es]

    def raw_est(c=cfg, k=1, p=eptr, est=_est(sigma_y=0.0)):
        return ctl.lib.ntm_mpc_run_est_from_device(ctl._ctx, ph, C.byref(c.to_c()), C.byref(est.to_c()), B, k, *p,
                                                   *([None] * 9), None)
    for i in range(6):
        assert raw_est(p=[None if j == i else q for j, q in enumerate(eptr)]) == -1
    assert raw_est(k=-1) == -1 and raw_est(c=dataclasses.replace(cfg, N=65)) == -1
    assert raw_est(est=_est()) == -1          # sigma_y != 0 without a generator: run_est's own check
    with pytest.raises(ValueError):
        ctl.run_from(state[0], state[1], state[2], None, 1, cfg)
    torch.cuda.synchronize()
    before = [t.clone() for t in state]
    assert raw(k=0) == 0
    for a, b in zip(state, before):
        assert torch.equal(a, b)


def test_host_entry_points_match_device_on_the_far_build(builds):
    """The host-array forms stage through the context's stream and share the far build's
    HBM block with the caller's stream: bit-identical to the device forms, 2 + 3 steps."""
    ctl = builds
    cfg, _ = cfgs(20, 2)
    select(ctl, "far")
    x0 = x0_of()
    sd = init_state(ctl, cfg, x0, OGEN)
    sh = [np.asfortranarray(H(t)) for t in sd]
    for n, k0 in ((2, 2), (3, 4)):
        ctl.set_scenarios(dev_gen(OGEN, k0=k0))
        d = ctl.run_from(*sd, n, cfg)
        h = ctl.run_from_host(*sh, n, cfg)
        for k in HIST:
            np.testing.assert_array_equal(h[k], H(d[k]), err_msg=k)
        for a, b in zip(sh, sd):
            np.testing.assert_array_equal(a, H(b))
    ed = init_est_state(ctl, cfg, x0)
    eh = [np.asfortranarray(H(t)) for t in ed]
    ctl.set_scenarios(dev_gen(OGEN))
    d = ctl.run_est_from(*ed, _est(), 3, cfg)
    h = ctl.run_est_from_host(*eh, _est(), 3, cfg)
    for k in EST_HIST:
        np.testing.assert_array_equal(h[k], H(d[k]), err_msg=k)
    for a, b in zip(eh, ed):
        np.testing.assert_array_equal(a, H(b))
