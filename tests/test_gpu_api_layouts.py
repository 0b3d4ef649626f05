"""Every closed-loop entry point of NtmMpc, device and host form, called once with arguments
in the ABI's scenario-major layout and once with C-contiguous (E, B) copies of the same
values: every output is the same bit for bit, every in/out argument is updated in the
caller's own array to the same bits, the returned dict has its keys in the documented order
and carries the caller's own d_hat / x_hat / u_queue objects.  A wrong shape and a wrong
dtype raise ValueError with the documented text.  N = 10, mode 2, B = 3, k_sim = 3, a
generator with a disturbance, sigma_y != 0 and a dead time of 2 steps: the smallest shapes
at which the two layouts differ for every argument, the queue included.
"""
import numpy as np
import pytest

N, B, K, STEPS = 10, 3, 3, 2

STEP = ["U", "x_pred", "x_next", "exitflag", "inner_iters"]
STEP_EST = ["U", "x_pred", "x_next", "y", "exitflag", "inner_iters", "d_hat", "x_hat"]
STEP_DLY = ["U", "x_pred", "x_next", "y", "x_plan", "u_applied", "exitflag", "inner_iters", "d_hat", "x_hat", "u_queue"]
RUN = ["xk", "uk", "Uk", "wpred", "exitflag", "inner_iters"]
RUN_OBS = ["xk", "uk", "Uk", "wpred", "dk", "exitflag", "inner_iters"]
RUN_EST = ["xk", "uk", "Uk", "wpred", "dk", "xhk", "yk", "exitflag", "inner_iters"]
RUN_DLY = ["xk", "uk", "Uk", "wpred", "dk", "xhk", "yk", "uak", "xpk", "exitflag", "inner_iters"]

# entry: (positional arguments, keyword arguments, the dict's keys, in/out arrays, the name the first array is
# reported under, the argument given a wrong dtype); "@name" stands for the array of that name
ENTRIES = {
    "step": (["@x", "@rho", "@U_old", "cfg"], {"active_ws": "@active_ws"}, STEP, ["rho", "U_old", "active_ws"], "x_k",
             "active_ws"),
    "step_dual": (["@x", "@rho", "@U_old", "cfg"], {"active_ws": "@active_ws"}, STEP + ["lambda", "rho_qp"],
                  ["rho", "U_old", "active_ws"], "x_k", "active_ws"),
    "step_obs": (["@x", "@rho", "@U_old", "@d_hat", "obs", "cfg"], {"active_ws": "@active_ws"}, STEP + ["d_hat"],
                 ["rho", "U_old", "active_ws", "d_hat"], "x_k", "active_ws"),
    "step_est": (["@x", "@rho", "@U_old", "@d_hat", "@x_hat", "est", "cfg"], {"active_ws": "@active_ws"}, STEP_EST,
                 ["rho", "U_old", "active_ws", "d_hat", "x_hat"], "x_k", "active_ws"),
    "step_dly": (["@x", "@rho", "@U_old", "@d_hat", "@x_hat", "@u_queue", "est", "dly", "cfg"],
                 {"active_ws": "@active_ws"}, STEP_DLY, ["rho", "U_old", "active_ws", "d_hat", "x_hat", "u_queue"], "x_k",
                 "active_ws"),
    "run": (["@x", "k", "cfg"], {}, RUN, [], "x0", "x"),
    "run_obs": (["@x", "obs", "k", "cfg"], {"d0": "@d0"}, RUN_OBS, [], "x0", "d0"),
    "run_est": (["@x", "est", "k", "cfg"], {"d0": "@d0", "xhat0": "@xhat0"}, RUN_EST, [], "x0", "xhat0"),
    "run_dly": (["@x", "est", "dly", "k", "cfg"], {"d0": "@d0", "xhat0": "@xhat0", "uq0": "@uq0"}, RUN_DLY, [], "x0",
                "uq0"),
    "run_from": (["@x", "@rho", "@U_old", "@active_ws", "k", "cfg"], {}, RUN, ["x", "rho", "U_old", "active_ws"], "x",
                 "active_ws"),
    "run_est_from": (["@x", "@rho", "@U_old", "@active_ws", "@d_hat", "@x_hat", "est", "k", "cfg"], {}, RUN_EST,
                     ["x", "rho", "U_old", "active_ws", "d_hat", "x_hat"], "x", "active_ws"),
    "run_dly_from": (["@x", "@rho", "@U_old", "@active_ws", "@d_hat", "@x_hat", "@u_queue", "est", "dly", "k", "cfg"], {},
                     RUN_DLY, ["x", "rho", "U_old", "active_ws", "d_hat", "x_hat", "u_queue"], "x", "active_ws"),
}
ROWS = {"x": 2, "rho": 3 * N, "U_old": N, "active_ws": 2 * (N + 1), "d_hat": 2, "x_hat": 2, "u_queue": STEPS, "d0": 2,
        "xhat0": 2, "uq0": STEPS}


def _opts():
    from ntm_mpc import Config, Delay, Estimator, Observer
    return {"cfg": Config(N=N, mode=2), "obs": Observer(True, 0.5), "k": K, "dly": Delay(steps=STEPS),
            "est": Estimator(True, (0.5, 0.25), (0.3, 0.6), (1e-4, 2.0))}


@pytest.fixture(scope="module")
def base(ctl):
    """The values every case starts from, host arrays: the controller state after one warm step
    (rho, U_old and a filled active_ws), estimates off the truth and a queue under way."""
    from ntm_mpc import ScenarioGen, scenarios_x0
    cfg = _opts()["cfg"]
    x0 = ctl.tensor(scenarios_x0(0, B))
    rho, U_old = ctl.initial_state(x0, cfg)
    ws = ctl.new_active_ws(B, cfg)
    x = ctl.step(x0, rho, U_old, cfg, active_ws=ws)["x_next"]
    s = np.arange(B)
    v = {"x": x.cpu().numpy(), "rho": rho.cpu().numpy(), "U_old": U_old.cpu().numpy(), "active_ws": ws.cpu().numpy()}
    v["d_hat"] = v["d0"] = np.stack([1e-5 * np.cos(s), 0.3 * np.sin(s)])
    v["x_hat"] = v["xhat0"] = v["x"] * 1.01
    v["u_queue"] = v["uq0"] = 2e5 + 1.1e5 * np.arange(STEPS)[:, None] + 7e3 * s[None, :]
    gen = ScenarioGen(seed=7, first_id=3, k0=2, sigma_w=1e-4, sigma_omega=5.0, jbs_spread=0.05, wdep_spread=0.04)
    return {k: np.array(a) for k, a in v.items()}, gen


def _arrays(ctl, vals, dev, abi, override=None):
    """Fresh copies of the values as device tensors or host arrays, scenario-major (the
    ABI's) or C-contiguous."""
    import torch
    out = {}
    for k, a in dict(vals, **(override or {})).items():
        if dev:
            t = torch.tensor(np.ascontiguousarray(a), device=f"cuda:{ctl.device}")
            out[k] = t.T.contiguous().T if abi else t
        else:
            out[k] = np.array(a, order="F" if abi else "C")        # a copy, whatever a's own order
        assert out[k].shape[0] >= 2 and out[k].shape[1] >= 2
    return out


def _call(ctl, entry, dev, a):
    pos, kw = ENTRIES[entry][:2]
    o = _opts()
    get = lambda s: a[s[1:]] if s.startswith("@") else o[s]      # noqa: E731
    return getattr(ctl, entry + ("" if dev else "_host"))(*[get(s) for s in pos], **{k: get(s) for k, s in kw.items()})


def _bits(v):
    return np.ascontiguousarray(v if isinstance(v, np.ndarray) else v.cpu().numpy()).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("dev", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_entry_point_is_layout_blind(ctl, base, entry, dev):
    from ntm_mpc.api import is_scenario_major
    vals, gen = base
    keys, inout = ENTRIES[entry][2:4]
    ctl.set_scenarios(gen)
    try:
        a_abi, a_c = _arrays(ctl, vals, dev, True), _arrays(ctl, vals, dev, False)
        for k in a_c:
            assert is_scenario_major(a_abi[k]) and not is_scenario_major(a_c[k]), k
        o_abi, o_c = _call(ctl, entry, dev, a_abi), _call(ctl, entry, dev, a_c)
    finally:
        ctl.set_scenarios(None)
    for o, a in ((o_abi, a_abi), (o_c, a_c)):
        assert list(o) == keys
        for k in ("d_hat", "x_hat", "u_queue"):
            if k in keys:
                assert o[k] is a[k], k                            # the caller's own objects
    for k in keys:
        assert type(o_abi[k]) is type(a_abi["x"]), k
        if k not in a_c:                                          # a new array: in the ABI layout
            assert is_scenario_major(o_abi[k]) and is_scenario_major(o_c[k]), k
        assert o_abi[k].shape == o_c[k].shape and o_abi[k].dtype == o_c[k].dtype, k
        assert _bits(o_abi[k]) == _bits(o_c[k]), k
    for k in inout:                                               # updated in the caller's own array, either layout
        assert _bits(a_abi[k]) == _bits(a_c[k]), k
        assert not is_scenario_major(a_c[k]), k
    for k in [k for k in ("rho", "U_old") if k in inout]:         # and updated at all
        assert _bits(a_abi[k]) != _bits(np.asfortranarray(vals[k])), k
    for k in set(a_c) - set(inout):                               # pure inputs are left alone
        assert _bits(a_c[k]) == _bits(np.ascontiguousarray(vals[k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("dev", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_entry_point_argument_errors(ctl, base, entry, dev):
    """A wrong shape (the first array, a row too many where that keeps B) and a wrong dtype
    raise ValueError with the validator's text, before anything is launched."""
    import torch
    vals, _ = base
    first, dt_arg = ENTRIES[entry][4:6]
    cases = []
    x3 = np.concatenate([vals["x"], vals["x"][:1]])
    cases.append(({"x": x3}, f"{first} must have shape (2, {B}), got (3, {B})" if dev
                  else f"{first}: expected float64 (2, {B})"))
    if "rho" in ENTRIES[entry][3]:
        cases.append(({"rho": vals["rho"][:-1]}, f"rho must have shape ({3 * N}, {B}), got ({3 * N - 1}, {B})" if dev
                      else f"rho: expected float64 ({3 * N}, {B})"))
    name = first if dt_arg == "x" else dt_arg
    if dt_arg == "active_ws":
        cases.append(({dt_arg: vals[dt_arg].astype(np.float64)}, f"{name} must be torch.int32, got torch.float64" if dev
                      else f"{name}: expected int32 ({ROWS[dt_arg]}, {B})"))
    else:
        cases.append(({dt_arg: vals[dt_arg].astype(np.float32)}, f"{name} must be torch.float64, got torch.float32"
                      if dev else f"{name}: expected float64 ({ROWS[dt_arg]}, {B})"))
    for override, text in cases:
        with pytest.raises(ValueError) as e:
            _call(ctl, entry, dev, _arrays(ctl, vals, dev, True, override))
        assert str(e.value) == text
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_step_reuses_out_and_checks_it(ctl, base):
    """step(..., out=): a dict from an earlier step() is filled again and returned, the same
    arrays in it, with the bits of a fresh call; an array of another shape or layout in it
    raises ValueError before the launch."""
    import torch
    vals, _ = base
    cfg = _opts()["cfg"]
    a, b = _arrays(ctl, vals, True, True), _arrays(ctl, vals, True, True)
    fresh = ctl.step(a["x"], a["rho"], a["U_old"], cfg, active_ws=a["active_ws"])
    old = ctl.step(b["x"], b["rho"], b["U_old"], cfg)            # another step's results, to be overwritten
    held = dict(old)
    b = _arrays(ctl, vals, True, True)
    again = ctl.step(b["x"], b["rho"], b["U_old"], cfg, out=old, active_ws=b["active_ws"])
    assert again is old and list(again) == STEP
    for k in STEP:
        assert again[k] is held[k], k
        assert _bits(again[k]) == _bits(fresh[k]), k
    for k in ("rho", "U_old", "active_ws"):
        assert _bits(a[k]) == _bits(b[k]), k
    for k, wrong, shp in (("U", torch.empty(B, N + 1, dtype=torch.float64, device=old["U"].device).T, (N, B)),
                          ("x_pred", old["x_pred"].contiguous(), (2 * (N + 1), B)),
                          ("x_next", old["x_next"][:, :2], (2, B))):
        with pytest.raises(ValueError) as e:
            ctl.step(b["x"], b["rho"], b["U_old"], cfg, out=dict(old, **{k: wrong}))
        assert str(e.value) == f"out[{k!r}] must be a {shp} array from an earlier step()"
    torch.cuda.synchronize()
