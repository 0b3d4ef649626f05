#!/usr/bin/env python
"""Every output of the closed-loop entry points, device and host forms, on fixed small
inputs, for a byte-for-byte comparison of two builds of the library (a refactor against
its parent commit).

    NTM_MPC_LIB=PARENT/libntm_mpc.so python tools/dump_entrypoints.py dump parent.npz
    python tools/dump_entrypoints.py dump change.npz
    python tools/dump_entrypoints.py compare parent.npz change.npz [--out RECORD.txt]

`dump` calls step_ws, step_dual, step_obs, run_obs, step_est, run_est, run, run_from,
run_est_from, step_dly, run_dly and run_dly_from through ntm_mpc.api (the library is the one NTM_MPC_LIB names, as for every
tool here) and writes each output array under "<case>/<entry>/<dev|host>/<name>".  Cases:
k_sim = 5; a partial last block (B no multiple of 64 / lanes); lanes 16 (N = 10) and 64
(N = 33, the runtime-N kernels), 32 when the process runs under NTM_LANES=32 (N = 24: run
`dump` once more under it, into a file of its own); N = 20 steered onto the far, the
all-LDS and the one-wave build; N = 50 in modes 2 and 3; modes 0, 2 and 3; a generator
with a plasma spread and a disturbance; the observer nominal and per scenario; the
estimator with sigma_y != 0; a dead time of 2 steps with and without the delay-compensating
plan; active_ws from the previous step, then with one slot made invalid (an id out of range);
the stats counters attached; k_sim = 0 for the _from forms.  One small case runs a second
time ("<case>_c") with every array argument handed over C-contiguous, not in the ABI's
layout, which drives the binding's staged copies and copy-backs.
`compare` compares every array and writes one line per case (its entries, array and byte
counts), then ALL IDENTICAL, or the arrays that differ (exit 1).
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "mpc-ntm-control_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

K = 5
# name, N, B, mode, (small_batch, one_wave_batch) or None
CASES = [("n10_m0", 10, 7, 0, None), ("n10_m2", 10, 7, 2, None), ("n10_m3", 10, 7, 3, None),
         ("n33_m2", 33, 3, 2, None), ("n33_m3", 33, 3, 3, None),
         ("n20_far", 20, 70, 2, (0, 0)), ("n20_near", 20, 70, 2, (1000, 0)), ("n20_near1w", 20, 70, 2, (1000, 1000)),
         ("n20_m3", 20, 5, 3, None), ("n50_m2", 50, 5, 2, None), ("n50_m3", 50, 5, 3, None)]
CASES32 = [("n24_p32_m2", 24, 3, 2, None), ("n24_p32_m3", 24, 3, 3, None)]      # under NTM_LANES=32
CASE_C = ("n10_m2", 10, 7, 2, None)                                              # once more, C-contiguous arguments


def host(t):
    """A device (E, B) tensor as the host array of the same layout."""
    import torch
    return t if not isinstance(t, torch.Tensor) else np.asfortranarray(t.cpu().numpy())


def dump_case(ctl, name, N, B, mode, steer, dev, out, abi=True):
    import torch
    from ntm_mpc import Config, Delay, Estimator, Observer, ScenarioGen, scenarios_x0
    cfg = Config(N=N, mode=mode)
    ctl.set_small_batch(*([steer[0]] if steer else []))
    ctl.set_one_wave_batch(*([steer[1]] if steer else []))
    ctl.set_scenarios(ScenarioGen(seed=7, first_id=3, k0=2, sigma_w=1e-4, sigma_omega=5.0, jbs_spread=0.05,
                                  wdep_spread=0.04))
    stats = torch.zeros(6, B, dtype=torch.int32, device=f"cuda:{ctl.device}")
    ctl.set_stats(stats)
    form = "dev" if dev else "host"
    # an (E, B) array in the layout under test: the ABI's (a no-op for what the API returns) or C-contiguous
    if dev:
        lay = (lambda t: t) if abi else (lambda t: t.contiguous())
    else:
        lay = np.asfortranarray if abi else np.ascontiguousarray
    arr = (lambda a: lay(ctl.tensor(a))) if dev else (lambda a: lay(np.asarray(a, dtype=float)))
    sfx = "" if dev else "_host"
    if not abi:
        name += "_c"

    def put(entry, d):
        for k, v in d.items():
            out[f"{name}/{entry}/{form}/{k}"] = np.ascontiguousarray(host(v))

    def state():
        x = ctl.tensor(scenarios_x0(0, B))
        rho, Uo = ctl.initial_state(x, cfg)
        ws = ctl.new_active_ws(B, cfg)
        s = [x, rho, Uo, ws]
        return [lay(t) for t in (s if dev else [host(t) for t in s])]

    def steps(entry, call, extra):
        # three steps: no candidates, the previous step's, then scenario 1's first slot made invalid
        x, rho, Uo, ws = state()
        for i in range(3):
            if i == 2:
                ws[0, 1], ws[N, 1] = 10 ** 6, 1
            o = call(x, rho, Uo, *extra, cfg=cfg, active_ws=ws)
            put(f"{entry}{i}", dict(o, rho=rho, U_old=Uo, active_ws=ws))
            x = lay(o["x_next"])

    d2 = lambda v: arr(np.full((2, B), v))                                       # noqa: E731
    est = Estimator(True, (0.5, 0.25), (0.3, 0.6), (1e-4, 2.0))
    steps("step_ws", getattr(ctl, "step" + sfx), ())
    steps("step_dual", getattr(ctl, "step_dual" + sfx), ())
    for tag, obs in (("nom", Observer(True, 0.5)), ("scn", Observer(False, 0.25))):
        steps(f"step_obs_{tag}", getattr(ctl, "step_obs" + sfx), (d2(1e-4), obs))
        put(f"run_obs_{tag}", getattr(ctl, "run_obs" + sfx)(state()[0], obs, K, cfg, d0=d2(-1e-4)))
    x0 = state()[0]
    uq = lambda: arr(2e5 + 1.1e5 * np.arange(2)[:, None] + 7e3 * np.arange(B)[None, :])   # noqa: E731
    steps("step_est", getattr(ctl, "step_est" + sfx), (d2(1e-4), lay(x0 * 1.01), est))
    put("run_est", getattr(ctl, "run_est" + sfx)(x0, est, K, cfg, d0=d2(-1e-4), xhat0=lay(x0 * 0.99)))
    put("run", getattr(ctl, "run" + sfx)(x0, K, cfg))
    froms = [("run_from", "run_from", (), ()), ("run_est_from", "run_est_from", (d2(1e-4), lay(x0 * 1.01)), (est,))]
    for tag, dly in (("p", Delay(2, True)), ("n", Delay(2, False))):
        steps(f"step_dly_{tag}", getattr(ctl, "step_dly" + sfx), (d2(1e-4), lay(x0 * 1.01), uq(), est, dly))
        put(f"run_dly_{tag}", getattr(ctl, "run_dly" + sfx)(x0, est, dly, K, cfg, d0=d2(-1e-4), xhat0=lay(x0 * 0.99),
                                                            uq0=uq()))
        froms.append(("run_dly_from", f"run_dly_from_{tag}", (d2(1e-4), lay(x0 * 1.01), uq()), (est, dly)))
    for entry, tag, carried, opts in froms:
        s = state() + list(carried)
        for i, k in enumerate((2, 0, K - 2)):                                    # chunks, k_sim = 0 among them
            o = getattr(ctl, entry + sfx)(*s, *opts, k, cfg)
            put(f"{tag}{i}", dict(o, **{f"state{j}": t for j, t in enumerate(s)}))
    torch.cuda.synchronize()
    out[f"{name}/stats/{form}"] = stats.cpu().numpy()
    ctl.set_stats(None)


def dump(path):
    import ctypes as C
    from ntm_mpc import NtmMpc
    ctl = NtmMpc(device=0)
    lanes, nn = C.c_int32(), C.c_int32()
    ctl.lib.ntm_step_launch_info(24, C.byref(lanes), C.byref(nn))
    out = {}
    for case in (CASES32 if lanes.value == 32 else CASES):
        for dev in (True, False):
            dump_case(ctl, *case, dev, out)
        print(case[0], "done", flush=True)
    if lanes.value != 32:
        for dev in (True, False):
            dump_case(ctl, *CASE_C, dev, out, abi=False)
        print(CASE_C[0] + "_c", "done", flush=True)
    ctl.close()
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


def compare(a_path, b_path, record):
    a, b = np.load(a_path), np.load(b_path)
    # one line per case: its entries (dev and host forms together) with their array counts
    lines, bad, groups = [f"# {Path(a_path).name} against {Path(b_path).name}"], [], {}
    if set(a.files) != set(b.files):
        bad.append("array names differ: " + " ".join(sorted(set(a.files) ^ set(b.files))))
    for k in sorted(set(a.files) & set(b.files)):
        same = a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        case, entry = k.split("/")[:2]
        g = groups.setdefault(case, {}).setdefault(entry, [0, 0])
        g[0] += 1
        g[1] += a[k].nbytes
        if not same:
            bad.append(k)
    n = 0
    for case, entries in groups.items():
        diff = [k for k in bad if k.startswith(case + "/")]
        n += sum(c for c, _ in entries.values())
        lines.append(f"{case}: " + " ".join(f"{e}:{c}" for e, (c, _) in entries.items()) +
                     f" = {sum(c for c, _ in entries.values())} arrays, {sum(b_ for _, b_ in entries.values())} bytes, " +
                     ("array-equal (bytes)" if not diff else f"{len(diff)} DIFFER"))
    lines.append("ALL IDENTICAL" if not bad else "DIFFERENT: " + "; ".join(bad))
    text = "\n".join(lines) + "\n"
    if record:
        Path(record).parent.mkdir(parents=True, exist_ok=True)
        Path(record).write_text(text)
    print(f"{n} arrays compared")
    print(lines[-1])
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("dump").add_argument("npz")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    c.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.cmd == "dump":
        dump(a.npz)
        return 0
    return compare(a.a, a.b, a.out)


if __name__ == "__main__":
    sys.exit(main())
