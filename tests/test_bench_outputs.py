"""bench.py --dump-outputs and --full: a plain run times its steps, writes the last
timed step's outputs when asked and prints the headline line; the legs that take
runs of their own (gather_verify, disturbed, cpu_baseline) are behind --full."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402

NAMES = ("U", "x_pred", "x_next", "exitflag", "inner_iters")


def _step_out(B, N):
    import torch
    g = torch.Generator().manual_seed(1)
    return {"U": torch.randn(B, N, generator=g, dtype=torch.float64).T,          # (E, B) views, as the record's
            "x_pred": torch.randn(B, 2 * (N + 1), generator=g, dtype=torch.float64).T,
            "x_next": torch.randn(B, 2, generator=g, dtype=torch.float64).T,
            "exitflag": torch.ones(B, dtype=torch.int32),
            "inner_iters": torch.arange(B, dtype=torch.int32)}


def test_dump_outputs_whole_batch(tmp_path):
    B, N = 7, 4
    out = _step_out(B, N)
    bench.dump_outputs(out, tmp_path / "d")
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == sorted([f"{k}.npy" for k in NAMES]
                                                                        + ["scenario_ids.npy"])
    for k in NAMES:
        a = np.load(tmp_path / "d" / f"{k}.npy")
        assert a.dtype == np.float64 and a.shape == tuple(out[k].shape)
        assert np.array_equal(a, out[k].double().numpy())
    assert np.array_equal(np.load(tmp_path / "d" / "scenario_ids.npy"), np.arange(B, dtype=np.float64))


def test_dump_outputs_samples_past_the_budget(tmp_path, monkeypatch):
    """Past the byte budget a fixed, seeded sample of the scenarios is written: the
    same ids on every call, ascending, every array cut to them, total under budget."""
    B, N = 50, 4
    out = _step_out(B, N)
    per_scenario = 8 * (1 + N + 2 * (N + 1) + 2 + 1 + 1)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 11 * per_scenario + 5)
    bench.dump_outputs(out, tmp_path / "a")
    bench.dump_outputs(out, tmp_path / "b")
    ids = np.load(tmp_path / "a" / "scenario_ids.npy")
    assert ids.shape == (11,) and np.all(np.diff(ids) > 0) and ids[0] >= 0 and ids[-1] < B
    total = 0
    for k in list(NAMES) + ["scenario_ids"]:
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert np.array_equal(a, b)
        total += a.nbytes
    assert total <= 11 * per_scenario + 5
    for k in NAMES:
        assert np.array_equal(np.load(tmp_path / "a" / f"{k}.npy"), out[k].double().numpy()[..., ids.astype(int)])


def test_plain_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not a.full and a.dump_outputs is None and a.steps == 3
    a = bench.parse(["--full", "--dump-outputs", "x"])
    assert a.full and a.dump_outputs == "x"


def _bench_line(monkeypatch, capsys, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    assert bench.main() == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_reproducible_outputs(tmp_path, monkeypatch, capsys):
    """Two plain runs with the same arguments write bit-identical outputs (the inputs
    are counter-based), every array has the step entry point's shape and finite
    values, the nominal loop's exit flags are optimal, and the line carries the
    headline entries and none of the --full legs."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    B, N, K = 300, 20, 2
    argv = ["--gpus", "1", "--steps", str(K), "--warmup", "1", "--batch", str(B)]
    d = _bench_line(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "a")])
    _bench_line(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "b")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d
    assert d["steps"] == K and d["ms_per_step"] > 0 and d["dtype"] == "f64"
    assert d["value"] == pytest.approx(B * 1e3 / d["ms_per_step"], rel=1e-9)
    assert d["gather_verify"] is None and "disturbed" not in d and "cpu_baseline" not in d
    shapes = {"U": (N, B), "x_pred": (2 * (N + 1), B), "x_next": (2, B), "exitflag": (B,), "inner_iters": (B,)}
    for k, shp in shapes.items():
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert a.dtype == np.float64 and a.shape == shp and np.isfinite(a).all()
        assert np.array_equal(a, b), k
    assert (np.load(tmp_path / "a" / "exitflag.npy") == 1).all()


@pytest.mark.gpu
def test_full_run_keeps_its_legs(monkeypatch, capsys):
    """--full (CPU leg skipped to stay quick) still recomputes the record's sample
    bit for bit and runs the disturbed leg."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = _bench_line(monkeypatch, capsys, ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "300",
                                          "--full", "--no-cpu", "--verify", "16"])
    assert d["gather_verify"]["bitwise_equal"] and d["gather_verify"]["scenarios"] == 16
    assert d["disturbed"]["ms_per_step"] > 0 and "cpu_baseline" not in d
