"""bench.py's command line: --dump-outputs writes what the timed path returned, a plain run
prints the headline only, --full adds the rest."""
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench


def test_dump_outputs_writes_float32_arrays(tmp_path):
    a = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    b = torch.ones(5, dtype=torch.float16)
    bench.dump_outputs(str(tmp_path / "out"), {"a": a, "b": b})
    got = np.load(tmp_path / "out" / "a.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3, 4)
    assert np.array_equal(got, a.numpy().astype(np.float32))
    assert np.load(tmp_path / "out" / "b.npy").dtype == np.float32


def test_dump_outputs_samples_past_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 64 << 10)
    big = torch.arange(100_000, dtype=torch.float32)
    small = torch.arange(1_000, dtype=torch.float32) + 0.5
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    total = sum(os.path.getsize(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one"))
    assert total <= 64 << 10
    one, two = np.load(tmp_path / "one" / "big.npy"), np.load(tmp_path / "two" / "big.npy")
    assert np.array_equal(one, two)                       # the same sample every run
    assert one.ndim == 1 and 1_000 < one.size < 100_000
    assert np.all(np.diff(one) > 0)                       # elements of the array, in order
    s = np.load(tmp_path / "one" / "small.npy")
    assert 0 < s.size < 1_000 and np.all((s - 0.5) % 1 == 0)


def test_options_default_off(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "d"


def _run(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.main()
    return json.loads(buf.getvalue().strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_frames(tmp_path, monkeypatch):
    """A 96^2 frame (several 10-row tiles, the last one ragged) through bench.main() twice: the
    line has the headline keys and none of the --full legs; the dumped frames are what the step
    returned, [1, 96, 96, 4] float32, and equal between the runs (seeded inputs; 1e-6 allows a
    last-bit difference only)."""
    argv = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--size", "96"]
    lines, frames = [], []
    for d in ("one", "two"):
        lines.append(_run(monkeypatch, argv + ["--dump-outputs", str(tmp_path / d)]))
        assert os.listdir(tmp_path / d) == ["frames.npy"]
        frames.append(np.load(tmp_path / d / "frames.npy"))
    line = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in line, k
    assert line["steps"] == 2 and line["warmup"] == 1 and line["dtype"] == "fp32"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 96 * 96 * 64 / (line["ms_per_step"] / 1e3)) / line["value"] < 1e-6
    assert line["roofline"]["launches"] == 2              # --steps sets the timed steps
    for k in ("cpu_baseline", "fp16", "mixed", "fp32_split", "train", "api_paths", "scan_free"):
        assert k not in line, k
    a, b = frames
    assert a.dtype == np.float32 and a.shape == (1, 96, 96, 4)
    assert np.isfinite(a).all() and a.max() > 0           # some rays hit
    diff = float(np.abs(a - b).max())
    print(f"run-to-run max|diff| = {diff:.3e}")
    assert diff <= 1e-6
