"""bench.py's plain run on the GPU (a tiny CMX-B0 step, in this process): the result line holds
the headline fields for exactly --steps timed steps and none of --full's measurements, and
--dump-outputs writes the last timed step's loss / gradients / weights, equal for equal
arguments whatever the warm-up and settle phases ran before the timed window."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--backbone", "mit_b0", "--height", "64", "--width", "96", "--batch", "2", "--classes", "9",
        "--steps", "3"]


def _run(monkeypatch, capsys, out, warmup, settle_s):
    import bench
    monkeypatch.setenv("CMX_BENCH_SETTLE_S", settle_s)
    monkeypatch.setenv("CMX_BENCH_SETTLE_MAX_S", "0.2")
    monkeypatch.delenv("CMX_BENCH_TRACE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + ARGS + ["--warmup", str(warmup), "--dump-outputs", str(out)])
    capsys.readouterr()
    bench.main()
    lines = [json.loads(s) for s in capsys.readouterr().out.splitlines() if s.startswith("{")]
    assert len(lines) == 1
    return lines[0], {k: np.load(os.path.join(out, k + ".npy")) for k in ("loss", "grad", "param")}


def test_plain_run_line_and_reproducible_outputs(dev, tmp_path, monkeypatch, capsys):
    """Two plain runs with 1 warm-up step and no settle phase, and with 4 warm-up steps and a
    settle phase of at least 10 replays.  Bounds: the same steps from the same state differ at most
    by the order of fp32 atomic additions (~1e-6 relative per sum); a timed window that started
    from another state draws other DropPath masks and differs by O(1) of the gradient's scale, so
    1e-5 of the loss and 1e-3 of the largest gradient / weight separate the two."""
    line, a = _run(monkeypatch, capsys, tmp_path / "a", 1, "0")
    assert line["steps"] == 3 and line["warmup"] == 1 and line["replay_ms"]["timed"]["n"] == 3
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 2 * 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]
    assert line["roofline"] is None and line["families_in_step"] is None and line["cpu_baseline"] is None
    assert line["replay_ms"]["host_enqueue_idle_queue"] == [] and line["replay_ms"]["settle"]["replays"] == 0
    line_b, b = _run(monkeypatch, capsys, tmp_path / "b", 4, "0.001")
    assert line_b["replay_ms"]["settle"]["replays"] >= 10
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a["loss"].shape == (1,) and a["grad"].shape == a["param"].shape and a["grad"].ndim == 1
    assert np.abs(a["grad"]).max() > 0
    assert abs(a["loss"][0] - b["loss"][0]) <= 1e-5 * abs(a["loss"][0])
    for k in ("grad", "param"):
        assert np.abs(a[k] - b[k]).max() <= 1e-3 * np.abs(a[k]).max(), k
