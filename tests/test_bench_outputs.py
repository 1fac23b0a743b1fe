"""bench.py --dump-outputs and the lean plain run: the sample of a large output is fixed and seeded, what is written is float32 /
float64 within 64 MB, --steps is validated before anything starts, and (GPU) a plain run times exactly --steps steps, carries no
--full object and writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


@pytest.fixture
def with_torch(monkeypatch):
    monkeypatch.setattr(bench, "torch", torch)        # main() sets it after the launcher decision


def test_dump_sample_is_one_element_per_stratum_and_fixed(with_torch):
    n = 3 * bench.DUMP_CAP + 7
    x = np.arange(n, dtype=np.float64)
    a, b = bench.dump_sample(x, seed=1), bench.dump_sample(x, seed=1)
    assert a.shape == (bench.DUMP_CAP,) and a.dtype == np.float64 and np.array_equal(a, b)
    strata = np.arange(bench.DUMP_CAP + 1, dtype=np.int64) * n // bench.DUMP_CAP
    assert np.all(a >= strata[:-1]) and np.all(a < strata[1:])
    assert not np.array_equal(a, bench.dump_sample(x, seed=2))
    # a torch tensor is sampled where it lives, with the same indices
    t = bench.dump_sample(torch.arange(n, dtype=torch.float32), seed=1)
    assert t.dtype == np.float32 and np.array_equal(t.astype(np.float64), a)


def test_dump_sample_keeps_small_outputs_whole(with_torch):
    assert np.array_equal(bench.dump_sample(torch.tensor(2.5)), np.array([2.5], dtype=np.float32))
    ints = bench.dump_sample(np.arange(6).reshape(2, 3))
    assert ints.dtype == np.float64 and np.array_equal(ints, np.arange(6.0))


def test_write_outputs(tmp_path, with_torch):
    out = tmp_path / "d"
    bench.write_outputs(str(out), {"prediction": torch.randn(512, dtype=torch.float64), "state": torch.randn(bench.DUMP_CAP + 5)})
    p, s = np.load(out / "prediction.npy"), np.load(out / "state.npy")
    assert p.shape == (512,) and p.dtype == np.float64 and s.shape == (bench.DUMP_CAP,) and s.dtype == np.float32


def test_steps_below_one_is_refused_before_anything_starts():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(dev, tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - 512 / (d["ms_per_step"] * 1e-3)) / d["value"] < 2e-3
    for k in ("roofline", "roofline_encoder", "cpu_baseline", "optimizer_ms_per_step"):
        assert k not in d, k
    pred, loss, state = (np.load(out / f"{k}.npy") for k in ("prediction", "loss", "state"))
    assert pred.shape == (512,) and pred.dtype == np.float32 and np.isfinite(pred).all()
    assert loss.shape == (1,) and abs(float(loss[0]) - d["final_loss"]) <= 1e-5 * max(1.0, abs(d["final_loss"]))
    assert state.shape == (bench.DUMP_CAP,) and state.dtype == np.float32 and np.isfinite(state).all()
