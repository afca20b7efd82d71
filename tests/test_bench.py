"""bench.py without a GPU: the options of the driver contract and what --dump-outputs writes (on CPU tensors)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

import bench  # noqa: E402


def _outputs(batch, n, seed=3):
    rng = np.random.default_rng(seed)
    out = torch.from_numpy(rng.standard_normal((batch, n, n)).astype(np.float32))
    status = torch.tensor([0, 2, 0][:batch], dtype=torch.int32)
    return out, status


def test_dump_outputs_whole_inverse(tmp_path):
    out, status = _outputs(2, 33)
    bench.dump_outputs(str(tmp_path), out, status)
    assert sorted(os.listdir(tmp_path)) == ["inverse.npy", "status.npy"]
    x, st = np.load(tmp_path / "inverse.npy"), np.load(tmp_path / "status.npy")
    assert x.dtype == np.float32 and np.array_equal(x, out.numpy())
    assert st.dtype == np.float32 and np.array_equal(st, [0, 2])


def test_dump_outputs_seeded_sample_of_a_large_inverse(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_INVERSE_BYTES", 1000)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 500)
    out, status = _outputs(3, 40)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, status)
    assert sorted(os.listdir(tmp_path / "a")) == ["inverse_sample.npy", "inverse_sample_index.npy", "status.npy"]
    vals, idx = np.load(tmp_path / "a" / "inverse_sample.npy"), np.load(tmp_path / "a" / "inverse_sample_index.npy")
    assert vals.dtype == np.float32 and idx.dtype == np.float64
    assert 400 < idx.size <= 500 and np.all(np.diff(idx) > 0) and idx.max() < out.numel()
    assert np.array_equal(vals, out.numpy().reshape(-1)[idx.astype(np.int64)])
    # the same indices on every run of the same shape: two builds compare entry for entry
    assert np.array_equal(idx, np.load(tmp_path / "b" / "inverse_sample_index.npy"))


def test_dump_outputs_per_rank_files(tmp_path):
    out, status = _outputs(1, 8)
    bench.dump_outputs(str(tmp_path), out, status[:1], world=2, rank=1)
    assert sorted(os.listdir(tmp_path)) == ["rank1_inverse.npy", "rank1_status.npy"]


def test_dump_budget_stays_under_64_mb():
    whole = bench.DUMP_INVERSE_BYTES
    sample = bench.DUMP_SAMPLE * (4 + 8)
    status = 4 * 4096  # status words of the largest batch bench.py is run with, generously
    assert max(whole, sample) + status + 3 * 128 < 64 * 10 ** 6


def test_bench_options():
    h = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr
