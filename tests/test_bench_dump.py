"""bench.py --dump-outputs: what the last timed step returned, as .npy files two builds can be compared on (float32 / float64, at most
64 MB in all, a fixed seeded sample of frames above that)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_dtypes(tmp_path):
    import bench
    det = torch.randn(3, 300, 6)
    idx = torch.arange(900, dtype=torch.int32).view(3, 300)
    bench.dump_outputs(str(tmp_path / "d"), dict(det=det, idx=idx))
    assert sorted(os.listdir(tmp_path / "d")) == ["det.npy", "idx.npy"]
    d, i = np.load(tmp_path / "d" / "det.npy"), np.load(tmp_path / "d" / "idx.npy")
    assert d.dtype == np.float32 and np.array_equal(d, det.numpy())
    assert i.dtype == np.float64 and np.array_equal(i, idx.numpy().astype(np.float64))


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", (1 << 20) + 100_000)
    det = torch.randn(200, 300, 6)                     # 1.4 MB: over the limit
    idx = torch.randint(0, 8400, (200, 300), dtype=torch.int32)
    for k in ("a", "b"):
        bench.dump_outputs(str(tmp_path / k), dict(det=det, idx=idx))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["det.npy", "frame_index.npy", "idx.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_LIMIT_BYTES
    sel = np.load(tmp_path / "a" / "frame_index.npy").astype(np.int64)
    assert 0 < len(sel) < 200 and np.all(np.diff(sel) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "det.npy"), det.numpy()[sel])
    assert np.array_equal(np.load(tmp_path / "a" / "idx.npy"), idx.numpy()[sel].astype(np.float64))
    for f in files:                                    # the same sample every time
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_bench_dump_outputs(tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4", "--imgsz", "320",
           "--in-flight", "1", "--no-cpu-baseline", "--no-roofline", "--no-dense-head", "--no-spread", "--no-steady", "--no-one-in-flight",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert sorted(os.listdir(out)) == ["det.npy", "idx.npy"]
    det, idx = np.load(out / "det.npy"), np.load(out / "idx.npy")
    assert det.dtype == np.float32 and det.shape == (4, 300, 6) and np.isfinite(det).all()
    n_anchors = sum((320 // s) ** 2 for s in (8, 16, 32))
    assert idx.dtype == np.float64 and idx.shape == (4, 300)
    assert np.array_equal(idx, np.round(idx)) and idx.min() >= 0 and idx.max() < n_anchors
