"""bench.py --dump-outputs writer: file names, float32, and the fixed seeded sample of an array above DUMP_MAX_ELEMS."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_names_dtype_and_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    big = np.arange(5000, dtype=np.float64)
    arrays = {"losses": np.array([1.5, 2.5, 3.5]), "grads": big, "bn_stats": np.ones(10, dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert sorted(os.listdir(tmp_path / "a")) == ["bn_stats.npy", "grads_sample.npy", "losses.npy"]
    for f in os.listdir(tmp_path / "a"):
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32 and np.array_equal(x, y), f
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "losses.npy"), [1.5, 2.5, 3.5])
    s = np.load(tmp_path / "a" / "grads_sample.npy")
    assert s.shape == (1000,) and np.all(np.diff(s) > 0)          # distinct elements, in index order
    assert np.all(s == np.round(s)) and s.min() >= 0 and s.max() < 5000   # values of `big` = their own indices
