"""bench.py --dump-outputs: the file format of write_outputs (no GPU: host arrays only)."""
import os

import numpy as np

import bench


def test_outputs_are_float_arrays_named_after_their_keys(tmp_path):
    arrays = {"decisions": np.arange(24, dtype=np.int32).reshape(6, 4), "done": np.array([0, 1, 1, 0, 0, 1], np.uint8),
              "metrics": np.arange(6, dtype=np.int64) * (1 << 40), "obs": np.linspace(0, 1, 12, dtype=np.float32).reshape(6, 2)}
    bench.write_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["decisions.npy", "done.npy", "metrics.npy", "obs.npy"]
    for k, a in arrays.items():
        b = np.load(tmp_path / f"{k}.npy")
        assert b.dtype == (np.float32 if a.dtype == np.float32 else np.float64) and np.array_equal(b, a), k


def test_outputs_above_the_limit_keep_the_same_seeded_rows(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 << 10)
    arrays = {"state": np.arange(4000 * 8, dtype=np.float32).reshape(4000, 8), "tick": np.arange(4000, dtype=np.int32)}
    for run in ("a", "b"):
        bench.write_outputs(str(tmp_path / run), arrays)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 << 10
    for f in ("state.npy", "state.rows.npy", "tick.npy", "tick.rows.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    rows = np.load(tmp_path / "a" / "state.rows.npy").astype(np.int64)
    assert len(rows) > 100 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "state.npy"), arrays["state"][rows])
    assert np.array_equal(np.load(tmp_path / "a" / "tick.npy"), rows.astype(np.float64))
