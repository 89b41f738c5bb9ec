"""bench.py --dump-outputs: the writer of the dumped arrays (no GPU needed)."""
import os

import numpy as np


def test_dump_outputs_whole_array_is_float32(tmp_path):
    import bench
    a = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4)
    info = bench.dump_outputs(str(tmp_path / "d"), {"frame": a})
    b = np.load(tmp_path / "d" / "frame.npy")
    assert b.dtype == np.float32 and b.shape == a.shape and np.array_equal(b, a)
    assert info["frame"] == {"shape": [2, 3, 4], "dtype": "float32"}
    d = np.linspace(0.0, 1.0, 7)
    bench.dump_outputs(str(tmp_path / "d"), {"x": d})
    assert np.load(tmp_path / "d" / "x.npy").dtype == np.float64


def test_dump_outputs_over_budget_is_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", bench.DUMP_HEADER_BYTES + 4 * 10)   # room for 10 float32 values
    a = (np.arange(24, dtype=np.float32) * 3).reshape(4, 6)
    info = bench.dump_outputs(str(tmp_path / "d1"), {"frame": a})
    bench.dump_outputs(str(tmp_path / "d2"), {"frame": a})
    b1, b2 = np.load(tmp_path / "d1" / "frame.npy"), np.load(tmp_path / "d2" / "frame.npy")
    assert b1.shape == (10,) and b1.dtype == np.float32 and np.array_equal(b1, b2)
    assert info["frame"]["sampled"] == 10 and info["frame"]["shape"] == [4, 6]
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(24, size=10, replace=False))
    assert np.array_equal(b1, a.reshape(-1)[idx])
    total = sum(os.path.getsize(tmp_path / "d1" / f) for f in os.listdir(tmp_path / "d1"))
    assert total <= bench.DUMP_MAX_BYTES   # the .npy header included
