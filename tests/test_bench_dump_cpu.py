"""bench.py --dump-outputs: dump_outputs writes float32 / float64 .npy files, whole arrays when they
fit their share of the 64 MB limit and otherwise the same seeded sample on every call."""
import os

import numpy as np

import bench


def test_dump_outputs_whole_arrays(tmp_path):
    rs = np.random.RandomState(1)
    arrays = {"rewards": rs.normal(size=1031), "state_T": rs.normal(size=1031).astype(np.float32),
              "state_on": rs.randint(0, 2, 1031).astype(bool), "state_lock": rs.randint(0, 11, 1031).astype(np.int32)}
    info = bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert sorted(info) == sorted(f"{k}.npy" for k in arrays)
    for k, a in arrays.items():
        got = np.load(tmp_path / "d" / f"{k}.npy")
        assert got.dtype == (a.dtype if a.dtype in (np.float32, np.float64) else np.float32)
        assert np.array_equal(got, a.astype(got.dtype))
        assert info[f"{k}.npy"] == {"dtype": str(got.dtype), "elements": 1031, "of": 1031}


def test_dump_outputs_samples_large_arrays(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)  # two arrays: 2,048 bytes each, header included
    big = np.arange(5000, dtype=np.float64)
    small = np.arange(100, dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small}, suffix="_rank1")
    a, b = (np.load(tmp_path / d / "big_rank1.npy") for d in ("a", "b"))
    assert a.size == 240 and np.array_equal(a, b)  # the same elements on every call
    assert np.all(np.diff(a) > 0) and set(a) <= set(big)  # distinct elements, in the array's order
    assert np.array_equal(np.load(tmp_path / "a" / "small_rank1.npy"), small)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 4096
