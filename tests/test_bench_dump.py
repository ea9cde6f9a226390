"""bench.py --dump-outputs, CPU side: the writer keeps within its byte budget with a fixed, seeded sample of the lanes, and
writes float32 arrays that hold the device's integer results exactly."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def _arrays(n):
    rng = np.random.default_rng(1)
    return {"obs": rng.integers(0, 761, n).astype(np.uint16), "reward": rng.integers(-1, 2, n).astype(np.int8),
            "terminated": rng.integers(0, 2, n).astype(np.uint8), "truncated": rng.integers(0, 2, n).astype(np.uint8)}


def test_small_outputs_are_written_whole(tmp_path):
    bench = _load_bench()
    src = _arrays(1000)
    bench.dump_outputs(str(tmp_path), src)
    assert sorted(os.listdir(str(tmp_path))) == sorted(k + ".npy" for k in src)
    for k, v in src.items():
        got = np.load(str(tmp_path / (k + ".npy")))
        assert got.dtype == np.float32 and np.array_equal(got, v.astype(np.float32))


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path):
    bench = _load_bench()
    bench.DUMP_BYTES_MAX = 24 * 100                     # room for 100 lanes: 4 float32 results + a float64 lane index each
    src = _arrays(5000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), src)
    total = sum(os.path.getsize(str(tmp_path / "a" / f)) - 128 for f in os.listdir(str(tmp_path / "a")))   # less the .npy headers
    assert total <= bench.DUMP_BYTES_MAX
    idx = np.load(str(tmp_path / "a" / "lane_index.npy"))
    assert idx.dtype == np.float64 and len(idx) == 100 and np.all(np.diff(idx) > 0) and idx.max() < 5000
    for k, v in src.items():
        got = np.load(str(tmp_path / "a" / (k + ".npy")))
        assert got.dtype == np.float32 and np.array_equal(got, v[idx.astype(np.int64)].astype(np.float32))
        assert np.array_equal(got, np.load(str(tmp_path / "b" / (k + ".npy"))))
