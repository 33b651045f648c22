"""bench.py --dump-outputs without a GPU: what an exported map becomes on disk (float32 / float64 files holding every value exactly, the
size limit, the seeded row sample of a map larger than it) and the arguments it refuses."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cells(n, first_idx_base=0):
    """An export-shaped dict (TwoDmap.export()): the field names and dtypes of the real one, seeded contents."""
    rng = np.random.default_rng(7)
    f32 = np.float32
    return {"sx": rng.integers(-400, 400, n).astype(np.int32), "sy": rng.integers(-400, 400, n).astype(np.int32),
            "sz": rng.integers(-4, 4, n).astype(np.int32), "count": rng.integers(1, 60, n).astype(np.uint32),
            "first_idx": (first_idx_base + np.arange(n)).astype(np.uint32), "mean": rng.standard_normal((n, 3)).astype(f32),
            "cov": rng.standard_normal((n, 6)).astype(f32), "rough": rng.random(n).astype(f32),
            "normal": rng.standard_normal((n, 3)).astype(f32), "flags": rng.integers(0, 8, n).astype(np.uint32),
            "num_nodes": n, "num_columns": n // 2, "num_slopes": n // 3}


def test_dump_writes_every_value_exactly(tmp_path):
    cells = _cells(1000, first_idx_base=(1 << 24) - 10)          # first_idx crosses 2^24: float32 would round it
    written, n, total = bench.dump_outputs(cells, str(tmp_path))
    assert written == n == 1000 and total == sum(f.stat().st_size for f in tmp_path.iterdir())
    assert sorted(f.name for f in tmp_path.iterdir()) == sorted(k + ".npy" for k in cells)
    for k, v in cells.items():
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype in (np.float32, np.float64), k
        assert got.shape == np.shape(v) and np.array_equal(got, v), k
    assert np.load(tmp_path / "first_idx.npy").dtype == np.float64 and np.load(tmp_path / "sx.npy").dtype == np.float32


def test_dump_of_a_map_over_the_limit_is_a_seeded_row_sample(tmp_path):
    cells = _cells(20_000)                                        # 76 B per row: 1.5 MB against a 0.4 MB limit
    a = bench.dump_outputs(cells, str(tmp_path / "a"), limit=400_000)
    b = bench.dump_outputs(cells, str(tmp_path / "b"), limit=400_000)
    assert a == b and a[1] == 20_000 and 0 < a[0] < 20_000 and a[2] <= 400_000
    for f in (tmp_path / "a").iterdir():
        assert f.read_bytes() == (tmp_path / "b" / f.name).read_bytes(), f.name
    idx = np.load(tmp_path / "a" / "row_index.npy")
    assert idx.size == a[0] and (np.diff(idx) > 0).all() and idx[-1] < 20_000
    rows = idx.astype(np.int64)
    for k in ("sx", "first_idx", "mean", "cov", "normal", "flags"):
        assert np.array_equal(np.load(tmp_path / "a" / (k + ".npy")), cells[k][rows]), k
    assert int(np.load(tmp_path / "a" / "num_nodes.npy")) == 20_000


def test_bench_refuses_zero_steps_and_multi_gpu_dumps():
    for args in (["--steps", "0"], ["--gpus", "2", "--dump-outputs", "x"], ["--mode", "owner", "--dump-outputs", "x"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "error" in r.stderr, (args, r.stderr[-500:])
