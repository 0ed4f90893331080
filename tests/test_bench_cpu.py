"""bench.py's host side: --dump-outputs writes float arrays under its size bound (a fixed, seeded sample of the leaves
when the outputs are larger), and the argument checks refuse what the benchmark cannot run."""
import os
import subprocess
import sys

import numpy as np

import bench
from conftest import ROOT


def test_dump_outputs_small_is_whole(tmp_path):
    bench.dump_outputs(str(tmp_path), {"alpha": np.arange(10, dtype=np.float32), "state": np.arange(10, dtype=np.uint8) % 3})
    assert sorted(p.name for p in tmp_path.iterdir()) == ["alpha.npy", "state.npy"]
    s = np.load(tmp_path / "state.npy")
    assert s.dtype == np.float32 and (s == np.arange(10) % 3).all()


def test_dump_outputs_large_is_seeded_sample(tmp_path):
    n = bench.DUMP_MAX_BYTES // 8 + 1000          # two float32 arrays: just over the bound
    arrays = {"A": np.arange(n, dtype=np.float32), "state": (np.arange(n) % 3).astype(np.uint8)}
    runs = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        bench.dump_outputs(str(out), arrays)
        assert sum(p.stat().st_size for p in out.iterdir()) < 64 * 10 ** 6
        runs.append({p.stem: np.load(p) for p in out.iterdir()})
    a, b = runs
    assert sorted(a) == ["A", "sample_index", "state"] and a["sample_index"].dtype == np.float64
    idx = a["sample_index"].astype(np.int64)
    assert (np.diff(idx) > 0).all() and (a["A"] == arrays["A"][idx]).all() and (a["state"] == idx % 3).all()
    assert all((a[k] == b[k]).all() for k in a)


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=60, cwd=ROOT)
    assert r.returncode == 2 and "--steps" in r.stderr
