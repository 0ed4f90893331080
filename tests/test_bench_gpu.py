"""bench.py contract (one JSON line, required keys) on one GPU, and the N > 1 code path in its single-GPU self-test
mode: two ranks on cuda:0, gloo instead of RCCL, the all-gather payload staged through host memory — it exercises the
launch protocol (torch.distributed.run, RANK / WORLD_SIZE / MASTER_*), the shard / scan split, the barrier + max
timing and the aggregate, never a measurement."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
        "dtype", "data", "config", "roofline")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _last_json(out):
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_single_gpu_line(built):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "1", "--rays", "50000",
                        "--no-cpu-omp", "--full"], capture_output=True, text=True, timeout=900, cwd=ROOT,
                       env={k: v for k, v in os.environ.items() if k != "LA3DM_BGK_SUM"})
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    for k in KEYS + ("cpu_baseline", "end_to_end", "gp", "lv", "bgkl"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 1 and d["value"] > 0 and d["dtype"] == "f32"
    assert d["scaling"] == "none"
    rf = d["roofline"]
    # the line is quoted on the library's default accumulate mode and carries the other one next to it
    assert d["config"]["bgk_sum"] == 1 and rf["kernel"] == "bgk_predict_fuse_t<0, false>"   # fresh map: no general path needed
    assert rf["general_instance"]["kernel"] == "bgk_predict_fuse_t<0, true>" and rf["general_instance"]["kernel_ms"] > 0
    assert rf["ordered"]["kernel"] == "bgk_predict_fuse_v5" and rf["ordered"]["kernel_ms"] > rf["kernel_ms"] > 0
    # every other BASELINE config rides on the same line, each with a roofline and a CPU leg of its own
    for depth in ("depth3", "depth4"):
        g = d["gp"][depth]
        assert g["ms_per_step"] > 0 and g["roofline"]["bound"] == "mfma" and g["roofline"]["kernel_ms"] > 0 and g["flops_per_step"] > 0
    assert d["gp"]["depth3"]["cpu_baseline"]["value"] > 0 and d["gp"]["depth3"]["max_N"] < d["gp"]["depth4"]["max_N"]
    assert d["lv"]["sequence_ms"] > 0 and d["lv"]["voxel_kernel_ms_sum"] > 0 and d["lv"]["cpu_baseline"]["value"] > 0
    assert d["lv"]["synthetic_50k"]["roofline"]["kernel_ms"] > 0
    assert d["bgkl"]["ms_per_step"] > 0 and d["bgkl"]["cpu_baseline"]["value"] > 0
    # the side legs time every insert on its own and quote the median (one stalled insert must not move the number)
    assert d["bgkl"]["ms_per_step"] <= d["bgkl"]["ms_per_step_mean"] * 1.5 and d["bgkl"]["ms_per_step_max"] >= d["bgkl"]["ms_per_step"]
    # the GP legs quote stamped instruction counts when profiles/gp_counters.json belongs to this build's gp_kernels.h
    vi = d["gp"]["depth3"]["roofline"].get("valu_issue")
    assert vi is None or (0 < vi["frac"] < 1 and vi["source"])
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert rf["kernel_ms"] > 0 and rf["algorithmic_bytes_per_launch"] > 0
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] == 1 and d["cpu_baseline"]["value"] > 0
    assert d["value"] > 100 * d["cpu_baseline"]["value"]
    assert d["end_to_end"]["ms_per_insert"] > 0


def test_plain_line_dumps_outputs(built, tmp_path):
    """a plain run: only the timed steps and the line (no leg of --full); --dump-outputs writes the leaves the last step
    updated, the same on every run with the same arguments"""
    dumps = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--rays", "50000", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        d = _last_json(r.stdout)
        for k in KEYS:
            assert k in d, k
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["roofline"]["kernel_ms"] > 0
        for k in ("cpu_baseline", "end_to_end", "scale_n1", "gp", "lv", "bgkl"):
            assert k not in d, k
        assert not {"ordered", "double_sum", "general_instance", "out_of_cache", "depth4"} & set(d["roofline"])
        assert sorted(p.name for p in out.iterdir()) == ["alpha.npy", "beta.npy", "state.npy"]
        dumps.append({k: np.load(out / f"{k}.npy") for k in ("alpha", "beta", "state")})
    a, b = dumps
    n = a["alpha"].shape[0]
    assert n > 0 and all(v.dtype == np.float32 and v.shape == (n,) for v in a.values())
    # state: 0 = leaf not updated, else LA3DM_LEAF_UPDATED (0x80) | the occupancy code (free, occupied, unknown, pruned)
    assert (a["alpha"] > 0).all() and (a["beta"] > 0).all() and np.isin(a["state"], (0, 128, 129, 130, 131)).all()
    assert (a["state"] >= 128).any()
    for k in a:
        assert (a[k].view(np.uint32) == b[k].view(np.uint32)).all(), k


@pytest.mark.parametrize("mode,scaling", [("scans", "weak"), ("shard", "strong")])
def test_two_ranks_self_test(built, mode, scaling):
    env = dict(os.environ, LA3DM_BENCH_TEST_SINGLE_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--rays", "50000", "--no-cpu", "--no-e2e", "--mode", mode]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    d = _last_json(r.stdout)
    for k in KEYS:
        assert k in d, k
    assert d["n_gpus"] == 2 and d["scaling"] == scaling and d["value"] > 0 and d["steps"] == 3
    if mode == "scans":
        per_rank = d["config"]["voxel_updates_per_scan"]
        total = d["value"] * d["ms_per_step"] * 1e-3
        assert abs(total - 2 * per_rank) / total < 0.35      # whole-job aggregate: both ranks' scans
    else:
        # block-sharded device-resident insert: the line carries its own single-GPU reference (same steps, unsharded)
        assert d["single_gpu"]["value"] > 0 and d["speedup_vs_single_gpu"] > 0
        assert "block-sharded over 2 GPUs" in d["config"]["parallelism"]
        assert d["roofline"]["kernel_ms"] > 0
        # per-stage wall times of EVERY rank, not only rank 0 (VERDICT r05 #1a)
        assert len(d["stages_ms_by_rank"]) == 2 and all(s["predict_fuse_own_range"] > 0 for s in d["stages_ms_by_rank"])


def test_shard_workload_at_world_1(built):
    """`--gpus 1 --mode shard`: the N > 1 workload (whole device-resident inserts) on ONE unsharded map, no process group — the
    N = 1 point of the series `--gpus 2/4/8` continue, so that value(N) is one workload for every N (VERDICT r05 #1a)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--mode", "shard", "--steps", "3", "--warmup", "1",
                        "--rays", "50000"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    for k in KEYS:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["scaling"] == "strong" and d["value"] > 0 and d["config"]["process_group"] is None
    assert "one GPU, unsharded" in d["config"]["parallelism"] and len(d["stages_ms_by_rank"]) == 1
    assert 0.7 < d["speedup_vs_single_gpu"] < 1.4            # the same map twice


@pytest.mark.parametrize("workload,extra", [("gp", []), ("lv", []), ("l", [])])
def test_side_benches(built, workload, extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", workload, "--steps", "2", "--warmup", "1",
                        "--no-cpu"] + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    for k in KEYS:
        assert k in d, k
    assert d["value"] > 0 and d["n_gpus"] == 1 and d["roofline"]["kernel_ms"] > 0
