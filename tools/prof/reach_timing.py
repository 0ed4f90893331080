"""Timing of BGKOctoMap.reach on the device-resident map against the route the map offered before it.

Map: sim_structured scans 1, 2 and 3 (0.1 m, block_depth 3) — the map of the tests and of examples/reachable_goals.cpp.
Queries, both seeded at the voxel that holds the sensor origin of scan 1, pass FREE, obstacles OCCUPIED, max_steps 2^16:
  recipe   the tests' 80 x 80 x 40 region (voxel (0, 0, 0) holds that origin - (4.03, 4.03, 1.53))
  large    256 x 256 x 32 voxels (voxel (0, 0, 0) holds that origin - (12.8, 12.8, 1.6)): ten times the recipe's voxels
each with clearance 0 and 2 at connectivity 6, and clearance 2 at connectivity 26.

 (a) the calls, host clock round calls that end in a stream synchronise, output arrays allocated once:
       device pointers  la3dm_devmap_reach_device on a pool of its own with the same scans: dense steps; the steps at the
                        frontier's list alone
       host pointers    la3dm_devmap_reach_host: dense steps (4 bytes per voxel come down); the targets alone
     the time of one level launch comes from a kernel trace of this same script, in a run of its own:
       rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/prof/reach_timing.py --trace
     and, without a profiler, from the calls themselves: (time of the call with max_steps = levels) - (time with max_steps
     = 1), over the launches in between.
 (b) the route of a client without this call: la3dm_devmap_box_host for cls alone (the classes cross to the host), then a
     flood fill on the CPU — this library's host form, timed on a host-mode map with the same scans (its own read of the
     classes from the host blocks and, with a clearance, its distance transform included).

Prints one JSON line per measurement.  Not a test and not part of bench.py."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import la3dm_amd  # noqa: E402
from la3dm_amd import _lib  # noqa: E402

INSERT = (0.1, 0.5, 8.0)
FREE_M, OCC_M = 0x1, 0x2
QUERIES = (("recipe", (80, 80, 40), (4.03, 4.03, 1.53)), ("large", (256, 256, 32), (12.8, 12.8, 1.6)))
CASES = ((0, 6), (2, 6), (2, 26))      # (clearance, connectivity)
MAX_STEPS = 1 << 16


def clock(fn, reps):
    fn()                                   # warm: code object, arenas
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), float(max(t))


def scans():
    for i in (1, 2, 3):
        yield la3dm_amd.load_pcd(os.path.join(ROOT, "tests", "golden", "data", "sim_structured", f"sim_structured_{i}.pcd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: only the device-pointer calls of (a)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("reach_timing: no GPU visible (a timing taken elsewhere says nothing)")
    md = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    mh = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)
    H, M = _lib.hip(), _lib.maplib()
    lender = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)
    dm = C.c_void_p()
    assert H.la3dm_devmap_create(lender.ctx(), C.byref(dm)) == 0
    first = None
    for xyz, origin in scans():
        first = origin if first is None else first
        md.insert_pointcloud(xyz, origin, *INSERT)
        mh.insert_pointcloud(xyz, origin, *INSERT)
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3, *INSERT, None) == 0
    assert md.is_device_resident()
    res = np.float32(md.get_resolution())
    dev = torch.device("cuda:0")
    reps = 5 if args.trace else args.reps
    for name, dims, back in QUERIES:
        lo = (np.asarray(first, np.float32) - np.array(back, np.float32)).astype(np.float32)
        d3 = np.array(dims, np.uint32)
        n = int(np.prod(dims))
        box = md.box(lo, dims, fields=())
        s = [int(np.floor((np.float32(first[a]) - box["origin"][a]) / res + np.float32(0.5))) for a in range(3)]
        seed = np.array([(s[0] * dims[1] + s[1]) * dims[2] + s[2]], np.uint32)
        assert box["cls"][tuple(s)] == 0, "the sensor's voxel is FREE"
        targets = md.frontier(lo, dims)["index"]
        nt = int(targets.size)
        d_seed = torch.from_numpy(seed.view(np.int32)).to(dev)
        d_targets = torch.from_numpy(targets.view(np.int32).copy()).to(dev)
        t_steps, t_tsteps = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(max(nt, 1), dtype=torch.int32, device=dev)
        k_steps, k_tsteps = np.zeros(n, np.uint32), np.zeros(max(nt, 1), np.uint32)
        torch.cuda.synchronize()
        print(json.dumps(dict(what=f"{name}: region", dims=dims, voxels=n, padded_words=((dims[0] + 2) * (dims[1] + 2) * (dims[2] + 2) + 31) // 32,
                              free=int((box["cls"] == 0).sum()), occupied=int((box["cls"] == 1).sum()), frontier_targets=nt)), flush=True)
        stats = _lib.ReachStats()
        for clearance, c in CASES:
            label = f"{name}, clearance {clearance}, connectivity {c}"
            g = md.reach(lo, dims, seed, clearance=clearance, connectivity=c, targets=targets)
            gh = mh.reach(lo, dims, seed, clearance=clearance, connectivity=c, targets=targets)
            assert (g["steps"] == gh["steps"]).all() and (g["target_steps"] == gh["target_steps"]).all()      # the answer timed is the right one
            assert all(g[k] == gh[k] for k in ("n_seeded", "n_reached", "levels"))
            levels = g["levels"]
            launched = min(-(-(levels + 1) // la3dm_amd.REACH_BATCH) * la3dm_amd.REACH_BATCH, MAX_STEPS)
            print(json.dumps(dict(what=f"workload: {label}", n_reached=g["n_reached"], levels=levels, level_launches=launched,
                                  targets_reached=int((g["target_steps"] != la3dm_amd.REACH_NONE).sum()))), flush=True)

            def dev_call(out, k, ms=MAX_STEPS):
                assert H.la3dm_devmap_reach_device(dm, lo.ctypes.data, d3.ctypes.data, d_seed.data_ptr(), 1, FREE_M, OCC_M, clearance, c, ms,
                                                   d_targets.data_ptr() if k else None, k, C.byref(out), C.byref(stats), None) == 0
            dense, listed = _lib.ReachOut(t_steps.data_ptr(), None), _lib.ReachOut(None, t_tsteps.data_ptr())
            med, lo_t, hi_t = clock(lambda: dev_call(dense, 0), reps)
            assert stats.levels == levels and (t_steps.cpu().numpy().view(np.uint32) == g["steps"].reshape(-1)).all()
            print(json.dumps(dict(what=f"{label}: device pointers, dense steps", median_s=med, min_s=lo_t, max_s=hi_t)), flush=True)
            if nt:
                med_t, lo_t, hi_t = clock(lambda: dev_call(listed, nt), reps)
                assert (t_tsteps[:nt].cpu().numpy().view(np.uint32) == g["target_steps"]).all()
                print(json.dumps(dict(what=f"{label}: device pointers, the steps at the frontier's list alone", median_s=med_t, min_s=lo_t, max_s=hi_t)), flush=True)
            # one level launch, without a profiler: the same call cut after its first batch
            med_1, lo_1, hi_1 = clock(lambda: dev_call(dense, 0, 1), reps)
            per_level = (med - med_1) / max(launched - 1, 1)
            print(json.dumps(dict(what=f"{label}: device pointers, max_steps = 1 (bits, seed and one level)", median_s=med_1, min_s=lo_1, max_s=hi_1,
                                  per_level_launch_s=per_level, batches=launched // la3dm_amd.REACH_BATCH)), flush=True)
            if args.trace:
                continue

            def host_call(out, k):
                assert H.la3dm_devmap_reach_host(dm, lo.ctypes.data, d3.ctypes.data, seed.ctypes.data, 1, FREE_M, OCC_M, clearance, c, MAX_STEPS,
                                                 targets.ctypes.data if k else None, k, C.byref(out), C.byref(stats), None) == 0
            med_h, lo_t, hi_t = clock(lambda: host_call(_lib.ReachOut(k_steps.ctypes.data, None), 0), reps)
            assert (k_steps == g["steps"].reshape(-1)).all()
            print(json.dumps(dict(what=f"{label}: host pointers, dense steps", median_s=med_h, min_s=lo_t, max_s=hi_t, bytes_down=4 * n)), flush=True)
            if nt:
                med_ht, lo_t, hi_t = clock(lambda: host_call(_lib.ReachOut(None, k_tsteps.ctypes.data), nt), reps)
                assert (k_tsteps[:nt] == g["target_steps"]).all()
                print(json.dumps(dict(what=f"{label}: host pointers, the steps at the frontier's list alone", median_s=med_ht, min_s=lo_t, max_s=hi_t,
                                      bytes_down=4 * nt, bytes_up=4 * nt)), flush=True)
            # (b) the classes to the host, the flood fill there
            cls = np.zeros(n, np.uint8)
            bout = _lib.BoxOut(cls.ctypes.data, None, None, None)

            def bcall():
                assert H.la3dm_devmap_box_host(dm, lo.ctypes.data, d3.ctypes.data, C.byref(bout), None) == 0
            med_b, lo_b, hi_b = clock(bcall, reps)
            hout = _lib.ReachOut(k_steps.ctypes.data, None)

            def fill():
                assert M.la3dm_map_reach(mh._h, lo.ctypes.data, d3.ctypes.data, seed.ctypes.data, 1, FREE_M, OCC_M, clearance, c, MAX_STEPS, None, 0,
                                         C.byref(hout), C.byref(stats), None) == 0
            med_f, lo_f, hi_f = clock(fill, 5)
            print(json.dumps(dict(what=f"parent route, {label}: la3dm_devmap_box_host (cls alone) + this library's host form on the CPU",
                                  box_median_s=med_b, box_min_s=lo_b, box_max_s=hi_b, bytes_down=n, fill_median_s=med_f, fill_min_s=lo_f, fill_max_s=hi_f,
                                  sum_s=med_b + med_f, ratio_to_host_pointer_dense=(med_b + med_f) / med_h,
                                  omp_num_threads=os.environ.get("OMP_NUM_THREADS"))), flush=True)
    H.la3dm_devmap_destroy(dm)


if __name__ == "__main__":
    main()
