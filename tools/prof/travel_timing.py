"""Timing of BGKOctoMap.travel on the device-resident map against reach on the same query and against the route the map
offered before it.

Map: sim_structured scans 1, 2 and 3 (0.1 m, block_depth 3) — the map of the tests and of examples/route.cpp.
Queries, both seeded at the voxel that holds the sensor origin of scan 1, pass FREE, obstacles OCCUPIED:
  recipe   the tests' 80 x 80 x 40 region (voxel (0, 0, 0) holds that origin - (4.03, 4.03, 1.53)): 500 bricks
  large    256 x 256 x 32 voxels (voxel (0, 0, 0) holds that origin - (12.8, 12.8, 1.6)): 4096 bricks
each as
  unit     move costs 1 / 1 / 1 at connectivity 6, no clearance — reach's answer, next to reach itself
  unit c2  the same with clearance 2 (DESIGN 3.12's 118-level query)
  soft     move costs 10 / 14 / 17 at connectivity 26, clearance 1, soft radius 4, penalty 40
  soft 6   the same at connectivity 6

 (a) the calls, host clock round calls that end in a stream synchronise, output arrays allocated once, medians of `reps`:
       device pointers  la3dm_devmap_travel_device on a pool of its own with the same scans: dense cost; dense cost and
                        parent; the costs at the frontier's list alone — and la3dm_devmap_reach_device, dense steps, for
                        the unit queries
       host pointers    la3dm_devmap_travel_host: dense cost
     with rounds, brick_runs and capped of every query, and the time per round: (time of the call) - (time of the same call
     with no seed: entry words, finish and the synchronise, no round) over the rounds launched.
 (b) the route of a client without this call: la3dm_devmap_box_host for cls alone (the classes cross to the host), then
     Dijkstra on the CPU — this library's host form, timed on a host-mode map with the same scans (its own read of the
     classes from the host blocks and its distance transform included).

Prints one JSON line per measurement.  Not a test and not part of bench.py.  --trace: only the device-pointer calls of (a),
the run to put under  rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/prof/travel_timing.py --trace"""
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
CASES = (("unit", dict(clearance=0, soft_radius=0, penalty=0, move_cost=(1, 1, 1), connectivity=6)),
         ("unit c2", dict(clearance=2, soft_radius=0, penalty=0, move_cost=(1, 1, 1), connectivity=6)),
         ("soft", dict(clearance=1, soft_radius=4, penalty=40, move_cost=(10, 14, 17), connectivity=26)),
         ("soft 6", dict(clearance=1, soft_radius=4, penalty=40, move_cost=(10, 14, 17), connectivity=6)))
MAX_COST = 1 << 31


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
        raise SystemExit("travel_timing: no GPU visible (a timing taken elsewhere says nothing)")
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
        t_cost, t_tcost = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(max(nt, 1), dtype=torch.int32, device=dev)
        t_parent = torch.zeros(n, dtype=torch.uint8, device=dev)
        k_cost = np.zeros(n, np.uint32)
        torch.cuda.synchronize()
        bricks = int(np.prod([(v + 7) // 8 for v in dims]))
        print(json.dumps(dict(what=f"{name}: region", dims=dims, voxels=n, bricks=bricks, free=int((box["cls"] == 0).sum()),
                              occupied=int((box["cls"] == 1).sum()), frontier_targets=nt)), flush=True)
        stats, rstats = _lib.TravelStats(), _lib.ReachStats()
        for case, kw in CASES:
            label = f"{name}, {case}"
            g = md.travel(lo, dims, seed, targets=targets, fields=("cost", "parent"), **kw)
            gh = mh.travel(lo, dims, seed, targets=targets, fields=("cost", "parent"), **kw)
            assert (g["cost"] == gh["cost"]).all() and (g["parent"] == gh["parent"]).all() and (g["target_cost"] == gh["target_cost"]).all()
            assert all(g[k] == gh[k] for k in ("n_seeded", "n_reached", "max_cost"))      # the answer timed is the right one
            launched = -(-(g["rounds"] + 1) // la3dm_amd.TRAVEL_BATCH) * la3dm_amd.TRAVEL_BATCH
            print(json.dumps(dict(what=f"workload: {label}", n_reached=g["n_reached"], max_cost=g["max_cost"], rounds=g["rounds"],
                                  rounds_launched=launched, brick_runs=g["brick_runs"], capped=g["capped"],
                                  targets_reached=int((g["target_cost"] != la3dm_amd.TRAVEL_NONE).sum()), **kw)), flush=True)
            p = _lib.TravelParams(FREE_M, OCC_M, kw["clearance"], kw["soft_radius"], kw["penalty"], (C.c_uint32 * 3)(*kw["move_cost"]),
                                  kw["connectivity"], MAX_COST)

            def dev_call(out, k, ns=1):
                assert H.la3dm_devmap_travel_device(dm, lo.ctypes.data, d3.ctypes.data, d_seed.data_ptr() if ns else None, ns, C.byref(p),
                                                    d_targets.data_ptr() if k else None, k, C.byref(out), C.byref(stats), None) == 0
            dense = _lib.TravelOut(t_cost.data_ptr(), None, None)
            med, lo_t, hi_t = clock(lambda: dev_call(dense, 0), reps)
            assert stats.rounds == g["rounds"] and (t_cost.cpu().numpy().view(np.uint32) == g["cost"].reshape(-1)).all()
            med_0, lo_0, hi_0 = clock(lambda: dev_call(dense, 0, 0), reps)
            print(json.dumps(dict(what=f"{label}: travel, device pointers, dense cost", median_s=med, min_s=lo_t, max_s=hi_t,
                                  no_seed_median_s=med_0, per_round_s=(med - med_0) / launched, batches=launched // la3dm_amd.TRAVEL_BATCH)), flush=True)
            med_p, lo_t, hi_t = clock(lambda: dev_call(_lib.TravelOut(t_cost.data_ptr(), None, t_parent.data_ptr()), 0), reps)
            assert (t_parent.cpu().numpy() == g["parent"].reshape(-1)).all()
            print(json.dumps(dict(what=f"{label}: travel, device pointers, dense cost and parent", median_s=med_p, min_s=lo_t, max_s=hi_t)), flush=True)
            if nt:
                med_t, lo_t, hi_t = clock(lambda: dev_call(_lib.TravelOut(None, t_tcost.data_ptr(), None), nt), reps)
                assert (t_tcost[:nt].cpu().numpy().view(np.uint32) == g["target_cost"]).all()
                print(json.dumps(dict(what=f"{label}: travel, device pointers, the costs at the frontier's list alone", median_s=med_t, min_s=lo_t,
                                      max_s=hi_t)), flush=True)
            if kw["move_cost"] == (1, 1, 1):
                rout = _lib.ReachOut(t_cost.data_ptr(), None)

                def reach_call():
                    assert H.la3dm_devmap_reach_device(dm, lo.ctypes.data, d3.ctypes.data, d_seed.data_ptr(), 1, FREE_M, OCC_M, kw["clearance"],
                                                       kw["connectivity"], 1 << 16, None, 0, C.byref(rout), C.byref(rstats), None) == 0
                med_r, lo_t, hi_t = clock(reach_call, reps)
                assert (t_cost.cpu().numpy().view(np.uint32) == g["cost"].reshape(-1)).all()          # reach's steps are travel's unit costs
                print(json.dumps(dict(what=f"{label}: reach, device pointers, dense steps", median_s=med_r, min_s=lo_t, max_s=hi_t, levels=rstats.levels,
                                      travel_over_reach=med / med_r)), flush=True)
            if args.trace:
                continue
            hout = _lib.TravelOut(k_cost.ctypes.data, None, None)

            def host_call():
                assert H.la3dm_devmap_travel_host(dm, lo.ctypes.data, d3.ctypes.data, seed.ctypes.data, 1, C.byref(p), None, 0, C.byref(hout),
                                                  C.byref(stats), None) == 0
            med_h, lo_t, hi_t = clock(host_call, reps)
            assert (k_cost == g["cost"].reshape(-1)).all()
            print(json.dumps(dict(what=f"{label}: travel, host pointers, dense cost", median_s=med_h, min_s=lo_t, max_s=hi_t, bytes_down=4 * n)), flush=True)
            # (b) the classes to the host, Dijkstra there
            cls = np.zeros(n, np.uint8)
            bout = _lib.BoxOut(cls.ctypes.data, None, None, None)

            def bcall():
                assert H.la3dm_devmap_box_host(dm, lo.ctypes.data, d3.ctypes.data, C.byref(bout), None) == 0
            med_b, lo_b, hi_b = clock(bcall, reps)

            def dijkstra():
                assert M.la3dm_map_travel(mh._h, lo.ctypes.data, d3.ctypes.data, seed.ctypes.data, 1, C.byref(p), None, 0, C.byref(hout), C.byref(stats),
                                          None) == 0
            med_f, lo_f, hi_f = clock(dijkstra, 5)
            print(json.dumps(dict(what=f"parent route, {label}: la3dm_devmap_box_host (cls alone) + this library's host form on the CPU",
                                  box_median_s=med_b, box_min_s=lo_b, box_max_s=hi_b, bytes_down=n, dijkstra_median_s=med_f, dijkstra_min_s=lo_f,
                                  dijkstra_max_s=hi_f, sum_s=med_b + med_f, ratio_to_host_pointer_dense=(med_b + med_f) / med_h,
                                  omp_num_threads=os.environ.get("OMP_NUM_THREADS"))), flush=True)
    H.la3dm_devmap_destroy(dm)


if __name__ == "__main__":
    main()
