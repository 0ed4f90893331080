"""Measurement of drive on the device-resident map.  Not a test and not part of bench.py.

Maps: BGK, 0.1 m, block_depth 3 — (a) scans 1 and 2 of sim_structured, the tests' two-scan map; (b) one synthetic 200k-ray
scan without a range limit (la3dm_amd.synthetic_scan, BASELINE configs[1]), the map of the other benches.  Region: 128 x 128 x
32 voxels round the last sensor origin.  Members: footing with the tests' recipe — support OCCUPIED, clear FREE | UNKNOWN |
MISSING, headroom 4, radius 2, step 1 — and min_support 0.  Moves: connectivity 8, 10 / 14, 5 per voxel climbed, 2 per voxel
dropped; step 1 and step 4.  The seed is the sensor's voxel with snap 32.

Per map one JSON line with
  drive_footing_s1, _s4   BGKOctoMap.drive in footing mode, cost and parent downloaded: footing's three launches, the entry
                          words, the rounds, finish
  drive_list_s1, _s4      the same over footing's list, uploaded with the call (the list itself is made before the clock starts)
  baseline_host           the route the map offered before: footing's list downloaded and scipy.sparse.csgraph.dijkstra over
                          the edges of shifted slices on the host (the tests' yardstick), step 1
  travel_26               BGKOctoMap.travel at connectivity 26 over the same region from the same voxel, cost and parent: the
                          query of a robot that flies
Host clock round calls that end in a stream synchronise, profiler off; median / min / max of --reps after one warm-up call.
The kernels alone — dm_dr_round against dm_tv_round, per launch — come from a kernel trace of this script in a run of its
own, with no counters, summarised by --split:
  rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/drive_bench.py --trace
  python tools/drive_bench.py --split <dir>/.../t_kernel_trace.csv"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import la3dm_amd  # noqa: E402

INSERT = (0.1, 0.5, 8.0)
DIMS = (128, 128, 32)
FOOTING = dict(support=0x2, clear=0xD, headroom=4, radius=2, step=1, min_support=0)
MOVES = dict(connectivity=8, snap=32, move_cost=(10, 14), climb_up=5, climb_down=2)


def ms(t):
    return dict(median_ms=1e3 * float(np.median(t)), min_ms=1e3 * float(min(t)), max_ms=1e3 * float(max(t)))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def scan(i):
    return la3dm_amd.load_pcd(os.path.join(ROOT, "tests", "golden", "data", "sim_structured", f"sim_structured_{i}.pcd"))


def maps():
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    for i in (1, 2):
        xyz, origin = scan(i)
        m.insert_pointcloud(xyz, origin, *INSERT)
    yield "two scans of sim_structured", m, np.asarray(origin, np.float32)
    xyz, origin = la3dm_amd.synthetic_scan(200000)
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    m.insert_pointcloud(xyz, origin, 0.1, 0.5, -1.0)          # (configs[1]: no range limit)
    yield "synthetic 200k-ray scan", m, np.asarray(origin, np.float32)


def host_baseline(m, lo, seed):
    """footing's list downloaded, then the tests' yardstick: scipy's Dijkstra on the host"""
    import drive_cases as D
    index = m.footing(lo, DIMS, **FOOTING)["index"]
    kw = dict(MOVES)
    kw.pop("snap")
    return D.yardstick(D.members_of(DIMS, index), [seed], step=1, snap=32, **kw)


def split(path):
    """per kernel of the two round kernels and of drive's other kernels: launches, mean, median and least duration in us"""
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if not re.search(r"dm_dr_|dm_tv_|dm_ft_", name):
                continue
            short = re.sub(r"^void ", "", name).split("(")[0].replace("la3dm_dev::", "")
            rows.setdefault(short, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for k in sorted(rows):
        t = np.array(rows[k])
        print(f"{k:24s} n {t.size:5d}  mean {t.mean():7.2f}  median {np.median(t):7.2f}  min {t.min():7.2f}  max {t.max():7.2f}  total {t.sum():9.1f}  (us)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: six calls of each query per map, nothing else")
    ap.add_argument("--split", metavar="KERNEL_TRACE_CSV", help="summarise a kernel trace of a --trace run and exit")
    args = ap.parse_args()
    if args.split:
        return split(args.split)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("drive_bench: no GPU visible (a timing taken elsewhere says nothing)")
    for map_name, m, o in maps():
        assert m.is_device_resident()
        lo = np.array([o[0] - np.float32(6.4), o[1] - np.float32(6.4), o[2] - np.float32(1.6)], np.float32)
        info = m.box(lo, (1, 1, 1), fields=())
        s = [min(max(int(round(float((o[a] - info["origin"][a]) / m.get_resolution()))), 0), DIMS[a] - 1) for a in range(3)]
        seed = (s[0] * DIMS[1] + s[1]) * DIMS[2] + s[2]
        index = m.footing(lo, DIMS, **FOOTING)["index"]
        both = ("cost", "parent")
        calls = dict(drive_footing_s1=lambda: m.drive(lo, DIMS, [seed], footing=FOOTING, step=1, fields=both, **MOVES),
                     drive_footing_s4=lambda: m.drive(lo, DIMS, [seed], footing=FOOTING, step=4, fields=both, **MOVES),
                     drive_list_s1=lambda: m.drive(lo, DIMS, [seed], members=index, step=1, fields=both, **MOVES),
                     drive_list_s4=lambda: m.drive(lo, DIMS, [seed], members=index, step=4, fields=both, **MOVES),
                     travel_26=lambda: m.travel(lo, DIMS, [seed], connectivity=26, fields=both))
        if args.trace:
            for k in ("drive_footing_s1", "drive_footing_s4", "travel_26"):
                for _ in range(6):
                    calls[k]()
            continue
        out, last = {}, {}
        for k, call in calls.items():
            call()                                       # warm-up: code objects and arenas
            t = [timed(call) for _ in range(args.reps)]
            out[k], last[k] = ms([dt for dt, _ in t]), t[-1][1]
        assert (last["drive_footing_s1"]["cost"] == last["drive_list_s1"]["cost"]).all() and (last["drive_footing_s4"]["parent"] == last["drive_list_s4"]["parent"]).all()
        t_host = []
        for _ in range(3):
            dt, base = timed(lambda: host_baseline(m, lo, seed))
            t_host.append(dt)
        assert (base["cost"] == last["drive_footing_s1"]["cost"]).all() and (base["parent"] == last["drive_footing_s1"]["parent"]).all()
        diag = lambda k: {n: int(last[k][n]) for n in ("n_seeded", "n_reached", "max_cost", "rounds", "brick_runs", "capped")}   # noqa: E731
        print(json.dumps(dict(map=map_name, blocks=int(m.block_count()), region="128 x 128 x 32", voxels=int(np.prod(DIMS)), members=int(index.size),
                              drive_s1=diag("drive_footing_s1"), drive_s4=diag("drive_footing_s4"), travel=diag("travel_26"),
                              baseline_host=ms(t_host), **out)), flush=True)


if __name__ == "__main__":
    main()
