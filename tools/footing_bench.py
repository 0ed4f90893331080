"""Measurement of footing on the device-resident map.  Not a test and not part of bench.py.

Maps: BGK, 0.1 m, block_depth 3 — (a) scans 1 and 2 of sim_structured, the tests' two-scan map; (b) one synthetic 200k-ray
scan without a range limit (la3dm_amd.synthetic_scan, BASELINE configs[1]), the map of the other benches.  Regions: 128 x 128 x 32 voxels
round the last sensor origin and the tests' recipe region (80 x 80 x 40 at origin + (-4.03, -4.03, -1.53)).  support =
OCCUPIED, clear = FREE | UNKNOWN | MISSING, headroom 4.

Per map and region one JSON line with
  footing_r0            BGKOctoMap.footing(radius 0): probe, derive, foot, scan, emit; count call + fill call as Python makes them
  footing_r4            the same at radius 4, step 1, min_support N / 2 = 24: 48 body windows and 48 near windows per word
                        that holds a standing voxel
  footing_r4_columns    ... with levels, lowest and highest as well (the column kernel and 12 bytes per column downloaded)
  frontier_26           BGKOctoMap.frontier at connectivity 26 on the same region: one pool probe per padded voxel as well,
                        so the floor the probe pass sets
  baseline_host         what the map offered before: box's classes of the padded box downloaded (1 byte per voxel) plus the
                        numpy yardstick of the tests on the host
Host clock round calls that end in a stream synchronise, profiler off; median / min / max of --reps after one warm-up call.
The kernels alone come from a kernel trace of this script in a run of its own, with no counters:
  rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/footing_bench.py --trace"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import la3dm_amd  # noqa: E402

INSERT = (0.1, 0.5, 8.0)
SUPPORT, CLEAR, H = 0x2, 0xD, 4
RECIPE_OFFSET, RECIPE_DIMS = (-4.03, -4.03, -1.53), (80, 80, 40)


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
    yield "two scans of sim_structured", m, np.asarray(origin, np.float32), np.asarray(scan(1)[1], np.float32)
    xyz, origin = la3dm_amd.synthetic_scan(200000)
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    m.insert_pointcloud(xyz, origin, 0.1, 0.5, -1.0)          # (configs[1]: no range limit)
    yield "synthetic 200k-ray scan", m, np.asarray(origin, np.float32), np.asarray(origin, np.float32)


def host_baseline(m, lo, dims, h, r, s, c):
    """box's classes of the padded box downloaded, then the tests' numpy yardstick"""
    import footing_cases as F
    res = np.float32(m.get_resolution())
    below, _ = F.pads(h, r, s)
    plo = (m.box(lo, (1, 1, 1), fields=())["origin"] - np.array(below, np.float32) * res).astype(np.float32)
    pcls = m.box(plo, F.padded_dims(dims, h, r, s), fields=())["cls"]
    return F.yardstick(pcls, dims, SUPPORT, CLEAR, h, r, s, c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: six calls of each query per region, nothing else")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("footing_bench: no GPU visible (a timing taken elsewhere says nothing)")
    N4 = la3dm_amd.footprint_cells(4)
    for map_name, m, o, o_recipe in maps():
        assert m.is_device_resident()
        regions = (("128 x 128 x 32", np.array([o[0] - np.float32(6.4), o[1] - np.float32(6.4), o[2] - np.float32(1.6)], np.float32), (128, 128, 32)),
                   ("recipe 80 x 80 x 40", (o_recipe + np.asarray(RECIPE_OFFSET, np.float32)).astype(np.float32), RECIPE_DIMS))
        for name, lo, dims in regions:
            kw = dict(support=SUPPORT, clear=CLEAR, headroom=H)
            calls = dict(footing_r0=lambda: m.footing(lo, dims, radius=0, **kw),
                         footing_r4=lambda: m.footing(lo, dims, radius=4, step=1, min_support=N4 // 2, **kw),
                         footing_r4_columns=lambda: m.footing(lo, dims, radius=4, step=1, min_support=N4 // 2,
                                                              fields=("index", "levels", "lowest", "highest"), **kw),
                         frontier_26=lambda: m.frontier(lo, dims, connectivity=26))
            if args.trace:
                for call in calls.values():
                    for _ in range(6):
                        call()
                continue
            out = {}
            for k, call in calls.items():
                call()                                       # warm-up: code objects and arenas
                out[k] = ms([timed(call)[0] for _ in range(args.reps)])
            a0, a4 = calls["footing_r0"](), calls["footing_r4_columns"]()
            t_host = []
            for _ in range(3):
                dt, base = timed(lambda: host_baseline(m, lo, dims, H, 4, 1, N4 // 2))
                t_host.append(dt)
            assert base["n"] == a4["n"] and (base["index"] == a4["index"]).all() and (base["levels"] == a4["levels"]).all()
            words = lambda r, s: (int(np.prod([dims[0] + 2 * r, dims[1] + 2 * r, dims[2] + H + 2 * s])) + 31) // 32   # noqa: E731
            print(json.dumps(dict(map=map_name, blocks=int(m.block_count()), region=name, voxels=int(np.prod(dims)), words_r0=words(0, 0),
                                  words_r4=words(4, 1), stand_r0=a0["n_stand"], foot_r0=a0["n"], stand_r4=a4["n_stand"], body_r4=a4["n_body"],
                                  foot_r4=a4["n"], disc_cells=a4["disc_cells"], min_support=N4 // 2, frontier_26_found=calls["frontier_26"]()["n"],
                                  baseline_host=ms(t_host), **out)), flush=True)


if __name__ == "__main__":
    main()
