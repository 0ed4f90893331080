"""Measurement of nearest and nearest_points on the device-resident map.  Not a test and not part of
bench.py.

Map: BGK, 0.1 m, block_depth 3, scans 1 to 3 of sim_structured (examples/localize.cpp's).  OCCUPIED obstacles, radius 16, on
two regions: 128 x 128 x 32 voxels round scan 4's origin and the tests' recipe region (80 x 80 x 40).

Per region one JSON line with
  nearest                BGKOctoMap.nearest (host pointers: the four launches, download of index and d2)
  nearest_index          the same with fields = index alone (4 bytes per voxel downloaded, as distance_field_d2)
  distance_field_d2      BGKOctoMap.distance_field(fields = d2) on the same region: its kernels are untouched by nearest, so
                         the ratio is the price of carrying the argmin
  baseline_host          what the map offered before: box's classes downloaded (1 byte per voxel) plus scipy's
                         distance_transform_edt(return_indices=True) on the host
  nearest_points         BGKOctoMap.nearest_points for 8 192 points drawn from scans 1 to 4 under a pose (upload, the transform
                         into working storage, one lane per point, download of the four arrays)
Host clock round calls that end in a stream synchronise, profiler off; median / min / max of --reps after one warm-up call.
The kernels alone come from a kernel trace of this script in a run of its own:
  rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/nearest_bench.py --trace"""
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
RADIUS = 16


def ms(t):
    return dict(median_ms=1e3 * float(np.median(t)), min_ms=1e3 * float(min(t)), max_ms=1e3 * float(max(t)))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def scan(i):
    return la3dm_amd.load_pcd(os.path.join(ROOT, "tests", "golden", "data", "sim_structured", f"sim_structured_{i}.pcd"))


def build():
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    for i in (1, 2, 3):
        xyz, origin = scan(i)
        m.insert_pointcloud(xyz, origin, *INSERT)
    assert m.is_device_resident()
    return m


def host_baseline(m, lo, dims):
    """box's classes downloaded, then scipy's feature transform: (index, d2) untruncated"""
    from scipy.ndimage import distance_transform_edt
    cls = m.box(lo, dims, fields=())["cls"]
    obs = cls == 1
    if not obs.any():
        return None
    dist, ind = distance_transform_edt(~obs, return_indices=True)
    return np.ravel_multi_index(tuple(ind), dims), np.rint(dist ** 2).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: six calls of each query per region, nothing else")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("nearest_bench: no GPU visible (a timing taken elsewhere says nothing)")
    import region_cases as R
    m = build()
    _, origin = scan(4)
    o = np.asarray(origin, np.float32)
    cloud = np.vstack([scan(i)[0] for i in (1, 2, 3, 4)]).astype(np.float32)
    pts = np.ascontiguousarray(cloud[np.random.default_rng(7).permutation(cloud.shape[0])[:8192]])
    pose = la3dm_amd.poses_xyz_yaw(o, [(0.05, -0.05, 0.0, 0.01)])[0]
    regions = (("128 x 128 x 32", np.array([o[0] - np.float32(6.4), o[1] - np.float32(6.4), o[2] - np.float32(1.6)], np.float32), (128, 128, 32)),
               ("recipe 80 x 80 x 40", R.recipe_lo(), R.RECIPE_DIMS))
    for name, lo, dims in regions:
        calls = dict(nearest=lambda: m.nearest(lo, dims, radius=RADIUS),
                     nearest_index=lambda: m.nearest(lo, dims, radius=RADIUS, fields="index"),
                     distance_field_d2=lambda: m.distance_field(lo, dims, radius=RADIUS, fields=("d2",)),
                     nearest_points=lambda: m.nearest_points(lo, dims, pts, pose, radius=RADIUS))
        if args.trace:
            for call in calls.values():
                for _ in range(6):
                    call()
            continue
        out = {}
        for k, call in calls.items():
            call()                                       # warm-up: code objects and arenas
            out[k] = ms([timed(call)[0] for _ in range(args.reps)])
        a = calls["nearest"]()
        assert (a["d2"] == calls["distance_field_d2"]()["d2"]).all()
        host_baseline(m, lo, dims)
        t_host = []
        for _ in range(3):
            dt, base = timed(lambda: host_baseline(m, lo, dims))
            t_host.append(dt)
        finite = a["index"] != 0xFFFFFFFF
        d2 = base[1]
        assert (a["d2"][finite] == d2[finite]).all() and (d2[~finite] > RADIUS * RADIUS).all()   # (scipy breaks ties its own way: d2 is what agrees)
        p = calls["nearest_points"]()
        print(json.dumps(dict(region=name, radius=RADIUS, voxels=int(np.prod(dims)), within_radius=int(finite.sum()), points=int(pts.shape[0]),
                              point_classes=np.bincount(p["cls"], minlength=5).tolist(), baseline_host=ms(t_host), **out)), flush=True)


if __name__ == "__main__":
    main()
