"""Measurement of score_poses on the device-resident map.  Not a test and not part of bench.py.

Map: BGK, 0.1 m, block_depth 3, scans 1 to 3 of sim_structured (examples/localize.cpp's).  The call: 4 096 poses — a
16 x 16 x 16 grid of (dx, dy, dyaw) about scan 4's origin — x 8 192 points drawn from scans 1 to 4 (map frame), OCCUPIED
obstacles, radius 16, on two regions: 128 x 128 x 32 voxels round scan 4's origin and the tests' recipe region (80 x 80 x 40).

Per region one JSON line with
  score_poses            BGKOctoMap.score_poses (host pointers: upload of points and poses, distance_field's launches, the
                         pair kernel, download)
  baseline_field         what the parent commit offers: distance_field (d2 downloaded) + the numpy yardstick's transform and
                         gather (tests/helpers/score_cases.py) on the host, timed on --field-poses poses and scaled to 4 096
  baseline_search        one search_many per pose over clouds transformed on the host, timed on 32 poses and scaled
Host clock round calls that end in a stream synchronise, profiler off; median / min / max of --reps after one warm-up call.
The kernels alone — the pair kernel and distance_field's share — come from a kernel trace of this script in a run of its
own:
  rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/score_bench.py --trace"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--field-poses", type=int, default=128, help="poses of the distance_field + numpy baseline (scaled to 4096)")
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: six calls per region, nothing else")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("score_bench: no GPU visible (a timing taken elsewhere says nothing)")
    import region_cases as R
    import score_cases as S
    m = build()
    _, origin = scan(4)
    o = np.asarray(origin, np.float32)
    cloud = np.vstack([scan(i)[0] for i in (1, 2, 3, 4)]).astype(np.float32)
    pts = np.ascontiguousarray(cloud[np.random.default_rng(7).permutation(cloud.shape[0])[:8192]])
    grid = [(0.05 * (i - 8), 0.05 * (j - 8), 0.0, 0.01 * (k - 8)) for i in range(16) for j in range(16) for k in range(16)]
    T = la3dm_amd.poses_xyz_yaw(o, grid)
    regions = (("128 x 128 x 32", np.array([o[0] - np.float32(6.4), o[1] - np.float32(6.4), o[2] - np.float32(1.6)], np.float32), (128, 128, 32)),
               ("recipe 80 x 80 x 40", R.recipe_lo(), R.RECIPE_DIMS))
    for name, lo, dims in regions:
        call = lambda: m.score_poses(lo, dims, pts, T, radius=RADIUS)   # noqa: E731
        if args.trace:
            for _ in range(6):
                call()
            continue
        a = call()                                       # warm-up: code objects and arenas
        t = [timed(call)[0] for _ in range(args.reps)]
        # baseline 1: the distance field downloaded, the pairs on the host
        depth, res = int(m.get_block_depth()), m.get_resolution()
        _, _, g0, _ = R.anchor(lo, res, depth)
        m.distance_field(lo, dims, radius=RADIUS, fields=("d2",))
        t_df, t_np = [], []
        for _ in range(3):
            dt, d2 = timed(lambda: m.distance_field(lo, dims, radius=RADIUS, fields=("d2",))["d2"])
            t_df.append(dt)
            dt, (cls, value) = timed(lambda: S.classify(S.transform(pts, T[:args.field_poses]), res, depth, g0, dims, d2))
            t_np.append(dt)
        counts = np.stack([(cls == k).sum(1) for k in range(5)], 1)
        assert (value.sum(1) == a["sum_d2"][:args.field_poses]).all() and (counts == a["counts"][:args.field_poses]).all()
        # baseline 2: search_many per pose
        t_sm = []
        for p in range(33):
            t_sm.append(timed(lambda: m.search_many(S.transform(pts, T[p:p + 1])[0]))[0])   # (the transform on the host included)
        scale = T.shape[0] / args.field_poses
        print(json.dumps(dict(region=name, poses=int(T.shape[0]), points=int(pts.shape[0]), radius=RADIUS,
                              identity=dict(sum_d2=int(a["sum_d2"][2184]), counts=a["counts"][2184].tolist()),
                              score_poses=ms(t),
                              baseline_field=dict(distance_field_d2=ms(t_df), numpy_pairs_measured=ms(t_np), poses_measured=args.field_poses,
                                                  total_scaled_ms=1e3 * (float(np.median(t_df)) + scale * float(np.median(t_np)))),
                              baseline_search=dict(search_many_per_pose=ms(t_sm[1:]), poses_measured=32,
                                                   total_scaled_ms=1e3 * T.shape[0] * float(np.median(t_sm[1:]))))), flush=True)


if __name__ == "__main__":
    main()
