"""Timing of BGKOctoMap.raycast_many on the device-resident map against what a client of the RayCaster iterator pays.

Map: BASELINE configs[1] (one synthetic 200k-ray scan, 0.1 m, block_depth 3).  Rays: 2^16 and 2^20 segments from the
sensor origin to random points of a sphere of radius 10 m, stop at the first OCCUPIED covering leaf, max_steps 4096.

 (a) raycast_many, host clock round calls that end in a stream synchronise:
       host pointers   BGKOctoMap.raycast_many (upload 24 B/ray, one launch, download 55 B/ray)
       device pointers la3dm_devmap_raycast_device on a pool of its own with the same scan (rays and results stay in HBM)
     the kernel alone comes from a kernel trace of this same script, in a run of its own:
       rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/prof/raycast_timing.py --trace
 (b) the iterator's client: the first raycast() after an insert (it refreshes the host mirror: every node of every block
     is downloaded and the host blocks rebuilt), then one raycast() per ray from Python on a sample of 2 000 rays, scaled
     to n; and the same loop in C++ on one core (the host form of raycast_many on a host-mode map), also on the sample.

Prints one JSON line per measurement.  Not a test and not part of bench.py."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import la3dm_amd  # noqa: E402
from la3dm_amd import _lib  # noqa: E402

INSERT = (0.1, 0.5, -1.0)


def rays_to_sphere(origin, n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.asarray(origin, np.float32)
    e = (o + 10.0 * d).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(o, e.shape)), e


def clock(fn, reps):
    fn()                                   # warm: code object, arenas
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), float(max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays-log2", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: only (a), three calls per size")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("raycast_timing: no GPU visible (a timing taken elsewhere says nothing)")
    xyz, origin = la3dm_amd.synthetic_scan(200000)
    md = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    t0 = time.perf_counter()
    md.insert_pointcloud(xyz, origin, *INSERT)
    t_insert_first = time.perf_counter() - t0
    assert md.is_device_resident()
    # a pool of its own for the device-pointer form (the Python class does not hand its pool out)
    H = _lib.hip()
    lender = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)
    dm = C.c_void_p()
    assert H.la3dm_devmap_create(lender.ctx(), C.byref(dm)) == 0
    o3 = (C.c_float * 3)(*[float(v) for v in origin])
    assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3,
                                                 *INSERT, None) == 0
    nb, npb = C.c_uint32(), C.c_uint32()
    H.la3dm_devmap_block_count(dm, C.byref(nb), C.byref(npb))
    print(json.dumps(dict(what="map", blocks=nb.value, nodes_per_block=npb.value, pool_bytes=9 * nb.value * npb.value,
                          first_insert_s=t_insert_first)), flush=True)
    dev = torch.device("cuda:0")
    reps = 3 if args.trace else args.reps
    for lg in args.rays_log2:
        n = 1 << lg
        s, e = rays_to_sphere(origin, n, 100 + lg)
        out = md.raycast_many(s, e)
        rows, valid = int(out["steps"].sum()), int(out["counts"][:, :3].sum())
        med, lo, hi = clock(lambda: md.raycast_many(s, e), reps)
        print(json.dumps(dict(what="raycast_many host pointers (python call)", n=n, median_s=med, min_s=lo, max_s=hi,
                              rows=rows, rows_in_existing_blocks=valid, hits=int((out["flags"] & 1).sum()),
                              longest=int(out["steps"].max()), mean_rows=rows / n, rays_per_s=n / med)), flush=True)
        t_rays = torch.from_numpy(np.ascontiguousarray(np.hstack([s, e]))).to(dev)
        t = dict(steps=torch.zeros(n, dtype=torch.int32, device=dev), flags=torch.zeros(n, dtype=torch.uint8, device=dev),
                 p=torch.zeros(n, 3, dtype=torch.float32, device=dev), block_key=torch.zeros(n, dtype=torch.int64, device=dev),
                 node_key=torch.zeros(n, dtype=torch.int32, device=dev), cls=torch.zeros(n, dtype=torch.uint8, device=dev),
                 leaf_depth=torch.zeros(n, dtype=torch.uint8, device=dev), A=torch.zeros(n, dtype=torch.float32, device=dev),
                 B=torch.zeros(n, dtype=torch.float32, device=dev), counts=torch.zeros(n, 4, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        d_out = _lib.RaycastOut(*[t[k].data_ptr() for k, _ in _lib.RaycastOut._fields_])

        def dev_call():
            assert H.la3dm_devmap_raycast_device(dm, t_rays.data_ptr(), n, 2, 4096, C.byref(d_out)) == 0
        med, lo, hi = clock(dev_call, reps)
        assert (t["steps"].cpu().numpy().view(np.uint32) == out["steps"]).all()
        print(json.dumps(dict(what="raycast_many device pointers (launch + synchronise)", n=n, median_s=med, min_s=lo,
                              max_s=hi, rows_per_s=rows / med, rays_per_s=n / med,
                              nominal_bytes_per_row="1 B state + 16 B LUT entry in an existing block; 12 B of block table per face crossed")),
              flush=True)
    if not args.trace:
        # (b) the iterator's client, after a further insert (the mirror is stale, as after every scan)
        s, e = rays_to_sphere(origin, args.sample, 7)
        t0 = time.perf_counter()
        md.insert_pointcloud(xyz, origin, *INSERT)
        t_insert = time.perf_counter() - t0
        before = md.mirror_syncs()
        t0 = time.perf_counter()
        md.raycast(s[0], e[0])
        t_first = time.perf_counter() - t0
        assert md.mirror_syncs() == before + 1
        t0 = time.perf_counter()
        for i in range(args.sample):
            md.raycast(s[i], e[i])
        t_loop = time.perf_counter() - t0
        per = t_loop / args.sample
        print(json.dumps(dict(what="iterator client: first raycast() after an insert (mirror refresh), then one raycast() "
                                   "per ray from Python", insert_s=t_insert, first_raycast_s=t_first, sample=args.sample,
                              sample_loop_s=t_loop, per_ray_s=per, scaled_to_2_16_s=t_first + per * 65536,
                              scaled_to_2_20_s=t_first + per * (1 << 20))), flush=True)
        mh = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)
        mh.insert_pointcloud(xyz, origin, *INSERT)
        med, lo, hi = clock(lambda: mh.raycast_many(s, e), 5)
        print(json.dumps(dict(what="C++ loop over the RayCaster on one core (host form of raycast_many, host-mode map)",
                              sample=args.sample, median_s=med, per_ray_s=med / args.sample,
                              scaled_to_2_16_s=med / args.sample * 65536, scaled_to_2_20_s=med / args.sample * (1 << 20))), flush=True)
    H.la3dm_devmap_destroy(dm)


if __name__ == "__main__":
    main()
