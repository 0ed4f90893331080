"""Timing of BGKOctoMap.distance_field on the device-resident map against the only route the map offered before it.

Map: BASELINE configs[1] (one synthetic 200k-ray scan, 0.1 m, block_depth 3) — the map of tools/prof/region_timing.py.
Region: the 256 x 256 x 64 voxels of that script (voxel (0, 0, 0) holds the sensor origin - (12.8, 12.8, 3.2)).
Workloads: obstacles OCCUPIED at radius 20 and 64, obstacles 0x1E (everything but FREE) at radius 20.

 (a) the calls, host clock round calls that end in a stream synchronise, output arrays allocated once:
       host pointers    la3dm_devmap_distance_host (four launches, download 8 B per voxel), and the Python method
       device pointers  la3dm_devmap_distance_device on a pool of its own with the same scan (results stay in HBM): both
                        outputs, d2 alone, dist alone
     the kernels alone come from a kernel trace of this same script, in a run of its own:
       rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/prof/distance_timing.py --trace
 (b) the route of a client without this call: box(fields=()) fetched to the host, a distance transform of that array
     on the CPU — this library's host form (timed on a host-mode map with the same scan: its host box loop and its
     transform, the loop also timed alone) and scipy's distance_transform_edt — and the upload of the 16.8 MB field for a
     consumer on the GPU.

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
DIMS = (256, 256, 64)
WORKLOADS = (("OCCUPIED, radius 20", 0x2, 20), ("OCCUPIED, radius 64", 0x2, 64), ("all but FREE (0x1E), radius 20", 0x1E, 20))
COPY_TBS = 6.29      # float4 copy, measured on this chip: the yardstick DESIGN.md 3.8 uses
FAR = 0xFFFFFFFF


def clock(fn, reps):
    fn()                                   # warm: code object, arenas
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), float(max(t))


def stage_bytes(n, outputs):
    """what the algorithm moves per stage, from the shapes (the pool reads of the first stage — one table entry per wave
    and block, one state byte per voxel and level climbed — are not counted)"""
    return dict(dm_df_bits=dict(written=n // 8), dm_df_z=dict(read=n // 8, written=2 * n),
                dm_df_pass_y=dict(read=2 * n, written=4 * n), dm_df_pass_x=dict(read=4 * n, written=4 * n * outputs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: only the device-pointer calls of (a)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("distance_timing: no GPU visible (a timing taken elsewhere says nothing)")
    xyz, origin = la3dm_amd.synthetic_scan(200000)
    md = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    md.insert_pointcloud(xyz, origin, *INSERT)
    assert md.is_device_resident()
    H = _lib.hip()
    lender = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)
    dm = C.c_void_p()
    assert H.la3dm_devmap_create(lender.ctx(), C.byref(dm)) == 0
    o3 = (C.c_float * 3)(*[float(v) for v in origin])
    assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3,
                                                 *INSERT, None) == 0
    lo = (np.asarray(origin, np.float32) - np.array([12.8, 12.8, 3.2], np.float32)).astype(np.float32)
    d3 = np.array(DIMS, np.uint32)
    n = int(np.prod(DIMS))
    cls = md.box(lo, DIMS, fields=())["cls"]
    classes = {k: int((cls == v).sum()) for k, v in (("free", 0), ("occupied", 1), ("unknown", 2), ("missing", 3))}
    print(json.dumps(dict(what="map and region", dims=DIMS, voxels=n, classes=classes)), flush=True)
    reps = 5 if args.trace else args.reps
    dev = torch.device("cuda:0")
    info = _lib.RegionInfo()
    keep = dict(d2=np.zeros(n, np.uint32), dist=np.zeros(n, np.float32))
    kout = _lib.DistanceOut(keep["d2"].ctypes.data, keep["dist"].ctypes.data)
    t = dict(d2=torch.zeros(n, dtype=torch.int32, device=dev), dist=torch.zeros(n, dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    for label, mask, radius in WORKLOADS:
        g = md.distance_field(lo, DIMS, obstacles=mask, radius=radius)
        d2 = g["d2"]
        print(json.dumps(dict(what="workload: " + label, obstacles=int((d2 == 0).sum()), finite_above_0=int(((d2 > 0) & (d2 != FAR)).sum()),
                              far=int((d2 == FAR).sum()), algorithmic_bytes=stage_bytes(n, 2))), flush=True)
        if not args.trace:
            from scipy.ndimage import distance_transform_edt
            obs = ((mask >> cls.astype(np.uint32)) & 1).astype(bool)
            want = np.rint(distance_transform_edt(~obs) ** 2).astype(np.int64)
            assert (d2 == np.where(want <= radius * radius, want, FAR).astype(np.uint32)).all()     # the answer timed is the right one
            med, lo_t, hi_t = clock(lambda: md.distance_field(lo, DIMS, obstacles=mask, radius=radius), reps)
            print(json.dumps(dict(what=f"{label}: host pointers, d2 + dist (python call, fresh arrays)", median_s=med, min_s=lo_t, max_s=hi_t,
                                  bytes_down=8 * n)), flush=True)

            def kcall():
                assert H.la3dm_devmap_distance_host(dm, lo.ctypes.data, d3.ctypes.data, mask, radius, C.byref(kout), C.byref(info)) == 0
            med, lo_t, hi_t = clock(kcall, reps)
            assert (keep["d2"] == d2.reshape(-1)).all()
            print(json.dumps(dict(what=f"{label}: host pointers, d2 + dist, arrays reused (la3dm_devmap_distance_host)", median_s=med,
                                  min_s=lo_t, max_s=hi_t, bytes_down=8 * n)), flush=True)
        for fields in (("d2", "dist"), ("d2",), ("dist",)):
            out = _lib.DistanceOut(*[t[k].data_ptr() if k in fields else None for k in ("d2", "dist")])

            def call():
                assert H.la3dm_devmap_distance_device(dm, lo.ctypes.data, d3.ctypes.data, mask, radius, C.byref(out), C.byref(info)) == 0
            med, lo_t, hi_t = clock(call, reps)
            k = fields[0]
            assert (t[k].cpu().numpy().view(np.uint32) == g[k].reshape(-1).view(np.uint32)).all()
            print(json.dumps(dict(what=f"{label}: device pointers (4 launches + synchronise), " + " + ".join(fields), median_s=med, min_s=lo_t,
                                  max_s=hi_t, voxels_per_s=n / med)), flush=True)
    if not args.trace:
        # (b) the parent's route: the classes to the host, a transform there, the field back up
        bkeep = np.zeros(n, np.uint8)
        bout = _lib.BoxOut(bkeep.ctypes.data, None, None, None)

        def bcall():
            assert H.la3dm_devmap_box_host(dm, lo.ctypes.data, d3.ctypes.data, C.byref(bout), C.byref(info)) == 0
        med, lo_t, hi_t = clock(bcall, reps)
        print(json.dumps(dict(what="parent route 1/3: box, cls only, to the host, array reused (la3dm_devmap_box_host)", median_s=med,
                              min_s=lo_t, max_s=hi_t, bytes_down=n)), flush=True)
        mh = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)
        mh.insert_pointcloud(xyz, origin, *INSERT)
        assert (mh.box(lo, DIMS, fields=())["cls"] == cls).all()
        med_b, lo_b, hi_b = clock(lambda: mh.box(lo, DIMS, fields=()), 3)
        print(json.dumps(dict(what="host-mode map: box, cls only (the loop over the host blocks the host form starts with)", median_s=med_b,
                              min_s=lo_b, max_s=hi_b, threads=os.cpu_count(), omp_num_threads=os.environ.get("OMP_NUM_THREADS"))), flush=True)
        from scipy.ndimage import distance_transform_edt
        for label, mask, radius in WORKLOADS:
            med, lo_t, hi_t = clock(lambda: mh.distance_field(lo, DIMS, obstacles=mask, radius=radius), 3)
            print(json.dumps(dict(what=f"parent route 2/3, {label}: this library's host form (host box loop + CPU transform, OpenMP)", median_s=med,
                                  min_s=lo_t, max_s=hi_t, transform_alone_s=med - med_b, omp_num_threads=os.environ.get("OMP_NUM_THREADS"))), flush=True)
            obs = ((mask >> cls.astype(np.uint32)) & 1).astype(bool)
            med, lo_t, hi_t = clock(lambda: distance_transform_edt(~obs), 3)
            print(json.dumps(dict(what=f"parent route 2/3, {label}: scipy.ndimage.distance_transform_edt of the fetched array (float64 distances, "
                                       "no radius, one thread)", median_s=med, min_s=lo_t, max_s=hi_t)), flush=True)
        field = torch.from_numpy(keep["dist"])
        pinned = field.pin_memory()
        dst = torch.zeros(n, dtype=torch.float32, device=dev)

        def up(src):
            dst.copy_(src)
            torch.cuda.synchronize()
        med, lo_t, hi_t = clock(lambda: up(field), reps)
        print(json.dumps(dict(what="parent route 3/3: upload of the float32 field, pageable host memory", median_s=med, min_s=lo_t, max_s=hi_t,
                              bytes_up=4 * n)), flush=True)
        med, lo_t, hi_t = clock(lambda: up(pinned), reps)
        print(json.dumps(dict(what="parent route 3/3: upload of the float32 field, pinned host memory", median_s=med, min_s=lo_t, max_s=hi_t,
                              bytes_up=4 * n)), flush=True)
    H.la3dm_devmap_destroy(dm)
    print(json.dumps(dict(what="yardstick", float4_copy_tb_per_s=COPY_TBS)), flush=True)


if __name__ == "__main__":
    main()
