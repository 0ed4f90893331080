"""Timing of BGKOctoMap.box / columns on the device-resident map against the only routes the map offered before them.

Map: BASELINE configs[1] (one synthetic 200k-ray scan, 0.1 m, block_depth 3) — the map of tools/prof/raycast_timing.py.
Region: 256 x 256 x 64 voxels whose voxel (0, 0, 0) holds the sensor origin - (12.8, 12.8, 3.2), and its columns.

 (a) the ABI calls, host clock round calls that end in a stream synchronise:
       host pointers    BGKOctoMap.box / columns (one launch, download 10 B per voxel / 24 B per column)
       device pointers  la3dm_devmap_box_device / columns_device on a pool of its own with the same scan (results stay
                        in HBM); box with all four outputs, with cls alone, and with every output one element off its
                        alignment (the one-voxel-per-thread kernel: the other decomposition of the stores)
     the kernels alone come from a kernel trace of this same script, in a run of its own:
       rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/prof/region_timing.py --trace
 (b) the routes of a client without these calls: search_many over the same voxel centres (12 B up and 10 B down per
     voxel, one probe per voxel; wrong inside collapsed regions), and the first leaves() after an insert (the mirror
     refresh a viewer-style client pays).

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
COPY_TBS = 6.29      # float4 copy, measured on this chip: the yardstick of a store-bound kernel


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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: only (a)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("region_timing: no GPU visible (a timing taken elsewhere says nothing)")
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
    nb, npb = C.c_uint32(), C.c_uint32()
    H.la3dm_devmap_block_count(dm, C.byref(nb), C.byref(npb))
    lo = (np.asarray(origin, np.float32) - np.array([12.8, 12.8, 3.2], np.float32)).astype(np.float32)
    d3 = np.array(DIMS, np.uint32)
    n, ncol = int(np.prod(DIMS)), DIMS[0] * DIMS[1]
    b = md.box(lo, DIMS)
    c = md.columns(lo, DIMS)
    classes = {k: int((b["cls"] == v).sum()) for k, v in (("free", 0), ("occupied", 1), ("unknown", 2), ("missing", 3))}
    print(json.dumps(dict(what="map and region", blocks=nb.value, nodes_per_block=npb.value, dims=DIMS, voxels=n,
                          classes=classes, under_a_coarser_leaf=int(((b["leaf_depth"] < 2)).sum()),
                          columns_with_occupied=int((c["counts"][:, :, 1] > 0).sum()))), flush=True)
    assert (c["counts"] == np.stack([(b["cls"] == k).sum(2) for k in range(4)], 2)).all()
    reps = 5 if args.trace else args.reps
    med, lo_t, hi_t = clock(lambda: md.box(lo, DIMS), reps)
    print(json.dumps(dict(what="box, host pointers, all outputs (python call)", median_s=med, min_s=lo_t, max_s=hi_t,
                          bytes_down=10 * n)), flush=True)
    med, lo_t, hi_t = clock(lambda: md.box(lo, DIMS, fields=()), reps)
    print(json.dumps(dict(what="box, host pointers, cls only (python call)", median_s=med, min_s=lo_t, max_s=hi_t, bytes_down=n)), flush=True)
    med, lo_t, hi_t = clock(lambda: md.columns(lo, DIMS), reps)
    print(json.dumps(dict(what="columns, host pointers (python call)", median_s=med, min_s=lo_t, max_s=hi_t, bytes_down=24 * ncol)), flush=True)
    dev = torch.device("cuda:0")
    info = _lib.RegionInfo()
    # the same host-pointer calls as a C client makes them: output arrays allocated once and reused (the Python
    # methods above allocate fresh arrays per call, whose pages the download touches for the first time)
    keep = dict(cls=np.zeros(n, np.uint8), leaf_depth=np.zeros(n, np.uint8), A=np.zeros(n, np.float32), B=np.zeros(n, np.float32))
    kout = _lib.BoxOut(*[keep[k].ctypes.data for k, _ in _lib.BoxOut._fields_])

    def kcall():
        assert H.la3dm_devmap_box_host(dm, lo.ctypes.data, d3.ctypes.data, C.byref(kout), C.byref(info)) == 0
    med, lo_t, hi_t = clock(kcall, reps)
    assert (keep["cls"] == b["cls"].reshape(-1)).all()
    print(json.dumps(dict(what="box, host pointers, all outputs, arrays reused (la3dm_devmap_box_host)", median_s=med, min_s=lo_t,
                          max_s=hi_t, bytes_down=10 * n)), flush=True)
    if not args.trace:
        ijk0 = np.stack(np.meshgrid(*[np.arange(v) for v in DIMS], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
        pts0 = np.ascontiguousarray((b["origin"][None, :] + ijk0 * np.float32(md.get_resolution())).astype(np.float32))
        ex, stt = np.zeros(n, np.uint8), np.zeros(n, np.uint8)

        def scall():
            assert H.la3dm_devmap_search_host(dm, pts0.ctypes.data, n, ex.ctypes.data, keep["A"].ctypes.data, keep["B"].ctypes.data,
                                              stt.ctypes.data) == 0
        med, lo_t, hi_t = clock(scall, reps)
        print(json.dumps(dict(what="search_many over the same voxel centres, host pointers, arrays reused (la3dm_devmap_search_host)",
                              median_s=med, min_s=lo_t, max_s=hi_t, bytes_up=12 * n, bytes_down=10 * n)), flush=True)
    for label, off, fields in (("all outputs, aligned (4 voxels per thread)", 0, ("cls", "leaf_depth", "A", "B")),
                               ("cls only, aligned (4 voxels per thread)", 0, ("cls",)),
                               ("all outputs, one element off (1 voxel per thread)", 1, ("cls", "leaf_depth", "A", "B")),
                               ("cls only, one byte off (1 voxel per thread)", 1, ("cls",))):
        t = dict(cls=torch.zeros(n + off, dtype=torch.uint8, device=dev), leaf_depth=torch.zeros(n + off, dtype=torch.uint8, device=dev),
                 A=torch.zeros(n + off, dtype=torch.float32, device=dev), B=torch.zeros(n + off, dtype=torch.float32, device=dev))
        torch.cuda.synchronize()
        out = _lib.BoxOut(*[t[k][off:].data_ptr() if k in fields else None for k, _ in _lib.BoxOut._fields_])

        def call():
            assert H.la3dm_devmap_box_device(dm, lo.ctypes.data, d3.ctypes.data, C.byref(out), C.byref(info)) == 0
        med, lo_t, hi_t = clock(call, reps)
        assert (t["cls"][off:].cpu().numpy() == b["cls"].reshape(-1)).all()
        written = n * sum(dict(cls=1, leaf_depth=1, A=4, B=4)[k] for k in fields)
        print(json.dumps(dict(what="box, device pointers (launch + synchronise): " + label, median_s=med, min_s=lo_t, max_s=hi_t,
                              bytes_written=written, written_tb_per_s_of_the_call=written / med / 1e12)), flush=True)
    tc = dict(counts=torch.zeros(ncol, 4, dtype=torch.int32, device=dev), low_occ=torch.zeros(ncol, dtype=torch.int32, device=dev),
              top_occ=torch.zeros(ncol, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    cout = _lib.ColumnsOut(*[tc[k].data_ptr() for k, _ in _lib.ColumnsOut._fields_])

    def ccall():
        assert H.la3dm_devmap_columns_device(dm, lo.ctypes.data, d3.ctypes.data, C.byref(cout), C.byref(info)) == 0
    med, lo_t, hi_t = clock(ccall, reps)
    assert (tc["counts"].cpu().numpy().view(np.uint32).reshape(c["counts"].shape) == c["counts"]).all()
    print(json.dumps(dict(what="columns, device pointers (launch + synchronise)", median_s=med, min_s=lo_t, max_s=hi_t,
                          bytes_written=24 * ncol, voxels_per_s=n / med)), flush=True)
    big = np.array((4096, 4096, 64), np.uint32)
    tcb = dict(counts=torch.zeros(4096 * 4096, 4, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    lo_big = (np.asarray(origin, np.float32) - np.array([204.8, 204.8, 3.2], np.float32)).astype(np.float32)
    bout = _lib.ColumnsOut(tcb["counts"].data_ptr(), None, None)

    def bcall():
        assert H.la3dm_devmap_columns_device(dm, lo_big.ctypes.data, big.ctypes.data, C.byref(bout), None) == 0
    med, lo_t, hi_t = clock(bcall, 3)
    print(json.dumps(dict(what="columns 4096 x 4096 x 64 (counts only), device pointers", median_s=med, min_s=lo_t, max_s=hi_t,
                          bytes_written=16 * 4096 * 4096, written_tb_per_s_of_the_call=16 * 4096 * 4096 / med / 1e12)), flush=True)
    if not args.trace:
        # (b) the parent's routes
        ijk = np.stack(np.meshgrid(*[np.arange(v) for v in DIMS], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
        pts = (b["origin"][None, :] + ijk * np.float32(md.get_resolution())).astype(np.float32)
        s = md.search_many(pts)
        wrong = int(((s["exists"] != 0) & (s["state"] == 3)).sum())
        assert ((s["exists"] != 0) == (b["cls"].reshape(-1) != 3)).all()
        med, lo_t, hi_t = clock(lambda: md.search_many(pts), 5)
        print(json.dumps(dict(what="search_many over the same voxel centres, host pointers (python call; the centres already built)",
                              median_s=med, min_s=lo_t, max_s=hi_t, bytes_up=12 * n, bytes_down=10 * n,
                              voxels_that_read_raw_PRUNED=wrong)), flush=True)
        t0 = time.perf_counter()
        md.insert_pointcloud(xyz, origin, *INSERT)
        t_insert = time.perf_counter() - t0
        before = md.mirror_syncs()
        t0 = time.perf_counter()
        lv = md.leaves()
        t_first = time.perf_counter() - t0
        assert md.mirror_syncs() == before + 1
        t0 = time.perf_counter()
        md.leaves()
        t_second = time.perf_counter() - t0
        print(json.dumps(dict(what="viewer-style client: first leaves() after an insert (mirror refresh + leaf dump), then a second one",
                              insert_s=t_insert, first_leaves_s=t_first, second_leaves_s=t_second, leaves=int(lv["state"].size))), flush=True)
    H.la3dm_devmap_destroy(dm)
    print(json.dumps(dict(what="yardstick", float4_copy_tb_per_s=COPY_TBS)), flush=True)


if __name__ == "__main__":
    main()
