"""Timing of BGKOctoMap.frontier on the device-resident map against the routes the map offered before it.

Map: BASELINE configs[1] (one synthetic 200k-ray scan, 0.1 m, block_depth 3) — the map of tools/prof/region_timing.py.
Region: the 256 x 256 x 64 voxels of that script (voxel (0, 0, 0) holds the sensor origin - (12.8, 12.8, 3.2)).
Workloads: open FREE, unknown UNKNOWN | MISSING, min_neighbours 1, connectivity 6 and 26.

 (a) the calls, host clock round calls that end in a stream synchronise, output arrays allocated once:
       device pointers  la3dm_devmap_frontier_device on a pool of its own with the same scan (the list stays in HBM): index +
                        nbrs, index alone, the count-only call, index + nbrs + the dense score
       host pointers    la3dm_devmap_frontier_host (the launches, download of the entries found), and the Python method
                        (count, then fill: two calls)
     the kernels alone come from a kernel trace of this same script, in a run of its own:
       rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/prof/frontier_timing.py --trace
 (b) the routes of a client without this call:
       GPU consumer   la3dm_devmap_box_device for the cls of the padded box, then the stencil in torch on the device: shifted
                      comparisons summed, then nonzero
       host consumer  la3dm_devmap_box_host for cls alone, then a stencil on the CPU — this library's host form, timed on a
                      host-mode map with the same scan (its own read of the classes from the host blocks included; that read
                      is also timed alone) — and the upload of the list where the planner lives on the GPU

Also counted from the data: the share of 32-voxel words of the padded open stream that hold an open voxel (what the stencil
kernel's time is made of).  Prints one JSON line per measurement.  Not a test and not part of bench.py."""
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
OPEN, UNKNOWN = 0x1, 0xC
CONNECTIVITIES = (6, 26)
COPY_TBS = 6.29      # float4 copy, measured on this chip: the yardstick DESIGN.md 3.8 uses


def clock(fn, reps):
    fn()                                   # warm: code object, arenas
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), float(max(t))


def offsets(c):
    reach = {6: 1, 18: 2, 26: 3}[c]
    return [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if 1 <= abs(i) + abs(j) + abs(k) <= reach]


def stage_bytes(padded, n_open_words, n_found, c, nbrs):
    """what the algorithm moves per stage, from the shapes (the pool reads of the first stage — one table entry per wave and
    block, one state byte per voxel and level climbed — are not counted; the windows of the stencil overlap and are served
    by the caches: counted once)"""
    words = (padded + 31) // 32
    return dict(dm_fr_bits=dict(written=8 * words), dm_fr_stencil=dict(read=4 * words + 4 * words, written=4 * words + 4 * n_open_words),
                dm_scan_lb=dict(read=4 * words, written=4 * words),
                dm_fr_emit=dict(read=8 * words, written=(5 if nbrs else 4) * n_found), windows_per_open_word=c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: only the device-pointer calls of (a)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("frontier_timing: no GPU visible (a timing taken elsewhere says nothing)")
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
    res = np.float32(md.get_resolution())
    pdims = tuple(d + 2 for d in DIMS)
    padded = int(np.prod(pdims))
    inner = md.box(lo, DIMS, fields=())
    plo = (inner["origin"] - res).astype(np.float32)          # the padded box: one voxel further out on every side
    pbox = md.box(plo, pdims, fields=())
    pcls = pbox["cls"]
    assert (pcls[1:-1, 1:-1, 1:-1] == inner["cls"]).all()
    classes = {k: int((inner["cls"] == v).sum()) for k, v in (("free", 0), ("occupied", 1), ("unknown", 2), ("missing", 3))}
    is_open = np.zeros(pdims, bool)
    is_open[1:-1, 1:-1, 1:-1] = ((OPEN >> inner["cls"].astype(np.uint32)) & 1).astype(bool)
    flat = np.zeros(((padded + 31) // 32) * 32, bool)
    flat[:padded] = is_open.reshape(-1)
    open_words = int(flat.reshape(-1, 32).any(1).sum())
    print(json.dumps(dict(what="map and region", dims=DIMS, voxels=n, padded_voxels=padded, classes=classes, words=flat.size // 32,
                          words_with_an_open_voxel=open_words, share=open_words / (flat.size // 32))), flush=True)
    reps = 5 if args.trace else args.reps
    dev = torch.device("cuda:0")
    info = _lib.RegionInfo()
    found = C.c_uint64(0)
    keep = dict(index=np.zeros(n, np.uint32), nbrs=np.zeros(n, np.uint8), score=np.zeros(n, np.uint8))
    t = dict(index=torch.zeros(n, dtype=torch.int32, device=dev), nbrs=torch.zeros(n, dtype=torch.uint8, device=dev),
             score=torch.zeros(n, dtype=torch.uint8, device=dev))
    pt = torch.zeros(padded, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    lists = {}
    for c in CONNECTIVITIES:
        label = f"connectivity {c}"
        g = md.frontier(lo, DIMS, open=OPEN, unknown=UNKNOWN, connectivity=c, fields=("index", "nbrs", "score"))
        lists[c] = g
        unk = ((UNKNOWN >> pcls.astype(np.uint32)) & 1).astype(np.uint8)
        want = np.zeros(DIMS, np.uint8)
        for i, j, k in offsets(c):
            want += unk[1 + i:1 + i + DIMS[0], 1 + j:1 + j + DIMS[1], 1 + k:1 + k + DIMS[2]]
        want[~is_open[1:-1, 1:-1, 1:-1]] = 0
        assert (g["score"] == want).all() and (g["index"] == np.flatnonzero(want.reshape(-1))).all()   # the answer timed is the right one
        nf = g["n"]
        front_words = int(np.unique((np.ravel_multi_index(tuple(a + 1 for a in np.unravel_index(g["index"], DIMS)), pdims)) >> 5).size)
        print(json.dumps(dict(what="workload: " + label, frontier_voxels=nf, share_of_voxels=nf / n, words_with_a_frontier_voxel=front_words,
                              algorithmic_bytes=stage_bytes(padded, open_words, nf, c, True))), flush=True)
        for fields, cap in ((("index", "nbrs"), n), (("index",), n), ((), 0), (("index", "nbrs", "score"), n)):
            out = _lib.FrontierOut(*[t[k].data_ptr() if k in fields else None for k in ("index", "nbrs", "score")])

            def call():
                assert H.la3dm_devmap_frontier_device(dm, lo.ctypes.data, d3.ctypes.data, OPEN, UNKNOWN, c, 1, cap, C.byref(out) if fields else None,
                                                      C.byref(found), C.byref(info)) == 0
            med, lo_t, hi_t = clock(call, reps)
            assert found.value == nf
            if fields:
                assert (t["index"][:nf].cpu().numpy().view(np.uint32) == g["index"]).all()
            print(json.dumps(dict(what=f"{label}: device pointers (launches + synchronise), " + (" + ".join(fields) if fields else "count only"),
                                  median_s=med, min_s=lo_t, max_s=hi_t, voxels_per_s=n / med)), flush=True)
        if args.trace:
            continue
        kout = _lib.FrontierOut(keep["index"].ctypes.data, keep["nbrs"].ctypes.data, None)

        def kcall():
            assert H.la3dm_devmap_frontier_host(dm, lo.ctypes.data, d3.ctypes.data, OPEN, UNKNOWN, c, 1, n, C.byref(kout), C.byref(found), C.byref(info)) == 0
        med, lo_t, hi_t = clock(kcall, reps)
        assert (keep["index"][:nf] == g["index"]).all() and (keep["nbrs"][:nf] == g["nbrs"]).all()
        print(json.dumps(dict(what=f"{label}: host pointers, index + nbrs, arrays reused (la3dm_devmap_frontier_host)", median_s=med, min_s=lo_t,
                              max_s=hi_t, bytes_down=5 * nf)), flush=True)
        med, lo_t, hi_t = clock(lambda: md.frontier(lo, DIMS, open=OPEN, unknown=UNKNOWN, connectivity=c), reps)
        print(json.dumps(dict(what=f"{label}: python call (count, then fill: two calls, fresh arrays)", median_s=med, min_s=lo_t, max_s=hi_t)), flush=True)
        # (b) GPU consumer: the classes of the padded box stay in HBM, the stencil in torch
        bout = _lib.BoxOut(pt.data_ptr(), None, None, None)
        pd3 = np.array(pdims, np.uint32)
        offs = offsets(c)

        def box_dev():
            assert H.la3dm_devmap_box_device(dm, plo.ctypes.data, pd3.ctypes.data, C.byref(bout), C.byref(info)) == 0

        def stencil():
            p = pt.view(pdims)
            unk_t = ((p == 2) | (p == 3)).to(torch.uint8)
            s = torch.zeros(DIMS, dtype=torch.uint8, device=dev)
            for i, j, k in offs:
                s += unk_t[1 + i:1 + i + DIMS[0], 1 + j:1 + j + DIMS[1], 1 + k:1 + k + DIMS[2]]
            s *= (p[1:-1, 1:-1, 1:-1] == 0)
            idx = torch.nonzero(s.view(-1)).view(-1)
            nb = s.view(-1)[idx]
            torch.cuda.synchronize()
            return idx, nb
        box_dev()
        idx, nb = stencil()
        assert (idx.cpu().numpy() == g["index"]).all() and (nb.cpu().numpy() == g["nbrs"]).all()
        med_b, lo_b, hi_b = clock(box_dev, reps)
        med_s, lo_s, hi_s = clock(stencil, reps)
        print(json.dumps(dict(what=f"parent route (a), {label}: la3dm_devmap_box_device, cls of the padded box", median_s=med_b, min_s=lo_b, max_s=hi_b)), flush=True)
        print(json.dumps(dict(what=f"parent route (a), {label}: torch stencil on the device (shifted comparisons summed, nonzero, gather of nbrs)",
                              median_s=med_s, min_s=lo_s, max_s=hi_s, sum_with_box_s=med_b + med_s)), flush=True)
    if not args.trace:
        # (b) host consumer: the classes to the host, the stencil there, the list back up
        bkeep = np.zeros(padded, np.uint8)
        bout = _lib.BoxOut(bkeep.ctypes.data, None, None, None)
        pd3 = np.array(pdims, np.uint32)

        def bcall():
            assert H.la3dm_devmap_box_host(dm, plo.ctypes.data, pd3.ctypes.data, C.byref(bout), C.byref(info)) == 0
        med, lo_t, hi_t = clock(bcall, reps)
        assert (bkeep.reshape(pdims) == pcls).all()
        print(json.dumps(dict(what="parent route (b) 1/3: box of the padded region, cls only, to the host, array reused (la3dm_devmap_box_host)",
                              median_s=med, min_s=lo_t, max_s=hi_t, bytes_down=padded)), flush=True)
        mh = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)
        mh.insert_pointcloud(xyz, origin, *INSERT)
        med_b, lo_b, hi_b = clock(lambda: mh.box(plo, pdims, fields=()), 3)
        print(json.dumps(dict(what="host-mode map: box of the padded region, cls only (a loop over the host blocks, one thread)", median_s=med_b,
                              min_s=lo_b, max_s=hi_b)), flush=True)
        for c in CONNECTIVITIES:
            gh = mh.frontier(lo, DIMS, open=OPEN, unknown=UNKNOWN, connectivity=c)
            assert gh["n"] == lists[c]["n"] and (gh["index"] == lists[c]["index"]).all() and (gh["nbrs"] == lists[c]["nbrs"]).all()
            M = _lib.maplib()
            kout = _lib.FrontierOut(keep["index"].ctypes.data, keep["nbrs"].ctypes.data, None)

            def hcall():
                assert M.la3dm_map_frontier(mh._h, lo.ctypes.data, d3.ctypes.data, OPEN, UNKNOWN, c, 1, n, C.byref(kout), C.byref(found), None) == 0
            med, lo_t, hi_t = clock(hcall, 5)
            print(json.dumps(dict(what=f"parent route (b) 2/3, connectivity {c}: this library's host form (classes of the padded box from the host "
                                       "blocks + stencil + list, OpenMP), one call with arrays reused", median_s=med, min_s=lo_t, max_s=hi_t,
                                  omp_num_threads=os.environ.get("OMP_NUM_THREADS"))), flush=True)
            nf = lists[c]["n"]
            src = torch.from_numpy(lists[c]["index"].view(np.int32).copy()).pin_memory()
            src_n = torch.from_numpy(np.ascontiguousarray(lists[c]["nbrs"])).pin_memory()
            dst, dst_n = torch.zeros(nf, dtype=torch.int32, device=dev), torch.zeros(nf, dtype=torch.uint8, device=dev)

            def up():
                dst.copy_(src)
                dst_n.copy_(src_n)
                torch.cuda.synchronize()
            med, lo_t, hi_t = clock(up, reps)
            print(json.dumps(dict(what=f"parent route (b) 3/3, connectivity {c}: upload of the list (index + nbrs), pinned host memory", median_s=med,
                                  min_s=lo_t, max_s=hi_t, bytes_up=5 * nf)), flush=True)
    H.la3dm_devmap_destroy(dm)
    print(json.dumps(dict(what="yardstick", float4_copy_tb_per_s=COPY_TBS)), flush=True)


if __name__ == "__main__":
    main()
