"""Timing of BGKOctoMap.clusters on the device-resident map against the route the map offered before it.

Map: sim_structured scans 1, 2 and 3 (0.1 m, block_depth 3) — the map of tools/prof/travel_timing.py.
Regions (DESIGN 3.13's two):
  recipe   the tests' 80 x 80 x 40 region (voxel (0, 0, 0) holds the first origin - (4.03, 4.03, 1.53)): 500 bricks
  large    256 x 256 x 32 voxels (voxel (0, 0, 0) holds that origin - (12.8, 12.8, 1.6)): 4096 bricks
Queries:
  tiled      frontier's default list, tile 8, connectivity 26, min_size 8 — the goal set
  sheet 6    the list untiled at connectivity 6
  sheet 26   the list untiled at connectivity 26
  occupied   member OCCUPIED from the classes, untiled, connectivity 26

 (a) the calls, host clock round calls that end in a stream synchronise, output arrays allocated once, medians of `reps`:
       device pointers  la3dm_devmap_clusters_device on a pool of its own with the same scans: label, of_member and every
                        record; the same with cap 0 (label and of_member alone); cap 0 and no array (count only)
       host pointers    la3dm_devmap_clusters_host: label, of_member and every record
       no member        the count-only call with a list of 0 entries: the set-up — clears, sizes, flags, scan and the
                        synchronises, no round
     and, derived from them: per round = (count only - no member) / rounds launched; the finish = the full call - the
     rounds; the accumulators = the full call - the call with cap 0 (record init, records, rep, emit and their storage).
 (b) the route of a client without this call: frontier's list fetched (la3dm_devmap_frontier_host) or the classes
     (la3dm_devmap_box_host, cls alone), then this library's host form on the CPU, timed on a host-mode map with the same
     scans (its own read of the classes from the host blocks included).

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
REGIONS = (("recipe", (80, 80, 40), (4.03, 4.03, 1.53)), ("large", (256, 256, 32), (12.8, 12.8, 1.6)))
CASES = (("tiled", dict(listed=True, mask=FREE_M, connectivity=26, tile=8, min_size=8)),
         ("sheet 6", dict(listed=True, mask=FREE_M, connectivity=6, tile=0, min_size=1)),
         ("sheet 26", dict(listed=True, mask=FREE_M, connectivity=26, tile=0, min_size=1)),
         ("occupied", dict(listed=False, mask=OCC_M, connectivity=26, tile=0, min_size=1)))
NAMES = ("label", "of_member", "first", "size", "lo", "hi", "sum", "rep")


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
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("clusters_timing: no GPU visible (a timing taken elsewhere says nothing)")
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
    dev = torch.device("cuda:0")
    reps = args.reps
    for name, dims, back in REGIONS:
        lo = (np.asarray(first, np.float32) - np.array(back, np.float32)).astype(np.float32)
        d3 = np.array(dims, np.uint32)
        n = int(np.prod(dims))
        listed = md.frontier(lo, dims)["index"]
        nl = int(listed.size)
        d_list = torch.from_numpy(listed.view(np.int32).copy()).to(dev)
        print(json.dumps(dict(what=f"{name}: region", dims=dims, voxels=n, bricks=int(np.prod([(v + 7) // 8 for v in dims])), listed=nl)), flush=True)
        for case, kw in CASES:
            label = f"{name}, {case}"
            members = listed if kw["listed"] else None
            q = dict(member=kw["mask"], connectivity=kw["connectivity"], tile=kw["tile"], min_size=kw["min_size"])
            fields = ("label", "of_member") if kw["listed"] else ("label",)
            g = md.clusters(lo, dims, members=members, fields=fields, **q)
            gh = mh.clusters(lo, dims, members=members, fields=fields, **q)
            assert all((g[k] == gh[k]).all() for k in fields + NAMES[2:]) and g["n"] == gh["n"]      # the answer timed is the right one
            launched = -(-(g["rounds"] + 1) // la3dm_amd.CLUSTERS_BATCH) * la3dm_amd.CLUSTERS_BATCH
            print(json.dumps(dict(what=f"workload: {label}", n=g["n"], n_members=g["n_members"], n_dropped=g["n_dropped"], largest=g["largest"],
                                  rounds=g["rounds"], rounds_launched=launched, brick_runs=g["brick_runs"], capped=g["capped"], **q)), flush=True)
            cap = max(g["n"], 1)
            nm = nl if kw["listed"] else 0
            sizes = dict(label=n, of_member=max(nm, 1), first=cap, size=cap, lo=3 * cap, hi=3 * cap, sum=3 * cap, rep=cap)
            t = {k: torch.zeros(sizes[k], dtype=torch.int64 if k == "sum" else torch.int32, device=dev) for k in NAMES}
            h = {k: np.zeros(sizes[k], np.uint64 if k == "sum" else np.uint32) for k in NAMES}
            torch.cuda.synchronize()
            stats, found = _lib.ClustersStats(), C.c_uint32(0)

            def params(mem, k, c):
                return _lib.ClustersParams(kw["mask"], 1 if kw["listed"] else 0, kw["connectivity"], kw["tile"], kw["min_size"], k, mem if k else None, c)

            def out_of(ptr, records=True, dense=True):
                use = [k for k in NAMES if (k in ("label", "of_member") and dense and (k == "label" or kw["listed"])) or (k not in ("label", "of_member") and records)]
                return _lib.ClustersOut(*[ptr(k) if k in use else None for k in NAMES])

            def dev_call(out, k, c):
                p = params(d_list.data_ptr(), k, c)
                assert H.la3dm_devmap_clusters_device(dm, lo.ctypes.data, d3.ctypes.data, C.byref(p), C.byref(out), C.byref(found), C.byref(stats), None) == 0
            dptr = lambda k: t[k].data_ptr()   # noqa: E731
            full = out_of(dptr)
            med, lo_t, hi_t = clock(lambda: dev_call(full, nm, cap), reps)
            assert found.value == g["n"] and stats.rounds == g["rounds"] and (t["label"].cpu().numpy().view(np.uint32) == g["label"].reshape(-1)).all()
            assert (t["rep"][:g["n"]].cpu().numpy().view(np.uint32) == g["rep"]).all()
            med_l, _, _ = clock(lambda: dev_call(out_of(dptr, records=False), nm, 0), reps)
            med_c, _, _ = clock(lambda: dev_call(out_of(dptr, records=False, dense=False), nm, 0), reps)
            empty = _lib.ClustersParams(kw["mask"], 1, kw["connectivity"], kw["tile"], kw["min_size"], 0, None, 0)

            def no_member():
                assert H.la3dm_devmap_clusters_device(dm, lo.ctypes.data, d3.ctypes.data, C.byref(empty), None, C.byref(found), None, None) == 0
            med_0, _, _ = clock(no_member, reps)
            per_round = (med_c - med_0) / launched
            print(json.dumps(dict(what=f"{label}: clusters, device pointers", full_median_s=med, full_min_s=lo_t, full_max_s=hi_t, cap0_median_s=med_l,
                                  count_only_median_s=med_c, no_member_median_s=med_0, per_round_s=per_round, batches=launched // la3dm_amd.CLUSTERS_BATCH,
                                  finish_s=med - per_round * launched, accumulators_s=med - med_l)), flush=True)
            hptr = lambda k: h[k].ctypes.data   # noqa: E731
            hout = out_of(hptr)

            def host_call():
                p = params(listed.ctypes.data, nm, cap)
                assert H.la3dm_devmap_clusters_host(dm, lo.ctypes.data, d3.ctypes.data, C.byref(p), C.byref(hout), C.byref(found), C.byref(stats), None) == 0
            med_h, lo_t, hi_t = clock(host_call, reps)
            assert (h["label"] == g["label"].reshape(-1)).all() and (h["rep"][:g["n"]] == g["rep"]).all()
            print(json.dumps(dict(what=f"{label}: clusters, host pointers", median_s=med_h, min_s=lo_t, max_s=hi_t)), flush=True)
            # (b) the list or the classes to the host, the host form there
            if kw["listed"]:
                idx = np.zeros(max(nl, 1), np.uint32)
                fo = _lib.FrontierOut(idx.ctypes.data, None, None)
                nf = C.c_uint64(0)

                def fetch():
                    assert H.la3dm_devmap_frontier_host(dm, lo.ctypes.data, d3.ctypes.data, FREE_M, 0xC, 6, 1, nl, C.byref(fo), C.byref(nf), None) == 0
            else:
                cls = np.zeros(n, np.uint8)
                bout = _lib.BoxOut(cls.ctypes.data, None, None, None)

                def fetch():
                    assert H.la3dm_devmap_box_host(dm, lo.ctypes.data, d3.ctypes.data, C.byref(bout), None) == 0
            med_b, _, _ = clock(fetch, reps)

            def flood():
                p = params(listed.ctypes.data, nm, cap)
                assert M.la3dm_map_clusters(mh._h, lo.ctypes.data, d3.ctypes.data, C.byref(p), C.byref(hout), C.byref(found), C.byref(stats), None) == 0
            med_f, lo_f, hi_f = clock(flood, 5)
            print(json.dumps(dict(what=f"parent route, {label}: {'frontier list' if kw['listed'] else 'box (cls alone)'} fetched + this library's host form on the CPU",
                                  fetch_median_s=med_b, host_form_median_s=med_f, host_form_min_s=lo_f, host_form_max_s=hi_f, sum_s=med_b + med_f,
                                  ratio_to_host_pointers=(med_b + med_f) / med_h, ratio_to_device_pointers=(med_b + med_f) / med,
                                  omp_num_threads=os.environ.get("OMP_NUM_THREADS"))), flush=True)
    H.la3dm_devmap_destroy(dm)


if __name__ == "__main__":
    main()
