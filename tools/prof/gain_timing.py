"""Timing of gain on the device-resident map against raycast_many over the same segments: the price of the sets.

Map: sim_structured scans 1 and 2, 0.1 m, block_depth 3 (the map of the region, distance, frontier and gain tests).
Region: the tests' recipe, 80 x 80 x 40 voxels whose voxel (0, 0, 0) holds the first sensor origin - (4.03, 4.03, 1.53).
Workload: 512 viewpoints (FREE voxels of the region, default_rng(41)) x 1024 offsets of 4 m (a Fibonacci sphere) =
524 288 segments; count UNKNOWN | MISSING, stop OCCUPIED, max_steps 4096.

Host clock round calls that end in a stream synchronise, arrays allocated once, the first call of each series left out,
medians:
  la3dm_devmap_gain_device     gain alone (the sets in the arena); every output (seen given: it is the working storage)
  la3dm_devmap_raycast_device  the same 524 288 segments with steps, flags and counts: the same walk without the marking
  la3dm_devmap_gain_host       upload of the origins and offsets, the launches, download of gain
The zeroing, the mark kernel and the count kernel alone come from a kernel trace of this same script, in a run of its own:
  rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/prof/gain_timing.py --trace
Also counted from the answers: rows marked per distinct voxel (what summing raycast_many's counts would overcount by).
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
DIMS = (80, 80, 40)
OFFSET = (-4.03, -4.03, -1.53)
COUNT, STOP, BUDGET = 0xC, 0x2, 4096
N, M = 512, 1024


def clock(fn, reps):
    fn()                                   # warm: code object, arenas
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), float(max(t))


def fan(m, radius):
    i = np.arange(m, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / m
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    return (np.stack([r * np.cos(phi), r * np.sin(phi), z], 1) * radius).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: only the device-pointer calls")
    ap.add_argument("--label", default="", help="copied into every line (which build is being timed)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gain_timing: no GPU visible (a timing taken elsewhere says nothing)")
    pcd = lambda i: os.path.join(ROOT, "tests", "golden", "data", "sim_structured", f"sim_structured_{i}.pcd")   # noqa: E731
    md = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    H = _lib.hip()
    lender = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)
    dm = C.c_void_p()
    assert H.la3dm_devmap_create(lender.ctx(), C.byref(dm)) == 0
    first = None
    for i in (1, 2):
        xyz, origin = la3dm_amd.load_pcd(pcd(i))
        first = origin if first is None else first
        md.insert_pointcloud(xyz, origin, *INSERT)
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3, *INSERT, None) == 0
    lo = (np.asarray(first, np.float32) + np.asarray(OFFSET, np.float32)).astype(np.float32)
    d3 = np.array(DIMS, np.uint32)
    W = (int(np.prod(DIMS)) + 31) // 32
    big = md.box(lo, DIMS, fields=())
    rng = np.random.default_rng(41)
    free = np.argwhere(big["cls"] == 0)
    pick = free[rng.choice(len(free), N, replace=False)]
    origins = (big["origin"] + pick.astype(np.float32) * np.float32(md.get_resolution())).astype(np.float32)
    offsets = fan(M, 4.0)
    starts = np.repeat(origins, M, 0)
    rays = np.ascontiguousarray(np.hstack([starts, (starts + np.tile(offsets, (N, 1))).astype(np.float32)]))
    ref = md.gain(lo, DIMS, origins, offsets, count=COUNT, stop=STOP, max_steps=BUDGET, fields=("gain", "started", "hits", "seen"))
    rc = md.raycast_many(rays[:, :3], rays[:, 3:], stop=STOP, max_steps=BUDGET)
    rows = int(rc["steps"].sum())
    unseen_rows = int(rc["counts"][:, 2:].sum())
    tag = dict(build=args.label) if args.label else {}
    print(json.dumps(dict(tag, what="workload", viewpoints=N, offsets=M, segments=N * M, region=DIMS, words_per_set=W, set_bytes=4 * N * W,
                          rows=rows, rows_per_ray=rows / (N * M), unknown_or_missing_rows=unseen_rows, sum_of_gains=int(ref["gain"].sum()),
                          unseen_rows_in_or_out_of_the_region_per_distinct_voxel=unseen_rows / max(1, int(ref["gain"].sum())),
                          hits=int(ref["hits"].sum()), gain_min=int(ref["gain"].min()), gain_max=int(ref["gain"].max()))), flush=True)
    dev = torch.device("cuda:0")
    d_o, d_f, d_r = torch.from_numpy(origins).to(dev), torch.from_numpy(offsets).to(dev), torch.from_numpy(rays).to(dev)
    t = dict(gain=torch.zeros(N, dtype=torch.int32, device=dev), started=torch.zeros(N, dtype=torch.int32, device=dev),
             hits=torch.zeros(N, dtype=torch.int32, device=dev), seen=torch.zeros(N * W, dtype=torch.int32, device=dev))
    r_steps, r_flags = torch.zeros(N * M, dtype=torch.int32, device=dev), torch.zeros(N * M, dtype=torch.uint8, device=dev)
    r_counts = torch.zeros(4 * N * M, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    reps = 5 if args.trace else args.reps

    def gain_call(fields):
        out = _lib.GainOut(*[t[k].data_ptr() if k in fields else None for k in ("gain", "started", "hits", "seen")])

        def call():
            assert H.la3dm_devmap_gain_device(dm, lo.ctypes.data, d3.ctypes.data, d_o.data_ptr(), N, d_f.data_ptr(), M, COUNT, STOP, BUDGET,
                                              C.byref(out), None) == 0
        return call
    ro = _lib.RaycastOut(r_steps.data_ptr(), r_flags.data_ptr(), None, None, None, None, None, None, None, r_counts.data_ptr())

    def ray_call():
        assert H.la3dm_devmap_raycast_device(dm, d_r.data_ptr(), N * M, STOP, BUDGET, C.byref(ro)) == 0
    series = (("gain: device pointers, gain alone (sets in the arena)", gain_call(("gain",))),
              ("raycast_many: device pointers, steps + flags + counts, the same segments", ray_call),
              ("gain: device pointers, gain + started + hits + seen (seen is the working storage)", gain_call(("gain", "started", "hits", "seen"))))
    med = {}
    for rnd in range(1 if args.trace else 2):          # the series alternate: two rounds each
        for what, fn in series:
            m_s, lo_s, hi_s = clock(fn, reps)
            med.setdefault(what, []).append(m_s)
            print(json.dumps(dict(tag, what=what, round=rnd, median_s=m_s, min_s=lo_s, max_s=hi_s, segments_per_s=N * M / m_s, rows_per_s=rows / m_s)), flush=True)
    for k in ("gain", "started", "hits"):
        assert (t[k].cpu().numpy().view(np.uint32) == ref[k]).all(), k            # the answer timed is the one the map gives
    assert (t["seen"].cpu().numpy().view(np.uint32).reshape(N, W) == ref["seen"]).all()
    assert (r_steps.cpu().numpy().view(np.uint32) == rc["steps"]).all()
    if not args.trace:
        g, r = (float(np.median(med[series[i][0]])) for i in (0, 1))
        print(json.dumps(dict(tag, what="ratio: gain (gain alone) / raycast_many (counts), medians of the rounds", gain_s=g, raycast_s=r, ratio=g / r)), flush=True)
        keep = np.zeros(N, np.uint32)
        ko = _lib.GainOut(keep.ctypes.data, None, None, None)

        def host_call():
            assert H.la3dm_devmap_gain_host(dm, lo.ctypes.data, d3.ctypes.data, origins.ctypes.data, N, offsets.ctypes.data, M, COUNT, STOP, BUDGET,
                                            C.byref(ko), None) == 0
        m_s, lo_s, hi_s = clock(host_call, args.reps)
        assert (keep == ref["gain"]).all()
        print(json.dumps(dict(tag, what="gain: host pointers, gain alone (la3dm_devmap_gain_host)", median_s=m_s, min_s=lo_s, max_s=hi_s)), flush=True)
    H.la3dm_devmap_destroy(dm)


if __name__ == "__main__":
    main()
