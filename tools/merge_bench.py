"""Measurement of merge on the device-resident map.  Not a test and not part of bench.py.

Pairs of maps (BGK, 0.1 m), destination and source built from different scans that overlap: BASELINE configs[1]'s synthetic
200k-ray scan from the bench's sensor poses 0 .. 2 against poses 2 .. 4, at block_depth 3 and 4; sim_structured scans 1 .. 6
against 7 .. 12 at block_depth 3.  Both are packed once; every repetition starts from a fresh device map with the
destination's stream unpacked into it (not timed).

Per pair, one JSON line with
  merge      la3dm_devmap_merge_host of the source's stream (validation, upload, find, scan, read-back, grow, insert, fuse,
             read-back), host clock round the call, which ends in a stream synchronise; median / min / max
  replaced   what it replaces, step by step: la3dm_devmap_download of the destination's pool; the host header's merge over the
             same blocks (a host-mode map holding the destination, merge(stream): validation, expansion, merge_block per
             block); la3dm_devmap_unpack_host of the result into a fresh device map.  Rebuilding host blocks from the download
             and packing the result on the host are left out, so the sum is a lower bound of that path
  fuse_bytes dm_merge_fuse's traffic from the streams: per stream block 4 W mask bytes and 9 nodes_per_block written; 9 B per
             source leaf; per block the map had, nodes_per_block state bytes and 8 B per leaf of it
The kernels alone come from a kernel trace of this script in a run of its own:
  rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/merge_bench.py --trace"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import la3dm_amd  # noqa: E402
from la3dm_amd import _lib  # noqa: E402

SEQ_POSES = [None, (1.5, 0.5, 1.0), (-1.5, 1.0, 1.2), (0.5, -2.0, 0.9), (2.5, 2.0, 1.1)]   # bench.py's e2e sequence


def ms(t):
    return dict(median_ms=1e3 * float(np.median(t)), min_ms=1e3 * float(min(t)), max_ms=1e3 * float(max(t)))


class Devmap:
    def __init__(self, H, ctx):
        self.H, self.ctx, self.dm = H, ctx, C.c_void_p()
        self.ok(H.la3dm_devmap_create(ctx, C.byref(self.dm)))

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(self.H.la3dm_last_error(self.ctx).decode())

    def insert(self, xyz, origin, insert):
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        self.ok(self.H.la3dm_devmap_insert_pointcloud_host(self.dm, xyz.ctypes.data, xyz.shape[0], 3, o3, *insert, None))

    def pack(self):
        size = C.c_uint64(0)
        self.ok(self.H.la3dm_devmap_pack_host(self.dm, None, 0, C.byref(size)))
        buf = np.zeros(size.value, np.uint8)
        self.ok(self.H.la3dm_devmap_pack_host(self.dm, buf.ctypes.data, buf.size, C.byref(size)))
        return buf

    def close(self):
        self.H.la3dm_devmap_destroy(self.dm)


def sections(stream, npb):
    """keys and leaves per block of a stream (layout: include/la3dm_hip.h)"""
    nb = int(stream[32:40].view("<u8")[0])
    a16 = lambda v: (v + 15) & ~15   # noqa: E731
    off = a16(128 + 8 * nb)
    return stream[128:128 + 8 * nb].view("<i8"), np.diff(stream[off:off + 4 * (nb + 1)].view("<u4").astype(np.int64))


def measure(name, depth, dst_scans, src_scans, insert, reps, trace):
    H = _lib.hip()
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    lender = la3dm_amd.BGKOctoMap(**params, device=0).set_device_resident(False)
    ctx = lender.ctx()
    streams = []
    for scans in (dst_scans, src_scans):
        d = Devmap(H, ctx)
        for xyz, origin in scans:
            d.insert(np.ascontiguousarray(xyz, np.float32), origin, insert)
        streams.append(d.pack())
        d.close()
    dst, src = streams
    npb = (8 ** depth - 1) // 7
    stats = _lib.MergeStats()

    def merged():
        f = Devmap(H, ctx)
        f.ok(H.la3dm_devmap_unpack_host(f.dm, dst.ctypes.data, dst.size))
        t0 = time.perf_counter()
        f.ok(H.la3dm_devmap_merge_host(f.dm, src.ctypes.data, src.size, C.byref(stats)))
        dt = time.perf_counter() - t0
        return f, dt

    if trace:
        for _ in range(3):
            merged()[0].close()
        return
    f, _ = merged()                                # warm: code objects, arenas
    result = f.pack()
    f.close()
    tm = []
    for _ in range(reps):
        f, dt = merged()
        f.close()
        tm.append(dt)
    # the replaced path
    f = Devmap(H, ctx)
    f.ok(H.la3dm_devmap_unpack_host(f.dm, dst.ctypes.data, dst.size))
    nb = int(dst[32:40].view("<u8")[0])
    keys, A, B, S = np.zeros(nb, np.int64), np.zeros(nb * npb, np.float32), np.zeros(nb * npb, np.float32), np.zeros(nb * npb, np.uint8)
    td, th, tu = [], [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        f.ok(H.la3dm_devmap_download(f.dm, keys.ctypes.data, A.ctypes.data, B.ctypes.data, S.ctypes.data))
        td.append(time.perf_counter() - t0)
        host = la3dm_amd.BGKOctoMap(**params, device=-1).unpack(dst)
        t0 = time.perf_counter()
        host.merge(src)
        th.append(time.perf_counter() - t0)
        g = Devmap(H, ctx)
        t0 = time.perf_counter()
        g.ok(H.la3dm_devmap_unpack_host(g.dm, result.ctypes.data, result.size))
        tu.append(time.perf_counter() - t0)
        g.close()
    f.close()
    td, th, tu = td[1:], th[1:], tu[1:]
    dk, dl = sections(dst, npb)
    sk, sl = sections(src, npb)
    had = np.isin(sk, dk)
    leaves_of = dict(zip(dk.tolist(), dl.tolist()))
    W = (npb + 31) // 32
    fuse = int(sk.size * (4 * W + 4 + 9 * npb) + 9 * sl.sum() + had.sum() * npb + 8 * sum(leaves_of[k] for k in sk[had].tolist()))
    out = dict(map=name, block_depth=depth, dst_blocks=nb, src_blocks=int(sk.size), stream_bytes=int(src.size),
               stats={k: int(getattr(stats, k)) for k, _ in _lib.MergeStats._fields_}, merge=ms(tm),
               replaced=dict(download=ms(td), host_merge=ms(th), unpack_host=ms(tu),
                             sum_of_medians_ms=1e3 * float(np.median(td) + np.median(th) + np.median(tu))),
               fuse_bytes=fuse)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: three merges per pair, nothing else")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("merge_bench: no GPU visible (a timing taken elsewhere says nothing)")
    synth = [la3dm_amd.synthetic_scan(200000, origin=p) for p in SEQ_POSES]
    from la3dm_amd import load_pcd
    sim = [load_pcd(os.path.join(ROOT, "tests", "golden", "data", "sim_structured", f"sim_structured_{i}.pcd")) for i in range(1, 13)]
    for depth in (3, 4):
        measure("configs[1] synthetic, poses 0-2 + poses 2-4", depth, synth[:3], synth[2:], (0.1, 0.5, -1.0), args.reps, args.trace)
    measure("sim_structured, scans 1-6 + scans 7-12", 3, sim[:6], sim[6:], (0.1, 0.5, 8.0), args.reps, args.trace)


if __name__ == "__main__":
    main()
