"""Measurement of save / load on the device-resident map.  Not a test and not part of bench.py.

Maps (BGK, 0.1 m): BASELINE configs[1]'s synthetic 200k-ray scan after 1 and after 5 inserts from the bench's sensor poses, at
block_depth 3 and 4; the 12 sim_structured scans at block_depth 3.  Every map is a bare la3dm_devmap on a lent context, so
that la3dm_devmap_download — the only snapshot the map offered before — runs on the very same pool in the same process.

Per map, one JSON line with
  bytes        the stream against the raw pool (8 + 9 nodes_per_block bytes per block), leaves per block
  pack         la3dm_devmap_pack_host into a buffer of the known size (count, scan, read-back, emit, one copy, one
               synchronise), the size-only call (count, scan, read-back), and la3dm_devmap_download of the same pool; host
               clock round calls that end in a stream synchronise, buffers allocated and touched once, median / min / max
  unpack       la3dm_devmap_unpack_host into a fresh device map (validation, pool allocation, upload, expand, table) against
               re-inserting the scans into a fresh device map, the only way back before; and the validation alone
               (la3dm_pack_info)
The kernels alone come from a kernel trace of this script in a run of its own:
  rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/pack_bench.py --trace"""
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


def clock(fn, reps):
    fn()                                   # warm: code objects, arenas
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
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

    def close(self):
        self.H.la3dm_devmap_destroy(self.dm)


def measure(name, depth, scans, insert, reps, trace):
    H = _lib.hip()
    lender = la3dm_amd.BGKOctoMap(**dict(la3dm_amd.BGK_YAML, block_depth=depth), device=0).set_device_resident(False)
    ctx = lender.ctx()
    scans = [(np.ascontiguousarray(x, np.float32), o) for x, o in scans]
    d = Devmap(H, ctx)
    for xyz, origin in scans:
        d.insert(xyz, origin, insert)
    nb, npb = C.c_uint32(), C.c_uint32()
    d.ok(H.la3dm_devmap_block_count(d.dm, C.byref(nb), C.byref(npb)))
    nb, npb = nb.value, npb.value
    size = C.c_uint64(0)
    d.ok(H.la3dm_devmap_pack_host(d.dm, None, 0, C.byref(size)))
    stream = np.zeros(size.value, np.uint8)
    keys, A, B, S = np.zeros(nb, np.int64), np.zeros(nb * npb, np.float32), np.zeros(nb * npb, np.float32), np.zeros(nb * npb, np.uint8)

    def pack():
        d.ok(H.la3dm_devmap_pack_host(d.dm, stream.ctypes.data, stream.size, C.byref(size)))

    def pack_size():
        d.ok(H.la3dm_devmap_pack_host(d.dm, None, 0, C.byref(size)))

    def download():
        d.ok(H.la3dm_devmap_download(d.dm, keys.ctypes.data, A.ctypes.data, B.ctypes.data, S.ctypes.data))

    def unpack():
        f = Devmap(H, ctx)
        t0 = time.perf_counter()
        f.ok(H.la3dm_devmap_unpack_host(f.dm, stream.ctypes.data, stream.size))
        dt = time.perf_counter() - t0
        f.close()
        return dt

    def reinsert():
        f = Devmap(H, ctx)
        t0 = time.perf_counter()
        for xyz, origin in scans:
            f.insert(xyz, origin, insert)
        dt = time.perf_counter() - t0
        f.close()
        return dt

    if trace:
        for _ in range(3):
            pack()
            unpack()
        d.close()
        return
    hdr = _lib.PackHeader()
    out = dict(map=name, block_depth=depth, scans=len(scans), n_blocks=nb, nodes_per_block=npb)
    pack()
    assert H.la3dm_pack_info(stream.ctypes.data, stream.size, C.byref(hdr)) == 0
    raw = nb * (8 + 9 * npb)
    out["bytes"] = dict(stream=int(size.value), raw_pool=raw, ratio=size.value / raw, n_leaves=int(hdr.n_leaves),
                        leaves_per_block=hdr.n_leaves / nb, finest_cells_per_block=8 ** (depth - 1))
    # pack and download alternate, so that both see the same neighbours on the host
    tp, td, ts = [], [], []
    download()
    for _ in range(reps):
        for fn, acc in ((pack, tp), (download, td), (pack_size, ts)):
            t0 = time.perf_counter()
            fn()
            acc.append(time.perf_counter() - t0)
    ms = lambda t: dict(median_ms=1e3 * float(np.median(t)), min_ms=1e3 * float(min(t)), max_ms=1e3 * float(max(t)))   # noqa: E731
    out["pack"] = dict(pack_host=ms(tp), size_only=ms(ts), download=ms(td))
    unpack()
    tu = [unpack() for _ in range(reps)]
    reinsert()
    tr = [reinsert() for _ in range(max(3, reps // 3))]
    out["unpack"] = dict(unpack_host=ms(tu), reinsert_scans=ms(tr),
                         validate_only=clock(lambda: H.la3dm_pack_info(stream.ctypes.data, stream.size, C.byref(hdr)), reps))
    print(json.dumps(out), flush=True)
    d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: pack and unpack only, three times per map")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pack_bench: no GPU visible (a timing taken elsewhere says nothing)")
    synth = [la3dm_amd.synthetic_scan(200000, origin=p) for p in SEQ_POSES]
    from la3dm_amd import load_pcd
    sim = [load_pcd(os.path.join(ROOT, "tests", "golden", "data", "sim_structured", f"sim_structured_{i}.pcd")) for i in range(1, 13)]
    for depth in (3, 4):
        measure("configs[1] synthetic, 1 insert", depth, synth[:1], (0.1, 0.5, -1.0), args.reps, args.trace)
        measure("configs[1] synthetic, 5 inserts", depth, synth, (0.1, 0.5, -1.0), args.reps, args.trace)
    measure("sim_structured, 12 scans", 3, sim, (0.1, 0.5, 8.0), args.reps, args.trace)


if __name__ == "__main__":
    main()
