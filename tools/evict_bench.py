"""Measurement of pack_region and erase_region on the device-resident map.  Not a test and not part of
bench.py.

Maps (BGK, 0.1 m), those of §3.15 / §3.16: BASELINE configs[1]'s synthetic 200k-ray scan from the bench's five sensor poses at
block_depth 3 and 4, and the 12 sim_structured scans at block_depth 3.  Each is built and packed once; every repetition
starts from a fresh device map with that stream unpacked into it (not timed).  Regions: a slab of block keys along x between
two quantiles of the blocks' x fields that keeps about half of the blocks, and one that keeps about a tenth.

Per map and region, one JSON line with
  pack_region   la3dm_devmap_pack_region_host of the kept box (inside = 1), sizing call and filling call together
  erase_region  la3dm_devmap_erase_region_host of everything else (inside = 0): the rolling window
  replaced      the path they replace, step by step, in the same run: la3dm_devmap_pack_host of the whole map (sizing and
                filling call); the host cut of the stream (numpy, this file's cut(): keys, masks and the leaf ranges of the
                kept blocks gathered into a new stream); la3dm_devmap_unpack_host of the cut stream into a fresh map.
                pack_region stands against pack + cut, erase_region against pack + cut + unpack_host
  move_bytes    what dm_evict_move must move: n_moved x (9 nodes_per_block + 8) bytes read and as many written
Host clock round calls that end in a stream synchronise, profiler off; median / min / max of --reps.  The kernels alone come
from a kernel trace of this script in a run of its own:
  rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/evict_bench.py --trace
--base: pack and merge only (la3dm_devmap_pack_host of every map; la3dm_devmap_merge_host of the half slab's stream into
the map that lost it) — entry points the parent commit has too, to compare the two commits."""
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
FIELD_MAX = 0xFFFFF


def ms(t):
    return dict(median_ms=1e3 * float(np.median(t)), min_ms=1e3 * float(min(t)), max_ms=1e3 * float(max(t)))


def a16(v):
    return (v + 15) & ~15


def layout(nb, nl, npb):
    W = (npb + 31) // 32
    if nb == 0:
        return W, [128] * 7
    keys = 128
    off = a16(keys + 8 * nb)
    mask = a16(off + 4 * (nb + 1))
    state = a16(mask + 4 * nb * W)
    A = a16(state + nl)
    B = a16(A + 4 * nl)
    return W, [keys, off, mask, state, A, B, a16(B + 4 * nl)]


def cut(stream, npb, keep):
    """the stream of the blocks keep[b] of a stream, in its order (layout: include/la3dm_hip.h)"""
    nb, nl = (int(v) for v in stream[32:48].view("<u8"))
    W, (k0, o0, m0, s0, a0, b0, _) = layout(nb, nl, npb)
    off = stream[o0:o0 + 4 * (nb + 1)].view("<u4").astype(np.int64)
    cnt = np.diff(off)[keep]
    new_off = np.zeros(cnt.size + 1, np.int64)
    np.cumsum(cnt, out=new_off[1:])
    leaves = np.repeat(off[:-1][keep] - new_off[:-1], cnt) + np.arange(new_off[-1])
    n2, l2 = int(cnt.size), int(new_off[-1])
    _, (k1, o1, m1, s1, a1, b1, total) = layout(n2, l2, npb)
    out = np.zeros(total, np.uint8)
    out[:128] = stream[:128]
    out[32:56].view("<u8")[:] = (n2, l2, total)
    if n2:
        out[k1:k1 + 8 * n2] = stream[k0:k0 + 8 * nb].reshape(nb, 8)[keep].reshape(-1)
        out[o1:o1 + 4 * (n2 + 1)] = new_off.astype("<u4").view(np.uint8)
        out[m1:m1 + 4 * n2 * W] = stream[m0:m0 + 4 * nb * W].reshape(nb, 4 * W)[keep].reshape(-1)
        out[s1:s1 + l2] = stream[s0:s0 + nl][leaves]
        out[a1:a1 + 4 * l2] = stream[a0:a0 + 4 * nl].reshape(nl, 4)[leaves].reshape(-1)
        out[b1:b1 + 4 * l2] = stream[b0:b0 + 4 * nl].reshape(nl, 4)[leaves].reshape(-1)
    return out


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

    def pack_region(self, klo, khi, inside):
        size = C.c_uint64(0)
        self.ok(self.H.la3dm_devmap_pack_region_host(self.dm, klo, khi, inside, None, 0, C.byref(size)))
        buf = np.zeros(size.value, np.uint8)
        self.ok(self.H.la3dm_devmap_pack_region_host(self.dm, klo, khi, inside, buf.ctypes.data, buf.size, C.byref(size)))
        return buf

    def unpack(self, s):
        self.ok(self.H.la3dm_devmap_unpack_host(self.dm, s.ctypes.data, s.size))
        return self

    def close(self):
        self.H.la3dm_devmap_destroy(self.dm)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def measure(name, depth, scans, insert, reps, mode):
    H = _lib.hip()
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    lender = la3dm_amd.BGKOctoMap(**params, device=0).set_device_resident(False)
    ctx = lender.ctx()
    d = Devmap(H, ctx)
    for xyz, origin in scans:
        d.insert(np.ascontiguousarray(xyz, np.float32), origin, insert)
    whole = d.pack()
    d.close()
    npb = (8 ** depth - 1) // 7
    nb = int(whole[32:40].view("<u8")[0])
    keys = whole[128:128 + 8 * nb].view("<i8")
    x = (keys >> 40) & FIELD_MAX
    for label, (q0, q1) in (("half", (0.25, 0.75)), ("tenth", (0.45, 0.55))):
        lo, hi = int(np.quantile(x, q0)), int(np.quantile(x, q1))
        klo, khi = (C.c_int32 * 3)(lo, 0, 0), (C.c_int32 * 3)(hi, FIELD_MAX, FIELD_MAX)
        keep = (x >= lo) & (x <= hi)
        if mode == "trace":
            for _ in range(3):
                f = Devmap(H, ctx).unpack(whole)
                f.pack_region(klo, khi, 1)
                f.ok(H.la3dm_devmap_erase_region_host(f.dm, klo, khi, 0, None))
                f.close()
            continue
        if mode == "base":
            if label == "tenth":
                continue
            gone, left = cut(whole, npb, ~keep), cut(whole, npb, keep)
            tp, tm = [], []
            for r in range(reps + 1):
                f = Devmap(H, ctx).unpack(whole)
                tp.append(timed(f.pack)[0])
                f.close()
                f = Devmap(H, ctx).unpack(left)
                tm.append(timed(lambda: f.ok(H.la3dm_devmap_merge_host(f.dm, gone.ctypes.data, gone.size, None)))[0])
                f.close()
            print(json.dumps(dict(map=name, block_depth=depth, blocks=nb, pack=ms(tp[1:]), merge_blocks=int((~keep).sum()), merge=ms(tm[1:]))), flush=True)
            continue
        st = _lib.EraseStats()
        tr, te, tpk, tc, tu = [], [], [], [], []
        for r in range(reps + 1):       # (the first repetition warms code objects and arenas and is dropped)
            f = Devmap(H, ctx).unpack(whole)
            dt, sub = timed(lambda: f.pack_region(klo, khi, 1))
            tr.append(dt)
            dt, full = timed(f.pack)
            tpk.append(dt)
            dt, kept = timed(lambda: cut(full, npb, keep))
            tc.append(dt)
            g = Devmap(H, ctx)
            tu.append(timed(lambda: g.unpack(kept))[0])
            te.append(timed(lambda: f.ok(H.la3dm_devmap_erase_region_host(f.dm, klo, khi, 0, C.byref(st))))[0])
            if r == 0:
                nb_f, nb_g, npb_ = C.c_uint32(), C.c_uint32(), C.c_uint32()
                H.la3dm_devmap_block_count(f.dm, C.byref(nb_f), C.byref(npb_))
                H.la3dm_devmap_block_count(g.dm, C.byref(nb_g), C.byref(npb_))
                assert sub.size == kept.size and (sub == kept).all() and nb_f.value == nb_g.value, "the two paths give one stream and one block count"
            f.close()
            g.close()
        tr, te, tpk, tc, tu = (t[1:] for t in (tr, te, tpk, tc, tu))
        med = lambda *ts: 1e3 * float(sum(np.median(t) for t in ts))   # noqa: E731
        print(json.dumps(dict(map=name, block_depth=depth, region=label, blocks=nb, kept=int(keep.sum()), stream_bytes=int(whole.size),
                              kept_stream_bytes=int(kept.size), stats={k: int(getattr(st, k)) for k, _ in _lib.EraseStats._fields_},
                              pack_region=ms(tr), erase_region=ms(te),
                              replaced=dict(pack_host=ms(tpk), host_cut_numpy=ms(tc), unpack_host=ms(tu), pack_plus_cut_ms=med(tpk, tc),
                                            pack_cut_unpack_ms=med(tpk, tc, tu)),
                              move_bytes=dict(read=int(st.n_moved) * (9 * npb + 8), written=int(st.n_moved) * (9 * npb + 8)))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: three pack_region + erase_region per map and region, nothing else")
    ap.add_argument("--base", action="store_true", help="pack and merge only (entry points the parent commit has too)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("evict_bench: no GPU visible (a timing taken elsewhere says nothing)")
    mode = "trace" if args.trace else "base" if args.base else "full"
    synth = [la3dm_amd.synthetic_scan(200000, origin=p) for p in SEQ_POSES]
    from la3dm_amd import load_pcd
    sim = [load_pcd(os.path.join(ROOT, "tests", "golden", "data", "sim_structured", f"sim_structured_{i}.pcd")) for i in range(1, 13)]
    for depth in (3, 4):
        measure("configs[1] synthetic, 5 inserts", depth, synth, (0.1, 0.5, -1.0), args.reps, mode)
    measure("sim_structured, 12 scans", 3, sim, (0.1, 0.5, 8.0), args.reps, mode)


if __name__ == "__main__":
    main()
