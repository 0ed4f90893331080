"""Measurement of diff on the device-resident map.  Not a test and not part of bench.py.

The map is merge_bench's: BGK, 0.1 m, block_depth 3, BASELINE configs[1]'s synthetic 200k-ray scan from the bench's five
sensor poses.  THEN is a pack() taken on the way, NOW the live map after the remaining scans:
  small  the snapshot after four scans, one further scan (the publisher's case: a scan changes a small share of the cells)
  large  the snapshot after one scan, four further scans

Per case, one JSON line with (host clock round calls that end in a stream synchronise; median / min / max)
  count        diff, class only, cap = 0: the 5 x 5 table and n, no list
  list         diff, class only, cap = n: block_key, cell, code of every changed cell
  full         diff with values of every class, cap = n: block_key, cell, code, centre, A, B
               (list and full: la3dm_map_diff into buffers that were allocated and written before the first timed call)
  pack         pack() of the live map — what a user of the parent commit has to do first
  host_diff    the host-mode map's diff of the same stream on an unpack()ed copy of the live map (the unpack is not timed):
               the CPU denominator for "expand both streams on the host and compare".  It is the library's own host rule
               (host/diff_block.h, one thread), not the numpy model of the tests
  replaced     pack + host_diff, the sum of the medians: a lower bound of the route at the parent commit, which would also
               have to expand the live map's stream
The kernels alone come from a kernel trace of this script in a run of its own:
  rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/diff_bench.py --trace"""
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
INSERT = (0.1, 0.5, -1.0)
ALL_FIELDS = ("block_key", "cell", "code", "centre", "A", "B")


def ms(t):
    return dict(median_ms=1e3 * float(np.median(t)), min_ms=1e3 * float(min(t)), max_ms=1e3 * float(max(t)))


def timed(fn, reps):
    fn()   # warm: code objects, arenas
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return ms(t)


def filler(m, then, value_mask, fields, n):
    """la3dm_map_diff into buffers of n entries that exist and were written before the first timed call"""
    bufs = {f: np.ones((n, w) if w > 1 else n, t) for f, (t, w) in m._DIFF_FIELDS.items() if f in fields}
    out = _lib.DiffOut(*[bufs[f].ctypes.data if f in bufs else None for f, _ in _lib.DiffOut._fields_])
    params, found, stats = _lib.DiffParams(la3dm_amd.DIFF_PAIRS_CHANGED, value_mask, 1), C.c_uint64(0), _lib.DiffStats()

    def call():
        rc = _lib.maplib().la3dm_map_diff(m._h, then.ctypes.data, then.size, C.byref(params), n, C.byref(out), C.byref(found), C.byref(stats))
        assert rc == 0 and found.value == n
    call.bufs = bufs   # (out holds bare addresses: the arrays live as long as the call does)
    return call


def measure(name, scans, n_then, reps, trace):
    params = dict(la3dm_amd.BGK_YAML, block_depth=3)
    m = la3dm_amd.BGKOctoMap(**params, device=0)
    then = None
    for i, (xyz, origin) in enumerate(scans):
        m.insert_pointcloud(xyz, origin, *INSERT)
        if i + 1 == n_then:
            then = m.pack()
    count = m.diff(then, cap=0)
    n = count["n"]
    full_n = m.diff(then, values=0x1F, cap=0)["n"]
    if trace:
        for _ in range(3):
            m.diff(then, cap=0)
            m.diff(then, cap=n)
            m.diff(then, values=0x1F, fields=ALL_FIELDS, cap=full_n)
            m.pack()
        return
    out = dict(map=name, block_depth=3, blocks_then=int(count["n_stream_blocks"]),
               blocks_now=int(count["n_stream_blocks"] + count["n_map_only_blocks"] - count["n_missing_now"]), stream_bytes=int(then.size),
               cells_compared=int(count["pairs"].sum()), cells_changed=n, cells_changed_or_value_changed=full_n,
               changed_share=n / float(count["pairs"].sum()))
    out["count"] = timed(lambda: m.diff(then, cap=0), reps)
    out["list"] = timed(filler(m, then, 0, ("block_key", "cell", "code"), n), reps)
    out["full"] = timed(filler(m, then, 0x1F, ALL_FIELDS, full_n), reps)
    out["pack"] = timed(m.pack, reps)
    host = la3dm_amd.BGKOctoMap(**params, device=-1).unpack(m.pack())
    assert host.diff(then, cap=0)["n"] == n
    out["host_diff"] = timed(lambda: host.diff(then, cap=n), max(3, reps // 3))
    out["replaced"] = dict(sum_of_medians_ms=out["pack"]["median_ms"] + out["host_diff"]["median_ms"])
    assert m.mirror_syncs() == 0
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: three diffs of each form per case, nothing else")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("diff_bench: no GPU visible (a timing taken elsewhere says nothing)")
    synth = [la3dm_amd.synthetic_scan(200000, origin=p) for p in SEQ_POSES]
    measure("configs[1] synthetic, snapshot after 4 scans, 1 further scan", synth, 4, args.reps, args.trace)
    measure("configs[1] synthetic, snapshot after 1 scan, 4 further scans", synth, 1, args.reps, args.trace)


if __name__ == "__main__":
    main()
