"""Measurement of surface on the device-resident map.  Not a test and not part of bench.py.

Maps: BGK, 0.1 m, block_depth 3 — (a) scans 1 and 2 of sim_structured, the tests' two-scan map; (b) one synthetic 200k-ray
scan without a range limit (la3dm_amd.synthetic_scan, BASELINE configs[1]), the map footing_bench uses.  Region: 128 x 128
x 32 voxels round the last sensor origin.  solid = OCCUPIED, open = FREE.

Per map one JSON line with
  surface_s0            BGKOctoMap.surface(smooth 0), index, faces and normal: probe, faces, scan, emit; count call + fill
                        call as Python makes them
  surface_s0_index_faces  smooth 0 with index and faces only: two arrays copied back, as frontier_6 copies two
  surface_s2, _s4       the same at smooth 2 and 4: the six face streams stored and the window pass (dm_sf_normals)
  surface_s0_dense      smooth 0 with dense_faces as well (the streams stored, one byte per voxel downloaded)
  surface_s2_dense      smooth 2 with dense_faces
  frontier_6            BGKOctoMap.frontier(open=occupied, unknown=free, connectivity=6) with index and nbrs on the same
                        region: the same probe, stencil, scan and emit, so where the smooth-0 call should land
  baseline_host         what the map offered before: box's classes of the padded box downloaded (1 byte per voxel) plus the
                        numpy yardstick of the tests on the host, at smooth 0 and at smooth 2
Host clock round calls that end in a stream synchronise, profiler off; median / min / max of --reps after one warm-up call.
The kernels alone come from a kernel trace of this script in a run of its own, with no counters:
  rocprofv3 --output-format csv --kernel-trace --stats -d <dir> -o t -- python tools/surface_bench.py --trace"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import la3dm_amd  # noqa: E402

INSERT = (0.1, 0.5, 8.0)
SOLID, OPEN = 0x2, 0x1
LIST = ("index", "faces", "normal")


def ms(t):
    return dict(median_ms=1e3 * float(np.median(t)), min_ms=1e3 * float(min(t)), max_ms=1e3 * float(max(t)))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def scan(i):
    return la3dm_amd.load_pcd(os.path.join(ROOT, "tests", "golden", "data", "sim_structured", f"sim_structured_{i}.pcd"))


def maps():
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    for i in (1, 2):
        xyz, origin = scan(i)
        m.insert_pointcloud(xyz, origin, *INSERT)
    yield "two scans of sim_structured", m, np.asarray(origin, np.float32)
    xyz, origin = la3dm_amd.synthetic_scan(200000)
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    m.insert_pointcloud(xyz, origin, 0.1, 0.5, -1.0)          # (configs[1]: no range limit)
    yield "synthetic 200k-ray scan", m, np.asarray(origin, np.float32)


def host_baseline(m, lo, dims, s):
    """box's classes of the padded box downloaded, then the tests' numpy yardstick"""
    import surface_cases as S
    res = np.float32(m.get_resolution())
    plo = (m.box(lo, (1, 1, 1), fields=())["origin"] - np.float32(S.pad_of(s)) * res).astype(np.float32)
    pcls = m.box(plo, S.padded_dims(dims, s), fields=())["cls"]
    return S.yardstick(pcls, dims, SOLID, OPEN, s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--trace", action="store_true", help="run under rocprofv3: six calls of each query per map, nothing else")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("surface_bench: no GPU visible (a timing taken elsewhere says nothing)")
    for map_name, m, o in maps():
        assert m.is_device_resident()
        lo, dims = np.array([o[0] - np.float32(6.4), o[1] - np.float32(6.4), o[2] - np.float32(1.6)], np.float32), (128, 128, 32)
        kw = dict(solid=SOLID, open=OPEN)
        calls = dict(surface_s0=lambda: m.surface(lo, dims, smooth=0, **kw),
                     surface_s0_index_faces=lambda: m.surface(lo, dims, smooth=0, fields=("index", "faces"), **kw),
                     surface_s2=lambda: m.surface(lo, dims, smooth=2, **kw),
                     surface_s4=lambda: m.surface(lo, dims, smooth=4, **kw),
                     surface_s0_dense=lambda: m.surface(lo, dims, smooth=0, fields=LIST + ("dense_faces",), **kw),
                     surface_s2_dense=lambda: m.surface(lo, dims, smooth=2, fields=LIST + ("dense_faces",), **kw),
                     frontier_6=lambda: m.frontier(lo, dims, open=SOLID, unknown=OPEN, connectivity=6, fields=("index", "nbrs")))
        if args.trace:
            for call in calls.values():
                for _ in range(6):
                    call()
            continue
        out = {}
        for k, call in calls.items():
            call()                                       # warm-up: code objects and arenas
            out[k] = ms([timed(call)[0] for _ in range(args.reps)])
        a0, a2, a4, fr = calls["surface_s0"](), calls["surface_s2_dense"](), calls["surface_s4"](), calls["frontier_6"]()
        assert fr["n"] == a0["n"] and (fr["index"] == a0["index"]).all()
        host = {}
        for s, got in ((0, a0), (2, a2)):
            t_host = []
            for _ in range(3):
                dt, base = timed(lambda: host_baseline(m, lo, dims, s))
                t_host.append(dt)
            assert base["n"] == got["n"] and (base["index"] == got["index"]).all() and (base["normal"] == got["normal"]).all()
            host[f"baseline_host_s{s}"] = ms(t_host)
        words = lambda s: (int(np.prod([d + 2 * (s + 1) for d in dims])) + 31) // 32   # noqa: E731
        print(json.dumps(dict(map=map_name, blocks=int(m.block_count()), region="128 x 128 x 32", voxels=int(np.prod(dims)), words_s0=words(0),
                              words_s2=words(2), words_s4=words(4), n_solid=a0["n_solid"], n_surface=a0["n"], face_count=a0["face_count"],
                              zero_normals_s0=int((a0["normal"] == 0).all(1).sum()), zero_normals_s2=int((a2["normal"] == 0).all(1).sum()),
                              zero_normals_s4=int((a4["normal"] == 0).all(1).sum()), **host, **out)), flush=True)


if __name__ == "__main__":
    main()
