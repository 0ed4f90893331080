"""score_paths on the device-resident map: distance_field's launches into working storage, then one kernel that takes a
wave per path — waypoint voxels and offsets in LDS, ordinals in chunks of 64, the first stop by ballot (csrc/devmap_paths.h).
The yardstick is the host form of the same class on a host-mode twin map with the same inserts (a plain loop), itself
checked against the independent yardstick of tests/helpers/paths_cases.py.  Every output is an integer: every comparison is
exact."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, pcd_path

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import distance_cases as D  # noqa: E402
import paths_cases as P  # noqa: E402
import region_cases as R  # noqa: E402
import score_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured
N_WAY = (1, 2, 3, 64, 65, 257, 1024)
WALKS = (0, 1, 63, 64, 65, 127, 128, 129, 257)       # T: a chunk of ordinals is 64
STOPS = (None, 0, 63, 64, 65, "T")
N_PATHS = (1, 2, 3, 4, 5, 257)                        # four paths a workgroup
LINE = (300, 3, 2)
GUARD = 0x5A5A5A5A
WORDS = dict(cost=2, steps=1, stop=1, min_d2=1, ways=1)   # 32-bit words per path; flags is a byte


def _pair(cls_name, params, scans, insert=INSERT):
    """the same inserts into a device-resident map and a host-mode one"""
    import la3dm_amd
    cls = getattr(la3dm_amd, cls_name)
    md = cls(**params, device=0)
    mh = cls(**params, device=0).set_device_resident(False)
    assert md.is_device_resident() and not mh.is_device_resident()
    for i in scans:
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        md.insert_pointcloud(xyz, origin, *insert)
        mh.insert_pointcloud(xyz, origin, *insert)
    return md, mh


def _compare(md, mh, lo, dims, paths, p, what, **kw):
    """device == host on the six arrays and the info; returns the host answer"""
    gd, gh = P.call(md, lo, dims, paths, p, **kw), P.call(mh, lo, dims, paths, p, **kw)
    assert set(gd) == set(gh)
    P.assert_same(gd, gh, (what, dims, p))
    R.assert_same(gd, gh, ("origin", "cell"), what)
    assert gd["block_key"] == gh["block_key"] and md.is_device_resident()
    return gh


@pytest.mark.parametrize("depth", [3, 4])
def test_device_equals_host_bit_for_bit(built, depth):
    """GPU test 1: BGK at block_depth 3 and 4, two fused (and pruned) scans: the recipe's kind of path set on the recipe
    region and the two small regions, clearance x soft_radius in {0, 1, 8}^2 and two masks; the host form == the independent
    yardstick on that map, with the input conditions; then a further insert (the pool grew, the table was rebuilt) and the
    same comparisons; no mirror refresh throughout"""
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    md, mh = _pair("BGKOctoMap", params, (1, 2))
    res = mh.get_resolution()
    lv = mh.leaves()
    lo = R.recipe_lo()
    P.assert_exercises_the_feature(P.input_conditions(mh, lv, lo, R.RECIPE_DIMS, P.recipe_paths(mh, lv, lo, R.RECIPE_DIMS)))
    _, _, _, origin = R.anchor(lo, res, depth)
    slo = S.small_lo(mh, origin)
    sets = [(rlo, dims, P.recipe_paths(mh, lv, rlo, dims)) for rlo, dims in [(lo, R.RECIPE_DIMS)] + [(slo, d) for d in P.REGIONS[1:]]]
    before_syncs = md.mirror_syncs()

    def everything(tag, check_yardstick):
        kinds = np.zeros(5, np.int64)
        for rlo, dims, paths in sets:
            for cl in P.RADII:
                for sr in P.RADII:
                    for mask in (D.MASKS[0], D.MASKS[2]) if (cl, sr) in ((0, 0), (1, 8)) else (D.MASKS[0],):
                        p = P.params(mask=mask, clearance=cl, soft_radius=sr, penalty=50 if sr else 0, max_steps=64 if cl != 8 else 4096)
                        gh = _compare(md, mh, rlo, dims, paths, p, f"bgk d{depth} {tag}")
                        kinds += [int((gh["flags"] == f).sum()) for f in (0, P.BLOCKED, P.LEFT, P.TRUNCATED, P.INVALID)]
                        if check_yardstick:
                            P.assert_same(gh, P.yardstick(mh, lv, rlo, dims, paths, p), ("host form vs yardstick", depth, dims, cl, sr, mask))
        print(f"bgk d{depth} {tag}: paths clean, BLOCKED, LEFT, TRUNCATED, INVALID {kinds.tolist()}")
        assert (kinds > 0).all()
    everything("two scans", True)
    assert md.mirror_syncs() == before_syncs
    before = md.block_count()          # (refreshes the mirror; the queries do not depend on it either way)
    xyz, origin5 = la3dm_amd.load_pcd(pcd_path("sim_structured", 5))
    for m in (md, mh):
        m.insert_pointcloud(xyz, origin5, *INSERT)
    assert md.block_count() > before
    syncs = md.mirror_syncs()
    everything("after a further insert", False)
    assert md.mirror_syncs() == syncs


def _bare_map(H, ctx, scans):
    import la3dm_amd
    dm = C.c_void_p()
    assert H.la3dm_devmap_create(ctx, C.byref(dm)) == OK
    for i in scans:
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3, *INSERT, None) == OK
    return dm


def _line_paths(origin, res, n_way, n_paths):
    """n_paths walks along x through the region LINE with n_way waypoints each, cycling through every (T, stop) of WALKS x
    STOPS that n_way allows: the walk has T moves, cut into n_way - 1 segments of nearly equal length (some of length 0 where
    n_way - 1 > T) that also weave in y and z, and starts at x = LINE[0] - stop so that ordinal `stop` is the first voxel
    outside the region (stop None: it ends inside; stop 0: it starts outside).  Returns the paths and the (T, stop) of each"""
    combos = [(T, T if s == "T" else s) for T in WALKS for s in STOPS if (s is None or s == "T" or s <= T) and (n_way > 1 or T == 0)]
    rows, kinds = [], []
    for i in range(n_paths):
        T, stop = combos[i % len(combos)]
        x0 = 5 + (i % 7) if stop is None else LINE[0] - stop
        at = (np.arange(n_way) * T) // max(n_way - 1, 1)                      # x offsets of the waypoints: 0 ... T
        y = np.array((0, 1, 2, 1))[(at + i) % 4]                               # a triangle wave in x: |dy| <= |dx| on every segment
        z = ((at + i) // 2) % 2
        rows.append(np.stack([x0 + at, y, z], 1))
        kinds.append((T, stop))
    return P.centre(origin, np.array(rows), res), kinds


def test_lanes_waves_and_neighbours(built):
    """GPU test 2: n_way in {1, 2, 3, 64, 65, 257, 1024} with 3 and 257 paths, n_paths in {1, 2, 3, 4, 5, 257} at n_way 2 and
    65, the paths cycling through walk
    lengths T in {0, 1, 63, 64, 65, 127, 128, 129, 257} with a stop forced at ordinal 0, 63, 64, 65, T or nowhere, on a
    300 x 3 x 2 region in which nothing blocks: the device-resident map == its host-mode twin, and the stops are where they
    were put; on a bare la3dm_devmap with the same scans the device-pointer form, its outputs 4 bytes off a 16-byte boundary
    between guard words, == the host-pointer form == the twin, the guard words untouched; then each optional output left
    out in turn"""
    import torch
    import la3dm_amd
    from la3dm_amd import _lib
    H = _lib.hip()
    md, mh = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML), (1, 2))
    res = mh.get_resolution()
    _, _, _, origin = R.anchor(R.recipe_lo(), res, 3)
    llo = P.centre(origin, (-100, 40, 14), res)
    _, _, _, lo_origin = R.anchor(llo, res, 3)
    dm = _bare_map(H, mh.ctx(), (1, 2))
    err = lambda: H.la3dm_last_error(mh.ctx()).decode()   # noqa: E731
    dev = torch.device("cuda:0")
    p = P.params(mask=0x10, max_steps=300)                # no voxel of a BGK map is UNCERTAIN: nothing blocks
    prm = _lib.PathsParams(p["mask"], 0, 0, 0, (C.c_uint32 * 3)(*p["move_cost"]), p["max_steps"])
    d3 = np.array(LINE, np.uint32)
    seen = set()

    def device_form(d_w, n, n_way, leave_out=None):
        t = {k: torch.full((w * n + 9,), GUARD, dtype=torch.int32, device=dev) for k, w in WORDS.items()}
        t["flags"] = torch.full((n + 23,), 0x5A, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert all(t[k][1:].data_ptr() % 16 == 4 for k in WORDS)
        ptr = {k: (t[k][1:] if k in WORDS else t[k][5:]).data_ptr() for k in t}
        do = _lib.PathsOut(*[None if k == leave_out else ptr[k] for k, _ in _lib.PathsOut._fields_])
        assert H.la3dm_devmap_score_paths_device(dm, llo.ctypes.data, d3.ctypes.data, d_w.data_ptr(), n, n_way, C.byref(prm), C.byref(do), None) == OK, err()
        got = {}
        for k, w in WORDS.items():
            g = t[k].cpu().numpy().view(np.uint32)
            assert g[0] == GUARD and (g[w * n + 1:] == GUARD).all(), (k, n, n_way)
            body = g[1:w * n + 1]
            got[k] = (body[0::2].astype(np.uint64) | (body[1::2].astype(np.uint64) << np.uint64(32))) if w == 2 else body.copy()
        f = t["flags"].cpu().numpy()
        assert (f[:5] == 0x5A).all() and (f[n + 5:] == 0x5A).all()
        got["flags"] = f[5:n + 5].copy()
        return got
    try:
        for n_way in N_WAY:
            paths, kinds = _line_paths(lo_origin, res, n_way, max(N_PATHS))
            d_all = torch.cat([torch.zeros(1, device=dev), torch.from_numpy(paths.reshape(-1)).to(dev)])[1:]      # 4 bytes off, too
            for n in N_PATHS if n_way in (2, 65) else (3, max(N_PATHS)):   # every n_paths at two n_way, two n_paths at every n_way
                gh = _compare(md, mh, llo, LINE, paths[:n], p, f"n_way {n_way} n_paths {n}")
                for i, (T, stop) in enumerate(kinds[:n]):
                    want = (P.LEFT, stop, stop) if stop is not None else (0, P.NONE, T + 1)
                    assert (gh["flags"][i], gh["stop"][i], gh["steps"][i]) == want, (n_way, i, T, stop, {k: gh[k][i] for k in P.FIELDS})
                    seen.add((T, stop))
                h = {k: np.full(n, 7, P.DTYPES[k]) for k in P.FIELDS}
                ho = _lib.PathsOut(*[h[k].ctypes.data for k, _ in _lib.PathsOut._fields_])
                w = np.ascontiguousarray(paths[:n])
                assert H.la3dm_devmap_score_paths_host(dm, llo.ctypes.data, d3.ctypes.data, w.ctypes.data, n, n_way, C.byref(prm), C.byref(ho), None) == OK, err()
                P.assert_same(h, gh, ("host pointers", n_way, n))
                got = device_form(d_all, n, n_way)
                P.assert_same(got, gh, ("device pointers", n_way, n))
        paths, _ = _line_paths(lo_origin, res, 65, 5)
        d_w = torch.from_numpy(paths.reshape(-1)).to(dev)
        gh = P.call(mh, llo, LINE, paths, p)
        for leave_out in P.FIELDS[1:]:
            got = device_form(d_w, 5, 65, leave_out)
            for k in P.FIELDS:
                assert (got[k] == (gh[k] if k != leave_out else (0x5A if k == "flags" else GUARD))).all(), (leave_out, k)
    finally:
        H.la3dm_devmap_destroy(dm)
    print(f"lanes and waves: {len(seen)} distinct (T, stop) walked")
    assert {(T, s) for T in WALKS for s in (None, T)} <= seen and {(257, s) for s in (0, 63, 64, 65)} <= seen and md.mirror_syncs() == 0


@pytest.mark.parametrize("variant", ["GPOctoMap", "BGKLOctoMap", "BGKLVOctoMap"])
def test_device_equals_host_on_other_variants(built, variant):
    """GPU test 3: GP, BGK-L and BGK-LV on their own configurations; on BGK-LV obstacles = bit 4 makes the UNCERTAIN voxels
    the obstacles, and the host form's box says whether the region holds some"""
    import la3dm_amd
    params, insert = {"GPOctoMap": (la3dm_amd.GP_YAML, INSERT), "BGKLOctoMap": (la3dm_amd.L_YAML, (0.1, 0.3, 8.0)),
                      "BGKLVOctoMap": (la3dm_amd.LV_YAML, (0.1, 0.3, 8.0))}[variant]
    md, mh = _pair(variant, dict(params), (1, 2), insert)
    lo = R.recipe_lo()
    big = mh.box(lo, R.RECIPE_DIMS, fields=())
    res, depth = mh.get_resolution(), int(mh.get_block_depth())
    rng = np.random.default_rng(9)
    ijk = np.stack([rng.integers(-2, n + 2, (96, 6)) for n in R.RECIPE_DIMS], -1)
    paths = P.centre(big["origin"], ijk, res)
    blocked = 0
    for cl, sr in ((0, 0), (1, 4), (8, 1)):
        for mask in (D.MASKS[0], D.MASKS[2]):
            gh = _compare(md, mh, lo, R.RECIPE_DIMS, paths, P.params(mask=mask, clearance=cl, soft_radius=sr, penalty=9 if sr else 0, max_steps=100), variant)
            blocked += int((gh["flags"] == P.BLOCKED).sum())
    assert blocked > 0
    gh = _compare(md, mh, lo, R.RECIPE_DIMS, paths, P.params(mask=1 << R.UNCERTAIN, clearance=1, max_steps=100), variant + " bit 4")
    n_unc = int((big["cls"] == R.UNCERTAIN).sum())
    print(variant, "paths BLOCKED by an UNCERTAIN voxel:", int((gh["flags"] == P.BLOCKED).sum()), "UNCERTAIN voxels in the region:", n_unc)
    assert (n_unc > 0) == (variant == "BGKLVOctoMap") and (n_unc > 0 or not (gh["flags"] == P.BLOCKED).any())
    slo = S.small_lo(mh, big["origin"])
    so = R.anchor(slo, res, depth)[3]
    ijk = np.stack([rng.integers(-1, n + 1, (33, 3)) for n in (3, 5, 7)], -1)
    _compare(md, mh, slo, (3, 5, 7), P.centre(so, ijk, res), P.params(mask=0x1E, clearance=1, soft_radius=2, penalty=5), variant + " small")


def test_device_pointer_form_refusals_and_storage(built):
    """GPU test 4 on a bare la3dm_devmap: the empty map in both pointer forms against an empty host-mode map; every refusal
    in both forms with its text and nothing written; the device-pointer form == the host-pointer form; 20 further calls and
    a smaller request reserve nothing; the map stays usable after another insert"""
    import torch
    import la3dm_amd
    from la3dm_amd import _lib
    H = _lib.hip()
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)   # (lends its context)
    ctx = m.ctx()
    dm = _bare_map(H, ctx, ())
    err = lambda: H.la3dm_last_error(ctx).decode()   # noqa: E731
    dev = torch.device("cuda:0")
    try:
        lo = R.recipe_lo()
        dims = np.array((77, 67, 39), np.uint32)
        tdims = tuple(int(v) for v in dims)
        empty = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
        origin = empty.box(lo, tdims, fields=())["origin"]
        rng = np.random.default_rng(17)
        ijk = np.stack([rng.integers(-2, n + 2, (61, 9)) for n in tdims], -1)
        paths = P.centre(origin, ijk, empty.get_resolution())
        paths[7, 3, 1] = np.nan
        n, n_way = paths.shape[0], paths.shape[1]
        lop, dp = lo.ctypes.data, dims.ctypes.data
        d_w = torch.from_numpy(paths.reshape(-1)).to(dev)
        h = {k: np.full(n, 9, P.DTYPES[k]) for k in P.FIELDS}
        ho = _lib.PathsOut(*[h[k].ctypes.data for k, _ in _lib.PathsOut._fields_])

        def tensors(fill, rows=n):
            t = {k: torch.full((w * rows + 8,), fill, dtype=torch.int32, device=dev) for k, w in WORDS.items()}
            t["flags"] = torch.full((rows + 8,), fill & 0xFF, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            return t, _lib.PathsOut(*[t[k].data_ptr() for k, _ in _lib.PathsOut._fields_])

        def read(t, rows=n):
            got, tails = {}, []
            for k, w in WORDS.items():
                g = t[k].cpu().numpy().view(np.uint32)
                body = g[:w * rows]
                got[k] = (body[0::2].astype(np.uint64) | (body[1::2].astype(np.uint64) << np.uint64(32))) if w == 2 else body.copy()
                tails.append(g[w * rows:])
            f = t["flags"].cpu().numpy()
            got["flags"] = f[:rows].copy()
            return got, tails, f[rows:]

        def call(form, out, **kw):
            a = dict(lo_p=lop, d_p=dp, w_p=paths.ctypes.data if form == "host" else d_w.data_ptr(), n=n, n_way=n_way, o=C.byref(out) if out is not None else None,
                     with_params=True, mask=0x2, clearance=1, soft_radius=3, penalty=20, move_cost=(10, 14, 17), max_steps=200)
            a.update(kw)
            prm = _lib.PathsParams(a["mask"], a["clearance"], a["soft_radius"], a["penalty"], (C.c_uint32 * 3)(*a["move_cost"]), a["max_steps"])
            f = getattr(H, f"la3dm_devmap_score_paths_{form}")
            return f(dm, a["lo_p"], a["d_p"], a["w_p"], a["n"], a["n_way"], C.byref(prm) if a["with_params"] else None, a["o"], None)
        # empty map: from the definition, host and device pointers, with and without bit 3
        for mask in (0x2, 0xA):
            want = empty.score_paths(lo, tdims, paths, obstacles=mask, clearance=1, soft_radius=3, penalty=20, max_steps=200)
            assert call("host", ho, mask=mask) == OK, err()
            P.assert_same(h, want, ("empty map, host pointers", mask))
            t, do = tensors(9)
            assert call("device", do, mask=mask) == OK, err()
            got, tails, ftail = read(t)
            P.assert_same(got, want, ("empty map, device pointers", mask))
            assert all((x == 9).all() for x in tails) and (ftail == 9).all()
            assert (int((want["flags"] == P.BLOCKED).sum()) > 0) == bool(mask & 8) and int((want["flags"] == P.INVALID).sum()) == 1
        xyz, o1 = la3dm_amd.load_pcd(pcd_path("sim_structured", 1))
        o3 = (C.c_float * 3)(*[float(v) for v in o1])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3, *INSERT, None) == OK

        def free():
            torch.cuda.synchronize()
            return torch.cuda.mem_get_info()[0]
        # refusals: LA3DM_ERR_ARG and a text that names the argument; nothing written, nothing reserved
        for k in h:
            h[k][...] = 7
        t, do = tensors(7)
        f0 = free()
        lo_nan, lo_far = np.array((np.nan, 0, 0), np.float32), np.array((-3.0e5, 0, 0), np.float32)
        d_zero, d_over = np.array((4, 0, 4), np.uint32), np.array(((1 << 28) + 1, 1, 1), np.uint32)
        for form, out in (("host", ho), ("device", do)):
            no_cost = _lib.PathsOut(None, out.steps, out.stop, out.min_d2, out.ways, out.flags)
            for kw, text in ((dict(with_params=False), "params is NULL"), (dict(mask=0), "obstacle_mask must hold"), (dict(mask=0x20), "obstacle_mask must hold"),
                             (dict(mask=0x80000002), "obstacle_mask must hold"), (dict(clearance=1025), "clearance must not exceed"),
                             (dict(soft_radius=1025), "soft_radius must not exceed"), (dict(penalty=0), "penalty must be >= 1 with soft_radius > 0"),
                             (dict(penalty=(1 << 16) + 1), "penalty must not exceed"), (dict(move_cost=(10, 0, 17)), "move_cost: every entry"),
                             (dict(max_steps=0), "max_steps must lie in"), (dict(max_steps=(1 << 20) + 1), "max_steps must lie in"),
                             (dict(n_way=0), "n_way must lie in"), (dict(n_way=1025, n=1), "n_way must lie in"),
                             (dict(n=(1 << 20) + 1, n_way=1), "LA3DM_PATHS_MAX_PATHS"), (dict(n=1 << 20, n_way=65), "LA3DM_PATHS_MAX_WAYPOINTS"),
                             (dict(w_p=None), "ways3 is NULL"), (dict(o=None), "out is NULL"), (dict(o=C.byref(no_cost)), "out->cost must not be NULL"),
                             (dict(lo_p=None), "lo is NULL"), (dict(d_p=None), "dims is NULL"),
                             (dict(lo_p=lo_nan.ctypes.data), "lo must be finite"), (dict(d_p=d_zero.ctypes.data), "dims must be >= 1"),
                             (dict(lo_p=lo_far.ctypes.data), "lo: the block field leaves"), (dict(d_p=d_over.ctypes.data), "LA3DM_DF_MAX_CELLS"),
                             (dict(n=1 << 16, n_way=1024, w_p=None), "ways3 is NULL"),                       # at the limit: the next check answers
                             (dict(with_params=False, n_way=0, lo_p=None, o=None), "params is NULL"),          # the order
                             (dict(mask=0, clearance=2000, max_steps=0, n_way=0, lo_p=None, o=None), "obstacle_mask must hold"),
                             (dict(clearance=2000, max_steps=0, n_way=0, lo_p=None, o=None), "clearance must not exceed"),
                             (dict(max_steps=0, n_way=0, n=1 << 21, lo_p=None, o=None), "max_steps must lie in"),
                             (dict(n_way=0, n=1 << 21, lo_p=None, o=None), "n_way must lie in"), (dict(n=1 << 21, lo_p=None, o=None), "LA3DM_PATHS_MAX_PATHS"),
                             (dict(w_p=None, o=None, lo_p=None), "ways3 is NULL"), (dict(o=None, lo_p=None), "out is NULL"),
                             (dict(lo_p=None, d_p=d_over.ctypes.data), "lo is NULL")):
                assert call(form, out, **kw) == ERR_ARG and text in err() and "score_paths" in err(), (form, kw, err())
            assert call(form, out, n=0, w_p=None, o=None) == OK, err()              # n_paths = 0: served, nothing written
        assert H.la3dm_devmap_score_paths_host(None, lop, dp, paths.ctypes.data, n, n_way, None, C.byref(ho), None) == ERR_ARG
        assert all((h[k] == 7).all() for k in h) and all((t[k].cpu().numpy() == 7).all() for k in t)
        f1 = free()
        print(f"free device memory before / after the refusals: {f0} / {f1}")
        assert f1 >= f0, (f0, f1)
        # device pointers == host pointers
        blocked = 0
        for kw in (dict(), dict(mask=0xE, clearance=0, soft_radius=0, penalty=0), dict(mask=0x1, clearance=8, soft_radius=2, max_steps=17)):
            assert call("host", ho, **kw) == OK, err()
            t, do = tensors(GUARD)
            assert call("device", do, **kw) == OK, err()
            got, tails, ftail = read(t)
            assert all((x == GUARD).all() for x in tails) and (ftail == (GUARD & 0xFF)).all()
            P.assert_same(got, h, ("device pointers == host pointers", kw))
            blocked += int((h["flags"] == P.BLOCKED).sum())
        assert blocked > 0 and int((h["flags"] == P.INVALID).sum()) == 1
        # storage: the calls above reserved the arenas; 20 more calls and a smaller request allocate nothing
        t, do = tensors(0)
        assert call("device", do) == OK and call("host", ho) == OK, err()
        f0 = free()
        small = np.array((31, 17, 23), np.uint32)
        for i in range(10):
            assert call("device", do, mask=1 + (i & 3), clearance=3 * i, max_steps=1 + 40 * i) == OK, err()
            assert call("host", ho, mask=1 + (i & 3), clearance=3 * i, max_steps=1 + 40 * i) == OK, err()
        assert call("device", do, d_p=small.ctypes.data, n=n // 2, n_way=n_way // 2) == OK, err()
        assert call("host", ho, d_p=small.ctypes.data, n=n // 2, n_way=n_way // 2) == OK, err()
        f1 = free()
        print(f"free device memory before / after 20 calls and a smaller request: {f0} / {f1}")
        # the figure is the whole device's: a process of another user may release memory meanwhile, so growth is what fails
        assert f1 >= f0, (f0, f1)
        # still usable: another scan, the two forms agree again and the answer has changed
        assert call("host", ho) == OK, err()
        before = {k: h[k].copy() for k in h}
        xyz, o2 = la3dm_amd.load_pcd(pcd_path("sim_structured", 2))
        o3 = (C.c_float * 3)(*[float(v) for v in o2])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3, *INSERT, None) == OK
        t, do = tensors(0)
        assert call("host", ho) == OK and call("device", do) == OK, err()
        got, _, _ = read(t)
        P.assert_same(got, h, "after another insert")
        assert any((h[k] != before[k]).any() for k in h)
    finally:
        H.la3dm_devmap_destroy(dm)


def _fan(o, n_head, n_curv, n_way, length):
    """the arcs of examples/rollouts.cpp, bit for bit: double arithmetic with libm's sin and cos, rounded to float32 once"""
    ox, oy = float(o[0]), float(o[1])
    out = np.empty((n_head * n_curv, n_way, 3), np.float32)
    for j in range(n_head):
        for i in range(n_curv):
            for k in range(n_way):
                theta, kappa, s = j * 3.14159265358979323846 / 4, 0.05 * (i - n_curv // 2), length * k / (n_way - 1)
                dx = s if i == n_curv // 2 else math.sin(kappa * s) / kappa
                dy = 0.0 if i == n_curv // 2 else (1.0 - math.cos(kappa * s)) / kappa
                c, sn = math.cos(theta), math.sin(theta)
                out[j * n_curv + i, k] = (ox + (c * dx - sn * dy), oy + (sn * dx + c * dy), o[2])
    return out


def test_planner_sized_call(built):
    """GPU test 5: 4 096 paths x 32 waypoints in one call (64 headings x 64 curvatures of 4 m arcs from scan 2's origin, the
    recipe region): every path equals the host form; a second call gives identical arrays; no mirror refresh"""
    import la3dm_amd
    md, mh = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML), (1, 2))
    lo = R.recipe_lo()
    _, o = la3dm_amd.load_pcd(pcd_path("sim_structured", 2))
    o = np.asarray(o, np.float64)
    k = np.arange(32) * (4.0 / 31)
    theta = (np.arange(64) * (2 * np.pi / 64))[:, None, None]
    kappa = ((np.arange(64) - 31.5) * 0.03)[None, :, None]
    dx, dy = np.sin(kappa * k) / kappa, (1 - np.cos(kappa * k)) / kappa
    paths = np.stack([o[0] + np.cos(theta) * dx - np.sin(theta) * dy, o[1] + np.sin(theta) * dx + np.cos(theta) * dy,
                      np.broadcast_to(o[2] + 0.01 * np.arange(32), (64, 64, 32))], -1).reshape(4096, 32, 3).astype(np.float32)
    p = P.params(clearance=2, soft_radius=5, penalty=20)
    syncs = md.mirror_syncs()
    a = P.call(md, lo, R.RECIPE_DIMS, paths, p)
    b = P.call(md, lo, R.RECIPE_DIMS, paths, p)
    P.assert_same(a, b, "twice")
    gh = P.call(mh, lo, R.RECIPE_DIMS, paths, p)
    P.assert_same(a, gh, "4096 paths")
    kinds = [int((gh["flags"] == f).sum()) for f in (0, P.BLOCKED, P.LEFT)]
    print("paths clean, BLOCKED, LEFT:", kinds, "distinct costs:", np.unique(gh["cost"]).size, "longest walk:", int(gh["steps"].max()))
    assert kinds[0] > 0 and kinds[1] > 0 and np.unique(gh["cost"]).size > 100
    assert md.mirror_syncs() == syncs and md.is_device_resident()


def test_example_program(built):
    """GPU test 6: examples/rollouts.cpp (built by build()) == the Python binding on the same map and fan of arcs: the
    cheapest clean arc, the tallies of the blocked ones and the counts by kind; no mirror refresh"""
    import la3dm_amd
    exe = os.path.join(ROOT, "examples", "rollouts")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "3"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    print(r.stdout)
    assert len(lines) == 4 and lines[0].startswith("best ") and lines[1].startswith("blocked ") and lines[2].startswith("left ")
    assert lines[3].startswith("rollouts 128 x 128 x 32 from ")
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    for i in (1, 2, 3):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        m.insert_pointcloud(xyz, origin, *INSERT)
    _, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 4))
    o = np.asarray(origin, np.float32)
    lo = np.array([o[0] - np.float32(6.4), o[1] - np.float32(6.4), o[2] - np.float32(1.6)], np.float32)
    start = np.array([o[0], o[1], o[2] + np.float32(0.3)], np.float32)
    got = m.score_paths(lo, (128, 128, 32), _fan(start, 8, 41, 32, 4.0), clearance=0, soft_radius=3, penalty=20, max_steps=4096)
    f = got["flags"]
    clean = np.nonzero(f == 0)[0]
    bt = lines[0].split()
    if clean.size:
        best = int(clean[np.argmin(got["cost"][clean])])                           # the first of equals
        assert [int(bt[1]), int(bt[3]), int(bt[7]), int(bt[9]), int(bt[11])] == [best, best // 41, int(got["cost"][best]), int(got["steps"][best]), int(got["min_d2"][best])]
    else:
        assert bt[1] == "none"
    blocked = got["steps"][f == P.BLOCKED].astype(np.int64)
    assert [int(v) for v in lines[1].split()[1::2][:1] + lines[1].split()[4::2]] == [blocked.size, int(blocked.min()) if blocked.size else 0,
                                                                                     int(blocked.max()) if blocked.size else 0, int(blocked.sum())]
    lt = lines[2].split()
    assert [int(lt[1]), int(lt[3]), int(lt[5]), int(lt[7])] == [int((f == P.LEFT).sum()), int((f == P.TRUNCATED).sum()), int((f == P.INVALID).sum()), int(clean.size)]
    tl = lines[3].split()
    tail = {tl[k]: tl[k + 1] for k in range(len(tl) - 1)}
    assert int(tail["paths"]) == 328 and int(tail["waypoints"]) == 32
    assert tail["mirror_syncs"] == "0" and tail["device_resident"] == "1" and m.mirror_syncs() == 0
    assert blocked.size > 0 and clean.size > 0
