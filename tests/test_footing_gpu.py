"""footing on the device-resident map: bit streams over the padded box, shifted windows for stand, near and body, a
bit-sliced support counter, the map's one-launch scan, an emit and a column kernel (csrc/devmap_footing.h) say where a ground
robot can stand straight from the device pool.  Device-resident map == host-mode map (host/footing_cells.h) == the numpy
yardstick written from the contract comment (tests/helpers/footing_cases.py).  Integer arithmetic on classes: every
comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pcd_path

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import frontier_cases as FR  # noqa: E402
import footing_cases as F  # noqa: E402

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured


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


def _compare(md, mh, lo, dims, support, clear, h, r, s, c, what, cap=None, fields=F.FIELDS):
    """device == host on n, the stats, the arrays and the info; returns the host answer"""
    kw = dict(support=support, clear=clear, headroom=h, radius=r, step=s, min_support=c, fields=fields, cap=cap)
    gd, gh = md.footing(lo, dims, **kw), mh.footing(lo, dims, **kw)
    assert set(gd) == set(gh)
    F.assert_same(gd, gh, (what, dims, support, clear, h, r, s, c, cap), fields)
    R.assert_same(gd, gh, ("origin", "cell"), what)
    assert gd["block_key"] == gh["block_key"]
    return gh


def _supports(r):
    N = len(F.disc(r))
    return sorted({0, N // 2, N})


def test_scene(built):
    """GPU test 1: the hand-built scene over the full parameter grid, c = 0, N / 2 and N: device == host == yardstick, and the
    issue's recorded counts"""
    import la3dm_amd
    params = dict(R.YAML, block_depth=4)
    stream = F.scene_stream(params)
    md = la3dm_amd.BGKOctoMap(**params, device=0).unpack(stream)
    mh = la3dm_amd.BGKOctoMap(**params, device=0).set_device_resident(False).unpack(stream)
    assert md.is_device_resident() and not mh.is_device_resident()
    lv = mh.leaves()
    syncs = md.mirror_syncs()
    for clear, h, r, s in F.SCENE_GRID:
        _, p = F.padded_case(mh, lv, F.SCENE_LO, F.SCENE_DIMS, h, r, s)
        assert (p == F.scene_padded(h, r, s)).all()
        for c in _supports(r):
            gh = _compare(md, mh, F.SCENE_LO, F.SCENE_DIMS, F.OCC_M, clear, h, r, s, c, "scene")
            F.assert_same(gh, F.yardstick(p, F.SCENE_DIMS, F.OCC_M, clear, h, r, s, c), ("scene, host vs yardstick", clear, h, r, s, c))
    for clear, h, r, s, stand, body, foots in F.SCENE_COUNTS:
        for c, n in (foots or {0: None}).items():
            g = md.footing(F.SCENE_LO, F.SCENE_DIMS, support=F.OCC_M, clear=clear, headroom=h, radius=r, step=s, min_support=c, fields=())
            assert (stand is None or g["n_stand"] == stand) and (body is None or g["n_body"] == body) and (n is None or g["n"] == n), g
    assert md.mirror_syncs() == syncs


@pytest.mark.parametrize("depth", [3, 4])
def test_two_scan_map(built, depth):
    """GPU test 2: BGK at block_depth 3 and 4, two fused (and pruned) scans.  The recipe region with the input conditions
    re-counted from the yardstick of this map; the word and long shapes; the cap and field cases; clusters over the list;
    then a third insert (the pool grew, the table was rebuilt) and the same comparison; no mirror refresh throughout"""
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    md, mh = _pair("BGKOctoMap", params, (1, 2))
    res = mh.get_resolution()
    lv = mh.leaves()
    lo, dims = R.recipe_lo(), R.RECIPE_DIMS
    cache = {}

    def pcls_of(h, r, s):
        if (h, r, s) not in cache:
            cache[(h, r, s)] = F.padded_case(mh, lv, lo, dims, h, r, s)[1]
        return cache[(h, r, s)]
    F.assert_exercises_the_feature(F.input_conditions(pcls_of, dims))
    before_syncs = md.mirror_syncs()
    q = F.RECIPE
    for support, clear, h, r, s in ((q["support"], q["clear"], q["h"], q["r"], q["s"]), (F.OCC_M, F.FREE_M, 2, 0, 0),
                                    (F.OCC_M | F.UNK_M, F.FREE_M | F.MISS_M, 3, 1, 2), (F.OCC_M, F.OPTIMISTIC, 6, 4, 1)):
        for c in _supports(r):
            gh = _compare(md, mh, lo, dims, support, clear, h, r, s, c, f"bgk d{depth}")
            F.assert_same(gh, F.yardstick(pcls_of(h, r, s), dims, support, clear, h, r, s, c), ("host vs yardstick", depth, h, r, s, c))
    # the cap and field cases
    want = F.yardstick(pcls_of(4, 2, 1), dims, F.OCC_M, F.OPTIMISTIC, 4, 2, 1, 6)
    n = want["n"]
    for cap in (0, 1, n - 1, n, n + 100):
        got = md.footing(lo, dims, support=F.OCC_M, clear=F.OPTIMISTIC, headroom=4, radius=2, step=1, min_support=6, cap=cap, fields=F.FIELDS)
        assert got["n"] == n and got["index"].size == min(cap, n) and (got["index"] == want["index"][:cap]).all()
        F.assert_same(got, want, ("cap", cap), F.FIELDS[1:])
    for fields in ((), ("index",), ("levels",), ("lowest", "highest"), ("index", "highest")):
        got = md.footing(lo, dims, support=F.OCC_M, clear=F.OPTIMISTIC, headroom=4, radius=2, step=1, min_support=6, fields=fields)
        assert set(got) == {"n"} | set(fields) | set(F.STATS) | set(R.INFO_FIELDS)
        F.assert_same(got, want, ("fields", fields), fields)
    # the list feeds clusters: every listed voxel is labelled
    cl = md.clusters(lo, dims, members=want["index"], member=F.OPTIMISTIC, connectivity=26, fields=("label", "of_member"))
    assert cl["n"] >= 1 and (cl["of_member"] != la3dm_amd.CLUSTERS_NONE).all()
    assert (cl["label"].reshape(-1)[want["index"]] == cl["of_member"]).all()
    assert md.mirror_syncs() == before_syncs
    # the word and long shapes, anchored on no block corner
    stand = F.yardstick(pcls_of(2, 0, 0), dims, F.OCC_M, F.FREE_M, 2, 0, 0)["stand"]
    origin0 = R.yardstick(mh, lv, lo, (1, 1, 1))["origin"]
    found = 0
    for shape in FR.SHAPES + FR.WORD_SHAPES + FR.LONG_SHAPES:
        anchor = (origin0 + np.array(F.shape_offset(stand, shape), np.float32) * np.float32(res)).astype(np.float32)
        for h, r, s in F.SHAPE_PARAMS:
            slo, p = F.padded_case(mh, lv, anchor, shape, h, r, s)
            for clear in (F.FREE_M, F.OPTIMISTIC):
                for c in _supports(r)[:2]:
                    gh = _compare(md, mh, slo, shape, F.OCC_M, clear, h, r, s, c, f"bgk d{depth} shapes")
                    F.assert_same(gh, F.yardstick(p, shape, F.OCC_M, clear, h, r, s, c), ("shape", shape, clear, h, r, s, c))
                    found += gh["n"]
    print(f"shapes: {found} foot voxels in all")
    assert found > 100
    assert md.mirror_syncs() == before_syncs
    before = md.block_count()
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 5))
    for m in (md, mh):
        m.insert_pointcloud(xyz, origin, *INSERT)
    assert md.block_count() > before
    syncs = md.mirror_syncs()
    for h, r, s in ((4, 2, 1), (2, 0, 0), (8, 3, 2)):
        for c in _supports(r):
            gh = _compare(md, mh, lo, dims, F.OCC_M, F.OPTIMISTIC, h, r, s, c, f"bgk d{depth} after a further insert")
    assert gh["n_stand"] > 0
    assert md.mirror_syncs() == syncs


@pytest.mark.parametrize("variant", ["GPOctoMap", "BGKLOctoMap", "BGKLVOctoMap"])
def test_other_variants(built, variant):
    """GPU test 3: GP, BGK-L and BGK-LV on their own configurations.  The classes the yardstick reads come from the
    host-mode map's box() over the padded box (region_cases.yardstick is written for BGK's leaf fields); on BGK-LV the
    UNCERTAIN bit stands in the clear mask and in the support mask, and the box says such voxels exist"""
    import la3dm_amd
    params, insert = {"GPOctoMap": (la3dm_amd.GP_YAML, INSERT), "BGKLOctoMap": (la3dm_amd.L_YAML, (0.1, 0.3, 8.0)),
                      "BGKLVOctoMap": (la3dm_amd.LV_YAML, (0.1, 0.3, 8.0))}[variant]
    md, mh = _pair(variant, dict(params), (1, 2), insert)
    res = np.float32(mh.get_resolution())
    dims = (60, 60, 30)
    cases = [(F.OCC_M, F.OPTIMISTIC, 4, 2, 1), (F.OCC_M, F.FREE_M, 2, 0, 0)]
    if variant == "BGKLVOctoMap":
        cases += [(F.OCC_M, F.OPTIMISTIC | F.UNC_M, 4, 2, 1), (F.OCC_M | F.UNC_M, F.FREE_M, 2, 1, 1)]
    for support, clear, h, r, s in cases:
        below, _ = F.pads(h, r, s)
        big = mh.box(R.recipe_lo(), F.padded_dims(dims, h, r, s), fields=())
        lo = (big["origin"] + np.array(below, np.float32) * res).astype(np.float32)
        if variant == "BGKLVOctoMap":
            assert (big["cls"] == R.UNCERTAIN).sum() > 0
        for c in _supports(r):
            gh = _compare(md, mh, lo, dims, support, clear, h, r, s, c, variant)
            F.assert_same(gh, F.yardstick(big["cls"], dims, support, clear, h, r, s, c), (variant, "host vs the yardstick over its own box", c))
    assert gh["n_stand"] > 0


def test_pointer_forms_and_the_empty_map(built):
    """GPU test 4 on a bare la3dm_devmap: the empty map in both pointer forms; refusals with their text and nothing written;
    the device-pointer form == the host-pointer form, with a cap below n leaving the entries past it alone"""
    import torch
    import la3dm_amd
    from la3dm_amd import _lib
    H = _lib.hip()
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)   # (lends its context)
    ctx = m.ctx()
    dm = C.c_void_p()
    assert H.la3dm_devmap_create(ctx, C.byref(dm)) == OK
    err = lambda: H.la3dm_last_error(ctx).decode()   # noqa: E731
    dev = torch.device("cuda:0")
    try:
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 1))
        lo = (np.asarray(origin, np.float32) + np.asarray(R.RECIPE_OFFSET, np.float32)).astype(np.float32)
        dims = np.array((77, 67, 39), np.uint32)
        n, n_col = int(dims.prod()), int(dims[0] * dims[1])
        lop, dp = lo.ctypes.data, dims.ctypes.data
        found, stats = C.c_uint64(5), _lib.FootingStats()
        sizes = dict(index=n, levels=n_col, lowest=n_col, highest=n_col)
        dt = dict(index=np.uint32, levels=np.uint32, lowest=np.int32, highest=np.int32)

        def host_arrays(fill):
            h = {k: np.full(sizes[k], fill, dt[k]) for k in F.FIELDS}
            return h, _lib.FootingOut(*[h[k].ctypes.data for k in F.FIELDS])

        def tensors(fill, fields=F.FIELDS):
            t = {k: torch.full((sizes[k],), fill, dtype=torch.int32, device=dev) for k in F.FIELDS}
            torch.cuda.synchronize()
            return t, _lib.FootingOut(*[t[k].data_ptr() if k in fields else None for k in F.FIELDS])
        par = _lib.FootingParams(F.OCC_M, F.OPTIMISTIC, 4, 2, 1, 6)
        # the empty map: n = 0, levels = 0, lowest = highest = -1, the list untouched
        h, ho = host_arrays(9)
        assert H.la3dm_devmap_footing_host(dm, lop, dp, C.byref(par), n, C.byref(ho), C.byref(found), C.byref(stats), None) == OK, err()
        assert found.value == 0 and (h["index"] == 9).all() and (h["levels"] == 0).all() and (h["lowest"] == -1).all() and (h["highest"] == -1).all()
        assert stats.as_dict() == dict(n_stand=0, n_body=0, n_foot=0, disc_cells=12)
        t, do = tensors(9)
        found.value = 5
        assert H.la3dm_devmap_footing_device(dm, lop, dp, C.byref(par), n, C.byref(do), C.byref(found), None, None) == OK, err()
        g = {k: t[k].cpu().numpy() for k in t}
        assert found.value == 0 and (g["index"] == 9).all() and (g["levels"] == 0).all() and (g["lowest"] == -1).all() and (g["highest"] == -1).all()
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3,
                                                     0.1, 0.5, 8.0, None) == OK
        # refusals: LA3DM_ERR_ARG and a text that names the argument; nothing written
        h, ho = host_arrays(7)
        t, do = tensors(7)
        found.value = 77
        for fn, out in ((H.la3dm_devmap_footing_host, ho), (H.la3dm_devmap_footing_device, do)):
            def call(p=par, lo_p=lop, d_p=dp, cap=n, o=C.byref(out), nf=C.byref(found)):
                return fn(dm, lo_p, d_p, C.byref(p) if p is not None else None, cap, o, nf, None, None)
            P = _lib.FootingParams
            for p, text in ((None, "params is NULL"), (P(0, 1, 2, 0, 0, 0), "support_mask"), (P(2, 0x20, 2, 0, 0, 0), "clear_mask"),
                            (P(3, 1, 2, 0, 0, 0), "must not overlap"), (P(2, 1, 0, 0, 0, 0), "headroom"), (P(2, 1, 33, 0, 0, 0), "headroom"),
                            (P(2, 1, 2, 9, 0, 0), "radius"), (P(2, 1, 8, 0, 5, 0), "step"), (P(2, 1, 2, 0, 2, 0), "step"),
                            (P(2, 1, 2, 2, 0, 13), "min_support")):
                assert call(p=p) == ERR_ARG and text in err(), (text, err())
            assert call(o=None) == ERR_ARG and "index must not be NULL" in err()
            assert call(o=C.byref(_lib.FootingOut(None, out.levels, None, None))) == ERR_ARG and "index must not be NULL" in err()
            assert call(lo_p=None) == ERR_ARG and "lo is NULL" in err()
            assert call(d_p=None) == ERR_ARG and "dims is NULL" in err()
            d0 = np.array((4, 0, 4), np.uint32)
            assert call(d_p=d0.ctypes.data) == ERR_ARG and "dims must be >= 1" in err()
            big = np.array(((1 << 10) - 4, (1 << 10) - 4, (1 << 8) - 5), np.uint32)      # padded by (4, 4, 6): one over 2^28
            assert call(d_p=big.ctypes.data, cap=0, o=None, nf=None) == ERR_ARG and "LA3DM_FOOTING_MAX_CELLS" in err(), err()
            at = np.array(((1 << 10) - 4, (1 << 10) - 4, (1 << 8) - 6), np.uint32)       # exactly 2^28: the next check answers
            assert call(d_p=at.ctypes.data, cap=0, o=None, nf=None) == ERR_ARG and "n_found is NULL" in err(), err()
            low = np.array((-209715.5, 0, 0), np.float32)
            assert call(lo_p=low.ctypes.data) == ERR_ARG and "padded box leave" in err(), err()
            assert call(nf=None) == ERR_ARG and "n_found is NULL" in err()
            assert fn(None, lop, dp, C.byref(par), n, C.byref(out), C.byref(found), None, None) == ERR_ARG
        assert found.value == 77 and all((h[k] == 7).all() for k in h) and all((t[k].cpu().numpy() == 7).all() for k in t)
        # the device-pointer form == the host-pointer form
        for p in (par, _lib.FootingParams(F.OCC_M, F.FREE_M, 2, 0, 0, 0), _lib.FootingParams(F.OCC_M, F.OPTIMISTIC, 32, 8, 4, 98)):
            h, ho = host_arrays(0x6E)
            assert H.la3dm_devmap_footing_host(dm, lop, dp, C.byref(p), n, C.byref(ho), C.byref(found), C.byref(stats), None) == OK, err()
            nf = int(found.value)
            assert stats.n_foot == nf and (h["index"][nf:] == 0x6E).all() and (np.diff(h["index"][:nf].astype(np.int64)) > 0).all()
            assert int(h["levels"].sum()) == nf
            for fields in (F.FIELDS, ("index",), ("levels", "highest"), ()):
                for cap in ((n, nf // 3) if "index" in fields else (0,)):
                    t, do = tensors(0x5A, fields)
                    found.value, stats2 = 0, _lib.FootingStats()
                    assert H.la3dm_devmap_footing_device(dm, lop, dp, C.byref(p), cap, C.byref(do) if fields else None, C.byref(found),
                                                         C.byref(stats2), None) == OK, err()
                    assert found.value == nf and stats2.as_dict() == stats.as_dict()
                    k_out = min(cap, nf)
                    for k in F.FIELDS:
                        g = t[k].cpu().numpy().view(dt[k])
                        if k not in fields:
                            assert (g == 0x5A).all(), k
                        elif k == "index":
                            assert (g[:k_out] == h[k][:k_out]).all() and (g[k_out:] == 0x5A).all()
                        else:
                            assert (g == h[k]).all(), k
        print("device-pointer form: last case found", nf)
        assert nf >= 0
    finally:
        H.la3dm_devmap_destroy(dm)
