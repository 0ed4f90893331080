"""surface on the device-resident map: bit streams over the padded box, six face streams from shifted windows, the map's
one-launch scan, an emit kernel and, for smooth > 0, bit-sliced window counts summed across a wave
(csrc/devmap_surface.h) give the exposed faces and integer normals straight from the device pool.  Device-resident map ==
host-mode map (host/surface_cells.h) == the numpy yardstick written from the contract comment
(tests/helpers/surface_cases.py).  Integer arithmetic on classes: every comparison is exact."""
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
import surface_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured
OPTIMISTIC = S.FREE_M | S.UNK_M | S.MISS_M


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


def _compare(md, mh, lo, dims, solid, open_, s, what, cap=None, fields=S.FIELDS):
    """device == host on n, the stats, the arrays and the info; returns the host answer"""
    kw = dict(solid=solid, open=open_, smooth=s, fields=fields, cap=cap)
    gd, gh = md.surface(lo, dims, **kw), mh.surface(lo, dims, **kw)
    assert set(gd) == set(gh)
    S.assert_same(gd, gh, (what, dims, solid, open_, s, cap), fields)
    R.assert_same(gd, gh, ("origin", "cell"), what)
    assert gd["block_key"] == gh["block_key"]
    return gh


def test_scene(built):
    """GPU test 1: the hand-built scene at every smooth and mask pair of the issue's table: device == host == yardstick, and
    the table's constants from the device"""
    import la3dm_amd
    params = dict(R.YAML, block_depth=4)
    stream = F.scene_stream(params)
    md = la3dm_amd.BGKOctoMap(**params, device=0).unpack(stream)
    mh = la3dm_amd.BGKOctoMap(**params, device=0).set_device_resident(False).unpack(stream)
    assert md.is_device_resident() and not mh.is_device_resident()
    syncs = md.mirror_syncs()
    for s in S.SMOOTHS:
        p = S.scene_padded(s)
        for solid, open_ in [row[:2] for row in S.SCENE_TABLE]:
            gh = _compare(md, mh, S.SCENE_LO, S.SCENE_DIMS, solid, open_, s, "scene")
            S.assert_same(gh, S.yardstick(p, S.SCENE_DIMS, solid, open_, s), ("scene, host vs yardstick", solid, open_, s))

    def dev_of(solid, open_, s):
        g = md.surface(S.SCENE_LO, S.SCENE_DIMS, solid=solid, open=open_, smooth=s, fields=S.FIELDS)
        g["dense_normal"] = S.dense_normal_of(g, S.SCENE_DIMS)
        return g
    S.assert_scene_table(dev_of)
    assert md.mirror_syncs() == syncs


@pytest.mark.parametrize("depth", [3, 4])
def test_two_scan_map(built, depth):
    """GPU test 2: BGK at block_depth 3 and 4, two fused (and pruned) scans.  The recipe region (80 x 80 x 40) at smooth 0, 2
    and 4 with the input conditions re-counted from the yardstick of this map; the cap cases — the normals of the capped
    prefix are the uncapped ones —; the word, wave and long shapes; then a third insert (the pool grew) and the same
    comparison; no mirror refresh throughout"""
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    md, mh = _pair("BGKOctoMap", params, (1, 2))
    res = mh.get_resolution()
    lv = mh.leaves()
    lo, dims = R.recipe_lo(), R.RECIPE_DIMS
    before_syncs = md.mirror_syncs()
    for s in (0, 2, 4):
        _, p = S.padded_case(mh, lv, lo, dims, s)
        S.assert_exercises_the_feature(S.exercises_the_feature(p, dims, S.OCC_M, OPTIMISTIC, s), ("two-scan", depth, s))
        for solid, open_ in ((S.OCC_M, S.FREE_M), (S.OCC_M, OPTIMISTIC)):
            gh = _compare(md, mh, lo, dims, solid, open_, s, f"bgk d{depth}")
            S.assert_same(gh, S.yardstick(p, dims, solid, open_, s), ("host vs yardstick", depth, solid, open_, s))
    # the cap and field cases at smooth 2
    want = S.yardstick(S.padded_case(mh, lv, lo, dims, 2)[1], dims, S.OCC_M, OPTIMISTIC, 2)
    n = want["n"]
    kw = dict(solid=S.OCC_M, open=OPTIMISTIC, smooth=2)
    for cap in (0, 1, n // 3, n - 1, n, n + 1):
        got = md.surface(lo, dims, cap=cap, fields=S.FIELDS, **kw)
        assert got["n"] == n and all(got[k].shape[0] == min(cap, n) for k in S.LIST_FIELDS)
        assert all((got[k] == want[k][:cap]).all() for k in S.LIST_FIELDS), cap
        S.assert_same(got, want, ("cap", cap), ("dense_faces",))
    for fields in ((), ("index",), ("faces",), ("dense_faces",), ("index", "normal"), ("index", "faces")):
        got = md.surface(lo, dims, fields=fields, **kw)
        assert set(got) == {"n"} | set(fields) | set(S.STATS) | set(R.INFO_FIELDS)
        S.assert_same(got, want, ("fields", fields), fields)
    assert md.mirror_syncs() == before_syncs
    # the word, wave and long shapes, placed where there is surface
    dense = S.yardstick(S.padded_case(mh, lv, lo, dims, 0)[1], dims, S.OCC_M, OPTIMISTIC, 0)["dense_faces"]
    origin0 = R.yardstick(mh, lv, lo, (1, 1, 1))["origin"]
    cases = [(shape, s) for shape in FR.SHAPES + FR.WORD_SHAPES + FR.LONG_SHAPES for s in (0, 1, 4)]
    cases += [(shape, s) for s in (0, 1) for shape in S.pz_shapes(s)]
    found = 0
    for shape, s in cases:
        anchor = (origin0 + np.array(S.shape_offset(dense, shape), np.float32) * np.float32(res)).astype(np.float32)
        slo, p = S.padded_case(mh, lv, anchor, shape, s)
        for open_ in (S.FREE_M, OPTIMISTIC):
            gh = _compare(md, mh, slo, shape, S.OCC_M, open_, s, f"bgk d{depth} shapes")
            S.assert_same(gh, S.yardstick(p, shape, S.OCC_M, open_, s), ("shape", shape, open_, s))
            found += gh["n"]
    print(f"shapes: {found} surface voxels in all")
    assert found > 300
    assert md.mirror_syncs() == before_syncs
    before = md.block_count()
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 5))
    for m in (md, mh):
        m.insert_pointcloud(xyz, origin, *INSERT)
    assert md.block_count() > before
    syncs = md.mirror_syncs()
    for s in (0, 3):
        gh = _compare(md, mh, lo, dims, S.OCC_M, OPTIMISTIC, s, f"bgk d{depth} after a further insert")
    assert gh["n"] > 0
    assert md.mirror_syncs() == syncs


@pytest.mark.parametrize("variant", ["GPOctoMap", "BGKLOctoMap", "BGKLVOctoMap"])
def test_other_variants(built, variant):
    """GPU test 3: GP, BGK-L and BGK-LV on their own configurations.  The classes the yardstick reads come from the
    host-mode map's box() over the padded box (region_cases.yardstick is written for BGK's leaf fields); on BGK-LV the
    UNCERTAIN bit stands in the open mask and in the solid mask, and the box says such voxels exist"""
    import la3dm_amd
    params, insert = {"GPOctoMap": (la3dm_amd.GP_YAML, INSERT), "BGKLOctoMap": (la3dm_amd.L_YAML, (0.1, 0.3, 8.0)),
                      "BGKLVOctoMap": (la3dm_amd.LV_YAML, (0.1, 0.3, 8.0))}[variant]
    md, mh = _pair(variant, dict(params), (1, 2), insert)
    res = np.float32(mh.get_resolution())
    dims = (60, 60, 30)
    cases = [(S.OCC_M, OPTIMISTIC, 2), (S.OCC_M, S.FREE_M, 0)]
    if variant == "BGKLVOctoMap":
        cases += [(S.OCC_M, OPTIMISTIC | S.UNC_M, 1), (S.OCC_M | S.UNC_M, S.FREE_M, 4)]
    for solid, open_, s in cases:
        big = mh.box(R.recipe_lo(), S.padded_dims(dims, s), fields=())
        lo = (big["origin"] + np.float32(S.pad_of(s)) * res).astype(np.float32)
        if variant == "BGKLVOctoMap":
            assert (big["cls"] == R.UNCERTAIN).sum() > 0
        gh = _compare(md, mh, lo, dims, solid, open_, s, variant)
        S.assert_same(gh, S.yardstick(big["cls"], dims, solid, open_, s), (variant, "host vs the yardstick over its own box", s))
        assert gh["n"] > 0


class _Bare:
    """a bare la3dm_devmap on the context of a host-mode map, the region of the pointer-form tests and their buffers"""
    DT = dict(index=np.uint32, faces=np.uint8, normal=np.int16, dense_faces=np.uint8)

    def __init__(self):
        import torch
        import la3dm_amd
        from la3dm_amd import _lib
        self.torch, self.lib, self.H = torch, _lib, _lib.hip()
        self.m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)   # (lends its context)
        self.ctx = self.m.ctx()
        self.dm = C.c_void_p()
        assert self.H.la3dm_devmap_create(self.ctx, C.byref(self.dm)) == OK
        self.xyz, self.origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 1))
        self.lo = (np.asarray(self.origin, np.float32) + np.asarray(R.RECIPE_OFFSET, np.float32)).astype(np.float32)
        self.dims = np.array((77, 67, 39), np.uint32)
        self.n = int(self.dims.prod())
        self.sizes = dict(index=self.n, faces=self.n, normal=3 * self.n, dense_faces=self.n)

    def err(self):
        return self.H.la3dm_last_error(self.ctx).decode()

    def insert(self):
        o3 = (C.c_float * 3)(*[float(v) for v in self.origin])
        assert self.H.la3dm_devmap_insert_pointcloud_host(self.dm, np.ascontiguousarray(self.xyz, np.float32).ctypes.data, self.xyz.shape[0], 3, o3,
                                                          0.1, 0.5, 8.0, None) == OK

    def host_arrays(self, fill):
        h = {k: np.full(self.sizes[k], fill, self.DT[k]) for k in S.FIELDS}
        return h, self.lib.SurfaceOut(*[h[k].ctypes.data for k in S.FIELDS])

    def tensors(self, fill, fields=S.FIELDS):
        torch = self.torch
        tdt = dict(index=torch.int32, faces=torch.uint8, normal=torch.int16, dense_faces=torch.uint8)
        t = {k: torch.full((self.sizes[k],), fill, dtype=tdt[k], device=torch.device("cuda:0")) for k in S.FIELDS}
        torch.cuda.synchronize()
        return t, self.lib.SurfaceOut(*[t[k].data_ptr() if k in fields else None for k in S.FIELDS])

    def close(self):
        self.H.la3dm_devmap_destroy(self.dm)


def test_the_empty_map_in_both_pointer_forms(built):
    """GPU test 4 on a bare la3dm_devmap with no block: n = 0, dense_faces = 0, the list untouched, and n_solid = every voxel
    of the region when MISSING is in the solid mask, 0 when it is not — what the host-mode map answers"""
    import la3dm_amd
    b = _Bare()
    try:
        H, n, lop, dp = b.H, b.n, b.lo.ctypes.data, b.dims.ctypes.data
        mh = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)
        md = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
        assert md.is_device_resident() and not mh.is_device_resident()
        for solid, open_, s in ((S.OCC_M, OPTIMISTIC, 2), (S.OCC_M | S.MISS_M, S.FREE_M | S.UNK_M, 0), (S.MISS_M, S.FREE_M, 4)):
            want = mh.surface(b.lo, tuple(b.dims), solid=solid, open=open_, smooth=s, fields=S.FIELDS)
            n_solid = n if solid & S.MISS_M else 0
            assert (want["n"], want["n_solid"], want["face_count"]) == (0, n_solid, (0,) * 6) and (want["dense_faces"] == 0).all()
            S.assert_same(md.surface(b.lo, tuple(b.dims), solid=solid, open=open_, smooth=s, fields=S.FIELDS), want, ("empty", solid))
            par = b.lib.SurfaceParams(solid, open_, s)
            found, stats = C.c_uint64(5), b.lib.SurfaceStats()
            h, ho = b.host_arrays(9)
            assert H.la3dm_devmap_surface_host(b.dm, lop, dp, C.byref(par), n, C.byref(ho), C.byref(found), C.byref(stats), None) == OK, b.err()
            assert found.value == 0 and all((h[k] == 9).all() for k in S.LIST_FIELDS) and (h["dense_faces"] == 0).all()
            assert stats.as_dict() == {k: want[k] for k in S.STATS}
            t, do = b.tensors(9)
            found.value, stats = 5, b.lib.SurfaceStats()
            assert H.la3dm_devmap_surface_device(b.dm, lop, dp, C.byref(par), n, C.byref(do), C.byref(found), C.byref(stats), None) == OK, b.err()
            g = {k: t[k].cpu().numpy() for k in t}
            assert found.value == 0 and all((g[k] == 9).all() for k in S.LIST_FIELDS) and (g["dense_faces"] == 0).all()
            assert stats.as_dict() == {k: want[k] for k in S.STATS}
    finally:
        b.close()


def test_refusals_in_both_pointer_forms(built):
    """GPU test 5: refusals with their text, LA3DM_ERR_ARG and nothing written, in both pointer forms"""
    b = _Bare()
    try:
        H, n, lop, dp = b.H, b.n, b.lo.ctypes.data, b.dims.ctypes.data
        b.insert()
        par = b.lib.SurfaceParams(S.OCC_M, OPTIMISTIC, 2)
        found = C.c_uint64(77)
        h, ho = b.host_arrays(7)
        t, do = b.tensors(7)
        for fn, out in ((H.la3dm_devmap_surface_host, ho), (H.la3dm_devmap_surface_device, do)):
            def call(p=par, lo_p=lop, d_p=dp, cap=n, o=C.byref(out), nf=C.byref(found)):
                return fn(b.dm, lo_p, d_p, C.byref(p) if p is not None else None, cap, o, nf, None, None)
            P = b.lib.SurfaceParams
            for p, text in ((None, "params is NULL"), (P(0, 1, 0), "solid_mask"), (P(2, 0x20, 0), "open_mask"), (P(3, 1, 0), "must not overlap"),
                            (P(2, 1, 5), "smooth must not exceed")):
                assert call(p=p) == ERR_ARG and text in b.err(), (text, b.err())
            assert call(o=None) == ERR_ARG and "must not be NULL with cap > 0" in b.err()
            assert call(o=C.byref(b.lib.SurfaceOut(None, None, None, out.dense_faces))) == ERR_ARG and "must not be NULL with cap > 0" in b.err()
            assert call(o=C.byref(b.lib.SurfaceOut(None, out.faces, out.normal, None))) == ERR_ARG and "normal is set without" in b.err()
            assert call(lo_p=None) == ERR_ARG and "lo is NULL" in b.err()
            assert call(d_p=None) == ERR_ARG and "dims is NULL" in b.err()
            d0 = np.array((4, 0, 4), np.uint32)
            assert call(d_p=d0.ctypes.data) == ERR_ARG and "dims must be >= 1" in b.err()
            big = np.array(((1 << 10) - 6, (1 << 10) - 6, (1 << 8) - 5), np.uint32)      # padded by 6: one layer over 2^28
            assert call(d_p=big.ctypes.data, cap=0, o=None, nf=None) == ERR_ARG and "LA3DM_SURFACE_MAX_CELLS" in b.err(), b.err()
            at = np.array(((1 << 10) - 6, (1 << 10) - 6, (1 << 8) - 6), np.uint32)       # exactly 2^28: the next check answers
            assert call(d_p=at.ctypes.data, cap=0, o=None, nf=None) == ERR_ARG and "n_found is NULL" in b.err(), b.err()
            low = np.array((-209715.5, 0, 0), np.float32)
            assert call(lo_p=low.ctypes.data) == ERR_ARG and "padded box leave" in b.err(), b.err()
            assert call(nf=None) == ERR_ARG and "n_found is NULL" in b.err()
            assert fn(None, lop, dp, C.byref(par), n, C.byref(out), C.byref(found), None, None) == ERR_ARG
        assert found.value == 77 and all((h[k] == 7).all() for k in h) and all((t[k].cpu().numpy() == 7).all() for k in t)
    finally:
        b.close()


@pytest.mark.parametrize("solid,open_,smooth", [(S.OCC_M, OPTIMISTIC, 2), (S.OCC_M, S.FREE_M, 0), (S.OCC_M | S.UNK_M, S.FREE_M | S.MISS_M, 4)])
def test_device_pointer_form(built, solid, open_, smooth):
    """GPU test 6: the device-pointer form == the host-pointer form for every served subset of the arrays, with a cap below n
    leaving the entries past it alone"""
    b = _Bare()
    try:
        H, n, lop, dp = b.H, b.n, b.lo.ctypes.data, b.dims.ctypes.data
        b.insert()
        p = b.lib.SurfaceParams(solid, open_, smooth)
        found, stats = C.c_uint64(0), b.lib.SurfaceStats()
        h, ho = b.host_arrays(0x6E)
        assert H.la3dm_devmap_surface_host(b.dm, lop, dp, C.byref(p), n, C.byref(ho), C.byref(found), C.byref(stats), None) == OK, b.err()
        nf = int(found.value)
        assert nf > 0 and stats.n_surface == nf and (h["index"][nf:] == 0x6E).all() and (np.diff(h["index"][:nf].astype(np.int64)) > 0).all()
        assert (h["faces"][nf:] == 0x6E).all() and (h["normal"][3 * nf:] == 0x6E).all()
        assert int((h["dense_faces"] != 0).sum()) == nf and (h["dense_faces"][h["index"][:nf]] == h["faces"][:nf]).all()
        for fields, caps in ((S.FIELDS, (n, nf // 3)), (("faces", "dense_faces"), (nf // 3,)), (("index", "normal"), (nf - 1,)), ((), (0,))):
            for cap in caps:
                t, do = b.tensors(0x5A, fields)
                found.value, stats2 = 0, b.lib.SurfaceStats()
                assert H.la3dm_devmap_surface_device(b.dm, lop, dp, C.byref(p), cap, C.byref(do) if fields else None, C.byref(found),
                                                     C.byref(stats2), None) == OK, b.err()
                assert found.value == nf and stats2.as_dict() == stats.as_dict()
                k_out = min(cap, nf)
                for k in S.FIELDS:
                    g = t[k].cpu().numpy().view(b.DT[k])
                    width = 3 if k == "normal" else 1
                    if k not in fields:
                        assert (g == 0x5A).all(), k
                    elif k == "dense_faces":
                        assert (g == h[k]).all(), k
                    else:
                        assert (g[:width * k_out] == h[k][:width * k_out]).all() and (g[width * k_out:] == 0x5A).all(), (k, cap)
        print("device-pointer form: found", nf)
    finally:
        b.close()
