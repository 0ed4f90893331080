"""box and columns on the device-resident map: one HIP launch reads the region from the device pool
(csrc/devmap_region.h).  The yardstick is the host form of the same class (a host-mode map, the loop over its host
blocks), itself checked against an independent walk of the leaf list (tests/helpers/region_cases.py).  Every comparison
is exact: integers by ==, floats by their bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, pcd_path

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402

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


def _compare(md, mh, lo, dims, what):
    """device == host on box (all fields, and cls alone) and columns, with the info; returns the host answers"""
    bd, bh = md.box(lo, dims), mh.box(lo, dims)
    R.assert_same(bd, bh, R.BOX_FIELDS + ("origin", "cell"), (what, "box"))
    assert bd["block_key"] == bh["block_key"]
    assert (md.box(lo, dims, fields=())["cls"] == bh["cls"]).all()
    cd, ch = md.columns(lo, dims), mh.columns(lo, dims)
    R.assert_same(cd, ch, R.COL_FIELDS + ("origin", "cell"), (what, "columns"))
    R.assert_same(cd, R.reduce_box(bd["cls"]), R.COL_FIELDS, (what, "columns vs box"))
    assert md.is_device_resident()
    return bh, ch


def _aligned_lo(m, lo):
    """the centre of the first voxel of the block that holds lo: a block-aligned region"""
    info = m.columns(lo, (1, 1, 1))
    res = np.float32(m.get_resolution())
    return (info["origin"] - info["cell"].astype(np.float32) * res).astype(np.float32)


@pytest.mark.parametrize("depth", [3, 4])
def test_device_equals_host_bit_for_bit(built, depth):
    """item 6: BGK at block_depth 3 and 4, two fused (and pruned) scans: the recipe region — shown from the yardstick to
    hold every class, collapsed groups and whole missing columns — and a block-aligned one; the host form == the
    yardstick on that map; then a third insert (the pool grew, the table was rebuilt) and the same comparison"""
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    md, mh = _pair("BGKOctoMap", params, (1, 2))
    lo = R.recipe_lo()
    lv = mh.leaves()
    y = R.yardstick(mh, lv, lo, R.RECIPE_DIMS)
    R.assert_region_exercises_the_feature(R.input_conditions(y, depth))
    before_syncs = md.mirror_syncs()
    bh, ch = _compare(md, mh, lo, R.RECIPE_DIMS, f"bgk d{depth}")
    assert md.mirror_syncs() == before_syncs
    R.assert_same(bh, y, R.BOX_FIELDS + ("origin", "cell"), f"host form vs yardstick d{depth}")
    R.assert_same(ch, y, R.COL_FIELDS, f"host form vs yardstick d{depth}")
    assert bh["block_key"] == y["block_key"]
    lo_al = _aligned_lo(mh, lo)
    lim = 1 << (depth - 1)
    al = _compare(md, mh, lo_al, (20 * lim, 12 * lim, 10 * lim), f"bgk d{depth} aligned")[0]
    assert (md.box(lo_al, (1, 1, 1))["cell"] == 0).all() and (al["cls"] == R.OCCUPIED).any()
    # odd sizes: the tail of the four-voxel threads, rows that are no multiple of four
    for dims in ((1, 1, 1), (1, 1, 3), (3, 5, 7), (2, 2, 2), (1, 1, 41), (33, 1, 1), (5, 64, 1)):
        _compare(md, mh, lo, dims, f"bgk d{depth} {dims}")
    before = md.block_count()          # (refreshes the mirror; the queries do not depend on it either way)
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 5))
    for m in (md, mh):
        m.insert_pointcloud(xyz, origin, *INSERT)
    _compare(md, mh, lo, R.RECIPE_DIMS, f"bgk d{depth} after a further insert")
    _compare(md, mh, lo_al, (20 * lim, 12 * lim, 10 * lim), f"bgk d{depth} aligned, after a further insert")
    assert md.block_count() > before


@pytest.mark.parametrize("variant", ["GPOctoMap", "BGKLOctoMap", "BGKLVOctoMap"])
def test_device_equals_host_on_other_variants(built, variant):
    """item 7: GP (A, B hold m_ivar, ivar), BGK-L and BGK-LV on their own configurations; on BGK-LV an UNCERTAIN leaf is
    class 4 in box and counted with UNKNOWN in columns"""
    import la3dm_amd
    params, insert = {"GPOctoMap": (la3dm_amd.GP_YAML, INSERT), "BGKLOctoMap": (la3dm_amd.L_YAML, (0.1, 0.3, 8.0)),
                      "BGKLVOctoMap": (la3dm_amd.LV_YAML, (0.1, 0.3, 8.0))}[variant]
    md, mh = _pair(variant, dict(params), (1, 2), insert)
    lo = R.recipe_lo()
    bh, ch = _compare(md, mh, lo, R.RECIPE_DIMS, variant)
    n = {k: int((bh["cls"] == v).sum()) for k, v in (("free", 0), ("occupied", 1), ("unknown", 2), ("missing", 3), ("uncertain", 4))}
    print(variant, n, "leaf depths", np.unique(bh["leaf_depth"]).tolist())
    assert n["occupied"] > 0 and n["free"] > 0 and n["missing"] > 0, n
    assert sum(n.values()) == bh["cls"].size                       # no other class, PRUNED never
    assert (n["uncertain"] > 0) == (variant == "BGKLVOctoMap"), n      # (the host form: the device answer equals it)
    assert int(ch["counts"][:, :, 2].sum()) == n["unknown"] + n["uncertain"]
    assert int(ch["counts"][:, :, 3].sum()) == n["missing"]
    _compare(md, mh, lo, (7, 9, 11), variant + " small")


def test_no_mirror_refresh(built):
    """item 8: the queries are answered from the pool; the leaf iterator afterwards pays exactly one refresh"""
    import la3dm_amd
    md = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    assert md.mirror_syncs() == 0
    lo = R.recipe_lo()
    for i in (1, 2):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        md.insert_pointcloud(xyz, origin, *INSERT)
        before = md.mirror_syncs()
        b = md.box(lo, R.RECIPE_DIMS)
        c = md.columns(lo, R.RECIPE_DIMS)
        assert (b["cls"] == R.OCCUPIED).any() and (c["counts"][:, :, 1] > 0).any()
        assert md.is_device_resident() and md.mirror_syncs() == before
        lv = md.leaves()                                   # the iterator pays the refresh
        assert md.mirror_syncs() == before + 1 and lv["state"].size > 1000
        md.leaves()
        assert md.mirror_syncs() == before + 1             # ... once per insert
        R.assert_same(md.box(lo, R.RECIPE_DIMS), b, R.BOX_FIELDS)


def _dev_box(torch, n, dev, offset=0):
    t = dict(cls=torch.zeros(n + offset, dtype=torch.uint8, device=dev), leaf_depth=torch.zeros(n + offset, dtype=torch.uint8, device=dev),
             A=torch.zeros(n + offset, dtype=torch.float32, device=dev), B=torch.zeros(n + offset, dtype=torch.float32, device=dev))
    return t


def test_abi_errors_and_the_device_pointer_forms(built):
    """item 9: on a bare la3dm_devmap — refusals with their text, an empty map, optional outputs; the device-pointer forms
    (outputs in HBM) give the same bytes as the host-pointer forms, also through the one-voxel-per-thread kernel that an
    output without 4- / 16-byte alignment gets"""
    import torch
    import la3dm_amd
    from la3dm_amd import _lib
    H = _lib.hip()
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)   # (lends its context)
    ctx = m.ctx()
    dm = C.c_void_p()
    assert H.la3dm_devmap_create(ctx, C.byref(dm)) == OK
    err = lambda: H.la3dm_last_error(ctx).decode()   # noqa: E731
    try:
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 1))
        lo = (np.asarray(origin, np.float32) + np.asarray(R.RECIPE_OFFSET, np.float32)).astype(np.float32)
        dims = np.array((77, 67, 39), np.uint32)
        nb, nc = int(dims.prod()), int(dims[0] * dims[1])
        hb = dict(cls=np.full(nb, 9, np.uint8), leaf_depth=np.zeros(nb, np.uint8), A=np.zeros(nb, np.float32), B=np.zeros(nb, np.float32))
        hc = dict(counts=np.full((nc, 4), 9, np.uint32), low_occ=np.zeros(nc, np.int32), top_occ=np.zeros(nc, np.int32))
        bo = _lib.BoxOut(*[hb[k].ctypes.data for k, _ in _lib.BoxOut._fields_])
        co = _lib.ColumnsOut(*[hc[k].ctypes.data for k, _ in _lib.ColumnsOut._fields_])
        info = _lib.RegionInfo()
        lop, dp = lo.ctypes.data, dims.ctypes.data
        dev = torch.device("cuda:0")
        tb = _dev_box(torch, nb, dev)
        tc = dict(counts=torch.full((nc, 4), 9, dtype=torch.int32, device=dev), low_occ=torch.zeros(nc, dtype=torch.int32, device=dev),
                  top_occ=torch.zeros(nc, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        dbo = _lib.BoxOut(*[tb[k].data_ptr() for k, _ in _lib.BoxOut._fields_])
        dco = _lib.ColumnsOut(*[tc[k].data_ptr() for k, _ in _lib.ColumnsOut._fields_])
        # empty map: all MISSING with the default node, {0, 0, 0, nz} per column — host and device pointers
        assert H.la3dm_devmap_box_host(dm, lop, dp, C.byref(bo), C.byref(info)) == OK, err()
        assert (hb["cls"] == R.MISSING).all() and (hb["leaf_depth"] == 255).all()
        assert (hb["A"] == np.float32(0.001)).all() and (hb["B"] == np.float32(0.001)).all()
        assert H.la3dm_devmap_columns_host(dm, lop, dp, C.byref(co), None) == OK, err()
        assert (hc["counts"] == np.array([0, 0, 0, dims[2]], np.uint32)).all() and (hc["low_occ"] == -1).all() and (hc["top_occ"] == -1).all()
        assert H.la3dm_devmap_box_device(dm, lop, dp, C.byref(dbo), None) == OK, err()
        assert H.la3dm_devmap_columns_device(dm, lop, dp, C.byref(dco), None) == OK, err()
        for k in hb:
            assert (tb[k].cpu().numpy().view(np.uint8) == hb[k].view(np.uint8)).all(), k
        for k in hc:
            assert (tc[k].cpu().numpy().view(np.uint8).reshape(-1) == hc[k].view(np.uint8).reshape(-1)).all(), k
        empty_origin = list(info.origin)
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3,
                                                     0.1, 0.5, 8.0, None) == OK
        # refusals: LA3DM_ERR_ARG and a text that names the argument; nothing written
        hb["cls"][:] = 7
        forms = ((H.la3dm_devmap_box_host, bo, _lib.BoxOut, "cls", "LA3DM_BOX_MAX_CELLS", (1 << 10, 1 << 10, (1 << 10) + 1)),
                 (H.la3dm_devmap_box_device, dbo, _lib.BoxOut, "cls", "LA3DM_BOX_MAX_CELLS", (1 << 16, 1 << 16, 1)),
                 (H.la3dm_devmap_columns_host, co, _lib.ColumnsOut, "counts", "LA3DM_COLUMNS_MAX_NZ", (1, 1, (1 << 16) + 1)),
                 (H.la3dm_devmap_columns_device, dco, _lib.ColumnsOut, "counts", "2^30 columns", ((1 << 15) + 1, 1 << 15, 1)))
        for fn, out, empty_out, mandatory, limit_text, too_big in forms:
            for bad in ((np.nan, 0, 0), (0, -np.inf, 0), (0, 0, 1.1e8)):
                b3 = np.array(bad, np.float32)
                assert fn(dm, b3.ctypes.data, dp, C.byref(out), None) == ERR_ARG and "lo must be finite" in err()
            for z in range(3):
                d0 = dims.copy()
                d0[z] = 0
                assert fn(dm, lop, d0.ctypes.data, C.byref(out), None) == ERR_ARG and "dims must be >= 1" in err()
            assert fn(dm, None, dp, C.byref(out), None) == ERR_ARG and "lo is NULL" in err()
            assert fn(dm, lop, None, C.byref(out), None) == ERR_ARG and "dims is NULL" in err()
            assert fn(dm, lop, dp, None, None) == ERR_ARG and "out is NULL" in err()
            assert fn(dm, lop, dp, C.byref(empty_out()), None) == ERR_ARG and mandatory + " must not be NULL" in err()
            assert fn(None, lop, dp, C.byref(out), None) == ERR_ARG
            big = np.array(too_big, np.uint32)
            assert fn(dm, lop, big.ctypes.data, C.byref(out), None) == ERR_ARG and limit_text in err(), err()
            far = np.array((-3.0e5, 0, 0), np.float32)
            assert fn(dm, far.ctypes.data, dp, C.byref(out), None) == ERR_ARG and "lo: the block field leaves" in err()
            far = np.array((2.09e5, 0, 0), np.float32)
            long_x = np.array((1 << 16, 1, 1), np.uint32)
            assert fn(dm, far.ctypes.data, long_x.ctypes.data, C.byref(out), None) == ERR_ARG and "region's block fields leave" in err()
        assert (hb["cls"] == 7).all()
        # the limits themselves pass the size check (no output array: the next check answers)
        at = np.array((1 << 10, 1 << 10, 1 << 10), np.uint32)
        assert H.la3dm_devmap_box_host(dm, lop, at.ctypes.data, C.byref(_lib.BoxOut()), None) == ERR_ARG and "cls must not be NULL" in err()
        at = np.array((1 << 15, 1 << 15, 1 << 16), np.uint32)
        assert H.la3dm_devmap_columns_device(dm, lop, at.ctypes.data, C.byref(_lib.ColumnsOut()), None) == ERR_ARG and "counts must not be NULL" in err()
        # the map is still usable: host pointers, all outputs and only the mandatory ones
        assert H.la3dm_devmap_box_host(dm, lop, dp, C.byref(bo), C.byref(info)) == OK, err()
        assert list(info.origin) == empty_origin and (hb["cls"] == R.OCCUPIED).any() and (hb["cls"] == R.FREE).any() and (hb["cls"] == R.MISSING).any()
        assert H.la3dm_devmap_columns_host(dm, lop, dp, C.byref(co), None) == OK, err()
        want = R.reduce_box(hb["cls"].reshape(tuple(int(v) for v in dims)))
        assert (hc["counts"].reshape(want["counts"].shape) == want["counts"]).all()
        assert (hc["low_occ"].reshape(want["low_occ"].shape) == want["low_occ"]).all() and (hc["top_occ"].reshape(want["top_occ"].shape) == want["top_occ"]).all()
        only_cls = np.zeros(nb, np.uint8)
        assert H.la3dm_devmap_box_host(dm, lop, dp, C.byref(_lib.BoxOut(only_cls.ctypes.data, None, None, None)), None) == OK
        assert (only_cls == hb["cls"]).all()
        only_counts = np.zeros((nc, 4), np.uint32)
        assert H.la3dm_devmap_columns_host(dm, lop, dp, C.byref(_lib.ColumnsOut(only_counts.ctypes.data, None, None)), None) == OK
        assert (only_counts == hc["counts"]).all()
        # device pointers: aligned (four voxels per thread), then every array one element off (one voxel per thread;
        # counts 4 bytes off: scalar stores)
        for offset in (0, 1):
            tb = _dev_box(torch, nb, dev, offset)
            tc = dict(counts=torch.zeros(4 * nc + offset, dtype=torch.int32, device=dev), low_occ=torch.zeros(nc + offset, dtype=torch.int32, device=dev),
                      top_occ=torch.zeros(nc + offset, dtype=torch.int32, device=dev))
            torch.cuda.synchronize()
            dbo = _lib.BoxOut(*[tb[k][offset:].data_ptr() for k, _ in _lib.BoxOut._fields_])
            dco = _lib.ColumnsOut(*[tc[k][offset:].data_ptr() for k, _ in _lib.ColumnsOut._fields_])
            assert (tb["cls"][offset:].data_ptr() & 3) == offset
            info2 = _lib.RegionInfo()
            assert H.la3dm_devmap_box_device(dm, lop, dp, C.byref(dbo), C.byref(info2)) == OK, err()
            assert H.la3dm_devmap_columns_device(dm, lop, dp, C.byref(dco), None) == OK, err()
            assert list(info2.origin) == list(info.origin) and info2.block_key == info.block_key and list(info2.cell) == list(info.cell)
            for k in hb:
                got = tb[k].cpu().numpy()
                assert (got[offset:].view(np.uint8) == hb[k].view(np.uint8)).all(), (offset, k)
                assert (got[:offset] == 0).all()
            for k in hc:
                got = tc[k].cpu().numpy()
                assert (got[offset:].view(np.uint8) == hc[k].reshape(-1).view(np.uint8)).all(), (offset, k)
                assert (got[:offset] == 0).all()
    finally:
        H.la3dm_devmap_destroy(dm)


def test_a_large_request(built):
    """item 10: columns of 2048 x 2048 x 64 and box of 512 x 512 x 64 (cls only) round the map, mostly MISSING; 20 random
    sub-regions of each agree with the host form (a sub-region is a slice of the big answer)"""
    import la3dm_amd
    md, mh = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML), (1, 2))
    _, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 2))
    res = np.float32(md.get_resolution())
    rng = np.random.default_rng(21)
    o = np.asarray(origin, np.float32)
    for kind, n_xy in (("columns", 2048), ("box", 512)):
        lo = (o - np.array([n_xy / 2 * 0.1, n_xy / 2 * 0.1, 3.2], np.float32)).astype(np.float32)
        dims = (n_xy, n_xy, 64)
        if kind == "columns":
            big = md.columns(lo, dims)
            assert (big["counts"].sum(2) == 64).all()
            inside = big["counts"][:, :, 3] < 64
        else:
            big = md.box(lo, dims, fields=())
            inside = (big["cls"] != R.MISSING).any(2)
        assert md.is_device_resident() and md.mirror_syncs() == 0
        frac = float(inside.mean())
        print(f"{kind} {dims}: {int(inside.sum())} columns touch a block ({frac:.4f})")
        assert 0.0 < frac < 0.5                            # mostly MISSING, and the map is in it
        ii, jj = np.nonzero(inside)
        for t in range(20):                                # half of them over the map, half anywhere
            if t % 2 == 0:
                q = int(rng.integers(0, ii.size))
                i0, j0 = min(max(int(ii[q]) - 16, 0), n_xy - 32), min(max(int(jj[q]) - 16, 0), n_xy - 32)
            else:
                i0, j0 = int(rng.integers(0, n_xy - 32)), int(rng.integers(0, n_xy - 32))
            sub_lo = (big["origin"] + np.array([i0, j0, 0], np.float32) * res).astype(np.float32)
            if kind == "columns":
                want = mh.columns(sub_lo, (32, 32, 64))
                R.assert_same({k: np.ascontiguousarray(big[k][i0:i0 + 32, j0:j0 + 32]) for k in R.COL_FIELDS}, want, R.COL_FIELDS, (kind, i0, j0))
            else:
                want = mh.box(sub_lo, (32, 32, 64), fields=())
                assert (big["cls"][i0:i0 + 32, j0:j0 + 32] == want["cls"]).all(), (kind, i0, j0)


def test_example_program(built):
    """item 11: examples/occupancy_grid.cpp (built by build()) == the Python binding on the same map and region"""
    import la3dm_amd
    exe = os.path.join(ROOT, "examples", "occupancy_grid")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "3"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("grid 128 x 128 x 32 from ")
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    for i in (1, 2, 3):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        m.insert_pointcloud(xyz, origin, *INSERT)
    o = np.asarray(origin, np.float32)
    lo = np.array([o[0] - np.float32(6.4), o[1] - np.float32(6.4), o[2] - np.float32(1.6)], np.float32)
    c = m.columns(lo, (128, 128, 32))
    occ = c["counts"][:, :, 1] > 0
    free_only = ~occ & (c["counts"][:, :, 0] > 0)
    tok = lines[0].split()
    got = {tok[k]: tok[k + 1] for k in range(len(tok) - 1)}
    assert int(got["occupied"]) == int(occ.sum()) and int(got["occupied"]) > 500
    assert int(got["free_only"]) == int(free_only.sum()) and int(got["free_only"]) > 500
    assert int(got["unknown"]) == 128 * 128 - int(occ.sum()) - int(free_only.sum())
    assert int(got["top_occ_max"]) == int(c["top_occ"].max())
    assert got["mirror_syncs"] == "0" and got["device_resident"] == "1"
    at = tok.index("from")
    assert np.allclose([float(tok[at + 1]), float(tok[at + 2]), float(tok[at + 3].rstrip(":"))], c["origin"], atol=1e-4)
