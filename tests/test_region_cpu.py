"""box and columns on a host-mode map (device = -1, no GPU): the voxels of an axis-aligned box as dense arrays and the same
box reduced along z, against an independent walk of the leaf list (tests/helpers/region_cases.py).  The map is two fused
and pruned scans, so the region holds collapsed groups — where the raw finest-layer node reads PRUNED and a box put
together from search_many is wrong."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402


def _recipe(depth):
    m, lv, lo = R.fused_map(depth)
    y = R.yardstick(m, lv, lo, R.RECIPE_DIMS)
    R.assert_region_exercises_the_feature(R.input_conditions(y, depth))
    return m, lv, lo, y


@pytest.mark.parametrize("depth", [3, 4])
def test_box_and_columns_equal_the_yardstick(built, depth):
    """item 1: every field, exact; columns == yardstick == the reduction of box's cls"""
    m, lv, lo, y = _recipe(depth)
    b = m.box(lo, R.RECIPE_DIMS)
    assert set(b) == set(R.BOX_FIELDS + R.INFO_FIELDS)
    R.assert_same(b, y, R.BOX_FIELDS + ("origin", "cell"), f"box d{depth}")
    assert b["block_key"] == y["block_key"]
    c = m.columns(lo, R.RECIPE_DIMS)
    assert set(c) == set(R.COL_FIELDS + R.INFO_FIELDS)
    R.assert_same(c, y, R.COL_FIELDS + ("origin", "cell"), f"columns d{depth}")
    R.assert_same(c, R.reduce_box(b["cls"]), R.COL_FIELDS, f"columns vs box d{depth}")
    assert c["block_key"] == y["block_key"]
    assert (c["counts"].sum(2) == R.RECIPE_DIMS[2]).all()
    assert m.mirror_syncs() == 0
    if depth == 3:
        assert np.abs(b["origin"] - np.array([-3.05, -3.05, -1.45], np.float32)).max() < 1e-5


@pytest.mark.parametrize("depth", [3, 4])
def test_box_against_search_many(built, depth):
    """item 2: where search_many reports an existing block and a state other than PRUNED, box agrees on state, A, B; where
    it reports PRUNED, box reports the covering leaf — the case a client that assembles the box from search_many gets
    wrong"""
    m, lv, lo, y = _recipe(depth)
    b = m.box(lo, R.RECIPE_DIMS)
    nx, ny, nz = R.RECIPE_DIMS
    res = np.float32(m.get_resolution())
    ijk = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    pts = (b["origin"][None, :] + ijk.astype(np.float32) * res).astype(np.float32)
    s = m.search_many(pts)
    cls, dep, A, B = (b[k].reshape(-1) for k in R.BOX_FIELDS)
    exists = s["exists"] != 0
    assert (exists == (cls != R.MISSING)).all()
    raw = exists & (s["state"] != 3)
    pruned = exists & (s["state"] == 3)
    print(f"d{depth}: {int(exists.sum())} voxels in existing blocks, {int(pruned.sum())} read raw PRUNED")
    assert (cls[raw] == s["state"][raw]).all() and (dep[raw] == depth - 1).all()
    assert (A[raw].view(np.uint32) == s["A"][raw].view(np.uint32)).all()
    assert (B[raw].view(np.uint32) == s["B"][raw].view(np.uint32)).all()
    assert pruned.sum() >= 5400 and (pruned == y["under_coarser"].reshape(-1)).all()
    assert (dep[pruned] < depth - 1).all() and np.isin(cls[pruned], (R.FREE, R.OCCUPIED)).all()
    assert (cls[exists] != 3).all()
    assert (dep[~exists] == 255).all()


@pytest.mark.parametrize("depth", [3, 4])
def test_sub_regions_are_slices(built, depth):
    """item 3: a box inside the recipe region, anchored at origin + (i0, j0, k0) * resolution, is a slice of the big one"""
    m, lv, lo, y = _recipe(depth)
    big = m.box(lo, R.RECIPE_DIMS)
    bigc = m.columns(lo, R.RECIPE_DIMS)
    nx, ny, nz = R.RECIPE_DIMS
    res = np.float32(m.get_resolution())
    rng = np.random.default_rng(11)
    cases = [((0, 0, 0), (1, 1, 1)), ((79, 79, 39), (1, 1, 1)), ((17, 42, 0), (1, 1, nz)), ((0, 0, 0), R.RECIPE_DIMS)]
    for _ in range(12):
        p0 = [int(rng.integers(0, n)) for n in (nx, ny, nz)]
        cases.append((tuple(p0), tuple(int(rng.integers(1, n - a + 1)) for n, a in zip((nx, ny, nz), p0))))
    for (i0, j0, k0), (dx, dy, dz) in cases:
        sub_lo = (big["origin"] + np.array([i0, j0, k0], np.float32) * res).astype(np.float32)
        sl = (slice(i0, i0 + dx), slice(j0, j0 + dy), slice(k0, k0 + dz))
        sub = m.box(sub_lo, (dx, dy, dz))
        R.assert_same(sub, {k: np.ascontiguousarray(big[k][sl]) for k in R.BOX_FIELDS}, R.BOX_FIELDS, ((i0, j0, k0), (dx, dy, dz)))
        subc = m.columns(sub_lo, (dx, dy, dz))
        R.assert_same(subc, R.reduce_box(big["cls"][sl]), R.COL_FIELDS, ("columns", (i0, j0, k0), (dx, dy, dz)))
        if dz == nz and k0 == 0:
            R.assert_same(subc, {k: np.ascontiguousarray(bigc[k][sl[:2]]) for k in R.COL_FIELDS}, R.COL_FIELDS)
        assert np.abs(sub["origin"] - sub_lo).max() < 1e-4


def test_arguments(built):
    """item 4: every refusal with its text, an empty map, optional outputs left out, the limits at their boundary"""
    import la3dm_amd
    from la3dm_amd import _lib
    m, lv, lo = R.fused_map(3)
    for q in (m.box, m.columns):
        for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, 1.1e8)):          # 1.1e8 / 0.1 >= 2^30
            with pytest.raises(RuntimeError, match="lo must be finite"):
                q(bad, (2, 2, 2))
        for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
            with pytest.raises(RuntimeError, match="dims must be >= 1"):
                q(lo, dims)
        with pytest.raises(RuntimeError, match="lo: the block field leaves"):
            q((-3.0e5, 0, 0), (2, 2, 2))                                     # block field < 0 at a block size of 0.4 m
        with pytest.raises(RuntimeError, match="dims: the region's block fields leave"):
            q((2.09e5, 0, 0), (1 << 16, 1, 1))                                # starts inside, ends beyond field 2^20 - 1
        with pytest.raises(ValueError):
            q(lo, (2, 2))
        with pytest.raises(ValueError):
            q(lo[:2], (2, 2, 2))
    with pytest.raises(ValueError, match="unknown fields"):
        m.box(lo, (2, 2, 2), fields=("cls", "state"))
    # the limits: refused before a buffer is looked at (the binding hands over one-element arrays for these)
    with pytest.raises(RuntimeError, match="LA3DM_BOX_MAX_CELLS"):
        m.box(lo, (1 << 10, 1 << 10, (1 << 10) + 1))
    with pytest.raises(RuntimeError, match="LA3DM_BOX_MAX_CELLS"):
        m.box(lo, (1 << 16, 1 << 16, 1))
    with pytest.raises(RuntimeError, match="more than 2\\^30 columns"):
        m.columns(lo, ((1 << 15) + 1, 1 << 15, 1))
    with pytest.raises(RuntimeError, match="LA3DM_COLUMNS_MAX_NZ"):
        m.columns(lo, (1, 1, (1 << 16) + 1))
    # ... and accepted at the boundary: the C view with no output array answers "cls / counts must not be NULL", i.e. the
    # region and its size passed (check order: limits before buffers); nothing of 2^30 cells is allocated
    M = _lib.maplib()
    lo3 = np.ascontiguousarray(lo, np.float32)
    info = _lib.RegionInfo()

    def c_call(fn, out, dims):
        d3 = np.array(dims, np.uint32)
        rc = fn(m._h, lo3.ctypes.data, d3.ctypes.data, C.byref(out), C.byref(info))
        return rc, M.la3dm_map_last_error().decode()
    rc, txt = c_call(M.la3dm_map_box, _lib.BoxOut(), (1 << 10, 1 << 10, 1 << 10))
    assert rc < 0 and "cls must not be NULL" in txt, txt
    rc, txt = c_call(M.la3dm_map_box, _lib.BoxOut(), (1 << 10, 1 << 10, (1 << 10) + 1))
    assert rc < 0 and "LA3DM_BOX_MAX_CELLS" in txt, txt
    rc, txt = c_call(M.la3dm_map_columns, _lib.ColumnsOut(), (1 << 15, 1 << 15, 1 << 16))
    assert rc < 0 and "counts must not be NULL" in txt, txt
    rc, txt = c_call(M.la3dm_map_columns, _lib.ColumnsOut(), (1 << 15, 1 << 15, (1 << 16) + 1))
    assert rc < 0 and "LA3DM_COLUMNS_MAX_NZ" in txt, txt
    d3 = np.array((2, 2, 2), np.uint32)
    assert M.la3dm_map_box(m._h, None, d3.ctypes.data, C.byref(_lib.BoxOut()), None) < 0 and "lo is NULL" in M.la3dm_map_last_error().decode()
    assert M.la3dm_map_box(m._h, lo3.ctypes.data, None, C.byref(_lib.BoxOut()), None) < 0 and "dims is NULL" in M.la3dm_map_last_error().decode()
    assert M.la3dm_map_columns(m._h, lo3.ctypes.data, d3.ctypes.data, None, None) < 0 and "out must not be NULL" in M.la3dm_map_last_error().decode()
    # nz = 2^16 itself is served
    tall = m.columns(lo, (1, 2, 1 << 16))
    assert tall["counts"].shape == (1, 2, 4) and (tall["counts"].sum(2) == 1 << 16).all()
    # optional outputs left out: the others are the same, info may be NULL
    full = m.box(lo, (9, 7, 5))
    only = m.box(lo, (9, 7, 5), fields=())
    assert set(only) == {"cls"} | set(R.INFO_FIELDS) and (only["cls"] == full["cls"]).all()
    ab = m.box(lo, (9, 7, 5), fields=("A",))
    assert set(ab) == {"cls", "A"} | set(R.INFO_FIELDS) and (ab["A"].view(np.uint32) == full["A"].view(np.uint32)).all()
    counts = np.zeros((9, 7, 4), np.uint32)
    d3 = np.array((9, 7, 5), np.uint32)
    assert M.la3dm_map_columns(m._h, lo3.ctypes.data, d3.ctypes.data, C.byref(_lib.ColumnsOut(counts.ctypes.data, None, None)), None) == 0
    assert (counts == m.columns(lo, (9, 7, 5))["counts"]).all()
    # an empty map: all MISSING, the default node, no mirror refresh
    empty = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
    _, a0, b0, _ = empty.search(0.0, 0.0, 0.0)
    b = empty.box(lo, (6, 5, 4))
    assert (b["cls"] == R.MISSING).all() and (b["leaf_depth"] == 255).all()
    assert (b["A"] == np.float32(a0)).all() and (b["B"] == np.float32(b0)).all()
    c = empty.columns(lo, (6, 5, 4))
    assert (c["counts"] == np.array([0, 0, 0, 4], np.uint32)).all() and (c["low_occ"] == -1).all() and (c["top_occ"] == -1).all()
    R.assert_same(b, m.box(lo, (6, 5, 4)), ("origin", "cell"))
    assert empty.mirror_syncs() == 0


def _anchor_coordinates(res, bs):
    """coordinates at and next to every boundary of the anchor arithmetic (voxel and block faces and centres, each with
    its two float32 neighbours), a seeded uniform sample and a few far values"""
    vals = []
    for k in range(-12, 13):
        for v in (np.float32(k) * res, np.float32(k + 0.5) * res, np.float32(k) * bs, np.float32(k + 0.5) * bs):
            v = np.float32(v)
            vals += [v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))]
    vals += list(np.random.default_rng(7).uniform(-50.0, 50.0, 600).astype(np.float32))
    vals += [1.0e5, -1.0e5, 52428.0, -52428.0]
    return np.array(vals, np.float32)


@pytest.mark.parametrize("depth", [3, 4])
def test_anchor_equals_the_yardstick_at_every_boundary(built, depth):
    """the anchor arithmetic (block field in float64, centre and cell in float32, the cell truncated and clamped) serves
    every region query of the host map and of the device library from one place: origin (bits), block_key and cell of
    columns(lo, (1, 1, 1)) against region_cases.anchor, every case accepted"""
    import la3dm_amd
    m = la3dm_amd.BGKOctoMap(**dict(R.YAML, block_depth=depth), device=-1)
    res = np.float32(m.get_resolution())
    bs = np.float32(np.float32(2.0 ** (depth - 1)) * res)
    vals = _anchor_coordinates(res, bs)
    rng = np.random.default_rng(13)
    los = np.stack([vals, vals[rng.permutation(vals.size)], vals[rng.permutation(vals.size)]], 1)
    assert los.shape == (904, 3)
    for lo in los:
        got = m.columns(lo, (1, 1, 1))
        b, c, _, origin = R.anchor(lo, res, depth)
        assert got["block_key"] == (b[0] << 40) | (b[1] << 20) | b[2], (lo, got["block_key"], b)
        assert (np.asarray(got["cell"]) == np.array(c)).all(), (lo, got["cell"], c)
        assert (np.asarray(got["origin"], np.float32).view(np.uint32) == origin.view(np.uint32)).all(), (lo, got["origin"], origin)


def test_header_declares_and_library_exports_the_new_symbols(built):
    """item 5"""
    from la3dm_amd import _lib
    for header, so, names in (("la3dm_map.h", _lib.MAP_SO, ("la3dm_map_box", "la3dm_map_columns")),
                              ("la3dm_hip.h", _lib.HIP_SO, ("la3dm_devmap_box_host", "la3dm_devmap_box_device",
                                                            "la3dm_devmap_columns_host", "la3dm_devmap_columns_device"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        if so == _lib.MAP_SO:
            C.CDLL(_lib.HIP_SO, mode=C.RTLD_GLOBAL)
        lib = C.CDLL(so)
        for n in names:
            assert re.search(r"\b" + n + r"\s*\(", txt), n
            assert hasattr(lib, n), n
    hip_h = open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
    for word in ("la3dm_box_out", "la3dm_columns_out", "la3dm_region_info", "LA3DM_BOX_MAX_CELLS (1u << 30)",
                 "LA3DM_COLUMNS_MAX_NZ (1u << 16)"):
        assert word in hip_h, word
