"""distance_field on a host-mode map (device = -1, no GPU): the exact Euclidean distance transform of a map region against
two independent yardsticks (tests/helpers/distance_cases.py) — scipy's EDT and the definition by brute force — over the
classes of region_cases.yardstick.  Squared distances in voxel units are integers: every comparison is exact, integers by
==, floats by their bits."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import distance_cases as D  # noqa: E402


def _recipe(depth):
    m, lv, lo = R.fused_map(depth)
    y = R.yardstick(m, lv, lo, R.RECIPE_DIMS)
    return m, lv, lo, y


@pytest.mark.parametrize("depth", [3, 4])
def test_against_two_yardsticks(built, depth):
    """items 1 and 2: the recipe region against scipy's EDT, a sub-box of it against the definition, for four masks and
    three radii; the input conditions are counted from the yardstick first"""
    m, lv, lo, y = _recipe(depth)
    res = m.get_resolution()
    D.assert_exercises_the_feature(D.input_conditions(y["cls"]))
    sl = tuple(slice(o, o + n) for o, n in zip(D.SUB_OFFSET, D.SUB_DIMS))
    sub_cls = np.ascontiguousarray(y["cls"][sl])
    sub_lo = (y["origin"] + np.array(D.SUB_OFFSET, np.float32) * np.float32(res)).astype(np.float32)
    brute = {mask: D.squared_brute(sub_cls, mask) for mask in D.MASKS}          # (radius only truncates: once per mask)
    b8 = D.finish(brute[D.MASKS[0]], 8, res)["d2"]
    n_sub = dict(zeros=int((b8 == 0).sum()), finite=int(((b8 > 0) & (b8 != D.FAR)).sum()), far=int((b8 == D.FAR).sum()))
    print(f"sub-box {D.SUB_OFFSET} + {D.SUB_DIMS}, mask OCCUPIED, radius 8: {n_sub}")
    assert min(n_sub.values()) >= 500, n_sub               # the sub-box holds obstacles, finite distances and FAR
    for mask in D.MASKS:
        for radius in D.RADII:
            got = m.distance_field(lo, R.RECIPE_DIMS, obstacles=mask, radius=radius)
            assert set(got) == {"d2", "dist"} | set(R.INFO_FIELDS)
            assert got["d2"].dtype == np.uint32 and got["dist"].dtype == np.float32
            D.assert_same(got, D.yardstick_a(y["cls"], mask, radius, res), ("A", depth, mask, radius))
            R.assert_same(got, y, ("origin", "cell"), ("info", depth))
            assert got["block_key"] == y["block_key"]
            sub = m.distance_field(sub_lo, D.SUB_DIMS, obstacles=mask, radius=radius)
            b = D.finish(brute[mask], radius, res)
            D.assert_same(sub, b, ("B", depth, mask, radius))
            D.assert_same(b, D.yardstick_a(sub_cls, mask, radius, res), ("A vs B", depth, mask, radius))
    assert m.mirror_syncs() == 0


@pytest.mark.parametrize("depth", [3, 4])
def test_algebra_of_the_definition(built, depth):
    """item 3, exact: the union of masks is the minimum; a smaller radius only truncates; zeros sit exactly on the
    obstacles; dist is the fp32 root times the resolution"""
    m, lv, lo, y = _recipe(depth)
    res = np.float32(m.get_resolution())
    dims = R.RECIPE_DIMS
    box_cls = m.box(lo, dims, fields=())["cls"]
    single = {c: m.distance_field(lo, dims, obstacles=1 << c, radius=40, fields=("d2",))["d2"] for c in range(4)}
    for a, b in ((0, 1), (1, 2), (2, 3), (0, 3)):
        both = m.distance_field(lo, dims, obstacles=(1 << a) | (1 << b), radius=40, fields=("d2",))["d2"]
        assert (both == np.minimum(single[a], single[b])).all(), (a, b)
    all4 = m.distance_field(lo, dims, obstacles=0xF, radius=40, fields=("d2",))["d2"]
    assert (all4 == 0).all()                                # every voxel has one of the four classes
    names = m.distance_field(lo, dims, obstacles=("occupied", "free"), radius=40, fields=("d2",))["d2"]
    assert (names == np.minimum(single[0], single[1])).all()
    assert (m.distance_field(lo, dims, obstacles="occupied", radius=40, fields="d2")["d2"] == single[1]).all()
    for mask in D.MASKS:
        big = m.distance_field(lo, dims, obstacles=mask, radius=40)
        for r1 in (1, 8, 20, 39):
            small = m.distance_field(lo, dims, obstacles=mask, radius=r1)
            cut = np.where(big["d2"] > r1 * r1, np.uint32(D.FAR), big["d2"])
            assert (small["d2"] == cut).all(), (mask, r1)
        assert ((big["d2"] == 0) == D.obstacles_of(box_cls, mask)).all(), mask
        far = big["d2"] == D.FAR
        want = np.where(far, np.float32(np.inf), np.sqrt(big["d2"].astype(np.float32)) * res).astype(np.float32)
        assert (big["dist"].view(np.uint32) == want.view(np.uint32)).all(), mask
        assert np.isinf(big["dist"][far]).all() and np.isfinite(big["dist"][~far]).all()


def test_shapes(built):
    """item 4: single voxels, single lines along every axis, nz = 1, lines shorter than the radius, radius 1 and a radius
    far beyond the region; lines of 3000 voxels across the map at radius 1024"""
    m, lv, lo, y = _recipe(3)
    res = m.get_resolution()
    rlo = (y["origin"] + np.array((37, 41, 14), np.float32) * np.float32(res)).astype(np.float32)   # in the thick of the map
    seen = dict(zeros=0, finite=0, far=0)
    for dims in D.SHAPES:
        cls = R.yardstick(m, lv, rlo, dims)["cls"]
        for mask in D.MASKS:
            for radius in D.SHAPE_RADII:
                got = m.distance_field(rlo, dims, obstacles=mask, radius=radius)
                assert got["d2"].shape == dims and got["dist"].shape == dims
                want = D.yardstick_a(cls, mask, radius, res)
                D.assert_same(got, want, (dims, mask, radius))
                seen["zeros"] += int((want["d2"] == 0).sum())
                seen["far"] += int((want["d2"] == D.FAR).sum())
                seen["finite"] += int(((want["d2"] > 0) & (want["d2"] != D.FAR)).sum())
    print(f"small shapes: {seen}")
    assert min(seen.values()) > 50, seen
    for dims in D.LONG_SHAPES:
        llo = D.long_line_lo(y, res, dims)
        cls = R.yardstick(m, lv, llo, dims)["cls"]
        for mask in (D.MASKS[0], (1 << R.OCCUPIED) | (1 << R.UNKNOWN)):
            want = D.yardstick_a(cls, mask, 1024, res)
            n = dict(zeros=int((want["d2"] == 0).sum()), far=int((want["d2"] == D.FAR).sum()), max=int(want["d2"][want["d2"] != D.FAR].max()))
            print(f"{dims} mask {mask} radius 1024: {n}")
            assert n["zeros"] > 0 and n["far"] > 0 and n["max"] > 1000 * 1000, n   # obstacles, FAR, and the window used in full
            D.assert_same(m.distance_field(llo, dims, obstacles=mask, radius=1024), want, (dims, mask))
            D.assert_same(m.distance_field(llo, dims, obstacles=mask, radius=300), D.yardstick_a(cls, mask, 300, res), (dims, mask, 300))


def test_arguments(built):
    """item 5: every refusal with its text, the limit at its boundary, one field at a time, info = NULL, an empty map"""
    import la3dm_amd
    from la3dm_amd import _lib
    m, lv, lo = R.fused_map(3)
    q = m.distance_field
    for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, 1.1e8)):
        with pytest.raises(RuntimeError, match="lo must be finite"):
            q(bad, (2, 2, 2))
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        with pytest.raises(RuntimeError, match="dims must be >= 1"):
            q(lo, dims)
    with pytest.raises(RuntimeError, match="lo: the block field leaves"):
        q((-3.0e5, 0, 0), (2, 2, 2))
    with pytest.raises(RuntimeError, match="dims: the region's block fields leave"):
        q((2.09e5, 0, 0), (1 << 16, 1, 1))
    with pytest.raises(ValueError):
        q(lo, (2, 2))
    with pytest.raises(ValueError):
        q(lo[:2], (2, 2, 2))
    with pytest.raises(ValueError, match="unknown fields"):
        q(lo, (2, 2, 2), fields=("d2", "cls"))
    for mask in (0, 0x20, 0x3F, 1 << 31, ()):
        with pytest.raises(RuntimeError, match="obstacle_mask must hold"):
            q(lo, (2, 2, 2), obstacles=mask)
    for radius in (0, 1025, 1 << 20):
        with pytest.raises(RuntimeError, match="radius must lie in"):
            q(lo, (2, 2, 2), radius=radius)
    assert q(lo, (2, 2, 2), obstacles=0x1F, radius=1024)["d2"].shape == (2, 2, 2)       # the limits themselves are served
    # the voxel limit: refused before a buffer is looked at (the binding hands over one-element arrays for these)
    for dims in (((1 << 28) + 1, 1, 1), (1 << 10, 1 << 10, (1 << 8) + 1), (1 << 16, 1 << 16, 1)):
        with pytest.raises(RuntimeError, match="LA3DM_DF_MAX_CELLS"):
            q(lo, dims)
    M = _lib.maplib()
    lo3 = np.ascontiguousarray(lo, np.float32)
    info = _lib.RegionInfo()

    def c_call(out, dims, mask=2, radius=8, lo_p=lo3.ctypes.data, with_dims=True, with_info=True):
        d3 = np.array(dims, np.uint32)
        rc = M.la3dm_map_distance_field(m._h, lo_p, d3.ctypes.data if with_dims else None, mask, radius, out,
                                        C.byref(info) if with_info else None)
        return rc, M.la3dm_map_last_error().decode()
    # ... and accepted at the boundary: with no output array the call answers "d2 or dist must not be NULL", i.e. the region
    # and its size passed (check order: limits before buffers); nothing of 2^28 cells is allocated
    rc, txt = c_call(C.byref(_lib.DistanceOut()), (1 << 10, 1 << 10, 1 << 8))
    assert rc < 0 and "d2 or dist must not be NULL" in txt, txt
    rc, txt = c_call(C.byref(_lib.DistanceOut()), (1 << 10, 1 << 10, (1 << 8) + 1))
    assert rc < 0 and "LA3DM_DF_MAX_CELLS" in txt, txt
    rc, txt = c_call(None, (2, 2, 2))
    assert rc < 0 and "d2 or dist must not be NULL" in txt, txt
    rc, txt = c_call(C.byref(_lib.DistanceOut()), (2, 2, 2), lo_p=None)
    assert rc < 0 and "lo is NULL" in txt, txt
    rc, txt = c_call(C.byref(_lib.DistanceOut()), (2, 2, 2), with_dims=False)
    assert rc < 0 and "dims is NULL" in txt, txt
    rc, txt = c_call(C.byref(_lib.DistanceOut()), (2, 2, 2), mask=0)
    assert rc < 0 and "obstacle_mask" in txt, txt
    rc, txt = c_call(C.byref(_lib.DistanceOut()), (2, 2, 2), radius=0)
    assert rc < 0 and "radius" in txt, txt
    # one field at a time gives the same values as both; info may be NULL
    dims = (9, 7, 5)
    full = q(lo, dims, radius=6)
    only = q(lo, dims, radius=6, fields=("d2",))
    assert set(only) == {"d2"} | set(R.INFO_FIELDS) and (only["d2"] == full["d2"]).all()
    only = q(lo, dims, radius=6, fields=("dist",))
    assert set(only) == {"dist"} | set(R.INFO_FIELDS) and (only["dist"].view(np.uint32) == full["dist"].view(np.uint32)).all()
    R.assert_same(full, m.box(lo, dims), ("origin", "cell"))
    d2 = np.zeros(dims, np.uint32)
    rc, txt = c_call(C.byref(_lib.DistanceOut(d2.ctypes.data, None)), dims, radius=6, with_info=False)
    assert rc == 0 and (d2 == full["d2"]).all(), txt
    dist = np.zeros(dims, np.float32)
    rc, txt = c_call(C.byref(_lib.DistanceOut(None, dist.ctypes.data)), dims, radius=6, with_info=False)
    assert rc == 0 and (dist.view(np.uint32) == full["dist"].view(np.uint32)).all(), txt
    # an empty map: every voxel is MISSING — all obstacles if the mask holds bit 3, none otherwise; no mirror refresh
    empty = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
    e = empty.distance_field(lo, (6, 5, 4), obstacles=("occupied", "missing"), radius=3)
    assert (e["d2"] == 0).all() and (e["dist"].view(np.uint32) == 0).all()
    e = empty.distance_field(lo, (6, 5, 4), obstacles=0x17, radius=3)
    assert (e["d2"] == D.FAR).all() and (e["dist"] == np.float32(np.inf)).all()
    R.assert_same(e, m.box(lo, (6, 5, 4)), ("origin", "cell"))
    assert empty.mirror_syncs() == 0
    assert la3dm_amd.DF_FAR == D.FAR


def test_header_declares_and_library_exports_the_new_symbols(built):
    """item 6"""
    from la3dm_amd import _lib
    for header, so, names in (("la3dm_map.h", _lib.MAP_SO, ("la3dm_map_distance_field",)),
                              ("la3dm_hip.h", _lib.HIP_SO, ("la3dm_devmap_distance_host", "la3dm_devmap_distance_device"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        if so == _lib.MAP_SO:
            C.CDLL(_lib.HIP_SO, mode=C.RTLD_GLOBAL)
        lib = C.CDLL(so)
        for n in names:
            assert re.search(r"\b" + n + r"\s*\(", txt), n
            assert hasattr(lib, n), n
            assert n in _lib.HIP_SYMBOLS + _lib.MAP_SYMBOLS, n
    hip_h = open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
    assert "la3dm_distance_out" in hip_h
    for define in (r"#define\s+LA3DM_DF_FAR\s+0xFFFFFFFFu", r"#define\s+LA3DM_DF_MAX_RADIUS\s+1024u",
                   r"#define\s+LA3DM_DF_MAX_CELLS\s+\(1u << 28\)"):
        assert re.search(define, hip_h), define
