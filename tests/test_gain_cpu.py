"""gain on a host-mode map (device = -1, no GPU): per candidate viewpoint the number of distinct voxels of a region that a
fan of rays walks over and whose class is in the count mask, against an independent yardstick
(tests/helpers/gain_cases.py: raycast_many's step counts, the plain RayCaster's rows, a decode of their keys and the classes
of region_cases.yardstick).  Everything after the walk is integers: every comparison is exact."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import gain_cases as G  # noqa: E402

_RECIPES = {}


def _recipe(depth):
    if depth not in _RECIPES:
        m, lv, lo = R.fused_map(depth)
        y = R.yardstick(m, lv, lo, R.RECIPE_DIMS)
        origins, _ = G.viewpoints(y, m.get_resolution())
        _RECIPES[depth] = (m, lv, lo, y, origins)
    return _RECIPES[depth]


@pytest.mark.parametrize("depth", [3, 4])
def test_recipe_against_the_yardstick(built, depth):
    """CPU test 1: seven viewpoints x 256 offsets of 4 m (and x 96 of 3 m) on the recipe region, the four cases: gain, seen,
    started and hits; the input conditions are counted from the yardstick first"""
    m, lv, lo, y, origins = _recipe(depth)
    G.assert_exercises_the_feature(G.input_conditions(m, lv, y, lo, R.RECIPE_DIMS, origins, depth))
    W = (int(np.prod(R.RECIPE_DIMS)) + 31) // 32
    for offsets in (G.fan(256, 4.0), G.fan(96, 3.0)):
        for count, stop, budget in G.CASES:
            want = G.yardstick(m, lv, lo, R.RECIPE_DIMS, origins, offsets, count, stop, budget, cls=y["cls"])
            got = m.gain(lo, R.RECIPE_DIMS, origins, offsets, count=count, stop=stop, max_steps=budget, fields=G.FIELDS)
            assert set(got) == set(G.FIELDS) | set(R.INFO_FIELDS)
            assert got["seen"].shape == (7, W) and all(got[k].dtype == np.uint32 for k in G.FIELDS)
            G.assert_same(got, want, (depth, offsets.shape[0], count, stop, budget))
            print(f"depth {depth} fan {offsets.shape[0]} count {count:#x} stop {stop:#x} budget {budget}: gains {want['gain'].tolist()}")
    R.assert_same(got, y, ("origin", "cell"), "info")
    assert got["block_key"] == y["block_key"]
    # names select the same masks; the defaults are the planner's: count UNKNOWN | MISSING, stop OCCUPIED, 4096 rows, gain alone
    want = G.yardstick(m, lv, lo, R.RECIPE_DIMS, origins, G.fan(96, 3.0), 0xC, 0x2, 4096, cls=y["cls"])
    dflt = m.gain(lo, R.RECIPE_DIMS, origins, G.fan(96, 3.0))
    assert set(dflt) == {"gain"} | set(R.INFO_FIELDS) and (dflt["gain"] == want["gain"]).all()
    names = m.gain(lo, R.RECIPE_DIMS, origins, G.fan(96, 3.0), count=("missing", "unknown"), stop="occupied", fields=("hits", "seen"))
    G.assert_same(names, want, "names", ("gain", "hits", "seen"))
    assert "started" not in names
    # the sum of raycast_many's per-ray counts is not the gain: it counts a voxel once per ray that crosses it
    assert int(want["marked"].sum()) > int(want["gain"].sum())
    assert m.mirror_syncs() == 0


def _small(depth):
    """(m, lv, y, three viewpoints near the anchor of the small shapes, their voxels)"""
    m, lv, lo, y, _ = _recipe(depth)
    near, pick = G.near_viewpoints(y, m.get_resolution())
    return m, lv, y, near, pick


@pytest.mark.parametrize("depth", [3, 4])
def test_small_shapes(built, depth):
    """CPU test 2: the region as a sub-box in the thick of the recipe, three viewpoints next to it, seen compared bit for
    bit: the word boundaries of the voxel count, a region that does not hold the viewpoints, a single offset and 256 copies
    of it, invalid origins between valid ones"""
    m, lv, y, near, pick = _small(depth)
    marked = 0
    for what, lo, dims, origins, offsets in G.small_cases(m, y, near, pick):
        for count, stop, budget in G.SMALL_CASES:
            want = G.yardstick(m, lv, lo, dims, origins, offsets, count, stop, budget)
            got = m.gain(lo, dims, origins, offsets, count=count, stop=stop, max_steps=budget, fields=G.FIELDS)
            G.assert_same(got, want, (depth, what, count, stop, budget))
            marked += int(want["gain"].sum())
            if what.startswith("a NaN"):
                alone = m.gain(lo, dims, near, offsets, count=count, stop=stop, max_steps=budget, fields=G.FIELDS)
                assert (got["gain"][[1, 3]] == 0).all() and (got["started"][[1, 3]] == 0).all() and (got["seen"][[1, 3]] == 0).all()
                for k in G.FIELDS:
                    assert (got[k][[0, 2, 4]] == alone[k]).all(), k                  # the neighbours' answers are untouched
            if what == "m = 1":
                copies = m.gain(lo, dims, origins, np.repeat(offsets, 256, 0), count=count, stop=stop, max_steps=budget, fields=G.FIELDS)
                G.assert_same(copies, dict(want, started=want["started"] * 256, hits=want["hits"] * 256), "256 copies of one offset")
    print(f"depth {depth} small shapes: {marked} voxels marked in all")
    assert marked > 200


def test_empty_map_trivial_cases_and_refusals(built):
    """CPU test 3: an empty map answers all zero; n = 0 is served and writes nothing; every refusal raises with a text that
    names the argument and leaves the output arrays alone"""
    import la3dm_amd
    from la3dm_amd import _lib
    m, lv, lo, y, origins = _recipe(3)
    f = G.fan(96, 3.0)
    empty = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
    e = empty.gain(lo, (6, 5, 4), origins, f, count=0x1F, stop=0, fields=G.FIELDS)
    assert all((e[k] == 0).all() for k in G.FIELDS) and e["seen"].shape == (7, 4)
    R.assert_same(e, m.box(lo, (6, 5, 4)), ("origin", "cell"))
    z = m.gain(lo, (6, 5, 4), np.zeros((0, 3), np.float32), f, fields=G.FIELDS)
    assert z["gain"].shape == (0,) and z["seen"].shape == (0, 4)
    q = lambda **kw: m.gain(kw.pop("lo", lo), kw.pop("dims", (4, 4, 4)), kw.pop("origins", origins), kw.pop("offsets", f), **kw)   # noqa: E731
    for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, 1.1e8)):
        with pytest.raises(RuntimeError, match="lo must be finite"):
            q(lo=bad)
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        with pytest.raises(RuntimeError, match="dims must be >= 1"):
            q(dims=dims)
    with pytest.raises(RuntimeError, match="lo: the block field leaves"):
        q(lo=(-3.0e5, 0, 0))
    with pytest.raises(RuntimeError, match="dims: the region's block fields leave"):
        q(lo=(2.09e5, 0, 0), dims=(1 << 16, 1, 1))
    for dims in (((1 << 28) + 1, 1, 1), (1 << 10, 1 << 10, (1 << 8) + 1), (0xFFFFFFFF,) * 3):
        with pytest.raises(RuntimeError, match="LA3DM_GAIN_MAX_CELLS"):
            q(dims=dims)
    with pytest.raises(ValueError, match="unknown fields"):
        q(fields=("gain", "cls"))
    for mask in (0, 0x20, 0x3F, 1 << 31, ()):
        with pytest.raises(RuntimeError, match="count_mask must hold"):
            q(count=mask)
    for mask in (0x20, 0x22, 1 << 31):
        with pytest.raises(RuntimeError, match="stop_mask must hold"):
            q(stop=mask)
    assert q(stop=(), max_steps=1)["gain"].shape == (7,) and q(count=0x1F, stop=0x1F, max_steps=1 << 20)["gain"].shape == (7,)
    for budget in (0, (1 << 20) + 1):
        with pytest.raises(RuntimeError, match="max_steps must lie in"):
            q(max_steps=budget)
    with pytest.raises(RuntimeError, match="m must be >= 1"):
        q(offsets=np.zeros((0, 3), np.float32))
    with pytest.raises(RuntimeError, match="m must be >= 1"):
        q(origins=np.zeros((0, 3), np.float32), offsets=np.zeros((0, 3), np.float32))
    # the products, through the C view: the pointers are never followed, the limits answer first
    M = _lib.maplib()
    lo3, d3 = np.ascontiguousarray(lo, np.float32), np.array((4, 4, 4), np.uint32)
    o3, f3 = np.ascontiguousarray(origins), np.ascontiguousarray(f)
    sent = {k: np.full(64, 7, np.uint32) for k in G.FIELDS}
    out = _lib.GainOut(*[sent[k].ctypes.data for k in G.FIELDS])

    def c_call(lo_p=lo3.ctypes.data, dims=(4, 4, 4), with_dims=True, o_p=o3.ctypes.data, n=7, f_p=f3.ctypes.data, nd=96, count=0xC, stop=0x2,
               budget=4096, o=C.byref(out)):
        d3 = np.array(dims, np.uint32)
        rc = M.la3dm_map_gain(m._h, lo_p, d3.ctypes.data if with_dims else None, o_p, n, f_p, nd, count, stop, budget, o, None)
        return rc, M.la3dm_map_last_error().decode()
    for kw, text in ((dict(count=0), "count_mask"), (dict(count=0x40), "count_mask"), (dict(stop=0x20), "stop_mask"),
                     (dict(budget=0), "max_steps"), (dict(budget=(1 << 20) + 1), "max_steps"), (dict(nd=0), "m must be >= 1"),
                     (dict(n=1 << 20, nd=(1 << 8) + 1), "LA3DM_GAIN_MAX_RAYS"), (dict(n=(1 << 28) + 1, nd=1), "LA3DM_GAIN_MAX_RAYS"),
                     (dict(lo_p=None), "lo is NULL"), (dict(with_dims=False), "dims is NULL"), (dict(dims=(4, 0, 4)), "dims must be >= 1"),
                     (dict(dims=((1 << 28) + 1, 1, 1), o=None), "LA3DM_GAIN_MAX_CELLS"),
                     # n * W: 2^28 voxels are 2^23 words; 33 viewpoints of them are over the limit, 32 are exactly at it
                     (dict(dims=(1 << 10, 1 << 10, 1 << 8), n=33, o=None), "LA3DM_GAIN_MAX_WORDS"),
                     (dict(dims=(1 << 10, 1 << 10, 1 << 8), n=32, o_p=None), "origins3 is NULL"),
                     (dict(o_p=None), "origins3 is NULL"), (dict(f_p=None), "offsets3 is NULL"),
                     (dict(o=None), "gain must not be NULL"), (dict(o=C.byref(_lib.GainOut(None, sent["started"].ctypes.data, None, None))), "gain must not be NULL")):
        rc, txt = c_call(**kw)
        assert rc < 0 and text in txt, (kw, txt)
    assert all((sent[k] == 7).all() for k in G.FIELDS)
    rc, txt = c_call(n=0, o_p=None, o=None)                                      # n = 0: served, nothing is written or read
    assert rc == 0, txt
    assert all((sent[k] == 7).all() for k in G.FIELDS)
    rc, txt = c_call()
    assert rc == 0 and (sent["gain"][:7] <= 64).all() and (sent["gain"][7:] == 7).all() and (sent["seen"][14:] == 7).all(), txt


def test_c_view_and_header(built):
    """CPU test 4: the headers declare and the libraries export the new symbols; the C view through ctypes, optional outputs
    NULL"""
    import la3dm_amd
    from la3dm_amd import _lib
    for header, so, names in (("la3dm_map.h", _lib.MAP_SO, ("la3dm_map_gain",)),
                              ("la3dm_hip.h", _lib.HIP_SO, ("la3dm_devmap_gain_host", "la3dm_devmap_gain_device"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        if so == _lib.MAP_SO:
            C.CDLL(_lib.HIP_SO, mode=C.RTLD_GLOBAL)
        lib = C.CDLL(so)
        for n in names:
            assert re.search(r"\b" + n + r"\s*\(", txt), n
            assert hasattr(lib, n), n
            assert n in _lib.HIP_SYMBOLS + _lib.MAP_SYMBOLS, n
    hip_h = open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
    assert "la3dm_gain_out" in hip_h
    for name in ("CELLS", "RAYS", "WORDS"):
        assert re.search(r"#define\s+LA3DM_GAIN_MAX_" + name + r"\s+\(1u << 28\)", hip_h)
        assert getattr(la3dm_amd, "GAIN_MAX_" + name) == 1 << 28
    m, lv, lo, y, origins = _recipe(3)
    f = G.fan(96, 3.0)
    want = G.yardstick(m, lv, lo, R.RECIPE_DIMS, origins, f, 0xC, 0x2, 4096, cls=y["cls"])
    M = _lib.maplib()
    lo3, d3 = np.ascontiguousarray(lo, np.float32), np.array(R.RECIPE_DIMS, np.uint32)
    info = _lib.RegionInfo()
    gain = np.full(7, 0xAB, np.uint32)
    args = (m._h, lo3.ctypes.data, d3.ctypes.data, origins.ctypes.data, 7, f.ctypes.data, 96, 0xC, 0x2, 4096)
    assert M.la3dm_map_gain(*args, C.byref(_lib.GainOut(gain.ctypes.data, None, None, None)), C.byref(info)) == 0
    assert (gain == want["gain"]).all()
    assert info.block_key == y["block_key"] and list(info.cell) == y["cell"].tolist()
    got = {k: np.full(want[k].shape, 0xAB, np.uint32) for k in G.FIELDS}
    assert M.la3dm_map_gain(*args, C.byref(_lib.GainOut(*[got[k].ctypes.data for k in G.FIELDS])), None) == 0
    G.assert_same(got, want, "C view")
