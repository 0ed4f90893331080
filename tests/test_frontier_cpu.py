"""frontier on a host-mode map (device = -1, no GPU): the free voxels that border unexplored space, as an ordered list,
against an independent numpy stencil (tests/helpers/frontier_cases.py) over the classes of region_cases.yardstick.
Everything is integer arithmetic on classes: every comparison is exact."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import frontier_cases as F  # noqa: E402

ALL = ("index", "nbrs", "score")


def _recipe(depth):
    m, lv, lo = R.fused_map(depth)
    y = R.yardstick(m, lv, lo, R.RECIPE_DIMS)
    ilo, pcls, dims = F.interior(y, m.get_resolution())
    return m, lv, y, ilo, pcls, dims


@pytest.mark.parametrize("depth", [3, 4])
def test_recipe_against_the_yardstick(built, depth):
    """CPU test 1: the interior box of the recipe region, every connectivity, four mask pairs, min_neighbours 1, 3 and
    connectivity: n, index, nbrs and score; the input conditions are counted from the yardstick first"""
    m, lv, y, ilo, pcls, dims = _recipe(depth)
    assert dims == (78, 78, 38)
    F.assert_exercises_the_feature(F.input_conditions(pcls))
    want_info = F.advanced_info(y, depth)
    for c in F.CONNECTIVITIES:
        for open_mask, unknown_mask in F.MASK_PAIRS:
            score = F.score_of(pcls, open_mask, unknown_mask, c)
            for mn in (1, 3, c):
                got = m.frontier(ilo, dims, open=open_mask, unknown=unknown_mask, connectivity=c, min_neighbours=mn, fields=ALL)
                assert set(got) == {"n", "index", "nbrs", "score"} | set(R.INFO_FIELDS)
                assert got["index"].dtype == np.uint32 and got["nbrs"].dtype == np.uint8 and got["score"].dtype == np.uint8
                F.assert_same(got, F.answer_of(score, mn), (depth, c, open_mask, unknown_mask, mn))
                assert got["block_key"] == want_info["block_key"] and (got["cell"] == want_info["cell"]).all()
    # the anchor is the yardstick's, advanced by one voxel
    res = np.float32(m.get_resolution())
    assert np.allclose(got["origin"], y["origin"] + res, atol=1e-5)
    # names select the same masks; the defaults are the planner's pair at connectivity 6
    names = m.frontier(ilo, dims, open=("free",), unknown=("unknown", "missing"), connectivity=26, fields=ALL)
    F.assert_same(names, F.yardstick(pcls, F.FREE_M, F.UNK_M | F.MISS_M, 26, 1), "names")
    dflt = m.frontier(ilo, dims)
    assert set(dflt) == {"n", "index", "nbrs"} | set(R.INFO_FIELDS)
    F.assert_same(dflt, F.yardstick(pcls, F.FREE_M, F.UNK_M | F.MISS_M, 6, 1), "defaults")
    F.assert_same(m.frontier(ilo, dims, open="free", unknown="unknown", fields="score"), F.yardstick(pcls, F.FREE_M, F.UNK_M, 6, 1), "strings")
    assert m.mirror_syncs() == 0


@pytest.mark.parametrize("depth", [3, 4])
def test_algebra_of_the_definition(built, depth):
    """CPU test 2, exact: two halves of the box merge into the whole (only because of the look past the faces); the list at
    min_neighbours = m is score >= m, each a subset of the one before; score 6 <= score 18 <= score 26; the scores of disjoint
    unknown masks add up; nbrs == score[index]; index strictly ascending"""
    m, lv, y, ilo, pcls, dims = _recipe(depth)
    res = np.float32(m.get_resolution())
    o_m, u_m = F.FREE_M, F.UNK_M | F.MISS_M
    for c in F.CONNECTIVITIES:
        whole = m.frontier(ilo, dims, open=o_m, unknown=u_m, connectivity=c, fields=ALL)
        assert whole["n"] == whole["index"].size > 1000
        assert (np.diff(whole["index"].astype(np.int64)) > 0).all()
        assert (whole["nbrs"] == whole["score"].reshape(-1)[whole["index"]]).all()
        for ax in range(3):
            cut = dims[ax] // 2 + 1
            d0, d1 = list(dims), list(dims)
            d0[ax], d1[ax] = cut, dims[ax] - cut
            step = np.zeros(3, np.float32)
            step[ax] = cut
            a = m.frontier(ilo, d0, open=o_m, unknown=u_m, connectivity=c, fields=ALL)
            b = m.frontier((ilo + step * res).astype(np.float32), d1, open=o_m, unknown=u_m, connectivity=c, fields=ALL)
            assert (np.concatenate([a["score"], b["score"]], ax) == whole["score"]).all(), (c, ax)
            ia = np.ravel_multi_index(np.unravel_index(a["index"], d0), dims)
            sub = list(np.unravel_index(b["index"], d1))
            sub[ax] = sub[ax] + cut
            ib = np.ravel_multi_index(sub, dims)
            merged = np.concatenate([ia, ib])
            order = np.argsort(merged, kind="stable")
            assert a["n"] + b["n"] == whole["n"] and (merged[order] == whole["index"]).all(), (c, ax)
            assert (np.concatenate([a["nbrs"], b["nbrs"]])[order] == whole["nbrs"]).all(), (c, ax)
        before = whole["index"]
        for mn in range(2, c + 1):
            g = m.frontier(ilo, dims, open=o_m, unknown=u_m, connectivity=c, min_neighbours=mn)
            assert (g["index"] == np.flatnonzero(whole["score"].reshape(-1) >= mn)).all(), (c, mn)
            assert np.isin(g["index"], before).all() and g["n"] <= before.size
            before = g["index"]
    s = {c: m.frontier(ilo, dims, open=o_m, unknown=u_m, connectivity=c, fields="score")["score"] for c in F.CONNECTIVITIES}
    assert (s[6] <= s[18]).all() and (s[18] <= s[26]).all() and (s[6] < s[26]).any()
    for u1, u2 in ((F.UNK_M, F.MISS_M), (F.FREE_M, F.OCC_M | F.UNK_M), (F.OCC_M, F.MISS_M)):
        parts = [m.frontier(ilo, dims, open=0xF, unknown=u, connectivity=26, fields="score")["score"] for u in (u1, u2, u1 | u2)]
        assert (parts[0] + parts[1] == parts[2]).all() and parts[0].any() and parts[1].any(), (u1, u2)
    every = m.frontier(ilo, dims, open=0xF, unknown=0xF, connectivity=26, min_neighbours=26, fields=ALL)
    assert every["n"] == int(np.prod(dims)) and (every["score"] == 26).all()     # every voxel has one of the four classes


def test_shapes(built):
    """CPU test 3: single voxels and lines, nz = 1, the word and wave boundaries of the voxel count, lines of 3000 voxels
    across the map — each anchored inside a larger yardstick region, so every neighbour's class is known"""
    m, lv, y, ilo, pcls, dims = _recipe(3)
    res = m.get_resolution()
    found = 0
    for shape in F.SHAPES + F.WORD_SHAPES:
        off = F.SHAPE_OFFSET if shape[2] <= 24 else F.SHAPE_OFFSET[:2] + (-10,)     # (the taller ones start below the map)
        lo, p, _ = F.padded_case(m, lv, (y["origin"] + np.array(off, np.float32) * np.float32(res)).astype(np.float32), shape)
        for c in F.CONNECTIVITIES:
            for open_mask, unknown_mask in F.MASK_PAIRS:
                for mn in (1, 3):
                    got = m.frontier(lo, shape, open=open_mask, unknown=unknown_mask, connectivity=c, min_neighbours=mn, fields=ALL)
                    assert got["score"].shape == shape
                    F.assert_same(got, F.yardstick(p, open_mask, unknown_mask, c, mn), (shape, c, open_mask, unknown_mask, mn))
                    found += got["n"]
    print(f"small shapes: {found} frontier voxels in all")
    assert found > 500
    seen = {}
    for shape in F.LONG_SHAPES:
        lo, p, info = F.padded_case(m, lv, F.long_line_lo(y, res, shape), shape)
        for c in F.CONNECTIVITIES:
            for open_mask, unknown_mask in F.MASK_PAIRS[:2] + ((F.MISS_M, F.FREE_M | F.UNK_M),):
                want = F.yardstick(p, open_mask, unknown_mask, c, 1)
                got = m.frontier(lo, shape, open=open_mask, unknown=unknown_mask, connectivity=c, fields=ALL)
                F.assert_same(got, want, (shape, c, open_mask, unknown_mask))
                assert got["block_key"] == info["block_key"] and (got["cell"] == info["cell"]).all()
                print(f"{shape} connectivity {c} masks {open_mask:#x} {unknown_mask:#x}: {want['n']} frontier voxels")
                seen[shape] = seen.get(shape, 0) + want["n"]
    assert len(seen) == len(F.LONG_SHAPES) and min(seen.values()) > 0, seen      # each line holds frontier voxels of some kind


def test_cap(built):
    """CPU test 4: cap < n gives the prefix and n stays the total; cap > n leaves the entries from n on alone; the
    count-only call, with and without score"""
    from la3dm_amd import _lib
    m, lv, y, ilo, pcls, dims = _recipe(3)
    want = F.yardstick(pcls, F.FREE_M, F.UNK_M | F.MISS_M, 18, 2)
    n = want["n"]
    assert n > 1000
    for cap in (1, 7, n - 1, n):
        got = m.frontier(ilo, dims, connectivity=18, min_neighbours=2, cap=cap)
        assert got["n"] == n and got["index"].size == cap
        assert (got["index"] == want["index"][:cap]).all() and (got["nbrs"] == want["nbrs"][:cap]).all()
    got = m.frontier(ilo, dims, connectivity=18, min_neighbours=2, cap=n + 100, fields=ALL)
    F.assert_same(got, want, "cap > n")
    got = m.frontier(ilo, dims, connectivity=18, min_neighbours=2, cap=0, fields=("score",))
    assert got["n"] == n and got["index"].size == 0 and (got["score"] == want["score"]).all()
    M = _lib.maplib()
    lo3, d3 = np.ascontiguousarray(ilo, np.float32), np.array(dims, np.uint32)
    found = C.c_uint64(0)
    call = lambda cap, out: M.la3dm_map_frontier(m._h, lo3.ctypes.data, d3.ctypes.data, F.FREE_M, F.UNK_M | F.MISS_M, 18, 2, cap,  # noqa: E731
                                                 out, C.byref(found), None)
    index, nbrs = np.full(n + 50, 0xDEADBEEF, np.uint32), np.full(n + 50, 0xAB, np.uint8)
    assert call(n + 50, C.byref(_lib.FrontierOut(index.ctypes.data, nbrs.ctypes.data, None))) == 0 and found.value == n
    assert (index[:n] == want["index"]).all() and (nbrs[:n] == want["nbrs"]).all()
    assert (index[n:] == 0xDEADBEEF).all() and (nbrs[n:] == 0xAB).all()            # entries at t >= n keep the sentinel
    index[:] = 0xDEADBEEF
    found.value = 0
    assert call(10, C.byref(_lib.FrontierOut(index.ctypes.data, None, None))) == 0 and found.value == n     # index alone
    assert (index[:10] == want["index"][:10]).all() and (index[10:] == 0xDEADBEEF).all()
    found.value = 0
    assert call(0, None) == 0 and found.value == n                                  # count only: out NULL
    score = np.full(dims, 0xCD, np.uint8)
    found.value = 0
    assert call(0, C.byref(_lib.FrontierOut(None, None, score.ctypes.data))) == 0 and found.value == n
    assert (score == want["score"]).all()


def test_refusals(built):
    """CPU test 5: every refused argument with its name in the text; the limit before any buffer is looked at; output
    buffers untouched"""
    from la3dm_amd import _lib
    m, lv, lo = R.fused_map(3)
    q = m.frontier
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
    with pytest.raises(ValueError, match="unknown fields"):
        q(lo, (2, 2, 2), fields=("index", "cls"))
    for mask in (0, 0x20, 0x3F, 1 << 31, ()):
        with pytest.raises(RuntimeError, match="open_mask must hold"):
            q(lo, (2, 2, 2), open=mask)
        with pytest.raises(RuntimeError, match="unknown_mask must hold"):
            q(lo, (2, 2, 2), unknown=mask)
    for c in (0, 4, 8, 27, 1 << 20):
        with pytest.raises(RuntimeError, match="connectivity must be 6, 18 or 26"):
            q(lo, (2, 2, 2), connectivity=c)
    for c, mn in ((6, 0), (6, 7), (18, 19), (26, 27), (26, 1 << 20)):
        with pytest.raises(RuntimeError, match="min_neighbours must lie in"):
            q(lo, (2, 2, 2), connectivity=c, min_neighbours=mn)
    assert q(lo, (2, 2, 2), open=0x1F, unknown=0x1F, connectivity=26, min_neighbours=26)["n"] >= 0   # the limits themselves are served
    # the region padded by one voxel must pass box's range check: box serves these two, frontier refuses them
    low = (-209715.5, 0.0, 0.0)
    b = m.box(low, (1, 1, 1), fields=())
    assert b["block_key"] >> 40 == 0 and b["cell"][0] == 0
    high = (2.09e5, 0.0, 0.0)
    b = m.box(high, (1, 1, 1), fields=())
    to_end = ((1 << 20) - int(b["block_key"] >> 40)) * 4 - int(b["cell"][0])
    assert m.box(high, (to_end, 1, 1), fields=())["cls"].shape == (to_end, 1, 1)
    for bad_lo, dims in ((low, (2, 2, 2)), (high, (to_end, 1, 1))):
        with pytest.raises(RuntimeError, match="padded by one voxel"):
            q(bad_lo, dims)
    assert q(high, (to_end - 1, 1, 1))["n"] == 0
    # the voxel limit, on the padded region
    for dims in (((1 << 28) - 1, 1, 1), (1 << 10, 1 << 10, (1 << 8) - 1), (1 << 16, 1 << 16, 1), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)):
        with pytest.raises(RuntimeError, match="LA3DM_FR_MAX_CELLS"):
            q(lo, dims)
    M = _lib.maplib()
    lo3 = np.ascontiguousarray(lo, np.float32)
    found = C.c_uint64(77)
    index, nbrs, score = np.full(64, 7, np.uint32), np.full(64, 7, np.uint8), np.full(64, 7, np.uint8)
    out = _lib.FrontierOut(index.ctypes.data, nbrs.ctypes.data, score.ctypes.data)

    def c_call(dims=(4, 4, 4), open_mask=1, unknown_mask=0xC, c=6, mn=1, cap=64, o=C.byref(out), lo_p=lo3.ctypes.data, with_dims=True,
               n_found=C.byref(found)):
        d3 = np.array(dims, np.uint32)
        rc = M.la3dm_map_frontier(m._h, lo_p, d3.ctypes.data if with_dims else None, open_mask, unknown_mask, c, mn, cap, o, n_found, None)
        return rc, M.la3dm_map_last_error().decode()
    at = ((1 << 10) - 2, (1 << 10) - 2, (1 << 8) - 2)              # padded: exactly 2^28
    for kw, text in ((dict(open_mask=0), "open_mask"), (dict(unknown_mask=0x40), "unknown_mask"), (dict(c=7), "connectivity"),
                     (dict(mn=0), "min_neighbours"), (dict(mn=7), "min_neighbours"), (dict(lo_p=None), "lo is NULL"),
                     (dict(with_dims=False), "dims is NULL"), (dict(dims=(4, 0, 4)), "dims must be >= 1"),
                     (dict(o=None), "index must not be NULL"), (dict(o=C.byref(_lib.FrontierOut(None, nbrs.ctypes.data, None))), "index must not be NULL"),
                     (dict(n_found=None), "n_found is NULL"), (dict(n_found=None, cap=0, o=None), "n_found is NULL"),
                     # the limit comes before any buffer is looked at: over it, the limit answers whatever the buffers are;
                     (dict(dims=at[:2] + (at[2] + 1,), o=None, n_found=None), "LA3DM_FR_MAX_CELLS"),
                     # at it, the region passed and the next check — the buffers — answers; nothing of 2^28 cells is allocated
                     (dict(dims=at, o=None), "index must not be NULL"), (dict(dims=at, cap=0, o=None, n_found=None), "n_found is NULL")):
        rc, txt = c_call(**kw)
        assert rc < 0 and text in txt, (kw, txt)
    assert found.value == 77 and (index == 7).all() and (nbrs == 7).all() and (score == 7).all()
    rc, txt = c_call()
    assert rc == 0 and found.value <= 64, txt


def test_empty_map(built):
    """CPU test 6: every voxel and its surroundings are MISSING — every voxel with score = connectivity if both masks hold
    bit 3, no voxel otherwise"""
    import la3dm_amd
    m, lv, lo = R.fused_map(3)
    empty = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
    dims = (6, 5, 4)
    for c in F.CONNECTIVITIES:
        e = empty.frontier(lo, dims, open=("free", "missing"), unknown=0xC, connectivity=c, min_neighbours=c, fields=ALL)
        assert e["n"] == 120 and (e["index"] == np.arange(120)).all() and (e["nbrs"] == c).all() and (e["score"] == c).all()
        e = empty.frontier(lo, dims, open=("free", "missing"), unknown=0xC, connectivity=c, cap=50)
        assert e["n"] == 120 and (e["index"] == np.arange(50)).all() and (e["nbrs"] == c).all()
        for open_mask, unknown_mask in ((0x7, 0xC), (0x8, 0x7), (0x17, 0x17)):
            e = empty.frontier(lo, dims, open=open_mask, unknown=unknown_mask, connectivity=c, fields=ALL)
            assert e["n"] == 0 and e["index"].size == 0 and e["nbrs"].size == 0 and (e["score"] == 0).all()
    R.assert_same(e, m.box(lo, dims), ("origin", "cell"))
    assert empty.mirror_syncs() == 0


def test_c_view_header_and_example(built):
    """CPU test 7: the headers declare and the libraries export the new symbols; the C view through ctypes; the example
    program (built by build()) runs on a host-mode map — without a GPU that map cannot insert a scan, so it stays empty"""
    import la3dm_amd
    from la3dm_amd import _lib
    for header, so, names in (("la3dm_map.h", _lib.MAP_SO, ("la3dm_map_frontier",)),
                              ("la3dm_hip.h", _lib.HIP_SO, ("la3dm_devmap_frontier_host", "la3dm_devmap_frontier_device"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        if so == _lib.MAP_SO:
            C.CDLL(_lib.HIP_SO, mode=C.RTLD_GLOBAL)
        lib = C.CDLL(so)
        for n in names:
            assert re.search(r"\b" + n + r"\s*\(", txt), n
            assert hasattr(lib, n), n
            assert n in _lib.HIP_SYMBOLS + _lib.MAP_SYMBOLS, n
    hip_h = open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
    assert "la3dm_frontier_out" in hip_h and re.search(r"#define\s+LA3DM_FR_MAX_CELLS\s+\(1u << 28\)", hip_h)
    assert la3dm_amd.FR_MAX_CELLS == 1 << 28
    # the C view on the recipe map: two calls, as a C client makes them
    m, lv, y, ilo, pcls, dims = _recipe(3)
    M = _lib.maplib()
    lo3, d3 = np.ascontiguousarray(ilo, np.float32), np.array(dims, np.uint32)
    found, info = C.c_uint64(0), _lib.RegionInfo()
    assert M.la3dm_map_frontier(m._h, lo3.ctypes.data, d3.ctypes.data, 1, 0xC, 26, 1, 0, None, C.byref(found), C.byref(info)) == 0
    want = F.yardstick(pcls, 1, 0xC, 26, 1)
    assert found.value == want["n"]
    index, nbrs, score = np.zeros(want["n"], np.uint32), np.zeros(want["n"], np.uint8), np.zeros(dims, np.uint8)
    out = _lib.FrontierOut(index.ctypes.data, nbrs.ctypes.data, score.ctypes.data)
    assert M.la3dm_map_frontier(m._h, lo3.ctypes.data, d3.ctypes.data, 1, 0xC, 26, 1, want["n"], C.byref(out), C.byref(found), None) == 0
    assert (index == want["index"]).all() and (nbrs == want["nbrs"]).all() and (score == want["score"]).all()
    wi = F.advanced_info(y, 3)
    assert info.block_key == wi["block_key"] and list(info.cell) == wi["cell"].tolist()
    exe = os.path.join(ROOT, "examples", "frontier")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "0"] +
                       "0.1 3 1.0 0.2 0.5 0.1 8.0 0.3 0.7 100.0 0.001 0.001 -1".split(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("frontier 128 x 128 x 16 from "), r.stdout
    assert lines[0].endswith("found 0 kept 0 mirror_syncs 0 device_resident 0"), r.stdout
