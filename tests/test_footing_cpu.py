"""footing on a host-mode map (device = -1, no GPU): where a ground robot can stand, as an ordered list and per column,
against an independent numpy yardstick written from the contract comment (tests/helpers/footing_cases.py) over the classes
of region_cases.yardstick.  Everything is integer arithmetic on classes: every comparison is exact."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import frontier_cases as FR  # noqa: E402
import footing_cases as F  # noqa: E402

_SCENE = {}


def _scene():
    if not _SCENE:
        import la3dm_amd
        params = dict(R.YAML, block_depth=4)
        m = la3dm_amd.BGKOctoMap(**params, device=-1).unpack(F.scene_stream(params))
        _SCENE.update(m=m, lv=m.leaves(), padded={})
    return _SCENE["m"], _SCENE["lv"]


def _scene_padded(h, r, s):
    """the classes of the scene's padded box, from the walk of the leaf list"""
    m, lv = _scene()
    if (h, r, s) not in _SCENE["padded"]:
        _SCENE["padded"][(h, r, s)] = F.padded_case(m, lv, F.SCENE_LO, F.SCENE_DIMS, h, r, s)[1]
    return _SCENE["padded"][(h, r, s)]


def _q(m, lo, dims, support, clear, h, r, s, c=None, **kw):
    return m.footing(lo, dims, support=support, clear=clear, headroom=h, radius=r, step=s, min_support=c, **kw)


def _supports(r):
    N = len(F.disc(r))
    return sorted({0, N // 2, N})


def test_scene_against_the_yardstick(built):
    """CPU test 1: the hand-built scene is what the issue lists; over the parameter grid, c = 0, N / 2 and N, the host form
    == the yardstick on n, the list, the columns and the stats; the recorded counts"""
    m, lv = _scene()
    box = m.box(F.SCENE_LO, F.SCENE_DIMS, fields=())
    assert box["cell"].tolist() == [0, 0, 0] and (box["cls"] == F.scene_classes()).all()
    for clear, h, r, s in F.SCENE_GRID:
        p = _scene_padded(h, r, s)
        assert (p == F.scene_padded(h, r, s)).all()                  # MISSING outside the 18 blocks
        for c in _supports(r):
            got = _q(m, F.SCENE_LO, F.SCENE_DIMS, F.OCC_M, clear, h, r, s, c, fields=F.FIELDS)
            assert set(got) == {"n"} | set(F.FIELDS) | set(F.STATS) | set(R.INFO_FIELDS)
            assert got["index"].dtype == np.uint32 and got["levels"].dtype == np.uint32 and got["lowest"].dtype == np.int32
            F.assert_same(got, F.yardstick(p, F.SCENE_DIMS, F.OCC_M, clear, h, r, s, c), ("scene", clear, h, r, s, c))
    for clear, h, r, s, stand, body, foots in F.SCENE_COUNTS:
        for c, n in (foots or {0: None}).items():
            y = F.yardstick(_scene_padded(h, r, s), F.SCENE_DIMS, F.OCC_M, clear, h, r, s, c)
            print(f"scene clear {clear:#x} h {h} r {r} s {s} c {c}: stand {y['n_stand']} body {y['n_body']} foot {y['n']}")
            assert (stand is None or y["n_stand"] == stand) and (body is None or y["n_body"] == body) and (n is None or y["n"] == n)
            F.assert_same(_q(m, F.SCENE_LO, F.SCENE_DIMS, F.OCC_M, clear, h, r, s, c, fields=F.FIELDS), y, "recorded")
    y = F.yardstick(_scene_padded(2, 0, 0), F.SCENE_DIMS, F.OCC_M, F.FREE_M, 2, 0, 0)
    assert int((y["levels"] == 2).sum()) == 16                       # 16 columns hold two levels: floor and table top
    assert m.mirror_syncs() == 0


def test_scene_named_voxels(built):
    """CPU test 2: the direct assertions of the issue on named voxels, taken from the yardstick, and the host form agrees"""
    m, lv = _scene()
    D, occ, free = F.SCENE_DIMS, F.OCC_M, F.FREE_M

    def both(clear, h, r, s, c=None):
        y = F.yardstick(_scene_padded(h, r, s), D, occ, clear, h, r, s, c)
        F.assert_same(_q(m, F.SCENE_LO, D, occ, clear, h, r, s, c, fields=F.FIELDS), y, ("named", clear, h, r, s, c))
        return y
    # under the table (k = 2 .. 4 free, the table at k = 5): stands at h = 3, not at h = 4
    assert both(free, 3, 0, 0)["stand"][3, 3, 2] and not both(free, 4, 0, 0)["stand"][3, 3, 2]
    # the table top is a second level of its column
    y = both(free, 2, 0, 0)
    assert y["foot"][3, 3, 2] and y["foot"][3, 3, 6] and y["levels"][3, 3] == 2 and y["lowest"][3, 3] == 2 and y["highest"][3, 3] == 6
    # no voxel over the hole stands
    assert not y["stand"][2:5, 14:17, :].any() and y["stand"][5, 14, 2]
    # with r = 2 no voxel within 2 of the pillar is a foot voxel, the floor's least of all, and none at all with a
    # footprint that must be carried (c = N / 2, N); with c = 0 the one exception is the pillar's own top, (9, 9, 11):
    # it has the pillar below it and nothing round it, which is all that c = 0 asks for
    near_pillar = [(9 + di, 9 + dj) for di, dj in F.disc(2) + [(0, 0)]]
    for c in (12, 6, 0):
        y = both(free, 4, 2, 1, c)
        on_top = np.zeros(D, bool)
        on_top[9, 9, 11] = c == 0
        assert all((y["foot"][i, j, :] == on_top[i, j, :]).all() for i, j in near_pillar), c
        assert y["foot"][9, 12, 2] and y["stand"][8, 9, 2] and not y["foot"][8, 9, 2]
    # beside the kerb (i = 11, the kerb from i = 12): a foot voxel at r = 1, c = N with s = 1, not with s = 0
    assert both(free, 4, 1, 1)["foot"][11, 12, 2] and not both(free, 4, 1, 0)["foot"][11, 12, 2]
    assert both(free, 4, 1, 0)["stand"][11, 12, 2]
    # beside the two-voxel step (i = 17 on the kerb, the step from i = 18) needs s = 2
    assert both(free, 4, 1, 2)["foot"][17, 4, 3] and not both(free, 4, 1, 1)["foot"][17, 4, 3]
    # a floor voxel under the missing block (k = 8 .. 15 MISSING over i, j >= 16) stands at h = 8 only when MISSING is clear
    assert both(F.OPTIMISTIC, 8, 0, 0)["stand"][17, 20, 3] and not both(free, 8, 0, 0)["stand"][17, 20, 3]
    assert both(free, 5, 0, 0)["stand"][17, 20, 3]


@pytest.mark.parametrize("depth", [3, 4])
def test_recipe_against_the_yardstick(built, depth):
    """CPU test 3: region_cases.fused_map over the recipe region (80, 80, 40): host form == yardstick, the input conditions
    counted from the yardstick first (at depth 3: the issue's figures)"""
    m, lv, lo = R.fused_map(depth)
    dims = R.RECIPE_DIMS
    cache = {}

    def pcls_of(h, r, s):
        if (h, r, s) not in cache:
            cache[(h, r, s)] = F.padded_case(m, lv, lo, dims, h, r, s)
        return cache[(h, r, s)][1]
    cond = F.input_conditions(pcls_of, dims)
    F.assert_exercises_the_feature(cond)
    q = F.RECIPE
    info = m.box(lo, (1, 1, 1), fields=())
    for support, clear, h, r, s in ((q["support"], q["clear"], q["h"], q["r"], q["s"]), (F.OCC_M, F.FREE_M, 2, 0, 0),
                                    (F.OCC_M | F.UNK_M, F.FREE_M | F.MISS_M, 3, 1, 2), (F.OCC_M, F.OPTIMISTIC, 6, 4, 1)):
        for c in _supports(r):
            got = _q(m, lo, dims, support, clear, h, r, s, c, fields=F.FIELDS)
            F.assert_same(got, F.yardstick(pcls_of(h, r, s), dims, support, clear, h, r, s, c), (depth, support, clear, h, r, s, c))
            assert got["block_key"] == info["block_key"] and (got["cell"] == info["cell"]).all() and (got["origin"] == info["origin"]).all()
    # names select the same masks; the defaults are OCCUPIED below, FREE above, h = 2, a point robot
    dflt = m.footing(lo, dims)
    assert set(dflt) == {"n", "index"} | set(F.STATS) | set(R.INFO_FIELDS)
    F.assert_same(dflt, F.yardstick(pcls_of(2, 0, 0), dims, F.OCC_M, F.FREE_M, 2, 0, 0), "defaults")
    names = m.footing(lo, dims, support="occupied", clear=("free", "unknown", "missing"), headroom=4, radius=2, step=1, fields=F.FIELDS)
    F.assert_same(names, F.yardstick(pcls_of(4, 2, 1), dims, F.OCC_M, F.OPTIMISTIC, 4, 2, 1), "names, min_support=None is N")
    assert m.mirror_syncs() == 0


def test_region_independence(built):
    """CPU test 4: footing of a sub-box == the restriction of footing of the enclosing box, for a sub-box touching each face,
    list and columns re-indexed"""
    m, lv, lo = R.fused_map(3)
    dims = R.RECIPE_DIMS
    res = m.get_resolution()
    h, r, s, c = 4, 2, 1, 6
    whole = _q(m, lo, dims, F.OCC_M, F.OPTIMISTIC, h, r, s, c, fields=F.FIELDS)
    foot = np.zeros(int(np.prod(dims)), bool)
    foot[whole["index"]] = True
    big = dict(foot=foot.reshape(dims))
    seen = 0
    for ax in range(3):
        for side in (0, 1):
            sub = [50, 50, 30]
            off = [15, 15, 5]
            off[ax] = 0 if side == 0 else dims[ax] - sub[ax]
            want = F.restrict(big, dims, off, sub)
            sub_lo = (whole["origin"] + np.array(off, np.float32) * np.float32(res)).astype(np.float32)
            got = _q(m, sub_lo, sub, F.OCC_M, F.OPTIMISTIC, h, r, s, c, fields=F.FIELDS)
            assert got["n"] == want["n"], (ax, side)
            R.assert_same(got, want, F.FIELDS, ("sub-box", ax, side))
            seen += want["n"]
    assert seen > 500


def test_shapes(built):
    """CPU test 5: single voxels and lines, nz = 1, columns that end with a word or a wave of the bit streams and columns
    that straddle them, lines of 3000 voxels — at an anchor that is on no block corner"""
    m, lv, lo = R.fused_map(3)
    res = m.get_resolution()
    y0 = R.yardstick(m, lv, lo, R.RECIPE_DIMS)
    stand = F.yardstick(F.padded_case(m, lv, lo, R.RECIPE_DIMS, 2, 0, 0)[1], R.RECIPE_DIMS, F.OCC_M, F.FREE_M, 2, 0, 0)["stand"]
    found = 0
    for shape in FR.SHAPES + FR.WORD_SHAPES + FR.LONG_SHAPES:
        anchor = (y0["origin"] + np.array(F.shape_offset(stand, shape), np.float32) * np.float32(res)).astype(np.float32)
        assert any(v != 0 for v in R.yardstick(m, lv, anchor, (1, 1, 1))["cell"]), shape     # on no block corner
        for h, r, s in F.SHAPE_PARAMS:
            slo, p = F.padded_case(m, lv, anchor, shape, h, r, s)
            for clear in (F.FREE_M, F.OPTIMISTIC):
                for c in _supports(r):
                    got = _q(m, slo, shape, F.OCC_M, clear, h, r, s, c, fields=F.FIELDS)
                    assert got["levels"].shape == shape[:2]
                    F.assert_same(got, F.yardstick(p, shape, F.OCC_M, clear, h, r, s, c), (shape, clear, h, r, s, c))
                    found += got["n"]
    print(f"shapes: {found} foot voxels in all")
    assert found > 100


def test_cap_and_fields(built):
    """CPU test 6: count only; cap < n gives the prefix and n stays the total; cap = n; cap > n leaves the entries from n on
    alone; the dense arrays do not depend on cap; every subset of fields"""
    from la3dm_amd import _lib
    m, lv, lo = R.fused_map(3)
    dims = R.RECIPE_DIMS
    p = F.padded_case(m, lv, lo, dims, 4, 2, 1)[1]
    want = F.yardstick(p, dims, F.OCC_M, F.OPTIMISTIC, 4, 2, 1, 6)
    n = want["n"]
    assert n > 200
    kw = dict(support=F.OCC_M, clear=F.OPTIMISTIC, headroom=4, radius=2, step=1, min_support=6)
    for cap in (0, 1, 7, n - 1, n, n + 100):
        got = m.footing(lo, dims, cap=cap, fields=F.FIELDS, **kw)
        assert got["n"] == n and got["index"].size == min(cap, n) and (got["index"] == want["index"][:cap]).all()
        F.assert_same(got, want, ("cap", cap), F.FIELDS[1:])
    for mask in range(16):
        fields = tuple(k for b, k in enumerate(F.FIELDS) if (mask >> b) & 1)
        got = m.footing(lo, dims, fields=fields, **kw)
        assert set(got) == {"n"} | set(fields) | set(F.STATS) | set(R.INFO_FIELDS)
        F.assert_same(got, want, ("fields", fields), fields)
    M = _lib.maplib()
    lo3, d3 = np.ascontiguousarray(lo, np.float32), np.array(dims, np.uint32)
    par = _lib.FootingParams(F.OCC_M, F.OPTIMISTIC, 4, 2, 1, 6)
    found, stats = C.c_uint64(0), _lib.FootingStats()
    call = lambda cap, out, st=None: M.la3dm_map_footing(m._h, lo3.ctypes.data, d3.ctypes.data, C.byref(par), cap, out, C.byref(found), st, None)  # noqa: E731
    index = np.full(n + 50, 0xDEADBEEF, np.uint32)
    assert call(n + 50, C.byref(_lib.FootingOut(index.ctypes.data, None, None, None)), C.byref(stats)) == 0 and found.value == n
    assert (index[:n] == want["index"]).all() and (index[n:] == 0xDEADBEEF).all()      # entries at t >= n keep the sentinel
    assert stats.as_dict() == {k: want[k] for k in F.STATS}
    found.value = 0
    assert call(0, None) == 0 and found.value == n                                      # count only: out NULL
    levels = np.full(dims[:2], 0xCDCDCDCD, np.uint32)
    found.value = 0
    assert call(0, C.byref(_lib.FootingOut(None, levels.ctypes.data, None, None))) == 0 and found.value == n   # only a dense array
    assert (levels == want["levels"]).all()


def test_refusals_in_the_contracts_order(built):
    """CPU test 7: every refusal with its argument in the text, each one tried with every LATER defect present as well, so the
    order is the contract's; the output buffers untouched; the limit values themselves are served"""
    from la3dm_amd import _lib
    import la3dm_amd
    m, lv, lo = R.fused_map(3)
    M = _lib.maplib()
    lo3 = np.ascontiguousarray(lo, np.float32)
    found = C.c_uint64(77)
    bufs = dict(index=np.full(64, 7, np.uint32), levels=np.full(64, 7, np.uint32), lowest=np.full(64, 7, np.int32), highest=np.full(64, 7, np.int32))
    out = _lib.FootingOut(*[bufs[k].ctypes.data for k in F.FIELDS])
    no_index = _lib.FootingOut(None, out.levels, out.lowest, out.highest)
    P = _lib.FootingParams
    bad_lo = np.array((np.nan, 0, 0), np.float32)
    over = ((1 << 10) - 4, (1 << 10) - 4, (1 << 8) - 5)             # padded by (4, 4, 6): one z layer over 2^28
    # the defects, in the contract's order: (what to change, the text of its refusal)
    defects = [
        (dict(p=None), "params is NULL"),
        (dict(support=0x20), "support_mask must hold"),
        (dict(clear=0), "clear_mask must hold"),
        (dict(support=0x3, clear=0x5), "must not overlap"),
        (dict(h=33), "headroom must lie in"),
        (dict(r=9), "radius must not exceed"),
        (dict(s=5), "step must not exceed"),
        (dict(c=13), "min_support must not exceed"),
        (dict(o=no_index), "index must not be NULL with cap > 0"),
        (dict(lo_p=bad_lo.ctypes.data), "lo must be finite"),
        (dict(dims=over), "LA3DM_FOOTING_MAX_CELLS"),
        (dict(nf=None), "n_found is NULL"),
    ]

    def c_call(p="build", support=F.OCC_M, clear=F.FREE_M | F.MISS_M, h=4, r=2, s=1, c=6, cap=64, o=out, lo_p=lo3.ctypes.data, dims=(4, 4, 4),
               nf=C.byref(found)):
        par = P(support, clear, h, r, s, c) if p == "build" else None
        d3 = np.array(dims, np.uint32)
        rc = M.la3dm_map_footing(m._h, lo_p, d3.ctypes.data, C.byref(par) if par is not None else None, cap, C.byref(o) if o is not None else None,
                                 nf, None, None)
        return rc, M.la3dm_map_last_error().decode()
    for at, (kw, text) in enumerate(defects):
        later = {}
        for kw2, _ in defects[at + 1:]:
            if not (set(kw2) & (set(kw) | set(later))) and "p" not in kw2:
                later.update(kw2)
        rc, txt = c_call(**kw, **later)
        assert rc < 0 and text in txt, (kw, later, txt)
    for kw, text in ((dict(h=0), "headroom"), (dict(s=4, h=4), "step"), (dict(s=2, h=2), "step"), (dict(support=0), "support_mask"),
                     (dict(clear=0x40), "clear_mask"), (dict(r=0, c=1), "min_support"), (dict(r=8, c=197), "min_support"), (dict(o=None), "index must not be NULL"),
                     (dict(dims=(4, 0, 4)), "dims must be >= 1"), (dict(lo_p=None), "lo is NULL"),
                     (dict(dims=(0xFFFFFFFF,) * 3), "LA3DM_FOOTING_MAX_CELLS"), (dict(dims=(1 << 16, 1 << 16, 1)), "LA3DM_FOOTING_MAX_CELLS")):
        rc, txt = c_call(**kw)
        assert rc < 0 and text in txt, (kw, txt)
    # the padded box exactly at the limit passes the size check: the next check answers, and nothing of 2^28 cells is allocated
    rc, txt = c_call(dims=((1 << 10) - 4, (1 << 10) - 4, (1 << 8) - 6), cap=0, o=None, nf=None)
    assert rc < 0 and "n_found is NULL" in txt, txt
    assert found.value == 77 and all((b == 7).all() for b in bufs.values())
    rc, txt = c_call()
    assert rc == 0 and found.value <= 64, txt
    # through Python: the same texts as exceptions; the block-field range of the padded box
    q = m.footing
    with pytest.raises(RuntimeError, match="must not overlap"):
        q(lo, (2, 2, 2), support=("occupied", "unknown"), clear=("free", "unknown"))
    with pytest.raises(RuntimeError, match="step must not exceed"):
        q(lo, (2, 2, 2), headroom=2, step=2)
    with pytest.raises(ValueError, match="unknown fields"):
        q(lo, (2, 2, 2), fields=("index", "cls"))
    with pytest.raises(ValueError):
        q(lo, (2, 2))
    low = (-209715.5, 0.0, 0.0)                                      # block field 0, cell 0: box serves it
    b = m.box(low, (1, 1, 1), fields=())
    assert b["block_key"] >> 40 == 0 and b["cell"][0] == 0
    assert q(low, (2, 2, 2), radius=0)["n"] == 0                      # no pad in x: served
    with pytest.raises(RuntimeError, match="padded box leave"):
        q(low, (2, 2, 2), radius=1)
    # the limit values are accepted: h = 32, r = 8, s = 4, c = N = 196
    assert la3dm_amd.footprint_cells(8) == 196 and [la3dm_amd.footprint_cells(r) for r in range(4)] == [0, 4, 12, 28]
    assert (la3dm_amd.FOOTING_MAX_HEADROOM, la3dm_amd.FOOTING_MAX_RADIUS, la3dm_amd.FOOTING_MAX_STEP, la3dm_amd.FOOTING_MAX_CELLS) == (32, 8, 4, 1 << 28)
    dims = (30, 30, 12)
    for c in (0, 98, 196):
        slo, p = F.padded_case(m, lv, lo, dims, 32, 8, 4)
        got = q(slo, dims, support=F.OCC_M, clear=F.OPTIMISTIC, headroom=32, radius=8, step=4, min_support=c, fields=F.FIELDS)
        F.assert_same(got, F.yardstick(p, dims, F.OCC_M, F.OPTIMISTIC, 32, 8, 4, c), ("limits", c))
        assert got["disc_cells"] == 196


def test_empty_map_and_all_four_classes(built):
    """CPU test 8: the empty map answers n = 0, levels = 0, lowest = highest = -1; GP, BGK-L and BGK-LV maps loaded from
    the scene's stream give the BGK map's answer, and on the BGK-LV map UNCERTAIN works as a mask bit"""
    import la3dm_amd
    m, lv = _scene()
    lo = R.recipe_lo()
    empty = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
    e = empty.footing(lo, (6, 5, 4), support=("occupied", "missing"), clear=("free", "unknown"), radius=1, min_support=0, fields=F.FIELDS)
    assert e["n"] == 0 and e["index"].size == 0 and (e["levels"] == 0).all() and (e["lowest"] == -1).all() and (e["highest"] == -1).all()
    assert (e["n_stand"], e["n_body"], e["n_foot"], e["disc_cells"]) == (0, 0, 0, 4)
    assert e["levels"].shape == (6, 5) and e["levels"].dtype == np.uint32 and e["lowest"].dtype == np.int32
    R.assert_same(e, empty.box(lo, (6, 5, 4)), ("origin", "cell"))
    assert empty.mirror_syncs() == 0
    h, r, s = 4, 2, 1
    for name, yaml in (("GPOctoMap", la3dm_amd.GP_YAML), ("BGKLOctoMap", la3dm_amd.L_YAML), ("BGKLVOctoMap", la3dm_amd.LV_YAML)):
        params = dict(yaml, block_depth=4, resolution=0.1)
        # on the BGK-LV map the scene's UNKNOWN cells (the layer under the floor, the hole) are UNCERTAIN
        swap = {R.UNKNOWN: R.UNCERTAIN} if name == "BGKLVOctoMap" else None
        mv = getattr(la3dm_amd, name)(**params, device=-1).unpack(F.scene_stream(params, name, swap))
        cls = mv.box(F.SCENE_LO, F.SCENE_DIMS, fields=())["cls"]
        want_cls = F.scene_classes()
        if swap:
            want_cls[want_cls == R.UNKNOWN] = R.UNCERTAIN
        assert (cls == want_cls).all(), name
        p = F.scene_padded(h, r, s)
        if swap:
            p[p == R.UNKNOWN] = R.UNCERTAIN
        masks = [(F.OCC_M, F.FREE_M), (F.OCC_M, F.OPTIMISTIC)]
        if swap:
            masks += [(F.OCC_M | F.UNC_M, F.FREE_M), (F.OCC_M, F.FREE_M | F.UNC_M | F.MISS_M)]
        for support, clear in masks:
            for c in (0, 6, 12):
                got = _q(mv, F.SCENE_LO, F.SCENE_DIMS, support, clear, h, r, s, c, fields=F.FIELDS)
                F.assert_same(got, F.yardstick(p, F.SCENE_DIMS, support, clear, h, r, s, c), (name, support, clear, c))
        if swap:   # the hole's UNCERTAIN cells carry when the bit is in the support mask
            over_hole = F.yardstick(F.scene_padded(2, 0, 0) + 0, F.SCENE_DIMS, F.OCC_M, F.FREE_M, 2, 0, 0)["stand"][2:5, 14:17, 2]
            p2 = F.scene_padded(2, 0, 0)
            p2[p2 == R.UNKNOWN] = R.UNCERTAIN
            assert not over_hole.any() and F.yardstick(p2, F.SCENE_DIMS, F.OCC_M | F.UNC_M, F.FREE_M, 2, 0, 0)["stand"][2:5, 14:17, 2].all()
            F.assert_same(_q(mv, F.SCENE_LO, F.SCENE_DIMS, F.OCC_M | F.UNC_M, F.FREE_M, 2, 0, 0, fields=F.FIELDS),
                          F.yardstick(p2, F.SCENE_DIMS, F.OCC_M | F.UNC_M, F.FREE_M, 2, 0, 0), "uncertain carries")


def test_abi_python_signature_and_example(built):
    """CPU test 9: the headers declare and the libraries export the new symbols; the Python signature row of the issue; the
    example program (built by build()) runs on a host-mode map — without a GPU that map cannot insert a scan, so it stays
    empty"""
    import la3dm_amd
    from la3dm_amd import _lib
    for header, so, names in (("la3dm_map.h", _lib.MAP_SO, ("la3dm_map_footing",)),
                              ("la3dm_hip.h", _lib.HIP_SO, ("la3dm_devmap_footing_host", "la3dm_devmap_footing_device"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        if so == _lib.MAP_SO:
            C.CDLL(_lib.HIP_SO, mode=C.RTLD_GLOBAL)
        lib = C.CDLL(so)
        for n in names:
            assert re.search(r"\b" + n + r"\s*\(", txt), n
            assert hasattr(lib, n), n
            assert n in _lib.HIP_SYMBOLS + _lib.MAP_SYMBOLS, n
    assert _lib.HIP_API["la3dm_devmap_footing_host"] == _lib.HIP_API["la3dm_devmap_footing_device"] == _lib.MAP_API["la3dm_map_footing"]
    hip_h = open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
    for name, value in (("MAX_CELLS", r"\(1u << 28\)"), ("MAX_HEADROOM", "32"), ("MAX_RADIUS", "8"), ("MAX_STEP", "4")):
        assert re.search(r"#define\s+LA3DM_FOOTING_" + name + r"\s+" + value, hip_h), name
    assert all(t in hip_h for t in ("la3dm_footing_params", "la3dm_footing_out", "la3dm_footing_stats"))
    assert C.sizeof(_lib.FootingParams) == 24 and C.sizeof(_lib.FootingStats) == 16 and C.sizeof(_lib.FootingOut) == 32
    sig = inspect.signature(la3dm_amd.BGKOctoMap.footing)
    assert str(sig) == ("(self, lo, dims, support=('occupied',), clear=('free',), headroom=2, radius=0, step=0, min_support=None, "
                        "fields=('index',), cap=None)")
    for cls in (la3dm_amd.GPOctoMap, la3dm_amd.BGKLOctoMap, la3dm_amd.BGKLVOctoMap):
        assert cls.footing is la3dm_amd.BGKOctoMap.footing
    exe = os.path.join(ROOT, "examples", "ground_goals")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "0"] +
                       "0.1 3 1.0 0.2 0.5 0.1 8.0 0.3 0.7 100.0 0.001 0.001 -1".split(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 4 and [ln.split(":")[0] for ln in lines[:3]] == ["support 12 of 12", "support 6 of 12", "support 0 of 12"], r.stdout
    assert all(ln.endswith("stand 0 body 0 foot 0 patches 0 patch none goals 0 on any patch 0") for ln in lines[:3]), r.stdout
    assert lines[3].startswith("ground_goals 128 x 128 x 32 from ") and lines[3].endswith("frontier 0 mirror_syncs 0 device_resident 0"), r.stdout
