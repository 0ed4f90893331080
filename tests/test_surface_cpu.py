"""surface on a host-mode map (device = -1, no GPU): the exposed faces of the solid voxels of a region and the integer
normals summed from them, against an independent numpy yardstick written from the contract comment
(tests/helpers/surface_cases.py) over the classes of region_cases.yardstick.  Everything is integer arithmetic on classes:
every comparison is exact."""
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
import surface_cases as S  # noqa: E402

_SCENE = {}
OPTIMISTIC = S.FREE_M | S.UNK_M | S.MISS_M


def _scene():
    if not _SCENE:
        import la3dm_amd
        params = dict(R.YAML, block_depth=4)
        m = la3dm_amd.BGKOctoMap(**params, device=-1).unpack(F.scene_stream(params))
        _SCENE.update(m=m, lv=m.leaves(), padded={})
    return _SCENE["m"], _SCENE["lv"]


def _scene_padded(s):
    """the classes of the scene's padded box, from the walk of the leaf list"""
    m, lv = _scene()
    if s not in _SCENE["padded"]:
        _SCENE["padded"][s] = S.padded_case(m, lv, S.SCENE_LO, S.SCENE_DIMS, s)[1]
    return _SCENE["padded"][s]


def _yard(solid, open_, s):
    return S.yardstick(_scene_padded(s), S.SCENE_DIMS, solid, open_, s)


def test_scene_against_the_yardstick(built):
    """CPU test 1: the hand-built scene is what the issue lists; every mask pair of its table at smooth 0 to 4: the host form
    == the yardstick on n, the list, the dense faces and the stats; the table's constants and named voxels"""
    m, lv = _scene()
    box = m.box(S.SCENE_LO, S.SCENE_DIMS, fields=())
    assert box["cell"].tolist() == [0, 0, 0] and (box["cls"] == F.scene_classes()).all()
    for s in S.SMOOTHS:
        assert (_scene_padded(s) == S.scene_padded(s)).all()                  # MISSING outside the 18 blocks
        S.assert_exercises_the_feature(S.exercises_the_feature(_scene_padded(s), S.SCENE_DIMS, S.OCC_M, OPTIMISTIC, s), ("scene", s))
        for solid, open_ in [row[:2] for row in S.SCENE_TABLE]:
            got = m.surface(S.SCENE_LO, S.SCENE_DIMS, solid=solid, open=open_, smooth=s, fields=S.FIELDS)
            assert set(got) == {"n"} | set(S.FIELDS) | set(S.STATS) | set(R.INFO_FIELDS)
            assert got["normal"].shape == (got["n"], 3) and got["dense_faces"].shape == S.SCENE_DIMS
            S.assert_same(got, _yard(solid, open_, s), ("scene", solid, open_, s))
    S.assert_scene_table(_yard)
    S.assert_scene_voxels(_yard)
    assert m.mirror_syncs() == 0


def test_scene_on_a_bgklv_map_with_uncertain(built):
    """CPU test 2: the BGK-LV scene has UNCERTAIN where the BGK scene has UNKNOWN; the bit works in either mask, and the
    third row of the table comes back with UNCERTAIN in solid"""
    import la3dm_amd
    params = dict(la3dm_amd.LV_YAML, block_depth=4, resolution=0.1)
    swap = {R.UNKNOWN: R.UNCERTAIN}
    mv = la3dm_amd.BGKLVOctoMap(**params, device=-1).unpack(F.scene_stream(params, "BGKLVOctoMap", swap))
    want_cls = F.scene_classes()
    want_cls[want_cls == R.UNKNOWN] = R.UNCERTAIN
    assert (mv.box(S.SCENE_LO, S.SCENE_DIMS, fields=())["cls"] == want_cls).all()
    for s in (0, 2, 4):
        p = S.scene_padded(s, swap)
        for solid, open_ in ((S.OCC_M, S.FREE_M), (S.OCC_M | S.UNC_M, S.FREE_M), (S.OCC_M, S.FREE_M | S.UNC_M | S.MISS_M), (S.OCC_M, S.UNC_M | S.MISS_M),
                             (S.OCC_M | S.UNK_M, S.FREE_M)):
            got = mv.surface(S.SCENE_LO, S.SCENE_DIMS, solid=solid, open=open_, smooth=s, fields=S.FIELDS)
            S.assert_same(got, S.yardstick(p, S.SCENE_DIMS, solid, open_, s), ("lv scene", solid, open_, s))
    got = mv.surface(S.SCENE_LO, S.SCENE_DIMS, solid=("occupied", "uncertain"), open="free", fields=())
    assert (got["n"], got["n_solid"], got["face_count"]) == (624, 1753, (85, 13, 13, 13, 16, 592))
    assert mv.surface(S.SCENE_LO, S.SCENE_DIMS, solid=S.OCC_M | S.UNK_M, open=S.FREE_M, fields=())["n"] == 615   # no UNKNOWN on this map


@pytest.mark.parametrize("depth", [3, 4])
def test_recipe_against_the_yardstick_and_frontier(built, depth):
    """CPU test 3: region_cases.fused_map over the recipe region (80, 80, 40) at smooth 0, 2 and 4: host form == yardstick,
    the input conditions counted from the yardstick first; at any smooth the list is frontier's with the roles swapped, and
    popcount(faces) its nbrs"""
    m, lv, lo = R.fused_map(depth)
    dims = R.RECIPE_DIMS
    info = m.box(lo, (1, 1, 1), fields=())
    for s in (0, 2, 4):
        origin, p = S.padded_case(m, lv, lo, dims, s)
        S.assert_exercises_the_feature(S.exercises_the_feature(p, dims, S.OCC_M, OPTIMISTIC, s), ("recipe", depth, s))
        pairs = ((S.OCC_M, S.FREE_M), (S.OCC_M, OPTIMISTIC)) + (((S.OCC_M | S.UNK_M, S.FREE_M | S.MISS_M),) if s == 0 else ())
        for solid, open_ in pairs:
            got = m.surface(lo, dims, solid=solid, open=open_, smooth=s, fields=S.FIELDS)
            S.assert_same(got, S.yardstick(p, dims, solid, open_, s), (depth, solid, open_, s))
            assert got["block_key"] == info["block_key"] and (got["cell"] == info["cell"]).all() and (got["origin"] == info["origin"]).all()
            fr = m.frontier(lo, dims, open=solid, unknown=open_, connectivity=6, min_neighbours=1, fields=("index", "nbrs"))
            assert fr["n"] == got["n"] and (fr["index"] == got["index"]).all()
            assert (np.unpackbits(got["faces"][:, None], axis=1).sum(1).astype(np.uint8) == fr["nbrs"]).all()
    # names select the same masks; the defaults are OCCUPIED against FREE, smooth 0, the three list fields
    dflt = m.surface(lo, dims)
    assert set(dflt) == {"n"} | set(S.LIST_FIELDS) | set(S.STATS) | set(R.INFO_FIELDS)
    S.assert_same(dflt, S.yardstick(S.padded_case(m, lv, lo, dims, 0)[1], dims, S.OCC_M, S.FREE_M, 0), "defaults")
    names = m.surface(lo, dims, solid="occupied", open=("free", "unknown", "missing"), smooth=2, fields=S.FIELDS)
    S.assert_same(names, S.yardstick(S.padded_case(m, lv, lo, dims, 2)[1], dims, S.OCC_M, OPTIMISTIC, 2), "names")
    assert m.mirror_syncs() == 0


def test_closed_forms(built):
    """CPU test 4: far from every edge an infinite floor gives (0, 0, (2s + 1)^2) and a wall (-(2s + 1)^2, 0, 0): the windowed
    sum of face vectors is the area vector of the patch"""
    import la3dm_amd
    params = dict(R.YAML, block_depth=4)
    for classes, (off, dims), axis, sign in ((S.floor_classes(), S.FLOOR_SUB, 2, 1), (S.wall_classes(), S.WALL_SUB, 0, -1)):
        m = la3dm_amd.BGKOctoMap(**params, device=-1).unpack(S.stream_of(classes, params))
        b = m.box(S.SCENE_LO, S.SCENE_DIMS, fields=())
        assert (b["cls"] == classes).all()
        lo = (b["origin"] + np.array(off, np.float32) * np.float32(m.get_resolution())).astype(np.float32)
        for s in S.SMOOTHS:
            got = m.surface(lo, dims, smooth=s)
            want = np.zeros((int(np.prod(dims)), 3), np.int16)
            want[:, axis] = sign * (2 * s + 1) ** 2
            assert got["n"] == int(np.prod(dims)) and got["normal"].dtype == np.int16 and (got["normal"] == want).all(), (axis, s, got["normal"][:3])
            assert (got["faces"] == (1 << (2 * axis + (sign > 0)))).all()


def test_region_independence(built):
    """CPU test 5: surface of a sub-box == the restriction of surface of the enclosing box, for a sub-box touching each face:
    the halo is read from the map, so the answer for a voxel does not depend on where the region's faces are"""
    m, lv, lo = R.fused_map(3)
    dims = R.RECIPE_DIMS
    res = m.get_resolution()
    seen = 0
    for s, open_ in ((0, S.FREE_M), (2, OPTIMISTIC), (4, S.FREE_M)):
        whole = m.surface(lo, dims, open=open_, smooth=s, fields=S.FIELDS)
        big = dict(dense_faces=whole["dense_faces"], dense_normal=S.dense_normal_of(whole, dims))
        for ax in range(3):
            for side in (0, 1):
                sub = [50, 50, 30]
                off = [15, 15, 5]
                off[ax] = 0 if side == 0 else dims[ax] - sub[ax]
                want = S.restrict(big, off, sub)
                sub_lo = (whole["origin"] + np.array(off, np.float32) * np.float32(res)).astype(np.float32)
                got = m.surface(sub_lo, sub, open=open_, smooth=s, fields=S.FIELDS)
                assert got["n"] == want["n"], (s, ax, side)
                R.assert_same(got, want, S.FIELDS, ("sub-box", s, ax, side))
                seen += want["n"]
    assert seen > 5000
    # and from the yardstick's side: a sub-box of the scene, its classes cut from the scene's padded box
    ms, _ = _scene()
    for s in (1, 3):
        big_cls = _scene_padded(4)
        origin = (np.array(S.SCENE_LO, np.float32) - np.float32(5) * np.float32(0.1)).astype(np.float32)   # the centre of the padded box's voxel (0, 0, 0)
        sub_lo, p = S.sub_case(big_cls, origin, (5 + 8, 5 + 4, 5 + 0), (10, 12, 12), s, 0.1)
        got = ms.surface(sub_lo, (10, 12, 12), smooth=s, fields=S.FIELDS)
        S.assert_same(got, S.yardstick(p, (10, 12, 12), S.OCC_M, S.FREE_M, s), ("scene sub-box", s))
        assert got["n"] > 50


def test_shapes(built):
    """CPU test 6: single voxels and lines, nz = 1, columns whose padded length ends with a word or a wave of the bit streams
    or straddles them (PZ = 31 .. 33 and 63 .. 65 at smooth 0 and 1), lines of 3000 voxels — placed where the two-scan map
    has surface"""
    m, lv, lo = R.fused_map(3)
    res = m.get_resolution()
    y0 = R.yardstick(m, lv, lo, R.RECIPE_DIMS)
    dense = S.yardstick(S.padded_case(m, lv, lo, R.RECIPE_DIMS, 0)[1], R.RECIPE_DIMS, S.OCC_M, OPTIMISTIC, 0)["dense_faces"]
    found = 0
    cases = [(shape, s) for shape in FR.SHAPES + FR.WORD_SHAPES + FR.LONG_SHAPES for s in (0, 1, 4)]
    cases += [(shape, s) for s in (0, 1) for shape in S.pz_shapes(s)]
    assert [sh[2] for sh in S.pz_shapes(0)] == [29, 30, 31, 61, 62, 63] and [sh[2] for sh in S.pz_shapes(1)] == [27, 28, 29, 59, 60, 61]
    for shape, s in cases:
        anchor = (y0["origin"] + np.array(S.shape_offset(dense, shape), np.float32) * np.float32(res)).astype(np.float32)
        slo, p = S.padded_case(m, lv, anchor, shape, s)
        for open_ in (S.FREE_M, OPTIMISTIC):
            got = m.surface(slo, shape, open=open_, smooth=s, fields=S.FIELDS)
            assert got["dense_faces"].shape == tuple(shape)
            S.assert_same(got, S.yardstick(p, shape, S.OCC_M, open_, s), (shape, open_, s))
            if open_ == OPTIMISTIC:
                assert got["n"] > 0, (shape, s)                       # placed where there is surface
            found += got["n"]
    print(f"shapes: {found} surface voxels in all")
    assert found > 300


def test_cap_and_fields(built):
    """CPU test 7: count only; cap < n gives the prefix — the normals of the capped prefix are the uncapped ones — and n
    stays the total; cap = n; cap > n leaves the entries from n on alone; the dense array does not depend on cap; every
    subset of fields that the contract serves"""
    from la3dm_amd import _lib
    m, lv, lo = R.fused_map(3)
    dims = R.RECIPE_DIMS
    s = 2
    want = S.yardstick(S.padded_case(m, lv, lo, dims, s)[1], dims, S.OCC_M, OPTIMISTIC, s)
    n = want["n"]
    assert n > 1000
    kw = dict(solid=S.OCC_M, open=OPTIMISTIC, smooth=s)
    for cap in (0, 1, n - 1, n, n + 1):
        got = m.surface(lo, dims, cap=cap, fields=S.FIELDS, **kw)
        assert got["n"] == n and all(got[k].shape[0] == min(cap, n) for k in S.LIST_FIELDS)
        assert all((got[k] == want[k][:cap]).all() for k in S.LIST_FIELDS)
        S.assert_same(got, want, ("cap", cap), ("dense_faces",))
    for mask in range(16):
        fields = tuple(k for b, k in enumerate(S.FIELDS) if (mask >> b) & 1)
        if "normal" in fields and "index" not in fields:
            with pytest.raises(RuntimeError, match="normal is set without"):
                m.surface(lo, dims, fields=fields, **kw)
            continue
        got = m.surface(lo, dims, fields=fields, **kw)
        assert set(got) == {"n"} | set(fields) | set(S.STATS) | set(R.INFO_FIELDS)
        S.assert_same(got, want, ("fields", fields), fields)
    got = m.surface(lo, dims, fields=("dense_faces",), cap=5, **kw)      # an integer cap with no list field counts
    S.assert_same(got, want, "cap without a list", ("dense_faces",))
    M = _lib.maplib()
    lo3, d3 = np.ascontiguousarray(lo, np.float32), np.array(dims, np.uint32)
    par = _lib.SurfaceParams(S.OCC_M, OPTIMISTIC, s)
    found, stats = C.c_uint64(0), _lib.SurfaceStats()
    call = lambda cap, out, st=None: M.la3dm_map_surface(m._h, lo3.ctypes.data, d3.ctypes.data, C.byref(par), cap, out, C.byref(found), st, None)  # noqa: E731
    index, faces, normal = np.full(n + 50, 0xDEADBEEF, np.uint32), np.full(n + 50, 0xEE, np.uint8), np.full((n + 50, 3), 0x7EEE, np.int16)
    assert call(n + 50, C.byref(_lib.SurfaceOut(index.ctypes.data, faces.ctypes.data, normal.ctypes.data, None)), C.byref(stats)) == 0 and found.value == n
    assert (index[:n] == want["index"]).all() and (index[n:] == 0xDEADBEEF).all()      # entries at t >= n keep the sentinel
    assert (faces[:n] == want["faces"]).all() and (faces[n:] == 0xEE).all() and (normal[:n] == want["normal"]).all() and (normal[n:] == 0x7EEE).all()
    assert stats.as_dict() == {k: want[k] for k in S.STATS}
    faces[:] = 0xEE
    assert call(7, C.byref(_lib.SurfaceOut(None, faces.ctypes.data, None, None))) == 0 and found.value == n      # faces alone
    assert (faces[:7] == want["faces"][:7]).all() and (faces[7:] == 0xEE).all()
    found.value = 0
    assert call(0, None) == 0 and found.value == n                                      # count only: out NULL
    dense = np.full(dims, 0xCD, np.uint8)
    found.value = 0
    assert call(0, C.byref(_lib.SurfaceOut(None, None, None, dense.ctypes.data))) == 0 and found.value == n   # only the dense array
    assert (dense == want["dense_faces"]).all()
    found.value = 0
    index[:] = 0xDEADBEEF
    assert call(0, C.byref(_lib.SurfaceOut(index.ctypes.data, None, None, None))) == 0 and found.value == n and (index == 0xDEADBEEF).all()


def test_refusals_in_the_contracts_order(built):
    """CPU test 8: every refusal with its argument in the text, each one tried with every LATER defect present as well, so the
    order is the contract's; the output buffers untouched and the map unchanged; the limit values themselves are served"""
    from la3dm_amd import _lib
    import la3dm_amd
    m, lv, lo = R.fused_map(3)
    before = m.pack()
    M = _lib.maplib()
    lo3 = np.ascontiguousarray(lo, np.float32)
    found = C.c_uint64(77)
    bufs = dict(index=np.full(64, 7, np.uint32), faces=np.full(64, 7, np.uint8), normal=np.full((64, 3), 7, np.int16), dense_faces=np.full(64, 7, np.uint8))
    out = _lib.SurfaceOut(*[bufs[k].ctypes.data for k in S.FIELDS])
    no_index = _lib.SurfaceOut(None, out.faces, out.normal, out.dense_faces)
    no_list = _lib.SurfaceOut(None, None, None, out.dense_faces)
    P = _lib.SurfaceParams
    bad_lo = np.array((np.nan, 0, 0), np.float32)
    over = ((1 << 10) - 6, (1 << 10) - 6, (1 << 8) - 5)             # smooth 2 pads by 6: one z layer over 2^28
    defects = [
        (dict(p=None), "params is NULL"),
        (dict(solid=0x20), "solid_mask must hold"),
        (dict(open_=0), "open_mask must hold"),
        (dict(solid=0x3, open_=0x5), "must not overlap"),
        (dict(s=5), "smooth must not exceed"),
        (dict(o=no_index), "normal is set without"),
        (dict(lo_p=bad_lo.ctypes.data), "lo must be finite"),
        (dict(dims=over), "LA3DM_SURFACE_MAX_CELLS"),
        (dict(nf=None), "n_found is NULL"),
    ]

    def c_call(p="build", solid=S.OCC_M, open_=S.FREE_M | S.MISS_M, s=2, cap=64, o=out, lo_p=lo3.ctypes.data, dims=(4, 4, 4), nf=C.byref(found)):
        par = P(solid, open_, s) if p == "build" else None
        d3 = np.array(dims, np.uint32)
        rc = M.la3dm_map_surface(m._h, lo_p, d3.ctypes.data, C.byref(par) if par is not None else None, cap, C.byref(o) if o is not None else None,
                                 nf, None, None)
        return rc, M.la3dm_map_last_error().decode()
    for at, (kw, text) in enumerate(defects):
        later = {}
        for kw2, _ in defects[at + 1:]:
            if not (set(kw2) & (set(kw) | set(later))) and "p" not in kw2:
                later.update(kw2)
        rc, txt = c_call(**kw, **later)
        assert rc < 0 and text in txt, (kw, later, txt)
    for kw, text in ((dict(solid=0), "solid_mask"), (dict(open_=0x40), "open_mask"), (dict(s=0xFFFFFFFF), "smooth"), (dict(o=None), "must not be NULL with cap > 0"),
                     (dict(o=no_list), "must not be NULL with cap > 0"), (dict(dims=(4, 0, 4)), "dims must be >= 1"), (dict(lo_p=None), "lo is NULL"),
                     (dict(dims=(0xFFFFFFFF,) * 3), "LA3DM_SURFACE_MAX_CELLS"), (dict(dims=(1 << 16, 1 << 16, 1)), "LA3DM_SURFACE_MAX_CELLS")):
        rc, txt = c_call(**kw)
        assert rc < 0 and text in txt, (kw, txt)
    # the padded box exactly at the limit passes the size check: the next check answers, and nothing of 2^28 cells is allocated
    rc, txt = c_call(dims=((1 << 10) - 6, (1 << 10) - 6, (1 << 8) - 6), cap=0, o=None, nf=None)
    assert rc < 0 and "n_found is NULL" in txt, txt
    assert found.value == 77 and all((b == 7).all() for b in bufs.values())
    rc, txt = c_call(dims=(4, 4, 4))
    assert rc == 0 and found.value <= 64, txt
    # through Python: the same texts as exceptions; the block-field range of the padded box
    q = m.surface
    with pytest.raises(RuntimeError, match="must not overlap"):
        q(lo, (2, 2, 2), solid=("occupied", "unknown"), open=("free", "unknown"))
    with pytest.raises(RuntimeError, match="smooth must not exceed"):
        q(lo, (2, 2, 2), smooth=5)
    with pytest.raises(ValueError, match="unknown fields"):
        q(lo, (2, 2, 2), fields=("index", "cls"))
    with pytest.raises(ValueError):
        q(lo, (2, 2))
    with pytest.raises(RuntimeError, match="padded box leave"):
        q((-209715.5, 0.0, 0.0), (2, 2, 2))                          # block field 0, cell 0: no room for the pad below
    assert (la3dm_amd.SURFACE_MAX_SMOOTH, la3dm_amd.SURFACE_MAX_CELLS) == (4, 1 << 28)
    assert (m.pack() == before).all() and m.mirror_syncs() == 0


def test_surface_quads(built):
    """CPU test 9: the quads of the scene's sub-box i, j in 1 .. 10, k in 3 .. 11, solid OCCUPIED, open FREE — the table and
    eight pillar voxels, no solid voxel at its x or y ends.  The plane coordinates of the +x quads minus those of the -x
    quads count the solid voxels (24), the same along y; every quad has four distinct corners in its plane, counter-clockwise
    seen from the open side"""
    import la3dm_amd
    m, lv = _scene()
    off, dims = (1, 1, 3), (10, 10, 9)
    lo = (np.array(S.SCENE_LO, np.float32) + np.array(off, np.float32) * np.float32(0.1)).astype(np.float32)      # the centre of cell `off`
    g = m.surface(lo, dims, fields=("index", "faces"))
    assert (m.box(lo, dims, fields=())["cls"] == F.scene_classes()[1:11, 1:11, 3:12]).all()
    assert g["n_solid"] == 24
    corners, direction, voxel = la3dm_amd.surface_quads(g["index"], g["faces"], dims)
    F_ = int(np.unpackbits(g["faces"]).sum())
    assert corners.shape == (F_, 4, 3) and corners.dtype == np.int32 and direction.dtype == np.uint8 and voxel.dtype == np.uint32
    assert sum(g["face_count"]) == F_
    # list order, then ascending d
    order = [(int(v), d) for v, f in zip(g["index"], g["faces"]) for d in range(6) if (f >> d) & 1]
    assert order == list(zip(voxel.tolist(), direction.tolist()))
    for axis in (0, 1):
        plane = corners[:, 0, axis].astype(np.int64)
        pos, neg = direction == 2 * axis + 1, direction == 2 * axis
        assert int(plane[pos].sum() - plane[neg].sum()) == 24, axis
    vox = np.stack([voxel // (dims[1] * dims[2]), voxel // dims[2] % dims[1], voxel % dims[2]], 1).astype(np.int64)
    for t in range(F_):
        a, positive = int(direction[t]) >> 1, int(direction[t]) & 1
        c = corners[t].astype(np.int64)
        assert (c[:, a] == vox[t, a] + positive).all()                               # coplanar in its axis, at the right plane
        assert len({tuple(r) for r in c.tolist()}) == 4                             # four distinct corners
        assert ((c >= vox[t]) & (c <= vox[t] + 1)).all()                            # corners of the voxel
        cross = np.cross(c[1] - c[0], c[2] - c[1])
        want = np.zeros(3, np.int64)
        want[a] = 1 if positive else -1
        assert (cross == want).all(), (t, cross, want)                               # counter-clockwise seen from the open side
    empty = la3dm_amd.surface_quads(np.zeros(0, np.uint32), np.zeros(0, np.uint8), dims)
    assert empty[0].shape == (0, 4, 3) and empty[1].shape == (0,) and empty[2].shape == (0,)
    with pytest.raises(ValueError):
        la3dm_amd.surface_quads(np.array([10 * 10 * 9], np.uint32), np.array([1], np.uint8), dims)


def test_empty_map_and_the_other_classes(built):
    """CPU test 10: the empty map answers n = 0 and dense_faces = 0; GP and BGK-L maps loaded from the scene's stream give the
    BGK map's answer"""
    import la3dm_amd
    lo = R.recipe_lo()
    empty = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
    e = empty.surface(lo, (6, 5, 4), solid=("occupied", "missing"), open=("free", "unknown"), smooth=3, fields=S.FIELDS)
    assert e["n"] == 0 and e["index"].size == 0 and e["normal"].shape == (0, 3) and (e["dense_faces"] == 0).all() and e["dense_faces"].shape == (6, 5, 4)
    assert (e["n_solid"], e["n_surface"], e["face_count"]) == (6 * 5 * 4, 0, (0,) * 6)
    R.assert_same(e, empty.box(lo, (6, 5, 4)), ("origin", "cell"))
    for name, yaml in (("GPOctoMap", la3dm_amd.GP_YAML), ("BGKLOctoMap", la3dm_amd.L_YAML)):
        params = dict(yaml, block_depth=4, resolution=0.1)
        mv = getattr(la3dm_amd, name)(**params, device=-1).unpack(F.scene_stream(params, name))
        for s in (0, 3):
            for solid, open_ in ((S.OCC_M, S.FREE_M), (S.OCC_M, OPTIMISTIC)):
                got = mv.surface(S.SCENE_LO, S.SCENE_DIMS, solid=solid, open=open_, smooth=s, fields=S.FIELDS)
                S.assert_same(got, S.yardstick(S.scene_padded(s), S.SCENE_DIMS, solid, open_, s), (name, solid, open_, s))


def test_abi_python_signature_and_example(built):
    """CPU test 11: the headers declare and the libraries export the new symbols; the Python signature row of the issue; the
    example program (built by build()) runs on a host-mode map — without a GPU that map cannot insert a scan, so it stays
    empty"""
    import la3dm_amd
    from la3dm_amd import _lib
    for header, so, names in (("la3dm_map.h", _lib.MAP_SO, ("la3dm_map_surface",)),
                              ("la3dm_hip.h", _lib.HIP_SO, ("la3dm_devmap_surface_host", "la3dm_devmap_surface_device"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        if so == _lib.MAP_SO:
            C.CDLL(_lib.HIP_SO, mode=C.RTLD_GLOBAL)
        lib = C.CDLL(so)
        for n in names:
            assert re.search(r"\b" + n + r"\s*\(", txt), n
            assert hasattr(lib, n), n
            assert n in _lib.HIP_SYMBOLS + _lib.MAP_SYMBOLS, n
    assert _lib.HIP_API["la3dm_devmap_surface_host"] == _lib.HIP_API["la3dm_devmap_surface_device"] == _lib.MAP_API["la3dm_map_surface"]
    hip_h = open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
    for name, value in (("MAX_CELLS", r"\(1u << 28\)"), ("MAX_SMOOTH", "4")):
        assert re.search(r"#define\s+LA3DM_SURFACE_" + name + r"\s+" + value, hip_h), name
    assert all(t in hip_h for t in ("la3dm_surface_params", "la3dm_surface_out", "la3dm_surface_stats"))
    assert C.sizeof(_lib.SurfaceParams) == 12 and C.sizeof(_lib.SurfaceStats) == 64 and C.sizeof(_lib.SurfaceOut) == 32
    sig = inspect.signature(la3dm_amd.BGKOctoMap.surface)
    assert str(sig) == "(self, lo, dims, solid=('occupied',), open=('free',), smooth=0, fields=('index', 'faces', 'normal'), cap=None)"
    for cls in (la3dm_amd.GPOctoMap, la3dm_amd.BGKLOctoMap, la3dm_amd.BGKLVOctoMap):
        assert cls.surface is la3dm_amd.BGKOctoMap.surface
    exe = os.path.join(ROOT, "examples", "surface_mesh")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "0"] +
                       "0.1 3 1.0 0.2 0.5 0.1 8.0 0.3 0.7 100.0 0.001 0.001 -1".split(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 10 and lines[0].startswith("surface_mesh 128 x 128 x 32 from ") and "surface voxels 0 solid 0 " in lines[0], r.stdout
    assert lines[0].endswith("quads 0 ply none") and lines[1].startswith("start ") and all(ln.startswith(f"iter {k} ") for k, ln in enumerate(lines[2:9])), r.stdout
    assert lines[-1].startswith("surface_mesh done: ") and lines[-1].endswith("mirror_syncs 0 device_resident 0"), r.stdout
