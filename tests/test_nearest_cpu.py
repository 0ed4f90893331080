"""nearest and nearest_points on a host-mode map (device = -1, no GPU): which obstacle voxel is the nearest, per voxel of a
region and per point of a cloud, compared with an independent yardstick (tests/helpers/nearest_cases.py: the brute-force
minimum over the obstacle list in ascending flat index, the first minimum kept; the classes from region_cases.yardstick; the
points' transform and anchor arithmetic from score_cases).  Every output is an integer: every comparison is exact."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import distance_cases as D  # noqa: E402
import nearest_cases as N  # noqa: E402
import region_cases as R  # noqa: E402
import score_cases as S  # noqa: E402

_RECIPES = {}


def _recipe(depth):
    """(map, leaves, recipe lo, the yardstick of the recipe region)"""
    if depth not in _RECIPES:
        m, lv, lo = R.fused_map(depth)
        _RECIPES[depth] = (m, lv, lo, R.yardstick(m, lv, lo, R.RECIPE_DIMS))
    return _RECIPES[depth]


def _at(m, y, offset):
    return (y["origin"] + np.array(offset, np.float32) * np.float32(m.get_resolution())).astype(np.float32)


@pytest.mark.parametrize("depth", [3, 4])
def test_host_form_equals_the_yardstick(built, depth):
    """CPU test 1: distance_cases.SHAPES plus (5, 5, 5), (1, 1, 65), (2, 33, 2) x radii 1, 3, 8, 255 x the four masks on the
    fused recipe map: index and d2 equal the brute force.  Counted from the yardstick: every region with at least two axes
    longer than 1 has voxels with more than one nearest obstacle; NONE occurs at radius 1"""
    m, lv, lo, y = _recipe(depth)
    none_at_1 = 0
    for dims in N.SHAPES:
        offset = N.place(y["cls"], dims)
        rlo = _at(m, y, offset)
        cls = R.yardstick(m, lv, rlo, dims)["cls"]                          # (a line may leave the recipe region)
        if offset != N.SHAPE_OFFSET:
            assert (y["cls"][tuple(slice(o, o + n) for o, n in zip(offset, dims))] == cls).all()   # the region is where place() looked
        cond = N.conditions(cls, N.MASKS[0], 8)
        print(f"depth {depth} dims {dims} at {offset}: {cond}")
        assert cond["tied"] > 0 or sum(n > 1 for n in dims) < 2, (dims, cond)
        none_at_1 += sum(N.conditions(cls, mask, 1)["none"] for mask in N.MASKS)
        for mask in N.MASKS:
            for radius in N.RADII:
                got = m.nearest(rlo, dims, obstacles=mask, radius=radius)
                assert set(got) == set(N.FIELDS) | set(R.INFO_FIELDS)
                assert all(got[k].dtype == np.uint32 and got[k].shape == tuple(dims) for k in N.FIELDS)
                N.assert_same(got, N.yardstick(cls, mask, radius), (depth, dims, mask, radius))
    assert none_at_1 > 0
    # names select the same masks; one field alone; the defaults are OCCUPIED and radius 16; the info is box's
    dims = (5, 5, 5)
    offset = N.place(y["cls"], dims)
    rlo = _at(m, y, offset)
    cls = y["cls"][tuple(slice(o, o + n) for o, n in zip(offset, dims))]
    only = m.nearest(rlo, dims, fields="index")
    assert set(only) == {"index"} | set(R.INFO_FIELDS) and (only["index"] == N.yardstick(cls, 2, 16)["index"]).all()
    only = m.nearest(rlo, dims, fields=("d2",))
    assert set(only) == {"d2"} | set(R.INFO_FIELDS) and (only["d2"] == N.yardstick(cls, 2, 16)["d2"]).all()
    names = m.nearest(rlo, dims, obstacles=("occupied", "unknown", "missing"), radius=3)
    N.assert_same(names, N.yardstick(cls, N.MASKS[2], 3), "names")
    R.assert_same(names, m.box(rlo, dims, fields=()), ("origin", "cell"), "info")
    assert m.mirror_syncs() == 0


def test_hand_built_map(built):
    """CPU test 2: the six face-centre voxels of a 5 x 5 x 5 region OCCUPIED: the centre has six nearest obstacles at d2 = 4
    and answers the smallest flat index, 12 = (0, 2, 2); radius 1 gives NONE there; the whole region equals the brute force"""
    import la3dm_amd
    params = dict(R.YAML, block_depth=4)
    m = la3dm_amd.BGKOctoMap(**params, device=-1).unpack(N.hand_built_stream(params))
    box = m.box(N.HAND_LO, N.HAND_DIMS)
    assert box["cell"].tolist() == [1, 1, 1]
    assert sorted(map(tuple, np.argwhere(box["cls"] == R.OCCUPIED).tolist())) == sorted(N.FACE_CENTRES) and (box["cls"] <= R.OCCUPIED).all()
    cls = np.zeros(N.HAND_DIMS, np.uint8)
    for v in N.FACE_CENTRES:
        cls[v] = R.OCCUPIED
    Dmin, first, count = N.brute(cls, 2)
    assert count.reshape(N.HAND_DIMS)[2, 2, 2] == 6 and Dmin.reshape(N.HAND_DIMS)[2, 2, 2] == 4
    for radius in (1, 2, 3, 255):
        got = m.nearest(N.HAND_LO, N.HAND_DIMS, radius=radius)
        N.assert_same(got, N.yardstick(cls, 2, radius), ("hand built", radius))
        centre = (int(got["index"][2, 2, 2]), int(got["d2"][2, 2, 2]))
        assert centre == ((12, 4) if radius >= 2 else (N.NONE, N.FAR)), (radius, centre)
    for v in N.FACE_CENTRES:                                      # an obstacle answers its own index
        assert got["index"][v] == (v[0] * 5 + v[1]) * 5 + v[2] and got["d2"][v] == 0


@pytest.mark.parametrize("depth", [3, 4])
def test_properties_on_the_recipe_region(built, depth):
    """CPU test 3: on 80 x 80 x 40 (too large for the brute force) d2 equals distance_field's d2 and scipy's EDT, every
    finite index is an obstacle at squared distance d2, an obstacle answers itself; the wide mask leaves no NONE at radius 8;
    on distance_cases.SUB_DIMS, queried as a region of its own, index and d2 equal the brute force"""
    m, lv, lo, y = _recipe(depth)
    dims = R.RECIPE_DIMS
    ijk = np.stack(np.meshgrid(*[np.arange(n) for n in dims], indexing="ij"), -1)
    for mask, radius in ((N.MASKS[0], 8), (N.MASKS[0], 255), (N.MASKS[1], 3), (N.MASKS[2], 8), (N.MASKS[3], 1)):
        got = m.nearest(lo, dims, obstacles=mask, radius=radius)
        df = m.distance_field(lo, dims, obstacles=mask, radius=radius, fields=("d2",))
        assert (got["d2"] == df["d2"]).all(), (mask, radius)
        assert (got["d2"] == D.finish(D.squared_edt(y["cls"], mask), radius, m.get_resolution())["d2"]).all(), (mask, radius)
        obs = D.obstacles_of(y["cls"], mask)
        finite = got["index"] != N.NONE
        assert (finite == (got["d2"] != N.FAR)).all()
        at = np.stack(np.unravel_index(got["index"][finite].astype(np.int64), dims), -1)
        assert obs[at[:, 0], at[:, 1], at[:, 2]].all(), (mask, radius)
        assert (((at - ijk[finite]) ** 2).sum(-1) == got["d2"][finite]).all(), (mask, radius)
        flat = np.arange(obs.size, dtype=np.uint32).reshape(dims)
        assert (got["index"][obs] == flat[obs]).all()
        print(f"depth {depth} mask {mask:#x} radius {radius}: {int(finite.sum())} voxels with an obstacle within the radius, {int(obs.sum())} obstacles")
        if (mask, radius) == (N.MASKS[2], 8):
            assert finite.all()
    sub = tuple(slice(o, o + n) for o, n in zip(D.SUB_OFFSET, D.SUB_DIMS))
    slo = _at(m, y, D.SUB_OFFSET)
    for mask in (N.MASKS[0], N.MASKS[2]):
        Dmin, first, count = N.brute(y["cls"][sub], mask)
        print(f"depth {depth} sub-box mask {mask:#x}: {int((count > 1).sum())} voxels with more than one nearest obstacle")
        assert int((count > 1).sum()) > 100
        for radius in (3, 8, 255):
            want = {k: a.reshape(D.SUB_DIMS) for k, a in N.finish(Dmin, first, radius).items()}
            N.assert_same(m.nearest(slo, D.SUB_DIMS, obstacles=mask, radius=radius), want, ("sub-box", depth, mask, radius))
    assert m.mirror_syncs() == 0


@pytest.mark.parametrize("depth", [3, 4])
def test_nearest_points_against_the_yardstick(built, depth):
    """CPU test 4: score_cases' cloud on the recipe region and the jittered cloud on a small one, with pose = None, the
    identity and a moved pose: cls, voxel, index and d2 equal the yardstick; pose = None equals the identity on the finite
    points; NaN, inf and 1e12 coordinates and a NaN in each pose entry are INVALID; all five classes occur"""
    m, lv, lo, y = _recipe(depth)
    res = m.get_resolution()
    pts, o = S.sensor_cloud()
    T = S.recipe_poses(o)
    world = np.vstack([(pts[:-3] + o).astype(np.float32), pts[-3:]])           # the cloud in the map frame
    classes = np.zeros(5, np.int64)
    small = (3, 5, 7)
    soff = N.place(y["cls"], small)
    slo = _at(m, y, soff)
    _, _, _, so = R.anchor(slo, res, depth)
    jit = N.jittered_cloud(so, small, res, n=257)
    for rlo, dims, cloud, pose in ((lo, R.RECIPE_DIMS, world, None), (lo, R.RECIPE_DIMS, world, S.IDENTITY), (lo, R.RECIPE_DIMS, pts, T[13]),
                                   (lo, R.RECIPE_DIMS, pts, T[5]), (lo, R.RECIPE_DIMS, pts, T[31]), (slo, small, jit, None),
                                   (slo, small, jit, S.IDENTITY), (slo, small, (jit - T[13, :, 3]).astype(np.float32), T[13])):
        for mask, radius in ((N.MASKS[0], 8), (N.MASKS[0], 1), (N.MASKS[2], 1), (N.MASKS[0], 255)):
            want = N.points_yardstick(m, lv, rlo, dims, cloud, pose, mask, radius)
            got = m.nearest_points(rlo, dims, cloud, pose, obstacles=mask, radius=radius)
            assert set(got) == set(N.POINT_FIELDS) | set(R.INFO_FIELDS)
            assert got["cls"].dtype == np.uint8 and all(got[k].dtype == np.uint32 for k in N.POINT_FIELDS[1:])
            N.assert_same(got, want, (depth, dims, mask, radius), N.POINT_FIELDS)
            classes += np.array(N.class_counts(want))
    print(f"depth {depth}: points per class over all cases {classes.tolist()}")
    assert (classes > 0).all(), classes
    # pose = None == the identity on the finite points (the identity's arithmetic adds and multiplies by 0 and 1 only)
    a = m.nearest_points(lo, R.RECIPE_DIMS, world[:-3], None, radius=8)
    b = m.nearest_points(lo, R.RECIPE_DIMS, world[:-3], S.IDENTITY, radius=8)
    N.assert_same(a, b, "None == identity", N.POINT_FIELDS)
    assert m.nearest_points(lo, R.RECIPE_DIMS, world, None)["cls"][-3:].tolist() == [N.INVALID] * 3
    for r in range(3):
        for c in range(4):
            bad = S.IDENTITY.copy()
            bad[r, c] = np.nan
            got = m.nearest_points(slo, small, jit[:16], bad, radius=8)
            assert (got["cls"] == N.INVALID).all() and (got["voxel"] == N.NONE).all() and (got["index"] == N.NONE).all() and (got["d2"] == N.FAR).all()
    # the region's own centres without a pose: voxel = the flat index, index and d2 = nearest's arrays
    dense = m.nearest(slo, small, obstacles=N.MASKS[2], radius=8)
    got = m.nearest_points(slo, small, S.centres(so, small, res), obstacles=N.MASKS[2], radius=8)
    assert (got["voxel"] == np.arange(105)).all() and (got["index"] == dense["index"].reshape(-1)).all() and (got["d2"] == dense["d2"].reshape(-1)).all()
    assert m.mirror_syncs() == 0


def test_arguments(built):
    """CPU test 5: every refusal with its text and its place in the order, nothing written; each output left out; n_points = 0;
    the empty map, both ways"""
    import la3dm_amd
    from la3dm_amd import _lib
    m, lv, lo, y = _recipe(3)
    pts = (S.sensor_cloud()[0][:64] + S.sensor_cloud()[1]).astype(np.float32)
    q = lambda **kw: m.nearest(kw.pop("lo", lo), kw.pop("dims", (4, 4, 4)), **kw)   # noqa: E731
    qp = lambda **kw: m.nearest_points(kw.pop("lo", lo), kw.pop("dims", (4, 4, 4)), kw.pop("points", pts), kw.pop("pose", None), **kw)   # noqa: E731
    for call in (q, qp):
        for mask in (0, 0x20, 0x3F, 1 << 31, ()):
            with pytest.raises(RuntimeError, match="obstacle_mask must hold"):
                call(obstacles=mask)
        for radius in (0, 256, 1024):
            with pytest.raises(RuntimeError, match=r"radius must lie in \[1, LA3DM_NEAREST_MAX_RADIUS \(255\)\]"):
                call(radius=radius)
        for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, 1.1e8)):
            with pytest.raises(RuntimeError, match="lo must be finite"):
                call(lo=bad)
        for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
            with pytest.raises(RuntimeError, match="dims must be >= 1"):
                call(dims=dims)
        with pytest.raises(RuntimeError, match="lo: the block field leaves"):
            call(lo=(-3.0e5, 0, 0))
        for dims in (((1 << 28) + 1, 1, 1), (1 << 10, 1 << 10, (1 << 8) + 1), (0xFFFFFFFF,) * 3):
            with pytest.raises(RuntimeError, match=r"LA3DM_DF_MAX_CELLS \(2\^28\)"):
                call(dims=dims)
        with pytest.raises(ValueError, match="unknown fields"):
            call(fields=("index", "dist"))
        assert call(radius=255, obstacles=0x1F)["d2"].dtype == np.uint32
    with pytest.raises(RuntimeError, match="index or d2 must not be NULL"):
        q(fields=())
    with pytest.raises(RuntimeError, match="cls, voxel, index or d2 must not be NULL"):
        qp(fields=())
    with pytest.raises(ValueError, match=r"\(3, 4\) or \(12,\)"):
        qp(pose=np.zeros((2, 12), np.float32))
    # each output left out: the others are what the full call gives
    full = qp(radius=8)
    for k in N.POINT_FIELDS:
        part = qp(radius=8, fields=[f for f in N.POINT_FIELDS if f != k])
        assert set(part) == (set(N.POINT_FIELDS) - {k}) | set(R.INFO_FIELDS)
        N.assert_same(part, full, ("without", k), N.POINT_FIELDS)
    z = qp(points=np.zeros((0, 3), np.float32))
    assert all(z[k].shape == (0,) for k in N.POINT_FIELDS)
    assert (qp(pose=S.IDENTITY.reshape(12))["index"] == qp(pose=S.IDENTITY)["index"]).all()
    # the limits, the NULL pointers and the order, through the C view: no pointer is followed before the checks have passed
    M = _lib.maplib()
    lo3 = np.ascontiguousarray(lo, np.float32)
    n = pts.shape[0]
    sent = dict(index=np.full(64 + 8, 7, np.uint32), d2=np.full(64 + 8, 7, np.uint32), cls=np.full(n + 8, 7, np.uint8),
                voxel=np.full(n + 8, 7, np.uint32), p_index=np.full(n + 8, 7, np.uint32), p_d2=np.full(n + 8, 7, np.uint32))
    out = _lib.NearestOut(sent["index"].ctypes.data, sent["d2"].ctypes.data)
    pout = _lib.NearestPointsOut(sent["cls"].ctypes.data, sent["voxel"].ctypes.data, sent["p_index"].ctypes.data, sent["p_d2"].ctypes.data)

    def c_call(points, lo_p=lo3.ctypes.data, dims=(4, 4, 4), with_dims=True, p_p=pts.ctypes.data, n=n, mask=0x2, radius=8, o=None):
        d3 = np.array(dims, np.uint32)
        dp = d3.ctypes.data if with_dims else None
        if points:
            rc = M.la3dm_map_nearest_points(m._h, lo_p, dp, p_p, n, None, mask, radius, C.byref(pout) if o is None else o[1], None)
        else:
            rc = M.la3dm_map_nearest(m._h, lo_p, dp, mask, radius, C.byref(out) if o is None else o[0], None)
        return rc, M.la3dm_map_last_error().decode()
    over = dict(dims=((1 << 28) + 1, 1, 1))
    null = (C.byref(_lib.NearestOut(None, None)), C.byref(_lib.NearestPointsOut(None, None, None, None)))
    gone = (None, None)
    shared = ((dict(mask=0), "obstacle_mask"), (dict(mask=0x40), "obstacle_mask"), (dict(radius=0), "radius must lie in"),
              (dict(radius=256), "radius must lie in"), (dict(lo_p=None), "lo is NULL"), (dict(with_dims=False), "dims is NULL"),
              (dict(dims=(4, 0, 4)), "dims must be >= 1"), (dict(over), "LA3DM_DF_MAX_CELLS"),
              # the order: each call breaks the rule named and every later one
              (dict(mask=0, radius=0, lo_p=None, o=gone, **over), "obstacle_mask"), (dict(radius=0, lo_p=None, o=gone, **over), "radius must lie in"),
              (dict(lo_p=None, o=gone, **over), "lo is NULL"), (dict(o=gone, **over), "LA3DM_DF_MAX_CELLS"))
    for kw, text in shared + ((dict(o=null), "index or d2 must not be NULL"), (dict(o=gone), "index or d2 must not be NULL")):
        rc, txt = c_call(False, **kw)
        assert rc < 0 and text in txt and "nearest" in txt and "nearest_points" not in txt, (kw, txt)
    for kw, text in shared + ((dict(n=(1 << 20) + 1), "LA3DM_SCORE_MAX_POINTS (2^20)"), (dict(p_p=None), "points3 is NULL"),
                              (dict(o=null), "cls, voxel, index or d2 must not be NULL"), (dict(o=gone), "cls, voxel, index or d2 must not be NULL"),
                              (dict(radius=0, n=1 << 21, lo_p=None, p_p=None, o=gone, **over), "radius must lie in"),
                              (dict(n=1 << 21, lo_p=None, p_p=None, o=gone, **over), "LA3DM_SCORE_MAX_POINTS"),
                              (dict(p_p=None, o=gone, **over), "LA3DM_DF_MAX_CELLS"), (dict(p_p=None, o=gone), "points3 is NULL")):
        rc, txt = c_call(True, **kw)
        assert rc < 0 and text in txt and "nearest_points" in txt, (kw, txt)
    rc, txt = c_call(True, n=0, p_p=None, o=gone)                          # n_points = 0: served, nothing written or read
    assert rc == 0, txt
    assert all((sent[k] == 7).all() for k in sent)
    rc, txt = c_call(False)
    want = m.nearest(lo, (4, 4, 4), radius=8)
    assert rc == 0 and (sent["index"][:64] == want["index"].reshape(-1)).all() and (sent["d2"][:64] == want["d2"].reshape(-1)).all(), txt
    assert (sent["index"][64:] == 7).all() and (sent["d2"][64:] == 7).all()
    rc, txt = c_call(True)
    want = m.nearest_points(lo, (4, 4, 4), pts, radius=8)
    assert rc == 0 and all((sent[s][:n] == want[k]).all() and (sent[s][n:] == 7).all()
                           for s, k in (("cls", "cls"), ("voxel", "voxel"), ("p_index", "index"), ("p_d2", "d2"))), txt
    # the empty map, both ways
    empty = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
    dims = (6, 5, 4)
    with_missing = empty.nearest(lo, dims, obstacles=("occupied", "missing"), radius=5)
    assert (with_missing["index"] == np.arange(120).reshape(dims)).all() and (with_missing["d2"] == 0).all()
    without = empty.nearest(lo, dims, obstacles="occupied", radius=5)
    assert (without["index"] == N.NONE).all() and (without["d2"] == N.FAR).all()
    R.assert_same(without, m.box(lo, dims, fields=()), ("origin", "cell"))
    inside = m.nearest_points(lo, dims, pts, obstacles=0x1F, radius=1)       # every voxel an obstacle: voxel = index
    a = empty.nearest_points(lo, dims, pts, obstacles=("occupied", "missing"), radius=5)
    N.assert_same(a, inside, "empty map with bit 3", N.POINT_FIELDS)
    b = empty.nearest_points(lo, dims, pts, obstacles="occupied", radius=5)
    hit = inside["cls"] == N.HIT
    assert (b["voxel"] == inside["voxel"]).all() and (b["index"] == N.NONE).all() and (b["d2"] == N.FAR).all()
    assert (b["cls"][hit] == N.FAR_CLS).all() and (b["cls"][~hit] == inside["cls"][~hit]).all()
    assert m.mirror_syncs() == 0


def test_symbols_and_forms(built):
    """CPU test 6: the headers declare and the libraries export the new symbols; the three forms of each query take the same
    arguments after the handle; the constants agree"""
    import la3dm_amd
    from la3dm_amd import _lib
    hip_h = open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
    map_h = open(os.path.join(ROOT, "include", "la3dm_map.h")).read()
    for stem in ("nearest", "nearest_points"):
        forms = [(_lib.hip(), hip_h, f"la3dm_devmap_{stem}_host"), (_lib.hip(), hip_h, f"la3dm_devmap_{stem}_device"),
                 (_lib.maplib(), map_h, f"la3dm_map_{stem}")]
        for lib, txt, name in forms:
            assert re.search(r"\b" + name + r"\s*\(", txt), name
            assert hasattr(lib, name) and name in _lib.HIP_SYMBOLS + _lib.MAP_SYMBOLS, name
        args = [list(getattr(lib, name).argtypes)[1:] for lib, _, name in forms]
        assert args[0] == args[1] == args[2] and len(args[0]) == (6 if stem == "nearest" else 9), stem
        assert f"la3dm_devmap_{stem}" not in "".join(f"la3dm_devmap_{s}_" for s in _lib.QUERIES)
    assert "la3dm_nearest_out" in hip_h and "la3dm_nearest_points_out" in hip_h and "SMALLEST FLAT INDEX" in hip_h
    assert re.search(r"#define\s+LA3DM_NEAREST_NONE\s+0xFFFFFFFFu", hip_h) and re.search(r"#define\s+LA3DM_NEAREST_MAX_RADIUS\s+255u", hip_h)
    assert la3dm_amd.NEAREST_NONE == 0xFFFFFFFF == N.NONE and la3dm_amd.NEAREST_MAX_RADIUS == 255
    assert C.sizeof(_lib.NearestOut) == 16 and C.sizeof(_lib.NearestPointsOut) == 32
