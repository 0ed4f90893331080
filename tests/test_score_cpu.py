"""score_poses on a host-mode map (device = -1, no GPU): one scan under many candidate poses against the distance field of
a region, compared with an independent yardstick (tests/helpers/score_cases.py: the float32 transform op by op, the anchor
arithmetic of region_cases.anchor vectorised, scipy's exact distance transform of region_cases.yardstick's classes).  Every
output is an integer: every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import score_cases as S  # noqa: E402

_RECIPES = {}


def _recipe(depth):
    """(map, leaves, recipe lo, the recipe region's origin, the cloud, the poses)"""
    if depth not in _RECIPES:
        m, lv, lo = R.fused_map(depth)
        _, _, _, origin = R.anchor(lo, m.get_resolution(), depth)
        pts, o = S.sensor_cloud()
        _RECIPES[depth] = (m, lv, lo, origin, pts, S.recipe_poses(o))
    return _RECIPES[depth]


def _regions(m, lo, origin):
    """(lo, dims) of the three regions: the recipe's, and two small ones in the thick of it"""
    return [(lo, S.REGIONS[0])] + [(S.small_lo(m, origin), d) for d in S.REGIONS[1:]]


def _tallies(m, lo, dims, mask, radius):
    """what the identity on a region's own voxel centres must give, from distance_field: sum_d2 and the five counts"""
    d2 = m.distance_field(lo, dims, obstacles=mask, radius=radius, fields=("d2",))["d2"].astype(np.int64)
    far = d2 == 0xFFFFFFFF
    return int(d2[~far].sum()), [int((d2 == 0).sum()), int(((d2 > 0) & ~far).sum()), int(far.sum()), 0, 0]


@pytest.mark.parametrize("depth", [3, 4])
def test_recipe_exercises_the_feature(built, depth):
    """CPU test 0: the input conditions, counted from the yardstick alone"""
    m, lv, lo, _, pts, T = _recipe(depth)
    S.assert_exercises_the_feature(S.input_conditions(m, lv, lo, R.RECIPE_DIMS, pts, T))


@pytest.mark.parametrize("depth", [3, 4])
def test_host_form_equals_the_yardstick(built, depth):
    """CPU test 1: the recipe cloud and pose set on the three regions, three masks, radii 1, 8 and 255; on the small regions
    the cloud is the centres of the region padded by two voxels, moved into the sensor frame, so that pairs fall on both
    sides of every face"""
    m, lv, lo, origin, pts, T = _recipe(depth)
    res = m.get_resolution()
    classes = np.zeros(5, np.int64)
    for rlo, dims in _regions(m, lo, origin):
        cloud = pts
        if dims != R.RECIPE_DIMS:
            _, _, _, o = R.anchor(rlo, res, depth)
            cloud = np.vstack([(S.centres(o, dims, res, pad=2) - T[13, :, 3]).astype(np.float32), pts[-3:]])
        for mask in S.MASKS:
            for radius in S.RADII:
                want = S.yardstick(m, lv, rlo, dims, cloud, T, mask, radius)
                got = m.score_poses(rlo, dims, cloud, T, obstacles=mask, radius=radius)
                assert set(got) == set(S.FIELDS) | set(R.INFO_FIELDS)
                assert got["sum_d2"].dtype == np.uint64 and got["counts"].dtype == np.uint32 and got["counts"].shape == (T.shape[0], 5)
                S.assert_same(got, want, (depth, dims, mask, radius))
                assert (got["counts"].sum(1) == cloud.shape[0]).all()
                classes += want["counts"].sum(0).astype(np.int64)
        print(f"depth {depth} dims {dims}: identity sum_d2 {int(want['sum_d2'][13])} counts {want['counts'][13].tolist()}")
    assert (classes > 0).all(), classes
    # names select the same masks; (P, 12) is (P, 3, 4); fields = sum_d2 alone; the defaults are OCCUPIED and radius 16
    want = S.yardstick(m, lv, lo, R.RECIPE_DIMS, pts, T, 1 << R.OCCUPIED, 16)
    dflt = m.score_poses(lo, R.RECIPE_DIMS, pts, T.reshape(-1, 12), fields="sum_d2")
    assert set(dflt) == {"sum_d2"} | set(R.INFO_FIELDS) and (dflt["sum_d2"] == want["sum_d2"]).all()
    names = m.score_poses(lo, R.RECIPE_DIMS, pts, T, obstacles=("occupied", "unknown", "missing"), radius=8)
    S.assert_same(names, S.yardstick(m, lv, lo, R.RECIPE_DIMS, pts, T, S.MASKS[2], 8), "names")
    R.assert_same(names, m.box(lo, R.RECIPE_DIMS, fields=()), ("origin", "cell"), "info")
    assert m.mirror_syncs() == 0


@pytest.mark.parametrize("depth", [3, 4])
def test_exact_algebra(built, depth):
    """CPU test 2: the identity on the region's own voxel centres gives distance_field's tallies; a pose that translates by
    whole voxels gives the tallies of the region shifted likewise; a 90 degree yaw with entries 0 and +-1 permutes the
    coordinates exactly; the counts sum to n_points"""
    m, lv, lo, origin, _, _ = _recipe(depth)
    res = np.float32(m.get_resolution())
    for rlo, dims in _regions(m, lo, origin)[:2]:
        _, _, _, o = R.anchor(rlo, res, depth)
        c = S.centres(o, dims, res)
        for mask, radius in ((S.MASKS[0], 8), (S.MASKS[2], 3)):
            kw = dict(obstacles=mask, radius=radius)
            total, counts = _tallies(m, rlo, dims, mask, radius)
            got = m.score_poses(rlo, dims, c, S.IDENTITY[None], **kw)
            assert int(got["sum_d2"][0]) == total and got["counts"][0].tolist() == counts, (dims, mask, got, total, counts)
            assert sum(counts) == c.shape[0]
            # translated by (3, -2, 1) voxels: the same points under that pose land on the centres of the shifted region
            shift = np.array((3, -2, 1), np.float32) * res
            slo = (np.asarray(rlo, np.float32) + shift).astype(np.float32)
            _, _, sg0, so = R.anchor(slo, res, depth)
            _, _, g0, _ = R.anchor(rlo, res, depth)
            assert [a - b for a, b in zip(sg0, g0)] == [3, -2, 1]
            moved = S.IDENTITY.copy()
            moved[:, 3] = shift
            total, counts = _tallies(m, slo, dims, mask, radius)
            got = m.score_poses(slo, dims, c, moved[None], **kw)
            same = m.score_poses(slo, dims, S.centres(so, dims, res), S.IDENTITY[None], **kw)
            assert int(got["sum_d2"][0]) == total and got["counts"][0].tolist() == counts, (dims, mask, got, total, counts)
            S.assert_same(got, same, "translated == the identity on the shifted region")
            # yaw by 90 degrees: w = (-y, x, z) exactly, so the points (cy, -cx, cz) land on the centres
            yaw = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0]], np.float32)
            turned = np.stack([c[:, 1], -c[:, 0], c[:, 2]], 1).astype(np.float32)
            S.assert_same(m.score_poses(rlo, dims, turned, yaw[None], **kw), m.score_poses(rlo, dims, c, S.IDENTITY[None], **kw), "yaw 90")
            both = m.score_poses(rlo, dims, np.vstack([c, turned]), np.stack([S.IDENTITY, yaw]), **kw)
            assert (both["counts"].sum(1) == 2 * c.shape[0]).all()
    assert m.mirror_syncs() == 0


def test_boundary_and_invalid_inputs(built):
    """CPU test 3: the centres of the voxels one step outside each of the six faces are OUTSIDE and their neighbours inside
    are not; NaN, inf and 1e12 m coordinates are INVALID one by one and leave the other pairs alone; a pose with a NaN
    entry makes every pair INVALID"""
    m, lv, lo, origin, _, _ = _recipe(3)
    res = np.float32(m.get_resolution())
    dims = (3, 5, 7)
    rlo = S.small_lo(m, origin)
    _, _, _, o = R.anchor(rlo, res, 3)
    ijk = np.stack(np.meshgrid(*[np.arange(-1, n + 1) for n in dims], indexing="ij"), -1).reshape(-1, 3)
    inside = ((ijk >= 0) & (ijk < np.array(dims))).all(1)
    pts = (o + ijk.astype(np.float32) * res).astype(np.float32)
    I1 = S.IDENTITY[None]
    for axis in range(3):
        for side, at in ((-1, -1), (1, dims[axis])):
            face = pts[(ijk[:, axis] == at)]
            got = m.score_poses(rlo, dims, face, I1, obstacles=0x1F, radius=1)
            assert got["counts"][0].tolist() == [0, 0, 0, face.shape[0], 0] and got["sum_d2"][0] == 0, (axis, side, got)
            skin = pts[inside & (ijk[:, axis] == at - side)]
            got = m.score_poses(rlo, dims, skin, I1, obstacles=0x1F, radius=1)                    # every class an obstacle: all HIT
            assert got["counts"][0].tolist() == [skin.shape[0], 0, 0, 0, 0], (axis, side, got)
    S.assert_same(m.score_poses(rlo, dims, pts, I1, radius=8), S.yardstick(m, lv, rlo, dims, pts, I1, 1 << R.OCCUPIED, 8), "padded box")
    good = pts[inside]
    alone = m.score_poses(rlo, dims, good, I1, radius=8)
    for bad in ((np.nan, 0, 0), (0, np.nan, 0), (0, 0, np.nan), (np.inf, 0, 0), (0, -np.inf, 0), (0, 0, 1.0e12), (-1.0e12, 0, 0), (1.1e8, 0, 0)):
        mixed = np.vstack([good[:5], np.array([bad], np.float32), good[5:]])
        got = m.score_poses(rlo, dims, mixed, I1, radius=8)
        assert got["counts"][0, S.INVALID] == 1 and got["sum_d2"][0] == alone["sum_d2"][0], (bad, got)
        assert (got["counts"][0, :4] == alone["counts"][0, :4]).all(), (bad, got)
    assert m.score_poses(rlo, dims, np.array([(1.0e8, 0, 0)], np.float32), I1)["counts"][0].tolist() == [0, 0, 0, 1, 0]   # |w / res| < 2^30: a voxel, not in the region
    for r in range(3):
        for c in range(4):
            T = np.stack([S.IDENTITY, S.IDENTITY, S.IDENTITY])
            T[1, r, c] = np.nan
            got = m.score_poses(rlo, dims, good, T, radius=8)
            assert got["counts"][1].tolist() == [0, 0, 0, 0, good.shape[0]] and got["sum_d2"][1] == 0, (r, c, got)
            for p in (0, 2):                                                                       # the neighbours' answers are untouched
                assert got["sum_d2"][p] == alone["sum_d2"][0] and (got["counts"][p] == alone["counts"][0]).all()
    inf_t = S.IDENTITY.copy()
    inf_t[0, 3] = np.inf
    assert m.score_poses(rlo, dims, good, inf_t[None])["counts"][0, S.INVALID] == good.shape[0]


def test_trivial_cases_and_the_empty_map(built):
    """CPU test 4: n_poses = 0 is served and writes nothing, n_points = 0 writes zeros; an empty map answers from the
    definition: every pair that is neither INVALID nor OUTSIDE is HIT with the mask's bit 3 and FAR without it"""
    import la3dm_amd
    m, lv, lo, origin, pts, T = _recipe(3)
    z = m.score_poses(lo, (6, 5, 4), pts, np.zeros((0, 12), np.float32))
    assert z["sum_d2"].shape == (0,) and z["counts"].shape == (0, 5)
    z = m.score_poses(lo, (6, 5, 4), np.zeros((0, 3), np.float32), T)
    assert z["sum_d2"].shape == (T.shape[0],) and (z["sum_d2"] == 0).all() and (z["counts"] == 0).all()
    z = m.score_poses(lo, (6, 5, 4), np.zeros((0, 3), np.float32), np.zeros((0, 3, 4), np.float32))
    assert z["sum_d2"].shape == (0,)
    empty = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
    full = m.score_poses(lo, R.RECIPE_DIMS, pts, T, obstacles=0x1F, radius=1)["counts"]          # every voxel an obstacle
    with_missing = empty.score_poses(lo, R.RECIPE_DIMS, pts, T, obstacles=("occupied", "missing"), radius=5)
    without = empty.score_poses(lo, R.RECIPE_DIMS, pts, T, obstacles="occupied", radius=5)
    assert (with_missing["counts"] == full).all() and (with_missing["sum_d2"] == 0).all()
    assert (without["counts"] == full[:, [2, 1, 0, 3, 4]]).all() and (without["sum_d2"] == 0).all() and (full[:, 1:3] == 0).all()
    assert int(full[:, 0].sum()) > 0
    R.assert_same(without, m.box(lo, R.RECIPE_DIMS, fields=()), ("origin", "cell"))


def test_refusals_in_their_order(built):
    """CPU test 5: every refusal raises with a text that names the argument and leaves the outputs alone; a call that
    breaks several rules is answered by the first of the contract's order"""
    from la3dm_amd import _lib
    m, lv, lo, origin, pts, T = _recipe(3)
    q = lambda **kw: m.score_poses(kw.pop("lo", lo), kw.pop("dims", (4, 4, 4)), kw.pop("points", pts), kw.pop("poses", T), **kw)   # noqa: E731
    for mask in (0, 0x20, 0x3F, 1 << 31, ()):
        with pytest.raises(RuntimeError, match="obstacle_mask must hold"):
            q(obstacles=mask)
    for radius in (0, 256, 1024):
        with pytest.raises(RuntimeError, match=r"radius must lie in \[1, LA3DM_SCORE_MAX_RADIUS \(255\)\]"):
            q(radius=radius)
    assert q(radius=255)["sum_d2"].shape == (T.shape[0],) and q(radius=1, obstacles=0x1F)["counts"].shape == (T.shape[0], 5)
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
        with pytest.raises(RuntimeError, match=r"LA3DM_SCORE_MAX_CELLS \(2\^28\)"):
            q(dims=dims)
    with pytest.raises(ValueError, match="unknown fields"):
        q(fields=("sum_d2", "cls"))
    with pytest.raises(ValueError, match=r"\(P, 3, 4\) or \(P, 12\)"):
        q(poses=np.zeros((4, 4, 4), np.float32))
    # the limits, the NULL pointers and the order, through the C view: no pointer is followed before the checks have passed
    M = _lib.maplib()
    lo3 = np.ascontiguousarray(lo, np.float32)
    p3, t12 = np.ascontiguousarray(pts), np.ascontiguousarray(T)
    n, P = pts.shape[0], T.shape[0]
    sent = dict(sum_d2=np.full(P + 8, 7, np.uint64), counts=np.full(5 * P + 8, 7, np.uint32))
    out = _lib.ScoreOut(sent["sum_d2"].ctypes.data, sent["counts"].ctypes.data)

    def c_call(lo_p=lo3.ctypes.data, dims=(4, 4, 4), with_dims=True, p_p=p3.ctypes.data, n=n, t_p=t12.ctypes.data, P=P, mask=0x2, radius=8,
               o=C.byref(out)):
        d3 = np.array(dims, np.uint32)
        rc = M.la3dm_map_score_poses(m._h, lo_p, d3.ctypes.data if with_dims else None, p_p, n, t_p, P, mask, radius, o, None)
        return rc, M.la3dm_map_last_error().decode()
    over = dict(dims=((1 << 28) + 1, 1, 1))
    for kw, text in ((dict(mask=0), "obstacle_mask"), (dict(mask=0x40), "obstacle_mask"), (dict(radius=0), "radius must lie in"),
                     (dict(radius=256), "radius must lie in"), (dict(n=(1 << 20) + 1, P=1), "LA3DM_SCORE_MAX_POINTS (2^20)"),
                     (dict(n=1, P=(1 << 20) + 1), "LA3DM_SCORE_MAX_POSES (2^20)"),
                     (dict(n=1 << 20, P=(1 << 12) + 1), "LA3DM_SCORE_MAX_PAIRS (2^32)"), (dict(n=(1 << 12) + 1, P=1 << 20), "LA3DM_SCORE_MAX_PAIRS (2^32)"),
                     (dict(lo_p=None), "lo is NULL"), (dict(with_dims=False), "dims is NULL"), (dict(dims=(4, 0, 4)), "dims must be >= 1"),
                     (dict(over), "LA3DM_SCORE_MAX_CELLS"), (dict(t_p=None), "poses12 is NULL"), (dict(o=None), "sum_d2 must not be NULL"),
                     (dict(o=C.byref(_lib.ScoreOut(None, sent["counts"].ctypes.data))), "sum_d2 must not be NULL"),
                     (dict(p_p=None), "points3 is NULL"),
                     # the order: each call breaks the rule named and every later one
                     (dict(mask=0, radius=0, n=1 << 21, P=1 << 21, lo_p=None, t_p=None, p_p=None, o=None, **over), "obstacle_mask"),
                     (dict(radius=0, n=1 << 21, P=1 << 21, lo_p=None, t_p=None, p_p=None, o=None, **over), "radius must lie in"),
                     (dict(n=1 << 21, P=1 << 21, lo_p=None, t_p=None, p_p=None, o=None, **over), "LA3DM_SCORE_MAX_POINTS"),
                     (dict(n=1 << 20, P=1 << 21, lo_p=None, t_p=None, p_p=None, o=None, **over), "LA3DM_SCORE_MAX_POSES"),
                     (dict(n=1 << 20, P=1 << 20, lo_p=None, t_p=None, p_p=None, o=None, **over), "LA3DM_SCORE_MAX_PAIRS"),
                     (dict(lo_p=None, t_p=None, p_p=None, o=None, **over), "lo is NULL"),
                     (dict(t_p=None, p_p=None, o=None, **over), "LA3DM_SCORE_MAX_CELLS"),
                     (dict(t_p=None, p_p=None, o=None), "poses12 is NULL"), (dict(p_p=None, o=None), "sum_d2 must not be NULL")):
        rc, txt = c_call(**kw)
        assert rc < 0 and text in txt and "score_poses" in txt, (kw, txt)
    assert all((sent[k] == 7).all() for k in sent)
    # at the limits: 2^20 points x 2^12 poses = 2^32 pairs pass the counts and stop at the buffers
    rc, txt = c_call(n=1 << 20, P=1 << 12, t_p=None)
    assert rc < 0 and "poses12 is NULL" in txt, txt
    for kw in (dict(P=0, t_p=None, p_p=None, o=None), dict(P=0, n=0, t_p=None, p_p=None, o=None)):   # n_poses = 0: served, nothing written or read
        rc, txt = c_call(**kw)
        assert rc == 0, txt
    assert all((sent[k] == 7).all() for k in sent)
    rc, txt = c_call(n=0, p_p=None)                                              # n_points = 0: zeros, points3 may be NULL
    assert rc == 0 and (sent["sum_d2"][:P] == 0).all() and (sent["counts"][:5 * P] == 0).all(), txt
    assert (sent["sum_d2"][P:] == 7).all() and (sent["counts"][5 * P:] == 7).all()
    rc, txt = c_call(o=C.byref(_lib.ScoreOut(sent["sum_d2"].ctypes.data, None)))  # counts NULL
    assert rc == 0 and (sent["sum_d2"][P:] == 7).all() and (sent["counts"][:5 * P] == 0).all(), txt
    want = m.score_poses(lo, (4, 4, 4), pts, T, radius=8)
    assert (sent["sum_d2"][:P] == want["sum_d2"]).all()
    assert m.mirror_syncs() == 0


def test_poses_xyz_yaw(built):
    """CPU test 6: yaw 0 is the identity rotation with t = d exactly where the centre cancels; a yaw keeps the centre where
    the translation puts it; the entries are float32 roundings of the double formula"""
    import math
    import la3dm_amd
    c = (1.5, -2.25, 0.5)
    T = la3dm_amd.poses_xyz_yaw(c, [(0.0, 0.0, 0.0, 0.0), (0.25, -0.5, 0.125, 0.0), (0.1, 0.2, 0.3, 0.7), (0, 0, 0, math.pi / 2)])
    assert T.shape == (4, 3, 4) and T.dtype == np.float32
    assert (T[0] == S.IDENTITY).all() and (T[1, :, :3] == S.IDENTITY[:, :3]).all() and T[1, :, 3].tolist() == [0.25, -0.5, 0.125]
    cs, sn = math.cos(0.7), math.sin(0.7)
    assert T[2, 0, 0] == np.float32(cs) and T[2, 0, 1] == np.float32(-sn) and T[2, 1, 0] == np.float32(sn) and T[2, 2, 3] == np.float32(0.3)
    assert T[2, 0, 3] == np.float32((c[0] + 0.1) - (cs * c[0] - sn * c[1])) and T[2, 1, 3] == np.float32((c[1] + 0.2) - (sn * c[0] + cs * c[1]))
    w = S.transform(np.array([c], np.float32), T)[:, 0]
    assert np.abs(w[2] - (np.array(c) + (0.1, 0.2, 0.3))).max() < 1e-5 and np.abs(w[3] - np.array(c)).max() < 1e-5
    assert la3dm_amd.poses_xyz_yaw(c, np.zeros((0, 4))).shape == (0, 3, 4)
