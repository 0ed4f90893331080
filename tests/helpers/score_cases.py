"""The yardstick, the recipe and the input conditions shared by tests/test_score_cpu.py and tests/test_score_gpu.py.

The yardstick never calls score_poses, distance_field or box.  It is written from the contract comment of
include/la3dm_hip.h: the float32 transform op by op in numpy (every product and every sum a float32 array operation of its
own), the anchor arithmetic vectorised after `region_cases.anchor` (the block field in float64, the centre and the cell in
float32), the classes of the region from `region_cases.yardstick` (a walk of the leaf list), d2 from
`distance_cases.yardstick_a` (scipy's exact Euclidean distance transform), the five classes and the sum with numpy."""
import numpy as np

import distance_cases as D
import region_cases as R
from conftest import pcd_path

HIT, NEAR, FAR, OUTSIDE, INVALID = range(5)
FIELDS = ("sum_d2", "counts")
MASKS = D.MASKS[:3]
RADII = (1, 8, 255)
SHAPE_OFFSET = (37, 41, 14)                              # in the thick of the recipe region (gain_cases' anchor)
REGIONS = (R.RECIPE_DIMS, (3, 5, 7), (1, 1, 33))
COND_MASK, COND_RADIUS = MASKS[0], 8                    # what the input conditions are counted with
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


def transform(points, poses):
    """(P, n, 3) float32: w[c] = ((R[c][0] * x + R[c][1] * y) + R[c][2] * z) + t[c], each operation rounded to float32"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    T = np.ascontiguousarray(poses, np.float32).reshape(-1, 3, 4)
    x, y, z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    w = np.empty((T.shape[0], p.shape[0], 3), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            a = (T[:, c, 0:1] * x).astype(np.float32)
            b = (T[:, c, 1:2] * y).astype(np.float32)
            s = (a + b).astype(np.float32)
            d = (T[:, c, 2:3] * z).astype(np.float32)
            s = (s + d).astype(np.float32)
            w[:, :, c] = (s + T[:, c, 3:4]).astype(np.float32)
    return w


def resolve(w, resolution, depth):
    """(invalid (...,) bool, b (..., 3) int64 block fields, g (..., 3) int64 global indices) of float32 coordinates w: the
    anchor arithmetic of region_cases.anchor, vectorised; b and g are 0 where the pair is invalid"""
    res = np.float32(resolution)
    lim = 1 << (depth - 1)
    bs = np.float32(np.float32(2.0 ** (depth - 1)) * res)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ok = (np.abs((w / res).astype(np.float32)) < np.float32(2.0 ** 30)).all(-1)      # false for NaN and inf
        v = np.where(ok[..., None], w, np.float32(0)).astype(np.float32)
        b = (v.astype(np.float64) / np.float64(bs) + 524288.5).astype(np.int64)          # truncation (positive: |v / bs| < 2^30 res / bs)
        center = ((b - 524288).astype(np.float32) * bs).astype(np.float32)
        t = (((v - center).astype(np.float32) / res).astype(np.float32) + np.float32(lim // 2)).astype(np.float32)
        cell = np.clip(np.trunc(t).astype(np.int64), 0, lim - 1)
    b = np.where(ok[..., None], b, 0)
    return ~ok, b, np.where(ok[..., None], b * lim + cell, 0)


def classify(w, resolution, depth, g0, dims, d2):
    """(cls (P, n) uint8, value (P, n) int64: d2 of the HIT and NEAR pairs, 0 elsewhere)"""
    invalid, b, g = resolve(w, resolution, depth)
    q = g - np.array(g0, np.int64)
    outside = ((b < 0) | (b >= (1 << 20))).any(-1) | ((q < 0) | (q >= np.array(dims, np.int64))).any(-1)
    inside = ~invalid & ~outside
    q = np.where(inside[..., None], q, 0)
    v = d2[q[..., 0], q[..., 1], q[..., 2]].astype(np.int64)
    cls = np.where(v == 0, HIT, np.where(v != D.FAR, NEAR, FAR))
    cls = np.where(invalid, INVALID, np.where(outside, OUTSIDE, cls)).astype(np.uint8)
    return cls, np.where(inside & (v != D.FAR), v, 0)


_CLS, _EDT = {}, {}


def cost_volume(m, lv, lo, dims, mask, radius):
    """d2 of the region by yardstick A; the classes and the untruncated transform are kept per (map, region, mask)"""
    lo = np.ascontiguousarray(lo, np.float32)
    key = (id(m), lo.tobytes(), tuple(dims))
    if key not in _CLS:
        _CLS[key] = R.yardstick(m, lv, lo, dims)["cls"]
    if key + (mask,) not in _EDT:
        _EDT[key + (mask,)] = D.squared_edt(_CLS[key], mask)
    return D.finish(_EDT[key + (mask,)], radius, m.get_resolution())["d2"]


def yardstick(m, lv, lo, dims, points, poses, mask, radius):
    """sum_d2 (P,) uint64 and counts (P, 5) uint32, and the classes of the pairs (P, n)"""
    depth = int(m.get_block_depth())
    _, _, g0, _ = R.anchor(lo, m.get_resolution(), depth)
    d2 = cost_volume(m, lv, lo, dims, mask, radius)
    cls, value = classify(transform(points, poses), m.get_resolution(), depth, g0, dims, d2)
    counts = np.stack([(cls == k).sum(1) for k in range(5)], 1).astype(np.uint32)
    return dict(sum_d2=value.sum(1).astype(np.uint64), counts=counts, cls=cls)


def assert_same(got, want, what, fields=FIELDS):
    """exact: every array by == with shape and dtype"""
    R.assert_same(got, want, [k for k in fields if k in want and k in got], what)
    if "counts" in got:
        assert got["counts"].shape[1:] == (5,)


# ---- the recipe: scan 2 of sim_structured in its sensor frame, candidate poses round the pose it was taken from --------
def sensor_cloud(scan=2, step=3):
    """every step-th point of the scan minus the scan's origin (one float32 subtract per coordinate), then a NaN, an inf and
    a 1e12 m point; returns the cloud and the origin"""
    import la3dm_amd
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", scan))
    o = np.asarray(origin, np.float32)
    pts = (np.ascontiguousarray(xyz, np.float32)[::step] - o).astype(np.float32)
    bad = np.array([(np.nan, 0, 0), (0, np.inf, 0), (0, 0, 1.0e12)], np.float32)
    return np.vstack([pts, bad]).astype(np.float32), o


def recipe_poses(origin):
    """27 poses of a (dx, dy, dyaw) grid round the scan's own pose — the identity is number 13 — and five more: a pose 50 m
    away (inside the lattice, outside the region), one 3e5 m away (block fields beyond 2^20), one with a NaN entry, one
    1e12 m away, one whose R halves every length (not a rotation)"""
    import la3dm_amd
    o = [float(v) for v in origin]
    grid = [(o[0] + dx, o[1] + dy, o[2], dyaw) for dx in (-0.2, 0.0, 0.2) for dy in (-0.2, 0.0, 0.2) for dyaw in (-0.05, 0.0, 0.05)]
    grid += [(o[0] + 50.0, o[1], o[2], 0.0), (o[0] + 3.0e5, o[1], o[2], 0.0)]
    T = la3dm_amd.poses_xyz_yaw((0.0, 0.0, 0.0), grid)
    nan = T[13].copy()
    nan[1, 2] = np.nan
    far = T[13].copy()
    far[2, 3] = np.float32(1.0e12)
    half = T[13].copy()
    half[:, :3] *= np.float32(0.5)
    return np.concatenate([T, nan[None], far[None], half[None]]).astype(np.float32)


def small_lo(m, y_origin, offset=SHAPE_OFFSET):
    return (np.asarray(y_origin, np.float32) + np.array(offset, np.float32) * np.float32(m.get_resolution())).astype(np.float32)


def centres(origin, dims, resolution, pad=0):
    """the voxel centres of a region (padded by `pad` voxels on every side) as float32 points, origin + (i, j, k) * resolution"""
    ijk = np.stack(np.meshgrid(*[np.arange(-pad, n + pad) for n in dims], indexing="ij"), -1).reshape(-1, 3)
    return (np.asarray(origin, np.float32) + ijk.astype(np.float32) * np.float32(resolution)).astype(np.float32)


def input_conditions(m, lv, lo, dims, points, poses):
    """counted from the yardstick, never from the code under test"""
    y = yardstick(m, lv, lo, dims, points, poses, COND_MASK, COND_RADIUS)
    c = y["counts"].astype(np.int64)
    return dict(n_points=int(np.asarray(points).reshape(-1, 3).shape[0]), n_poses=int(c.shape[0]), identity=c[13].tolist(),
                poses_with=[int((c[:, k] > 0).sum()) for k in range(5)], most=[int(c[:, k].max()) for k in range(5)],
                distinct_sums=int(np.unique(y["sum_d2"]).size), identity_sum=int(y["sum_d2"][13]),
                best=int(np.argmin(np.where(c[:, HIT] + c[:, NEAR] > 0, y["sum_d2"].astype(np.int64) + 64 * (c[:, FAR] + c[:, OUTSIDE]), 2 ** 62))))


def assert_exercises_the_feature(cond):
    """every one of the five classes is non-empty for at least one pose, sum_d2 differs between poses, and the scan's own
    pose sees the map: at least a tenth of the cloud on or next to an obstacle.  (On region_cases.fused_map(3), OCCUPIED
    obstacles and radius 8, the identity pose of the recipe counts 742 HIT, 370 NEAR, no FAR, 55 OUTSIDE and 3 INVALID of
    1170 points with a sum of 597; the FAR pairs, 14, are the halving pose's, whose points end in open space.)"""
    print(f"score input conditions: {cond}")
    assert all(v > 0 for v in cond["poses_with"]), cond
    assert cond["distinct_sums"] >= 2, cond
    h, nr, fr, out, inv = cond["identity"]
    assert h + nr + fr + out + inv == cond["n_points"] and inv == 3, cond
    assert h + nr >= cond["n_points"] // 10 and h > 0 and nr > 0, cond
    assert cond["most"][OUTSIDE] == cond["n_points"] - 3 and cond["most"][INVALID] == cond["n_points"], cond
