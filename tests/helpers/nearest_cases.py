"""The yardstick, the cases and the input conditions shared by tests/test_nearest_cpu.py and tests/test_nearest_gpu.py.

The yardstick never calls nearest, nearest_points, distance_field or box.  It is written from the contract comment of
include/la3dm_hip.h: the classes of the region from `region_cases.yardstick` (a walk of the leaf list); per voxel the
minimum of |v - o|^2 over the obstacle list in ascending flat index, chunked as `distance_cases.squared_brute` chunks it,
the FIRST minimum kept — the smallest flat index among the nearest obstacles; the points' transform and anchor arithmetic
from `score_cases` (float32 op by op, the block field in float64)."""
import numpy as np

import distance_cases as D
import region_cases as R
import score_cases as S

NONE = 0xFFFFFFFF
FAR = D.FAR
HIT, NEAR, FAR_CLS, OUTSIDE, INVALID = range(5)
FIELDS = ("index", "d2")
POINT_FIELDS = ("cls", "voxel", "index", "d2")
SHAPES = D.SHAPES + ((5, 5, 5), (1, 1, 65), (2, 33, 2))
RADII = (1, 3, 8, 255)
MASKS = D.MASKS
SHAPE_OFFSET = S.SHAPE_OFFSET


def brute(cls, mask, voxels=None, chunk=256):
    """The definition, untruncated, for the voxels (n, 3) of the region (None: all of them, in flat order): Dmin int64 = the
    least squared distance to an obstacle (-1: the region holds none), first int64 = the flat index of the first obstacle,
    in ascending flat index, that attains it (-1: none), minimisers int64 = how many obstacles attain it"""
    obs = D.obstacles_of(cls, mask)
    nx, ny, nz = cls.shape
    if voxels is None:
        voxels = np.stack(np.meshgrid(*[np.arange(n) for n in cls.shape], indexing="ij"), -1).reshape(-1, 3)
    v = np.asarray(voxels, np.int32).reshape(-1, 3)
    n = v.shape[0]
    if not obs.any():
        return np.full(n, -1, np.int64), np.full(n, -1, np.int64), np.zeros(n, np.int64)
    o = np.argwhere(obs).astype(np.int32)                   # C order: ascending flat index
    flat = (o[:, 0].astype(np.int64) * ny + o[:, 1]) * nz + o[:, 2]
    best = np.full(n, np.iinfo(np.int32).max, np.int32)
    first = np.full(n, -1, np.int64)
    count = np.zeros(n, np.int64)
    for s in range(0, o.shape[0], chunk):
        oc = o[s:s + chunk]
        acc = np.zeros((n, oc.shape[0]), np.int32)
        for ax in range(3):
            d = v[:, ax:ax + 1] - oc[None, :, ax]
            acc += d * d
        m = acc.min(1)
        a = acc.argmin(1)                                   # the first of equals
        c = (acc == m[:, None]).sum(1)
        better, equal = m < best, m == best                 # an earlier chunk keeps a tie
        count = np.where(better, c, np.where(equal, count + c, count))
        first = np.where(better, flat[s + a], first)
        best = np.where(better, m, best)
    return best.astype(np.int64), first, count


def finish(Dmin, first, radius):
    """index and d2 of nearest from the untruncated answer"""
    far = (Dmin < 0) | (Dmin > radius * radius)
    return dict(index=np.where(far, NONE, first).astype(np.uint32), d2=np.where(far, FAR, Dmin).astype(np.uint32))


def yardstick(cls, mask, radius):
    """nearest over a region with the classes cls: index and d2 of shape cls.shape"""
    Dmin, first, _ = brute(cls, mask)
    return {k: a.reshape(cls.shape) for k, a in finish(Dmin, first, radius).items()}


def conditions(cls, mask, radius):
    """counted from the yardstick: voxels with more than one nearest obstacle (within the radius), voxels with NONE, obstacles"""
    Dmin, first, count = brute(cls, mask)
    far = (Dmin < 0) | (Dmin > radius * radius)
    return dict(tied=int(((count > 1) & ~far).sum()), none=int(far.sum()), obstacles=int((Dmin == 0).sum()), voxels=int(Dmin.size))


_CLS = {}


def region_classes(m, lv, lo, dims):
    lo = np.ascontiguousarray(lo, np.float32)
    key = (id(m), lo.tobytes(), tuple(dims))
    if key not in _CLS:
        _CLS[key] = R.yardstick(m, lv, lo, dims)["cls"]
    return _CLS[key]


def points_yardstick(m, lv, lo, dims, points, pose, mask, radius):
    """cls, voxel, index, d2 of nearest_points; pose None: the points' floats as they are"""
    depth, res = int(m.get_block_depth()), m.get_resolution()
    _, _, g0, _ = R.anchor(lo, res, depth)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    w = p[None] if pose is None else S.transform(p, np.asarray(pose, np.float32).reshape(1, 3, 4))
    invalid, b, g = S.resolve(w, res, depth)
    invalid, b, g = invalid[0], b[0], g[0]
    q = g - np.array(g0, np.int64)
    outside = ((b < 0) | (b >= (1 << 20))).any(-1) | ((q < 0) | (q >= np.array(dims, np.int64))).any(-1)
    inside = ~invalid & ~outside
    n = p.shape[0]
    out = dict(cls=np.where(invalid, INVALID, OUTSIDE).astype(np.uint8), voxel=np.full(n, NONE, np.uint32),
               index=np.full(n, NONE, np.uint32), d2=np.full(n, FAR, np.uint32))
    if inside.any():
        vox = q[inside]
        Dmin, first, _ = brute(region_classes(m, lv, lo, dims), mask, voxels=vox)
        f = finish(Dmin, first, radius)
        out["voxel"][inside] = ((vox[:, 0] * dims[1] + vox[:, 1]) * dims[2] + vox[:, 2]).astype(np.uint32)
        out["index"][inside] = f["index"]
        out["d2"][inside] = f["d2"]
        out["cls"][inside] = np.where(f["d2"] == 0, HIT, np.where(f["d2"] != FAR, NEAR, FAR_CLS)).astype(np.uint8)
    return out


def class_counts(y):
    return [int((y["cls"] == k).sum()) for k in range(5)]


def assert_same(got, want, what, fields=FIELDS):
    """exact: every array by == with shape and dtype"""
    R.assert_same(got, want, [k for k in fields if k in want and k in got], what)


def small_lo(m, origin, offset=SHAPE_OFFSET):
    return S.small_lo(m, origin, offset)


def place(big_cls, dims):
    """Where in the recipe region (classes big_cls, from the yardstick) a small region of `dims` goes: SHAPE_OFFSET for a line
    or a single voxel; for a region with at least two axes longer than 1 the first offset of a fixed grid at which the
    yardstick counts voxels with more than one nearest OCCUPIED voxel within 8 — so that every such case has ties to break"""
    if sum(n > 1 for n in dims) < 2 or any(n > b for n, b in zip(dims, big_cls.shape)):   # (or a region that does not fit)
        return SHAPE_OFFSET
    for a in range(0, big_cls.shape[0] - dims[0] + 1, 7):
        for b in range(0, big_cls.shape[1] - dims[1] + 1, 7):
            for c in range(0, big_cls.shape[2] - dims[2] + 1, 3):
                sub = big_cls[a:a + dims[0], b:b + dims[1], c:c + dims[2]]
                if (sub == R.OCCUPIED).sum() >= 2 and conditions(sub, MASKS[0], 8)["tied"] > 0:
                    return (a, b, c)
    raise AssertionError(f"no offset with tied voxels for {dims}")


def jittered_cloud(origin, dims, res, n=1025, seed=3):
    """n points round a small region: the centres of the region padded by two voxels and the same jittered by up to a voxel,
    in a seeded order, the first the region's own first centre; then a NaN, an inf and a 1e12 m point"""
    rng = np.random.default_rng(seed)
    c = S.centres(origin, dims, res, pad=2)
    jit = (c[rng.integers(0, c.shape[0], 2048)] + rng.uniform(-1, 1, (2048, 3)).astype(np.float32) * np.float32(res)).astype(np.float32)
    pts = np.vstack([c, jit])
    pts = np.vstack([S.centres(origin, dims, res)[:1], pts[rng.permutation(pts.shape[0])]])[:n - 3]
    bad = np.array([(np.nan, 0, 0), (0, np.inf, 0), (0, 0, 1.0e12)], np.float32)
    return np.ascontiguousarray(np.vstack([pts, bad]), np.float32)


# ---- the hand-built map: one block of depth 4 (8 x 8 x 8 cells round the origin), a 5 x 5 x 5 region at cell (1, 1, 1) whose
# six face-centre voxels are OCCUPIED and every other cell FREE
FACE_CENTRES = ((0, 2, 2), (4, 2, 2), (2, 0, 2), (2, 4, 2), (2, 2, 0), (2, 2, 4))
HAND_DIMS = (5, 5, 5)
HAND_LO = (-0.25, -0.25, -0.25)       # the centre of cell (1, 1, 1): block centre 0, 0.1 m cells from -0.4


def hand_built_stream(params):
    import pack_cases as P
    assert int(params["block_depth"]) == 4
    h = P.header_fields("BGKOctoMap", params)
    npb = P.npb_of(4)
    A = np.full((1, npb), np.float32(h["init_A"]), np.float32)
    B = np.full((1, npb), np.float32(h["init_B"]), np.float32)
    St = np.full((1, npb), P.UNKNOWN, np.uint8)
    fine = P.base(3)
    St[0, fine:] = R.FREE
    A[0, fine:], B[0, fine:] = np.float32(0.001), np.float32(5.0)
    for i, j, k in FACE_CENTRES:
        x, y, z = i + 1, j + 1, k + 1
        node = 0
        for level in (2, 1, 0):
            node = node * 8 + ((((x >> level) & 1) << 2) | (((y >> level) & 1) << 1) | ((z >> level) & 1))
        St[0, fine + node] = R.OCCUPIED
        A[0, fine + node], B[0, fine + node] = np.float32(5.0), np.float32(0.001)
    key = (524288 << 40) | (524288 << 20) | 524288
    return P.stream_from_pool(h, np.array([key], np.int64), A, B, St)
