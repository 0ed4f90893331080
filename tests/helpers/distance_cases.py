"""The two yardsticks, the cases and the input conditions shared by tests/test_distance_cpu.py and
tests/test_distance_gpu.py.

Neither yardstick calls distance_field or box: the classes come from `region_cases.yardstick` (a walk of the leaf list),
yardstick A is scipy's exact Euclidean distance transform, yardstick B is the definition itself (the minimum over the
obstacle list, chunked)."""
import numpy as np

import region_cases as R

FAR = 0xFFFFFFFF
MASKS = (1 << R.OCCUPIED, 1 << R.FREE, (1 << R.OCCUPIED) | (1 << R.UNKNOWN) | (1 << R.MISSING), 0x1E)
RADII = (8, 20, 40)
SUB_OFFSET, SUB_DIMS = (30, 10, 5), (40, 40, 20)        # yardstick B's sub-box of the recipe region
SHAPES = ((1, 1, 1), (1, 1, 41), (33, 1, 1), (5, 64, 1), (3, 5, 7), (1, 1, 5), (2, 3, 1), (4, 1, 6))
SHAPE_RADII = (1, 3, 8, 1024)                           # lines shorter than the radius, a radius far beyond the region
LONG_SHAPES = ((1, 1, 3000), (3000, 2, 2))              # at radius 1024


def obstacles_of(cls, mask):
    return ((np.uint32(mask) >> cls.astype(np.uint32)) & 1).astype(bool)


def finish(D, radius, resolution):
    """d2 and dist from the untruncated squared distances D (int64; a negative value = no obstacle at all)"""
    far = (D < 0) | (D > radius * radius)
    d2 = np.where(far, FAR, D).astype(np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        root = np.sqrt(d2.astype(np.float32))            # fp32 in, fp32 out: correctly rounded
        dist = np.where(far, np.float32(np.inf), root * np.float32(resolution)).astype(np.float32)
    return dict(d2=d2, dist=dist)


def squared_edt(cls, mask):
    """yardstick A, untruncated: scipy's exact EDT, squared and rounded to the integer it stands for; -1 without obstacles"""
    from scipy.ndimage import distance_transform_edt
    obs = obstacles_of(cls, mask)
    if not obs.any():
        return np.full(cls.shape, -1, np.int64)
    return np.rint(distance_transform_edt(~obs) ** 2).astype(np.int64)


def yardstick_a(cls, mask, radius, resolution):
    return finish(squared_edt(cls, mask), radius, resolution)


def squared_brute(cls, mask, chunk=512):
    """yardstick B, untruncated — the definition: min over the obstacles o of |v - o|^2, the obstacle list in chunks, in
    the narrowest integer type that holds the largest squared distance of the box; -1 without obstacles"""
    obs = obstacles_of(cls, mask)
    if not obs.any():
        return np.full(cls.shape, -1, np.int64)
    t = np.int16 if sum((n - 1) ** 2 for n in cls.shape) < 2 ** 15 else np.int32
    v = np.stack(np.meshgrid(*[np.arange(n, dtype=t) for n in cls.shape], indexing="ij"), -1).reshape(-1, 3)
    o = np.argwhere(obs).astype(t)
    best = np.full(v.shape[0], np.iinfo(t).max, t)
    for s in range(0, o.shape[0], chunk):
        oc = o[s:s + chunk]
        acc = np.zeros((v.shape[0], oc.shape[0]), t)
        for ax in range(3):
            d = v[:, ax:ax + 1] - oc[None, :, ax]
            acc += d * d
        np.minimum(best, acc.min(1), out=best)
    return best.astype(np.int64).reshape(cls.shape)


def yardstick_b(cls, mask, radius, resolution):
    return finish(squared_brute(cls, mask), radius, resolution)


def assert_same(got, want, what):
    """exact: d2 by ==, dist by its bits"""
    R.assert_same(got, want, ("d2", "dist"), what)


def input_conditions(cls):
    """counted from the yardstick's classes, never from the code under test"""
    D = squared_edt(cls, 1 << R.OCCUPIED)
    far20 = (D < 0) | (D > 400)
    W = squared_edt(cls, MASKS[2])
    return dict(zeros=int((D == 0).sum()), finite=int(((D > 0) & ~far20).sum()), far=int(far20.sum()),
                distinct=int(np.unique(D[~far20]).size), far40=int(((D < 0) | (D > 1600)).sum()), max_d=int(D.max()),
                wide_zeros=int((W == 0).sum()), wide_finite=int((W > 0).sum()), wide_max=int(W.max()),
                wide_far=int(((W < 0) | (W > 64)).sum()))


def assert_exercises_the_feature(cond):
    """at least half of what was counted on the restatement's map at depth 3 (mask OCCUPIED, radius 20: 6 579 zeros,
    164 949 finite values above 0, 84 472 FAR, 336 distinct finite values; radius 40: 7 659 FAR; mask
    OCCUPIED|UNKNOWN|MISSING: 239 159 zeros, 16 841 finite values up to 13, no FAR) — the margin
    region_cases.assert_region_exercises_the_feature uses between that map and the product's"""
    print(f"distance input conditions: {cond}")
    assert cond["zeros"] >= 3290 and cond["finite"] >= 82475 and cond["far"] >= 42236 and cond["distinct"] >= 168, cond
    assert cond["far40"] >= 3830 and cond["max_d"] > 1600, cond
    assert cond["wide_zeros"] >= 119580 and cond["wide_finite"] >= 8421 and cond["wide_max"] >= 7, cond
    assert cond["wide_far"] == 0, cond                   # the no-FAR case really has none, down to radius 8


def long_line_lo(y, resolution, shape):
    """an anchor for a LONG_SHAPES region whose long axis crosses the recipe region through its most occupied column /
    row, centred on it; from the recipe's yardstick y"""
    occ = y["cls"] == R.OCCUPIED
    res = np.float32(resolution)
    if shape[2] > 1000:                                  # along z through the column with the most occupied voxels
        i, j = np.unravel_index(int(occ.sum(2).argmax()), occ.shape[:2])
        off = (i, j, y["cls"].shape[2] // 2 - shape[2] // 2)
    else:                                                # along x through the (j, k) with the most occupied voxels
        j, k = np.unravel_index(int(occ.sum(0).argmax()), occ.shape[1:])
        off = (y["cls"].shape[0] // 2 - shape[0] // 2, j, k)
    return (y["origin"] + np.array(off, np.float32) * res).astype(np.float32)
