"""The yardstick, the recipe and the input conditions shared by tests/test_gain_cpu.py and tests/test_gain_gpu.py.

The yardstick never calls gain or box.  Per ray the number of rows comes from `m.raycast_many` with the same stop mask
and budget, the rows themselves from `m.raycast(start, end)[:steps]` (the plain RayCaster, row by row), the lattice
position of a row from its block key and the decoded node key (digits base 8, bit 4 = x, 2 = y, 1 = z, the most
significant digit the coarsest level) minus `region_cases.anchor`'s g0, and the class of a voxel of the region from
`region_cases.yardstick` (a walk of the leaf list).  The sets are numpy booleans, packed at the end."""
import numpy as np

import region_cases as R

FREE_M, OCC_M, UNK_M, MISS_M = 1 << R.FREE, 1 << R.OCCUPIED, 1 << R.UNKNOWN, 1 << R.MISSING
RAY_HIT = 1
FIELDS = ("gain", "started", "hits", "seen")
# (count, stop, max_steps): the planner's masks; stopping on UNKNOWN as well; FREE rows of a short budget; every class
CASES = ((0xC, 0x2, 4096), (0xC, 0xA, 4096), (FREE_M, 0, 9), (0x1F, 0, 7))
SMALL_DIMS = ((1, 1, 1), (1, 1, 31), (1, 1, 32), (1, 1, 33), (3, 5, 7), (33, 1, 1))
SMALL_CASES = ((0xC, 0x2, 4096), (0x1F, 0, 64))
SHAPE_OFFSET = (37, 41, 14)                              # in the thick of the recipe region (frontier_cases' anchor)
NEVER_STARTS = (500.0, 500.0, 500.0)


def fan(m, radius):
    """m points of a Fibonacci sphere, computed in float64 and cast to float32"""
    i = np.arange(m, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / m
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    return (np.stack([r * np.cos(phi), r * np.sin(phi), z], 1) * radius).astype(np.float32)


def viewpoints(y, res):
    """the recipe's seven: six FREE voxels of the yardstick region drawn by default_rng(23), as their centres in fp32, and one
    that never starts"""
    rng = np.random.default_rng(23)
    free = np.argwhere(y["cls"] == R.FREE)
    pick = free[rng.choice(len(free), 6, replace=False)]
    o = (y["origin"] + pick.astype(np.float32) * np.float32(res)).astype(np.float32)
    return np.vstack([o, np.array(NEVER_STARTS, np.float32)]).astype(np.float32), pick


def near_viewpoints(y, res, at=SHAPE_OFFSET, k=3):
    """the k FREE voxels of the yardstick region nearest to voxel `at` (ties: the lower flat index), as centres"""
    free = np.argwhere(y["cls"] == R.FREE)
    d2 = ((free - np.array(at)) ** 2).sum(1)
    pick = free[np.argsort(d2, kind="stable")[:k]]
    return (y["origin"] + pick.astype(np.float32) * np.float32(res)).astype(np.float32), pick


def sub_lo(y, offset, res):
    return (y["origin"] + np.array(offset, np.float32) * np.float32(res)).astype(np.float32)


def small_cases(m, y, near, pick):
    """(what, lo, dims, origins, offsets) of the small-shape tests"""
    res = m.get_resolution()
    lo = sub_lo(y, SHAPE_OFFSET, res)
    f96 = fan(96, 3.0)
    cases = [(f"dims {d}", lo, d, near, f96) for d in SMALL_DIMS]
    away = tuple(int(v) for v in pick[0] + np.array((3, 3, 1)))
    box = (4, 4, 4)
    assert not any(all(a <= int(p[k]) < a + b for k, (a, b) in enumerate(zip(away, box))) for p in pick)
    cases.append(("region without the viewpoints", sub_lo(y, away, res), box, near, f96))
    cases.append(("m = 1", lo, (3, 5, 7), near, f96[40:41]))
    bad = np.array([near[0], (np.nan, 0, 0), near[1], (3.0e8, 0, 0), near[2]], np.float32)
    cases.append(("a NaN origin and a 3e8 m origin", lo, (3, 5, 7), bad, f96))
    return cases


_WALKS = {}


def walk(m, origins, offsets, stop_mask, max_steps):
    """every ray's rows as global lattice positions: dict(steps (n, m), flags (n, m), pos = list over rays of (steps, 3) int64)"""
    origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    offsets = np.ascontiguousarray(offsets, np.float32).reshape(-1, 3)
    key = (id(m), origins.tobytes(), offsets.tobytes(), int(stop_mask), int(max_steps))
    if key in _WALKS:
        return _WALKS[key]
    n, nd = origins.shape[0], offsets.shape[0]
    dl = int(m.get_block_depth()) - 1
    lim = 1 << dl
    starts = np.repeat(origins, nd, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        ends = (starts + np.tile(offsets, (n, 1))).astype(np.float32)          # one fp32 add per coordinate
    rc = m.raycast_many(starts, ends, stop=int(stop_mask), max_steps=int(max_steps))
    pos = []
    for r in range(n * nd):
        steps = int(rc["steps"][r])
        if steps == 0:
            pos.append(np.zeros((0, 3), np.int64))
            continue
        rows = m.raycast(starts[r], ends[r], cap=steps)
        assert rows["block_key"].shape[0] == steps, (r, steps)
        bk, idx = rows["block_key"].astype(np.int64), rows["node_key"].astype(np.int64) & 0xFFFF
        assert ((rows["node_key"] >> 16) == dl).all()
        c = np.zeros((steps, 3), np.int64)
        for level in range(dl):
            digit = (idx >> (3 * level)) & 7
            c[:, 0] |= ((digit >> 2) & 1) << level
            c[:, 1] |= ((digit >> 1) & 1) << level
            c[:, 2] |= (digit & 1) << level
        field = np.stack([(bk >> 40) & 0xFFFFF, (bk >> 20) & 0xFFFFF, bk & 0xFFFFF], 1)
        pos.append(field * lim + c)
    out = dict(steps=rc["steps"].reshape(n, nd), flags=rc["flags"].reshape(n, nd), pos=pos)
    _WALKS[key] = out
    return out


def pack(sets):
    """(n, total) booleans -> (n, W) uint32, bit f % 32 of word f // 32"""
    n, total = sets.shape
    W = (total + 31) // 32
    padded = np.zeros((n, W * 32), np.uint8)
    padded[:, :total] = sets
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view(np.uint32).reshape(n, W)


def yardstick(m, lv, lo, dims, origins, offsets, count_mask, stop_mask, max_steps, cls=None):
    """gain, started, hits, seen — and what the input conditions count: marked rows and rays with rows outside the region"""
    depth = int(m.get_block_depth())
    _, _, g0, _ = R.anchor(lo, m.get_resolution(), depth)
    if cls is None:
        cls = R.yardstick(m, lv, lo, dims)["cls"]
    assert cls.shape == tuple(dims)
    w = walk(m, origins, offsets, stop_mask, max_steps)
    n, nd = w["steps"].shape
    total = int(np.prod(dims))
    sets = np.zeros((n, total), bool)
    marked = np.zeros(n, np.int64)
    leaving = np.zeros(n, np.int64)
    g0 = np.array(g0, np.int64)
    for r, p in enumerate(w["pos"]):
        if p.shape[0] == 0:
            continue
        q = p - g0
        inside = ((q >= 0) & (q < np.array(dims))).all(1)
        leaving[r // nd] += int(not inside.all())
        q = q[inside]
        c = cls[q[:, 0], q[:, 1], q[:, 2]].astype(np.uint32)
        hit = ((np.uint32(count_mask) >> c) & 1).astype(bool)
        marked[r // nd] += int(hit.sum())
        f = (q[hit, 0] * dims[1] + q[hit, 1]) * dims[2] + q[hit, 2]
        sets[r // nd, f] = True
    return dict(gain=sets.sum(1).astype(np.uint32), started=(w["steps"] > 0).sum(1).astype(np.uint32),
                hits=((w["flags"] & RAY_HIT) != 0).sum(1).astype(np.uint32), seen=pack(sets), marked=marked, leaving=leaving,
                union=int(sets.any(0).sum()))


def assert_same(got, want, what, fields=FIELDS):
    """exact: every array by == with shape and dtype"""
    R.assert_same(got, want, [k for k in fields if k in want and k in got], what)


def input_conditions(m, lv, y, lo, dims, origins, depth):
    """counted from the yardstick, never from the code under test: the planner's case on the 256-ray fan, and the
    short-budget FREE case"""
    a = yardstick(m, lv, lo, dims, origins, fan(256, 4.0), 0xC, 0x2, 4096, cls=y["cls"])
    b = yardstick(m, lv, lo, dims, origins, fan(256, 4.0), FREE_M, 0, 9, cls=y["cls"])
    wb = walk(m, origins, fan(256, 4.0), 0, 9)
    return dict(depth=depth, gains=a["gain"].tolist(), marked=a["marked"].tolist(), hits=a["hits"].tolist(), started=a["started"].tolist(),
                leaving=a["leaving"].tolist(), union=a["union"], free_gains=b["gain"].tolist(), free_marked=b["marked"].tolist(),
                free_steps=sorted(set(wb["steps"][:6].reshape(-1).tolist())))


def assert_exercises_the_feature(cond):
    """At block_depth 3: about half of what was counted on region_cases.fused_map(3) (gains 2244, 1252, 1998, 1987, 1597,
    1292, 0 from 3823, 2243, 4119, 3685, 2670, 1967 marked rows; 119-163 hits of 256; 14-39 rays per viewpoint with rows
    outside the region; union of the six sets 9102 against a sum of gains of 10 370): the margin the other helpers use
    between that map and the product's.  At block_depth 4 each of those counts must be > 0."""
    print(f"gain input conditions: {cond}")
    g, mk, h, lv = cond["gains"][:6], cond["marked"][:6], cond["hits"][:6], cond["leaving"][:6]
    assert cond["started"][6] == 0 and cond["gains"][6] == 0, cond          # the seventh viewpoint never starts
    assert all(s == 256 for s in cond["started"][:6]), cond
    if cond["depth"] == 3:
        assert min(g) >= 600 and sum(mk) >= 1.3 * sum(g), cond
        assert min(h) >= 50 and max(h) <= 256 - 50 and min(lv) >= 7, cond
        assert cond["free_steps"] == [9], cond                               # FREE / 0 / 9: every ray has exactly 9 rows
    else:
        assert min(g) > 0 and sum(mk) > sum(g) and min(h) > 0 and max(h) < 256 and min(lv) > 0, cond
    assert cond["union"] < sum(g), cond                                      # the sets of the viewpoints overlap
    assert min(cond["free_gains"][:6]) > 0 and sum(cond["free_marked"][:6]) > sum(cond["free_gains"][:6]), cond
