"""The yardstick, the path sets and the input conditions shared by tests/test_paths_cpu.py and tests/test_paths_gpu.py.

The yardstick never calls score_paths, distance_field, travel or box.  It is written from the contract comment of
include/la3dm_hip.h: the waypoint voxels from `score_cases.resolve` (the anchor arithmetic of region_cases.anchor,
vectorised), the walk vectorised over the ordinals of a path (numpy's cumsum, searchsorted and floor_divide on int64), the
classes of the region from `region_cases.yardstick` (a walk of the leaf list), d2 from `distance_cases` (scipy's exact
Euclidean distance transform), the stop, the cost and the other outputs with numpy."""
import numpy as np

import distance_cases as D
import region_cases as R
import score_cases as S

BLOCKED, LEFT, TRUNCATED, INVALID = 1, 2, 4, 8
NONE = 0xFFFFFFFF
FIELDS = ("cost", "steps", "stop", "min_d2", "ways", "flags")
DTYPES = dict(cost=np.uint64, steps=np.uint32, stop=np.uint32, min_d2=np.uint32, ways=np.uint32, flags=np.uint8)
REGIONS = S.REGIONS                                       # the recipe's, (3, 5, 7) and (1, 1, 33)
RADII = (0, 1, 8)                                         # clearance and soft_radius
COND = dict(mask=1 << R.OCCUPIED, clearance=1, soft_radius=3, penalty=50, move_cost=(10, 14, 17), max_steps=64)


def params(mask=1 << R.OCCUPIED, clearance=0, soft_radius=0, penalty=0, move_cost=(10, 14, 17), max_steps=4096):
    return dict(mask=mask, clearance=clearance, soft_radius=soft_radius, penalty=penalty, move_cost=tuple(move_cost), max_steps=max_steps)


def call(m, lo, dims, paths, p, **kw):
    """score_paths with a params dict of this module"""
    return m.score_paths(lo, dims, paths, obstacles=p["mask"], clearance=p["clearance"], soft_radius=p["soft_radius"], penalty=p["penalty"],
                         move_cost=p["move_cost"], max_steps=p["max_steps"], **kw)


def walk(G, max_steps):
    """the voxels of ordinals 0 ... E of the waypoint voxels G (W, 3) int64, the offsets, T and E"""
    d = np.diff(G, axis=0)
    n = np.abs(d).max(1) if d.shape[0] else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    T = int(off[-1])
    E = min(T, max_steps)
    o = np.arange(1, E + 1, dtype=np.int64)
    k = np.searchsorted(off, o, side="left")               # the smallest k with off[k] >= o
    s = (o - off[k - 1])[:, None]
    nk = n[k - 1][:, None]
    v = G[k - 1] + np.floor_divide(2 * s * d[k - 1] + nk, 2 * nk)
    return np.vstack([G[:1], v]).astype(np.int64), off, T, E


def pen(word, p):
    s2 = p["soft_radius"] ** 2
    w = word.astype(np.int64)
    return np.where((s2 > 0) & (w <= s2), p["penalty"] * (s2 - np.minimum(w, s2)) // max(s2, 1), 0)


def one_path(G, g0, dims, d2, p):
    """the six outputs of one valid path, and what the input conditions count: the moves by class and the penalties charged"""
    V, off, T, E = walk(G, p["max_steps"])
    q = V - np.array(g0, np.int64)
    inside = ((q >= 0) & (q < np.array(dims, np.int64))).all(1)
    q = np.where(inside[:, None], q, 0)
    word = np.where(inside, d2[q[:, 0], q[:, 1], q[:, 2]], D.FAR).astype(np.int64)
    blocked = inside & (word != D.FAR) & (word <= p["clearance"] ** 2)
    halt = ~inside | blocked
    flags, stop = 0, NONE
    if halt.any():
        stop = int(halt.argmax())
        flags = BLOCKED if inside[stop] else LEFT
    elif T > p["max_steps"]:
        flags = TRUNCATED
    L = stop if stop != NONE else E + 1
    nz = (np.diff(V, axis=0) != 0).sum(1)                  # the move into ordinal 1, 2, ...
    assert ((nz >= 1) & (nz <= 3)).all() and (np.abs(np.diff(V, axis=0)) <= 1).all()   # a 26-connected walk
    charged = slice(1, max(L, 1))
    pens = pen(word[charged], p)
    cost = int((np.array(p["move_cost"], np.int64)[nz[:max(L - 1, 0)] - 1] + pens).sum())
    out = dict(cost=cost, steps=L, stop=stop, min_d2=int(word[:L].min()) if L else D.FAR, ways=int((off < L).sum()), flags=flags)
    return out, np.bincount(nz[:max(L - 1, 0)], minlength=4)[1:4], int((pens > 0).sum())


def yardstick(m, lv, lo, dims, paths, p):
    """the six arrays, and `moves` (3,) = the charged moves with 1, 2, 3 components, `penalised` = the charged voxels with a
    penalty above 0"""
    depth = int(m.get_block_depth())
    _, _, g0, _ = R.anchor(lo, m.get_resolution(), depth)
    d2 = S.cost_volume(m, lv, lo, dims, p["mask"], max(1, p["clearance"], p["soft_radius"]))
    W = np.ascontiguousarray(paths, np.float32)
    invalid, _, G = S.resolve(W, m.get_resolution(), depth)
    out = {k: np.zeros(W.shape[0], DTYPES[k]) for k in FIELDS}
    moves, penalised = np.zeros(3, np.int64), 0
    for i in range(W.shape[0]):
        if invalid[i].any():
            one = dict(cost=0, steps=0, stop=NONE, min_d2=D.FAR, ways=0, flags=INVALID)
        else:
            one, mv, pn = one_path(G[i], g0, dims, d2, p)
            moves += mv
            penalised += pn
        for k in FIELDS:
            out[k][i] = one[k]
    out.update(moves=moves, penalised=penalised)
    return out


def assert_same(got, want, what, fields=FIELDS):
    """exact: every array by == with shape and dtype"""
    R.assert_same(got, want, [k for k in fields if k in got], what)


def centre(origin, ijk, resolution):
    """voxel centres origin + (i, j, k) * resolution as float32, any leading shape"""
    return (np.asarray(origin, np.float32) + np.asarray(ijk, np.float32) * np.float32(resolution)).astype(np.float32)


def padded(rows, n_way):
    """(P, n_way, 3) float32 from lists of waypoints: a shorter path repeats its last waypoint"""
    out = np.empty((len(rows), n_way, 3), np.float32)
    for i, r in enumerate(rows):
        r = np.asarray(r, np.float32).reshape(-1, 3)
        assert 1 <= r.shape[0] <= n_way
        out[i, :r.shape[0]] = r
        out[i, r.shape[0]:] = r[-1]
    return out


def open_voxel(m, lv, lo, dims, mask=1 << R.OCCUPIED):
    """(a, occ): a = the voxel of the region farthest from every obstacle whose 26 neighbours lie in the region (the first
    such in flat order), occ = the obstacle voxel nearest to it; from the yardstick's classes and scipy's transform"""
    S.cost_volume(m, lv, lo, dims, mask, 1)
    key = (id(m), np.ascontiguousarray(lo, np.float32).tobytes(), tuple(dims))
    edt, cls = S._EDT[key + (mask,)], S._CLS[key]
    inner = np.zeros(dims, bool)
    inner[tuple(slice(1, n - 1) if n > 2 else slice(0, n) for n in dims)] = True
    a = np.array(np.unravel_index(int(np.where(inner, edt, -2).argmax()), dims))
    obs = np.argwhere(D.obstacles_of(cls, mask))
    occ = obs[((obs - a) ** 2).sum(1).argmin()] if obs.shape[0] else None
    return a, occ


def recipe_paths(m, lv, lo, dims, n_way=8, n_random=40, seed=5):
    """hand-built paths round the region's most open voxel `a` and random ones, as voxel centres with a sub-voxel jitter on
    the random ones.  In the order built: a zigzag a, b, a, b, ... of n_way waypoints with b up to ten voxels from a towards
    the middle of the longest axis (T = 10 (n_way - 1): TRUNCATED with max_steps below that), the same zigzag cut after three
    waypoints (clean), one-step paths along an axis, a plane diagonal and the space diagonal (moves with 1, 2, 3 components),
    a path from a to the centre of the nearest obstacle voxel (BLOCKED, past voxels that carry a penalty), a path from a out
    through the nearer face of axis 0 (LEFT, unless something blocks it before), a path that starts two voxels outside (LEFT
    at 0), a NaN in the last waypoint, an inf in the first and 1e12 in the middle (INVALID), then the random ones: n_way
    waypoints drawn from the region padded by two voxels."""
    depth, res = int(m.get_block_depth()), m.get_resolution()
    _, _, _, origin = R.anchor(lo, res, depth)
    a, occ = open_voxel(m, lv, lo, dims)
    c = lambda *ijk: centre(origin, ijk, res)   # noqa: E731
    step = lambda axis: np.eye(3, dtype=np.int64)[axis] * (1 if dims[axis] > 1 and a[axis] + 1 < dims[axis] else 0)   # noqa: E731
    axis = int(np.argmax(dims))
    b = a.copy()
    b[axis] = a[axis] + min(10, dims[axis] - 1 - a[axis]) if 2 * a[axis] < dims[axis] else a[axis] - min(10, a[axis])
    rows = [[c(*(a if k % 2 == 0 else b)) for k in range(n_way)], [c(*a), c(*b), c(*a)]]
    rows += [[c(*a), c(*(a + step(0)))], [c(*a), c(*(a + step(0) + step(1)))], [c(*a), c(*(a + step(0) + step(1) + step(2)))]]
    if occ is not None:
        rows.append([c(*a), c(*occ)])
    out = a.copy()
    out[0] = -3 if 2 * a[0] < dims[0] else dims[0] + 2
    rows += [[c(*a), c(*out)], [c(-2, 0, 0), c(*a)]]
    bad = [[c(*a), c(*b), (np.nan, 0, 0)], [(0, np.inf, 0), c(*a)], [c(*a), (0, 0, 1.0e12), c(*b)]]
    rng = np.random.default_rng(seed)
    ijk = np.stack([rng.integers(-2, n + 2, (n_random, n_way)) for n in dims], -1)
    rnd = (centre(origin, ijk, res) + (rng.random((n_random, n_way, 3), np.float32) - np.float32(0.5)) * np.float32(0.8 * res)).astype(np.float32)
    return np.concatenate([padded(rows + bad, n_way), rnd])


def input_conditions(m, lv, lo, dims, paths, p=None):
    """counted from the yardstick, never from the code under test"""
    y = yardstick(m, lv, lo, dims, paths, p or COND)
    f = y["flags"]
    return dict(n_paths=int(f.size), n_way=int(np.asarray(paths).shape[1]), clean=int((f == 0).sum()), blocked=int((f == BLOCKED).sum()),
                left=int((f == LEFT).sum()), truncated=int((f == TRUNCATED).sum()), invalid=int((f == INVALID).sum()),
                moves=y["moves"].tolist(), penalised=int(y["penalised"]), distinct_costs=int(np.unique(y["cost"]).size),
                longest=int(y["steps"].max()), left_at_0=int(((f == LEFT) & (y["stop"] == 0)).sum()))


def assert_exercises_the_feature(cond):
    """at least one path of every kind — clean, BLOCKED, LEFT (one of them at ordinal 0), TRUNCATED, INVALID — charged moves
    with 1, 2 and 3 components, a charged voxel with a penalty above 0, and costs that differ between paths"""
    print(f"paths input conditions: {cond}")
    for k in ("clean", "blocked", "left", "truncated", "invalid", "penalised", "left_at_0"):
        assert cond[k] > 0, (k, cond)
    assert all(v > 0 for v in cond["moves"]), cond
    assert cond["distinct_costs"] >= 4 and cond["longest"] > 1, cond
    assert cond["clean"] + cond["blocked"] + cond["left"] + cond["truncated"] + cond["invalid"] == cond["n_paths"], cond
