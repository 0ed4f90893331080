"""The yardstick, the brick model, the hand-built sets and the input conditions shared by tests/test_clusters_cpu.py and
tests/test_clusters_gpu.py.

The yardstick never calls clusters, box or frontier: the classes come from `region_cases.yardstick` (a walk of the leaf
list), the frontier's list from `frontier_cases.score_of` over the padded classes, the labels from `scipy.ndimage.label`
— a tile is imposed by spreading the member array, index a -> a + a // tile on every axis, which puts an empty plane
between tiles — numbered by first occurrence in flat order (numpy min-label sweeps of shifted slices where scipy is
missing), and the records and `rep` from the definition.

`brick_model` is a numpy model of the device form's scheme — bricks of 8 x 8 x 8 voxels, each relaxed (min over the
adjacent members' labels) against a frozen one-voxel halo for at most INNER iterations per round, a halo cell of another
tile a non-member, the neighbour bricks of changed border voxels activated for the next round.  It counts rounds, brick
runs and capped runs from the yardstick's members, so what the GPU tests expect of the diagnostics is never taken from
the code under test."""
import numpy as np

import region_cases as R
import frontier_cases as F

NONE = 0xFFFFFFFF
INF = np.int64(1) << 40
BRICK, INNER, BATCH = 8, 16, 8       # what the header must say (asserted by the tests)
CONNECTIVITIES = F.CONNECTIVITIES
TILES = (0, 8, 16)
FREE_M, OCC_M, UNK_M, MISS_M = F.FREE_M, F.OCC_M, F.UNK_M, F.MISS_M
RECORDS = ("first", "size", "lo", "hi", "sum", "rep")
STATS = ("n", "n_members", "n_clusters", "n_dropped", "largest")
DIAG = ("rounds", "brick_runs", "capped")


def flat(ijk, dims):
    return (int(ijk[0]) * int(dims[1]) + int(ijk[1])) * int(dims[2]) + int(ijk[2])


_RECIPES = {}


def recipe(m, lv, key):
    """(lo, cls, list, info) of the recipe region on map m: its classes and frontier's default list (open FREE, unknown
    UNKNOWN | MISSING, connectivity 6, one neighbour) from the yardstick over the region padded by one voxel"""
    if key not in _RECIPES:
        res = np.float32(m.get_resolution())
        lo, pcls, info = F.padded_case(m, lv, (R.recipe_lo() - res).astype(np.float32), R.RECIPE_DIMS)
        listed = F.answer_of(F.score_of(pcls, FREE_M, UNK_M | MISS_M, 6), 1)["index"]
        _RECIPES[key] = (lo, np.ascontiguousarray(pcls[1:-1, 1:-1, 1:-1]), listed, info)
    return _RECIPES[key]


def members_of(cls, member_mask, members=None):
    """the member array from the contract: the class test, and with a list only the listed voxels in range"""
    ok = F.in_mask(cls, member_mask)
    if members is None:
        return ok
    t = np.asarray(members, np.int64)
    listed = np.zeros(cls.size, bool)
    listed[t[(t >= 0) & (t < cls.size)]] = True
    return ok & listed.reshape(cls.shape)


def _spread(shape, tile):
    return [np.arange(n) + (np.arange(n) // tile if tile else 0) for n in shape]


def components(member, connectivity, tile=0):
    """int64 labels 0 ... numbered by first occurrence in flat order, -1 for a non-member"""
    ax = _spread(member.shape, tile)
    wide = np.zeros([int(a[-1]) + 1 for a in ax], bool)
    wide[np.ix_(*ax)] = member
    try:
        from scipy import ndimage
        lab, _ = ndimage.label(wide, structure=ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity]))
        lab = lab[np.ix_(*ax)].astype(np.int64)
    except ImportError:
        lab = _sweeps(wide, connectivity)[np.ix_(*ax)]
    out = np.full(member.shape, -1, np.int64)
    fl = lab.reshape(-1)
    at = np.flatnonzero(fl > 0)
    if at.size:
        ids, first = np.unique(fl[at], return_index=True)
        rank = np.empty(ids.size, np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(ids.size)       # the cluster met first gets 0
        out.reshape(-1)[at] = rank[np.searchsorted(ids, fl[at])]
    return out


def _sweeps(wide, connectivity):
    """(slow path) min-label sweeps of shifted slices to the fixed point: label = 1 + the smallest flat index of the component"""
    nx, ny, nz = wide.shape
    pad = np.full((nx + 2, ny + 2, nz + 2), INF, np.int64)
    cur = pad[1:-1, 1:-1, 1:-1]
    cur[wide] = 1 + np.flatnonzero(wide.reshape(-1))
    while True:
        best = cur.copy()
        for di, dj, dk in F.offsets(connectivity):
            np.minimum(best, pad[1 + di:1 + di + nx, 1 + dj:1 + dj + ny, 1 + dk:1 + dk + nz], out=best)
        better = wide & (best < cur)
        if not better.any():
            return np.where(wide, cur, 0)
        cur[better] = best[better]


def yardstick(cls, member_mask=FREE_M, members=None, connectivity=26, tile=0, min_size=1, cap=None):
    """the whole answer from the definition; `cap` None: every record"""
    member = members_of(cls, member_mask, members)
    comp = components(member, connectivity, tile)
    n_all = int(comp.max()) + 1 if member.any() else 0
    sizes = np.bincount(comp[comp >= 0], minlength=n_all)
    keep = sizes >= min_size
    number = np.where(keep, np.cumsum(keep) - 1, -1)
    lab = np.where(comp >= 0, number[np.maximum(comp, 0)], -1) if n_all else np.full(cls.shape, -1, np.int64)
    n = int(keep.sum())
    out = dict(label=np.where(lab >= 0, lab, NONE).astype(np.uint32), n=n, n_members=int(member.sum()), n_clusters=n,
               n_dropped=int((~keep).sum()), largest=int(sizes[keep].max()) if n else 0, sizes_all=sizes)
    if members is not None:
        t = np.asarray(members, np.int64)
        of = np.full(t.size, NONE, np.uint32)
        inside = (t >= 0) & (t < cls.size)
        of[inside] = out["label"].reshape(-1)[t[inside]]
        out["of_member"] = of
    m = n if cap is None else min(n, int(cap))
    f = np.flatnonzero((lab.reshape(-1) >= 0) & (lab.reshape(-1) < m))
    c = lab.reshape(-1)[f]
    v = np.stack(np.unravel_index(f, cls.shape), 1).astype(np.int64)
    size = np.bincount(c, minlength=m).astype(np.int64)
    first = np.full(m, INF, np.int64)
    np.minimum.at(first, c, f)
    lo, hi, s = np.full((m, 3), INF, np.int64), np.full((m, 3), -1, np.int64), np.zeros((m, 3), np.int64)
    for a in range(3):
        np.minimum.at(lo[:, a], c, v[:, a])
        np.maximum.at(hi[:, a], c, v[:, a])
        np.add.at(s[:, a], c, v[:, a])
    centre = (2 * s + size[:, None]) // np.maximum(2 * size[:, None], 1)
    key = (((v - centre[c]) ** 2).sum(1) << 32) | f
    best = np.full(m, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(best, c, key)
    out.update(first=first.astype(np.uint32), size=size.astype(np.uint32), lo=lo.astype(np.uint32), hi=hi.astype(np.uint32),
               sum=s.astype(np.uint64), rep=(best & 0xFFFFFFFF).astype(np.uint32))
    return out


def brick_model(member, connectivity, tile=0, inner_cap=INNER):
    """The device form's scheme in numpy: dict(first, rounds, brick_runs, capped).  first = the fixed point (the smallest
    flat index of the voxel's cluster, INF for a non-member); rounds = the rounds in which a voxel changed; capped = the
    brick runs whose inner_cap-th iteration still changed a voxel."""
    nx, ny, nz = member.shape
    B = [(n + BRICK - 1) // BRICK for n in member.shape]
    tb = tile // BRICK if tile else 1 << 20
    G = np.full([b * BRICK + 2 for b in B], INF, np.int64)
    inner = G[1:-1, 1:-1, 1:-1]
    own = np.arange(member.size, dtype=np.int64).reshape(member.shape)
    inner[:nx, :ny, :nz] = np.where(member, own, INF)
    open_ = inner != INF                                                       # a copy
    tiles = np.lib.stride_tricks.sliding_window_view(G, (10, 10, 10))[::8, ::8, ::8]
    bricks = lambda a: a.reshape(B[0], 8, B[1], 8, B[2], 8).transpose(0, 2, 4, 1, 3, 5)    # noqa: E731
    open_b = bricks(open_)
    offs = F.offsets(connectivity)
    active = open_b.any(axis=(3, 4, 5))                                        # every brick that holds a member
    rounds = brick_runs = capped = 0
    while active.any():
        at = np.argwhere(active)
        T = tiles[at[:, 0], at[:, 1], at[:, 2]].copy()                         # this round's inputs
        for axis in range(3):                                                  # a halo cell of another tile is a non-member
            idx = [slice(None)] * 4
            idx[0], idx[axis + 1] = at[:, axis] % tb == 0, 0
            T[tuple(idx)] = INF
            idx[0], idx[axis + 1] = (at[:, axis] + 1) % tb == 0, 9
            T[tuple(idx)] = INF
        o = open_b[at[:, 0], at[:, 1], at[:, 2]]
        running = np.ones(len(at), bool)
        ever = np.zeros(o.shape, bool)
        brick_runs += len(at)
        for _ in range(inner_cap):
            cur = T[:, 1:9, 1:9, 1:9]
            best = cur.copy()
            for di, dj, dk in offs:
                np.minimum(best, T[:, 1 + di:9 + di, 1 + dj:9 + dj, 1 + dk:9 + dk], out=best)
            changed = o & (best < cur) & running[:, None, None, None]
            cur[changed] = best[changed]
            ever |= changed
            running &= changed.any(axis=(1, 2, 3))
            if not running.any():
                break
        capped += int(running.sum())
        nxt = np.zeros_like(active)
        wrote = ever.any(axis=(1, 2, 3))
        for n in np.flatnonzero(wrote):
            i, j, k = (int(v) for v in at[n])
            G[1 + 8 * i:9 + 8 * i, 1 + 8 * j:9 + 8 * j, 1 + 8 * k:9 + 8 * k] = T[n, 1:9, 1:9, 1:9]
            if running[n]:
                nxt[i, j, k] = True
            for di, dj, dk in offs:
                sel = tuple(slice(None) if d == 0 else (0 if d < 0 else 7) for d in (di, dj, dk))
                q = (i + di, j + dj, k + dk)
                if all(0 <= q[a] < B[a] and q[a] // tb == (i, j, k)[a] // tb for a in range(3)) and ever[n][sel].any():
                    nxt[q] = True
        if wrote.any():
            rounds += 1
        active = nxt
    return dict(first=inner[:nx, :ny, :nz].copy(), rounds=rounds, brick_runs=brick_runs, capped=capped)


def model_of(cls, member_mask, members, connectivity, tile):
    """the model's counts, with the model's fixed point checked against the labelling"""
    member = members_of(cls, member_mask, members)
    m = brick_model(member, connectivity, tile)
    comp = components(member, connectivity, tile)
    firsts = np.full(int(comp.max()) + 2, INF, np.int64)
    np.minimum.at(firsts, comp[member], np.flatnonzero(member.reshape(-1)))
    assert (m["first"][member] == firsts[comp[member]]).all() and (m["first"][~member] == INF).all(), "the brick model gives the labelling"
    return {k: m[k] for k in DIAG}


TABLE = ((0, 6), (0, 26), (8, 6), (8, 26), (16, 26), (32, 26))
_CONDITIONS = {}


def input_conditions(cls, listed, key=None):
    """counted from the yardstick, never from the code under test.  `key` caches the answer (a depth)"""
    if key is not None and key in _CONDITIONS:
        return _CONDITIONS[key]
    out = dict(listed=int(np.asarray(listed).size), rows={}, model={})
    for tile, c in TABLE:
        s = yardstick(cls, FREE_M, listed, c, tile, cap=0)["sizes_all"]
        out["rows"][(tile, c)] = dict(clusters=int(s.size), largest=int(s.max()), singletons=int((s == 1).sum()), ge8=int((s >= 8).sum()),
                                      in_ge8=int(s[s >= 8].sum()))
    for tile, c in ((0, 6), (8, 26)):
        out["model"][(tile, c)] = model_of(cls, FREE_M, listed, c, tile)
    if key is not None:
        _CONDITIONS[key] = out
    return out


def assert_exercises_the_feature(cond):
    """At least half of what was counted on region_cases.fused_map at block_depth 3 / 4 over the recipe region, from
    frontier's default list of 8 767 / 8 735 voxels (the smaller of the two halved): clusters, the largest, singletons,
    clusters of at least 8 voxels and the voxels in them, per (tile, connectivity) —
      (0, 6) 405 / 6 774 / 207 / 39 / 8 015; (0, 26) 14 / 8 711 / 11 / 1 / 8 711; (8, 6) 1 031 / 144 / 359 / 282 / 7 048;
      (8, 26) 233 / 221 / 32 / 141 / 8 480; (16, 26) 91 / 1 344 / 19 / 37 / 8 578; (32, 26) 38 / 3 477 / 13 / 10 / 8 669.
    The untiled connectivity-6 query needs more rounds than one batch and hits the inner cap in this file's model."""
    print(f"clusters input conditions: {cond}")
    assert cond["listed"] >= 4367, cond
    half = {(0, 6): (202, 3387, 103, 19, 4007), (0, 26): (7, 4355, 5, 1, 4355), (8, 6): (515, 72, 179, 141, 3524),
            (8, 26): (116, 110, 16, 70, 4240), (16, 26): (45, 672, 9, 18, 4289), (32, 26): (19, 1738, 6, 5, 4334)}
    for q, want in half.items():
        got = cond["rows"][q]
        assert all(got[k] >= w for k, w in zip(("clusters", "largest", "singletons", "ge8", "in_ge8"), want)), (q, got, want)
    m = cond["model"][(0, 6)]
    assert m["rounds"] > BATCH and m["capped"] >= 1, cond


# ---- hand-built sets: (name, dims, member voxels, tile, {connectivity: clusters expected} or None) ------------------------
def _box(lo, hi):
    return [(i, j, k) for i in range(lo[0], hi[0]) for j in range(lo[1], hi[1]) for k in range(lo[2], hi[2])]


def snake():
    """35 voxels wound through the plane i = 0 of one brick: the rows j = 0, 2, 4, 6 joined at alternating ends; the
    smallest index (0, 0, 0) is one end, so its label walks 34 steps at connectivity 6"""
    v = []
    for r, j in enumerate((0, 2, 4, 6)):
        v += [(0, j, k) for k in range(8)]
        if j < 6:
            v.append((0, j + 1, 7 if r % 2 == 0 else 0))
    return v


def shell():
    """the surface of a 5 x 5 x 5 cube at (1, 1, 1): the centroid (3, 3, 3) is no member, six face centres tie at distance 2"""
    return [v for v in _box((1, 1, 1), (6, 6, 6)) if any(c in (1, 5) for c in v)]


def hand_sets():
    rng = np.random.default_rng(20261019)
    sets = []
    for dims in ((1, 1, 1), (1, 1, 41), (33, 1, 1), (3, 5, 7), (9, 8, 17)):
        every = _box((0, 0, 0), dims)
        sets.append((f"all of {dims}", dims, every, 0, {6: 1, 18: 1, 26: 1}))
        some = [v for v in every if rng.random() < 0.55]
        sets.append((f"half of {dims}", dims, some or every, 0, None))
        sets.append((f"half of {dims}, tile 8", dims, some or every, 8, None))
    corner, edge = [(7, 7, 7), (8, 8, 8)], [(7, 7, 3), (8, 8, 3)]
    sets.append(("a brick corner", (16, 16, 16), corner, 0, {6: 2, 18: 2, 26: 1}))
    sets.append(("a brick edge", (16, 16, 16), edge, 0, {6: 2, 18: 1, 26: 1}))
    sets.append(("a brick corner, tile 16", (16, 16, 16), corner, 16, {6: 2, 18: 2, 26: 1}))
    sets.append(("a tile corner", (16, 16, 16), corner, 8, {6: 2, 18: 2, 26: 2}))
    sets.append(("a tile edge", (16, 16, 16), edge, 8, {6: 2, 18: 2, 26: 2}))
    sets.append(("a snake in one brick", (8, 8, 8), snake(), 0, {6: 1, 18: 1, 26: 1}))
    for axis in range(3):
        dims = [3, 3, 3]
        dims[axis] = 32
        line = [tuple(t if a == axis else 1 for a in range(3)) for t in range(32)]
        sets.append((f"a line along axis {axis}", tuple(dims), line, 0, {6: 1, 18: 1, 26: 1}))
        sets.append((f"a line along axis {axis}, tile 8", tuple(dims), line, 8, {6: 4, 18: 4, 26: 4}))
    ell = [(0, j, 0) for j in range(5)] + [(i, 0, 0) for i in range(1, 5)]
    sets.append(("overlapping boxes", (6, 6, 2), ell + [(3, 3, 0)], 0, {6: 2, 18: 2, 26: 2}))
    sets.append(("a hollow shell", (7, 7, 7), shell(), 0, {6: 1, 18: 1, 26: 1}))
    return sets


def assert_same(got, want, what, fields=("label", "of_member") + RECORDS + STATS):
    for k in STATS:
        if k in fields:
            assert got[k] == want[k], (what, k, got[k], want[k])
    R.assert_same(got, want, [k for k in ("label", "of_member") + RECORDS if k in fields and k in want and k in got], what)
