"""The yardstick, the brick model, the cases and the input conditions shared by tests/test_travel_cpu.py and
tests/test_travel_gpu.py.

The yardstick never calls travel, reach, box or distance_field: the classes come from `region_cases.yardstick` (a walk of
the leaf list), the squared distances from scipy's Euclidean distance transform (its nearest-obstacle indices, so d2 is an
integer with no rounding; the ball dilation of reach_cases where scipy is missing), the costs from Jacobi sweeps of
shifted slices to the fixed point, and the parents from the definition.

`brick_model` is a numpy model of the device form's scheme — bricks of 8 x 8 x 8 voxels, each relaxed against a frozen
one-voxel halo for at most INNER iterations per round, neighbours of changed voxels (and of the seeds) activated for the
next round.  It
counts rounds and inner-cap hits from the yardstick's classes, so what the GPU tests expect of the diagnostics is never
taken from the code under test."""
import numpy as np

import region_cases as R
import frontier_cases as F
import reach_cases as RC

NONE = 0xFFFFFFFF
FAR = 0xFFFFFFFF
INF = np.int64(1) << 40              # "no cost" inside the yardstick: adding a move and a penalty cannot reach it
BRICK, INNER, BATCH = 8, 16, 8       # what the header must say (asserted by the tests)
CONNECTIVITIES = F.CONNECTIVITIES
FREE_M, OCC_M, UNK_M, MISS_M = F.FREE_M, F.OCC_M, F.UNK_M, F.MISS_M
SEED = RC.SEED
WEIGHTS = ((1, 1, 1), (10, 14, 17), (5, 7, 9))
PLAIN = dict(clearance=0, soft_radius=0, penalty=0)
SOFT = dict(clearance=1, soft_radius=4, penalty=40)
STATS = ("n_seeded", "n_reached", "max_cost")
flat = RC.flat
far_lo = RC.far_lo


def d2_of(cls, obstacle_mask, radius):
    """distance_field's d2 from the definition: the squared distance in voxels to the nearest voxel OF THE REGION with a
    class in obstacle_mask, FAR beyond radius^2"""
    obst = F.in_mask(cls, obstacle_mask)
    out = np.full(cls.shape, FAR, np.int64)
    if not obst.any():
        return out
    try:
        from scipy import ndimage
    except ImportError:
        for r2 in range(radius * radius, -1, -1):       # (slow path) the ball dilation at every squared radius, largest first
            near = _dilate(obst, r2)
            out[near] = np.minimum(out[near], r2)
        return out
    idx = ndimage.distance_transform_edt(~obst, return_distances=False, return_indices=True)
    grid = np.indices(cls.shape)
    d2 = ((idx.astype(np.int64) - grid) ** 2).sum(0)
    return np.where(d2 <= radius * radius, d2, FAR)


def _dilate(obst, r2):
    nx, ny, nz = obst.shape
    r = int(np.floor(np.sqrt(r2)))
    pad = np.zeros((nx + 2 * r, ny + 2 * r, nz + 2 * r), bool)
    pad[r:r + nx, r:r + ny, r:r + nz] = obst
    near = np.zeros(obst.shape, bool)
    for di in range(-r, r + 1):
        for dj in range(-r, r + 1):
            for dk in range(-r, r + 1):
                if di * di + dj * dj + dk * dk <= r2:
                    near |= pad[r + di:r + di + nx, r + dj:r + dj + ny, r + dk:r + dk + nz]
    return near


def entry_of(cls, pass_mask, obstacle_mask=OCC_M, clearance=0, soft_radius=0, penalty=0):
    """(open, pen): the passable voxels and their penalty, from the contract's formulas"""
    ok = F.in_mask(cls, pass_mask)
    pen = np.zeros(cls.shape, np.int64)
    radius = max(clearance, soft_radius)
    if radius > 0:
        d2 = d2_of(cls, obstacle_mask, radius)
        if clearance > 0:
            ok &= (d2 == FAR) | (d2 > clearance * clearance)
        s2 = soft_radius * soft_radius
        if s2 > 0:
            near = d2 <= s2
            pen[near] = penalty * (s2 - d2[near]) // s2
    return ok, pen


def _moves(connectivity, move_cost):
    """(offset, move cost, code q) in the order of q"""
    return [((di, dj, dk), int(move_cost[abs(di) + abs(dj) + abs(dk) - 1]), (di + 1) * 9 + (dj + 1) * 3 + (dk + 1))
            for di, dj, dk in F.offsets(connectivity)]


def _seeded(ok, seeds):
    mask = np.zeros(ok.shape, bool)
    for s in seeds:
        if 0 <= int(s) < ok.size and ok.reshape(-1)[int(s)]:
            mask.reshape(-1)[int(s)] = True
    return mask


def jacobi(ok, pen, seeds, connectivity, move_cost, max_cost):
    """costs (int64, INF where unreached) by Jacobi sweeps of shifted slices to the fixed point, and the number of sweeps
    that changed a voxel"""
    nx, ny, nz = ok.shape
    pad = np.full((nx + 2, ny + 2, nz + 2), INF, np.int64)
    cost = pad[1:-1, 1:-1, 1:-1]                                   # a view
    cost[_seeded(ok, seeds)] = 0
    kinds = {}                                                     # offsets by their move cost's index: one add per kind and sweep
    for di, dj, dk in F.offsets(connectivity):
        kinds.setdefault(abs(di) + abs(dj) + abs(dk) - 1, []).append((di, dj, dk))
    best, tmp = np.empty(ok.shape, np.int64), np.empty(ok.shape, np.int64)
    sweeps = 0
    while True:
        best[...] = INF
        for kind, offs in kinds.items():
            tmp[...] = INF
            for di, dj, dk in offs:
                np.minimum(tmp, pad[1 + di:1 + di + nx, 1 + dj:1 + dj + ny, 1 + dk:1 + dk + nz], out=tmp)
            tmp += int(move_cost[kind])
            np.minimum(best, tmp, out=best)
        best += pen
        better = ok & (best <= max_cost) & (best < cost)
        if not better.any():
            return cost.copy(), sweeps
        cost[better] = best[better]                                # (every candidate was read before: best is a copy)
        sweeps += 1


def parents_of(cost, pen, connectivity, move_cost):
    """the parent codes from the definition: the smallest q whose offset stays in the region and leads to a voxel u with a
    finite cost and cost[u] + move + pen(v) == cost[v]; 13 at cost 0, 255 where unreached"""
    nx, ny, nz = cost.shape
    pad = np.full((nx + 2, ny + 2, nz + 2), INF, np.int64)
    pad[1:-1, 1:-1, 1:-1] = cost
    parent = np.full(cost.shape, 255, np.uint8)
    parent[cost == 0] = 13
    todo = (cost != INF) & (cost != 0)
    for (di, dj, dk), mv, q in _moves(connectivity, move_cost):
        u = pad[1 + di:1 + di + nx, 1 + dj:1 + dj + ny, 1 + dk:1 + dk + nz]
        hit = todo & (u != INF) & (u + mv + pen == cost)
        parent[hit] = q
        todo &= ~hit
    assert not todo.any(), "every reached voxel that is no seed has a parent"
    return parent


_YARDSTICKS = {}


def yardstick(cls, seeds, pass_mask=FREE_M, obstacle_mask=OCC_M, clearance=0, soft_radius=0, penalty=0, move_cost=(10, 14, 17),
              connectivity=26, max_cost=1 << 31, targets=None, key=None):
    """`key` names the class array (a depth, say): the answer is then computed once per key and query and shared; nobody
    writes to it"""
    query = (key, tuple(int(s) for s in seeds), pass_mask, obstacle_mask, clearance, soft_radius, penalty, tuple(move_cost), connectivity, max_cost)
    if key is not None and query in _YARDSTICKS:
        out = dict(_YARDSTICKS[query])
    else:
        ok, pen = entry_of(cls, pass_mask, obstacle_mask, clearance, soft_radius, penalty)
        c, sweeps = jacobi(ok, pen, seeds, connectivity, move_cost, max_cost)
        fin = c != INF
        out = dict(cost=np.where(fin, c, NONE).astype(np.uint32), parent=parents_of(c, pen, connectivity, move_cost),
                   n_seeded=int(_seeded(ok, seeds).sum()), n_reached=int(fin.sum()), max_cost=int(c[fin].max()) if fin.any() else 0,
                   sweeps=sweeps, passable=int(ok.sum()), penalised=int((ok & (pen > 0)).sum()), pen=pen)
        if key is not None:
            _YARDSTICKS[query] = dict(out)
    if targets is not None:
        t = np.asarray(targets, np.int64)
        tc = np.full(t.size, NONE, np.uint32)
        inside = (t >= 0) & (t < cls.size)
        tc[inside] = out["cost"].reshape(-1)[t[inside]]
        out["target_cost"] = tc
    return out


def brick_model(ok, pen, seeds, connectivity, move_cost, max_cost=1 << 31, inner_cap=INNER):
    """The device form's scheme in numpy: dict(cost, rounds, brick_runs, capped, longest).  rounds = the rounds in which a
    voxel changed (the round that confirms the fixed point is not counted); capped = the brick runs whose inner_cap-th
    iteration still changed a voxel; longest = the most iterations in a row that changed a voxel of one brick run."""
    nx, ny, nz = ok.shape
    B = [(n + BRICK - 1) // BRICK for n in ok.shape]
    G = np.full([b * BRICK + 2 for b in B], INF, np.int64)             # the bricks, padded by the halo of the outermost ones
    inner = G[1:-1, 1:-1, 1:-1]
    open_ = np.zeros(inner.shape, bool)
    open_[:nx, :ny, :nz] = ok
    P = np.zeros(inner.shape, np.int64)
    P[:nx, :ny, :nz] = pen
    seeded = np.zeros(inner.shape, bool)
    seeded[:nx, :ny, :nz] = _seeded(ok, seeds)
    inner[seeded] = 0
    tiles = np.lib.stride_tricks.sliding_window_view(G, (10, 10, 10))[::8, ::8, ::8]       # [BX, BY, BZ, 10, 10, 10], a view of G
    bricks = lambda a: a.reshape(B[0], 8, B[1], 8, B[2], 8).transpose(0, 2, 4, 1, 3, 5)    # noqa: E731  [BX, BY, BZ, 8, 8, 8], a view
    open_b, pen_b = bricks(open_), bricks(P)
    moves = _moves(connectivity, move_cost)
    active = np.zeros(B, bool)
    for i, j, k in np.argwhere(seeded):                                 # a seed's own brick and the bricks that touch the seed
        active[i // 8, j // 8, k // 8] = True
        for (di, dj, dk), _, _ in moves:
            if all(d == 0 or v % 8 == (0 if d < 0 else 7) for d, v in zip((di, dj, dk), (i, j, k))):
                qi, qj, qk = i // 8 + di, j // 8 + dj, k // 8 + dk
                if 0 <= qi < B[0] and 0 <= qj < B[1] and 0 <= qk < B[2]:
                    active[qi, qj, qk] = True
    rounds = brick_runs = capped = longest = 0
    while active.any():
        at = np.argwhere(active)
        bi, bj, bk = at[:, 0], at[:, 1], at[:, 2]
        T = tiles[bi, bj, bk].copy()                                    # this round's inputs: every halo as the round found it
        o, p = open_b[bi, bj, bk], pen_b[bi, bj, bk]
        running = np.ones(len(at), bool)                               # bricks whose every iteration so far changed a voxel
        ever = np.zeros(o.shape, bool)
        brick_runs += len(at)
        for it in range(1, inner_cap + 1):
            cur = T[:, 1:9, 1:9, 1:9]                                   # a view
            best = np.full(cur.shape, INF, np.int64)
            for (di, dj, dk), mv, _q in moves:
                np.minimum(best, T[:, 1 + di:9 + di, 1 + dj:9 + dj, 1 + dk:9 + dk] + mv, out=best)
            best += p
            changed = o & (best <= max_cost) & (best < cur) & running[:, None, None, None]
            cur[changed] = best[changed]                                # (Jacobi: every candidate was computed before)
            ever |= changed
            running &= changed.any(axis=(1, 2, 3))
            if not running.any():
                break
            longest = max(longest, it)
        hit_cap = running                                               # the last allowed iteration still changed a voxel
        capped += int(hit_cap.sum())
        nxt = np.zeros_like(active)
        wrote = ever.any(axis=(1, 2, 3))
        for n in np.flatnonzero(wrote):
            i, j, k = at[n]
            G[1 + 8 * i:9 + 8 * i, 1 + 8 * j:9 + 8 * j, 1 + 8 * k:9 + 8 * k] = T[n, 1:9, 1:9, 1:9]
            if hit_cap[n]:
                nxt[i, j, k] = True
            for (di, dj, dk), _, _ in moves:
                sel = tuple(slice(None) if d == 0 else (0 if d < 0 else 7) for d in (di, dj, dk))
                qi, qj, qk = i + di, j + dj, k + dk
                if 0 <= qi < B[0] and 0 <= qj < B[1] and 0 <= qk < B[2] and ever[n][sel].any():
                    nxt[qi, qj, qk] = True
        if wrote.any():
            rounds += 1
        active = nxt
    return dict(cost=inner[:nx, :ny, :nz].copy(), rounds=rounds, brick_runs=brick_runs, capped=capped, longest=longest)


_CONDITIONS = {}


def input_conditions(cls, seed, key=None):
    """counted from the yardstick's classes, never from the code under test.  `key` caches the answer (a depth)"""
    if key is not None and key in _CONDITIONS:
        return _CONDITIONS[key]
    unit = yardstick(cls, [seed], move_cost=(1, 1, 1), connectivity=6, key=key)
    soft = yardstick(cls, [seed], connectivity=26, key=key, **SOFT)
    hard = yardstick(cls, [seed], connectivity=26, clearance=1, key=key)         # the same passable set without the penalty
    both = (soft["cost"] != NONE) & (hard["cost"] != NONE)
    moved = int((both & (soft["pen"] == 0) & (soft["cost"].astype(np.int64) > hard["cost"].astype(np.int64))).sum())
    out = dict(seed_free=bool(cls.reshape(-1)[seed] == R.FREE),
               unit=dict(reached=unit["n_reached"], sweeps=unit["sweeps"]),
               soft=dict(reached=soft["n_reached"], passable=soft["passable"], penalised=soft["penalised"], sweeps=soft["sweeps"]),
               moved=moved, model={})
    for name, y, kw in (("unit", unit, dict(connectivity=6, move_cost=(1, 1, 1))), ("soft", soft, dict(connectivity=26, move_cost=(10, 14, 17), **SOFT))):
        ok, pen = entry_of(cls, FREE_M, OCC_M, kw.get("clearance", 0), kw.get("soft_radius", 0), kw.get("penalty", 0))
        m = brick_model(ok, pen, [seed], kw["connectivity"], kw["move_cost"])
        assert (np.where(m["cost"] == INF, NONE, m["cost"]).astype(np.uint32) == y["cost"]).all(), "the brick model gives the Jacobi costs"
        out["model"][name] = {k: m[k] for k in ("rounds", "brick_runs", "capped")}
    if key is not None:
        _CONDITIONS[key] = out
    return out


def assert_exercises_the_feature(cond):
    """At least half of what was counted on region_cases.fused_map(3), FREE passable, OCCUPIED obstacles, seed (40, 41, 15):
    unit weights at connectivity 6 reach 16 818 voxels in 92 sweeps; 10 / 14 / 17 at connectivity 26 with clearance 1, soft
    radius 4 and penalty 40 reach 14 748 of 14 756 passable voxels, 8 659 of them penalised; the penalty raises the cost of
    at least 2 900 voxels whose own penalty is 0 (5 825 counted): paths moved; the brick model needs more rounds than one
    batch and at least one brick run stops at the inner cap.  Counted with this file's model (Jacobi iterations inside a
    brick, as the kernel runs them): 12 rounds that change a voxel, and a thirteenth that confirms, for both queries; the
    unit-weight query at connectivity 6 has 6 capped runs of 292; the connectivity-26 query has none of 695 — the wave
    crosses a brick in fewer than 16 diagonal iterations there — so the cap is expected where the model counts it"""
    print(f"travel input conditions: {cond}")
    assert cond["seed_free"], cond
    assert cond["unit"]["reached"] >= 8409 and cond["unit"]["sweeps"] >= 46, cond
    assert cond["soft"]["reached"] >= 7374 and cond["soft"]["passable"] >= 7378 and cond["soft"]["penalised"] >= 4330, cond
    assert cond["moved"] >= 2900, cond
    assert all(m["rounds"] > BATCH for m in cond["model"].values()), cond
    assert any(m["capped"] >= 1 for m in cond["model"].values()), cond


def closed_form(dims, seed_ijk, connectivity, move_cost):
    """costs on an open box from one seed, |d| sorted x >= y >= z: c z + b (y - z) + a (x - y) at connectivity 26 when the
    diagonals pay (b <= 2a, c <= a + b, c + a <= 2b, as for 10 / 14 / 17, 5 / 7 / 9 and 1 / 1 / 1); a (x + y + z) at connectivity 6"""
    a, b, c = (int(v) for v in move_cost)
    d = np.stack(np.meshgrid(*[np.abs(np.arange(n, dtype=np.int64) - s) for n, s in zip(dims, seed_ijk)], indexing="ij"), -1)
    d = np.sort(d, -1)
    z, y, x = d[..., 0], d[..., 1], d[..., 2]
    if connectivity == 6:
        return (a * (x + y + z)).astype(np.uint32)
    assert connectivity == 26 and b <= 2 * a and c <= a + b and c + a <= 2 * b
    return (c * z + b * (y - z) + a * (x - y)).astype(np.uint32)


def walk(parent, dims, index):
    """the path from `index` through the parent codes: flat indices and the code followed at each, the seed last"""
    par = parent.reshape(-1)
    f, path = int(index), []
    while True:
        q = int(par[f])
        assert q != 255 and len(path) <= par.size, (index, f, q)
        path.append((f, q))
        if q == 13:
            return path
        f += ((q // 9 - 1) * dims[1] + ((q // 3) % 3 - 1)) * dims[2] + (q % 3 - 1)


def assert_same(got, want, what, fields=("cost", "parent", "target_cost") + STATS):
    for k in STATS:
        if k in fields:
            assert got[k] == want[k], (what, k, got[k], want[k])
    R.assert_same(got, want, [k for k in ("cost", "parent", "target_cost") if k in fields and k in want and k in got], what)
