"""The yardstick, the hand-built member sets and the input conditions shared by tests/test_drive_cpu.py and
tests/test_drive_gpu.py.

The yardstick never calls drive, travel or footing.  It is written from the contract comment above la3dm_devmap_drive_host
(include/la3dm_hip.h): the members are a boolean array, the edges of every allowed offset are a pair of shifted slices,
the costs come from scipy.sparse.csgraph.dijkstra run from a virtual source that is joined to the seeded members (integer
weights below 2^53 are exact in float64: the result is asserted to be integral), the cut is at max_cost, the parents are
the smallest code q from the costs alone, and snap is an argmax over a slice of a column.  Every comparison is exact."""
import numpy as np

import region_cases as R
import footing_cases as F

NONE = 0xFFFFFFFF
SEED_CODE = 40
MAX_STEP, MAX_SNAP, MAX_MOVE, MAX_COST = 4, 32, 1 << 16, 1 << 31
BRICK, INNER, BATCH = 8, 16, 8       # what the header must say (asserted by the tests)
INF = np.int64(1) << 40
STATS = ("n_members", "n_seeded", "n_reached", "max_cost")
FIELDS = ("cost", "parent", "of_member", "target_cost", "target_index")
DEFAULTS = dict(connectivity=8, step=1, snap=0, move_cost=(10, 14), climb_up=0, climb_down=0, max_cost=MAX_COST)


def flat(dims, i, j, k):
    return (int(i) * dims[1] + int(j)) * dims[2] + int(k)


def offsets(connectivity, step):
    """the allowed offsets (a, b, c) in the order of their code"""
    assert connectivity in (4, 8) and 0 <= step <= MAX_STEP
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in range(-step, step + 1)
            if 1 <= abs(a) + abs(b) <= (1 if connectivity == 4 else 2)]


def code(a, b, c):
    return ((a + 1) * 3 + (b + 1)) * 9 + (c + 4)


def move(a, b, c, move_cost, climb_up, climb_down):
    """what the move along (a, b, c) costs"""
    return int(move_cost[abs(a) + abs(b) - 1]) + (int(climb_up) * c if c > 0 else int(climb_down) * -c)


def _slices(n, d):
    """(from, to) slices of an axis of n for a move by d: u = from, v = u + d = to"""
    return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))


def snapped(member, snap, f):
    """the flat index of the member that f stands for, or NONE"""
    dims = member.shape
    f = int(f)
    if not 0 <= f < member.size:
        return NONE
    i, j, k = f // (dims[1] * dims[2]), (f // dims[2]) % dims[1], f % dims[2]
    low = max(0, k - snap)
    col = member[i, j, low:k + 1][::-1]                      # from k downwards
    return f - int(col.argmax()) if col.any() else NONE


def members_of(dims, index):
    """the member array of a list: an index out of range is ignored, a voxel listed twice counts once"""
    m = np.zeros(dims, bool)
    idx = np.asarray(index, np.int64).reshape(-1)
    m.reshape(-1)[idx[(idx >= 0) & (idx < m.size)]] = True
    return m


def costs_of(member, seeded, connectivity, step, move_cost, climb_up, climb_down, max_cost):
    """int64 costs, INF where there is none: Dijkstra from a virtual source over the edges of shifted slices"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    n = member.size
    ids = np.arange(n, dtype=np.int64).reshape(member.shape)
    rows, cols, w = [], [], []
    for a, b, c in offsets(connectivity, step):
        (ui, vi), (uj, vj), (uk, vk) = (_slices(m, d) for m, d in zip(member.shape, (a, b, c)))
        both = member[ui, uj, uk] & member[vi, vj, vk]
        rows.append(ids[ui, uj, uk][both])
        cols.append(ids[vi, vj, vk][both])
        w.append(np.full(int(both.sum()), move(a, b, c, move_cost, climb_up, climb_down), np.float64))
    s = np.flatnonzero(seeded.reshape(-1))
    rows.append(np.full(s.size, n, np.int64))                 # the virtual source; its edges weigh 1 (csgraph drops a 0), taken off below
    cols.append(s)
    w.append(np.ones(s.size))
    g = csr_matrix((np.concatenate(w), (np.concatenate(rows), np.concatenate(cols))), shape=(n + 1, n + 1))
    d = dijkstra(g, directed=True, indices=n)[:n]
    fin = np.isfinite(d)
    assert (d[fin] == np.floor(d[fin])).all() and (d[fin] < 2.0 ** 53).all(), "integer weights: an integral answer"
    cost = np.full(n, INF, np.int64)
    cost[fin] = d[fin].astype(np.int64) - 1
    cost[cost > max_cost] = INF                                 # the cut
    return cost.reshape(member.shape)


def parents_of(cost, connectivity, step, move_cost, climb_up, climb_down):
    """the parent codes from the costs alone (a finite cost: a member): the smallest q whose offset o = u - v leads to a voxel
    u of the region with a finite cost and cost[u] + move(u -> v) == cost[v]; 40 at cost 0, 255 where there is no cost"""
    nx, ny, nz = cost.shape
    pad = np.full((nx + 2, ny + 2, nz + 2 * MAX_STEP), INF, np.int64)
    pad[1:-1, 1:-1, MAX_STEP:-MAX_STEP] = cost
    parent = np.full(cost.shape, 255, np.uint8)
    parent[cost == 0] = SEED_CODE
    todo = (cost != INF) & (cost != 0)
    for a, b, c in offsets(connectivity, step):                   # o = (a, b, c); the move u -> v is -o
        u = pad[1 + a:1 + a + nx, 1 + b:1 + b + ny, MAX_STEP + c:MAX_STEP + c + nz]
        hit = todo & (u != INF) & (u + move(-a, -b, -c, move_cost, climb_up, climb_down) == cost)
        parent[hit] = code(a, b, c)
        todo &= ~hit
    assert not todo.any(), "every reached member that is no seed has a parent"
    return parent


def yardstick(member, seeds, targets=None, members=None, connectivity=8, step=1, snap=0, move_cost=(10, 14), climb_up=0, climb_down=0,
              max_cost=MAX_COST):
    """drive over the boolean member array; `members` = the list, for of_member"""
    seeded = np.zeros(member.shape, bool)
    for s in np.asarray(seeds, np.int64).reshape(-1):
        f = snapped(member, snap, s)
        if f != NONE:
            seeded.reshape(-1)[f] = True
    c = costs_of(member, seeded, connectivity, step, move_cost, climb_up, climb_down, max_cost)
    fin = c != INF
    cost = np.where(fin, c, NONE).astype(np.uint32)
    out = dict(cost=cost, parent=parents_of(c, connectivity, step, move_cost, climb_up, climb_down), n_members=int(member.sum()),
               n_seeded=int(seeded.sum()), n_reached=int(fin.sum()), max_cost=int(c[fin].max()) if fin.any() else 0)
    if targets is not None:
        ti = np.array([snapped(member, snap, t) for t in np.asarray(targets, np.int64).reshape(-1)], np.int64).reshape(-1)
        tc = np.full(ti.size, NONE, np.uint32)
        tc[ti != NONE] = cost.reshape(-1)[ti[ti != NONE]]
        out.update(target_cost=tc, target_index=ti.astype(np.uint32))
    if members is not None:
        idx = np.asarray(members, np.int64).reshape(-1)
        om = np.full(idx.size, NONE, np.uint32)
        inside = (idx >= 0) & (idx < member.size)
        om[inside] = cost.reshape(-1)[idx[inside]]
        out["of_member"] = om
    return out


def assert_same(got, want, what, fields=FIELDS + STATS):
    for k in STATS:
        if k in fields and k in got:
            assert got[k] == want[k], (what, k, got[k], want[k])
    R.assert_same(got, want, [k for k in FIELDS if k in fields and k in want and k in got], what)


def walk(y, member, dims, index, connectivity, step, move_cost, climb_up, climb_down):
    """Follows the parents from `index` to a seed: every step is an allowed move between members and strictly lowers the cost,
    the walk ends on code 40, and the moves sum to cost[index].  Returns the flat indices, `index` first."""
    cost, par, mem = y["cost"].reshape(-1).astype(np.int64), y["parent"].reshape(-1), member.reshape(-1)
    allowed = set(offsets(connectivity, step))
    f, path, total = int(index), [], 0
    while True:
        q = int(par[f])
        assert q != 255 and mem[f] and len(path) <= par.size, (index, f, q)
        path.append(f)
        if q == SEED_CODE:
            assert cost[f] == 0 and total == cost[int(index)], (index, total, cost[int(index)])
            return path
        assert q <= 80, q
        o = (q // 27 - 1, (q // 9) % 3 - 1, q % 9 - 4)
        assert (-o[0], -o[1], -o[2]) in allowed, (index, f, o)
        i, j, k = f // (dims[1] * dims[2]) + o[0], (f // dims[2]) % dims[1] + o[1], f % dims[2] + o[2]
        assert 0 <= i < dims[0] and 0 <= j < dims[1] and 0 <= k < dims[2], (index, f, o)
        u = flat(dims, i, j, k)
        mv = move(-o[0], -o[1], -o[2], move_cost, climb_up, climb_down)
        assert mem[u] and cost[u] != NONE and cost[u] + mv == cost[f] and cost[u] < cost[f], (index, f, u, cost[u], mv, cost[f])
        total += mv
        f = u


def climbs(y):
    """reached members whose parent lies at another height: moves with c != 0 on least-cost walks"""
    p = y["parent"]
    return int(((p != 255) & (p != SEED_CODE) & (p % 9 != 4)).sum())


# ---- the hand-built member sets ---------------------------------------------------------------------------------------------
FLOOR_DIMS = (17, 17, 9)              # 3 x 3 x 2 bricks with ragged edges


def flat_floor():
    m = np.zeros(FLOOR_DIMS, bool)
    m[:, :, 3] = True
    return m


def floor_closed_form(dims, seed_ij, k, connectivity, move_cost):
    """costs on a flat floor at height k from one seed: octile distance at connectivity 8 (the diagonal pays: move_cost[1] <= 2
    move_cost[0]), Manhattan at connectivity 4"""
    a, b = (int(v) for v in move_cost)
    dx = np.abs(np.arange(dims[0], dtype=np.int64) - seed_ij[0])[:, None]
    dy = np.abs(np.arange(dims[1], dtype=np.int64) - seed_ij[1])[None, :]
    if connectivity == 4:
        layer = a * (dx + dy)
    else:
        assert b <= 2 * a
        layer = b * np.minimum(dx, dy) + a * np.abs(dx - dy)
    out = np.full(dims, NONE, np.uint32)
    out[:, :, k] = layer
    return out


STAIR_COLUMNS = 5


def stairs(rise):
    """single-column stairs: STAIR_COLUMNS members along x at j = 1, each `rise` voxels above the one before; returns (dims,
    members, the flat indices of the bottom and the top member)"""
    dims = (STAIR_COLUMNS, 3, (STAIR_COLUMNS - 1) * rise + 1)
    m = np.zeros(dims, bool)
    for i in range(STAIR_COLUMNS):
        m[i, 1, i * rise] = True
    return dims, m, flat(dims, 0, 1, 0), flat(dims, STAIR_COLUMNS - 1, 1, (STAIR_COLUMNS - 1) * rise)


LINK_DIMS = (17, 17, 16)
# (member, member, step, connectivity): each pair is the only connection between seed and target and crosses a brick border,
# so a brick that is not woken leaves NONE
LINKS = (((3, 3, 7), (4, 3, 9), 2, 4),       # the brick straight above, reached by a move that stays inside the brick's columns
         ((3, 3, 8), (4, 3, 4), 4, 4),       # the brick straight below, four levels down
         ((7, 7, 7), (8, 8, 11), 4, 8),      # the corner brick, four levels up
         ((7, 3, 0), (8, 3, 0), 0, 4),       # step 0: a face neighbour in x
         ((0, 8, 3), (1, 7, 7), 4, 8),       # across the y face and the z face at once
         ((7, 7, 7), (8, 7, 7), 1, 4))       # a seed on a brick face whose only neighbour is in the next brick


def link(a, b):
    m = np.zeros(LINK_DIMS, bool)
    m[a] = m[b] = True
    return m


SHELF_DIMS = (9, 9, 8)
SHELF_STEP = 2


def shelf(ramp):
    """a floor at k = 2 and a shelf at k = 6 over the columns i >= 4: one column holds both.  They are not joined at step 2;
    with the ramp member (3, 0, 4) they are: (2, 0, 2) -> (3, 0, 4) -> (4, 0, 6)"""
    m = np.zeros(SHELF_DIMS, bool)
    m[:, :, 2] = True
    m[4:, :, 6] = True
    if ramp:
        m[3, 0, 4] = True
    return m


def serpentine(nx):
    """a one-voxel-wide path at connectivity 4 in (nx, 8, 8) at k = 0: the rows j = 0, 2, 4, 6 joined at alternating ends;
    returns (dims, members, the flat index of its first and of its last member, the moves between them)"""
    dims = (nx, 8, 8)
    m = np.zeros(dims, bool)
    m[:, 0::2, 0] = True
    for t, j in enumerate((1, 3, 5)):
        m[nx - 1 if t % 2 == 0 else 0, j, 0] = True
    return dims, m, flat(dims, 0, 0, 0), flat(dims, 0, 6, 0), 4 * (nx - 1) + 6


EDGE_DIMS = ((1, 1, 1), (1, 64, 1), (8, 8, 1), (9, 8, 8))


def random_members(dims, seed, density=0.35):
    rng = np.random.default_rng(seed)
    return rng.random(dims) < density


# ---- the two-scan map -----------------------------------------------------------------------------------------------------
def input_conditions(y):
    """counted from the yardstick, never from the code under test"""
    return dict(members=y["n_members"], seeded=y["n_seeded"], reached=y["n_reached"], unreached=y["n_members"] - y["n_reached"],
                climbs=climbs(y))


def assert_exercises_the_feature(cond, least):
    """the feature is exercised: there are members, the wave leaves the seeds, some members stay unreached, and least-cost walks
    change height; and at least `least` of each figure (half of what was counted when the test was written)"""
    print(f"drive input conditions: {cond}")
    assert cond["members"] > 0 and cond["reached"] > cond["seeded"] > 0 and cond["unreached"] > 0 and cond["climbs"] >= 1, cond
    for k, v in least.items():
        assert cond[k] >= v, (k, cond)


# ---- refusals: the contract's order, each with every later defect present -----------------------------------------------------
REFUSAL_DIMS = (9, 8, 8)
ERR_ARG = -1


def refusal_chain(call, put, room):
    """call(lo, dims, seeds, n_seeds, params, targets, n_targets, out) -> (rc, text) with pointers as integers or None, params a
    _lib.DriveParams or None, out a _lib.DriveOut or None; put(array) -> the address of a copy where the call reads it (host or
    device memory); room(name, n, dtype) -> the address of an output array of n elements that the caller fills with a sentinel
    and checks afterwards.  Starts with every defect of the contract's list present and mends them one by one in its order;
    every call but the last is refused with the text of the first defect left.  The last call is served, at the limit values.
    Returns what the served call was given: (members, seeds, targets, params as a dict)."""
    import ctypes as C
    from la3dm_amd import _lib
    dims = REFUSAL_DIMS
    n = dims[0] * dims[1] * dims[2]
    member = random_members(dims, 11, 0.5)
    index = np.flatnonzero(member.reshape(-1)).astype(np.uint32)
    seeds = np.array([index[0], n + 5], np.uint32)
    targets = np.array([index[-1], n], np.uint32)
    lo = np.array((0.05, 0.05, 0.05), np.float32)
    d_ok, d_zero, d_big = np.array(dims, np.uint32), np.array((9, 0, 8), np.uint32), np.array((1 << 10, 1 << 10, 257), np.uint32)
    fp = _lib.FootingParams(2, 1, 2, 0, 0, 0)
    s = dict(lo=None, dims=None, seeds=None, n_seeds=(1 << 20) + 1, targets=None, n_targets=(1 << 28) + 1, params=False, members=None,
             footing=C.pointer(fp), n_members=(1 << 28) + 1, connectivity=5, step=5, snap=33, move=[0, 70000], up=65537, down=65537,
             max_cost=(1 << 31) + 1, out=None)
    keep = [lo, d_ok, d_zero, d_big, fp]

    def attempt():
        p = None
        if s["params"]:
            p = _lib.DriveParams(s["members"], s["footing"], s["n_members"], s["connectivity"], s["step"], s["snap"], (C.c_uint32 * 2)(*s["move"]),
                                 s["up"], s["down"], s["max_cost"])
        return call(s["lo"], s["dims"], s["seeds"], s["n_seeds"], p, s["targets"], s["n_targets"], s["out"])
    cost, parent = room("cost", n, np.uint32), room("parent", n, np.uint8)
    tcost, tindex = room("target_cost", 2, np.uint32), room("target_index", 2, np.uint32)
    steps = (
        ("params is NULL", dict(params=True)),
        ("connectivity must be 4 or 8", dict(connectivity=8)),
        ("step must not exceed", dict(step=4)),
        ("snap must not exceed", dict(snap=32)),
        ("move_cost", dict(move=[1 << 16, 70000])),
        ("move_cost", dict(move=[1 << 16, 1 << 16])),
        ("climb_up", dict(up=1 << 16)),
        ("climb_down", dict(down=1 << 16)),
        ("max_cost must lie", dict(max_cost=1 << 31)),
        ("n_members: more than", dict(n_members=int(index.size))),
        ("n_seeds: more than", dict(n_seeds=2)),
        ("n_targets: more than", dict(n_targets=2)),
        ("seeds is NULL", dict(seeds=put(seeds))),
        ("targets is NULL", dict(targets=put(targets))),
        ("members is NULL", dict(members=put(index))),
        ("footing and members are both set", dict(footing=None)),
        ("out is NULL", dict(out=_lib.DriveOut(None, parent, None, None, tindex))),
        ("target_cost must not be NULL", dict(out=_lib.DriveOut(cost, parent, None, None, tindex))),
        ("target_cost must not be NULL with n_targets > 0", dict(out=_lib.DriveOut(cost, parent, None, tcost, tindex))),
        ("lo is NULL", dict(lo=lo.ctypes.data)),
        ("dims is NULL", dict(dims=d_zero.ctypes.data)),
        ("dims must be >= 1", dict(dims=d_big.ctypes.data)),
        ("LA3DM_DRIVE_MAX_CELLS", None),
    )
    for text, mend in steps:
        rc, msg = attempt()
        assert rc == ERR_ARG and text in msg, (text, rc, msg)
        if mend:
            s.update(mend)
    # single defects on an otherwise valid call
    s["dims"] = d_ok.ctypes.data
    good = dict(s)
    om = room("of_member", int(index.size), np.uint32)
    bad_fp = _lib.FootingParams(2, 1, 2, 0, 5, 0)
    deep = _lib.FootingParams(2, 1, 4, 2, 1, 6)
    d_pad = np.array(((1 << 10) - 4, (1 << 10) - 4, (1 << 8) - 5), np.uint32)   # whole bricks hold 2^28, footing's padded box one more
    keep += [bad_fp, deep, d_pad]
    for text, change in (
            ("max_cost must lie", dict(max_cost=0)),
            ("both NULL", dict(members=None, n_members=0)),
            ("of_member is set in footing mode", dict(members=None, n_members=0, footing=C.pointer(fp), out=_lib.DriveOut(cost, None, om, tcost, None))),
            ("of_member is set with n_members = 0", dict(n_members=0, out=_lib.DriveOut(cost, None, om, tcost, None))),
            ("target_cost is set with n_targets = 0", dict(n_targets=0)),
            ("target_index is set with n_targets = 0", dict(n_targets=0, out=_lib.DriveOut(cost, None, None, None, tindex))),
            ("step must not exceed LA3DM_FOOTING_MAX_STEP", dict(members=None, n_members=0, footing=C.pointer(bad_fp))),
            ("LA3DM_FOOTING_MAX_CELLS", dict(members=None, n_members=0, footing=C.pointer(deep), dims=d_pad.ctypes.data))):
        s.clear()
        s.update(good, **change)
        rc, msg = attempt()
        assert rc == ERR_ARG and text in msg, (text, rc, msg)
    s.clear()
    s.update(good)
    return attempt, member, index, seeds, targets, dict(connectivity=8, step=4, snap=32, move_cost=(1 << 16, 1 << 16), climb_up=1 << 16,
                                                        climb_down=1 << 16, max_cost=1 << 31), keep


# ---- footing's hand-built scene and the two-scan map: queries over one or several maps that must all agree ------------------------
def scene_query(maps, clear, h, r, s, c, seeds, targets, **kw):
    """drive over the scene in footing mode and over footing's own list: the two are equal, and equal the yardstick over the
    foot voxels of footing's yardstick.  Returns (the yardstick's answer, the member array)."""
    foot = F.yardstick(F.scene_padded(h, r, s), F.SCENE_DIMS, F.OCC_M, clear, h, r, s, c)["foot"]
    want = yardstick(foot, seeds, targets=targets, **kw)
    fkw = dict(support=F.OCC_M, clear=clear, headroom=h, radius=r, step=s, min_support=c)
    for m in maps:
        a = m.drive(F.SCENE_LO, F.SCENE_DIMS, seeds, footing=fkw, targets=targets, fields=("cost", "parent", "target_index"), **kw)
        lst = m.footing(F.SCENE_LO, F.SCENE_DIMS, **fkw)["index"]
        b = m.drive(F.SCENE_LO, F.SCENE_DIMS, seeds, members=lst, targets=targets, fields=("cost", "parent", "target_index"), **kw)
        assert_same(a, want, ("scene, footing mode", clear, h, r, s, c, kw))
        assert_same(b, want, ("scene, list mode", clear, h, r, s, c, kw))
    return want, foot


def scene_named_voxels(maps):
    """the issue's named voxels of footing's scene (floor: stand at k = 2; kerb from i = 12: k = 3; step from i = 18: k = 5; table
    over 2 .. 5 x 2 .. 5: under it k = 2, its top k = 6; pillar at (9, 9); hole over 2 .. 4 x 14 .. 16; a missing block over i,
    j >= 16 from k = 8)"""
    dims, free = F.SCENE_DIMS, F.FREE_M
    f = lambda i, j, k: flat(dims, i, j, k)   # noqa: E731
    seed = [f(7, 12, 4)]                        # two voxels above the floor: snap
    targets = [f(13, 12, 3), f(19, 4, 5), f(3, 3, 2), f(3, 3, 6), f(3, 15, 2), f(20, 20, 5)]
    res = {}
    for step in range(5):
        y, foot = scene_query(maps, free, 3, 0, 0, 0, seed, targets, step=step, snap=2, climb_up=4, climb_down=1)
        res[step] = y["target_cost"]
        assert y["n_seeded"] == 1 and y["cost"][7, 12, 2] == 0
        assert foot[3, 3, 2] and foot[3, 3, 6] and not foot[2:5, 14:17, :].any()
    # across the kerb at step 1 and not at step 0
    assert res[0][0] == NONE and res[1][0] != NONE
    # up the two-voxel step at step 2 only
    assert res[1][1] == NONE and res[2][1] != NONE
    # under the table at h = 3 (and not a member at h = 4)
    assert all(res[s][2] != NONE for s in range(5))
    y4, foot4 = scene_query(maps, free, 4, 0, 0, 0, seed, targets, step=1, snap=2)
    assert not foot4[3, 3, 2] and y4["target_cost"][2] == NONE
    # the table top, four voxels above the floor beside it, is not reached below step 4: there is no ramp
    assert all(res[s][3] == NONE for s in range(4)) and res[4][3] != NONE
    # nothing stands over the hole, and the floor round it is reached
    assert all(res[s][4] == NONE for s in range(5)) and scene_query(maps, free, 3, 0, 0, 0, seed, [f(5, 14, 2)], step=0, snap=2)[0]["target_cost"][0] != NONE
    # under the missing block the body needs MISSING in the clear mask at h = 8
    y, foot = scene_query(maps, free, 8, 0, 0, 0, seed, [f(20, 20, 5)], step=2, snap=2)
    assert not foot[20, 20, 5] and y["target_cost"][0] == NONE
    y, foot = scene_query(maps, F.OPTIMISTIC, 8, 0, 0, 0, seed, [f(20, 20, 5)], step=2, snap=2)
    assert foot[20, 20, 5] and y["target_cost"][0] != NONE
    # with a footprint: r = 2, s = 1, half the disc carried
    scene_query(maps, free, 4, 2, 1, 6, seed, targets, step=1, snap=2, connectivity=4, climb_up=3)


RECIPE_KW = dict(connectivity=8, step=1, snap=4, move_cost=(10, 14), climb_up=5, climb_down=2)
RECIPE_SUPPORT = 0      # min_support: an unobstructed body is enough on this sparsely observed floor
# counted from the yardstick on region_cases.fused_map(depth) over the recipe region when this test was written (2 seeds; the
# members lie in the layers k = 15 .. 18 and 25 .. 38); asserted at half, the margin the other region tests use
RECIPE_COUNTED = {3: dict(members=694, reached=155, unreached=539, climbs=51), 4: dict(members=688, reached=103, unreached=585, climbs=43)}


def recipe_case(m, lv, lo, dims, offset=(0, 0, 0), sub=None):
    """(lo, members, seeds, targets) of the recipe region or of its sub-box: the members are footing's yardstick over the classes
    of region_cases.yardstick, the seeds two voxels above the first and the middle member (snap finds the ground), the targets
    every 97th voxel"""
    q = F.RECIPE
    res = np.float32(m.get_resolution())
    sub = dims if sub is None else sub
    origin0 = R.yardstick(m, lv, lo, (1, 1, 1))["origin"]
    slo = (origin0 + np.array(offset, np.float32) * res).astype(np.float32)
    _, p = F.padded_case(m, lv, slo, sub, q["h"], q["r"], q["s"])
    foot = F.yardstick(p, sub, q["support"], q["clear"], q["h"], q["r"], q["s"], RECIPE_SUPPORT)["foot"]
    idx = np.flatnonzero(foot.reshape(-1))
    seeds = [int(f) + min(2, sub[2] - 1 - int(f) % sub[2]) for f in (idx[[0, idx.size // 2]] if idx.size else [])] or [0]
    return slo, foot, np.array(seeds, np.uint32), np.arange(0, foot.size, 97, dtype=np.uint32)


def recipe_queries(maps, slo, foot, seeds, targets, what):
    """footing mode == list mode == yardstick over one region; returns the yardstick's answer"""
    q = F.RECIPE
    fkw = dict(support=q["support"], clear=q["clear"], headroom=q["h"], radius=q["r"], step=q["s"], min_support=RECIPE_SUPPORT)
    want = yardstick(foot, seeds, targets=targets, **RECIPE_KW)
    lst = np.flatnonzero(foot.reshape(-1)).astype(np.uint32)
    want_list = yardstick(foot, seeds, targets=targets, members=lst, **RECIPE_KW)
    for m in maps:
        a = m.drive(slo, foot.shape, seeds, footing=fkw, targets=targets, fields=("cost", "parent", "target_index"), **RECIPE_KW)
        assert_same(a, want, (what, "footing mode"))
        b = m.drive(slo, foot.shape, seeds, members=lst, targets=targets, fields=("cost", "parent", "of_member", "target_index"), **RECIPE_KW)
        assert_same(b, want_list, (what, "list mode"))
    return want


# (offset, dims) of sub-regions of the recipe region (80, 80, 40), one against each of its faces
FACE_BOXES = (((0, 3, 2), (43, 70, 30)), ((37, 3, 2), (43, 70, 30)), ((5, 0, 2), (70, 43, 30)), ((5, 37, 2), (70, 43, 30)),
              ((5, 3, 0), (70, 70, 20)), ((5, 3, 20), (70, 70, 20)))
