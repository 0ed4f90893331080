"""The comparisons shared by tests/test_pool_queries_cpu.py and tests/test_pool_queries_gpu.py: every function takes a map
loaded from a case of pool_cases.py (any map mode) and compares one query with its numpy yardstick on the expander's classes.
Integers by ==, floats by their bits; no tolerance anywhere.  `pool` = (keys, A, B, S) replaces the case's pool where the map
was changed after it was loaded."""
import numpy as np

import clusters_cases as CL
import distance_cases as D
import footing_cases as FT
import frontier_cases as F
import gain_cases as G
import nearest_cases as N
import pool_cases as PC
import raycast_cases as RC
import reach_cases as RE
import region_cases as R
import surface_cases as SF
import travel_cases as T

SHAPES = ((1, 1, 1), (1, 1, 3), (3, 5, 7), (33, 1, 1), (5, 64, 1))
RADII = (1, 8, 1024)
OPTIMISTIC = F.FREE_M | F.UNK_M | F.MISS_M
INFO = ("origin", "cell")


def _pool(c, pool):
    return (c["keys"], c["A"], c["B"], c["S"]) if pool is None else pool


def _fields(c, g0, dims, pool=None):
    return PC.fields(*_pool(c, pool), c["depth"], g0, dims, c["a0"], c["b0"])


def _pcls(c, g0, dims, below, above=None, pool=None):
    p = _pool(c, pool)
    return PC.padded_classes(p[0], p[3], c["depth"], g0, dims, below, above)


def _info(got, c, lo, what):
    want = PC.info_of(lo, c["res"], c["depth"])
    R.assert_same(got, want, INFO, what)
    assert got["block_key"] == want["block_key"], (what, got["block_key"], want["block_key"])


def regions(c):
    """(what, g0, dims): the case's region, the small shapes at its anchor, a block-aligned region and the small region"""
    out = [("region", c["g0"], c["dims"])] + [(f"shape {s}", c["g0"], s) for s in SHAPES]
    out.append(("block-aligned",) + PC.aligned_region_of(c["notes"], c["depth"]))
    out.append(("small",) + tuple(PC.small_region_of(c["depth"])))
    return out


def box_and_columns(m, c, pool=None, cls_only=False, which=None):
    """box (all fields, and fields=()) and columns against the expander; cls_only: the pool's leaf layers and values are not
    the map's any more (after a merge), its classes are"""
    for what, g0, dims in regions(c) if which is None else which:
        lo = PC.lo_of(g0, c["res"], c["depth"])
        want = _fields(c, g0, dims, pool)
        got = m.box(lo, dims)
        R.assert_same(got, want, ("cls",) if cls_only else R.BOX_FIELDS, (c["name"], c["depth"], "box", what))
        _info(got, c, lo, ("box", what))
        bare = m.box(lo, dims, fields=())
        assert set(bare) == {"cls"} | set(R.INFO_FIELDS)
        R.assert_same(bare, want, ("cls",), (c["name"], c["depth"], "box fields=()", what))
        cols = m.columns(lo, dims)
        R.assert_same(cols, R.reduce_box(want["cls"]), R.COL_FIELDS, (c["name"], c["depth"], "columns", what))
        _info(cols, c, lo, ("columns", what))


def leaves(m, c):
    """m.leaves() through region_cases.yardstick against the expander (a class whose leaves() lists every block)"""
    lv = m.leaves()
    want = PC.leaves_of(c["keys"], c["A"], c["B"], c["S"], c["depth"])
    assert lv["A"].size == want["A"].size, (lv["A"].size, want["A"].size)
    y = R.yardstick(m, lv, c["lo"], c["dims"], c["a0"], c["b0"])
    R.assert_same(y, dict(cls=c["cls"], leaf_depth=c["leaf_depth"], A=c["fA"], B=c["fB"]), R.BOX_FIELDS, (c["name"], c["depth"], "leaves"))


def distance(m, c, pool=None):
    res = m.get_resolution()
    cls = _fields(c, c["g0"], c["dims"], pool)["cls"]
    for mask in D.MASKS:
        for radius in RADII:
            got = m.distance_field(c["lo"], c["dims"], obstacles=mask, radius=radius)
            D.assert_same(got, D.yardstick_a(cls, mask, radius, res), (c["name"], c["depth"], "distance A", mask, radius))
    if pool is not None:
        return
    for what, g0, dims in regions(c)[1:]:
        if int(np.prod(dims)) > 2000:
            continue
        lo = PC.lo_of(g0, c["res"], c["depth"])
        sub = _fields(c, g0, dims)["cls"]
        for mask in D.MASKS:
            for radius in RADII:
                got = m.distance_field(lo, dims, obstacles=mask, radius=radius)
                D.assert_same(got, D.yardstick_b(sub, mask, radius, res), (c["name"], c["depth"], "distance B", what, mask, radius))
                D.assert_same(got, D.yardstick_a(sub, mask, radius, res), (c["name"], c["depth"], "distance A", what, mask, radius))


def nearest(m, c):
    """the quadratic yardstick: the small region, and the case's region where it has at most 8 000 voxels"""
    todo = [("small",) + tuple(PC.small_region_of(c["depth"]))]
    if c["cls"].size <= 8000:
        todo.append(("region", c["g0"], c["dims"]))
    for what, g0, dims in todo:
        lo = PC.lo_of(g0, c["res"], c["depth"])
        cls = _fields(c, g0, dims)["cls"]
        for mask in D.MASKS[:3]:
            Dmin, first, _ = N.brute(cls, mask)
            for radius in (1, 8):
                want = {k: a.reshape(cls.shape) for k, a in N.finish(Dmin, first, radius).items()}
                N.assert_same(m.nearest(lo, dims, obstacles=mask, radius=radius), want, (c["name"], c["depth"], "nearest", what, mask, radius))


def frontier(m, c, pool=None, which=None):
    found = 0
    for what, g0, dims in (regions(c)[:1] + regions(c)[3:4]) if which is None else which:
        lo = PC.lo_of(g0, c["res"], c["depth"])
        p = _pcls(c, g0, dims, 1, pool=pool)
        for open_, unknown in (F.MASK_PAIRS[0], F.MASK_PAIRS[3]):
            for conn in F.CONNECTIVITIES:
                got = m.frontier(lo, dims, open=open_, unknown=unknown, connectivity=conn, min_neighbours=1, fields=("index", "nbrs", "score"))
                want = F.yardstick(p, open_, unknown, conn, 1)
                F.assert_same(got, want, (c["name"], c["depth"], "frontier", what, open_, unknown, conn))
                found += want["n"]
    assert found > 0
    return found


def _seeds(cls, clearance):
    """a seed in the largest component of the passable FREE voxels (from the expander), the region's corners besides"""
    ok = RE.passable_of(cls, F.FREE_M, F.OCC_M, clearance)
    if not ok.any():
        ok = RE.passable_of(cls, F.FREE_M, F.OCC_M, 0)
    seed, size = PC.largest_component(ok)
    return [seed, 0, cls.size - 1], size


def reach(m, c):
    cls = c["cls"]
    targets = np.arange(0, cls.size + 40, 37, dtype=np.uint32)
    for pass_mask, clearance in (RE.PAIRS[0], RE.PAIRS[1]):
        seeds, size = _seeds(cls, clearance)
        for conn in (6, 26):
            got = m.reach(c["lo"], c["dims"], seeds, passable=pass_mask, obstacles=F.OCC_M, clearance=clearance, connectivity=conn, targets=targets)
            want = RE.yardstick(cls, seeds, pass_mask, F.OCC_M, clearance, conn, targets=targets)
            RE.assert_same(got, want, (c["name"], c["depth"], "reach", pass_mask, clearance, conn))
        if clearance == 0:
            assert want["n_reached"] >= size > 1


def travel(m, c):
    cls = c["cls"]
    dims = c["dims"]
    for soft in (T.PLAIN, T.SOFT):
        seeds, _ = _seeds(cls, soft["clearance"])
        got = m.travel(c["lo"], dims, seeds, passable=F.FREE_M, obstacles=F.OCC_M, move_cost=(10, 14, 17), connectivity=26, fields=("cost", "parent"), **soft)
        want = T.yardstick(cls, seeds, F.FREE_M, F.OCC_M, move_cost=(10, 14, 17), connectivity=26, **soft)
        T.assert_same(got, want, (c["name"], c["depth"], "travel", soft))
        reached = np.flatnonzero(got["cost"].reshape(-1) != T.NONE)
        if reached.size:
            far = int(reached[got["cost"].reshape(-1)[reached].argmax()])
            path = T.walk(got["parent"], dims, far)
            cost = got["cost"].reshape(-1)[[f for f, _ in path]].astype(np.int64)
            assert cost[-1] == 0 and (np.diff(cost) < 0).all(), (c["name"], c["depth"], "the parents lead downhill to a seed")


def clusters(m, c):
    for conn in (6, 26):
        for tile in (0, 8):
            got = m.clusters(c["lo"], c["dims"], member=F.FREE_M, connectivity=conn, tile=tile, fields=("label",))
            CL.assert_same(got, CL.yardstick(c["cls"], F.FREE_M, None, conn, tile), (c["name"], c["depth"], "clusters", conn, tile))


def footing(m, c):
    total = 0
    for h, r, s, cmin in ((2, 1, 1, 1), (1, 0, 0, None)):
        below, above = FT.pads(h, r, s)
        p = _pcls(c, c["g0"], c["dims"], below, above)
        got = m.footing(c["lo"], c["dims"], support=FT.OCC_M, clear=OPTIMISTIC, headroom=h, radius=r, step=s, min_support=cmin, fields=FT.FIELDS)
        want = FT.yardstick(p, c["dims"], FT.OCC_M, OPTIMISTIC, h, r, s, cmin)
        FT.assert_same(got, want, (c["name"], c["depth"], "footing", h, r, s))
        total += want["n"]
    assert total > 0


def surface(m, c):
    total = 0
    for solid, open_, s in ((SF.OCC_M, OPTIMISTIC, 1), (SF.OCC_M, SF.FREE_M, 0)):
        p = _pcls(c, c["g0"], c["dims"], SF.pad_of(s))
        got = m.surface(c["lo"], c["dims"], solid=solid, open=open_, smooth=s, fields=SF.FIELDS)
        want = SF.yardstick(p, c["dims"], solid, open_, s)
        SF.assert_same(got, want, (c["name"], c["depth"], "surface", solid, open_, s))
        total += want["n"]
    assert total > 0


# ---- rays -------------------------------------------------------------------------------------------------------------------
def centres(origin, idx, res):
    """voxel centres as box's origin plus multiples of the fp32 resolution"""
    return (np.asarray(origin, np.float32) + np.asarray(idx, np.float32) * np.float32(res)).astype(np.float32)


def _sample(n, must):
    """up to six indices of an axis of n voxels, `must` among them"""
    s = sorted(set(int(v) for v in np.linspace(0, n - 1, min(n, 6)).round()))
    if 0 <= must < n and must not in s:
        s[int(np.abs(np.array(s) - must).argmin())] = must
    return sorted(set(s))


def axis_rays(c):
    """for every axis and both directions, rays from the centre of a voxel on one face of the region to the centre of the
    voxel on the opposite face, one per column of a 6 x 6 sample that holds the column through the root-collapsed block:
    (start voxels (n, 3), axis (n,), direction (n,))"""
    lim = 1 << (c["depth"] - 1)
    dims = c["dims"]
    through = [min(max(int(f) * lim - g, 0), d - 1) for f, g, d in zip(c["notes"]["root"], c["g0"], dims)]
    v, ax, sg = [], [], []
    for a in range(3):
        u, w = [b for b in range(3) if b != a]
        for i in _sample(dims[u], through[u]):
            for j in _sample(dims[w], through[w]):
                for sign in (1, -1):
                    s = [0, 0, 0]
                    s[u], s[w], s[a] = i, j, 0 if sign > 0 else dims[a] - 1
                    v.append(s)
                    ax.append(a)
                    sg.append(sign)
    return np.array(v, np.int64), np.array(ax), np.array(sg)


def closed_form_rays(m, c, pool=None, cls_only=False):
    """raycast_many against a closed form that uses no map code: the rows of an axis-parallel ray are the voxels from its
    start on, |trunc(e / res) - trunc(s / res)| + 1 of them (the truncation toward zero makes that one fewer than the voxels
    where the ray crosses coordinate 0); a ray whose start block is missing never starts.  `pool`: the map's pool after a
    change (what the rays must run through is then not asserted); cls_only: as box_and_columns takes it"""
    depth, dims, res = c["depth"], c["dims"], np.float32(m.get_resolution())
    dl = depth - 1
    f = _fields(c, c["g0"], dims, pool)
    origin = PC.info_of(c["lo"], c["res"], depth)["origin"]
    v, ax, sg = axis_rays(c)
    e = v.copy()
    e[np.arange(v.shape[0]), ax] = np.where(sg > 0, np.array(dims)[ax] - 1, 0)
    starts, ends = centres(origin, v, res), centres(origin, e, res)
    with np.errstate(invalid="ignore"):
        a0, a1 = np.trunc(starts / res).astype(np.int64), np.trunc(ends / res).astype(np.int64)
    rows = np.abs(a1 - a0).sum(1) + 1
    span = np.array(dims)[ax]
    assert ((rows == span) | (rows == span - 1)).all() and (np.abs(a1 - a0).sum(1) == np.abs(a1 - a0).max(1)).all(), "axis-parallel, within the region"
    if depth >= 2:   # (at depth 1 a voxel's centre is a multiple of the resolution and the quotient's rounding decides)
        assert (rows == span - 1).all(), "every ray crosses coordinate 0: one row fewer than voxels"
    lim = 1 << dl
    full = m.raycast_many(starts, ends, stop=(), max_steps=4096)
    occ = m.raycast_many(starts, ends, stop=("occupied",), max_steps=4096)
    seen = dict(missing=0, coarse=0, root=0, never=0, hits=0)
    for r in range(v.shape[0]):
        line = [slice(int(t), int(t) + 1) for t in v[r]]
        a, n = int(ax[r]), int(rows[r])
        first = int(v[r, a])
        line[a] = slice(first, first + n) if sg[r] > 0 else slice(first, first - n if first - n >= 0 else None, -1)
        cl, ld = f["cls"][tuple(line)].reshape(-1), f["leaf_depth"][tuple(line)].reshape(-1)
        assert cl.size == n
        what = (c["name"], depth, "ray", r, v[r].tolist(), a, int(sg[r]))
        if cl[0] == R.MISSING:                               # never starts
            seen["never"] += 1
            for g in (full, occ):
                assert g["steps"][r] == 0 and g["flags"][r] == 0 and g["cls"][r] == R.MISSING and g["leaf_depth"][r] == 255, what
                assert (g["counts"][r] == 0).all() and g["A"][r].view(np.uint32) == c["a0"].view(np.uint32), what
            continue
        hist = np.bincount(np.where(cl == R.UNCERTAIN, R.UNKNOWN, cl), minlength=4).astype(np.uint32)
        assert full["steps"][r] == n and full["flags"][r] == 0 and (full["counts"][r] == hist).all(), (what, full["steps"][r], n, full["counts"][r], hist)
        hit = np.flatnonzero(cl == R.OCCUPIED)
        last_occ = int(hit[0]) if hit.size else n - 1
        assert occ["steps"][r] == last_occ + 1 and occ["flags"][r] == (RC.HIT if hit.size else 0), (what, occ["steps"][r], last_occ)
        seen["hits"] += int(hit.size > 0)
        for g, last in ((full, n - 1), (occ, last_occ)):
            at = v[r].copy()
            at[a] += sg[r] * last
            gl = np.array(c["g0"], np.int64) + at
            t = tuple(int(q) for q in at)
            cell = int(R._cell_index(gl[0] & (lim - 1), gl[1] & (lim - 1), gl[2] & (lim - 1), dl))
            assert g["block_key"][r] == int(PC.key_of(gl >> dl)) and g["node_key"][r] == (dl << 16) | cell, (what, last)
            assert g["cls"][r] == f["cls"][t], (what, last, g["cls"][r], f["cls"][t])
            if cls_only:
                continue
            assert g["leaf_depth"][r] == f["leaf_depth"][t], (what, last, g["leaf_depth"][r], f["leaf_depth"][t])
            assert g["A"][r].view(np.uint32) == f["A"][t].view(np.uint32) and g["B"][r].view(np.uint32) == f["B"][t].view(np.uint32), (what, last)
        seen["missing"] += int((cl == R.MISSING).any())
        seen["coarse"] += int((ld < dl).any())
        seen["root"] += int((ld[cl != R.MISSING] == 0).any())
    print(f"closed-form rays {c['name']} depth {depth}: {v.shape[0]} rays, {seen}")
    # counted from the expander: the rays run through left-out blocks (dead reckoning), coarse leaves and a block collapsed to its root
    if pool is None:
        assert seen["missing"] > 0 and seen["root"] > 0 and seen["hits"] > 0 and (depth == 1 or seen["coarse"] > 0), seen
    return starts, ends


def oblique_rays(c, n=40, seed=11):
    """n rays between the centres of voxels of the region, from FREE voxels, in no special direction"""
    rng = np.random.default_rng(seed)
    free = np.argwhere(c["cls"] == R.FREE)
    s = free[rng.integers(0, free.shape[0], n)]
    e = np.stack([rng.integers(0, d, n) for d in c["dims"]], 1)
    origin = PC.info_of(c["lo"], c["res"], c["depth"])["origin"]
    jitter = rng.uniform(-0.3, 0.3, (2, n, 3))
    return centres(origin, s + jitter[0], c["res"]), centres(origin, e + jitter[1], c["res"])


def reduced_rays(m, host, c, starts, ends):
    """raycast_many of `m` against raycast_cases.reduce_rays over the iterator of the host-mode map `host` and the pool's
    leaf list, for every stop mask and max_steps 4096 and 7"""
    lv = PC.leaves_of(c["keys"], c["A"], c["B"], c["S"], c["depth"])
    stops = dict(RC.STOPS)
    if c["name"] == "BGKLVOctoMap":
        stops["uncertain"] = 1 << R.UNCERTAIN
    for name, mask in stops.items():
        for max_steps in (4096, 7):
            want = RC.reduce_rays(host, lv, starts, ends, mask, max_steps)
            RC.assert_same(m.raycast_many(starts, ends, stop=mask, max_steps=max_steps), want, (c["name"], c["depth"], "rays", name, max_steps))


def gain(m, host, c):
    """one fan from the centre of a FREE voxel in the middle of the region"""
    free = np.argwhere(c["cls"] == R.FREE)
    pick = free[((free - np.array(c["dims"]) // 2) ** 2).sum(1).argmin()]
    origin = PC.info_of(c["lo"], c["res"], c["depth"])["origin"]
    origins = centres(origin, pick[None], c["res"])
    offsets = G.fan(96, 12 * c["res"])
    for count, stop, max_steps in ((0xC, 0x2, 4096), (0x1F, 0, 7)):
        want = G.yardstick(host, None, c["lo"], c["dims"], origins, offsets, count, stop, max_steps, cls=c["cls"])
        got = m.gain(c["lo"], c["dims"], origins, offsets, count=count, stop=stop, max_steps=max_steps, fields=G.FIELDS)
        G.assert_same(got, want, (c["name"], c["depth"], "gain", count, stop, max_steps))
        assert want["gain"][0] > 0 and want["started"][0] == 96


# ---- after a change of the pool ---------------------------------------------------------------------------------------------
def erase_an_octant(maps, c):
    """erase_region of the blocks at and above key field 524288 on every axis in every map of `maps`; returns the numpy pool
    without those keys (the expander does not care about slot order) and a stream of the erased blocks"""
    import pack_cases as P
    f = PC.fields_of(c["keys"])
    gone = c["keys"][(f >= PC.ZERO).all(1)]
    assert 0 < gone.size < c["keys"].size
    pool, removed = PC.without(c["keys"], c["A"], c["B"], c["S"], gone)
    bs = float(np.float32(c["res"])) * (1 << (c["depth"] - 1))
    lo, hi = (0.0, 0.0, 0.0), tuple(float(v - PC.ZERO) * bs for v in f.max(0))      # block centres
    for m in maps:
        stats = m.erase_region(lo, hi)
        assert stats["n_removed"] == gone.size and stats["n_blocks"] == pool[0].size == m.block_count(), stats
    return pool, P.stream_from_pool(c["h"], *removed)


def after_the_erase(m, c, pool):
    box_and_columns(m, c, pool=pool)
    frontier(m, c, pool=pool)
    distance(m, c, pool=pool)
    closed_form_rays(m, c, pool=pool)


def merge_it_back(maps, c, stream):
    import pack_cases as P
    n = P.parse(stream)["n_blocks"]
    for m in maps:
        stats = m.merge(stream)
        assert stats["n_blocks"] == stats["n_created"] == n and m.block_count() == c["keys"].size, stats


def after_the_merge(m, c):
    """against the original classes: merge prunes the blocks it writes, so their leaf layers and values are its own"""
    original = (c["keys"], c["A"], c["B"], c["S"])
    box_and_columns(m, c, cls_only=True)
    frontier(m, c)
    distance(m, c, pool=original)
    closed_form_rays(m, c, pool=original, cls_only=True)
