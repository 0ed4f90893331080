"""Rays and the independent yardstick shared by tests/test_raycast_many_cpu.py and tests/test_raycast_many_gpu.py.

Nothing here calls raycast_many: `reduce_rays` restates its contract on top of the per-row walk `m.raycast(s, e)` (the
RayCaster iterator, unchanged) and a covering-leaf lookup in `m.leaves()`."""
import numpy as np

FREE, OCCUPIED, UNKNOWN, MISSING = 0, 1, 2, 3
HIT, TRUNCATED, INVALID = 1, 2, 4
STOPS = {"occupied": 1 << OCCUPIED, "occupied|missing": (1 << OCCUPIED) | (1 << MISSING), "none": 0}
FIELDS = ("steps", "flags", "p", "block_key", "node_key", "cls", "leaf_depth", "A", "B", "counts")
N_RECIPE = 400


def recipe_rays(lv):
    """400 rays from inside FREE leaves, uniform directions, 2 .. 12 m (seed 5; the order of the generator's calls is part
    of the recipe)"""
    rng = np.random.default_rng(5)
    free = np.nonzero(lv["state"] == 0)[0]
    starts, ends = [], []
    for _ in range(N_RECIPE):
        s3 = lv["loc"][free[rng.integers(0, free.size)]] + rng.uniform(-0.04, 0.04, 3).astype(np.float32)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        e3 = (s3 + d * rng.uniform(2, 12)).astype(np.float32)
        starts.append(s3)
        ends.append(e3)
    return np.array(starts, np.float32), np.array(ends, np.float32)


def hand_rays(lv):
    """10 axis-aligned, 10 planar, 5 exact diagonals (the double step), then one each: zero length, start outside the map,
    start inside and leaving for good, a NaN coordinate, a start 3e8 m out.  Returns starts, ends, names of the last five."""
    rng = np.random.default_rng(17)
    free = np.nonzero(lv["state"] == 0)[0]
    s = (lv["loc"][free[rng.integers(0, free.size, 30)]] + rng.uniform(-0.04, 0.04, (30, 3))).astype(np.float32)
    e = (s + rng.uniform(-3, 3, (30, 3))).astype(np.float32)
    e[:10, 1:] = s[:10, 1:]                                   # axis-aligned (x)
    e[4:7, 0], e[4:7, 1] = s[4:7, 0], s[4:7, 1] + np.float32(2.3)    # ... three along y
    e[7:10, 0], e[7:10, 2] = s[7:10, 0], s[7:10, 2] - np.float32(1.7)   # ... three along z
    e[10:20, 2] = s[10:20, 2]                                 # planar
    e[20:25] = s[20:25] + np.float32(0.7) * np.sign(rng.uniform(-1, 1, (5, 3))).astype(np.float32)   # exact diagonals
    e[25] = s[25]                                             # zero length
    s[26], e[26] = (500, 500, 500), (501, 500, 500)           # starts outside the map
    e[27] = s[27] + np.array([0, 0, 30], np.float32)          # leaves the map for good
    e[28, 1] = np.nan                                         # one NaN
    s[29, 0] = 3e8                                            # one at 3e8 m
    return s, e, {25: "zero", 26: "outside", 27: "leaving", 28: "nan", 29: "far"}


def all_rays(lv):
    a, b = recipe_rays(lv)
    c, d, names = hand_rays(lv)
    return np.concatenate([a, c]), np.concatenate([b, d]), {N_RECIPE + k: v for k, v in names.items()}


def leaf_table(lv):
    return {(int(b), int(k)): i for i, (b, k) in enumerate(zip(lv["block_key"], lv["node_key"]))}


def reduce_rays(m, lv, starts, ends, mask, max_steps, cap=8192):
    """the contract of raycast_many, from the iterator's rows and the leaf list"""
    tab = leaf_table(lv)
    _, a0, b0, _ = m.search(500.0, 500.0, 500.0)       # what search answers for a missing block: the default node
    res = np.float32(m.get_resolution())
    n = starts.shape[0]
    out = dict(steps=np.zeros(n, np.uint32), flags=np.zeros(n, np.uint8), p=np.zeros((n, 3), np.float32),
               block_key=np.zeros(n, np.int64), node_key=np.zeros(n, np.int32), cls=np.full(n, MISSING, np.uint8),
               leaf_depth=np.full(n, 255, np.uint8), A=np.full(n, a0, np.float32), B=np.full(n, b0, np.float32),
               counts=np.zeros((n, 4), np.uint32))
    for r in range(n):
        c = np.concatenate([starts[r], ends[r]]).astype(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            if not (np.abs(c / res) < np.float32(2.0 ** 30)).all():
                out["flags"][r] = INVALID
                continue
        rows = m.raycast(starts[r], ends[r], cap=cap)
        assert rows["p"].shape[0] < cap
        steps = flags = 0
        for j in range(rows["p"].shape[0]):
            if steps == max_steps:
                flags |= TRUNCATED
                break
            steps += 1
            bk, nk = int(rows["block_key"][j]), int(rows["node_key"][j])
            if rows["valid"][j]:
                d, i = nk >> 16, nk & 0xFFFF
                while (bk, (d << 16) + i) not in tab:
                    assert d > 0, "an existing block has a leaf over every finest cell"
                    d, i = d - 1, i >> 3
                li = tab[(bk, (d << 16) + i)]
                cls, depth, A, B = int(lv["state"][li]), d, lv["A"][li], lv["B"][li]
                assert (d == nk >> 16) == (rows["state"][j] != 3)      # the raw node reads PRUNED exactly when a coarser leaf covers it
            else:
                cls, depth, A, B = MISSING, 255, np.float32(a0), np.float32(b0)
            out["counts"][r, UNKNOWN if cls == 4 else cls] += 1          # (a BGK-LV map's UNCERTAIN is counted with UNKNOWN)
            out["p"][r], out["block_key"][r], out["node_key"][r] = rows["p"][j], bk, nk
            out["cls"][r], out["leaf_depth"][r], out["A"][r], out["B"][r] = cls, depth, A, B
            if mask & (1 << cls):
                flags |= HIT
                break
        out["steps"][r], out["flags"][r] = steps, flags
    return out


def assert_same(a, b, what=""):
    """exact: integers by ==, floats by their bits"""
    for k in FIELDS:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        bad = np.nonzero((x != y).reshape(x.shape[0], -1).any(1))[0]
        assert bad.size == 0, (what, k, bad[:8].tolist(), a[k][bad[:3]].tolist(), b[k][bad[:3]].tolist())


def category_counts(occ, full, block_depth):
    """occ = the host form with stop = occupied, full = with stop = none (max_steps 4096), recipe rays only: hits,
    non-hits, rays that cross a missing block before they stop, hits whose covering leaf is coarser than the
    base resolution (the raw voxel reads PRUNED), truncated rays, longest walk, mean walk"""
    q = slice(0, N_RECIPE)
    hit = (occ["flags"][q] & HIT) != 0
    return dict(hits=int(hit.sum()), non_hits=int((~hit).sum()), missing=int((occ["counts"][q, MISSING] > 0).sum()),
                pruned_hits=int((hit & (occ["leaf_depth"][q] < block_depth - 1)).sum()),
                truncated=int(((occ["flags"][q] | full["flags"][q]) & TRUNCATED != 0).sum()),
                longest=int(full["steps"][q].max()), mean=float(full["steps"][q].mean()))


def assert_rays_exercise_the_feature(cat, block_depth):
    print(f"raycast input conditions at block_depth {block_depth}: {cat}")
    assert cat["truncated"] == 0
    if block_depth == 4:   # about half of what was counted on the restatement's map (229 / 171 / 89 / 57)
        assert cat["hits"] >= 100 and cat["non_hits"] >= 100 and cat["missing"] >= 40 and cat["pruned_hits"] >= 20, cat
    else:
        assert min(cat["hits"], cat["non_hits"], cat["missing"], cat["pruned_hits"]) > 0, cat
