"""The yardstick, the cases and the input conditions shared by tests/test_reach_cpu.py and tests/test_reach_gpu.py.

The yardstick never calls reach, box or distance_field: the classes come from `region_cases.yardstick` (a walk of the leaf
list), the clearance mask is a ball dilation of the obstacle classes with zeros outside the region (shifted slices ORed),
and the wave is a loop of shifted boolean slices: the voxels of level l are the passable, not yet reached voxels with a
neighbour in level l - 1."""
import numpy as np

import region_cases as R
import frontier_cases as F

NONE = 0xFFFFFFFF
CONNECTIVITIES = F.CONNECTIVITIES
FREE_M, OCC_M, UNK_M, MISS_M = F.FREE_M, F.OCC_M, F.UNK_M, F.MISS_M
SEED = (40, 41, 15)                  # the voxel of the recipe region that holds scan 1's sensor origin
# (pass mask, clearance) with obstacles OCCUPIED: the four pairs of the measured table
PAIRS = ((FREE_M, 0), (FREE_M, 2), (FREE_M, 3), (FREE_M | UNK_M, 0))
STATS = ("n_seeded", "n_reached", "levels")
# closed-form boxes of the empty map
OPEN_BOXES = ((9, 10, 11), (1, 1, 40), (2, 2, 17), (1, 5, 9), (3, 1, 7), (2, 3, 2), (33, 1, 1), (5, 64, 1))


def flat(ijk, dims):
    return int((ijk[0] * dims[1] + ijk[1]) * dims[2] + ijk[2])


def passable_of(cls, pass_mask, obstacle_mask=0, clearance=0):
    """class in pass_mask, and no voxel OF THE REGION with a class in obstacle_mask within `clearance` voxels (Euclidean)"""
    ok = F.in_mask(cls, pass_mask)
    if clearance == 0:
        return ok
    nx, ny, nz = cls.shape
    r = int(clearance)
    obst = np.zeros((nx + 2 * r, ny + 2 * r, nz + 2 * r), bool)            # zeros outside the region
    obst[r:r + nx, r:r + ny, r:r + nz] = F.in_mask(cls, obstacle_mask)
    near = np.zeros(cls.shape, bool)
    for di in range(-r, r + 1):
        for dj in range(-r, r + 1):
            for dk in range(-r, r + 1):
                if di * di + dj * dj + dk * dk <= r * r:
                    near |= obst[r + di:r + di + nx, r + dj:r + dj + ny, r + dk:r + dk + nz]
    return ok & ~near


def wave(ok, seeds, connectivity, max_steps=None):
    """steps (uint32, NONE where unreached) and the stats of the wave over the boolean array `ok` from the flat seed indices"""
    nx, ny, nz = ok.shape
    n = ok.size
    steps = np.full(ok.shape, NONE, np.uint32)
    front = np.zeros((nx + 2, ny + 2, nz + 2), bool)
    inner = front[1:-1, 1:-1, 1:-1]                      # a view: the front without its pad
    for s in seeds:
        if 0 <= int(s) < n and ok.reshape(-1)[int(s)]:
            i, j, k = np.unravel_index(int(s), ok.shape)
            inner[i, j, k] = True
    open_ = ok & ~inner
    steps[inner] = 0
    stats = dict(n_seeded=int(inner.sum()), n_reached=int(inner.sum()), levels=0)
    offs = F.offsets(connectivity)
    level = 0
    while inner.any() and (max_steps is None or level < max_steps):
        level += 1
        new = np.zeros(ok.shape, bool)
        for di, dj, dk in offs:
            new |= front[1 + di:1 + di + nx, 1 + dj:1 + dj + ny, 1 + dk:1 + dk + nz]
        new &= open_
        if not new.any():
            break
        steps[new] = level
        open_ &= ~new
        inner[...] = new
        stats["n_reached"] += int(new.sum())
        stats["levels"] = level
    return dict(steps=steps, **stats)


def yardstick(cls, seeds, pass_mask, obstacle_mask=OCC_M, clearance=0, connectivity=6, max_steps=None, targets=None):
    ok = passable_of(cls, pass_mask, obstacle_mask, clearance)
    out = wave(ok, seeds, connectivity, max_steps)
    if targets is not None:
        t = np.asarray(targets, np.int64)
        ts = np.full(t.size, NONE, np.uint32)
        inside = (t >= 0) & (t < cls.size)
        ts[inside] = out["steps"].reshape(-1)[t[inside]]
        out["target_steps"] = ts
    return out


def closed_form(dims, seed_ijk, connectivity):
    """steps on an open box from one seed: sum |d| (6), max |d| (26), max(max |d|, ceil(sum |d| / 2)) (18)"""
    d = [np.abs(np.arange(n, dtype=np.int64) - s) for n, s in zip(dims, seed_ijk)]
    a, b, c = d[0][:, None, None], d[1][None, :, None], d[2][None, None, :]
    total, most = a + b + c, np.maximum(np.maximum(a, b), c)
    steps = {6: total, 26: most + 0 * total, 18: np.maximum(most, (total + 1) // 2)}[connectivity]
    return np.broadcast_to(steps, dims).astype(np.uint32)


def corner_seeds(dims):
    """a corner, the centre and the far corner"""
    return ((0, 0, 0), tuple(n // 2 for n in dims), tuple(n - 1 for n in dims))


def assert_same(got, want, what, fields=("steps", "target_steps") + STATS):
    for k in STATS:
        if k in fields:
            assert got[k] == want[k], (what, k, got[k], want[k])
    R.assert_same(got, want, [k for k in ("steps", "target_steps") if k in fields and k in want and k in got], what)


def input_conditions(cls, seed, batch):
    """counted from the yardstick's classes, never from the code under test: per (clearance, connectivity 6) of the FREE
    rows passable / reached / unreachable voxels and the levels"""
    out = dict(seed_passable={c: bool(passable_of(cls, FREE_M, OCC_M, c).reshape(-1)[seed]) for c in (0, 2, 3)}, batch=batch)
    for clearance in (0, 2):
        ok = passable_of(cls, FREE_M, OCC_M, clearance)
        w = wave(ok, [seed], 6)
        out[clearance] = dict(passable=int(ok.sum()), reached=w["n_reached"], unreachable=int(ok.sum()) - w["n_reached"], levels=w["levels"])
    return out


def assert_exercises_the_feature(cond):
    """The seed is passable; at least half of what was counted on region_cases.fused_map(3) — FREE, connectivity 6:
    clearance 0 reaches 16 818 voxels and leaves 23, in 92 levels; clearance 2 reaches 8 789 and leaves 2 480, in 118 — the
    margin the region tests use between that map and the product's; and more levels than one batch of launches"""
    print(f"reach input conditions: {cond}")
    assert all(cond["seed_passable"].values()), cond
    assert cond[0]["reached"] >= 8409 and cond[0]["unreachable"] >= 12, cond
    assert cond[2]["reached"] >= 4395 and cond[2]["unreachable"] >= 1240, cond
    assert cond[0]["levels"] > cond["batch"] and cond[2]["levels"] > cond["batch"], cond


def far_lo(m, lo, metres=100.0):
    """a region 100 m from the scans: every voxel MISSING"""
    return (np.asarray(lo, np.float32) + np.array((metres, metres, 0.0), np.float32)).astype(np.float32)
