"""Hand-built pools at block_depth 1 to 5 and their numpy expansion to the classes of a region: the cases, the yardstick and
the input conditions shared by tests/test_pool_queries_cpu.py and tests/test_pool_queries_gpu.py.

Written from the pool and stream contract comments of include/la3dm_hip.h (la3dm_devmap_download's node numbering, the
lattice of la3dm_devmap_box_host, the climb of la3dm_devmap_raycast_host); nothing here calls a query.  `build` writes a
pool (keys, A, B, S) with pack_cases and its stream; `classes` / `fields` expand the pool arrays to dense cls, leaf_depth, A
and B of a region, which the class-array yardsticks of the other helpers take.  Every comparison made with them is exact."""
import numpy as np

import pack_cases as P
import region_cases as R

ZERO = 524288                          # the key field of the block round the coordinate origin
YAMLS = dict(BGKOctoMap=None, BGKLOctoMap="L_YAML", GPOctoMap="GP_YAML", BGKLVOctoMap="LV_YAML")
# (class, block_depth, seed): BGK and BGK-LV at every depth la3dm_devmap_create accepts, GP and BGK-L at one depth each.  The
# seeds are chosen so that the expander alone meets assert_exercises_the_feature (the first of 1, 2, 3, ... that does)
CASES = (("BGKOctoMap", 1, 1), ("BGKOctoMap", 2, 1), ("BGKOctoMap", 3, 1), ("BGKOctoMap", 4, 1), ("BGKOctoMap", 5, 1),
         ("BGKLVOctoMap", 1, 1), ("BGKLVOctoMap", 2, 1), ("BGKLVOctoMap", 3, 1), ("BGKLVOctoMap", 4, 1), ("BGKLVOctoMap", 5, 1),
         ("GPOctoMap", 3, 1), ("BGKLOctoMap", 4, 1))
CASE_IDS = [f"{c}-d{d}" for c, d, _ in CASES]
SMALL_DIMS = (13, 12, 9)               # the region of the quadratic yardsticks (nearest, distance_cases.yardstick_b)
SMALL_START = (-7, -5, -3)             # its first voxel, relative to the lattice's origin voxel: odd, so no cell is 0


def params_of(cls_name, depth):
    import la3dm_amd
    return dict(getattr(la3dm_amd, YAMLS[cls_name]) if YAMLS[cls_name] else R.YAML, block_depth=depth)


def nbx_of(depth):
    return max(3, 24 >> (depth - 1))


def key_of(b):
    b = np.asarray(b, np.int64)
    return (b[..., 0] << 40) | (b[..., 1] << 20) | b[..., 2]


def fields_of(keys):
    keys = np.asarray(keys, np.int64)
    return np.stack([(keys >> 40) & 0xFFFFF, (keys >> 20) & 0xFFFFF, keys & 0xFFFFF], -1)


def build(cls_name, depth, seed, shape=None, left_out=0.2, collapse=0.15, force=True):
    """(params, header, keys, A, B, S, stream, notes).  The blocks are a box of `shape` blocks (default: a cube of nbx_of(depth)
    per axis) centred on key field 524288, a seeded share `left_out` of them missing, the kept ones in shuffled pool order;
    the tiling from pack_cases.tiling with a seeded collapse probability per node; leaf states of the variant's own set, A
    and B from pack_cases.odd_values.  With `force` three blocks are set by hand — one collapsed to its root (a face
    neighbour of a left-out block), one with exactly one sibling group of the deepest layer collapsed, one un-pruned;
    notes = dict(first = the fields of the box's first block, shape, root / group / full = the fields of the forced blocks,
    left_out = the fields of the missing blocks)"""
    params = params_of(cls_name, depth)
    h = P.header_fields(cls_name, params)
    rng = np.random.default_rng(1000 * seed + 10 * depth + P.VARIANT[cls_name])
    shape = (nbx_of(depth),) * 3 if shape is None else tuple(shape)
    first = np.array([ZERO - s // 2 for s in shape], np.int64)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    out = np.zeros(shape, bool)
    out.reshape(-1)[rng.permutation(grid.shape[0])[:int(round(left_out * grid.shape[0]))]] = True
    kept = grid[~out.reshape(-1)]
    kept = kept[rng.permutation(kept.shape[0])]                       # the pool order: no order
    nb, npb = kept.shape[0], P.npb_of(depth)
    col = rng.random((nb, npb)) < collapse
    notes = dict(first=first, shape=shape, left_out=grid[out.reshape(-1)] + first)
    if force:
        padded = np.zeros(tuple(s + 2 for s in shape), bool)
        padded[1:-1, 1:-1, 1:-1] = out
        beside = np.zeros(nb, bool)                                   # kept blocks with a left-out face neighbour
        for ax in range(3):
            for step in (-1, 1):
                q = kept + 1
                q[:, ax] += step
                beside |= padded[q[:, 0], q[:, 1], q[:, 2]]
        # blocks with a voxel in the region of region_of
        lim = 1 << (depth - 1)
        ends = np.array(shape) * lim + np.array((1, 0, -4))
        inner = ((kept * lim + lim - 1 >= 3) & (kept * lim < ends)).all(1)
        cand = np.flatnonzero(beside & inner)
        assert cand.size, "no kept block beside a left-out one"
        root = int(cand[rng.integers(0, cand.size)])
        rest = np.flatnonzero(inner & (np.arange(nb) != root))
        group, full = (int(v) for v in rest[rng.permutation(rest.size)[:2]])
        col[root], col[group], col[full] = False, False, False
        col[root, 0] = True
        if depth >= 2:
            col[group] = P.one_group_collapsed(depth, depth - 1, int(rng.integers(0, 8 ** (depth - 2))))[0]
        notes.update(root=kept[root] + first, group=kept[group] + first, full=kept[full] + first)
    keys, A, B, S = P.random_pool(rng, h, nb, col, keys=key_of(kept + first))
    return params, h, keys, A, B, S, P.stream_from_pool(h, keys, A, B, S), notes


def region_of(notes, depth):
    """(g0, dims) of the case's region: it starts three voxels inside the box's corner, overhangs the box by one voxel on x,
    ends on the box's face on y and four voxels short of it on z — at most 46 x 45 x 41 voxels"""
    lim = 1 << (depth - 1)
    n = [s * lim for s in notes["shape"]]
    return [int(f) * lim + 3 for f in notes["first"]], (n[0] - 2, n[1] - 3, n[2] - 7)


def small_region_of(depth):
    lim = 1 << (depth - 1)
    return [ZERO * lim + s for s in SMALL_START], SMALL_DIMS


def aligned_region_of(notes, depth):
    """a region whose faces are block faces: the box without its outermost layer of blocks, at least one block"""
    lim = 1 << (depth - 1)
    lo = [int(f) + 1 for f in notes["first"]]
    return [f * lim for f in lo], tuple(max(1, s - 2) * lim for s in notes["shape"])


def lo_of(g, resolution, depth):
    """a world point inside voxel g (its centre in float64, rounded to float32), checked with region_cases.anchor.  Block
    524288 is centred on coordinate 0, so the coordinate origin lies lim / 2 voxels above the block's first face"""
    lim = 1 << (depth - 1)
    lo = np.array([(int(v) - ZERO * lim - lim / 2 + 0.5) * float(np.float32(resolution)) for v in g], np.float32)
    b, c, g0, origin = R.anchor(lo, resolution, depth)
    assert list(g0) == [int(v) for v in g], (g, g0)
    return lo


def info_of(lo, resolution, depth):
    """origin, block_key and cell a region query returns for `lo`"""
    b, c, _, origin = R.anchor(lo, resolution, depth)
    return dict(origin=origin, block_key=(b[0] << 40) | (b[1] << 20) | b[2], cell=np.array(c, np.int32))


def _covering(keys, S, depth, g0, dims):
    """per voxel of the region: exists, pool row, node number and layer of the covering leaf"""
    dl, lim = depth - 1, 1 << (depth - 1)
    keys = np.asarray(keys, np.int64)
    g = [(int(g0[a]) + np.arange(dims[a], dtype=np.int64)).reshape([-1 if a == b else 1 for b in range(3)]) for a in range(3)]
    key = np.broadcast_to(((g[0] >> dl) << 40) | ((g[1] >> dl) << 20) | (g[2] >> dl), dims).reshape(-1)
    cell = np.broadcast_to(R._cell_index(g[0] & (lim - 1), g[1] & (lim - 1), g[2] & (lim - 1), dl), dims).reshape(-1).copy()
    n = key.size
    if keys.size == 0:
        return np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    order = np.argsort(keys)
    pos = np.minimum(np.searchsorted(keys[order], key), keys.size - 1)
    row = order[pos]
    exists = keys[row] == key
    layer = np.full(n, dl, np.int64)
    climbing = exists.copy()
    for d in range(dl, 0, -1):                                        # climb while the state is PRUNED and the layer is above 0
        climbing &= (S[row, P.base(d) + cell] & 7) == P.PRUNED
        cell[climbing] >>= 3
        layer[climbing] -= 1
    base = (8 ** layer - 1) // 7
    return exists, row, base + cell, layer


def fields(keys, A, B, S, depth, g0, dims, a0, b0):
    """the expander: dense cls, leaf_depth, A, B (and node_key = layer << 16 | index of the covering leaf, -1 where MISSING) of
    the region of `dims` whose voxel (0, 0, 0) has the global index g0; a0, b0 = the default node's values"""
    dims = tuple(int(d) for d in dims)
    if np.asarray(keys).size == 0:                                    # one default block that no voxel finds
        A, B, S = (np.zeros((1, P.npb_of(depth)), t) for t in (np.float32, np.float32, np.uint8))
    exists, row, node, layer = _covering(keys, np.asarray(S, np.uint8), depth, g0, dims)
    state = np.where(exists, np.asarray(S, np.uint8)[row, node] & 7, R.MISSING).astype(np.uint8)
    assert not (state[exists] == P.PRUNED).any(), "a block's root is never PRUNED"
    out = dict(cls=state, leaf_depth=np.where(exists, layer, 255).astype(np.uint8),
               A=np.where(exists, np.asarray(A, np.float32)[row, node], np.float32(a0)).astype(np.float32),
               B=np.where(exists, np.asarray(B, np.float32)[row, node], np.float32(b0)).astype(np.float32),
               leaf_key=np.where(exists, (layer << 16) | (node - (8 ** layer - 1) // 7), -1).astype(np.int64))
    return {k: v.reshape(dims) for k, v in out.items()}


def classes(keys, S, depth, g0, dims):
    """cls and leaf_depth of the expander"""
    zeros = np.zeros(np.asarray(S).shape, np.float32)
    f = fields(keys, zeros, zeros, S, depth, g0, dims, 0, 0)
    return f["cls"], f["leaf_depth"]


def padded_classes(keys, S, depth, g0, dims, below, above=None):
    """cls of the region grown by `below` voxels before voxel (0, 0, 0) and `above` after the last one (per axis, or one
    number for all): what the queries that read a halo from the map see"""
    below = (below,) * 3 if np.isscalar(below) else tuple(below)
    above = below if above is None else ((above,) * 3 if np.isscalar(above) else tuple(above))
    return classes(keys, S, depth, [int(g) - b for g, b in zip(g0, below)], [int(d) + a + b for d, a, b in zip(dims, below, above)])[0]


def leaves_of(keys, A, B, S, depth):
    """the pool's covering leaves in the fields of a map's leaves() that the ray and region yardsticks read"""
    m = P.leaf_mask(S, depth)
    row, node = np.nonzero(m)
    layer = np.searchsorted(np.array([P.base(d + 1) for d in range(depth)]), node, side="right")
    S = np.asarray(S, np.uint8)
    return dict(block_key=np.asarray(keys, np.int64)[row], node_key=((layer << 16) | (node - (8 ** layer - 1) // 7)).astype(np.int32),
                A=np.asarray(A, np.float32)[m], B=np.asarray(B, np.float32)[m], state=S[m] & 7, classified=S[m] >> 7)


def without(keys, A, B, S, gone):
    """the pool without the blocks whose keys are in `gone`, and the removed part"""
    drop = np.isin(keys, np.asarray(gone, np.int64))
    return (keys[~drop], A[~drop], B[~drop], S[~drop]), (keys[drop], A[drop], B[drop], S[drop])


def largest_component(ok):
    """flat index of the first voxel of the largest 6-connected component of the boolean array, and the component's size"""
    from scipy.ndimage import label
    lab, n = label(ok)
    assert n > 0
    sizes = np.bincount(lab.reshape(-1))[1:]
    best = int(sizes.argmax()) + 1
    return int(np.flatnonzero(lab.reshape(-1) == best)[0]), int(sizes.max())


# ---- what a case must hold to count -----------------------------------------------------------------------------------------
def input_conditions(cls, leaf_depth, g0, depth, variant_classes):
    """counted from the expander, never from the code under test"""
    lim = 1 << (depth - 1)
    n = cls.size
    share = {int(c): float((cls == c).sum()) / n for c in sorted(set(variant_classes) | {R.MISSING})}
    last = [int(g) + int(d) - 1 for g, d in zip(g0, cls.shape)]
    return dict(depth=depth, dims=tuple(cls.shape), share={k: round(v, 4) for k, v in share.items()},
                leaf_depths=sorted(int(v) for v in np.unique(leaf_depth[leaf_depth != 255])), cell=tuple(int(g) % lim for g in g0),
                straddles=tuple(int(g) < ZERO * lim <= e for g, e in zip(g0, last)))


def assert_exercises_the_feature(cond, what=""):
    """every class of the variant on at least 5 % of the region's voxels and MISSING on 15 to 45 %; every leaf depth 0 to
    block_depth - 1; an anchor cell that is non-zero on every axis from depth 2 up; the region's first and last voxel on
    opposite sides of the lattice's origin on every axis"""
    print(f"pool input conditions {what}: {cond}")
    depth = cond["depth"]
    assert all(v >= 0.05 for c, v in cond["share"].items() if c != R.MISSING), cond
    assert 0.15 <= cond["share"][R.MISSING] <= 0.45, cond
    assert cond["leaf_depths"] == list(range(depth)), cond
    assert depth == 1 or all(c != 0 for c in cond["cell"]), cond
    assert all(cond["straddles"]), cond


def variant_classes(cls_name):
    return (R.FREE, R.OCCUPIED, R.UNKNOWN, R.UNCERTAIN) if cls_name == "BGKLVOctoMap" else (R.FREE, R.OCCUPIED, R.UNKNOWN)


_BUILT = {}


SLAB = dict(shape=(48, 48, 32), left_out=0.05, force=False)      # at depth 1: 70 041 one-voxel blocks, two 4 096-item scan tiles


def case(cls_name, depth, seed, **how):
    """the case, built once and shared; nobody writes to it: dict(params, h, keys, A, B, S, stream, notes, g0, dims, lo, res,
    a0, b0, cls, leaf_depth, fA, fB, leaf_key = the expander over the region); `how`: build's other arguments"""
    k = (cls_name, depth, seed, tuple(sorted(how.items())))
    if k not in _BUILT:
        params, h, keys, A, B, S, stream, notes = build(cls_name, depth, seed, **how)
        g0, dims = region_of(notes, depth)
        res = params["resolution"]
        c = dict(name=cls_name, depth=depth, params=params, h=h, keys=keys, A=A, B=B, S=S, stream=stream, notes=notes, g0=g0, dims=dims,
                 res=res, lo=lo_of(g0, res, depth), a0=np.float32(h["init_A"]), b0=np.float32(h["init_B"]))
        f = fields(keys, A, B, S, depth, g0, dims, c["a0"], c["b0"])
        c.update(cls=f["cls"], leaf_depth=f["leaf_depth"], fA=f["A"], fB=f["B"], leaf_key=f["leaf_key"])
        for a in (keys, A, B, S, stream, c["cls"], c["leaf_depth"], c["fA"], c["fB"]):
            a.setflags(write=False)
        _BUILT[k] = c
    return _BUILT[k]


def sub(c, g0, dims):
    """the expander's fields over another region of the case's pool"""
    return fields(c["keys"], c["A"], c["B"], c["S"], c["depth"], g0, dims, c["a0"], c["b0"])


def pcls(c, g0, dims, below, above=None, pool=None):
    keys, S = (c["keys"], c["S"]) if pool is None else (pool[0], pool[3])
    return padded_classes(keys, S, c["depth"], g0, dims, below, above)
