"""The yardstick, the cases and the input conditions shared by tests/test_footing_cpu.py and tests/test_footing_gpu.py.

The yardstick never calls footing or box.  It is written from the contract comment of include/la3dm_hip.h: the classes of
the padded box come from `region_cases.yardstick` (a walk of the leaf list); stand, near and body are shifted slices of the
two mask arrays, the support count is a sum of shifted slices and the list is np.flatnonzero.  Every comparison is exact."""
import numpy as np

import region_cases as R

FREE_M, OCC_M, UNK_M, MISS_M, UNC_M = (1 << c for c in range(5))
OPTIMISTIC = FREE_M | UNK_M | MISS_M
FIELDS = ("index", "levels", "lowest", "highest")
STATS = ("n_stand", "n_body", "n_foot", "disc_cells")
MAX_HEADROOM, MAX_RADIUS, MAX_STEP, MAX_CELLS = 32, 8, 4, 1 << 28


def disc(r):
    return [(di, dj) for di in range(-r, r + 1) for dj in range(-r, r + 1) if 0 < di * di + dj * dj <= r * r]


def pads(h, r, s):
    """voxels of the padded box below voxel (0, 0, 0) and above the last voxel, per axis"""
    return (r, r, 1 + s), (r, r, h - 1 + s)


def padded_dims(dims, h, r, s):
    lo, hi = pads(h, r, s)
    return tuple(int(d) + a + b for d, a, b in zip(dims, lo, hi))


def in_mask(cls, mask):
    return ((np.uint32(mask) >> cls.astype(np.uint32)) & 1).astype(bool)


def yardstick(pcls, dims, support, clear, h, r, s, c=None, cap=None):
    """footing of the region `dims` whose padded box has the classes pcls (shape padded_dims(dims, h, r, s)): the definition
    of the contract, term by term"""
    nx, ny, nz = dims
    assert pcls.shape == padded_dims(dims, h, r, s), (pcls.shape, dims, h, r, s)
    N = len(disc(r))
    c = N if c is None else c
    sup, clr = in_mask(pcls, support), in_mask(pcls, clear)
    z0 = 1 + s                                              # padded z of the region's k = 0

    def clear_run(z_from, t0, t1, n):
        """for the n padded z from z_from on: cls(z + t) in clear for every t in [t0, t1)"""
        out = np.ones(pcls.shape[:2] + (n,), bool)
        for t in range(t0, t1):
            out &= clr[:, :, z_from + t:z_from + t + n]
        return out

    # stand at padded z in [1, nz + 2s]: all that near asks for
    stand_all = sup[:, :, 0:nz + 2 * s] & clear_run(1, 0, h, nz + 2 * s)          # index q <-> padded z = q + 1
    stand = stand_all[:, :, s:s + nz]                                             # the region's own z
    near = np.zeros(pcls.shape[:2] + (nz,), bool)
    for dk in range(-s, s + 1):
        near |= stand_all[:, :, s + dk:s + dk + nz]
    body = clear_run(z0, s, h, nz)
    inner = (slice(r, r + nx), slice(r, r + ny))
    ok_body = np.ones((nx, ny, nz), bool)
    count = np.zeros((nx, ny, nz), np.int32)
    for di, dj in disc(r):
        sl = (slice(r + di, r + di + nx), slice(r + dj, r + dj + ny))
        ok_body &= body[sl]
        count += near[sl]
    st = stand[inner]
    with_body = st & ok_body
    foot = with_body & (count >= c)
    index = np.flatnonzero(foot.reshape(-1)).astype(np.uint32)
    n = int(index.size)
    if cap is not None:
        index = index[:cap]
    any_foot = foot.any(2)
    return dict(n=n, index=index, levels=foot.sum(2).astype(np.uint32),
                lowest=np.where(any_foot, foot.argmax(2), -1).astype(np.int32),
                highest=np.where(any_foot, nz - 1 - foot[:, :, ::-1].argmax(2), -1).astype(np.int32),
                n_stand=int(st.sum()), n_body=int(with_body.sum()), n_foot=n, disc_cells=N, foot=foot, stand=st)


def assert_same(got, want, what, fields=FIELDS):
    """exact: n and the stats by ==, the arrays by == with shape and dtype"""
    assert got["n"] == want["n"], (what, got["n"], want["n"])
    for k in STATS:
        if k in got:
            assert got[k] == want[k], (what, k, got[k], want[k])
    R.assert_same(got, want, [k for k in fields if k in want and k in got], what)


def padded_case(m, lv, lo, dims, h, r, s):
    """(lo to query, classes of the padded box) of the region of `dims` whose voxel (0, 0, 0) holds `lo`: the yardstick region
    starts pads() below it"""
    res = np.float32(m.get_resolution())
    below, _ = pads(h, r, s)
    y = R.yardstick(m, lv, np.asarray(lo, np.float32), (1, 1, 1))
    big_lo = (y["origin"] - np.array(below, np.float32) * res).astype(np.float32)
    big = R.yardstick(m, lv, big_lo, padded_dims(dims, h, r, s))
    return y["origin"], big["cls"]


def sub_case(big_cls, big_origin, offset, dims, h, r, s, res):
    """the same from the classes of an enclosing box: the sub-box of `dims` at `offset`, whose pads lie inside the big box"""
    below, above = pads(h, r, s)
    assert all(o >= b and o + d + a <= n for o, d, b, a, n in zip(offset, dims, below, above, big_cls.shape)), (offset, dims)
    lo = (big_origin + np.array(offset, np.float32) * np.float32(res)).astype(np.float32)
    sl = tuple(slice(o - b, o + d + a) for o, d, b, a in zip(offset, dims, below, above))
    return lo, np.ascontiguousarray(big_cls[sl])


def restrict(want_big, big_dims, offset, dims):
    """the answer over the enclosing box restricted to the sub-box, list and columns re-indexed"""
    foot = want_big["foot"][tuple(slice(o, o + d) for o, d in zip(offset, dims))]
    nz = dims[2]
    any_foot = foot.any(2)
    return dict(n=int(foot.sum()), index=np.flatnonzero(foot.reshape(-1)).astype(np.uint32), levels=foot.sum(2).astype(np.uint32),
                lowest=np.where(any_foot, foot.argmax(2), -1).astype(np.int32),
                highest=np.where(any_foot, nz - 1 - foot[:, :, ::-1].argmax(2), -1).astype(np.int32))


# ---- the hand-built scene: 3 x 3 x 2 blocks of depth 4 (8^3 cells each), the region all of them ----------------------------
SCENE_DIMS = (24, 24, 16)
SCENE_LO = (-0.35, -0.35, -0.35)      # the centre of cell (0, 0, 0) of the block round the origin: 0.1 m cells from -0.4
SCENE_LEFT_OUT = (2, 2, 1)            # the block that is not in the stream
# (clear, h, r, s) -> stand, body, {c: foot}: counted with a numpy sketch of the definition, recorded in the issue
SCENE_COUNTS = (
    (FREE_M, 2, 0, 0, 583, None, {0: 583}),
    (FREE_M, 4, 0, 0, 519, None, {}),
    (FREE_M, 4, 2, 1, 519, 290, {0: 290, 6: 285, 12: 229}),
    (FREE_M, 4, 3, 2, None, None, {0: 245, 14: 239, 28: 187}),
    (OPTIMISTIC, 4, 2, 1, 567, 471, {12: 245}),
)
SCENE_GRID = tuple((clear, h, r, s) for clear in (FREE_M, OPTIMISTIC) for h, r, s in
                   ((1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (2, 1, 0), (2, 1, 1), (4, 2, 1), (4, 3, 2), (8, 0, 0), (5, 2, 4), (32, 8, 4)))


def scene_classes():
    """the scene's classes over the region, from the issue's list, in its order"""
    c = np.full(SCENE_DIMS, R.FREE, np.uint8)
    c[:, :, 0] = R.UNKNOWN
    c[:, :, 1] = R.OCCUPIED
    c[12:, :, 2] = R.OCCUPIED
    c[18:, :, 3:5] = R.OCCUPIED
    c[2:6, 2:6, 5] = R.OCCUPIED
    c[9, 9, 2:11] = R.OCCUPIED
    c[2:5, 14:17, 1] = R.UNKNOWN
    c[16:24, 16:24, 8:16] = R.MISSING
    return c


def scene_padded(h, r, s):
    """the classes of the scene's padded box: MISSING outside the 18 blocks"""
    below, _ = pads(h, r, s)
    p = np.full(padded_dims(SCENE_DIMS, h, r, s), R.MISSING, np.uint8)
    p[tuple(slice(b, b + d) for b, d in zip(below, SCENE_DIMS))] = scene_classes()
    return p


def scene_stream(params, cls_name="BGKOctoMap", swap=None):
    """the scene as a map stream: every cell a finest-level leaf; `swap` {class: class} replaces classes (the BGK-LV scene
    has UNCERTAIN where this one has UNKNOWN)"""
    import pack_cases as P
    assert int(params["block_depth"]) == 4
    h = P.header_fields(cls_name, params)
    npb, fine = P.npb_of(4), P.base(3)
    cls = scene_classes()
    for a, b in (swap or {}).items():
        cls = np.where(scene_classes() == a, np.uint8(b), cls)
    blocks = [(bi, bj, bk) for bi in range(3) for bj in range(3) for bk in range(2) if (bi, bj, bk) != SCENE_LEFT_OUT]
    nb = len(blocks)
    A = np.full((nb, npb), np.float32(h["init_A"]), np.float32)
    B = np.full((nb, npb), np.float32(h["init_B"]), np.float32)
    St = np.full((nb, npb), P.UNKNOWN, np.uint8)
    x, y, z = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    node = np.zeros((8, 8, 8), np.int64)
    for level in (2, 1, 0):
        node = node * 8 + ((((x >> level) & 1) << 2) | (((y >> level) & 1) << 1) | ((z >> level) & 1))
    keys = []
    for t, (bi, bj, bk) in enumerate(blocks):
        sub = cls[8 * bi:8 * bi + 8, 8 * bj:8 * bj + 8, 8 * bk:8 * bk + 8]
        St[t, fine + node.reshape(-1)] = sub.reshape(-1)
        occ = (sub == R.OCCUPIED).reshape(-1)
        A[t, fine + node.reshape(-1)] = np.where(occ, np.float32(5.0), np.float32(0.001))
        B[t, fine + node.reshape(-1)] = np.where(occ, np.float32(0.001), np.float32(5.0))
        keys.append(((524288 + bi) << 40) | ((524288 + bj) << 20) | (524288 + bk))
    return P.stream_from_pool(h, np.array(keys, np.int64), A, B, St)


# ---- small shapes: frontier_cases' SHAPES, WORD_SHAPES and LONG_SHAPES ----------------------------------------------------------
# (h, r, s): PZ = nz + h + 2s.  h = 1 keeps nz = 31 and 63 at PZ = 32 and 64, columns that end with a word and with a wave; the
# others (PZ = nz + 2, nz + 6, nz + 7) make every column straddle them
SHAPE_PARAMS = ((1, 0, 0), (2, 0, 0), (4, 2, 1), (3, 1, 2))


def shape_offset(stand, shape):
    """Where in a region whose standing voxels are `stand` (from the yardstick) a small region of `shape` goes, so that it
    holds ground: the standing voxel of the fullest layer with the most standing voxels in the 5 x 5 round it comes to lie
    at most 2 voxels (3 along z) inside the shape, or in the middle of an axis longer than the region.  May be negative."""
    k = int(stand.sum((0, 1)).argmax())
    layer = np.pad(stand[:, :, k].astype(np.int32), 2)
    dense = sum(layer[2 + di:2 + di + stand.shape[0], 2 + dj:2 + dj + stand.shape[1]] for di in range(-2, 3) for dj in range(-2, 3))
    i, j = np.unravel_index(int(np.where(stand[:, :, k], dense, 0).argmax()), dense.shape)
    at = (int(i), int(j), k)
    inside = (2, 2, 3)
    return tuple(a - (n // 2 if n > big else min(n - 1, m)) for a, n, big, m in zip(at, shape, stand.shape, inside))


# ---- the two-scan map ---------------------------------------------------------------------------------------------------
RECIPE = dict(support=OCC_M, clear=OPTIMISTIC, h=4, r=2, s=1)


def input_conditions(pcls_of, dims):
    """counted from the yardstick, never from the code under test; pcls_of(h, r, s) = the classes of the padded box"""
    q = RECIPE
    p = pcls_of(q["h"], q["r"], q["s"])
    y = {c: yardstick(p, dims, q["support"], q["clear"], q["h"], q["r"], q["s"], c) for c in (0, 6, 12)}
    plain = yardstick(pcls_of(2, 0, 0), dims, OCC_M, FREE_M, 2, 0, 0)
    return dict(n_stand=y[0]["n_stand"], n_body=y[0]["n_body"], foot0=y[0]["n"], foot6=y[6]["n"], foot12=y[12]["n"], plain=plain["n"])


def assert_exercises_the_feature(cond):
    """at least half of each non-zero figure counted on region_cases.fused_map(3) over the recipe region (n_stand 1067, n_body
    694, foot 694 / 458 / 0 at c = 0 / 6 / 12; 147 with clear = FREE, h = 2, r = 0): the margin the other region tests use
    between that map and the product's; and c = 6 strictly between c = 0 and c = 12"""
    print(f"footing input conditions: {cond}")
    assert cond["n_stand"] >= 534 and cond["n_body"] >= 347 and cond["foot0"] >= 347 and cond["foot6"] >= 229 and cond["plain"] >= 74, cond
    assert cond["foot12"] < cond["foot6"] < cond["foot0"], cond
