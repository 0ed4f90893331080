"""The yardstick of tests/test_evict_cpu.py and tests/test_evict_gpu.py: the region test on block keys, the sub-stream of a
parsed stream for a region, the pool order after erase_region by the hole / tail rule and the resulting stream — numpy on
top of helpers/pack_cases.py, written from the contract comment in include/la3dm_hip.h (la3dm_devmap_pack_region_host),
not from the kernels; nothing here calls pack_region, erase_region or evict.

A stream's block order stands for the pool's slot order: a device map that unpacked a stream holds block b in slot b."""
import numpy as np

import pack_cases as P

FIELD_MAX = 0xFFFFF
EVERYTHING = ((0, 0, 0), (FIELD_MAX, FIELD_MAX, FIELD_MAX))


def key_fields(keys):
    """[n, 3] the x, y, z fields of block keys: bits 59..40, 39..20, 19..0"""
    k = np.asarray(keys, np.int64).reshape(-1)
    return np.stack([(k >> 40) & FIELD_MAX, (k >> 20) & FIELD_MAX, k & FIELD_MAX], axis=1)


def make_keys(x, y, z):
    return (np.asarray(x, np.int64) << 40) | (np.asarray(y, np.int64) << 20) | np.asarray(z, np.int64)


def selected(keys, klo, khi, inside):
    """bool per key: in the closed box klo <= k <= khi (inside) or not in it (not inside)"""
    klo, khi = np.asarray(klo, np.int64), np.asarray(khi, np.int64)
    assert klo.shape == (3,) and khi.shape == (3,) and (klo <= khi).all(), "klo > khi is refused, not a region"
    f = key_fields(keys)
    in_box = ((f >= klo) & (f <= khi)).all(axis=1)
    return in_box if inside else ~in_box


def take_blocks(stream, order):
    """the stream of the blocks `order` (indices into the stream's blocks) in that order, each block's mask and leaves as
    they stand"""
    p = P.parse(stream)
    order = np.asarray(order, np.int64).reshape(-1)
    off = p["leaf_off"].astype(np.int64) if p["n_blocks"] else np.zeros(1, np.int64)
    leaves = np.concatenate([np.arange(off[b], off[b + 1]) for b in order]) if order.size else np.zeros(0, np.int64)
    return P.write(P.header_of(p), p["keys"][order], p["mask"][order], p["state"][leaves], p["A"][leaves], p["B"][leaves])


def sub_stream(stream, klo, khi, inside):
    """pack_region: the selected blocks in the stream's own order"""
    sel = selected(P.parse(stream)["keys"], klo, khi, inside)
    return take_blocks(stream, np.nonzero(sel)[0])


def compact_order(removed):
    """(order, n_moved): order[s] = the old slot whose block the new slot s holds.  n_new = n_old - n_removed; survivors below
    n_new stay; the holes (removed slots < n_new, ascending) take the tail survivors (surviving slots >= n_new, ascending)
    pairwise"""
    removed = np.asarray(removed, bool).reshape(-1)
    n_new = int(removed.size - removed.sum())
    holes = np.nonzero(removed[:n_new])[0]
    tail = n_new + np.nonzero(~removed[n_new:])[0]
    assert holes.size == tail.size
    order = np.arange(n_new)
    order[holes] = tail
    return order, int(holes.size)


def erased_stream(stream, klo, khi, inside):
    """(stream, stats) after erase_region: pack of the pool the contract describes"""
    p = P.parse(stream)
    removed = selected(p["keys"], klo, khi, inside)
    order, n_moved = compact_order(removed)
    return take_blocks(stream, order), dict(n_removed=int(removed.sum()), n_moved=n_moved, n_blocks=int(order.size))


# ---- pools whose slots a box can pick out ----
PATTERNS = ("nothing", "everything", "last slot", "slot 0", "first half", "second half", "alternating", "most removed",
            "all but one box")
X_IN, X_OUT = 1000, 2000


def pattern_flags(name, n, rng):
    """bool per slot: the slots the pattern selects"""
    s = np.arange(n)
    if name == "nothing":
        return np.zeros(n, bool)
    if name == "everything":
        return np.ones(n, bool)
    if name == "last slot":
        return s == n - 1
    if name == "slot 0":
        return s == 0
    if name == "first half":          # every hole is filled from the tail: the most moves
        return s < (n + 1) // 2
    if name == "second half":         # no moves
        return s >= n // 2
    if name == "alternating":
        return s % 2 == 0
    if name == "most removed":        # n_removed > n_new, and the tail itself holds removed blocks
        f = rng.random(n) < 0.7
        f[-1] = f[0] = True
        if n > 2:
            f[n // 2] = False
        return f
    if name == "all but one box":     # inside = 0 of a one-block box: every slot but one in the middle
        return s != n // 2
    raise KeyError(name)


def pattern_case(name, n, rng):
    """(keys[n], klo, khi, inside, flags): distinct keys in no order such that the region selects exactly the pattern's slots"""
    flags = pattern_flags(name, n, rng)
    y = 524288 - 300 + rng.permutation(4 * n + 8)[:n]
    z = rng.integers(0, 1 << 20, n)
    if name == "all but one box":
        keys = make_keys(rng.integers(0, 1 << 20, n), y, z)
        f = key_fields(keys[n // 2])[0]
        region = (tuple(int(v) for v in f), tuple(int(v) for v in f), 0)
    else:
        keys = make_keys(np.where(flags, X_IN, X_OUT), y, z)
        region = ((X_IN, 0, 0), (X_IN, FIELD_MAX, FIELD_MAX), 1)
    assert (selected(keys, *region) == flags).all()
    return keys, region[0], region[1], region[2], flags


def stable_pool(rng, h, nb, collapse, keys):
    """P.random_pool made stable under merge's prune: no coarse leaf is UNKNOWN (it would be split for good) and in every
    sibling group child 0 is FREE and child 1 OCCUPIED where they are leaves (no group collapses)"""
    keys, A, B, S = P.random_pool(rng, h, nb, collapse, keys=keys)
    depth = int(h["block_depth"])
    m = P.leaf_mask(S, depth)
    for d in range(depth):
        for i in range(8 ** d):
            n = P.base(d) + i
            rows = m[:, n]
            want = None
            if d and i % 8 < 2:
                want = i % 8
            if d < depth - 1 and want is None:
                S[rows, n] = (S[rows, n] & 0x80) | (S[rows, n] & 1)          # FREE or OCCUPIED
            elif want is not None:
                S[rows, n] = (S[rows, n] & 0x80) | want
    return keys, A, B, S


def assert_merge_restores(stream):
    """the condition under which evict followed by merge of the stream gives the map back: no leaf carries the default A, B
    with another state byte than the default node's (merge keeps such a cell default), no coarse leaf is UNKNOWN and no
    complete sibling group of leaves has one state other than UNKNOWN (merge's prune would split / collapse them)"""
    p = P.parse(stream)
    bits = lambda x: np.asarray(x, np.float32).view(np.uint32)   # noqa: E731
    default = (bits(p["A"]) == bits(np.float32(p["init_A"]))) & (bits(p["B"]) == bits(np.float32(p["init_B"])))
    assert not (default & (p["state"] != P.UNKNOWN)).any(), "a default-valued leaf with a non-default state byte"
    depth = p["block_depth"]
    keys, A, B, S = P.canonical_pool(stream)
    m = p["mask"]
    assert not (m[:, :P.base(depth - 1)] & ((S[:, :P.base(depth - 1)] & 7) == P.UNKNOWN)).any(), "an UNKNOWN coarse leaf"
    for d in range(1, depth):
        g = slice(P.base(d), P.base(d + 1))
        leaves = m[:, g].reshape(m.shape[0], -1, 8)
        st = (S[:, g] & 7).reshape(m.shape[0], -1, 8)
        same = leaves.all(axis=2) & (st == st[:, :, :1]).all(axis=2) & (st[:, :, 0] != P.UNKNOWN)
        assert not same.any(), "a sibling group that merge's prune would collapse"
