"""The yardstick of tests/test_merge_cpu.py and tests/test_merge_gpu.py: merge_ref, the fusion of two map streams in numpy
float32, written from the contract comment of la3dm_devmap_merge_host in include/la3dm_hip.h alone — the covering leaves of
both sides per finest cell, the three cases (kept, copied, fused), the prune in which the parent takes child 0's whole S
byte, the canonical form, new blocks behind the old ones in stream order — and the hand-built pairs of streams both test
files run.  It is built on pack_cases.py and calls nothing of the library.  Every comparison against it is exact.

Values: A and B of hand-built leaves are finite and lie in [init, 1e4] (or are the default node bit for bit), so no fused
sum overflows or is NaN; states are drawn at will, consistent with the values or not."""
import numpy as np

import pack_cases as P

KEPT, COPIED, FUSED = 0, 1, 2
CLASSIFIED = 0x80


def cover_cells(A, B, S, depth):
    """(A, B, S) [nb, 8^(depth - 1)]: the covering leaf of every finest cell — climb while PRUNED"""
    nb = S.shape[0]
    dl = depth - 1
    ncell = 8 ** dl
    d = np.full((nb, ncell), dl, np.int64)
    i = np.tile(np.arange(ncell, dtype=np.int64), (nb, 1))
    rows = np.arange(nb)[:, None]
    base = np.array([P.base(k) for k in range(depth + 1)], np.int64)
    for _ in range(dl):
        up = ((S[rows, base[d] + i] & 7) == P.PRUNED) & (d > 0)
        d = np.where(up, d - 1, d)
        i = np.where(up, i >> 3, i)
    n = base[d] + i
    return A[rows, n], B[rows, n], S[rows, n]


def classify(A, B, thresholds):
    """Occupancy::update's state in float32 with IEEE divisions: var = (A B) / ((s s)(s + 1)), p = A / s"""
    free, occ, vt = (np.float32(t) for t in thresholds)
    with np.errstate(all="ignore"):
        s = A + B
        var = (A * B) / ((s * s) * (s + np.float32(1)))
        p = A / s
    assert var.dtype == np.float32 and p.dtype == np.float32
    return np.where(var > vt, 2, np.where(p > occ, 1, np.where(p < free, 0, 2))).astype(np.uint8), var, p


def fuse_cells(one, two, a0, b0, thresholds):
    """the rule per finest cell: one = the map's (A1, B1, S1), two = the stream's; -> (A, B, S, case)"""
    A1, B1, S1 = one
    A2, B2, S2 = two
    bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)   # noqa: E731
    a0, b0 = np.float32(a0), np.float32(b0)
    none2 = (bits(A2) == bits(a0)) & (bits(B2) == bits(b0))
    none1 = (bits(A1) == bits(a0)) & (bits(B1) == bits(b0))
    case = np.where(none2, KEPT, np.where(none1, COPIED, FUSED))
    with np.errstate(all="ignore"):
        fA = A1 + (A2 - a0)
        fB = B1 + (B2 - b0)
    assert fA.dtype == np.float32
    fS = classify(fA, fB, thresholds)[0] | CLASSIFIED
    pick = lambda k, c, f: np.where(case == KEPT, k, np.where(case == COPIED, c, f))   # noqa: E731
    return pick(A1, A2, fA), pick(B1, B2, fB), pick(S1, S2, fS).astype(np.uint8), case


def prune_and_write(cA, cB, cS, depth, a0, b0):
    """the blocks of the cells' results, pruned bottom up (eight sibling leaves of one state other than UNKNOWN collapse; the
    parent takes child 0's A, B and whole S byte) and written in canonical form"""
    nb = cS.shape[0]
    dl, npb = depth - 1, P.npb_of(depth)
    fine = P.base(dl)
    T = np.full((nb, npb), P.UNKNOWN, np.uint8)      # a node above the leaves is UNKNOWN and never a leaf
    src = np.zeros((nb, npb), np.int64)               # the finest cell a leaf has its values from
    T[:, fine:] = cS
    src[:, fine:] = np.arange(8 ** dl)
    for d in range(dl, 0, -1):
        lb, pb, ng = P.base(d), P.base(d - 1), 8 ** (d - 1)
        g = T[:, lb:lb + 8 * ng].reshape(nb, ng, 8)
        st = g & 7
        ok = (st[:, :, 0] != P.PRUNED) & (st[:, :, 0] != P.UNKNOWN) & (st == st[:, :, :1]).all(2)
        T[:, pb:pb + ng] = np.where(ok, g[:, :, 0], T[:, pb:pb + ng])
        src[:, pb:pb + ng] = np.where(ok, src[:, lb:lb + 8 * ng:8], src[:, pb:pb + ng])
        T[:, lb:lb + 8 * ng] = np.where(np.repeat(ok, 8, axis=1), P.PRUNED, T[:, lb:lb + 8 * ng])
    st = T & 7
    is_fine = np.arange(npb) >= fine
    leaf = (st != P.PRUNED) & (is_fine | (st != P.UNKNOWN))
    rows = np.arange(nb)[:, None]
    A = np.where(leaf, cA[rows, src], np.float32(a0)).astype(np.float32)
    B = np.where(leaf, cB[rows, src], np.float32(b0)).astype(np.float32)
    S = np.where(leaf, T, np.where(st == P.PRUNED, P.PRUNED, P.UNKNOWN)).astype(np.uint8)
    return A, B, S


def merge_ref(dst_stream, src_stream, thresholds, details=None):
    """(stream, stats) of src_stream merged into the map dst_stream: the map's blocks in their order (those the stream names
    rewritten, the others in canonical form), then the created blocks in the stream's order.  thresholds = (free_thresh,
    occupied_thresh, var_thresh) of the map.  details (a dict) receives case [n_src, cells] and the fused cells' var and p"""
    pd, ps = P.parse(dst_stream), P.parse(src_stream)
    depth = pd["block_depth"]
    assert ps["block_depth"] == depth and ps["variant"] == pd["variant"] and (ps["float_bits"][:3] == pd["float_bits"][:3]).all()
    a0, b0 = np.float32(pd["init_A"]), np.float32(pd["init_B"])
    kd, Ad, Bd, Sd = P.canonical_pool(dst_stream)
    ks, As, Bs, Ss = P.canonical_pool(src_stream)
    nd, ns, ncell = kd.size, ks.size, 8 ** (depth - 1)
    where = {int(k): r for r, k in enumerate(kd)}
    row = np.array([where.get(int(k), -1) for k in ks], np.int64)
    created = row < 0
    two = cover_cells(As, Bs, Ss, depth)
    one = [np.full((ns, ncell), a0, np.float32), np.full((ns, ncell), b0, np.float32), np.full((ns, ncell), P.UNKNOWN, np.uint8)]
    if (~created).any():
        have = cover_cells(Ad[row[~created]], Bd[row[~created]], Sd[row[~created]], depth)
        for x, y in zip(one, have):
            x[~created] = y
    cA, cB, cS, case = fuse_cells(one, two, a0, b0, thresholds)
    A, B, S = prune_and_write(cA, cB, cS, depth, a0, b0)
    n_new = int(created.sum())
    row[created] = nd + np.arange(n_new)
    keys = np.concatenate([kd, ks[created]])
    oA, oB, oS = (np.concatenate([x, np.zeros((n_new, x.shape[1]), x.dtype)]) for x in (Ad, Bd, Sd))
    oA[row], oB[row], oS[row] = A, B, S
    stats = dict(n_blocks=ns, n_created=n_new, cells_kept=int((case == KEPT).sum()), cells_copied=int((case == COPIED).sum()),
                 cells_fused=int((case == FUSED).sum()))
    if details is not None:
        _, var, p = classify(cA, cB, thresholds)
        details.update(case=case, var=var[case == FUSED], p=p[case == FUSED], rows=row, created=created)
    return P.stream_from_pool(P.header_of(pd), keys, oA, oB, oS), stats


# ---- hand-built inputs -------------------------------------------------------------------------------------------------
def near_keys(rng, nb):
    """distinct block keys round the origin of the key lattice, in no order"""
    cell = rng.permutation(32 ** 3)[:nb]
    f = [524288 - 16 + ((cell >> s) & 31).astype(np.int64) for s in (10, 5, 0)]
    return (f[0] << 40) | (f[1] << 20) | f[2]


def evidence(rng, n, h, p_default=0.3, small=False):
    """n pairs (A, B) in [init, 1e4]: the default node bit for bit with probability p_default; else each of A, B is small
    (init .. 0.05: sums whose variance straddles a small var_thresh), middling (0.1 .. 10, ratios on both sides of the
    thresholds) or large (up to 1e4); small: every value small"""
    a0, b0 = np.float32(h["init_A"]), np.float32(h["init_B"])

    def draw(lo):
        kind = rng.integers(0, 1 if small else 3, n)
        v = np.where(kind == 0, 10.0 ** rng.uniform(-3, -1.3, n), np.where(kind == 1, rng.uniform(0.1, 10.0, n), 10.0 ** rng.uniform(1, 4, n)))
        return np.clip(v.astype(np.float32), lo, np.float32(1e4))
    A, B = draw(a0), draw(b0)
    none = rng.random(n) < p_default
    return np.where(none, a0, A).astype(np.float32), np.where(none, b0, B).astype(np.float32)


def pool(rng, h, keys, collapse, p_default=0.3, small=False):
    """a canonical pool over the tiling of `collapse` [nb, npb]: leaf states random among FREE, OCCUPIED, UNKNOWN with bit 7 both
    ways (consistent with the values or not), A / B from evidence()"""
    depth = int(h["block_depth"])
    m = P.tiling(depth, collapse)
    nb, npb = m.shape
    nl = int(m.sum())
    A = np.full((nb, npb), np.float32(h["init_A"]), np.float32)
    B = np.full((nb, npb), np.float32(h["init_B"]), np.float32)
    S = np.where(P.under_leaf(m, depth), P.PRUNED, P.UNKNOWN).astype(np.uint8)
    S[m] = rng.integers(0, 3, nl).astype(np.uint8) | (rng.integers(0, 2, nl).astype(np.uint8) << 7)
    A[m], B[m] = evidence(rng, nl, h, p_default, small)
    return np.asarray(keys, np.int64), A, B, S


def uniform_pool(h, keys, collapse, A, B, S):
    """a canonical pool over the tiling of `collapse` whose every leaf is (A, B, S)"""
    depth = int(h["block_depth"])
    m = P.tiling(depth, collapse)
    pa = np.full(m.shape, np.float32(h["init_A"]), np.float32)
    pb = np.full(m.shape, np.float32(h["init_B"]), np.float32)
    ps = np.where(P.under_leaf(m, depth), P.PRUNED, P.UNKNOWN).astype(np.uint8)
    pa[m], pb[m], ps[m] = np.float32(A), np.float32(B), S
    return np.asarray(keys, np.int64), pa, pb, ps


def empty_stream(h):
    return P.write(h, [], np.zeros((0, P.npb_of(int(h["block_depth"]))), bool), [], [], [])


def _rows(depth, nb, rng, row=None, p=0.0):
    npb = P.npb_of(depth)
    c = rng.random((nb, npb)) < p
    if row is not None:
        c[:] = row
    return c


def shape_cases(h, rng):
    """[(name, dst_stream, src_stream)]: stream block counts 1, 3, 4, 5, 9 against a destination that is empty, disjoint from
    the stream, equal to it (same keys) and half overlapping; the stream's blocks in shuffled order; random tilings"""
    depth = int(h["block_depth"])
    out = []
    for ns in (1, 3, 4, 5, 9):
        keys = near_keys(rng, 2 * ns + 2)
        src_keys = keys[:ns]
        for rel, dst_keys in (("empty", keys[:0]), ("disjoint", keys[ns:2 * ns + 2]), ("equal", rng.permutation(src_keys)),
                              ("half overlapping", rng.permutation(np.concatenate([src_keys[:(ns + 1) // 2], keys[ns:ns + 2]])))):
            src = P.stream_from_pool(h, *pool(rng, h, src_keys, _rows(depth, ns, rng, p=0.2)))
            nd = dst_keys.size
            dst = P.stream_from_pool(h, *pool(rng, h, dst_keys, _rows(depth, nd, rng, p=0.2))) if nd else empty_stream(h)
            out.append((f"{ns} stream blocks, destination {rel}", dst, src))
    # weak evidence on both sides of the same 9 blocks: fused sums whose variance lies round 0.25 / (s + 1), on both sides of a
    # small var_thresh
    keys = near_keys(rng, 9)
    weak = [P.stream_from_pool(h, *pool(rng, h, keys, _rows(depth, 9, rng), 0.0, True)) for _ in range(2)]
    out.append(("9 blocks of weak evidence on both sides", weak[0], weak[1]))
    return out


def tiling_cases(h, rng):
    """[(name, dst_stream, src_stream)] over the same 3 keys on both sides (block_depth >= 2): both sides un-pruned; either side
    collapsed to the root against the other un-pruned; one mid-layer group collapsed on either side; a fuse that makes the
    eight siblings of one group agree; one that makes every cell agree (the chain collapses to the root: two levels at
    block_depth 3, three at 4); one cell changed under a coarse leaf, which splits it; a source that is the default node
    everywhere (kept, also under a coarse destination leaf); a destination that is (copied verbatim)"""
    depth = int(h["block_depth"])
    npb, dl = P.npb_of(depth), depth - 1
    ncell, fine = 8 ** dl, P.base(dl)
    a0, b0 = np.float32(h["init_A"]), np.float32(h["init_B"])
    keys = near_keys(rng, 3)
    flat = np.zeros((3, npb), bool)
    root = flat.copy()
    root[:, 0] = True
    mk = lambda c, p=0.3: P.stream_from_pool(h, *pool(rng, h, keys, c, p))   # noqa: E731
    out = [("both sides un-pruned", mk(flat), mk(flat)),
           ("destination collapsed to the root, source un-pruned", mk(root), mk(flat)),
           ("destination un-pruned, source collapsed to the root", mk(flat), mk(root))]
    for layer in range(1, depth):
        one = np.repeat(P.one_group_collapsed(depth, layer), 3, axis=0)
        out.append((f"one group of layer {layer} collapsed in the destination", mk(one), mk(flat)))
        out.append((f"one group of layer {layer} collapsed in the source", mk(flat), mk(one)))
        out.append((f"one group of layer {layer} collapsed on both sides", mk(one), mk(one)))
    out.append(("random tilings on both sides", mk(_rows(depth, 3, rng, p=0.3)), mk(_rows(depth, 3, rng, p=0.3))))
    # every source leaf the default node: kept — under un-pruned, root-collapsed and random destinations
    none = P.stream_from_pool(h, *uniform_pool(h, keys, flat, a0, b0, P.UNKNOWN))
    none_root = P.stream_from_pool(h, *uniform_pool(h, keys, root, a0, b0, 0x81))   # (the state of a kept-out leaf is not looked at)
    out.append(("source all default, destination collapsed to the root", mk(root, 0.0), none))
    out.append(("source all default and collapsed, destination random", mk(_rows(depth, 3, rng, p=0.3)), none_root))
    # every destination leaf the default node: copied verbatim, odd states and bit 7 both ways
    out.append(("destination all default, source random", none, mk(_rows(depth, 3, rng, p=0.3), 0.0)))
    out.append(("destination all default and collapsed, source un-pruned", none_root, mk(flat, 0.0)))
    # fuses that change the tiling.  Destination: OCCUPIED cells (5, 0.5) with one FREE cell (0.5, 5); the source adds 100 to that
    # cell's A and nothing elsewhere: p = 100.5 / 105.5 -> OCCUPIED, so its group agrees; with every other cell OCCUPIED the
    # chain collapses to the root, with one other group's cell UNKNOWN only the lower levels do
    odd = ncell - 1 if ncell > 1 else 0
    for name, spoil in (("every cell agrees after the fuse: the chain collapses to the root", False),
                        ("one group agrees after the fuse, another keeps an UNKNOWN cell", True)):
        k, A, B, S = uniform_pool(h, keys, flat, 5.0, 0.5, 0x81)
        A[:, fine + odd], B[:, fine + odd], S[:, fine + odd] = 0.5, 5.0, 0x80
        if spoil and ncell > 8:
            S[:, fine] = P.UNKNOWN | CLASSIFIED
        k2, A2, B2, S2 = uniform_pool(h, keys, flat, a0, b0, P.UNKNOWN)
        A2[:, fine + odd], S2[:, fine + odd] = 100.0, 0x81
        out.append((name, P.stream_from_pool(h, k, A, B, S), P.stream_from_pool(h, k2, A2, B2, S2)))
    # one cell fused under a coarse FREE leaf (the root): the leaf splits, the other cells keep its bytes
    k, A, B, S = uniform_pool(h, keys, root, 0.5, 7.0, 0x00)
    k2, A2, B2, S2 = uniform_pool(h, keys, flat, a0, b0, P.UNKNOWN)
    cell = fine + (19 % ncell)
    A2[:, cell], S2[:, cell] = 50.0, 0x81
    out.append(("one cell fused under a coarse leaf splits it", P.stream_from_pool(h, k, A, B, S), P.stream_from_pool(h, k2, A2, B2, S2)))
    return out


def cases(h, seed=0):
    """every hand-built pair for a map with header fields h"""
    rng = np.random.default_rng(1000 * int(h["block_depth"]) + 10 * int(h["variant"]) + seed)
    out = shape_cases(h, rng)
    if int(h["block_depth"]) >= 2:
        out += tiling_cases(h, rng)
    return out


def conditions(h, thresholds, all_cases):
    """counted from the yardstick alone: how often each case and each side of each threshold occurs among all_cases"""
    free, occ, vt = (np.float32(t) for t in thresholds)
    c = dict(kept=0, copied=0, fused=0, p_below_free=0, p_between=0, p_above_occ=0, var_above=0, var_below=0, created=0, collapsed=0, split=0)
    depth = int(h["block_depth"])
    for _, dst, src in all_cases:
        d = {}
        ref, st = merge_ref(dst, src, thresholds, d)
        c["kept"] += st["cells_kept"]
        c["copied"] += st["cells_copied"]
        c["fused"] += st["cells_fused"]
        c["created"] += st["n_created"]
        c["var_above"] += int((d["var"] > vt).sum())
        c["var_below"] += int((d["var"] <= vt).sum())
        low = d["var"] <= vt
        c["p_below_free"] += int((d["p"][low] < free).sum())
        c["p_above_occ"] += int((d["p"][low] > occ).sum())
        c["p_between"] += int(((d["p"][low] >= free) & (d["p"][low] <= occ)).sum())
        # tilings: leaves per named block before (in the destination) and after
        pr, pdst = P.parse(ref), P.parse(dst)
        after = pr["mask"][d["rows"]].sum(1)
        before = np.full(after.shape, 8 ** (depth - 1))
        old = ~d["created"]
        if old.any():
            before[old] = pdst["mask"][d["rows"][old]].sum(1)
        c["collapsed"] += int((after < before).sum())
        c["split"] += int((after > before).sum())
    return c
