"""The yardstick of tests/test_diff_cpu.py and tests/test_diff_gpu.py: diff_ref, the comparison of a map (NOW, given as its
pack()) with a stream (THEN) in numpy, written from the contract comment of la3dm_devmap_diff_host in include/la3dm_hip.h
alone — the compared blocks and their order, the class of the covering leaf of every finest cell on both sides, MISSING for
an absent side, the 5 x 5 pair table, the value-changed cells, the selection and the list — and the hand-built pairs of
streams both test files run.  It is built on pack_cases.py (parser, canonical pool, tilings, random pools) and calls nothing
of the library.  Every comparison against it is exact, floats by their bits."""
import numpy as np

import pack_cases as P

MISSING = 3
PAIRS_CHANGED = sum(1 << (5 * t + n) for t in range(5) for n in range(5) if t != n)
STAT_KEYS = ("n_stream_blocks", "n_map_only_blocks", "n_missing_now")


def pair_bit(then, now):
    return 1 << (5 * then + now)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def cells(stream):
    """(keys [nb], cls, A, B [nb, 8^(depth - 1)]): per finest cell c the class (S & 7) and the values of its covering leaf —
    from node (depth - 1, c) up while the node is PRUNED"""
    p = P.parse(stream)
    depth = p["block_depth"]
    keys, A, B, S = P.canonical_pool(stream)
    nb, dl = keys.size, depth - 1
    ncell = 8 ** dl
    node = np.tile(P.base(dl) + np.arange(ncell, dtype=np.int64), (nb, 1))
    rows = np.arange(nb)[:, None]
    for d in range(dl, 0, -1):   # a PRUNED node of layer d hands over to its parent
        up = (node >= P.base(d)) & ((S[rows, node] & 7) == P.PRUNED)
        node = np.where(up, P.base(d - 1) + ((node - P.base(d)) >> 3), node)
    cls = S[rows, node] & 7
    assert (cls != P.PRUNED).all()
    return keys, cls, A[rows, node], B[rows, node]


def diff_ref(now_stream, then_stream, pair_mask=PAIRS_CHANGED, value_mask=0, map_only=True, lut=None, centre_of=None):
    """the whole answer as a dict: n, block_key, cell, code, A, B (and centre, with lut = the map's LUT [npb, 3] float32 and
    centre_of(key) = the block's centre), pairs (5, 5), value_changed (5,), the three block counts.  The order of NOW's blocks
    in now_stream is the order pack() writes them, which is the order of the map-only blocks."""
    pn, pt = P.parse(now_stream), P.parse(then_stream)
    depth = pn["block_depth"]
    assert pt["block_depth"] == depth and pt["variant"] == pn["variant"] and (pt["float_bits"][:3] == pn["float_bits"][:3]).all()
    a0, b0 = np.float32(pn["init_A"]), np.float32(pn["init_B"])
    kn, cn, An, Bn = cells(now_stream)
    kt, ct, At, Bt = cells(then_stream)
    ncell = 8 ** (depth - 1)
    where = {int(k): r for r, k in enumerate(kn)}
    row = np.array([where.get(int(k), -1) for k in kt], np.int64)
    named = set(int(k) for k in kt)
    rest = np.array([r for r, k in enumerate(kn) if int(k) not in named], np.int64) if map_only else np.zeros(0, np.int64)
    nt, nr = kt.size, rest.size
    keys = np.concatenate([kt, kn[rest]]).astype(np.int64)
    then = np.full((nt + nr, ncell), MISSING, np.int64)
    now = np.full((nt + nr, ncell), MISSING, np.int64)
    A = np.full((nt + nr, ncell), a0, np.float32)
    B = np.full((nt + nr, ncell), b0, np.float32)
    both = np.zeros((nt + nr, ncell), bool)
    then[:nt] = ct
    have = row >= 0
    now[:nt][have], A[:nt][have], B[:nt][have] = cn[row[have]], An[row[have]], Bn[row[have]]
    now[nt:], A[nt:], B[nt:] = cn[rest], An[rest], Bn[rest]
    both[:nt][have] = True
    changed = np.zeros((nt + nr, ncell), bool)
    if value_mask:
        tA, tB = np.zeros((nt + nr, ncell), np.uint32), np.zeros((nt + nr, ncell), np.uint32)
        tA[:nt], tB[:nt] = bits(At).reshape(nt, ncell), bits(Bt).reshape(nt, ncell)
        changed = both & (then == now) & ((tA != bits(A).reshape(A.shape)) | (tB != bits(B).reshape(B.shape)))
    pairs = np.zeros((5, 5), np.uint64)
    np.add.at(pairs, (then.reshape(-1), now.reshape(-1)), 1)
    value_changed = np.bincount(now[changed], minlength=5).astype(np.uint64)
    sel = (((pair_mask >> (5 * then + now)) & 1) == 1) | (changed & (((value_mask >> now) & 1) == 1))
    b, c = np.nonzero(sel)   # row-major: the block order above, ascending c within a block
    out = dict(n=int(sel.sum()), block_key=keys[b], cell=c.astype(np.uint32), code=(then[b, c] | (now[b, c] << 4)).astype(np.uint8),
               A=A[b, c], B=B[b, c], pairs=pairs, value_changed=value_changed, n_stream_blocks=nt, n_map_only_blocks=nr,
               n_missing_now=int((~have).sum()))
    if lut is not None:
        centre_block = {int(k): np.asarray(centre_of(int(k)), np.float32) for k in set(keys[b].tolist())}
        fine = P.base(depth - 1)
        out["centre"] = (np.asarray(lut, np.float32)[fine + c] + np.array([centre_block[int(k)] for k in keys[b]], np.float32).reshape(-1, 3)).astype(np.float32)
    return out


# ---- hand-built inputs -------------------------------------------------------------------------------------------------
def near_keys(rng, nb):
    """distinct block keys round the origin of the key lattice, in no order"""
    cell = rng.permutation(32 ** 3)[:nb]
    f = [524288 - 16 + ((cell >> s) & 31).astype(np.int64) for s in (10, 5, 0)]
    return (f[0] << 40) | (f[1] << 20) | f[2]


def empty_stream(h):
    return P.write(h, [], np.zeros((0, P.npb_of(int(h["block_depth"]))), bool), [], [], [])


def _pool(rng, h, keys, collapse=None, p=0.25):
    depth = int(h["block_depth"])
    nb = len(keys)
    if collapse is None:
        collapse = rng.random((nb, P.npb_of(depth))) < p
    return P.random_pool(rng, h, nb, np.broadcast_to(collapse, (nb, P.npb_of(depth))), keys=np.asarray(keys, np.int64))


def _stream(h, pool, rows=None):
    if rows is not None:
        pool = tuple(np.ascontiguousarray(x[rows]) for x in pool)
    return P.stream_from_pool(h, *pool) if len(pool[0]) else empty_stream(h)


def union_case(h, rng, n):
    """(name, now, then) whose union has n blocks (n >= 3): then names blocks 0 .. n - 2, now holds blocks 1 .. n - 1 in another
    order — block 0 is missing now, block n - 1 is map-only; of the shared blocks every other one is identical, the rest have
    another tiling, other states and other values"""
    keys = near_keys(rng, n)
    then = _pool(rng, h, keys[:n - 1])
    other = _pool(rng, h, keys[1:])
    now = tuple(x.copy() for x in other)
    same = np.arange(1, n - 1, 2)   # then's rows that stay as they are; row r of then is row r - 1 of now
    for x, y in zip(now, then):
        x[same - 1] = y[same]
    return f"{n} blocks in the union", _stream(h, now, rng.permutation(n - 1)), _stream(h, then)


def tiling_cases(h, rng):
    """[(name, now, then)] over the same 3 keys on both sides (block_depth >= 2)"""
    depth = int(h["block_depth"])
    npb = P.npb_of(depth)
    keys = near_keys(rng, 3)
    flat, root = np.zeros((1, npb), bool), np.zeros((1, npb), bool)
    root[0, 0] = True
    mk = lambda c=None: _stream(h, _pool(rng, h, keys, c))   # noqa: E731
    out = [("then a single root leaf, now all finest cells", mk(flat), mk(root)),
           ("then all finest cells, now a single root leaf", mk(root), mk(flat)),
           ("leaves at mixed layers on both sides", mk(), mk())]
    for layer in range(1, depth):
        one = P.one_group_collapsed(depth, layer)
        out.append((f"one group of layer {layer} collapsed now", mk(one), mk(flat)))
        out.append((f"one group of layer {layer} collapsed then", mk(flat), mk(one)))
    same = mk()
    out.append(("identical blocks", same, same.copy()))
    return out


def value_case(h, rng):
    """(name, now, then): the same tilings and states on both sides; now differs from then in the lowest bit of B of every
    third leaf and in the lowest bit of A of every fifth"""
    keys = near_keys(rng, 3)
    k, A, B, S = _pool(rng, h, keys)
    then = P.stream_from_pool(h, k, A, B, S)
    m = P.leaf_mask(S, int(h["block_depth"]))
    leaf = np.flatnonzero(m.reshape(-1))
    A2, B2 = A.copy(), B.copy()
    B2.reshape(-1).view(np.uint32)[leaf[::3]] ^= 1
    A2.reshape(-1).view(np.uint32)[leaf[2::5]] ^= 1
    return "same classes, values one bit apart", P.stream_from_pool(h, k, A2, B2, S), then


def cases(h, seed=0, unions=(3, 4, 5, 6)):
    """every hand-built pair (name, now_stream, then_stream) for a map with header fields h; now_stream goes into the map by
    unpack, then_stream is what diff is given"""
    rng = np.random.default_rng(2000 * int(h["block_depth"]) + 10 * int(h["variant"]) + seed)
    k1 = near_keys(rng, 2)
    one = _pool(rng, h, k1[:1])
    out = [("one block, changed", _stream(h, _pool(rng, h, k1[:1])), _stream(h, one)),
           ("one stream block absent from the map", _stream(h, _pool(rng, h, k1[1:])), _stream(h, one)),
           ("the empty stream", _stream(h, one), empty_stream(h)),
           ("the empty map", empty_stream(h), _stream(h, one)),
           ("both empty", empty_stream(h), empty_stream(h))]
    out += [union_case(h, rng, n) for n in unions]
    out.append(value_case(h, rng))
    if int(h["block_depth"]) >= 2:
        out += tiling_cases(h, rng)
    return out


def conditions(all_cases, value_mask=0x1F):
    """counted from the yardstick alone: the pair table summed over all_cases (map_only on), the value-changed cells, the
    blocks missing now and the map-only blocks"""
    pairs, vc, missing, only = np.zeros((5, 5), np.uint64), np.zeros(5, np.uint64), 0, 0
    for _, now, then in all_cases:
        r = diff_ref(now, then, PAIRS_CHANGED, value_mask, True)
        pairs += r["pairs"]
        vc += r["value_changed"]
        missing += r["n_missing_now"]
        only += r["n_map_only_blocks"]
    return dict(pairs=pairs, value_changed=vc, n_missing_now=missing, n_map_only_blocks=only)


LIST_FIELDS = ("block_key", "cell", "code", "centre", "A", "B")


def assert_same(got, want, what, fields=LIST_FIELDS, cap=None):
    """a diff() dict against diff_ref's: n, the counts and the first min(n, cap) entries of every field both hold, bit for bit"""
    assert got["n"] == want["n"], (what, "n", got["n"], want["n"])
    for k in STAT_KEYS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert (np.asarray(got["pairs"]) == want["pairs"]).all(), (what, "pairs", got["pairs"], want["pairs"])
    assert (np.asarray(got["value_changed"]) == want["value_changed"]).all(), (what, "value_changed", got["value_changed"], want["value_changed"])
    m = want["n"] if cap is None else min(want["n"], cap)
    for f in fields:
        if f not in want or f not in got:
            continue
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f][:m])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, f, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.nonzero(g.view(np.uint8).reshape(-1) != w.view(np.uint8).reshape(-1))[0]
        assert bad.size == 0, (what, f, bad.size, bad[:8].tolist())
