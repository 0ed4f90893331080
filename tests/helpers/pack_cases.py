"""The yardstick of tests/test_pack_cpu.py and tests/test_pack_gpu.py: a numpy writer and parser of the map stream, the
leaf rule, the canonical-pool expansion, a generator of valid tilings, the key-order normaliser and the table of corrupt
streams.  Written from the layout comment in include/la3dm_hip.h (la3dm_devmap_pack_host), not from the implementation;
nothing here calls pack, unpack or pack_info.

A pool is (keys[nb] int64, A[nb, npb] float32, B[nb, npb] float32, S[nb, npb] uint8) in la3dm_devmap_download's depth-major
node numbering: node (d, i) is number (8^d - 1) / 7 + i, its children are (d + 1, 8 i + c)."""
import struct

import numpy as np

MAGIC = b"LA3DMAP\0"
HEADER = struct.Struct("<8s6I3Q16f8s")            # 128 bytes
assert HEADER.size == 128
FLOATS = ("init_A", "init_B", "resolution", "sf2", "ell", "free_thresh", "occupied_thresh", "var_thresh", "prior_A", "prior_B",
          "noise", "l", "min_var", "max_var", "max_known_var", "min_W")
PRUNED, UNKNOWN, UNCERTAIN = 3, 2, 4
VARIANT = dict(BGKOctoMap=0, GPOctoMap=1, BGKLVOctoMap=2, BGKLOctoMap=3)


def base(d):
    return (8 ** d - 1) // 7


def npb_of(depth):
    return base(depth)


def align16(v):
    return (v + 15) & ~15


def layout(nb, nl, npb):
    """byte offsets of the sections and the stream's size"""
    W = (npb + 31) // 32
    if nb == 0:
        return dict(W=W, keys=128, leaf_off=128, mask=128, state=128, A=128, B=128, total=128)
    keys = 128
    leaf_off = align16(keys + 8 * nb)
    mask = align16(leaf_off + 4 * (nb + 1))
    state = align16(mask + 4 * nb * W)
    A = align16(state + nl)
    B = align16(A + 4 * nl)
    return dict(W=W, keys=keys, leaf_off=leaf_off, mask=mask, state=state, A=A, B=B, total=align16(B + 4 * nl))


def header_fields(cls_name, params):
    """the header of a map of class `cls_name` constructed with `params` (the keyword arguments of its Python class)"""
    f32 = lambda v: float(np.float32(v))   # noqa: E731
    variant = VARIANT[cls_name]
    h = dict(variant=variant, block_depth=int(params["block_depth"]), flags=0)
    h.update({k: 0.0 for k in FLOATS})
    for k in ("resolution", "sf2", "ell", "free_thresh", "occupied_thresh"):
        h[k] = f32(params[k])
    if variant == 1:
        for k in ("noise", "l", "min_var", "max_var", "max_known_var"):
            h[k] = f32(params[k])
        h["init_A"], h["init_B"] = 0.0, float(np.float32(1.0) / np.float32(params["max_var"]))
    else:
        for k in ("var_thresh", "prior_A", "prior_B"):
            h[k] = f32(params[k])
        h["init_A"], h["init_B"] = h["prior_A"], h["prior_B"]
    if variant == 2:
        h["min_W"] = f32(params["min_W"])
        h["flags"] = 1 if params.get("original_size", True) else 0
    return h


def leaf_mask(S, depth):
    """the leaf rule over a pool's states [nb, npb]: not PRUNED, and on the finest layer or with child 0 PRUNED"""
    S = np.asarray(S, np.uint8)
    not_pruned = (S & 7) != PRUNED
    m = np.zeros(S.shape, bool)
    dl = depth - 1
    for d in range(depth):
        sl = slice(base(d), base(d + 1))
        if d == dl:
            m[:, sl] = not_pruned[:, sl]
        else:
            child0 = S[:, base(d + 1) + 8 * np.arange(8 ** d)]
            m[:, sl] = not_pruned[:, sl] & ((child0 & 7) == PRUNED)
    return m


def mask_words(mask):
    """[nb, npb] bool -> [nb, W] uint32, bit n % 32 of word n / 32"""
    nb, npb = mask.shape
    W = (npb + 31) // 32
    padded = np.zeros((nb, W * 32), np.uint8)
    padded[:, :npb] = mask
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").reshape(nb, W)


def write(h, keys, mask, state, A, B, total_bytes=None):
    """the stream of header fields h, block keys, the per-block node mask [nb, npb] and the leaf arrays in stream order"""
    keys = np.asarray(keys, "<i8").reshape(-1)
    nb = keys.size
    depth = int(h["block_depth"])
    npb = npb_of(depth)
    mask = np.asarray(mask, bool).reshape(nb, npb)
    nl = int(np.asarray(state).size)
    lay = layout(nb, nl, npb)
    buf = np.zeros(lay["total"], np.uint8)
    buf[:128] = np.frombuffer(HEADER.pack(MAGIC, h.get("version", 1), h.get("header_bytes", 128), h["variant"], depth,
                                          h.get("nodes_per_block", npb), h["flags"], nb, nl,
                                          lay["total"] if total_bytes is None else total_bytes,
                                          *[h[k] for k in FLOATS], b"\0" * 8), np.uint8)
    if nb:
        off = np.zeros(nb + 1, "<u4")
        off[1:] = np.cumsum(mask.sum(1))
        buf[lay["keys"]:lay["keys"] + 8 * nb] = keys.view(np.uint8)
        buf[lay["leaf_off"]:lay["leaf_off"] + 4 * (nb + 1)] = off.view(np.uint8)
        buf[lay["mask"]:lay["mask"] + 4 * nb * lay["W"]] = mask_words(mask).reshape(-1).view(np.uint8)
        buf[lay["state"]:lay["state"] + nl] = np.asarray(state, np.uint8)
        buf[lay["A"]:lay["A"] + 4 * nl] = np.ascontiguousarray(A, "<f4").view(np.uint8)
        buf[lay["B"]:lay["B"] + 4 * nl] = np.ascontiguousarray(B, "<f4").view(np.uint8)
    return buf


def stream_from_pool(h, keys, A, B, S):
    """the stream of a pool: its covering leaves, a block's in ascending node number"""
    m = leaf_mask(S, int(h["block_depth"]))
    return write(h, keys, m, np.asarray(S, np.uint8)[m], np.asarray(A, np.float32)[m], np.asarray(B, np.float32)[m])


def parse(stream):
    """dict of the header fields and the sections (mask as [nb, npb] bool, mask_words as stored)"""
    buf = np.ascontiguousarray(stream, np.uint8).reshape(-1)
    v = HEADER.unpack(buf[:128].tobytes())
    out = dict(magic=v[0], version=v[1], header_bytes=v[2], variant=v[3], block_depth=v[4], nodes_per_block=v[5], flags=v[6],
               n_blocks=v[7], n_leaves=v[8], total_bytes=v[9], reserved=v[26])
    out.update(dict(zip(FLOATS, v[10:26])))
    out["float_bits"] = buf[56:120].view("<u4").copy()
    nb, nl, npb = out["n_blocks"], out["n_leaves"], out["nodes_per_block"]
    lay = layout(nb, nl, npb)
    assert lay["total"] == buf.size == out["total_bytes"], (lay, buf.size, out["total_bytes"])
    W = lay["W"]
    out["layout"] = lay
    out["keys"] = buf[lay["keys"]:lay["keys"] + 8 * nb].view("<i8").copy()
    out["leaf_off"] = buf[lay["leaf_off"]:lay["leaf_off"] + 4 * (nb + 1) * (nb > 0)].view("<u4").copy()
    out["mask_words"] = buf[lay["mask"]:lay["mask"] + 4 * nb * W].view("<u4").reshape(nb, W).copy()
    bits = np.unpackbits(out["mask_words"].view(np.uint8).reshape(nb, 4 * W), axis=1, bitorder="little")
    assert not bits[:, npb:].any()
    out["mask"] = bits[:, :npb].astype(bool)
    out["state"] = buf[lay["state"]:lay["state"] + nl].copy()
    out["A"] = buf[lay["A"]:lay["A"] + 4 * nl].view("<f4").copy()
    out["B"] = buf[lay["B"]:lay["B"] + 4 * nl].view("<f4").copy()
    return out


def header_of(p):
    return {k: p[k] for k in ("variant", "block_depth", "flags") + FLOATS}


def under_leaf(mask, depth):
    """[nb, npb] bool: the node has a set ancestor"""
    nb = mask.shape[0]
    under = np.zeros(mask.shape, bool)
    above = np.zeros((nb, 1), bool)
    for d in range(depth):
        sl = slice(base(d), base(d + 1))
        under[:, sl] = above
        above = np.repeat(above | mask[:, sl], 8, axis=1)
    return under


def canonical_pool(stream):
    """(keys, A, B, S): a set node takes its leaf's values, a node under a leaf (init, PRUNED), every other (init, UNKNOWN)"""
    p = parse(stream)
    nb, npb = p["n_blocks"], p["nodes_per_block"]
    m = p["mask"]
    A = np.full((nb, npb), np.float32(p["init_A"]), np.float32)
    B = np.full((nb, npb), np.float32(p["init_B"]), np.float32)
    S = np.where(under_leaf(m, p["block_depth"]), PRUNED, UNKNOWN).astype(np.uint8)
    A[m], B[m], S[m] = p["A"], p["B"], p["state"]
    return p["keys"], A, B, S


def canonicalise(h, keys, A, B, S):
    """the canonical form of a downloaded pool"""
    return canonical_pool(stream_from_pool(h, keys, A, B, S))


def tiling(depth, collapse):
    """[nb, npb] bool mask of a valid tiling: top down, a node that is not under a leaf becomes one where collapse[b, n] is set
    or on the finest layer.  collapse all False: un-pruned; collapse[:, 0]: collapsed to the root"""
    collapse = np.asarray(collapse, bool)
    nb = collapse.shape[0]
    m = np.zeros((nb, npb_of(depth)), bool)
    above = np.zeros((nb, 1), bool)
    for d in range(depth):
        sl = slice(base(d), base(d + 1))
        m[:, sl] = ~above & (collapse[:, sl] | (d == depth - 1))
        above = np.repeat(above | m[:, sl], 8, axis=1)
    cover = sum(m[:, base(d):base(d + 1)].sum(1) * 8 ** (depth - 1 - d) for d in range(depth))
    assert (cover == 8 ** (depth - 1)).all()
    return m


def odd_values(rng, n):
    """n float32 of random bit patterns, with -0, denormals, infinities and NaN payloads among them"""
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0], np.uint32)
    k = min(n, special.size)
    bits[rng.permutation(n)[:k]] = special[:k]
    return bits.view(np.float32)


def random_pool(rng, h, nb, collapse, keys=None):
    """a canonical pool over the tiling of `collapse`: leaf states random among the variant's (classified bit both ways), A / B
    odd_values at the leaves"""
    depth = int(h["block_depth"])
    m = tiling(depth, collapse)
    npb = m.shape[1]
    if keys is None:   # distinct 60-bit keys, all three fields used, in no order
        keys = (rng.permutation(1 << 20)[:nb].astype(np.int64) << 40) | (rng.integers(0, 1 << 20, nb).astype(np.int64) << 20) | \
               rng.integers(0, 1 << 20, nb).astype(np.int64)
    states = np.array([0, 1, 2, 4] if h["variant"] == 2 else [0, 1, 2], np.uint8)
    nl = int(m.sum())
    A = np.full((nb, npb), np.float32(h["init_A"]), np.float32)
    B = np.full((nb, npb), np.float32(h["init_B"]), np.float32)
    S = np.where(under_leaf(m, depth), PRUNED, UNKNOWN).astype(np.uint8)
    S[m] = states[rng.integers(0, states.size, nl)] | (rng.integers(0, 2, nl).astype(np.uint8) << 7)
    A[m], B[m] = odd_values(rng, nl), odd_values(rng, nl)
    return np.asarray(keys, np.int64), A, B, S


def one_group_collapsed(depth, layer, group=None):
    """collapse row [1, npb]: exactly the sibling group `group` of `layer` (1 .. depth - 1) collapsed into its parent"""
    c = np.zeros((1, npb_of(depth)), bool)
    g = (8 ** (layer - 1)) // 2 if group is None else group
    c[0, base(layer - 1) + g] = True
    return c


def sorted_by_key(stream):
    """the same map with its blocks in ascending key order"""
    p = parse(stream)
    keys, A, B, S = canonical_pool(stream)
    order = np.argsort(keys, kind="stable")
    return stream_from_pool(header_of(p), keys[order], A[order], B[order], S[order])


def pool_of_leaves(h, lv, block_keys):
    """a pool with the leaves of `lv` (a map's leaves(): block_key, node_key = depth << 16 | index, A, B, state, classified) in
    the blocks `block_keys`, PRUNED under them and UNKNOWN above"""
    depth = int(h["block_depth"])
    keys = np.asarray(block_keys, np.int64)
    nb, npb = keys.size, npb_of(depth)
    order = np.argsort(keys)
    row = order[np.searchsorted(keys[order], lv["block_key"])]
    d, i = lv["node_key"] >> 16, lv["node_key"] & 0xFFFF
    node = (8 ** d.astype(np.int64) - 1) // 7 + i
    m = np.zeros((nb, npb), bool)
    m[row, node] = True
    A = np.full((nb, npb), np.float32(h["init_A"]), np.float32)
    B = np.full((nb, npb), np.float32(h["init_B"]), np.float32)
    S = np.where(under_leaf(m, depth), PRUNED, UNKNOWN).astype(np.uint8)
    A[row, node], B[row, node] = lv["A"], lv["B"]
    S[row, node] = lv["state"] | (lv["classified"].astype(np.uint8) << 7)
    return keys, A, B, S


def raw_pool_bytes(nb, npb):
    return nb * (8 + 9 * npb)


def assert_size_bound(stream):
    """per block 12 + 4 W + 9 L bytes; from block_depth 2 up never more than the raw pool"""
    p = parse(stream)
    nb, npb, depth = p["n_blocks"], p["nodes_per_block"], p["block_depth"]
    L = np.diff(p["leaf_off"].astype(np.int64)) if nb else np.zeros(0, np.int64)
    assert (L <= 8 ** (depth - 1)).all() and (L >= 1).all()
    payload = int((12 + 4 * p["layout"]["W"] + 9 * L).sum()) + (4 if nb else 0)
    assert payload <= p["total_bytes"] - 128 <= payload + 6 * 15
    if depth >= 2 and nb:
        assert payload - 4 <= raw_pool_bytes(nb, npb), (payload, raw_pool_bytes(nb, npb))
    return p["total_bytes"], raw_pool_bytes(nb, npb)


def corrupt_table(h, rng=None):
    """[(name, stream, fragment of the refusal)] for a map with header fields h (block_depth >= 3): every row is one defect
    away from `valid`, which is returned last as ("valid", stream, None)"""
    rng = np.random.default_rng(7) if rng is None else rng
    depth = int(h["block_depth"])
    npb = npb_of(depth)
    collapse = np.zeros((3, npb), bool)
    collapse[1] = one_group_collapsed(depth, depth - 1)[0]
    keys, A, B, S = random_pool(rng, h, 3, collapse)
    valid = stream_from_pool(h, keys, A, B, S)
    p = parse(valid)
    lay = p["layout"]
    rows = []

    def patched(name, frag, fn):
        b = valid.copy()
        fn(b)
        rows.append((name, b, frag))

    def put(b, at, fmt, v):
        b[at:at + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, v), np.uint8)

    patched("wrong magic", "magic", lambda b: put(b, 0, "<8s", b"LA3DMAQ\0"))
    patched("wrong version", "version", lambda b: put(b, 8, "<I", 2))
    rows.append(("truncated", valid[:-16].copy(), "total_bytes"))
    rows.append(("truncated inside the header", valid[:100].copy(), "truncated"))
    rows.append(("one byte too long", np.concatenate([valid, np.zeros(1, np.uint8)]), "total_bytes"))
    patched("duplicate key", "duplicate", lambda b: put(b, lay["keys"] + 16, "<q", int(keys[0])))
    patched("key field out of range", "out of range", lambda b: put(b, lay["keys"] + 8, "<q", int(keys[1]) | (1 << 60)))
    patched("negative key", "out of range", lambda b: put(b, lay["keys"] + 8, "<q", -1))
    patched("leaf_off off by one", "leaf_off", lambda b: put(b, lay["leaf_off"] + 4, "<I", int(p["leaf_off"][1]) + 1))
    patched("leaf_off[0] not 0", "leaf_off", lambda b: put(b, lay["leaf_off"], "<I", 1))
    last = lay["mask"] + 4 * (lay["W"] - 1)
    patched("mask bit past the end", "past", lambda b: put(b, last, "<I", int(p["mask_words"][0, -1]) | (1 << (npb % 32))))
    coarse = int(np.nonzero(p["mask"][1, :base(depth - 1)])[0][0])          # block 1's collapsed parent
    child = base(depth - 1) + 8 * (coarse - base(depth - 2))
    at = lay["mask"] + 4 * (lay["W"] + child // 32)
    patched("a leaf under a leaf", "under a leaf", lambda b: put(b, at, "<I", int(p["mask_words"][1, child // 32]) | (1 << (child % 32))))
    m = p["mask"].copy()
    m[2, npb - 1] = False                                                   # a finest leaf removed, the sections consistent
    keep = np.ones(p["n_leaves"], bool)
    keep[p["leaf_off"][3] - 1] = False
    rows.append(("a hole in the tiling", write(h, keys, m, p["state"][keep], p["A"][keep], p["B"][keep]), "tile"))
    patched("PRUNED as a leaf state", "PRUNED", lambda b: put(b, lay["state"], "<B", PRUNED))
    patched("state bits 3-6", "bits 3-6", lambda b: put(b, lay["state"] + 1, "<B", 0x41))
    if h["variant"] != 2:
        patched("a state the variant lacks", "unknown to the variant", lambda b: put(b, lay["state"] + 2, "<B", UNCERTAIN))
    assert lay["leaf_off"] - (lay["keys"] + 24) == 8                        # three keys leave eight bytes of padding
    patched("non-zero padding", "padding", lambda b: put(b, lay["leaf_off"] - 1, "<B", 1))
    patched("non-zero reserved byte", "reserved", lambda b: put(b, 127, "<B", 1))
    # valid streams of another map
    other = dict(h, block_depth=depth + 1)
    rows.append(("mismatching block_depth", stream_from_pool(other, *random_pool(rng, other, 2, np.zeros((2, npb_of(depth + 1)), bool))), "block_depth"))
    other = dict(h, variant=3 if h["variant"] == 0 else 0)
    rows.append(("mismatching variant", stream_from_pool(other, keys, A, B, S), "variant"))
    other = dict(h, resolution=float(np.nextafter(np.float32(h["resolution"]), np.float32(1))))
    rows.append(("mismatching resolution", stream_from_pool(other, keys, A, B, S), "resolution"))
    other = dict(h, init_B=float(np.nextafter(np.float32(h["init_B"]), np.float32(1))))
    rows.append(("mismatching prior", stream_from_pool(other, keys, A, B, S), "default node"))
    rows.append(("valid", valid, None))
    return rows
