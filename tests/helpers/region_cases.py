"""The recipe map, the recipe region and the independent yardstick shared by tests/test_region_cpu.py and
tests/test_region_gpu.py.

Nothing in `yardstick` calls box or columns: it builds the table (block_key, node_key) -> leaf from `m.leaves()`, walks
the region's lattice in integer arithmetic, climbs (depth, index >> 3) until a leaf is found and reduces along k with
numpy."""
import ctypes as C

import numpy as np

from conftest import pcd_path

FREE, OCCUPIED, UNKNOWN, MISSING, UNCERTAIN = 0, 1, 2, 3, 4
BOX_FIELDS = ("cls", "leaf_depth", "A", "B")
COL_FIELDS = ("counts", "low_occ", "top_occ")
INFO_FIELDS = ("origin", "block_key", "cell")
YAML = dict(resolution=0.1, block_depth=3, sf2=1.0, ell=0.2, free_thresh=0.3, occupied_thresh=0.7, var_thresh=100.0,
            prior_A=0.001, prior_B=0.001)
RECIPE_OFFSET = (-4.03, -4.03, -1.53)
RECIPE_DIMS = (80, 80, 40)


def _emulate_device(pk, params):
    """what la3dm_bgk_scan_* computes, done with the oracle's predict + node update (as in tests/test_host_logic.py)"""
    from oracle import oracle as O
    o = O.OracleMap(**params)
    lut = np.concatenate(o.lut())
    base = [(8 ** d - 1) // 7 for d in range(8)]
    a, b, s = C.c_float(), C.c_float(), C.c_uint8()
    for t in range(pk.n_test_blk):
        l0, l1 = int(pk.leaf_off[t]), int(pk.leaf_off[t + 1])
        keys = pk.leaf_key[l0:l1]
        xs = lut[[base[k >> 16] + (k & 0xFFFF) for k in keys]] + pk.blk_center[t]
        for nb in pk.nbr[t]:
            if nb < 0:
                continue
            p0, p1 = int(pk.train_off[nb]), int(pk.train_off[nb + 1])
            yb, kb = O.bgk_predict(params["sf2"], params["ell"], xs, pk.train_xyzy[p0:p1, :3], pk.train_xyzy[p0:p1, 3])
            for j in np.nonzero(kb > 0)[0]:
                a.value, b.value, s.value = pk.alpha[l0 + j], pk.beta[l0 + j], pk.state[l0 + j] & 3
                o.L.orc_node_update(o.h, C.byref(a), C.byref(b), C.byref(s), float(yb[j]), float(kb[j]))
                pk.alpha[l0 + j], pk.beta[l0 + j], pk.state[l0 + j] = a.value, b.value, s.value | 0x80


_MAPS = {}


def fused_map(depth):
    """sim_structured scans 1 and 2, fused and pruned on a bookkeeping-only (host-mode, device = -1) map; returns the map,
    its leaves and the recipe's lo"""
    if depth not in _MAPS:
        import la3dm_amd
        params = dict(YAML, block_depth=depth)
        m = la3dm_amd.BGKOctoMap(**params, device=-1)
        for i in (1, 2):
            xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
            assert m.prepare(xyz, origin, 0.1, 0.5, 8.0)
            _emulate_device(m.packed(), params)
            m.commit()
        lv = m.leaves()
        assert (lv["node_key"] >> 16).min() < depth - 1          # pruning produced coarse leaves
        _MAPS[depth] = (m, lv, recipe_lo())
    return _MAPS[depth]


def recipe_lo():
    import la3dm_amd
    _, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 1))
    return (np.asarray(origin, np.float32) + np.asarray(RECIPE_OFFSET, np.float32)).astype(np.float32)


def anchor(lo, resolution, depth):
    """block fields, cells and global indices of the voxel that holds lo, and its centre — in the number formats of the
    contract: the block field in float64, the cell and the centre in float32"""
    res = np.float32(resolution)
    lim = 1 << (depth - 1)
    bs = np.float32(np.float32(2.0 ** (depth - 1)) * res)
    b, c, origin = [], [], []
    for k in range(3):
        v = np.float32(lo[k])
        bk = int(np.float64(v) / np.float64(bs) + 524288.5)
        center = np.float32(np.float32(bk - 524288) * bs)
        t = int(np.float32(np.float32(np.float32(v - center) / res) + np.float32(lim // 2)))      # truncation
        ck = max(0, min(t, lim - 1))
        off = np.float32(0)              # the LUT entry of the cell along this axis (init_key_loc_map: float64 steps, float32 kept)
        for d in range(depth - 1):
            half = np.float32(np.float64(res) * 2.0 ** (depth - d - 1) * 0.5)
            off = np.float32(np.float64(off) + np.float64(half) * (0.5 if (ck >> (depth - 2 - d)) & 1 else -0.5))
        b.append(bk)
        c.append(ck)
        origin.append(np.float32(off + center))
    return b, c, [bk * lim + ck for bk, ck in zip(b, c)], np.array(origin, np.float32)


def _cell_index(cx, cy, cz, levels):
    idx = np.zeros_like(cx)
    for level in range(levels - 1, -1, -1):
        idx = idx * 8 + ((((cx >> level) & 1) << 2) | (((cy >> level) & 1) << 1) | ((cz >> level) & 1))
    return idx


def yardstick(m, lv, lo, dims, a0=None, b0=None):
    """box and columns of the region from the leaf list; dict with the box fields, the columns fields, the info and
    `under_coarser` (voxels of an existing block whose covering leaf is coarser than the finest layer)"""
    depth, res = int(m.get_block_depth()), m.get_resolution()
    dl, lim = depth - 1, 1 << (depth - 1)
    if a0 is None:
        _, a0, b0, _ = m.search(1.0e4, 1.0e4, 1.0e4)       # what search answers for a missing block: the default node
    b, c, g0, origin = anchor(lo, res, depth)
    nx, ny, nz = dims
    gx = (g0[0] + np.arange(nx, dtype=np.int64))[:, None, None]
    gy = (g0[1] + np.arange(ny, dtype=np.int64))[None, :, None]
    gz = (g0[2] + np.arange(nz, dtype=np.int64))[None, None, :]
    key = np.broadcast_to(((gx // lim) << 40) | ((gy // lim) << 20) | (gz // lim), dims).reshape(-1)
    cell = np.broadcast_to(_cell_index(gx % lim, gy % lim, gz % lim, dl), dims).reshape(-1)
    blocks = np.unique(lv["block_key"])
    ordinal = np.searchsorted(blocks, key)
    exists = (ordinal < blocks.size) & (blocks[np.minimum(ordinal, blocks.size - 1)] == key) if blocks.size else np.zeros(key.size, bool)
    leaf_code = (np.searchsorted(blocks, lv["block_key"]).astype(np.int64) << 20) | lv["node_key"].astype(np.int64)
    order = np.argsort(leaf_code)
    sorted_code = leaf_code[order]
    n = key.size
    cls = np.full(n, MISSING, np.uint8)
    leaf_depth = np.full(n, 255, np.uint8)
    A = np.full(n, np.float32(a0), np.float32)
    B = np.full(n, np.float32(b0), np.float32)
    todo = np.nonzero(exists)[0]
    d, idx = dl, cell[todo]
    while todo.size:
        assert d >= 0, "an existing block has a leaf over every finest cell"
        code = (ordinal[todo].astype(np.int64) << 20) | (d << 16) | idx
        pos = np.minimum(np.searchsorted(sorted_code, code), sorted_code.size - 1)
        found = sorted_code[pos] == code
        li = order[pos[found]]
        at = todo[found]
        cls[at], leaf_depth[at], A[at], B[at] = lv["state"][li], d, lv["A"][li], lv["B"][li]
        todo, idx, d = todo[~found], idx[~found] >> 3, d - 1
    out = dict(cls=cls.reshape(dims), leaf_depth=leaf_depth.reshape(dims), A=A.reshape(dims), B=B.reshape(dims))
    out.update(reduce_box(out["cls"]))
    out.update(origin=origin, block_key=(b[0] << 40) | (b[1] << 20) | b[2], cell=np.array(c, np.int32))
    out["under_coarser"] = exists.reshape(dims) & (out["leaf_depth"] < dl)
    return out


def reduce_box(cls):
    """columns from a box's cls: the definition"""
    nz = cls.shape[2]
    counts = np.stack([(cls == FREE).sum(2), (cls == OCCUPIED).sum(2), ((cls == UNKNOWN) | (cls == UNCERTAIN)).sum(2),
                       (cls == MISSING).sum(2)], 2).astype(np.uint32)
    occ = cls == OCCUPIED
    any_occ = occ.any(2)
    low = np.where(any_occ, occ.argmax(2), -1).astype(np.int32)
    top = np.where(any_occ, nz - 1 - occ[:, :, ::-1].argmax(2), -1).astype(np.int32)
    return dict(counts=counts, low_occ=low, top_occ=top)


def assert_same(a, b, fields, what=""):
    """exact: integers by ==, floats by their bits"""
    for k in fields:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        bad = np.argwhere(x != y)
        assert bad.shape[0] == 0, (what, k, bad.shape[0], bad[:5].tolist(), np.asarray(a[k])[tuple(bad[0])], np.asarray(b[k])[tuple(bad[0])])


def input_conditions(y, depth):
    """counted from the yardstick, never from the code under test"""
    cls, cnt, under = y["cls"], y["counts"], y["under_coarser"]
    nz = cls.shape[2]
    return dict(free=int((cls == FREE).sum()), occupied=int((cls == OCCUPIED).sum()), unknown=int((cls == UNKNOWN).sum()),
                missing=int((cls == MISSING).sum()), coarser_occ=int((under & (cls == OCCUPIED)).sum()),
                coarser_free=int((under & (cls == FREE)).sum()), cols_occ=int((cnt[:, :, 1] > 0).sum()),
                cols_free_only=int(((cnt[:, :, 0] > 0) & (cnt[:, :, 1] == 0)).sum()), cols_missing=int((cnt[:, :, 3] == nz).sum()),
                cell=tuple(int(v) for v in y["cell"]), lim=1 << (depth - 1))


def assert_region_exercises_the_feature(cond):
    """at least half of what was counted on the restatement's map (the margin the ray tests use between that map and the
    product's), and an anchor that is not on a block corner"""
    print(f"region input conditions: {cond}")
    assert cond["free"] >= 8000 and cond["occupied"] >= 3000 and cond["unknown"] >= 20000 and cond["missing"] >= 70000, cond
    assert cond["coarser_occ"] >= 900 and cond["coarser_free"] >= 4500, cond
    assert cond["cols_occ"] >= 450 and cond["cols_free_only"] >= 500 and cond["cols_missing"] >= 1400, cond
    assert all(v != 0 for v in cond["cell"]), cond          # the region is not aligned to the blocks on any axis
