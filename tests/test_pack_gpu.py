"""save / load on the device-resident map (csrc/devmap_pack.h): the pool's covering leaves compacted into the stream on the
GPU, and the stream expanded into the canonical pool.  The yardstick is tests/helpers/pack_cases.py (a numpy writer, parser
and expander written from the layout comment in include/la3dm_hip.h); every comparison is exact, floats by their bits.  No
test here feeds a kernel a corrupt stream: the validator is host code that runs before any launch (tests/test_pack_cpu.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, pcd_path

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import pack_cases as P  # noqa: E402

pytestmark = pytest.mark.gpu

OK = 0
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured
LEAF_FIELDS = ("block_key", "node_key", "loc", "size", "A", "B", "state", "classified")
_LENDERS = {}


def _same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    assert a.size == b.size, (what, a.size, b.size)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, (what, bad.size, bad[:8].tolist())


def _lender(cls, params):
    """a host-mode map that lends its context to bare device maps"""
    import la3dm_amd
    key = (cls, tuple(sorted(params.items())))
    if key not in _LENDERS:
        _LENDERS[key] = getattr(la3dm_amd, cls)(**params, device=0).set_device_resident(False)
    return _LENDERS[key]


class Devmap:
    """a bare la3dm_devmap on a lent context: the raw ABI"""

    def __init__(self, lender):
        from la3dm_amd import _lib
        self.H, self.ctx = _lib.hip(), lender.ctx()
        self.dm = C.c_void_p()
        assert self.H.la3dm_devmap_create(self.ctx, C.byref(self.dm)) == OK, self.err()

    def err(self):
        return self.H.la3dm_last_error(self.ctx).decode()

    def close(self):
        if self.dm:
            self.H.la3dm_devmap_destroy(self.dm)
            self.dm = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def insert(self, scan, insert):
        import la3dm_amd
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", scan))
        xyz = np.ascontiguousarray(xyz, np.float32)
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert self.H.la3dm_devmap_insert_pointcloud_host(self.dm, xyz.ctypes.data, xyz.shape[0], 3, o3, *insert, None) == OK, self.err()

    def counts(self):
        nb, npb = C.c_uint32(), C.c_uint32()
        assert self.H.la3dm_devmap_block_count(self.dm, C.byref(nb), C.byref(npb)) == OK
        return nb.value, npb.value

    def download(self):
        nb, npb = self.counts()
        keys, A, B, S = np.zeros(nb, np.int64), np.zeros((nb, npb), np.float32), np.zeros((nb, npb), np.float32), np.zeros((nb, npb), np.uint8)
        assert self.H.la3dm_devmap_download(self.dm, keys.ctypes.data, A.ctypes.data, B.ctypes.data, S.ctypes.data) == OK, self.err()
        return keys, A, B, S

    def pack_size(self):
        size = C.c_uint64(0)
        assert self.H.la3dm_devmap_pack_host(self.dm, None, 0, C.byref(size)) == OK, self.err()
        return int(size.value)

    def pack(self):
        n = self.pack_size()
        buf = np.full(n + 64, 0xAB, np.uint8)                 # (a guard behind the stream: nothing is written past it)
        size = C.c_uint64(0)
        assert self.H.la3dm_devmap_pack_host(self.dm, buf.ctypes.data, n, C.byref(size)) == OK, self.err()
        assert size.value == n and (buf[n:] == 0xAB).all()
        return buf[:n].copy()

    def unpack(self, stream):
        s = np.ascontiguousarray(stream, np.uint8)
        return self.H.la3dm_devmap_unpack_host(self.dm, s.ctypes.data, s.size)

    def search(self, xyz):
        q = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = q.shape[0]
        out = dict(exists=np.zeros(n, np.uint8), A=np.zeros(n, np.float32), B=np.zeros(n, np.float32), state=np.zeros(n, np.uint8))
        assert self.H.la3dm_devmap_search_host(self.dm, q.ctypes.data, n, *[out[k].ctypes.data for k in ("exists", "A", "B", "state")]) == OK
        return out


def _near_keys(rng, nb):
    """distinct block keys round the origin of the key lattice, in no order (the search points stay exactly representable)"""
    cell = rng.permutation(32 ** 3)[:nb]
    f = [524288 - 16 + ((cell >> s) & 31).astype(np.int64) for s in (10, 5, 0)]
    return (f[0] << 40) | (f[1] << 20) | f[2]


def _structures(depth, npb):
    """name -> collapse row: un-pruned, collapsed to the root, exactly one group collapsed at each layer"""
    out = {"un-pruned": np.zeros((1, npb), bool)}
    root = np.zeros((1, npb), bool)
    root[0, 0] = True
    out["collapsed to the root"] = root
    for layer in range(1, depth):
        out[f"one group of layer {layer} collapsed"] = P.one_group_collapsed(depth, layer)
    return out


def _hand_cases(depth):
    """(name, n_blocks, collapse [n_blocks, npb]): every structure alone in one block; 3 and 5 blocks (not a multiple of the
    waves per workgroup) that mix the structures with random tilings; at depth 3 the block counts round the scan's 4096-item
    tile (the scan runs over n_blocks + 1 counts) and 9000"""
    npb = P.npb_of(depth)
    rng = np.random.default_rng(depth)
    structs = _structures(depth, npb)
    cases = [(name, 1, c) for name, c in structs.items()]
    cases.append(("a random tiling", 1, rng.random((1, npb)) < 0.25))
    counts = [3, 5] + ([4095, 4096, 4097, 9000] if depth == 3 else [])
    for nb in counts:
        c = rng.random((nb, npb)) < 0.2
        rows = list(structs.values())
        for b in range(min(nb, len(rows))):
            c[b] = rows[b][0]
        cases.append((f"{nb} blocks, mixed", nb, c))
    return cases


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_hand_built_pools_through_the_raw_abi(built, depth):
    """GPU test 1: for every block_depth the device map accepts and every structure — un-pruned, collapsed to the root, exactly
    one group collapsed at each layer, random valid tilings — with the classified bit both ways and A / B random bit patterns
    (-0, denormals, NaN payloads): unpack_host then download == the helper's canonical pool, pack_host == the input stream
    (pool order is kept), buf = NULL returns the size, and search_host agrees with the canonical pool at cell centres"""
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    lender = _lender("BGKOctoMap", params)
    h = P.header_fields("BGKOctoMap", params)
    lut = lender.lut()[P.base(depth - 1):]
    rng = np.random.default_rng(1000 + depth)
    for name, nb, collapse in _hand_cases(depth):
        keys, A, B, S = P.random_pool(rng, h, nb, collapse, keys=_near_keys(rng, nb))
        stream = P.stream_from_pool(h, keys, A, B, S)
        P.assert_size_bound(stream)
        ck, cA, cB, cS = P.canonical_pool(stream)
        _same_bytes(cS, S, "the helper's own round trip")
        with Devmap(lender) as d:
            assert d.unpack(stream) == OK, (name, d.err())
            assert d.counts() == (nb, P.npb_of(depth))
            gk, gA, gB, gS = d.download()
            assert (gk == ck).all(), name
            _same_bytes(gS, cS, (depth, name, "S"))
            _same_bytes(gA, cA, (depth, name, "A"))
            _same_bytes(gB, cB, (depth, name, "B"))
            assert d.pack_size() == stream.size, name
            _same_bytes(d.pack(), stream, (depth, name, "pack"))
            # search at the centres of a few finest cells of a few blocks, and where no block is
            blocks = np.unique(np.concatenate([[0, nb - 1], rng.integers(0, nb, 6)]))
            cells = np.unique(np.concatenate([[0, 8 ** (depth - 1) - 1], rng.integers(0, 8 ** (depth - 1), 6)]))
            centres = np.stack([lender.hash_key_to_block(int(keys[b])) for b in blocks])
            q = (centres[:, None, :] + lut[cells][None, :, :]).reshape(-1, 3)
            got = d.search(np.concatenate([q, [[900.0, 900.0, 900.0]]]))
            node = P.base(depth - 1) + cells
            assert got["exists"][:-1].all() and got["exists"][-1] == 0
            _same_bytes(got["A"][:-1], cA[blocks][:, node], (depth, name, "search A"))
            _same_bytes(got["B"][:-1], cB[blocks][:, node], (depth, name, "search B"))
            assert (got["state"][:-1] == (cS[blocks][:, node] & 7).reshape(-1)).all(), name
            # a second stream is refused: the map holds blocks now
            assert d.unpack(stream) == -1 and "already holds blocks" in d.err()


def test_hand_built_lv_pool_and_empty_stream(built):
    """the BGK-LV state UNCERTAIN as a leaf state and the original_size flag through the raw ABI; an empty map packs to the header
    alone and unpacking that stream leaves the map empty"""
    import la3dm_amd
    params = dict(la3dm_amd.LV_YAML, block_depth=3)
    lender = _lender("BGKLVOctoMap", params)
    h = P.header_fields("BGKLVOctoMap", dict(params, original_size=False))   # (a bare device map starts with original_size set)
    rng = np.random.default_rng(5)
    keys, A, B, S = P.random_pool(rng, h, 6, rng.random((6, 73)) < 0.2, keys=_near_keys(rng, 6))
    assert ((S & 7) == P.UNCERTAIN).any()
    stream = P.stream_from_pool(h, keys, A, B, S)
    with Devmap(lender) as d:
        empty = d.pack()
        assert empty.size == 128 and P.parse(empty)["n_blocks"] == 0 and P.parse(empty)["flags"] == 1 and h["flags"] == 0
        assert d.unpack(empty) == OK and d.counts()[0] == 0
        assert d.unpack(stream) == OK, d.err()
        _same_bytes(d.download()[3], S, "LV S")
        _same_bytes(d.pack(), stream, "LV pack (the flag is the stream's)")


VARIANTS = {"BGKOctoMap d3": ("BGKOctoMap", "BGK_YAML", 3, INSERT), "BGKOctoMap d4": ("BGKOctoMap", "BGK_YAML", 4, INSERT),
            "GPOctoMap": ("GPOctoMap", "GP_YAML", None, INSERT), "BGKLOctoMap": ("BGKLOctoMap", "L_YAML", None, (0.1, 0.3, 8.0)),
            "BGKLVOctoMap": ("BGKLVOctoMap", "LV_YAML", None, (0.1, 0.3, 8.0))}


def _class_map(cls, params, scans, insert):
    import la3dm_amd
    m = getattr(la3dm_amd, cls)(**params, device=0)
    assert m.is_device_resident()
    for i in scans:
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        m.insert_pointcloud(xyz, origin, *insert)
    return m


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_real_maps(built, variant):
    """GPU test 2: two fused sim_structured scans.  Through the class: pack with mirror_syncs unchanged, unpack into a fresh
    device map, leaves() equal, box and frontier on the recipe region equal, a third scan into both gives equal leaves().
    Through the raw ABI (the same inserts into a bare device map): download of the loaded map == the helper's canonicalisation
    of the original's download; the stream == the helper's stream of the original's download, and it obeys the size bound.
    The map has coarse leaves and un-pruned blocks."""
    import la3dm_amd
    cls, yaml, depth, insert = VARIANTS[variant]
    params = dict(getattr(la3dm_amd, yaml))
    if depth:
        params["block_depth"] = depth
    depth = params["block_depth"]
    h = P.header_fields(cls, params)
    # raw ABI
    lender = _lender(cls, params)
    with Devmap(lender) as a, Devmap(lender) as b:
        for i in (1, 2):
            a.insert(i, insert)
        keys, A, B, S = a.download()
        leaves = P.leaf_mask(S, depth)
        assert leaves[:, :P.base(depth - 1)].any(), "coarse leaves exist"
        assert leaves[:, P.base(depth - 1):].all(axis=1).any(), "un-pruned blocks exist"
        want = P.stream_from_pool(h, keys, A, B, S)
        stream = a.pack()
        as_packed = stream.copy()
        if cls == "GPOctoMap":     # (the raw ABI writes the inverses of the context's 1 / x; the class its arguments: below)
            assert np.allclose(stream[104:116].view(np.float32), want[104:116].view(np.float32), rtol=1e-6)
            stream[104:116] = want[104:116]
        _same_bytes(stream, want, (variant, "pack vs helper"))
        total, raw = P.assert_size_bound(stream)
        print(f"{variant}: {keys.size} blocks, {int(leaves.sum())} leaves, stream {total} bytes, raw pool {raw} bytes ({total / raw:.3f})")
        _same_bytes(a.download()[3], S, "pack changes nothing in the pool")
        assert b.unpack(stream) == OK, b.err()
        ck, cA, cB, cS = P.canonicalise(h, keys, A, B, S)
        gk, gA, gB, gS = b.download()
        assert (gk == ck).all()
        _same_bytes(gS, cS, (variant, "S"))
        _same_bytes(gA, cA, (variant, "A"))
        _same_bytes(gB, cB, (variant, "B"))
        _same_bytes(b.pack(), as_packed, (variant, "pack of the loaded map"))
    # the class
    m = _class_map(cls, params, (1, 2), insert)
    syncs = m.mirror_syncs()
    packed = m.pack()
    assert m.mirror_syncs() == syncs
    # (two maps given the same scans hold the same blocks, but new blocks take their pool slots in no fixed order)
    _same_bytes(P.sorted_by_key(packed), P.sorted_by_key(want), (variant, "class pack vs helper"))
    copy = getattr(la3dm_amd, cls)(**params, device=0).unpack(packed)
    assert copy.is_device_resident() and copy.mirror_syncs() == 0
    lo = R.recipe_lo()
    R.assert_same(copy.box(lo, R.RECIPE_DIMS), m.box(lo, R.RECIPE_DIMS), R.BOX_FIELDS, variant)
    fa, fb = m.frontier(lo, R.RECIPE_DIMS), copy.frontier(lo, R.RECIPE_DIMS)
    assert fa["n"] == fb["n"] > 0 and (fa["index"] == fb["index"]).all() and (fa["nbrs"] == fb["nbrs"]).all()
    assert m.mirror_syncs() == syncs and copy.mirror_syncs() == 0
    lv = m.leaves()
    assert lv["A"].size > 0
    R.assert_same(copy.leaves(), lv, LEAF_FIELDS, (variant, "leaves"))
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 3))
    for x in (m, copy):
        x.insert_pointcloud(xyz, origin, *insert)
    after = m.leaves()
    assert after["A"].size != lv["A"].size or (after["A"].view(np.uint32) != lv["A"].view(np.uint32)).any()
    R.assert_same(copy.leaves(), after, LEAF_FIELDS, (variant, "leaves after a third scan"))
    _same_bytes(P.sorted_by_key(copy.pack()), P.sorted_by_key(m.pack()), (variant, "streams after a third scan"))


@pytest.mark.parametrize("depth", [3, 4])
def test_both_modes_write_one_stream(built, depth, tmp_path):
    """GPU test 3: the same inserts into a device-resident and a host-mode map: the two streams are byte-identical once in key
    order; the host stream loads into a device map and the device stream into a host map with equal leaves(); the device map
    loaded from the host stream continues with a third scan exactly as the original; save / load_map on the GPU"""
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    md = _class_map("BGKOctoMap", params, (1, 2), INSERT)
    mh = la3dm_amd.BGKOctoMap(**params, device=0).set_device_resident(False)
    for i in (1, 2):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        mh.insert_pointcloud(xyz, origin, *INSERT)
    sd, sh = md.pack(), mh.pack()
    _same_bytes(P.sorted_by_key(sh), sh, "the host writer's order is ascending key")
    _same_bytes(P.sorted_by_key(sd), sh, "device stream == host stream in key order")
    lv = mh.leaves()
    from_host = la3dm_amd.BGKOctoMap(**params, device=0).unpack(sh)
    from_dev = la3dm_amd.BGKOctoMap(**params, device=0).set_device_resident(False).unpack(sd)
    assert from_host.is_device_resident() and not from_dev.is_device_resident()
    R.assert_same(from_host.leaves(), lv, LEAF_FIELDS, "host stream in a device map")
    R.assert_same(from_dev.leaves(), lv, LEAF_FIELDS, "device stream in a host map")
    path = str(tmp_path / "map.la3dm")
    md.save(path)
    _same_bytes(np.fromfile(path, np.uint8), sd, "file bytes")
    lm = la3dm_amd.load_map(path)
    assert lm.is_device_resident() and type(lm).__name__ == "BGKOctoMap"
    _same_bytes(lm.pack(), sd, "load_map keeps the pool order")
    assert not la3dm_amd.load_map(path, device_resident=False).is_device_resident()
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 3))
    fresh = la3dm_amd.BGKOctoMap(**params, device=0).unpack(sh)
    for x in (md, fresh):
        x.insert_pointcloud(xyz, origin, *INSERT)
    R.assert_same(fresh.leaves(), md.leaves(), LEAF_FIELDS, "continuation on the device side")


def test_refusals_that_need_a_gpu(built):
    """GPU test 4: unpack into a device map that holds blocks, and a stream of another block_depth: both refused with a message,
    both leave the map usable"""
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=3)
    m = _class_map("BGKOctoMap", params, (1,), INSERT)
    stream, lv = m.pack(), m.leaves()
    with pytest.raises(RuntimeError, match="already holds blocks"):
        m.unpack(stream)
    R.assert_same(m.leaves(), lv, LEAF_FIELDS, "the refused map is unchanged")
    _same_bytes(m.pack(), stream, "and packs as before")
    other = la3dm_amd.BGKOctoMap(**dict(params, block_depth=4), device=0)
    with pytest.raises(RuntimeError, match="block_depth"):
        other.unpack(stream)
    assert other.pack().size == 128
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 1))
    other.insert_pointcloud(xyz, origin, *INSERT)
    assert other.leaves()["A"].size > 0
    empty = la3dm_amd.BGKOctoMap(**params, device=0)
    empty.unpack(stream)
    R.assert_same(empty.leaves(), lv, LEAF_FIELDS, "the valid stream is accepted")


def test_example_program(built, tmp_path):
    """examples/resume_map on two scans: saved, loaded into a second object, the frontier lists agree, no mirror refresh"""
    exe = os.path.join(ROOT, "examples", "resume_map")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "2"] +
                       "0.1 3 1.0 0.2 0.5 0.1 8.0 0.3 0.7 100.0 0.001 0.001 0".split() + [str(tmp_path / "resume_map.la3dm")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    line = r.stdout.strip().splitlines()[-1]
    assert "lists agree" in line and line.endswith("mirror_syncs 0 0 device_resident 1") and "frontier 0 /" not in line, r.stdout
