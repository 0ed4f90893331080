"""pack_region / erase_region / evict on the device-resident map (csrc/devmap_evict.h) against tests/helpers/evict_cases.py,
the numpy yardstick written from the contract comment of la3dm_devmap_pack_region_host in include/la3dm_hip.h.  The maps are
built by unpack of hand-built streams, so block b of the stream is pool slot b and the slot order after an erase is known
exactly: every comparison is byte for byte.  Shapes: block_depth 1, 3 and 4 (1, 73 and 585 nodes per block: the S rows are
unaligned and the copy length is no multiple of 64); 1, 3, 4, 5, 64, 65 and 257 blocks (one wave, a partly filled workgroup
of four waves, several workgroups) and 4096 blocks, the smallest pool whose 4097 flags span two tiles of the one-launch scan
(kScanTile = 512 x 8, devmap_scan.h)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import pack_cases as P  # noqa: E402
import merge_cases as MC  # noqa: E402
import evict_cases as EC  # noqa: E402

pytestmark = pytest.mark.gpu

OK = 0
YAMLS = dict(BGKOctoMap="BGK_YAML", BGKLOctoMap="L_YAML", GPOctoMap="GP_YAML", BGKLVOctoMap="LV_YAML")
STAT_KEYS = ("n_removed", "n_moved", "n_blocks")
TWO_TILES = 4096
_LENDERS = {}


def _same_bytes(a, b, what):
    if isinstance(a, (bytes, bytearray)):
        a = np.frombuffer(a, np.uint8)
    a, b = np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    assert a.size == b.size, (what, a.size, b.size)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, (what, bad.size, bad[:8].tolist())


def _params(cls, depth):
    import la3dm_amd
    return dict(getattr(la3dm_amd, YAMLS[cls]), block_depth=depth)


def _lender(cls, params):
    """a host-mode map that lends its context to bare device maps"""
    import la3dm_amd
    key = (cls, tuple(sorted(params.items())))
    if key not in _LENDERS:
        _LENDERS[key] = getattr(la3dm_amd, cls)(**params, device=0).set_device_resident(False)
    return _LENDERS[key]


def _i3(v):
    return (C.c_int32 * 3)(*[int(x) for x in v])


class Devmap:
    """a bare la3dm_devmap on a lent context: the raw ABI"""

    def __init__(self, lender):
        from la3dm_amd import _lib
        self._lib = _lib
        self.H, self.ctx = _lib.hip(), lender.ctx()
        self.dm = C.c_void_p()
        assert self.H.la3dm_devmap_create(self.ctx, C.byref(self.dm)) == OK, self.err()

    def err(self):
        return self.H.la3dm_last_error(self.ctx).decode()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if self.dm:
            self.H.la3dm_devmap_destroy(self.dm)
            self.dm = None

    def counts(self):
        nb, npb = C.c_uint32(), C.c_uint32()
        assert self.H.la3dm_devmap_block_count(self.dm, C.byref(nb), C.byref(npb)) == OK
        return nb.value, npb.value

    def keys(self):
        nb, npb = self.counts()
        keys, A, B, S = np.zeros(nb, np.int64), np.zeros((nb, npb), np.float32), np.zeros((nb, npb), np.float32), np.zeros((nb, npb), np.uint8)
        if nb:
            assert self.H.la3dm_devmap_download(self.dm, keys.ctypes.data, A.ctypes.data, B.ctypes.data, S.ctypes.data) == OK, self.err()
        return keys

    def pack(self):
        size = C.c_uint64(0)
        assert self.H.la3dm_devmap_pack_host(self.dm, None, 0, C.byref(size)) == OK, self.err()
        buf = np.zeros(int(size.value), np.uint8)
        assert self.H.la3dm_devmap_pack_host(self.dm, buf.ctypes.data, buf.size, C.byref(size)) == OK, self.err()
        return buf

    def unpack(self, stream):
        s = np.ascontiguousarray(stream, np.uint8)
        return self.H.la3dm_devmap_unpack_host(self.dm, s.ctypes.data, s.size)

    def pack_region(self, klo, khi, inside):
        size = C.c_uint64(0)
        rc = self.H.la3dm_devmap_pack_region_host(self.dm, _i3(klo), _i3(khi), inside, None, 0, C.byref(size))
        if rc != OK:
            return rc, None
        buf = np.zeros(int(size.value), np.uint8)
        rc = self.H.la3dm_devmap_pack_region_host(self.dm, _i3(klo), _i3(khi), inside, buf.ctypes.data, buf.size, C.byref(size))
        return rc, buf

    def erase_region(self, klo, khi, inside, want_stats=True):
        st = self._lib.EraseStats()
        rc = self.H.la3dm_devmap_erase_region_host(self.dm, _i3(klo), _i3(khi), inside, C.byref(st) if want_stats else None)
        return rc, {k: int(getattr(st, k)) for k in STAT_KEYS}

    def exists(self, lender, keys):
        """search at the centre of the finest cell 0 of every block of `keys`"""
        q = (np.stack([lender.hash_key_to_block(int(k)) for k in keys]) + lender.lut()[-1]).astype(np.float32)
        ex = np.zeros(q.shape[0], np.uint8)
        out = [np.zeros(q.shape[0], t) for t in (np.float32, np.float32, np.uint8)]
        assert self.H.la3dm_devmap_search_host(self.dm, q.ctypes.data, q.shape[0], ex.ctypes.data, *[o.ctypes.data for o in out]) == OK, self.err()
        return ex.astype(bool)


def _pool_stream(h, name, n, seed, stable=False):
    rng = np.random.default_rng(seed)
    keys, klo, khi, inside, flags = EC.pattern_case(name, n, rng)
    collapse = rng.random((n, P.npb_of(int(h["block_depth"])))) < 0.1
    pool = EC.stable_pool(rng, h, n, collapse, keys) if stable else P.random_pool(rng, h, n, collapse, keys=keys)
    return P.stream_from_pool(h, *pool), klo, khi, inside, flags


def _check_case(lender, h, name, n, seed, probe=True):
    stream, klo, khi, inside, flags = _pool_stream(h, name, n, seed)
    what = (h["variant"], h["block_depth"], n, name)
    want_sub = EC.sub_stream(stream, klo, khi, inside)
    want_left, stats = EC.erased_stream(stream, klo, khi, inside)
    with Devmap(lender) as dev:
        assert dev.unpack(stream) == OK, (what, dev.err())
        before = dev.pack()
        _same_bytes(before, stream, (what, "slot order = stream order"))
        rc, sub = dev.pack_region(klo, khi, inside)
        assert rc == OK, (what, dev.err())
        _same_bytes(sub, want_sub, (what, "pack_region"))
        _same_bytes(dev.pack(), before, (what, "pack of the untouched map"))
        rc, got = dev.erase_region(klo, khi, inside)
        assert rc == OK, (what, dev.err())
        assert got == stats, (what, got, stats)
        assert dev.counts()[0] == stats["n_blocks"]
        _same_bytes(dev.pack(), want_left, (what, "pack after erase_region: the yardstick's slot order"))
        _same_bytes(dev.keys(), P.parse(want_left)["keys"], (what, "blk_key"))
        if probe:
            k = P.parse(stream)["keys"]
            pick = np.unique(np.concatenate([np.arange(0, n, max(1, n // 64)), [n - 1]]))
            assert (dev.exists(lender, k[pick]) == ~flags[pick]).all(), (what, "the rebuilt table finds exactly the survivors")
    return stats


CASES = [("BGKOctoMap", 1, (1, 3, 4, 5, 64, 65, 257)), ("BGKOctoMap", 3, (1, 3, 4, 5, 64, 65, 257)), ("BGKOctoMap", 4, (1, 3, 4, 5, 64, 65, 257)),
         ("BGKLOctoMap", 3, (5, 65)), ("GPOctoMap", 3, (5, 65)), ("BGKLVOctoMap", 3, (5, 65)), ("GPOctoMap", 4, (65,)), ("BGKLVOctoMap", 1, (65,))]


@pytest.mark.parametrize("cls,depth,counts", CASES, ids=[f"{c}-d{d}" for c, d, _ in CASES])
def test_every_pattern_through_the_raw_abi(built, cls, depth, counts):
    """every selection pattern at every block count: pack_region == the yardstick's sub-stream, pack of the untouched map
    unchanged, erase_region's stats, then pack and the downloaded keys == the yardstick's stream in its exact slot order, and
    one search per original block through the rebuilt table.  GP and BGK-LV pools carry their own default node, the LV state
    codes (UNCERTAIN) and the original_size flag in the header."""
    params = _params(cls, depth)
    lender = _lender(cls, params)
    with Devmap(lender) as dev:
        h = P.header_of(P.parse(dev.pack()))      # (the empty map's header: a GP context only knows the inverses of its variances)
    assert h["variant"] == P.VARIANT[cls] and h["block_depth"] == depth
    moved = removed = 0
    for n in counts:
        for k, name in enumerate(EC.PATTERNS):
            st = _check_case(lender, h, name, n, 1000 * depth + 10 * n + k)
            moved += st["n_moved"]
            removed += st["n_removed"]
    assert removed > 0 and (moved > 0 or max(counts) < 3)
    if cls == "BGKLVOctoMap":
        stream = _pool_stream(h, "alternating", 65, 3)[0]
        assert h["flags"] == 1 and ((P.parse(stream)["state"] & 7) == P.UNCERTAIN).any()


@pytest.mark.parametrize("depth", [1, 3])
def test_a_pool_whose_flags_span_two_scan_tiles(built, depth):
    """4096 blocks: 4097 flags, two tiles of the one-launch scan; the patterns with the most moves, alternating slots and a
    tail that holds removed blocks"""
    params = _params("BGKOctoMap", depth)
    lender = _lender("BGKOctoMap", params)
    h = P.header_fields("BGKOctoMap", params)
    for k, name in enumerate(("first half", "alternating", "most removed")):
        st = _check_case(lender, h, name, TWO_TILES, 40 + k)
        assert st["n_moved"] > 500


def _near_case(cls, depth, seed, stable=False, evidence=False):
    """a pool of 4 x 4 x 2 blocks round the origin of the key lattice in shuffled slot order, and the region x <= 524287"""
    params = _params(cls, depth)
    h = P.header_fields(cls, params)
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(-2, 2), np.arange(-2, 2), np.arange(-1, 1), indexing="ij"), -1).reshape(-1, 3) + 524288
    keys = EC.make_keys(*g[rng.permutation(g.shape[0])].T)
    n = keys.size
    collapse = rng.random((n, P.npb_of(depth))) < 0.1
    if evidence:
        pool = MC.pool(rng, h, keys, collapse)
    else:
        pool = EC.stable_pool(rng, h, n, collapse, keys) if stable else P.random_pool(rng, h, n, collapse, keys=keys)
    return params, h, P.stream_from_pool(h, *pool), (524288 - 2, 0, 0), (524288 - 1, EC.FIELD_MAX, EC.FIELD_MAX)


def _world(m, klo, khi):
    return m.hash_key_to_block(int(EC.make_keys(*klo))), m.hash_key_to_block(int(EC.make_keys(*np.minimum(khi, 524288 + 4096))))


def _dicts_equal(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if isinstance(a[k], np.ndarray):
            R.assert_same(a, b, (k,), (what, k))
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


@pytest.mark.parametrize("cls", ["BGKOctoMap", "BGKLVOctoMap"])
def test_the_table_and_the_queries_after_an_erase(built, cls):
    """the class on a device-resident map: after erase_region of half the lattice, search_many at a point in every original
    block (exists 0 in removed blocks, 1 elsewhere), box over a region that straddles the cut, frontier and raycast_many on
    it — each against a host-mode map and a fresh device-resident map that unpacked the yardstick's post-erase stream
    (MISSING where the blocks were removed); block_count; no mirror refresh for pack_region, erase_region or the queries"""
    import la3dm_amd
    depth = 3
    params, h, stream, klo, khi = _near_case(cls, depth, 11)
    want_left, stats = EC.erased_stream(stream, klo, khi, 1)
    assert 0 < stats["n_moved"] and stats["n_removed"] == 16
    make = lambda resident: getattr(la3dm_amd, cls)(**params, device=0).set_device_resident(resident)   # noqa: E731
    md, fresh, host = make(True).unpack(stream), make(True).unpack(want_left), make(False).unpack(want_left)
    lo, hi = _world(md, klo, khi)
    syncs = md.mirror_syncs()
    _same_bytes(md.pack_region(lo, hi), EC.sub_stream(stream, klo, khi, 1), "pack_region through the class")
    assert md.erase_region(lo, hi) == stats
    _same_bytes(md.pack(), want_left, "pack after the erase")
    keys = P.parse(stream)["keys"]
    q = (np.stack([md.hash_key_to_block(int(k)) for k in keys]) + md.lut()[-1]).astype(np.float32)
    ex = md.search_many(q)["exists"].astype(bool)
    assert (ex == ~EC.selected(keys, klo, khi, 1)).all() and ex.any() and not ex.all()
    res = params["resolution"]
    box_lo = (np.asarray(md.hash_key_to_block(int(EC.make_keys(524288 - 2, 524288 - 2, 524288 - 1))), np.float32) - 0.15).astype(np.float32)
    dims = (16, 16, 8)
    bd = md.box(box_lo, dims)
    assert (bd["cls"] == 3).any() and (bd["cls"] != 3).any(), "the box straddles the cut (3 = MISSING)"
    for other, name in ((fresh, "a fresh device map"), (host, "a host-mode map")):
        R.assert_same(bd, other.box(box_lo, dims), R.BOX_FIELDS, (cls, "box", name))
        _dicts_equal(md.frontier(box_lo, dims), other.frontier(box_lo, dims), (cls, "frontier", name))
    rng = np.random.default_rng(2)
    span = np.asarray(dims) * res
    starts = (box_lo + rng.uniform(0, 1, (256, 3)) * span).astype(np.float32)
    ends = (box_lo + rng.uniform(0, 1, (256, 3)) * span).astype(np.float32)
    _dicts_equal(md.raycast_many(starts, ends, stop=("occupied", "missing")), fresh.raycast_many(starts, ends, stop=("occupied", "missing")),
                 (cls, "raycast_many"))
    assert md.mirror_syncs() == syncs, "no mirror refresh"
    assert md.block_count() == stats["n_blocks"] and md.mirror_syncs() == syncs + 1


@pytest.mark.parametrize("cls", ["BGKOctoMap", "GPOctoMap"])
def test_life_goes_on_after_an_erase(built, cls):
    """erase_region, then insert_pointcloud of a small synthetic scan: the same leaves as a fresh map that unpacked the
    yardstick's post-erase stream and got the same scan — once with half the lattice erased, once with everything erased
    (the next insert starts on an empty map)"""
    import la3dm_amd
    depth = 3
    params, h, stream, klo, khi = _near_case(cls, depth, 21, evidence=True)
    xyz, origin = la3dm_amd.synthetic_scan(3000, seed=5)
    insert = (0.1, 0.5, 4.0)
    for region in ((klo, khi), EC.EVERYTHING):
        want_left, stats = EC.erased_stream(stream, *region, 1)
        a = getattr(la3dm_amd, cls)(**params, device=0).unpack(stream)
        b = getattr(la3dm_amd, cls)(**params, device=0)
        if stats["n_blocks"]:
            b.unpack(want_left)
        assert a.erase_region(*_world(a, *region)) == stats
        assert a.block_count() == stats["n_blocks"]
        for m in (a, b):
            m.insert_pointcloud(xyz, origin, *insert)
        pa, pb = a.pack(), b.pack()
        assert P.parse(pa)["n_blocks"] > stats["n_blocks"], "the scan created blocks"
        _same_bytes(P.sorted_by_key(pa), P.sorted_by_key(pb), (cls, region, "packs after the insert, in key order"))


@pytest.mark.parametrize("cls", ["BGKOctoMap", "BGKLOctoMap"])
def test_evict_then_merge_gives_the_map_back(built, cls, tmp_path):
    """evict, then merge of the returned stream: pack in key order == the original in key order, on an input the helper
    asserts to be stable under merge (no default-valued leaf with another state byte, nothing merge's prune would change);
    the same through evict_file / merge_file, outside the box (the rolling window)"""
    import la3dm_amd
    params, h, stream, klo, khi = _near_case(cls, 3, 31, stable=True)
    EC.assert_merge_restores(stream)
    want = P.sorted_by_key(stream)
    m = getattr(la3dm_amd, cls)(**params, device=0).unpack(stream)
    lo, hi = _world(m, klo, khi)
    syncs = m.mirror_syncs()
    out = m.evict(lo, hi)
    assert isinstance(out, bytes)
    _same_bytes(out, EC.sub_stream(stream, klo, khi, 1), "evict's stream")
    _same_bytes(m.pack(), EC.erased_stream(stream, klo, khi, 1)[0], "after evict")
    st = m.merge(out)
    assert st["n_created"] == st["n_blocks"] == 16 and st["cells_fused"] == 0
    _same_bytes(P.sorted_by_key(m.pack()), want, (cls, "evict, merge"))
    path = str(tmp_path / "outside.la3dm")
    es = m.evict_file(path, lo, hi, inside=False)
    assert es["n_removed"] == 16 and es["n_blocks"] == 16 and os.listdir(tmp_path) == ["outside.la3dm"]
    assert m.merge_file(path)["n_created"] == 16
    _same_bytes(P.sorted_by_key(m.pack()), want, (cls, "evict_file, merge_file"))
    assert m.mirror_syncs() == syncs


def test_device_resident_against_host_mode(built):
    """the same region on the same stream: pack_region and pack after erase_region equal once in key order"""
    import la3dm_amd
    for cls in ("BGKOctoMap", "GPOctoMap"):
        params, h, stream, klo, khi = _near_case(cls, 4, 41)
        md = getattr(la3dm_amd, cls)(**params, device=0).unpack(stream)
        mh = getattr(la3dm_amd, cls)(**params, device=0).set_device_resident(False).unpack(stream)
        lo, hi = _world(md, klo, khi)
        for inside in (True, False):
            _same_bytes(P.sorted_by_key(md.pack_region(lo, hi, inside)), mh.pack_region(lo, hi, inside), (cls, inside, "pack_region"))
        sd, sh = md.erase_region(lo, hi), mh.erase_region(lo, hi)
        assert sd["n_removed"] == sh["n_removed"] == 16 and sd["n_blocks"] == sh["n_blocks"] == 16
        _same_bytes(P.sorted_by_key(md.pack()), mh.pack(), (cls, "after the erase"))


def test_refusals_on_the_device_map(built):
    """klo > khi on each axis, null bounds, inside = 2: LA3DM_ERR_ARG with a text, zero stats, pack() unchanged; a buffer that
    is too small sets *size; nothing selected is a no-op that reports the block count"""
    params = _params("BGKOctoMap", 3)
    lender = _lender("BGKOctoMap", params)
    h = P.header_fields("BGKOctoMap", params)
    stream, klo, khi, inside, flags = _pool_stream(h, "alternating", 5, 9)
    zero = dict.fromkeys(STAT_KEYS, 0)
    with Devmap(lender) as dev:
        assert dev.unpack(stream) == OK
        for axis in range(3):
            bad = list(khi)
            bad[axis] = klo[axis] - 1
            rc, got = dev.erase_region(klo, bad, 1)
            assert rc == -1 and f"klo > khi on axis {axis}" in dev.err() and "la3dm_devmap_erase_region_host" in dev.err() and got == zero, dev.err()
            rc, _ = dev.pack_region(klo, bad, 1)
            assert rc == -1 and f"klo > khi on axis {axis}" in dev.err() and "la3dm_devmap_pack_region_host" in dev.err(), dev.err()
            _same_bytes(dev.pack(), stream, ("klo > khi", axis))
        rc, got = dev.erase_region(klo, khi, 2)
        assert rc == -1 and "inside" in dev.err() and got == zero
        size = C.c_uint64(0)
        assert dev.H.la3dm_devmap_pack_region_host(dev.dm, None, _i3(khi), 1, None, 0, C.byref(size)) == -1
        assert dev.H.la3dm_devmap_erase_region_host(dev.dm, _i3(klo), None, 1, None) == -1
        want = EC.sub_stream(stream, klo, khi, 1)
        buf = np.zeros(want.size, np.uint8)
        assert dev.H.la3dm_devmap_pack_region_host(dev.dm, _i3(klo), _i3(khi), 1, buf.ctypes.data, want.size - 1, C.byref(size)) == -1
        assert size.value == want.size and "smaller than the stream" in dev.err() and not buf.any()
        _same_bytes(dev.pack(), stream, "after the refusals")
        rc, got = dev.erase_region((1, 1, 1), (2, 2, 2), 1)
        assert rc == OK and got == dict(n_removed=0, n_moved=0, n_blocks=5)
        rc, sub = dev.pack_region((1, 1, 1), (2, 2, 2), 1)
        assert rc == OK and sub.size == 128 and P.parse(sub)["n_blocks"] == 0
        _same_bytes(dev.pack(), stream, "nothing selected")
        rc, _ = dev.erase_region(klo, khi, inside, want_stats=False)
        assert rc == OK and dev.counts()[0] == 5 - int(flags.sum())
    with Devmap(lender) as dev:     # an empty map: nothing to select
        rc, got = dev.erase_region(klo, khi, 1)
        assert rc == OK and got == zero
        rc, sub = dev.pack_region(klo, khi, 0)
        assert rc == OK and sub.size == 128


def test_a_poisoned_map_refuses(built, monkeypatch):
    """a map poisoned by the look-back error hook (LA3DM_INJECT_SCAN_STUCK, read when the map is created: the second counter
    read-back of its first insert reports a stuck prefix sum) refuses pack_region and erase_region before anything is
    launched; its block count stays"""
    import la3dm_amd
    params = _params("BGKOctoMap", 3)
    lender = _lender("BGKOctoMap", params)
    monkeypatch.setenv("LA3DM_INJECT_SCAN_STUCK", "2")
    with Devmap(lender) as dev:
        monkeypatch.delenv("LA3DM_INJECT_SCAN_STUCK")
        xyz, origin = la3dm_amd.synthetic_scan(2000, seed=5)
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert dev.H.la3dm_devmap_insert_pointcloud_host(dev.dm, xyz.ctypes.data, xyz.shape[0], 3, o3, 0.1, 0.5, 4.0, None) != OK
        assert "prefix-sum launch found its state in use" in dev.err()
        before = dev.counts()
        rc, got = dev.erase_region(*EC.EVERYTHING, 1)
        assert rc == -1 and "poisoned" in dev.err() and "la3dm_devmap_erase_region_host" in dev.err(), dev.err()
        assert got == dict.fromkeys(STAT_KEYS, 0) and dev.counts() == before
        rc, _ = dev.pack_region(*EC.EVERYTHING, 1)
        assert rc == -1 and "poisoned" in dev.err() and "la3dm_devmap_pack_region_host" in dev.err(), dev.err()


def test_example_program(built, tmp_path):
    """examples/rolling_map on six scans: everything outside a box round the sensor is evicted to a file after every scan, the
    files are merged back at the end; the blocks held stay below the whole map's, blocks are evicted, and the result has the
    blocks and the frontier of a map that never evicted"""
    exe = os.path.join(ROOT, "examples", "rolling_map")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "6", str(tmp_path)] +
                       "4.0 0.1 3 1.0 0.2 0.5 0.1 8.0 0.3 0.7 100.0 0.001 0.001 0".split(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 7 and all(l.startswith(f"scan {i + 1}: ") for i, l in enumerate(lines[:6])), r.stdout
    assert sum(", 0 evicted" not in l for l in lines[:6]) >= 3, r.stdout
    last = lines[-1]
    assert last.startswith("rolling_map: held at most ") and " equal 1; device_resident 1" in last and "frontier 0 vs" not in last, r.stdout
    held, whole = [int(x) for x in last.split("held at most ")[1].split(" blocks;")[0].split(" of ")]
    assert 0 < held < whole, r.stdout
    assert sorted(os.listdir(tmp_path)) == sorted(f"evicted_{i}.la3dm" for i in range(1, 7))
