"""merge on the device-resident map (csrc/devmap_merge.h): a validated map stream fused into the live pool on the GPU.  The
yardstick is tests/helpers/merge_cases.py (merge_ref: numpy float32, written from the contract comment of
la3dm_devmap_merge_host in include/la3dm_hip.h); every comparison is exact, floats by their bits.  The raw-ABI harness is
that of tests/test_pack_gpu.py: unpack(dst), merge(src), download, the blocks the stream named canonicalised and compared
with the yardstick, the others compared byte for byte with the download from before the call.  No test here feeds a kernel
an invalid stream: the validator is host code that runs before any launch."""
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
import merge_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu

OK = 0
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured
LEAF_FIELDS = ("block_key", "node_key", "loc", "size", "A", "B", "state", "classified")
STAT_KEYS = ("n_blocks", "n_created", "cells_kept", "cells_copied", "cells_fused")
_LENDERS = {}


def _same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    assert a.size == b.size, (what, a.size, b.size)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, (what, bad.size, bad[:8].tolist())


def _params(cls, depth):
    import la3dm_amd
    return dict(la3dm_amd.BGK_YAML if cls == "BGKOctoMap" else la3dm_amd.L_YAML, block_depth=depth)   # (BGK-L: var_thresh 0.15)


def _thresholds(params):
    return params["free_thresh"], params["occupied_thresh"], params["var_thresh"]


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
        self._lib = _lib
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
        if nb:
            assert self.H.la3dm_devmap_download(self.dm, keys.ctypes.data, A.ctypes.data, B.ctypes.data, S.ctypes.data) == OK, self.err()
        return keys, A, B, S

    def pack(self):
        size = C.c_uint64(0)
        assert self.H.la3dm_devmap_pack_host(self.dm, None, 0, C.byref(size)) == OK, self.err()
        buf = np.zeros(int(size.value), np.uint8)
        assert self.H.la3dm_devmap_pack_host(self.dm, buf.ctypes.data, buf.size, C.byref(size)) == OK, self.err()
        return buf

    def unpack(self, stream):
        s = np.ascontiguousarray(stream, np.uint8)
        return self.H.la3dm_devmap_unpack_host(self.dm, s.ctypes.data, s.size)

    def merge(self, stream, want_stats=True):
        """(return code, stats dict)"""
        s = np.ascontiguousarray(stream, np.uint8)
        st = self._lib.MergeStats()
        rc = self.H.la3dm_devmap_merge_host(self.dm, s.ctypes.data if s.size else None, s.size, C.byref(st) if want_stats else None)
        return rc, {k: int(getattr(st, k)) for k in STAT_KEYS}


def _merge_and_check(lender, h, th, dst, src, what):
    """the harness: returns the device map's pack() after the merge"""
    d = {}
    want, stats = MC.merge_ref(dst, src, th, d)
    wk, wA, wB, wS = P.canonical_pool(want)
    nd = P.parse(dst)["n_blocks"]
    with Devmap(lender) as dev:
        if nd:
            assert dev.unpack(dst) == OK, (what, dev.err())
        bk, bA, bB, bS = dev.download()
        rc, got = dev.merge(src)
        assert rc == OK, (what, dev.err())
        assert got == stats, (what, got, stats)
        gk, gA, gB, gS = dev.download()
        assert gk.size == wk.size and (gk == wk).all(), (what, "the old blocks keep their slots, new blocks follow in stream order")
        named = np.zeros(gk.size, bool)
        named[d["rows"]] = True
        ck, cA, cB, cS = P.canonicalise(h, gk[named], gA[named], gB[named], gS[named])
        _same_bytes(cS, wS[named], (what, "S"))
        _same_bytes(cA, wA[named], (what, "A"))
        _same_bytes(cB, wB[named], (what, "B"))
        _same_bytes(gS[named], cS, (what, "the merge writes the canonical form itself"))
        old = ~named[:nd]
        for x, y, n in ((gS, bS, "S"), (gA, bA, "A"), (gB, bB, "B")):
            _same_bytes(x[:nd][old], y[old], (what, "blocks the stream does not name", n))
        packed = dev.pack()
        _same_bytes(packed, want, (what, "pack"))
        _same_bytes(dev.pack(), packed, (what, "two packs"))
        return packed


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("cls", ["BGKOctoMap", "BGKLOctoMap"])
def test_hand_built_pairs_through_the_raw_abi(built, cls, depth):
    """GPU tests 1, 2, 3: block_depth 1 (one node), 2 (under one wave), 3 (one pass of 64 cells), 4 (eight passes, 19 mask words);
    1, 3, 4, 5 and 9 stream blocks against an empty, disjoint, equal and half-overlapping destination, the stream's blocks in
    no order; every tiling pair (un-pruned, collapsed to the root on either side, one mid-layer group collapsed on either
    side, fuses that collapse a group and a whole chain, a fuse that splits a coarse leaf); kept, copied and fused cells with
    the stats of the yardstick.  BGKLOctoMap runs the small var_thresh."""
    params = _params(cls, depth)
    lender = _lender(cls, params)
    h, th = P.header_fields(cls, params), _thresholds(params)
    pairs = MC.cases(h)
    cond = MC.conditions(h, th, pairs)
    print(f"{cls} depth {depth}: {len(pairs)} pairs, {cond}")
    assert cond["kept"] and cond["copied"] and cond["fused"] and cond["created"]
    assert cond["p_below_free"] and cond["p_between"] and cond["p_above_occ"]
    if cls == "BGKLOctoMap":
        assert cond["var_above"] and cond["var_below"]
    if depth >= 2:
        assert cond["collapsed"] and cond["split"]
    for name, dst, src in pairs:
        _merge_and_check(lender, h, th, dst, src, (cls, depth, name))


def test_order_of_the_stream_and_the_empty_stream(built):
    """the stream's blocks reversed: the same map apart from the slots of the created blocks (equal once in key order); the
    empty stream is a no-op with zero stats, with and without a stats pointer"""
    cls, depth = "BGKOctoMap", 3
    params = _params(cls, depth)
    lender = _lender(cls, params)
    h, th = P.header_fields(cls, params), _thresholds(params)
    name, dst, src = [c for c in MC.cases(h) if c[0] == "5 stream blocks, destination half overlapping"][0]
    reverse = P.stream_from_pool(h, *[np.ascontiguousarray(x[::-1]) for x in P.canonical_pool(src)])
    a = _merge_and_check(lender, h, th, dst, src, "as given")
    b = _merge_and_check(lender, h, th, dst, reverse, "reversed")
    assert (P.parse(a)["keys"] != P.parse(b)["keys"]).any(), "the created blocks' slots follow the stream"
    _same_bytes(P.sorted_by_key(a), P.sorted_by_key(b), "order independence")
    with Devmap(lender) as dev:
        assert dev.unpack(dst) == OK
        before = dev.pack()
        for want_stats in (True, False):
            rc, got = dev.merge(MC.empty_stream(h), want_stats)
            assert rc == OK and got == dict.fromkeys(STAT_KEYS, 0)
        _same_bytes(dev.pack(), before, "after the empty stream")
        rc, _ = dev.merge(src, False)
        assert rc == OK
        _same_bytes(dev.pack(), a, "stats = NULL")


def _lattice_keys(rng, n, side=64):
    cell = rng.permutation(side ** 3)[:n]
    f = [524288 - side // 2 + ((cell // side ** k) % side).astype(np.int64) for k in (2, 1, 0)]
    return (f[0] << 40) | (f[1] << 20) | f[2]


def test_growth_with_live_contents(built):
    """GPU test 5, block_depth 2: a map of 100 blocks (pool capacity 4096); a merge of 4100 blocks, 50 of them the map's, takes
    the pool across that capacity; one of 33000 blocks, 500 of them the map's, takes the block table across its bound of
    32768 blocks (and the pool across its second capacity).  Each against the yardstick: old blocks in their slots — those
    not named byte-identical —, new slots in stream order; then one search per block finds every block through the table"""
    cls, depth = "BGKOctoMap", 2
    params = _params(cls, depth)
    lender = _lender(cls, params)
    h, th = P.header_fields(cls, params), _thresholds(params)
    rng = np.random.default_rng(55)
    keys = _lattice_keys(rng, 100 + 4050 + 32500)
    mk = lambda k: P.stream_from_pool(h, *MC.pool(rng, h, k, rng.random((k.size, 9)) < 0.1))   # noqa: E731
    dst = mk(keys[:100])
    first = mk(rng.permutation(np.concatenate([keys[:50], keys[100:4150]])))
    second = mk(rng.permutation(np.concatenate([keys[3000:3500], keys[4150:]])))
    assert P.parse(first)["n_blocks"] == 4100 and P.parse(second)["n_blocks"] == 33000
    after_first = _merge_and_check(lender, h, th, dst, first, "across the pool's first capacity")
    assert P.parse(after_first)["n_blocks"] == 4150
    after_second = _merge_and_check(lender, h, th, after_first, second, "across the table's bound")
    p = P.parse(after_second)
    assert p["n_blocks"] == 36650 > 32768
    # the same two merges in one map (the second grows a pool and a table with live, merged contents)
    with Devmap(lender) as dev:
        assert dev.unpack(dst) == OK
        for s in (first, second):
            rc, _ = dev.merge(s)
            assert rc == OK, dev.err()
        _same_bytes(dev.pack(), after_second, "both merges in one map")
        centres = np.stack([lender.hash_key_to_block(int(k)) for k in p["keys"][::37]])
        q = np.concatenate([centres + lender.lut()[1], [[900.0, 900.0, 900.0]]]).astype(np.float32)
        ex = np.zeros(q.shape[0], np.uint8)
        out = [np.zeros(q.shape[0], t) for t in (np.float32, np.float32, np.uint8)]
        assert dev.H.la3dm_devmap_search_host(dev.dm, q.ctypes.data, q.shape[0], ex.ctypes.data, *[o.ctypes.data for o in out]) == OK
        assert ex[:-1].all() and ex[-1] == 0, "every block is found through the grown table"


@pytest.mark.parametrize("variant", ["BGKOctoMap d3", "BGKOctoMap d4", "BGKLOctoMap"])
def test_real_pools(built, variant):
    """GPU tests 4, 6, 7.  Two device maps fed different sim_structured scans (1, 2 and 3, 4): one packed and merged into the
    other against merge_ref of their two packs, through the raw ABI (the harness) and through the class, whose pack equals
    the yardstick's stream in key order; search_many and box over the merged region agree with a host-mode map that merged
    the same streams; a further scan into both gives the same leaves bit for bit.  Merging the two-scan map's pack into an
    empty map equals unpack of it, canonical pool for canonical pool."""
    import la3dm_amd
    cls, yaml, depth, insert = {"BGKOctoMap d3": ("BGKOctoMap", "BGK_YAML", 3, INSERT), "BGKOctoMap d4": ("BGKOctoMap", "BGK_YAML", 4, INSERT),
                                "BGKLOctoMap": ("BGKLOctoMap", "L_YAML", 3, (0.1, 0.3, 8.0))}[variant]
    params = dict(getattr(la3dm_amd, yaml), block_depth=depth)
    h, th = P.header_fields(cls, params), _thresholds(params)
    lender = _lender(cls, params)
    with Devmap(lender) as a, Devmap(lender) as b:
        for i in (1, 2):
            a.insert(i, insert)
        for i in (3, 4):
            b.insert(i, insert)
        sa, sb = a.pack(), b.pack()
    d = {}
    want, stats = MC.merge_ref(sa, sb, th, d)
    print(f"{variant}: {P.parse(sa)['n_blocks']} + {P.parse(sb)['n_blocks']} blocks, {stats}; fused var > var_thresh: "
          f"{int((d['var'] > np.float32(th[2])).sum())}")
    assert 0 < stats["n_created"] < stats["n_blocks"] and stats["cells_kept"] and stats["cells_copied"] and stats["cells_fused"]
    assert P.parse(sa)["mask"][:, :P.base(depth - 1)].any(), "coarse leaves exist"
    _merge_and_check(lender, h, th, sa, sb, (variant, "real pools"))
    # into an empty map: the real map's pack is prune-stable, so merge == unpack
    with Devmap(lender) as e, Devmap(lender) as u:
        rc, got = e.merge(sa)
        assert rc == OK and got["n_created"] == got["n_blocks"] == P.parse(sa)["n_blocks"] and got["cells_fused"] == 0, (e.err(), got)
        assert u.unpack(sa) == OK
        for x, y, n in zip(P.canonicalise(h, *e.download()), P.canonicalise(h, *u.download()), "kABS"):
            _same_bytes(x, y, (variant, "merge into an empty map == unpack", n))
        _same_bytes(e.pack(), sa, (variant, "and packs to the stream"))
    # the class, device-resident and host-mode
    md = getattr(la3dm_amd, cls)(**params, device=0).unpack(sa)
    mh = getattr(la3dm_amd, cls)(**params, device=0).set_device_resident(False).unpack(sa)
    assert md.is_device_resident() and not mh.is_device_resident()
    syncs = md.mirror_syncs()
    assert md.merge(sb) == stats and mh.merge(sb) == stats
    _same_bytes(P.sorted_by_key(md.pack()), P.sorted_by_key(want), (variant, "class pack vs yardstick"))
    _same_bytes(mh.pack(), P.sorted_by_key(want), (variant, "host-mode pack vs yardstick"))
    lo = R.recipe_lo()
    R.assert_same(md.box(lo, R.RECIPE_DIMS), mh.box(lo, R.RECIPE_DIMS), R.BOX_FIELDS, (variant, "box"))
    rng = np.random.default_rng(9)
    q = (lo + rng.uniform(0, 1, (4000, 3)) * (np.asarray(R.RECIPE_DIMS) * params["resolution"])).astype(np.float32)
    sd_, sh_ = md.search_many(q), mh.search_many(q)
    assert sd_["exists"].any() and (sd_["exists"] == sh_["exists"]).all() and (sd_["state"] == sh_["state"]).all()
    # (search at a collapsed voxel reads a dead node: PRUNED with the default values on both, the merge having written them)
    _same_bytes(sd_["A"], sh_["A"], (variant, "search A"))
    _same_bytes(sd_["B"], sh_["B"], (variant, "search B"))
    assert md.mirror_syncs() == syncs, "no mirror refresh for merge, pack, box or search_many"
    # going on: a further scan into both
    lv = md.leaves()
    R.assert_same(mh.leaves(), lv, LEAF_FIELDS, (variant, "leaves after the merge"))
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 5))
    for m in (md, mh):
        m.insert_pointcloud(xyz, origin, *insert)
    after = md.leaves()
    assert after["A"].size != lv["A"].size or (after["A"].view(np.uint32) != lv["A"].view(np.uint32)).any()
    R.assert_same(mh.leaves(), after, LEAF_FIELDS, (variant, "leaves after a further scan"))
    _same_bytes(P.sorted_by_key(md.pack()), mh.pack(), (variant, "streams after a further scan"))
    # a map object as the argument
    other = getattr(la3dm_amd, cls)(**params, device=0).unpack(sb)
    again = getattr(la3dm_amd, cls)(**params, device=0).unpack(sa)
    assert again.merge(other) == stats
    _same_bytes(P.sorted_by_key(again.pack()), P.sorted_by_key(want), (variant, "merge(map)"))


def test_refusals_on_the_device_map(built):
    """GPU test 8: GPOctoMap and BGKLVOctoMap contexts; a stream of another variant, block_depth, resolution or default node; a
    truncated stream and the other rows of the corrupt-stream table; block_depth 5 (the staging does not fit a compute
    unit's LDS).  Each returns LA3DM_ERR_ARG with a text and leaves pack() unchanged; the valid stream merges afterwards."""
    import la3dm_amd
    cls, depth = "BGKOctoMap", 3
    params = _params(cls, depth)
    lender = _lender(cls, params)
    h, th = P.header_fields(cls, params), _thresholds(params)
    rows = P.corrupt_table(h)
    names = [r[0] for r in rows]
    for need in ("truncated", "mismatching block_depth", "mismatching variant", "mismatching resolution", "mismatching prior"):
        assert need in names
    dst = [c for c in MC.cases(h) if c[0] == "4 stream blocks, destination disjoint"][0][1]
    with Devmap(lender) as dev:
        assert dev.unpack(dst) == OK
        before = dev.pack()
        for name, stream, frag in rows[:-1]:
            rc, got = dev.merge(stream)
            assert rc == -1 and frag in dev.err() and "la3dm_devmap_merge_host" in dev.err(), (name, rc, dev.err())
            assert got == dict.fromkeys(STAT_KEYS, 0), name
            _same_bytes(dev.pack(), before, name)
        rc, _ = dev.merge(np.zeros(0, np.uint8))
        assert rc == -1
        _same_bytes(dev.pack(), before, "a null stream")
        name, valid, _ = rows[-1]      # (its odd values are only ever copied: its blocks are not the map's)
        assert not set(P.parse(valid)["keys"].tolist()) & set(P.parse(dst)["keys"].tolist())
        rc, got = dev.merge(valid)
        assert rc == OK and got["n_created"] == 3 and got["cells_fused"] == 0, dev.err()
        _same_bytes(dev.pack(), MC.merge_ref(dst, valid, th)[0], "the valid stream afterwards")
    for other, yaml in (("GPOctoMap", la3dm_amd.GP_YAML), ("BGKLVOctoMap", la3dm_amd.LV_YAML)):
        po = dict(yaml, block_depth=3)
        with Devmap(_lender(other, po)) as dev:
            ho = P.header_of(P.parse(dev.pack()))          # (the empty map's header: the context's own numbers)
            own = P.stream_from_pool(ho, *P.random_pool(np.random.default_rng(3), ho, 3, np.zeros((3, 73), bool)))
            assert dev.unpack(own) == OK, dev.err()
            before = dev.pack()
            rc, _ = dev.merge(own)
            assert rc == -1 and "variant 0" in dev.err() and "BGKLOctoMap" in dev.err(), dev.err()
            _same_bytes(dev.pack(), before, other)
    p5 = _params(cls, 5)
    h5 = P.header_fields(cls, p5)
    s5 = P.stream_from_pool(h5, *MC.pool(np.random.default_rng(4), h5, MC.near_keys(np.random.default_rng(4), 2), np.zeros((2, P.npb_of(5)), bool)))
    with Devmap(_lender(cls, p5)) as dev:
        assert dev.unpack(s5) == OK
        rc, _ = dev.merge(s5)
        assert rc == -1 and "LDS" in dev.err() and "block_depth 5" in dev.err(), dev.err()
        _same_bytes(dev.pack(), s5, "block_depth 5 is refused, the map unchanged")


def test_a_poisoned_map_refuses(built, monkeypatch):
    """a map poisoned by the look-back error hook (LA3DM_INJECT_SCAN_STUCK, read when the map is created: the second counter
    read-back of its first insert reports a stuck prefix sum) refuses a valid stream before anything is launched; its block
    count stays (pack refuses such a map too, so the count is what can be compared)"""
    import la3dm_amd
    cls, depth = "BGKOctoMap", 3
    params = _params(cls, depth)
    lender = _lender(cls, params)
    h = P.header_fields(cls, params)
    src = MC.cases(h)[0][2]
    monkeypatch.setenv("LA3DM_INJECT_SCAN_STUCK", "2")
    with Devmap(lender) as dev:
        monkeypatch.delenv("LA3DM_INJECT_SCAN_STUCK")
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 1))
        xyz = np.ascontiguousarray(xyz, np.float32)
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert dev.H.la3dm_devmap_insert_pointcloud_host(dev.dm, xyz.ctypes.data, xyz.shape[0], 3, o3, *INSERT, None) != OK
        assert "prefix-sum launch found its state in use" in dev.err()
        before = dev.counts()
        rc, got = dev.merge(src)
        assert rc == -1 and "poisoned" in dev.err() and "la3dm_devmap_merge_host" in dev.err(), dev.err()
        assert got == dict.fromkeys(STAT_KEYS, 0) and dev.counts() == before
    with Devmap(lender) as dev:       # the next map of the process merges the stream
        rc, got = dev.merge(src)
        assert rc == OK and got["n_created"] == got["n_blocks"] == P.parse(src)["n_blocks"], dev.err()


def test_example_program(built):
    """examples/merge_maps on four scans: two maps from the odd and the even scans, one merged into the other; the numbers are
    consistent, blocks are created and cells fused, no mirror refresh"""
    exe = os.path.join(ROOT, "examples", "merge_maps")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "4"] +
                       "0.1 3 1.0 0.2 0.5 0.1 8.0 0.3 0.7 100.0 0.001 0.001 0".split(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    line = r.stdout.strip().splitlines()[-1]
    assert line.startswith("merge_maps: ") and "INCONSISTENT" not in line and line.endswith("mirror_syncs 0 device_resident 1"), r.stdout
    assert " fused 0;" not in line and "(0 created)" not in line and "frontier 0 ->" not in line, r.stdout
