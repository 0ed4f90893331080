"""diff on the device-resident map (csrc/devmap_diff.h): the finest cells whose class, or whose values, differ between the
live pool and a validated map stream, compared on the GPU.  The yardstick is tests/helpers/diff_cases.py (diff_ref: numpy,
written from the contract comment of la3dm_devmap_diff_host in include/la3dm_hip.h), where NOW is the map's own pack() parsed
by pack_cases; every comparison is exact, floats by their bits.  Every case is also run on a host-mode map that holds the
same blocks: the lists agree after a sort by (block_key, cell) — the two maps keep their blocks in different orders — and
the counts agree exactly.  Around every group of calls: pack() before == pack() after, and no mirror refresh.  No test here
feeds a kernel an invalid stream: the validator is host code that runs before any launch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, pcd_path

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import pack_cases as P  # noqa: E402
import diff_cases as D  # noqa: E402

pytestmark = pytest.mark.gpu

INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured
ALL_PAIRS = (1 << 25) - 1
# pair_mask, value_mask, map_only: the default; values of every class without the map's other blocks; a single pair; value
# changes alone, of one class; everything
COMBOS = ((D.PAIRS_CHANGED, 0, True), (D.PAIRS_CHANGED, 0x1F, False), (D.pair_bit(0, 1), 0, True), (0, 1 << 2, True), (ALL_PAIRS, 0x1F, True))


def _yaml(cls):
    import la3dm_amd
    return dict(BGKOctoMap=la3dm_amd.BGK_YAML, GPOctoMap=la3dm_amd.GP_YAML, BGKLVOctoMap=la3dm_amd.LV_YAML, BGKLOctoMap=la3dm_amd.L_YAML)[cls]


def _maps(cls, params, now):
    """the device-resident map and a host-mode map with the blocks of the stream `now`"""
    import la3dm_amd
    md = getattr(la3dm_amd, cls)(**params, device=0).unpack(now)
    mh = getattr(la3dm_amd, cls)(**params, device=0).set_device_resident(False).unpack(now)
    assert md.is_device_resident() and not mh.is_device_resident()
    return md, mh


def _same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    assert a.size == b.size, (what, a.size, b.size)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, (what, bad.size, bad[:8].tolist())


def _sorted(r):
    order = np.lexsort((r["cell"], r["block_key"]))
    return {f: np.ascontiguousarray(r[f][order]) for f in D.LIST_FIELDS}


def _check(md, mh, then, combos, what):
    """md.diff(then) against the yardstick and against the host-mode map, for every combination; the map untouched"""
    before, syncs = md.pack(), md.mirror_syncs()
    lut, centre_of = md.lut(), md.hash_key_to_block
    last = None
    for pm, vm, mo in combos:
        want = D.diff_ref(before, then, pm, vm, mo, lut, centre_of)
        got = md.diff(then, pairs=pm, values=vm, map_only=mo, fields=D.LIST_FIELDS)
        D.assert_same(got, want, (what, pm, vm, mo))
        host = mh.diff(then, pairs=pm, values=vm, map_only=mo, fields=D.LIST_FIELDS)
        assert host["n"] == got["n"] and all(host[k] == got[k] for k in D.STAT_KEYS), (what, pm, vm, mo)
        assert (host["pairs"] == got["pairs"]).all() and (host["value_changed"] == got["value_changed"]).all(), (what, pm, vm, mo)
        for f, x in _sorted(host).items():
            _same_bytes(x, _sorted(got)[f], (what, pm, vm, mo, "host-mode map", f))
        last = got
    _same_bytes(md.pack(), before, (what, "pack() after the diffs"))
    assert md.mirror_syncs() == syncs, (what, "no mirror refresh")
    return last


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_hand_built_cases(built, depth):
    """block_depth 1 (one cell), 2 (8 cells, under a wave), 3 (64 cells, one chunk), 4 (512 cells: 8 chunks, 19 mask words, the
    running base across chunks) and 5 (the deepest that runs); 1 compared block, 4 (one full workgroup), 5 (a tail workgroup
    with idle waves) and more with map_only on and off; a single root leaf against all finest cells both ways, leaves at mixed
    layers, a stream block absent from the map, a map block absent from the stream, identical blocks, the empty stream, the
    empty map; the masks of COMBOS"""
    cls = "BGKOctoMap"
    params = dict(_yaml(cls), block_depth=depth)
    h = P.header_fields(cls, params)
    cases = D.cases(h, unions=(3, 4, 5, 6) if depth < 5 else (3,))
    cond = D.conditions(cases)
    print(f"{cls} depth {depth}: {len(cases)} cases, pairs {cond['pairs'].astype(int).tolist()}, value_changed {cond['value_changed'].astype(int).tolist()}")
    if depth >= 2:   # (block_depth 1 has one cell per block: too few cells for every pair)
        assert cond["pairs"][:3, :3].all() and cond["pairs"][3, :3].all() and cond["pairs"][:3, 3].all()
    assert np.trace(cond["pairs"]) and cond["pairs"].sum() > np.trace(cond["pairs"]) and cond["value_changed"][:3].any()
    assert cond["n_missing_now"] and cond["n_map_only_blocks"]
    for name, now, then in cases:
        md, mh = _maps(cls, params, now)
        got = _check(md, mh, then, COMBOS, (cls, depth, name))
        if name == "identical blocks":
            assert md.diff(then)["n"] == 0 and got["pairs"].sum() == np.trace(got["pairs"]) > 0 and got["value_changed"].sum() == 0


@pytest.mark.parametrize("cls", ["GPOctoMap", "BGKLVOctoMap", "BGKLOctoMap"])
def test_every_map_class(built, cls):
    """the other three classes at block_depth 3; the BGK-LV cases carry UNCERTAIN leaves (class 4) on both sides"""
    params = dict(_yaml(cls), block_depth=3)
    h = P.header_fields(cls, params)
    cases = D.cases(h)
    cond = D.conditions(cases)
    if cls == "BGKLVOctoMap":
        assert cond["pairs"][4].all() and cond["pairs"][:, 4].all() and cond["value_changed"][4]
    else:
        assert not cond["pairs"][4].any() and not cond["pairs"][:, 4].any()
    for name, now, then in cases:
        md, mh = _maps(cls, params, now)
        got = _check(md, mh, then, COMBOS[:2] + COMBOS[-1:], (cls, name))
        if cls == "BGKLVOctoMap" and name.startswith("leaves at mixed"):
            assert ((got["code"] & 15) == 4).any() and ((got["code"] >> 4) == 4).any()


@pytest.mark.parametrize("n", [257, 258])
def test_one_past_the_find_group(built, n):
    """257 compared blocks, and 257 stream blocks of 258 compared: one past dm_merge_find's 256-lane group, many workgroups
    of the count and the emit launch, the offsets of 258 counts"""
    cls = "BGKOctoMap"
    params = dict(_yaml(cls), block_depth=3)
    h = P.header_fields(cls, params)
    name, now, then = D.union_case(h, np.random.default_rng(n), n)
    assert P.parse(then)["n_blocks"] == n - 1 and P.parse(now)["n_blocks"] == n - 1
    md, mh = _maps(cls, params, now)
    got = _check(md, mh, then, COMBOS[:2] + COMBOS[-1:], (cls, name))
    assert got["n_stream_blocks"] + got["n_map_only_blocks"] == n and got["n_missing_now"] == 1


def _raw(m, then, pm, vm, mo, cap, room, with_out=True):
    """la3dm_map_diff itself on buffers of `room` entries filled with a guard pattern: (rc, n_found, buffers, stats)"""
    from la3dm_amd import _lib
    M = _lib.maplib()
    buf = {f: np.frombuffer(bytes([0xA5]) * (room * w * np.dtype(t).itemsize), np.uint8).copy() for f, (t, w) in m._DIFF_FIELDS.items()}
    o = _lib.DiffOut(*[buf[f].ctypes.data for f, _ in _lib.DiffOut._fields_])
    params = _lib.DiffParams(pm, vm, 1 if mo else 0)
    found, stats = C.c_uint64(0xA5A5), _lib.DiffStats()
    C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
    s = np.ascontiguousarray(then, np.uint8)
    rc = M.la3dm_map_diff(m._h, s.ctypes.data, s.size, C.byref(params), cap, C.byref(o) if with_out else None, C.byref(found), C.byref(stats))
    return rc, int(found.value), buf, stats


def test_cap_and_count_only(built):
    """cap = 0 (with out NULL and with buffers), 1 and n - 1: *n_found and the stats are those of the full call, the first
    min(n, cap) entries are the full list's, and not a byte past them is written (a guard pattern fills the buffers)"""
    cls = "BGKOctoMap"
    params = dict(_yaml(cls), block_depth=4)
    h = P.header_fields(cls, params)
    name, now, then = D.union_case(h, np.random.default_rng(77), 6)
    md, _ = _maps(cls, params, now)
    pm, vm, mo = D.PAIRS_CHANGED, 0x1F, True
    want = D.diff_ref(md.pack(), then, pm, vm, mo, md.lut(), md.hash_key_to_block)
    n = want["n"]
    assert n > 600, "more than one block's cells, so caps fall inside a block and between blocks"
    D.assert_same(md.diff(then, values=vm, fields=D.LIST_FIELDS), want, "cap=None counts first, then fills")
    rc, found, _, stats = _raw(md, then, pm, vm, mo, 0, 4, with_out=False)
    assert rc == 0 and found == n and np.array(stats.pairs, np.uint64).reshape(5, 5).tolist() == want["pairs"].tolist()
    for cap in (0, 1, n // 2, n - 1, n, n + 3):
        room = n + 8
        rc, found, buf, stats = _raw(md, then, pm, vm, mo, cap, room)
        assert rc == 0 and found == n, (cap, rc, found)
        assert np.array(stats.pairs, np.uint64).reshape(5, 5).tolist() == want["pairs"].tolist(), cap
        m = min(cap, n)
        for f, (t, w) in md._DIFF_FIELDS.items():
            size = w * np.dtype(t).itemsize
            _same_bytes(buf[f][:m * size], np.ascontiguousarray(want[f][:m]), (cap, f))
            assert (buf[f][m * size:] == 0xA5).all(), (cap, f, "written past min(n, cap)")
        D.assert_same(md.diff(then, values=vm, fields=D.LIST_FIELDS, cap=cap), want, ("cap", cap), cap=cap)


def test_real_scans_centres_and_values(built):
    """a publisher's round on real pools: scan 1, pack, scan 2, diff — against the yardstick and a host-mode map that holds
    the same blocks; centre is bit-equal to dump_leaves' location for the listed cells that are finest leaves, A and B are
    bit-equal to search_many at those centres; the map against its own fresh pack lists nothing"""
    import la3dm_amd
    cls, depth = "BGKOctoMap", 3
    params = dict(_yaml(cls), block_depth=depth)
    md = getattr(la3dm_amd, cls)(**params, device=0)
    clouds = [la3dm_amd.load_pcd(pcd_path("sim_structured", i)) for i in (1, 2)]
    md.insert_pointcloud(*clouds[0], *INSERT)
    then = md.pack()
    md.insert_pointcloud(*clouds[1], *INSERT)
    now = md.pack()
    mh = getattr(la3dm_amd, cls)(**params, device=0).set_device_resident(False).unpack(now)
    got = _check(md, mh, then, (COMBOS[0], COMBOS[-1]), "two scans")
    print(f"two scans: {got['n_stream_blocks']} + {got['n_map_only_blocks']} blocks, {got['n']} cells, pairs {got['pairs'].astype(int).tolist()}")
    assert got["n_map_only_blocks"] > 0 and got["n_missing_now"] == 0 and got["pairs"][3, :3].all() and got["pairs"][2, :2].all()
    assert P.parse(now)["mask"][:, :P.base(depth - 1)].any(), "coarse leaves exist"
    fresh = md.diff(now, values=0x1F)
    assert fresh["n"] == 0 and fresh["pairs"].sum() == np.trace(fresh["pairs"]) == P.parse(now)["n_blocks"] * 8 ** (depth - 1)
    assert md.mirror_syncs() == 0
    # `got` lists every cell (ALL_PAIRS); leaves() refreshes the mirror, hence last
    lv = md.leaves()
    fine = (lv["node_key"] >> 16) == depth - 1
    where = {(int(k), int(c)): i for i, (k, c) in enumerate(zip(got["block_key"], got["cell"]))}
    rows = np.array([where[(int(k), int(nk) & 0xFFFF)] for k, nk in zip(lv["block_key"][fine], lv["node_key"][fine])], np.int64)
    assert rows.size > 1000
    _same_bytes(got["centre"][rows], lv["loc"][fine], "centre == dump_leaves' location")
    _same_bytes(got["A"][rows], lv["A"][fine], "A == the leaf's")
    s = md.search_many(got["centre"][rows])
    assert s["exists"].all()
    _same_bytes(got["A"][rows], s["A"], "A == search_many at the centre")
    _same_bytes(got["B"][rows], s["B"], "B == search_many at the centre")


def test_refusals_on_the_device_map(built):
    """a stream the validator rejects, a mismatch with the map, mask bits out of range, a NULL n_found, cap > 0 with out NULL:
    each returns -1 with a text, writes neither *n_found nor the stats nor a buffer, and leaves pack() as it was; the valid
    call works afterwards.  (The LDS refusal cannot be reached: it is for block_depth 6, and a device-resident map stops at
    5, which test_hand_built_cases runs.)"""
    import la3dm_amd
    from la3dm_amd import _lib
    cls = "BGKOctoMap"
    params = dict(_yaml(cls), block_depth=3)
    h = P.header_fields(cls, params)
    rows = P.corrupt_table(h)
    name, now, then = D.union_case(h, np.random.default_rng(5), 5)
    md, _ = _maps(cls, params, now)
    before = md.pack()
    err = lambda: _lib.maplib().la3dm_map_last_error().decode()   # noqa: E731

    def untouched(rc, found, buf, stats, what):
        assert rc == -1 and found == 0xA5A5, (what, rc, found)
        assert all((b == 0xA5).all() for b in buf.values()) and set(bytes(stats)) == {0xA5}, what
        _same_bytes(md.pack(), before, what)

    for name, stream, frag in rows[:-1]:
        untouched(*_raw(md, stream, D.PAIRS_CHANGED, 0, True, 4, 4), name)
        assert frag in err() and "diff" in err(), (name, err())
    untouched(*_raw(md, then, 1 << 25, 0, True, 4, 4), "pair_mask bit 25")
    assert "pair_mask" in err()
    untouched(*_raw(md, then, D.PAIRS_CHANGED, 1 << 5, True, 4, 4), "value_mask bit 5")
    assert "value_mask" in err()
    untouched(*_raw(md, then, D.PAIRS_CHANGED, 0, True, 4, 4, with_out=False), "cap > 0 with out NULL")
    assert "out is NULL" in err()
    params_c = _lib.DiffParams(D.PAIRS_CHANGED, 0, 1)
    assert _lib.maplib().la3dm_map_diff(md._h, then.ctypes.data, then.size, C.byref(params_c), 0, None, None, None) == -1
    assert "n_found" in err()
    _same_bytes(md.pack(), before, "n_found NULL")
    with pytest.raises(RuntimeError, match="pair_mask"):
        md.diff(then, pairs=1 << 25)
    with pytest.raises(TypeError):
        md.diff(la3dm_amd.BGKLOctoMap(**dict(_yaml("BGKLOctoMap"), block_depth=3), device=0))
    assert md.diff(then)["n"] == D.diff_ref(before, then)["n"] > 0


def test_map_argument_file_and_example(built, tmp_path):
    """a map object and a file as the argument; examples/changes on four scans: cells became occupied, the map against its
    own pack differs nowhere, no mirror refresh"""
    cls = "BGKOctoMap"
    params = dict(_yaml(cls), block_depth=3)
    h = P.header_fields(cls, params)
    name, now, then = D.union_case(h, np.random.default_rng(8), 5)
    md, mh = _maps(cls, params, now)
    other, _ = _maps(cls, params, then)
    want = D.diff_ref(md.pack(), other.pack(), D.PAIRS_CHANGED, 0, True)
    D.assert_same(md.diff(other), want, "diff(map)")
    path = str(tmp_path / "then.la3dm")
    other.save(path)
    D.assert_same(md.diff_file(path), want, "diff_file")
    exe = os.path.join(ROOT, "examples", "changes")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "4"] +
                       "0.1 3 1.0 0.2 0.5 0.1 8.0 0.3 0.7 100.0 0.001 0.001 0".split(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    line = r.stdout.strip().splitlines()[0]
    assert line.startswith("changes: ") and "INCONSISTENT" not in line and line.endswith("self diff 0; mirror_syncs 0 device_resident 1"), r.stdout
    assert "newly occupied 0 " not in line and "newly observed 0 " not in line and "  newly occupied at " in r.stdout, r.stdout
