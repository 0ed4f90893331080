"""save / load on host-mode maps (device = -1, no GPU): pack() against the stream tests/helpers/pack_cases.py writes from
leaves(), the round trip, the continuation with a further scan, save / load / load_map / pack_info, the empty map and the
table of corrupt streams.  The helper is written from the layout comment in include/la3dm_hip.h; every comparison is exact
(floats by their bits)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, pcd_path

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import pack_cases as P  # noqa: E402

LEAF_FIELDS = ("block_key", "node_key", "loc", "size", "A", "B", "state", "classified")
INSERT = (0.1, 0.5, 8.0)


def _params(depth):
    return dict(R.YAML, block_depth=depth)


def _same_bytes(a, b, what):
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    assert a.size == b.size, (what, a.size, b.size)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, (what, bad.size, bad[:8].tolist())


def _insert_emulated(m, params, scan):
    import la3dm_amd
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", scan))
    assert m.prepare(xyz, origin, *INSERT)
    R._emulate_device(m.packed(), params)
    m.commit()


def _fresh(depth, cls="BGKOctoMap", params=None):
    import la3dm_amd
    return getattr(la3dm_amd, cls)(**(params or _params(depth)), device=-1)


@pytest.mark.parametrize("depth", [3, 4])
def test_pack_is_the_helpers_stream_and_round_trips(built, depth, tmp_path):
    """CPU tests 1, 2, 4, 5: pack() of the fused two-scan map == the helper's stream from leaves() + the block list (ascending
    key), with the input conditions first; unpack into a fresh map gives equal leaves() and an equal pack(); save writes
    those bytes (no .tmp left), load and load_map build equal maps; pack_info returns the header; the size bound holds"""
    import la3dm_amd
    m, lv, _ = R.fused_map(depth)
    h = P.header_fields("BGKOctoMap", _params(depth))
    blocks = np.unique(lv["block_key"])
    per_block = np.unique(lv["block_key"], return_counts=True)[1]
    assert (lv["node_key"] >> 16).min() < depth - 1, "coarse leaves exist"
    assert (per_block == 8 ** (depth - 1)).any() and (per_block < 8 ** (depth - 1)).any(), "un-pruned and pruned blocks exist"
    assert lv["classified"].any() and not lv["classified"].all()
    want = P.stream_from_pool(h, *P.pool_of_leaves(h, lv, blocks))
    got = m.pack()
    _same_bytes(got, want, "pack vs helper")
    total, raw = P.assert_size_bound(got)
    print(f"depth {depth}: {blocks.size} blocks, {lv['A'].size} leaves, stream {total} bytes, raw pool {raw} bytes ({total / raw:.3f})")
    assert m.block_count() == blocks.size
    # round trip
    copy = _fresh(depth).unpack(got)
    R.assert_same(copy.leaves(), lv, LEAF_FIELDS, "leaves after unpack")
    _same_bytes(copy.pack(), got, "pack of the copy")
    # pack_info
    info = la3dm_amd.pack_info(got)
    p = P.parse(want)
    for k in ("version", "header_bytes", "variant", "block_depth", "nodes_per_block", "flags", "n_blocks", "n_leaves", "total_bytes"):
        assert info[k] == p[k], k
    assert [np.float32(info[k]).view(np.uint32) for k in P.FLOATS] == p["float_bits"].tolist()
    assert info["cls"] == "BGKOctoMap" and info["magic"] in (b"LA3DMAP", P.MAGIC) and info["n_blocks"] == blocks.size
    # save / load / load_map
    path = str(tmp_path / f"map{depth}.la3dm")
    m.save(path)
    _same_bytes(np.fromfile(path, np.uint8), got, "file bytes")
    assert not os.path.exists(path + ".tmp")
    assert la3dm_amd.pack_info(path) == info
    R.assert_same(_fresh(depth).load(path).leaves(), lv, LEAF_FIELDS, "leaves after load")
    lm = la3dm_amd.load_map(path, device=-1)
    assert type(lm).__name__ == "BGKOctoMap" and lm.get_block_depth() == depth and not lm.is_device_resident()
    R.assert_same(lm.leaves(), lv, LEAF_FIELDS, "leaves after load_map")
    _same_bytes(lm.pack(), got, "pack after load_map")
    with pytest.raises(RuntimeError, match="cannot open"):
        _fresh(depth).load(path + ".missing")


@pytest.mark.parametrize("depth", [3, 4])
def test_a_loaded_map_continues_bit_for_bit(built, depth):
    """CPU test 3: a third sim_structured scan (prepare / the emulated device step / commit, as fused_map inserts) into the
    original and into its unpacked copy: leaves() equal bit for bit, and so are the streams"""
    params = _params(depth)
    orig = _fresh(depth)
    for i in (1, 2):
        _insert_emulated(orig, params, i)
    R.assert_same(orig.leaves(), R.fused_map(depth)[1], LEAF_FIELDS, "the recipe map rebuilt")
    copy = _fresh(depth).unpack(orig.pack())
    before = orig.leaves()
    _insert_emulated(orig, params, 3)
    _insert_emulated(copy, params, 3)
    after = orig.leaves()
    assert after["A"].size != before["A"].size or (after["A"].view(np.uint32) != before["A"].view(np.uint32)).any()
    R.assert_same(copy.leaves(), after, LEAF_FIELDS, "leaves after the third scan")
    _same_bytes(copy.pack(), orig.pack(), "streams after the third scan")


CLASSES = {"BGKOctoMap": None, "BGKLOctoMap": "L_YAML", "GPOctoMap": "GP_YAML", "BGKLVOctoMap": "LV_YAML"}


@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("depth", [2, 3, 4])
def test_host_mode_loads_and_writes_any_valid_stream(built, cls, depth):
    """every class in host mode: a stream of random tilings (odd bit patterns, keys in no order) unpacks, and pack() is that
    stream in ascending key order; a BGK-LV map of the other original_size takes the stream's flag"""
    import la3dm_amd
    params = dict(getattr(la3dm_amd, CLASSES[cls]) if CLASSES[cls] else R.YAML, block_depth=depth)
    h = P.header_fields(cls, params)
    rng = np.random.default_rng(100 * depth + P.VARIANT[cls])
    nb, npb = 7, P.npb_of(depth)
    collapse = rng.random((nb, npb)) < 0.3
    collapse[0] = False
    collapse[1, 0] = True
    stream = P.stream_from_pool(h, *P.random_pool(rng, h, nb, collapse))
    P.assert_size_bound(stream)
    m = _fresh(depth, cls, params).unpack(stream)
    assert m.block_count() == nb
    _same_bytes(m.pack(), P.sorted_by_key(stream), (cls, depth))
    if cls != "BGKLVOctoMap":
        keys, A, B, S = P.canonical_pool(P.sorted_by_key(stream))
        lv, mask = m.leaves(), P.parse(P.sorted_by_key(stream))["mask"]
        assert lv["A"].size == mask.sum()
        assert sorted(lv["A"].view(np.uint32).tolist()) == sorted(A[mask].view(np.uint32).tolist())
    else:
        other = _fresh(depth, cls, dict(params, original_size=False)).unpack(stream)
        _same_bytes(other.pack(), P.sorted_by_key(stream), "the flag travels with the stream")
    with pytest.raises(RuntimeError, match="already holds blocks"):
        m.unpack(stream)
    assert m.block_count() == nb


def test_empty_map(built):
    """CPU test 6: an empty map packs to the header alone; unpacking that stream is a success that leaves the map empty"""
    import la3dm_amd
    h = P.header_fields("BGKOctoMap", _params(3))
    want = P.write(h, [], np.zeros((0, 73), bool), [], [], [])
    assert want.size == 128
    m = _fresh(3)
    _same_bytes(m.pack(), want, "empty map")
    m.unpack(want)
    assert m.block_count() == 0 and m.leaves()["A"].size == 0
    _same_bytes(m.pack(), want, "empty map after unpack")
    info = la3dm_amd.pack_info(want)
    assert info["n_blocks"] == 0 and info["n_leaves"] == 0 and info["total_bytes"] == 128


def test_corrupt_streams_are_refused(built):
    """CPU test 7: every row of the helper's table is refused with a message that names the defect, the map is still empty,
    and the valid stream is accepted afterwards; pack_info refuses the rows that are no stream of any map"""
    import la3dm_amd
    h = P.header_fields("BGKOctoMap", _params(3))
    rows = P.corrupt_table(h)
    names = [r[0] for r in rows]
    for want in ("wrong magic", "wrong version", "truncated", "one byte too long", "duplicate key", "key field out of range",
                 "leaf_off off by one", "mask bit past the end", "a leaf under a leaf", "a hole in the tiling", "PRUNED as a leaf state",
                 "non-zero padding", "mismatching block_depth", "mismatching variant", "mismatching resolution", "mismatching prior"):
        assert want in names, want
    m = _fresh(3)
    empty = m.pack()
    for name, stream, frag in rows[:-1]:
        with pytest.raises(RuntimeError) as e:
            m.unpack(stream)
        assert frag in str(e.value) and "unpack" in str(e.value), (name, str(e.value))
        assert m.block_count() == 0, name
        _same_bytes(m.pack(), empty, name)
        if name.startswith("mismatching"):
            assert la3dm_amd.pack_info(stream)["n_blocks"] > 0        # a valid stream, of another map
        else:
            with pytest.raises(RuntimeError) as e:
                la3dm_amd.pack_info(stream)
            assert frag in str(e.value), (name, str(e.value))
    name, valid, _ = rows[-1]
    m.unpack(valid)
    assert m.block_count() == 3
    _same_bytes(m.pack(), P.sorted_by_key(valid), "the valid stream afterwards")
    with pytest.raises(RuntimeError):
        m.unpack(b"")


def test_header_symbols_and_example(built, tmp_path):
    """CPU test 8: the headers declare and the libraries export the new symbols; the layout comment is there; the C view's
    size protocol; the example program (built by build()) runs on an empty host-mode map"""
    from la3dm_amd import _lib
    for header, so, names in (("la3dm_map.h", _lib.MAP_SO, ("la3dm_map_pack", "la3dm_map_unpack", "la3dm_map_save", "la3dm_map_load")),
                              ("la3dm_hip.h", _lib.HIP_SO, ("la3dm_devmap_pack_host", "la3dm_devmap_unpack_host", "la3dm_pack_info"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        if so == _lib.MAP_SO:
            C.CDLL(_lib.HIP_SO, mode=C.RTLD_GLOBAL)
        lib = C.CDLL(so)
        for n in names:
            assert re.search(r"\b" + n + r"\s*\(", txt), n
            assert hasattr(lib, n), n
            assert n in _lib.HIP_SYMBOLS + _lib.MAP_SYMBOLS, n
    hip_h = open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
    assert "la3dm_pack_header" in hip_h and 'magic[8] = "LA3DMAP' in hip_h and "NOT in the stream" in hip_h
    assert C.sizeof(_lib.PackHeader) == 128
    m, lv, _ = R.fused_map(3)
    M = _lib.maplib()
    size = C.c_uint64(0)
    assert M.la3dm_map_pack(m._h, None, 0, C.byref(size)) == 0 and size.value == m.pack().size
    small = np.zeros(64, np.uint8)
    assert M.la3dm_map_pack(m._h, small.ctypes.data, small.size, C.byref(size)) == -1
    assert b"smaller" in M.la3dm_map_last_error() and size.value == m.pack().size
    exe = os.path.join(ROOT, "examples", "resume_map")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "0"] +
                       "0.1 3 1.0 0.2 0.5 0.1 8.0 0.3 0.7 100.0 0.001 0.001 -1".split() + [str(tmp_path / "resume_map.la3dm")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("resume_map: 0 blocks, stream 128 bytes, raw pool 0 bytes; frontier 0 / 0: lists agree"), r.stdout
    assert lines[0].endswith("mirror_syncs 0 0 device_resident 0"), r.stdout
