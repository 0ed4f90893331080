"""merge on host-mode maps (device = -1, no GPU): every hand-built pair of tests/helpers/merge_cases.py — the shapes and tilings
tests/test_merge_gpu.py runs on the device pool — through m.merge against merge_ref, the refusals with pack() unchanged,
merge_file, the real two-scan maps, and the stand-alone checker of the per-block header.  The yardstick is written from the
contract comment in include/la3dm_hip.h (la3dm_devmap_merge_host); every comparison is exact, floats by their bits."""
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
import merge_cases as MC  # noqa: E402

INSERT = (0.1, 0.5, 8.0)
LEAF_FIELDS = ("block_key", "node_key", "loc", "size", "A", "B", "state", "classified")
STAT_KEYS = ("n_blocks", "n_created", "cells_kept", "cells_copied", "cells_fused")


def _params(cls, depth):
    import la3dm_amd
    return dict(R.YAML if cls == "BGKOctoMap" else la3dm_amd.L_YAML, block_depth=depth)   # (BGK-L: the small var_thresh, 0.15)


def _thresholds(params):
    return params["free_thresh"], params["occupied_thresh"], params["var_thresh"]


def _fresh(cls, params):
    import la3dm_amd
    return getattr(la3dm_amd, cls)(**params, device=-1)


def _same_bytes(a, b, what):
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    assert a.size == b.size, (what, a.size, b.size)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, (what, bad.size, bad[:8].tolist())


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("cls", ["BGKOctoMap", "BGKLOctoMap"])
def test_hand_built_pairs_against_the_yardstick(built, cls, depth):
    """every shape and tiling pair: unpack(dst), merge(src), then pack() == merge_ref's stream in key order and the stats are
    the yardstick's; the input conditions (all three cases, both sides of every threshold, collapses and splits) are counted
    from the yardstick first"""
    params = _params(cls, depth)
    h = P.header_fields(cls, params)
    th = _thresholds(params)
    pairs = MC.cases(h)
    cond = MC.conditions(h, th, pairs)
    print(f"{cls} depth {depth}: {len(pairs)} pairs, {cond}")
    assert cond["kept"] and cond["copied"] and cond["fused"] and cond["created"]
    assert cond["p_below_free"] and cond["p_between"] and cond["p_above_occ"]
    if cls == "BGKLOctoMap":
        assert cond["var_above"] and cond["var_below"], "the small var_thresh is straddled"
    if depth >= 2:
        assert cond["collapsed"] and cond["split"]
    for name, dst, src in pairs:
        want, stats = MC.merge_ref(dst, src, th)
        m = _fresh(cls, params).unpack(dst)
        got = m.merge(src)
        assert got == stats, (name, got, stats)
        assert tuple(got) == STAT_KEYS
        _same_bytes(m.pack(), P.sorted_by_key(want), (cls, depth, name))
        assert m.block_count() == P.parse(want)["n_blocks"], name


def test_forms_of_the_argument_order_and_repeatability(built, tmp_path):
    """bytes, a uint8 array, a map object and a file give one result; the stream's block order does not matter; merging the
    empty stream is a no-op with zero stats; a map is not merged into itself or into another class"""
    import la3dm_amd
    cls, depth = "BGKOctoMap", 3
    params = _params(cls, depth)
    h, th = P.header_fields(cls, params), _thresholds(params)
    name, dst, src = MC.cases(h)[-6]
    want = P.sorted_by_key(MC.merge_ref(dst, src, th)[0])
    other = _fresh(cls, params).unpack(src)
    path = str(tmp_path / "src.la3dm")
    other.save(path)
    p = P.parse(src)
    shuffled = P.stream_from_pool(h, *[np.ascontiguousarray(x[::-1]) for x in P.canonical_pool(src)])
    assert (P.parse(shuffled)["keys"] == p["keys"][::-1]).all() and p["n_blocks"] > 1
    results = []
    for arg in (src, src.tobytes(), bytearray(src.tobytes()), other, shuffled):
        m = _fresh(cls, params).unpack(dst)
        results.append(m.merge(arg))
        _same_bytes(m.pack(), want, type(arg).__name__)
    m = _fresh(cls, params).unpack(dst)
    results.append(m.merge_file(path))
    _same_bytes(m.pack(), want, "merge_file")
    assert all(r == results[0] for r in results), results
    with pytest.raises(RuntimeError, match="cannot open"):
        m.merge_file(path + ".missing")
    _same_bytes(m.pack(), want, "after a missing file")
    zero = m.merge(MC.empty_stream(h))
    assert zero == dict.fromkeys(STAT_KEYS, 0)
    _same_bytes(m.pack(), want, "after the empty stream")
    with pytest.raises(ValueError):
        m.merge(m)
    with pytest.raises(TypeError):
        m.merge(_fresh("BGKLOctoMap", _params("BGKLOctoMap", depth)))
    _same_bytes(m.pack(), want, "after the refused objects")


def test_refusals_leave_the_map_as_it_was(built):
    """every row of the corrupt-stream table (the validator's refusals and the mismatches with the map), and GPOctoMap and
    BGKLVOctoMap maps: RuntimeError that names the defect, pack() before == pack() after; the valid stream merges afterwards.
    (A poisoned map and a pool past 2^32 nodes cannot be brought about on a host-mode map in a test's time.)"""
    import la3dm_amd
    cls, depth = "BGKOctoMap", 3
    params = _params(cls, depth)
    h, th = P.header_fields(cls, params), _thresholds(params)
    rows = P.corrupt_table(h)
    dst = MC.cases(h)[5][1]
    assert P.parse(dst)["n_blocks"] > 0
    m = _fresh(cls, params).unpack(dst)
    before = m.pack()
    for name, stream, frag in rows[:-1]:
        with pytest.raises(RuntimeError) as e:
            m.merge(stream)
        assert frag in str(e.value) and "merge" in str(e.value), (name, str(e.value))
        _same_bytes(m.pack(), before, name)
    with pytest.raises(RuntimeError):
        m.merge(b"")
    _same_bytes(m.pack(), before, "the empty byte string")
    for other, yaml in (("GPOctoMap", la3dm_amd.GP_YAML), ("BGKLVOctoMap", la3dm_amd.LV_YAML)):
        po = dict(yaml, block_depth=3)
        ho = P.header_fields(other, po)
        rng = np.random.default_rng(3)
        own = P.stream_from_pool(ho, *P.random_pool(rng, ho, 3, np.zeros((3, 73), bool)))
        mo = _fresh(other, po).unpack(own)
        was = mo.pack()
        with pytest.raises(RuntimeError, match="BGKOctoMap .variant 0. and BGKLOctoMap"):
            mo.merge(own)
        _same_bytes(mo.pack(), was, other)
    # odd_values never reach a fused cell: the table's valid stream has them, so it goes into a map whose blocks are elsewhere
    name, valid, _ = rows[-1]
    assert not set(P.parse(valid)["keys"].tolist()) & set(P.parse(dst)["keys"].tolist())
    stats = m.merge(valid)
    assert stats["n_created"] == 3 and stats["cells_fused"] == 0
    _same_bytes(m.pack(), P.sorted_by_key(MC.merge_ref(dst, valid, th)[0]), "the valid stream afterwards")


def _insert_emulated(m, params, scan):
    import la3dm_amd
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", scan))
    assert m.prepare(xyz, origin, *INSERT)
    R._emulate_device(m.packed(), params)
    m.commit()


@pytest.mark.parametrize("depth", [3, 4])
def test_real_maps(built, depth):
    """two maps from different sim_structured scans (coarse leaves, un-pruned blocks, shared and private blocks): one merged
    into the other == merge_ref of their two packs; merging into an empty map == unpack of the stream (a real map's pack is
    prune-stable); a further scan goes into the merged map"""
    params = _params("BGKOctoMap", depth)
    h, th = P.header_fields("BGKOctoMap", params), _thresholds(params)
    a, b = _fresh("BGKOctoMap", params), _fresh("BGKOctoMap", params)
    _insert_emulated(a, params, 1)
    _insert_emulated(b, params, 2)
    sa, sb = a.pack(), b.pack()
    d = {}
    want, stats = MC.merge_ref(sa, sb, th, d)
    print(f"depth {depth}: {P.parse(sa)['n_blocks']} + {P.parse(sb)['n_blocks']} blocks, {stats}")
    assert stats["n_created"] > 0 and stats["n_created"] < stats["n_blocks"] and stats["cells_fused"] and stats["cells_kept"] and stats["cells_copied"]
    assert a.merge(b) == stats
    _same_bytes(a.pack(), P.sorted_by_key(want), "merged real maps")
    _same_bytes(a.pack(), a.pack(), "two packs")
    empty = _fresh("BGKOctoMap", params)
    got = empty.merge(sb)
    assert got["n_created"] == got["n_blocks"] == P.parse(sb)["n_blocks"] and got["cells_fused"] == 0
    _same_bytes(empty.pack(), sb, "merge into an empty map == unpack")
    R.assert_same(empty.leaves(), b.leaves(), LEAF_FIELDS, "leaves")
    before = a.leaves()
    _insert_emulated(a, params, 3)
    after = a.leaves()
    assert after["A"].size != before["A"].size or (after["A"].view(np.uint32) != before["A"].view(np.uint32)).any()


def test_header_symbols_checker_and_example(built, tmp_path):
    """the headers declare and the libraries export the new symbols; the contract comment is there; the C view with stats =
    NULL; the per-block header's checker (tools/check/merge_block.cpp, a stand-alone CPU program) builds and runs clean under
    the host sanitizers; examples/merge_maps (built by build()) runs on empty host-mode maps"""
    from la3dm_amd import _lib
    for header, so, names in (("la3dm_map.h", _lib.MAP_SO, ("la3dm_map_merge", "la3dm_map_merge_file")),
                              ("la3dm_hip.h", _lib.HIP_SO, ("la3dm_devmap_merge_host",))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        if so == _lib.MAP_SO:
            C.CDLL(_lib.HIP_SO, mode=C.RTLD_GLOBAL)
        lib = C.CDLL(so)
        for n in names:
            assert re.search(r"\b" + n + r"\s*\(", txt), n
            assert hasattr(lib, n), n
            assert n in _lib.HIP_SYMBOLS + _lib.MAP_SYMBOLS, n
    hip_h = open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
    assert "la3dm_merge_stats" in hip_h and "A1 + (A2 - init_A)" in hip_h and "STREAM ORDER" in hip_h
    assert C.sizeof(_lib.MergeStats) == 40
    params = _params("BGKOctoMap", 3)
    h = P.header_fields("BGKOctoMap", params)
    name, dst, src = MC.cases(h)[7]
    m = _fresh("BGKOctoMap", params).unpack(dst)
    assert _lib.maplib().la3dm_map_merge(m._h, src.ctypes.data, src.size, None) == 0
    _same_bytes(m.pack(), P.sorted_by_key(MC.merge_ref(dst, src, _thresholds(params))[0]), "stats = NULL")
    exe = str(tmp_path / "merge_block")
    # (the sanitizers' runtimes are linked into the program itself: it runs the same whatever else the process environment loads)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "check", "merge_block.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all cases hold" in r.stdout and "FAIL" not in r.stdout, (r.stdout, r.stderr)
    exe = os.path.join(ROOT, "examples", "merge_maps")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "0"] +
                       "0.1 3 1.0 0.2 0.5 0.1 8.0 0.3 0.7 100.0 0.001 0.001 -1".split(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("merge_maps: 0 + 0 blocks -> 0 (0 created); cells kept 0 copied 0 fused 0; frontier 0 -> 0"), r.stdout
    assert lines[0].endswith("mirror_syncs 0 device_resident 0"), r.stdout
