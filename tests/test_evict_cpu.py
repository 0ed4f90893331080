"""pack_region / erase_region / evict on host-mode maps (device = -1, no GPU) against tests/helpers/evict_cases.py, the numpy
yardstick written from the contract comment in include/la3dm_hip.h (la3dm_devmap_pack_region_host): the sub-stream byte for
byte, inside and outside as a partition of pack, erase then pack, evict_file then load_map, the refusals, the yardstick's
own hole / tail rule on hand-written flags, and the stand-alone checker of the shared header.  A host-mode map writes its
blocks in ascending key order, so the yardstick runs on the key-sorted stream."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import pack_cases as P  # noqa: E402
import evict_cases as EC  # noqa: E402

YAMLS = dict(BGKOctoMap="BGK_YAML", BGKLOctoMap="L_YAML", GPOctoMap="GP_YAML", BGKLVOctoMap="LV_YAML")
STAT_KEYS = ("n_removed", "n_moved", "n_blocks")


def _params(cls, depth):
    import la3dm_amd
    return dict(getattr(la3dm_amd, YAMLS[cls]), block_depth=depth)


def _fresh(cls, params):
    import la3dm_amd
    return getattr(la3dm_amd, cls)(**params, device=-1)


def _same_bytes(a, b, what):
    if isinstance(a, (bytes, bytearray)):
        a = np.frombuffer(a, np.uint8)
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    assert a.size == b.size, (what, a.size, b.size)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, (what, bad.size, bad[:8].tolist())


def _points(m, klo, khi):
    """the centres of the blocks klo and khi: the world points that name the box"""
    return (m.hash_key_to_block(int(EC.make_keys(*klo))), m.hash_key_to_block(int(EC.make_keys(*khi))))


def _case(cls, depth, name, n, seed):
    params = _params(cls, depth)
    h = P.header_fields(cls, params)
    rng = np.random.default_rng(seed)
    keys, klo, khi, inside, flags = EC.pattern_case(name, n, rng)
    stream = P.stream_from_pool(h, *P.random_pool(rng, h, n, rng.random((n, P.npb_of(depth))) < 0.1, keys=keys))
    return params, P.sorted_by_key(stream), klo, khi, inside, flags


def test_the_hole_tail_rule_on_hand_written_flags():
    """pure numpy: the order and the number of moves the contract prescribes"""
    for removed, order, moved in (([], [], 0), ([0, 0, 0], [0, 1, 2], 0), ([1, 1, 1], [], 0), ([0, 0, 1], [0, 1], 0),
                                  ([1, 0, 0], [2, 1], 1), ([1, 1, 0, 0], [2, 3], 2), ([1, 0, 1, 0, 1], [3, 1], 1),
                                  ([1, 0, 1, 1, 0, 1], [4, 1], 1), ([0, 1, 1, 0, 0, 1, 0], [0, 4, 6, 3], 2),
                                  ([1, 1, 1, 0, 1, 0, 0, 0], [5, 6, 7, 3], 3)):
        got, n_moved = EC.compact_order(removed)
        assert got.tolist() == order and n_moved == moved, (removed, got.tolist(), n_moved)
    rng = np.random.default_rng(1)
    for n in (1, 2, 5, 64, 65, 257):
        for name in EC.PATTERNS:
            f = EC.pattern_flags(name, n, rng)
            order, moved = EC.compact_order(f)
            n_new = n - int(f.sum())
            assert order.size == n_new and not f[order].any() and np.unique(order).size == n_new
            stay = ~f[:n_new]
            assert (order[stay] == np.nonzero(stay)[0]).all() and moved == int(f[:n_new].sum())
            assert (np.diff(order[~stay]) > 0).all() and (order[~stay] >= n_new).all()
    assert EC.pattern_flags("first half", 257, rng).sum() == 129 and EC.compact_order(EC.pattern_flags("first half", 257, rng))[1] == 128
    assert EC.compact_order(EC.pattern_flags("second half", 257, rng))[1] == 0
    f = EC.pattern_flags("most removed", 257, rng)
    assert f.sum() > 257 - f.sum() and f[257 - int(f.sum()):].any() and not f[257 - int(f.sum()):].all()


@pytest.mark.parametrize("depth", [1, 3, 4])
@pytest.mark.parametrize("cls", ["BGKOctoMap", "BGKLOctoMap", "GPOctoMap", "BGKLVOctoMap"])
def test_pack_region_and_erase_region_against_the_yardstick(built, cls, depth):
    """every selection pattern on 5 and 65 blocks: pack_region byte for byte the yardstick's sub-stream, the map unchanged;
    inside and outside of the same box partition pack's blocks; erase_region then pack == the yardstick's stream in key
    order, the stats, block_count; the GP map's exact header floats and the LV map's flag and UNCERTAIN leaves travel"""
    seen_uncertain = False
    for n in (5, 65):
        for k, name in enumerate(EC.PATTERNS):
            params, stream, klo, khi, inside, flags = _case(cls, depth, name, n, 100 * depth + 10 * n + k)
            m = _fresh(cls, params).unpack(stream)
            lo, hi = _points(m, klo, khi)
            what = (cls, depth, n, name)
            got = m.pack_region(lo, hi, inside=bool(inside))
            _same_bytes(got, EC.sub_stream(stream, klo, khi, inside), what)
            _same_bytes(m.pack(), stream, (what, "the map is not changed"))
            other = m.pack_region(lo, hi, inside=not inside)
            ka, kb, kall = P.parse(got)["keys"], P.parse(other)["keys"], P.parse(stream)["keys"]
            assert not set(ka.tolist()) & set(kb.tolist()) and sorted(ka.tolist() + kb.tolist()) == kall.tolist(), what
            assert ka.size == int(flags.sum())
            import la3dm_amd
            assert la3dm_amd.pack_info(got)["n_blocks"] == ka.size and la3dm_amd.pack_info(got)["cls"] == cls
            seen_uncertain |= bool(((P.parse(got)["state"] & 7) == P.UNCERTAIN).any())
            want, stats = EC.erased_stream(stream, klo, khi, inside)
            st = m.erase_region(lo, hi, inside=bool(inside))
            assert tuple(st) == STAT_KEYS and st["n_removed"] == stats["n_removed"] and st["n_blocks"] == stats["n_blocks"], (what, st, stats)
            _same_bytes(m.pack(), P.sorted_by_key(want), (what, "after the erase"))
            assert m.block_count() == stats["n_blocks"]
            # what was erased comes back through unpack of the sub-stream into a fresh map; an erased map takes blocks again
            if name == "everything":
                _same_bytes(m.unpack(got).pack(), stream, (what, "an emptied map loads like a new one"))
    if cls == "BGKLVOctoMap":
        assert seen_uncertain, "UNCERTAIN leaves went through pack_region"
        assert P.parse(got)["flags"] == 1


def test_evict_and_evict_file(built, tmp_path):
    """evict returns pack_region's bytes and erases; evict_file writes the same stream through path + ".tmp" (no .tmp left),
    load_map reads it; merging the evicted file back restores the map (a prune-stable pool: the helper asserts it)"""
    import la3dm_amd
    cls, depth, n = "BGKOctoMap", 3, 9
    params = _params(cls, depth)
    h = P.header_fields(cls, params)
    rng = np.random.default_rng(5)
    keys, klo, khi, inside, flags = EC.pattern_case("alternating", n, rng)
    stream = P.sorted_by_key(P.stream_from_pool(h, *EC.stable_pool(rng, h, n, rng.random((n, 73)) < 0.1, keys)))
    EC.assert_merge_restores(stream)
    want_sub = EC.sub_stream(stream, klo, khi, inside)
    want_left = P.sorted_by_key(EC.erased_stream(stream, klo, khi, inside)[0])
    m = _fresh(cls, params).unpack(stream)
    lo, hi = _points(m, klo, khi)
    got = m.evict(lo, hi)
    assert isinstance(got, bytes)
    _same_bytes(got, want_sub, "evict's stream")
    _same_bytes(m.pack(), want_left, "after evict")
    m2 = _fresh(cls, params).unpack(stream)
    path = str(tmp_path / "far.la3dm")
    st = m2.evict_file(path, lo, hi, inside=True)
    assert st["n_removed"] == int(flags.sum()) and st["n_blocks"] == n - int(flags.sum())
    assert os.listdir(tmp_path) == ["far.la3dm"]
    _same_bytes(np.fromfile(path, np.uint8), want_sub, "the file")
    loaded = la3dm_amd.load_map(path, device=-1)
    assert type(loaded).__name__ == cls and loaded.block_count() == int(flags.sum())
    _same_bytes(loaded.pack(), want_sub, "load_map of the file")
    _same_bytes(m2.pack(), want_left, "after evict_file")
    back = m2.merge_file(path)
    assert back["n_created"] == back["n_blocks"] == int(flags.sum()) and back["cells_fused"] == 0
    _same_bytes(m2.pack(), stream, "evict_file, then merge_file: the map is back")
    assert m.merge(got)["n_created"] == int(flags.sum())
    _same_bytes(m.pack(), stream, "evict, then merge")


def test_refusals_leave_the_map_as_it_was(built, tmp_path):
    """klo > khi on each axis; a path that cannot be written (evict_file removes nothing); a buffer that is too small (the C
    view sets *size); null points; each with pack() unchanged.  (A poisoned map cannot be brought about in host mode.)"""
    from la3dm_amd import _lib
    cls, depth, n = "BGKOctoMap", 3, 5
    params, stream, klo, khi, inside, flags = _case(cls, depth, "alternating", n, 77)
    m = _fresh(cls, params).unpack(stream)
    X = EC.X_IN
    box = ((X, 524288 - 300, 0), (X, 524288 + 8 * n + 300, 524288 + 300))   # every selected block of the pattern, by its y
    lo, hi = _points(m, *box)
    bs = m.hash_key_to_block(int(EC.make_keys(524289, 524288, 524288)))[0]      # one block's width
    for axis in range(3):
        bad_lo = np.array(lo, np.float32)
        bad_lo[axis] = hi[axis] + 2 * bs
        for call in (lambda: m.pack_region(bad_lo, hi), lambda: m.erase_region(bad_lo, hi), lambda: m.evict(bad_lo, hi),
                     lambda: m.evict_file(str(tmp_path / "x"), bad_lo, hi)):
            with pytest.raises(RuntimeError, match=f"klo > khi on axis {axis}"):
                call()
        _same_bytes(m.pack(), stream, ("klo > khi", axis))
    assert os.listdir(tmp_path) == []
    with pytest.raises(RuntimeError, match="cannot open"):
        m.evict_file(str(tmp_path / "no_such_dir" / "far.la3dm"), lo, hi)
    _same_bytes(m.pack(), stream, "a bad path: nothing was removed")
    with pytest.raises(ValueError):
        m.pack_region([0.0, 0.0], hi)
    M = _lib.maplib()
    lo3, hi3 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    want = EC.sub_stream(stream, *box, 1)
    assert 0 < P.parse(want)["n_blocks"] <= int(flags.sum())
    n_sel = P.parse(want)["n_blocks"]
    for fn, extra in ((M.la3dm_map_pack_region, ()), (M.la3dm_map_evict, (None,))):
        size = C.c_uint64(0)
        buf = np.zeros(want.size, np.uint8)
        assert fn(m._h, lo3.ctypes.data, hi3.ctypes.data, 1, buf.ctypes.data, want.size - 1, C.byref(size), *extra) == -1
        assert size.value == want.size and "smaller than the stream" in M.la3dm_map_last_error().decode()
        assert not buf.any()
        _same_bytes(m.pack(), stream, "cap too small")
        assert fn(m._h, lo3.ctypes.data, hi3.ctypes.data, 1, None, 0, C.byref(size), *extra) == 0 and size.value == want.size
        _same_bytes(m.pack(), stream, "buf = NULL only sizes")
        assert fn(m._h, None, hi3.ctypes.data, 1, None, 0, C.byref(size), *extra) == -1
        assert fn(m._h, lo3.ctypes.data, hi3.ctypes.data, 1, None, 0, None, *extra) == -1
    assert M.la3dm_map_erase_region(m._h, lo3.ctypes.data, None, 1, None) == -1
    assert M.la3dm_map_evict_file(m._h, None, lo3.ctypes.data, hi3.ctypes.data, 1, None) == -1
    _same_bytes(m.pack(), stream, "after the C view's refusals")
    assert M.la3dm_map_erase_region(m._h, lo3.ctypes.data, hi3.ctypes.data, 1, None) == 0      # stats = NULL
    assert m.block_count() == n - n_sel


def test_header_symbols_checker_and_example(built, tmp_path):
    """the headers declare and the libraries export the new symbols; the contract comment is there; the shared header's checker
    (tools/check/region_blocks.cpp, a stand-alone CPU program) builds and runs clean under the host sanitizers;
    examples/rolling_map (built by build()) runs on empty host-mode maps"""
    from la3dm_amd import _lib
    for header, so, names in (("la3dm_map.h", _lib.MAP_SO, ("la3dm_map_pack_region", "la3dm_map_erase_region", "la3dm_map_evict", "la3dm_map_evict_file")),
                              ("la3dm_hip.h", _lib.HIP_SO, ("la3dm_devmap_pack_region_host", "la3dm_devmap_erase_region_host"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        if so == _lib.MAP_SO:
            C.CDLL(_lib.HIP_SO, mode=C.RTLD_GLOBAL)
        lib = C.CDLL(so)
        for n in names:
            assert re.search(r"\b" + n + r"\s*\(", txt), n
            assert hasattr(lib, n), n
            assert n in _lib.HIP_SYMBOLS + _lib.MAP_SYMBOLS, n
    hip_h = open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
    assert "la3dm_erase_stats" in hip_h and "the block in t_i moves to h_i" in hip_h and "n_new = n_old - n_removed" in hip_h
    assert C.sizeof(_lib.EraseStats) == 24
    exe = str(tmp_path / "region_blocks")
    # (the sanitizers' runtimes are linked into the program itself: it runs the same whatever else the process environment loads)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "check", "region_blocks.cpp"), "-o", exe, "-lpthread"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all cases hold" in r.stdout and "FAIL" not in r.stdout, (r.stdout, r.stderr)
    exe = os.path.join(ROOT, "examples", "rolling_map")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "0", str(tmp_path)] +
                       "4.0 0.1 3 1.0 0.2 0.5 0.1 8.0 0.3 0.7 100.0 0.001 0.001 -1".split(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0] == ("rolling_map: held at most 0 of 0 blocks; 0 files merged back (0 created) -> 0 blocks; frontier 0 vs 0 "
                                            "equal 1; device_resident 0"), r.stdout
