"""diff on host-mode maps (device = -1, no GPU): every hand-built pair of tests/helpers/diff_cases.py — the shapes and tilings
tests/test_diff_gpu.py runs on the device pool — through m.diff against diff_ref, the map against its own pack, the refusals
with everything untouched, cap and count-only, diff_file, and the stand-alone checker of the per-block header.  The yardstick
is written from the contract comment in include/la3dm_hip.h (la3dm_devmap_diff_host); every comparison is exact, floats by
their bits."""
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
import diff_cases as D  # noqa: E402

ALL_PAIRS = (1 << 25) - 1
COMBOS = ((D.PAIRS_CHANGED, 0, True), (D.PAIRS_CHANGED, 0x1F, False), (D.pair_bit(0, 1), 0, True), (0, 1 << 2, True), (ALL_PAIRS, 0x1F, True))


def _yaml(cls):
    import la3dm_amd
    return dict(BGKOctoMap=la3dm_amd.BGK_YAML, GPOctoMap=la3dm_amd.GP_YAML, BGKLVOctoMap=la3dm_amd.LV_YAML, BGKLOctoMap=la3dm_amd.L_YAML)[cls]


def _fresh(cls, params):
    import la3dm_amd
    return getattr(la3dm_amd, cls)(**params, device=-1)


def _same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    assert a.size == b.size, (what, a.size, b.size)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, (what, bad.size, bad[:8].tolist())


@pytest.mark.parametrize("cls,depth", [("BGKOctoMap", 1), ("BGKOctoMap", 2), ("BGKOctoMap", 3), ("BGKOctoMap", 4), ("GPOctoMap", 3),
                                       ("BGKLVOctoMap", 3), ("BGKLOctoMap", 3)])
def test_hand_built_cases_against_the_yardstick(built, cls, depth):
    """every case and every mask combination: the list in order (stream blocks in stream order, then the map's other blocks
    in ascending key), centre, A, B, the 5 x 5 table, the value-changed counts and the block counts; pack() is unchanged"""
    params = dict(_yaml(cls), block_depth=depth)
    h = P.header_fields(cls, params)
    cases = D.cases(h)
    cond = D.conditions(cases)
    print(f"{cls} depth {depth}: {len(cases)} cases, pairs {cond['pairs'].astype(int).tolist()}, value_changed {cond['value_changed'].astype(int).tolist()}")
    assert np.trace(cond["pairs"]) and cond["pairs"].sum() > np.trace(cond["pairs"]) and cond["value_changed"].any()
    assert cond["n_missing_now"] and cond["n_map_only_blocks"]
    if cls == "BGKLVOctoMap":
        assert cond["pairs"][4].all() and cond["pairs"][:, 4].all(), "UNCERTAIN leaves on both sides"
    for name, now, then in cases:
        m = _fresh(cls, params).unpack(now)
        before = m.pack()
        assert (np.diff(P.parse(before)["keys"]) > 0).all()
        for pm, vm, mo in COMBOS:
            want = D.diff_ref(before, then, pm, vm, mo, m.lut(), m.hash_key_to_block)
            D.assert_same(m.diff(then, pairs=pm, values=vm, map_only=mo, fields=D.LIST_FIELDS), want, (cls, depth, name, pm, vm, mo))
        _same_bytes(m.pack(), before, (name, "pack() after the diffs"))


def test_the_map_against_its_own_pack(built):
    """n = 0 and a diagonal pairs table, values included; as bytes, a uint8 array, a map object and a file; names for pairs"""
    cls, depth = "BGKOctoMap", 3
    params = dict(_yaml(cls), block_depth=depth)
    h = P.header_fields(cls, params)
    name, now, then = D.union_case(h, np.random.default_rng(1), 6)
    m = _fresh(cls, params).unpack(now)
    own = m.pack()
    for arg in (own, own.tobytes(), bytearray(own.tobytes()), _fresh(cls, params).unpack(own)):
        r = m.diff(arg, values=0x1F)
        assert r["n"] == 0 and r["block_key"].size == 0 and r["value_changed"].sum() == 0, type(arg).__name__
        assert r["pairs"].sum() == np.trace(r["pairs"]) == 5 * 64 and r["n_map_only_blocks"] == 0 == r["n_missing_now"]
    want = D.diff_ref(own, then, D.pair_bit(0, 1) | D.pair_bit(3, 2), 1 << 1, True)
    got = m.diff(then, pairs=[("free", "occupied"), ("missing", "unknown")], values=("occupied",), fields=("cell", "code", "A"))
    D.assert_same(got, want, "pairs and values by name")
    assert set(got) >= {"cell", "code", "A"} and "block_key" not in got and "B" not in got
    assert m.diff(then, pairs="changed")["n"] == D.diff_ref(own, then)["n"] > 0
    with pytest.raises(TypeError):
        m.diff(_fresh("BGKLOctoMap", dict(_yaml("BGKLOctoMap"), block_depth=depth)))
    with pytest.raises(ValueError):
        m.diff(then, fields=("nothing",))
    with pytest.raises(KeyError):
        m.diff(then, pairs=[("free", "solid")])


def _raw(m, then, pm, vm, mo, cap, room, with_out=True, with_found=True):
    """la3dm_map_diff itself on buffers of `room` entries filled with a guard pattern: (rc, n_found, buffers, stats)"""
    from la3dm_amd import _lib
    M = _lib.maplib()
    buf = {f: np.frombuffer(bytes([0xA5]) * (room * w * np.dtype(t).itemsize), np.uint8).copy() for f, (t, w) in m._DIFF_FIELDS.items()}
    o = _lib.DiffOut(*[buf[f].ctypes.data for f, _ in _lib.DiffOut._fields_])
    params = _lib.DiffParams(pm, vm, 1 if mo else 0)
    found, stats = C.c_uint64(0xA5A5), _lib.DiffStats()
    C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
    s = np.ascontiguousarray(then, np.uint8)
    rc = M.la3dm_map_diff(m._h, s.ctypes.data if s.size else None, s.size, C.byref(params), cap, C.byref(o) if with_out else None,
                          C.byref(found) if with_found else None, C.byref(stats))
    return rc, int(found.value), buf, stats


def test_refusals_leave_everything_untouched(built):
    """every row of the corrupt-stream table (the validator's refusals and the mismatches with the map), mask bits out of
    range, a NULL n_found, cap > 0 with out NULL: -1 and a text that names the defect; *n_found, the stats and the buffers
    keep their guard pattern, pack() before == pack() after; the valid stream is compared afterwards"""
    from la3dm_amd import _lib
    cls, depth = "BGKOctoMap", 3
    params = dict(_yaml(cls), block_depth=depth)
    h = P.header_fields(cls, params)
    rows = P.corrupt_table(h)
    name, now, then = D.union_case(h, np.random.default_rng(5), 5)
    m = _fresh(cls, params).unpack(now)
    before = m.pack()
    err = lambda: _lib.maplib().la3dm_map_last_error().decode()   # noqa: E731

    def untouched(rc, found, buf, stats, what):
        assert rc == -1 and found == 0xA5A5, (what, rc, found)
        assert all((b == 0xA5).all() for b in buf.values()) and set(bytes(stats)) == {0xA5}, what
        _same_bytes(m.pack(), before, what)

    for name, stream, frag in rows[:-1]:
        untouched(*_raw(m, stream, D.PAIRS_CHANGED, 0, True, 4, 4), name)
        assert frag in err() and "diff" in err(), (name, err())
        with pytest.raises(RuntimeError):
            m.diff(stream)
    untouched(*_raw(m, np.zeros(0, np.uint8), D.PAIRS_CHANGED, 0, True, 4, 4), "a null stream")
    untouched(*_raw(m, then, 1 << 25, 0, True, 4, 4), "pair_mask bit 25")
    assert "pair_mask" in err()
    untouched(*_raw(m, then, D.PAIRS_CHANGED, 1 << 5, True, 4, 4), "value_mask bit 5")
    assert "value_mask" in err()
    untouched(*_raw(m, then, D.PAIRS_CHANGED, 0, True, 4, 4, with_out=False), "cap > 0 with out NULL")
    assert "out is NULL" in err()
    untouched(*_raw(m, then, D.PAIRS_CHANGED, 0, True, 4, 4, with_found=False), "n_found NULL")
    assert "n_found" in err()
    with pytest.raises(RuntimeError, match="pair_mask"):
        m.diff(then, pairs=1 << 25)
    with pytest.raises(RuntimeError, match="value_mask"):
        m.diff(then, values=1 << 5)
    name, valid, _ = rows[-1]
    D.assert_same(m.diff(valid, fields=D.LIST_FIELDS), D.diff_ref(before, valid, lut=m.lut(), centre_of=m.hash_key_to_block), "the valid stream afterwards")


def test_cap_count_only_and_file(built, tmp_path):
    """cap = 0 (out NULL: count-only), 1, inside the list, n - 1, n and beyond: *n_found and the stats are the full call's, the
    first min(n, cap) entries the full list's, not a byte past them written; diff_file == diff; stats = NULL"""
    from la3dm_amd import _lib
    cls, depth = "BGKOctoMap", 4
    params = dict(_yaml(cls), block_depth=depth)
    h = P.header_fields(cls, params)
    name, now, then = D.union_case(h, np.random.default_rng(77), 6)
    m = _fresh(cls, params).unpack(now)
    pm, vm, mo = D.PAIRS_CHANGED, 0x1F, True
    want = D.diff_ref(m.pack(), then, pm, vm, mo, m.lut(), m.hash_key_to_block)
    n = want["n"]
    assert n > 600
    rc, found, _, stats = _raw(m, then, pm, vm, mo, 0, 4, with_out=False)
    assert rc == 0 and found == n and np.array(stats.pairs, np.uint64).reshape(5, 5).tolist() == want["pairs"].tolist()
    for cap in (0, 1, n // 2, n - 1, n, n + 3):
        rc, found, buf, stats = _raw(m, then, pm, vm, mo, cap, n + 8)
        assert rc == 0 and found == n, (cap, rc, found)
        assert np.array(stats.value_changed, np.uint64).tolist() == want["value_changed"].tolist(), cap
        k = min(cap, n)
        for f, (t, w) in m._DIFF_FIELDS.items():
            size = w * np.dtype(t).itemsize
            _same_bytes(buf[f][:k * size], np.ascontiguousarray(want[f][:k]), (cap, f))
            assert (buf[f][k * size:] == 0xA5).all(), (cap, f, "written past min(n, cap)")
        D.assert_same(m.diff(then, values=vm, fields=D.LIST_FIELDS, cap=cap), want, ("cap", cap), cap=cap)
    path = str(tmp_path / "then.la3dm")
    _fresh(cls, params).unpack(then).save(path)
    by_file = m.diff_file(path, values=vm, fields=D.LIST_FIELDS)
    D.assert_same(by_file, D.diff_ref(m.pack(), P.sorted_by_key(then), pm, vm, mo, m.lut(), m.hash_key_to_block), "diff_file")
    with pytest.raises(RuntimeError, match="cannot open"):
        m.diff_file(path + ".missing")
    s = np.ascontiguousarray(then, np.uint8)
    found = C.c_uint64(0)
    p = _lib.DiffParams(pm, vm, 1)
    assert _lib.maplib().la3dm_map_diff(m._h, s.ctypes.data, s.size, C.byref(p), 0, None, C.byref(found), None) == 0 and found.value == n


def test_header_symbols_checker_and_example(built, tmp_path):
    """the headers declare and the libraries export the new symbols; the contract comment is there; the per-block header's
    checker (tools/check/diff_block.cpp, a stand-alone CPU program) builds and runs clean under the host sanitizers;
    examples/changes (built by build()) runs on an empty host-mode map"""
    from la3dm_amd import _lib
    for header, so, names in (("la3dm_map.h", _lib.MAP_SO, ("la3dm_map_diff", "la3dm_map_diff_file")),
                              ("la3dm_hip.h", _lib.HIP_SO, ("la3dm_devmap_diff_host",))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        if so == _lib.MAP_SO:
            C.CDLL(_lib.HIP_SO, mode=C.RTLD_GLOBAL)
        lib = C.CDLL(so)
        for n in names:
            assert re.search(r"\b" + n + r"\s*\(", txt), n
            assert hasattr(lib, n), n
            assert n in _lib.HIP_SYMBOLS + _lib.MAP_SYMBOLS, n
    hip_h = open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
    assert "la3dm_diff_stats" in hip_h and "VALUE-CHANGED" in hip_h and "5 * then + now" in hip_h
    m = re.search(r"#define LA3DM_DIFF_PAIRS_CHANGED (0x[0-9A-Fa-f]+)u", hip_h)
    import la3dm_amd
    assert m and int(m.group(1), 16) == D.PAIRS_CHANGED == la3dm_amd.DIFF_PAIRS_CHANGED
    assert C.sizeof(_lib.DiffStats) == 8 * 33 and C.sizeof(_lib.DiffParams) == 12 and C.sizeof(_lib.DiffOut) == 48
    exe = str(tmp_path / "diff_block")
    # (the sanitizers' runtimes are linked into the program itself: it runs the same whatever else the process environment loads)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "check", "diff_block.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all cases hold" in r.stdout and "FAIL" not in r.stdout, (r.stdout, r.stderr)
    exe = os.path.join(ROOT, "examples", "changes")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "0"] +
                       "0.1 3 1.0 0.2 0.5 0.1 8.0 0.3 0.7 100.0 0.001 0.001 -1".split(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0] == ("changes: 0 -> 0 blocks; cells newly occupied 0 no longer occupied 0 newly observed 0 changed 0; "
                                            "self diff 0; mirror_syncs 0 device_resident 0"), r.stdout
