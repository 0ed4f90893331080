"""raycast_many on a host-mode map (device = -1, no GPU): the batched client loop over the RayCaster with the covering
leaf of every row, against an independent reduction of the iterator's rows (tests/helpers/raycast_cases.py).  The map is
two fused and pruned scans, so collapsed regions — where the raw finest-layer node reads PRUNED — are on the rays."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, pcd_path

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import raycast_cases as RC  # noqa: E402

YAML = dict(resolution=0.1, block_depth=3, sf2=1.0, ell=0.2, free_thresh=0.3, occupied_thresh=0.7, var_thresh=100.0,
            prior_A=0.001, prior_B=0.001)


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


def _fused_map(depth):
    """sim_structured scans 1 and 2, fused and pruned on a bookkeeping-only map; with its leaves, rays and the two
    host-form runs the input conditions are computed from"""
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
        s, e, names = RC.all_rays(lv)
        _MAPS[depth] = (m, lv, s, e, names)
    return _MAPS[depth]


@pytest.mark.parametrize("depth", [3, 4])
def test_rays_exercise_the_feature(built, depth):
    """conditions on the INPUTS, from the host form: enough hits, non-hits, missing blocks and hits on collapsed regions"""
    m, lv, s, e, names = _fused_map(depth)
    if depth == 4:
        print(f"leaves {lv['state'].size}, FREE {(lv['state'] == 0).sum()}, OCCUPIED {(lv['state'] == 1).sum()}, "
              f"coarser than the base resolution {((lv['node_key'] >> 16) < depth - 1).sum()}")
    occ = m.raycast_many(s, e, stop=("occupied",), max_steps=4096)
    full = m.raycast_many(s, e, stop=(), max_steps=4096)
    RC.assert_rays_exercise_the_feature(RC.category_counts(occ, full, depth), depth)
    # a client that walks the raw nodes until state == OCCUPIED misses every hit on a collapsed region
    q = np.nonzero((occ["flags"][:RC.N_RECIPE] & RC.HIT != 0) & (occ["leaf_depth"][:RC.N_RECIPE] < depth - 1))[0]
    for r in q[:10]:
        rows = m.raycast(s[r], e[r])
        j = int(occ["steps"][r]) - 1
        assert rows["state"][j] == 3 and occ["cls"][r] == RC.OCCUPIED          # PRUNED raw node, OCCUPIED covering leaf


@pytest.mark.parametrize("max_steps", [4096, 7])
@pytest.mark.parametrize("stop", ["occupied", "occupied|missing", "none"])
@pytest.mark.parametrize("depth", [3, 4])
def test_raycast_many_equals_the_reduction_of_the_iterator(built, depth, stop, max_steps):
    m, lv, s, e, names = _fused_map(depth)
    mask = RC.STOPS[stop]
    got = m.raycast_many(s, e, stop=mask, max_steps=max_steps)
    want = RC.reduce_rays(m, lv, s, e, mask, max_steps)
    RC.assert_same(got, want, (depth, stop, max_steps))
    by = {v: k for k, v in names.items()}
    assert got["flags"][by["nan"]] == RC.INVALID and got["flags"][by["far"]] == RC.INVALID
    assert got["steps"][by["nan"]] == 0 and got["steps"][by["far"]] == 0
    assert got["steps"][by["outside"]] == 0 and got["flags"][by["outside"]] == 0 and got["cls"][by["outside"]] == RC.MISSING
    assert got["steps"][by["zero"]] == 1
    assert (got["counts"].sum(1) == got["steps"]).all()
    trunc = (got["flags"] & RC.TRUNCATED) != 0
    if max_steps == 7:
        assert trunc.sum() > 50 and (got["steps"][trunc] == 7).all()
    else:
        assert trunc.sum() == 0
        if stop == "none":
            assert got["cls"][by["leaving"]] == RC.MISSING and got["leaf_depth"][by["leaving"]] == 255
            assert got["counts"][by["leaving"], RC.MISSING] > 100
    if mask:
        hit = (got["flags"] & RC.HIT) != 0
        assert hit.any() and ((mask >> got["cls"][hit].astype(np.int64)) & 1).all()
        assert (((mask >> got["cls"][~hit & (got["steps"] > 0)].astype(np.int64)) & 1) == 0).all()
    else:
        assert (got["flags"] & RC.HIT == 0).all()


def test_names_and_masks_of_the_python_binding(built):
    import la3dm_amd
    assert (la3dm_amd.MISSING, la3dm_amd.RAY_HIT, la3dm_amd.RAY_TRUNCATED, la3dm_amd.RAY_INVALID) == (3, 1, 2, 4)
    m, lv, s, e, _ = _fused_map(3)
    a = m.raycast_many(s[:50], e[:50], stop=("occupied", "missing"))
    b = m.raycast_many(s[:50], e[:50], stop=(1 << la3dm_amd.OCCUPIED) | (1 << la3dm_amd.MISSING))
    c = m.raycast_many(s[:50], e[:50])                       # default: stop at OCCUPIED, 4096 rows
    d = m.raycast_many(s[:50], e[:50], stop="occupied", max_steps=4096)
    RC.assert_same(a, b)
    RC.assert_same(c, d)


def test_arguments(built):
    import la3dm_amd
    m, lv, s, e, _ = _fused_map(3)
    for bad in (0, 2 ** 20 + 1):
        with pytest.raises(RuntimeError, match="max_steps"):
            m.raycast_many(s[:4], e[:4], max_steps=bad)
    assert m.raycast_many(s[:4], e[:4], max_steps=2 ** 20)["steps"].min() >= 1
    with pytest.raises(ValueError):
        m.raycast_many(s[:4], e[:3])
    out = m.raycast_many(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert set(out) == set(RC.FIELDS)
    assert all(out[k].shape[0] == 0 for k in RC.FIELDS) and out["p"].shape == (0, 3) and out["counts"].shape == (0, 4)
    # an empty map answers "never started" for every ray
    empty = la3dm_amd.BGKOctoMap(**YAML, device=-1)
    out = empty.raycast_many(s[:16], e[:16], stop=())
    _, a0, b0, _ = empty.search(0.0, 0.0, 0.0)
    assert (out["steps"] == 0).all() and (out["flags"] == 0).all() and (out["cls"] == RC.MISSING).all()
    assert (out["leaf_depth"] == 255).all() and (out["counts"] == 0).all() and (out["p"] == 0).all()
    assert (out["block_key"] == 0).all() and (out["node_key"] == 0).all()
    assert (out["A"] == np.float32(a0)).all() and (out["B"] == np.float32(b0)).all()
    assert empty.mirror_syncs() == 0


def test_header_declares_and_library_exports_the_new_symbols(built):
    from la3dm_amd import _lib
    for header, so, names in (("la3dm_map.h", _lib.MAP_SO, ("la3dm_map_raycast_many", "la3dm_map_mirror_syncs")),
                              ("la3dm_hip.h", _lib.HIP_SO, ("la3dm_devmap_raycast_host", "la3dm_devmap_raycast_device"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        if so == _lib.MAP_SO:
            C.CDLL(_lib.HIP_SO, mode=C.RTLD_GLOBAL)
        lib = C.CDLL(so)
        for n in names:
            assert re.search(r"\b" + n + r"\s*\(", txt), n
            assert hasattr(lib, n), n
    assert "la3dm_raycast_out" in open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
