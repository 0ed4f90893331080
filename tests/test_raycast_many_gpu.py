"""raycast_many on the device-resident map: one HIP launch walks every ray on the device pool (csrc/devmap_raycast.h).
The yardstick is the host form of the same class (a host-mode map, the loop over its own RayCaster), itself checked
against an independent reduction of the iterator's rows and, at block_depth 4, against the oracle's walk.  Every
comparison is exact: integers by ==, floats by their bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, pcd_path

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import raycast_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured


def _pair(cls_name, params, scans, insert=INSERT):
    """the same inserts into a device-resident map and a host-mode one"""
    import la3dm_amd
    cls = getattr(la3dm_amd, cls_name)
    md = cls(**params, device=0)
    mh = cls(**params, device=0).set_device_resident(False)
    assert md.is_device_resident() and not mh.is_device_resident()
    for i in scans:
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        md.insert_pointcloud(xyz, origin, *insert)
        mh.insert_pointcloud(xyz, origin, *insert)
    return md, mh


def _compare_all(md, mh, s, e, what):
    for stop, mask in RC.STOPS.items():
        for max_steps in (4096, 7):
            RC.assert_same(md.raycast_many(s, e, stop=mask, max_steps=max_steps),
                           mh.raycast_many(s, e, stop=mask, max_steps=max_steps), (what, stop, max_steps))
    assert md.is_device_resident()


@pytest.mark.parametrize("depth", [3, 4])
def test_device_equals_host_bit_for_bit(built, depth):
    """items 1 and 3: BGK at block_depth 3 and 4, two fused (and pruned) scans; the rays are shown to exercise hits,
    non-hits, missing blocks and hits on collapsed regions from the HOST form; then a further insert (the pool grew,
    the table was rebuilt) and the same comparison"""
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    md, mh = _pair("BGKOctoMap", params, (1, 2))
    lv = mh.leaves()
    s, e, names = RC.all_rays(lv)
    occ = mh.raycast_many(s, e, stop=("occupied",), max_steps=4096)
    full = mh.raycast_many(s, e, stop=(), max_steps=4096)
    RC.assert_rays_exercise_the_feature(RC.category_counts(occ, full, depth), depth)
    by = {v: k for k, v in names.items()}
    assert occ["flags"][by["nan"]] == RC.INVALID and occ["flags"][by["far"]] == RC.INVALID
    assert occ["steps"][by["outside"]] == 0 and occ["steps"][by["zero"]] == 1
    assert full["cls"][by["leaving"]] == RC.MISSING and full["counts"][by["leaving"], RC.MISSING] > 100
    _compare_all(md, mh, s, e, f"bgk d{depth}")
    before = md.block_count()          # (refreshes the mirror; raycast_many does not depend on it either way)
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 5))
    for m in (md, mh):
        m.insert_pointcloud(xyz, origin, *INSERT)
    _compare_all(md, mh, s, e, f"bgk d{depth} after a further insert")
    assert md.block_count() > before


@pytest.mark.parametrize("variant", ["GPOctoMap", "BGKLOctoMap"])
def test_device_equals_host_on_other_variants(built, variant):
    """the query serves every map family unchanged: GP (A, B hold m_ivar, ivar) and BGK-L on their own configurations"""
    import la3dm_amd
    params, insert = {"GPOctoMap": (la3dm_amd.GP_YAML, INSERT), "BGKLOctoMap": (la3dm_amd.L_YAML, (0.1, 0.3, 8.0))}[variant]
    md, mh = _pair(variant, dict(params), (1, 2), insert)
    lv = mh.leaves()
    s, e, _ = RC.all_rays(lv)
    occ = mh.raycast_many(s, e)
    print(variant, "hits", int((occ["flags"] & RC.HIT != 0).sum()), "of", s.shape[0], "mean rows", float(occ["steps"].mean()))
    assert 0 < int((occ["flags"] & RC.HIT != 0).sum()) < s.shape[0]
    _compare_all(md, mh, s, e, variant)


def test_host_form_equals_the_iterator_and_the_oracle(built):
    """item 2, block_depth 4: the test's own reduction of mh.raycast rows == mh.raycast_many; and for the recipe's rays
    the oracle's walk == mh.raycast on p, keys and valid"""
    import la3dm_amd
    from oracle import oracle as O
    params = dict(la3dm_amd.BGK_YAML, block_depth=4)
    mh = la3dm_amd.BGKOctoMap(**params, device=0).set_device_resident(False)
    o = O.OracleMap(**params)
    for i in (1, 2):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        mh.insert_pointcloud(xyz, origin, *INSERT)
        o.insert_pointcloud(xyz, origin, *INSERT)
    lv = mh.leaves()
    s, e, _ = RC.all_rays(lv)
    for stop, mask in RC.STOPS.items():
        for max_steps in (4096, 7):
            RC.assert_same(mh.raycast_many(s, e, stop=mask, max_steps=max_steps),
                           RC.reduce_rays(mh, lv, s, e, mask, max_steps), (stop, max_steps))
    rows = 0
    for s3, e3 in zip(s[:RC.N_RECIPE], e[:RC.N_RECIPE]):      # the oracle's walk: with the recipe's rays only
        a, b = mh.raycast(s3, e3), o.raycast(s3, e3)
        assert a["p"].shape == b["p"].shape and a["p"].shape[0] >= 1
        for k in ("p", "block_key", "node_key", "valid"):
            assert (a[k] == b[k]).all(), k
        rows += a["p"].shape[0]
    assert rows > 20000


def test_no_mirror_refresh(built):
    """item 4: the query is answered from the pool — the map stays device resident and nothing is downloaded"""
    import la3dm_amd
    md = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    assert md.mirror_syncs() == 0
    rng = np.random.default_rng(3)
    for i in (1, 2):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        md.insert_pointcloud(xyz, origin, *INSERT)
        before = md.mirror_syncs()
        e = (origin + rng.uniform(-6, 6, (500, 3))).astype(np.float32)
        s = np.broadcast_to(np.asarray(origin, np.float32), e.shape)
        out = md.raycast_many(s, e)
        assert (out["steps"] > 0).all()
        assert md.is_device_resident() and md.mirror_syncs() == before
        rows = md.raycast(s[0], e[0])                      # the iterator pays the refresh
        assert md.mirror_syncs() == before + 1 and rows["p"].shape[0] >= out["steps"][0]
        md.raycast(s[1], e[1])
        assert md.mirror_syncs() == before + 1             # ... once per insert


def test_example_program(built):
    """item 5: examples/raycast.cpp (built by build()) == the Python binding on the same map and rays"""
    import la3dm_amd
    exe = os.path.join(ROOT, "examples", "raycast")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "3"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("ray (1, 1, 0.3) -> (6, 7, 8): steps ") and lines[1].startswith("fan 4096 rays from ")
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    for i in (1, 2, 3):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        m.insert_pointcloud(xyz, origin, *INSERT)
    i = np.arange(4096)
    a, b, f = i & 63, (i >> 6) & 15, i >> 10
    u = ((a.astype(np.float32) - np.float32(31.5)) * np.float32(0.25)).astype(np.float32)
    w = ((b.astype(np.float32) - np.float32(7.5)) * np.float32(0.25)).astype(np.float32)
    dx = np.where(f == 0, np.float32(8), np.where(f == 1, np.float32(-8), u)).astype(np.float32)
    dy = np.where(f == 2, np.float32(8), np.where(f == 3, np.float32(-8), u)).astype(np.float32)
    o = np.asarray(origin, np.float32)
    e = (o[None, :] + np.stack([dx, dy, w], 1)).astype(np.float32)
    out = m.raycast_many(np.broadcast_to(o, e.shape), e)
    tok = lines[1].split()
    got = {tok[k]: tok[k + 1] for k in range(len(tok) - 1)}
    assert int(got["hits"]) == int((out["flags"] & RC.HIT != 0).sum()) and int(got["hits"]) > 500
    assert int(got["total_steps"]) == int(out["steps"].sum())
    assert int(got["unknown_or_missing_rows"]) == int(out["counts"][:, 2:].sum())
    assert got["mirror_syncs"] == "0" and got["device_resident"] == "1"
    one = m.raycast_many([[1, 1, 0.3]], [[6, 7, 8]])
    tok = lines[0].split()
    assert int(tok[tok.index("steps") + 1]) == int(one["steps"][0]) and int(tok[tok.index("cls") + 1]) == int(one["cls"][0])


def _out_struct(n, skip=()):
    from la3dm_amd import _lib
    arr = dict(steps=np.zeros(n, np.uint32), flags=np.zeros(n, np.uint8), p=np.zeros((n, 3), np.float32),
               block_key=np.zeros(n, np.int64), node_key=np.zeros(n, np.int32), cls=np.zeros(n, np.uint8),
               leaf_depth=np.zeros(n, np.uint8), A=np.zeros(n, np.float32), B=np.zeros(n, np.float32),
               counts=np.zeros((n, 4), np.uint32))
    return arr, _lib.RaycastOut(*[None if k in skip else arr[k].ctypes.data for k, _ in _lib.RaycastOut._fields_])


def test_abi_errors_and_the_device_pointer_form(built):
    """item 6: bad arguments answer LA3DM_ERR_ARG with a text, n = 0 and an empty map are fine; optional outputs may be
    NULL; la3dm_devmap_raycast_device (rays and results in HBM) gives the same answers as the host-pointer form"""
    import torch
    import la3dm_amd
    from la3dm_amd import _lib
    H = _lib.hip()
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)   # (lends its context)
    ctx = m.ctx()
    dm = C.c_void_p()
    assert H.la3dm_devmap_create(ctx, C.byref(dm)) == OK
    try:
        n = 64
        rng = np.random.default_rng(2)
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 1))
        rays = np.concatenate([np.broadcast_to(np.asarray(origin, np.float32), (n, 3)),
                               (origin + rng.uniform(-6, 6, (n, 3))).astype(np.float32)], 1).astype(np.float32)
        rays = np.ascontiguousarray(rays)
        arr, out = _out_struct(n)
        # empty map: every ray "never started", nothing launched
        arr["steps"][:] = 9
        arr["cls"][:] = 9
        assert H.la3dm_devmap_raycast_host(dm, rays.ctypes.data, n, 2, 4096, C.byref(out)) == OK
        assert (arr["steps"] == 0).all() and (arr["flags"] == 0).all() and (arr["cls"] == RC.MISSING).all()
        assert (arr["leaf_depth"] == 255).all() and (arr["A"] == np.float32(0.001)).all() and (arr["B"] == np.float32(0.001)).all()
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3,
                                                     0.1, 0.5, 8.0, None) == OK
        for bad in (0, 2 ** 20 + 1):
            assert H.la3dm_devmap_raycast_host(dm, rays.ctypes.data, n, 2, bad, C.byref(out)) == ERR_ARG
            assert "max_steps" in H.la3dm_last_error(ctx).decode()
            assert H.la3dm_devmap_raycast_device(dm, rays.ctypes.data, n, 2, bad, C.byref(out)) == ERR_ARG
        assert H.la3dm_devmap_raycast_host(dm, None, n, 2, 4096, C.byref(out)) == ERR_ARG and "rays6" in H.la3dm_last_error(ctx).decode()
        assert H.la3dm_devmap_raycast_host(dm, rays.ctypes.data, n, 2, 4096, None) == ERR_ARG
        _, no_steps = _out_struct(n, skip=("steps",))
        assert H.la3dm_devmap_raycast_host(dm, rays.ctypes.data, n, 2, 4096, C.byref(no_steps)) == ERR_ARG
        assert "steps" in H.la3dm_last_error(ctx).decode()
        _, no_flags = _out_struct(n, skip=("flags",))
        assert H.la3dm_devmap_raycast_device(dm, rays.ctypes.data, n, 2, 4096, C.byref(no_flags)) == ERR_ARG
        assert H.la3dm_devmap_raycast_host(None, rays.ctypes.data, n, 2, 4096, C.byref(out)) == ERR_ARG
        assert H.la3dm_devmap_raycast_host(dm, None, 0, 2, 4096, None) == OK          # n = 0
        assert H.la3dm_devmap_raycast_device(dm, None, 0, 2, 4096, None) == OK
        # the map is still usable; all outputs vs only the mandatory ones
        assert H.la3dm_devmap_raycast_host(dm, rays.ctypes.data, n, 2, 4096, C.byref(out)) == OK
        assert (arr["steps"] > 0).all() and (arr["flags"] & RC.HIT != 0).any()
        few, only = _out_struct(n, skip=("p", "block_key", "node_key", "cls", "leaf_depth", "A", "B", "counts"))
        assert H.la3dm_devmap_raycast_host(dm, rays.ctypes.data, n, 2, 4096, C.byref(only)) == OK
        assert (few["steps"] == arr["steps"]).all() and (few["flags"] == arr["flags"]).all() and (few["p"] == 0).all()
        # device pointers
        dev = torch.device("cuda:0")
        t_rays = torch.from_numpy(rays).to(dev)
        t = dict(steps=torch.zeros(n, dtype=torch.int32, device=dev), flags=torch.zeros(n, dtype=torch.uint8, device=dev),
                 p=torch.zeros(n, 3, dtype=torch.float32, device=dev), block_key=torch.zeros(n, dtype=torch.int64, device=dev),
                 node_key=torch.zeros(n, dtype=torch.int32, device=dev), cls=torch.zeros(n, dtype=torch.uint8, device=dev),
                 leaf_depth=torch.zeros(n, dtype=torch.uint8, device=dev), A=torch.zeros(n, dtype=torch.float32, device=dev),
                 B=torch.zeros(n, dtype=torch.float32, device=dev), counts=torch.zeros(n, 4, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        d_out = _lib.RaycastOut(*[t[k].data_ptr() for k, _ in _lib.RaycastOut._fields_])
        assert H.la3dm_devmap_raycast_device(dm, t_rays.data_ptr(), n, 2, 4096, C.byref(d_out)) == OK
        for k in RC.FIELDS:
            got = t[k].cpu().numpy()
            assert (got.view(arr[k].dtype).reshape(arr[k].shape).view(np.uint8) == arr[k].view(np.uint8)).all(), k
    finally:
        H.la3dm_devmap_destroy(dm)


def test_a_million_rays(built):
    """item 7: 2^20 rays from the sensor origin to random points of a 10 m sphere on the depth-3 map: one launch; a
    random sample of 2 000 of them agrees with the host form"""
    import la3dm_amd
    md, mh = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML), (1, 2))
    _, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 2))
    rng = np.random.default_rng(9)
    n = 1 << 20
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.asarray(origin, np.float32)
    e = (o + 10.0 * d).astype(np.float32)
    s = np.ascontiguousarray(np.broadcast_to(o, e.shape))
    out = md.raycast_many(s, e)
    assert md.is_device_resident() and md.mirror_syncs() == 0
    assert (out["steps"] > 0).all() and (out["flags"] & RC.TRUNCATED == 0).all()
    hits = int((out["flags"] & RC.HIT != 0).sum())
    print(f"2^20 rays: {hits} hits, {int(out['steps'].sum())} rows, longest {int(out['steps'].max())}")
    assert n // 20 < hits < n
    pick = rng.choice(n, 2000, replace=False)
    want = mh.raycast_many(s[pick], e[pick])
    RC.assert_same({k: np.ascontiguousarray(v[pick]) for k, v in out.items()}, want, "sample of 2^20")
