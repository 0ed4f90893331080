"""nearest and nearest_points on the device-resident map: distance_field's obstacle bits, then the z, y and x stages with
their argmins and the chase (csrc/devmap_nearest.h).  The yardstick is the host form of the same class on a host-mode twin
map with the same inserts, itself checked against the independent brute force of tests/helpers/nearest_cases.py.  Every
output is an integer: every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, pcd_path

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import nearest_cases as N  # noqa: E402
import region_cases as R  # noqa: E402
import score_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured
MASKS = N.MASKS[:3]
RADII = (1, 8, 255)
SMALL = ((3, 5, 7), (1, 1, 33))
GUARD = 0x5A5A5A5A
# the edges of the kernels: nz round the 32-bit words of the obstacle stream, ny nz round the 64-lane tiles, line lengths
# round the 32-row tiles, ny = 1 (a y pass over lines of length 1), lines of every axis shorter than the radius
EDGE_DIMS = ((3, 5, 1), (2, 3, 31), (2, 3, 32), (2, 3, 33), (2, 2, 65), (2, 9, 7), (2, 8, 8), (5, 5, 13), (1, 1, 9), (31, 2, 2), (32, 2, 2),
             (33, 2, 2), (2, 31, 2), (2, 32, 2), (2, 33, 2), (40, 1, 3), (1, 40, 3), (70, 36, 5))
# dm_nt_pass stages rows + halo in LDS up to radius 240 (y pass, 16-bit) and 112 (x pass, 32-bit): either side of both, and 255
EDGE_RADII = (1, 3, 112, 113, 240, 241, 255)


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


def _compare(md, mh, lo, dims, mask, radius, what):
    """device == host on index, d2 and the info; returns the host answer"""
    kw = dict(obstacles=mask, radius=radius)
    gd, gh = md.nearest(lo, dims, **kw), mh.nearest(lo, dims, **kw)
    N.assert_same(gd, gh, (what, dims, mask, radius))
    R.assert_same(gd, gh, ("origin", "cell"), what)
    assert gd["block_key"] == gh["block_key"] and md.is_device_resident()
    return gh


def _compare_points(md, mh, lo, dims, points, pose, mask, radius, what):
    kw = dict(obstacles=mask, radius=radius)
    gd, gh = md.nearest_points(lo, dims, points, pose, **kw), mh.nearest_points(lo, dims, points, pose, **kw)
    N.assert_same(gd, gh, (what, dims, mask, radius), N.POINT_FIELDS)
    R.assert_same(gd, gh, ("origin", "cell"), what)
    return gh


@pytest.mark.parametrize("depth", [3, 4])
def test_device_equals_host_exactly(built, depth):
    """GPU test 1: BGK at block_depth 3 and 4, two fused scans: the recipe region and the small regions, three masks x radii 1,
    8, 255, nearest and nearest_points (the recipe cloud with a pose and, in the map frame, without); the host form == the
    brute force on the small regions; then a further insert and the same comparisons; no mirror refresh throughout"""
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    md, mh = _pair("BGKOctoMap", params, (1, 2))
    res = mh.get_resolution()
    lv = mh.leaves()
    lo = R.recipe_lo()
    pts, o = S.sensor_cloud()
    T = S.recipe_poses(o)
    world = np.vstack([(pts[:-3] + o).astype(np.float32), pts[-3:]])
    _, _, _, origin = R.anchor(lo, res, depth)
    slo = N.small_lo(mh, origin)
    before_syncs = md.mirror_syncs()

    def everything(tag, check_yardstick):
        found = classes = 0
        for rlo, dims in [(lo, R.RECIPE_DIMS)] + [(slo, d) for d in SMALL]:
            cls = R.yardstick(mh, lv, rlo, dims)["cls"] if check_yardstick and dims != R.RECIPE_DIMS else None
            for mask in MASKS:
                for radius in RADII:
                    gh = _compare(md, mh, rlo, dims, mask, radius, f"bgk d{depth} {tag}")
                    found += int((gh["index"] != N.NONE).sum())
                    if cls is not None:
                        N.assert_same(gh, N.yardstick(cls, mask, radius), ("host form vs yardstick", depth, dims, mask, radius))
                    for cloud, pose in ((pts, T[13]), (world, None), (pts, T[5])):
                        gp = _compare_points(md, mh, rlo, dims, cloud, pose, mask, radius, f"bgk d{depth} {tag} points")
                        classes = classes + np.bincount(gp["cls"], minlength=5)
        print(f"bgk d{depth} {tag}: {found} voxels with an obstacle within the radius, points per class {classes.tolist()}")
        assert found > 0 and (classes > 0).all()
    everything("two scans", True)
    assert md.mirror_syncs() == before_syncs
    before = md.block_count()          # (refreshes the mirror; the queries do not depend on it either way)
    xyz, origin5 = la3dm_amd.load_pcd(pcd_path("sim_structured", 5))
    for m in (md, mh):
        m.insert_pointcloud(xyz, origin5, *INSERT)
    assert md.block_count() > before
    syncs = md.mirror_syncs()
    everything("after a further insert", False)
    assert md.mirror_syncs() == syncs


@pytest.mark.parametrize("variant", ["GPOctoMap", "BGKLOctoMap", "BGKLVOctoMap"])
def test_device_equals_host_on_other_variants(built, variant):
    """GPU test 2: GP, BGK-L and BGK-LV on their own configurations; on BGK-LV obstacles = bit 4 selects the UNCERTAIN
    voxels, and the host form's box says whether the region holds some"""
    import la3dm_amd
    params, insert = {"GPOctoMap": (la3dm_amd.GP_YAML, INSERT), "BGKLOctoMap": (la3dm_amd.L_YAML, (0.1, 0.3, 8.0)),
                      "BGKLVOctoMap": (la3dm_amd.LV_YAML, (0.1, 0.3, 8.0))}[variant]
    md, mh = _pair(variant, dict(params), (1, 2), insert)
    lo = R.recipe_lo()
    big = mh.box(lo, R.RECIPE_DIMS, fields=())
    pts, o = S.sensor_cloud()
    T = S.recipe_poses(o)
    for mask, radius in ((MASKS[0], 8), (MASKS[1], 1), (MASKS[2], 255)):
        gh = _compare(md, mh, lo, R.RECIPE_DIMS, mask, radius, variant)
        _compare_points(md, mh, lo, R.RECIPE_DIMS, pts, T[13], mask, radius, variant)
    gh = _compare(md, mh, lo, R.RECIPE_DIMS, 1 << R.UNCERTAIN, 8, variant + " bit 4")
    n_unc = int((big["cls"] == R.UNCERTAIN).sum())
    near = int((gh["index"] != N.NONE).sum())
    print(variant, "voxels within 8 of an UNCERTAIN voxel:", near, "UNCERTAIN voxels in the region:", n_unc)
    assert (n_unc > 0) == (variant == "BGKLVOctoMap") and (near > 0) == (n_unc > 0)
    slo = N.small_lo(mh, big["origin"])
    _compare(md, mh, slo, (3, 5, 7), 0x1E, 3, variant + " small")


def test_the_edges_of_the_kernels(built):
    """GPU test 3: EDGE_DIMS x EDGE_RADII x two masks, each placed in the thick of the recipe region: the device-resident map
    == its host-mode twin; the regions of at most 260 voxels also == the brute force"""
    import la3dm_amd
    md, mh = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML), (1, 2))
    res = mh.get_resolution()
    lv = mh.leaves()
    big = R.yardstick(mh, lv, R.recipe_lo(), R.RECIPE_DIMS)
    origin = big["origin"]
    found = tied = planes = 0
    for dims in EDGE_DIMS:
        small = dims[0] * dims[1] * dims[2] <= 260
        # a small region with two axes longer than 1 goes where the yardstick counts ties to break (nearest_cases.place)
        rlo = N.small_lo(mh, origin, offset=N.place(big["cls"], dims) if small else (5, 22, 14))
        cls = R.yardstick(mh, lv, rlo, dims)["cls"] if small else None
        planes += small and sum(n > 1 for n in dims) >= 2 and all(n <= b for n, b in zip(dims, R.RECIPE_DIMS))
        for mask in (MASKS[0], MASKS[2]):
            if small and mask == MASKS[0]:
                tied += N.conditions(cls, mask, 8)["tied"]
            for radius in EDGE_RADII:
                gh = _compare(md, mh, rlo, dims, mask, radius, "edges")
                found += int((gh["index"] != N.NONE).sum())
                if small:
                    N.assert_same(gh, N.yardstick(cls, mask, radius), ("host form vs yardstick", dims, mask, radius))
    print(f"edges: {found} voxels with an obstacle within the radius in all, {tied} tied voxels in the small regions")
    assert found > 10000 and tied >= planes > 0 and md.mirror_syncs() == 0


def _bare_map(H, ctx, scans):
    import la3dm_amd
    dm = C.c_void_p()
    assert H.la3dm_devmap_create(ctx, C.byref(dm)) == OK
    for i in scans:
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3, *INSERT, None) == OK
    return dm


def test_nearest_points_lanes_and_forms(built):
    """GPU test 4: 1, 63, 64, 65, 257 and 1025 points, with and without a pose: the device-resident map == its twin; on a bare
    la3dm_devmap the host-pointer form == the twin, and the device-pointer form, its inputs and outputs 4 bytes (cls: 1 byte)
    off a 16-byte boundary between guard words, with each output left out in turn, == the twin, the guard words untouched"""
    import torch
    import la3dm_amd
    from la3dm_amd import _lib
    H = _lib.hip()
    md, mh = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML), (1, 2))
    res = mh.get_resolution()
    _, _, _, origin = R.anchor(R.recipe_lo(), res, 3)
    dims = (3, 5, 7)
    slo = N.small_lo(mh, origin, offset=(20, 22, 14))
    _, _, _, so = R.anchor(slo, res, 3)
    dm = _bare_map(H, mh.ctx(), (1, 2))
    err = lambda: H.la3dm_last_error(mh.ctx()).decode()   # noqa: E731
    dev = torch.device("cuda:0")
    pts = N.jittered_cloud(so, dims, res, n=1025)
    pose = la3dm_amd.poses_xyz_yaw(so, [(0.05, -0.1, 0.1, 0.2)])[0]
    d3 = np.array(dims, np.uint32)
    inside = 0
    try:
        d_pts = torch.cat([torch.zeros(1, device=dev), torch.from_numpy(pts.reshape(-1)).to(dev)])[1:]
        d_T = torch.cat([torch.zeros(1, device=dev), torch.from_numpy(pose.reshape(-1)).to(dev)])[1:]
        for n in (1, 63, 64, 65, 257, 1025):
            for T, dT in ((None, None), (pose, d_T.data_ptr())):
                gh = _compare_points(md, mh, slo, dims, pts[:n], T, 0xE, 3, f"n {n}")
                inside += int((gh["voxel"] != N.NONE).sum())
                h = {k: np.full(n, 7, gh[k].dtype) for k in N.POINT_FIELDS}
                ho = _lib.NearestPointsOut(*[h[k].ctypes.data for k in N.POINT_FIELDS])
                tp = None if T is None else np.ascontiguousarray(T.reshape(-1)).ctypes.data
                assert H.la3dm_devmap_nearest_points_host(dm, slo.ctypes.data, d3.ctypes.data, pts.ctypes.data, n, tp, 0xE, 3, C.byref(ho), None) == OK, err()
                N.assert_same(h, gh, ("host pointers", n), N.POINT_FIELDS)
                for left_out in (None,) + N.POINT_FIELDS:
                    t = {k: torch.full((n + 9,), GUARD, dtype=torch.int32, device=dev) for k in N.POINT_FIELDS[1:]}
                    t["cls"] = torch.full((n + 9,), 0x5A, dtype=torch.uint8, device=dev)
                    torch.cuda.synchronize()
                    assert all(t[k][1:].data_ptr() % 16 == 4 for k in N.POINT_FIELDS[1:]) and t["cls"][1:].data_ptr() % 16 == 1
                    do = _lib.NearestPointsOut(*[None if k == left_out else t[k][1:].data_ptr() for k in N.POINT_FIELDS])
                    assert H.la3dm_devmap_nearest_points_device(dm, slo.ctypes.data, d3.ctypes.data, d_pts.data_ptr(), n, dT, 0xE, 3,
                                                                C.byref(do), None) == OK, err()
                    for k in N.POINT_FIELDS:
                        g = t[k].cpu().numpy()
                        g = g if k == "cls" else g.view(np.uint32)
                        guard = 0x5A if k == "cls" else GUARD
                        assert g[0] == guard and (g[n + 1:] == guard).all(), (k, n)
                        assert (g[1:n + 1] == (guard if k == left_out else gh[k])).all(), (k, n, left_out)
    finally:
        H.la3dm_devmap_destroy(dm)
    print(f"lanes: {inside} points inside the region in all")
    assert inside > 200 and md.mirror_syncs() == 0


def test_bare_devmap_forms_refusals_and_storage(built):
    """GPU test 5 on a bare la3dm_devmap: the empty map in both pointer forms against an empty host-mode map; every refusal in
    both forms with its text and nothing written or reserved; the device-pointer form on torch tensors == the host-pointer
    form; 20 further calls and a smaller request reserve nothing; the map stays usable after another insert"""
    import torch
    import la3dm_amd
    from la3dm_amd import _lib
    H = _lib.hip()
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)   # (lends its context)
    ctx = m.ctx()
    dm = _bare_map(H, ctx, ())
    err = lambda: H.la3dm_last_error(ctx).decode()   # noqa: E731
    dev = torch.device("cuda:0")
    try:
        lo = R.recipe_lo()
        dims = np.array((77, 67, 39), np.uint32)
        n = int(dims.prod())
        pts, o = S.sensor_cloud()
        pts = np.ascontiguousarray(np.vstack([(pts[:-3] + o).astype(np.float32), pts[-3:]]))
        P = pts.shape[0]
        lop, dp = lo.ctypes.data, dims.ctypes.data
        d_p = torch.from_numpy(pts).to(dev)
        h = dict(index=np.full(n, 9, np.uint32), d2=np.full(n, 9, np.uint32))
        ho = _lib.NearestOut(h["index"].ctypes.data, h["d2"].ctypes.data)
        hp = {k: np.full(P, 9, np.uint8 if k == "cls" else np.uint32) for k in N.POINT_FIELDS}
        hpo = _lib.NearestPointsOut(*[hp[k].ctypes.data for k in N.POINT_FIELDS])

        def tensors(fill, with_index=True):
            t = dict(index=torch.full((n + 8,), fill, dtype=torch.int32, device=dev), d2=torch.full((n + 8,), fill, dtype=torch.int32, device=dev))
            torch.cuda.synchronize()
            return t, _lib.NearestOut(t["index"].data_ptr() if with_index else None, t["d2"].data_ptr())

        def read(t):
            g = {k: t[k].cpu().numpy().view(np.uint32) for k in t}
            return {k: g[k][:n] for k in g}, {k: g[k][n:] for k in g}

        def ptensors(fill):
            t = {k: torch.full((P + 8,), fill, dtype=torch.uint8 if k == "cls" else torch.int32, device=dev) for k in N.POINT_FIELDS}
            torch.cuda.synchronize()
            return t, _lib.NearestPointsOut(*[t[k].data_ptr() for k in N.POINT_FIELDS])

        def call(out, device=False, **kw):
            a = dict(lo_p=lop, d_p=dp, mask=0x2, radius=8, o=C.byref(out))
            a.update(kw)
            f = H.la3dm_devmap_nearest_device if device else H.la3dm_devmap_nearest_host
            return f(dm, a["lo_p"], a["d_p"], a["mask"], a["radius"], a["o"], None)

        def pcall(out, device=False, **kw):
            a = dict(lo_p=lop, d_p=dp, p_p=d_p.data_ptr() if device else pts.ctypes.data, n=P, mask=0x2, radius=8, o=C.byref(out))
            a.update(kw)
            f = H.la3dm_devmap_nearest_points_device if device else H.la3dm_devmap_nearest_points_host
            return f(dm, a["lo_p"], a["d_p"], a["p_p"], a["n"], None, a["mask"], a["radius"], a["o"], None)
        # empty map: from the definition, host and device pointers, with and without bit 3
        empty = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
        tdims = tuple(int(v) for v in dims)
        for mask in (0x2, 0xA):
            want = {k: a.reshape(-1) for k, a in empty.nearest(lo, tdims, obstacles=mask, radius=8).items() if k in N.FIELDS}
            assert call(ho, mask=mask) == OK, err()
            N.assert_same(h, want, ("empty map, host pointers", mask))
            t, do = tensors(9)
            assert call(do, True, mask=mask) == OK, err()
            got, tail = read(t)
            N.assert_same(got, want, ("empty map, device pointers", mask))
            assert all((tail[k] == 9).all() for k in tail)
            assert (want["index"] == (np.arange(n) if mask & 8 else N.NONE)).all()
            wantp = empty.nearest_points(lo, tdims, pts, obstacles=mask, radius=8)
            tp, dpo = ptensors(9)
            assert pcall(hpo, mask=mask) == OK and pcall(dpo, True, mask=mask) == OK, err()
            N.assert_same(hp, wantp, ("empty map, points, host pointers", mask), N.POINT_FIELDS)
            for k in N.POINT_FIELDS:
                g = tp[k].cpu().numpy()
                g = g if k == "cls" else g.view(np.uint32)
                assert (g[:P] == wantp[k]).all() and (g[P:] == 9).all(), (k, mask)
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 1))
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3, *INSERT, None) == OK

        def free():
            torch.cuda.synchronize()
            return torch.cuda.mem_get_info()[0]
        # refusals: LA3DM_ERR_ARG and a text that names the argument; nothing written, nothing reserved
        for d in (h, hp):
            for k in d:
                d[k][...] = 7
        t, do = tensors(7)
        tp, dpo = ptensors(7)
        f0 = free()
        lo_nan, lo_far = np.array((np.nan, 0, 0), np.float32), np.array((-3.0e5, 0, 0), np.float32)
        d_zero, d_over = np.array((4, 0, 4), np.uint32), np.array(((1 << 28) + 1, 1, 1), np.uint32)
        shared = ((dict(mask=0), "obstacle_mask must hold"), (dict(mask=0x20), "obstacle_mask must hold"), (dict(mask=0x80000002), "obstacle_mask must hold"),
                  (dict(radius=0), "radius must lie in [1, LA3DM_NEAREST_MAX_RADIUS (255)]"), (dict(radius=256), "radius must lie in"),
                  (dict(lo_p=None), "lo is NULL"), (dict(d_p=None), "dims is NULL"), (dict(lo_p=lo_nan.ctypes.data), "lo must be finite"),
                  (dict(d_p=d_zero.ctypes.data), "dims must be >= 1"), (dict(lo_p=lo_far.ctypes.data), "lo: the block field leaves"),
                  (dict(d_p=d_over.ctypes.data, o=None), "LA3DM_DF_MAX_CELLS"), (dict(o=None), "out is NULL"),
                  (dict(mask=0, radius=0, lo_p=None, o=None), "obstacle_mask must hold"),             # the order
                  (dict(radius=0, lo_p=None, o=None), "radius must lie in"), (dict(lo_p=None, d_p=d_over.ctypes.data, o=None), "lo is NULL"))
        for device, out, pout in ((False, ho, hpo), (True, do, dpo)):
            for kw, text in shared + ((dict(o=C.byref(_lib.NearestOut(None, None))), "out: index or d2 must not be NULL"),):
                assert call(out, device, **kw) == ERR_ARG and text in err() and "la3dm_devmap_nearest_" in err(), (kw, err())
            for kw, text in shared + ((dict(n=(1 << 20) + 1), "LA3DM_SCORE_MAX_POINTS"), (dict(p_p=None), "points3 is NULL"),
                                      (dict(o=C.byref(_lib.NearestPointsOut(None, None, None, None))), "out: cls, voxel, index or d2 must not be NULL"),
                                      (dict(n=1 << 21, lo_p=None, p_p=None), "LA3DM_SCORE_MAX_POINTS"), (dict(p_p=None, o=None), "points3 is NULL")):
                assert pcall(pout, device, **kw) == ERR_ARG and text in err() and "la3dm_devmap_nearest_points_" in err(), (kw, err())
            assert pcall(pout, device, n=0, p_p=None, o=None) == OK, err()                # n_points = 0: served, nothing written
        assert H.la3dm_devmap_nearest_host(None, lop, dp, 2, 8, C.byref(ho), None) == ERR_ARG
        assert all((d[k] == 7).all() for d in (h, hp) for k in d) and all((d[k].cpu().numpy() == 7).all() for d in (t, tp) for k in d)
        f1 = free()
        print(f"free device memory before / after the refusals: {f0} / {f1}")
        assert f1 >= f0, (f0, f1)
        # device pointers == host pointers, with index and without
        for mask, radius in ((0x2, 8), (0xE, 1), (0x1, 255)):
            assert call(ho, mask=mask, radius=radius) == OK, err()
            for with_index in (True, False):
                t, do = tensors(GUARD, with_index)
                assert call(do, True, mask=mask, radius=radius) == OK, err()
                got, tail = read(t)
                assert all((tail[k] == GUARD).all() for k in tail) and (got["d2"] == h["d2"]).all()
                assert (got["index"] == (h["index"] if with_index else GUARD)).all()
            tp, dpo = ptensors(0x5A)
            assert pcall(hpo, mask=mask, radius=radius) == OK and pcall(dpo, True, mask=mask, radius=radius) == OK, err()
            for k in N.POINT_FIELDS:
                g = tp[k].cpu().numpy()
                g = g if k == "cls" else g.view(np.uint32)
                assert (g[:P] == hp[k]).all() and (g[P:] == 0x5A).all(), (k, mask)
        assert int((h["index"] != N.NONE).sum()) > n // 10
        # storage: the calls above reserved the arenas; 20 more calls and a smaller request allocate nothing
        t, do = tensors(0)
        tp, dpo = ptensors(0)
        assert call(do, True) == OK and call(ho) == OK and pcall(dpo, True) == OK and pcall(hpo) == OK, err()
        f0 = free()
        small = np.array((31, 17, 23), np.uint32)
        for i in range(5):
            kw = dict(mask=1 + (i & 3), radius=1 + 60 * i)
            assert call(do, True, **kw) == OK and call(ho, **kw) == OK and pcall(dpo, True, **kw) == OK and pcall(hpo, **kw) == OK, err()
        assert call(do, True, d_p=small.ctypes.data) == OK and call(ho, d_p=small.ctypes.data) == OK, err()
        assert pcall(dpo, True, d_p=small.ctypes.data, n=P // 2) == OK and pcall(hpo, d_p=small.ctypes.data, n=P // 2) == OK, err()
        f1 = free()
        print(f"free device memory before / after 20 calls and a smaller request: {f0} / {f1}")
        # the figure is the whole device's: a process of another user may release memory meanwhile, so growth is what fails
        assert f1 >= f0, (f0, f1)
        # still usable: another scan, the two forms agree again and the answer has changed
        assert call(ho) == OK, err()
        before = h["index"].copy()
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 2))
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3, *INSERT, None) == OK
        t, do = tensors(0)
        assert call(ho) == OK and call(do, True) == OK, err()
        got, _ = read(t)
        N.assert_same(got, h, "after another insert")
        assert (h["index"] != before).any()
    finally:
        H.la3dm_devmap_destroy(dm)


def test_example_program(built):
    """GPU test 6: examples/align.cpp (built by build()) runs; every `iter` line's sum of d2 and counts equal the Python
    binding's nearest_points on the same map with the pose the line prints; no mirror refresh.  What the steps do to the sum
    is printed, not asserted: the data decide it"""
    import la3dm_amd
    exe = os.path.join(ROOT, "examples", "align")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "3"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    print(r.stdout)
    assert len(lines) == 9 and lines[0].startswith("start ") and lines[-1].startswith("align 128 x 128 x 32 from ")
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    for i in (1, 2, 3):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        m.insert_pointcloud(xyz, origin, *INSERT)
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 4))
    o = np.asarray(origin, np.float32)
    lo = np.array([o[0] - np.float32(6.4), o[1] - np.float32(6.4), o[2] - np.float32(1.6)], np.float32)
    sums = []
    for k, line in enumerate(lines[1:-1]):
        tok = line.split()
        assert tok[0] == "iter" and int(tok[1]) == k and tok[14] == "rms_xy_m" and tok[16] == "pose" and len(tok) == 29, line
        pose = np.array([float.fromhex(v) for v in tok[17:]], np.float32)
        got = m.nearest_points(lo, (128, 128, 32), xyz, pose, radius=16)
        near = got["cls"] <= N.NEAR
        assert int(tok[3]) == int(got["d2"][near].astype(np.int64).sum()), line
        assert [int(tok[i]) for i in (5, 7, 9, 11, 13)] == np.bincount(got["cls"], minlength=5).tolist(), line
        sums.append(int(tok[3]))
    tail = lines[-1].split()
    tail = {tail[k]: tail[k + 1] for k in range(len(tail) - 1)}
    assert int(tail["start_sum"]) == sums[0] and int(tail["end_sum"]) == sums[-1] and int(tail["least_sum"]) == min(sums)
    assert int(tail["rises"]) == sum(b > a for a, b in zip(sums, sums[1:])) and int(tail["points"]) == xyz.shape[0]
    assert tail["mirror_syncs"] == "0" and tail["device_resident"] == "1" and m.mirror_syncs() == 0
    print(f"sum of d2 per step: {sums}")
