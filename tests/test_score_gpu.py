"""score_poses on the device-resident map: distance_field's launches into working storage, then one kernel that moves
every point by every pose, resolves its voxel, gathers the cost and reduces per pose (csrc/devmap_score.h).  The yardstick is
the host form of the same class on a host-mode twin map with the same inserts (a plain loop), itself checked against the
independent yardstick of tests/helpers/score_cases.py.  Every output is an integer: every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, pcd_path

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import score_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured
N_POINTS = (1, 63, 64, 65, 255, 256, 257, 1025)      # a wave, a workgroup, one lane more, a chunk and one point
N_POSES = (1, 2, 3, 257)
SMALL = ((3, 5, 7), (1, 1, 33))
GUARD = 0x5A5A5A5A


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


def _compare(md, mh, lo, dims, points, poses, mask, radius, what):
    """device == host on sum_d2, counts and the info; returns the host answer"""
    kw = dict(obstacles=mask, radius=radius)
    gd, gh = md.score_poses(lo, dims, points, poses, **kw), mh.score_poses(lo, dims, points, poses, **kw)
    S.assert_same(gd, gh, (what, dims, mask, radius))
    R.assert_same(gd, gh, ("origin", "cell"), what)
    assert gd["block_key"] == gh["block_key"] and md.is_device_resident()
    assert (gh["counts"].sum(1) == np.asarray(points).reshape(-1, 3).shape[0]).all()
    return gh


def _small_inputs(origin, dims, res, seed=3):
    """1025 points round a small region (the centres of the region padded by two voxels, the same jittered by up to a
    voxel, drawn in a seeded order, the first the region's own first centre) and 257 poses about its middle: the identity,
    then small seeded moves"""
    import la3dm_amd
    rng = np.random.default_rng(seed)
    c = S.centres(origin, dims, res, pad=2)
    jit = (c[rng.integers(0, c.shape[0], 2048)] + rng.uniform(-1, 1, (2048, 3)).astype(np.float32) * np.float32(res)).astype(np.float32)
    pts = np.vstack([c, jit])
    pts = np.vstack([S.centres(origin, dims, res)[:1], pts[rng.permutation(pts.shape[0])]])[:1025]
    mid = np.asarray(origin, np.float64) + 0.5 * (np.array(dims) - 1) * float(res)
    moves = np.vstack([np.zeros((1, 4)), rng.uniform(-1, 1, (256, 4)) * (0.25, 0.25, 0.25, 0.3)])
    return np.ascontiguousarray(pts, np.float32), la3dm_amd.poses_xyz_yaw(mid, moves)


@pytest.mark.parametrize("depth", [3, 4])
def test_device_equals_host_bit_for_bit(built, depth):
    """GPU test 1: BGK at block_depth 3 and 4, two fused (and pruned) scans: the recipe region, cloud and pose set and the
    two small regions, three masks x radii 1, 8, 255; the host form == the independent yardstick on that map, with the
    input conditions; then a further insert (the pool grew, the table was rebuilt) and the same comparisons; no mirror
    refresh throughout"""
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    md, mh = _pair("BGKOctoMap", params, (1, 2))
    res = mh.get_resolution()
    lv = mh.leaves()
    lo = R.recipe_lo()
    pts, o = S.sensor_cloud()
    T = S.recipe_poses(o)
    S.assert_exercises_the_feature(S.input_conditions(mh, lv, lo, R.RECIPE_DIMS, pts, T))
    _, _, _, origin = R.anchor(lo, res, depth)
    slo = S.small_lo(mh, origin)
    _, _, _, so = R.anchor(slo, res, depth)
    before_syncs = md.mirror_syncs()

    def everything(tag, check_yardstick):
        pairs = np.zeros(5, np.int64)
        for rlo, dims in [(lo, R.RECIPE_DIMS)] + [(slo, d) for d in SMALL]:
            cloud = pts if dims == R.RECIPE_DIMS else np.vstack([(S.centres(so, dims, res, pad=2) - T[13, :, 3]).astype(np.float32), pts[-3:]])
            for mask in S.MASKS:
                for radius in S.RADII:
                    gh = _compare(md, mh, rlo, dims, cloud, T, mask, radius, f"bgk d{depth} {tag}")
                    pairs += gh["counts"].sum(0).astype(np.int64)
                    if check_yardstick:
                        S.assert_same(gh, S.yardstick(mh, lv, rlo, dims, cloud, T, mask, radius), ("host form vs yardstick", depth, dims, mask, radius))
        print(f"bgk d{depth} {tag}: pairs per class {pairs.tolist()}")
        assert (pairs > 0).all()
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


def _bare_map(H, ctx, scans):
    import la3dm_amd
    dm = C.c_void_p()
    assert H.la3dm_devmap_create(ctx, C.byref(dm)) == OK
    for i in scans:
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3, *INSERT, None) == OK
    return dm


def test_lanes_waves_and_neighbours(built):
    """GPU test 2: n_points in {1, 63, 64, 65, 255, 256, 257, 1025} x n_poses in {1, 2, 3, 257} at dims (3, 5, 7) and
    (1, 1, 33): the device-resident map == its host-mode twin; and on a bare la3dm_devmap with the same scans the
    device-pointer form, its outputs 4 bytes off a 16-byte boundary between guard words, with counts given and NULL, ==
    the host-pointer form == the twin, the guard words untouched"""
    import torch
    import la3dm_amd
    from la3dm_amd import _lib
    H = _lib.hip()
    md, mh = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML), (1, 2))
    res = mh.get_resolution()
    _, _, _, origin = R.anchor(R.recipe_lo(), res, 3)
    slo = S.small_lo(mh, origin)
    _, _, _, so = R.anchor(slo, res, 3)
    dm = _bare_map(H, mh.ctx(), (1, 2))
    err = lambda: H.la3dm_last_error(mh.ctx()).decode()   # noqa: E731
    dev = torch.device("cuda:0")
    inside = 0
    try:
        for dims in SMALL:
            pts, T = _small_inputs(so, dims, res)
            T12 = np.ascontiguousarray(T.reshape(-1, 12))
            d3 = np.array(dims, np.uint32)
            d_pts = torch.cat([torch.zeros(1, device=dev), torch.from_numpy(pts.reshape(-1)).to(dev)])[1:]      # 4 bytes off, too
            d_T = torch.cat([torch.zeros(1, device=dev), torch.from_numpy(T12.reshape(-1)).to(dev)])[1:]
            for n in N_POINTS:
                for P in N_POSES:
                    gh = _compare(md, mh, slo, dims, pts[:n], T[:P], 1 << R.OCCUPIED, 8, f"n {n} P {P}")
                    inside += int(gh["counts"][:, :3].sum())
                    h_sum, h_cnt = np.full(P, 7, np.uint64), np.full(5 * P, 7, np.uint32)
                    ho = _lib.ScoreOut(h_sum.ctypes.data, h_cnt.ctypes.data)
                    assert H.la3dm_devmap_score_poses_host(dm, slo.ctypes.data, d3.ctypes.data, pts.ctypes.data, n, T12.ctypes.data, P, 2, 8,
                                                           C.byref(ho), None) == OK, err()
                    assert (h_sum == gh["sum_d2"]).all() and (h_cnt.reshape(P, 5) == gh["counts"]).all(), (dims, n, P)
                    for with_counts in (True, False):
                        t_sum = torch.full((2 * P + 9,), GUARD, dtype=torch.int32, device=dev)
                        t_cnt = torch.full((5 * P + 9,), GUARD, dtype=torch.int32, device=dev)
                        torch.cuda.synchronize()
                        assert t_sum[1:].data_ptr() % 16 == 4 and t_cnt[1:].data_ptr() % 16 == 4
                        do = _lib.ScoreOut(t_sum[1:].data_ptr(), t_cnt[1:].data_ptr() if with_counts else None)
                        assert H.la3dm_devmap_score_poses_device(dm, slo.ctypes.data, d3.ctypes.data, d_pts.data_ptr(), n, d_T.data_ptr(), P, 2, 8,
                                                                 C.byref(do), None) == OK, err()
                        g_sum, g_cnt = t_sum.cpu().numpy().view(np.uint32), t_cnt.cpu().numpy().view(np.uint32)
                        assert g_sum[0] == GUARD and (g_sum[2 * P + 1:] == GUARD).all() and g_cnt[0] == GUARD and (g_cnt[5 * P + 1:] == GUARD).all()
                        got = g_sum[1:2 * P + 1].astype(np.uint64)
                        assert ((got[0::2] | (got[1::2] << np.uint64(32))) == gh["sum_d2"]).all(), (dims, n, P)
                        if with_counts:
                            assert (g_cnt[1:5 * P + 1].reshape(P, 5) == gh["counts"]).all(), (dims, n, P)
                        else:
                            assert (g_cnt == GUARD).all()
    finally:
        H.la3dm_devmap_destroy(dm)
    print(f"lanes and waves: {inside} pairs inside the regions in all")
    assert inside > 1000 and md.mirror_syncs() == 0


@pytest.mark.parametrize("variant", ["GPOctoMap", "BGKLOctoMap", "BGKLVOctoMap"])
def test_device_equals_host_on_other_variants(built, variant):
    """GPU test 3: GP, BGK-L and BGK-LV on their own configurations; on BGK-LV obstacles = bit 4 selects the UNCERTAIN
    voxels, and the host form's box says whether the region holds some"""
    import la3dm_amd
    params, insert = {"GPOctoMap": (la3dm_amd.GP_YAML, INSERT), "BGKLOctoMap": (la3dm_amd.L_YAML, (0.1, 0.3, 8.0)),
                      "BGKLVOctoMap": (la3dm_amd.LV_YAML, (0.1, 0.3, 8.0))}[variant]
    md, mh = _pair(variant, dict(params), (1, 2), insert)
    lo = R.recipe_lo()
    big = mh.box(lo, R.RECIPE_DIMS, fields=())
    pts, o = S.sensor_cloud()
    T = S.recipe_poses(o)
    for mask in S.MASKS:
        for radius in S.RADII:
            gh = _compare(md, mh, lo, R.RECIPE_DIMS, pts, T, mask, radius, variant)
    assert int(gh["counts"][13, :3].sum()) > pts.shape[0] // 2
    gh = _compare(md, mh, lo, R.RECIPE_DIMS, pts, T, 1 << R.UNCERTAIN, 8, variant + " bit 4")
    n_unc = int((big["cls"] == R.UNCERTAIN).sum())
    print(variant, "pairs on or near an UNCERTAIN voxel per pose:", gh["counts"][:, :2].sum(1).tolist(), "UNCERTAIN voxels in the region:", n_unc)
    assert (n_unc > 0) == (variant == "BGKLVOctoMap") and (int(gh["counts"][:, :2].sum()) > 0) == (n_unc > 0)
    res = mh.get_resolution()
    slo = S.small_lo(mh, big["origin"])
    spts, sT = _small_inputs(R.anchor(slo, res, int(mh.get_block_depth()))[3], (3, 5, 7), res)
    _compare(md, mh, slo, (3, 5, 7), spts, sT, 0x1E, 3, variant + " small")


def test_device_pointer_form_refusals_and_storage(built):
    """GPU test 4 on a bare la3dm_devmap: the empty map in both pointer forms against an empty host-mode map; every refusal
    in both forms with its text and nothing written; the device-pointer form == the host-pointer form; 20 further calls and
    a smaller request reserve nothing; the map stays usable after another insert"""
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
        pts, o = S.sensor_cloud()
        T = np.ascontiguousarray(S.recipe_poses(o).reshape(-1, 12))
        n, P = pts.shape[0], T.shape[0]
        lop, dp = lo.ctypes.data, dims.ctypes.data
        d_p, d_T = torch.from_numpy(pts).to(dev), torch.from_numpy(T).to(dev)
        h = dict(sum_d2=np.full(P, 9, np.uint64), counts=np.full((P, 5), 9, np.uint32))
        ho = _lib.ScoreOut(h["sum_d2"].ctypes.data, h["counts"].ctypes.data)

        def tensors(fill, with_counts=True, rows=P):
            t = dict(sum_d2=torch.full((2 * rows + 8,), fill, dtype=torch.int32, device=dev),
                     counts=torch.full((5 * rows + 8,), fill, dtype=torch.int32, device=dev))
            torch.cuda.synchronize()
            return t, _lib.ScoreOut(t["sum_d2"].data_ptr(), t["counts"].data_ptr() if with_counts else None)

        def read(t, rows=P):
            s = t["sum_d2"].cpu().numpy().view(np.uint32).astype(np.uint64)
            c = t["counts"].cpu().numpy().view(np.uint32)
            return dict(sum_d2=s[0:2 * rows:2] | (s[1:2 * rows:2] << np.uint64(32)), counts=c[:5 * rows].reshape(rows, 5)), s[2 * rows:], c[5 * rows:]

        def host_call(out=ho, **kw):
            a = dict(lo_p=lop, d_p=dp, p_p=pts.ctypes.data, n=n, t_p=T.ctypes.data, P=P, mask=0x2, radius=8, o=C.byref(out))
            a.update(kw)
            return H.la3dm_devmap_score_poses_host(dm, a["lo_p"], a["d_p"], a["p_p"], a["n"], a["t_p"], a["P"], a["mask"], a["radius"], a["o"], None)

        def dev_call(out, **kw):
            a = dict(lo_p=lop, d_p=dp, p_p=d_p.data_ptr(), n=n, t_p=d_T.data_ptr(), P=P, mask=0x2, radius=8, o=C.byref(out))
            a.update(kw)
            return H.la3dm_devmap_score_poses_device(dm, a["lo_p"], a["d_p"], a["p_p"], a["n"], a["t_p"], a["P"], a["mask"], a["radius"], a["o"], None)
        # empty map: from the definition, host and device pointers, with and without bit 3
        empty = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
        for mask in (0x2, 0xA):
            want = empty.score_poses(lo, tuple(int(v) for v in dims), pts, T, obstacles=mask, radius=8)
            assert host_call(mask=mask) == OK, err()
            S.assert_same(h, want, ("empty map, host pointers", mask))
            t, do = tensors(9)
            assert dev_call(do, mask=mask) == OK, err()
            got, tail_s, tail_c = read(t)
            S.assert_same(got, want, ("empty map, device pointers", mask))
            assert (tail_s == 9).all() and (tail_c == 9).all()
            assert int(want["counts"][:, S.HIT if mask & 8 else S.FAR].sum()) > 0 and int(want["counts"][:, S.NEAR].sum()) == 0
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 1))
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3, *INSERT, None) == OK

        def free():
            torch.cuda.synchronize()
            return torch.cuda.mem_get_info()[0]
        # refusals: LA3DM_ERR_ARG and a text that names the argument; nothing written, nothing reserved
        for k in h:
            h[k][...] = 7
        t, do = tensors(7)
        f0 = free()
        lo_nan, lo_far = np.array((np.nan, 0, 0), np.float32), np.array((-3.0e5, 0, 0), np.float32)
        d_zero, d_over = np.array((4, 0, 4), np.uint32), np.array(((1 << 28) + 1, 1, 1), np.uint32)
        for call, out in ((host_call, ho), (dev_call, do)):
            for kw, text in ((dict(mask=0), "obstacle_mask must hold"), (dict(mask=0x20), "obstacle_mask must hold"),
                             (dict(mask=0x80000002), "obstacle_mask must hold"), (dict(radius=0), "radius must lie in"),
                             (dict(radius=256), "radius must lie in"), (dict(n=(1 << 20) + 1, P=1), "LA3DM_SCORE_MAX_POINTS"),
                             (dict(n=1, P=(1 << 20) + 1), "LA3DM_SCORE_MAX_POSES"), (dict(n=1 << 20, P=(1 << 12) + 1), "LA3DM_SCORE_MAX_PAIRS"),
                             (dict(lo_p=None), "lo is NULL"), (dict(d_p=None), "dims is NULL"),
                             (dict(lo_p=lo_nan.ctypes.data), "lo must be finite"), (dict(d_p=d_zero.ctypes.data), "dims must be >= 1"),
                             (dict(lo_p=lo_far.ctypes.data), "lo: the block field leaves"),
                             (dict(d_p=d_over.ctypes.data, o=None), "LA3DM_SCORE_MAX_CELLS"),
                             (dict(n=1 << 20, P=1 << 12, t_p=None), "poses12 is NULL"),                  # at the limit: the next check answers
                             (dict(t_p=None), "poses12 is NULL"), (dict(o=None), "out is NULL"),
                             (dict(o=C.byref(_lib.ScoreOut(None, out.counts))), "out->sum_d2 must not be NULL"), (dict(p_p=None), "points3 is NULL"),
                             (dict(mask=0, radius=0, lo_p=None, o=None), "obstacle_mask must hold"),             # the order
                             (dict(radius=0, n=1 << 21, lo_p=None, o=None), "radius must lie in"),
                             (dict(n=1 << 21, P=1 << 21, lo_p=None), "LA3DM_SCORE_MAX_POINTS"), (dict(lo_p=None, t_p=None), "lo is NULL")):
                assert call(out, **kw) == ERR_ARG and text in err(), (kw, err())
            assert call(out, P=0, t_p=None, p_p=None, o=None) == OK, err()              # n_poses = 0: served, nothing written
        assert H.la3dm_devmap_score_poses_host(None, lop, dp, pts.ctypes.data, n, T.ctypes.data, P, 2, 8, C.byref(ho), None) == ERR_ARG
        assert all((h[k] == 7).all() for k in h) and all((t[k].cpu().numpy() == 7).all() for k in t)
        f1 = free()
        print(f"free device memory before / after the refusals: {f0} / {f1}")
        assert f1 >= f0, (f0, f1)
        # n_points = 0: zeros, in both forms
        t, do = tensors(7)
        assert host_call(n=0, p_p=None) == OK and dev_call(do, n=0, p_p=None) == OK, err()
        got, tail_s, tail_c = read(t)
        assert (h["sum_d2"] == 0).all() and (h["counts"] == 0).all() and (got["sum_d2"] == 0).all() and (got["counts"] == 0).all()
        assert (tail_s == 7).all() and (tail_c == 7).all()
        # device pointers == host pointers, with counts and without
        for mask, radius in ((0x2, 8), (0xE, 1), (0x1, 255)):
            assert host_call(mask=mask, radius=radius) == OK, err()
            for with_counts in (True, False):
                t, do = tensors(GUARD, with_counts)
                assert dev_call(do, mask=mask, radius=radius) == OK, err()
                got, tail_s, tail_c = read(t)
                assert (tail_s == GUARD).all() and (tail_c == GUARD).all() and (got["sum_d2"] == h["sum_d2"]).all()
                assert (got["counts"] == (h["counts"] if with_counts else GUARD)).all()
        assert int(h["counts"][13, :2].sum()) > n // 10 and (h["counts"].sum(1) == n).all()
        # storage: the calls above reserved the arenas; 20 more calls and a smaller request allocate nothing
        t, do = tensors(0)
        assert dev_call(do) == OK and host_call() == OK, err()
        f0 = free()
        small = np.array((31, 17, 23), np.uint32)
        for i in range(10):
            assert dev_call(do, mask=1 + (i & 3), radius=1 + 25 * i) == OK, err()
            assert host_call(mask=1 + (i & 3), radius=1 + 25 * i) == OK, err()
        assert dev_call(do, d_p=small.ctypes.data, n=n // 2, P=P // 2) == OK, err()
        assert host_call(d_p=small.ctypes.data, n=n // 2, P=P // 2) == OK, err()
        f1 = free()
        print(f"free device memory before / after 20 calls and a smaller request: {f0} / {f1}")
        # the figure is the whole device's: a process of another user may release memory meanwhile, so growth is what fails
        assert f1 >= f0, (f0, f1)
        # still usable: another scan, the two forms agree again and the answer has changed
        assert host_call() == OK, err()
        before = h["sum_d2"].copy()
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 2))
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3, *INSERT, None) == OK
        t, do = tensors(0)
        assert host_call() == OK and dev_call(do) == OK, err()
        got, _, _ = read(t)
        S.assert_same(got, h, "after another insert")
        assert (h["sum_d2"] != before).any()
    finally:
        H.la3dm_devmap_destroy(dm)


def test_planner_sized_call(built):
    """GPU test 5: 4 096 poses (a 16 x 16 x 16 grid of dx, dy, dyaw) x 8 192 points (scans 1 to 3 in scan 2's sensor frame)
    in one call: 8 randomly chosen poses equal the host form; a second call gives identical arrays; no mirror refresh"""
    import la3dm_amd
    md, mh = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML), (1, 2))
    lo = R.recipe_lo()
    _, o = S.sensor_cloud()
    pts = np.vstack([la3dm_amd.load_pcd(pcd_path("sim_structured", i))[0] for i in (1, 2, 3)]).astype(np.float32)
    pts = (pts[np.random.default_rng(11).permutation(pts.shape[0])[:8192]] - o).astype(np.float32)
    assert pts.shape == (8192, 3)
    oo = [float(v) for v in o]
    grid = [(oo[0] + 0.05 * (i - 8), oo[1] + 0.05 * (j - 8), oo[2], 0.01 * (k - 8)) for i in range(16) for j in range(16) for k in range(16)]
    T = la3dm_amd.poses_xyz_yaw((0.0, 0.0, 0.0), grid)
    syncs = md.mirror_syncs()
    a = md.score_poses(lo, R.RECIPE_DIMS, pts, T)
    b = md.score_poses(lo, R.RECIPE_DIMS, pts, T)
    S.assert_same(a, b, "twice")
    assert (a["counts"].sum(1) == 8192).all() and np.unique(a["sum_d2"]).size > 1000
    some = np.sort(np.random.default_rng(41).choice(4096, 8, replace=False))
    gh = mh.score_poses(lo, R.RECIPE_DIMS, pts, T[some])
    S.assert_same({k: a[k][some] for k in S.FIELDS}, gh, "8 of 4096")
    print("sum_d2 of 8 of the 4096 poses:", gh["sum_d2"].tolist(), "counts of the first:", gh["counts"][0].tolist())
    assert md.mirror_syncs() == syncs and md.is_device_resident()


def test_example_program(built):
    """GPU test 6: examples/localize.cpp (built by build()) == the Python binding on the same map and pose grid: the best
    candidate, its sum and counts and the identity's sum; no mirror refresh.  On this data the best candidate does not lie
    within one grid step of the identity (the CPU form on the emulated map puts it at dx = +0.1, dy = -0.3, dyaw = 0:
    DESIGN.md 3.18), so where it lies is printed, not asserted"""
    import la3dm_amd
    exe = os.path.join(ROOT, "examples", "localize")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "3"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    print(r.stdout)
    assert len(lines) == 3 and lines[0].startswith("best ") and lines[1].startswith("identity 364 ") and lines[2].startswith("localize 128 x 128 x 32 from ")
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    for i in (1, 2, 3):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        m.insert_pointcloud(xyz, origin, *INSERT)
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 4))
    o = np.asarray(origin, np.float32)
    lo = np.array([o[0] - np.float32(6.4), o[1] - np.float32(6.4), o[2] - np.float32(1.6)], np.float32)
    grid = [(0.1 * (i - 4), 0.1 * (j - 4), 0.0, 0.02 * (k - 4)) for i in range(9) for j in range(9) for k in range(9)]
    got = m.score_poses(lo, (128, 128, 32), xyz, la3dm_amd.poses_xyz_yaw(o, grid), radius=16)
    c = got["counts"].astype(np.int64)
    score = got["sum_d2"].astype(np.int64) + 256 * (c[:, S.FAR] + c[:, S.OUTSIDE])
    best = int(np.argmin(score))                                                   # the first of equals
    bt, it, lt = lines[0].split(), lines[1].split(), lines[2].split()
    assert int(bt[1]) == best and int(bt[9]) == int(score[best]) and int(bt[11]) == int(got["sum_d2"][best])
    assert [int(v) for v in bt[13:18]] == c[best].tolist()
    assert int(it[3]) == int(score[364]) and int(it[5]) == int(got["sum_d2"][364]) and [int(v) for v in it[7:12]] == c[364].tolist()
    tail = {lt[k]: lt[k + 1] for k in range(len(lt) - 1)}
    assert int(tail["poses"]) == 729 and int(tail["points"]) == xyz.shape[0]
    assert tail["mirror_syncs"] == "0" and tail["device_resident"] == "1" and m.mirror_syncs() == 0
    steps = [abs(best // 81 - 4), abs(best // 9 % 9 - 4), abs(best % 9 - 4)]
    print(f"best candidate {best} = (dx, dy, dyaw) {grid[best][0]:g} {grid[best][1]:g} {grid[best][3]:g}: {steps} grid steps from the identity; "
          f"score {int(score[best])} against the identity's {int(score[364])}")
    assert score[best] <= score[364]
