"""reach on the device-resident map: a pass stream from the device pool, seeds, one launch per level of the wave and a
gather at the targets (csrc/devmap_reach.h).  The yardstick is the host form of the same class (a host-mode map, a queue
BFS over box's classes), itself checked against an independent numpy wave over a walk of the leaf list
(tests/helpers/reach_cases.py) and against closed forms.  The answer is integer and unique: every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, pcd_path

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import frontier_cases as F  # noqa: E402
import reach_cases as Q  # noqa: E402

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured
DIMS = R.RECIPE_DIMS
SEED = Q.flat(Q.SEED, DIMS)
_PAIRS = {}


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


def _bgk_pair():
    """BGK at depth 3 after scans 1 and 2, shared by the tests that only read it"""
    import la3dm_amd
    if "bgk" not in _PAIRS:
        _PAIRS["bgk"] = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML, block_depth=3), (1, 2))
    return _PAIRS["bgk"]


def _compare(md, mh, lo, dims, seeds, what, targets=None, **kw):
    """device == host on steps, target_steps, the stats and the info; returns the host answer"""
    gd, gh = md.reach(lo, dims, seeds, targets=targets, **kw), mh.reach(lo, dims, seeds, targets=targets, **kw)
    Q.assert_same(gd, gh, (what, dims, kw))
    R.assert_same(gd, gh, ("origin", "cell"), what)
    assert gd["block_key"] == gh["block_key"]
    assert md.is_device_resident()
    return gh


@pytest.mark.parametrize("depth", [3, 4])
def test_device_equals_host_bit_for_bit(built, depth):
    """GPU test 1: BGK at block_depth 3 and 4, two fused (and pruned) scans: the recipe region from the sensor's voxel, the
    four pass / clearance pairs at connectivity 6 and 26, with the frontier's list as targets; the host form == the
    yardstick on that map, with the input conditions; then a third insert (the pool grew, the table was rebuilt) and the
    same comparison; no mirror refresh throughout"""
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    md, mh = _pair("BGKOctoMap", params, (1, 2))
    lo = R.recipe_lo()
    y = R.yardstick(mh, mh.leaves(), lo, DIMS)
    assert y["cls"][Q.SEED] == R.FREE
    Q.assert_exercises_the_feature(Q.input_conditions(y["cls"], SEED, la3dm_amd.REACH_BATCH))
    before_syncs = md.mirror_syncs()
    targets = md.frontier(lo, DIMS)["index"]
    assert targets.size > 1000
    for pass_mask, clearance in Q.PAIRS:
        for c in (6, 26):
            kw = dict(passable=pass_mask, obstacles=Q.OCC_M, clearance=clearance, connectivity=c)
            gh = _compare(md, mh, lo, DIMS, [SEED], f"bgk d{depth}", targets=targets, **kw)
            want = Q.yardstick(y["cls"], [SEED], pass_mask, Q.OCC_M, clearance, c, targets=targets)
            Q.assert_same(gh, want, ("host form vs yardstick", depth, kw))
            print(f"depth {depth} pass {pass_mask:#x} clearance {clearance} connectivity {c}: reached {want['n_reached']} "
                  f"levels {want['levels']} goals reached {int((want['target_steps'] != Q.NONE).sum())} of {targets.size}")
    only = md.reach(lo, DIMS, [SEED], clearance=2, targets=targets, fields=())
    assert "steps" not in only and (only["target_steps"] == Q.yardstick(y["cls"], [SEED], Q.FREE_M, Q.OCC_M, 2, 6, targets=targets)["target_steps"]).all()
    assert md.mirror_syncs() == before_syncs
    before = mh.block_count()          # (counted on the host-mode map: the device-resident one keeps its mirror untouched)
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 5))
    for m in (md, mh):
        m.insert_pointcloud(xyz, origin, *INSERT)
    assert mh.block_count() > before
    for pass_mask, clearance in Q.PAIRS:
        for c in (6, 26):
            _compare(md, mh, lo, DIMS, [SEED], f"bgk d{depth} after a further insert", targets=targets, passable=pass_mask,
                     obstacles=Q.OCC_M, clearance=clearance, connectivity=c)
    assert md.mirror_syncs() == before_syncs


def test_word_and_row_boundaries(built):
    """GPU test 2: single voxels and lines, nz = 1, the word and wave boundaries of the voxel count, in the thick of the
    map: pass 0xF is an open box with the closed form; pass FREE is seeded at the first FREE voxel of the host form's box"""
    md, mh = _bgk_pair()
    res = np.float32(mh.get_resolution())
    origin = mh.box(R.recipe_lo(), (1, 1, 1), fields=())["origin"]
    free_seen = 0
    syncs = md.mirror_syncs()
    for shape in F.SHAPES + F.WORD_SHAPES:
        lo = (origin + np.array(F.SHAPE_OFFSET, np.float32) * res).astype(np.float32)
        cls = mh.box(lo, shape, fields=())["cls"]
        centre = tuple(n // 2 for n in shape)
        free = np.flatnonzero(cls.reshape(-1) == R.FREE)
        for c in Q.CONNECTIVITIES:
            gh = _compare(md, mh, lo, shape, [Q.flat(centre, shape)], "open box", passable=0xF, connectivity=c)
            assert (gh["steps"] == Q.closed_form(shape, centre, c)).all(), (shape, c)
            assert gh["n_reached"] == int(np.prod(shape))
            seeds = free[:1]
            gh = _compare(md, mh, lo, shape, seeds, "free", targets=np.arange(int(np.prod(shape)) + 2, dtype=np.uint32), connectivity=c)
            Q.assert_same(gh, Q.yardstick(cls, seeds, Q.FREE_M, connectivity=c), ("free vs the wave over the host box", shape, c),
                          fields=("steps",) + Q.STATS)
            free_seen += gh["n_reached"]
    print(f"small shapes: {free_seen} FREE voxels reached in all")
    assert free_seen > 100
    assert md.mirror_syncs() == syncs


def test_batch_boundaries(built):
    """GPU test 3: lines 100 m from the scans of a non-empty map (every voxel MISSING, pass = MISSING: the probes and all
    kernels run) whose length puts the end of the wave before, on and after the end of a batch of level launches;
    max_steps round a batch boundary; 3000 levels; steps and levels are the closed form; the empty map answers the same, and with a
    clearance as the host-mode empty map does"""
    import la3dm_amd
    md, mh = _bgk_pair()
    empty = la3dm_amd.BGKOctoMap(**dict(la3dm_amd.BGK_YAML, block_depth=3), device=0)
    assert md.leaves()["A"].size > 0 and empty.is_device_resident()
    B = la3dm_amd.REACH_BATCH
    lo = Q.far_lo(md, R.recipe_lo())
    assert (md.box(lo, (3, 3, 3 * B), fields=())["cls"] == R.MISSING).all()
    syncs = md.mirror_syncs()
    for m in (md, empty):
        for length in (2, B, B + 1, B + 2, 2 * B + 1, 2 * B + 2):
            for axis in range(3):
                dims = [1, 1, 1]
                dims[axis] = length
                for seed in (0, length - 1):
                    for c in (6, 26):
                        g = m.reach(lo, dims, [seed], passable=Q.MISS_M, connectivity=c)
                        assert (g["steps"].reshape(-1) == np.abs(np.arange(length) - seed)).all(), (dims, seed, c)
                        assert g["levels"] == length - 1 and g["n_reached"] == length and g["n_seeded"] == 1, (dims, seed, c, g["levels"])
        dims = (1, 1, 3 * B)
        for k in (B - 1, B, B + 1):
            g = m.reach(lo, dims, [0], passable=Q.MISS_M, max_steps=k)
            want = np.arange(3 * B)
            assert (g["steps"].reshape(-1) == np.where(want <= k, want, Q.NONE)).all(), k
            assert g["levels"] == k and g["n_reached"] == k + 1, (k, g["levels"])
        for dims in F.LONG_SHAPES:
            for c in (6, 26):
                seed = tuple(n - 1 for n in dims)
                g = m.reach(lo, dims, [Q.flat(seed, dims)], passable=Q.MISS_M, connectivity=c)
                want = Q.closed_form(dims, seed, c)
                assert (g["steps"] == want).all() and g["levels"] == int(want.max()) >= 2999 and g["n_reached"] == want.size, (dims, c)
    # a clearance on the empty map (the obstacle field is the same word everywhere, no transform runs), two bricks along x
    # with a ragged edge: OCCUPIED as the obstacle leaves the box open, MISSING closes it (tests/test_reach_cpu.py's closed
    # forms); the device-resident map == the host-mode one
    host_empty = la3dm_amd.BGKOctoMap(**dict(la3dm_amd.BGK_YAML, block_depth=3), device=-1)
    dims, n = (9, 5, 3), 9 * 5 * 3
    for obstacles in (Q.OCC_M, Q.MISS_M):
        gh = _compare(empty, host_empty, R.recipe_lo(), dims, [0], "empty map", targets=np.array([0, n - 1, n + 1], np.uint32),
                      passable=Q.MISS_M, obstacles=obstacles, clearance=2)
        if obstacles == Q.MISS_M:
            assert (gh["steps"] == Q.NONE).all() and gh["n_seeded"] == gh["n_reached"] == gh["levels"] == 0
        else:
            want = Q.closed_form(dims, (0, 0, 0), 6)
            assert (gh["steps"] == want).all() and gh["n_seeded"] == 1 and gh["n_reached"] == n and gh["levels"] == int(want.max())
    assert md.mirror_syncs() == syncs and empty.mirror_syncs() == 0
    # the host-mode map agrees where the line crosses a batch boundary
    _compare(md, mh, lo, (1, B + 2, 1), [0], "far line", passable=Q.MISS_M)


@pytest.mark.parametrize("variant", ["GPOctoMap", "BGKLOctoMap", "BGKLVOctoMap"])
def test_device_equals_host_on_other_variants(built, variant):
    """GPU test 4: GP, BGK-L and BGK-LV on their own configurations; the host form == the numpy wave over its own box; on
    BGK-LV the UNCERTAIN bit as passable changes the answer, and the wave says so.  The classes the wave reads here come from
    the host-mode map's box(), not from the leaf-list walk of region_cases.yardstick, which is written for BGK's leaf
    fields (the choice of test_frontier_gpu.py); device == host is compared exactly all the same"""
    import la3dm_amd
    params, insert = {"GPOctoMap": (la3dm_amd.GP_YAML, INSERT), "BGKLOctoMap": (la3dm_amd.L_YAML, (0.1, 0.3, 8.0)),
                      "BGKLVOctoMap": (la3dm_amd.LV_YAML, (0.1, 0.3, 8.0))}[variant]
    md, mh = _pair(variant, dict(params), (1, 2), insert)
    lo = R.recipe_lo()
    cls = mh.box(lo, DIMS, fields=())["cls"]
    free = np.flatnonzero(cls.reshape(-1) == R.FREE)
    seeds = [SEED] if cls[Q.SEED] == R.FREE else free[free.size // 2:free.size // 2 + 1]
    for pass_mask, clearance in Q.PAIRS:
        for c in (6, 26):
            kw = dict(passable=pass_mask, obstacles=Q.OCC_M, clearance=clearance, connectivity=c)
            gh = _compare(md, mh, lo, DIMS, seeds, variant, **kw)
            Q.assert_same(gh, Q.yardstick(cls, seeds, pass_mask, Q.OCC_M, clearance, c), (variant, "host form vs the wave over its own box", kw))
    _compare(md, mh, lo, (7, 9, 11), [0, 5, 100], variant + " small", passable=0x1F, connectivity=18)
    unc = 1 << R.UNCERTAIN
    plain = Q.yardstick(cls, free, Q.FREE_M, connectivity=26)
    wider = Q.yardstick(cls, free, Q.FREE_M | unc, connectivity=26)
    print(variant, "voxels reached from every FREE voxel without / with UNCERTAIN passable:", plain["n_reached"], wider["n_reached"])
    assert (wider["n_reached"] > plain["n_reached"]) == (variant == "BGKLVOctoMap")
    gh = _compare(md, mh, lo, DIMS, free, variant + " bit 4", passable=Q.FREE_M | unc, connectivity=26)
    Q.assert_same(gh, wider, variant + " bit 4")


def test_device_pointer_form_refusals_and_storage(built):
    """GPU test 5 on a bare la3dm_devmap: refusals in both pointer forms with their text and nothing written; the
    device-pointer form == the host-pointer form with steps on a pointer 4 bytes off a 16-byte boundary; arrays not asked
    for are untouched; free device memory is the same before and after 50 calls and a following smaller request"""
    import torch
    import la3dm_amd
    from la3dm_amd import _lib
    H = _lib.hip()
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)   # (lends its context)
    ctx = m.ctx()
    dm = C.c_void_p()
    assert H.la3dm_devmap_create(ctx, C.byref(dm)) == OK
    err = lambda: H.la3dm_last_error(ctx).decode()   # noqa: E731
    dev = torch.device("cuda:0")
    try:
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 1))
        lo = (np.asarray(origin, np.float32) + np.asarray(R.RECIPE_OFFSET, np.float32)).astype(np.float32)
        dims = np.array((77, 67, 39), np.uint32)
        n = int(dims.prod())
        lop, dp = lo.ctypes.data, dims.ctypes.data
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3,
                                                     0.1, 0.5, 8.0, None) == OK
        cls = np.zeros(n, np.uint8)
        assert H.la3dm_devmap_box_host(dm, lop, dp, C.byref(_lib.BoxOut(cls.ctypes.data, None, None, None)), None) == OK, err()
        free = np.flatnonzero(cls == R.FREE)
        assert free.size > 1000
        at = int(Q.flat(Q.SEED, dims))                  # the sensor's voxel where it is FREE, else a FREE voxel in the middle of the list
        seeds = np.array([at if cls[at] == R.FREE else free[free.size // 2], n + 3], np.uint32)
        targets = np.concatenate([np.arange(0, n, 97), [n, 0xFFFFFFFF]]).astype(np.uint32)
        nt = targets.size
        h = dict(steps=np.full(n, 7, np.uint32), target_steps=np.full(nt, 7, np.uint32))
        ho = _lib.ReachOut(h["steps"].ctypes.data, h["target_steps"].ctypes.data)
        d_seeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
        d_targets = torch.from_numpy(targets.view(np.int32)).to(dev)

        def tensors(fill, offset=0):
            t = dict(steps=torch.full((n + 4,), fill, dtype=torch.int32, device=dev), target_steps=torch.full((nt + 4,), fill, dtype=torch.int32, device=dev))
            torch.cuda.synchronize()
            return t, _lib.ReachOut(t["steps"][offset:].data_ptr(), t["target_steps"][offset:].data_ptr())
        t, do = tensors(7)
        stats = _lib.ReachStats(77, 77, 77)
        over = np.array(((1 << 10) - 2, (1 << 10) - 2, (1 << 8) - 1), np.uint32)      # padded: above 2^28
        for fn, out, sp, tp in ((H.la3dm_devmap_reach_host, ho, seeds.ctypes.data, targets.ctypes.data),
                                (H.la3dm_devmap_reach_device, do, d_seeds.data_ptr(), d_targets.data_ptr())):
            call = lambda lo_p=lop, d_p=dp, s=sp, ns=2, pm=1, om=2, cl=2, c=6, ms=1 << 16, tg=tp, k=nt, o=C.byref(out): \
                fn(dm, lo_p, d_p, s, ns, pm, om, cl, c, ms, tg, k, o, C.byref(stats), None)   # noqa: E731
            assert fn(None, lop, dp, sp, 2, 1, 2, 2, 6, 1 << 16, tp, nt, C.byref(out), C.byref(stats), None) == ERR_ARG
            for mask in (0, 0x20, 0x80000002):
                assert call(pm=mask) == ERR_ARG and "pass_mask must hold" in err()
            for mask in (0, 0x20, 0x80000002):
                assert call(om=mask) == ERR_ARG and "obstacle_mask must hold" in err()
            assert call(cl=1025) == ERR_ARG and "clearance must not exceed" in err()
            for c in (0, 7, 27, 0xFFFFFFFF):
                assert call(c=c) == ERR_ARG and "connectivity must be 6, 18 or 26" in err()
            for k in (0, (1 << 16) + 1):
                assert call(ms=k) == ERR_ARG and "max_steps must lie in" in err()
            assert call(ns=(1 << 20) + 1) == ERR_ARG and "LA3DM_REACH_MAX_SEEDS" in err()
            assert call(k=(1 << 28) + 1) == ERR_ARG and "n_targets" in err()
            assert call(s=None) == ERR_ARG and "seeds is NULL" in err()
            assert call(tg=None) == ERR_ARG and "targets is NULL" in err()
            assert call(o=None) == ERR_ARG and "out is NULL" in err()
            assert call(o=C.byref(_lib.ReachOut(None, None)), k=0) == ERR_ARG and "must not be NULL" in err()
            assert call(k=0) == ERR_ARG and "target_steps is set with n_targets = 0" in err()
            assert call(o=C.byref(_lib.ReachOut(out.steps, None))) == ERR_ARG and "target_steps must not be NULL with n_targets > 0" in err()
            assert call(pm=0, lo_p=None) == ERR_ARG and "pass_mask" in err()             # reach's checks come first
            assert call(lo_p=None) == ERR_ARG and "lo is NULL" in err()
            assert call(d_p=None) == ERR_ARG and "dims is NULL" in err()
            bad = np.array((np.nan, 0, 0), np.float32)
            assert call(lo_p=bad.ctypes.data) == ERR_ARG and "lo must be finite" in err()
            d0 = dims.copy()
            d0[1] = 0
            assert call(d_p=d0.ctypes.data) == ERR_ARG and "dims must be >= 1" in err()
            assert call(d_p=over.ctypes.data) == ERR_ARG and "LA3DM_REACH_MAX_CELLS" in err(), err()
            low = np.array((-209715.5, 0, 0), np.float32)
            assert call(lo_p=low.ctypes.data) == ERR_ARG and "padded by one voxel" in err(), err()
        assert all((h[k] == 7).all() for k in h) and all((t[k].cpu().numpy() == 7).all() for k in t)
        assert (stats.n_seeded, stats.n_reached, stats.levels) == (77, 77, 77)
        # the device-pointer form == the host-pointer form; steps 4 bytes off a 16-byte boundary; what was not asked for is untouched
        for (pass_mask, clearance), c in zip(Q.PAIRS, (6, 26, 18, 6)):
            hs = _lib.ReachStats()
            info = _lib.RegionInfo()
            assert H.la3dm_devmap_reach_host(dm, lop, dp, seeds.ctypes.data, 2, pass_mask, 2, clearance, c, 1 << 16, targets.ctypes.data, nt,
                                             C.byref(ho), C.byref(hs), C.byref(info)) == OK, err()
            fin = h["steps"] != Q.NONE
            assert hs.n_reached == int(fin.sum()) and hs.levels == (int(h["steps"][fin].max()) if fin.any() else 0)
            assert clearance > 0 or (hs.n_seeded == 1 and hs.n_reached > 100), (pass_mask, clearance, c, hs.n_seeded, hs.n_reached)
            assert (h["target_steps"][:-2] == h["steps"][targets[:-2]]).all() and (h["target_steps"][-2:] == Q.NONE).all()
            for offset in (0, 1):
                for fields in (("steps", "target_steps"), ("steps",), ("target_steps",)):
                    t, _ = tensors(0x5A5A5A5A)
                    assert (t["steps"][offset:].data_ptr() & 15) == 4 * offset
                    do = _lib.ReachOut(*[t[k][offset:].data_ptr() if k in fields else None for k in ("steps", "target_steps")])
                    k = nt if "target_steps" in fields else 0
                    ds, info2 = _lib.ReachStats(), _lib.RegionInfo()
                    assert H.la3dm_devmap_reach_device(dm, lop, dp, d_seeds.data_ptr(), 2, pass_mask, 2, clearance, c, 1 << 16,
                                                       d_targets.data_ptr() if k else None, k, C.byref(do), C.byref(ds), C.byref(info2)) == OK, err()
                    assert (ds.n_seeded, ds.n_reached, ds.levels) == (hs.n_seeded, hs.n_reached, hs.levels)
                    assert list(info2.origin) == list(info.origin) and info2.block_key == info.block_key and list(info2.cell) == list(info.cell)
                    g = {key: t[key].cpu().numpy().view(np.uint32) for key in t}
                    for key, size in (("steps", n), ("target_steps", nt)):
                        if key in fields:
                            assert (g[key][:offset] == 0x5A5A5A5A).all() and (g[key][offset + size:] == 0x5A5A5A5A).all(), (key, offset)
                            assert (g[key][offset:offset + size] == h[key]).all(), (key, offset, fields, pass_mask, clearance, c)
                        else:
                            assert (g[key] == 0x5A5A5A5A).all(), (key, fields)
        # storage: the first call at a size reserves, 50 more do not; a smaller region afterwards allocates nothing
        t, do = tensors(0)
        small = np.array((31, 17, 23), np.uint32)
        dev_call = lambda d_p, cl, c: H.la3dm_devmap_reach_device(dm, lop, d_p, d_seeds.data_ptr(), 2, 1, 2, cl, c, 1 << 16, d_targets.data_ptr(), nt,   # noqa: E731
                                                                  C.byref(do), None, None)
        host_call = lambda d_p, cl, c: H.la3dm_devmap_reach_host(dm, lop, d_p, seeds.ctypes.data, 2, 1, 2, cl, c, 1 << 16, targets.ctypes.data, nt,   # noqa: E731
                                                                 C.byref(ho), None, None)

        def free():
            torch.cuda.synchronize()
            return torch.cuda.mem_get_info()[0]
        assert dev_call(dp, 2, 26) == OK and host_call(dp, 2, 26) == OK, err()
        f0 = free()
        for i in range(25):
            assert dev_call(dp, i % 3, F.CONNECTIVITIES[i % 3]) == OK and host_call(dp, i % 3, F.CONNECTIVITIES[i % 3]) == OK, err()
        assert dev_call(small.ctypes.data, 2, 6) == OK and host_call(small.ctypes.data, 2, 6) == OK, err()
        f1 = free()
        print(f"free device memory before / after 50 calls and a smaller region: {f0} / {f1}")
        # the figure is the whole device's: a process of another user may release memory meanwhile, so growth is what fails
        assert f1 >= f0, (f0, f1)
    finally:
        H.la3dm_devmap_destroy(dm)


def test_example_program(built):
    """GPU test 6: examples/reachable_goals.cpp (built by build()) == the Python binding on the same map: the summary line
    and the goals"""
    import la3dm_amd
    exe = os.path.join(ROOT, "examples", "reachable_goals")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "3"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    print(r.stdout)
    assert all(ln.startswith("goal ") for ln in lines[:-1]) and lines[-1].startswith("reach 128 x 128 x 16 from ")
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    for i in (1, 2, 3):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        m.insert_pointcloud(xyz, origin, *INSERT)
    before = m.mirror_syncs()
    o = np.asarray(origin, np.float32)
    lo = np.array([o[0] - np.float32(6.4), o[1] - np.float32(6.4), o[2] - np.float32(0.8)], np.float32)
    dims = (128, 128, 16)
    res = np.float32(m.get_resolution())
    fr = m.frontier(lo, dims)
    s = [int(min(max(np.floor((o[a] - fr["origin"][a]) / res + np.float32(0.5)), 0), dims[a] - 1)) for a in range(3)]
    g = m.reach(lo, dims, [Q.flat(s, dims)], clearance=3, targets=fr["index"], fields=())
    assert m.is_device_resident() and m.mirror_syncs() == before
    ok = g["target_steps"] != Q.NONE
    tok = lines[-1].split()
    got = {tok[k]: tok[k + 1] for k in range(len(tok) - 1)}
    assert int(got["found"]) == fr["n"] > 0 and int(got["reachable"]) == int(ok.sum()) and int(got["levels"]) == g["levels"]
    assert got["mirror_syncs"] == "0" and got["device_resident"] == "1"
    assert len(lines) == min(5, int(ok.sum())) + 1
    order = np.argsort(g["target_steps"][ok], kind="stable")[:5]
    ijk = np.stack(np.unravel_index(fr["index"][ok][order], dims), 1).astype(np.float32)
    p = fr["origin"] + ijk * res
    for ln, q, st in zip(lines[:-1], p, g["target_steps"][ok][order]):
        tk = ln.split()
        assert np.allclose([float(v) for v in tk[1:4]], q, atol=1e-4) and int(tk[5]) == int(st), (ln, q, st)
