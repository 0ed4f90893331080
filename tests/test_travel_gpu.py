"""travel on the device-resident map: entry words from the device pool, seeds, rounds of brick relaxations in LDS, the
dense cost with parents and a gather at the targets (csrc/devmap_travel.h).  The yardstick is the host form of the same
class (a host-mode map, Dijkstra over box's classes), itself checked against independent Jacobi sweeps over a walk of the
leaf list (tests/helpers/travel_cases.py) and against closed forms.  The answer is integer and unique: every comparison is
exact.  What is expected of the diagnostics (rounds, capped brick runs) comes from the helper's numpy model of the scheme."""
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
import travel_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured
DIMS = R.RECIPE_DIMS
SEED = T.flat(T.SEED, DIMS)
FIELDS = ("cost", "parent")
DIAG = ("rounds", "brick_runs", "capped")
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


def _bgk_pair(depth=3):
    """BGK after scans 1 and 2, shared by the tests that only read it; with the yardstick of the recipe region"""
    import la3dm_amd
    if depth not in _PAIRS:
        md, mh = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML, block_depth=depth), (1, 2))
        _PAIRS[depth] = (md, mh, R.yardstick(mh, mh.leaves(), R.recipe_lo(), DIMS))
    return _PAIRS[depth]


def _compare(md, mh, lo, dims, seeds, what, targets=None, **kw):
    """device == host on cost, parent, target_cost, the contract's stats and the info; returns both answers"""
    gd = md.travel(lo, dims, seeds, targets=targets, fields=FIELDS, **kw)
    gh = mh.travel(lo, dims, seeds, targets=targets, fields=FIELDS, **kw)
    T.assert_same(gd, gh, (what, dims, kw))
    R.assert_same(gd, gh, ("origin", "cell"), what)
    assert gd["block_key"] == gh["block_key"]
    assert md.is_device_resident()
    return gd, gh


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("depth", [3, 4])
def test_device_equals_host_bit_for_bit(built, depth, connectivity):
    """GPU test 1: BGK at block_depth 3 and 4, two fused (and pruned) scans: the recipe region from the sensor's voxel,
    weights 1/1/1, 10/14/17 and 5/7/9 without and with clearance 1, soft radius 4 and penalty 40, the frontier's list as
    targets; the host form == the yardstick on that map, with the input conditions first; the device form's rounds, brick
    runs and capped runs are those of the helper's model on the two queries it counts — more rounds than one batch, and the
    inner cap hit where the model says so; no mirror refresh.  (The third insert: test_device_equals_host_after_a_further_insert.)"""
    md, mh, y = _bgk_pair(depth)
    lo = R.recipe_lo()
    cond = T.input_conditions(y["cls"], SEED, key=("gpu", depth))
    T.assert_exercises_the_feature(cond)
    before_syncs = md.mirror_syncs()
    targets = md.frontier(lo, DIMS)["index"]
    assert targets.size > 1000
    for weights in T.WEIGHTS:
        for kw in (T.PLAIN, T.SOFT):
            q = dict(connectivity=connectivity, move_cost=weights, **kw)
            gd, gh = _compare(md, mh, lo, DIMS, [SEED], f"bgk d{depth}", targets=targets, **q)
            want = T.yardstick(y["cls"], [SEED], targets=targets, key=("gpu", depth), **q)
            T.assert_same(gh, want, ("host form vs yardstick", depth, q))
            print(f"depth {depth} {q}: reached {want['n_reached']} max_cost {want['max_cost']} goals reached "
                  f"{int((want['target_cost'] != T.NONE).sum())} of {targets.size}; device rounds {gd['rounds']} brick_runs {gd['brick_runs']} capped {gd['capped']}")
            assert gd["rounds"] >= 1 and gd["brick_runs"] >= gd["rounds"] and gd["capped"] <= gd["brick_runs"]
            model = {(6, (1, 1, 1), 0): "unit", (26, (10, 14, 17), 4): "soft"}.get((connectivity, weights, kw["soft_radius"]))
            if model:
                m = cond["model"][model]
                print(f"  the model: {m}")
                assert gd["rounds"] > T.BATCH and (gd["capped"] > 0) == (m["capped"] > 0), (gd["rounds"], gd["capped"], m)
                assert tuple(gd[k] for k in DIAG) == tuple(m[k] for k in DIAG), ([gd[k] for k in DIAG], m)
    only = md.travel(lo, DIMS, [SEED], targets=targets, fields=(), **T.SOFT)
    assert "cost" not in only and "parent" not in only
    assert (only["target_cost"] == T.yardstick(y["cls"], [SEED], targets=targets, key=("gpu", depth), **T.SOFT)["target_cost"]).all()
    assert md.mirror_syncs() == before_syncs


@pytest.mark.parametrize("depth", [3, 4])
def test_device_equals_host_after_a_further_insert(built, depth):
    """GPU test 1, second half: a third insert (the pool grew, the table was rebuilt) and the same comparison at both
    connectivities; the unit-weight query runs more rounds than one batch and hits the cap; no mirror refresh"""
    import la3dm_amd
    md, mh = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML, block_depth=depth), (1, 2))
    lo = R.recipe_lo()
    targets = md.frontier(lo, DIMS)["index"]
    first = md.travel(lo, DIMS, [SEED], **T.SOFT)
    before_syncs = md.mirror_syncs()
    before = mh.block_count()          # (counted on the host-mode map: the device-resident one keeps its mirror untouched)
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 5))
    for m in (md, mh):
        m.insert_pointcloud(xyz, origin, *INSERT)
    assert mh.block_count() > before
    for c in (6, 26):
        for weights in T.WEIGHTS:
            for kw in (T.PLAIN, T.SOFT):
                gd, _ = _compare(md, mh, lo, DIMS, [SEED], f"bgk d{depth} after a further insert", targets=targets, connectivity=c, move_cost=weights, **kw)
                if c == 26 and weights == (10, 14, 17) and kw is T.SOFT:
                    assert (gd["cost"] != first["cost"]).any()          # the map changed, and the answer with it
    assert md.mirror_syncs() == before_syncs


def test_brick_boundaries(built):
    """GPU test 2: open boxes in the thick of the map (pass 0xF), seeded at a corner and at the centre: every axis length in
    {1, 7, 8, 9, 15, 16, 17} along every axis, mixed boxes, and the cubes 8, 9 and 17 at connectivity 26 with weights
    10/14/3, under which the least path runs through voxel corners and so through the corners of bricks; then
    frontier_cases.SHAPES with pass FREE from the first FREE voxel.  Device == host form == yardstick."""
    md, mh, _ = _bgk_pair()
    res = np.float32(mh.get_resolution())
    origin = mh.box(R.recipe_lo(), (1, 1, 1), fields=())["origin"]
    lo = (origin + np.array(F.SHAPE_OFFSET, np.float32) * res).astype(np.float32)
    syncs = md.mirror_syncs()
    lengths = (1, 7, 8, 9, 15, 16, 17)
    shapes = [tuple(n if a == axis else 1 for a in range(3)) for axis in range(3) for n in lengths]
    shapes += [(7, 9, 17), (16, 8, 15), (17, 1, 9), (9, 16, 1), (8, 8, 8), (9, 9, 9), (17, 17, 17)]
    for shape in shapes:
        open_cls = np.zeros(shape, np.uint8)
        cube = shape[0] == shape[1] == shape[2] > 1
        for seed in ((0, 0, 0), tuple(n // 2 for n in shape)):
            for c, weights in ((26, (10, 14, 3)), (26, (10, 14, 17))) if cube else ((6, (10, 14, 17)), (18, (5, 7, 9)), (26, (10, 14, 3))):
                s = [T.flat(seed, shape)]
                _, gh = _compare(md, mh, lo, shape, s, "open box", passable=0xF, connectivity=c, move_cost=weights)
                T.assert_same(gh, T.yardstick(open_cls, s, 0xF, connectivity=c, move_cost=weights), ("open box vs yardstick", shape, seed, c, weights))
                assert gh["n_reached"] == int(np.prod(shape))
    free_seen = 0
    for shape in F.SHAPES:
        cls = mh.box(lo, shape, fields=())["cls"]
        seeds = np.flatnonzero(cls.reshape(-1) == R.FREE)[:1]
        for c in T.CONNECTIVITIES:
            kw = dict(connectivity=c, soft_radius=2, penalty=25)
            _, gh = _compare(md, mh, lo, shape, seeds, "free", targets=np.arange(int(np.prod(shape)) + 2, dtype=np.uint32), **kw)
            T.assert_same(gh, T.yardstick(cls, seeds, **kw), ("free vs the yardstick over the host box", shape, c), fields=FIELDS + T.STATS)
            free_seen += gh["n_reached"]
    print(f"small shapes: {free_seen} FREE voxels reached in all")
    assert free_seen > 100
    assert md.mirror_syncs() == syncs


def test_batch_boundaries(built):
    """GPU test 3: lines 100 m from the scans of a non-empty map (every voxel MISSING, pass = MISSING: the probes and all
    kernels run) of 8 B k + {-1, 0, 1, 2} voxels, k = 1, 2, B = LA3DM_TRAVEL_BATCH, along each axis and from both ends: the
    wave crosses one brick per round, so it ends before, on and after the end of a batch of rounds (rounds, brick runs and
    capped runs as the helper's model counts them); cost = a |d|; max_cost
    round the cost of the first voxel of the brick reached at a batch boundary; the empty map answers the same, and with an
    obstacle field as the host-mode empty map does"""
    import la3dm_amd
    md, mh, _ = _bgk_pair()
    empty = la3dm_amd.BGKOctoMap(**dict(la3dm_amd.BGK_YAML, block_depth=3), device=0)
    assert md.leaves()["A"].size > 0 and empty.is_device_resident()
    B = la3dm_amd.TRAVEL_BATCH
    assert B == T.BATCH and la3dm_amd.TRAVEL_BRICK == T.BRICK and la3dm_amd.TRAVEL_INNER == T.INNER
    lo = T.far_lo(md, R.recipe_lo())
    assert (md.box(lo, (3, 3, 16 * B + 2), fields=())["cls"] == R.MISSING).all()
    syncs = md.mirror_syncs()
    rounds_seen = set()
    for m in (md, empty):
        for length in [8 * B * k + d for k in (1, 2) for d in (-1, 0, 1, 2)]:
            for axis in range(3):
                dims = [1, 1, 1]
                dims[axis] = length
                for seed in (0, length - 1):
                    g = m.travel(lo, dims, [seed], passable=T.MISS_M, connectivity=6 if seed else 26, move_cost=(10, 14, 17), fields=FIELDS)
                    d = np.abs(np.arange(length) - seed)
                    assert (g["cost"].reshape(-1) == 10 * d).all(), (dims, seed)
                    assert g["max_cost"] == 10 * (length - 1) and g["n_reached"] == length and g["n_seeded"] == 1, (dims, seed)
                    code = 13 + (1 if seed else -1) * (9, 3, 1)[axis]          # towards the seed along the axis
                    assert (g["parent"].reshape(-1) == np.where(d == 0, 13, code)).all(), (dims, seed)
                    # one brick per round; a seed alone in the last brick wakes the brick next door itself, in the same round
                    rounds = (length + 7) // 8 - (1 if seed and length % 8 == 1 else 0)
                    assert g["rounds"] == rounds and g["capped"] == 0, (dims, seed, g["rounds"])
                    if m is md and axis == 2:
                        model = T.brick_model(np.ones(dims, bool), np.zeros(dims, np.int64), [seed], 6 if seed else 26, (10, 14, 17))
                        assert tuple(g[k] for k in DIAG) == tuple(model[k] for k in DIAG), (dims, seed, [g[k] for k in DIAG], model)
                    rounds_seen.add(g["rounds"])
        dims = (1, 1, 16 * B + 2)
        at = 10 * 8 * B                                    # the cost of the first voxel of the brick reached in round B + 1
        for cut in (at - 10, at - 1, at, at + 1, at + 10):
            g = m.travel(lo, dims, [0], passable=T.MISS_M, max_cost=cut, connectivity=6)
            want = 10 * np.arange(dims[2])
            assert (g["cost"].reshape(-1) == np.where(want <= cut, want, T.NONE)).all(), cut
            assert g["max_cost"] == cut // 10 * 10 and g["n_reached"] == cut // 10 + 1, (cut, g["max_cost"])
    assert {B, B + 1, 2 * B, 2 * B + 1} <= rounds_seen, rounds_seen
    # an obstacle field on the empty map (the same word everywhere, no transform runs), two bricks along x with a ragged
    # edge: OCCUPIED as the obstacle leaves the box open and free of charge, MISSING closes it (clearance) or charges every
    # step the whole penalty (soft radius alone: d2 = 0; the seed's own is not charged) — tests/test_travel_cpu.py's closed
    # forms; the device-resident map == the host-mode one
    host_empty = la3dm_amd.BGKOctoMap(**dict(la3dm_amd.BGK_YAML, block_depth=3), device=-1)
    dims, n = (9, 5, 3), 9 * 5 * 3
    for obstacles in (T.OCC_M, T.MISS_M):
        for field in (dict(clearance=2), dict(clearance=0, soft_radius=3, penalty=50)):
            _, gh = _compare(empty, host_empty, R.recipe_lo(), dims, [0], "empty map", targets=np.array([0, n - 1, n + 1], np.uint32),
                             passable=T.MISS_M, obstacles=obstacles, connectivity=6, move_cost=(10, 10, 10), **field)
            if obstacles == T.MISS_M and field["clearance"]:
                assert (gh["cost"] == T.NONE).all() and (gh["parent"] == 255).all() and gh["n_seeded"] == gh["n_reached"] == gh["max_cost"] == 0
            else:
                want = T.closed_form(dims, (0, 0, 0), 6, (10 + (50 if obstacles == T.MISS_M else 0),) * 3)
                assert (gh["cost"] == want).all() and gh["n_seeded"] == 1 and gh["n_reached"] == n and gh["max_cost"] == int(want.max())
    assert md.mirror_syncs() == syncs and empty.mirror_syncs() == 0
    # the host-mode map agrees where the line crosses a batch boundary
    _compare(md, mh, lo, (1, 8 * B + 2, 1), [0], "far line", passable=T.MISS_M)


def test_count_ring_wrap(built):
    """A line of 8 * 1024 + 9 voxels on the empty map: the wave crosses one brick per round, so the query runs past round
    1024, where the ring of per-round counts in the working storage is cleared and used again; cost = 10 k, parents towards
    the seed; rounds, brick runs and capped runs as the helper's model counts them"""
    import la3dm_amd
    empty = la3dm_amd.BGKOctoMap(**dict(la3dm_amd.BGK_YAML, block_depth=3), device=0)
    dims = (1, 1, 8 * 1024 + 9)
    g = empty.travel(np.array((0.05, 0.05, 0.05), np.float32), dims, [0], passable=T.MISS_M, connectivity=6, move_cost=(10, 14, 17), fields=FIELDS)
    k = np.arange(dims[2])
    assert (g["cost"].reshape(-1) == 10 * k).all()
    assert (g["parent"].reshape(-1) == np.where(k == 0, 13, 12)).all()
    assert g["n_reached"] == dims[2] and g["max_cost"] == 10 * (dims[2] - 1)
    model = T.brick_model(np.ones(dims, bool), np.zeros(dims, np.int64), [0], 6, (10, 14, 17))
    print(f"ring wrap: device {[g[d] for d in DIAG]}, the model {[model[d] for d in DIAG]}")
    assert tuple(g[d] for d in DIAG) == (1026, 2051, 0) == tuple(model[d] for d in DIAG)
    assert empty.is_device_resident() and empty.mirror_syncs() == 0


@pytest.mark.parametrize("variant", ["GPOctoMap", "BGKLOctoMap", "BGKLVOctoMap"])
def test_device_equals_host_on_other_variants(built, variant):
    """GPU test 4: GP, BGK-L and BGK-LV on their own configurations; the host form == the yardstick over its own box; on
    BGK-LV the UNCERTAIN bit as passable changes the answer, and the yardstick says so.  The classes the yardstick reads
    here come from the host-mode map's box(), not from the leaf-list walk of region_cases.yardstick, which is written for
    BGK's leaf fields (the choice of test_reach_gpu.py); device == host is compared exactly all the same"""
    import la3dm_amd
    params, insert = {"GPOctoMap": (la3dm_amd.GP_YAML, INSERT), "BGKLOctoMap": (la3dm_amd.L_YAML, (0.1, 0.3, 8.0)),
                      "BGKLVOctoMap": (la3dm_amd.LV_YAML, (0.1, 0.3, 8.0))}[variant]
    md, mh = _pair(variant, dict(params), (1, 2), insert)
    lo = R.recipe_lo()
    cls = mh.box(lo, DIMS, fields=())["cls"]
    free = np.flatnonzero(cls.reshape(-1) == R.FREE)
    seeds = [SEED] if cls[T.SEED] == R.FREE else free[free.size // 2:free.size // 2 + 1]
    for c, weights, kw in ((6, (1, 1, 1), T.PLAIN), (26, (10, 14, 17), T.SOFT), (18, (5, 7, 9), T.SOFT), (26, (5, 7, 9), T.PLAIN)):
        q = dict(connectivity=c, move_cost=weights, **kw)
        _, gh = _compare(md, mh, lo, DIMS, seeds, variant, **q)
        T.assert_same(gh, T.yardstick(cls, seeds, **q), (variant, "host form vs the yardstick over its own box", q))
    _compare(md, mh, lo, (7, 9, 11), [0, 5, 100], variant + " small", passable=0x1F, connectivity=18)
    unc = 1 << R.UNCERTAIN
    plain = T.yardstick(cls, free[::50], T.FREE_M)
    wider = T.yardstick(cls, free[::50], T.FREE_M | unc)
    print(variant, "voxels reached from FREE voxels without / with UNCERTAIN passable:", plain["n_reached"], wider["n_reached"])
    assert (wider["n_reached"] > plain["n_reached"]) == (variant == "BGKLVOctoMap")
    gd, gh = _compare(md, mh, lo, DIMS, free[::50], variant + " bit 4", passable=T.FREE_M | unc)
    T.assert_same(gh, wider, variant + " bit 4")


def test_device_pointer_form_refusals_and_storage(built):
    """GPU test 5 on a bare la3dm_devmap: refusals in both pointer forms with their text and nothing written; the
    device-pointer form == the host-pointer form with the arrays on pointers 4 bytes off a 16-byte boundary; arrays not
    asked for are untouched; free device memory is the same before and after 50 calls and a following smaller request"""
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
        at = int(T.flat(T.SEED, dims))                  # the sensor's voxel where it is FREE, else a FREE voxel in the middle of the list
        seeds = np.array([at if cls[at] == R.FREE else free[free.size // 2], n + 3], np.uint32)
        targets = np.concatenate([np.arange(0, n, 97), [n, 0xFFFFFFFF]]).astype(np.uint32)
        nt = targets.size
        names = ("cost", "target_cost", "parent")
        h = dict(cost=np.full(n, 7, np.uint32), target_cost=np.full(nt, 7, np.uint32), parent=np.full(n, 7, np.uint8))
        ho = _lib.TravelOut(*[h[k].ctypes.data for k in names])
        d_seeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
        d_targets = torch.from_numpy(targets.view(np.int32)).to(dev)

        def tensors(fill, offset=0):
            """cost and target_cost `offset` words into their tensors, parent 4 * offset bytes"""
            t = dict(cost=torch.full((n + 4,), fill, dtype=torch.int32, device=dev), target_cost=torch.full((nt + 4,), fill, dtype=torch.int32, device=dev),
                     parent=torch.full((n + 16,), fill & 0x7F, dtype=torch.uint8, device=dev))
            torch.cuda.synchronize()
            return t, _lib.TravelOut(t["cost"][offset:].data_ptr(), t["target_cost"][offset:].data_ptr(), t["parent"][4 * offset:].data_ptr())

        def params(pm=1, om=2, cl=1, sr=4, pen=40, mv=(10, 14, 17), c=26, mc=1 << 31):
            return _lib.TravelParams(pm, om, cl, sr, pen, (C.c_uint32 * 3)(*mv), c, mc)
        t, do = tensors(7)
        stats = _lib.TravelStats(77, 77, 77, 77, 77, 77)
        over = np.array((1 << 10, 1 << 10, (1 << 8) + 1), np.uint32)      # whole bricks: above 2^28
        for fn, out, sp, tp in ((H.la3dm_devmap_travel_host, ho, seeds.ctypes.data, targets.ctypes.data),
                                (H.la3dm_devmap_travel_device, do, d_seeds.data_ptr(), d_targets.data_ptr())):
            def call(lo_p=lop, d_p=dp, s=sp, ns=2, tg=tp, k=nt, o=C.byref(out), no_params=False, **kw):
                p = params(**kw)
                return fn(dm, lo_p, d_p, s, ns, None if no_params else C.byref(p), tg, k, o, C.byref(stats), None)
            assert fn(None, lop, dp, sp, 2, C.byref(params()), tp, nt, C.byref(out), C.byref(stats), None) == ERR_ARG
            assert call(no_params=True) == ERR_ARG and "params is NULL" in err()
            for mask in (0, 0x20, 0x80000002):
                assert call(pm=mask) == ERR_ARG and "pass_mask must hold" in err()
            for mask in (0, 0x20, 0x80000002):
                assert call(om=mask) == ERR_ARG and "obstacle_mask must hold" in err()
            assert call(cl=1025) == ERR_ARG and "clearance must not exceed" in err()
            assert call(sr=1025) == ERR_ARG and "soft_radius must not exceed" in err()
            assert call(pen=0) == ERR_ARG and "penalty must be >= 1" in err()
            assert call(pen=(1 << 16) + 1) == ERR_ARG and "LA3DM_TRAVEL_MAX_PENALTY" in err()
            for mv in ((0, 14, 17), (10, 14, 0), (10, (1 << 16) + 1, 17)):
                assert call(mv=mv) == ERR_ARG and "move_cost" in err()
            for c in (0, 7, 27, 0xFFFFFFFF):
                assert call(c=c) == ERR_ARG and "connectivity must be 6, 18 or 26" in err()
            for k in (0, (1 << 31) + 1):
                assert call(mc=k) == ERR_ARG and "max_cost must lie in" in err()
            assert call(ns=(1 << 20) + 1) == ERR_ARG and "LA3DM_TRAVEL_MAX_SEEDS" in err()
            assert call(k=(1 << 28) + 1) == ERR_ARG and "n_targets" in err()
            assert call(s=None) == ERR_ARG and "seeds is NULL" in err()
            assert call(tg=None) == ERR_ARG and "targets is NULL" in err()
            assert call(o=None) == ERR_ARG and "out is NULL" in err()
            assert call(o=C.byref(_lib.TravelOut(None, None, out.parent)), k=0) == ERR_ARG and "must not be NULL" in err()
            assert call(k=0) == ERR_ARG and "target_cost is set with n_targets = 0" in err()
            assert call(o=C.byref(_lib.TravelOut(out.cost, None, None))) == ERR_ARG and "target_cost must not be NULL with n_targets > 0" in err()
            assert call(pm=0, lo_p=None) == ERR_ARG and "pass_mask" in err()             # travel's checks come first
            assert call(lo_p=None) == ERR_ARG and "lo is NULL" in err()
            assert call(d_p=None) == ERR_ARG and "dims is NULL" in err()
            bad = np.array((np.nan, 0, 0), np.float32)
            assert call(lo_p=bad.ctypes.data) == ERR_ARG and "lo must be finite" in err()
            d0 = dims.copy()
            d0[1] = 0
            assert call(d_p=d0.ctypes.data) == ERR_ARG and "dims must be >= 1" in err()
            assert call(d_p=over.ctypes.data) == ERR_ARG and "LA3DM_TRAVEL_MAX_CELLS" in err(), err()
        assert all((h[k] == 7).all() for k in h) and all((t[k].cpu().numpy() == 7).all() for k in t)
        assert [getattr(stats, k) for k, _ in stats._fields_] == [77] * 6
        # the device-pointer form == the host-pointer form; arrays 4 bytes off a 16-byte boundary; what was not asked for is untouched
        for kw in (dict(c=6, mv=(1, 1, 1), cl=0, sr=0, pen=0), dict(), dict(c=18, mv=(5, 7, 9), cl=2, sr=3, pen=9), dict(pm=5, c=26, mc=700)):
            hs = _lib.TravelStats()
            info = _lib.RegionInfo()
            p = params(**kw)
            assert H.la3dm_devmap_travel_host(dm, lop, dp, seeds.ctypes.data, 2, C.byref(p), targets.ctypes.data, nt, C.byref(ho), C.byref(hs),
                                              C.byref(info)) == OK, err()
            fin = h["cost"] != T.NONE
            assert hs.n_seeded <= 1 and hs.n_reached == int(fin.sum()) and hs.max_cost == (int(h["cost"][fin].max()) if fin.any() else 0), (kw, hs.n_seeded, hs.n_reached)
            assert kw.get("cl", 1) > 0 or (hs.n_seeded == 1 and hs.n_reached > 100), (kw, hs.n_seeded, hs.n_reached)
            assert ((h["parent"] == 255) == ~fin).all() and ((h["parent"] == 13) == (h["cost"] == 0)).all()
            assert (h["target_cost"][:-2] == h["cost"][targets[:-2]]).all() and (h["target_cost"][-2:] == T.NONE).all()
            for offset in (0, 1):
                for fields in (names, ("cost",), ("target_cost",), ("cost", "parent"), ("target_cost", "parent")):
                    t, full = tensors(0x5A5A5A5A, offset)
                    assert (t["cost"][offset:].data_ptr() & 15) == 4 * offset
                    do = _lib.TravelOut(*[getattr(full, k) if k in fields else None for k in names])
                    k = nt if "target_cost" in fields else 0
                    ds, info2 = _lib.TravelStats(), _lib.RegionInfo()
                    assert H.la3dm_devmap_travel_device(dm, lop, dp, d_seeds.data_ptr(), 2, C.byref(p), d_targets.data_ptr() if k else None, k,
                                                        C.byref(do), C.byref(ds), C.byref(info2)) == OK, err()
                    assert [getattr(ds, f) for f, _ in ds._fields_] == [getattr(hs, f) for f, _ in hs._fields_]
                    assert list(info2.origin) == list(info.origin) and info2.block_key == info.block_key and list(info2.cell) == list(info.cell)
                    g = dict(cost=t["cost"].cpu().numpy().view(np.uint32), target_cost=t["target_cost"].cpu().numpy().view(np.uint32),
                             parent=t["parent"].cpu().numpy())
                    for key, size, step, fill in (("cost", n, 1, 0x5A5A5A5A), ("target_cost", nt, 1, 0x5A5A5A5A), ("parent", n, 4, 0x5A)):
                        off = offset * step
                        if key in fields:
                            assert (g[key][:off] == fill).all() and (g[key][off + size:] == fill).all(), (key, offset)
                            assert (g[key][off:off + size] == h[key]).all(), (key, offset, fields, kw)
                        else:
                            assert (g[key] == fill).all(), (key, fields)
        # storage: the first call at a size reserves, 50 more do not; a smaller region afterwards allocates nothing
        t, do = tensors(0)
        small = np.array((31, 17, 23), np.uint32)
        ps = [params(cl=i % 3, sr=(i % 2) * 4, c=F.CONNECTIVITIES[i % 3]) for i in range(6)]
        big = params(cl=2, sr=4)
        dev_call = lambda d_p, p: H.la3dm_devmap_travel_device(dm, lop, d_p, d_seeds.data_ptr(), 2, C.byref(p), d_targets.data_ptr(), nt,   # noqa: E731
                                                               C.byref(do), None, None)
        host_call = lambda d_p, p: H.la3dm_devmap_travel_host(dm, lop, d_p, seeds.ctypes.data, 2, C.byref(p), targets.ctypes.data, nt,   # noqa: E731
                                                              C.byref(ho), None, None)

        def free_mem():
            torch.cuda.synchronize()
            return torch.cuda.mem_get_info()[0]
        assert dev_call(dp, big) == OK and host_call(dp, big) == OK, err()
        f0 = free_mem()
        for i in range(25):
            assert dev_call(dp, ps[i % 6]) == OK and host_call(dp, ps[i % 6]) == OK, err()
        assert dev_call(small.ctypes.data, big) == OK and host_call(small.ctypes.data, big) == OK, err()
        f1 = free_mem()
        print(f"free device memory before / after 50 calls and a smaller region: {f0} / {f1}")
        # the figure is the whole device's: a process of another user may release memory meanwhile, so growth is what fails
        assert f1 >= f0, (f0, f1)
    finally:
        H.la3dm_devmap_destroy(dm)


def test_example_program(built):
    """GPU test 6: examples/route.cpp (built by build()) == the Python binding on the same map: the goals, the path and the
    summary line"""
    import la3dm_amd
    exe = os.path.join(ROOT, "examples", "route")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "3"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    print(r.stdout)
    assert lines[-1].startswith("route 128 x 128 x 16 from ") and lines[-2].startswith("path ") and all(ln.startswith("goal ") for ln in lines[:-2])
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
    g = m.travel(lo, dims, [T.flat(s, dims)], targets=fr["index"], fields=("parent",), **T.SOFT)
    assert m.is_device_resident() and m.mirror_syncs() == before
    ok = g["target_cost"] != T.NONE
    tok = lines[-1].split()
    got = {tok[k]: tok[k + 1] for k in range(len(tok) - 1)}
    assert int(got["found"]) == fr["n"] > 0 and int(got["reachable"]) == int(ok.sum()) > 0 and int(got["max_cost"]) == g["max_cost"]
    assert got["mirror_syncs"] == "0" and got["device_resident"] == "1"
    assert len(lines) == min(5, int(ok.sum())) + 2
    order = np.argsort(g["target_cost"][ok], kind="stable")[:5]
    ijk = np.stack(np.unravel_index(fr["index"][ok][order], dims), 1).astype(np.float32)
    p = fr["origin"] + ijk * res
    for ln, q, st in zip(lines[:-2], p, g["target_cost"][ok][order]):
        tk = ln.split()
        assert np.allclose([float(v) for v in tk[1:4]], q, atol=1e-4) and int(tk[5]) == int(st), (ln, q, st)
    path = la3dm_amd.follow_parents(g["parent"], dims, fr["index"][ok][order][0])
    d2 = m.distance_field(lo, dims, obstacles=("occupied",), radius=4, fields=("d2",))["d2"].reshape(-1)[path]
    steps = np.diff(np.stack(np.unravel_index(path, dims), 1), axis=0)
    tk = lines[-2].split()
    assert int(tk[1]) == path.size and abs(float(tk[4]) - float(np.sqrt((steps ** 2).sum(1)).sum() * res)) < 2e-3
    assert tk[6] == ("far" if d2.min() == 0xFFFFFFFF else str(int(d2.min())))
