"""drive on the device-resident map: brick relaxation in a 10 x 10 x 16 LDS tile over a member list or over footing's foot
words (csrc/devmap_drive.h).  Device-resident map == host-mode map (host/drive_cells.h) == the yardstick written from the
contract comment (tests/helpers/drive_cases.py).  Integers throughout and a unique answer: every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pcd_path

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import footing_cases as F  # noqa: E402
import drive_cases as D  # noqa: E402

pytestmark = pytest.mark.gpu

OK = 0
LO = F.SCENE_LO
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured
ALL = ("cost", "parent", "of_member", "target_index")
DIAG = ("rounds", "brick_runs", "capped")
_MAPS = {}


def _scene_pair(cls_name="BGKOctoMap", yaml=None, swap=None):
    """footing's scene in a device-resident map and in a host-mode one (list mode never reads the pool; a loaded map makes sure
    the device map exists)"""
    if cls_name not in _MAPS:
        import la3dm_amd
        params = dict(yaml or R.YAML, block_depth=4, resolution=0.1)
        stream = F.scene_stream(params, cls_name, swap)
        cls = getattr(la3dm_amd, cls_name)
        md = cls(**params, device=0).unpack(stream)
        mh = cls(**params, device=0).set_device_resident(False).unpack(stream)
        assert md.is_device_resident() and not mh.is_device_resident()
        _MAPS[cls_name] = (md, mh)
    return _MAPS[cls_name]


def _three(member, seeds, targets=None, what="", **kw):
    """device == host-mode twin == yardstick over the list of `member`; returns (the yardstick's answer, the device's)"""
    md, mh = _scene_pair()
    index = np.flatnonzero(member.reshape(-1)).astype(np.uint32)
    fields = ALL if targets is not None else ALL[:3]
    want = D.yardstick(member, seeds, targets=targets, members=index, **kw)
    gd = md.drive(LO, member.shape, seeds, members=index, targets=targets, fields=fields, **kw)
    gh = mh.drive(LO, member.shape, seeds, members=index, targets=targets, fields=fields, **kw)
    assert set(gd) == set(gh)
    D.assert_same(gd, want, (what, "device", kw))
    D.assert_same(gh, want, (what, "host", kw))
    R.assert_same(gd, gh, ("origin", "cell"), what)
    assert gd["block_key"] == gh["block_key"] and all(gh[k] == 0 for k in DIAG)
    assert (gd["brick_runs"] > 0) == (want["n_seeded"] > 0)            # the device form ran
    return want, gd


def test_hand_built_sets(built):
    """GPU test 1: the flat floor against the closed form, the stairs both ways, the brick-border links (under-waking leaves NONE),
    floor and shelf, the region dims, the cut, the lists, the seeds and snap"""
    md, _ = _scene_pair()
    syncs = md.mirror_syncs()
    m, dims = D.flat_floor(), D.FLOOR_DIMS
    for connectivity in (4, 8):
        for si, sj in ((8, 8), (0, 16)):
            y, _ = _three(m, [D.flat(dims, si, sj, 3)], targets=[D.flat(dims, 16, 0, 3), D.flat(dims, 0, 0, 4)], what="floor",
                          connectivity=connectivity, step=0, move_cost=(5, 9))
            assert (y["cost"] == D.floor_closed_form(dims, (si, sj), 3, connectivity, (5, 9))).all()
    up, down = 7, 3
    for rise in (1, 2, 3, 4, 5):
        sdims, sm, bottom, top = D.stairs(rise)
        for step in range(5):
            kw = dict(connectivity=4 if step % 2 else 8, step=step, climb_up=up, climb_down=down)
            y, _ = _three(sm, [bottom], targets=[top], what=("stairs up", rise), **kw)
            assert y["target_cost"][0] == ((D.STAIR_COLUMNS - 1) * (10 + up * rise) if rise <= step else D.NONE), (rise, step)
            y, _ = _three(sm, [top], targets=[bottom], what=("stairs down", rise), **kw)
            assert y["target_cost"][0] == ((D.STAIR_COLUMNS - 1) * (10 + down * rise) if rise <= step else D.NONE), (rise, step)
    for a, b, step, connectivity in D.LINKS:
        lm = D.link(a, b)
        fa, fb = D.flat(D.LINK_DIMS, *a), D.flat(D.LINK_DIMS, *b)
        for seed, target in ((fa, fb), (fb, fa)):
            y, _ = _three(lm, [seed], targets=[target], what=("link", a, b), connectivity=connectivity, step=step, climb_up=2, climb_down=1)
            assert y["target_cost"][0] != D.NONE and y["n_reached"] == 2
            if abs(a[2] - b[2]) == step and step > 0:
                assert _three(lm, [seed], targets=[target], what="one short", connectivity=connectivity, step=step - 1)[0]["target_cost"][0] == D.NONE
    seed, on_shelf = D.flat(D.SHELF_DIMS, 0, 4, 2), D.flat(D.SHELF_DIMS, 6, 4, 6)
    assert _three(D.shelf(False), [seed], targets=[on_shelf], what="shelf", step=D.SHELF_STEP, climb_up=3)[0]["target_cost"][0] == D.NONE
    assert _three(D.shelf(True), [seed], targets=[on_shelf], what="ramp", step=D.SHELF_STEP, climb_up=3)[0]["target_cost"][0] != D.NONE
    _three(D.shelf(True), [D.flat(D.SHELF_DIMS, 6, 4, 7)], targets=[D.flat(D.SHELF_DIMS, 6, 4, 5)], what="snap", step=D.SHELF_STEP, snap=5)
    for edims in D.EDGE_DIMS:
        em = D.random_members(edims, 3, 0.8)
        em[0, 0, 0] = True
        for connectivity, step in ((4, 0), (8, 1), (8, 4)):
            _three(em, [0, em.size - 1], targets=[0, em.size - 1, em.size], what=("dims", edims), connectivity=connectivity, step=step, snap=2,
                   climb_up=1, climb_down=2)
    seed = D.flat(dims, 8, 8, 3)
    for cut in (1, 10, 27, 28):
        _three(m, [seed], targets=[D.flat(dims, 10, 9, 3)], what=("cut", cut), step=0, max_cost=cut)
    index = np.flatnonzero(m.reshape(-1)).astype(np.uint32)
    lst = np.concatenate([index[::-1], index[:40], np.array([m.size, m.size + 7, 0xFFFFFFFF], np.uint32)])
    want = D.yardstick(m, [seed], members=lst, step=0)
    D.assert_same(md.drive(LO, dims, [seed], members=lst, step=0, fields=ALL[:3]), want, "a list with duplicates and strays")
    for seeds in ([], [D.flat(dims, 8, 8, 2), m.size, 0xFFFFFFFF], [seed, seed, D.flat(dims, 8, 8, 4)]):
        _three(m, np.array(seeds, np.uint32), targets=[seed], what=("seeds", seeds), step=0)
    _three(np.zeros(dims, bool), [seed], targets=[seed], what="no members")
    tall = (3, 3, 40)
    for snap in (0, 1, 32):
        col = np.zeros(tall, bool)
        col[:, :, 2] = True
        at, beyond = D.flat(tall, 1, 1, 2 + snap), D.flat(tall, 1, 1, 3 + snap)
        y, _ = _three(col, [at], targets=[at, beyond, D.flat(tall, 0, 0, 1), col.size], what=("snap", snap), snap=snap, step=0)
        assert y["n_seeded"] == 1 and y["target_index"].tolist() == [D.flat(tall, 1, 1, 2), D.NONE, D.NONE, D.NONE]
        assert _three(col, [beyond], what=("snap, one further", snap), snap=snap, step=0)[0]["n_seeded"] == 0
    assert md.mirror_syncs() == syncs


def test_random_sets_and_output_subsets(built):
    """GPU test 2: random member sets in ragged bricks over both connectivities and every step — the ten instantiations of the
    round kernel — with up != down; then every subset of outputs"""
    md, _ = _scene_pair()
    dims = (19, 13, 21)
    rm = D.random_members(dims, 1, 0.45)
    idx = np.flatnonzero(rm.reshape(-1)).astype(np.uint32)
    for connectivity in (4, 8):
        for step in range(5):
            y, _ = _three(rm, idx[[0, idx.size // 2]], targets=idx[::37], what="random", connectivity=connectivity, step=step, climb_up=6, climb_down=1)
            for t in idx[::211]:
                if y["cost"].reshape(-1)[t] != D.NONE:
                    D.walk(y, rm, dims, t, connectivity, step, (10, 14), 6, 1)
    seed = int(idx[0])
    for fields in ((), ("cost",), ("parent",), ("of_member",), ("cost", "parent"), ALL):
        t = [seed] if ("cost" not in fields and "of_member" not in fields) or "target_index" in fields else None
        got = md.drive(LO, dims, [seed], members=idx, targets=t, step=2, fields=fields)
        assert set(got) == set(fields) | ({"target_cost"} if t is not None else set()) | set(D.STATS) | set(DIAG) | set(R.INFO_FIELDS)
        D.assert_same(got, D.yardstick(rm, [seed], targets=t, members=idx, step=2), ("fields", fields))


def test_serpentines(built):
    """GPU test 3: a one-voxel-wide path of 35 members inside one brick stops a brick run at the inner cap; one through 64 x 8 x 8
    crosses 31 brick borders, and a round moves the wave by one brick at most, so it needs more rounds than one batch"""
    dims, m, first, last, moves = D.serpentine(8)
    y, gd = _three(m, [first], targets=[last], what="serpentine in one brick", connectivity=4, step=0, move_cost=(3, 5))
    assert y["target_cost"][0] == 3 * moves and moves > D.INNER and gd["capped"] > 0
    dims, m, first, last, moves = D.serpentine(64)
    y, gd = _three(m, [first], targets=[last], what="serpentine through bricks", connectivity=4, step=0, move_cost=(3, 5))
    assert y["target_cost"][0] == 3 * moves and gd["rounds"] > D.BATCH and gd["brick_runs"] >= 32
    print(f"serpentine through bricks: rounds {gd['rounds']} brick_runs {gd['brick_runs']} capped {gd['capped']}")


def test_scene_named_voxels(built):
    """GPU test 4: footing's hand-built scene through footing's list and through footing mode, on the device and on the host:
    all equal the yardstick; the issue's named voxels; no mirror refresh"""
    md, mh = _scene_pair()
    syncs = md.mirror_syncs()
    D.scene_named_voxels([md, mh])
    assert md.mirror_syncs() == syncs


@pytest.mark.parametrize("variant", ["GPOctoMap", "BGKLOctoMap", "BGKLVOctoMap"])
def test_other_variants(built, variant):
    """GPU test 5: the other three map classes loaded from the scene's stream (UNCERTAIN where BGK has UNKNOWN on BGK-LV)"""
    import la3dm_amd
    yaml = {"GPOctoMap": la3dm_amd.GP_YAML, "BGKLOctoMap": la3dm_amd.L_YAML, "BGKLVOctoMap": la3dm_amd.LV_YAML}[variant]
    md, mh = _scene_pair(variant, yaml, {R.UNKNOWN: R.UNCERTAIN} if variant == "BGKLVOctoMap" else None)
    f = lambda i, j, k: D.flat(F.SCENE_DIMS, i, j, k)   # noqa: E731
    for step in (0, 1, 2):
        y, _ = D.scene_query([md, mh], F.FREE_M, 3, 0, 0, 0, [f(7, 12, 4)], [f(13, 12, 3), f(19, 4, 5)], step=step, snap=2, climb_up=4, climb_down=1)
        assert (y["target_cost"] != D.NONE).tolist() == [step >= 1, step >= 2]
    D.scene_query([md, mh], F.FREE_M, 4, 2, 1, 6, [f(7, 12, 4)], [f(13, 12, 3)], step=1, snap=2, connectivity=4)


def _pair(params, scans):
    import la3dm_amd
    md = la3dm_amd.BGKOctoMap(**params, device=0)
    mh = la3dm_amd.BGKOctoMap(**params, device=0).set_device_resident(False)
    for i in scans:
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        md.insert_pointcloud(xyz, origin, *INSERT)
        mh.insert_pointcloud(xyz, origin, *INSERT)
    return md, mh


@pytest.mark.parametrize("depth", [3, 4])
def test_two_scan_map(built, depth):
    """GPU test 6: BGK at block_depth 3 and 4, two fused scans, the recipe region: the input conditions re-counted from the
    yardstick of this map, then footing mode == list mode == yardstick on both maps, over the region and over a sub-region
    against each of its faces; no mirror refresh"""
    import la3dm_amd
    md, mh = _pair(dict(la3dm_amd.BGK_YAML, block_depth=depth), (1, 2))
    lv = mh.leaves()
    lo, dims = R.recipe_lo(), R.RECIPE_DIMS
    slo, foot, seeds, targets = D.recipe_case(mh, lv, lo, dims)
    y = D.yardstick(foot, seeds, targets=targets, **D.RECIPE_KW)
    D.assert_exercises_the_feature(D.input_conditions(y), {k: v // 2 for k, v in D.RECIPE_COUNTED[depth].items()})
    syncs = md.mirror_syncs()
    D.recipe_queries([md, mh], slo, foot, seeds, targets, ("recipe", depth))
    for offset, sub in D.FACE_BOXES:
        D.recipe_queries([md, mh], *D.recipe_case(mh, lv, lo, dims, offset, sub), ("face box", depth, offset, sub))
    assert md.mirror_syncs() == syncs


def test_pointer_forms_refusals_and_the_empty_map(built):
    """GPU test 7 on a bare la3dm_devmap, in both pointer forms: the empty map (list mode served, footing mode without a member);
    every refusal in the contract's order with nothing written, the limit values served; after a scan, footing mode == list mode
    over footing's own list == the yardstick over that list, device-pointer form == host-pointer form"""
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
        for device_form in (False, True):
            fn = H.la3dm_devmap_drive_device if device_form else H.la3dm_devmap_drive_host
            held, rooms = [], {}

            def put(a):
                a = np.ascontiguousarray(a)
                if not device_form:
                    held.append(a)
                    return a.ctypes.data
                held.append(torch.from_numpy(a.view(np.int32).copy()).to(dev))
                return held[-1].data_ptr()

            def room(name, n, dtype):
                if not device_form:
                    rooms[name] = np.full(n, 0x5A, dtype)
                    return rooms[name].ctypes.data
                rooms[name] = torch.full((n,), 0x5A, dtype=torch.uint8 if dtype == np.uint8 else torch.int32, device=dev)
                return rooms[name].data_ptr()

            def fetch(name, dtype):
                torch.cuda.synchronize()
                return rooms[name] if not device_form else rooms[name].cpu().numpy().view(dtype)

            def call(lo, dims, seeds, n_seeds, p, targets, n_targets, out, stats=None):
                torch.cuda.synchronize()
                rc = fn(dm, lo, dims, seeds, n_seeds, C.byref(p) if p is not None else None, targets, n_targets,
                        C.byref(out) if out is not None else None, C.byref(stats) if stats is not None else None, None)
                return rc, err()
            serve, member, index, seeds, targets, kw, keep = D.refusal_chain(call, put, room)
            dt = dict(cost=np.uint32, parent=np.uint8, target_cost=np.uint32, target_index=np.uint32, of_member=np.uint32)
            assert all((fetch(k, dt[k]) == 0x5A).all() for k in rooms), "a refused call writes nothing"
            rc, msg = serve()                                              # list mode on the empty map, at the limit values
            assert rc == OK, msg
            want = D.yardstick(member, seeds, targets=targets, **kw)
            got = dict(cost=fetch("cost", np.uint32).reshape(member.shape), parent=fetch("parent", np.uint8).reshape(member.shape),
                       target_cost=fetch("target_cost", np.uint32), target_index=fetch("target_index", np.uint32))
            D.assert_same(got, want, ("the limit values", device_form), D.FIELDS)
            assert (fetch("of_member", np.uint32) == 0x5A).all() and want["n_reached"] > 1
            # footing mode on the empty map: no member, all NONE
            dims = np.array(D.REFUSAL_DIMS, np.uint32)
            lo = np.array((0.05, 0.05, 0.05), np.float32)
            fp = _lib.FootingParams(F.OCC_M, F.OPTIMISTIC, 4, 2, 1, 6)
            p = _lib.DriveParams(None, C.pointer(fp), 0, 8, 1, 3, (C.c_uint32 * 2)(10, 14), 0, 0, 1 << 31)
            stats = _lib.DriveStats()
            out = _lib.DriveOut(room("cost", member.size, np.uint32), room("parent", member.size, np.uint8), None, room("target_cost", 2, np.uint32), None)
            rc, msg = call(lo.ctypes.data, dims.ctypes.data, put(seeds), 2, p, put(targets), 2, out, stats)
            assert rc == OK, msg
            assert (fetch("cost", np.uint32) == D.NONE).all() and (fetch("parent", np.uint8) == 255).all() and (fetch("target_cost", np.uint32) == D.NONE).all()
            assert stats.as_dict() == dict(n_members=0, n_seeded=0, n_reached=0, max_cost=0, rounds=0, brick_runs=0, capped=0)
            assert fn(None, lo.ctypes.data, dims.ctypes.data, None, 0, C.byref(p), None, 0, C.byref(out), None, None) != OK
        # one scan: footing mode against footing's own list, in both pointer forms
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 1))
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3, 0.1, 0.5, 8.0, None) == OK
        lo = (np.asarray(origin, np.float32) + np.asarray(R.RECIPE_OFFSET, np.float32)).astype(np.float32)
        dims = np.array((77, 67, 39), np.uint32)
        n = int(dims.prod())
        fp = _lib.FootingParams(F.OCC_M, F.OPTIMISTIC, 4, 2, 1, 0)
        lst, found = np.zeros(n, np.uint32), C.c_uint64(0)
        fo = _lib.FootingOut(lst.ctypes.data, None, None, None)
        assert H.la3dm_devmap_footing_host(dm, lo.ctypes.data, dims.ctypes.data, C.byref(fp), n, C.byref(fo), C.byref(found), None, None) == OK, err()
        lst = lst[:found.value].copy()
        member = D.members_of(tuple(int(v) for v in dims), lst)
        seeds = np.array([int(lst[0]) + 1, int(lst[lst.size // 2]) + 1], np.uint32)
        targets = np.arange(0, n, 97, dtype=np.uint32)
        kw = dict(connectivity=8, step=1, snap=3, move_cost=(10, 14), climb_up=5, climb_down=2)
        want = D.yardstick(member, seeds, targets=targets, members=lst, **kw)
        print(f"bare devmap: {D.input_conditions(want)}")
        assert want["n_members"] == found.value > 0 and want["n_reached"] > want["n_seeded"] > 0
        d_seeds, d_targets, d_lst = (torch.from_numpy(a.view(np.int32).copy()).to(dev) for a in (seeds, targets, lst))
        for footing_mode in (False, True):
            base = (None, C.pointer(fp), 0) if footing_mode else (lst.ctypes.data, None, lst.size)
            p = _lib.DriveParams(*base, 8, 1, 3, (C.c_uint32 * 2)(10, 14), 5, 2, 1 << 31)
            h = dict(cost=np.zeros(n, np.uint32), parent=np.zeros(n, np.uint8), of_member=np.zeros(lst.size, np.uint32),
                     target_cost=np.zeros(targets.size, np.uint32), target_index=np.zeros(targets.size, np.uint32))
            names = [k for k in D.FIELDS if not (footing_mode and k == "of_member")]
            out = _lib.DriveOut(*[h[k].ctypes.data if k in names else None for k in D.FIELDS])
            stats = _lib.DriveStats()
            assert H.la3dm_devmap_drive_host(dm, lo.ctypes.data, dims.ctypes.data, seeds.ctypes.data, 2, C.byref(p), targets.ctypes.data, targets.size,
                                             C.byref(out), C.byref(stats), None) == OK, err()
            got = {k: (h[k].reshape(member.shape) if k in ("cost", "parent") else h[k]) for k in names}
            D.assert_same(dict(got, **stats.as_dict()), want, ("bare devmap, host pointers", footing_mode))
            t = {k: torch.full((h[k].size,), 0x5A, dtype=torch.uint8 if k == "parent" else torch.int32, device=dev) for k in D.FIELDS}
            for subset in (names, ["target_cost"], ["cost", "parent"]):
                pd = _lib.DriveParams(*((None, C.pointer(fp), 0) if footing_mode else (d_lst.data_ptr(), None, lst.size)), 8, 1, 3,
                                      (C.c_uint32 * 2)(10, 14), 5, 2, 1 << 31)
                for v in t.values():
                    v.fill_(0x5A)
                torch.cuda.synchronize()
                nt = targets.size if "target_cost" in subset else 0
                do = _lib.DriveOut(*[t[k].data_ptr() if k in subset else None for k in D.FIELDS])
                stats2 = _lib.DriveStats()
                assert H.la3dm_devmap_drive_device(dm, lo.ctypes.data, dims.ctypes.data, d_seeds.data_ptr(), 2, C.byref(pd), d_targets.data_ptr() if nt else None,
                                                   nt, C.byref(do), C.byref(stats2), None) == OK, err()
                assert {k: getattr(stats2, k) for k in D.STATS} == {k: getattr(stats, k) for k in D.STATS}
                for k in D.FIELDS:
                    g = t[k].cpu().numpy().view(h[k].dtype)
                    assert (g == (h[k] if k in subset else 0x5A)).all(), (k, subset, footing_mode)
    finally:
        H.la3dm_devmap_destroy(dm)
