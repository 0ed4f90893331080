"""drive on a host-mode map (device = -1, no GPU): least-cost ground routes over a member list or over footing's voxels,
against an independent yardstick written from the contract comment (tests/helpers/drive_cases.py: shifted slices and
scipy's Dijkstra).  Integers throughout and a unique answer: every comparison is exact."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import footing_cases as F  # noqa: E402
import drive_cases as D  # noqa: E402

LO = (0.05, 0.05, 0.05)
ALL = ("cost", "parent", "of_member", "target_index")
_MAP = {}


def _empty():
    """an empty host-mode map: list mode never reads the map"""
    if "m" not in _MAP:
        import la3dm_amd
        _MAP["m"] = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
    return _MAP["m"]


def _both(member, seeds, targets=None, what="", **kw):
    """the host form over the list of `member` == the yardstick, on every field and stat; returns the yardstick's answer"""
    index = np.flatnonzero(member.reshape(-1)).astype(np.uint32)
    got = _empty().drive(LO, member.shape, seeds, members=index, targets=targets, fields=ALL if targets is not None else ALL[:3], **kw)
    want = D.yardstick(member, seeds, targets=targets, members=index, **kw)
    D.assert_same(got, want, (what, kw))
    assert got["rounds"] == got["brick_runs"] == got["capped"] == 0
    return want


def test_symbols_structs_and_signature(built):
    """the entry points are exported and bound, the structs have the header's layout, the constants agree, and the Python
    method has the documented signature"""
    import la3dm_amd
    from la3dm_amd import _lib
    hip, mp = _lib.hip(), _lib.maplib()
    for lib, n in ((hip, "la3dm_devmap_drive_host"), (hip, "la3dm_devmap_drive_device"), (mp, "la3dm_map_drive")):
        assert hasattr(lib, n) and n in _lib.HIP_SYMBOLS + _lib.MAP_SYMBOLS, n
        assert list(getattr(lib, n).argtypes)[1:] == list(_lib._DRIVE[n][1])[1:]
    assert C.sizeof(_lib.DriveParams) == 56 and _lib.DriveParams.n_members.offset == 16 and _lib.DriveParams.max_cost.offset == 48
    assert C.sizeof(_lib.DriveOut) == 40 and C.sizeof(_lib.DriveStats) == 28
    assert C.sizeof(_lib.TravelParams) == 40                       # travel's struct kept its layout
    hdr = open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
    val = lambda n: eval(re.search(rf"#define {n}\s+(.+)", hdr).group(1).replace("u", ""))   # noqa: E731
    assert val("LA3DM_DRIVE_NONE") == la3dm_amd.DRIVE_NONE == D.NONE
    assert val("LA3DM_DRIVE_MAX_STEP") == val("LA3DM_FOOTING_MAX_STEP") == la3dm_amd.DRIVE_MAX_STEP == D.MAX_STEP
    assert val("LA3DM_DRIVE_MAX_SNAP") == la3dm_amd.DRIVE_MAX_SNAP == D.MAX_SNAP
    assert (val("LA3DM_DRIVE_BRICK"), val("LA3DM_DRIVE_INNER"), val("LA3DM_DRIVE_BATCH")) == (D.BRICK, D.INNER, D.BATCH)
    assert val("LA3DM_DRIVE_MAX_CELLS") == val("LA3DM_DRIVE_MAX_MEMBERS") == 1 << 28 and val("LA3DM_DRIVE_MAX_SEEDS") == 1 << 20
    assert val("LA3DM_DRIVE_MAX_ROUNDS") == 1 << 16
    assert re.search(r"static_assert\(LA3DM_DRIVE_MAX_STEP == LA3DM_FOOTING_MAX_STEP", open(os.path.join(ROOT, "la3dm_amd", "csrc", "host", "region_contract.h")).read())
    sig = inspect.signature(la3dm_amd.BGKOctoMap.drive)
    assert list(sig.parameters) == ["self", "lo", "dims", "seeds", "members", "footing", "connectivity", "step", "snap", "move_cost",
                                    "climb_up", "climb_down", "max_cost", "targets", "fields"]
    assert sig.parameters["connectivity"].default == 8 and sig.parameters["move_cost"].default == (10, 14)
    for cls in (la3dm_amd.GPOctoMap, la3dm_amd.BGKLOctoMap, la3dm_amd.BGKLVOctoMap):
        assert cls.drive is la3dm_amd.BGKOctoMap.drive


@pytest.mark.parametrize("connectivity", [4, 8])
def test_flat_floor_closed_form(built, connectivity):
    """a floor at k = 3 in 17 x 17 x 9 (3 x 3 x 2 ragged bricks): octile / Manhattan distance, and the parents walk home"""
    m, dims = D.flat_floor(), D.FLOOR_DIMS
    for si, sj in ((8, 8), (0, 16), (7, 8)):
        for mc in ((10, 14), (1, 1), (5, 9)):
            kw = dict(connectivity=connectivity, step=0, move_cost=mc)
            y = _both(m, [D.flat(dims, si, sj, 3)], targets=[D.flat(dims, 16, 0, 3), D.flat(dims, 0, 0, 4)], what="floor", **kw)
            assert (y["cost"] == D.floor_closed_form(dims, (si, sj), 3, connectivity, mc)).all()
            assert y["target_cost"][1] == D.NONE and y["n_reached"] == 17 * 17
            for t in (D.flat(dims, 16, 0, 3), D.flat(dims, 0, 16, 3), D.flat(dims, 9, 3, 3)):
                D.walk(y, m, dims, t, connectivity, 0, mc, 0, 0)


def test_stairs(built):
    """single-column stairs that rise 1 .. 5 voxels a column are climbed iff rise <= step; up and down cost differently"""
    up, down = 7, 3
    for rise in (1, 2, 3, 4, 5):
        dims, m, bottom, top = D.stairs(rise)
        for step in range(5):
            for connectivity in (4, 8):
                kw = dict(connectivity=connectivity, step=step, move_cost=(10, 14), climb_up=up, climb_down=down)
                y = _both(m, [bottom], targets=[top], what=("stairs up", rise), **kw)
                assert y["target_cost"][0] == ((D.STAIR_COLUMNS - 1) * (10 + up * rise) if rise <= step else D.NONE), (rise, step)
                y = _both(m, [top], targets=[bottom], what=("stairs down", rise), **kw)
                assert y["target_cost"][0] == ((D.STAIR_COLUMNS - 1) * (10 + down * rise) if rise <= step else D.NONE), (rise, step)
                if rise <= step:
                    D.walk(y, m, dims, bottom, connectivity, step, (10, 14), up, down)


def test_brick_border_links(built):
    """two members on either side of a brick border, joined by one move: reached at that step, not one step below it"""
    for a, b, step, connectivity in D.LINKS:
        m = D.link(a, b)
        fa, fb = D.flat(D.LINK_DIMS, *a), D.flat(D.LINK_DIMS, *b)
        for seed, target in ((fa, fb), (fb, fa)):
            y = _both(m, [seed], targets=[target], what=("link", a, b), connectivity=connectivity, step=step, climb_up=2, climb_down=1)
            assert y["target_cost"][0] != D.NONE and y["n_reached"] == 2
            if abs(a[2] - b[2]) == step and step > 0:
                y = _both(m, [seed], targets=[target], what=("link, one short", a, b), connectivity=connectivity, step=step - 1)
                assert y["target_cost"][0] == D.NONE
        if abs(a[0] - b[0]) + abs(a[1] - b[1]) == 2:
            assert _both(m, [fa], targets=[fb], connectivity=4, step=step)["target_cost"][0] == D.NONE


def test_floor_and_shelf(built):
    """a floor and a shelf in one column are not joined at step 2, whatever the column; a ramp member joins them"""
    dims = D.SHELF_DIMS
    seed, on_shelf = D.flat(dims, 0, 4, 2), D.flat(dims, 6, 4, 6)
    y = _both(D.shelf(False), [seed], targets=[on_shelf, D.flat(dims, 6, 4, 2)], what="shelf", step=D.SHELF_STEP, climb_up=3)
    assert y["target_cost"][0] == D.NONE and y["target_cost"][1] == 60 and y["n_reached"] == 81
    m = D.shelf(True)
    y = _both(m, [seed], targets=[on_shelf], what="shelf with ramp", step=D.SHELF_STEP, climb_up=3)
    assert y["target_cost"][0] != D.NONE and y["n_reached"] == 81 + 45 + 1
    path = D.walk(y, m, dims, on_shelf, 8, D.SHELF_STEP, (10, 14), 3, 0)
    assert D.flat(dims, 3, 0, 4) in path
    # a seed above the shelf snaps to the shelf, not to the floor below it
    y = _both(m, [D.flat(dims, 6, 4, 7)], targets=[D.flat(dims, 6, 4, 5)], what="snap picks the highest", step=D.SHELF_STEP, snap=5)
    assert y["cost"][6, 4, 6] == 0 and y["target_index"][0] == D.flat(dims, 6, 4, 2)


def test_serpentines(built):
    """one-voxel-wide paths at connectivity 4: the cost is the number of moves"""
    for nx in (8, 64):
        dims, m, first, last, moves = D.serpentine(nx)
        y = _both(m, [first], targets=[last], what=("serpentine", nx), connectivity=4, step=0, move_cost=(3, 5))
        assert y["target_cost"][0] == 3 * moves and y["n_reached"] == y["n_members"] == 4 * nx + 3
        assert len(D.walk(y, m, dims, last, 4, 0, (3, 5), 0, 0)) == moves + 1


@pytest.mark.parametrize("dims", D.EDGE_DIMS)
def test_region_dims(built, dims):
    """regions of one voxel, one row, one layer, and a ninth plane in a brick of its own"""
    for density in (1.0, 0.6):
        m = D.random_members(dims, 3, density)
        m[0, 0, 0] = True
        for connectivity, step in ((4, 0), (8, 1), (8, 4)):
            _both(m, [0, m.size - 1], targets=[0, m.size - 1, m.size], what=("dims", dims), connectivity=connectivity, step=step, snap=2,
                  climb_up=1, climb_down=2)


def test_random_sets_every_parameter(built):
    """random member sets in ragged bricks over both connectivities and every step, with up != down"""
    dims = (19, 13, 11)
    for seed, density in ((1, 0.35), (2, 0.6)):
        m = D.random_members(dims, seed, density)
        idx = np.flatnonzero(m.reshape(-1))
        for connectivity in (4, 8):
            for step in range(5):
                y = _both(m, idx[[0, idx.size // 2]], targets=idx[::37], what=("random", seed), connectivity=connectivity, step=step,
                          move_cost=(10, 14), climb_up=6, climb_down=1)
                for t in idx[::53]:
                    if y["cost"].reshape(-1)[t] != D.NONE:
                        D.walk(y, m, dims, t, connectivity, step, (10, 14), 6, 1)


def test_cut_lists_seeds_snap_and_targets(built):
    """the max_cost cut; duplicate and out-of-range members; seeds that are no members; no seed at all; snap 0, 1 and 32 with the
    member exactly snap below and one further; targets out of range"""
    m, dims = D.flat_floor(), D.FLOOR_DIMS
    seed = D.flat(dims, 8, 8, 3)
    for cut in (1, 9, 10, 27, 28, 112):
        y = _both(m, [seed], targets=[D.flat(dims, 10, 9, 3)], what=("cut", cut), step=0, max_cost=cut)
        full = D.floor_closed_form(dims, (8, 8), 3, 8, (10, 14))
        assert (y["cost"] == np.where(full <= cut, full, D.NONE)).all() and y["max_cost"] <= cut
    # the list: duplicates count once, entries out of range are ignored and get NONE
    index = np.flatnonzero(m.reshape(-1)).astype(np.uint32)
    lst = np.concatenate([index[::-1], index[:40], np.array([m.size, m.size + 7, 0xFFFFFFFF], np.uint32)])
    got = _empty().drive(LO, dims, [seed], members=lst, step=0, fields=ALL[:3])
    want = D.yardstick(m, [seed], members=lst, step=0)
    D.assert_same(got, want, "a list with duplicates and strays")
    assert got["n_members"] == 289 and (got["of_member"][-3:] == D.NONE).all() and (got["of_member"][:-3] != D.NONE).all()
    # seeds: none, non-members, out of range, twice
    for seeds, n_seeded in (([], 0), ([D.flat(dims, 8, 8, 2), m.size, 0xFFFFFFFF], 0), ([seed, seed, D.flat(dims, 8, 8, 4)], 1)):
        y = _both(m, np.array(seeds, np.uint32), targets=[seed], what=("seeds", seeds), step=0)
        assert y["n_seeded"] == n_seeded and y["n_reached"] == (289 if n_seeded else 0)
    y = _both(np.zeros(dims, bool), [seed], targets=[seed], what="no members")
    assert y["n_members"] == 0 and (y["cost"] == D.NONE).all() and (y["parent"] == 255).all()
    # snap: the member lies exactly snap below the seed, or one further
    tall = (3, 3, 40)
    for snap in (0, 1, 32):
        col = np.zeros(tall, bool)
        col[:, :, 2] = True
        at, beyond = D.flat(tall, 1, 1, 2 + snap), D.flat(tall, 1, 1, 3 + snap)
        y = _both(col, [at], targets=[at, beyond, D.flat(tall, 0, 0, 1), col.size], what=("snap", snap), snap=snap, step=0)
        assert y["n_seeded"] == 1 and y["target_index"].tolist() == [D.flat(tall, 1, 1, 2), D.NONE, D.NONE, D.NONE]
        assert y["target_cost"].tolist() == [0, D.NONE, D.NONE, D.NONE]
        assert _both(col, [beyond], what=("snap, one further", snap), snap=snap, step=0)["n_seeded"] == 0
    # every subset of outputs, and what the wrapper refuses itself
    for fields in ((), ("cost",), ("parent",), ("of_member",), ("cost", "parent", "of_member", "target_index")):
        t = [seed] if "cost" not in fields and "of_member" not in fields else None
        if t is None and "target_index" in fields:
            t = [seed]
        got = _empty().drive(LO, dims, [seed], members=index, targets=t, step=0, fields=fields)
        assert set(got) == set(fields) | ({"target_cost"} if t is not None else set()) | set(D.STATS) | {"rounds", "brick_runs", "capped"} | set(R.INFO_FIELDS)
        D.assert_same(got, D.yardstick(m, [seed], targets=t, members=index, step=0), ("fields", fields))
    with pytest.raises(ValueError):
        _empty().drive(LO, dims, [seed], members=index, fields=("steps",))
    with pytest.raises(ValueError):
        _empty().drive(LO, dims, [seed], members=index, move_cost=(1, 2, 3))


def test_refusals_in_the_contracts_order(built):
    """every refusal of the contract in its order, each with every later defect present; nothing is written; the limit values
    are served"""
    from la3dm_amd import _lib
    M, m = _lib.maplib(), _empty()
    held, rooms = [], {}

    def put(a):
        held.append(np.ascontiguousarray(a))
        return held[-1].ctypes.data

    def room(name, n, dtype):
        rooms[name] = np.full(n, 0x5A, dtype)
        return rooms[name].ctypes.data

    def call(lo, dims, seeds, n_seeds, p, targets, n_targets, out):
        rc = M.la3dm_map_drive(m._h, lo, dims, seeds, n_seeds, C.byref(p) if p is not None else None, targets, n_targets,
                               C.byref(out) if out is not None else None, None, None)
        return rc, M.la3dm_map_last_error().decode()
    serve, member, index, seeds, targets, kw, keep = D.refusal_chain(call, put, room)
    assert all((a == 0x5A).all() for a in rooms.values())
    rc, msg = serve()
    assert rc == 0, msg
    want = D.yardstick(member, seeds, targets=targets, **kw)
    got = dict(cost=rooms["cost"].reshape(member.shape), parent=rooms["parent"].reshape(member.shape), target_cost=rooms["target_cost"],
               target_index=rooms["target_index"])
    D.assert_same(got, want, "the limit values", D.FIELDS)
    assert (rooms["of_member"] == 0x5A).all() and want["n_reached"] > 1
    # the Python wrapper raises the library's text
    with pytest.raises(Exception, match="both NULL"):
        m.drive(LO, (4, 4, 4), [0])
    with pytest.raises(Exception, match="both set"):
        m.drive(LO, (4, 4, 4), [0], members=[0], footing=dict())


# ---- footing's hand-built scene ------------------------------------------------------------------------------------------------
_SCENE = {}


def _scene():
    if not _SCENE:
        import la3dm_amd
        params = dict(R.YAML, block_depth=4)
        _SCENE["m"] = la3dm_amd.BGKOctoMap(**params, device=-1).unpack(F.scene_stream(params))
    return _SCENE["m"]


def test_scene_named_voxels(built):
    m = _scene()
    D.scene_named_voxels([m])
    assert m.mirror_syncs() == 0


# ---- region_cases.fused_map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [3, 4])
def test_recipe_against_the_yardstick(built, depth):
    """region_cases.fused_map over the recipe region: the input conditions counted from the yardstick first, then footing mode
    == list mode == yardstick over the region and over a sub-region touching each of its faces"""
    m, lv, lo = R.fused_map(depth)
    dims = R.RECIPE_DIMS
    slo, foot, seeds, targets = D.recipe_case(m, lv, lo, dims)
    y = D.yardstick(foot, seeds, targets=targets, **D.RECIPE_KW)
    D.assert_exercises_the_feature(D.input_conditions(y), {k: v // 2 for k, v in D.RECIPE_COUNTED[depth].items()})
    D.recipe_queries([m], slo, foot, seeds, targets, ("recipe", depth))
    reached = np.flatnonzero((y["cost"] != D.NONE).reshape(-1))
    for t in reached[::max(1, reached.size // 25)]:
        D.walk(y, foot, dims, t, 8, 1, (10, 14), 5, 2)
    for offset, sub in D.FACE_BOXES:
        assert all(o + s <= d for o, s, d in zip(offset, sub, dims)) and any(o == 0 or o + s == d for o, s, d in zip(offset, sub, dims))
        D.recipe_queries([m], *D.recipe_case(m, lv, lo, dims, offset, sub), ("face box", depth, offset, sub))
    assert m.mirror_syncs() == 0


def test_empty_map(built):
    """an empty map is served: list mode as any other map, footing mode with no member"""
    m, dims = _empty(), (9, 9, 9)
    got = m.drive(LO, dims, [0, 40], footing=dict(support=F.OCC_M, clear=F.OPTIMISTIC, headroom=2), targets=[0, 800], snap=3,
                  fields=("cost", "parent", "target_index"))
    assert got["n_members"] == got["n_seeded"] == got["n_reached"] == got["max_cost"] == 0
    assert (got["cost"] == D.NONE).all() and (got["parent"] == 255).all() and (got["target_cost"] == D.NONE).all() and (got["target_index"] == D.NONE).all()
    got = m.drive(LO, dims, [0], members=np.zeros(0, np.uint32), fields=("cost",))       # n_members = 0 is served
    assert got["n_members"] == 0 and (got["cost"] == D.NONE).all()
    _both(D.random_members(dims, 5, 0.7), [0, 40, 400], targets=[1, 2, 3], what="list mode on the empty map", snap=2, step=2)


@pytest.mark.parametrize("variant", ["GPOctoMap", "BGKLOctoMap", "BGKLVOctoMap"])
def test_other_classes(built, variant):
    """the other three map classes loaded from the scene's stream (UNCERTAIN where BGK has UNKNOWN on BGK-LV): footing mode ==
    list mode == yardstick across the kerb and up the step"""
    import la3dm_amd
    yaml = {"GPOctoMap": la3dm_amd.GP_YAML, "BGKLOctoMap": la3dm_amd.L_YAML, "BGKLVOctoMap": la3dm_amd.LV_YAML}[variant]
    params = dict(yaml, block_depth=4, resolution=0.1)
    swap = {R.UNKNOWN: R.UNCERTAIN} if variant == "BGKLVOctoMap" else None
    m = getattr(la3dm_amd, variant)(**params, device=-1).unpack(F.scene_stream(params, variant, swap))
    f = lambda i, j, k: D.flat(F.SCENE_DIMS, i, j, k)   # noqa: E731
    for step in (0, 1, 2):
        y, _ = D.scene_query([m], F.FREE_M, 3, 0, 0, 0, [f(7, 12, 4)], [f(13, 12, 3), f(19, 4, 5)], step=step, snap=2, climb_up=4, climb_down=1)
        assert (y["target_cost"] != D.NONE).tolist() == [step >= 1, step >= 2]
