"""score_paths on a host-mode map (device = -1, no GPU): many polylines walked through the distance field of a region,
compared with an independent yardstick (tests/helpers/paths_cases.py: the waypoint voxels by the anchor arithmetic of
region_cases.anchor vectorised, the walk by numpy's cumsum, searchsorted and floor_divide, scipy's exact distance transform
of region_cases.yardstick's classes).  Every output is an integer: every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import distance_cases as D  # noqa: E402
import paths_cases as P  # noqa: E402
import region_cases as R  # noqa: E402
import score_cases as S  # noqa: E402

_RECIPES = {}


def _recipe(depth):
    """(map, leaves, recipe lo, the recipe region's origin, the recipe paths)"""
    if depth not in _RECIPES:
        m, lv, lo = R.fused_map(depth)
        _, _, _, origin = R.anchor(lo, m.get_resolution(), depth)
        _RECIPES[depth] = (m, lv, lo, origin, P.recipe_paths(m, lv, lo, R.RECIPE_DIMS))
    return _RECIPES[depth]


def _regions(m, lo, origin):
    return [(lo, P.REGIONS[0])] + [(S.small_lo(m, origin), d) for d in P.REGIONS[1:]]


@pytest.mark.parametrize("depth", [3, 4])
def test_recipe_exercises_the_feature(built, depth):
    """CPU test 0: the input conditions, counted from the yardstick alone"""
    m, lv, lo, _, paths = _recipe(depth)
    P.assert_exercises_the_feature(P.input_conditions(m, lv, lo, R.RECIPE_DIMS, paths))


@pytest.mark.parametrize("depth", [3, 4])
def test_host_form_equals_the_yardstick(built, depth):
    """CPU test 1: the recipe's kind of path set on the three regions, clearance x soft_radius in {0, 1, 8}^2 with OCCUPIED
    obstacles, two of them with OCCUPIED | UNKNOWN | MISSING as well, max_steps 64 and 4096"""
    m, lv, lo, origin, _ = _recipe(depth)
    kinds = np.zeros(5, np.int64)
    for rlo, dims in _regions(m, lo, origin):
        paths = P.recipe_paths(m, lv, rlo, dims)
        for cl in P.RADII:
            for sr in P.RADII:
                for mask in (D.MASKS[0], D.MASKS[2]) if (cl, sr) in ((0, 0), (1, 8)) else (D.MASKS[0],):
                    p = P.params(mask=mask, clearance=cl, soft_radius=sr, penalty=50 if sr else 0, max_steps=64 if cl != 8 else 4096)
                    want = P.yardstick(m, lv, rlo, dims, paths, p)
                    got = P.call(m, rlo, dims, paths, p)
                    assert set(got) == set(P.FIELDS) | set(R.INFO_FIELDS)
                    assert all(got[k].dtype == P.DTYPES[k] and got[k].shape == (paths.shape[0],) for k in P.FIELDS)
                    P.assert_same(got, want, (depth, dims, cl, sr, mask))
                    kinds += [int((want["flags"] == f).sum()) for f in (0, P.BLOCKED, P.LEFT, P.TRUNCATED, P.INVALID)]
        print(f"depth {depth} dims {dims}: cost {want['cost'][:8].tolist()} flags {want['flags'][:12].tolist()}")
    assert (kinds > 0).all(), kinds
    # the defaults are OCCUPIED, no clearance, no penalty, 10 / 14 / 17 and 4096 steps; names select the same masks; fields
    paths = _recipe(depth)[4]
    want = P.yardstick(m, lv, lo, R.RECIPE_DIMS, paths, P.params())
    P.assert_same(m.score_paths(lo, R.RECIPE_DIMS, paths), want, "defaults")
    only = m.score_paths(lo, R.RECIPE_DIMS, paths, fields="flags")
    assert set(only) == {"cost", "flags"} | set(R.INFO_FIELDS) and (only["cost"] == want["cost"]).all() and (only["flags"] == want["flags"]).all()
    names = m.score_paths(lo, R.RECIPE_DIMS, paths, obstacles=("occupied", "unknown", "missing"), clearance=1, soft_radius=3, penalty=7,
                          move_cost=(1, 2, 3), max_steps=33)
    P.assert_same(names, P.yardstick(m, lv, lo, R.RECIPE_DIMS, paths, P.params(D.MASKS[2], 1, 3, 7, (1, 2, 3), 33)), "names")
    R.assert_same(names, m.box(lo, R.RECIPE_DIMS, fields=()), ("origin", "cell"), "info")
    assert m.mirror_syncs() == 0


def _chain(parent, dims, index):
    import la3dm_amd
    return np.stack(np.unravel_index(la3dm_amd.follow_parents(parent, dims, index), dims), 1)


@pytest.mark.parametrize("depth", [3, 4])
def test_exact_algebra(built, depth):
    """CPU test 2: a one-waypoint path on a voxel centre returns distance_field's word there (BLOCKED at 0 where that word is
    within the clearance); the reversed waypoint list gives the same cost, steps and min_d2 for an unstopped path with no
    penalty; the chain of travel's parents, walked from the seed to a target, costs cost[target] with flags 0 and steps =
    the chain's length — and the same walked from the target with no penalty"""
    m, lv, lo, origin, paths = _recipe(depth)
    res = m.get_resolution()
    dims = R.RECIPE_DIMS
    # one waypoint per path: every voxel of a small region
    slo, sd = S.small_lo(m, origin), (3, 5, 7)
    _, _, _, so = R.anchor(slo, res, depth)
    c = S.centres(so, sd, res)[:, None, :]
    for cl, radius in ((0, 1), (2, 2), (8, 8)):
        d2 = m.distance_field(slo, sd, obstacles=D.MASKS[0], radius=radius, fields=("d2",))["d2"].reshape(-1)
        got = m.score_paths(slo, sd, c, clearance=cl)
        blocked = (d2 != D.FAR) & (d2 <= cl * cl)
        assert (got["flags"] == np.where(blocked, P.BLOCKED, 0)).all() and (got["min_d2"] == np.where(blocked, D.FAR, d2)).all()
        assert (got["steps"] == ~blocked).all() and (got["ways"] == ~blocked).all() and (got["cost"] == 0).all()
        assert (got["stop"] == np.where(blocked, 0, P.NONE)).all()
    # reversed waypoints
    kw = dict(clearance=1, max_steps=4096)
    fwd, back = m.score_paths(lo, dims, paths, **kw), m.score_paths(lo, dims, paths[:, ::-1], **kw)
    free = fwd["flags"] == 0
    assert free.sum() >= 4 and (back["flags"][free] == 0).all()
    for k in ("cost", "steps", "min_d2", "ways"):
        assert (fwd[k][free] == back[k][free]).all(), k
    # travel's parents
    a, _ = P.open_voxel(m, lv, lo, dims)
    seed = int(np.ravel_multi_index(tuple(a), dims))
    for cl, sr, pn, mc in ((0, 0, 0, (10, 14, 17)), (1, 4, 60, (10, 14, 17)), (2, 0, 0, (1, 1, 1)), (0, 6, 1000, (3, 5, 9))):
        tkw = dict(obstacles=("occupied",), clearance=cl, soft_radius=sr, penalty=pn, move_cost=mc)
        t = m.travel(lo, dims, [seed], passable=("free", "unknown", "missing"), connectivity=26, fields=("cost", "parent"), **tkw)
        assert t["n_seeded"] == 1 and t["n_reached"] > 1000
        cost = t["cost"].reshape(-1).astype(np.int64)
        reached = np.nonzero(cost != 0xFFFFFFFF)[0]
        order = reached[np.argsort(cost[reached], kind="stable")]
        targets = [int(order[-1]), int(order[len(order) // 2]), int(order[len(order) // 7]), seed]
        chains = [_chain(t["parent"], dims, i)[::-1] for i in targets]                       # seed first
        n_way = max(ch.shape[0] for ch in chains)
        assert 8 < n_way <= 1024
        ways = P.padded([P.centre(origin, ch, res) for ch in chains], n_way)
        got = m.score_paths(lo, dims, ways, max_steps=4096, **tkw)
        assert (got["cost"] == cost[targets]).all() and (got["flags"] == 0).all(), (cl, sr, got, cost[targets])
        assert got["steps"].tolist() == [ch.shape[0] for ch in chains] and (got["ways"] == n_way).all()
        if sr == 0:
            back = m.score_paths(lo, dims, P.padded([P.centre(origin, ch[::-1], res) for ch in chains], n_way), max_steps=4096, **tkw)
            assert (back["cost"] == cost[targets]).all() and (back["flags"] == 0).all()
        print(f"depth {depth} clearance {cl} soft {sr}: chains of {[ch.shape[0] for ch in chains]} voxels cost {cost[targets].tolist()}")
    assert m.mirror_syncs() == 0


def test_edges(built):
    """CPU test 3: duplicate waypoints at the start, in the middle, at the end and all equal change nothing but `ways`;
    leaving through each of the six faces stops at the first voxel outside; a start outside is LEFT at 0 with steps 0; NaN,
    inf and 1e12 in each coordinate make the path INVALID and leave its neighbours alone, also in a waypoint beyond a stop;
    max_steps = T, T - 1 and 1"""
    m, lv, lo, origin, _ = _recipe(3)
    res = m.get_resolution()
    dims = (3, 5, 7)
    slo = S.small_lo(m, origin)
    _, _, _, so = R.anchor(slo, res, 3)
    c = lambda *ijk: P.centre(so, ijk, res)   # noqa: E731
    q = lambda rows, n_way, **kw: m.score_paths(slo, dims, P.padded(rows, n_way), obstacles=0x10, **kw)   # noqa: E731  (no voxel is UNCERTAIN: nothing blocks)
    a, b, d = c(0, 0, 0), c(2, 4, 6), c(2, 0, 0)
    plain = q([[a, b, d]], 3)
    assert plain["steps"][0] == 6 + 6 + 1 and plain["flags"][0] == 0 and plain["ways"][0] == 3 and plain["min_d2"][0] == D.FAR
    assert plain["cost"][0] == 6 * 14 + 4 * 14 + 2 * 10       # a -> b: z moves every step and x or y with it; b -> d: y rests twice
    P.assert_same(plain, P.yardstick(m, lv, slo, dims, P.padded([[a, b, d]], 3), P.params(mask=0x10)), "plain")
    for rows, ways in (([a, a, a, b, d], 5), ([a, b, b, b, d], 5), ([a, b, d, d, d], 5), ([a, a, b, b, d], 5)):
        got = q([rows], 5)
        assert got["ways"][0] == ways and all(got[k][0] == plain[k][0] for k in ("cost", "steps", "stop", "min_d2", "flags")), rows
    same = q([[b, b, b, b]], 4)
    assert same["steps"][0] == 1 and same["cost"][0] == 0 and same["ways"][0] == 4 and same["flags"][0] == 0 and same["stop"][0] == P.NONE
    mid = np.array((1, 2, 3))
    for axis in range(3):
        for at in (-1, dims[axis]):
            out = mid.copy()
            out[axis] = at + (2 if at > 0 else -2)
            got = q([[c(*mid), c(*out)]], 2)
            n_in = abs(at - mid[axis])                                                # voxels inside, the start included
            assert got["flags"][0] == P.LEFT and got["stop"][0] == n_in and got["steps"][0] == n_in and got["ways"][0] == 1, (axis, at, got)
            assert got["cost"][0] == 10 * (n_in - 1)
    got = q([[c(-1, 0, 0), a], [c(0, 0, 7), a], [c(3, 5, 7), c(4, 6, 8)]], 2)
    assert (got["flags"] == P.LEFT).all() and (got["stop"] == 0).all() and (got["steps"] == 0).all() and (got["ways"] == 0).all()
    assert (got["cost"] == 0).all() and (got["min_d2"] == D.FAR).all()
    # invalid coordinates, one by one, in a waypoint before and after the stop of a path that leaves the region
    leaving = [c(*mid), c(1, 2, 9), c(1, 2, 3)]
    alone = q([[a, b, d], leaving, [a, b, d]], 3)
    assert alone["flags"].tolist() == [0, P.LEFT, 0]
    for bad in (np.nan, np.inf, -np.inf, 1.0e12, -1.0e12, 1.1e8):
        for k in range(3):
            for axis in range(3):
                rows = [np.array(w, np.float32) for w in leaving]
                rows[k][axis] = bad
                got = q([[a, b, d], rows, [a, b, d]], 3)
                assert got["flags"].tolist() == [0, P.INVALID, 0], (bad, k, axis, got)
                assert [int(got[f][1]) for f in ("cost", "steps", "stop", "min_d2", "ways")] == [0, 0, P.NONE, D.FAR, 0]
                for f in P.FIELDS:
                    assert got[f][0] == alone[f][0] and got[f][2] == alone[f][2]
    assert q([[np.array((1.0e8, 0, 0), np.float32), a]], 2)["flags"][0] == P.LEFT     # |w / res| < 2^30: a voxel, not in the region
    # max_steps against T = 12
    for max_steps, flags, steps, ways in ((12, 0, 13, 3), (11, P.TRUNCATED, 12, 2), (1, P.TRUNCATED, 2, 1), (6, P.TRUNCATED, 7, 2), (5, P.TRUNCATED, 6, 1)):
        got = q([[a, b, d]], 3, max_steps=max_steps)
        assert (got["flags"][0], got["steps"][0], got["ways"][0], got["stop"][0]) == (flags, steps, ways, P.NONE), (max_steps, got)
    # a stop at ordinal E is a stop, not a truncation
    got = q([[c(*mid), c(1, 2, 9)]], 2, max_steps=4)
    assert got["flags"][0] == P.LEFT and got["stop"][0] == 4
    got = q([[c(*mid), c(1, 2, 9)]], 2, max_steps=3)
    assert got["flags"][0] == P.TRUNCATED and got["steps"][0] == 4


def test_trivial_cases_and_the_empty_map(built):
    """CPU test 4: n_paths = 0 is served and writes nothing; an empty map answers from the definition: with the mask's bit 3
    every voxel of the region is an obstacle (BLOCKED at 0 where the start is inside), without it nothing blocks"""
    import la3dm_amd
    m, lv, lo, origin, paths = _recipe(3)
    z = m.score_paths(lo, (6, 5, 4), np.zeros((0, 4, 3), np.float32))
    assert all(z[k].shape == (0,) for k in P.FIELDS)
    empty = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
    full = m.score_paths(lo, R.RECIPE_DIMS, paths, obstacles=0x1F, max_steps=64)                 # every voxel an obstacle
    with_missing = empty.score_paths(lo, R.RECIPE_DIMS, paths, obstacles=("occupied", "missing"), clearance=3, max_steps=64)
    P.assert_same(with_missing, full, "empty map, bit 3")
    assert set(full["flags"].tolist()) == {P.BLOCKED, P.LEFT, P.INVALID} and (full["steps"] == 0).all()
    without = empty.score_paths(lo, R.RECIPE_DIMS, paths, obstacles="occupied", clearance=3, soft_radius=5, penalty=9, max_steps=64)
    nothing = m.score_paths(lo, R.RECIPE_DIMS, paths, obstacles=0x10, max_steps=64)              # no voxel is UNCERTAIN
    P.assert_same(without, nothing, "empty map, no bit 3")
    assert (without["min_d2"] == D.FAR).all() and P.BLOCKED not in without["flags"].tolist() and int((without["flags"] == 0).sum()) > 0
    R.assert_same(without, m.box(lo, R.RECIPE_DIMS, fields=()), ("origin", "cell"))


def test_refusals_in_their_order(built):
    """CPU test 5: every refusal raises with a text that names the argument and leaves the outputs alone; a call that
    breaks several rules is answered by the first of the contract's order"""
    from la3dm_amd import _lib
    m, lv, lo, origin, paths = _recipe(3)
    q = lambda **kw: m.score_paths(kw.pop("lo", lo), kw.pop("dims", (4, 4, 4)), kw.pop("paths", paths), **kw)   # noqa: E731
    for mask in (0, 0x20, 0x3F, 1 << 31, ()):
        with pytest.raises(RuntimeError, match="obstacle_mask must hold"):
            q(obstacles=mask)
    for kw, text in ((dict(clearance=1025), r"clearance must not exceed LA3DM_DF_MAX_RADIUS \(1024\)"),
                     (dict(soft_radius=1025, penalty=1), r"soft_radius must not exceed LA3DM_DF_MAX_RADIUS \(1024\)"),
                     (dict(soft_radius=1), "penalty must be >= 1 with soft_radius > 0"),
                     (dict(penalty=(1 << 16) + 1), r"penalty must not exceed LA3DM_TRAVEL_MAX_PENALTY \(2\^16\)"),
                     (dict(move_cost=(0, 1, 1)), "move_cost: every entry"), (dict(move_cost=(1, 1, (1 << 16) + 1)), "move_cost: every entry"),
                     (dict(max_steps=0), r"max_steps must lie in \[1, LA3DM_PATHS_MAX_STEPS \(2\^20\)\]"),
                     (dict(max_steps=(1 << 20) + 1), "max_steps must lie in"),
                     (dict(paths=np.zeros((2, 0, 3), np.float32)), r"n_way must lie in \[1, LA3DM_PATHS_MAX_WAY \(1024\)\]"),
                     (dict(paths=np.zeros((1, 1025, 3), np.float32)), "n_way must lie in"),
                     (dict(lo=(np.nan, 0, 0)), "lo must be finite"), (dict(lo=(0, 0, 1.1e8)), "lo must be finite"),
                     (dict(dims=(2, 0, 2)), "dims must be >= 1"), (dict(lo=(-3.0e5, 0, 0)), "lo: the block field leaves"),
                     (dict(lo=(2.09e5, 0, 0), dims=(1 << 16, 1, 1)), "dims: the region's block fields leave"),
                     (dict(dims=((1 << 28) + 1, 1, 1)), r"LA3DM_DF_MAX_CELLS \(2\^28\)"), (dict(dims=(0xFFFFFFFF,) * 3), "LA3DM_DF_MAX_CELLS")):
        with pytest.raises(RuntimeError, match=text):
            q(**kw)
    assert q(clearance=1024, soft_radius=1024, penalty=1 << 16, move_cost=(1 << 16,) * 3, max_steps=1 << 20)["cost"].shape == (paths.shape[0],)
    with pytest.raises(ValueError, match="unknown fields"):
        q(fields=("cost", "cls"))
    with pytest.raises(ValueError, match=r"\(P, W, 3\)"):
        q(paths=np.zeros((4, 12), np.float32))
    # the limits, the NULL pointers and the order, through the C view: no pointer is followed before the checks have passed
    M = _lib.maplib()
    lo3 = np.ascontiguousarray(lo, np.float32)
    w = np.ascontiguousarray(paths)
    n, n_way = w.shape[0], w.shape[1]
    sent = {k: np.full(n + 8, 7, P.DTYPES[k]) for k in P.FIELDS}
    ptrs = lambda **kw: _lib.PathsOut(*[kw.get(k, sent[k].ctypes.data) for k, _ in _lib.PathsOut._fields_])   # noqa: E731
    out = ptrs()

    def c_call(lo_p=lo3.ctypes.data, dims=(4, 4, 4), with_dims=True, w_p=w.ctypes.data, n=n, n_way=n_way, o=C.byref(out), with_params=True,
               mask=0x2, clearance=0, soft_radius=0, penalty=0, move_cost=(10, 14, 17), max_steps=64):
        d3 = np.array(dims, np.uint32)
        prm = _lib.PathsParams(mask, clearance, soft_radius, penalty, (C.c_uint32 * 3)(*move_cost), max_steps)
        rc = M.la3dm_map_score_paths(m._h, lo_p, d3.ctypes.data if with_dims else None, w_p, n, n_way, C.byref(prm) if with_params else None, o, None)
        return rc, M.la3dm_map_last_error().decode()
    over = dict(dims=((1 << 28) + 1, 1, 1))
    rest = dict(lo_p=None, w_p=None, o=None, **over)
    for kw, text in ((dict(with_params=False), "params is NULL"), (dict(mask=0), "obstacle_mask"), (dict(mask=0x40), "obstacle_mask"),
                     (dict(clearance=1025), "clearance must not exceed"), (dict(soft_radius=1025, penalty=1), "soft_radius must not exceed"),
                     (dict(soft_radius=2), "penalty must be >= 1"), (dict(penalty=1 << 17), "penalty must not exceed"),
                     (dict(move_cost=(1, 0, 1)), "move_cost"), (dict(max_steps=0), "max_steps must lie in"),
                     (dict(n_way=0), "n_way must lie in"), (dict(n_way=1025, n=1), "n_way must lie in"),
                     (dict(n=(1 << 20) + 1, n_way=1), "LA3DM_PATHS_MAX_PATHS (2^20)"), (dict(n=1 << 20, n_way=65), "LA3DM_PATHS_MAX_WAYPOINTS (2^26)"),
                     (dict(n=(1 << 16) + 1, n_way=1024), "LA3DM_PATHS_MAX_WAYPOINTS (2^26)"),
                     (dict(w_p=None), "ways3 is NULL"), (dict(o=None), "cost must not be NULL"), (dict(o=C.byref(ptrs(cost=None))), "cost must not be NULL"),
                     (dict(lo_p=None), "lo is NULL"), (dict(with_dims=False), "dims is NULL"), (dict(dims=(4, 0, 4)), "dims must be >= 1"),
                     (dict(over), "LA3DM_DF_MAX_CELLS"),
                     # the order: each call breaks the rule named and every later one
                     (dict(with_params=False, n_way=0, n=1 << 21, **rest), "params is NULL"),
                     (dict(mask=0, clearance=2000, soft_radius=2000, penalty=1 << 20, move_cost=(0, 0, 0), max_steps=0, n_way=0, n=1 << 21, **rest), "obstacle_mask"),
                     (dict(clearance=2000, soft_radius=2000, penalty=1 << 20, move_cost=(0, 0, 0), max_steps=0, n_way=0, n=1 << 21, **rest), "clearance must not"),
                     (dict(soft_radius=2000, penalty=1 << 20, move_cost=(0, 0, 0), max_steps=0, n_way=0, n=1 << 21, **rest), "soft_radius must not"),
                     (dict(soft_radius=2, penalty=0, move_cost=(0, 0, 0), max_steps=0, n_way=0, n=1 << 21, **rest), "penalty must be >= 1"),
                     (dict(penalty=1 << 20, move_cost=(0, 0, 0), max_steps=0, n_way=0, n=1 << 21, **rest), "penalty must not exceed"),
                     (dict(move_cost=(0, 0, 0), max_steps=0, n_way=0, n=1 << 21, **rest), "move_cost"),
                     (dict(max_steps=0, n_way=0, n=1 << 21, **rest), "max_steps must lie in"), (dict(n_way=0, n=1 << 21, **rest), "n_way must lie in"),
                     (dict(n_way=1024, n=1 << 21, **rest), "LA3DM_PATHS_MAX_PATHS"), (dict(n_way=1024, n=1 << 20, **rest), "LA3DM_PATHS_MAX_WAYPOINTS"),
                     (dict(**rest), "ways3 is NULL"), (dict(lo_p=None, o=None, **over), "cost must not be NULL"),
                     (dict(lo_p=None, **over), "lo is NULL"), (dict(**over), "LA3DM_DF_MAX_CELLS")):
        rc, txt = c_call(**kw)
        assert rc < 0 and text in txt and "score_paths" in txt, (kw, txt)
    assert all((sent[k] == 7).all() for k in sent)
    rc, txt = c_call(n=1 << 16, n_way=1024, w_p=None)                            # at the limits: 2^26 waypoints pass the counts
    assert rc < 0 and "ways3 is NULL" in txt, txt
    rc, txt = c_call(n=0, w_p=None, o=None)                                      # n_paths = 0: served, nothing written or read
    assert rc == 0 and all((sent[k] == 7).all() for k in sent), txt
    want = m.score_paths(lo, (4, 4, 4), paths, max_steps=64)
    for leave_out in (None,) + P.FIELDS[1:]:                                     # each optional output left out
        for k in sent:
            sent[k][...] = 7
        rc, txt = c_call(o=C.byref(ptrs(**({leave_out: None} if leave_out else {}))))
        assert rc == 0, txt
        for k in P.FIELDS:
            assert (sent[k][n:] == 7).all() and (sent[k][:n] == (7 if k == leave_out else want[k])).all(), (leave_out, k)
    assert m.mirror_syncs() == 0
