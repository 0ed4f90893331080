"""travel on a host-mode map (device = -1, no GPU): least path costs and parents from seed voxels through the passable
voxels of a region, against an independent numpy yardstick (tests/helpers/travel_cases.py: Jacobi sweeps over the classes
of region_cases.yardstick and scipy's distance transform), against reach at unit weights, and against closed forms on the
empty map.  The answer is integer and unique: every comparison is exact."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import travel_cases as T  # noqa: E402

DIMS = R.RECIPE_DIMS
SEED = T.flat(T.SEED, DIMS)
FIELDS = ("cost", "parent")
_RECIPES = {}


def _recipe(depth):
    if depth not in _RECIPES:
        m, lv, lo = R.fused_map(depth)
        _RECIPES[depth] = (m, lo, R.yardstick(m, lv, lo, DIMS))
    return _RECIPES[depth]


@pytest.mark.parametrize("connectivity", T.CONNECTIVITIES)
@pytest.mark.parametrize("depth", [3, 4])
def test_recipe_against_the_yardstick(built, depth, connectivity):
    """CPU test 1: the recipe region from the sensor's voxel; weights 1/1/1, 10/14/17 and 5/7/9, without and with
    clearance 1, soft radius 4 and penalty 40: cost, parent, target_cost, n_seeded, n_reached, max_cost and the info; 1/1/1
    equals reach's steps; the input conditions are counted from the yardstick first"""
    m, lo, y = _recipe(depth)
    T.assert_exercises_the_feature(T.input_conditions(y["cls"], SEED, key=depth))
    rng = np.random.default_rng(7)
    targets = np.concatenate([rng.integers(0, y["cls"].size, 300), [y["cls"].size, 0xFFFFFFFF, SEED]]).astype(np.uint32)
    for weights in T.WEIGHTS:
        for kw in (T.PLAIN, T.SOFT):
            want = T.yardstick(y["cls"], [SEED], connectivity=connectivity, move_cost=weights, targets=targets, key=depth, **kw)
            got = m.travel(lo, DIMS, [SEED], connectivity=connectivity, move_cost=weights, targets=targets, fields=FIELDS, **kw)
            assert set(got) == {"cost", "parent", "target_cost", "rounds", "brick_runs", "capped"} | set(T.STATS) | set(R.INFO_FIELDS)
            assert got["cost"].dtype == np.uint32 and got["cost"].shape == DIMS and got["parent"].dtype == np.uint8 and got["parent"].shape == DIMS
            T.assert_same(got, want, (depth, connectivity, weights, kw))
            assert got["rounds"] == got["brick_runs"] == got["capped"] == 0          # the host form has no rounds
            R.assert_same(got, y, ("origin", "cell"), "info")
            assert got["block_key"] == y["block_key"]
            print(f"depth {depth} connectivity {connectivity} weights {weights} {kw}: reached {want['n_reached']} max_cost {want['max_cost']} sweeps {want['sweeps']}")
            if weights == (1, 1, 1):
                steps = m.reach(lo, DIMS, [SEED], clearance=kw["clearance"], connectivity=connectivity)["steps"]
                if kw["soft_radius"] == 0:
                    assert (got["cost"] == steps).all(), (depth, connectivity)
                else:                                    # the same passable set; the penalty only raises costs
                    assert ((got["cost"] == T.NONE) == (steps == T.NONE)).all() and (got["cost"] >= steps).all()
    assert m.mirror_syncs() == 0


def test_defaults_and_names(built):
    """the defaults are FREE, OCCUPIED, no clearance, no penalty, 10/14/17 at connectivity 26; names select the same masks"""
    m, lo, y = _recipe(3)
    T.assert_same(m.travel(lo, DIMS, [SEED]), T.yardstick(y["cls"], [SEED]), "defaults", fields=("cost",) + T.STATS)
    got = m.travel(lo, DIMS, [SEED], passable=("free", "unknown"), obstacles="occupied", clearance=2, soft_radius=3, penalty=9, connectivity=18,
                   fields=FIELDS)
    T.assert_same(got, T.yardstick(y["cls"], [SEED], T.FREE_M | T.UNK_M, T.OCC_M, 2, 3, 9, connectivity=18), "names")


def test_closed_forms_on_the_empty_map(built):
    """CPU test 2: pass = MISSING on a map without blocks is an open box: with |d| sorted x >= y >= z the cost is
    c z + b (y - z) + a (x - y) at connectivity 26 and a (x + y + z) at connectivity 6; two seeds give the pointwise minimum;
    MISSING as an obstacle closes the box (clearance) or charges the full penalty everywhere (soft radius alone)"""
    import la3dm_amd
    empty = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
    lo = R.recipe_lo()
    for dims in T.RC.OPEN_BOXES:
        n = int(np.prod(dims))
        corners = T.RC.corner_seeds(dims)
        forms = {}
        for seed in corners:
            for c, weights in ((26, (10, 14, 17)), (26, (5, 7, 9)), (6, (10, 14, 17)), (6, (3, 1, 1))):
                want = T.closed_form(dims, seed, c, weights)
                forms[seed, c, weights] = want
                got = empty.travel(lo, dims, [T.flat(seed, dims)], passable=T.MISS_M, connectivity=c, move_cost=weights, fields=FIELDS)
                assert (got["cost"] == want).all(), (dims, seed, c, weights)
                assert got["n_seeded"] == 1 and got["n_reached"] == n and got["max_cost"] == int(want.max()), (dims, seed, c)
                assert got["parent"].reshape(-1)[T.flat(seed, dims)] == 13 and (got["parent"] != 255).all()
        a, b = corners[0], corners[2]
        for c in (6, 26):
            got = empty.travel(lo, dims, [T.flat(a, dims), T.flat(b, dims)], passable=T.MISS_M | T.FREE_M, connectivity=c)
            assert (got["cost"] == np.minimum(forms[a, c, (10, 14, 17)], forms[b, c, (10, 14, 17)])).all(), (dims, c)
            assert got["n_seeded"] == (1 if a == b else 2)
        got = empty.travel(lo, dims, [0], passable=T.MISS_M, obstacles=T.OCC_M, clearance=2, soft_radius=3, penalty=50, connectivity=6)
        assert (got["cost"] == forms[(0, 0, 0), 6, (10, 14, 17)]).all()
        got = empty.travel(lo, dims, [0], passable=T.MISS_M, obstacles=T.MISS_M, clearance=2)
        assert (got["cost"] == T.NONE).all() and got["n_seeded"] == got["n_reached"] == got["max_cost"] == 0
        got = empty.travel(lo, dims, [0], passable=T.MISS_M, obstacles=T.MISS_M, soft_radius=2, penalty=50, connectivity=6, move_cost=(10, 10, 10))
        steps = T.closed_form(dims, (0, 0, 0), 6, (1, 1, 1))
        assert (got["cost"] == steps * 60).all()             # every voxel is an obstacle: d2 = 0, the whole penalty; the seed's own is not charged
        got = empty.travel(lo, dims, [0], passable=0x17, fields=FIELDS)
        assert (got["cost"] == T.NONE).all() and (got["parent"] == 255).all() and got["n_seeded"] == got["n_reached"] == got["max_cost"] == 0
    assert empty.mirror_syncs() == 0


def test_brick_model_agrees_with_the_sweeps():
    """the helper's model of the device scheme gives the costs of the plain sweeps — seeds on the faces, edges and corners of
    bricks, partial bricks, corner-cheap weights — so what it counts (rounds, capped runs) is counted on the right answer"""
    for dims, seed, c, weights in (((15, 1, 1), (7, 0, 0), 6, (10, 14, 17)), ((1, 17, 1), (0, 8, 0), 26, (10, 14, 17)), ((17, 17, 17), (8, 8, 8), 26, (10, 14, 3)),
                                   ((17, 17, 17), (7, 7, 7), 18, (5, 7, 9)), ((9, 16, 3), (8, 15, 0), 26, (10, 14, 3)), ((24, 9, 8), (0, 0, 0), 6, (1, 1, 1))):
        ok, pen = np.ones(dims, bool), np.zeros(dims, np.int64)
        ok[dims[0] // 2, dims[1] // 3:, :dims[2] // 2] = False            # a partial wall
        ok[seed] = True
        s = [T.flat(seed, dims)]
        want, sweeps = T.jacobi(ok, pen, s, c, weights, 1 << 31)
        m = T.brick_model(ok, pen, s, c, weights)
        assert (m["cost"] == want).all() and (want != T.INF).sum() == ok.sum(), (dims, seed, c)
        assert 1 <= m["rounds"] <= sweeps and m["brick_runs"] >= m["rounds"], (dims, m["rounds"], sweeps)


def test_algebra_on_the_recipe(built):
    """CPU test 3, exact: max_cost cuts the full answer; following parent from every reached target ends at the seed, the
    cost falls at every step and the moves and penalties along the way sum to the target's cost; with equal move costs
    cost 6 >= 18 >= 26; seeds that are impassable, out of range or listed twice are ignored; follow_parents agrees"""
    import la3dm_amd
    m, lo, y = _recipe(3)
    n = int(np.prod(DIMS))
    kw = dict(T.SOFT)
    full = m.travel(lo, DIMS, [SEED], fields=FIELDS, **kw)
    assert full["n_reached"] > 7000
    for cut in (1, 9, 10, 17, 500, full["max_cost"] - 1, full["max_cost"], 1 << 31):
        got = m.travel(lo, DIMS, [SEED], max_cost=cut, fields=FIELDS, **kw)
        keep = full["cost"] <= cut
        assert (got["cost"] == np.where(keep, full["cost"], T.NONE)).all(), cut
        assert (got["parent"] == np.where(keep, full["parent"], 255)).all(), cut
        assert got["n_reached"] == int(keep.sum()) and got["max_cost"] == int(full["cost"][keep].max()), cut
    # paths: the parents of every reached target lead to the seed and account for the cost
    pen = T.entry_of(y["cls"], T.FREE_M, T.OCC_M, **kw)[1].reshape(-1)
    cost = full["cost"].reshape(-1)
    rng = np.random.default_rng(11)
    reached = np.flatnonzero(cost != T.NONE)
    for f in np.concatenate([rng.choice(reached, 200), reached[np.argsort(cost[reached])[-3:]]]):
        path = T.walk(full["parent"], DIMS, f)
        assert path[-1][0] == SEED
        total = 0
        for (v, q), (u, _) in zip(path[:-1], path[1:]):
            assert cost[u] < cost[v]
            total += (10, 14, 17)[sum(1 for d in (q // 9 - 1, (q // 3) % 3 - 1, q % 3 - 1) if d) - 1] + int(pen[v])
        assert total == int(cost[f]), (f, total, cost[f])
        assert (la3dm_amd.follow_parents(full["parent"], DIMS, f) == [v for v, _ in path]).all()
    unreached = int(np.flatnonzero(cost == T.NONE)[0])
    assert la3dm_amd.follow_parents(full["parent"], DIMS, unreached).size == 0
    # equal move costs: more offsets can only help
    c6, c18, c26 = (m.travel(lo, DIMS, [SEED], connectivity=c, move_cost=(7, 7, 7), **kw)["cost"].astype(np.int64) for c in T.CONNECTIVITIES)
    assert (c6 >= c18).all() and (c18 >= c26).all() and (c6 > c26).any()
    # seeds: an OCCUPIED voxel, indices out of range and a voxel listed three times change nothing
    occ = int(np.flatnonzero(y["cls"].reshape(-1) == R.OCCUPIED)[0])
    got = m.travel(lo, DIMS, [occ, SEED, n, SEED, 0xFFFFFFFF, SEED, n + 5], fields=FIELDS, **kw)
    T.assert_same(got, full, "ignored seeds")
    assert got["n_seeded"] == 1
    for seeds in ([occ, n], []):
        got = m.travel(lo, DIMS, seeds, fields=FIELDS)
        assert got["n_seeded"] == got["n_reached"] == got["max_cost"] == 0 and (got["cost"] == T.NONE).all() and (got["parent"] == 255).all()
    other = int(reached[np.argsort(cost[reached])[-1]])
    two = m.travel(lo, DIMS, [SEED, other], **kw)
    alone = m.travel(lo, DIMS, [other], **kw)
    assert two["n_seeded"] == 2 and (two["cost"] == np.minimum(full["cost"], alone["cost"])).all()
    # targets alone
    targets = np.concatenate([rng.integers(0, n, 500), [n, n + 1, 0xFFFFFFFF, SEED, 0, n - 1]]).astype(np.uint32)
    want_t = np.where(targets < n, cost[np.minimum(targets, n - 1)], T.NONE).astype(np.uint32)
    only = m.travel(lo, DIMS, [SEED], targets=targets, fields=(), **kw)
    assert "cost" not in only and "parent" not in only and (only["target_cost"] == want_t).all() and all(only[k] == full[k] for k in T.STATS)
    assert (want_t != T.NONE).any() and (want_t[:500] == T.NONE).any()


def test_c_view_refusals_header_and_example(built):
    """CPU test 4: every refused argument with its name in the text and nothing written; the C view through ctypes; the
    headers declare and the libraries export the new symbols; the constants; the example program on a host-mode (empty) map"""
    import la3dm_amd
    from la3dm_amd import _lib
    m, lo, y = _recipe(3)
    q = m.travel
    small = (2, 2, 2)
    for mask in (0, 0x20, 0x3F, 1 << 31, ()):
        with pytest.raises(RuntimeError, match="pass_mask must hold"):
            q(lo, small, [0], passable=mask)
    for mask in (0x20, 0x3F, 1 << 31):
        with pytest.raises(RuntimeError, match="obstacle_mask must hold"):
            q(lo, small, [0], obstacles=mask)
    for kw in (dict(clearance=1), dict(soft_radius=1, penalty=1)):
        with pytest.raises(RuntimeError, match="obstacle_mask must hold"):
            q(lo, small, [0], obstacles=(), **kw)
    assert q(lo, small, [0], obstacles=())["n_seeded"] <= 1                              # ignored when R = 0
    with pytest.raises(RuntimeError, match="clearance must not exceed LA3DM_DF_MAX_RADIUS"):
        q(lo, small, [0], clearance=1025)
    with pytest.raises(RuntimeError, match="soft_radius must not exceed LA3DM_DF_MAX_RADIUS"):
        q(lo, small, [0], soft_radius=1025, penalty=1)
    with pytest.raises(RuntimeError, match="penalty must be >= 1 with soft_radius > 0"):
        q(lo, small, [0], soft_radius=2)
    with pytest.raises(RuntimeError, match="penalty must not exceed LA3DM_TRAVEL_MAX_PENALTY"):
        q(lo, small, [0], soft_radius=2, penalty=(1 << 16) + 1)
    for moves in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, (1 << 16) + 1)):
        with pytest.raises(RuntimeError, match="move_cost: every entry must lie in"):
            q(lo, small, [0], move_cost=moves)
    for c in (0, 4, 8, 27, 1 << 20):
        with pytest.raises(RuntimeError, match="connectivity must be 6, 18 or 26"):
            q(lo, small, [0], connectivity=c)
    for k in (0, (1 << 31) + 1, 0xFFFFFFFF):
        with pytest.raises(RuntimeError, match="max_cost must lie in"):
            q(lo, small, [0], max_cost=k)
    served = q(lo, small, [0], max_cost=1 << 31, clearance=1024, soft_radius=1024, penalty=1 << 16, move_cost=(1 << 16,) * 3, passable=0x1F, obstacles=0x1F)
    assert served["max_cost"] == 0 and served["n_reached"] == 0                          # the limits are served (every voxel is an obstacle)
    with pytest.raises(RuntimeError, match="LA3DM_TRAVEL_MAX_SEEDS"):
        q(lo, small, np.zeros((1 << 20) + 1, np.uint32))
    for kw in (dict(fields=()), dict(fields=(), targets=[]), dict(fields=("parent",))):          # parent alone is not enough
        with pytest.raises(RuntimeError, match="cost or out.target_cost must not be NULL"):
            q(lo, small, [0], **kw)
    assert q(lo, small, [0], targets=[])["target_cost"].size == 0
    with pytest.raises(ValueError, match="unknown fields"):
        q(lo, small, [0], fields=("cost", "cls"))
    for bad in ((np.nan, 0, 0), (0, np.inf, 0)):
        with pytest.raises(RuntimeError, match="lo must be finite"):
            q(bad, small, [0])
    with pytest.raises(RuntimeError, match="dims must be >= 1"):
        q(lo, (2, 0, 2), [0])
    # the cell limit counts whole bricks: 2^25 + 1 voxels in a line are 2^22 + 1 bricks of 512 cells
    for dims in (((1 << 28) - 7, 1, 1), ((1 << 22) + 1, 1, 1), (1, 1, (1 << 22) + 1), (1 << 10, 1 << 10, (1 << 8) + 1), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)):
        with pytest.raises(RuntimeError, match="LA3DM_TRAVEL_MAX_CELLS"):
            q(lo, dims, [0])
    # the C view: refusals leave every buffer and the stats alone
    M = _lib.maplib()
    lo3 = np.ascontiguousarray(lo, np.float32)
    seeds, targets = np.array([SEED], np.uint32), np.array([SEED, 5, 0xFFFFFFFF], np.uint32)
    cost, parent, tcost = np.full(DIMS, 7, np.uint32), np.full(DIMS, 7, np.uint8), np.full(3, 7, np.uint32)
    stats = _lib.TravelStats(77, 77, 77, 77, 77, 77)
    out = _lib.TravelOut(cost.ctypes.data, tcost.ctypes.data, parent.ctypes.data)

    def c_call(dims=DIMS, sp=seeds.ctypes.data, ns=1, tp=targets.ctypes.data, nt=3, o=C.byref(out), lo_p=lo3.ctypes.data, no_params=False, **kw):
        d3 = np.array(dims, np.uint32)
        p = dict(pm=1, om=2, cl=1, sr=4, pen=40, mv=(10, 14, 17), c=26, mc=1 << 31)
        p.update(kw)
        params = _lib.TravelParams(p["pm"], p["om"], p["cl"], p["sr"], p["pen"], (C.c_uint32 * 3)(*p["mv"]), p["c"], p["mc"])
        rc = M.la3dm_map_travel(m._h, lo_p, d3.ctypes.data, sp, ns, None if no_params else C.byref(params), tp, nt, o, C.byref(stats), None)
        return rc, M.la3dm_map_last_error().decode()
    over = (1 << 10, 1 << 10, (1 << 8) + 1)             # whole bricks: above 2^28
    for kw, text in ((dict(no_params=True), "params is NULL"), (dict(pm=0), "pass_mask"), (dict(pm=0x40), "pass_mask"), (dict(om=0x20), "obstacle_mask"),
                     (dict(om=0), "obstacle_mask"), (dict(cl=1025), "clearance"), (dict(sr=1025), "soft_radius"), (dict(pen=0), "penalty"),
                     (dict(pen=(1 << 16) + 1), "penalty"), (dict(mv=(10, 0, 17)), "move_cost"), (dict(mv=(10, 14, 1 << 17)), "move_cost"),
                     (dict(c=7), "connectivity"), (dict(mc=0), "max_cost"), (dict(mc=(1 << 31) + 1), "max_cost"),
                     (dict(ns=(1 << 20) + 1), "n_seeds"), (dict(nt=(1 << 28) + 1), "n_targets"), (dict(sp=None), "seeds is NULL"),
                     (dict(tp=None), "targets is NULL"), (dict(o=None), "out is NULL"),
                     (dict(o=C.byref(_lib.TravelOut(None, None, parent.ctypes.data)), nt=0), "cost or out.target_cost must not be NULL"),
                     (dict(nt=0), "target_cost is set with n_targets = 0"),
                     (dict(o=C.byref(_lib.TravelOut(cost.ctypes.data, None, None))), "target_cost must not be NULL with n_targets > 0"),
                     # travel's own checks come before the region's: a bad mask answers whatever the region is
                     (dict(pm=0, dims=(0, 1, 1), lo_p=None), "pass_mask"), (dict(pm=0, o=None), "pass_mask"), (dict(o=None, dims=over), "out is NULL"),
                     (dict(lo_p=None), "lo is NULL"), (dict(dims=(4, 0, 4)), "dims must be >= 1"), (dict(dims=over), "LA3DM_TRAVEL_MAX_CELLS")):
        rc, txt = c_call(**kw)
        assert rc < 0 and text in txt, (kw, txt)
    assert (cost == 7).all() and (parent == 7).all() and (tcost == 7).all()
    assert [getattr(stats, k) for k, _ in stats._fields_] == [77] * 6
    # served: everything, targets alone, cost alone with no targets
    want = T.yardstick(y["cls"], [SEED], targets=targets, **T.SOFT)
    rc, txt = c_call()
    assert rc == 0, txt
    assert (cost == want["cost"]).all() and (parent == want["parent"]).all() and (tcost == want["target_cost"]).all() and tcost[0] == 0 and tcost[2] == T.NONE
    assert (stats.n_seeded, stats.n_reached, stats.max_cost) == tuple(want[k] for k in T.STATS)
    assert (stats.rounds, stats.brick_runs, stats.capped) == (0, 0, 0)
    cost[:], parent[:], tcost[:] = 7, 7, 7
    rc, txt = c_call(o=C.byref(_lib.TravelOut(None, tcost.ctypes.data, None)))
    assert rc == 0 and (tcost == want["target_cost"]).all() and (cost == 7).all() and (parent == 7).all(), txt
    tcost[:] = 7
    rc, txt = c_call(o=C.byref(_lib.TravelOut(cost.ctypes.data, None, None)), tp=None, nt=0)
    assert rc == 0 and (cost == want["cost"]).all() and (tcost == 7).all() and (parent == 7).all(), txt
    rc, txt = c_call(sp=None, ns=0)                                   # no seed is served: nothing is reachable
    assert rc == 0 and (cost == T.NONE).all() and (parent == 255).all() and (tcost == T.NONE).all() and stats.n_seeded == stats.n_reached == stats.max_cost == 0
    # headers, exports, constants
    for header, so, names in (("la3dm_map.h", _lib.MAP_SO, ("la3dm_map_travel",)),
                              ("la3dm_hip.h", _lib.HIP_SO, ("la3dm_devmap_travel_host", "la3dm_devmap_travel_device"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        if so == _lib.MAP_SO:
            C.CDLL(_lib.HIP_SO, mode=C.RTLD_GLOBAL)
        lib = C.CDLL(so)
        for name in names:
            assert re.search(r"\b" + name + r"\s*\(", txt), name
            assert hasattr(lib, name), name
            assert name in _lib.HIP_SYMBOLS + _lib.MAP_SYMBOLS, name
    hip_h = open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
    assert all(name in hip_h for name in ("la3dm_travel_params", "la3dm_travel_out", "la3dm_travel_stats"))
    for name, text, value in (("TRAVEL_MAX_CELLS", r"\(1u << 28\)", 1 << 28), ("TRAVEL_MAX_COST", r"\(1u << 31\)", 1 << 31),
                              ("TRAVEL_MAX_MOVE", r"\(1u << 16\)", 1 << 16), ("TRAVEL_MAX_PENALTY", r"\(1u << 16\)", 1 << 16),
                              ("TRAVEL_MAX_SEEDS", r"\(1u << 20\)", 1 << 20), ("TRAVEL_MAX_ROUNDS", r"\(1u << 16\)", 1 << 16),
                              ("TRAVEL_BRICK", "8", T.BRICK), ("TRAVEL_INNER", "16", T.INNER), ("TRAVEL_BATCH", "8", T.BATCH),
                              ("TRAVEL_NONE", "0xFFFFFFFFu", T.NONE)):
        assert re.search(r"#define\s+LA3DM_" + name + r"\s+" + text + r"\s*$", hip_h, flags=re.M), name
        assert getattr(la3dm_amd, name) == value, name
    exe = os.path.join(ROOT, "examples", "route")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "0"] +
                       "0.1 3 1.0 0.2 0.5 0.1 8.0 0.3 0.7 100.0 0.001 0.001 -1".split(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("route 128 x 128 x 16 from "), r.stdout
    assert lines[0].endswith("found 0 reachable 0 max_cost 0 mirror_syncs 0 device_resident 0"), r.stdout
