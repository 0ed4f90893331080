"""reach on a host-mode map (device = -1, no GPU): hop distances from seed voxels through the passable voxels of a region,
against an independent numpy wave (tests/helpers/reach_cases.py) over the classes of region_cases.yardstick, and against
closed forms on the empty map.  The answer is integer and unique: every comparison is exact."""
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
import reach_cases as Q  # noqa: E402

DIMS = R.RECIPE_DIMS
SEED = Q.flat(Q.SEED, DIMS)


def _recipe(depth):
    m, lv, lo = R.fused_map(depth)
    return m, lo, R.yardstick(m, lv, lo, DIMS)


@pytest.mark.parametrize("depth", [3, 4])
def test_recipe_against_the_yardstick(built, depth):
    """CPU test 1: the recipe region from the sensor's voxel, every connectivity, the four pass / clearance pairs: steps,
    n_seeded, n_reached, levels and the info; the input conditions are counted from the yardstick first"""
    import la3dm_amd
    m, lo, y = _recipe(depth)
    assert y["cls"][Q.SEED] == R.FREE
    Q.assert_exercises_the_feature(Q.input_conditions(y["cls"], SEED, la3dm_amd.REACH_BATCH))
    for pass_mask, clearance in Q.PAIRS:
        for c in Q.CONNECTIVITIES:
            want = Q.yardstick(y["cls"], [SEED], pass_mask, Q.OCC_M, clearance, c)
            got = m.reach(lo, DIMS, [SEED], passable=pass_mask, obstacles=Q.OCC_M, clearance=clearance, connectivity=c)
            assert set(got) == {"steps"} | set(Q.STATS) | set(R.INFO_FIELDS)
            assert got["steps"].dtype == np.uint32 and got["steps"].shape == DIMS
            Q.assert_same(got, want, (depth, pass_mask, clearance, c))
            R.assert_same(got, y, ("origin", "cell"), "info")
            assert got["block_key"] == y["block_key"]
            print(f"depth {depth} pass {pass_mask:#x} clearance {clearance} connectivity {c}: reached {want['n_reached']} levels {want['levels']}")
    # names select the same masks; the defaults are FREE, no clearance, connectivity 6
    Q.assert_same(m.reach(lo, DIMS, [SEED]), Q.yardstick(y["cls"], [SEED], Q.FREE_M), "defaults")
    Q.assert_same(m.reach(lo, DIMS, [SEED], passable=("free", "unknown"), obstacles="occupied", clearance=2, connectivity=26),
                  Q.yardstick(y["cls"], [SEED], Q.FREE_M | Q.UNK_M, Q.OCC_M, 2, 26), "names")
    assert m.mirror_syncs() == 0


def test_closed_forms_on_the_empty_map(built):
    """CPU test 2: pass = MISSING on a map without blocks is an open box: sum |d| at connectivity 6, max |d| at 26,
    max(max |d|, ceil(sum |d| / 2)) at 18; two seeds give the pointwise minimum; without bit 3 nothing is reached"""
    import la3dm_amd
    empty = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
    lo = R.recipe_lo()
    for dims in Q.OPEN_BOXES:
        n = int(np.prod(dims))
        forms = {}
        for seed in Q.corner_seeds(dims):
            for c in Q.CONNECTIVITIES:
                want = Q.closed_form(dims, seed, c)
                forms[seed, c] = want
                got = empty.reach(lo, dims, [Q.flat(seed, dims)], passable=Q.MISS_M, connectivity=c)
                assert (got["steps"] == want).all(), (dims, seed, c)
                assert got["n_seeded"] == 1 and got["n_reached"] == n and got["levels"] == int(want.max()), (dims, seed, c, got["levels"])
        a, b = Q.corner_seeds(dims)[0], Q.corner_seeds(dims)[2]
        for c in Q.CONNECTIVITIES:
            got = empty.reach(lo, dims, [Q.flat(a, dims), Q.flat(b, dims)], passable=Q.MISS_M | Q.FREE_M, connectivity=c)
            assert (got["steps"] == np.minimum(forms[a, c], forms[b, c])).all(), (dims, c)
            assert got["n_seeded"] == (1 if a == b else 2)
        # a clearance on the empty map: MISSING as an obstacle closes the box, any other obstacle class leaves it open
        got = empty.reach(lo, dims, [0], passable=Q.MISS_M, obstacles=Q.OCC_M, clearance=2)
        assert (got["steps"] == forms[(0, 0, 0), 6]).all()
        got = empty.reach(lo, dims, [0], passable=Q.MISS_M, obstacles=Q.MISS_M, clearance=2)
        assert (got["steps"] == Q.NONE).all() and got["n_seeded"] == got["n_reached"] == got["levels"] == 0
        got = empty.reach(lo, dims, [0], passable=0x17)
        assert (got["steps"] == Q.NONE).all() and got["n_seeded"] == got["n_reached"] == got["levels"] == 0
    assert empty.mirror_syncs() == 0


def test_algebra_on_the_recipe(built):
    """CPU test 3, exact: max_steps cuts the full answer; steps 6 >= 18 >= 26 and the reached sets are nested; reached
    neighbours differ by at most 1; seeds that are impassable, out of range or listed twice are ignored; targets gather the
    steps; finite steps with a clearance imply a FAR distance field"""
    m, lo, y = _recipe(3)
    n = int(np.prod(DIMS))
    full = {c: m.reach(lo, DIMS, [SEED], clearance=2, connectivity=c) for c in Q.CONNECTIVITIES}
    for c in (6, 26):
        for k in (1, 31, 32, 33, 60):
            got = m.reach(lo, DIMS, [SEED], clearance=2, connectivity=c, max_steps=k)
            assert (got["steps"] == np.where(full[c]["steps"] <= k, full[c]["steps"], Q.NONE)).all(), (c, k)
            assert got["levels"] == min(k, full[c]["levels"]) and got["n_reached"] == int((full[c]["steps"] <= k).sum()), (c, k)
    s6, s18, s26 = (full[c]["steps"].astype(np.int64) for c in Q.CONNECTIVITIES)
    f6, f18, f26 = s6 != Q.NONE, s18 != Q.NONE, s26 != Q.NONE
    assert (f18 | ~f6).all() and (f26 | ~f18).all() and f6.sum() < f26.sum()
    assert (s6[f6] >= s18[f6]).all() and (s18[f18] >= s26[f18]).all() and (s6[f6] > s26[f6]).any()
    for c, s in zip(Q.CONNECTIVITIES, (s6, s18, s26)):
        fin = s != Q.NONE
        for di, dj, dk in Q.F.offsets(c):
            if (di, dj, dk) < (0, 0, 0):
                continue
            a = s[max(di, 0):DIMS[0] + min(di, 0), max(dj, 0):DIMS[1] + min(dj, 0), max(dk, 0):DIMS[2] + min(dk, 0)]
            b = s[max(-di, 0):DIMS[0] + min(-di, 0), max(-dj, 0):DIMS[1] + min(-dj, 0), max(-dk, 0):DIMS[2] + min(-dk, 0)]
            both = (a != Q.NONE) & (b != Q.NONE)
            assert (np.abs(a[both] - b[both]) <= 1).all(), (c, di, dj, dk)
        assert fin.sum() == full[c]["n_reached"]
    # seeds: an OCCUPIED voxel, indices out of range and a voxel listed three times change nothing
    occ = int(np.flatnonzero(y["cls"].reshape(-1) == R.OCCUPIED)[0])
    got = m.reach(lo, DIMS, [occ, SEED, n, SEED, 0xFFFFFFFF, SEED, n + 5], clearance=2)
    Q.assert_same(got, full[6], "ignored seeds")
    assert got["n_seeded"] == 1
    got = m.reach(lo, DIMS, [occ, n])
    assert got["n_seeded"] == got["n_reached"] == got["levels"] == 0 and (got["steps"] == Q.NONE).all()
    got = m.reach(lo, DIMS, [])
    assert got["n_seeded"] == got["n_reached"] == got["levels"] == 0 and (got["steps"] == Q.NONE).all()
    other = int(np.flatnonzero((s6 > 40) & f6)[0])
    two = m.reach(lo, DIMS, [SEED, other], clearance=2)
    alone = m.reach(lo, DIMS, [other], clearance=2)
    assert two["n_seeded"] == 2 and (two["steps"] == np.minimum(full[6]["steps"], alone["steps"])).all()
    # targets
    rng = np.random.default_rng(5)
    targets = np.concatenate([rng.integers(0, n, 500), [n, n + 1, 0xFFFFFFFF, SEED, 0, n - 1]]).astype(np.uint32)
    got = m.reach(lo, DIMS, [SEED], clearance=2, targets=targets)
    want_t = np.where(targets < n, full[6]["steps"].reshape(-1)[np.minimum(targets, n - 1)], Q.NONE).astype(np.uint32)
    assert got["target_steps"].dtype == np.uint32 and (got["target_steps"] == want_t).all() and (got["steps"] == full[6]["steps"]).all()
    assert (want_t != Q.NONE).any() and (want_t[:500] == Q.NONE).any()
    only = m.reach(lo, DIMS, [SEED], clearance=2, targets=targets, fields=())
    assert "steps" not in only and (only["target_steps"] == want_t).all() and all(only[k] == full[6][k] for k in Q.STATS)
    # finite steps with clearance r imply d2 == FAR at radius r
    for r in (1, 2, 3):
        g = m.reach(lo, DIMS, [SEED], clearance=r, connectivity=26)
        d2 = m.distance_field(lo, DIMS, obstacles=("occupied",), radius=r, fields=("d2",))["d2"]
        assert g["n_reached"] > 100 and (d2[g["steps"] != Q.NONE] == 0xFFFFFFFF).all(), r


def test_c_view_refusals_header_and_example(built):
    """CPU test 4: every refused argument with its name in the text and nothing written; the C view through ctypes; the
    headers declare and the libraries export the new symbols; the example program on a host-mode (empty) map"""
    import la3dm_amd
    from la3dm_amd import _lib
    m, lo, y = _recipe(3)
    q = m.reach
    for mask in (0, 0x20, 0x3F, 1 << 31, ()):
        with pytest.raises(RuntimeError, match="pass_mask must hold"):
            q(lo, (2, 2, 2), [0], passable=mask)
    for mask in (0x20, 0x3F, 1 << 31):
        with pytest.raises(RuntimeError, match="obstacle_mask must hold"):
            q(lo, (2, 2, 2), [0], obstacles=mask)
    with pytest.raises(RuntimeError, match="obstacle_mask must hold"):
        q(lo, (2, 2, 2), [0], obstacles=(), clearance=1)
    assert q(lo, (2, 2, 2), [0], obstacles=(), clearance=0)["n_seeded"] <= 1          # ignored without a clearance
    with pytest.raises(RuntimeError, match="clearance must not exceed LA3DM_DF_MAX_RADIUS"):
        q(lo, (2, 2, 2), [0], clearance=1025)
    for c in (0, 4, 8, 27, 1 << 20):
        with pytest.raises(RuntimeError, match="connectivity must be 6, 18 or 26"):
            q(lo, (2, 2, 2), [0], connectivity=c)
    for k in (0, (1 << 16) + 1, 0xFFFFFFFF):
        with pytest.raises(RuntimeError, match="max_steps must lie in"):
            q(lo, (2, 2, 2), [0], max_steps=k)
    assert q(lo, (2, 2, 2), [0], max_steps=1 << 16, clearance=1024, passable=0x1F, obstacles=0x1F)["levels"] == 0   # the limits are served
    with pytest.raises(RuntimeError, match="LA3DM_REACH_MAX_SEEDS"):
        q(lo, (2, 2, 2), np.zeros((1 << 20) + 1, np.uint32))
    with pytest.raises(RuntimeError, match="steps or out.target_steps must not be NULL"):
        q(lo, (2, 2, 2), [0], fields=())
    with pytest.raises(RuntimeError, match="steps or out.target_steps must not be NULL"):
        q(lo, (2, 2, 2), [0], fields=(), targets=[])
    assert q(lo, (2, 2, 2), [0], targets=[])["target_steps"].size == 0
    with pytest.raises(ValueError, match="unknown fields"):
        q(lo, (2, 2, 2), [0], fields=("steps", "cls"))
    # the region's own checks follow, with frontier's limits under reach's names
    for bad in ((np.nan, 0, 0), (0, np.inf, 0)):
        with pytest.raises(RuntimeError, match="lo must be finite"):
            q(bad, (2, 2, 2), [0])
    with pytest.raises(RuntimeError, match="dims must be >= 1"):
        q(lo, (2, 0, 2), [0])
    with pytest.raises(RuntimeError, match="padded by one voxel"):
        q((-209715.5, 0.0, 0.0), (2, 2, 2), [0])
    for dims in (((1 << 28) - 1, 1, 1), (1 << 10, 1 << 10, (1 << 8) - 1), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)):
        with pytest.raises(RuntimeError, match="LA3DM_REACH_MAX_CELLS"):
            q(lo, dims, [0])
    # the C view: refusals leave every buffer and the stats alone
    M = _lib.maplib()
    lo3 = np.ascontiguousarray(lo, np.float32)
    seeds, targets = np.array([SEED], np.uint32), np.array([SEED, 5, 0xFFFFFFFF], np.uint32)
    steps, tsteps = np.full(DIMS, 7, np.uint32), np.full(3, 7, np.uint32)
    stats = _lib.ReachStats(77, 77, 77)
    out = _lib.ReachOut(steps.ctypes.data, tsteps.ctypes.data)

    def c_call(dims=DIMS, sp=seeds.ctypes.data, ns=1, pm=1, om=2, cl=2, c=6, ms=1 << 16, tp=targets.ctypes.data, nt=3, o=C.byref(out),
               lo_p=lo3.ctypes.data):
        d3 = np.array(dims, np.uint32)
        rc = M.la3dm_map_reach(m._h, lo_p, d3.ctypes.data, sp, ns, pm, om, cl, c, ms, tp, nt, o, C.byref(stats), None)
        return rc, M.la3dm_map_last_error().decode()
    over = ((1 << 10) - 2, (1 << 10) - 2, (1 << 8) - 1)             # padded: above 2^28
    for kw, text in ((dict(pm=0), "pass_mask"), (dict(pm=0x40), "pass_mask"), (dict(om=0x20), "obstacle_mask"), (dict(om=0), "obstacle_mask"),
                     (dict(cl=1025), "clearance"), (dict(c=7), "connectivity"), (dict(ms=0), "max_steps"), (dict(ms=(1 << 16) + 1), "max_steps"),
                     (dict(ns=(1 << 20) + 1), "n_seeds"), (dict(nt=(1 << 28) + 1), "n_targets"), (dict(sp=None), "seeds is NULL"),
                     (dict(tp=None), "targets is NULL"), (dict(o=None), "out is NULL"),
                     (dict(o=C.byref(_lib.ReachOut(None, None)), nt=0), "steps or out.target_steps must not be NULL"),
                     (dict(nt=0), "target_steps is set with n_targets = 0"),
                     (dict(o=C.byref(_lib.ReachOut(steps.ctypes.data, None))), "target_steps must not be NULL with n_targets > 0"),
                     # reach's own checks come before the region's: a bad mask answers whatever the region is
                     (dict(pm=0, dims=(0, 1, 1), lo_p=None), "pass_mask"), (dict(o=None, dims=over), "out is NULL"),
                     (dict(lo_p=None), "lo is NULL"), (dict(dims=(4, 0, 4)), "dims must be >= 1"), (dict(dims=over), "LA3DM_REACH_MAX_CELLS")):
        rc, txt = c_call(**kw)
        assert rc < 0 and text in txt, (kw, txt)
    assert (steps == 7).all() and (tsteps == 7).all() and (stats.n_seeded, stats.n_reached, stats.levels) == (77, 77, 77)
    # served: steps and targets, targets alone, steps alone with no targets
    want = Q.yardstick(y["cls"], [SEED], Q.FREE_M, Q.OCC_M, 2, 6, targets=targets)
    rc, txt = c_call()
    assert rc == 0, txt
    assert (steps == want["steps"]).all() and (tsteps == want["target_steps"]).all() and tsteps[0] == 0 and tsteps[2] == Q.NONE
    assert (stats.n_seeded, stats.n_reached, stats.levels) == tuple(want[k] for k in Q.STATS)
    steps[:], tsteps[:] = 7, 7
    rc, txt = c_call(o=C.byref(_lib.ReachOut(None, tsteps.ctypes.data)))
    assert rc == 0 and (tsteps == want["target_steps"]).all() and (steps == 7).all(), txt
    tsteps[:] = 7
    rc, txt = c_call(o=C.byref(_lib.ReachOut(steps.ctypes.data, None)), tp=None, nt=0)
    assert rc == 0 and (steps == want["steps"]).all() and (tsteps == 7).all(), txt
    rc, txt = c_call(sp=None, ns=0)                                   # no seed is served: nothing is reachable
    assert rc == 0 and (steps == Q.NONE).all() and (tsteps == Q.NONE).all() and stats.n_seeded == stats.n_reached == stats.levels == 0
    # headers, exports, constants
    for header, so, names in (("la3dm_map.h", _lib.MAP_SO, ("la3dm_map_reach",)),
                              ("la3dm_hip.h", _lib.HIP_SO, ("la3dm_devmap_reach_host", "la3dm_devmap_reach_device"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        if so == _lib.MAP_SO:
            C.CDLL(_lib.HIP_SO, mode=C.RTLD_GLOBAL)
        lib = C.CDLL(so)
        for name in names:
            assert re.search(r"\b" + name + r"\s*\(", txt), name
            assert hasattr(lib, name), name
            assert name in _lib.HIP_SYMBOLS + _lib.MAP_SYMBOLS, name
    hip_h = open(os.path.join(ROOT, "include", "la3dm_hip.h")).read()
    assert "la3dm_reach_out" in hip_h and "la3dm_reach_stats" in hip_h and "corner cutting" in hip_h.lower()
    for name, text, value in (("REACH_MAX_CELLS", r"\(1u << 28\)", 1 << 28), ("REACH_MAX_STEPS", r"\(1u << 16\)", 1 << 16),
                              ("REACH_MAX_SEEDS", r"\(1u << 20\)", 1 << 20), ("REACH_BATCH", "32", 32), ("REACH_NONE", "0xFFFFFFFFu", Q.NONE)):
        assert re.search(r"#define\s+LA3DM_" + name + r"\s+" + text, hip_h), name
        assert getattr(la3dm_amd, name) == value, name
    exe = os.path.join(ROOT, "examples", "reachable_goals")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "0"] +
                       "0.1 3 1.0 0.2 0.5 0.1 8.0 0.3 0.7 100.0 0.001 0.001 -1".split(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("reach 128 x 128 x 16 from "), r.stdout
    assert lines[0].endswith("found 0 reachable 0 levels 0 mirror_syncs 0 device_resident 0"), r.stdout
