"""Every map query on hand-built pools at block_depth 1 to 5, on host-mode maps (device = -1, no GPU): pins
tests/helpers/pool_cases.py — the numpy expander from pool arrays to the classes of a region — and the host forms of the
queries at the depths, tilings and key ranges tests/test_pool_queries_gpu.py runs on the device.  The pool comes from
pack_cases (random tilings, a block collapsed to its root, one sibling group collapsed, an un-pruned block, a fifth of the
blocks left out, BGK-LV's UNCERTAIN leaves), is loaded with unpack, and every query is compared with its class-array
yardstick on the expander's classes.  Every comparison is exact (floats by their bits)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import pack_cases as P  # noqa: E402
import pool_cases as PC  # noqa: E402
import pool_checks as Q  # noqa: E402

_MAPS = {}


def _map(case):
    """the case and its host-mode map, loaded once"""
    import la3dm_amd
    if case not in _MAPS:
        c = PC.case(*case)
        _MAPS[case] = (c, getattr(la3dm_amd, c["name"])(**c["params"], device=-1).unpack(c["stream"]))
    return _MAPS[case]


cases = pytest.mark.parametrize("case", PC.CASES, ids=PC.CASE_IDS)


@cases
def test_the_case_exercises_the_feature(built, case):
    """the input conditions, counted from the expander alone; the forced blocks are what they are meant to be"""
    c, m = _map(case)
    depth, notes = c["depth"], c["notes"]
    PC.assert_exercises_the_feature(PC.input_conditions(c["cls"], c["leaf_depth"], c["g0"], depth, PC.variant_classes(c["name"])), case)
    assert m.block_count() == c["keys"].size and not m.is_device_resident()
    lim, npb = 1 << (depth - 1), P.npb_of(depth)
    mask = P.leaf_mask(c["S"], depth)
    row = {k: int(np.flatnonzero(c["keys"] == PC.key_of(notes[k]))[0]) for k in ("root", "group", "full")}
    assert mask[row["root"], 0] and mask[row["root"]].sum() == 1
    assert mask[row["full"]].sum() == 8 ** (depth - 1)
    if depth >= 2:
        assert mask[row["group"]].sum() == 8 ** (depth - 1) - 7 and mask[row["group"], P.base(depth - 2):P.base(depth - 1)].sum() == 1
    gone = set(int(k) for k in PC.key_of(notes["left_out"]))
    beside = [int(PC.key_of(notes["root"] + np.array(step))) for step in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    assert gone.isdisjoint(int(k) for k in c["keys"]) and any(k in gone for k in beside)
    assert (PC.fields_of(c["keys"]).min(0) < PC.ZERO).all() and (PC.fields_of(c["keys"]).max(0) >= PC.ZERO).all()
    assert npb == c["S"].shape[1] and lim * PC.nbx_of(depth) >= 24


@cases
def test_box_columns_and_leaves(built, case):
    c, m = _map(case)
    Q.box_and_columns(m, c)
    if c["name"] != "BGKLVOctoMap":                      # (a BGK-LV map's leaves() lists the blocks its scans touched)
        Q.leaves(m, c)


@cases
def test_distance_and_nearest(built, case):
    c, m = _map(case)
    Q.distance(m, c)
    Q.nearest(m, c)


@cases
def test_frontier(built, case):
    c, m = _map(case)
    Q.frontier(m, c)


@cases
def test_reach(built, case):
    c, m = _map(case)
    Q.reach(m, c)


@cases
def test_travel(built, case):
    c, m = _map(case)
    Q.travel(m, c)


@cases
def test_clusters(built, case):
    c, m = _map(case)
    Q.clusters(m, c)


@cases
def test_footing_and_surface(built, case):
    c, m = _map(case)
    Q.footing(m, c)
    Q.surface(m, c)


@cases
def test_rays_and_gain(built, case):
    """the host loop of raycast_many against the closed form and against the iterator's rows, and gain: what the GPU file
    asks of the device form"""
    c, m = _map(case)
    starts, ends = Q.closed_form_rays(m, c)
    o = Q.oblique_rays(c)
    Q.reduced_rays(m, m, c, np.vstack([starts[::5], o[0]]), np.vstack([ends[::5], o[1]]))
    Q.gain(m, m, c)


def test_the_expander_on_an_empty_pool_and_off_the_map(built):
    """no block: every voxel MISSING with the default node; and a region far from the blocks"""
    c = PC.case(*PC.CASES[2])
    empty = (c["keys"][:0], c["A"][:0], c["B"][:0], c["S"][:0])
    for pool, g0 in ((empty, c["g0"]), (None, [g + 5000 for g in c["g0"]])):
        f = PC.fields(*(pool or (c["keys"], c["A"], c["B"], c["S"])), c["depth"], g0, (3, 4, 5), c["a0"], c["b0"])
        assert (f["cls"] == R.MISSING).all() and (f["leaf_depth"] == 255).all() and (f["leaf_key"] == -1).all()
        assert (f["A"].view(np.uint32) == c["a0"].view(np.uint32)).all() and (f["B"].view(np.uint32) == c["b0"].view(np.uint32)).all()


@pytest.mark.parametrize("depth", [2, 5])
def test_after_a_change_of_the_pool(built, depth):
    """erase_region of an octant of the blocks, the same keys removed from the numpy pool, then merge of the erased blocks
    from a stream of the helper: the host forms of what the GPU file asks of the device pool (the host-mode merge has no
    staging to fit, it runs at block_depth 5 too)"""
    import la3dm_amd
    c = PC.case("BGKOctoMap", depth, 1)
    m = la3dm_amd.BGKOctoMap(**c["params"], device=-1).unpack(c["stream"])
    pool, stream = Q.erase_an_octant((m,), c)
    Q.after_the_erase(m, c, pool)
    Q.merge_it_back((m,), c, stream)
    Q.after_the_merge(m, c)


def test_the_slab_of_70000_blocks(built):
    """the probe-run pool of the GPU file, on the host"""
    c = PC.case("BGKOctoMap", 1, 2, **PC.SLAB)
    assert c["keys"].size >= 70000 and c["dims"] == (46, 45, 25)
    assert 0.03 <= float((c["cls"] == R.MISSING).mean()) <= 0.12
    import la3dm_amd
    m = la3dm_amd.BGKOctoMap(**c["params"], device=-1).unpack(c["stream"])
    which = [("region", c["g0"], c["dims"]), ("shape (5, 64, 1)", c["g0"], (5, 64, 1))]
    Q.box_and_columns(m, c, which=which)
    Q.frontier(m, c, which=which)
