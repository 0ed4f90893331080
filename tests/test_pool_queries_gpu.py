"""Every query of the device-resident map on hand-built pools at block_depth 1 to 5: pool_find_block's probe, pool_block_key /
pool_cell_index, the climb through PRUNED nodes (csrc/devmap_pool.h) and the copies of those steps in dm_raycast, dm_box,
dm_columns and the walk of csrc/devmap_gain.h, at the depths, tilings and key ranges the scan-built maps of the other tests
never reach: a block that is its own root (depth 1), 4 681-node blocks (depth 5), a block collapsed to its root beside a
missing block, one collapsed sibling group, BGK-LV's UNCERTAIN at coarse layers, key fields on both sides of 524288, a table
of 70 000 blocks.  The stream of tests/helpers/pool_cases.py is loaded with unpack; every query's device form is compared
with the numpy yardstick on the expander's classes (tests/helpers/pool_checks.py; tests/test_pool_queries_cpu.py pins the
host forms).  Integers by ==, floats by their bits."""
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

pytestmark = pytest.mark.gpu

_MAPS = {}


def _load(c):
    """the case's stream in a device-resident map and in a host-mode one"""
    import la3dm_amd
    cls = getattr(la3dm_amd, c["name"])
    md = cls(**c["params"], device=0).unpack(c["stream"])
    mh = cls(**c["params"], device=0).set_device_resident(False).unpack(c["stream"])
    assert md.is_device_resident() and not mh.is_device_resident() and md.block_count() == mh.block_count() == c["keys"].size
    return md, mh


def _maps(case):
    if case not in _MAPS:
        c = PC.case(*case)
        PC.assert_exercises_the_feature(PC.input_conditions(c["cls"], c["leaf_depth"], c["g0"], c["depth"], PC.variant_classes(c["name"])), case)
        _MAPS[case] = (c,) + _load(c)
    return _MAPS[case]


class _Resident:
    """the map stays device resident and its host mirror is not refreshed"""

    def __init__(self, md):
        self.md = md

    def __enter__(self):
        self.syncs = self.md.mirror_syncs()
        return self.md

    def __exit__(self, kind, *rest):
        if kind is None:
            assert self.md.is_device_resident() and self.md.mirror_syncs() == self.syncs


cases = pytest.mark.parametrize("case", PC.CASES, ids=PC.CASE_IDS)


@cases
def test_box_and_columns(built, case):
    c, md, mh = _maps(case)
    with _Resident(md):
        Q.box_and_columns(md, c)
    R.assert_same(md.box(c["lo"], c["dims"]), mh.box(c["lo"], c["dims"]), R.BOX_FIELDS, "device vs host")


@cases
def test_distance_and_nearest(built, case):
    c, md, _ = _maps(case)
    with _Resident(md):
        Q.distance(md, c)
        Q.nearest(md, c)


@cases
def test_frontier(built, case):
    c, md, _ = _maps(case)
    with _Resident(md):
        Q.frontier(md, c)


@cases
def test_reach(built, case):
    c, md, _ = _maps(case)
    with _Resident(md):
        Q.reach(md, c)


@cases
def test_travel(built, case):
    c, md, _ = _maps(case)
    with _Resident(md):
        Q.travel(md, c)


@cases
def test_clusters(built, case):
    c, md, _ = _maps(case)
    with _Resident(md):
        Q.clusters(md, c)


@cases
def test_footing_and_surface(built, case):
    c, md, _ = _maps(case)
    with _Resident(md):
        Q.footing(md, c)
        Q.surface(md, c)


@cases
def test_rays(built, case):
    """raycast_many against the closed form, and against raycast_cases.reduce_rays over the host-mode map's iterator"""
    c, md, mh = _maps(case)
    with _Resident(md):
        starts, ends = Q.closed_form_rays(md, c)
        o = Q.oblique_rays(c)
        Q.reduced_rays(md, mh, c, np.vstack([starts[::5], o[0]]), np.vstack([ends[::5], o[1]]))


@cases
def test_gain(built, case):
    c, md, mh = _maps(case)
    with _Resident(md):
        Q.gain(md, mh, c)


def test_probe_runs_in_a_table_of_70000_blocks(built):
    """a second depth-1 pool: a 48 x 48 x 32 slab of one-voxel blocks, 5 % left out — two 4 096-item scan tiles, a larger
    table, one uncached probe per voxel of box"""
    c = PC.case("BGKOctoMap", 1, 2, **PC.SLAB)
    assert c["keys"].size >= 70000 and c["dims"] == (46, 45, 25)
    share = float((c["cls"] == R.MISSING).mean())
    print(f"slab: {c['keys'].size} blocks, MISSING on {share:.4f} of the region")
    assert 0.03 <= share <= 0.12
    md, _ = _load(c)
    which = [("region", c["g0"], c["dims"]), ("shape (5, 64, 1)", c["g0"], (5, 64, 1))]
    with _Resident(md):
        Q.box_and_columns(md, c, which=which)
        Q.frontier(md, c, which=which)


@pytest.mark.parametrize("depth", [2, 5])
def test_after_a_change_of_the_pool(built, depth):
    """erase_region of the octant of blocks at and above key field 524288 on every axis (the pool is compacted, the table
    rebuilt), the same keys removed from the numpy pool; then merge of the erased blocks from a stream of the helper, against
    the original classes (merge prunes, so the layers and values of a block it wrote are its own); at block_depth 5 merge's
    documented refusal"""
    c = PC.case("BGKOctoMap", depth, 1)
    md, mh = _load(c)
    pool, stream = Q.erase_an_octant((md, mh), c)
    with _Resident(md):
        Q.after_the_erase(md, c, pool)
    if depth == 5:
        before = md.pack()
        with pytest.raises(RuntimeError, match="merge runs at block_depth 1 to 4"):
            md.merge(stream)
        assert (md.pack() == before).all() and md.block_count() == pool[0].size
        return
    Q.merge_it_back((md, mh), c, stream)
    with _Resident(md):
        Q.after_the_merge(md, c)
    R.assert_same(md.box(c["lo"], c["dims"]), mh.box(c["lo"], c["dims"]), R.BOX_FIELDS, "device vs host after the merge")
