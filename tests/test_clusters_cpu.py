"""clusters on a host-mode map (device = -1): the host form — a flood fill over box's classes, the definition the device
kernels reproduce — against the independent yardstick of tests/helpers/clusters_cases.py (scipy's labelling over a walk
of the leaf list, records and rep from the definition).  Integers throughout and a unique answer: every comparison is
exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import clusters_cases as K  # noqa: E402

DIMS = R.RECIPE_DIMS
FIELDS = ("label", "of_member")


def _check(m, lo, dims, cls, what, members=None, member=K.FREE_M, **kw):
    fields = FIELDS if members is not None else ("label",)
    got = m.clusters(lo, dims, members=members, member=member, fields=fields, **kw)
    want = K.yardstick(cls, member, members, kw.get("connectivity", 26), kw.get("tile", 0), kw.get("min_size", 1), kw.get("cap"))
    K.assert_same(got, want, (what, kw))
    assert got["rounds"] == got["brick_runs"] == got["capped"] == 0          # the host form reports no diagnostics
    return got, want


@pytest.mark.parametrize("depth", [3, 4])
def test_recipe_region(built, depth):
    """CPU test 1: the recipe region at block_depth 3 and 4.  From frontier's list at every connectivity, tile 0, 8 and 16
    and min_size 1 and 8; from the classes with OCCUPIED and FREE, untiled; label, of_member, every record array, the
    stats and the info against the yardstick; cap below n and cap 0; the list reversed and with duplicates"""
    m, lv, _ = R.fused_map(depth)
    lo, cls, listed, info = K.recipe(m, lv, ("cpu", depth))
    cond = K.input_conditions(cls, listed, key=("cpu", depth))
    K.assert_exercises_the_feature(cond)
    assert (m.frontier(lo, DIMS)["index"] == listed).all()                      # the list the issue counts: frontier's default
    for c in K.CONNECTIVITIES:
        for tile in K.TILES:
            for min_size in (1, 8):
                got, want = _check(m, lo, DIMS, cls, f"list d{depth}", members=listed, connectivity=c, tile=tile, min_size=min_size)
                assert got["block_key"] == info["block_key"] and (got["cell"] == info["cell"]).all()
                row = cond["rows"].get((tile, c))
                if row:
                    assert got["n"] == (row["clusters"] if min_size == 1 else row["ge8"]) and got["largest"] == row["largest"]
                print(f"depth {depth} c {c} tile {tile} min_size {min_size}: n {got['n']} dropped {got['n_dropped']} largest {got['largest']}")
    for mask in (K.OCC_M, K.FREE_M):
        got, _ = _check(m, lo, DIMS, cls, f"classes d{depth}", member=mask, connectivity=26)
        assert got["n"] >= 1 and got["n_members"] == int(K.members_of(cls, mask).sum())
    q = dict(connectivity=26, tile=8, min_size=8)
    full, _ = _check(m, lo, DIMS, cls, "tiled", members=listed, **q)
    assert full["n"] > 40
    few, _ = _check(m, lo, DIMS, cls, "cap below n", members=listed, cap=40, **q)
    assert few["n"] == full["n"] and few["first"].size == 40 and all((few[k] == full[k][:40]).all() for k in K.RECORDS)
    none, _ = _check(m, lo, DIMS, cls, "cap 0", members=listed, cap=0, **q)
    assert none["n"] == full["n"] and none["first"].size == 0
    again = np.concatenate([listed[::-1], listed[::3], [DIMS[0] * DIMS[1] * DIMS[2], 0xFFFFFFFF]]).astype(np.uint32)
    twice, _ = _check(m, lo, DIMS, cls, "reversed, with duplicates", members=again, **q)
    assert all((twice[k] == full[k]).all() for k in K.RECORDS + ("label",)) and twice["n_members"] == full["n_members"]
    assert (twice["of_member"][-2:] == K.NONE).all() and (twice["of_member"][:listed.size] == full["of_member"][::-1]).all()


def test_hand_built_sets(built):
    """CPU test 2: member sets on an empty map (member = MISSING, from a list): shapes whose axes are no multiples of 8;
    pairs across a brick corner and edge, and across a tile border; a snake wound inside one brick; lines through four
    bricks; overlapping boxes; a hollow shell, whose rep is a member though the centroid is not, with the tie rule; and
    min_size above every cluster"""
    import la3dm_amd
    m = la3dm_amd.BGKOctoMap(**R.YAML, device=-1)
    lo = np.array((0.05, 0.05, 0.05), np.float32)
    for name, dims, voxels, tile, expect in K.hand_sets():
        cls = np.full(dims, R.MISSING, np.uint8)
        listed = np.array([K.flat(v, dims) for v in voxels], np.uint32)
        for c in K.CONNECTIVITIES:
            got, _ = _check(m, lo, dims, cls, name, members=listed, member=K.MISS_M, connectivity=c, tile=tile)
            assert got["n_members"] == len(set(voxels)) and (expect is None or got["n"] == expect[c]), (name, c, got["n"], expect)
            assert (np.isin(got["rep"], listed)).all() and (got["label"].reshape(-1)[got["rep"]] == np.arange(got["n"])).all()
            if name == "a hollow shell":
                assert got["size"][0] == 98 and (got["sum"][0] == 3 * 98).all() and got["label"][3, 3, 3] == K.NONE
                assert got["rep"][0] == K.flat((1, 3, 3), dims)              # six face centres at distance 2: the smallest index
            if name == "overlapping boxes":
                assert (got["lo"][0] == 0).all() and (got["hi"][0] == (4, 4, 0)).all() and (got["lo"][1] == got["hi"][1]).all()
            big = m.clusters(lo, dims, members=listed, member=K.MISS_M, connectivity=c, tile=tile, min_size=len(voxels) + 1)
            assert big["n"] == 0 and (big["label"] == K.NONE).all() and big["n_dropped"] == got["n"] and big["largest"] == 0
    everything = m.clusters(lo, (9, 8, 17), member=K.MISS_M, connectivity=6)
    assert everything["n"] == 1 and everything["size"][0] == 9 * 8 * 17 and (everything["label"] == 0).all()
    assert m.clusters(lo, (9, 8, 17), member=K.FREE_M)["n"] == 0
    empty = m.clusters(lo, (9, 8, 17), members=np.zeros(0, np.uint32), member=K.MISS_M, fields=FIELDS)
    assert empty["n"] == 0 and empty["n_members"] == 0 and empty["of_member"].size == 0 and (empty["label"] == K.NONE).all()


def test_refusals(built):
    """CPU test 3: every refusal of the contract, in its order, with the argument named and the buffers untouched"""
    import la3dm_amd
    from la3dm_amd import _lib
    M = _lib.maplib()
    m, _, _ = R.fused_map(3)
    lo = R.recipe_lo()
    dims = np.array(DIMS, np.uint32)
    n = int(dims.prod())
    listed = np.arange(0, n, 7, dtype=np.uint32)
    names = [k for k, _ in _lib.ClustersOut._fields_]
    h = {k: np.full(3 * n if k in ("lo", "hi", "sum") else n, 7, np.uint64 if k == "sum" else np.uint32) for k in names}
    full = _lib.ClustersOut(*[h[k].ctypes.data for k in names])
    stats, found = _lib.ClustersStats(*[77] * 7), C.c_uint32(77)

    def call(lo_p=lo.ctypes.data, d_p=dims.ctypes.data, out=full, no_params=False, mask=1, fl=1, c=26, tile=8, ms=1, nm=listed.size,
             mem=listed.ctypes.data, cap=n):
        p = _lib.ClustersParams(mask, fl, c, tile, ms, nm, mem, cap)
        rc = M.la3dm_map_clusters(m._h, lo_p, d_p, None if no_params else C.byref(p), C.byref(out) if out is not None else None,
                                  C.byref(found), C.byref(stats), None)
        return rc, M.la3dm_map_last_error(m._h).decode()

    def refused(text, **kw):
        rc, err = call(**kw)
        assert rc != 0 and text in err, (kw, rc, err)

    assert call()[0] == 0
    for k in h:
        h[k][...] = 7
    found.value = 77
    stats = _lib.ClustersStats(*[77] * 7)
    refused("params is NULL", no_params=True)
    for mask in (0, 0x20, 0x80000001):
        refused("member_mask", mask=mask)
    for c in (0, 7, 27, 0xFFFFFFFF):
        refused("connectivity must be 6, 18 or 26", c=c)
    for tile in (4, 12, (1 << 15) + 8):
        refused("tile must be", tile=tile)
    refused("min_size must be >= 1", ms=0)
    refused("from_list must be 0 or 1", fl=2)
    refused("LA3DM_CLUSTERS_MAX_MEMBERS", nm=(1 << 28) + 1)
    refused("members is NULL", mem=None)
    refused("of_member is set with from_list = 0", fl=0)
    none = _lib.ClustersOut(full.label, None, None, None, None, None, None, None)
    refused("cap > 0 with no record array", out=none, fl=0)
    refused("cap > 0 with no record array", out=None)
    refused("member_mask", mask=0, c=7, tile=4, ms=0, lo_p=None)                # the order: the mask answers first
    refused("connectivity", c=7, tile=4, ms=0, lo_p=None)
    refused("tile must be", tile=4, ms=0, lo_p=None)
    refused("min_size", ms=0, fl=2, lo_p=None)
    refused("lo is NULL", lo_p=None)                                             # then what box refuses
    refused("dims is NULL", d_p=None)
    refused("lo must be finite", lo_p=np.array((np.nan, 0, 0), np.float32).ctypes.data)
    d0 = dims.copy()
    d0[1] = 0
    refused("dims must be >= 1", d_p=d0.ctypes.data)
    refused("LA3DM_BOX_MAX_CELLS", d_p=np.array((1 << 11, 1 << 11, 1 << 9), np.uint32).ctypes.data, out=none, cap=0, fl=0)
    refused("LA3DM_CLUSTERS_MAX_AXIS", d_p=np.array(((1 << 15) + 1, 1, 1), np.uint32).ctypes.data, out=none, cap=0, fl=0)
    refused("LA3DM_CLUSTERS_MAX_CELLS", d_p=np.array((1 << 10, 1 << 10, (1 << 8) + 1), np.uint32).ctypes.data, out=none, cap=0, fl=0)
    assert all((v == 7).all() for v in h.values()) and found.value == 77
    assert [getattr(stats, k) for k, _ in stats._fields_] == [77] * 7
    with pytest.raises(Exception, match="tile must be"):
        m.clusters(lo, DIMS, tile=12)
    with pytest.raises(ValueError, match="unknown fields"):
        m.clusters(lo, DIMS, fields=("labels",))
    assert la3dm_amd.CLUSTERS_BRICK == K.BRICK and la3dm_amd.CLUSTERS_INNER == K.INNER and la3dm_amd.CLUSTERS_BATCH == K.BATCH
    assert la3dm_amd.CLUSTERS_NONE == K.NONE
