"""frontier on the device-resident map: bit streams, a bit-sliced stencil, the map's one-launch scan and an emit kernel
(csrc/devmap_frontier.h) list the free voxels that border unexplored space straight from the device pool.  The yardstick
is the host form of the same class (a host-mode map, a plain loop over the classes of the padded box), itself checked
against an independent numpy stencil over a walk of the leaf list (tests/helpers/frontier_cases.py).  Everything is integer
arithmetic on classes: every comparison is exact."""
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

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured
ALL = ("index", "nbrs", "score")


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


def _compare(md, mh, lo, dims, open_mask, unknown_mask, c, mn, what, cap=None):
    """device == host on n, index, nbrs, score and the info; returns the host answer"""
    kw = dict(open=open_mask, unknown=unknown_mask, connectivity=c, min_neighbours=mn, fields=ALL, cap=cap)
    gd, gh = md.frontier(lo, dims, **kw), mh.frontier(lo, dims, **kw)
    F.assert_same(gd, gh, (what, dims, open_mask, unknown_mask, c, mn, cap))
    R.assert_same(gd, gh, ("origin", "cell"), what)
    assert gd["block_key"] == gh["block_key"]
    assert md.is_device_resident()
    return gh


def _aligned_lo(m, lo):
    """the centre of the first voxel of the block that holds lo: a block-aligned region"""
    info = m.columns(lo, (1, 1, 1))
    res = np.float32(m.get_resolution())
    return (info["origin"] - info["cell"].astype(np.float32) * res).astype(np.float32)


@pytest.mark.parametrize("depth", [3, 4])
def test_device_equals_host_bit_for_bit(built, depth):
    """GPU test 1: BGK at block_depth 3 and 4, two fused (and pruned) scans: the recipe interior and a block-aligned box with
    every connectivity, mask pair and min_neighbours 1, 3, connectivity; all shapes of the CPU tests; the host form ==
    the yardstick on that map, with the input conditions; then a third insert (the pool grew, the table was rebuilt) and the
    same comparison; no mirror refresh throughout"""
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    md, mh = _pair("BGKOctoMap", params, (1, 2))
    res = mh.get_resolution()
    lv = mh.leaves()
    y = R.yardstick(mh, lv, R.recipe_lo(), R.RECIPE_DIMS)
    ilo, pcls, dims = F.interior(y, res)
    assert dims == (78, 78, 38)
    F.assert_exercises_the_feature(F.input_conditions(pcls))
    before_syncs = md.mirror_syncs()
    lim = 1 << (depth - 1)
    lo_al, al_dims = _aligned_lo(mh, R.recipe_lo()), (20 * lim, 12 * lim, 10 * lim)
    assert (md.box(lo_al, (1, 1, 1))["cell"] == 0).all()
    for c in F.CONNECTIVITIES:
        for open_mask, unknown_mask in F.MASK_PAIRS:
            score = F.score_of(pcls, open_mask, unknown_mask, c)
            for mn in (1, 3, c):
                gh = _compare(md, mh, ilo, dims, open_mask, unknown_mask, c, mn, f"bgk d{depth}")
                F.assert_same(gh, F.answer_of(score, mn), ("host form vs yardstick", depth, c, open_mask, unknown_mask, mn))
                al = _compare(md, mh, lo_al, al_dims, open_mask, unknown_mask, c, mn, f"bgk d{depth} aligned")
                assert mn > 1 or al["n"] > 0
    # index and nbrs without score, index alone (count first, then fill), a cap below n
    want = F.yardstick(pcls, F.FREE_M, F.UNK_M | F.MISS_M, 26, 2)
    F.assert_same(md.frontier(ilo, dims, connectivity=26, min_neighbours=2), want, "no score")
    got = md.frontier(ilo, dims, connectivity=26, min_neighbours=2, cap=100)
    assert got["n"] == want["n"] and (got["index"] == want["index"][:100]).all() and (got["nbrs"] == want["nbrs"][:100]).all()
    got = md.frontier(ilo, dims, connectivity=26, min_neighbours=2, cap=0, fields="score")
    assert got["n"] == want["n"] and (got["score"] == want["score"]).all()
    assert md.mirror_syncs() == before_syncs
    for shape in F.SHAPES + F.WORD_SHAPES:
        off = F.SHAPE_OFFSET if shape[2] <= 24 else F.SHAPE_OFFSET[:2] + (-10,)
        lo = (y["origin"] + np.array(off, np.float32) * np.float32(res)).astype(np.float32)
        for c in F.CONNECTIVITIES:
            for open_mask, unknown_mask in F.MASK_PAIRS:
                _compare(md, mh, lo, shape, open_mask, unknown_mask, c, 1, f"bgk d{depth} shapes")
        _compare(md, mh, lo, shape, F.FREE_M, F.UNK_M | F.MISS_M, 26, 3, f"bgk d{depth} shapes")
    for shape in F.LONG_SHAPES:
        lo, p, _ = F.padded_case(mh, lv, F.long_line_lo(y, res, shape), shape)
        for c in F.CONNECTIVITIES:
            for open_mask, unknown_mask in F.MASK_PAIRS[:2]:
                gh = _compare(md, mh, lo, shape, open_mask, unknown_mask, c, 1, f"bgk d{depth} long")
                F.assert_same(gh, F.yardstick(p, open_mask, unknown_mask, c, 1), ("long", shape, c))
    assert md.mirror_syncs() == before_syncs
    before = md.block_count()          # (refreshes the mirror; the queries do not depend on it either way)
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 5))
    for m in (md, mh):
        m.insert_pointcloud(xyz, origin, *INSERT)
    assert md.block_count() > before
    syncs = md.mirror_syncs()
    for c in F.CONNECTIVITIES:
        for open_mask, unknown_mask in F.MASK_PAIRS:
            for mn in (1, 3, c):
                _compare(md, mh, ilo, dims, open_mask, unknown_mask, c, mn, f"bgk d{depth} after a further insert")
            _compare(md, mh, lo_al, al_dims, open_mask, unknown_mask, c, 2, f"bgk d{depth} aligned, after a further insert")
    assert md.mirror_syncs() == syncs


def test_scan_tile_boundary(built):
    """GPU test 2: the compaction scans one popcount per 32-voxel word of the PADDED box plus one closing element, in tiles of
    4 096 items.  (62, 62, 30) pads to 131 072 voxels = 4 096 words, the closing element opens a second tile; (63, 61, 30) pads
    to 65 x 63 x 32 = 131 040 voxels = 4 095 words, with the closing element exactly one full tile; (64, 64, 32) and
    (64, 64, 33) are the unpadded counts the issue names (4 629 and 4 765 words: a second tile partly filled)"""
    import la3dm_amd
    md, mh = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML), (1, 2))
    lo = R.recipe_lo()
    for dims in ((64, 64, 32), (64, 64, 33), (62, 62, 30), (63, 61, 30)):
        for c in (6, 26):
            gh = _compare(md, mh, lo, dims, F.FREE_M, F.UNK_M | F.MISS_M, c, 1, "tile boundary")
            print(f"tile boundary {dims} connectivity {c}: {gh['n']} frontier voxels")
            assert gh["n"] > 0
            _compare(md, mh, lo, dims, 0xF, 0xF, c, c, "tile boundary, every voxel")      # every word full: n = all voxels
            _compare(md, mh, lo, dims, F.FREE_M, F.UNK_M | F.MISS_M, c, 1, "tile boundary, cap", cap=gh["n"] // 2)
    assert md.mirror_syncs() == 0


def test_more_tiles_than_workgroups(built, tmp_path):
    """GPU test 3: the recipe query in a fresh child process with LA3DM_SCAN_RESIDENT=1 — the scan's three tiles (82 x 82 x 42
    padded voxels = 8 826 words + the closing element, 4 096 per tile) are handed out through the ticket to one workgroup — equals the host form"""
    import la3dm_amd
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, LA3DM_SCAN_RESIDENT="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "frontier_cases.py"), out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.load(out)
    mh = la3dm_amd.BGKOctoMap(**dict(la3dm_amd.BGK_YAML, block_depth=3), device=0).set_device_resident(False)
    for i in (1, 2):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        mh.insert_pointcloud(xyz, origin, *INSERT)
    for c in F.CONNECTIVITIES:
        gh = mh.frontier(R.recipe_lo(), R.RECIPE_DIMS, open=F.FREE_M, unknown=F.UNK_M | F.MISS_M, connectivity=c, fields=ALL)
        assert gh["n"] > 4000 and int(got[f"n{c}"]) == gh["n"]
        for k in ALL:
            assert got[f"{k}{c}"].dtype == gh[k].dtype and (got[f"{k}{c}"] == gh[k]).all(), (c, k)


@pytest.mark.parametrize("variant", ["GPOctoMap", "BGKLOctoMap", "BGKLVOctoMap"])
def test_device_equals_host_on_other_variants(built, variant):
    """GPU test 4: GP, BGK-L and BGK-LV on their own configurations; the host form == the numpy stencil over its own box; on
    BGK-LV unknown = bit 4 alone selects the UNCERTAIN neighbours, and the stencil says there are some.  The classes the
    stencil reads here come from the host-mode map's box(), not from the leaf-list walk of region_cases.yardstick, which
    is written for BGK's leaf fields (the choice of test_distance_gpu.py); device == host is compared exactly all the same"""
    import la3dm_amd
    params, insert = {"GPOctoMap": (la3dm_amd.GP_YAML, INSERT), "BGKLOctoMap": (la3dm_amd.L_YAML, (0.1, 0.3, 8.0)),
                      "BGKLVOctoMap": (la3dm_amd.LV_YAML, (0.1, 0.3, 8.0))}[variant]
    md, mh = _pair(variant, dict(params), (1, 2), insert)
    res = np.float32(mh.get_resolution())
    big = mh.box(R.recipe_lo(), R.RECIPE_DIMS, fields=())
    pcls = big["cls"]
    dims = tuple(s - 2 for s in pcls.shape)
    ilo = (big["origin"] + res).astype(np.float32)
    for c in F.CONNECTIVITIES:
        for open_mask, unknown_mask in F.MASK_PAIRS + ((0x1F, 0x1F),):
            for mn in (1, 3):
                gh = _compare(md, mh, ilo, dims, open_mask, unknown_mask, c, mn, variant)
                F.assert_same(gh, F.yardstick(pcls, open_mask, unknown_mask, c, mn), (variant, "host form vs the stencil of its own box", c, mn))
    _compare(md, mh, ilo, (7, 9, 11), F.FREE_M, F.UNK_M | F.MISS_M, 26, 1, variant + " small")
    want = F.yardstick(pcls, F.FREE_M, 1 << R.UNCERTAIN, 26, 1)
    print(variant, "FREE voxels with an UNCERTAIN neighbour in the recipe interior:", want["n"])
    assert (want["n"] > 0) == (variant == "BGKLVOctoMap")
    gh = _compare(md, mh, ilo, dims, F.FREE_M, 1 << R.UNCERTAIN, 26, 1, variant + " bit 4")
    F.assert_same(gh, want, variant + " bit 4")


def test_device_pointer_form_refusals_and_storage(built):
    """GPU tests 5 and 6 on a bare la3dm_devmap: the empty map in both pointer forms; refusals with their text and nothing
    written; the device-pointer form == the host-pointer form with index on a pointer that is only 4-byte aligned and nbrs
    and score on odd addresses; a cap below n leaves the entries past it alone; free device memory is the same before and
    after 50 calls and a following smaller request"""
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
        found = C.c_uint64(0)
        h = dict(index=np.full(n, 9, np.uint32), nbrs=np.full(n, 9, np.uint8), score=np.full(n, 9, np.uint8))
        ho = _lib.FrontierOut(*[h[k].ctypes.data for k in ALL])

        def tensors(fill):
            t = dict(index=torch.full((n,), fill, dtype=torch.int32, device=dev), nbrs=torch.full((n,), fill, dtype=torch.uint8, device=dev),
                     score=torch.full((n,), fill, dtype=torch.uint8, device=dev))
            torch.cuda.synchronize()
            return t, _lib.FrontierOut(*[t[k].data_ptr() for k in ALL])
        t, do = tensors(9)
        # empty map: every voxel with score = connectivity when both masks hold bit 3, none otherwise — host and device pointers
        for c in F.CONNECTIVITIES:
            for cap in (n, 1000):
                for k in h:
                    h[k][:] = 9
                t, do = tensors(9)
                assert H.la3dm_devmap_frontier_host(dm, lop, dp, 0x9, 0xC, c, c, cap, C.byref(ho), C.byref(found), None) == OK, err()
                assert found.value == n and (h["index"][:cap] == np.arange(cap)).all() and (h["nbrs"][:cap] == c).all() and (h["score"] == c).all()
                assert (h["index"][cap:] == 9).all() and (h["nbrs"][cap:] == 9).all()
                found.value = 0
                assert H.la3dm_devmap_frontier_device(dm, lop, dp, 0x9, 0xC, c, c, cap, C.byref(do), C.byref(found), None) == OK, err()
                g = {k: t[k].cpu().numpy() for k in t}
                assert found.value == n and (g["index"][:cap] == np.arange(cap)).all() and (g["nbrs"][:cap] == c).all() and (g["score"] == c).all()
                assert (g["index"][cap:] == 9).all() and (g["nbrs"][cap:] == 9).all()
            for open_mask, unknown_mask in ((0x7, 0xC), (0x8, 0x7)):
                for k in h:
                    h[k][:] = 9
                t, do = tensors(9)
                assert H.la3dm_devmap_frontier_host(dm, lop, dp, open_mask, unknown_mask, c, 1, n, C.byref(ho), C.byref(found), None) == OK, err()
                assert found.value == 0 and (h["index"] == 9).all() and (h["nbrs"] == 9).all() and (h["score"] == 0).all()
                found.value = 5
                assert H.la3dm_devmap_frontier_device(dm, lop, dp, open_mask, unknown_mask, c, 1, n, C.byref(do), C.byref(found), None) == OK, err()
                assert found.value == 0 and (t["index"].cpu().numpy() == 9).all() and (t["score"].cpu().numpy() == 0).all()
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3,
                                                     0.1, 0.5, 8.0, None) == OK
        # refusals: LA3DM_ERR_ARG and a text that names the argument; nothing written
        for k in h:
            h[k][:] = 7
        t, do = tensors(7)
        found.value = 77
        at = np.array(((1 << 10) - 2, (1 << 10) - 2, (1 << 8) - 2), np.uint32)      # padded: exactly 2^28
        over = at + np.array((0, 0, 1), np.uint32)
        for fn, out in ((H.la3dm_devmap_frontier_host, ho), (H.la3dm_devmap_frontier_device, do)):
            call = lambda lo_p=lop, d_p=dp, om=1, um=0xC, c=6, mn=1, cap=n, o=C.byref(out), nf=C.byref(found): \
                fn(dm, lo_p, d_p, om, um, c, mn, cap, o, nf, None)   # noqa: E731
            for bad in ((np.nan, 0, 0), (0, -np.inf, 0), (0, 0, 1.1e8)):
                b3 = np.array(bad, np.float32)
                assert call(lo_p=b3.ctypes.data) == ERR_ARG and "lo must be finite" in err()
            for z in range(3):
                d0 = dims.copy()
                d0[z] = 0
                assert call(d_p=d0.ctypes.data) == ERR_ARG and "dims must be >= 1" in err()
            assert call(lo_p=None) == ERR_ARG and "lo is NULL" in err()
            assert call(d_p=None) == ERR_ARG and "dims is NULL" in err()
            assert fn(None, lop, dp, 1, 0xC, 6, 1, n, C.byref(out), C.byref(found), None) == ERR_ARG
            for mask in (0, 0x20, 0x80000002):
                assert call(om=mask) == ERR_ARG and "open_mask must hold" in err()
                assert call(um=mask) == ERR_ARG and "unknown_mask must hold" in err()
            for c in (0, 7, 27, 0xFFFFFFFF):
                assert call(c=c) == ERR_ARG and "connectivity must be 6, 18 or 26" in err()
            for c, mn in ((6, 0), (6, 7), (18, 19), (26, 27)):
                assert call(c=c, mn=mn) == ERR_ARG and "min_neighbours must lie in" in err()
            for too_big in (((1 << 28) - 1, 1, 1), tuple(int(v) for v in over), (1 << 16, 1 << 16, 1), (0xFFFFFFFF,) * 3):
                big = np.array(too_big, np.uint32)
                assert call(d_p=big.ctypes.data, o=None, nf=None) == ERR_ARG and "LA3DM_FR_MAX_CELLS" in err(), err()
            far = np.array((-3.0e5, 0, 0), np.float32)
            assert call(lo_p=far.ctypes.data) == ERR_ARG and "lo: the block field leaves" in err()
            far = np.array((2.09e5, 0, 0), np.float32)
            long_x = np.array((1 << 16, 1, 1), np.uint32)
            assert call(lo_p=far.ctypes.data, d_p=long_x.ctypes.data) == ERR_ARG and "region's block fields leave" in err()
            low = np.array((-209715.5, 0, 0), np.float32)
            assert call(lo_p=low.ctypes.data) == ERR_ARG and "padded by one voxel" in err(), err()
            assert call(o=None) == ERR_ARG and "out is NULL" in err()
            assert call(o=C.byref(_lib.FrontierOut(None, out.nbrs, out.score))) == ERR_ARG and "out->index must not be NULL" in err()
            assert call(nf=None) == ERR_ARG and "n_found is NULL" in err()
            # the limit itself passes the size check: the next check — the buffers — answers
            assert call(d_p=at.ctypes.data, o=None) == ERR_ARG and "out is NULL" in err()
            assert call(d_p=at.ctypes.data, cap=0, o=None, nf=None) == ERR_ARG and "n_found is NULL" in err()
        assert found.value == 77 and all((h[k] == 7).all() for k in h) and all((t[k].cpu().numpy() == 7).all() for k in t)
        # the device-pointer form == the host-pointer form: index 4 bytes off a 16-byte boundary, nbrs and score on odd addresses
        for (open_mask, unknown_mask), c, mn in zip(F.MASK_PAIRS, (6, 18, 26, 26), (1, 2, 3, 5)):
            for k in h:
                h[k][:] = 0xEEEEEEEE if k == "index" else 0xEE
            assert H.la3dm_devmap_frontier_host(dm, lop, dp, open_mask, unknown_mask, c, mn, n, C.byref(ho), C.byref(found), None) == OK, err()
            nf = int(found.value)
            assert 0 < nf <= n and (h["index"][nf:] == 0xEEEEEEEE).all() and (h["nbrs"][nf:] == 0xEE).all()
            assert (h["nbrs"][:nf] == h["score"][h["index"][:nf]]).all() and (np.diff(h["index"][:nf].astype(np.int64)) > 0).all()
            for offset in (0, 1, 3):
                for fields in (ALL, ("index",), ("index", "nbrs"), ("score",)):
                    for cap in ((n, nf // 3) if "index" in fields else (0,)):
                        t = dict(index=torch.full((n + 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev),
                                 nbrs=torch.full((n + 4,), 0x5A, dtype=torch.uint8, device=dev),
                                 score=torch.full((n + 4,), 0x5A, dtype=torch.uint8, device=dev))
                        torch.cuda.synchronize()
                        assert (t["index"][offset:].data_ptr() & 15) == 4 * offset and (offset == 0 or t["nbrs"][offset:].data_ptr() & 1)
                        do = _lib.FrontierOut(*[t[k][offset:].data_ptr() if k in fields else None for k in ALL])
                        info, info2 = _lib.RegionInfo(), _lib.RegionInfo()
                        assert H.la3dm_devmap_frontier_host(dm, lop, dp, open_mask, unknown_mask, c, mn, 0, None, C.byref(found), C.byref(info)) == OK
                        found.value = 0
                        assert H.la3dm_devmap_frontier_device(dm, lop, dp, open_mask, unknown_mask, c, mn, cap, C.byref(do), C.byref(found),
                                                              C.byref(info2)) == OK, err()
                        assert found.value == nf
                        assert list(info2.origin) == list(info.origin) and info2.block_key == info.block_key and list(info2.cell) == list(info.cell)
                        g = {k: t[k].cpu().numpy() for k in t}
                        g["index"] = g["index"].view(np.uint32)
                        k_out = min(cap, nf)
                        for k in ("index", "nbrs"):
                            fill = 0x5A5A5A5A if k == "index" else 0x5A
                            if k in fields:
                                assert (g[k][:offset] == fill).all() and (g[k][offset + k_out:] == fill).all(), (k, offset, cap)
                                assert (g[k][offset:offset + k_out] == h[k][:k_out]).all(), (k, offset, cap, fields)
                            else:
                                assert (g[k] == fill).all()
                        if "score" in fields:
                            assert (g["score"][:offset] == 0x5A).all() and (g["score"][offset + n:] == 0x5A).all()
                            assert (g["score"][offset:offset + n] == h["score"]).all()
                        else:
                            assert (g["score"] == 0x5A).all()
        # storage: the first call at a size reserves, 50 more do not; a smaller region afterwards allocates nothing
        t, do = tensors(0)
        small = np.array((31, 17, 23), np.uint32)

        def free():
            torch.cuda.synchronize()
            return torch.cuda.mem_get_info()[0]
        assert H.la3dm_devmap_frontier_device(dm, lop, dp, 1, 0xC, 26, 1, n, C.byref(do), C.byref(found), None) == OK, err()
        assert H.la3dm_devmap_frontier_host(dm, lop, dp, 1, 0xC, 26, 1, n, C.byref(ho), C.byref(found), None) == OK, err()
        f0 = free()
        for i in range(25):
            c = F.CONNECTIVITIES[i % 3]
            assert H.la3dm_devmap_frontier_device(dm, lop, dp, 1 + (i & 1), 0xC, c, 1 + i % c, n, C.byref(do), C.byref(found), None) == OK, err()
            assert H.la3dm_devmap_frontier_host(dm, lop, dp, 1 + (i & 1), 0xC, c, 1 + i % c, n, C.byref(ho), C.byref(found), None) == OK, err()
        assert H.la3dm_devmap_frontier_device(dm, lop, small.ctypes.data, 1, 0xC, 6, 1, n, C.byref(do), C.byref(found), None) == OK, err()
        assert H.la3dm_devmap_frontier_host(dm, lop, small.ctypes.data, 1, 0xC, 6, 1, n, C.byref(ho), C.byref(found), None) == OK, err()
        f1 = free()
        print(f"free device memory before / after 50 calls and a smaller region: {f0} / {f1}")
        # the figure is the whole device's: a process of another user may release memory meanwhile, so growth is what fails
        assert f1 >= f0, (f0, f1)
    finally:
        H.la3dm_devmap_destroy(dm)


def test_no_mirror_refresh_and_example_program(built):
    """the query is answered from the pool; examples/frontier.cpp (built by build()) == the Python binding on the same map"""
    import la3dm_amd
    exe = os.path.join(ROOT, "examples", "frontier")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "3"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert all(ln.startswith("goal ") for ln in lines[:-1]) and lines[-1].startswith("frontier 128 x 128 x 16 from ")
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    e = m.frontier(R.recipe_lo(), (6, 5, 4), open=("free", "missing"), unknown=("missing",), connectivity=18, min_neighbours=18)
    assert e["n"] == 120 and (e["nbrs"] == 18).all() and m.mirror_syncs() == 0          # the empty map
    for i in (1, 2, 3):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        m.insert_pointcloud(xyz, origin, *INSERT)
    before = m.mirror_syncs()
    o = np.asarray(origin, np.float32)
    lo = np.array([o[0] - np.float32(6.4), o[1] - np.float32(6.4), o[2] - np.float32(0.8)], np.float32)
    dims = (128, 128, 16)
    g = m.frontier(lo, dims)
    dist = m.distance_field(lo, dims, radius=8, fields=("dist",))["dist"].reshape(-1)
    assert m.is_device_resident() and m.mirror_syncs() == before
    keep = dist[g["index"]] >= np.float32(0.3)
    tok = lines[-1].split()
    got = {tok[k]: tok[k + 1] for k in range(len(tok) - 1)}
    print(lines[-1])
    assert int(got["found"]) == g["n"] > 0 and int(got["kept"]) == int(keep.sum()) > 0
    assert len(lines) == min(5, int(keep.sum())) + 1
    assert got["mirror_syncs"] == "0" and got["device_resident"] == "1"
    at = tok.index("from")
    assert np.allclose([float(tok[at + 1]), float(tok[at + 2]), float(tok[at + 3].rstrip(":"))], g["origin"], atol=1e-4)
    ijk = np.stack(np.unravel_index(g["index"][keep], dims), 1).astype(np.float32)
    p = g["origin"] + ijk * np.float32(m.get_resolution())
    rng = np.sqrt(((p - o) ** 2).sum(1))
    order = np.argsort(rng, kind="stable")[:5]
    for ln, q in zip(lines[:-1], order):
        tk = ln.split()
        assert abs(float(tk[7]) - rng[q]) < 1e-3, (ln, rng[q])
