"""gain on the device-resident map: one ray per lane marks the voxels it walks over in a bit set per viewpoint, a second
kernel counts the sets (csrc/devmap_gain.h).  The yardstick is the host form of the same class on a host-mode twin map with
the same inserts (a plain loop over the map's own RayCaster), itself checked against the independent yardstick of
tests/helpers/gain_cases.py.  Everything after the walk is integers: every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, pcd_path

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import gain_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured


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


def _compare(md, mh, lo, dims, origins, offsets, count, stop, budget, what):
    """device == host on gain, started, hits, seen and the info; returns the host answer"""
    kw = dict(count=count, stop=stop, max_steps=budget, fields=G.FIELDS)
    gd, gh = md.gain(lo, dims, origins, offsets, **kw), mh.gain(lo, dims, origins, offsets, **kw)
    G.assert_same(gd, gh, (what, dims, count, stop, budget))
    R.assert_same(gd, gh, ("origin", "cell"), what)
    assert gd["block_key"] == gh["block_key"] and md.is_device_resident()
    return gh


@pytest.mark.parametrize("depth", [3, 4])
def test_device_equals_host_bit_for_bit(built, depth):
    """GPU test 1: BGK at block_depth 3 and 4, two fused (and pruned) scans: the recipe with both fans and the four cases,
    every small shape of the CPU tests; the host form == the independent yardstick on that map, with the input conditions;
    then a further insert (the pool grew, the table was rebuilt) and the same comparisons; no mirror refresh throughout"""
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    md, mh = _pair("BGKOctoMap", params, (1, 2))
    res = mh.get_resolution()
    lv = mh.leaves()
    lo = R.recipe_lo()
    y = R.yardstick(mh, lv, lo, R.RECIPE_DIMS)
    origins, _ = G.viewpoints(y, res)
    G.assert_exercises_the_feature(G.input_conditions(mh, lv, y, lo, R.RECIPE_DIMS, origins, depth))
    near, pick = G.near_viewpoints(y, res)
    before_syncs = md.mirror_syncs()

    def everything(tag, check_yardstick):
        for offsets in (G.fan(256, 4.0), G.fan(96, 3.0)):
            for count, stop, budget in G.CASES:
                gh = _compare(md, mh, lo, R.RECIPE_DIMS, origins, offsets, count, stop, budget, f"bgk d{depth} {tag}")
                if check_yardstick and offsets.shape[0] == 256:
                    want = G.yardstick(mh, lv, lo, R.RECIPE_DIMS, origins, offsets, count, stop, budget, cls=y["cls"])
                    G.assert_same(gh, want, ("host form vs yardstick", depth, count, stop, budget))
        marked = 0
        for what, slo, dims, o, f in G.small_cases(mh, y, near, pick):
            for count, stop, budget in G.SMALL_CASES:
                marked += int(_compare(md, mh, slo, dims, o, f, count, stop, budget, f"bgk d{depth} {tag} {what}")["gain"].sum())
                if what == "m = 1":
                    _compare(md, mh, slo, dims, o, np.repeat(f, 256, 0), count, stop, budget, f"bgk d{depth} {tag} 256 copies")
        assert marked > 200
    everything("two scans", True)
    assert md.mirror_syncs() == before_syncs
    before = md.block_count()          # (refreshes the mirror; the queries do not depend on it either way)
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 5))
    for m in (md, mh):
        m.insert_pointcloud(xyz, origin, *INSERT)
    assert md.block_count() > before
    syncs = md.mirror_syncs()
    everything("after a further insert", False)
    assert md.mirror_syncs() == syncs


def test_lanes_waves_and_neighbouring_sets(built):
    """GPU test 2: m in {1, 63, 64, 65, 255, 256, 257} (a wave, a workgroup, one lane more) x n in {1, 2, 3} at dims
    (3, 5, 7) (4 words, 9 spare bits) and (1, 1, 33) (one bit in the second word): seen, compared whole, shows that a set
    never bleeds into its neighbour's first word"""
    import la3dm_amd
    md, mh = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML), (1, 2))
    res = mh.get_resolution()
    big = mh.box(R.recipe_lo(), R.RECIPE_DIMS, fields=())
    near, _ = G.near_viewpoints(big, res)
    lo = G.sub_lo(big, G.SHAPE_OFFSET, res)
    f = G.fan(257, 3.0)
    marked = 0
    for dims in ((3, 5, 7), (1, 1, 33)):
        for m in (1, 63, 64, 65, 255, 256, 257):
            for n in (1, 2, 3):
                for count, stop, budget in G.SMALL_CASES:
                    gh = _compare(md, mh, lo, dims, near[:n], f[:m], count, stop, budget, f"n {n} m {m}")
                    assert gh["seen"].shape == (n, (int(np.prod(dims)) + 31) // 32)
                    marked += int(gh["gain"].sum())
    print(f"lanes and waves: {marked} voxels marked in all")
    assert marked > 1000 and md.mirror_syncs() == 0


@pytest.mark.parametrize("variant", ["GPOctoMap", "BGKLOctoMap", "BGKLVOctoMap"])
def test_device_equals_host_on_other_variants(built, variant):
    """GPU test 3: GP, BGK-L and BGK-LV on their own configurations; on BGK-LV count = bit 4 selects the UNCERTAIN voxels, and
    the host form's box says the rays cross some.  The viewpoints are FREE voxels of the host-mode map's box()"""
    import la3dm_amd
    params, insert = {"GPOctoMap": (la3dm_amd.GP_YAML, INSERT), "BGKLOctoMap": (la3dm_amd.L_YAML, (0.1, 0.3, 8.0)),
                      "BGKLVOctoMap": (la3dm_amd.LV_YAML, (0.1, 0.3, 8.0))}[variant]
    md, mh = _pair(variant, dict(params), (1, 2), insert)
    lo = R.recipe_lo()
    big = mh.box(lo, R.RECIPE_DIMS, fields=())
    origins, _ = G.viewpoints(big, mh.get_resolution())
    for offsets in (G.fan(256, 4.0), G.fan(96, 3.0)):
        for count, stop, budget in G.CASES + ((0x1F, 0x2, 4096),):
            gh = _compare(md, mh, lo, R.RECIPE_DIMS, origins, offsets, count, stop, budget, variant)
            assert count != 0x1F or (gh["gain"][:6] > 0).all(), (variant, gh["gain"])      # every row of a started ray counts
    gh = _compare(md, mh, lo, R.RECIPE_DIMS, origins, G.fan(256, 4.0), 1 << R.UNCERTAIN, 0x2, 4096, variant + " bit 4")
    print(variant, "UNCERTAIN voxels seen per viewpoint:", gh["gain"].tolist(), "in the region:", int((big["cls"] == R.UNCERTAIN).sum()))
    assert (int(gh["gain"].sum()) > 0) == (variant == "BGKLVOctoMap")
    _compare(md, mh, G.sub_lo(big, G.SHAPE_OFFSET, mh.get_resolution()), (3, 5, 7), origins, G.fan(96, 3.0), 0x1F, 0, 64, variant + " small")


def test_device_pointer_form_refusals_and_storage(built):
    """GPU test 4 on a bare la3dm_devmap: the empty map in both pointer forms; refusals with their text and nothing written;
    the device-pointer form == the host-pointer form with the optional outputs NULL and with seen given or not; seen given
    leaves the arena alone; a large request followed by a smaller one reserves nothing new; the map stays usable"""
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
        W = (int(dims.prod()) + 31) // 32
        f = G.fan(300, 4.0)
        nd = f.shape[0]
        rng = np.random.default_rng(5)
        o = (np.asarray(origin, np.float32) + rng.uniform(-1.5, 1.5, (40, 3)).astype(np.float32) * np.array((1, 1, 0.3), np.float32)).astype(np.float32)
        n = o.shape[0]
        lop, dp = lo.ctypes.data, dims.ctypes.data
        d_o, d_f = torch.from_numpy(o).to(dev), torch.from_numpy(f).to(dev)
        h = {k: np.full((n, W) if k == "seen" else n, 9, np.uint32) for k in G.FIELDS}
        ho = _lib.GainOut(*[h[k].ctypes.data for k in G.FIELDS])

        def tensors(fill, fields=G.FIELDS, rows=n):
            t = {k: torch.full((rows * W + 8,) if k == "seen" else (rows + 8,), fill, dtype=torch.int32, device=dev) for k in G.FIELDS}
            torch.cuda.synchronize()
            return t, _lib.GainOut(*[t[k].data_ptr() if k in fields else None for k in G.FIELDS])

        def host_call(out=ho, **kw):
            a = dict(lo_p=lop, d_p=dp, o_p=o.ctypes.data, n=n, f_p=f.ctypes.data, m=nd, count=0xC, stop=0x2, budget=4096, o=C.byref(out))
            a.update(kw)
            return H.la3dm_devmap_gain_host(dm, a["lo_p"], a["d_p"], a["o_p"], a["n"], a["f_p"], a["m"], a["count"], a["stop"], a["budget"], a["o"], None)

        def dev_call(out, **kw):
            a = dict(lo_p=lop, d_p=dp, o_p=d_o.data_ptr(), n=n, f_p=d_f.data_ptr(), m=nd, count=0xC, stop=0x2, budget=4096, o=C.byref(out))
            a.update(kw)
            return H.la3dm_devmap_gain_device(dm, a["lo_p"], a["d_p"], a["o_p"], a["n"], a["f_p"], a["m"], a["count"], a["stop"], a["budget"], a["o"], None)
        # empty map: all zero, host and device pointers
        assert host_call() == OK, err()
        assert all((h[k] == 0).all() for k in G.FIELDS)
        t, do = tensors(9)
        assert dev_call(do) == OK, err()
        for k in G.FIELDS:
            g = t[k].cpu().numpy()
            assert (g[:-8] == 0).all() and (g[-8:] == 9).all(), k
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3,
                                                     0.1, 0.5, 8.0, None) == OK
        # refusals: LA3DM_ERR_ARG and a text that names the argument; nothing written
        for k in h:
            h[k][...] = 7
        t, do = tensors(7)
        cube = np.array((1 << 10, 1 << 10, 1 << 8), np.uint32)                       # exactly 2^28 voxels, 2^23 words
        lo_nan, lo_far = np.array((np.nan, 0, 0), np.float32), np.array((-3.0e5, 0, 0), np.float32)
        d_zero, d_over = np.array((4, 0, 4), np.uint32), np.array(((1 << 28) + 1, 1, 1), np.uint32)
        for call, out in ((host_call, ho), (dev_call, do)):
            for kw, text in ((dict(count=0), "count_mask must hold"), (dict(count=0x20), "count_mask must hold"),
                             (dict(count=0x8000000C), "count_mask must hold"), (dict(stop=0x22), "stop_mask must hold"),
                             (dict(budget=0), "max_steps must lie in"), (dict(budget=(1 << 20) + 1), "max_steps must lie in"),
                             (dict(m=0), "m must be >= 1"), (dict(n=1 << 20, m=257), "LA3DM_GAIN_MAX_RAYS"),
                             (dict(lo_p=None), "lo is NULL"), (dict(d_p=None), "dims is NULL"),
                             (dict(lo_p=lo_nan.ctypes.data), "lo must be finite"),
                             (dict(d_p=d_zero.ctypes.data), "dims must be >= 1"),
                             (dict(lo_p=lo_far.ctypes.data), "lo: the block field leaves"),
                             (dict(d_p=d_over.ctypes.data, o=None), "LA3DM_GAIN_MAX_CELLS"),
                             (dict(d_p=cube.ctypes.data, n=33, m=1, o=None), "LA3DM_GAIN_MAX_WORDS"),
                             (dict(d_p=cube.ctypes.data, n=32, m=1, o=None), "out is NULL"),      # at the limit: the next check answers
                             (dict(o_p=None), "origins3 is NULL"), (dict(f_p=None), "offsets3 is NULL"), (dict(o=None), "out is NULL"),
                             (dict(o=C.byref(_lib.GainOut(None, out.started, out.hits, out.seen))), "out->gain must not be NULL")):
                assert call(out, **kw) == ERR_ARG and text in err(), (kw, err())
            assert call(out, n=0, o_p=None, o=None) == OK, err()                     # n = 0: served, nothing written
        assert H.la3dm_devmap_gain_host(None, lop, dp, o.ctypes.data, n, f.ctypes.data, nd, 0xC, 0x2, 4096, C.byref(ho), None) == ERR_ARG
        assert all((h[k] == 7).all() for k in h) and all((t[k].cpu().numpy() == 7).all() for k in t)

        def free():
            torch.cuda.synchronize()
            return torch.cuda.mem_get_info()[0]
        # seen given: it is the working storage, the arena is not touched — nothing has been reserved for the sets so far
        t, do = tensors(0x5A5A5A5A)
        f0 = free()
        assert dev_call(do) == OK, err()
        f1 = free()
        print(f"free device memory before / after the first call, seen given: {f0} / {f1}")
        assert f1 >= f0, (f0, f1)
        assert host_call() == OK, err()                                               # (the host form reserves the arena)
        assert int(h["gain"].sum()) > 1000 and int(h["started"].sum()) > n * nd // 2 and 0 < int(h["hits"].sum()) < n * nd
        for k in G.FIELDS:
            g = t[k].cpu().numpy().view(np.uint32)
            assert (g[:-8].reshape(h[k].shape) == h[k]).all() and (g[-8:] == 0x5A5A5A5A).all(), k
        # the optional outputs NULL, in every combination with seen; 4 bytes off a 16-byte boundary
        for count, stop, budget in G.CASES:
            assert host_call(count=count, stop=stop, budget=budget) == OK, err()
            for fields in (("gain",), ("gain", "seen"), ("gain", "started"), ("gain", "hits", "seen")):
                t = {k: torch.full((n * W + 8,) if k == "seen" else (n + 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev) for k in G.FIELDS}
                torch.cuda.synchronize()
                do = _lib.GainOut(*[t[k][1:].data_ptr() if k in fields else None for k in G.FIELDS])
                assert dev_call(do, count=count, stop=stop, budget=budget) == OK, err()
                for k in G.FIELDS:
                    g = t[k].cpu().numpy().view(np.uint32)
                    if k in fields:
                        assert g[0] == 0x5A5A5A5A and (g[-7:] == 0x5A5A5A5A).all() and (g[1:-7].reshape(h[k].shape) == h[k]).all(), (k, fields)
                    else:
                        assert (g == 0x5A5A5A5A).all(), (k, fields)
        # storage: a large request reserved the arena; 20 more calls and a smaller request allocate nothing
        t, do = tensors(0, fields=("gain", "started", "hits"))
        assert dev_call(do) == OK, err()
        f0 = free()
        small = np.array((31, 17, 23), np.uint32)
        for i in range(10):
            assert dev_call(do, count=1 + (i & 3)) == OK, err()
            assert host_call(count=1 + (i & 3)) == OK, err()
        assert dev_call(do, d_p=small.ctypes.data, n=n // 2) == OK, err()
        assert host_call(d_p=small.ctypes.data, n=n // 2) == OK, err()
        f1 = free()
        print(f"free device memory before / after 20 calls and a smaller request: {f0} / {f1}")
        # the figure is the whole device's: a process of another user may release memory meanwhile, so growth is what fails
        assert f1 >= f0, (f0, f1)
        # still usable: another scan, the two forms agree again
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 2))
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3,
                                                     0.1, 0.5, 8.0, None) == OK
        t, do = tensors(0)
        assert host_call() == OK and dev_call(do) == OK, err()
        for k in G.FIELDS:
            assert (t[k].cpu().numpy().view(np.uint32)[:-8].reshape(h[k].shape) == h[k]).all(), k
    finally:
        H.la3dm_devmap_destroy(dm)


def test_planner_sized_call(built):
    """GPU test 5: 512 viewpoints (FREE voxels) x 1024 offsets of 4 m in one call: 8 randomly chosen viewpoints equal the
    host form on gain and seen; a second call gives identical arrays; no mirror refresh"""
    import la3dm_amd
    md, mh = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML), (1, 2))
    lo = R.recipe_lo()
    big = mh.box(lo, R.RECIPE_DIMS, fields=())
    rng = np.random.default_rng(41)
    free = np.argwhere(big["cls"] == R.FREE)
    pick = free[rng.choice(len(free), 512, replace=False)]
    origins = (big["origin"] + pick.astype(np.float32) * np.float32(mh.get_resolution())).astype(np.float32)
    offsets = G.fan(1024, 4.0)
    syncs = md.mirror_syncs()
    a = md.gain(lo, R.RECIPE_DIMS, origins, offsets, fields=G.FIELDS)
    b = md.gain(lo, R.RECIPE_DIMS, origins, offsets, fields=G.FIELDS)
    G.assert_same(a, b, "twice")
    assert (a["started"] == 1024).all() and int(a["gain"].sum()) > 0
    some = np.sort(rng.choice(512, 8, replace=False))
    gh = mh.gain(lo, R.RECIPE_DIMS, origins[some], offsets, fields=G.FIELDS)
    G.assert_same({k: a[k][some] for k in G.FIELDS}, gh, "8 of 512")
    print("gain of 8 of the 512 viewpoints:", gh["gain"].tolist())
    assert md.mirror_syncs() == syncs and md.is_device_resident()


def test_example_program(built):
    """GPU test 6: examples/next_view.cpp (built by build()) == the Python binding on the same map: the best viewpoint, its
    gain and the sum of gains; no mirror refresh"""
    import la3dm_amd
    exe = os.path.join(ROOT, "examples", "next_view")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "3"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    print(r.stdout)
    assert len(lines) == 2 and lines[0].startswith("best ") and lines[1].startswith("next_view 128 x 128 x 16 from ")
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    for i in (1, 2, 3):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        m.insert_pointcloud(xyz, origin, *INSERT)
    o = np.asarray(origin, np.float32)
    lo = np.array([o[0] - np.float32(6.4), o[1] - np.float32(6.4), o[2] - np.float32(0.8)], np.float32)
    dims = (128, 128, 16)
    g = m.frontier(lo, dims)
    dist = m.distance_field(lo, dims, radius=8, fields=("dist",))["dist"].reshape(-1)
    kept = g["index"][~(dist[g["index"]] < np.float32(0.3))]
    cand = kept[::(kept.size + 511) // 512]
    ijk = np.stack(np.unravel_index(cand, dims), 1).astype(np.float32)
    origins = (g["origin"] + ijk * np.float32(m.get_resolution())).astype(np.float32)
    u = (np.float32(-2.625) + np.float32(0.75) * np.arange(8, dtype=np.float32)).astype(np.float32)
    offsets = []
    for axis in range(3):
        for side in (-1, 1):
            for i in range(8):
                for j in range(8):
                    p = [0.0, 0.0, 0.0]
                    p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = 3.0 * side, u[i], u[j]
                    offsets.append(p)
    gain = m.gain(lo, dims, origins, np.array(offsets, np.float32))["gain"]
    best = int(np.argmax(gain))                                                    # the first of equals
    tok = lines[1].split()
    got = {tok[k]: tok[k + 1] for k in range(len(tok) - 1)}
    assert int(got["found"]) == g["n"] and int(got["kept"]) == kept.size > 0 and int(got["candidates"]) == cand.size > 0
    assert int(got["sum_gain"]) == int(gain.sum()) > 0
    assert got["mirror_syncs"] == "0" and got["device_resident"] == "1" and m.mirror_syncs() == 0
    bt = lines[0].split()
    assert int(bt[5]) == int(cand[best]) and int(bt[7]) == int(gain[best])
    assert np.allclose([float(v) for v in bt[1:4]], origins[best], atol=1e-4)
