"""clusters on the device-resident map: members from the device pool or a list, rounds of brick relaxations in LDS (min
over the adjacent members' labels), sizes, the scan over the kept roots, labels and records (csrc/devmap_clusters.h).  The
yardstick is the host form of the same class (a host-mode map, a flood fill over box's classes), itself checked against
scipy's labelling over a walk of the leaf list (tests/helpers/clusters_cases.py).  The answer is integer and unique: every
comparison is exact.  What is expected of the diagnostics (rounds, brick runs, capped runs) comes from the helper's numpy
model of the scheme."""
import ctypes as C
import os
import sys
import subprocess
import time

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, pcd_path

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import region_cases as R  # noqa: E402
import reach_cases as RC  # noqa: E402
import clusters_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

OK = 0
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured
DIMS = R.RECIPE_DIMS
FIELDS = ("label", "of_member")
_PAIRS = {}


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


def _bgk_pair(depth=3):
    import la3dm_amd
    if depth not in _PAIRS:
        _PAIRS[depth] = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML, block_depth=depth), (1, 2))
    return _PAIRS[depth]


def _compare(md, mh, lo, dims, what, members=None, **kw):
    """device == host on every output, the contract's stats and the info; returns both answers"""
    fields = FIELDS if members is not None else ("label",)
    gd = md.clusters(lo, dims, members=members, fields=fields, **kw)
    gh = mh.clusters(lo, dims, members=members, fields=fields, **kw)
    K.assert_same(gd, gh, (what, dims, kw))
    R.assert_same(gd, gh, ("origin", "cell"), what)
    assert gd["block_key"] == gh["block_key"] and md.is_device_resident()
    assert gd["brick_runs"] >= gd["rounds"] and gd["capped"] <= gd["brick_runs"]
    return gd, gh


def _queries(md, mh, lo, cls, listed, what, yard):
    """CPU test 1's queries: device == host, and (yard) host == yardstick"""
    out = {}
    for c in K.CONNECTIVITIES:
        for tile in K.TILES:
            for min_size in (1, 8):
                q = dict(connectivity=c, tile=tile, min_size=min_size)
                gd, gh = _compare(md, mh, lo, DIMS, what, members=listed, **q)
                if yard:
                    K.assert_same(gh, K.yardstick(cls, K.FREE_M, listed, c, tile, min_size), ("host form vs yardstick", what, q))
                out[(c, tile, min_size)] = gd
    for mask in (K.OCC_M, K.FREE_M):
        gd, gh = _compare(md, mh, lo, DIMS, what, member=mask, connectivity=26)
        if yard:
            K.assert_same(gh, K.yardstick(cls, mask), ("host form vs yardstick, classes", what, mask))
        assert gd["n"] >= 1
    q = dict(connectivity=26, tile=8, min_size=8)
    full = out[(26, 8, 8)]
    few, _ = _compare(md, mh, lo, DIMS, what + " cap below n", members=listed, cap=40, **q)
    assert few["n"] == full["n"] > 40 and all((few[k] == full[k][:40]).all() for k in K.RECORDS)
    none, _ = _compare(md, mh, lo, DIMS, what + " cap 0", members=listed, cap=0, **q)
    assert none["n"] == full["n"] and none["first"].size == 0
    again = np.concatenate([listed[::-1], listed[::3], [DIMS[0] * DIMS[1] * DIMS[2], 0xFFFFFFFF]]).astype(np.uint32)
    twice, _ = _compare(md, mh, lo, DIMS, what + " reversed, with duplicates", members=again, **q)
    assert all((twice[k] == full[k]).all() for k in K.RECORDS + ("label",)) and twice["n_members"] == full["n_members"]
    return out


@pytest.mark.parametrize("depth", [3, 4])
def test_device_equals_host_bit_for_bit(built, depth):
    """GPU test 1: BGK at block_depth 3 and 4, two fused (and pruned) scans, the recipe region: CPU test 1's queries,
    device == host on every output; the host form == the yardstick on that map, with the input conditions first; rounds,
    brick runs and capped runs of the untiled connectivity-6 query and of tile 8 at connectivity 26 are the helper's
    model's — the first needs more rounds than one batch and hits the inner cap; no mirror refresh"""
    md, mh = _bgk_pair(depth)
    lo, cls, listed, _ = K.recipe(mh, mh.leaves(), ("gpu", depth))
    cond = K.input_conditions(cls, listed, key=("gpu", depth))
    K.assert_exercises_the_feature(cond)
    before = md.mirror_syncs()
    assert (md.frontier(lo, DIMS)["index"] == listed).all()
    got = _queries(md, mh, lo, cls, listed, f"bgk d{depth}", True)
    for (tile, c), model in cond["model"].items():
        gd = got[(c, tile, 1)]
        print(f"depth {depth} tile {tile} connectivity {c}: device {[gd[k] for k in K.DIAG]}, the model {model}")
        assert tuple(gd[k] for k in K.DIAG) == tuple(model[k] for k in K.DIAG), ([gd[k] for k in K.DIAG], model)
    untiled = got[(6, 0, 1)]
    assert untiled["rounds"] > K.BATCH and untiled["capped"] >= 1
    assert md.mirror_syncs() == before


@pytest.mark.parametrize("depth", [3, 4])
def test_device_equals_host_after_a_further_insert(built, depth):
    """GPU test 2: a third insert (the pool grew, the table was rebuilt) and the same queries; the answer changed"""
    import la3dm_amd
    md, mh = _pair("BGKOctoMap", dict(la3dm_amd.BGK_YAML, block_depth=depth), (1, 2))
    lo = R.recipe_lo()
    first = md.clusters(lo, DIMS, members=md.frontier(lo, DIMS)["index"], tile=8, min_size=8)
    before_syncs, before = md.mirror_syncs(), mh.block_count()
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 5))
    for m in (md, mh):
        m.insert_pointcloud(xyz, origin, *INSERT)
    assert mh.block_count() > before
    listed = mh.frontier(lo, DIMS)["index"]
    got = _queries(md, mh, lo, None, listed, f"bgk d{depth} after a further insert", False)
    assert got[(26, 8, 8)]["n"] != first["n"] or (got[(26, 8, 8)]["label"] != first["label"]).any()
    assert md.mirror_syncs() == before_syncs


def test_hand_built_sets(built):
    """GPU test 3: CPU test 2's sets through the device form — on an empty device-resident map and 100 m from the scans of
    a non-empty one (every voxel MISSING there: the probes run) — against the yardstick and, for the diagnostics, the
    model: the snake hits the inner cap in a single brick; a list with 0 entries; both entry points of the device
    library, _host and _device, on a bare devmap; a smaller region after a larger one reuses the arena"""
    import torch
    import la3dm_amd
    from la3dm_amd import _lib
    md, _ = _bgk_pair()
    empty = la3dm_amd.BGKOctoMap(**dict(la3dm_amd.BGK_YAML, block_depth=3), device=0)
    assert md.leaves()["A"].size > 0 and empty.is_device_resident()
    far = RC.far_lo(md, R.recipe_lo())
    assert (md.box(far, (33, 16, 41), fields=())["cls"] == R.MISSING).all()
    syncs = md.mirror_syncs()
    near = np.array((0.05, 0.05, 0.05), np.float32)
    t0, calls = time.perf_counter(), 0
    for name, dims, voxels, tile, expect in K.hand_sets():
        cls = np.full(dims, R.MISSING, np.uint8)
        listed = np.array([K.flat(v, dims) for v in voxels], np.uint32)
        member = K.members_of(cls, K.MISS_M, listed)
        for c in K.CONNECTIVITIES:
            want = K.yardstick(cls, K.MISS_M, listed, c, tile)
            model = K.brick_model(member, c, tile)
            for m, lo in ((empty, near), (md, far)) if c == 26 else ((empty, near),):    # (the probes: one connectivity is enough)
                got = m.clusters(lo, dims, members=listed, member=K.MISS_M, connectivity=c, tile=tile, fields=FIELDS)
                calls += 1
                K.assert_same(got, want, (name, c, m is md))
                assert expect is None or got["n"] == expect[c], (name, c, got["n"])
                assert tuple(got[k] for k in K.DIAG) == tuple(model[k] for k in K.DIAG), (name, c, [got[k] for k in K.DIAG], model)
            if c == 6:
                big = empty.clusters(near, dims, members=listed, member=K.MISS_M, connectivity=c, tile=tile, min_size=len(voxels) + 1)
                assert big["n"] == 0 and (big["label"] == K.NONE).all() and big["n_dropped"] == want["n"]
            if name == "a snake in one brick":
                assert model["capped"] >= 1 and model["brick_runs"] >= model["rounds"] >= 2, model   # one brick, run after run
            if name == "a hollow shell":
                assert want["rep"][0] == K.flat((1, 3, 3), dims)
    print(f"hand-built sets: {calls} device calls with their yardsticks and models in {time.perf_counter() - t0:.2f} s")
    for m, lo in ((empty, near), (md, far)):
        none = m.clusters(lo, (9, 8, 17), members=np.zeros(0, np.uint32), member=K.MISS_M, fields=FIELDS)
        assert none["n"] == 0 and none["n_members"] == 0 and (none["label"] == K.NONE).all() and none["rounds"] == 0
        every = m.clusters(lo, (9, 8, 17), member=K.MISS_M, connectivity=6)
        assert every["n"] == 1 and every["size"][0] == 9 * 8 * 17 and (every["label"] == 0).all()
    assert md.mirror_syncs() == syncs and empty.mirror_syncs() == 0
    # both entry points of the device library on a bare devmap with one scan: a larger region, then a smaller one
    H = _lib.hip()
    mc = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)   # (lends its context)
    ctx = mc.ctx()
    dm = C.c_void_p()
    assert H.la3dm_devmap_create(ctx, C.byref(dm)) == OK
    dev = torch.device("cuda:0")
    try:
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 1))
        lo = (np.asarray(origin, np.float32) + np.asarray(R.RECIPE_OFFSET, np.float32)).astype(np.float32)
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3, *INSERT, None) == OK
        names = [k for k, _ in _lib.ClustersOut._fields_]
        for dims, mask in ((np.array((77, 67, 39), np.uint32), K.FREE_M), (np.array((31, 17, 23), np.uint32), 0xE)):
            n = int(dims.prod())
            cls = np.zeros(n, np.uint8)
            assert H.la3dm_devmap_box_host(dm, lo.ctypes.data, dims.ctypes.data, C.byref(_lib.BoxOut(cls.ctypes.data, None, None, None)), None) == OK
            listed = np.concatenate([np.flatnonzero(K.members_of(cls, mask))[::2], [n, 0xFFFFFFFF]]).astype(np.uint32)
            want = K.yardstick(cls.reshape(tuple(int(v) for v in dims)), mask, listed, 18, 8, 2)
            cap = want["n"] + 3
            assert want["n"] > 5, (dims, want["n"], listed.size)
            sizes = dict(label=n, of_member=listed.size, first=cap, size=cap, lo=3 * cap, hi=3 * cap, sum=3 * cap, rep=cap)
            h = {k: np.full(sizes[k], 7, np.uint64 if k == "sum" else np.uint32) for k in names}
            d_list = torch.from_numpy(listed.view(np.int32)).to(dev)
            t = {k: torch.full((sizes[k],), 7, dtype=torch.int64 if k == "sum" else torch.int32, device=dev) for k in names}
            torch.cuda.synchronize()
            for fn, out, mem in ((H.la3dm_devmap_clusters_host, _lib.ClustersOut(*[h[k].ctypes.data for k in names]), listed.ctypes.data),
                                 (H.la3dm_devmap_clusters_device, _lib.ClustersOut(*[t[k].data_ptr() for k in names]), d_list.data_ptr())):
                p = _lib.ClustersParams(mask, 1, 18, 8, 2, listed.size, mem, cap)
                found, stats = C.c_uint32(0), _lib.ClustersStats()
                assert fn(dm, lo.ctypes.data, dims.ctypes.data, C.byref(p), C.byref(out), C.byref(found), C.byref(stats), None) == OK, H.la3dm_last_error(ctx).decode()
                assert found.value == want["n"] == stats.n_clusters and stats.n_members == want["n_members"] and stats.largest == want["largest"]
            g = {k: v.cpu().numpy().view(np.uint64 if k == "sum" else np.uint32) for k, v in t.items()}
            for k in names:
                m_ = want["n"] * (3 if k in ("lo", "hi", "sum") else 1)
                w = want[k].reshape(-1)
                for got in (h[k], g[k]):
                    if k in ("label", "of_member"):
                        assert (got == w).all(), (k, dims)
                    else:
                        assert (got[:m_] == w).all() and (got[m_:] == 7).all(), (k, dims)    # past n nothing is written
    finally:
        H.la3dm_devmap_destroy(dm)


def test_batch_boundaries(built):
    """Lines of 8 B k + {-1, 0, 1, 2} voxels, k = 1, 2, B = LA3DM_CLUSTERS_BATCH, along each axis, every voxel a member, at
    connectivity 6 and untiled, on the empty map and 100 m from the scans of a non-empty one (the probes run): the smallest
    label crosses one brick per round, so the query ends before, on and after the end of a batch of rounds.  One cluster;
    the outputs against the yardstick; rounds, brick runs and capped runs as the helper's model counts them"""
    import la3dm_amd
    md, _ = _bgk_pair()
    empty = la3dm_amd.BGKOctoMap(**dict(la3dm_amd.BGK_YAML, block_depth=3), device=0)
    assert md.leaves()["A"].size > 0 and empty.is_device_resident()
    B = la3dm_amd.CLUSTERS_BATCH
    assert B == K.BATCH and la3dm_amd.CLUSTERS_BRICK == K.BRICK and la3dm_amd.CLUSTERS_INNER == K.INNER
    far = RC.far_lo(md, R.recipe_lo())
    assert (md.box(far, (3, 3, 16 * B + 2), fields=())["cls"] == R.MISSING).all()
    syncs = md.mirror_syncs()
    rounds_seen = set()
    for length in [8 * B * k + d for k in (1, 2) for d in (-1, 0, 1, 2)]:
        for axis in range(3):
            dims = [1, 1, 1]
            dims[axis] = length
            cls = np.full(dims, R.MISSING, np.uint8)
            want = K.yardstick(cls, K.MISS_M, None, 6)
            model = K.brick_model(np.ones(dims, bool), 6)
            assert model["capped"] == 0
            for m, lo in ((empty, np.array((0.05, 0.05, 0.05), np.float32)), (md, far)):
                got = m.clusters(lo, dims, member=K.MISS_M, connectivity=6)
                assert got["n"] == 1 and (got["label"] == 0).all() and got["size"][0] == length, (dims, m is md)
                K.assert_same(got, want, (dims, m is md))
                assert tuple(got[k] for k in K.DIAG) == tuple(model[k] for k in K.DIAG), (dims, m is md, [got[k] for k in K.DIAG], model)
                rounds_seen.add(got["rounds"])
    assert {B, B + 1, 2 * B, 2 * B + 1} <= rounds_seen, rounds_seen
    assert md.mirror_syncs() == syncs and empty.mirror_syncs() == 0


def test_count_ring_wrap(built):
    """A line of 8 * 1024 + 9 members on the empty map: the smallest label crosses one brick per round, so the query runs
    past round 1024, where the ring of per-round counts in the working storage is cleared and used again.  The brick runs
    are a recorded figure: the helper's model (K.brick_model on this line, connectivity 6, untiled) gave rounds 1026, brick
    runs 528901, capped 0 — it takes about a minute on the CPU, so it is not run here"""
    import la3dm_amd
    empty = la3dm_amd.BGKOctoMap(**dict(la3dm_amd.BGK_YAML, block_depth=3), device=0)
    dims = (1, 1, 8 * 1024 + 9)
    g = empty.clusters(np.array((0.05, 0.05, 0.05), np.float32), dims, member=K.MISS_M, connectivity=6)
    print(f"ring wrap: device {[g[k] for k in K.DIAG]}")
    assert g["n"] == 1 and (g["label"] == 0).all() and g["size"][0] == dims[2] and g["n_members"] == dims[2]
    assert tuple(g[k] for k in K.DIAG) == (1026, 528901, 0)
    assert empty.is_device_resident() and empty.mirror_syncs() == 0


@pytest.mark.parametrize("variant", ["GPOctoMap", "BGKLOctoMap", "BGKLVOctoMap"])
def test_device_equals_host_on_other_variants(built, variant):
    """GPU test 4: GP, BGK-L and BGK-LV on their own configurations: the frontier's list at tile 8 and the FREE voxels
    untiled, against the host-mode twin and the yardstick over the twin's own box"""
    import la3dm_amd
    params, insert = {"GPOctoMap": (la3dm_amd.GP_YAML, INSERT), "BGKLOctoMap": (la3dm_amd.L_YAML, (0.1, 0.3, 8.0)),
                      "BGKLVOctoMap": (la3dm_amd.LV_YAML, (0.1, 0.3, 8.0))}[variant]
    md, mh = _pair(variant, dict(params), (1, 2), insert)
    lo = R.recipe_lo()
    cls = mh.box(lo, DIMS, fields=())["cls"]
    listed = mh.frontier(lo, DIMS)["index"]
    assert listed.size > 100
    _, gh = _compare(md, mh, lo, DIMS, variant, members=listed, connectivity=26, tile=8, min_size=8)
    K.assert_same(gh, K.yardstick(cls, K.FREE_M, listed, 26, 8, 8), (variant, "host form vs the yardstick over its own box"))
    _, gh = _compare(md, mh, lo, DIMS, variant + " classes", member=K.FREE_M | (1 << R.UNCERTAIN), connectivity=6)
    K.assert_same(gh, K.yardstick(cls, K.FREE_M | (1 << R.UNCERTAIN), None, 6), (variant, "classes"))


def test_example_program(built):
    """examples/goal_clusters.cpp (built by build()) == the Python binding on the same map: the summary line and the
    cheapest representatives"""
    import la3dm_amd
    exe = os.path.join(ROOT, "examples", "goal_clusters")
    r = subprocess.run([exe, os.path.join(GOLDEN, "data", "sim_structured"), "sim_structured", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    print(r.stdout)
    assert lines[-1].startswith("goal_clusters 128 x 128 x 16 from ") and all(ln.startswith("cluster ") for ln in lines[:-1])
    m = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0)
    for i in (1, 2, 3):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        m.insert_pointcloud(xyz, origin, *INSERT)
    before = m.mirror_syncs()
    o = np.asarray(origin, np.float32)
    lo = np.array([o[0] - np.float32(6.4), o[1] - np.float32(6.4), o[2] - np.float32(0.8)], np.float32)
    dims = (128, 128, 16)
    res = np.float32(m.get_resolution())
    fr = m.frontier(lo, dims)
    d2 = m.distance_field(lo, dims, obstacles=("occupied",), radius=2, fields=("d2",))["d2"].reshape(-1)
    kept = fr["index"][d2[fr["index"]] == la3dm_amd.DF_FAR]
    g = m.clusters(lo, dims, members=kept, connectivity=26, tile=8, min_size=8, fields=())
    s = [int(min(max(np.floor((o[a] - fr["origin"][a]) / res + np.float32(0.5)), 0), dims[a] - 1)) for a in range(3)]
    t = m.travel(lo, dims, [K.flat(s, dims)], targets=g["rep"], fields=(), clearance=1, soft_radius=4, penalty=40)
    assert m.is_device_resident() and m.mirror_syncs() == before
    ok = t["target_cost"] != la3dm_amd.TRAVEL_NONE
    tok = lines[-1].split()
    got = {tok[k]: tok[k + 1] for k in range(len(tok) - 1)}
    assert int(got["found"]) == fr["n"] > 0 and int(got["kept"]) == kept.size > 0 and int(got["clusters"]) == g["n"] > 0
    assert int(got["dropped"]) == g["n_dropped"] and int(got["largest"]) == g["largest"] and int(got["reachable"]) == int(ok.sum())
    assert got["mirror_syncs"] == "0" and got["device_resident"] == "1" and len(lines) == min(5, int(ok.sum())) + 1
    order = np.flatnonzero(ok)[np.argsort(t["target_cost"][ok], kind="stable")[:5]]
    for ln, c in zip(lines[:-1], order):
        tk = ln.split()
        p = fr["origin"] + np.array(np.unravel_index(g["rep"][c], dims), np.float32) * res
        assert int(tk[1]) == c and int(tk[3]) == g["size"][c] and np.allclose([float(v) for v in tk[5:8]], p, atol=1e-4) and int(tk[9]) == t["target_cost"][c], (ln, c)
