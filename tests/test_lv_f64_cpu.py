"""CPU: the restatement's BGK-LV voxel body (oracle.OracleLVMap.packed_scan: the gather order, the full search for a ray's
lowest-index sample in the box, both sum modes, the gate, lv_update) against an independent float64 evaluation of the
reference's formulas (tests/lv_f64_ref.py, numpy only) on the hand-built scans of tests/helpers/lv_scans.py — the scans
tests/test_lv_scans_gpu.py sends through the BGK-LV kernels.  Every other BGK-LV check compares the kernels with the
restatement; this one would notice both misreading bgklvinference.h or the LV node the same way.

The bound is derived in lv_f64_ref's docstring; discontinuities are conditions, not tolerances: a voxel whose float64 kbar
lies within its bound of 0.001 is left out of the gate comparison, a voxel whose float64 p or variance lies within its bound
of a threshold, or which sits on a branch of get_prob, out of the state comparison, and at most 2 % of either may be left out
per scan (asserted on the reference alone).  LA3DM_LV_HAS_INFO is compared everywhere.

Teeth: every near row (a hit or a ray within a quarter of ell of an active voxel) has a voxel where its own k exceeds twice
that voxel's kbar bound, and the comparison rejects seven misreadings of the reference (lv_f64_ref.MUTANTS), each from alpha,
beta and the state alone, without the HAS_INFO bit.  The packer is checked against the library's own arrays.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import lv_f64_ref as R   # noqa: E402
import lv_scans as S     # noqa: E402

from conftest import pcd_path   # noqa: E402

CONST = R.lv_constants()
IDS = ["-".join(map(str, c)) for c in S.CASES]


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def results(O):
    """per case: the scan, what its builder says about it, the float64 answers and the restatement's, in both sum modes
    (computed once, never changed)"""
    luts = S.luts(O, R.LV_YAML)
    out = {}
    for case in S.CASES:
        sc, extra = S.build_case(case, luts, CONST)
        P = S.params(case)
        out[case] = (sc, extra, [R.scan64(sc, P, m) for m in (0, 1)], [S.expect_restatement(O, sc, m) for m in (0, 1)])
    return out


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_restatement_within_the_float64_bound(results, case):
    """both sum modes within the derived bound at every voxel, HAS_INFO equal everywhere, gates and states equal outside the
    excluded sets, and the reference alone leaves out at most 2 % of the gates and 2 % of the states"""
    sc, _, f64, rest = results[case]
    for mode in (0, 1):
        bad, worst = R.compare(rest[mode], f64[mode])
        assert bad == [], (case, mode, bad)
        assert worst <= 1.0
        gate_share, state_share, n_gate, n_state = R.left_out(f64[mode])
        assert gate_share <= 0.02 and state_share <= 0.02, (case, mode, n_gate, n_state)
        assert np.isfinite(f64[mode]["eA"]).all() and np.isfinite(f64[mode]["eB"]).all()


def test_every_class_is_hit(results):
    """the size lists follow the parsed constants, and the scans hit every class the GPU test's docstring names"""
    ch, w, t, d = CONST["kLvChunk"], CONST["kWave"], CONST["kLvAddRows"], CONST["kLvAddDepth"]
    assert R.stream_sizes(CONST) == [ch - 1, ch, ch + 1, 2 * ch, 2 * ch + 1, 3 * ch + 5]
    assert {15, 16, 17, w - 1, w, w + 1, 2 * w + 1} <= set(R.kept_sizes(CONST))
    assert R.split_row_sizes(CONST) == [t - 1, t, t + 1, d * t, d * t + 1] and d * t + 1 <= ch
    got = {case: S.classes(results[case][0], CONST) for case in S.CASES}
    every = set().union(*got.values())
    streams = {"stream " + n for n in ("chunk-1", "chunk", "chunk+1", "2 chunks", "2 chunks+1", "3 chunks+5")}
    want = streams | {f"{k} kept candidates" for k in R.kept_sizes(CONST)} | {f"{k} rows in a sub-task" for k in R.split_row_sizes(CONST)} | {
        "sub-task boundary inside a bucket", "sub-task boundary on a bucket boundary", "sub-task boundary on a group boundary",
        "sub-task spans two groups", "sub-task all culled", "round with no hit row", "hit rows in consecutive rounds",
        "uncounted candidates between counted ones", "a ray with 1 samples in a box", "a ray with 2 samples in a box",
        "a ray with many samples in a box", "first sample in the box", "first sample in the core box",
        "previous sample in another bucket", "previous sample in another group", "previous sample outside the stream",
        "a sample in the outer box but in no voxel's box", "64 active", "37 active", "1 active", "cube with no active voxel",
        "block with no sample in reach", "a block's buckets partly outside the grid", "empty bucket", "two blocks share buckets",
        "split and unsplit cubes in one block", "split and unsplit cubes in one plan wave",
        "split and unsplit cubes in different plan waves", "split cubes in several plan waves",
        "split cubes in several plan workgroups"} | {f"{n} cubes" for n in (15, 16, 17, 63, 64, 65)} | {
        f"neighbourhood sticks out at the {s} side of axis {a}" for s in ("low", "high") for a in range(3)}
    assert want <= every, sorted(want - every)
    # every stream length at every depth, the plan's classes where a block holds several cubes
    for case in S.CASES:
        if case[0] in ("stream", "stream far"):
            assert streams <= got[case], (case, sorted(streams - got[case]))
            assert {"sub-task all culled", "sub-task boundary inside a bucket", "sub-task boundary on a bucket boundary"} <= got[case], case
            if case[1] >= 4:
                assert {"split and unsplit cubes in one block", "split and unsplit cubes in different plan waves"} <= got[case], case
            if (2 * results[case][0].reach + 1) ** 3 > CONST["kLvGroup"] and case[1] <= 3:
                assert {"sub-task boundary on a group boundary", "sub-task spans two groups"} <= got[case], case
        if case[0] in ("dedupe", "dedupe far"):
            assert {"a ray with 1 samples in a box", "a ray with 2 samples in a box", "a ray with many samples in a box",
                    "first sample in the box", "first sample in the core box", "previous sample in another bucket"} <= got[case], case
    # reach 1, 2 and 3; one cube of 8 nodes, one cube, 8 cubes and 64 cubes per block
    assert {results[c][0].reach for c in S.CASES if c[1] >= 3} == {1, 2, 3}
    assert {results[c][0].npb for c in S.CASES} == {8, 64, 512, 4096}


def test_both_sides_of_the_gate_every_state_and_rows_out_of_reach(results):
    """kbar below and above 0.001 and every output state, UNCERTAIN included, outside the excluded sets; UNKNOWN only below
    min_W; a voxel whose only rows lie at or beyond ell: kbar < 0, HAS_INFO, not updated, alpha and beta untouched"""
    D = R.derived(R.LV_YAML)
    seen_states = set()
    for case in S.CASES:
        sc, extra, f64, rest = results[case]
        f = f64[0]
        ok = f["updated"] & ~f["state_out"]
        seen_states |= set(f["state"][ok].tolist())
        unknown = ok & (f["state"] == R.UNKNOWN)
        assert (f["A"][unknown] + f["B"][unknown] < D["min_W"]).all()
        if case[0] in ("dedupe", "stream"):
            # every branch of point_to_line_dist: a segment shorter than 0.0001, a voxel before the start, beyond the end, beside it
            assert all(v > 0 for v in f["branches"].values()), (case, f["branches"])
        if case[0] == "dedupe":
            only = f["info"] & (f["kbar"] < 0) & ~f["gate_out"]
            assert only.any(), case
            for mode in (0, 1):
                a, b, st = rest[mode]
                assert (st[only] == R.HAS_INFO).all() and (a[only] == sc.a0[only]).all() and (b[only] == sc.b0[only]).all()
        if case[0] == "node":
            k = f["kbar"][extra]
            sure = ~f["gate_out"][extra]
            assert (sure & (k > 0) & (k < R.GATE)).any() and (sure & (k > R.GATE) & (k < 0.0011)).any()
            s = (f["A"] + f["B"])[extra]
            upd = f["updated"][extra]
            assert (upd & (s < D["min_W"])).any() and (upd & (s > D["min_W"])).any() and (upd & (f["B"][extra] < 0)).any()
    assert seen_states == {R.FREE, R.OCCUPIED, R.UNKNOWN, R.UNCERTAIN}


@pytest.mark.parametrize("case", [c for c in S.CASES if c[0].startswith("face")], ids=lambda c: "-".join(map(str, c)))
def test_box_faces(results, case):
    """a sample exactly on fl(c + ell) or fl(c - ell) is in the box, the next float beyond is not: on each axis, at a corner,
    as a hit and as the only sample of a ray whose segment runs through the voxel's centre (alpha unchanged, beta + sf2)"""
    sc, want, f64, rest = results[case]
    assert len(want) == 24 and sum(on for _, on in want) == 12
    sf2 = R.derived(S.params(case))["sf2"]
    for mode in (0, 1):
        a, b, st = rest[mode]
        for node, on in want:
            assert bool(f64[mode]["info"][node]) == on and bool(st[node] & R.HAS_INFO) == on, (node, on)
        rays = [node for node, on in want[16:] if on]
        assert len(rays) == 4 and all(abs(float(b[n]) - float(sc.b0[n]) - sf2) < 1e-6 for n in rays)
        assert all(b[n] == sc.b0[n] for n, on in want[16:] if not on)


@pytest.mark.parametrize("case", [c for c in S.CASES if c[0] in ("stream", "dedupe", "kept")], ids=lambda c: "-".join(map(str, c)))
def test_the_bound_has_something_to_say(results, case):
    """every near row has a voxel where its own k exceeds twice that voxel's kbar bound (ordered mode, the wider one)"""
    sc, _, f64, _ = results[case]
    f = f64[0]
    hits = np.isin(sc.kinds, S.NEAR) & (sc.samples[:, 3] < 0) & f["row_hit"]
    rays = np.isin(sc.ray_kinds, S.NEAR) & f["row_ray"]
    assert hits.sum() + rays.sum() >= 8
    assert f["seen_hit"][hits].all() and f["seen_ray"][rays].all(), (case, int((hits & ~f["seen_hit"]).sum()), int((rays & ~f["seen_ray"]).sum()))
    # nearly all of them are rows at all
    assert f["row_hit"][np.isin(sc.kinds, S.NEAR) & (sc.samples[:, 3] < 0)].mean() > 0.9
    assert f["row_ray"][np.isin(sc.ray_kinds, S.NEAR)].mean() > 0.9


def _values_only(bad):
    return [b for b in bad if b[0] != "has_info"]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_comparison_can_fail(results, mutant):
    """the restatement's answer to the true scan against a misreading of the reference: rejected on at least one scan, in
    both sum modes, from alpha, beta and the state alone"""
    cases = [c for c in S.CASES if c[1] == 3 and c[2] == 0.2 and c[0] in ("stream", "dedupe", "face", "node", "kept")]
    for mode in (0, 1):
        caught = []
        for case in cases:
            sc, _, f64, rest = results[case]
            assert R.compare(rest[mode], f64[mode])[0] == []
            if _values_only(R.compare(rest[mode], R.scan64(sc, S.params(case), mode, mutant=mutant))[0]):
                caught.append(case[0])
        assert caught, (mutant, mode)


def _array(ptr, n, dtype):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * np.dtype(dtype).itemsize,)).view(dtype).copy()


@pytest.mark.parametrize("depth", [3, 4])
def test_packer_against_the_library(O, depth):
    """the helper's packer, written from the contract comment, against the arrays a host-mode map packs for one cloud"""
    import la3dm_amd
    P = dict(la3dm_amd.LV_YAML, block_depth=depth)
    m = la3dm_amd.BGKLVOctoMap(**P, device=-1)
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_unstructured", 1))
    assert m.lv_prepare(xyz[::4], origin, 0.1, 0.1, 8.0)
    s, r = m.lv_training()
    pk = m.lv_packed()
    n, nb = int(pk.n_samples), int(pk.n_blk)
    ncell = int(np.prod([pk.cell_dim[i] for i in range(3)]))
    centres = _array(pk.blk_center, 3 * nb, np.float32).reshape(-1, 3)
    sc = S.from_arrays(depth, P, S.luts(O, R.LV_YAML)[depth], s, r, centres)
    assert n == len(sc.samples) and nb == sc.n_blk and int(pk.n_rays) == len(sc.rays8)
    assert [pk.cell_min[i] for i in range(3)] == sc.cell_min.tolist() and [pk.cell_dim[i] for i in range(3)] == sc.cell_dim.tolist()
    assert (_array(pk.cell_off, ncell + 1, np.uint32) == sc.cell_off).all()
    assert (_array(pk.sorted, 4 * n, np.uint32) == sc.sorted.view(np.uint32).ravel()).all()
    assert (_array(pk.samples, 4 * n, np.uint32) == sc.samples.view(np.uint32).ravel()).all()
    assert (_array(pk.rays, 8 * len(sc.rays8), np.uint32) == sc.rays8.view(np.uint32).ravel()).all()
    assert (_array(pk.blk_cell0, 3 * nb, np.int32).reshape(-1, 3) == sc.blk_cell0).all()
    assert (centres.view(np.uint32) == sc.blk_center.view(np.uint32)).all()
