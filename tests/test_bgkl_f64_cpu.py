"""CPU: the restatement's BGK-L path (oracle.l_predict = BGKLInference::predict in both sum modes, the kbar > 0.001f gate,
orc_node_update) against an independent float64 evaluation of the reference's formulas (tests/bgkl_f64_ref.py, numpy only) on
the hand-built scans of tests/helpers/bgkl_scans.py — the scans tests/test_bgkl_scans_gpu.py sends through every form of the
BGK-L kernels.  Every other BGK-L check compares the kernels with the restatement; this one would notice both misreading
point_to_line_dist, covSparseLine or the update loop the same way.

The bound is derived in bgkl_f64_ref's docstring; discontinuities are conditions, not tolerances: a (leaf, neighbour) pair
whose float64 kbar lies within its bound of 0.001 is left out of the gate comparison, a leaf whose float64 p or variance
lies within its bound of a threshold out of the state comparison, and at most 2 % of either may be left out per scan
(asserted on the reference alone).  Observed here: the restatement's alpha / beta reach at most 0.6 of their bound (the
share of u |alpha| in it is large where a leaf carries 5000 from earlier scans), ybar / kbar at most 0.1; no gate and at
most one state of a scan are left out.

Teeth: every row built as near (a hit or a crossing beam within a quarter of ell of a leaf) has a leaf where its own k
exceeds twice that leaf's kbar bound of the ordered mode — rows built just inside ell, just outside and far are exempt by
construction (k of a row at 0.97 ell is 2e-9 sf2) —, and the comparison rejects three mutants of the reference: a near row
dropped, the labels of one training block flipped, the leaf positions rotated by one lane.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import bgkl_f64_ref as R   # noqa: E402
import bgkl_scans as S     # noqa: E402

CONST = R.bgkl_constants()
PARAMS = {"yaml": R.L_YAML, "ell05": R.P5}
SHIFT = (2000.0, -1500.0, 30.0)
CASES = [("rows", d, k) for d in (2, 3, 4) for k in PARAMS] + [(c, 3, k) for c in ("cull", "cull far") for k in PARAMS]


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def results(O):
    """per case: the scan, the float64 answers and the restatement's, in both sum modes (computed once, never changed)"""
    luts = S.luts(O, R.L_YAML)
    out = {}
    for what, depth, k in CASES:
        P = PARAMS[k]
        sc = S.rows_scan(depth, P, luts[depth], CONST) if what == "rows" else \
            S.cull_scan(P, luts[3], SHIFT if what == "cull far" else (0.0, 0.0, 0.0))
        out[what, depth, k] = (sc, [R.scan64(sc, P, m) for m in (0, 1)], [S.expect_restatement(O, P, sc, m) for m in (0, 1)])
    return out


def check(got, f):
    """the comparison: node values and states (what the GPU test has), and the sums of every (leaf, neighbour)"""
    return R.compare(got[:3], f)[0] + R.compare_sums(got[3], got[4], f)[0]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_restatement_within_the_float64_bound(results, case):
    """both sum modes within the derived bound at every leaf, gates and states equal outside the excluded sets, and the
    reference alone leaves out at most 2 % of the gates and 2 % of the states"""
    sc, f64, rest = results[case]
    for mode in (0, 1):
        assert check(rest[mode], f64[mode]) == [], (case, mode)
        gate_share, state_share, n_gate, n_state = R.left_out(f64[mode])
        assert gate_share <= 0.02 and state_share <= 0.02, (case, mode, n_gate, n_state)
        assert np.isfinite(f64[mode]["eA"]).all() and np.isfinite(f64[mode]["eB"]).all()


def test_both_sides_of_the_gate_and_every_state_occur(results):
    """0 < kbar < 0.001 (rows present, no update) and kbar > 0.001; FREE, OCCUPIED and UNKNOWN, the last one also by the
    variance rule (p beyond a threshold, the variance above var_thresh) — each outside the excluded sets"""
    for k, P in PARAMS.items():
        D = R.derived(P)
        for depth in (3, 4):
            sc, f64, rest = results["rows", depth, k]
            f = f64[0]
            sure = f["live"] & ~f["gate_out"]
            assert (sure & (f["kbar"] > 0) & (f["kbar"] < R.GATE)).any() and (sure & (f["kbar"] > R.GATE)).any()
            ok = f["updated"] & ~f["state_out"]
            assert {R.FREE, R.OCCUPIED, R.UNKNOWN} <= set(f["state"][ok].tolist()), (k, depth)
            by_var = ok & (f["var"] > D["var_thresh"]) & ((f["p"] > D["occupied_thresh"]) | (f["p"] < D["free_thresh"]))
            assert by_var.any(), (k, depth)
            st = rest[0][2]
            assert (st[by_var] == (0x80 | R.UNKNOWN)).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_the_bound_has_something_to_say(results, case):
    """every near row has a leaf where its own k exceeds twice that leaf's kbar bound (ordered mode, the wider one)"""
    sc, f64, _ = results[case]
    f = f64[0]
    seen = np.zeros(len(sc.rows), bool)
    for t in range(len(sc.tests)):
        sl = sc.leaves_of(t)
        for q, tb in enumerate(sc.nbr[t]):
            if tb >= 0 and (t, int(tb)) in f["k"] and sc.sizes[tb]:
                seen[sc.rows_of(tb)] |= (f["k"][t, int(tb)] > 2.0 * f["ek"][sl, q][:, None]).any(0)
    near = np.isin(sc.kinds, S.NEAR)
    assert near.sum() >= 8 and seen[near].all(), (case, int(near.sum()), int((near & ~seen).sum()))


@pytest.mark.parametrize("k", list(PARAMS))
def test_the_comparison_can_fail(results, k):
    """the restatement's answer to the true scan against three mutants of the float64 reference: each is rejected, by the
    node values alone (what the device hands back) and by the full comparison"""
    P = PARAMS[k]
    sc, f64, rest = results["rows", 3, k]
    b = int(sc.nbr[0][0])                                       # the self block of the 64-leaf test block
    j = int(np.nonzero(np.isin(sc.blocks[b][1], S.NEAR))[0][0])
    rows, kinds = sc.blocks[b]
    dropped = list(sc.blocks)
    dropped[b] = (np.delete(rows, j, axis=0), np.delete(kinds, j))
    flipped = list(sc.blocks)
    lab = rows.copy()
    lab[:, 6] = 1.0 - lab[:, 6]
    flipped[b] = (lab, kinds)
    mutants = {"near row dropped": sc.rebuilt(dropped), "labels flipped": sc.rebuilt(flipped),
               "leaves rotated by one lane": sc.rebuilt(pos_roll=1)}
    for mode in (0, 1):
        assert check(rest[mode], f64[mode]) == []
        for name, m in mutants.items():
            f = R.scan64(m, P, mode)
            assert R.compare(rest[mode][:3], f)[0] != [], (name, mode)
            assert check(rest[mode], f) != [], (name, mode)


def test_every_class_is_hit():
    """the size lists follow the parsed constants: the row counts straddle the row trip and the item, reach 7, 8 and 9
    items; the leaf lists hold 1, 37, 63, 64 leaves at depth 3, 512 and 65 (a second tile of one leaf) at depth 4"""
    w, it = CONST["kWave"], CONST["kLItemRows"]
    ns = R.row_sizes(CONST)
    for t in (w, it):
        assert {t - 1, t, t + 1} <= set(ns)
    assert 2 * it + 1 in ns and {(n + it - 1) // it for n in ns} >= {1, 2, 3, 7, 8, 9}
    assert CONST["kLRing"] > 2 * w and CONST["kLItemRows"] % CONST["kLBatch"] == 0
    assert {1, w - 27, w - 1, w} <= set(x for x in S.LEAVES[3] if x != "pruned")
    assert {8 * w, w + 1} <= set(x for x in S.LEAVES[4] if x != "pruned")


def test_every_class_is_hit_by_the_scans(results):
    want = {"trip-1", "trip+0", "trip+1", "item-1", "item+0", "item+1", "two items and a row", "7 items", "8 items", "9 items",
            "empty training block", "no neighbour", "no self entry", "-1 between live slots", "pruned keys", "0 leaves", "1 leaves"}
    w = CONST["kWave"]
    for k, P in PARAMS.items():
        for depth in (2, 3, 4):
            sc = results["rows", depth, k][0]
            got = S.classes(sc, CONST)
            assert want <= got, (k, depth, sorted(want - got))
            if depth == 3:
                assert {f"{n} leaves" for n in (1, w - 27, w - 1, w)} <= got
            if depth == 4:
                assert {f"{8 * w} leaves", f"{w + 1} leaves", "last tile holds one leaf"} <= got
            # a threshold between the tile totals exists, and splits some tiles but not all
            mid = S.mid_threshold(sc, CONST)
            n_split, n_items, n_tiles = S.split_totals(sc, CONST, mid)
            assert 0 < n_split < S.split_totals(sc, CONST, 0)[0] <= n_tiles and n_items > 0
    # the hit ring flushes with a remainder and without one (ell = 0.5: every row reaches every leaf)
    rems = S.ring_flushes(results["rows", 3, "ell05"][0], R.P5, CONST)
    assert 0 in rems and any(r for r in rems), sorted(rems)
    # the cull scan: beams on both sides of the bounding sphere's reach, and a tile of one leaf (radius 0) elsewhere
    for k, P in PARAMS.items():
        for what in ("cull", "cull far"):
            sc = results[what, 3, k][0]
            c, rad = S.tile_sphere(sc.pos)
            ell = R.derived(P)["ell"]
            for kind, sign in (("I", -1), ("O", 1)):
                rows = sc.rows[sc.kinds == kind].astype(np.float64)
                d = R.dist64(np.float32([c]), sc.rows[sc.kinds == kind])[0][0]
                assert len(rows) > w and np.abs(d - (rad + ell + sign * 0.02)).max() < 2e-3, (k, what, kind)
