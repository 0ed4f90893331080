"""CPU: the restatement's BGK path (oracle.bgk_predict = BGKInference::predict, the kbar > 0 gate, orc_node_update; in sum
mode 1 the same fp32 terms summed in float64 over all seven neighbours) against an independent float64 evaluation of the
reference's formulas (tests/bgk_f64_ref.py, numpy only) on the hand-built scans of tests/helpers/bgk_scans.py — the scans
tests/test_bgk_scans_gpu.py sends through every BGK predict + fuse kernel.  Every other BGK check compares the kernels with
the restatement; this one would notice both misreading the distance, covSparse or the update loop the same way.

The bound is derived in bgk_f64_ref's docstring; discontinuities are conditions, not tolerances: a gate whose float64
kbar is positive but at most its bound is left out of the gate comparison, a leaf whose float64 p or variance lies within
its bound of a threshold out of the state comparison, and at most 2 % of either may be left out per scan (asserted on the
reference alone).  The test prints the restatement's worst fraction of the bound per scan and mode, and the left-out counts.

Teeth: the comparison rejects three mutants of the reference's inputs (one neighbour's points dropped, a label flipped, the
leaf positions rotated by one lane), and every class of edge the scans were built for is hit by some scan at every depth
where it applies (helpers/bgk_scans.classes, from the constants parsed out of the kernel header).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import bgk_f64_ref as R   # noqa: E402
import bgk_scans as S     # noqa: E402

CONST = R.bgk_constants()
CASES = S.cases()
TAGS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def results(O):
    """per case, lazily and once: the scan, the float64 answers and the restatement's, in both sum modes (never changed)"""
    luts = S.luts(O, R.BGK_YAML)
    by_tag = {c[0]: c for c in CASES}
    cache = {}

    def get(tag):
        if tag not in cache:
            _, depth, k, make, ungated = by_tag[tag]
            P = S.PARAMS[k]
            sc = make(luts[depth], CONST)
            pairs = {}
            cache[tag] = (sc, P, [R.scan64(sc, P, m, ungated, cache=pairs) for m in (0, 1)],
                          [S.expect_restatement(O, P, sc, m, ungated) for m in (0, 1)])
        return cache[tag]
    return get


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_within_the_float64_bound(results, tag):
    """both sum modes within the derived bound at every leaf, gates and states equal outside the excluded sets, and the
    reference alone leaves out at most 2 % of the gates and 2 % of the states"""
    sc, P, f64, rest = results(tag)
    line = []
    for mode in (0, 1):
        bad, worst = R.compare(rest[mode], f64[mode])
        gate_share, state_share, n_gate, n_state = R.left_out(f64[mode])
        line.append(f"mode {mode}: {worst:.3f} of the bound, left out (gates, states) ({n_gate}, {n_state}) = "
                    f"({100 * gate_share:.2f} %, {100 * state_share:.2f} %)")
        assert bad == [], (tag, mode, bad)
        assert gate_share <= 0.02 and state_share <= 0.02, (tag, mode, n_gate, n_state, gate_share, state_share)
        assert np.isfinite(f64[mode]["eA"]).all() and np.isfinite(f64[mode]["eB"]).all()
    print(f"\nBGK-F64-CPU {tag}: leaves {sc.keys.size}; " + "; ".join(line))


def test_the_bound_is_not_vacuous(results):
    """somewhere the restatement uses more than a hundredth of its bound, in either mode; and a leaf out of reach of everything
    is compared, not left out: kbar exactly 0, bound 0, state byte 0"""
    worst = [0.0, 0.0]
    for tag in ("counts d3 yaml", "faces d4 yaml", "reach d3 yaml translated"):
        sc, P, f64, rest = results(tag)
        for mode in (0, 1):
            worst[mode] = max(worst[mode], R.compare(rest[mode], f64[mode])[1])
            f = f64[mode]
            dead = f["live"].any(1) & ~f["updated"] & ~f["updated_out"]
            assert dead.any() and (f["eA"][dead] == 0).all() and (rest[mode][2][dead] == 0).all()
            assert (rest[mode][0][dead] == sc.a0[dead]).all() and (rest[mode][1][dead] == sc.b0[dead]).all()
    assert min(worst) > 0.01, worst


DEPTHS = {2: ["counts d2", "lists d2"], 3: ["counts d3", "rings d3", "labels d3", "reach d3", "ungated d3", "lists d3"],
          4: ["counts d4", "rings d4", "labels d4", "reach d4", "ungated d4", "lists d4", "faces d4"],
          5: ["counts d5", "lists d5", "faces d5"]}


def test_every_class_is_hit_by_the_scans(results):
    """(a)-(h): per depth, the union over the scans of that depth holds every class that applies there"""
    vals = R.count_values(CONST)
    w = CONST["kWave"]
    for depth, prefixes in DEPTHS.items():
        got = set()
        for tag in TAGS:
            if any(tag.startswith(p) for p in prefixes):
                sc, P, _, _ = results(tag)
                assert sc.depth == depth
                got |= S.classes(sc, CONST, P)
        want = {f"{n}={v}" for n in "MS" for v in vals} | {"M~300", "S~300", "trip over 1 neighbours", "trip over 2 neighbours",
                                                          "trip over 3 neighbours", "hits and free samples", "full block",
                                                          "pruned keys", "one leaf", "no leaves", "no neighbour"}
        if depth <= 4:
            want |= {"no self entry", "-1 between live slots", "empty neighbour between live ones", "training block in several slots"}
        if depth >= 3:
            want |= {f"{n}={v} table" for n in "MS" for v in vals}
        if depth in (3, 4):
            want |= {"d2 == 0 with label 1", "d2 == 0 with label 0", "d2 == 0 on one axis with label 1", "non-binary labels"}
            for ring in ("kRing5", "kRingR", "kRingT"):
                want |= {f"{ring} below", f"{ring} above"} | ({f"{ring} at"} if CONST[ring] % w == 0 else set())
        want |= {2: {"8 live lanes"}, 3: {"64 live lanes", "37 live lanes", "1 live lanes"}, 4: {"corner cube", "1 live lanes"},
                 5: {"corner cube", "edge cube", "face cube", "interior cube"}}[depth]
        assert want <= got, (depth, sorted(want - got))


def test_the_cases_follow_the_constants():
    t, w = CONST["kTabSlots"], CONST["kWave"]
    assert {0, 1, t // 2 - 1, t // 2, t // 2 + 1, t - 1, t, t + 1, w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1} == set(R.count_values(CONST))
    n = R.ring_counts(CONST)
    for ring in ("kRing5", "kRingR", "kRingT"):
        assert any(w * x < CONST[ring] for x in n) and any(w * x > CONST[ring] for x in n) and max(n) < 10
        assert CONST[ring] % w or CONST[ring] // w in n
    assert 1.02 < R.R0 < 1.04 and abs(CONST["hit_t"] - 0.96778184) < 1e-7


@pytest.mark.parametrize("tag", ["counts d3 yaml", "faces d4 ell04", "labels d3 non-binary"])
def test_the_comparison_can_fail(results, tag):
    """the restatement's answer to the true scan against three mutants of the float64 reference's inputs: each is rejected"""
    sc, P, f64, rest = results(tag)
    t = int(np.argmax([sc.leaf_off[i + 1] - sc.leaf_off[i] > 0 and max(sc.nbr[i]) >= 0 and
                       sum(sc.sizes[b] for b in sc.nbr[i] if b >= 0) >= 15 for i in range(len(sc.tests))]))
    D = R.derived(P)
    b = max((int(x) for x in sc.nbr[t] if x >= 0 and sc.sizes[x]),        # the neighbour that adds the most
            key=lambda x: R.pairs64(sc.pos[sc.leaves_of(t)], sc.blocks[x], D)[0].sum())
    dropped = list(sc.blocks)
    dropped[b] = sc.blocks[b][:0]
    flipped = list(sc.blocks)
    lab = sc.blocks[b].copy()
    j = int(np.argmax(R.pairs64(sc.pos[sc.leaves_of(t)], lab, R.derived(P))[0].max(0)))     # the point with the largest k
    lab[j, 3] = 1.0 - lab[j, 3] if lab[j, 3] != 0.5 else -0.5
    flipped[b] = lab
    mutants = {"one neighbour's points dropped": sc.rebuilt(dropped), "a label flipped": sc.rebuilt(flipped),
               "leaves rotated by one lane": sc.rebuilt(pos_roll=1)}
    for mode in (0, 1):
        assert R.compare(rest[mode], f64[mode])[0] == []
        for name, m in mutants.items():
            assert R.compare(rest[mode], R.scan64(m, P, mode))[0] != [], (tag, name, mode)


def test_non_finite_points_in_the_restatement(O):
    """(i): what the restatement does with a NaN coordinate and a point at 3e19 m (helpers/bgk_scans.nonfinite_scan): the
    neighbour that holds them is rejected at every leaf in mode 0, the others stand; mode 1 updates nothing"""
    lut = S.luts(O, R.BGK_YAML, (3,))[3]
    sc = S.nonfinite_scan(R.BGK_YAML, lut)
    a0, b0, st0 = S.expect_restatement(O, R.BGK_YAML, sc, 0)
    clean = S.Scan(3)
    clean.blocks = sc.blocks
    clean.tests = [dict(t, nbr=[x if s != 3 else -1 for s, x in enumerate(t["nbr"])]) for t in sc.tests]
    clean.pack(lut)
    for x, y in zip((a0, b0, st0), S.expect_restatement(O, R.BGK_YAML, clean, 0)):
        assert (x.view(np.uint8) == y.view(np.uint8)).all()
    assert ((st0 & 0x80) != 0).any()
    a1, b1, st1 = S.expect_restatement(O, R.BGK_YAML, sc, 1)
    assert (st1 == 0).all() and (a1 == sc.a0).all() and (b1 == sc.b0).all()
    assert ((S.expect_restatement(O, R.BGK_YAML, clean, 1)[2] & 0x80) != 0).any()
