"""The production instance of the one-launch BGK scan (bgk_scan1_tile<0, true> behind bgk_predict_fuse_t1 / bgk_predict_fuse_t1s,
la3dm_amd/csrc/bgk_scan1_kernels.h): depth 3, one tile per block, leaf base 64 * blk, the default workgroup remap, x / ell by the
reciprocal, sf2 == 1, a gated scan and no profiling switch compiled in; t = r * 6.2831852f; the last column group of a table
sub-round through a trip that pushes its nr % 4 candidates only.  The yardstick is the two-launch path of the same build
("bgk_one_launch" 0), which shares none of that: alpha, beta and state equal bit for bit, on hand-built depth-3 scans of full
blocks (the builders of tests/test_bgk_one_launch_trim_gpu.py and tests/helpers/bgk_scans.py), each the smallest that can show
one piece wrong.  Which instance a call launched is read back (la3dm_get_option "bgk_scan1_instance": 2 production, 1 generic).

  point counts   M = 0, 1, 63, 64, 65, 128, 129 points in a tile's seven blocks (some of the seven ranges empty)
  neighbours     exactly one of the seven present (each), two adjacent slots of the row (each pair), all; a scan of a single block
  kept counts    one chunk whose cull keeps 1, 2, 3, 4, 5, 31, 32, 33, 36 points: nr % 4 = 1, 2, 3, 0 in a first and a second sub-round
  flushes        all 64 leaves in reach of 8 or more of 64 points: the ring passes its mark between the trips of a sub-round
  labels         all 0, all 1, mixed; a coordinate whose square overflows, a NaN coordinate
  dispatch       sf2 0.5, an ell the host divides by, remap 0, extra LDS, an ungated scan, fast_trig 1: the generic instance, same bits
  switch         "bgk_scan1_generic" 1 on the default configuration: the generic instance, the production instance's bits
  stamps         "time_kernel" 1 (the stamped production instance): same bits, one positive time per call
  t              the literal in the source is 0x40c90fda, and r * it == (r * 2) * 3.1415926f over the fp32 r of [0, 1] (CPU)"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bgk_f64_ref as R                      # noqa: E402
import bgk_scans as S                        # noqa: E402
import test_bgk_one_launch_trim_gpu as T     # noqa: E402

gpu = pytest.mark.gpu
P, CONST, FLAGS, KEYS, f32 = T.P, T.CONST, T.FLAGS, T.KEYS, np.float32
PROD, GENERIC = 2, 1
ELL_ALL_ONES = 0.24999998509883881   # fp32 0x3E7FFFFF: the context keeps inv_ell = 0 and the kernel divides (tests/test_bgk_one_launch_gpu.py)


class Ctx(T.Ctx):
    """T.Ctx with map parameters of the caller's and the launched instance read back"""

    def __init__(self, lut, **over):
        import torch
        from la3dm_amd import _lib
        self.torch, self.lib, self.H = torch, _lib, _lib.hip()
        q = dict(P, **over)
        p = _lib.Params(resolution=q["resolution"], block_depth=3, sf2=q["sf2"], ell=q["ell"], free_thresh=q["free_thresh"],
                        occupied_thresh=q["occupied_thresh"], var_thresh=q["var_thresh"], prior_A=q["prior_A"], prior_B=q["prior_B"],
                        device=0, lut_xyz=lut.ctypes.data, lut_count=len(lut), variant=0)
        h = C.c_void_p()
        assert self.H.la3dm_create(C.byref(p), C.byref(h)) == 0, self.H.la3dm_last_error(None).decode()
        self.h = h
        self.set(bgk_sum=1, bgk_tables=1, bgk_one_launch=1, fast_trig=0, time_kernel=0, bgk_scan1_generic=0, remap=2, lds_pad=0, ablate=0)

    def instance(self):
        v = C.c_int(-1)
        assert self.H.la3dm_get_option(self.h, b"bgk_scan1_instance", C.byref(v)) == 0
        return v.value

    def check(self, sc, flags=FLAGS, expect=PROD, timing=0, fast_trig=0, **opts):
        """the two launches and the one launch (options `opts` on) on the same scan: equal bit for bit, and the one launch ran
        the instance `expect`; returns the one launch's answer and its times"""
        ref, _ = self.run(sc, flags, 0, fast_trig=fast_trig)
        assert self.instance() == 0
        self.set(**opts)
        try:
            new, kt = self.run(sc, flags, 1, timing=timing, fast_trig=fast_trig)
            assert self.instance() == expect, (self.instance(), expect, opts)
        finally:
            self.set(bgk_scan1_generic=0, remap=2, lds_pad=0, ablate=0)
        T.assert_same_bits(ref, new, sc)
        return new, kt


@pytest.fixture(scope="module")
def lut(built):
    from oracle import oracle as O
    return S.luts(O, P, depths=(3,))[3]


@pytest.fixture(scope="module")
def ctx(lut):
    c = Ctx(lut)
    yield c
    c.close()


# ---- the scans ------------------------------------------------------------------------------------------------------------

def _slot_points(w, rng, ijk, s, n):
    """n points of slot s of test block ijk, the first half (rounded up) in reach of its leaves"""
    near = (n + 1) // 2
    if s == 0:
        p = np.concatenate([T._middle(w, ijk)[None] + S._jit(rng, near), w.centre(ijk) + rng.uniform(-0.19, 0.19, (n - near, 3))])
    else:
        p = np.concatenate([S._near_face(rng, w, ijk, s, T._middle(w, ijk), near), S._far_face(rng, w, ijk, s, n - near, P["ell"])])
    return p[rng.permutation(n)]


POINT_M = (0, 1, 63, 64, 65, 128, 129)


def counts_scan(lut):
    """per M a test block with all seven neighbours trained and M points spread over them (M < 7: empty ranges among them); then
    a block with no neighbour at all, M = 0 by another way"""
    w, rng = T._world(lut)
    for i, M in enumerate(POINT_M):
        ijk = (4 * i, 0, 0)
        for s, idx in enumerate(np.array_split(np.arange(M), 7)):
            w.add(np.add(ijk, S.DIRS[s]), _slot_points(w, rng, ijk, s, len(idx)), S._labels(rng, len(idx)), free=True)
        w.test(ijk, KEYS, *S.priors(rng, len(KEYS)))
    w.test((0, 40, 0), KEYS, *S.priors(rng, len(KEYS)))
    return w.build()


SUBSETS = [(s,) for s in range(7)] + [(s, s + 1) for s in range(6)] + [tuple(range(7))]


def neighbours_scan(lut, subsets=SUBSETS):
    """per subset a test block with 11 points in every slot of it except, where it has more than one, its last (an empty range);
    the other slots hold a trained block the row does not name"""
    w, rng = T._world(lut)
    for i, sub in enumerate(subsets):
        ijk = (4 * (i % 5), 4 * (i // 5), 0)
        for s in range(7):
            n = 0 if (len(sub) == 2 and s == sub[-1]) else 11
            w.add(np.add(ijk, S.DIRS[s]), _slot_points(w, rng, ijk, s, n), S._labels(rng, n), free=True)
        w.test(ijk, KEYS, *S.priors(rng, len(KEYS)), drop=set(range(7)) - set(sub))
    return w.build()


KEPT_N = (1, 2, 3, 4, 5, 31, 32, 33, 36)


def kept_scan(lut):
    """T.groups_scan with this file's counts: n points at the cube's middle (self block), 64 - n in the +x neighbour out of reach"""
    w, rng = T._world(lut)
    for k, n in enumerate(KEPT_N):
        ijk = (4 * k, 0, 0)
        w.add(ijk, T._middle(w, ijk)[None] + S._jit(rng, n), S._labels(rng, n))
        w.add(np.add(ijk, S.DIRS[1]), S._far_face(rng, w, ijk, 1, 64 - n, P["ell"]), S._labels(rng, 64 - n), free=True)
        w.test(ijk, KEYS, *S.priors(rng, len(KEYS)))
    return w.build()


def dense_scan(lut):
    """8 points at the middle of each 2 x 2 x 2 voxel group of a block: 64 points, every leaf in reach of 8 or more"""
    w, rng = T._world(lut)
    p = np.repeat(S._subcubes(w, (0, 0, 0)), 8, axis=0)
    w.add((0, 0, 0), p + S._jit(rng, len(p)), S._labels(rng, len(p)))
    w.test((0, 0, 0), KEYS, *S.priors(rng, len(KEYS)))
    return w.build()


def overflow_scan(lut):
    """T.nan_scan with a coordinate whose square overflows instead of the NaN"""
    sc = T.nan_scan(lut)
    bad = np.argwhere(np.isnan(sc.pts[:, :3]))
    assert len(bad) == 1
    sc.pts[bad[0][0], bad[0][1]] = f32(1e20)             # (1e20 / ell)^2 is past fp32
    return sc


# ---- the cases --------------------------------------------------------------------------------------------------------------

@gpu
def test_point_counts(ctx, lut):
    sc = counts_scan(lut)
    assert sc.full and sc.binary
    for t, M in enumerate(POINT_M):
        assert T.flat_count(sc, t) == M and (sc.nbr[t] >= 0).all()
        if M and M < 7:
            assert any(sc.sizes[b] == 0 for b in sc.nbr[t])
    assert (sc.nbr[len(POINT_M)] < 0).all()
    new, _ = ctx.check(sc)
    for t in (0, len(POINT_M)):                                                  # the M == 0 exit: state 0, nothing else written
        sl = sc.leaves_of(t)
        assert (new[2][sl] == 0).all() and (new[0][sl] == sc.a0[sl]).all() and (new[1][sl] == sc.b0[sl]).all()
    for t in range(1, len(POINT_M)):
        assert (new[2][sc.leaves_of(t)] & 0x80).any(), POINT_M[t]


@gpu
def test_neighbour_subsets(ctx, lut):
    sc = neighbours_scan(lut)
    for t, sub in enumerate(SUBSETS):
        assert {s for s in range(7) if sc.nbr[t][s] >= 0} == set(sub)
        assert T.flat_count(sc, t) == 11 * (len(sub) - (len(sub) == 2))
    new, _ = ctx.check(sc)
    assert all((new[2][sc.leaves_of(t)] & 0x80).any() for t in range(len(SUBSETS)))


@gpu
def test_a_single_block(ctx, lut):
    sc = neighbours_scan(lut, [(0,)])
    assert len(sc.tests) == 1 and len(sc.blocks) == 7 and (sc.nbr[0][1:] < 0).all() and sc.nbr[0][0] >= 0
    ctx.check(sc)


@gpu
def test_kept_counts(ctx, lut):
    sc = kept_scan(lut)
    assert sc.full and sc.binary
    for t, n in enumerate(KEPT_N):
        keep, _ = T.cull_keeps(sc, t)
        assert T.flat_count(sc, t) == 64 and int(keep.sum()) == n and keep[:n].all(), (n, int(keep.sum()))
        hit, _ = T.pair_hits(sc, t)
        assert not hit[:, n:].any() and hit[:, :n].any(axis=0).all()
    rounds = [[min(32, n - b) for b in range(0, n, 32)] for n in KEPT_N]
    assert {r[0] % 4 for r in rounds if len(r) == 1} == {0, 1, 2, 3} and {r[1] % 4 for r in rounds if len(r) == 2} == {0, 1}
    assert {(r[0] + 3) // 4 for r in rounds} >= {1, 2, 8}
    ctx.check(sc)


@gpu
def test_a_flush_between_the_trips_of_a_sub_round(ctx, lut):
    sc = dense_scan(lut)
    hit, pts = T.pair_hits(sc, 0)
    keep, _ = T.cull_keeps(sc, 0)
    assert T.flat_count(sc, 0) == 64 and keep.all()
    assert (hit.sum(axis=1) >= 8).all()                                          # every leaf is in reach of 8 or more points
    room = CONST["kRingT"] - 4 * CONST["kWave"]
    per_trip = hit.sum(axis=0).reshape(16, 4).sum(axis=1)                        # entries pushed by each of the 2 x 8 trips
    assert (per_trip[:8].cumsum()[:7] > room).any() and (per_trip[8:].cumsum()[:7] > room).any()   # drained before a sub-round's last trip
    assert set(np.unique(pts[:, 3])) == {0.0, 1.0}
    ctx.check(sc)


@gpu
@pytest.mark.parametrize("label", (0, 1))
def test_one_label(ctx, lut, label):
    ctx.check(T.flush_scan(lut, label))


@gpu
@pytest.mark.parametrize("what", ("nan", "overflow"))
def test_a_point_at_no_finite_distance(ctx, lut, what):
    sc = T.nan_scan(lut) if what == "nan" else overflow_scan(lut)
    _, md = T.cull_keeps(sc, 0)
    assert int((~np.isfinite(md)).sum()) == 1 and np.isfinite(T.cull_keeps(sc, 1)[1]).all()
    new, _ = ctx.check(sc)
    assert (new[2][:64] == 0).all() and (new[0][:64] == sc.a0[:64]).all() and (new[1][:64] == sc.b0[:64]).all()
    assert np.isfinite(new[0][64:]).all() and (new[2][64:] & 0x80).any()


@gpu
@pytest.mark.parametrize("case", ("sf2", "ell", "remap", "lds_pad", "ungated", "fast_trig"))
def test_what_the_generic_instance_keeps(ctx, lut, case):
    sc = T.chunks_scan(lut)[0]
    if case in ("sf2", "ell"):
        c = Ctx(lut, **({"sf2": 0.5} if case == "sf2" else {"ell": ELL_ALL_ONES}))
        try:
            c.check(sc, expect=GENERIC)
        finally:
            c.close()
    elif case == "remap":
        ctx.check(sc, expect=GENERIC, remap=0)
    elif case == "lds_pad":
        ctx.check(sc, expect=GENERIC, ablate=0, lds_pad=4096)
    elif case == "ungated":
        ctx.check(T.exits_scan(lut), FLAGS | R.UNGATED, expect=GENERIC)
    else:
        ctx.check(sc, expect=GENERIC, fast_trig=1)


@gpu
def test_the_switch_and_the_stamped_instance(ctx, lut):
    sc = T.chunks_scan(lut)[0]
    prod, _ = ctx.check(sc)
    gen, _ = ctx.check(sc, expect=GENERIC, bgk_scan1_generic=1)
    T.assert_same_bits(prod, gen, sc, "forced generic ")
    stamped, kt = ctx.check(sc, timing=1)
    T.assert_same_bits(prod, stamped, sc, "time_kernel 1 ")
    print(f"time_kernel 1: {kt} ms")
    assert kt.size == 1 and np.isfinite(kt).all() and (kt > 0).all(), kt


# ---- no GPU -------------------------------------------------------------------------------------------------------------------

def test_the_literal_of_t_and_the_identity():
    """t = (r * 2.0f) * 3.1415926f == r * 6.2831852f: r * 2 is exact, 2 * RN(3.1415926) = 0x40c90fda is a float and the literal
    rounds to it, so both forms round the same real product once — that is the proof; the sweep takes every seventh fp32 r of
    [0, 1] (every r would be 2^30 values) and every r of the first and the last 2^20"""
    with open(os.path.join(ROOT, "la3dm_amd", "csrc", "bgk_scan1_kernels.h")) as fh:
        src = fh.read()
    body = src[src.index("float scan1_cov_unit(float r) {"):]
    lit = re.search(r"const float t = r \* ([0-9.]+)f;", body[:body.index("}")])
    assert lit, "scan1_cov_unit no longer forms t in one multiply"
    k = f32(lit.group(1))
    assert int(k.view(np.uint32)) == 0x40c90fda
    assert k == f32(2) * f32(3.1415926) and int(f32(3.1415926).view(np.uint32)) == 0x40490fda
    one = int(f32(1).view(np.uint32))
    pi = f32(3.1415926)
    for lo, hi, step in ((0, one + 1, 7), (0, 1 << 20, 1), (one + 1 - (1 << 20), one + 1, 1)):
        for b in range(lo, hi, step << 24):
            r = np.arange(b, min(b + (step << 24), hi), step, dtype=np.uint32).view(f32)
            assert np.array_equal((r * f32(2)).astype(f32) * pi, r * k), (lo, hi, step, b)
