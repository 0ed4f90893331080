"""The one-launch BGK scan (bgk_predict_fuse_t1 / bgk_predict_fuse_t1s, la3dm_amd/csrc/bgk_scan1_kernels.h) after its bookkeeping was
trimmed: the constant addends of the sin / cos polynomials come from vcc, alpha / beta / state / the stamp record are read again
from the kernel arguments on the way out, the eight column groups of a table sub-round are eight trips with immediate offsets,
and the cull's masks are the compares' own ballots.  None of that may change a bit: the yardstick is the two-launch path of the
same build ("bgk_one_launch" 0: bgk_prepare + bgk_predict_fuse_t<.., false>, which shares none of the changed code), equal bit for
bit in alpha, beta and state, on hand-built depth-3 scans of full blocks (tests/helpers/bgk_scans.py) aimed at each changed place:

  group counts   one 64-point chunk whose cull keeps exactly n points, n = 1, 4, 5, 16, 17, 28, 29, 32, 33: 1 to 8 column groups,
                 with and without padding, and the second sub-round of a chunk
  flushes        32 survivors that reach 32 leaves each: every trip pushes 128 entries, the ring is drained inside every group;
                 with label 0 and with label 1; at fast_trig 0, 1, 2, 3 (every instance of the kernel)
  chunk counts   M = 64, 65, 128, 129, 192, 193 with the missing neighbour in the first, a middle and the last slot
  exits          an M == 0 block as the first and as the last block, gated and ungated; "time_kernel" 0, 1 and 2 (the plain
                 instance, the stamped one, the plain one between events) give the same bits, 1 returns one time per call
  non-finite     one NaN coordinate in an ordinary tile: NaN sums; gated, the leaves are left alone

What a case is about is asserted on the CPU first, from the points alone (fp32, the kernel's own association).  The source of the
evaluation is compared too: the constant words the one-launch header moves into vcc are the words of bgk_kernels.h's addends."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import bgk_f64_ref as R   # noqa: E402
import bgk_scans as S     # noqa: E402

gpu = pytest.mark.gpu

P = R.BGK_YAML            # ell = 0.2: from a cube's middle the leaves at 0.087 and 0.166 m are in reach, those at 0.218 and 0.260 m are not
CONST = R.bgk_constants()
FLAGS = R.LABELS_01 | R.FULL_BLOCKS
KEYS = S.full_keys(3)
f32 = np.float32


# ---- what the kernel will see, from the points alone ----------------------------------------------------------------

def _scaled(x, ell):
    return (np.asarray(x, f32) / f32(ell)).astype(f32)


def pair_hits(sc, t):
    """[leaf, point] of test block t: d2 < T with d2 = dx^2 + (dy^2 + dz^2) in fp32 on coordinates divided by ell (the B stage)"""
    pts = np.concatenate([sc.pts[sc.pts_of(b)] for b in sc.nbr[t] if b >= 0] + [np.zeros((0, 4), f32)])
    xs, xn = _scaled(sc.pos[sc.leaves_of(t)], P["ell"]), _scaled(pts[:, :3], P["ell"])
    with np.errstate(invalid="ignore", over="ignore"):
        d = (xn[None] - xs[:, None]).astype(f32)
        q = (d * d).astype(f32)
        d2 = (q[..., 0] + (q[..., 1] + q[..., 2]).astype(f32)).astype(f32)
        return d2 < f32(CONST["hit_t"]), pts


def cull_keeps(sc, t):
    """per point of test block t (flat order): does the A stage keep it — the minimum per axis over the 64 leaves, mx + (my + mz) < T"""
    pts = np.concatenate([sc.pts[sc.pts_of(b)] for b in sc.nbr[t] if b >= 0] + [np.zeros((0, 4), f32)])
    xs, xn = _scaled(sc.pos[sc.leaves_of(t)], P["ell"]), _scaled(pts[:, :3], P["ell"])
    with np.errstate(invalid="ignore", over="ignore"):
        d = (xn[None] - xs[:, None]).astype(f32)
        m = (d * d).astype(f32).min(axis=0)              # [point, axis]
        md = (m[:, 0] + (m[:, 1] + m[:, 2]).astype(f32)).astype(f32)
        return md < f32(CONST["hit_t"]), md


def flat_count(sc, t):
    return int(sum(sc.sizes[b] for b in sc.nbr[t] if b >= 0))


# ---- the scans ------------------------------------------------------------------------------------------------------------

def _world(lut):
    return S.World(3, lut), np.random.default_rng(7300)


def _middle(w, ijk):
    cc, n = S.cube_centres(w, ijk)
    assert n == 1                                        # depth 3: the block is one 4 x 4 x 4 cube
    return cc[(0, 0, 0)]


GROUP_N = (1, 4, 5, 16, 17, 28, 29, 32, 33)


def groups_scan(lut):
    """per n a test block whose 64 points are one chunk: n at the cube's middle (self block), 64 - n in the +x neighbour out of reach"""
    w, rng = _world(lut)
    for k, n in enumerate(GROUP_N):
        ijk = (4 * k, 0, 0)
        w.add(ijk, _middle(w, ijk)[None] + S._jit(rng, n), S._labels(rng, n))
        w.add(np.add(ijk, S.DIRS[1]), S._far_face(rng, w, ijk, 1, 64 - n, P["ell"]), S._labels(rng, 64 - n), free=True)
        w.test(ijk, KEYS, *S.priors(rng, len(KEYS)))
    return w.build()


def flush_scan(lut, label):
    """32 points at the cube's middle, all with one label, + a block of mixed labels so that both accumulators are in play"""
    w, rng = _world(lut)
    w.add((0, 0, 0), _middle(w, (0, 0, 0))[None] + S._jit(rng, 32), np.full(32, label, f32))
    w.test((0, 0, 0), KEYS, *S.priors(rng, len(KEYS)))
    p = S._subcubes(w, (4, 0, 0))
    w.add((4, 0, 0), p + S._jit(rng, len(p)), S._labels(rng, len(p)))
    w.test((4, 0, 0), KEYS, *S.priors(rng, len(KEYS)))
    return w.build()


CHUNK_M = (64, 65, 128, 129, 192, 193)
MISSING = (0, 3, 6)


def chunks_scan(lut):
    """per (M, missing slot) a test block whose other six neighbours hold M points together, half of them in reach"""
    w, rng = _world(lut)
    want = []
    for i, M in enumerate(CHUNK_M):
        for j, gone in enumerate(MISSING):
            ijk = (4 * i, 4 * j, 0)
            live = [s for s in range(7) if s != gone]
            for s, idx in zip(live, np.array_split(np.arange(M), len(live))):
                n, near = len(idx), (len(idx) + 1) // 2
                if s == 0:
                    p = np.concatenate([_middle(w, ijk)[None] + S._jit(rng, near), w.centre(ijk) + rng.uniform(-0.19, 0.19, (n - near, 3))])
                else:
                    p = np.concatenate([S._near_face(rng, w, ijk, s, _middle(w, ijk), near), S._far_face(rng, w, ijk, s, n - near, P["ell"])])
                w.add(np.add(ijk, S.DIRS[s]), p[rng.permutation(n)], S._labels(rng, n), free=True)
            if gone:                                     # a trained block stands there, the row says -1
                w.add(np.add(ijk, S.DIRS[gone]), S._near_face(rng, w, ijk, gone, _middle(w, ijk), 9), S._labels(rng, 9), free=True)
            w.test(ijk, KEYS, *S.priors(rng, len(KEYS)), drop={gone})
            want.append((M, gone))
    return w.build(), want


def exits_scan(lut):
    """M == 0 blocks as the first and the last of the arrays, two trained blocks between them"""
    w, rng = _world(lut)
    w.test((40, 0, 0), KEYS, *S.priors(rng, len(KEYS)))
    for k in range(2):
        p = S._subcubes(w, (4 * k, 0, 0))
        w.add((4 * k, 0, 0), p + S._jit(rng, len(p)), S._labels(rng, len(p)))
        w.test((4 * k, 0, 0), KEYS, *S.priors(rng, len(KEYS)))
    w.test((80, 0, 0), KEYS, *S.priors(rng, len(KEYS)))
    return w.build()


def nan_scan(lut):
    """an ordinary tile (40 points at the middles of its voxel groups, 30 opposite a face) with one NaN coordinate, and a clean one"""
    w, rng = _world(lut)
    for k in range(2):
        ijk = (4 * k, 0, 0)
        p = np.repeat(S._subcubes(w, ijk), 5, axis=0)
        p = p + S._jit(rng, len(p))
        if k == 0:
            p[17, 1] = np.nan
        w.add(ijk, p, S._labels(rng, len(p)), free=True)
        w.add(np.add(ijk, S.DIRS[3]), S._near_face(rng, w, ijk, 3, _middle(w, ijk), 30), S._labels(rng, 30))
        w.test(ijk, KEYS, *S.priors(rng, len(KEYS)))
    return w.build()


# ---- running them -------------------------------------------------------------------------------------------------------

class Ctx:
    """a bare depth-3 context; scans go through la3dm_bgk_scan_device on arrays resident on the device"""

    def __init__(self, lut):
        import torch
        from la3dm_amd import _lib
        self.torch, self.lib, self.H = torch, _lib, _lib.hip()
        p = _lib.Params(resolution=P["resolution"], block_depth=3, sf2=P["sf2"], ell=P["ell"], free_thresh=P["free_thresh"],
                        occupied_thresh=P["occupied_thresh"], var_thresh=P["var_thresh"], prior_A=P["prior_A"], prior_B=P["prior_B"],
                        device=0, lut_xyz=lut.ctypes.data, lut_count=len(lut), variant=0)
        h = C.c_void_p()
        assert self.H.la3dm_create(C.byref(p), C.byref(h)) == 0, self.H.la3dm_last_error(None).decode()
        self.h = h
        self.set(bgk_sum=1, bgk_tables=1, bgk_one_launch=1, fast_trig=0, time_kernel=0)

    def set(self, **opts):
        for name, v in opts.items():
            assert self.H.la3dm_set_option(self.h, name.encode(), int(v)) == 0, name

    def close(self):
        self.torch.cuda.synchronize()
        self.H.la3dm_destroy(self.h)

    def run(self, sc, flags, one, timing=0, fast_trig=0):
        """one scan from the scan's own priors -> ((alpha, beta, state), the times la3dm_kernel_times returns)"""
        torch, dev = self.torch, self.torch.device("cuda", 0)
        self.set(bgk_one_launch=one, time_kernel=timing, fast_trig=fast_trig)

        def up(a):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)

        t = dict(train_xyzy=up(sc.pts), train_off=up(sc.train_off), nbr=up(sc.nbr), blk_center=up(sc.centre), leaf_off=up(sc.leaf_off),
                 leaf_key=up(sc.keys), alpha=up(sc.a0), beta=up(sc.b0),
                 state=torch.full((sc.keys.size,), 0x55, dtype=torch.uint8, device=dev))   # (0x55: a leaf no kernel wrote shows)
        s, cnt = self.lib.BgkScan(), self.lib.BgkCounters()
        for k, v in t.items():
            setattr(s, k, v.data_ptr())
        s.n_train_pts, s.n_train_blk, s.n_test_blk, s.n_leaf = int(sc.train_off[-1]), len(sc.blocks), len(sc.tests), int(sc.keys.size)
        s.flags = flags
        try:
            rc = self.H.la3dm_bgk_scan_device(self.h, C.byref(s), torch.cuda.current_stream().cuda_stream, C.byref(cnt))
            assert rc == 0, self.H.la3dm_last_error(self.h)
            torch.cuda.synchronize()
            assert (int(cnt.scratch_bytes) == 0) == bool(one), "the launch form the case is about did not run"
            kt, n = np.full(4, np.nan, f32), C.c_uint32(99)
            assert self.H.la3dm_kernel_times(self.h, kt.ctypes.data, 4, C.byref(n)) == 0
        finally:
            self.set(bgk_one_launch=1, time_kernel=0, fast_trig=0)
        return tuple(t[k].cpu().numpy().copy() for k in ("alpha", "beta", "state")), kt[:int(n.value)]

    def both(self, sc, flags=FLAGS, fast_trig=0):
        """the two launches and the one launch on the same scan: equal bit for bit; returns the one launch's answer"""
        ref, _ = self.run(sc, flags, 0, fast_trig=fast_trig)
        new, _ = self.run(sc, flags, 1, fast_trig=fast_trig)
        assert_same_bits(ref, new, sc)
        return new


def assert_same_bits(ref, new, sc, what=""):
    for name, x, y in zip(("alpha", "beta", "state"), ref, new):
        bad = np.flatnonzero(x.view(np.uint8 if x.dtype == np.uint8 else np.uint32) != y.view(np.uint8 if y.dtype == np.uint8 else np.uint32))
        blocks = sorted({int(np.searchsorted(sc.leaf_off, i, side="right")) - 1 for i in bad})
        print(f"{what}{name}: {bad.size} of {x.size} differ (test blocks {blocks})")
        assert bad.size == 0, (what, name, blocks)


@pytest.fixture(scope="module")
def lut(built):
    from oracle import oracle as O
    return S.luts(O, P, depths=(3,))[3]


@pytest.fixture(scope="module")
def ctx(lut):
    c = Ctx(lut)
    yield c
    c.close()


# ---- the cases --------------------------------------------------------------------------------------------------------------

@gpu
def test_group_counts(ctx, lut):
    sc = groups_scan(lut)
    assert sc.full and sc.binary
    for t, n in enumerate(GROUP_N):
        keep, md = cull_keeps(sc, t)
        assert flat_count(sc, t) == 64 and keep.size == 64                      # one chunk
        assert int(keep.sum()) == n and keep[:n].all(), (n, int(keep.sum()))    # the cull keeps the n points at the middle
        hit, _ = pair_hits(sc, t)
        assert not hit[:, n:].any() and hit[:, :n].any(axis=0).all()            # the rest is beyond every leaf's support
        groups, pad = (min(n, 32) + 3) // 4, (-min(n, 32)) % 4
        print(f"n = {n}: {groups} column groups, {pad} padded slots, {'two sub-rounds' if n > 32 else 'one sub-round'}")
    assert {(min(n, 32) + 3) // 4 for n in GROUP_N} == {1, 2, 4, 5, 7, 8}       # the first and the last trip of either table half
    new = ctx.both(sc)
    assert (new[2] & 0x80).reshape(-1, 64).any(axis=1).all()                    # every block was updated somewhere


@gpu
@pytest.mark.parametrize("label", (0, 1))
def test_a_flush_in_every_group(ctx, lut, label):
    sc = flush_scan(lut, label)
    hit, pts = pair_hits(sc, 0)
    keep, _ = cull_keeps(sc, 0)
    assert flat_count(sc, 0) == 32 and keep.all() and (pts[:, 3] == label).all()
    assert (hit.sum(axis=0) == 32).all()                                         # every point reaches 32 leaves: 128 entries per trip
    room = CONST["kRingT"] - 4 * CONST["kWave"]                                  # the ring is drained when more than this is in it
    assert 4 * 32 > room + 63                                                    # (whatever a drain left behind: < 64 entries)
    ctx.both(sc)


@gpu
@pytest.mark.parametrize("fast_trig", (0, 1, 2, 3))
def test_every_instance(ctx, lut, fast_trig):
    ctx.both(flush_scan(lut, 1), fast_trig=fast_trig)


@gpu
def test_chunk_counts(ctx, lut):
    sc, want = chunks_scan(lut)
    assert sc.full and sc.binary
    for t, (M, gone) in enumerate(want):
        assert flat_count(sc, t) == M and sc.nbr[t][gone] == -1 and (np.delete(sc.nbr[t], gone) >= 0).all(), (M, gone)
        keep, _ = cull_keeps(sc, t)
        for c0 in range(0, M, 64):                                               # every chunk stages something and drops something
            assert 0 < int(keep[c0:c0 + 64].sum()) < min(64, M - c0) or M - c0 == 1, (M, gone, c0)
    assert {(M + 63) // 64 for M in CHUNK_M} == {1, 2, 3, 4}
    ctx.both(sc)


@gpu
@pytest.mark.parametrize("ungated", (False, True))
def test_exits(ctx, lut, ungated):
    sc = exits_scan(lut)
    flags = FLAGS | (R.UNGATED if ungated else 0)
    assert flat_count(sc, 0) == 0 and flat_count(sc, len(sc.tests) - 1) == 0 and flat_count(sc, 1) > 0
    new = ctx.both(sc, flags)
    empty = np.r_[0:64, sc.keys.size - 64:sc.keys.size]
    if ungated:
        assert (new[2] & 0x80).all()                                             # classified although nothing reached them
    else:
        assert (new[2][empty] == 0).all()
    assert (new[0][empty] == sc.a0[empty]).all() and (new[1][empty] == sc.b0[empty]).all()
    assert (new[0][64:128] != sc.a0[64:128]).any()
    for timing in (1, 2):
        got, kt = ctx.run(sc, flags, 1, timing=timing)
        assert_same_bits(new, got, sc, f"time_kernel {timing} ")
        print(f"time_kernel {timing}: {kt} ms")
        assert kt.size == 1 and np.isfinite(kt).all() and (kt > 0).all(), (timing, kt)


@gpu
@pytest.mark.parametrize("ungated", (False, True))
def test_a_point_at_no_finite_distance(ctx, lut, ungated):
    sc = nan_scan(lut)
    pts = sc.pts[sc.pts_of(int(sc.nbr[0][0]))]
    assert int(np.isnan(pts[:, :3]).sum()) == 1 and np.isfinite(sc.pts[sc.pts_of(int(sc.nbr[1][0]))]).all()
    _, md = cull_keeps(sc, 0)
    assert int(np.isnan(md).sum()) == 1 and cull_keeps(sc, 0)[0].sum() > 32     # an ordinary tile otherwise
    new = ctx.both(sc, FLAGS | (R.UNGATED if ungated else 0))
    if ungated:
        assert np.isnan(new[0][:64]).all() and np.isnan(new[1][:64]).all()
    else:
        assert (new[2][:64] == 0).all() and (new[0][:64] == sc.a0[:64]).all() and (new[1][:64] == sc.b0[:64]).all()
    assert np.isfinite(new[0][64:]).all() and (new[2][64:] & 0x80).any()


def test_the_copied_evaluation_keeps_the_constants():
    """scan1_sincos_cr_eval moves the words of its four addends into vcc as literals: they are sincos_cr_eval's constants, in its
    order, and the two multiplier constants are the same"""
    csrc = os.path.join(ROOT, "la3dm_amd", "csrc")
    with open(os.path.join(csrc, "bgk_kernels.h")) as fh:
        orig = fh.read()
    with open(os.path.join(csrc, "bgk_scan1_kernels.h")) as fh:
        copy = fh.read()
    body = orig[orig.index("void sincos_cr_eval("):orig.index("template <class Fetch>")]
    addends = [int(c, 16) for c in re.findall(r"fma64_sc\([^;]*?,\s*__builtin_bit_cast\(double, (0x[0-9a-f]{16})ull\)\);", body)]
    factors = [int(c, 16) for c in re.findall(r"fma64_sc\(z, __builtin_bit_cast\(double, (0x[0-9a-f]{16})ull\)", body)]
    assert len(addends) == 4 and len(factors) == 2
    mine = copy[copy.index("void scan1_sincos_cr_eval("):copy.index("template <int kTrig>\n__device__ __forceinline__ float scan1_cov")]
    words = [(int(lo, 16), int(hi, 16)) for lo, hi in re.findall(r'LA3DM_FMA64_VCC\(\w+, \w+, \w+, "(0x[0-9a-f]{8})", "(0x[0-9a-f]{8})"\);', mine)]
    assert [(hi << 32) | lo for lo, hi in words] == addends
    assert [int(c, 16) for c in re.findall(r"__builtin_bit_cast\(double, (0x[0-9a-f]{16})ull\)", mine)] == factors
