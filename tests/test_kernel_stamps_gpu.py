"""Option "time_kernel" on the one-launch BGK scan (la3dm_bgk_scan_device, la3dm_amd/csrc/la3dm_hip.hip): 1 launches
bgk_predict_fuse_t1s, the instance of the kernel that stamps itself with the device's wall clock (bgk_scan1_kernels.h: first
wave in to last wave out, no event, nothing on the stream but the kernel), 2 the event pair handed to the launch of
bgk_predict_fuse_t1, 0 the plain launch.

Scans (depth 3, the packers of tests/helpers/bgk_scans.py, arrays resident on the device):
  one       one full test block: a grid of ONE workgroup, 63 entry slots of the record stay zero
  three     three full test blocks
  empty     a full test block with points and one none of whose seven neighbours holds a point (the kernel's M == 0 exit)
  rays20000 the 20 000-ray synthetic scan of tests/test_kernel_times_gpu.py (more workgroups than slots)
  pruned    a full block and a pruned one: the host falls back to the two launches, which events time at 1 and 2 alike
For each: alpha, beta and state bit-equal between "time_kernel" 0, 1 and 2; one time per call, finite and > 0, none at 0;
K = 20 back-to-back scans cannot take less synchronised wall time than their times add up to (a condition, not a
tolerance); the stamped time is at most the event time of the same scan in the same process plus MARGIN_MS (medians of
the 20).  One drain returns stamped and event-timed calls in call order.

MARGIN_MS is measured, not chosen: 3 x (max - min) of the EVENT form ("time_kernel" 2) over its 20 launches of the
20 000-ray scan.  Measured on an MI355X (HIP 7.2), two runs: event form 35.88 - 43.88 us (median 36.12; the first launch of a burst
is the slow one) and 35.80 - 44.36 us (median 36.22): 3 x spread = 24.0 and 25.7 us; the smaller is taken.  Stamped form of the same
scan in the same processes: median 36.32 us (36.08 - 37.53).  The small scans: stamped 3.3 - 3.4 us against 4.4 - 4.8 us."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import bgk_f64_ref as R   # noqa: E402
import bgk_scans as S     # noqa: E402

pytestmark = pytest.mark.gpu

K = 20
MARGIN_MS = 0.024   # 3 x (43.88 - 35.88) us, see above
FLAGS = R.LABELS_01 | R.FULL_BLOCKS


class DeviceScan:
    """a packed scan resident on the device, run through la3dm_bgk_scan_device on one context"""

    def __init__(self, H, ctx, arrays, counts, flags):
        import torch
        from la3dm_amd import _lib
        self.H, self.ctx, self.torch = H, ctx, torch
        dev = torch.device("cuda", 0)

        def up(a):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)

        self.a0, self.b0 = arrays["alpha"].copy(), arrays["beta"].copy()
        self.t = {k: up(v) for k, v in arrays.items()}
        self.t["state"] = torch.zeros(self.a0.size, dtype=torch.uint8, device=dev)
        self.s = _lib.BgkScan()
        for k, t in self.t.items():
            setattr(self.s, k, t.data_ptr())
        for k, v in counts.items():
            setattr(self.s, k, v)
        self.s.flags = flags
        self.stream = torch.cuda.current_stream().cuda_stream

    def option(self, name, v):
        assert self.H.la3dm_set_option(self.ctx, name.encode(), int(v)) == 0, name

    def reset(self):
        self.t["alpha"].copy_(self.torch.from_numpy(self.a0))
        self.t["beta"].copy_(self.torch.from_numpy(self.b0))
        self.t["state"].fill_(0x55)      # (neither a state nor 0: a leaf that a kernel leaves untouched shows)
        self.torch.cuda.synchronize()

    def call(self):
        from la3dm_amd import _lib
        cnt = _lib.BgkCounters()
        assert self.H.la3dm_bgk_scan_device(self.ctx, C.byref(self.s), self.stream, C.byref(cnt)) == 0, self.H.la3dm_last_error(self.ctx)
        return int(cnt.scratch_bytes) == 0          # did the one launch run

    def times(self, cap):
        kt = np.full(cap + 2, np.nan, np.float32)
        n = C.c_uint32(12345)
        assert self.H.la3dm_kernel_times(self.ctx, kt.ctypes.data, cap, C.byref(n)) == 0
        assert np.isnan(kt[cap:]).all()
        return kt[:cap], int(n.value)

    def bits(self, timing):
        """one scan from the scan's own leaves -> (alpha, beta, state, one launch?, the times read back)"""
        self.option("time_kernel", timing)
        self.reset()
        one = self.call()
        self.torch.cuda.synchronize()
        out = tuple(self.t[k].cpu().numpy().copy() for k in ("alpha", "beta", "state"))
        return out, one, self.times(4)

    def burst(self, timing):
        """K back-to-back scans, one synchronise at the end -> (wall ms, the K times)"""
        self.option("time_kernel", timing)
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            self.call()
        self.torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        kt, n = self.times(K)
        assert n == K and np.isfinite(kt).all() and (kt > 0).all(), (n, kt)
        return wall_ms, kt.astype(np.float64)


def _hand_built(lut, which):
    """the hand-built scans of the module docstring (+ `long`: one block under 5 000 points, for the order of a drain)"""
    rng = np.random.default_rng(4100)
    w = S.World(3, lut)
    keys = S.full_keys(3)

    def trained(ijk, n=None):
        p = S._subcubes(w, ijk) if n is None else w.centre(ijk) + rng.uniform(-0.19, 0.19, (n, 3))
        w.add(ijk, p + S._jit(rng, len(p)), S._labels(rng, len(p)))

    if which == "one":
        trained((0, 0, 0))
        w.test((0, 0, 0), keys, *S.priors(rng, len(keys)))
    elif which == "three":
        for k in range(3):
            trained((4 * k, 0, 0))
            w.test((4 * k, 0, 0), keys, *S.priors(rng, len(keys)))
    elif which == "empty":
        trained((0, 0, 0))
        w.test((0, 0, 0), keys, *S.priors(rng, len(keys)))
        w.test((8, 0, 0), keys, *S.priors(rng, len(keys)))      # no training block within reach: seven times -1
    elif which == "pruned":
        for k, kk in enumerate((keys, S.pruned_keys(3)[::-1].copy())):
            trained((4 * k, 0, 0))
            w.test((4 * k, 0, 0), kk, *S.priors(rng, len(kk)))
    elif which == "long":
        trained((0, 0, 0), 5000)
        w.test((0, 0, 0), keys, *S.priors(rng, len(keys)))
    sc = w.build()
    assert sc.binary and sc.full == (which != "pruned")
    if which == "empty":
        assert (sc.nbr[1] < 0).all()
    return sc


@pytest.fixture(scope="module")
def bare(built):
    """a bare depth-3 context with the hand-built scans on the device: get(name) -> DeviceScan"""
    from la3dm_amd import _lib
    from oracle import oracle as O
    H, P = _lib.hip(), R.BGK_YAML
    lut = S.luts(O, P, depths=(3,))[3]
    p = _lib.Params(resolution=P["resolution"], block_depth=3, sf2=P["sf2"], ell=P["ell"], free_thresh=P["free_thresh"],
                    occupied_thresh=P["occupied_thresh"], var_thresh=P["var_thresh"], prior_A=P["prior_A"], prior_B=P["prior_B"],
                    device=0, lut_xyz=lut.ctypes.data, lut_count=len(lut), variant=0)
    h = C.c_void_p()
    assert H.la3dm_create(C.byref(p), C.byref(h)) == 0, H.la3dm_last_error(None).decode()
    made = {}
    try:
        for name, v in dict(bgk_sum=1, bgk_tables=1, bgk_one_launch=1, fast_trig=0).items():
            assert H.la3dm_set_option(h, name.encode(), v) == 0, name

        def get(which):
            if which not in made:
                sc = _hand_built(lut, which)
                arrays = dict(train_xyzy=sc.pts, train_off=sc.train_off, nbr=sc.nbr, blk_center=sc.centre, leaf_off=sc.leaf_off,
                              leaf_key=sc.keys, alpha=sc.a0, beta=sc.b0)
                counts = dict(n_train_pts=int(sc.train_off[-1]), n_train_blk=len(sc.blocks), n_test_blk=len(sc.tests), n_leaf=int(sc.keys.size))
                made[which] = DeviceScan(H, h, arrays, counts, FLAGS)
            return made[which]

        yield get
    finally:
        import torch
        torch.cuda.synchronize()
        made.clear()
        H.la3dm_destroy(h)


@pytest.fixture(scope="module")
def rays20000(built):
    import la3dm_amd
    from la3dm_amd import _lib
    xyz, origin = la3dm_amd.synthetic_scan(20000)
    m = la3dm_amd.BGKOctoMap(**dict(la3dm_amd.BGK_YAML, block_depth=3), device=0).set_device_resident(False)
    m.set_option("bgk_sum", 1)
    assert m.prepare(xyz, origin, 0.1, 0.5, -1.0)
    pk = m.packed()
    assert pk.flags & 2 and pk.flags & 4
    arrays = {k: getattr(pk, k) for k in ("train_xyzy", "train_off", "nbr", "blk_center", "leaf_off", "leaf_key", "alpha", "beta")}
    counts = {k: getattr(pk.c, k) for k in ("n_train_pts", "n_train_blk", "n_test_blk", "n_leaf")}
    ds = DeviceScan(_lib.hip(), m.ctx(), arrays, counts, int(pk.flags))
    ds.keep = (m, pk)
    return ds


def _scan(name, request):
    return request.getfixturevalue("rays20000") if name == "rays20000" else request.getfixturevalue("bare")(name)


CASES = ("one", "three", "empty", "rays20000", "pruned")


@pytest.mark.parametrize("name", CASES)
def test_same_bits_and_one_time_per_call(name, request):
    ds = _scan(name, request)
    try:
        got = {tk: ds.bits(tk) for tk in (0, 1, 2)}
    finally:
        ds.option("time_kernel", 0)
    for tk, (out, one, (kt, n)) in got.items():
        assert one == (name != "pruned"), (tk, "the launch form the case is about did not run")
        assert n == (1 if tk else 0), (tk, n)
        assert (np.isfinite(kt[:n]).all() and (kt[:n] > 0).all() and np.isnan(kt[n:]).all()), (tk, kt)
        print(f"{name} time_kernel {tk}: {kt[:n]} ms")
    off = got[0][0]
    assert (off[0] != ds.a0).any() and (off[2] != 0x55).any()
    if name == "empty":      # the block without a neighbour: state 0, alpha and beta as they were
        assert (off[2][-64:] == 0).all() and (off[0][-64:] == ds.a0[-64:]).all() and (off[1][-64:] == ds.b0[-64:]).all()
    for tk in (1, 2):
        for what, x, y in zip(("alpha", "beta", "state"), off, got[tk][0]):
            differ = int((x.view(np.uint8) != y.view(np.uint8)).sum())
            print(f"{name} time_kernel {tk} {what}: {differ} of {x.nbytes} bytes differ")
            assert differ == 0, (tk, what)


@pytest.mark.parametrize("name", CASES)
def test_times_fit_the_wall_and_the_event_form(name, request):
    ds = _scan(name, request)
    try:
        for _ in range(5):
            ds.call()
        wall1, t1 = ds.burst(1)
        wall2, t2 = ds.burst(2)
        ds.option("time_kernel", 0)
        ds.call()
        assert ds.times(4)[1] == 0            # nothing accumulates with timing off
    finally:
        ds.option("time_kernel", 0)
        ds.reset()
    print(f"{name}: time_kernel 1: wall {wall1:.4f} ms, sum {t1.sum():.4f}, median {np.median(t1) * 1e3:.2f} us (min {t1.min() * 1e3:.2f}, max {t1.max() * 1e3:.2f})")
    print(f"{name}: time_kernel 2: wall {wall2:.4f} ms, sum {t2.sum():.4f}, median {np.median(t2) * 1e3:.2f} us (min {t2.min() * 1e3:.2f}, max {t2.max() * 1e3:.2f}), "
          f"3 x spread {3e3 * (t2.max() - t2.min()):.2f} us")
    assert t1.sum() <= wall1 and t2.sum() <= wall2
    if name != "pruned":      # (the fallback is timed by events at 1 and 2 alike: there is no stamped time to compare)
        assert np.median(t1) <= np.median(t2) + MARGIN_MS, (np.median(t1), np.median(t2), MARGIN_MS)


def test_one_drain_keeps_the_call_order(bare):
    """stamped and event-timed calls in one drain: a one-launch scan of a block under 5 000 points (one wave that stages 79
    chunks of 64 points: measured 0.50 ms) against the two-launch fallback of a full and a pruned block under 64 points each
    (measured 4.4 - 4.8 us).  The pattern of long and short times is
    the pattern of the calls."""
    long_, short = bare("long"), bare("pruned")
    order = "LSSLSLLS"
    try:
        long_.option("time_kernel", 1)          # (one context: the option and the drain are shared)
        for _ in range(2):
            long_.call(), short.call()
        long_.torch.cuda.synchronize()
        assert long_.times(8)[1] == 4
        for c in order:
            assert (long_ if c == "L" else short).call() == (c == "L")
        kt, n = long_.times(len(order))
    finally:
        long_.option("time_kernel", 0)
        long_.reset(), short.reset()
    print("order", order, "times (ms)", kt)
    assert n == len(order) and np.isfinite(kt).all() and (kt > 0).all()
    L, Sh = [t for t, c in zip(kt, order) if c == "L"], [t for t, c in zip(kt, order) if c == "S"]
    assert min(L) > max(Sh), (L, Sh)
