"""Option "time_kernel" of the BGK scan (la3dm_bgk_scan_device, la3dm_amd/csrc/la3dm_hip.hip): with it on, the predict + fuse kernel is
launched through hipExtLaunchKernelGGL with the start / stop events handed to the launch, with it off through the plain launch.

  * every kernel the launch macro can pick computes the same bits either way (alpha, beta, state EQUAL, not close: the kernel and
    its arguments are the same, only the launch call differs);
  * la3dm_kernel_times keeps its contract: one value per scan call since the last read, oldest first, at most `cap` written,
    n_out = the count, the list reset afterwards; nothing accumulates with the option off;
  * a kernel time is the kernel's own: K back-to-back scans cannot take less wall time than their kernel times add up to.

The scans are the 3 000-ray synthetic scan of tests/test_bgk_one_launch_gpu.py (the smallest with full blocks in every class of M)
through la3dm_bgk_scan_host; which path a call took is read from the counters it returns (scratch_bytes: 0 for the one launch)."""
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RAYS = 3000


def _fresh(depth=3, rays=RAYS):
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth)
    xyz, origin = la3dm_amd.synthetic_scan(rays)
    m = la3dm_amd.BGKOctoMap(**params, device=0).set_device_resident(False)
    m.set_option("bgk_sum", 1)
    assert m.prepare(xyz, origin, 0.1, 0.5, -1.0)
    pk = m.packed()
    assert pk.flags & 2 and pk.flags & 4          # LA3DM_SCAN_LABELS_01, LA3DM_SCAN_FULL_BLOCKS
    return m, pk


@pytest.fixture(scope="module")
def scan3(built):
    m, pk = _fresh()
    return m, pk, pk.alpha.copy(), pk.beta.copy()


@pytest.fixture(scope="module")
def scan4(built):
    m, pk = _fresh(depth=4, rays=1500)
    return m, pk, pk.alpha.copy(), pk.beta.copy()


def _times(m, cap):
    """la3dm_kernel_times into a buffer of `cap` + 2 NaNs -> (the buffer, n_out)"""
    from la3dm_amd import _lib
    kt = np.full(cap + 2, np.nan, np.float32)
    n = C.c_uint32(12345)
    assert _lib.hip().la3dm_kernel_times(m.ctx(), kt.ctypes.data, cap, C.byref(n)) == 0
    return kt, int(n.value)


def _scan(m, pk, a0, b0, flags, timing):
    """one scan from (a0, b0) -> (alpha, beta, state, scratch_bytes)"""
    m.set_option("time_kernel", timing)
    pk.alpha[:], pk.beta[:], pk.c.flags = a0, b0, flags
    pk.state[:] = 0x55     # (neither a state nor 0: a leaf that a kernel leaves untouched shows)
    cnt = m.scan_host(pk)
    out = (pk.alpha.copy(), pk.beta.copy(), pk.state.copy(), int(cnt.scratch_bytes))
    kt, n = _times(m, 4)
    assert n == (1 if timing else 0)
    if timing:
        assert np.isfinite(kt[0]) and kt[0] > 0
    return out


# (fixture, options, scan flags to clear, does the one launch run) — every kernel LAUNCH_BGK can pick
FORMS = {
    "t1": ("scan3", dict(bgk_sum=1, bgk_one_launch=1), 0, True),
    "t_full": ("scan3", dict(bgk_sum=1, bgk_one_launch=0), 0, False),
    "t_general": ("scan3", dict(bgk_sum=1, bgk_one_launch=1), 4, False),      # without LA3DM_SCAN_FULL_BLOCKS
    "r": ("scan3", dict(bgk_sum=1, bgk_one_launch=1), 2, False),              # without LA3DM_SCAN_LABELS_01
    "v5_w1": ("scan3", dict(bgk_sum=0, waves_per_wg=1), 0, False),
    "v5_w2": ("scan3", dict(bgk_sum=0, waves_per_wg=2), 0, False),
    "v5_w4": ("scan3", dict(bgk_sum=0, waves_per_wg=4), 0, False),
    "depth4": ("scan4", dict(bgk_sum=1, bgk_one_launch=1), 0, False),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_same_bits_with_timing_on_and_off(form, request):
    fixture, options, clear, one = FORMS[form]
    m, pk, a0, b0 = request.getfixturevalue(fixture)
    flags = pk.flags
    try:
        for k, v in options.items():
            m.set_option(k, v)
        off = _scan(m, pk, a0, b0, flags & ~clear, 0)
        on = _scan(m, pk, a0, b0, flags & ~clear, 1)
    finally:
        m.set_option("time_kernel", 0)
        m.set_option("bgk_sum", 1)
        m.set_option("bgk_one_launch", 1)
        m.set_option("waves_per_wg", 1)
        pk.alpha[:], pk.beta[:], pk.c.flags = a0, b0, flags
    assert (off[3] == 0) == one and (on[3] == 0) == one       # the path the case is about ran, both times
    assert (off[0] != a0).any() and (off[2] != 0x55).any()
    for name, x, y in zip(("alpha", "beta", "state"), off, on):
        differ = int((x.view(np.uint8) != y.view(np.uint8)).sum())
        print(f"{form} {name}: {differ} of {x.nbytes} bytes differ")
        assert differ == 0, name


def test_kernel_times_with_timing_on(scan3):
    m, pk, a0, b0 = scan3
    try:
        m.set_option("time_kernel", 1)
        for _ in range(4):
            m.scan_host(pk)
        kt, n = _times(m, 4)
        print("kernel times (ms):", kt[:4])
        assert n == 4
        assert np.isfinite(kt[:4]).all() and (kt[:4] > 0).all() and np.isnan(kt[4:]).all()
        kt, n = _times(m, 4)                  # the read reset the list
        assert n == 0 and np.isnan(kt).all()
        for _ in range(4):
            m.scan_host(pk)
        kt, n = _times(m, 2)                  # cap 2: two written, four counted
        assert n == 4
        assert np.isfinite(kt[:2]).all() and (kt[:2] > 0).all() and np.isnan(kt[2:]).all()
        assert _times(m, 4)[1] == 0
    finally:
        m.set_option("time_kernel", 0)
        pk.alpha[:], pk.beta[:] = a0, b0


def test_nothing_accumulates_with_timing_off(scan3):
    m, pk, a0, b0 = scan3
    try:
        m.set_option("time_kernel", 0)
        for _ in range(4):
            m.scan_host(pk)
        kt, n = _times(m, 4)
        assert n == 0 and np.isnan(kt).all()
    finally:
        pk.alpha[:], pk.beta[:] = a0, b0


def test_kernel_times_fit_into_the_wall_time(built):
    """K back-to-back la3dm_bgk_scan_device calls on a 20 000-ray scan resident on the device, one synchronise at the end: the K kernels
    run one after the other on one stream inside the timed window, so their times add up to at most the window.  A condition,
    not a tolerance."""
    import torch
    from la3dm_amd import _lib
    K = 20
    m, pk = _fresh(rays=20000)
    H, ctx, dev = _lib.hip(), m.ctx(), torch.device("cuda", 0)
    def up(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)

    keep = {k: up(getattr(pk, k)) for k in ("train_xyzy", "train_off", "nbr", "blk_center", "leaf_off", "leaf_key", "alpha", "beta", "state")}
    s = _lib.BgkScan()
    for k, t in keep.items():
        setattr(s, k, t.data_ptr())
    for k in ("n_train_pts", "n_train_blk", "n_test_blk", "n_leaf", "flags"):
        setattr(s, k, getattr(pk.c, k))
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        assert H.la3dm_bgk_scan_device(ctx, C.byref(s), stream, None) == 0, H.la3dm_last_error(ctx)

    for _ in range(5):
        call()
    try:
        m.set_option("time_kernel", 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            call()
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        kt, n = _times(m, K)
    finally:
        m.set_option("time_kernel", 0)
    print(f"{K} scans: wall {wall_ms:.4f} ms, kernel times sum {float(kt[:K].sum()):.4f} ms, each {kt[:K]}")
    assert n == K and np.isfinite(kt[:K]).all() and (kt[:K] > 0).all()
    assert float(kt[:K].astype(np.float64).sum()) <= wall_ms
