"""GPU: the BGK-LV voxel kernels (la3dm_amd/csrc/lv_kernels.h) on hand-built packed scans through la3dm_bgklv_scan_host on a bare
context (variant 2), against the CPU restatement's voxel loop body and against the float64 reference of tests/lv_f64_ref.py.

Every other BGK-LV test inserts a cloud through the map class, so the cloud decides which cubes are split, how many bucket
groups a stream spans and how full a round of staged candidates is.  Here the samples, rays, blocks and node states are chosen
(tests/helpers/lv_scans.py; the sizes follow the constants parsed from lv_kernels.h, tests/test_lv_f64_cpu.py asserts that
every class below is hit), and one option selects the form:

  bgk_sum 0 (ordered)      bgklv_cand_kernel, bgklv_plan_kernel, bgklv_voxel_kernel<false>, bgklv_split_add_kernel
  bgk_sum 1 (order-free)   bgklv_cand_kernel, bgklv_plan_kernel, bgklv_voxel_kernel_w8, bgklv_split_apply64
  (bgklv_voxel_kernel<true>, the six-wave build of the order-free body, is launched by nothing.)

Scans, at block_depth 2 (one cube of 8 nodes, 56 idle lanes, bucket = block), 3 (one cube), 4 (8 cubes) and 5 (64 cubes) and
with LV_YAML at ell = 0.2 (reach 1, 27 buckets, one group), 0.5 (reach 2, 125 buckets, two groups) and 0.9 (reach 3, 343
buckets, six groups):
  a. stream length per cube: kLvChunk - 1, kLvChunk, + 1, two chunks, two chunks + 1, three chunks + 5; split and unsplit cubes
     in one block, in one plan wave and in different ones; a sub-task boundary inside a bucket, on a bucket boundary and on a
     group boundary; a sub-task that spans two groups; a sub-task all of whose samples are culled;
  b. kept candidates per staging pass: 1, 15, 16, 17, 63, 64, 65, 129; rounds without a hit row, hit rows in consecutive
     rounds, candidates no voxel counts between counted ones;
  c. rows of a split cube's sub-task in the ordered add: 127, 128, 129, 384, 385;
  d. de-duplication: a ray with 1, 2 and many samples in a voxel's box, its first sample in the box and in the cube's core
     box, its previous sample in another bucket, another group, and outside the stream; a sample inside the cube's outer box
     but in no voxel's box; rows whose segment passes at or beyond ell (k = sf2 g(1) < 0), and a voxel with only such rows:
     HAS_INFO, not updated, alpha and beta untouched;
  e. box faces: a coordinate exactly fl(c + ell) or fl(c - ell) counts, the next float beyond does not; each axis, a corner;
  f. segments of length 0, 5e-5 and >= 2e-4; voxels before the start, beyond the end, beside the segment; 0.97 and 1.03 ell;
  g. cubes with 64, 37, 1 and no active voxel (state 4 in: the byte comes back 0, nothing else changes), a block with no
     sample in reach, alpha / beta carried in (the prior, 0.5, 50, 5000 on either side, A = B, A + B on either side of
     min_W), both sides of the gate, every output state;
  h. neighbourhoods that stick out of the bucket grid on every side, a block partly outside it, empty buckets, shared buckets;
  i. 15, 16, 17, 63, 64 and 65 cubes, split cubes in several plan waves and workgroups; a block's bytes do not depend on how
     many blocks follow it, nor on being scanned alone;
  j. (a), (d) and (e) translated by whole blocks to about (2000, -1500, 30) m;
  k. a large split scan, then a small unsplit one, then the reverse, on one context.

Expected values: n_tiles of the returned counters equals the workgroups the stream lengths imply (that proves which cubes were
split); ordered mode bit-identical to the restatement (alpha, beta as uint32, every state byte); order-free mode within one
fp32 ulp of the restatement's sum mode 1 and >= 99.99 % bit-equal, states equal except where that ulp straddles a threshold;
both within the derived float64 bound, HAS_INFO equal everywhere, gates and states equal outside the excluded sets, at most
2 % of either left out.  la3dm_bgklv_scan_device on torch tensors gives the host form's bytes; fast_trig 3 is bit-identical to
the restatement under set_modes(1, 0) (no float64 bound is derived for that trig).
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

pytestmark = pytest.mark.gpu

CONST = R.lv_constants()
IDS = ["-".join(map(str, c)) for c in S.CASES]


class Ctx:
    """a bare BGKLVOctoMap context (variant 2), destroyed on exit"""

    def __init__(self, P, depth, lut):
        from la3dm_amd import _lib
        self.H = _lib.hip()
        lut = np.ascontiguousarray(lut, np.float32)
        p = _lib.Params(resolution=P["resolution"], block_depth=depth, sf2=P["sf2"], ell=P["ell"], free_thresh=P["free_thresh"],
                        occupied_thresh=P["occupied_thresh"], var_thresh=P["var_thresh"], prior_A=P["prior_A"],
                        prior_B=P["prior_B"], device=0, lut_xyz=lut.ctypes.data, lut_count=len(lut), variant=2, min_W=P["min_W"])
        h = C.c_void_p()
        assert self.H.la3dm_create(C.byref(p), C.byref(h)) == 0, self.H.la3dm_last_error(None).decode()
        self.h = h.value

    def option(self, name, v):
        assert self.H.la3dm_set_option(self.h, name.encode(), int(v)) == 0, name

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.H.la3dm_destroy(self.h)


def _fill(s, sc, samples, sorted_, rays, cell_off, centre, cell0, alpha, beta, state):
    s.samples, s.sorted, s.n_samples, s.rays, s.n_rays = samples, sorted_, len(sc.samples), rays, len(sc.rays8)
    s.cell_off, s.n_blk, s.blk_center, s.blk_cell0 = cell_off, sc.n_blk, centre, cell0
    for i in range(3):
        s.cell_min[i], s.cell_dim[i] = int(sc.cell_min[i]), int(sc.cell_dim[i])
    s.alpha, s.beta, s.state = alpha, beta, state


def run(m, sc, mode):
    """la3dm_bgklv_scan_host on the context: (alpha, beta, state) of every node and n_tiles"""
    from la3dm_amd import _lib
    m.option("bgk_sum", mode)
    s, cnt = _lib.LvScan(), _lib.BgkCounters()
    alpha, beta, state = sc.a0.copy(), sc.b0.copy(), sc.state0.copy()
    blk_center, blk_cell0 = np.ascontiguousarray(sc.blk_center), np.ascontiguousarray(sc.blk_cell0)
    _fill(s, sc, sc.samples.ctypes.data, sc.sorted.ctypes.data, sc.rays8.ctypes.data, sc.cell_off.ctypes.data,
          blk_center.ctypes.data, blk_cell0.ctypes.data, alpha.ctypes.data, beta.ctypes.data, state.ctypes.data)
    if m.H.la3dm_bgklv_scan_host(m.h, C.byref(s), C.byref(cnt)) != 0:
        raise RuntimeError(m.H.la3dm_last_error(m.h).decode())
    return (alpha, beta, state), int(cnt.n_tiles)


@pytest.fixture(scope="module")
def lib(built):
    from oracle import oracle as O
    return O, S.luts(O, R.LV_YAML)


@pytest.fixture(scope="module")
def cases(lib):
    """scan, builder's list and expected values per case, computed once and never changed afterwards"""
    O, luts = lib
    cache = {}

    def get(case):
        if case not in cache:
            sc, extra = S.build_case(case, luts, CONST)
            cache[case] = (sc, extra, expect(O, sc))
        return cache[case]
    return get


def expect(O, sc):
    """the restatement's answers in both sum modes, the float64 reference's, and the workgroups of the plan"""
    return dict(rest=[S.expect_restatement(O, sc, m) for m in (0, 1)], f64=[R.scan64(sc, sc.P, m) for m in (0, 1)],
                tiles=S.expected_tiles(sc, CONST))


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check(got, tiles, exp, P, mode, tag, f64=True):
    """the expected values of the module docstring; returns the largest |device - float64| as a fraction of its bound"""
    assert tiles == exp["tiles"], (tag, "n_tiles", tiles, exp["tiles"])
    want = exp["rest"][mode]
    if mode == 0:
        for k, a, b in zip(("alpha", "beta"), got[:2], want[:2]):
            bad = a.view(np.uint32) != b.view(np.uint32)
            assert not bad.any(), (tag, k, int(bad.sum()), int(np.argmax(bad)), float(np.abs(a - b)[bad].max()))
        assert (got[2] == want[2]).all(), (tag, "state", int((got[2] != want[2]).sum()), int(np.argmax(got[2] != want[2])))
    else:
        assert ((got[2] & 0xC0) == (want[2] & 0xC0)).all(), (tag, "updated / has_info")
        for k, a, b in zip(("alpha", "beta"), got[:2], want[:2]):
            u = _ulps(a, b)
            assert u.max() <= 1, (tag, k, int(u.max()))
            assert (u == 0).mean() >= 0.9999, (tag, k, float((u == 0).mean()))
        far = got[2] != want[2]
        if far.any():      # only where the 1-ulp difference straddles a threshold or a branch of the node
            f = exp["f64"][mode]
            assert f["state_out"][far].all(), (tag, int(far.sum()))
    if not f64:
        return None
    f = exp["f64"][mode]
    bad, worst = R.compare(got, f)
    assert bad == [], (tag, bad)
    assert worst <= 1.0, (tag, worst)
    gate_share, state_share, n_gate, n_state = R.left_out(f)
    assert gate_share <= 0.02 and state_share <= 0.02, (tag, n_gate, n_state)
    return worst


def run_both(m, sc, exp, P, tag):
    out, worst = {}, [0.0, 0.0]
    for mode in (0, 1):
        got, tiles = run(m, sc, mode)
        worst[mode] = check(got, tiles, exp, P, mode, (tag, mode))
        out[mode] = got
    lo = [R.left_out(f)[2:] for f in exp["f64"]]
    print(f"\nLV-F64 {tag}: nodes {len(sc.pos)}, samples {len(sc.samples)}, workgroups {exp['tiles']}, largest |device - float64| / "
          f"bound: ordered {worst[0]:.3f}, order-free {worst[1]:.3f}; left out (gates, states): ordered {lo[0]}, order-free {lo[1]}")
    return out


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_scan(lib, cases, case):
    """every scan of (a) to (j) in both accumulate modes"""
    sc, extra, exp = cases(case)
    P = S.params(case)
    with Ctx(P, case[1], lib[1][case[1]]) as m:
        out = run_both(m, sc, exp, P, " ".join(map(str, case)))
    inactive = ~sc.active
    for mode in (0, 1):
        a, b, st = out[mode]
        assert (st[inactive] == 0).all() and (a[inactive] == sc.a0[inactive]).all() and (b[inactive] == sc.b0[inactive]).all()
    if case[0].startswith("face"):
        for mode in (0, 1):
            for node, on in extra:
                assert bool(out[mode][2][node] & R.HAS_INFO) == on, (case, mode, node, on)
    if case[0] == "dedupe":
        f = exp["f64"][0]
        only = f["info"] & (f["kbar"] < 0) & ~f["gate_out"]
        assert only.any()
        for mode in (0, 1):
            a, b, st = out[mode]
            assert (st[only] == R.HAS_INFO).all() and (a[only] == sc.a0[only]).all() and (b[only] == sc.b0[only]).all()


def test_a_cube_does_not_depend_on_the_plan(lib, cases):
    """(i): block b of the 65-cube scan, scanned alone against the same samples, gives the bytes it has in the full scan,
    whatever workgroup numbers, scratch rows and list places the plan handed out there: the split cubes, the first and last
    cube, and the cubes on either side of a plan wave's and a plan workgroup's end"""
    P = S.params(("cubes 65", 3, 0.2))
    full, _, exp = cases(("cubes 65", 3, 0.2))
    split = [b for b in range(full.n_blk) if S.stream_lengths(full)[b] > CONST["kLvChunk"]]
    assert len(split) >= 4
    p = CONST["kLvPlanPerWave"]
    with Ctx(P, 3, lib[1][3]) as m:
        for mode in (0, 1):
            got, _ = run(m, full, mode)
            for b in sorted(set(split + [0, p - 1, p, 4 * p - 1, 4 * p])):
                one = S.one_block(full, b)
                alone, tiles = run(m, one, mode)
                assert tiles == S.expected_tiles(one, CONST)
                for x, y in zip(got, alone):
                    assert (x[full.nodes_of(b)].view(np.uint8) == y.view(np.uint8)).all(), (mode, b)


def test_stale_arenas(lib, cases):
    """(k): a large split scan and then a small one whose cubes are unsplit, and the reverse, on one context, in both modes and
    across a change of mode: plan and scratch arenas of the earlier scan are not read"""
    P = S.params(("stream", 3, 0.2))
    big, _, ebig = cases(("stream", 3, 0.2))
    small, _, esmall = cases(("dedupe", 3, 0.2))
    assert ebig["tiles"] > big.n_blk and esmall["tiles"] == small.n_blk
    with Ctx(P, 3, lib[1][3]) as m:
        for sc, exp, mode in ((big, ebig, 0), (small, esmall, 0), (big, ebig, 1), (small, esmall, 1), (small, esmall, 0),
                              (big, ebig, 0), (small, esmall, 1), (big, ebig, 1)):
            got, tiles = run(m, sc, mode)
            check(got, tiles, exp, P, mode, ("stale", len(sc.samples), mode))


@pytest.mark.parametrize("case", [("stream", 3, 0.2), ("stream", 4, 0.5)], ids=lambda c: "-".join(map(str, c)))
def test_device_pointer_form(lib, cases, case):
    """la3dm_bgklv_scan_device on torch tensors, scan (a) in both modes: the host form's bytes and its n_tiles"""
    import torch
    from la3dm_amd import _lib
    sc, _, exp = cases(case)
    P = S.params(case)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(
        samples=sc.samples, sorted=sc.sorted, rays=sc.rays8, cell_off=sc.cell_off.view(np.int32), centre=sc.blk_center,
        cell0=sc.blk_cell0).items()}
    for mode in (0, 1):
        with Ctx(P, case[1], lib[1][case[1]]) as m:
            host, host_tiles = run(m, sc, mode)
            alpha, beta = torch.from_numpy(sc.a0.copy()).to(dev), torch.from_numpy(sc.b0.copy()).to(dev)
            state = torch.from_numpy(sc.state0.copy()).to(dev)
            torch.cuda.synchronize()
            s, cnt = _lib.LvScan(), _lib.BgkCounters()
            _fill(s, sc, t["samples"].data_ptr(), t["sorted"].data_ptr(), t["rays"].data_ptr(), t["cell_off"].data_ptr(),
                  t["centre"].data_ptr(), t["cell0"].data_ptr(), alpha.data_ptr(), beta.data_ptr(), state.data_ptr())
            assert m.H.la3dm_bgklv_scan_device(m.h, C.byref(s), None, C.byref(cnt)) == 0, m.H.la3dm_last_error(m.h).decode()
            torch.cuda.synchronize()
            got = (alpha.cpu().numpy(), beta.cpu().numpy(), state.cpu().numpy())
        assert int(cnt.n_tiles) == host_tiles == exp["tiles"]
        for a, b in zip(got, host):
            assert (a.view(np.uint8) == b.view(np.uint8)).all(), mode
        check(got, int(cnt.n_tiles), exp, P, mode, ("device form", mode))


def test_fast_trig_3(lib, cases):
    """Eigen 3.3.7's psin / pcos: scan (d), ordered mode, bit-identical to the restatement under set_modes(1, 0)"""
    O, luts = lib
    case = ("dedupe", 3, 0.2)
    sc, _, exp = cases(case)
    P = S.params(case)
    want = S.expect_restatement(O, sc, 0, trig=1)
    assert (want[0].view(np.uint32) != exp["rest"][0][0].view(np.uint32)).any()       # the trig matters
    with Ctx(P, 3, luts[3]) as m:
        m.option("fast_trig", 3)
        got, tiles = run(m, sc, 0)
    check(got, tiles, dict(exp, rest=[want, None]), P, 0, "fast_trig 3", f64=False)
