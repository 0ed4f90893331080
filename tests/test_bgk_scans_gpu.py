"""GPU: every BGK predict + fuse kernel (la3dm_amd/csrc/bgk_kernels.h, bgk_scan1_kernels.h) on hand-built scans through
la3dm_bgk_scan_host on a bare context (variant 0), against the CPU restatement and against the float64 reference of
tests/bgk_f64_ref.py.

Every other BGK test inserts a cloud through the map's front end, so the cloud decides which kernel runs, how many points
a tile sees, how full the hit ring gets and which descriptor a tile reads.  Here the points, leaf lists and neighbour tables
are chosen (tests/helpers/bgk_scans.py; the sizes follow the constants parsed from the header, tests/test_bgk_f64_cpu.py
asserts that every class is hit and that the reference alone keeps every scan within the 2 % caps), and options and flags
select the form; expected_dispatch() restates la3dm_bgk_scan_device's choice and the call's counters must agree
(scratch_bytes: 0 for the one launch, 16 n_train_pts otherwise; n_tiles; the options read back):

  form                                   options and flags                                       kernel
  ordered, 1 / 2 / 4 waves               bgk_sum 0, waves_per_wg 1, 2, 4                         bgk_predict_fuse_v5<.., 1|2|4>
  general                                bgk_sum 1, bgk_tables 0                                 bgk_predict_fuse_r
  general, labels not vouched for        bgk_sum 1, bgk_tables 1, no LABELS_01                   bgk_predict_fuse_r
  tables + general path                  bgk_tables 1, LABELS_01, no FULL_BLOCKS                 bgk_predict_fuse_t<.., true>
  tables only                            + FULL_BLOCKS, bgk_one_launch 0 (a scan with a block    bgk_predict_fuse_t<.., false>
                                         that is not full falls back to the line above)
  one launch                             the same, bgk_one_launch 1, depth 3                     bgk_predict_fuse_t1
  per-tile descriptors on / off          depth >= 4, bgk_tile_desc 1 / 0, every order-free form  bgk_prepare's keep mask

Scans (block_depth 2 to 5; BGK_YAML with ell = 0.2, ell = 0.4 = 4 * resolution, ell = 0.5):
  a. points per tile, flat count and survivors of the cull: 0, 1, around kTabSlots / 2 and kTabSlots, 63-65, 127-129, ~300,
     over one, three and seven neighbours; an empty neighbour and a -1 between live ones, no self entry, a shared block;
  b. n all-hit points so that 64 n lands below, at and above kRing5, kRingR and kRingT, then chunks without hits;
  c. labels: mixed in one trip; d2 == 0 with label 1 and with label 0; d2 == 0 on one axis; labels 0.5, -1, 2 without
     LABELS_01, and the label_seq stamp across a non-binary, a binary and a non-binary scan on one context;
  d. reach: r = 0.97, 0.99, 1.01 and either side of the fp32 hit threshold of one leaf, 0.97 / 1.03 of the support along the
     axes and the diagonal, far points; as built and translated by (2000, -1500, 30) m;
  e. leaf lists: full, pruned, one leaf, none, no neighbour, a last tile of one leaf; full and pruned in one launch;
  f. all six face neighbours with points on the shared face and within ell behind it (depth 4, 5);
  g. alpha / beta carried in: the PRIORS table of the BGK-L helper;
  h. LA3DM_SCAN_UPDATE_UNGATED: trained neighbours out of reach, an untrained slot, M == 0;
  i. a NaN coordinate and a point at 3e19 m in one neighbour, against the restatement only: the reference's kernel matrix
     holds NaN in their columns, that neighbour's ybar / kbar are NaN at every leaf and `kbar > 0` rejects its update (mode
     0); with one sum over all seven neighbours (mode 1) nothing is updated.

Expected values: ordered forms bit-identical to the restatement's mode 0 (alpha, beta as uint32, every state byte) and so to
each other; order-free forms within one fp32 ulp of the restatement's mode 1 and >= 99.99 % bit-equal, `updated` bits equal,
states equal except where the ulp straddles a threshold; one launch == two launches bit for bit; both modes within the
derived float64 bound, gates (through `updated`) and states equal outside the left-out sets, at most 2 % of either left out.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import bgk_f64_ref as R   # noqa: E402
import bgk_scans as S     # noqa: E402

pytestmark = pytest.mark.gpu

CONST = R.bgk_constants()
CASES = S.cases()
TAGS = [c[0] for c in CASES]

# (name, options, flag bits wanted of {LABELS_01, FULL_BLOCKS}, sum mode)
ORDERED = [(f"ordered, {w} waves", dict(bgk_sum=0, waves_per_wg=w), R.LABELS_01, 0) for w in (1, 2, 4)]
ORDER_FREE = [("general", dict(bgk_sum=1, bgk_tables=0, bgk_one_launch=0), R.LABELS_01, 1),
              ("general, labels not vouched for", dict(bgk_sum=1, bgk_tables=1, bgk_one_launch=0), 0, 1),
              ("tables + general path", dict(bgk_sum=1, bgk_tables=1, bgk_one_launch=0), R.LABELS_01, 1),
              ("tables only", dict(bgk_sum=1, bgk_tables=1, bgk_one_launch=0), R.LABELS_01 | R.FULL_BLOCKS, 1),
              ("one launch", dict(bgk_sum=1, bgk_tables=1, bgk_one_launch=1), R.LABELS_01 | R.FULL_BLOCKS, 1)]


class Ctx:
    """a bare BGKOctoMap context (variant 0), destroyed on exit"""

    def __init__(self, P, depth, lut):
        from la3dm_amd import _lib
        self.H = _lib.hip()
        self.P, self.depth = P, depth
        p = _lib.Params(resolution=P["resolution"], block_depth=depth, sf2=P["sf2"], ell=P["ell"], free_thresh=P["free_thresh"],
                        occupied_thresh=P["occupied_thresh"], var_thresh=P["var_thresh"], prior_A=P["prior_A"],
                        prior_B=P["prior_B"], device=0, lut_xyz=lut.ctypes.data, lut_count=len(lut), variant=0)
        h = C.c_void_p()
        assert self.H.la3dm_create(C.byref(p), C.byref(h)) == 0, self.H.la3dm_last_error(None).decode()
        self.h = h.value
        self.opts = {}
        self.set(fast_trig=0, bgk_tile_desc=1, bgk_one_launch=0, bgk_tables=1, waves_per_wg=4)

    def set(self, **opts):
        for name, v in opts.items():
            assert self.H.la3dm_set_option(C.c_void_p(self.h), name.encode(), int(v)) == 0, name
            got = C.c_int(-1)
            assert self.H.la3dm_get_option(C.c_void_p(self.h), name.encode(), C.byref(got)) == 0 and got.value == int(v), name
            self.opts[name] = int(v)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.H.la3dm_destroy(C.c_void_p(self.h))


def scan_flags(sc, want, ungated=False):
    """the flags a caller may set on this scan: LABELS_01 only where every label is 0 or 1 (FULL_BLOCKS is a hint the host
    verifies, so it is passed on scans with pruned blocks too)"""
    f = want if sc.binary else want & ~R.LABELS_01
    return f | (R.UNGATED if ungated else 0)


def expected_dispatch(m, sc, flags):
    """la3dm_bgk_scan_device's choice restated: (kernel, per-tile descriptors, scratch_bytes, n_tiles)"""
    o, depth = m.opts, m.depth
    n_pts, n_tiles = int(sc.train_off[-1]), len(sc.tests) * max(8 ** (depth - 1) // CONST["kWave"], 1)
    if o["bgk_sum"] == 0:
        return f"v5 x{o['waves_per_wg']}", False, 16 * n_pts, n_tiles
    tables = bool(o["bgk_tables"]) and depth >= 3 and bool(flags & R.LABELS_01)
    full = bool(flags & R.FULL_BLOCKS) and sc.keys.size == len(sc.tests) * 8 ** (depth - 1)
    one = tables and full and depth == 3 and o["bgk_one_launch"] == 1
    desc = depth >= 4 and bool(o["bgk_tile_desc"]) and not flags & R.UNGATED and np.float32(m.P["ell"]) <= np.float32(4.0) * np.float32(m.P["resolution"])
    return ("t1" if one else "t only" if tables and full else "t + general" if tables else "r"), desc, 0 if one else 16 * n_pts, n_tiles


def _fill(s, sc, pts, off, nbr, centre, leaf_off, keys, alpha, beta, state, flags):
    s.train_xyzy, s.train_off, s.nbr, s.blk_center, s.leaf_off, s.leaf_key = pts, off, nbr, centre, leaf_off, keys
    s.n_train_pts, s.n_train_blk = int(sc.train_off[-1]), len(sc.blocks)
    s.n_test_blk, s.n_leaf = len(sc.tests), int(sc.keys.size)
    s.alpha, s.beta, s.state, s.flags = alpha, beta, state, flags


def run(m, sc, flags):
    """la3dm_bgk_scan_host on the context: (alpha, beta, state) of every leaf; the counters must name the expected form"""
    from la3dm_amd import _lib
    s, cnt = _lib.BgkScan(), _lib.BgkCounters()
    alpha, beta = sc.a0.copy(), sc.b0.copy()
    state = np.full(sc.keys.size, 0xEE, np.uint8)
    pts = sc.pts if len(sc.pts) else np.zeros((1, 4), np.float32)
    keys = sc.keys if sc.keys.size else np.zeros(1, np.uint32)
    _fill(s, sc, pts.ctypes.data, sc.train_off.ctypes.data, sc.nbr.ctypes.data, sc.centre.ctypes.data, sc.leaf_off.ctypes.data,
          keys.ctypes.data, alpha.ctypes.data if alpha.size else keys.ctypes.data, beta.ctypes.data if beta.size else keys.ctypes.data,
          state.ctypes.data if state.size else keys.ctypes.data, flags)
    if m.H.la3dm_bgk_scan_host(C.c_void_p(m.h), C.byref(s), C.byref(cnt)) != 0:
        raise RuntimeError(m.H.la3dm_last_error(C.c_void_p(m.h)).decode())
    kernel, desc, scratch, n_tiles = expected_dispatch(m, sc, flags)
    assert (int(cnt.scratch_bytes), int(cnt.n_tiles)) == (scratch, n_tiles), (kernel, int(cnt.scratch_bytes), scratch, int(cnt.n_tiles), n_tiles)
    return (alpha, beta, state), (kernel, desc)


@pytest.fixture(scope="module")
def lib(built):
    from oracle import oracle as O
    return O, S.luts(O, R.BGK_YAML)


def expect(O, P, sc, ungated=False, f64=True):
    """the restatement's answers in both sum modes and the float64 reference's (never changed afterwards)"""
    pairs = {}
    return dict(rest=[S.expect_restatement(O, P, sc, m, ungated) for m in (0, 1)],
                f64=[R.scan64(sc, P, m, ungated, cache=pairs) for m in (0, 1)] if f64 else None)


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def same_bits(a, b):
    return all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(a, b))


def check(got, exp, P, mode, tag):
    """the expected values of the module docstring; returns the largest |device - float64| as a fraction of its bound"""
    want = exp["rest"][mode]
    if mode == 0:
        for k, a, b in zip(("alpha", "beta"), got[:2], want[:2]):
            bad = a.view(np.uint32) != b.view(np.uint32)
            assert not bad.any(), (tag, k, int(bad.sum()), float(np.abs(a - b)[bad].max()))
        assert (got[2] == want[2]).all(), (tag, "state", int((got[2] != want[2]).sum()))
    else:
        assert ((got[2] & 0x80) == (want[2] & 0x80)).all(), (tag, "updated", int(((got[2] ^ want[2]) & 0x80 != 0).sum()))
        for k, a, b in zip(("alpha", "beta"), got[:2], want[:2]):
            same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
            u = np.where(same, 0, _ulps(a, b))
            assert u.max(initial=0) <= 1, (tag, k, int(u.max()))
            assert same.mean() >= 0.9999 if same.size else True, (tag, k, float(same.mean()))
        far = got[2] != want[2]
        if far.any():      # only where the 1-ulp difference straddles a threshold
            p = got[0][far].astype(np.float64) / (got[0][far].astype(np.float64) + got[1][far])
            d = np.minimum(np.abs(p - P["free_thresh"]), np.abs(p - P["occupied_thresh"]))
            assert (d < 1e-6).all(), (tag, int(far.sum()))
    if exp["f64"] is None:
        return None
    f = exp["f64"][mode]
    bad, worst = R.compare(got, f)
    assert bad == [], (tag, bad)
    gate_share, state_share, n_gate, n_state = R.left_out(f)
    assert gate_share <= 0.02 and state_share <= 0.02, (tag, n_gate, n_state)
    return worst


def forms_for(sc, depth):
    out = list(ORDERED)
    for name, opts, want, mode in ORDER_FREE:
        if name == "one launch" and depth != 3:
            continue
        for desc in ((1, 0) if depth >= 4 else (1,)):
            out.append((name + (", per-tile descriptors off" if not desc else ""), dict(opts, bgk_tile_desc=desc), want, mode))
    return out


def run_forms(m, sc, exp, P, tag, ungated=False):
    """every form on one context, one after the other; returns {form: result}, prints the BGK-F64 line"""
    worst = [0.0, 0.0]
    out, seen = {}, set()
    for name, opts, want, mode in forms_for(sc, m.depth):
        m.set(**opts)
        flags = scan_flags(sc, want, ungated)
        got, ran = run(m, sc, flags)
        seen.add(ran)
        res = check(got, exp, P, mode, (tag, name, ran))
        out[name] = got
        if res is not None:
            worst[mode] = max(worst[mode], res)
    if exp["f64"] is not None:
        lo = [R.left_out(f)[2:] for f in exp["f64"]]
        print(f"\nBGK-F64 {tag}: leaves {sc.keys.size}, largest |device - float64| / bound: ordered {worst[0]:.3f}, "
              f"order-free {worst[1]:.3f}; left out (gates, states): ordered {lo[0]}, order-free {lo[1]}; "
              f"kernels {sorted(k + (' / tile' if d else '') for k, d in seen)}")
    # the ordered forms are identical to each other, the one launch to the two launches
    assert same_bits(out["ordered, 1 waves"], out["ordered, 2 waves"]) and same_bits(out["ordered, 1 waves"], out["ordered, 4 waves"])
    if "one launch" in out:
        assert same_bits(out["one launch"], out["tables only"]), tag
    return out, seen


@pytest.fixture(scope="module")
def scans(lib):
    """scan and expected values per case, built once"""
    O, luts = lib
    by_tag = {c[0]: c for c in CASES}
    cache = {}

    def get(tag):
        if tag not in cache:
            _, depth, k, make, ungated = by_tag[tag]
            sc = make(luts[depth], CONST)
            cache[tag] = (sc, S.PARAMS[k], depth, ungated, expect(O, S.PARAMS[k], sc, ungated))
        return cache[tag]
    return get


@pytest.mark.parametrize("tag", TAGS)
def test_every_form_on_every_scan(lib, scans, tag):
    """(a)-(h) through every form the depth and the labels admit"""
    sc, P, depth, ungated, exp = scans(tag)
    with Ctx(P, depth, lib[1][depth]) as m:
        out, seen = run_forms(m, sc, exp, P, tag, ungated)
    kernels = {k for k, _ in seen}
    assert {"v5 x1", "v5 x2", "v5 x4", "r"} <= kernels
    if sc.binary and depth >= 3:
        assert "t + general" in kernels and ("t only" in kernels) == sc.full and ("t1" in kernels) == (sc.full and depth == 3)
    if depth >= 4 and not ungated and P["ell"] <= 0.4:
        assert {d for _, d in seen} == {True, False}
    # FULL_BLOCKS on a scan with a block that is not full: the kernel with the general path, the same result
    if sc.binary and not sc.full and depth >= 3:
        assert same_bits(out["tables only"], out["tables + general path"])
    # a test block with no neighbour: state 0, alpha and beta untouched (gated scans)
    if not ungated:
        for t in range(len(sc.tests)):
            if all(b < 0 for b in sc.nbr[t]):
                sl = sc.leaves_of(t)
                for got in out.values():
                    assert (got[2][sl] == 0).all() and (got[0][sl] == sc.a0[sl]).all() and (got[1][sl] == sc.b0[sl]).all()


def test_ungated_updates(lib, scans):
    """(h): what the restatement answers — a trained neighbour out of reach still updates (alpha, beta unchanged, the leaf
    marked), once per trained neighbour in mode 0 and once in mode 1; a block with no point in its seven neighbours (M == 0)
    is not touched in mode 0 (bgk_predict_fuse_v5 marks it; bgk_ungated_unmark in la3dm_hip.hip takes the mark back) and
    is marked in mode 1 (bgk_f64_ref's docstring)"""
    sc, P, depth, ungated, exp = scans("ungated d3")
    assert ungated
    a, b, st = exp["rest"][0]
    first, last = sc.leaves_of(0), sc.leaves_of(2)
    assert (st[first] & 0x80).all() and (a[first] == sc.a0[first]).all() and (b[first] == sc.b0[first]).all()
    assert (st[last] == 0).all()
    assert (exp["rest"][1][2][last] & 0x80).all() and (exp["rest"][1][0][last] == sc.a0[last]).all()


def test_label_stamp_follows_the_scan(lib, scans):
    """(c): a non-binary scan, a binary one and a non-binary one again on ONE context, through the kernels that read the
    stamp bgk_prepare leaves in label_seq (bgk_tile_r's two accumulate paths)"""
    O, luts = lib
    nb, P, depth, _, exp_nb = scans("labels d3 non-binary")
    bi, _, _, _, exp_bi = scans("labels d3 binary")
    assert not nb.binary and bi.binary and {0.5, -1.0, 2.0} <= set(nb.pts[:, 3].tolist())
    for opts, want in ((dict(bgk_sum=1, bgk_tables=0), R.LABELS_01), (dict(bgk_sum=1, bgk_tables=1), 0)):
        with Ctx(P, depth, luts[depth]) as m:
            m.set(**opts)
            for i, (sc, exp) in enumerate(((nb, exp_nb), (bi, exp_bi), (nb, exp_nb), (bi, exp_bi))):
                got, ran = run(m, sc, scan_flags(sc, want))
                assert ran[0] == "r"
                check(got, exp, P, 1, ("label stamp", opts, i))


def test_device_pointer_form(lib, scans):
    """la3dm_bgk_scan_device with the arrays in torch tensors: the host form's bits (tables + general path, and ordered)"""
    import torch
    from la3dm_amd import _lib
    sc, P, depth, _, exp = scans("lists d3 yaml")
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(
        pts=sc.pts, off=sc.train_off.view(np.int32), nbr=sc.nbr, centre=sc.centre, leaf_off=sc.leaf_off.view(np.int32),
        keys=sc.keys.view(np.int32)).items()}
    for opts, mode in ((dict(bgk_sum=1, bgk_tables=1), 1), (dict(bgk_sum=0, waves_per_wg=4), 0)):
        with Ctx(P, depth, lib[1][depth]) as m:
            m.set(**opts)
            flags = scan_flags(sc, R.LABELS_01)
            host, ran = run(m, sc, flags)
            alpha, beta = torch.from_numpy(sc.a0.copy()).to(dev), torch.from_numpy(sc.b0.copy()).to(dev)
            state = torch.full((sc.keys.size,), 0xEE, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            s, cnt = _lib.BgkScan(), _lib.BgkCounters()
            _fill(s, sc, t["pts"].data_ptr(), t["off"].data_ptr(), t["nbr"].data_ptr(), t["centre"].data_ptr(),
                  t["leaf_off"].data_ptr(), t["keys"].data_ptr(), alpha.data_ptr(), beta.data_ptr(), state.data_ptr(), flags)
            assert m.H.la3dm_bgk_scan_device(C.c_void_p(m.h), C.byref(s), None, C.byref(cnt)) == 0, m.H.la3dm_last_error(C.c_void_p(m.h)).decode()
            torch.cuda.synchronize()
            got = (alpha.cpu().numpy(), beta.cpu().numpy(), state.cpu().numpy())
        assert int(cnt.scratch_bytes) == 16 * len(sc.pts)
        assert same_bits(got, host), mode
        check(got, exp, P, mode, ("device form", mode))


def test_eigen_trig(lib, scans):
    """fast_trig 3 on one scan per sum mode against the restatement under oracle.set_modes(1, 0)"""
    O, luts = lib
    sc, P, depth, _, _ = scans("counts d3 yaml")
    O.set_modes(1, 0)
    try:
        exp = dict(rest=[S.expect_restatement(O, P, sc, m) for m in (0, 1)], f64=None)
    finally:
        O.set_modes(0, 0)
    with Ctx(P, depth, luts[depth]) as m:
        m.set(fast_trig=3)
        for opts, want, mode in ((dict(bgk_sum=0, waves_per_wg=4), R.LABELS_01, 0), (dict(bgk_sum=1, bgk_tables=1, bgk_one_launch=1), R.LABELS_01 | R.FULL_BLOCKS, 1)):
            m.set(**opts)
            got, ran = run(m, sc, scan_flags(sc, want))
            check(got, exp, P, mode, ("fast_trig 3", ran))


def test_non_finite_points(lib):
    """(i): against the restatement only, every form (see the module docstring for what the restatement does).

    The kernels of bgk_kernels.h drop a point whose distance is not finite at their distance tests; before this test
    they went on with the neighbour's other points (alpha off by up to 4.6 at 16 of 64 leaves in the ordered forms, at 49
    in the order-free ones, which updated 51 leaves where the restatement updates none).  Now bgk_poison_nbr
    (la3dm_hip.hip) takes such a neighbour out of the table they read, and bgk_predict_fuse_t1 finds the point itself."""
    O, luts = lib
    P = R.BGK_YAML
    sc = S.nonfinite_scan(P, luts[3])
    exp = expect(O, P, sc, f64=False)
    assert ((exp["rest"][0][2] & 0x80) != 0).any() and (exp["rest"][1][2] == 0).all()
    with Ctx(P, 3, luts[3]) as m:
        out, seen = run_forms(m, sc, exp, P, "non-finite points")
    assert {k for k, _ in seen} == {"v5 x1", "v5 x2", "v5 x4", "r", "t + general", "t only", "t1"}


def test_non_finite_points_ungated(lib):
    """(i) with LA3DM_SCAN_UPDATE_UNGATED: the update runs with the NaN sums, alpha and beta of every leaf are NaN and the
    state is UNKNOWN, in both sum modes and every form (NaN payloads are not compared)"""
    O, luts = lib
    P = R.BGK_YAML
    sc = S.nonfinite_scan(P, luts[3])
    exp = expect(O, P, sc, ungated=True, f64=False)
    for a, b, st in exp["rest"]:
        assert np.isnan(a).all() and np.isnan(b).all() and (st == (0x80 | R.UNKNOWN)).all()
    with Ctx(P, 3, luts[3]) as m:
        for name, opts, want, mode in forms_for(sc, 3):
            m.set(**opts)
            got, ran = run(m, sc, scan_flags(sc, want, True))
            assert np.isnan(got[0]).all() and np.isnan(got[1]).all() and (got[2] == (0x80 | R.UNKNOWN)).all(), (name, ran)
