"""GPU: every form of the BGK-L kernels (la3dm_amd/csrc/bgkl_kernels.h) on hand-built scans through la3dm_bgkl_scan_host on a
bare context (variant 3), against the CPU restatement and against the float64 reference of tests/bgkl_f64_ref.py.

Every other BGK-L test inserts a cloud through the map class, so the cloud decides which form and which edge runs.  Here the
rows, leaf lists and neighbour tables are chosen (tests/helpers/bgkl_scans.py; the sizes follow the constants parsed from the
headers, tests/test_bgkl_f64_cpu.py asserts that every class is hit), and two options select the form:

  form (bgk_sum, bgkl_split_rows, bgkl_dense_add)     kernels                                                    scans
  ordered, never split (0, -1)                        bgkl_rows_prepare, bgkl_predict_fuse_kernel<8>             a b c d f g h
  ordered, > kLWideTiles tiles                        bgkl_predict_fuse_kernel<1>                                e
  ordered, split (0, 0 or mid, 1)                     bgkl_split_mark / items_wide / eval / bdesc / kernelize,   a b c d e f g
                                                      bgkl_split_expand + bgkl_split_add, bgkl_split_apply
  ordered, split, the replay expands (0, 0 or mid, 0) ... bgkl_split_fuse, bgkl_split_apply                      a b c d e f g
  order-free, never split (1, -1)                     bgkl_predict_fuse_f64<8>                                   a b c d f g
  order-free, > kLWideTiles tiles                     bgkl_predict_fuse_f64<1> (rows staged 64 per trip, the     e
                                                      row cull, the hit ring, ds_add_f64)
  order-free, split (1, 0 or mid)                     bgkl_split_mark / items_wide, bgkl_split_sum (the same     a b c d e f g
                                                      staging, cull and ring), bgkl_split_apply64
  "mid" is a threshold between the scan's tile totals: split and unsplit tiles share a launch.  (bgkl_split_items, the
  one-thread form of bgkl_split_items_wide, is launched by nothing.)

Scans (block_depth 2, 3 and 4; L_YAML with ell = 0.2 and a second set with ell = 0.5, where nearly every row reaches every
leaf of a 0.4 m tile):
  a. rows per training block: 63, 64, 65 (the 64-row trip), 255, 256, 257 (the item), 513, and 7, 8 and 9 items (1792, 2048,
     2049: bgkl_split_apply64 adds eight items per trip); each block is used by two or three test blocks in different slots;
     hits (label 1, length 0 and 5e-5) and beams (label 0) that cross the leaves, pass them at 0.97 ell, at 1.03 ell, and far;
  b. leaf lists of 1 (bounding sphere of radius 0), 37, 63 and 64 leaves at depth 3 — a block of depth 3 holds at most 64 —,
     512 and 65 (a second tile of one leaf) at depth 4, pruned keys, a test block without leaves, one with no neighbour
     (state 0, alpha and beta untouched), a -1 between live slots, no self entry, an empty training block next to split and
     unsplit tiles;
  c. the hit ring (ell = 0.5, depth 3): 5, 6, 7 and 64 hits next to a 37-leaf and a 64-leaf tile: flushes with a remainder
     and without one;
  d. the row cull: beams at the tile's float64 bounding-sphere radius + ell -+ 0.02, as built and translated by
     (2000, -1500, 30) m, split (culled) and unsplit (unculled);
  e. more than kLWideTiles tiles: (a)-(c) plus one-leaf test blocks without neighbours; the live blocks' bits equal the small scan's;
  f. alpha / beta carried in: the prior 0.001 and 0.5, 50, 5000 on either side;
  g. a NaN coordinate and a hit at 3e19 m (its squared distance overflows) in one neighbour: that neighbour's update is
     rejected at every leaf, the others stand (compared with the restatement only: the overflow is fp32's, not the formula's);
  h. la3dm_bgkl_scan_device with LA3DM_SCAN_ROWS_PREPARED: the 12-float rows computed here from include/la3dm_hip.h's
     contract, arrays in torch tensors, bit for bit the host form.

Expected values: ordered mode bit-identical to the restatement (alpha, beta as uint32, every state byte: LEAF_UPDATED | state,
0 for a leaf no neighbour updated); order-free mode within one fp32 ulp of the restatement's sum mode 1 and >= 99.99 %
bit-equal, states equal except where the ulp straddles a threshold; both within the derived float64 bound, gates (through
`updated`) and states equal outside the excluded sets, at most 2 % of either left out.  scratch_bytes of the returned
counters must be exactly 48 n_rows plus the split scratch of the items the thresholds imply: a split case in which nothing
was split fails, as does the reverse.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import bgkl_f64_ref as R   # noqa: E402
import bgkl_scans as S     # noqa: E402

pytestmark = pytest.mark.gpu

CONST = R.bgkl_constants()
PARAMS = {"yaml": R.L_YAML, "ell05": R.P5}
SHIFT = (2000.0, -1500.0, 30.0)
ROWS_PREPARED = 0x8
# (bgk_sum, bgkl_split_rows, bgkl_dense_add)
FORMS = [(0, -1, 1), (0, 0, 1), (0, 0, 0), (0, "mid", 1), (0, "mid", 0), (1, -1, 1), (1, 0, 1), (1, "mid", 1)]
FORMS_NO_MID = [f for f in FORMS if f[1] != "mid"]


class Ctx:
    """a bare BGKLOctoMap context (variant 3), destroyed on exit"""

    def __init__(self, P, depth, lut):
        from la3dm_amd import _lib
        self.H = _lib.hip()
        p = _lib.Params(resolution=P["resolution"], block_depth=depth, sf2=P["sf2"], ell=P["ell"], free_thresh=P["free_thresh"],
                        occupied_thresh=P["occupied_thresh"], var_thresh=P["var_thresh"], prior_A=P["prior_A"],
                        prior_B=P["prior_B"], device=0, lut_xyz=lut.ctypes.data, lut_count=len(lut), variant=3)
        h = C.c_void_p()
        assert self.H.la3dm_create(C.byref(p), C.byref(h)) == 0, self.H.la3dm_last_error(None).decode()
        self.h = h.value

    def set_form(self, form, mid=None):
        bgk_sum, split, dense = form
        for name, v in (("bgk_sum", bgk_sum), ("bgkl_split_rows", mid if split == "mid" else split), ("bgkl_dense_add", dense)):
            assert self.H.la3dm_set_option(self.h, name.encode(), int(v)) == 0, name
        return mid if split == "mid" else split

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.H.la3dm_destroy(self.h)


def _fill(s, sc, rows, off, nbr, centre, leaf_off, keys, alpha, beta, state, flags=0):
    s.train_xyzy, s.train_off, s.nbr, s.blk_center, s.leaf_off, s.leaf_key = rows, off, nbr, centre, leaf_off, keys
    s.n_train_pts, s.n_train_blk = int(sc.train_off[-1]), len(sc.blocks)
    s.n_test_blk, s.n_leaf = len(sc.tests), int(sc.keys.size)
    s.alpha, s.beta, s.state, s.flags = alpha, beta, state, flags


def run(m, sc):
    """la3dm_bgkl_scan_host on the context: (alpha, beta, state) of every leaf and scratch_bytes"""
    from la3dm_amd import _lib
    s, cnt = _lib.BgkScan(), _lib.BgkCounters()
    alpha, beta = sc.a0.copy(), sc.b0.copy()
    state = np.full(sc.keys.size, 0xEE, np.uint8)
    _fill(s, sc, sc.rows.ctypes.data, sc.train_off.ctypes.data, sc.nbr.ctypes.data, sc.centre.ctypes.data,
          sc.leaf_off.ctypes.data, sc.keys.ctypes.data, alpha.ctypes.data, beta.ctypes.data, state.ctypes.data)
    if m.H.la3dm_bgkl_scan_host(m.h, C.byref(s), C.byref(cnt)) != 0:
        raise RuntimeError(m.H.la3dm_last_error(m.h).decode())
    return (alpha, beta, state), int(cnt.scratch_bytes)


def expected_scratch(sc, form, threshold):
    """48 bytes per row for the 12-float rows; a split tile's items add two double sums per leaf (order-free) or their row
    records and value slots (ordered)"""
    n_split, n_items, _ = S.split_totals(sc, CONST, threshold)
    w, it = CONST["kWave"], CONST["kLItemRows"]
    per_item = 16 * w if form[0] == 1 else 16 * it + 4 * it * w
    return 48 * int(sc.train_off[-1]) + per_item * n_items, n_items


@pytest.fixture(scope="module")
def lib(built):
    from oracle import oracle as O
    return O, S.luts(O, R.L_YAML)


def expect(O, P, sc, f64=True):
    """the restatement's answers in both sum modes and the float64 reference's (never changed afterwards)"""
    return dict(rest=[S.expect_restatement(O, P, sc, m)[:3] for m in (0, 1)],
                f64=[R.scan64(sc, P, m) for m in (0, 1)] if f64 else None)


def widen_expected(exp, sc, wide):
    """the expected values of `wide` (sc plus one-leaf test blocks without neighbours: untouched, state 0) from those of sc"""
    n = wide.keys.size - sc.keys.size
    rest = [(np.concatenate([a, wide.a0[-n:]]), np.concatenate([b, wide.b0[-n:]]), np.concatenate([st, np.zeros(n, np.uint8)]))
            for a, b, st in exp["rest"]]
    f64 = []
    for f in exp["f64"]:
        g = {}
        for k, v in f.items():
            if k == "k":
                continue
            fill = wide.a0[-n:].astype(np.float64) if k == "A" else wide.b0[-n:].astype(np.float64) if k == "B" else \
                np.zeros((n,) + v.shape[1:], v.dtype)
            g[k] = np.concatenate([v, fill])
        f64.append(g)
    return dict(rest=rest, f64=f64)


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check(got, exp, P, form, tag):
    """the expected values of the module docstring; returns the largest |device - float64| as a fraction of its bound"""
    mode = form[0]
    want = exp["rest"][mode]
    if mode == 0:
        for k, a, b in zip(("alpha", "beta"), got[:2], want[:2]):
            bad = a.view(np.uint32) != b.view(np.uint32)
            assert not bad.any(), (tag, k, int(bad.sum()), float(np.abs(a - b)[bad].max()))
        assert (got[2] == want[2]).all(), (tag, "state", int((got[2] != want[2]).sum()))
    else:
        assert ((got[2] & 0x80) == (want[2] & 0x80)).all(), (tag, "updated")
        for k, a, b in zip(("alpha", "beta"), got[:2], want[:2]):
            u = _ulps(a, b)
            assert u.max() <= 1, (tag, k, int(u.max()))
            assert (u == 0).mean() >= 0.9999, (tag, k, float((u == 0).mean()))
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
    return worst, n_gate, n_state


def run_forms(m, sc, exp, P, forms, tag, must_split=True):
    """every form on one context, one after the other (what a form leaves in the scratch arenas is never read by the next);
    scratch_bytes says which path ran"""
    mid = S.mid_threshold(sc, CONST)
    worst = [0.0, 0.0]
    out = {}
    for form in forms:
        thr = m.set_form(form, mid)
        got, scratch = run(m, sc)
        want_scratch, n_items = expected_scratch(sc, form, thr)
        assert scratch == want_scratch, (tag, form, scratch, want_scratch)
        if must_split:
            assert (n_items > 0) == (form[1] != -1), (tag, form)
        res = check(got, exp, P, form, (tag, form))
        out[form] = got
        if res:
            worst[form[0]] = max(worst[form[0]], res[0])
    if exp["f64"] is not None:
        lo = [R.left_out(f)[2:] for f in exp["f64"]]
        print(f"\nBGKL-F64 {tag}: leaves {sc.keys.size}, largest |device - float64| / bound: ordered {worst[0]:.3f}, "
              f"order-free {worst[1]:.3f}; left out (gates, states): ordered {lo[0]}, order-free {lo[1]}")
    # all ordered forms are identical to each other (each equals the restatement)
    return out


@pytest.fixture(scope="module")
def rows_cases(lib):
    """(a), (b), (c), (f): scan and expected values per (depth, parameter set), computed once"""
    O, luts = lib
    cache = {}

    def get(depth, k):
        if (depth, k) not in cache:
            sc = S.rows_scan(depth, PARAMS[k], luts[depth], CONST)
            cache[depth, k] = (sc, expect(O, PARAMS[k], sc))
        return cache[depth, k]
    return get


@pytest.mark.parametrize("k", list(PARAMS))
@pytest.mark.parametrize("depth", [2, 3, 4])
def test_rows_and_leaf_lists(lib, rows_cases, depth, k):
    """(a), (b), (c), (f) through every form"""
    sc, exp = rows_cases(depth, k)
    with Ctx(PARAMS[k], depth, lib[1][depth]) as m:
        run_forms(m, sc, exp, PARAMS[k], FORMS, f"rows depth {depth} {k}")
    none = [t for t in range(len(sc.tests)) if all(b < 0 for b in sc.nbr[t]) and sc.leaf_off[t] < sc.leaf_off[t + 1]]
    assert none
    for mode in (0, 1):
        a, b, st = exp["rest"][mode]
        for t in none:
            sl = sc.leaves_of(t)
            assert (st[sl] == 0).all() and (a[sl] == sc.a0[sl]).all() and (b[sl] == sc.b0[sl]).all()


@pytest.mark.parametrize("k", list(PARAMS))
@pytest.mark.parametrize("far", [False, True], ids=["as built", "translated"])
def test_row_cull(lib, k, far):
    """(d): culled (split: bgkl_split_sum) and unculled kernels see the same rows, next to the origin and 2.5 km from it"""
    O, luts = lib
    P = PARAMS[k]
    sc = S.cull_scan(P, luts[3], SHIFT if far else (0.0, 0.0, 0.0))
    with Ctx(P, 3, luts[3]) as m:
        run_forms(m, sc, expect(O, P, sc), P, FORMS_NO_MID, f"cull {k} {'translated' if far else 'as built'}")


@pytest.mark.parametrize("depth,k", [(3, "yaml"), (3, "ell05"), (4, "yaml")])
def test_more_tiles_than_the_wide_form_takes(lib, rows_cases, depth, k):
    """(e): kLWideTiles + 1 test blocks at depth 3, kLWideTiles / 8 + 1 at depth 4: the one-wave-per-tile kernels; the live
    blocks' results are those of the small scan bit for bit in the ordered mode (both equal the restatement)"""
    sc, exp = rows_cases(depth, k)
    tiles_per_block = max(8 ** (depth - 1) // CONST["kWave"], 1)
    n_blocks = CONST["kLWideTiles"] // tiles_per_block + 1
    wide = S.widened(sc, n_blocks)
    assert len(sc.tests) * tiles_per_block <= CONST["kLWideTiles"] < len(wide.tests) * tiles_per_block
    wexp = widen_expected(exp, sc, wide)
    n = sc.keys.size
    with Ctx(PARAMS[k], depth, lib[1][depth]) as m:
        out = run_forms(m, wide, wexp, PARAMS[k], FORMS, f"wide depth {depth} {k}")
        m.set_form((0, -1, 1))
        small, _ = run(m, sc)
    for form, got in out.items():
        if form[0] == 0:
            for a, b in zip(got, small):
                assert (a[:n].view(np.uint8) == b.view(np.uint8)).all(), form
        assert (got[2][n:] == 0).all() and (got[0][n:] == wide.a0[n:]).all() and (got[1][n:] == wide.b0[n:]).all()


def test_non_finite_rows(lib):
    """(g): kbar of the neighbour with the NaN row and the overflowing hit is NaN at every leaf: its update is rejected, the
    other two neighbours' updates stand; both sum modes, split and unsplit, equal to the restatement"""
    O, luts = lib
    P = R.L_YAML
    sc = S.nonfinite_scan(P, luts[3])
    exp = expect(O, P, sc, f64=False)
    for mode in (0, 1):
        _, _, st, yb, kb = S.expect_restatement(O, P, sc, mode)
        assert np.isnan(kb[:, 1]).all() and np.isfinite(kb[:, [0, 3]]).all() and (kb[:, [0, 3]] > np.float32(0.001)).any()
        assert ((st & 0x80) != 0).any()
        # the same scan without the bad neighbour gives the same answer
        tests = [dict(t, nbr=[t["nbr"][0], -1] + t["nbr"][2:]) for t in sc.tests]
        clean = S.LScan(3)
        clean.blocks, clean.tests = sc.blocks, tests
        clean.pack(luts[3])
        for a, b in zip(S.expect_restatement(O, P, clean, mode)[:3], exp["rest"][mode]):
            assert (a.view(np.uint8) == b.view(np.uint8)).all()
    with Ctx(P, 3, luts[3]) as m:
        run_forms(m, sc, exp, P, FORMS_NO_MID, "non-finite rows")


def test_an_empty_training_block_after_a_full_scan(lib):
    """an empty training block in a slot of a split tile, on a context whose previous scan left sums above the gate in that
    slot of the split scratch: the slot adds nothing (ordered split path, both replays, and the order-free one)"""
    O, luts = lib
    P = R.L_YAML
    rng = np.random.default_rng(5)
    centre, keys = np.float32(S.C0), S.finest(3)
    pos = S.leaf_pos(luts[3], keys, centre).astype(np.float64)
    blocks = [S.make_rows(rng, 70, pos, 0.2) for _ in range(7)]
    a0, b0 = S.priors(rng, 64)
    scans = []
    for empty in (None, 4):
        sc = S.LScan(3)
        for i, (rows, kinds) in enumerate(blocks):
            sc.block(*((rows[:0], kinds[:0]) if i == empty else (rows, kinds)))
        sc.test(centre, keys, list(range(7)), a0, b0)
        scans.append((sc.pack(luts[3]), None))
    scans = [(sc, expect(O, P, sc)) for sc, _ in scans]
    assert (scans[0][1]["rest"][0][0] != scans[1][1]["rest"][0][0]).any()       # the block matters
    for form in FORMS_NO_MID:
        with Ctx(P, 3, luts[3]) as m:
            for sc, exp in scans:
                m.set_form(form)
                got, _ = run(m, sc)
                check(got, exp, P, form, ("empty block", form, int(sc.sizes.min())))


def rows12(rows):
    """the kernels' 12-float form of the 8-float rows, from the contract of LA3DM_SCAN_ROWS_PREPARED (include/la3dm_hip.h):
    {x0 y0 z0 x1 | y1 z1 label [shorter than 0.1 mm ? 1 : 0] | lx ly lz |l|^2}, the fp32 expressions of point_to_line_dist"""
    f = np.float32
    r = np.asarray(rows, f)
    l = (r[:, 3:6] - r[:, 0:3]).astype(f)
    c2 = ((l[:, 0] * l[:, 0]).astype(f) + (l[:, 1] * l[:, 1]).astype(f)).astype(f)
    c2 = (c2 + (l[:, 2] * l[:, 2]).astype(f)).astype(f)
    out = np.zeros((len(r), 12), f)
    out[:, 0:7] = r[:, 0:7]
    out[:, 7] = (np.sqrt(c2).astype(f) < f(0.0001)).astype(f)
    out[:, 8:11] = l
    out[:, 11] = c2
    return out


def test_device_pointer_form_with_prepared_rows(lib, rows_cases):
    """(h): la3dm_bgkl_scan_device, LA3DM_SCAN_ROWS_PREPARED, bgkl_split_rows -1 (a call that never waits): the host form's bits"""
    import torch
    from la3dm_amd import _lib
    sc, exp = rows_cases(3, "yaml")
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(
        rows=rows12(sc.rows), off=sc.train_off.view(np.int32), nbr=sc.nbr, centre=sc.centre, leaf_off=sc.leaf_off.view(np.int32),
        keys=sc.keys.view(np.int32)).items()}
    for mode in (0, 1):
        with Ctx(R.L_YAML, 3, lib[1][3]) as m:
            m.set_form((mode, -1, 1))
            host, _ = run(m, sc)
            alpha, beta = torch.from_numpy(sc.a0.copy()).to(dev), torch.from_numpy(sc.b0.copy()).to(dev)
            state = torch.full((sc.keys.size,), 0xEE, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            s, cnt = _lib.BgkScan(), _lib.BgkCounters()
            _fill(s, sc, t["rows"].data_ptr(), t["off"].data_ptr(), t["nbr"].data_ptr(), t["centre"].data_ptr(),
                  t["leaf_off"].data_ptr(), t["keys"].data_ptr(), alpha.data_ptr(), beta.data_ptr(), state.data_ptr(), ROWS_PREPARED)
            assert m.H.la3dm_bgkl_scan_device(m.h, C.byref(s), None, C.byref(cnt)) == 0, m.H.la3dm_last_error(m.h).decode()
            torch.cuda.synchronize()
            got = (alpha.cpu().numpy(), beta.cpu().numpy(), state.cpu().numpy())
        assert int(cnt.scratch_bytes) == 48 * len(sc.rows)
        for a, b in zip(got, host):
            assert (a.view(np.uint8) == b.view(np.uint8)).all(), mode
        check(got, exp, R.L_YAML, (mode, -1, 1), ("device form", mode))
