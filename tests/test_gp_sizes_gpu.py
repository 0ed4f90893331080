"""GPU: the GPOctoMap kernels at every training-block size class, on hand-built scans through la3dm_gp_scan_host.

Every other GP test feeds a real or synthetic scan and compares whole maps, so a size class is covered only when a scan
happens to hold such a block.  Here N is chosen: the thresholds are parsed from la3dm_amd/csrc/gp_kernels.h and
gp_eigen_kernels.h (tests/gp_f64_ref.py gp_constants, size_list), and every scan asserts that its N list hits every class
of this table (values of the constants at the time of writing):

  N (training block)               train kernel (gp_mode 0)                        predict path of a tile whose largest
                                                                                   neighbour block holds N points
  1 .. kGpTrainTinyN (32)          gp_train_wave_kernel, tiny launch               small kernel, launch N <= 16 or 16 < N <= 32
  33 .. kGpLdsRows (64)            gp_train_wave_kernel, second launch             small kernel, launch 32 < N <= 64
  kGpMfmaMinN (65) .. kGpTrainLdsMaxN (128)   the second launch, two rows per lane mixed kernel, gp_solve_mfma
  > kGpTrainLdsMaxN                gp_train_kernel, 32 x 32 MFMA tiles             mixed kernel, gp_solve_mfma
                                   (last tile column partial when N % 32 != 0)     (vscratch rows rounded up to 32)
  In the mixed kernel the neighbours with N < kGpMfmaMinN still take the four-row path; N % 4 != 0 is its min(k0 + u, N - 1)
  tail.  gp_mode 1 (gp_eigen_kernels.h): unblocked below 32 points, blocks of 8 from 32, of 16 at 128, triangular solves in
  panels of 8, two rows per lane above 64; N > kGpEigenMaxN (128) is refused.

Expected values:
  * bit-identical to the CPU restatement (oracle/): OracleGPMap.train_predict once per training block with the leaves of
    every test block that uses it, then orc_gp_node_update in nbr (ExtendedBlock) order — m_ivar / ivar as uint32, every
    state byte (LEAF_UPDATED | state, 0 for a leaf no neighbour updated), for GP_YAML and for gp_f64_ref.P2;
  * for P2 (sf2 = 1, noise = 1, ell = 0.3: kappa(K) <= N + 1), within the derived bound of the float64 reference
    (gp_f64_ref: gp_bounds, node_bounds), and the same states except where the float64 p lies within its bound of a
    threshold.  The bound is finite (has something to say) at every leaf up to N = 257 (asserted); at 531 and 1025 a
    leaf's variance can lie inside its bound, and bit identity with the restatement carries the check there.

Scans:
  a. one class per scan: one training block of N points (labels +-1, inside a block cube) and 1-3 test blocks that use it in
     different nbr slots, at block_depth 3 (one tile per block) and 4 (eight tiles); each on a fresh context once without
     hints (the library sizes the factor arena with one sync) and once with the exact train_max_n / train_sum_n2;
  b. stale arenas: the (a) scans on one context, largest N to smallest and back, bit-identical to the fresh contexts;
  c. one mixed scan: more than kGpOffThreads training blocks (gp_factor_offsets' threads walk several each; the count
     straddles kGpOffThreads), every N of the list, duplicate points, an empty block in nbr (treated like -1), neighbour
     sets that mix classes, a test block without neighbours (state 0, alpha / beta untouched), 13 test blocks (the XCD
     remap covers the first 8), leaf lists of 1, 63 and 65 leaves and a pruned block, priors that make every state and the
     max_ivar clamp occur;
  d. gp_mode 1 at the Eigen-order factorisation's edges, bit-identical to oracle.set_gp_mode(1); N = 129 refused.
The kernels do not look at where a block is: positions only set the kernel values, chosen so that every neighbour matters.
"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import gp_f64_ref as R

pytestmark = pytest.mark.gpu

CONST = R.gp_constants()
NS = R.size_list(CONST)
PARAMS = {"yaml": R.GP_YAML, "p2": R.P2}
DIRS = np.float32([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])   # ExtendedBlock order
BASE = [(8 ** d - 1) // 7 for d in range(8)]
POOL = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))   # ctypes releases the GIL: restatement calls in parallel


def train_class(n):
    if n <= CONST["kGpTrainTinyN"]:
        return "wave tiny"
    if n <= CONST["kGpTrainLdsMaxN"]:
        return "wave two rows" if n > CONST["kGpLdsRows"] else "wave"
    return "mfma partial tile" if n % 32 else "mfma"


def predict_class(n):
    if n >= CONST["kGpMfmaMinN"]:
        return "mixed"
    return "small <= 16" if n <= 16 else "small <= 32" if n <= 32 else "small <= 64"


def assert_every_class(ns):
    """the table of the module docstring, from the parsed constants: every train kernel class, every predict path and the
    four-row tail are hit"""
    assert {train_class(n) for n in ns} == {"wave tiny", "wave", "wave two rows", "mfma", "mfma partial tile"}, ns
    assert {predict_class(n) for n in ns} == {"small <= 16", "small <= 32", "small <= 64", "mixed"}, ns
    assert {n % 4 for n in ns if n < CONST["kGpMfmaMinN"]} == {0, 1, 2, 3}, ns
    for t in ("kGpTrainTinyN", "kGpTrainLdsMaxN", "kGpLdsRows", "kGpMfmaMinN"):
        assert {CONST[t] - 1, CONST[t], CONST[t] + 1} <= set(ns), t


class Scan:
    """a la3dm_bgk_scan built from numpy arrays"""

    def __init__(self, depth):
        self.depth, self.blocks, self.tests = depth, [], []

    def block(self, x, y):
        self.blocks.append((np.asarray(x, np.float32).reshape(-1, 3), np.asarray(y, np.float32)))
        return len(self.blocks) - 1

    def test(self, centre, keys, nbr, mi0, iv0):
        self.tests.append(dict(centre=np.asarray(centre, np.float32), keys=np.asarray(keys, np.uint32), nbr=list(nbr),
                               mi0=np.asarray(mi0, np.float32), iv0=np.asarray(iv0, np.float32)))

    def pack(self, lut):
        n = np.array([len(b[1]) for b in self.blocks], np.int64)
        self.train_off = np.concatenate([[0], np.cumsum(n)]).astype(np.uint32)
        self.xyzy = np.zeros((max(int(n.sum()), 1), 4), np.float32)
        for b, (x, y) in enumerate(self.blocks):
            self.xyzy[self.train_off[b]:self.train_off[b + 1]] = np.column_stack([x, y])
        self.nbr = np.array([t["nbr"] for t in self.tests], np.int32).reshape(-1, 7)
        self.centre = np.array([t["centre"] for t in self.tests], np.float32).reshape(-1, 3)
        self.leaf_off = np.concatenate([[0], np.cumsum([len(t["keys"]) for t in self.tests])]).astype(np.uint32)
        self.keys = np.concatenate([t["keys"] for t in self.tests]).astype(np.uint32)
        self.mi0 = np.concatenate([t["mi0"] for t in self.tests]).astype(np.float32)
        self.iv0 = np.concatenate([t["iv0"] for t in self.tests]).astype(np.float32)
        # Block::get_loc: lut[key] + centre in fp32
        ctr = np.repeat(self.centre, np.diff(self.leaf_off.astype(np.int64)), axis=0)
        self.pos = (lut[np.array([BASE[k >> 16] for k in self.keys], np.int64) + (self.keys & 0xFFFF)] + ctr).astype(np.float32)
        self.sizes = n
        return self

    def leaves_of(self, t):
        return slice(int(self.leaf_off[t]), int(self.leaf_off[t + 1]))

    def users(self):
        """training block -> leaf indices of every test block that uses it (in any slot)"""
        u = {}
        for t in range(len(self.tests)):
            for b in set(int(b) for b in self.nbr[t] if b >= 0 and self.sizes[b] > 0):
                u.setdefault(b, []).append(np.arange(self.leaf_off[t], self.leaf_off[t + 1]))
        return {b: np.concatenate(v) for b, v in u.items()}


class Ctx:
    """a bare GPOctoMap context (variant 1) with the statics the host map derives (1.0f / x in fp32), destroyed on exit"""

    def __init__(self, P, depth, lut, gp_mode=0):
        from la3dm_amd import _lib
        self.H, f = _lib.hip(), np.float32
        p = _lib.Params(resolution=P["resolution"], block_depth=depth, sf2=P["sf2"], ell=P["ell"],
                        free_thresh=P["free_thresh"], occupied_thresh=P["occupied_thresh"], device=0,
                        lut_xyz=lut.ctypes.data, lut_count=len(lut), variant=1, noise=P["noise"], l=P["l"],
                        min_ivar=float(f(1) / f(P["max_var"])), max_ivar=float(f(1) / f(P["min_var"])),
                        min_known_ivar=float(f(1) / f(P["max_known_var"])))
        h = C.c_void_p()
        assert self.H.la3dm_create(C.byref(p), C.byref(h)) == 0, self.H.la3dm_last_error(None).decode()
        self.h = h.value
        if gp_mode:
            assert self.H.la3dm_set_option(self.h, b"gp_mode", gp_mode) == 0

    def ctx(self):
        return self.h

    def set_option(self, name, value):
        assert self.H.la3dm_set_option(self.h, name.encode(), value) == 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.H.la3dm_destroy(self.h)


def run(m, sc, hints=False):
    """la3dm_gp_scan_host on the context; (m_ivar, ivar, state) of every leaf"""
    from la3dm_amd import _lib
    s = _lib.BgkScan()
    alpha, beta = sc.mi0.copy(), sc.iv0.copy()
    state = np.full(sc.keys.size, 0xEE, np.uint8)
    s.train_xyzy, s.train_off, s.nbr, s.blk_center = (sc.xyzy.ctypes.data, sc.train_off.ctypes.data, sc.nbr.ctypes.data,
                                                      sc.centre.ctypes.data)
    s.leaf_off, s.leaf_key = sc.leaf_off.ctypes.data, sc.keys.ctypes.data
    s.n_train_pts, s.n_train_blk = int(sc.train_off[-1]), len(sc.blocks)
    s.n_test_blk, s.n_leaf = len(sc.tests), int(sc.keys.size)
    s.alpha, s.beta, s.state, s.flags = alpha.ctypes.data, beta.ctypes.data, state.ctypes.data, 0
    if hints:
        s.train_max_n, s.train_sum_n2 = int(sc.sizes.max()), int((sc.sizes ** 2).sum())
    H = _lib.hip()
    if H.la3dm_gp_scan_host(m.ctx(), C.byref(s), None) != 0:
        raise RuntimeError(H.la3dm_last_error(m.ctx()).decode())
    return alpha, beta, state


def expect_restatement(O, P, sc, mode=0):
    """the restatement's answer: train_predict per training block (all its users' leaves), node updates in nbr order"""
    o = O.OracleGPMap(**dict(P, block_depth=sc.depth))
    users = sc.users()
    O.set_gp_mode(mode)
    try:
        res = dict(zip(users, POOL.map(lambda b: o.train_predict(*sc.blocks[b], sc.pos[users[b]])[2:], users)))
    finally:
        O.set_gp_mode(0)
    mi, iv = sc.mi0.copy(), sc.iv0.copy()
    st = np.zeros(sc.keys.size, np.uint8)
    where = {b: {int(l): j for j, l in enumerate(users[b])} for b in users}
    a, b_, s = C.c_float(), C.c_float(), C.c_uint8()
    for t in range(len(sc.tests)):
        for b in sc.nbr[t]:
            if b < 0 or sc.sizes[b] == 0:
                continue
            mu, var = res[int(b)]
            for li in range(sc.leaf_off[t], sc.leaf_off[t + 1]):
                j = where[int(b)][li]
                a.value, b_.value, s.value = mi[li], iv[li], st[li] & 3
                o.L.orc_gp_node_update(o.h, C.byref(a), C.byref(b_), C.byref(s), float(mu[j]), float(var[j]))
                mi[li], iv[li], st[li] = a.value, b_.value, s.value | 0x80
    return mi, iv, st


def expect_f64(P, sc):
    """the float64 reference's node values, their bounds and the states it allows (P = P2)"""
    D = R.derived(P)
    users = sc.users()

    def one(b):
        x, y = sc.blocks[b]
        m, var = R.GP64(x, y, P).predict(sc.pos[users[b]])
        return m, var, R.gp_bounds(len(y), R.max_scaled(P, x, sc.pos[users[b]]))

    res = dict(zip(users, POOL.map(one, users)))
    where = {b: np.searchsorted(users[b], np.arange(sc.keys.size)) for b in users}
    mi, iv = sc.mi0.astype(np.float64), sc.iv0.astype(np.float64)
    emi, eiv = np.zeros_like(mi), np.zeros_like(iv)
    unknown = np.ones(mi.size, bool)
    updated = np.zeros(mi.size, bool)
    for t in range(len(sc.tests)):
        sl = sc.leaves_of(t)
        for b in sc.nbr[t]:
            if b < 0 or sc.sizes[b] == 0:
                continue
            m, var, (bm, bv) = res[int(b)]
            j = where[int(b)][sl]
            mi[sl], iv[sl], unknown[sl] = R.node_update64(mi[sl], iv[sl], m[j], var[j], D)
            emi[sl], eiv[sl] = R.node_bounds(emi[sl], eiv[sl], mi[sl], iv[sl], m[j], var[j], bm, bv)
            updated[sl] = True
    st, p = R.node_state64(mi, unknown, D)
    ex = R.state_exempt(mi, p, iv, emi, eiv, D) | ~np.isfinite(emi) | ~np.isfinite(eiv)
    return dict(mi=mi, iv=iv, emi=emi, eiv=eiv, st=st, exempt=ex, updated=updated)


def assert_bits(got, want, tag):
    for k, a, b in zip(("m_ivar", "ivar"), got[:2], want[:2]):
        bad = a.view(np.uint32) != b.view(np.uint32)
        assert not bad.any(), (tag, k, int(bad.sum()), float(np.abs(a - b).max()))
    assert (got[2] == want[2]).all(), (tag, "state", int((got[2] != want[2]).sum()))


def assert_f64(got, f, tag):
    """within the float64 bound where it is finite; states equal except where the bound allows either"""
    fin = np.isfinite(f["emi"]) & np.isfinite(f["eiv"]) & f["updated"]
    assert (np.abs(got[0] - f["mi"]) <= f["emi"])[fin].all(), (tag, "m_ivar")
    assert (np.abs(got[1] - f["iv"]) <= f["eiv"])[fin].all(), (tag, "ivar")
    keep = f["updated"] & ~f["exempt"]
    assert ((got[2] & 3) == f["st"])[keep].all(), (tag, "state", int(((got[2] & 3) != f["st"])[keep].sum()))
    return int(fin.sum())


def _finest(depth):
    d = depth - 1
    return (d << 16) | np.arange(8 ** d, dtype=np.uint32)


def one_class_scan(N, depth, i, lut):
    """one training block of N points in the depth-3 cube at C0 (also inside the depth-4 one), 1-3 test blocks that have it
    as their neighbour in different slots, all their finest leaves"""
    rng = np.random.default_rng(100 * N + depth)
    c0 = np.float32([0.2, -0.2, 0.6])
    bs = np.float32(0.1 * 2 ** (depth - 1))
    sc = Scan(depth)
    sc.block(c0 + rng.uniform(-0.2, 0.2, (N, 3)), rng.choice([-1.0, 1.0], N))
    keys = _finest(depth)
    for k in sorted({(i + 3 * j) % 7 for j in range(1 + i % 3)}):
        nbr = [-1] * 7
        nbr[k] = 0
        sc.test(c0 - DIRS[k] * bs, keys, nbr, rng.uniform(-20, 20, keys.size), rng.uniform(0, 60, keys.size))
    return sc.pack(lut)


@pytest.fixture(scope="module")
def lib(built):
    from oracle import oracle as O
    luts = {d: np.ascontiguousarray(np.concatenate(O.OracleGPMap(**dict(R.GP_YAML, block_depth=d)).lut()), np.float32)
            for d in (3, 4)}   # Block::key_loc_map, depth-major (the host map hands the device the same table)
    return O, luts


@pytest.fixture(scope="module")
def one_class(lib):
    """(a)'s scans and their expected values, per depth: [(N, scan, {params: (restatement, f64 or None)})]"""
    O, luts = lib
    out = {}
    for depth in (3, 4):
        scans = [(N, one_class_scan(N, depth, i, luts[depth])) for i, N in enumerate(NS)]
        out[depth] = [(N, sc, {k: (expect_restatement(O, P, sc), expect_f64(P, sc) if k == "p2" else None)
                               for k, P in PARAMS.items()}) for N, sc in scans]
    return out


@pytest.mark.parametrize("depth", [3, 4])
def test_one_class_per_scan(lib, one_class, depth):
    """(a): every N alone chooses every launch; bit-identical to the restatement with and without the hints, within the
    float64 bound at P2 (which has something to say, finite bounds, for every leaf up to N = 257)"""
    lut = lib[1][depth]
    assert_every_class([N for N, _, _ in one_class[depth]])
    for N, sc, exp in one_class[depth]:
        for k, P in PARAMS.items():
            want, f = exp[k]
            for hints in (False, True):
                with Ctx(P, depth, lut) as m:
                    assert_bits(run(m, sc, hints), want, (N, depth, k, hints))
            if f is not None:
                n_fin = assert_f64(want, f, (N, depth))
                assert N > 257 or n_fin == sc.keys.size, (N, depth, n_fin)


@pytest.mark.parametrize("depth", [3, 4])
def test_stale_arenas(lib, one_class, depth):
    """(b): the (a) scans one after the other on ONE context, largest N to smallest and back: what a call leaves in the
    arenas (padded factor rows, vscratch rows, offsets) is never read by the next — the same bits as on a fresh context"""
    cases = one_class[depth]
    order = list(range(len(cases)))[::-1] + list(range(1, len(cases)))
    for k, P in PARAMS.items():
        with Ctx(P, depth, lib[1][depth]) as m:
            for i in order:
                N, sc, exp = cases[i]
                assert_bits(run(m, sc, hints=bool(i % 2)), exp[k][0], (N, depth, k, "stale"))


def mixed_scan(lut, n_blocks):
    """(c) at block_depth 4; the first part of the block list is the same for every n_blocks, the rest is 1-4-point fill"""
    rng = np.random.default_rng(7)
    sc = Scan(4)
    pt = lambda n: rng.uniform(-0.6, 0.6, (n, 3))   # noqa: E731 (every block near every test block: all neighbours matter)
    lab = lambda n: rng.choice([-1.0, 1.0], n)      # noqa: E731
    idx = {}
    for N in NS:
        for _ in range(30):
            sc.block(pt(f := int(rng.integers(1, 5))), lab(f))
        x = pt(N)
        if N == 129:
            x[-10:] = x[:10]                                 # duplicates in an MFMA-factored block
        idx[N] = sc.block(x, lab(N))
    x = pt(6)
    dup = sc.block(np.concatenate([x, x]), lab(12))           # every point twice: only the noise keeps K positive definite
    empty = sc.block(np.zeros((0, 3)), np.zeros(0))
    fill = [sc.block(pt(f := int(rng.integers(1, 5))), lab(f)) for _ in range(8)]
    assert len(sc.blocks) < CONST["kGpOffThreads"] - 1
    F = lambda *ns: [idx[n] if isinstance(n, int) and n > 0 else n for n in ns]   # noqa: E731
    E = "empty"
    sets = [(F(3, 64, 65, 129, -1, E, 1025), 65), (F(-1, -1, -1, -1, -1, -1, -1), 20),
            (F(1, 2, 4, 5, 31, 32, 33), 1), (F(63, 66, 127, 128, 159, 160, 161), 63),
            (F(255, 256, 257, 531, -1, -1, -1)[:4] + [dup, fill[0], fill[1]], "pruned"), (F(1, -1, -1, -1, -1, -1, -1), 64),
            (F(-1, 31, -1, 3, -1, -1, -1), 64), (F(E, 64, 2, -1, 63, -1, 4), 40), (F(-1, -1, -1, 65, -1, -1, -1), 64),
            (F(E, -1, -1, -1, -1, -1, -1), 10), ([fill[2], fill[3], fill[4], dup, fill[5], fill[6], fill[7]], 64),
            (F(1025, 531, 257, 129, 65, 33, 1), 8), (F(161, 160, 159, 127, 66, 32, 5), 100)]
    finest = _finest(4)
    for t, (nb, nl) in enumerate(sets):
        nb = [empty if b == E else b for b in nb]
        if nl == "pruned":   # depth-1 leaves 0-2, the depth-2 children of node 3, the finest leaves below nodes 4-7
            keys = np.concatenate([(1 << 16) | np.arange(3), (2 << 16) | np.arange(24, 32), (3 << 16) | np.arange(32 * 8, 512)])
        else:
            keys = np.sort(rng.choice(finest, nl, replace=False))
        n = keys.size
        mi0 = rng.uniform(-30, 30, n)
        iv0 = np.where(np.arange(n) % 3 == 0, rng.uniform(985, 1000, n), rng.uniform(0, 60, n))   # a third near the clamp
        sc.test(rng.uniform(-0.4, 0.4, 3), keys.astype(np.uint32), nb, mi0, iv0)
    while len(sc.blocks) < n_blocks:   # (drawn last: the rest of the scan does not depend on n_blocks)
        sc.block(pt(f := int(rng.integers(1, 5))), lab(f))
    sc.pack(lut)
    return sc, idx, empty


def test_mixed_scan(lib):
    """(c): everything at once, with kGpOffThreads - 1, kGpOffThreads, kGpOffThreads + 1 and 3 kGpOffThreads + 5 training
    blocks (gp_factor_offsets' threads walk 1, 1, 2 and 4 blocks each): the same referenced blocks in the same places, so
    the same answer"""
    O, luts = lib
    T = CONST["kGpOffThreads"]
    sc0, idx, empty = mixed_scan(luts[4], T - 1)
    assert_every_class(sorted(idx))
    assert len(sc0.tests) % 8 != 0 and set(NS) <= {int(sc0.sizes[b]) for t in sc0.nbr for b in t if b >= 0}
    assert {1, 63, 65} <= set(np.diff(sc0.leaf_off.astype(np.int64)).tolist()) and (sc0.keys >> 16 < 3).any()
    none = [t for t in range(len(sc0.tests)) if all(b < 0 or sc0.sizes[b] == 0 for b in sc0.nbr[t])]
    assert len(none) == 2 and any(empty in sc0.nbr[t] for t in none)
    exp = {k: expect_restatement(O, P, sc0) for k, P in PARAMS.items()}
    f = expect_f64(R.P2, sc0)
    for k, P in PARAMS.items():
        mi, iv, st = exp[k]
        D = R.derived(P)
        upd = (st & 0x80) != 0
        # the priors and blocks make every outcome occur: free, occupied, unknown (by ivar and by p), the clamp
        assert {0, 1, 2} <= set((st[upd] & 3).tolist()), k
        assert (iv[upd] == np.float32(D["max_ivar"])).any() and (iv[upd] < np.float32(D["min_known_ivar"])).any(), k
        for t in none:
            sl = sc0.leaves_of(t)
            assert (st[sl] == 0).all() and (mi[sl] == sc0.mi0[sl]).all() and (iv[sl] == sc0.iv0[sl]).all()
    for n_blocks in (T - 1, T, T + 1, 3 * T + 5):
        sc = sc0 if n_blocks == T - 1 else mixed_scan(luts[4], n_blocks)[0]
        assert len(sc.blocks) == n_blocks and (sc.nbr == sc0.nbr).all() and (sc.pos == sc0.pos).all()
        for k, P in PARAMS.items():
            with Ctx(P, 4, luts[4]) as m:
                got = run(m, sc, hints=n_blocks > T)
            assert_bits(got, exp[k], (n_blocks, k))
            if k == "p2":
                assert_f64(got, f, n_blocks)


EIGEN_NS = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 127, 128]


@pytest.mark.parametrize("depth", [3, 4])
def test_gp_mode_1_at_the_eigen_edges(lib, depth):
    """(d): gp_mode 1 bit-identical to oracle.set_gp_mode(1) where the Eigen-order factorisation changes shape: unblocked
    below 32, blocks of 8 from 32 to 127, of 16 at 128, panels of 8 (N % 8), two rows per lane above 64"""
    O, luts = lib
    assert max(EIGEN_NS) == CONST["kGpEigenMaxN"]
    bs = lambda n: min(max(n // 8 // 16 * 16, 8), 128) if n >= 32 else 0   # noqa: E731 (llt_inplace's block size)
    assert {bs(n) for n in EIGEN_NS} == {0, 8, 16} and {n % 8 == 0 for n in EIGEN_NS} == {True, False}
    assert {n > 64 for n in EIGEN_NS} == {True, False}
    for i, N in enumerate(EIGEN_NS):
        sc = one_class_scan(N, depth, i, luts[depth])
        for k, P in PARAMS.items():
            want = expect_restatement(O, P, sc, mode=1)
            with Ctx(P, depth, luts[depth], gp_mode=1) as m:
                assert_bits(run(m, sc, hints=bool(i % 2)), want, (N, depth, k, "gp_mode 1"))


def test_gp_mode_1_refuses_one_point_too_many(lib):
    """(d): one block of kGpEigenMaxN + 1 points is refused in gp_mode 1 with the cause named; the context then runs the
    same scan in gp_mode 0 (bit-identical to the restatement)"""
    O, luts = lib
    N = CONST["kGpEigenMaxN"] + 1
    sc = one_class_scan(N, 3, 0, luts[3])
    want = expect_restatement(O, R.GP_YAML, sc)
    with Ctx(R.GP_YAML, 3, luts[3], gp_mode=1) as m:
        with pytest.raises(RuntimeError, match=f"gp_mode 1.*{CONST['kGpEigenMaxN']}.*{N}"):
            run(m, sc)
        m.set_option("gp_mode", 0)
        assert_bits(run(m, sc), want, (N, "after refusal"))
