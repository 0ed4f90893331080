"""CPU: the restatement's GP regressor (oracle.OracleGPMap.train_predict: gp_mode 0 = FMA chains in ascending order, the
order the HIP kernels use; gp_mode 1 = Eigen 3.3.7's order) against an independent float64 evaluation of the reference's
formulas (tests/gp_f64_ref.py, numpy only), at every training-block size the GP kernels dispatch on (gp_f64_ref.size_list:
the thresholds parsed from la3dm_amd/csrc/gp_kernels.h and gp_eigen_kernels.h).  Every other GP check compares the kernels
with the restatement; this one would notice both misreading gpregressor.h / gpoctree_node.cpp the same way.

Parameter set gp_f64_ref.P2: sf2 = 1, noise = 1, ell = 0.3, the rest from GP_YAML.  K = Matern + I, so lambda_min(K) >= 1
and lambda_max(K) <= N + 1 (asserted in float64): kappa(K) <= N + 1 by construction.  The bound on |m - m64| and
|var - var64| is derived in gp_f64_ref's docstring (gp_bounds): var within 6 N^2 u (1 + O(N u)), m within 6 N^2.5 u (...),
u = 2^-24.  Worst-case constants: at N = 65 the bounds are 1.3e-2 (m) and 1.6e-3 (var); the largest errors observed over
the whole N list are 1.0e-5 (m) and 2.8e-6 (var), both at N = 1025 in gp_mode 0, and no error exceeds 5 % of its bound
(the largest ratios at the smallest N, where the bound is tightest).

Teeth.  The last training point sits next to a leaf, the other points away from it; dropping that point (the classic
partial-tile off-by-one) must move the float64 result at that leaf by more than 10x the bound.  That holds for var at
N = 65, 129 and 257, and for m at N = 65 only: from N = 129 on, m's bound (7e-2, 0.4 at 257) is too loose for a single point
to stand out 10x, and the float64 comparison of m has no teeth there — at those sizes the kernels are held to the
restatement bit for bit (tests/test_gp_sizes_gpu.py), and the restatement to this file's var comparison.
"""
import numpy as np
import pytest

import gp_f64_ref as R

NS = R.size_list()
P = R.P2
CENTRE = np.float32([0.6, -0.2, 0.2])   # a block centre at block_depth 3 (0.4 m cube)


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def leaves(O):
    """the 64 finest leaves of the block at CENTRE: lut[key] + centre in fp32, as Block::get_loc computes them"""
    lut = O.OracleGPMap(**dict(P, block_depth=3)).lut()[2]
    return (lut + CENTRE).astype(np.float32)


def _block(N, seed=0):
    rng = np.random.default_rng(1000 + N + seed)
    x = (CENTRE + rng.uniform(-0.2, 0.2, (N, 3))).astype(np.float32)
    y = rng.choice(np.float32([-1.0, 1.0]), N)   # labels as gpoctomap.cpp:383, 399 writes them
    return x, y


def _train_predict(O, mode, x, y, xs):
    o = O.OracleGPMap(**P)
    O.set_gp_mode(mode)
    try:
        return o.train_predict(x, y, xs)
    finally:
        O.set_gp_mode(0)


@pytest.mark.parametrize("N", NS)
def test_restatement_within_the_float64_bound(O, leaves, N):
    """gp_mode 0 (every N) and gp_mode 1 (N <= kGpEigenMaxN) against the float64 reference, within the derived bound"""
    x, y = _block(N)
    g = R.GP64(x, y, P)
    lam = np.linalg.eigvalsh(g.K)
    assert lam[0] >= 1.0 - 1e-9 and lam[-1] <= N + 1.0 + 1e-9, (lam[0], lam[-1])
    m64, v64 = g.predict(leaves)
    bm, bv = R.gp_bounds(N, R.max_scaled(P, x, leaves))
    assert np.isfinite(bm) and np.isfinite(bv)
    modes = (0, 1) if N <= R.gp_constants()["kGpEigenMaxN"] else (0,)
    for mode in modes:
        _, _, m, var = _train_predict(O, mode, x, y, leaves)
        assert np.abs(m - m64).max() <= bm, (mode, float(np.abs(m - m64).max()), bm)
        assert np.abs(var - v64).max() <= bv, (mode, float(np.abs(var - v64).max()), bv)


def test_the_f64_mode_is_the_helper(O, leaves):
    """oracle.set_gp_mode(2) (the restatement's own float64 path, outputs rounded to fp32) and gp_f64_ref compute the same
    formula: they agree to within one fp32 rounding of the outputs, plus the two float64 evaluations' own bound (gp_bounds
    with u = 2^-53)"""
    for N in NS:
        x, y = _block(N)
        m64, v64 = R.GP64(x, y, P).predict(leaves)
        bm, bv = R.gp_bounds(N, R.max_scaled(P, x, leaves), u=2.0 ** -53)
        _, _, m, var = _train_predict(O, 2, x, y, leaves)
        assert (np.abs(m - m64) <= R.U * np.abs(m64) + 2 * bm).all(), (N, float(np.abs(m - m64).max()))
        assert (np.abs(var - v64) <= R.U * np.abs(v64) + 2 * bv).all(), (N, float(np.abs(var - v64).max()))


@pytest.mark.parametrize("N", [65, 129, 257])
def test_the_bound_has_teeth(O, leaves, N):
    """the last training point 1 cm from a leaf, the other N - 1 in a cube of the block's size 1 m away from it (Matern
    weight < 0.01 at ell = 0.3): the float64 result without that point differs from the full one by more than 10x the bound
    (var at every N here, m at N = 65; see the module docstring), and the restatement at that leaf stays within the bound
    of the full result"""
    x, y = _block(N)
    j = int(np.argmax(leaves[:, 0]))                     # a leaf on the +x face
    x[:-1, 0] -= np.float32(1.0) + (leaves[j, 0] - CENTRE[0])
    x[-1] = leaves[j] + np.float32([0.0, 0.0, 0.01])
    y[-1] = 1.0
    xs = leaves[j:j + 1]
    m1, v1 = R.GP64(x, y, P).predict(xs)
    m0, v0 = R.GP64(x[:-1], y[:-1], P).predict(xs)
    bm, bv = R.gp_bounds(N, R.max_scaled(P, x, xs))
    assert abs(v1[0] - v0[0]) > 10 * bv, (float(abs(v1[0] - v0[0])), bv)
    if N == 65:
        assert abs(m1[0] - m0[0]) > 10 * bm, (float(abs(m1[0] - m0[0])), bm)
    _, _, m, var = _train_predict(O, 0, x, y, xs)
    assert abs(m[0] - m1[0]) <= bm and abs(var[0] - v1[0]) <= bv
