"""Float64 GP reference for the GPOctoMap tests (tests/test_gp_f64_cpu.py, tests/test_gp_sizes_gpu.py).

Written from the reference's formulas, not from oracle/:
  train    include/gpoctomap/gpregressor.h:42-51    K = Matern32(x, x) sf2 + noise I, LLT, alpha = K^-1 y
  predict  include/gpoctomap/gpregressor.h:80-92    m = Ks^T alpha, v = L^-1 Ks, var = sf2 - sum_k v_k^2
  kernel   include/gpoctomap/gpregressor.h:114-117  a = |(1.73205 / ell)(x - x')|, k = (1 + a) exp(-a) sf2
  update   src/gpoctomap/gpoctree_node.cpp:31-49    ivar += 1 / var - sf2, m_ivar += m / var, unknown below
                                                    min_known_ivar, else ivar clamped at max_ivar; logistic p
numpy only (np.linalg.cholesky, np.linalg.solve).  Inputs are the fp32 values the kernels see: the training points and the
leaf positions (lut[key] + block centre, added in fp32), and the fp32 scale (float)(1.73205 / ell) that the kernels and the
restatement multiply by, widened.  Everything after that is float64.

Error bound (gp_bounds) of an fp32 evaluation of the same regressor, u = 2^-24, gamma_n = n u / (1 - n u), for the parameter
set P2 (sf2 = 1, noise = 1), where lambda_min(K) >= 1 and lambda_max(K) <= N + 1, so ||K^-1|| <= 1 and kappa(K) <= N + 1:
  * kernel values: a scaled coordinate is off by <= u X (X = largest |scaled coordinate|), a difference by 2 u X + u |dx|,
    the distance by <= 2 sqrt(3) u X + 4 u a; |d/da (1 + a) e^-a| <= 1/e and a^2 e^-a <= 4/e^2, and the three roundings of
    (1 + a) exp(-a) add 3 u:  eps = (2 sqrt(3) / e X + 16 / e^2 + 3) u  per entry of K and of Ks.
  * the Cholesky factorisation (|dK| <= gamma_{N+2} |L||L^T|, the +1 for a reciprocal of the diagonal) and a triangular
    solve with the computed factor (|dL| <= gamma_N |L|) act as one perturbation of K; (|L||L^T|)_ij <= sqrt(K_ii K_jj) =
    sf2 + noise = 2, so entrywise E = 2 gamma_{N+2} + 4 gamma_N + 2 gamma_N^2 + eps, and ||dK||_2 <= N E.
  * var: v^T v = Ks^T K^-1 Ks <= sf2 and ||K^-1 Ks|| <= 1, hence
      |dvar| <= (1 + sqrt(N) eps)^2 N E / (1 - N E) + 2 sqrt(N) eps + N eps^2 + gamma_N (1 + sqrt(N) eps)^2 + 2 u
  * m: |dm| <= ||K^-1 Ks|| ||dK|| ||alpha^|| + (||dKs|| + gamma_N ||Ks^||) ||alpha^||, ||alpha^|| <= ||y|| / (1 - N E):
      |dm| <= sqrt(N) / (1 - N E) (N E + sqrt(N) eps + sqrt(N) gamma_N (1 + eps))
  var's bound grows like 6 N^2 u, m's like 6 N^2.5 u.  Worst-case constants and no assumption about the order of the
  operations: the same bound covers the FMA-chain order (gp_mode 0), the Eigen order (gp_mode 1) and the matrix-core tiles.
  node_bounds carries the two through the fp32 node update, leaf by leaf, from the float64 m and var.
"""
import os
import re

import numpy as np

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "la3dm_amd", "csrc")

# config/methods/gpoctomap.yaml (la3dm_amd.GP_YAML), restated so that this module imports nothing of the package
GP_YAML = dict(resolution=0.1, block_depth=3, sf2=1.0, ell=1.0, noise=0.01, l=100.0, min_var=0.001, max_var=1000.0,
               max_known_var=0.02, free_thresh=0.3, occupied_thresh=0.7)
# the parameter set in which a float64 comparison bounds something: lambda_min(K) >= noise = 1, kappa(K) <= N + 1
P2 = dict(GP_YAML, sf2=1.0, noise=1.0, ell=0.3)


def gp_constants():
    """the kernel-size thresholds of the GP path, parsed from the headers the library is built from"""
    src = ""
    for f in ("gp_kernels.h", "gp_eigen_kernels.h"):
        with open(os.path.join(CSRC, f)) as fh:
            src += fh.read()
    c = {k: int(v) for k, v in re.findall(r"constexpr\s+(?:int|uint32_t)\s+(kGp\w+)\s*=\s*(\d+)\s*;", src)}
    c["kGpMfmaMinN"] = int(re.search(r"#define\s+LA3DM_GP_MFMA_MIN_N\s+(\d+)", src).group(1))
    for k in ("kGpTrainTinyN", "kGpTrainLdsMaxN", "kGpOffThreads", "kGpLdsRows", "kGpMfmaMinN", "kGpEigenMaxN"):
        assert k in c, k
    return c


def size_list(c=None):
    """training-block sizes N: t - 1, t, t + 1 of every size threshold (kGpOffThreads counts blocks, not points: the mixed
    scan straddles it with its number of training blocks), the four-row tails, the 32 x 32 tile edges, configs[2]'s largest
    depth-4 block (531) and one beyond anything the BASELINE configs produce (1025)"""
    c = c or gp_constants()
    t = (c["kGpTrainTinyN"], c["kGpTrainLdsMaxN"], c["kGpLdsRows"], c["kGpMfmaMinN"], c["kGpEigenMaxN"])
    ns = {n for x in t for n in (x - 1, x, x + 1)}
    ns |= {1, 2, 3, 4, 5, 159, 160, 161, 255, 256, 257, 531, 1025}
    return sorted(n for n in ns if n >= 1)


def derived(P):
    """the node statics as the library and the reference hold them (fp32), widened"""
    f = np.float32
    return dict(sf2=float(f(P["sf2"])), l=float(f(P["l"])), max_ivar=float(f(1.0) / f(P["min_var"])),
                min_known_ivar=float(f(1.0) / f(P["max_known_var"])), free=float(f(P["free_thresh"])),
                occ=float(f(P["occupied_thresh"])))


def scale(ell):
    return float(np.float32(1.73205 / ell))


def matern(a, b, s, sf2):
    """covMaterniso3(a, b): [len(a), len(b)] in float64 (a, b unscaled positions)"""
    a = np.asarray(a, np.float64) * s
    b = np.asarray(b, np.float64) * s
    d = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
    return (1.0 + d) * np.exp(-d) * sf2


class GP64:
    """GPRegressor<3, double> on the fp32 inputs"""

    def __init__(self, x, y, P):
        self.x = np.asarray(x, np.float32).reshape(-1, 3)
        self.s, self.sf2 = scale(P["ell"]), float(np.float32(P["sf2"]))
        self.K = matern(self.x, self.x, self.s, self.sf2) + float(np.float32(P["noise"])) * np.eye(len(self.x))
        self.L = np.linalg.cholesky(self.K)
        self.alpha = np.linalg.solve(self.K, np.asarray(y, np.float64))

    def predict(self, xs):
        Ks = matern(self.x, np.asarray(xs, np.float32).reshape(-1, 3), self.s, self.sf2)
        m = Ks.T @ self.alpha
        v = np.linalg.solve(self.L, Ks)
        return m, self.sf2 - (v * v).sum(0)


def gamma(n, u=U):
    return n * u / (1.0 - n * u)


def gp_bounds(N, X, u=U):
    """(|dm|, |dvar|) bounds of an fp32 evaluation at P2 (module docstring); X = largest |scaled coordinate|"""
    eps = (2.0 * np.sqrt(3.0) / np.e * X + 16.0 / np.e ** 2 + 3.0) * u
    gN = gamma(N, u)
    E = 2.0 * gamma(N + 2, u) + 4.0 * gN + 2.0 * gN * gN + eps
    NE = N * E
    if NE >= 1.0:
        return np.inf, np.inf
    rN = np.sqrt(N)
    bvar = (1 + rN * eps) ** 2 * NE / (1 - NE) + 2 * rN * eps + N * eps * eps + gN * (1 + rN * eps) ** 2 + 2 * u
    bm = rN / (1 - NE) * (NE + rN * eps + rN * gN * (1 + eps))
    return bm, bvar


def max_scaled(P, *pts):
    """X of gp_bounds for these point sets"""
    return scale(P["ell"]) * max(float(np.abs(np.asarray(p, np.float64)).max()) for p in pts if np.size(p))


def node_update64(mi, iv, m, var, D):
    """Occupancy::update in float64 (arrays); returns (m_ivar, ivar, unknown)"""
    iv = iv + (1.0 / var - D["sf2"])
    mi = mi + m / var
    unknown = iv < D["min_known_ivar"]
    iv = np.where(unknown, iv, np.minimum(iv, D["max_ivar"]))
    return mi, iv, unknown


def node_bounds(emi, eiv, mi, iv, m, var, bm, bvar, u=U):
    """bounds on the fp32 node after one more update (m_ivar = fl(m_ivar + fl(m / var)); ivar = ivar + (1 / var - sf2) in
    double, rounded once, then clamped: 1-Lipschitz) from the bounds before it (emi, eiv), the float64 node after it
    (mi, iv) and the float64 m, var with their bounds; inf where var is within its bound of 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        ok = var > bvar
        den = np.where(ok, var * (var - bvar), 1.0)
        dq = np.where(ok, (bm * var + np.abs(m) * bvar) / den, np.inf)
        dq = dq + u * (np.abs(m / var) + dq)
        dr = np.where(ok, bvar / den, np.inf)
        emi = (emi + dq) * (1 + u) + u * np.abs(mi)
        eiv = (eiv + dr) * (1 + u) + u * np.abs(iv) + 8 * 2.0 ** -53 * (np.abs(iv) + np.abs(1.0 / var))
    return emi, eiv


def node_state64(mi, unknown, D):
    """state code of gpoctree_node.cpp (FREE 0, OCCUPIED 1, UNKNOWN 2) and the float64 p"""
    p = 1.0 / (1.0 + np.exp(-D["l"] * mi / D["max_ivar"]))
    st = np.where(p > D["occ"], 1, np.where(p < D["free"], 0, 2))
    return np.where(unknown, 2, st).astype(np.uint8), p


def state_exempt(mi, p, iv, emi, eiv, D, u=U):
    """leaves whose state an fp32 evaluation within the bounds may decide either way: p within its bound of a threshold, or
    ivar within its bound of min_known_ivar (the logistic's slope is <= 1/4; its fp32 evaluation adds a few u)"""
    arg = D["l"] * np.abs(mi) / D["max_ivar"]
    dp = 0.25 * D["l"] / D["max_ivar"] * emi + (0.5 * arg + 4.0) * u
    return (np.abs(p - D["occ"]) <= dp) | (np.abs(p - D["free"]) <= dp) | (np.abs(iv - D["min_known_ivar"]) <= eiv)
