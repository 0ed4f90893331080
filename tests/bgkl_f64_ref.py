"""Float64 BGK-L reference for the BGKLOctoMap tests (tests/test_bgkl_f64_cpu.py, tests/test_bgkl_scans_gpu.py).

Written from the reference's formulas, not from oracle/ or la3dm_amd (numpy only, imports neither):
  predict   include/bgkloctomap/bgklinference.h:80-88     ybar = Ks y, kbar = Ks.rowwise().sum()
  distance  include/bgkloctomap/bgklinference.h:104-140   point_to_line_dist: |p - p0| for a segment shorter than 0.0001, else
                                                          c1 = (p - p0).l, c2 = l.l; c1 <= 0: |p - p0|; c2 <= c1: |p - p1|;
                                                          else |p - (p0 + l c1 / c2)|
  kernel    include/bgkloctomap/bgklinference.h:186-200   r = d / ell, k = ((2 + cos(2 pi r)) (1 - r) / 3 + sin(2 pi r) / (2 pi)) sf2
                                                          with pi = 3.1415926f, k < 0 -> 0
  update    src/bgkloctomap/bgkloctomap.cpp:206-231       for every trained neighbour in ExtendedBlock order: kbar > 0.001f ?
  node      src/bgkloctomap/bgkloctree_node.cpp:31-44     A += ybar, B += kbar - ybar; var = A B / ((A + B)^2 (A + B + 1));
                                                          var > var_thresh: UNKNOWN, else p = A / (A + B) against the thresholds
Inputs are the fp32 values the kernels see, widened: rows of 8 floats {x0 y0 z0 x1 y1 z1 label 0}, leaf positions (lut[key] +
block centre, added in fp32), ell, sf2, the thresholds, 0.001f, 0.0001f and 3.1415926f.  Everything after that is float64.

Error bound of an fp32 evaluation of the same formulas (u = 2^-24, gamma_n = n u / (1 - n u)), worst-case constants, no
assumption about the order of the operations or about fused multiply-adds:
  * distance.  X = largest |coordinate| of the leaf and the row.  A hit (degenerate row) and the two end-point branches
    subtract two inputs: fl(p_i - q_i) is off by u |p_i - q_i|, three squares, two additions and the root add 2.5 u d:
    |dd| <= 4 u d, no X.  In the projection branch l_i and v_i = p_i - p0_i carry u each, c1 = v.l is off by gamma_5 |v||l|,
    c2 by gamma_5 c2, b = c1 / c2 (clamped to [0, 1], 1-Lipschitz, which also covers a branch decided the other way: the
    distance is continuous across the branches) moves the nearest point along the line by |l||db| <= gamma_5 |v| + gamma_6 |l|
    <= gamma_11 2 sqrt(3) X <= 38.2 u X; nearest_i = fl(p0_i + fl(l_i b)) is off by u (2 |l_i| + |q_i|) <= 5 u X per
    component, 8.7 u X as a vector — this is the cancellation in p - q: the difference is taken of numbers of size X.  The
    distance to a displaced point differs by at most the displacement:
        E_d = (48 X [row is a beam] + 4 d) u
  * r = d / ell adds u r:  E_r = E_d / ell + u r.
  * kernel.  g(r) = (2 + cos t)(1 - r) / 3 + sin t / (2 pi), t = 2 pi r:  g' = (2/3)(cos t - 1) - (2 pi / 3)(1 - r) sin t,
    |g''| <= 2 pi / 3 + (4 pi^2 / 3) |1 - r|.  Taylor at the float64 r:  |g(r') - g(r)| <= |g'(r)| E_r + M2 E_r^2 / 2 with
    M2 = 2 pi / 3 + (4 pi^2 / 3)(|1 - r| + E_r).  The fp32 evaluation of g at r' (t to 2 pi u, correctly rounded or not the
    sine and cosine to (1 + 2 pi) u + their own u, eleven roundings of values <= 3) adds less than 12 u; the clean-up
    max(., 0) is 1-Lipschitz:
        e_k = sf2 (|g'(r)| E_r + M2 E_r^2 / 2 + 12 u)
    A row out of reach, r - E_r >= 1: g <= g(1) for every r' >= 1 (on [1, 1.5] g' <= 0 <=> x cos x <= sin x, x = pi (r - 1);
    beyond, g <= -(r - 1) / 3 + 1 / (2 pi) < 0), and g(1) = 2.8e-8 only because 3.1415926f is not pi:  e_k = sf2 13 u there,
    whatever its distance.  g is flat at 1 (g ~ 8.7 (1 - r)^5), so rows that graze the support cost almost nothing.
  * sums of a neighbour with N rows, S = sum k, E = sum e_k (likewise for ybar over k * label, labels 0 / 1 exact):
        ordered mode (bgk_sum 0)     an fp32 chain of N non-negative terms, any order:   e = E + gamma_N (S + E)
        order-free mode (bgk_sum 1)  a double chain, one rounding to fp32:               e = E + (u + gamma_N(2^-53)) (S + E)
  * gate: kbar > 0.001f.  A (leaf, neighbour) pair whose float64 kbar lies within e of 0.001f is left out of the gate
    comparison; its update then enters the node's bound in full (either decision is allowed).
  * the (up to) seven updates A = fl(A + ybar), B = fl(B + fl(kbar - ybar)):
        eA <- (eA + e_y)(1 + u) + u |A|,   eB <- (eB + (e_k + e_y)(1 + u) + u |kbar - ybar|)(1 + u) + u |B|
  * state: |dp| <= (B eA + A eB) / (s (s - eA - eB)) + 3 u, the variance relatively (1 + eA / A)(1 + eB / B)(1 + u)^8 /
    (1 - rho_s)^3 - 1 with rho_s = (eA + eB) / s + u.  A leaf whose float64 p or variance lies within that of a threshold is
    left out of the state comparison.
Hand-built segments keep their length away from the 0.0001 switch (0, 5e-5 or >= 2e-4: asserted by dist64).
"""
import os
import re

import numpy as np

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "la3dm_amd", "csrc")

# config/methods/bgkloctomap.yaml (la3dm_amd.L_YAML), restated so that this module imports nothing of the package
L_YAML = dict(resolution=0.1, block_depth=3, sf2=0.1, ell=0.2, free_thresh=0.3, occupied_thresh=0.7, var_thresh=0.15,
              prior_A=0.001, prior_B=0.001)
# nearly every row reaches every leaf of a 0.4 m tile; the hit ring of the order-free kernels fills in three rows
P5 = dict(L_YAML, ell=0.5)

PI_F = float(np.float32(3.1415926))
GATE = float(np.float32(0.001))
EPSILON = float(np.float32(0.0001))
FREE, OCCUPIED, UNKNOWN = 0, 1, 2
CX, CD, CK = 48.0, 4.0, 12.0


def bgkl_constants():
    """the sizes the BGK-L kernels dispatch on, parsed from the headers the library is built from"""
    src = ""
    for f in ("bgk_kernels.h", "bgkl_kernels.h"):
        with open(os.path.join(CSRC, f)) as fh:
            src += fh.read()
    c = {k: int(v) for k, v in re.findall(r"constexpr\s+(?:int|uint32_t)\s+(k\w+)\s*=\s*(\d+)\s*;", src)}
    for k in ("kLItemRows", "kLBatch", "kLRing", "kLWideTiles", "kWave"):
        assert k in c, k
    return {k: c[k] for k in ("kLItemRows", "kLBatch", "kLRing", "kLWideTiles", "kWave")}


def row_sizes(c=None):
    """rows per training block: t - 1, t, t + 1 for the row trip (kWave) and the item (kLItemRows), two items and one row,
    and 7, 8 and 9 items (bgkl_split_apply64 adds eight items per trip)"""
    c = c or bgkl_constants()
    w, it = c["kWave"], c["kLItemRows"]
    return sorted({w - 1, w, w + 1, it - 1, it, it + 1, 2 * it + 1, 7 * it, 8 * it, 8 * it + 1})


def derived(P):
    """the parameters as the library and the reference hold them (fp32), widened"""
    f = np.float32
    return {k: float(f(P[k])) for k in ("sf2", "ell", "free_thresh", "occupied_thresh", "var_thresh")}


def gamma(n, u=U):
    return n * u / (1.0 - n * u)


def dist64(pos, rows):
    """point_to_line_dist: [len(pos), len(rows)] in float64, and which rows are beams (not degenerate)"""
    p = np.asarray(pos, np.float32).astype(np.float64).reshape(-1, 3)
    r = np.asarray(rows, np.float32).astype(np.float64).reshape(-1, 8)
    a, b = r[:, 0:3], r[:, 3:6]
    lv = b - a
    ln = np.sqrt((lv * lv).sum(-1))
    assert not ((ln > 7e-5) & (ln < 1.5e-4)).any(), "a segment too close to the 0.0001 degeneracy switch"
    beam = ~(ln < EPSILON)
    v = p[:, None, :] - a[None, :, :]
    c1 = (v * lv[None]).sum(-1)
    c2 = (lv * lv).sum(-1)
    t = np.where(c1 <= 0.0, 0.0, np.where(c2[None] <= c1, 1.0, c1 / np.where(c2 > 0.0, c2, 1.0)[None]))
    t = np.where(beam[None], t, 0.0)
    q = a[None] + lv[None] * t[..., None]
    return np.sqrt(((p[:, None, :] - q) ** 2).sum(-1)), beam


def g64(r):
    t = 2.0 * PI_F * r
    return (2.0 + np.cos(t)) * (1.0 - r) / 3.0 + np.sin(t) / (2.0 * PI_F)


def kernel64(d, D):
    """covSparseLine on distances"""
    return np.maximum(g64(d / D["ell"]) * D["sf2"], 0.0)


def kernel_bound(d, beam, X, D, u=U):
    """e_k of the module docstring for distances d [leaf, row]"""
    r = d / D["ell"]
    Ed = (CX * X * beam[None].astype(np.float64) + CD * d) * u
    Er = Ed / D["ell"] + u * r
    t = 2.0 * PI_F * r
    g1 = np.abs((2.0 / 3.0) * (np.cos(t) - 1.0) - (2.0 * PI_F / 3.0) * (1.0 - r) * np.sin(t))
    M2 = 2.0 * PI_F / 3.0 + (4.0 * PI_F ** 2 / 3.0) * (np.abs(1.0 - r) + Er)
    e = D["sf2"] * (g1 * Er + 0.5 * M2 * Er * Er + CK * u)
    return np.where(r - Er >= 1.0, D["sf2"] * (CK + 1.0) * u, e)


def predict64(pos, rows, P, mode=0, u=U):
    """(ybar, kbar, e_y, e_k, k) of the leaves at pos against one training block: the float64 sums, their bounds for an
    fp32 evaluation in the ordered (mode 0) or order-free (mode 1) accumulate mode, and the float64 k [leaf, row]"""
    D = derived(P)
    rows = np.asarray(rows, np.float32).reshape(-1, 8)
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    n = len(rows)
    if n == 0 or len(pos) == 0:
        z = np.zeros(len(pos))
        return z, z.copy(), z.copy(), z.copy(), np.zeros((len(pos), n))
    d, beam = dist64(pos, rows)
    X = max(float(np.abs(pos.astype(np.float64)).max()), float(np.abs(rows[:, :6].astype(np.float64)).max()))
    k = kernel64(d, D)
    ek = kernel_bound(d, beam, X, D, u)
    lab = rows[:, 6].astype(np.float64)
    kb, yb = k.sum(1), (k * lab[None]).sum(1)
    Ek, Ey = ek.sum(1), (ek * np.abs(lab)[None]).sum(1)
    c = gamma(n, u) if mode == 0 else u + gamma(n, 2.0 ** -53)
    return yb, kb, Ey + c * (np.abs(yb) + Ey), Ek + c * (kb + Ek), k


def node_state64(A, B, D):
    s = A + B
    var = A * B / (s * s * (s + 1.0))
    p = A / s
    st = np.where(p > D["occupied_thresh"], OCCUPIED, np.where(p < D["free_thresh"], FREE, UNKNOWN))
    return np.where(var > D["var_thresh"], UNKNOWN, st).astype(np.uint8), p, var


def state_exempt(A, B, eA, eB, D, u=U):
    """leaves whose state an fp32 evaluation within (eA, eB) may decide either way"""
    with np.errstate(divide="ignore", invalid="ignore"):
        s = A + B
        _, p, var = node_state64(A, B, D)
        room = s - eA - eB
        dp = np.where(room > 0, (B * eA + A * eB) / (s * room), np.inf) + 3.0 * u
        rs = (eA + eB) / s + u
        dv = np.where(rs < 0.5, var * ((1 + eA / A) * (1 + eB / B) * (1 + u) ** 8 / (1 - rs) ** 3 - 1.0), np.inf)
        ex = (np.abs(p - D["occupied_thresh"]) <= dp) | (np.abs(p - D["free_thresh"]) <= dp) | \
             (np.abs(var - D["var_thresh"]) <= dv)
    return ex | ~np.isfinite(dp) | ~np.isfinite(dv)


def scan64(sc, P, mode=0, u=U):
    """the float64 answer to a packed scan (tests/helpers/bgkl_scans.py LScan: pos, rows, train_off, nbr, leaf_off, a0, b0)
    with its bounds:
      A, B, eA, eB     per leaf
      ybar, kbar, ey, ek, gate, gate_out   [leaf, 7]: the sums of every live slot, the float64 gate decision and the pairs
                       left out of the gate comparison; live [leaf, 7] says which slots hold a trained neighbour
      updated, updated_out   per leaf: any gate passed; the decision depends on a pair that is left out
      state, state_out       per leaf (of the updated leaves)
      k                      {(test block, training block): float64 k [leaf, row]}"""
    D = derived(P)
    n = len(sc.pos)
    A, B = sc.a0.astype(np.float64), sc.b0.astype(np.float64)
    eA, eB = np.zeros(n), np.zeros(n)
    out = {k: np.zeros((n, 7)) for k in ("ybar", "kbar", "ey", "ek")}
    gate, gate_out, live = (np.zeros((n, 7), bool) for _ in range(3))
    cache = {}
    for t in range(len(sc.nbr)):
        sl = slice(int(sc.leaf_off[t]), int(sc.leaf_off[t + 1]))
        if sl.start == sl.stop:
            continue
        for b, tb in enumerate(sc.nbr[t]):
            if tb < 0:
                continue
            live[sl, b] = True
            key = (t, int(tb))
            if key not in cache:
                cache[key] = predict64(sc.pos[sl], sc.rows[sc.train_off[tb]:sc.train_off[tb + 1]], P, mode, u)
            yb, kb, ey, ek, _ = cache[key]
            out["ybar"][sl, b], out["kbar"][sl, b], out["ey"][sl, b], out["ek"][sl, b] = yb, kb, ey, ek
            g = kb > GATE
            amb = np.abs(kb - GATE) <= ek
            gate[sl, b], gate_out[sl, b] = g, amb
            dB = (ek + ey) * (1 + u) + u * np.abs(kb - yb)
            A1, B1 = A[sl] + yb, B[sl] + (kb - yb)
            eA1 = (eA[sl] + ey) * (1 + u) + u * np.abs(A1)
            eB1 = (eB[sl] + dB) * (1 + u) + u * np.abs(B1)
            # a pair left out of the gate comparison: the float64 decision stands, the other one is within the bound
            eA1 = np.where(amb, eA1 + np.abs(yb) + ey, eA1)
            eB1 = np.where(amb, eB1 + np.abs(kb - yb) + dB, eB1)
            take = g | amb
            A[sl], B[sl] = np.where(g, A1, A[sl]), np.where(g, B1, B[sl])
            eA[sl], eB[sl] = np.where(take, eA1, eA[sl]), np.where(take, eB1, eB[sl])
    updated = gate.any(1)
    updated_out = ~(gate & ~gate_out).any(1) & gate_out.any(1)
    st, p, var = node_state64(A, B, D)
    return dict(out, k={key: v[4] for key, v in cache.items()}, A=A, B=B, eA=eA, eB=eB, gate=gate, gate_out=gate_out, live=live, updated=updated,
                updated_out=updated_out, state=st, p=p, var=var, state_out=state_exempt(A, B, eA, eB, D, u) | updated_out)


def compare(got, f):
    """alpha / beta / state bytes of an fp32 evaluation (got = (alpha, beta, state)) against scan64's answer f.  Returns the
    list of violations (empty: within the bound everywhere, `updated` and the states equal outside the excluded sets) and
    the largest |got - float64| as a fraction of its bound"""
    a, b, st = (np.asarray(x) for x in got)
    bad = []
    worst = 0.0
    for name, x, x64, e in (("alpha", a, f["A"], f["eA"]), ("beta", b, f["B"], f["eB"])):
        err = np.abs(x.astype(np.float64) - x64)
        over = ~(err <= e)
        if over.any():
            i = int(np.argmax(np.where(over, err - e, -np.inf)))
            bad.append((name, int(over.sum()), i, float(err[i]), float(e[i])))
        nz = e > 0
        if nz.any():
            worst = max(worst, float((err[nz] / e[nz]).max()))
    upd = (st & 0x80) != 0
    keep = ~f["updated_out"]
    if (upd != f["updated"])[keep].any():
        bad.append(("updated", int((upd != f["updated"])[keep].sum())))
    keep = f["updated"] & upd & ~f["state_out"]
    if ((st & 3) != f["state"])[keep].any():
        bad.append(("state", int(((st & 3) != f["state"])[keep].sum())))
    if (st[~upd] != 0).any():
        bad.append(("state byte of a leaf that was not updated", int((st[~upd] != 0).sum())))
    return bad, worst


def compare_sums(ybar, kbar, f):
    """the [leaf, 7] sums of an fp32 evaluation against scan64's, on the live slots; gates outside the excluded set"""
    bad = []
    worst = 0.0
    L = f["live"]
    for name, x, x64, e in (("ybar", ybar, f["ybar"], f["ey"]), ("kbar", kbar, f["kbar"], f["ek"])):
        err = np.abs(np.asarray(x, np.float64) - x64)
        over = L & ~(err <= e)
        if over.any():
            bad.append((name, int(over.sum()), float((err - e)[over].max())))
        nz = L & (e > 0)
        if nz.any():
            worst = max(worst, float((err[nz] / e[nz]).max()))
    g = np.asarray(kbar, np.float32) > np.float32(0.001)
    keep = L & ~f["gate_out"]
    if (g != f["gate"])[keep].any():
        bad.append(("gate", int((g != f["gate"])[keep].sum())))
    return bad, worst


def left_out(f):
    """(share of live (leaf, neighbour) gates left out, share of updated leaves' states left out, their counts)"""
    n_live = int(f["live"].sum())
    n_gate = int((f["gate_out"] & f["live"]).sum())
    n_upd = int(f["updated"].sum())
    n_state = int((f["state_out"] & f["updated"]).sum())
    return n_gate / max(n_live, 1), n_state / max(n_upd, 1), n_gate, n_state
