"""Float64 BGK-LV reference for the BGKLVOctoMap tests (tests/test_lv_f64_cpu.py, tests/test_lv_scans_gpu.py).

Written from the reference's formulas, not from oracle/ or la3dm_amd (numpy only, imports neither):
  rows      src/bgklvoctomap/bgklvoctomap.cpp:162-205       the closed box p +- ell (point3f arithmetic: the faces are the
                                                            fp32 values fl(p - ell), fl(p + ell)); a hit in the box adds the
                                                            row (hit, hit) with y = 1; a ray adds one row, its segment, with
                                                            y = 0, if any of its samples is in the box (ray_keys)
  distance  include/bgklvoctomap/bgklvinference.h:100-134   point_to_line_dist: |p - p0| for line_len < 0.0001, else
                                                            c1 = (p - p0).l, c2 = l.l; c1 <= 0: |p - p0|; c2 <= c1: |p - p1|;
                                                            else |p - (p0 + l c1 / c2)|
  kernel    include/bgklvoctomap/bgklvinference.h:143-156   r = min(d / ell, 1), k = ((2 + cos(2 pi r)) (1 - r) / 3 +
                                                            sin(2 pi r) / (2 pi)) sf2 with pi = 3.1415926f, negative values kept
  update    src/bgklvoctomap/bgklvoctomap.cpp:206-238       ybar = sum k y, kbar = sum k over all rows; kbar > 0.001f ? once
  node      src/bgklvoctomap/bgklvoctree_node.cpp:29-77     A += ybar, B += kbar - ybar; W = max(A + B, min_W);
                                                            A > B: p = A / (W - B) + (W - A - B) / 2 / (W - B), else
                                                            p = (W - B - A) / 2 / (W - A); var = A / W (1 - p)^2 +
                                                            (W - A - B) / W (1/2 - p)^2 + B / W p^2; var > var_thresh:
                                                            UNCERTAIN, else p against the two thresholds
Inputs are the fp32 values the kernels see, widened: sample positions, segment end points, voxel positions (lut + block
centre, added in fp32), the box faces, ell, sf2, the thresholds, min_W, 0.001f, 0.0001f and 3.1415926f.  Everything after
that is float64.

Error bound of an fp32 evaluation of the same formulas (u = 2^-24, gamma_n = n u / (1 - n u)), worst-case constants, no
assumption about the order of the operations or about fused multiply-adds.  Distance, r and the kernel are those of
tests/bgkl_f64_ref.py; what differs is marked (LV):
  * distance.  X = largest |coordinate| of the scan.  A hit, a segment shorter than 0.0001 and the two end-point branches
    subtract two inputs: |dd| <= 4 u d.  The projection branch displaces the nearest point by at most 48 u X (the
    cancellation in p - q, numbers of size X):  E_d = (48 X [row is a ray's segment] + 4 d) u.
  * r = min(d / ell, 1) (LV): the division adds u r, the clamp is 1-Lipschitz:  E_r = E_d / ell + u r bounds the clamped r too.
  * kernel.  g(r) = (2 + cos t)(1 - r) / 3 + sin t / (2 pi), t = 2 pi r, g' = (2/3)(cos t - 1) - (2 pi / 3)(1 - r) sin t,
    |g''| <= 2 pi / 3 + (4 pi^2 / 3) |1 - r|.  Taylor at the clamped float64 r, plus less than 12 u for the fp32 evaluation
    of g itself:  e_k = sf2 (|g'(r)| E_r + M2 E_r^2 / 2 + 12 u), M2 = 2 pi / 3 + (4 pi^2 / 3)(|1 - r| + E_r).
    (LV) there is no max(., 0): k may be negative.  3.1415926f lies 1.5e-7 below pi, so sin(2 pi_f) = -3.0e-7 and
    g(1) = -4.8e-8: a row out of reach (d >= ell: a sample in the cubic box whose segment passes the centre beyond ell)
    adds sf2 g(1) = -4.8e-9, not 0.  Both sides clamp such a row to r = 1 exactly once r - E_r >= 1, and then only the
    evaluation of g differs.  The general 12 u would hide the value itself (sf2 12 u = 7e-8), so that evaluation is followed
    step by step: t = 2 pi_f is exact (a doubling), 1 - r is exactly 0 and so is the first term whatever the cosine returns,
    the sine of t is off by at most u absolutely (its own error; |sin| <= 1), and the division, the addition of 0 and the
    product with sf2 add 3 u relatively:  e_k = sf2 (u / (2 pi) + 3 u |g(1)|) = 9.5e-10 there, a fifth of the row.
    (First written with e_k = sf2 12 u out of reach: sound, but then no bound could tell k clamped at 0 from k kept.)
  * sums over the N rows of a voxel (LV: one voxel, all its rows; terms of either sign, so the chain's error is relative to
    S = sum |k|, not to |sum k|), E = sum e_k; ybar likewise over the hit rows (y = 1; a ray's row adds k * 0):
        ordered mode (bgk_sum 0)     an fp32 chain of N terms, any order:          e = E + gamma_N (S + E)
        order-free mode (bgk_sum 1)  a double chain, one rounding to fp32:         e = E + (u + gamma_N(2^-53)) (S + E)
  * gate (LV: one per voxel): kbar > 0.001f.  A voxel whose float64 kbar lies within e of 0.001f is left out of the gate
    comparison; its update then enters the node's bound in full (either decision is allowed).  Whether the box holds any
    sample at all (LA3DM_LV_HAS_INFO) is a comparison of fp32 inputs: exact, nothing is left out.
  * the update A = fl(A + ybar), B = fl(B + fl(kbar - ybar)).  (LV) kbar - ybar is the sum over the rays' rows: the hit
    rows enter both sums with the same fp32 k, so their kernel errors cancel and only the two chains' roundings remain,
    e_f = sum over the rays' rows of e_k + c (S + E) + c (S_y + E_y) with c the chain factor of the mode (e_k + e_y, the
    bound of two unrelated sums, is sound too but lets a hit's 12 u hide what the rays' rows add to beta):
        eA = e_y (1 + u) + u |A|,   eB = (e_f (1 + u) + u |kbar - ybar|)(1 + u) + u |B|
  * node (LV).  s = A + B, W = max(s, min_W).  Two branch points: A > B, and s < min_W; a voxel whose float64 A - B or
    s - min_W lies within eA + eB + 2 u (|A| + |B|) of zero is left out of the state comparison.  Inside a branch:
      s >= min_W: W = s, and p is 1 (A > B) or 0 identically, whatever A and B are: only roundings remain.  fl(A + B) - B
        and fl(A + B) - A are off by at most 2 u s of a denominator >= s / 2, the second term's numerator is at most 2 u s:
        |dp| <= 12 u.
      s < min_W: W = min_W exactly; p = (W + A - B) / (2 (W - B)) or (W - A - B) / (2 (W - A)), denominator >= W.  The
        numerator moves by eA + eB and three roundings of numbers <= 2 W, the denominator by 2 max(eA, eB) and 4 u W, p <= 1:
        |dp| <= (3 (eA + eB) + 10 u W) / (W - 2 (eA + eB) - 4 u W) + 6 u.
      var = sum of three weights in [0, 1] (A / W, (W - A - B) / W, B / W) times three squares in [0, 1].  A weight moves by
        at most (2 eA + 2 eB) / (W - eA - eB) + 3 u — W moves with A and B — a square by 2 |dp| + dp^2 + 3 u, and the
        three products and two additions add 8 u:
        |dvar| <= 3 (2 eA + 2 eB) / (W - eA - eB) + 2 |dp| + dp^2 + 32 u   (the weights sum to 1: the squares' share once).
    A voxel whose float64 p or var lies within that of a threshold is left out of the state comparison.
Hand-built segments keep their length away from the 0.0001 switch (0, 5e-5 or >= 2e-4: asserted by dist64).
"""
import os
import re

import numpy as np

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "la3dm_amd", "csrc")

# config/methods/bgklvoctomap.yaml (la3dm_amd.LV_YAML), restated so that this module imports nothing of the package
LV_YAML = dict(resolution=0.1, block_depth=5, sf2=0.1, ell=0.2, free_thresh=0.3, occupied_thresh=0.7, var_thresh=0.2,
               prior_A=0.001, prior_B=0.001, original_size=True, min_W=0.001)

PI_F = float(np.float32(3.1415926))
GATE = float(np.float32(0.001))
EPSILON = float(np.float32(0.0001))
FREE, OCCUPIED, UNKNOWN, UNCERTAIN, PRUNED = 0, 1, 2, 3, 4
LEAF_UPDATED, HAS_INFO = 0x80, 0x40
CX, CD, CK = 48.0, 4.0, 12.0
MUTANTS = ("no de-duplication", "distance to the sample", "open box", "k clamped at 0", "r not clamped at 1", "gate at 0.0011",
           "W without min_W")
NAMES = ("kLvWaves", "kLvChunk", "kLvGroup", "kLvPlanPerWave", "kLvAddRows", "kLvAddDepth", "kWave")


def lv_constants():
    """the sizes the BGK-LV kernels dispatch on, parsed from the headers the library is built from"""
    src = ""
    for f in ("bgk_kernels.h", "lv_kernels.h"):
        with open(os.path.join(CSRC, f)) as fh:
            src += fh.read()
    c = {k: int(v) for k, v in re.findall(r"constexpr\s+(?:int|uint32_t)\s+(k\w+)\s*=\s*(\d+)\s*;", src)}
    for k in NAMES:
        assert k in c, k
    return {k: c[k] for k in NAMES}


def stream_sizes(c=None):
    """stream lengths of a cube: chunk - 1, chunk, chunk + 1, two chunks, two chunks and a sample, three and five"""
    ch = (c or lv_constants())["kLvChunk"]
    return [ch - 1, ch, ch + 1, 2 * ch, 2 * ch + 1, 3 * ch + 5]


def kept_sizes(c=None):
    """kept candidates of a staging pass: round the 16-row padding of the dense add and the 64-candidate round"""
    w = (c or lv_constants())["kWave"]
    return [1, 15, 16, 17, w - 1, w, w + 1, 2 * w + 1]


def split_row_sizes(c=None):
    """rows of a split cube's sub-task: round one tile of the ordered add and the tiles in flight"""
    c = c or lv_constants()
    t, d = c["kLvAddRows"], c["kLvAddDepth"]
    return [t - 1, t, t + 1, d * t, d * t + 1]


def derived(P):
    """the parameters as the library and the reference hold them (fp32), widened"""
    f = np.float32
    return {k: float(f(P[k])) for k in ("sf2", "ell", "free_thresh", "occupied_thresh", "var_thresh", "min_W")}


def gamma(n, u=U):
    return n * u / (1.0 - n * u)


def dist64(p, a, b):
    """point_to_line_dist of points p [m, 3] against segments a -> b [m, 3], pairwise, in float64; which are not degenerate"""
    lv = b - a
    ln = np.sqrt((lv * lv).sum(-1))
    assert not ((ln > 7e-5) & (ln < 1.5e-4)).any(), "a segment too close to the 0.0001 degeneracy switch"
    beam = ~(ln < EPSILON)
    v = p - a
    c1 = (v * lv).sum(-1)
    c2 = (lv * lv).sum(-1)
    t = np.where(c1 <= 0.0, 0.0, np.where(c2 <= c1, 1.0, c1 / np.where(c2 > 0.0, c2, 1.0)))
    t = np.where(beam, t, 0.0)
    q = a + lv * t[:, None]
    return np.sqrt(((p - q) ** 2).sum(-1)), beam, t


def g64(r):
    t = 2.0 * PI_F * r
    return (2.0 + np.cos(t)) * (1.0 - r) / 3.0 + np.sin(t) / (2.0 * PI_F)


def kernel_bound(d, beam, X, D, u=U):
    """e_k of the module docstring for distances d"""
    r = d / D["ell"]
    Ed = (CX * X * beam.astype(np.float64) + CD * d) * u
    Er = Ed / D["ell"] + u * r
    rc = np.minimum(r, 1.0)
    t = 2.0 * PI_F * rc
    g1 = np.abs((2.0 / 3.0) * (np.cos(t) - 1.0) - (2.0 * PI_F / 3.0) * (1.0 - rc) * np.sin(t))
    M2 = 2.0 * PI_F / 3.0 + (4.0 * PI_F ** 2 / 3.0) * (np.abs(1.0 - rc) + Er)
    e = D["sf2"] * (g1 * Er + 0.5 * M2 * Er * Er + CK * u)
    far = D["sf2"] * (u / (2.0 * PI_F) + 3.0 * u * abs(float(g64(1.0))))
    return np.where(r - Er >= 1.0, far, e)


def node64(A, B, D, no_min_w=False):
    """get_prob, get_var and the state of update()"""
    with np.errstate(divide="ignore", invalid="ignore"):
        s = A + B
        W = s if no_min_w else np.where(s < D["min_W"], D["min_W"], s)
        p = np.where(A > B, A / (W - B) + (W - A - B) * 0.5 / (W - B), 0.5 * (W - B - A) / (W - A))
        var = A / W * (1 - p) ** 2 + (W - A - B) / W * (0.5 - p) ** 2 + B / W * p ** 2
    st = np.where(p > D["occupied_thresh"], OCCUPIED, np.where(p < D["free_thresh"], FREE, UNKNOWN))
    return np.where(var > D["var_thresh"], UNCERTAIN, st).astype(np.uint8), p, var


def state_exempt(A, B, eA, eB, D, u=U):
    """voxels whose state an fp32 evaluation within (eA, eB) may decide either way"""
    with np.errstate(divide="ignore", invalid="ignore"):
        _, p, var = node64(A, B, D)
        s = A + B
        W = np.maximum(s, D["min_W"])
        e = eA + eB
        slack = e + 2.0 * u * (np.abs(A) + np.abs(B))
        branch = (np.abs(A - B) <= slack) | (np.abs(s - D["min_W"]) <= slack)
        room = W - 2.0 * e - 4.0 * u * W
        dp = np.where(s >= D["min_W"], 12.0 * u, np.where(room > 0, (3.0 * e + 10.0 * u * W) / room + 6.0 * u, np.inf))
        dv = np.where(W - e > 0, 6.0 * e / (W - e), np.inf) + 2.0 * dp + dp * dp + 32.0 * u
        ex = (np.abs(p - D["occupied_thresh"]) <= dp) | (np.abs(p - D["free_thresh"]) <= dp) | (np.abs(var - D["var_thresh"]) <= dv)
    return ex | branch | ~np.isfinite(dp) | ~np.isfinite(dv) | ~np.isfinite(p) | ~np.isfinite(var)


def _in_box(lo, hi, S, open_box):
    if open_box:
        return ((lo[:, None, :] < S[None]) & (S[None] < hi[:, None, :])).all(-1)
    return ((lo[:, None, :] <= S[None]) & (S[None] <= hi[:, None, :])).all(-1)


def scan64(sc, P, mode=0, u=U, mutant=None):
    """the float64 answer to a packed scan (tests/helpers/lv_scans.py LvScan: pos, active, a0, b0, samples, rays) with its
    bounds, per node of the finest layer:
      A, B, eA, eB, ybar, kbar, ey, ek, rows (how many)
      info                  the box of an active voxel holds a sample (exact)
      gate, gate_out        the float64 gate decision (with info), and the voxels left out of the gate comparison
      updated, updated_out  the same two, as the LA3DM_LEAF_UPDATED bit sees them
      state, p, var, state_out   of the updated voxels
      branches              rays' rows per branch of point_to_line_dist: short (< 0.0001), start (c1 <= 0), end (c2 <= c1), projection
      row_hit, row_ray      per sample / per ray: it is a row of some voxel
      seen_hit, seen_ray    per sample / per ray: some voxel where its own k exceeds twice that voxel's kbar bound
    mutant: one of MUTANTS, a deliberately wrong reading of the reference"""
    assert mutant is None or mutant in MUTANTS
    D = derived(P)
    f32 = np.float32
    pos32 = np.asarray(sc.pos, f32).reshape(-1, 3)
    pos = pos32.astype(np.float64)
    ell32 = f32(P["ell"])
    lo, hi = (pos32 - ell32).astype(np.float64), (pos32 + ell32).astype(np.float64)      # fp32 faces
    smp = np.asarray(sc.samples, f32).reshape(-1, 4)
    S = smp[:, :3].astype(np.float64)
    ray = smp[:, 3].astype(np.int64)
    rays = np.asarray(sc.rays, f32).reshape(-1, 6).astype(np.float64)
    n = len(pos)
    X = max(float(np.abs(pos).max()), float(np.abs(S).max()) if len(S) else 0.0, float(np.abs(rays).max()) if len(rays) else 0.0)
    act = np.nonzero(np.asarray(sc.active, bool))[0]
    # (voxel, row) pairs, voxel-major, ascending sample index inside a voxel
    vs, ss = [], []
    for c0 in range(0, len(act), 512):
        v = act[c0:c0 + 512]
        near = np.nonzero(((S >= lo[v].min(0)) & (S <= hi[v].max(0))).all(1))[0]
        if len(near) == 0:
            continue
        vi, si = np.nonzero(_in_box(lo[v], hi[v], S[near], mutant == "open box"))
        vs.append(v[vi])
        ss.append(near[si])
    vs = np.concatenate(vs) if vs else np.zeros(0, np.int64)
    ss = np.concatenate(ss) if ss else np.zeros(0, np.int64)
    info = np.zeros(n, bool)
    info[vs] = True
    is_ray = ray[ss] >= 0
    hv, hs = vs[~is_ray], ss[~is_ray]
    rv, rs, rr = vs[is_ray], ss[is_ray], ray[ss[is_ray]]
    if mutant != "no de-duplication" and len(rv):
        _, first = np.unique(rv * (len(rays) + 1) + rr, return_index=True)      # the lowest-index sample of (voxel, ray)
        rv, rs, rr = rv[first], rs[first], rr[first]
    pv = np.concatenate([hv, rv])
    pa = np.concatenate([S[hs], S[rs] if mutant == "distance to the sample" else rays[rr, 0:3]])
    pb = np.concatenate([S[hs], S[rs] if mutant == "distance to the sample" else rays[rr, 3:6]])
    y = np.concatenate([np.ones(len(hv)), np.zeros(len(rv))])
    d, beam, tt = dist64(pos[pv], pa, pb)
    is_seg = y == 0
    branches = dict(short=int((is_seg & ~beam).sum()), start=int((is_seg & beam & (tt == 0.0)).sum()),
                    end=int((is_seg & beam & (tt == 1.0)).sum()), projection=int((is_seg & beam & (tt > 0.0) & (tt < 1.0)).sum()))
    r = d / D["ell"]
    k = D["sf2"] * g64(r if mutant == "r not clamped at 1" else np.minimum(r, 1.0))
    if mutant == "k clamped at 0":
        k = np.maximum(k, 0.0)
    e = kernel_bound(d, beam, X, D, u)

    def total(w):
        return np.bincount(pv, weights=w, minlength=n)

    N = total(np.ones(len(pv)))
    kb, yb = total(k), total(k * y)
    Sk, Sy, Ek, Ey = total(np.abs(k)), total(np.abs(k) * y), total(e), total(e * y)
    c = gamma(N, u) if mode == 0 else np.where(N > 0, u + gamma(N, 2.0 ** -53), 0.0)
    ek, ey = Ek + c * (Sk + Ek), Ey + c * (Sy + Ey)
    ef = (Ek - Ey) + c * (Sk + Ek) + c * (Sy + Ey)                   # of kbar - ybar: the hit rows' k cancel
    gate_at = float(f32(0.0011)) if mutant == "gate at 0.0011" else GATE
    gate = info & (kb > gate_at)
    amb = info & (np.abs(kb - GATE) <= ek)
    A0, B0 = np.asarray(sc.a0, f32).astype(np.float64), np.asarray(sc.b0, f32).astype(np.float64)
    A1, B1 = A0 + yb, B0 + (kb - yb)
    dB = ef * (1 + u) + u * np.abs(kb - yb)
    eA1 = ey * (1 + u) + u * np.abs(A1)
    eB1 = dB * (1 + u) + u * np.abs(B1)
    eA1 = np.where(amb, eA1 + np.abs(yb) + ey, eA1)
    eB1 = np.where(amb, eB1 + np.abs(kb - yb) + dB, eB1)
    A, B = np.where(gate, A1, A0), np.where(gate, B1, B0)
    eA, eB = np.where(gate | amb, eA1, 0.0), np.where(gate | amb, eB1, 0.0)
    st, p, var = node64(A, B, D, mutant == "W without min_W")
    seen = k > 2.0 * ek[pv]
    seen_hit, seen_ray = np.zeros(len(S), bool), np.zeros(len(rays), bool)
    seen_hit[hs[seen[:len(hv)]]] = True
    seen_ray[rr[seen[len(hv):]]] = True
    row_hit, row_ray = np.zeros(len(S), bool), np.zeros(len(rays), bool)
    row_hit[hs] = True
    row_ray[rr] = True
    return dict(A=A, B=B, eA=eA, eB=eB, ybar=yb, kbar=kb, ey=ey, ek=ek, rows=N.astype(np.int64), info=info, gate=gate, gate_out=amb,
                updated=gate, updated_out=amb, state=st, p=p, var=var, state_out=state_exempt(A, B, eA, eB, D, u) | amb,
                branches=branches, seen_hit=seen_hit, seen_ray=seen_ray, row_hit=row_hit, row_ray=row_ray, active=np.asarray(sc.active, bool).copy())


def compare(got, f):
    """alpha / beta / state bytes of an fp32 evaluation (got = (alpha, beta, state)) against scan64's answer f.  Returns the
    list of violations (empty: alpha and beta within the bound everywhere, LA3DM_LV_HAS_INFO equal everywhere,
    LA3DM_LEAF_UPDATED and the states equal outside the excluded sets, nothing else in a byte) and the largest
    |got - float64| as a fraction of its bound"""
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
    if (((st & HAS_INFO) != 0) != f["info"]).any():
        bad.append(("has_info", int((((st & HAS_INFO) != 0) != f["info"]).sum())))
    upd = (st & LEAF_UPDATED) != 0
    keep = ~f["updated_out"]
    if (upd != f["updated"])[keep].any():
        bad.append(("updated", int((upd != f["updated"])[keep].sum())))
    keep = f["updated"] & upd & ~f["state_out"]
    if ((st & 7) != f["state"])[keep].any():
        bad.append(("state", int(((st & 7) != f["state"])[keep].sum())))
    if ((st[~upd] & ~np.uint8(HAS_INFO)) != 0).any():
        bad.append(("state bits of a voxel that was not updated", int(((st[~upd] & ~np.uint8(HAS_INFO)) != 0).sum())))
    if (st[~f["active"]] != 0).any():
        bad.append(("state byte of a node that is no base-resolution leaf", int((st[~f["active"]] != 0).sum())))
    return bad, worst


def left_out(f):
    """(share of the voxels with a sample in the box whose gate is left out, share of the updated voxels whose state is left
    out, their counts)"""
    n_info = int(f["info"].sum())
    n_gate = int((f["gate_out"] & f["info"]).sum())
    n_upd = int(f["updated"].sum())
    n_state = int((f["state_out"] & f["updated"]).sum())
    return n_gate / max(n_info, 1), n_state / max(n_upd, 1), n_gate, n_state
