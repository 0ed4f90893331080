"""Float64 BGK reference for the BGKOctoMap tests (tests/test_bgk_f64_cpu.py, tests/test_bgk_scans_gpu.py).

Written from the reference's formulas, not from oracle/ or la3dm_amd (numpy only, imports neither; node_state64, state_exempt
and gamma are bgkl_f64_ref's: the node is the same formula):
  predict   include/bgkoctomap/bgkinference.h:73-93      ybar = Ks y, kbar = Ks.rowwise().sum(); the distance of x / ell and
                                                         z / ell: d2 = dx^2 + (dy^2 + dz^2), r = sqrt(d2)
  kernel    include/bgkoctomap/bgkinference.h:108-118    k = ((2 + cos(2 pi r)) (1 - r) / 3 + sin(2 pi r) / (2 pi)) sf2 with
                                                         pi = 3.1415926f, k < 0 -> 0
  update    src/bgkoctomap/bgkoctomap.cpp:314-335        for every trained neighbour in ExtendedBlock order: kbar > 0 ?
                                                         update(ybar, kbar); :179-185 is the same loop without the gate
  node      src/bgkoctomap/bgkoctree_node.cpp:36-43      A += ybar, B += kbar - ybar; var > var_thresh: UNKNOWN, else
                                                         p = A / (A + B) against the thresholds
Inputs are the fp32 values the kernels see, widened: points (x, y, z, label), leaf positions (lut[key] + block centre, added
in fp32), ell, sf2, the thresholds and 3.1415926f.  Everything after that is float64.

Sum modes.  0: one node update per trained neighbour (a training block with at least one point) whose kbar > 0.  1: one pair
of sums over all seven neighbours, one gate K > 0, one update A = A + Y, B = B + (K - Y) — what bgk_sum 1 and the
restatement's sum mode 1 (oracle/la3dm_oracle.cpp:1203-1260) do.  Ungated (LA3DM_SCAN_UPDATE_UNGATED): mode 0 runs the
update for every trained neighbour whatever kbar is (a test block without one is not touched, bgkoctomap.cpp:168-181);
mode 1 runs its one update for every leaf, in the restatement's form (:1251-1262) also where no neighbour is trained —
alpha and beta then stay, the leaf counts as updated (the library's contract for bgk_sum 1,
tests/test_bgk_one_launch_gpu.py::test_ungated_update; it differs from the reference in that mark alone).

Error bound of an fp32 evaluation of the same formulas (u = 2^-24, gamma_n = n u / (1 - n u)), worst-case constants, no
assumption about the order of the operations or about fused multiply-adds:
  * distance.  The quotients q = fl(x / ell) carry u |x| / ell each (one rounding per quotient: the kernels' reciprocal plus
    one correction is swept exhaustively to equal the IEEE quotient), so the difference of two of them is off by
    u (|a_i| + |b_i|) / ell on axis i BEFORE it is rounded: this is the cancellation, it scales with the coordinates'
    magnitude X over ell and not with the distance; 2.5 km from the origin at ell = 0.2 it is 1.5e-3 and dominates
    everything else.  As a vector:  E_q = u sqrt(sum_i (|a_i| + |b_i|)^2) / ell  (<= 2 sqrt(3) u X / ell).  The rounded
    difference, three squares, two additions and the root add 4 u r (bgkl_f64_ref), whatever the association:
        E_r = (E_q + 4 u r)(1 + 8 u)
  * kernel.  g(r) = (2 + cos t)(1 - r) / 3 + sin t / (2 pi), t = 2 pi r.  Taylor at the float64 r as in bgkl_f64_ref:
    |g(r') - g(r)| <= |g'(r)| E_r + M2 E_r^2 / 2.  The fp32 evaluation of g at r' (x = |1 - r'|, 1 - r' is exact near 1):
    t = fl(2 r' pi) is off by u t; sine and cosine by that plus 2 u of their own (correctly rounded or not);
    a = fl(fl((2 + c) x) / 3) by x u (2 pi r / 3 + 11 / 3); b = fl(s / 2 pi) by u (r + 1 / pi + 0.16); the sum and the
    product with sf2 by u |g| each:
        e_g(r) = 1.001 u (x (2 pi r / 3 + 11 / 3) + r + 1 / pi + 0.16 + 2 |g|)       (1.5 u at r = 1, 6.2 u at r = 0)
        e_k = sf2 (|g'(r)| E_r + M2 E_r^2 / 2 + e_g(r))
    (BGK-L's flat 12 u would leave a tenth of the unit ball inside the zone where k is below its own bound.)
  * the gate is at 0.  3.1415926f is 3.14159250..., below pi, so sin(2 pi' r) is already -3.0e-7 at r = 1: in float64
    g(1) = -4.8e-8 and g < 0 from r = 0.97768 on (computed here, not assumed: the kernel is NOT slightly positive beyond 1),
    while fp32 evaluations are still positive (7.5e-9 at r = 0.97965) up to the radius sqrt(0.96778184) = 0.98376 from which
    the kernels drop a pair (kHitTBits).  From which radius MUST an fp32 evaluation clamp to 0?  fl g(r')
    <= g(r') + e_g(r'), so from R0 = the last zero of g + e_g on [1, 1.5] (found on a grid of 1e-6 and moved out by 1e-4; g is
    decreasing on [1, 1.5], see bgkl_f64_ref; R0 = 1.0226); beyond 1.5 no e_g is needed: any cosine and sine in [-1, 1] give
    a <= -(r - 1)(1 - 3 u) / 3 <= -0.1666 and b <= 0.1592.  A pair with r - E_r >= R0 is 0 on both sides: k = 0, e_k = 0.
    A leaf out of reach of everything therefore has kbar = 0 EXACTLY and is compared (state byte 0, alpha / beta
    untouched).  Only a gate whose bound is POSITIVE and whose float64 kbar is at most that bound is left out of the gate
    comparison; its update then enters the node's bound in full.  (kbar itself may be 0 there: a leaf whose only points
    lie at 0.9777 ... 0.9838 ell has a float64 sum of exactly 0 and a positive fp32 sum, so a zero with a positive bound
    decides nothing; a zero with a zero bound does.)
  * labels need not be 0 / 1: a term k y is off by |y| e_k + u |y| (k + e_k) (the product's own rounding).
  * sums.  mode 0, a neighbour of N points: an fp32 chain in any order, e = E + gamma_N (S + E).  mode 1: double sums over
    all seven neighbours, e = E + gamma_N(2^-53)(S + E), no rounding to fp32 of their own.
  * updates.  mode 0, per neighbour: eA <- (eA + e_y)(1 + u) + u |A|, eB <- (eB + (e_k + e_y)(1 + u) + u |kbar - ybar|)
    (1 + u) + u |B|.  mode 1, once: A = fl(A + Y): eA = e_Y (1 + u) + u |A|; B = fl(B + (K - Y)): eB = (e_K + e_Y)(1 + u)
    + u |B|.
  * state: as bgkl_f64_ref.state_exempt; a leaf whose float64 p or variance lies within its bound of a threshold is left
    out of the state comparison.
"""
import os
import re

import numpy as np

from bgkl_f64_ref import FREE, OCCUPIED, UNKNOWN, U, gamma, node_state64, state_exempt   # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "la3dm_amd", "csrc")

# config/methods/bgkoctomap.yaml (la3dm_amd.BGK_YAML), restated so that this module imports nothing of the package
BGK_YAML = dict(resolution=0.1, block_depth=3, sf2=1.0, ell=0.2, free_thresh=0.3, occupied_thresh=0.7, var_thresh=100.0,
                prior_A=0.001, prior_B=0.001)
P4 = dict(BGK_YAML, ell=0.4)    # exactly 4 * resolution: the last ell with per-tile descriptors; a point near a tile's middle reaches its 64 leaves
P5 = dict(BGK_YAML, ell=0.5)    # per-tile descriptors off
PI_F = float(np.float32(3.1415926))
UNGATED, LABELS_01, FULL_BLOCKS = 1, 2, 4


def bgk_constants():
    """the sizes the BGK kernels dispatch on, parsed from the header the library is built from"""
    with open(os.path.join(CSRC, "bgk_kernels.h")) as fh:
        src = fh.read()
    c = {k: int(v, 0) for k, v in re.findall(r"constexpr\s+(?:int|uint32_t)\s+(k\w+)\s*=\s*(0x[0-9a-fA-F]+|\d+)u?\s*;", src)}
    names = ("kWave", "kCand5", "kRing5", "kRingR", "kTabSlots", "kRingT", "kHitTBits")
    for k in names:
        assert k in c, k
    out = {k: c[k] for k in names}
    out["hit_t"] = float(np.uint32(out["kHitTBits"]).view(np.float32))
    return out


def count_values(c=None):
    """the point counts per tile the scans must reach: 0, 1, around half the table, the table, the 64-point staging trip,
    the 128 points from which the descriptor is read again"""
    c = c or bgk_constants()
    t, w = c["kTabSlots"], c["kWave"]
    return sorted({0, 1, t // 2 - 1, t // 2, t // 2 + 1, t - 1, t, t + 1, w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1})


def ring_counts(c=None):
    """n all-hit points per tile so that 64 n lands below, at (where the capacity is a multiple of 64) and above each ring"""
    c = c or bgk_constants()
    w = c["kWave"]
    out = set()
    for k in ("kRing5", "kRingR", "kRingT"):
        q = c[k] // w
        out |= {q - 1, q, q + 1} if c[k] % w == 0 else {q, q + 1}
    return sorted(out)


def derived(P):
    """the parameters as the library and the reference hold them (fp32), widened"""
    f = np.float32
    return {k: float(f(P[k])) for k in ("sf2", "ell", "free_thresh", "occupied_thresh", "var_thresh")}


def g64(r):
    t = 2.0 * PI_F * r
    return (2.0 + np.cos(t)) * (1.0 - r) / 3.0 + np.sin(t) / (2.0 * PI_F)


def e_g(r, u=U):
    x = np.abs(1.0 - r)
    return 1.001 * u * (x * (2.0 * PI_F * r / 3.0 + 11.0 / 3.0) + r + 1.0 / PI_F + 0.16 + 2.0 * np.abs(g64(r)))


def zero_radius(u=U):
    """R0 of the module docstring"""
    r = np.linspace(1.0, 1.5, 500001)
    pos = np.nonzero(g64(r) + e_g(r, u) > 0.0)[0]
    assert len(pos) and pos[-1] < len(r) - 1000
    return float(r[pos[-1]]) + 1e-4


R0 = zero_radius()


def pairs64(pos, pts, D, u=U):
    """float64 k [leaf, point] and its bound e_k for leaves at pos and the points of one training block"""
    a = np.asarray(pos, np.float32).astype(np.float64).reshape(-1, 3)
    b = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 4)[:, :3]
    ell = D["ell"]
    d = (b[None, :, :] - a[:, None, :]) / ell
    r = np.sqrt(d[..., 0] ** 2 + (d[..., 1] ** 2 + d[..., 2] ** 2))
    m = np.abs(a)[:, None, :] + np.abs(b)[None, :, :]
    Eq = u * np.sqrt((m * m).sum(-1)) / ell
    Er = (Eq + 4.0 * u * r) * (1.0 + 8.0 * u)
    t = 2.0 * PI_F * r
    g1 = np.abs((2.0 / 3.0) * (np.cos(t) - 1.0) - (2.0 * PI_F / 3.0) * (1.0 - r) * np.sin(t))
    M2 = 2.0 * PI_F / 3.0 + (4.0 * PI_F ** 2 / 3.0) * (np.abs(1.0 - r) + Er)
    k = np.maximum(g64(r) * D["sf2"], 0.0)
    ek = D["sf2"] * (g1 * Er + 0.5 * M2 * Er * Er + e_g(r, u))
    out = r - Er >= R0
    assert not (out & (k > 0)).any()
    return np.where(out, 0.0, k), np.where(out, 0.0, ek), r


def sums64(k, ek, lab, u=U):
    """(Y, K, E_Y, E_K) of one neighbour before the error of the summation itself"""
    al = np.abs(lab)[None]
    return (k * lab[None]).sum(1), k.sum(1), (ek * al + u * al * (k + ek)).sum(1), ek.sum(1), (k * al).sum(1)


def scan64(sc, P, mode=0, ungated=False, u=U, cache=None):
    """the float64 answer to a packed scan (tests/helpers/bgk_scans.py Scan) with its bounds:
      A, B, eA, eB           per leaf
      gate, gate_out, live   [leaf, 7] in mode 0 (one gate per trained neighbour), [leaf, 1] in mode 1 (one gate per leaf
                             with a trained neighbour): the float64 decision and the gates left out of the comparison
      kbar, ek               the same shape: the float64 sums and their bounds
      updated, updated_out, state, p, var, state_out   per leaf
    cache: a dict that keeps the pairs of a scan between calls (both modes use the same ones)"""
    D = derived(P)
    n = len(sc.pos)
    A, B = sc.a0.astype(np.float64), sc.b0.astype(np.float64)
    eA, eB = np.zeros(n), np.zeros(n)
    G = 7 if mode == 0 else 1
    gate, gate_out, live = (np.zeros((n, G), bool) for _ in range(3))
    kbar, ekb = np.zeros((n, G)), np.zeros((n, G))
    cache = {} if cache is None else cache
    for t in range(len(sc.nbr)):
        sl = sc.leaves_of(t)
        if sl.start == sl.stop:
            continue
        nl = sl.stop - sl.start
        Y, K, EY, EK, SY, N = (np.zeros(nl) for _ in range(6))
        for b, tb in enumerate(sc.nbr[t]):
            if tb < 0 or sc.sizes[tb] == 0:
                continue
            key = (t, int(tb))
            if key not in cache:
                cache[key] = pairs64(sc.pos[sl], sc.pts[sc.pts_of(tb)], D, u)
            k, ek, _ = cache[key]
            yb, kb, ey, ekk, sy = sums64(k, ek, sc.pts[sc.pts_of(tb), 3].astype(np.float64), u)
            if mode == 1:
                Y, K, EY, EK, SY, N = Y + yb, K + kb, EY + ey, EK + ekk, SY + sy, N + k.shape[1]
                live[sl, 0] = True
                continue
            c = gamma(k.shape[1], u)
            ey, ekk = ey + c * (sy + ey), ekk + c * (kb + ekk)
            live[sl, b] = True
            kbar[sl, b], ekb[sl, b] = kb, ekk
            g = np.ones(nl, bool) if ungated else kb > 0.0
            amb = np.zeros(nl, bool) if ungated else (ekk > 0.0) & (kb <= ekk)
            gate[sl, b], gate_out[sl, b] = g, amb
            dB = (ekk + ey) * (1 + u) + u * np.abs(kb - yb)
            A1, B1 = A[sl] + yb, B[sl] + (kb - yb)
            eA1 = (eA[sl] + ey) * (1 + u) + u * np.abs(A1)
            eB1 = (eB[sl] + dB) * (1 + u) + u * np.abs(B1)
            eA1 = np.where(amb, eA1 + np.abs(yb) + ey, eA1)
            eB1 = np.where(amb, eB1 + np.abs(kb - yb) + dB, eB1)
            A[sl], B[sl] = np.where(g, A1, A[sl]), np.where(g, B1, B[sl])
            eA[sl], eB[sl] = np.where(g | amb, eA1, eA[sl]), np.where(g | amb, eB1, eB[sl])
        if mode == 1:
            c = gamma(float(N.max()), 2.0 ** -53) if N.max() else 0.0
            EY, EK = EY + c * (SY + EY), EK + c * (K + EK)
            kbar[sl, 0], ekb[sl, 0] = K, EK
            if ungated:
                live[sl, 0] = True
            g = np.ones(nl, bool) if ungated else K > 0.0
            amb = np.zeros(nl, bool) if ungated else (EK > 0.0) & (K <= EK)
            gate[sl, 0], gate_out[sl, 0] = g, amb
            A1, B1 = A[sl] + Y, B[sl] + (K - Y)
            eA1 = EY * (1 + u) + u * np.abs(A1)
            eB1 = (EK + EY) * (1 + u) + u * np.abs(B1)
            eA1 = np.where(amb, eA1 + np.abs(Y) + EY, eA1)
            eB1 = np.where(amb, eB1 + np.abs(K - Y) + EK + EY, eB1)
            A[sl], B[sl] = np.where(g, A1, A[sl]), np.where(g, B1, B[sl])
            eA[sl], eB[sl] = np.where(g | amb, eA1, 0.0), np.where(g | amb, eB1, 0.0)
    updated = gate.any(1)
    updated_out = ~(gate & ~gate_out).any(1) & gate_out.any(1)
    st, p, var = node_state64(A, B, D)
    return dict(A=A, B=B, eA=eA, eB=eB, gate=gate, gate_out=gate_out, live=live, kbar=kbar, ek=ekb, updated=updated,
                updated_out=updated_out, state=st, p=p, var=var, state_out=state_exempt(A, B, eA, eB, D, u) | updated_out)


def compare(got, f):
    """alpha / beta / state bytes of an fp32 evaluation (got = (alpha, beta, state)) against scan64's answer f.  Returns the
    list of violations (empty: within the bound everywhere, `updated` and the states equal outside the excluded sets, the
    state byte of a leaf that was not updated 0) and the largest |got - float64| as a fraction of its bound"""
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


def left_out(f):
    """(share of live gates left out, share of updated leaves' states left out, their counts)"""
    n_live = int(f["live"].sum())
    n_gate = int((f["gate_out"] & f["live"]).sum())
    n_upd = int(f["updated"].sum())
    n_state = int((f["state_out"] & f["updated"]).sum())
    return n_gate / max(n_live, 1), n_state / max(n_upd, 1), n_gate, n_state
