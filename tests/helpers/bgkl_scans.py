"""Hand-built BGK-L scans for tests/test_bgkl_f64_cpu.py and tests/test_bgkl_scans_gpu.py: a packer for la3dm_bgk_scan with
rows of 8 floats, the scans (a) to (g) of the GPU test's docstring, what the CPU restatement answers to them
(oracle.l_predict per (test block, neighbour), the kbar > 0.001f gate in fp32, orc_node_update in ExtendedBlock order) and the
classes a scan hits, computed from the constants parsed out of the kernel headers.

Every row carries the kind it was built as:
  H  a hit (degenerate segment of length 0 or 5e-5, label 1) within a quarter of ell of a leaf                  near
  B  a beam (label 0) through a point within a quarter of ell of a leaf                                         near
  I  a beam that passes the users' leaves just inside ell (0.97 ell from the outermost leaf along a direction)
  O  the same just outside (1.03 ell)
  F  a beam or a hit several ell away
  W  a weak hit, 0.7 ell from the nearest leaf
The kernels do not look at where a training block is: its rows are placed round the leaves of the test blocks that use it.
Test blocks stand three block sizes apart, so the rows aimed at one user are out of reach of the others."""
import ctypes as C

import numpy as np

import bgkl_f64_ref as R

DIRS = np.float64([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])   # ExtendedBlock order
BASE = [(8 ** d - 1) // 7 for d in range(8)]
NEAR = ("H", "B")
# alpha, beta of a leaf before the scan: the prior of a new node, and what earlier scans left on either side
PRIORS = np.float32([(0.001, 0.001)] * 4 + [(0.5, 0.001), (0.001, 0.5), (50, 0.001), (0.001, 50), (5000, 0.001), (0.001, 5000),
                                            (0.5, 0.5), (50, 50)])


class LScan:
    """a la3dm_bgk_scan for la3dm_bgkl_scan_* built from numpy arrays"""

    def __init__(self, depth):
        self.depth, self.blocks, self.tests = depth, [], []

    def block(self, rows, kinds):
        rows = np.asarray(rows, np.float32).reshape(-1, 8)
        assert len(rows) == len(kinds)
        self.blocks.append((rows, np.asarray(list(kinds), "U1")))
        return len(self.blocks) - 1

    def test(self, centre, keys, nbr, a0, b0):
        self.tests.append(dict(centre=np.asarray(centre, np.float32), keys=np.asarray(keys, np.uint32), nbr=list(nbr),
                               a0=np.asarray(a0, np.float32), b0=np.asarray(b0, np.float32)))

    def pack(self, lut):
        n = np.array([len(b[0]) for b in self.blocks], np.int64)
        self.lut = lut
        self.sizes = n
        self.train_off = np.concatenate([[0], np.cumsum(n)]).astype(np.uint32)
        self.rows = np.ascontiguousarray(np.concatenate([b[0] for b in self.blocks] + [np.zeros((0, 8), np.float32)]))
        self.kinds = np.concatenate([b[1] for b in self.blocks] + [np.zeros(0, "U1")])
        self.nbr = np.array([t["nbr"] for t in self.tests], np.int32).reshape(-1, 7)
        self.centre = np.array([t["centre"] for t in self.tests], np.float32).reshape(-1, 3)
        self.leaf_off = np.concatenate([[0], np.cumsum([len(t["keys"]) for t in self.tests])]).astype(np.uint32)
        self.keys = np.concatenate([t["keys"] for t in self.tests]).astype(np.uint32)
        self.a0 = np.concatenate([t["a0"] for t in self.tests]).astype(np.float32)
        self.b0 = np.concatenate([t["b0"] for t in self.tests]).astype(np.float32)
        ctr = np.repeat(self.centre, np.diff(self.leaf_off.astype(np.int64)), axis=0)
        self.pos = leaf_pos(lut, self.keys, ctr)
        return self

    def leaves_of(self, t):
        return slice(int(self.leaf_off[t]), int(self.leaf_off[t + 1]))

    def rows_of(self, b):
        return slice(int(self.train_off[b]), int(self.train_off[b + 1]))

    def tiles(self, wave):
        """(test block, first leaf, leaves, rows of its seven neighbours) of every tile that holds leaves"""
        out = []
        for t in range(len(self.tests)):
            l0, l1 = int(self.leaf_off[t]), int(self.leaf_off[t + 1])
            for s in range(l0, l1, wave):
                out.append((t, s, min(wave, l1 - s), [int(self.sizes[b]) if b >= 0 else 0 for b in self.nbr[t]]))
        return out

    def rebuilt(self, blocks=None, pos_roll=0):
        """a copy with other training blocks, or with the leaf positions of every test block rotated by one lane"""
        sc = LScan(self.depth)
        sc.blocks = list(self.blocks if blocks is None else blocks)
        sc.tests = self.tests
        sc.pack(self.lut)
        if pos_roll:
            for t in range(len(sc.tests)):
                sl = sc.leaves_of(t)
                sc.pos[sl] = np.roll(sc.pos[sl], pos_roll, axis=0)
        return sc


def leaf_pos(lut, keys, centre):
    """Block::get_loc: lut[key] + centre in fp32"""
    keys = np.asarray(keys, np.uint32)
    idx = np.array([BASE[k >> 16] for k in keys], np.int64) + (keys & 0xFFFF).astype(np.int64)
    return (lut[idx].reshape(-1, 3) + np.asarray(centre, np.float32)).astype(np.float32)


def finest(depth):
    d = depth - 1
    return ((d << 16) | np.arange(8 ** d, dtype=np.uint32)).astype(np.uint32)


def pruned_keys(depth):
    """a leaf list with coarser-level keys mixed in"""
    if depth == 2:
        return np.uint32([0])                                            # the whole block pruned into its root
    if depth == 3:
        return np.concatenate([(1 << 16) | np.arange(3), (2 << 16) | np.arange(24, 64)]).astype(np.uint32)
    return np.concatenate([(1 << 16) | np.arange(3), (2 << 16) | np.arange(24, 32), (3 << 16) | np.arange(256, 512)]).astype(np.uint32)


def _unit(rng, n=None):
    v = rng.normal(size=(3,) if n is None else (n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _perp(rng, w):
    e = np.cross(w, _unit(rng))
    return e / np.linalg.norm(e)


def hit_row(p, i=0):
    """hits alternate between a segment of length 0 and one of 5e-5 (both degenerate for point_to_line_dist)"""
    q = np.array(p, np.float64)
    if i % 2:
        q = q + np.float64([5e-5, 0, 0])
    return np.concatenate([p, q, [1.0, 0.0]])


def beam_row(a, b):
    return np.concatenate([a, b, [0.0, 0.0]])


def graze_row(rng, targets, w, dist):
    """a beam perpendicular to w whose foot lies `dist` beyond the outermost target along w: every target is at least dist away"""
    t = targets[int(np.argmax(targets @ w))]
    foot, e = t + w * dist, _perp(rng, w)
    return beam_row(foot - e * rng.uniform(0.5, 2.0), foot + e * rng.uniform(0.5, 2.0))


def make_rows(rng, n, targets, ell, mix=(0.35, 0.25, 0.1, 0.1, 0.2)):
    """n rows round the leaves `targets` (float64 [m, 3]); mix = shares of H, B, I, O, F"""
    kinds = list("HBIOF"[:min(n, 5)]) + list(rng.choice(list("HBIOF"), max(n - 5, 0), p=mix))
    rng.shuffle(kinds)
    rows = []
    for i, k in enumerate(kinds):
        t = targets[int(rng.integers(len(targets)))]
        if k == "H":
            rows.append(hit_row(t + _unit(rng) * rng.uniform(0, 0.25 * ell), i))
        elif k == "B":
            p, d = t + _unit(rng) * rng.uniform(0, 0.25 * ell), _unit(rng)
            rows.append(beam_row(p - d * rng.uniform(0.5, 2.0), p + d * rng.uniform(0.5, 2.0)))
        elif k == "I":
            rows.append(graze_row(rng, targets, _unit(rng), 0.97 * ell))
        elif k == "O":
            rows.append(graze_row(rng, targets, _unit(rng), 1.03 * ell))
        elif i % 3:
            rows.append(graze_row(rng, targets, _unit(rng), rng.uniform(2.0, 6.0) * ell))
        else:
            w = _unit(rng)
            rows.append(hit_row(targets[int(np.argmax(targets @ w))] + w * rng.uniform(2.0, 6.0) * ell, i))
    return np.float32(rows).reshape(-1, 8), kinds


def priors(rng, n, choice=None):
    p = PRIORS[rng.integers(len(PRIORS), size=n)] if choice is None else np.float32(choice)[np.arange(n) % len(choice)]
    return p[:, 0].copy(), p[:, 1].copy()


E = "empty"
# scan (a)/(b): the ten row counts of R.row_sizes by index, each used by two or three test blocks in different slots
NBR_TABLE = [[0, 3, -1, 6, 9, -1, E],          # a -1 between live slots, an empty training block
             [-1, 1, 4, 7, -1, 9, -1],         # no self entry
             [2, 5, 8, -1, 0, -1, 3],
             [6, -1, 1, 4, E, 7, 2],           # one leaf: bounding sphere of radius 0
             [5, 8, -1, -1, -1, -1, 9],        # pruned keys
             [-1] * 7,                         # no neighbour at all: state 0, alpha and beta untouched
             [0, 1, 2, 3, 4, 5, 6]]            # no leaves
LEAVES = {2: [8, 5, 7, 1, "pruned", 3, 0], 3: [64, 37, 63, 1, "pruned", 20, 0], 4: [512, 65, 37, 1, "pruned", 20, 0]}
C0 = np.float64([0.2, -0.2, 0.6])


def _keys(rng, depth, nl):
    if nl == "pruned":
        return pruned_keys(depth)
    return np.sort(rng.choice(finest(depth), nl, replace=False)).astype(np.uint32)


def rows_scan(depth, P, lut, consts, shift=(0.0, 0.0, 0.0)):
    """(a), (b), (f) and, at ell = 0.5 and depth 3, (c)"""
    rng = np.random.default_rng(1000 * depth + int(100 * P["ell"]))
    ell, bs = float(np.float32(P["ell"])), 0.1 * 2 ** (depth - 1)
    sizes = R.row_sizes(consts)
    tests = []
    for t, (nb, nl) in enumerate(zip(NBR_TABLE, LEAVES[depth])):
        tests.append(dict(centre=np.float32(C0 + np.float64(shift) + np.float64([3 * bs * t, 0, 0])), keys=_keys(rng, depth, nl),
                          nbr=[len(sizes) if b == E else b for b in nb]))
    ring = []
    if depth == 3 and ell == 0.5:
        # (c) the hit ring: 5, 6, 7 and 64 hits next to the middle of a 37-leaf and of a 64-leaf tile — every row reaches every
        # leaf, the ring flushes with a remainder (37 leaves) and without one (64 leaves)
        c = C0 + np.float64(shift) + np.float64([0, 3 * bs, 0])
        n0 = len(sizes) + 1
        tests.append(dict(centre=np.float32(c), keys=_keys(rng, 3, 37), nbr=[n0, n0 + 1, n0 + 2, n0 + 3, -1, -1, -1]))
        tests.append(dict(centre=np.float32(c + [0.1, 0, 0]), keys=finest(3), nbr=[n0 + 3, -1, n0 + 2, n0 + 1, n0, -1, -1]))
        ring = [(m, c + [0.05, 0, 0]) for m in (5, 6, 7, consts["kWave"])]
    # a test block of new nodes with one neighbour of weak hits, 0.7 ell beyond the outermost leaf along an axis: that leaf's
    # update (k = 0.018 sf2) passes the gate and leaves a variance above var_thresh with p = 0.73 — UNKNOWN by the variance rule
    weak = len(sizes) + 1 + len(ring)
    tests.append(dict(centre=np.float32(C0 + np.float64(shift) + np.float64([0, -3 * bs, 0])), keys=_keys(rng, depth, LEAVES[depth][5]),
                      nbr=[-1, -1, -1, weak, -1, -1, -1], new=True))
    sc = LScan(depth)
    pos = [leaf_pos(lut, t["keys"], t["centre"]).astype(np.float64) for t in tests]
    for b, N in enumerate(sizes):
        users = [pos[t] for t in range(len(tests)) if b in tests[t]["nbr"] and len(pos[t])]
        sc.block(*make_rows(rng, N, np.concatenate(users), ell))
    sc.block(np.zeros((0, 8)), [])
    for m, mid in ring:
        sc.block([hit_row(mid + _unit(rng) * rng.uniform(0, 0.05), i) for i in range(m)], "H" * m)
    sc.block([hit_row(pos[-1][int(np.argmax(pos[-1] @ w))] + 0.7 * ell * w) for w in DIRS[1:]], "W" * 6)
    for t in tests:
        sc.test(t["centre"], t["keys"], t["nbr"], *priors(rng, len(t["keys"]), [(0.001, 0.001)] if t.get("new") else None))
    return sc.pack(lut)


def tile_sphere(pos):
    """bounding sphere of a tile's leaves in float64: centre of their box, radius to the farthest one"""
    p = np.asarray(pos, np.float64)
    c = 0.5 * (p.min(0) + p.max(0))
    return c, float(np.sqrt(((p - c) ** 2).sum(1)).max())


def cull_scan(P, lut, shift=(0.0, 0.0, 0.0), delta=0.02):
    """(d): one 64-leaf tile; slot 0 hits only, slot 1 a hit on every leaf and two crossing beams, slot 3 beams at the
    bounding sphere's radius + ell - delta, slot 4 the same beams at + delta, slot 6 rows several ell away.  Most beams
    stand over a face or an edge of the tile (inside the sphere's reach, out of every leaf's), two over a corner (they reach
    that corner's leaf).  The leaves carry 50 on one side, so that no state sits near a threshold."""
    rng = np.random.default_rng(77)
    ell = float(np.float32(P["ell"]))
    centre = np.float32(C0 + np.float64(shift))
    keys = finest(3)
    pos = leaf_pos(lut, keys, centre).astype(np.float64)
    c, rad = tile_sphere(pos)
    ws = [np.float64(w) / np.linalg.norm(w) for w in
          ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [1, 0, -1], [0, -1, 1], [-1, -1, 0])]
    corner = [np.float64(w) / np.sqrt(3.0) for w in ([1, 1, 1], [-1, 1, -1])]
    dirs = [ws[i % len(ws)] for i in range(68)] + corner
    es = [_perp(rng, w) for w in dirs]
    lens = rng.uniform(0.5, 2.0, (len(dirs), 2))

    def shell(d):
        return [beam_row(c + w * d - e * l[0], c + w * d + e * l[1]) for w, e, l in zip(dirs, es, lens)]

    sc = LScan(3)
    # (hits of length 0 only: 5e-5 is below the spacing of fp32 at the translated scan's coordinates)
    sc.block([hit_row(pos[i] + _unit(rng) * 0.02) for i in rng.choice(64, 8, replace=False)], "H" * 8)
    cross = [beam_row(pos[i] - d * 1.5, pos[i] + d * 1.2) for i, d in ((5, _unit(rng)), (40, _unit(rng)))]
    sc.block([hit_row(p, 0) for p in pos] + cross, "H" * 64 + "BB")
    sc.block(shell(rad + ell - delta), "I" * len(dirs))
    sc.block(shell(rad + ell + delta), "O" * len(dirs))
    far = [graze_row(rng, pos, _unit(rng), rng.uniform(2.0, 6.0) * ell) for _ in range(66)]
    sc.block(far, "F" * len(far))
    sc.test(centre, keys, [0, 1, -1, 2, 3, -1, 4], *priors(rng, 64, [(50, 0.001), (0.001, 50)]))
    return sc.pack(lut)


def nonfinite_scan(P, lut):
    """(g): the middle one of three neighbours holds a row with a NaN coordinate and a hit at 3e19 m (its squared distance
    overflows) among 70 rows: kbar of that neighbour is NaN at every leaf, the gate rejects it; the other two stand"""
    rng = np.random.default_rng(99)
    ell = float(np.float32(P["ell"]))
    centre, keys = np.float32(C0), finest(3)
    pos = leaf_pos(lut, keys, centre).astype(np.float64)
    sc = LScan(3)
    sc.block(*make_rows(rng, 40, pos, ell))
    bad, kinds = make_rows(rng, 70, pos, ell)
    bad[3, 1] = np.nan
    bad[66] = np.float32([3e19, 0, 0, 3e19, 0, 0, 1, 0])
    sc.block(bad, kinds)
    sc.block(*make_rows(rng, 66, pos, ell))
    sc.test(centre, keys, [0, 1, -1, 2, -1, -1, -1], *priors(rng, 64))
    return sc.pack(lut)


def widened(sc, n_blocks):
    """(e): the scan with one-leaf test blocks without neighbours appended until it holds n_blocks test blocks"""
    w = LScan(sc.depth)
    w.blocks = sc.blocks
    w.tests = list(sc.tests)
    key = finest(sc.depth)[:1]
    for i in range(len(sc.tests), n_blocks):
        w.test(np.float32([50.0 + 0.1 * i, 7.0, -3.0]), key, [-1] * 7, [0.001], [0.001])
    return w.pack(sc.lut)


def split_totals(sc, consts, threshold):
    """(tiles split, items, tiles with leaves) at bgkl_split_rows = threshold (bgkl_split_mark)"""
    it = consts["kLItemRows"]
    tiles = sc.tiles(consts["kWave"])
    if threshold < 0:
        return 0, 0, len(tiles)
    split = [c for _, _, _, c in tiles if sum(c) > threshold]
    return len(split), sum((x + it - 1) // it for c in split for x in c), len(tiles)


def mid_threshold(sc, consts):
    """a bgkl_split_rows between the scan's tile totals: split and unsplit tiles share a launch"""
    tot = sorted({sum(c) for _, _, _, c in sc.tiles(consts["kWave"]) if sum(c)})
    return tot[len(tot) // 2 - 1] if len(tot) > 1 else None


def ring_flushes(sc, P, consts):
    """remainders left at the front of the hit ring (bgkl_rows_sum: flush at tail > kLRing - kWave, tail & (kWave - 1) rows
    stay) over every (tile, neighbour) of the scan, from the float64 distances"""
    ell, w, ring = float(np.float32(P["ell"])), consts["kWave"], consts["kLRing"]
    rems = set()
    for t, s, nl, _ in sc.tiles(w):
        for b in sc.nbr[t]:
            if b < 0 or sc.sizes[b] == 0:
                continue
            d, _ = R.dist64(sc.pos[s:s + nl], sc.rows[sc.rows_of(b)])
            tail = 0
            for cnt in (d < ell).sum(0):
                tail += int(cnt)
                if tail > ring - w:
                    rems.add(tail & (w - 1))
                    tail &= w - 1
    return rems


def classes(sc, consts):
    """what the scan hits, as a set of names (module docstring of tests/test_bgkl_scans_gpu.py)"""
    w, it = consts["kWave"], consts["kLItemRows"]
    out = set()
    used = {int(b) for t in range(len(sc.tests)) if sc.leaf_off[t] < sc.leaf_off[t + 1] for b in sc.nbr[t] if b >= 0}
    for b in used:
        n = int(sc.sizes[b])
        for name, t in (("trip", w), ("item", it)):
            for d in (-1, 0, 1):
                if n == t + d:
                    out.add(f"{name}{d:+d}")
        if n == 2 * it + 1:
            out.add("two items and a row")
        if n and (n + it - 1) // it in (7, 8, 9):
            out.add(f"{(n + it - 1) // it} items")
        if n == 0:
            out.add("empty training block")
    nl = np.diff(sc.leaf_off.astype(np.int64))
    for t in range(len(sc.tests)):
        live = [b >= 0 for b in sc.nbr[t]]
        out.add(f"{int(nl[t])} leaves")
        if nl[t] > w and nl[t] % w == 1:
            out.add("last tile holds one leaf")
        if nl[t] and not any(live):
            out.add("no neighbour")
        if nl[t] and any(live) and not live[0]:
            out.add("no self entry")
        if nl[t] and any(not live[i] and any(live[:i]) and any(live[i + 1:]) for i in range(7)):
            out.add("-1 between live slots")
        if nl[t] and (sc.keys[sc.leaves_of(t)] >> 16 < sc.depth - 1).any():
            out.add("pruned keys")
    return out


def expect_restatement(O, P, sc, mode=0):
    """the restatement's answer: (alpha, beta, state byte, ybar [leaf, 7], kbar [leaf, 7]) — l_predict per (test block,
    neighbour) in the given sum mode, the gate in fp32, orc_node_update in nbr (ExtendedBlock) order"""
    o = O.OracleLMap(**dict(P, block_depth=sc.depth))
    f = np.float32
    A, B = sc.a0.copy(), sc.b0.copy()
    st = np.zeros(sc.keys.size, np.uint8)
    yb, kb = np.zeros((sc.keys.size, 7), f), np.zeros((sc.keys.size, 7), f)
    a, b_, s = C.c_float(), C.c_float(), C.c_uint8()
    O.set_sum_mode(mode)
    try:
        for t in range(len(sc.tests)):
            sl = sc.leaves_of(t)
            if sl.start == sl.stop:
                continue
            for q, tb in enumerate(sc.nbr[t]):
                if tb < 0:
                    continue
                rows = sc.rows[sc.rows_of(tb)]
                y, k = O.l_predict(P["sf2"], P["ell"], sc.pos[sl], rows[:, :6], rows[:, 6])
                yb[sl, q], kb[sl, q] = y, k
                for j in np.nonzero(k > f(0.001))[0]:
                    li = sl.start + int(j)
                    a.value, b_.value, s.value = A[li], B[li], st[li] & 3
                    o.L.orc_node_update(o.h, C.byref(a), C.byref(b_), C.byref(s), float(y[j]), float(k[j]))
                    A[li], B[li], st[li] = a.value, b_.value, s.value | 0x80
    finally:
        O.set_sum_mode(0)
    return A, B, st, yb, kb


def luts(O, P):
    """Block::key_loc_map per depth, depth-major (the host map hands the device the same table)"""
    return {d: np.ascontiguousarray(np.concatenate(O.OracleLMap(**dict(P, block_depth=d)).lut()), np.float32) for d in (2, 3, 4)}
