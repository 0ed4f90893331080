"""Hand-built BGK scans for tests/test_bgk_f64_cpu.py and tests/test_bgk_scans_gpu.py: a packer for la3dm_bgk_scan with rows
of 4 floats {x y z label}, the scans (a) to (i) of the GPU test's docstring, what the CPU restatement answers to them and the
classes a scan hits, computed from the constants parsed out of the kernel header.

Blocks stand on a grid: block (i, j, k) has the centre origin + (i, j, k) * block_size, and slot b of a test block is the
training block one step along DIRS[b] (ExtendedBlock order), -1 where none was added.  With per-tile descriptors on
(block_depth >= 4) the library assumes that the points of slot b lie in the closed box of that block and drops a face
neighbour from a tile whose cube does not touch that face, so World.add() asserts that every point lies in its block's
box; at depth 2 and 3 a point may be placed freely (free=True), as no descriptor is cut there.

Positions are chosen so that few leaves see ONLY points at 0.975 ... 1.02 ell, where the kernel value is below its own
rounding error (bgk_f64_ref: such gates are left out, and at most 2 % may be): clusters sit at the middle of a 4 x 4 x 4
voxel cube or on a face opposite one (leaf distances 0.087, 0.166, 0.218, 0.260 m), points on faces on the voxel lattice."""
import ctypes as C

import numpy as np

import bgk_f64_ref as R
from bgkl_scans import DIRS, PRIORS, finest, leaf_pos, priors, pruned_keys   # noqa: F401

VOXEL = 0.1
C0 = np.float64([0.0, 0.0, 0.0])
SHIFT = np.float64([2000.0, -1500.0, 30.0])
NONBINARY = np.float32([0.5, -1.0, 2.0, 0.0, 1.0])


def full_keys(depth):
    """every finest-level leaf in LeafIterator order (descending index): what the table kernels assume of a full block"""
    return finest(depth)[::-1].copy()


class Scan:
    """a la3dm_bgk_scan for la3dm_bgk_scan_* built from numpy arrays"""

    def __init__(self, depth):
        self.depth, self.blocks, self.tests = depth, [], []

    def block(self, pts):
        self.blocks.append(np.asarray(pts, np.float32).reshape(-1, 4))
        return len(self.blocks) - 1

    def test(self, centre, keys, nbr, a0, b0):
        self.tests.append(dict(centre=np.asarray(centre, np.float32), keys=np.asarray(keys, np.uint32), nbr=list(nbr),
                               a0=np.asarray(a0, np.float32), b0=np.asarray(b0, np.float32)))

    def pack(self, lut):
        n = np.array([len(b) for b in self.blocks], np.int64)
        self.lut = lut
        self.sizes = n
        self.train_off = np.concatenate([[0], np.cumsum(n)]).astype(np.uint32)
        self.pts = np.ascontiguousarray(np.concatenate(self.blocks + [np.zeros((0, 4), np.float32)]))
        self.nbr = np.array([t["nbr"] for t in self.tests], np.int32).reshape(-1, 7)
        self.centre = np.array([t["centre"] for t in self.tests], np.float32).reshape(-1, 3)
        self.leaf_off = np.concatenate([[0], np.cumsum([len(t["keys"]) for t in self.tests])]).astype(np.uint32)
        self.keys = np.concatenate([t["keys"] for t in self.tests] + [np.zeros(0, np.uint32)]).astype(np.uint32)
        self.a0 = np.concatenate([t["a0"] for t in self.tests] + [np.zeros(0, np.float32)]).astype(np.float32)
        self.b0 = np.concatenate([t["b0"] for t in self.tests] + [np.zeros(0, np.float32)]).astype(np.float32)
        ctr = np.repeat(self.centre, np.diff(self.leaf_off.astype(np.int64)), axis=0)
        self.pos = leaf_pos(lut, self.keys, ctr) if self.keys.size else np.zeros((0, 3), np.float32)
        self.n_fine = 8 ** (self.depth - 1)
        self.full = all(len(t["keys"]) == self.n_fine for t in self.tests)
        lab = self.pts[:, 3]
        self.binary = bool(((lab == 0) | (lab == 1)).all())
        return self

    def leaves_of(self, t):
        return slice(int(self.leaf_off[t]), int(self.leaf_off[t + 1]))

    def pts_of(self, b):
        return slice(int(self.train_off[b]), int(self.train_off[b + 1]))

    def tiles(self, wave):
        """(test block, first leaf, leaves) of every tile that holds leaves"""
        out = []
        for t in range(len(self.tests)):
            l0, l1 = int(self.leaf_off[t]), int(self.leaf_off[t + 1])
            out += [(t, s, min(wave, l1 - s)) for s in range(l0, l1, wave)]
        return out

    def rebuilt(self, blocks=None, pos_roll=0):
        """a copy with other training blocks, or with the leaf positions of every test block rotated by one lane"""
        sc = Scan(self.depth)
        sc.blocks = list(self.blocks if blocks is None else blocks)
        sc.tests = self.tests
        sc.pack(self.lut)
        if pos_roll:
            for t in range(len(sc.tests)):
                sl = sc.leaves_of(t)
                sc.pos[sl] = np.roll(sc.pos[sl], pos_roll, axis=0)
        return sc


class World:
    """blocks on a grid; build() derives the neighbour table from where the training blocks stand"""

    def __init__(self, depth, lut, origin=C0):
        self.depth, self.lut, self.origin = depth, lut, np.float64(origin)
        self.bs = VOXEL * 2 ** (depth - 1)
        self.train, self.tests = {}, []

    def centre(self, ijk):
        return self.origin + np.float64(ijk) * self.bs

    def face(self, ijk, s, beyond=0.0):
        """a point of test block ijk's face towards slot s, `beyond` metres inside that neighbour"""
        return self.centre(ijk) + DIRS[s] * (0.5 * self.bs + beyond)

    def add(self, ijk, xyz, labels, free=False):
        ijk = tuple(int(v) for v in ijk)
        xyz = np.float32(np.reshape(xyz, (-1, 3)))
        pts = np.concatenate([xyz, np.float32(labels).reshape(-1, 1)], axis=1).astype(np.float32)
        if not free or self.depth >= 4:
            # the rule of the per-tile descriptors: inside the block's closed box (fp32 positions, half a millimetre of rounding 2.5 km out)
            assert (np.abs(xyz.astype(np.float64) - self.centre(ijk)) <= 0.5 * self.bs + 5e-4).all(), (ijk, "a point outside its block")
        self.train[ijk] = np.concatenate([self.train[ijk], pts]) if ijk in self.train else pts
        return self

    def test(self, ijk, keys, a0, b0, drop=()):
        self.tests.append(dict(ijk=tuple(int(v) for v in ijk), keys=keys, a0=a0, b0=b0, drop=set(drop)))

    def leaves(self, ijk, keys):
        return leaf_pos(self.lut, keys, np.float32(self.centre(ijk))).astype(np.float64)

    def build(self):
        sc = Scan(self.depth)
        index = {ijk: sc.block(p) for ijk, p in self.train.items()}
        for t in self.tests:
            nbr = [-1 if s in t["drop"] else index.get(tuple(int(v) for v in np.add(t["ijk"], DIRS[s])), -1) for s in range(7)]
            sc.test(np.float32(self.centre(t["ijk"])), t["keys"], nbr, t["a0"], t["b0"])
        return sc.pack(self.lut)


def cube_centres(w, ijk):
    """{(cx, cy, cz): centre} of the 4 x 4 x 4 voxel cubes of a block (depth >= 3); at depth 2 the block itself"""
    n = max(int(round(w.bs / (4 * VOXEL))), 1)
    e = w.bs / n
    lo = w.centre(ijk) - 0.5 * w.bs
    return {(i, j, k): lo + (np.float64([i, j, k]) + 0.5) * e for i in range(n) for j in range(n) for k in range(n)}, n


def _labels(rng, n, binary=True):
    return rng.integers(0, 2, n).astype(np.float32) if binary else NONBINARY[rng.integers(len(NONBINARY), size=n)]


def _jit(rng, n, j=0.003):
    return rng.uniform(-j, j, (n, 3))


def _near_face(rng, w, ijk, s, cube_c, n, j=0.003):
    """n points of slot s on the shared face (or up to j behind it), opposite the cube whose centre is cube_c"""
    ax = int(np.argmax(np.abs(DIRS[s])))
    p = np.repeat(cube_c[None], n, axis=0) + _jit(rng, n, j / 3)
    p[:, ax] = w.face(ijk, s)[ax] + DIRS[s][ax] * rng.uniform(0.5 * j, 0.8 * j, n)   # (2 mm behind: 1.027 ell from the leaves at (0.35, 0.15, 0.15) at ell = 0.4)
    return p


def _far_face(rng, w, ijk, s, n, ell):
    """n points of slot s that reach nothing: at least 1.15 ell behind the shared face (inside the box from depth 4 on)"""
    ax = int(np.argmax(np.abs(DIRS[s])))
    lat = rng.uniform(-0.45 * w.bs, 0.45 * w.bs, (n, 3))
    lo = 1.15 * ell
    hi = max(w.bs - 0.01, lo + 0.01) if w.depth >= 4 else lo + ell
    assert w.depth < 4 or hi > lo + 0.005, "no room for a far point in this neighbour"
    p = w.centre(ijk) + lat
    p[:, ax] = w.face(ijk, s, 0.0)[ax] + DIRS[s][ax] * rng.uniform(lo, hi, n)
    return p


def _base_points(rng, w, ijk, ell):
    """one point at the middle of every cube of the block, from ell = 0.4 on and depth 4 on: every leaf then has a solid
    contribution of its own block (see the module docstring)"""
    if w.depth >= 4 and ell >= 0.39:
        cc, _ = cube_centres(w, ijk)
        p = np.float64(list(cc.values())) + _jit(rng, len(cc))
        w.add(ijk, p, _labels(rng, len(p)))


def counts_scan(depth, P, lut, consts, origin=C0):
    """(a) at depth 2, 3 and 4, with (g): one test block per pair (M, S) = (V[k], V[k - 1]) of flat count and survivors of the
    tile at the block's (+, +, +) corner; the points spread over one (+x only: no self entry), three (self, +y, +z, an empty
    training block at +x and -1 at -x between them) and seven neighbours; one more test block shares training blocks with
    another in different slots"""
    assert depth <= 4
    rng = np.random.default_rng(100 * depth + int(100 * P["ell"]))
    ell = float(np.float32(P["ell"]))
    V = R.count_values(consts) + [300, 301]
    w = World(depth, lut, origin)
    for k, M in enumerate(V):
        S = V[k - 1] if k else 0
        ijk = (4 * k, 0, 0)
        cc, n = cube_centres(w, ijk)
        cube = cc[(n - 1,) * 3]
        live = [[1], [0, 3, 5], [0, 1, 2, 3, 4, 5, 6]][k % 3]
        near_ok = [s for s in live if s in (0, 1, 3, 5)]
        far_ok = [s for s in live if s != 0]
        near = {s: len(x) for s, x in zip(near_ok, np.array_split(np.arange(S), len(near_ok)))}
        far = {s: len(x) for s, x in zip(far_ok, np.array_split(np.arange(M - S), len(far_ok)))}
        for s in live:
            a, b = near.get(s, 0), far.get(s, 0)
            p = [cube[None] + _jit(rng, a) if s == 0 else _near_face(rng, w, ijk, s, cube, a), _far_face(rng, w, ijk, s, b, ell) if b else np.zeros((0, 3))]
            p = np.concatenate(p)
            w.add(np.add(ijk, DIRS[s]), p[rng.permutation(len(p))], _labels(rng, len(p)), free=True)
        if k % 3 == 1:
            w.add(np.add(ijk, DIRS[1]), np.zeros((0, 3)), [])           # an empty training block between live ones
        if 0 in live:
            _base_points(rng, w, ijk, ell)
        keys = full_keys(depth)
        w.test(ijk, keys, *priors(rng, len(keys)))
        if k == 8:   # its +x neighbour is block k's self block, its self block is block k's -x neighbour
            w.test(np.add(ijk, DIRS[2]), keys, *priors(rng, len(keys)))
    return w.build()


# (self count, {slot: face count}) of the three depth-5 test blocks: the 27 subset sums a block's cubes see with per-tile
# descriptors on hold every value of R.count_values and 300; every face count is ONE cluster opposite a face cube and the
# self count one cluster in an inner cube, so the same numbers are survivor counts
DEPTH5 = [(0, {1: 1, 2: 15, 3: 16, 4: 17, 5: 31, 6: 32}),
          (64, {1: 1, 2: 63, 3: 64, 4: 65}),
          (300, {1: 127, 2: 128, 3: 129, 4: 33})]


def counts_scan5(P, lut, consts, origin=C0):
    """(a) at depth 5: three full test blocks, see DEPTH5 (derived for kTabSlots = 32, kWave = 64; classes() says what is hit)"""
    rng = np.random.default_rng(500 + int(100 * P["ell"]))
    ell = float(np.float32(P["ell"]))
    w = World(5, lut, origin)
    keys = full_keys(5)
    for k, (n_self, faces) in enumerate(DEPTH5):
        ijk = (4 * k, 0, 0)
        cc, n = cube_centres(w, ijk)
        if n_self:
            w.add(ijk, cc[(1, 2, 1)][None] + _jit(rng, n_self), _labels(rng, n_self))
        _base_points(rng, w, ijk, ell)
        for s, m in faces.items():
            ax = int(np.argmax(np.abs(DIRS[s])))
            c = [2, 1, 2]
            c[ax] = n - 1 if DIRS[s][ax] > 0 else 0
            w.add(np.add(ijk, DIRS[s]), _near_face(rng, w, ijk, s, cc[tuple(c)], m), _labels(rng, m))
        for s in range(1, 7):
            if s not in faces:
                w.add(np.add(ijk, DIRS[s]), np.zeros((0, 3)), [])
        w.test(ijk, keys, *priors(rng, len(keys)))
    return w.build()


def rings_scan(depth, P, lut, consts, origin=C0):
    """(b): per n of R.ring_counts a full test block with n points at the middle of a cube (every one reaches its 64 leaves
    from ell = 0.4 on) and a +x neighbour of 70 points that reach nothing: a drain is followed by chunks without hits"""
    rng = np.random.default_rng(200 + depth + int(100 * P["ell"]))
    ell = float(np.float32(P["ell"]))
    w = World(depth, lut, origin)
    keys = full_keys(depth)
    for k, m in enumerate(R.ring_counts(consts)):
        ijk = (4 * k, 0, 0)
        cc, n = cube_centres(w, ijk)
        w.add(ijk, cc[(n - 1,) * 3][None] + _jit(rng, m, 0.01), _labels(rng, m))
        w.add(np.add(ijk, DIRS[1]), _far_face(rng, w, ijk, 1, 70, ell), _labels(rng, 70), free=True)
        w.test(ijk, keys, *priors(rng, len(keys)))
    for k in range(10 if depth >= 4 else 0):     # blocks whose every leaf has a solid sum: the ring blocks' outer cubes see their cluster from 1 ell only
        ijk = (4 * k, 4, 0)
        p = _subcubes(w, ijk)
        w.add(ijk, p + _jit(rng, len(p)), _labels(rng, len(p)))
        w.test(ijk, keys, *priors(rng, len(keys)))
    return w.build()


def _subcubes(w, ijk):
    """the middles of the 2 x 2 x 2 voxel groups of a block: every leaf is 0.087 m from one"""
    cc, _ = cube_centres(w, ijk)
    off = np.float64([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)]) * VOXEL
    return np.concatenate([c[None] + (off if w.depth >= 3 else 0 * off[:1]) for c in cc.values()])


def labels_scan(depth, P, lut, binary=True, origin=C0):
    """(c): hits and free samples mixed in one staging trip; a label-1 point exactly at a leaf centre (d2 == 0: the table
    kernel carries the label in the sign of d2), a label-0 point at another, a label-1 point with d2 == 0 on one axis only;
    binary=False: the same places with labels 0.5, -1, 2, 0, 1 on leaves that carry (50, 50)"""
    rng = np.random.default_rng(300 + depth)
    w = World(depth, lut, origin)
    keys = full_keys(depth)
    ijk = (0, 0, 0)
    pos = w.leaves(ijk, keys)
    cc, n = cube_centres(w, ijk)
    sub = _subcubes(w, ijk)
    p = np.concatenate([pos[[5, 40]], pos[[17]] + [0.0, 0.03, -0.03], sub + _jit(rng, len(sub)), cc[(0, 0, 0)][None] + _jit(rng, 37, 0.02)])
    lab = _labels(rng, len(p), binary)
    lab[:3] = [1.0, 0.0, 1.0]
    w.add(ijk, p, lab)
    q = _near_face(rng, w, ijk, 3, cc[(0, n - 1, 0)], 30)
    w.add(np.add(ijk, DIRS[3]), q, _labels(rng, 30, binary))
    w.test(ijk, keys, *priors(rng, len(keys), None if binary else [(50, 50)]))
    sc = w.build()
    sc.exact = np.float32(pos[[5, 40, 17]])
    return sc


def reach_scan(depth, P, lut, consts, origin=C0):
    """(d) at depth 3 and 4: points at r = 0.97, 0.99, 1.01 and on either side of the fp32 hit threshold of ONE leaf (the
    (+, +, +) corner leaf of its cube, approached along +y); at 0.97 and 1.03 of the support from a cube's outermost leaf
    along the six axes and the diagonal; far points.  The leaves these points graze are left out of the float64 gate
    comparison by construction (the restatement decides them), so further test blocks whose every leaf has a solid sum keep
    the scan within the 2 % caps"""
    rng = np.random.default_rng(400 + depth)
    ell = float(np.float32(P["ell"]))
    w = World(depth, lut, origin)
    keys = full_keys(depth)
    ijk = (0, 0, 0)
    pos = w.leaves(ijk, keys)
    hi, lo = pos.max(0), pos.min(0)                       # the corner leaves of the block
    rt = float(np.sqrt(np.float64(consts["hit_t"])))
    for s in range(1, 7):
        c = hi if DIRS[s].sum() > 0 else lo
        rr = [0.97, 1.03] + ([0.99, 1.01, rt * (1 - 2e-6), rt * (1 + 2e-6)] if s == 3 else [])
        p = np.float64([c + DIRS[s] * ell * r for r in rr])
        if s == 5:
            p = np.concatenate([p, _far_face(rng, w, ijk, s, 20, ell)])
        w.add(np.add(ijk, DIRS[s]), p, _labels(rng, len(p)), free=True)
    # the diagonal: inwards from the outermost leaf of an inner cube where there is one (the points stay in this block),
    # outwards at depth 3
    cc, n = cube_centres(w, ijk)
    d = np.float64([1, 1, 1]) / np.sqrt(3.0)
    c = lo + (0.3 if n > 1 else 0.0)                      # the (+, +, +) leaf of cube (0, 0, 0)
    if n == 1:
        c = hi
    w.add(ijk, np.float64([c + d * ell * r for r in (0.97, 1.03)]), [1.0, 0.0], free=True)
    w.test(ijk, keys, *priors(rng, len(keys)))
    for k in range(1, 13 if depth == 3 else 5):
        other = (4 * k, 0, 0)
        p = _subcubes(w, other)                      # every leaf of these has a solid sum
        w.add(other, p + _jit(rng, len(p)), _labels(rng, len(p)))
        w.test(other, keys, *priors(rng, len(keys)))
    return w.build()


def lists_scan(depth, P, lut, origin=C0):
    """(e): a full block, pruned keys, one leaf, no leaves, a block with no neighbour, a partial list whose last tile holds
    one leaf (depth >= 4) or 37 leaves (depth 3) — full and pruned blocks in one launch; every block with points at the
    middle of its cubes and opposite two of its faces"""
    rng = np.random.default_rng(600 + depth + int(100 * P["ell"]))
    w = World(depth, lut, origin)
    fk = full_keys(depth)
    part = np.sort(rng.choice(fk, {2: 5, 3: 37}.get(depth, 65), replace=False))[::-1].astype(np.uint32)
    lists = [fk, pruned_keys(depth)[::-1].copy(), fk[:1], fk[:0], fk, part, fk]
    for k, keys in enumerate(lists):
        ijk = (4 * k, 0, 0)
        if k != 4:                                        # k == 4: no neighbour at all
            cc, n = cube_centres(w, ijk)
            p = np.repeat(np.float64(list(cc.values())), 3, axis=0)
            w.add(ijk, p + _jit(rng, len(p), 0.01), _labels(rng, len(p)))
            for s in (2, 5):
                ax = int(np.argmax(np.abs(DIRS[s])))
                sel = [c for key, c in cc.items() if key[ax] == (n - 1 if DIRS[s][ax] > 0 else 0)]
                q = np.concatenate([_near_face(rng, w, ijk, s, c, 2) for c in sel])
                w.add(np.add(ijk, DIRS[s]), q, _labels(rng, len(q)))
        w.test(ijk, keys, *priors(rng, len(keys)))
    return w.build()


def faces_scan(depth, P, lut, origin=C0):
    """(f): one full test block, all six face neighbours trained, each with points on the shared face itself and within ell
    behind it, opposite a corner, two edge and a face cube (depth 5), plus the self block; on the voxel lattice"""
    rng = np.random.default_rng(700 + depth + int(100 * P["ell"]))
    ell = float(np.float32(P["ell"]))
    w = World(depth, lut, origin)
    keys = full_keys(depth)
    ijk = (0, 0, 0)
    pos = w.leaves(ijk, keys)
    cc, n = cube_centres(w, ijk)
    p = np.float64(list(cc.values()))
    w.add(ijk, p + _jit(rng, len(p)), _labels(rng, len(p)))
    for s in range(1, 7):
        ax = int(np.argmax(np.abs(DIRS[s])))
        side = pos[:, ax].max() if DIRS[s][ax] > 0 else pos[:, ax].min()
        lat = [a for a in range(3) if a != ax]
        first = pos[(pos[:, ax] == side) & (pos[:, lat[0]] >= pos[:, lat[0]].max() - 0.75) & (pos[:, lat[1]] >= pos[:, lat[1]].max() - 0.75)]
        q = first[rng.choice(len(first), min(48, len(first)), replace=False)].copy()
        behind = np.where(np.arange(len(q)) % 2 == 0, 0.0, np.minimum(0.1 * rng.integers(1, 4, len(q)), ell - 0.1))
        q[:, ax] = w.face(ijk, s)[ax] + DIRS[s][ax] * behind
        w.add(np.add(ijk, DIRS[s]), q + _jit(rng, len(q), 0.0005) * (np.arange(3) != ax), _labels(rng, len(q)))
    w.test(ijk, keys, *priors(rng, len(keys)))
    return w.build()


def ungated_scan(depth, P, lut, origin=C0):
    """(h) for LA3DM_SCAN_UPDATE_UNGATED: a block whose trained neighbours are wholly out of reach (two of them), with an
    untrained slot between; a block with points in reach; a block with no point in any of its seven neighbours (M == 0)"""
    rng = np.random.default_rng(800 + depth)
    ell = float(np.float32(P["ell"]))
    w = World(depth, lut, origin)
    keys = full_keys(depth)
    for k in range(3):
        ijk = (4 * k, 0, 0)
        if k == 0:
            for s in (1, 4):
                w.add(np.add(ijk, DIRS[s]), _far_face(rng, w, ijk, s, 5, ell), _labels(rng, 5), free=True)
        if k == 1:
            cc, n = cube_centres(w, ijk)
            p = np.float64(list(cc.values()))
            w.add(ijk, p + _jit(rng, len(p)), _labels(rng, len(p)))
            w.add(np.add(ijk, DIRS[6]), _far_face(rng, w, ijk, 6, 5, ell), _labels(rng, 5), free=True)
        w.test(ijk, keys, *priors(rng, len(keys)))
    return w.build()


def nonfinite_scan(P, lut):
    """(i), depth 3: the +y neighbour holds a point with a NaN coordinate and a point at 3e19 m among 40 others; the self
    block and the -z neighbour are clean.  The reference's dense kernel matrix holds NaN in those two columns (cos of an
    infinite or NaN argument; the `< 0 -> 0` clean-up lets NaN through), so ybar and kbar of that neighbour are NaN at every
    leaf and `kbar > 0` rejects its update: mode 0 keeps the other neighbours' updates, mode 1 — one sum over all seven —
    updates nothing."""
    rng = np.random.default_rng(900)
    w = World(3, lut)
    keys = full_keys(3)
    ijk = (0, 0, 0)
    cc, n = cube_centres(w, ijk)
    c = cc[(0, 0, 0)]
    w.add(ijk, c[None] + _jit(rng, 20, 0.02), _labels(rng, 20))
    q = _near_face(rng, w, ijk, 3, c, 42, 0.02)
    q[7, 0] = np.nan
    q[30] = [3e19, 0.0, 0.0]
    w.add(np.add(ijk, DIRS[3]), q, _labels(rng, 42), free=True)
    w.add(np.add(ijk, DIRS[6]), _near_face(rng, w, ijk, 6, c, 25, 0.02), _labels(rng, 25))
    w.test(ijk, keys, *priors(rng, len(keys)))
    return w.build()


# ---- what a scan hits ----------------------------------------------------------------------------------------------

def tile_stats(sc, P, consts):
    """per tile with leaves: dict(t, first, nl, full, M = flat count of the block's seven neighbours, Mk = the same without the
    face neighbours a full block's cube does not touch (what a per-tile descriptor holds), S = points with a hit in this
    tile, hits = pairs that hit, kind = how many of the cube's sides lie on the block's surface (full blocks), ranges =
    the flat ends of the seven neighbours)"""
    ell = float(np.float32(P["ell"]))
    T = consts["hit_t"]
    out = []
    bs = VOXEL * 2 ** (sc.depth - 1)
    for t, s0, nl in sc.tiles(consts["kWave"]):
        pos = sc.pos[s0:s0 + nl].astype(np.float64)
        full = len(sc.tests[t]["keys"]) == sc.n_fine
        ctr = sc.centre[t].astype(np.float64)
        touch = [True] * 7
        kind = None
        if full and sc.depth >= 3:
            lo, hi = pos.min(0) - ctr, pos.max(0) - ctr
            edge = 0.5 * bs - 0.5 * VOXEL - 1e-3
            touch = [True] + [bool((hi if DIRS[s].sum() > 0 else -lo)[int(np.argmax(np.abs(DIRS[s])))] > edge) for s in range(1, 7)]
            kind = sum(touch[1:]) if sc.depth >= 4 else None
        M = Mk = S = hits = 0
        ends = []
        for s, tb in enumerate(sc.nbr[t]):
            if tb >= 0 and sc.sizes[tb]:
                p = sc.pts[sc.pts_of(tb), :3].astype(np.float64)
                M += len(p)
                Mk += len(p) if touch[s] else 0
                with np.errstate(invalid="ignore", over="ignore"):
                    d = (p[None] - pos[:, None]) / ell
                    h = (d[..., 0] ** 2 + (d[..., 1] ** 2 + d[..., 2] ** 2)) < T
                S += int(h.any(0).sum())
                hits += int(h.sum())
            ends.append(M)
        out.append(dict(t=t, first=s0, nl=nl, full=full, M=M, Mk=Mk, S=S, hits=hits, kind=kind, ends=ends))
    return out


def classes(sc, consts, P):
    """what the scan hits, as a set of names (module docstring of tests/test_bgk_scans_gpu.py)"""
    w = consts["kWave"]
    out = set()
    vals = set(R.count_values(consts))
    for ts in tile_stats(sc, P, consts):
        path = "table" if ts["full"] and sc.depth >= 3 else "general"
        for name, v in (("M", ts["M"]), ("M", ts["Mk"]), ("S", ts["S"])):
            if v in vals:
                out.add(f"{name}={v}")
                out.add(f"{name}={v} {path}")
            if 280 <= v <= 320:
                out.add(f"{name}~300")
        for ring in ("kRing5", "kRingR", "kRingT"):
            if ts["nl"] == w and ts["hits"] and ts["hits"] % w == 0 and ts["hits"] // w in R.ring_counts(consts):
                out.add(f"{ring} {'below' if ts['hits'] < consts[ring] else 'at' if ts['hits'] == consts[ring] else 'above'}")
        for c0 in range(0, ts["M"], w):            # a 64-point trip that holds points of k neighbours
            k = len({int(np.searchsorted(ts["ends"], f, side="right")) for f in range(c0, min(c0 + w, ts["M"]))})
            out.add(f"trip over {min(k, 3)} neighbours")      # (3: three or more)
        if ts["kind"] is not None:
            out.add(("interior", "face", "edge", "corner")[ts["kind"]] + " cube")
        out.add(f"{ts['nl']} live lanes")
    nl = np.diff(sc.leaf_off.astype(np.int64))
    for t in range(len(sc.tests)):
        live = [b >= 0 for b in sc.nbr[t]]
        some = [b >= 0 and sc.sizes[b] > 0 for b in sc.nbr[t]]
        if nl[t] == 0:
            out.add("no leaves")
        if nl[t] == 1:
            out.add("one leaf")
        if nl[t] and not any(live):
            out.add("no neighbour")
        if nl[t] and any(live) and not live[0]:
            out.add("no self entry")
        if nl[t] and any(not live[i] and any(live[:i]) and any(live[i + 1:]) for i in range(7)):
            out.add("-1 between live slots")
        if nl[t] and any(live[i] and not some[i] and any(some[:i]) and any(some[i + 1:]) for i in range(7)):
            out.add("empty neighbour between live ones")
        if nl[t] and (sc.keys[sc.leaves_of(t)] >> 16 < sc.depth - 1).any():
            out.add("pruned keys")
        if nl[t] == sc.n_fine:
            out.add("full block")
    used = {}
    for t in range(len(sc.tests)):
        for s, b in enumerate(sc.nbr[t]):
            if b >= 0 and nl[t]:
                used.setdefault(int(b), set()).add(s)
    if any(len(v) > 1 for v in used.values()):
        out.add("training block in several slots")
    lab = sc.pts[:, 3]
    if not sc.binary:
        out.add("non-binary labels")
    if ((lab == 0).any() and (lab == 1).any()):
        out.add("hits and free samples")
    if sc.keys.size and len(sc.pts):
        same = (sc.pts[None, :, :3] == sc.pos[:, None, :]) if sc.keys.size * len(sc.pts) < 4e6 else None
        if same is not None:
            if (same.all(-1) & (lab[None] == 1)).any():
                out.add("d2 == 0 with label 1")
            if (same.all(-1) & (lab[None] == 0)).any():
                out.add("d2 == 0 with label 0")
            if (same.any(-1) & ~same.all(-1) & (lab[None] == 1)).any():
                out.add("d2 == 0 on one axis with label 1")
    return out


# ---- the restatement's answers ---------------------------------------------------------------------------------------

def _update(o, A, B, st, li, y, k, a, b_, s):
    a.value, b_.value, s.value = A[li], B[li], st[li] & 3
    o.L.orc_node_update(o.h, C.byref(a), C.byref(b_), C.byref(s), float(y), float(k))
    A[li], B[li], st[li] = a.value, b_.value, s.value | 0x80


def expect_restatement(O, P, sc, mode=0, ungated=False):
    """the restatement's answer (alpha, beta, state byte).
    mode 0: oracle.bgk_predict per (test block, trained neighbour), the kbar > 0 gate in fp32, orc_node_update in nbr order.
    mode 1: the same fp32 k (oracle.kernel on an r formed with numpy fp32 operations in the order of
    oracle/la3dm_oracle.cpp:403-426) and fl(k y) per pair, summed in float64 over all seven neighbours; one gate K > 0; alpha =
    fl(alpha + Y), beta = fl(beta + (K - Y)) from the double sums, then orc_node_update(0, 0) for the state (:1251-1262).
    A training block without points is no model (a model has at least one point).  Ungated, mode 0 updates once per model
    (a test block without one among its seven neighbours is not touched, src/bgkoctomap/bgkoctomap.cpp:168-181 of the
    reference); mode 1 runs its one update for every leaf, as the restatement's sum mode 1 does (:1251-1262)."""
    o = O.OracleMap(**dict(P, block_depth=sc.depth))
    f = np.float32
    A, B = sc.a0.copy(), sc.b0.copy()
    st = np.zeros(sc.keys.size, np.uint8)
    a, b_, s = C.c_float(), C.c_float(), C.c_uint8()
    ell, sf2 = f(P["ell"]), float(P["sf2"])
    for t in range(len(sc.tests)):
        sl = sc.leaves_of(t)
        if sl.start == sl.stop:
            continue
        nl = sl.stop - sl.start
        Y, K = np.zeros(nl), np.zeros(nl)
        trained = False
        for tb in sc.nbr[t]:
            if tb < 0 or sc.sizes[tb] == 0:
                continue
            trained = True
            pts = sc.pts[sc.pts_of(tb)]
            if mode == 0:
                y, k = O.bgk_predict(sf2, float(ell), sc.pos[sl], pts[:, :3], pts[:, 3])
                for j in (range(nl) if ungated else np.nonzero(k > f(0.0))[0]):
                    _update(o, A, B, st, sl.start + int(j), y[j], k[j], a, b_, s)
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                xs, xn = (sc.pos[sl] / ell).astype(f), (pts[:, :3] / ell).astype(f)
                d = (xn[None] - xs[:, None]).astype(f)
                d2 = (d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])).astype(f)
                r = np.sqrt(d2).astype(f)
                k = O.kernel(r.reshape(-1), sf2).reshape(r.shape)
                ky = (k * pts[None, :, 3]).astype(f)
                K += k.astype(np.float64).sum(1)
                Y += ky.astype(np.float64).sum(1)
        if mode == 1:
            for j in (range(nl) if ungated else np.nonzero(K > 0.0)[0]):
                li = sl.start + int(j)
                with np.errstate(invalid="ignore"):
                    A[li], B[li] = f(np.float64(A[li]) + Y[j]), f(np.float64(B[li]) + (K[j] - Y[j]))
                _update(o, A, B, st, li, 0.0, 0.0, a, b_, s)
    return A, B, st


def luts(O, P, depths=(2, 3, 4, 5)):
    """Block::key_loc_map per depth, depth-major (the host map hands the device the same table)"""
    return {d: np.ascontiguousarray(np.concatenate(O.OracleMap(**dict(P, block_depth=d)).lut()), np.float32) for d in depths}


PARAMS = {"yaml": R.BGK_YAML, "ell04": R.P4, "ell05": R.P5}


def cases():
    """every scan both test files run: (tag, depth, parameter set, builder(lut, consts), ungated)"""
    out = []
    for k in PARAMS:
        for d in (2, 3, 4):
            out.append((f"counts d{d} {k}", d, k, lambda lut, c, d=d, k=k: counts_scan(d, PARAMS[k], lut, c), False))
        out.append((f"counts d5 {k}", 5, k, lambda lut, c, k=k: counts_scan5(PARAMS[k], lut, c), False))
    for k in ("ell04", "ell05"):
        for d in (3, 4):
            out.append((f"rings d{d} {k}", d, k, lambda lut, c, d=d, k=k: rings_scan(d, PARAMS[k], lut, c), False))
    for d in (3, 4):
        for binary in (True, False):
            out.append((f"labels d{d} {'binary' if binary else 'non-binary'}", d, "yaml",
                        lambda lut, c, d=d, b=binary: labels_scan(d, R.BGK_YAML, lut, b), False))
        for k in ("yaml", "ell04"):
            for far in (False, True):
                out.append((f"reach d{d} {k}{' translated' if far else ''}", d, k,
                            lambda lut, c, d=d, k=k, far=far: reach_scan(d, PARAMS[k], lut, c, SHIFT if far else C0), False))
        out.append((f"ungated d{d}", d, "yaml", lambda lut, c, d=d: ungated_scan(d, R.BGK_YAML, lut), True))
    for d in (2, 3, 4, 5):
        out.append((f"lists d{d} yaml", d, "yaml", lambda lut, c, d=d: lists_scan(d, R.BGK_YAML, lut), False))
    for d in (4, 5):
        for k in ("yaml", "ell04"):
            out.append((f"faces d{d} {k}", d, k, lambda lut, c, d=d, k=k: faces_scan(d, PARAMS[k], lut), False))
    return out
