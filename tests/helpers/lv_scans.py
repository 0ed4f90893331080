"""Hand-built BGK-LV scans for tests/test_lv_f64_cpu.py and tests/test_lv_scans_gpu.py: a packer for la3dm_lv_scan written
from the contract comment of include/la3dm_hip.h, a ray builder whose samples are monotone per coordinate, the scans (a) to
(k) of the GPU test's docstring, the stream length of every cube (and with it the workgroups the plan must hand out), and
the classes a scan hits, computed from the constants parsed out of lv_kernels.h by a model of the kernel's staging loop.

Every sample carries the kind it was built as:
  H  a hit within a quarter of ell of an active voxel                                                      near
  B  a ray through a point within a quarter of ell of an active voxel, sampled every 0.07 m                 near
  S  the same, sampled every 0.45 m (often one sample in a voxel's box)                                     near
  N  a ray that starts next to an active voxel (its first sample is in the box, often in the core box)      near
  M  a ray that ends next to an active voxel (voxels beyond the end of the segment)                         near
  Z  a ray of length 0 or 5e-5 next to an active voxel (point_to_line_dist measures to its start)           near
  I  a ray that passes an active voxel at 0.97 ell, with a sample at the foot
  O  the same at 1.03 ell (the foot is in the voxel's cubic box: a row with k = sf2 g(1))
  C  a ray that passes an active voxel's box near an edge, 1.13 ell from the centre
  W  a weak hit at a distance chosen for its k
  X  a hit on, or one float beyond, a face of a voxel's box
  F  a filler: a hit in a corner bucket of a cube's neighbourhood, outside every voxel's box
  U  a hit inside a cube's outer box but in no active voxel's box"""
import numpy as np

import lv_f64_ref as R

NEAR = ("H", "B", "S", "N", "M", "Z")
# alpha, beta of a voxel before the scan: the prior of a new node, and what earlier scans left on either side
PRIORS = np.float32([(0.001, 0.001)] * 4 + [(0.5, 0.001), (0.001, 0.5), (50, 0.001), (0.001, 50), (5000, 0.001), (0.001, 5000),
                                            (0.5, 0.5), (50, 50), (0.0004, 0.0003)])
HEAVY = np.float32([(50, 0.001), (0.001, 50)])


class LvScan:
    """a la3dm_lv_scan built from hits, rays and blocks; pack() lays the arrays out as the contract words them"""

    def __init__(self, depth, P, lut):
        f = np.float32
        self.depth, self.P = depth, P
        self.res = f(P["resolution"])
        self.bs32 = f(2 ** (depth - 1)) * self.res
        self.bs = float(self.bs32)
        self.g = 4.0 * float(self.res) if depth >= 3 else self.bs
        self.half = 0.5 * self.bs
        self.ell = float(f(P["ell"]))
        self.reach = int(np.ceil(self.ell / self.g))
        self.npb = 8 ** (depth - 1)
        self.cubes = max(self.npb // 64, 1)
        self.bpb = max(2 ** (depth - 3), 1)                   # buckets per block edge
        self.lut_f = np.asarray(lut, f).reshape(-1, 3)[(8 ** (depth - 1) - 1) // 7:]
        assert len(self.lut_f) == self.npb
        self._smp, self._kinds, self._rays, self._ray_kinds, self._blocks = [], [], [], [], []

    # ---- building
    def hit(self, p, kind):
        self._smp.append([p[0], p[1], p[2], -1.0])
        self._kinds.append(kind)

    def ray(self, a, b, ts, kind):
        """a segment a -> b with samples a + t (b - a), t ascending from 0: the first sample is the segment start, and every
        coordinate is monotone along the ray, also after rounding to fp32 (rounding is monotone)"""
        ts = np.asarray(ts, np.float64)
        assert ts[0] == 0.0 and (np.diff(ts) >= 0).all()
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        a32 = a.astype(np.float32).astype(np.float64)
        pts = np.float32(a32[None] + ts[:, None] * (b - a32)[None])
        k = len(self._rays)
        for p in pts:
            self._smp.append([p[0], p[1], p[2], float(k)])
            self._kinds.append(kind)
        self._rays.append(np.concatenate([np.float32(a32), np.float32(b)]))
        self._ray_kinds.append(kind)
        return k

    def centre(self, idx):
        """Block centre of block index idx (hash_key_to_block: index * block_size in fp32)"""
        return np.float32(idx) * self.bs32

    def voxels(self, idx):
        """fp32 positions of the finest layer's nodes of block idx: lut + centre"""
        return (self.lut_f + self.centre(idx)[None]).astype(np.float32)

    def block(self, idx, active, a0, b0):
        active = np.asarray(active, bool)
        assert active.shape == (self.npb,)
        self._blocks.append(dict(idx=np.asarray(idx, np.int64), active=active, a0=np.float32(a0), b0=np.float32(b0)))
        return len(self._blocks) - 1

    # ---- packing (include/la3dm_hip.h, la3dm_lv_scan)
    def cidx(self, v):
        return np.floor((np.asarray(v, np.float32).astype(np.float64) + self.half) / self.g).astype(np.int64)

    def pack(self):
        f = np.float32
        self.samples = np.ascontiguousarray(np.array(self._smp, np.float64).reshape(-1, 4), f)
        self.kinds = np.array(self._kinds, "U1")
        n = len(self.samples)
        rays6 = np.array(self._rays, f).reshape(-1, 6)
        self.rays = rays6
        self.ray_kinds = np.array(self._ray_kinds, "U1")
        ray = self.samples[:, 3].astype(np.int64)
        first = np.full(len(rays6), -1, np.int64)
        for i in np.nonzero(ray >= 0)[0][::-1]:
            first[ray[i]] = i
        self.ray_first = first
        self.rays8 = np.zeros((len(rays6), 8), f)
        self.rays8[:, 0:3], self.rays8[:, 4:7] = rays6[:, 0:3], rays6[:, 3:6]
        self.rays8[:, 3] = first.astype(np.int32).view(f)
        assert (self.samples[first, :3] == rays6[:, :3]).all()
        cc = self.cidx(self.samples[:, :3])
        self.cell_min = cc.min(0).astype(np.int32)
        self.cell_dim = (cc.max(0) - cc.min(0) + 1).astype(np.int32)
        rel = cc - cc.min(0)
        lin = (rel[:, 2] * int(self.cell_dim[1]) + rel[:, 1]) * int(self.cell_dim[0]) + rel[:, 0]
        order = np.argsort(lin, kind="stable")
        self.order = order
        self.sorted = np.zeros((n, 4), f)
        self.sorted[:, :3] = self.samples[order, :3]
        self.sorted[:, 3] = order.astype(np.int32).view(f)
        ncell = int(np.prod(self.cell_dim.astype(np.int64)))
        self.cell_off = np.concatenate([[0], np.cumsum(np.bincount(lin, minlength=ncell))]).astype(np.uint32)
        self.n_blk = len(self._blocks)
        self.blk_idx = np.array([b["idx"] for b in self._blocks], np.int64).reshape(-1, 3)
        self.blk_center = np.ascontiguousarray([self.centre(b["idx"]) for b in self._blocks], f).reshape(-1, 3)
        self.blk_cell0 = np.rint(self.blk_center.astype(np.float64) / self.g).astype(np.int32)
        self.active = np.concatenate([b["active"] for b in self._blocks])
        self.a0 = np.concatenate([np.broadcast_to(b["a0"], (self.npb,)) for b in self._blocks]).astype(f)
        self.b0 = np.concatenate([np.broadcast_to(b["b0"], (self.npb,)) for b in self._blocks]).astype(f)
        # state in: the node's LV code, whatever it is, for a base-resolution leaf; 4 for the others
        self.state0 = np.where(self.active, np.arange(len(self.active)) % 4, 4).astype(np.uint8)
        self.pos = np.concatenate([self.voxels(b["idx"]) for b in self._blocks]).astype(f)
        return self

    def nodes_of(self, b):
        return slice(b * self.npb, (b + 1) * self.npb)


def luts(O, P):
    """Block::key_loc_map per depth, depth-major (the restatement's table, pinned against the reference's)"""
    return {d: O.OracleLVMap(**dict(P, block_depth=d)).lut(d) for d in (2, 3, 4, 5)}


def expect_restatement(O, sc, mode=0, trig=0):
    """(alpha, beta, state byte) of the packed scan from the restatement's voxel loop body (oracle.OracleLVMap.packed_scan)"""
    o = O.OracleLVMap(**dict(sc.P, block_depth=sc.depth))
    O.set_sum_mode(mode)
    O.set_modes(trig, 0)
    try:
        return o.packed_scan(sc.samples, sc.sorted, sc.rays8, sc.cell_off, sc.cell_min, sc.cell_dim, sc.blk_center, sc.a0, sc.b0,
                             sc.state0)
    finally:
        O.set_sum_mode(0)
        O.set_modes(0, 0)


# ---- what the kernel will do with a scan --------------------------------------------------------------------------------
def _cube_streams(sc):
    """per cube (block-major, octree order): its bucket, and the sorted-array ranges of its (2 reach + 1)^3 buckets, z-major"""
    r, dim = sc.reach, sc.cell_dim.astype(np.int64)
    w = 2 * r + 1
    dz, dy, dx = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")
    d = np.stack([dx.ravel(), dy.ravel(), dz.ravel()], 1)
    out = []
    for b in range(sc.n_blk):
        for c in range(sc.cubes):
            first = b * sc.npb + c * 64
            cell = sc.cidx(sc.pos[first]) - sc.cell_min
            q = cell[None] + d
            ok = ((q >= 0) & (q < dim[None])).all(1)
            lin = (q[:, 2] * dim[1] + q[:, 1]) * dim[0] + q[:, 0]
            lin = np.where(ok, lin, 0)
            c0 = np.where(ok, sc.cell_off[lin], 0).astype(np.int64)
            c1 = np.where(ok, sc.cell_off[lin + 1], 0).astype(np.int64)
            out.append(dict(block=b, cube=c, cell=cell, ok=ok, c0=c0, c1=c1, nodes=slice(first, min(first + 64, (b + 1) * sc.npb))))
    assert w ** 3 == len(d)
    return out


def stream_lengths(sc):
    """samples in the (2 reach + 1)^3 buckets of every cube, block-major"""
    return np.array([int((s["c1"] - s["c0"]).sum()) for s in _cube_streams(sc)], np.int64)


def expected_tiles(sc, consts):
    """workgroups of the voxel kernel: max(1, ceil(stream / kLvChunk)) for a cube with an active voxel, 1 for a cube with none"""
    ch = consts["kLvChunk"]
    n = 0
    for s, L in zip(_cube_streams(sc), stream_lengths(sc)):
        n += max(1, -(-int(L) // ch)) if sc.active[s["nodes"]].any() else 1
    return n


def _boxes(sc, nodes):
    f = np.float32
    p = sc.pos[nodes]
    e = f(sc.P["ell"])
    return (p - e).astype(f), (p + e).astype(f)


def _inside(lo, hi, q):
    """closed fp32 boxes [m, 3] against points [n, 3] -> [m, n]"""
    return ((lo[:, None, :] <= q[None]) & (q[None] <= hi[:, None, :])).all(-1)


def classes(sc, consts):
    """what the scan hits, as a set of names (module docstring of tests/test_lv_scans_gpu.py), from a model of
    bgklv_plan_kernel and of the staging loop of bgklv_voxel_body"""
    ch, grp, w = consts["kLvChunk"], consts["kLvGroup"], consts["kWave"]
    out = set()
    streams = _cube_streams(sc)
    L = stream_lengths(sc)
    ray = sc.samples[:, 3].astype(np.int64)
    xyz = sc.samples[:, :3]
    first_of = np.where(ray >= 0, sc.ray_first[np.maximum(ray, 0)], -1)
    is_later = (ray >= 0) & (np.arange(len(ray)) != first_of)
    prev = np.where(is_later, np.arange(len(ray)) - 1, np.arange(len(ray)))
    split_tasks, light_tasks = [], []
    out.add(f"{len(streams)} cubes")
    for task, (s, n) in enumerate(zip(streams, L)):
        act = sc.active[s["nodes"]]
        out.add(f"{int(act.sum())} active")
        if not act.any():
            out.add("cube with no active voxel")
            continue
        for a in range(3):
            if s["cell"][a] - sc.reach < 0:
                out.add("neighbourhood sticks out at the low side of axis %d" % a)
            if s["cell"][a] + sc.reach >= sc.cell_dim[a]:
                out.add("neighbourhood sticks out at the high side of axis %d" % a)
        cnt = s["c1"] - s["c0"]
        if (s["ok"] & (cnt == 0)).any():
            out.add("empty bucket")
        if n == 0:
            out.add("cube with no sample in reach")
            continue
        nsub = max(1, -(-int(n) // ch))
        (split_tasks if nsub > 1 else light_tasks).append(task)
        for k, name in zip(R.stream_sizes(consts), ("chunk-1", "chunk", "chunk+1", "2 chunks", "2 chunks+1", "3 chunks+5")):
            if n == k:
                out.add("stream " + name)
        # the stream: sample indices in gather order, the bucket number of every position
        idx = np.concatenate([sc.order[a:b] for a, b in zip(s["c0"], s["c1"])])
        bucket = np.repeat(np.arange(len(cnt)), cnt)
        cum = np.cumsum(cnt)
        lo, hi = _boxes(sc, s["nodes"])
        lo, hi = lo[act], hi[act]
        outer = _inside(lo.min(0)[None], hi.max(0)[None], xyz[idx])[0]
        core_lo, core_hi = lo.max(0)[None], hi.min(0)[None]
        later = is_later[idx]
        p_core = _inside(core_lo, core_hi, xyz[prev[idx]])[0]
        f_core = _inside(core_lo, core_hi, xyz[np.maximum(first_of[idx], 0)])[0]
        keep = outer & ~(later & (p_core | f_core))
        inb = _inside(lo, hi, xyz[idx])                                            # [voxel, position]
        f_in = _inside(lo, hi, xyz[np.maximum(first_of[idx], 0)])
        p_in = _inside(lo, hi, xyz[prev[idx]])
        count = np.where(later[None], inb & ~f_in & ~p_in, inb)
        counted = count.any(0)
        if (outer & ~inb.any(0)).any():
            out.add("a sample in the outer box but in no voxel's box")
        if (later & outer & f_core).any():
            out.add("first sample in the core box")
        if (later[None] & inb & f_in).any():
            out.add("first sample in the box")
        # samples of one ray in one voxel's box
        rr = ray[idx]
        for k in np.unique(rr[rr >= 0]):
            m = inb[:, rr == k].sum(1)
            for v, name in ((1, "1"), (2, "2")):
                if (m == v).any():
                    out.add(f"a ray with {name} samples in a box")
            if (m >= 3).any():
                out.add("a ray with many samples in a box")
        # the previous sample of a counted later sample: in another bucket / group of this stream, or in none
        pos_of = {int(i): j for j, i in enumerate(idx)}
        for j in np.nonzero(later & counted)[0]:
            pj = pos_of.get(int(prev[idx[j]]))
            if pj is None:
                out.add("previous sample outside the stream")
            elif bucket[pj] != bucket[j]:
                out.add("previous sample in another bucket")
                if bucket[pj] // grp != bucket[j] // grp:
                    out.add("previous sample in another group")
        # sub-tasks and staging passes
        bounds = [(k * ch, min((k + 1) * ch, int(n))) for k in range(nsub)] if nsub > 1 else [(0, int(n))]
        gstart = np.concatenate([[0], cum[grp - 1::grp], [cum[-1]]]) if len(cnt) > grp else np.array([0, cum[-1]])
        gstart = np.unique(gstart)
        if nsub > 1:
            for k in range(1, nsub):
                b0 = k * ch
                if b0 in set(cum[grp - 1::grp].tolist()) and len(cnt) > grp:
                    out.add("sub-task boundary on a group boundary")
                if b0 in set(cum.tolist()):
                    out.add("sub-task boundary on a bucket boundary")
                else:
                    out.add("sub-task boundary inside a bucket")
        for a, b in bounds:
            parts = [(max(a, int(g0)), min(b, int(g1))) for g0, g1 in zip(gstart[:-1], gstart[1:]) if max(a, g0) < min(b, g1)]
            if nsub > 1 and len(parts) > 1:
                out.add("sub-task spans two groups")
            rows = 0
            kept_any = False
            for pa, pb in parts:
                for q in range(pa, pb, ch):
                    sel = slice(q, min(q + ch, pb))
                    kk, cc, hh = keep[sel], counted[sel][keep[sel]], (ray[idx[sel]] < 0)[keep[sel]]
                    K = int(kk.sum())
                    kept_any |= K > 0
                    if K in R.kept_sizes(consts):
                        out.add(f"{K} kept candidates")
                    rows += int(cc.sum())
                    prev_hit = False
                    for r0 in range(0, K, w):
                        c_r, h_r = cc[r0:r0 + w], hh[r0:r0 + w]
                        has_hit = bool((c_r & h_r).any())
                        if not has_hit:
                            out.add("round with no hit row")
                        if has_hit and prev_hit:
                            out.add("hit rows in consecutive rounds")
                        prev_hit = has_hit
                        nz = np.nonzero(c_r)[0]
                        if len(nz) and not c_r[nz[0]:nz[-1] + 1].all():
                            out.add("uncounted candidates between counted ones")
            if nsub > 1:
                if not kept_any:
                    out.add("sub-task all culled")
                if rows in R.split_row_sizes(consts):
                    out.add(f"{rows} rows in a sub-task")
    # the plan: kLvPlanPerWave cubes per wave, four waves per workgroup
    ppw = consts["kLvPlanPerWave"]
    sb, lb = {t // sc.cubes for t in split_tasks}, {t // sc.cubes for t in light_tasks}
    if sb & lb:
        out.add("split and unsplit cubes in one block")
    sw, lw = {t // ppw for t in split_tasks}, {t // ppw for t in light_tasks}
    if sw & lw:
        out.add("split and unsplit cubes in one plan wave")
    if sw and lw and (lw - sw):
        out.add("split and unsplit cubes in different plan waves")
    if len(sw) > 1:
        out.add("split cubes in several plan waves")
    if len({t // (4 * ppw) for t in split_tasks}) > 1:
        out.add("split cubes in several plan workgroups")
    # the grid
    for b in range(sc.n_blk):
        c0 = sc.blk_cell0[b].astype(np.int64) - sc.cell_min
        if ((c0 < 0) | (c0 + sc.bpb > sc.cell_dim)).any():
            out.add("a block's buckets partly outside the grid")
        if all(L[b * sc.cubes + c] == 0 for c in range(sc.cubes)) and sc.active[sc.nodes_of(b)].any():
            out.add("block with no sample in reach")
    d = np.abs(sc.blk_cell0[:, None, :].astype(np.int64) - sc.blk_cell0[None].astype(np.int64)).max(-1)
    if ((d > 0) & (d < sc.bpb + 2 * sc.reach)).any():
        out.add("two blocks share buckets")
    return out


# ---- content ------------------------------------------------------------------------------------------------------------
def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _perp(rng, w):
    e = np.cross(w, _unit(rng))
    return e / np.linalg.norm(e)


def _ts(length, step):
    return np.arange(0.0, 1.0, step / length)


def content(sc, rng, targets, kinds, short_ok=True):
    """samples of the given kinds round the active voxels `targets` (float64 [m, 3])"""
    ell = sc.ell
    for i, k in enumerate(kinds):
        t = targets[int(rng.integers(len(targets)))]
        if k == "H":
            sc.hit(t + _unit(rng) * rng.uniform(0, 0.25 * ell), "H")
        elif k in ("B", "S"):
            q, w = t + _unit(rng) * rng.uniform(0, 0.25 * ell), _unit(rng)
            la, lb = rng.uniform(0.6, 1.6, 2)
            sc.ray(q - w * la, q + w * lb, _ts(la + lb, 0.07 if k == "B" else 0.45), k)
        elif k == "N":
            q, w = t + _unit(rng) * rng.uniform(0, 0.25 * ell), _unit(rng)
            lb = rng.uniform(0.3, 1.2)
            sc.ray(q, q + w * lb, _ts(lb, 0.07), "N")
        elif k == "M":
            q, w = t + _unit(rng) * rng.uniform(0, 0.25 * ell), _unit(rng)
            la = rng.uniform(0.3, 1.2)
            sc.ray(q - w * la, q, np.append(_ts(la, 0.07), 1.0), "M")
        elif k == "Z":
            q = t + _unit(rng) * rng.uniform(0, 0.25 * ell)
            if i % 2 and short_ok:
                sc.ray(q, q + np.float64([5e-5, 0, 0]), [0.0, 1.0], "Z")
            else:
                sc.ray(q, q, [0.0], "Z")
        elif k in ("I", "O"):
            w = _unit(rng)
            e = _perp(rng, w)
            foot = t + e * ell * (0.97 if k == "I" else 1.03)
            la, lb = rng.uniform(0.5, 1.5, 2)
            a, b = foot - w * la, foot + w * lb
            ts = np.sort(np.concatenate([_ts(la + lb, 0.11), [la / (la + lb)]]))
            sc.ray(a, b, ts, k)
        elif k == "C":
            s = rng.choice([-1.0, 1.0], 3)
            ax = int(rng.integers(3))
            off = 0.8 * ell * s
            off[ax] = 0.0
            w = np.zeros(3)
            w[ax] = s[ax]
            q = t + off
            sc.ray(q - w * 0.7, q + w * 0.9, np.sort(np.concatenate([_ts(1.6, 0.13), [0.7 / 1.6]])), "C")
        else:
            raise ValueError(k)


def fillers(sc, idx, n, where):
    """n hits in the corner bucket of the block's neighbourhood (where = 'first': the lowest bucket on all three axes — the
    first one of the stream of the block's first cube, and in no other cube's reach; 'last': the highest, for the last
    cube), 2 to 10 % of a bucket edge from its outer faces: outside every voxel's box"""
    if n <= 0:
        return
    g, r = sc.g, sc.reach
    c0 = np.rint(sc.centre(idx).astype(np.float64) / g)
    rng = np.random.default_rng(int(n) * 7 + ("first", "second", "last").index(where))
    if where in ("first", "second"):
        edge = (c0 - r) * g - sc.half
        p = edge[None] + rng.uniform(0.02, 0.1, (n, 3)) * g
        if where == "second":      # the bucket above the first one: also in the reach of the first cube's upper neighbour
            p[:, 2] += g
    else:
        edge = (c0 + sc.bpb - 1 + r + 1) * g - sc.half
        p = edge[None] - rng.uniform(0.02, 0.1, (n, 3)) * g
    for q in p:
        sc.hit(q, "F")


def _active(rng, sc, how):
    """active voxels of a block: 'all', a number (that many per cube of 64), 'none'"""
    a = np.zeros(sc.npb, bool)
    if how == "all":
        a[:] = True
    elif how != "none":
        for c in range(sc.cubes):
            n = min(64, sc.npb)
            a[c * n + rng.choice(n, min(int(how), n), replace=False)] = True
    return a


def _priors(rng, n, heavy=False):
    p = (HEAVY if heavy else PRIORS)[rng.integers(len(HEAVY if heavy else PRIORS), size=n)]
    return p[:, 0].copy(), p[:, 1].copy()


def _count_in_cells(sc, idx_lo, idx_hi, first):
    """samples built so far whose bucket lies in [idx_lo, idx_hi] on every axis"""
    if not sc._smp:
        return 0
    cc = sc.cidx(np.array(sc._smp, np.float64)[first:, :3].astype(np.float32))
    return int(((cc >= idx_lo[None]) & (cc <= idx_hi[None])).all(1).sum())


def spacing(sc):
    """blocks this many block indices apart have disjoint neighbourhoods"""
    return -(-(sc.bpb + 2 * sc.reach + 1) // sc.bpb)


MIX = "HHHBBSNMZIOC"


def stream_scan(depth, P, lut, consts, shift=(0, 0, 0), heavy=False):
    """(a), (g), (h): one block per stream length of R.stream_sizes, far enough apart that no neighbourhood overlaps; the
    fillers go before and behind the block's own samples in the stream so that the sub-task boundaries fall inside a bucket,
    on a bucket boundary and — with more than kLvGroup buckets — on a group boundary; the active sets are 64, 37 and 1
    voxels per cube; plus a block without an active voxel, one without a sample in reach, one next to the first block
    (shared buckets) and, at depth >= 4, a gradient of fillers that splits some cubes of a block and not others"""
    rng = np.random.default_rng(100 * depth + int(10 * P["ell"]))
    sc = LvScan(depth, P, lut)
    ch = consts["kLvChunk"]
    sp = spacing(sc)
    shift = np.asarray(shift, np.int64)
    hows = ["all", 37, "all", 1, "all", 37]
    def add(idx, how, kinds):
        # (far from the origin a ray's bound is wide: few active voxels, and a hit at each keeps kbar clear of the gate)
        act = _active(rng, sc, how if not heavy or how in (1, "none") else 8)
        tg = sc.voxels(idx)[act if act.any() else slice(None)].astype(np.float64)
        if heavy and act.any():
            for t in tg:
                sc.hit(t + rng.uniform(-0.02, 0.02, 3), "H")
        content(sc, rng, tg, kinds, short_ok=not heavy)
        sc.block(idx, act, *_priors(rng, sc.npb, heavy))

    for i, Lw in enumerate(R.stream_sizes(consts)):
        add(shift + np.int64([sp * i, 0, 0]), hows[i], list(MIX) * 2 + ["H"] * 8)
    add(shift + np.int64([0, sp, 0]), "none", "HHBN")                  # no active voxel, samples around
    add(shift + np.int64([0, -2 * sp, 0]), "all", "")                  # no sample in reach
    for dz in (0, 1):                                                  # two blocks next to each other: shared buckets
        add(shift + np.int64([3 * sp, sp, dz]), "all", "HHHBS")
    if sc.cubes > 1:
        # a wall of hits beside a block, out of every box: the cubes on that side are split, the others are not
        idx = shift + np.int64([sp, 2 * sp, 0])
        add(idx, "all", "HHHHBBSN")
        c = sc.centre(idx).astype(np.float64)
        x = c[0] - sc.half - sc.reach * sc.g + rng.uniform(0.02, 0.1, ch + 40) * sc.g
        yz = c[None, 1:] + rng.uniform(-0.45, 0.45, (ch + 40, 2)) * sc.bs
        for q in np.column_stack([x, yz]):
            sc.hit(q, "F")
    # the fillers, once every other sample stands (a long ray reaches into the next block's neighbourhood)
    for i, Lw in enumerate(R.stream_sizes(consts)):
        idx = shift + np.int64([sp * i, 0, 0])
        c0 = np.rint(sc.centre(idx).astype(np.float64) / sc.g).astype(np.int64)
        # the stream of the block's first cube (at depth <= 3: of its only cube)
        need = Lw - _count_in_cells(sc, c0 - sc.reach, c0 + sc.reach, 0)
        assert need >= 0, (Lw, need)
        if i == 3:                       # a whole chunk of fillers first: the boundary is a bucket boundary, sub-task 0 is culled
            before = ch - _count_in_cells(sc, c0 - sc.reach, c0 - sc.reach, 0)
        elif i == 5 and (2 * sc.reach + 1) ** 3 > consts["kLvGroup"]:
            # the first kLvGroup buckets end on the second sub-task boundary
            w = 2 * sc.reach + 1
            cc = sc.cidx(np.array(sc._smp, np.float64)[:, :3].astype(np.float32)) - (c0 - sc.reach)
            inside = ((cc >= 0) & (cc < w)).all(1)
            lin = (cc[:, 2] * w + cc[:, 1]) * w + cc[:, 0]
            before = 2 * ch - int((inside & (lin < consts["kLvGroup"])).sum())
        else:
            before = need // 2
        before = min(before, need)
        fillers(sc, idx, before, "first")
        fillers(sc, idx, need - before, "last" if sc.cubes == 1 else "second")
    return sc.pack()


def corner_pair(sc):
    """two voxels in opposite corners of the block's first cube, far enough apart that their boxes leave room in the outer box"""
    p = sc.lut_f[:min(64, sc.npb)].astype(np.float64)
    a = int(np.argmin(p.sum(1)))
    b = int(np.argmax(p.sum(1)))
    return a, b


def kept_scan(P, lut, consts):
    """(b), (c) at depth 3: one block per number of kept candidates (R.kept_sizes) with two active voxels in opposite
    corners — hits next to either, and hits that lie in the outer box but in neither voxel's box, interleaved; a block whose
    first round holds only such hits; and one block per number of rows in a split cube's sub-task (R.split_row_sizes): a
    chunk minus that many fillers, the rows (hits, every fifth a ray of one sample), and more than a chunk of fillers"""
    rng = np.random.default_rng(7)
    sc = LvScan(3, P, lut)
    ch, w = consts["kLvChunk"], consts["kWave"]
    sp = spacing(sc)
    a, b = corner_pair(sc)

    def pair_block(idx, kinds):
        act = np.zeros(sc.npb, bool)
        act[[a, b]] = True
        v = sc.voxels(idx).astype(np.float64)
        cross = np.where([True, False, True], v[a], v[b])
        for j, k in enumerate(kinds):
            if k == "U":
                sc.hit(cross + rng.uniform(-0.02, 0.02, 3), "U")
            elif k == "r":
                q = v[a if j % 2 else b] + rng.uniform(-0.03, 0.03, 3)
                sc.ray(q, q + _unit(rng) * 0.8, [0.0], "N")
            else:
                sc.hit(v[a if j % 2 else b] + rng.uniform(-0.03, 0.03, 3), "H")
        sc.block(idx, act, *_priors(rng, sc.npb))

    for i, K in enumerate(R.kept_sizes(consts)):
        kinds = ["U" if j % 3 == 1 else "r" if j % 7 == 3 else "H" for j in range(K)]
        pair_block(np.int64([sp * i, 0, 0]), kinds)
    pair_block(np.int64([0, sp, 0]), ["U"] * w + ["H"] * 5 + ["r"] * 3)            # a first round without a counted row
    pair_block(np.int64([sp, sp, 0]), ["r"] * w + ["H"] * (w + 3))                  # a round of ray rows, then hit rows twice
    for i, Rn in enumerate(R.split_row_sizes(consts)):
        idx = np.int64([sp * i, 2 * sp, 0])
        act = _active(rng, sc, "all" if i % 2 == 0 else 37)
        v = sc.voxels(idx)[act].astype(np.float64)
        fillers(sc, idx, ch - Rn, "first")
        for j in range(Rn):
            q = v[int(rng.integers(len(v)))] + rng.uniform(-0.03, 0.03, 3)
            if j % 5 == 4:
                sc.ray(q, q + _unit(rng) * 0.8, [0.0], "N")
            else:
                sc.hit(q, "H")
        fillers(sc, idx, ch + 7, "last")
        sc.block(idx, act, *_priors(rng, sc.npb))
    return sc.pack()


def dedupe_scan(depth, P, lut, shift=(0, 0, 0), heavy=False):
    """(d), (f): rays with one, two and many samples in a voxel's box, rays that start in the box and in the core box, rays
    whose samples come from other buckets and groups, samples in the outer box of a sparse cube but in no voxel's box, rows
    out of reach (k = sf2 g(1)), and a block with one active voxel whose only rows are such rays; segments of length 0,
    5e-5 and longer, voxels before the start, beyond the end and beside the segment"""
    rng = np.random.default_rng(300 + depth + int(10 * P["ell"]))
    sc = LvScan(depth, P, lut)
    sp = spacing(sc)
    shift = np.asarray(shift, np.int64)
    for i, how in enumerate(["all", 37, 1]):
        idx = shift + np.int64([sp * i, 0, 0])
        act = _active(rng, sc, how)
        tg = sc.voxels(idx)[act].astype(np.float64)
        if heavy:      # far from the origin a ray's bound is wide: a hit at every voxel keeps kbar clear of the gate
            for t in tg:
                sc.hit(t + rng.uniform(-0.02, 0.02, 3), "H")
        content(sc, rng, tg, list("BBBBSSSSNNNNMMMZZZZIIOOCCCHHHH"), short_ok=not heavy)
        sc.block(idx, act, *_priors(rng, sc.npb, heavy))
    # one active voxel, two rays past the edges of its box: HAS_INFO, kbar < 0, not updated
    idx = shift + np.int64([0, -4 * sp, 0])          # (out of every other block's rays' reach)
    act = _active(rng, sc, 1)
    act[64:] = False
    content(sc, rng, sc.voxels(idx)[act].astype(np.float64), "CC")
    sc.block(idx, act, *_priors(rng, sc.npb, heavy))
    # a block above all the others with one hit: the top of the grid, its neighbourhood sticks out
    idx = shift + np.int64([0, 0, 3 * sp])
    act = _active(rng, sc, "all")
    sc.hit(sc.voxels(idx)[0].astype(np.float64) + 0.01, "H")
    sc.block(idx, act, *_priors(rng, sc.npb, heavy))
    return sc.pack()


def face_cases():
    """(axis or 'corner', sign, on the face or one float beyond)"""
    return [(ax, s, on) for ax in (0, 1, 2, "corner") for s in (-1, 1) for on in (True, False)]


def face_scan(depth, P, lut, shift=(0, 0, 0)):
    """(e): one block per case of face_cases() with one active voxel and one hit whose coordinate on the axis (on all three
    for 'corner') is exactly fl(c + ell) or fl(c - ell), or the next float beyond, the others a little inside; and the same
    eight cases on the x axis and the corner with a ray instead: its segment runs through the voxel's centre, its start lies
    a metre outside, and its only other sample is the one on (or beyond) the face.  Returns the scan and, per block, the
    node and whether its box holds the sample."""
    f = np.float32
    rng = np.random.default_rng(11)
    sc = LvScan(depth, P, lut)
    sp = spacing(sc)
    shift = np.asarray(shift, np.int64)
    ell = f(P["ell"])
    want = []
    n = 0
    for as_ray in (False, True):
        for ax, s, on in face_cases():
            if as_ray and ax in (1, 2):
                continue
            idx = shift + np.int64([sp * (n % 8), sp * (n // 8), 0])
            n += 1
            act = np.zeros(sc.npb, bool)
            node = int(rng.integers(sc.npb))
            act[node] = True
            c = sc.voxels(idx)[node]
            face = (c + ell).astype(f) if s > 0 else (c - ell).astype(f)
            if not on:
                face = np.nextafter(face, f(np.inf) if s > 0 else f(-np.inf)).astype(f)
            p = (c.astype(np.float64) + rng.uniform(-0.1, 0.1, 3) * float(ell)).astype(f)
            axes = (0, 1, 2) if ax == "corner" else (ax,)
            if as_ray:
                p = c.copy()
            for a_ in axes:
                p[a_] = face[a_]
            if as_ray:
                d = (p.astype(np.float64) - c.astype(np.float64))
                d /= np.linalg.norm(d)
                start = p.astype(np.float64) + d * 1.0
                end = c.astype(np.float64) - d * 0.5
                k = sc.ray(start, end, [0.0], "X")
                start32 = sc._rays[k][:3]
                assert (np.sign(start32.astype(np.float64) - p)[list(axes)] == s).all()
                sc._smp.append([p[0], p[1], p[2], float(k)])
                sc._kinds.append("X")
            else:
                sc.hit(p, "X")
            b = sc.block(idx, act, [0.001], [0.001])
            want.append((b * sc.npb + node, on))
    return sc.pack(), want


def k_at(d, D):
    return D["sf2"] * float(R.g64(min(d / D["ell"], 1.0)))


def dist_for_k(k, D):
    """the distance on the falling flank of the kernel where a hit's k is the given value"""
    lo, hi = 0.0, D["ell"]
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if k_at(mid, D) > k else (lo, mid)
    return 0.5 * (lo + hi)


# (k of the one hit, alpha and beta after the update): both sides of the gate; A + B on either side of min_W with A > B and
# A < B — UNKNOWN exists only below min_W, where p is not 0 or 1 —; the last three carry rays out of reach (below)
NODE_CASES = [(0.00105, None, None), (0.00095, None, None), (0.002, 0.0002, 0.0001), (0.002, 0.0004, 0.0001),
              (0.002, 0.0001, 0.0004), (0.002, 0.00015, 0.0002), (0.002, 0.0007, 0.0005), (0.002, 0.0005, 0.0007),
              (0.004, 0.004, 0.0), (0.004, 0.004, 0.0), (0.004, 0.004, 0.0)]


def node_scan(depth, P, lut):
    """(g): one block per case of NODE_CASES with one active voxel and one weak hit on the +x side at the distance where its
    k is the wanted one; alpha carried in is the wanted alpha minus that k (negative where the sum is to stay below min_W:
    the kernel's input space, if not the map's).  The last three blocks add 6 rays past the edges of the box, 1.13 ell from
    the centre: beta = 6 sf2 g(1) = -2.9e-8, which a kernel clamped at 0 does not give."""
    rng = np.random.default_rng(13)
    sc = LvScan(depth, P, lut)
    sp = spacing(sc)
    D = R.derived(P)
    nodes = []
    for i, (k, A, B) in enumerate(NODE_CASES):
        idx = np.int64([sp * (i % 4), sp * (i // 4), 0])
        act = np.zeros(sc.npb, bool)
        node = int(rng.integers(sc.npb))
        act[node] = True
        c = sc.voxels(idx)[node].astype(np.float64)
        d = dist_for_k(k, D)
        sc.hit(c + np.float64([d, 0, 0]), "W")
        a0, b0 = (0.001, 0.001) if A is None else (A - k, B)
        if i >= len(NODE_CASES) - 3:
            content(sc, rng, c[None], "CCCCCC")
        b = sc.block(idx, act, [a0], [b0])
        nodes.append(b * sc.npb + node)
    return sc.pack(), nodes


def cubes_scan(n_cubes, P, lut, consts, depth=3):
    """(i): n_cubes cubes — blocks of depth 3 in a 5 x 5 x n arrangement, side by side (shared buckets) —, each with hits
    and a ray of its own; cubes 3, 20, 40 and 64 get more than a chunk of fillers: split cubes in several plan waves and
    plan workgroups.  The first n blocks of a larger scan are the blocks of the smaller one."""
    sc = LvScan(depth, P, lut)
    assert n_cubes % sc.cubes == 0
    ch = consts["kLvChunk"]
    for b in range(n_cubes // sc.cubes):
        rng = np.random.default_rng(5000 + b)
        idx = np.int64([2 * (b % 5), 2 * ((b // 5) % 5), 2 * (b // 25)])
        act = _active(rng, sc, "all" if b % 3 else 37)
        tg = sc.voxels(idx)[act].astype(np.float64)
        content(sc, rng, tg, "HHHBSNZ")
        if b in (3, 20, 40, 64):
            fillers(sc, idx, ch + 30 + b, "first")
        sc.block(idx, act, *_priors(rng, sc.npb))
    return sc.pack()


def one_block(sc, b):
    """the scan of block b alone, with all of sc's samples"""
    o = LvScan(sc.depth, sc.P, _lut_of(sc))
    o._smp, o._kinds, o._rays, o._ray_kinds = sc._smp, sc._kinds, sc._rays, sc._ray_kinds
    o._blocks = [sc._blocks[b]]
    return o.pack()


def from_arrays(depth, P, lut, samples, rays6, centres):
    """a scan of the given training data (samples [n, 4], segments [m, 6]) and block centres, every node a new leaf"""
    sc = LvScan(depth, P, lut)
    sc._smp = np.asarray(samples, np.float64).reshape(-1, 4).tolist()
    sc._kinds = ["H"] * len(sc._smp)
    sc._rays = list(np.asarray(rays6, np.float32).reshape(-1, 6))
    sc._ray_kinds = ["B"] * len(sc._rays)
    for c in np.asarray(centres, np.float64).reshape(-1, 3):
        sc.block(np.rint(c / sc.bs).astype(np.int64), np.ones(sc.npb, bool), [P["prior_A"]], [P["prior_B"]])
    return sc.pack()


def _lut_of(sc):
    """a depth-major table whose finest layer is sc's"""
    base = (8 ** (sc.depth - 1) - 1) // 7
    return np.concatenate([np.zeros((base, 3), np.float32), sc.lut_f])


# ---- the cases both test files run ---------------------------------------------------------------------------------------
FAR = (2000.0, -1500.0, 30.0)


def far_shift(depth, P):
    """FAR in whole blocks"""
    bs = float(np.float32(2 ** (depth - 1)) * np.float32(P["resolution"]))
    return tuple(int(round(v / bs)) for v in FAR)


CASES = [("stream", d, 0.2) for d in (2, 3, 4, 5)] + [("stream", d, 0.5) for d in (3, 4)] + [("stream", d, 0.9) for d in (2, 3)] + \
        [("stream far", d, 0.2) for d in (3, 4)] + [("kept", 3, 0.2)] + \
        [("dedupe", d, 0.2) for d in (2, 3, 4, 5)] + [("dedupe", 3, 0.5), ("dedupe", 3, 0.9), ("dedupe far", 3, 0.2), ("dedupe far", 4, 0.2)] + \
        [("face", d, 0.2) for d in (2, 3, 4, 5)] + [("face far", 3, 0.2), ("face", 3, 0.9)] + [("node", 3, 0.2), ("node", 5, 0.2)] + \
        [("cubes %d" % n, 3, 0.2) for n in (15, 16, 17, 63, 64, 65)] + [("cubes 16", 4, 0.2), ("cubes 64", 4, 0.5), ("cubes 64", 5, 0.2)]


def params(case, P0=None):
    return dict(P0 or R.LV_YAML, ell=case[2], block_depth=case[1])


def build_case(case, luts, consts):
    """(scan, extra) of a case of CASES: extra is face_scan's or node_scan's list, else None"""
    what, d, _ = case
    P = params(case)
    lut = luts[d]
    if what == "stream":
        return stream_scan(d, P, lut, consts), None
    if what == "stream far":
        return stream_scan(d, P, lut, consts, far_shift(d, P), True), None
    if what == "kept":
        return kept_scan(P, lut, consts), None
    if what == "dedupe":
        return dedupe_scan(d, P, lut), None
    if what == "dedupe far":
        return dedupe_scan(d, P, lut, far_shift(d, P), True), None
    if what == "face":
        return face_scan(d, P, lut)
    if what == "face far":
        return face_scan(d, P, lut, far_shift(d, P))
    if what == "node":
        return node_scan(d, P, lut)
    if what.startswith("cubes"):
        return cubes_scan(int(what.split()[1]), P, lut, consts, d), None
    raise ValueError(case)
