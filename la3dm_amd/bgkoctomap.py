"""Python mirror of la3dm::BGKOctoMap (reference include/bgkoctomap/bgkoctomap.h:26-367).

Same constructor argument order, same method names and argument meaning as the C++
class; all work is done by libla3dm_map.so (host bookkeeping, C++) and
libla3dm_hip.so (HIP kernels).  No Python compute path exists.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _lib

FREE, OCCUPIED, UNKNOWN, PRUNED = 0, 1, 2, 3
# raycast_many: class of a row whose block does not exist (a covering leaf is never PRUNED, so the slot is free), ray flags
MISSING = 3
RAY_HIT, RAY_TRUNCATED, RAY_INVALID = 1, 2, 4
DF_FAR = 0xFFFFFFFF                 # LA3DM_DF_FAR: beyond the radius of distance_field (dist: +inf)
FR_MAX_CELLS = 1 << 28             # LA3DM_FR_MAX_CELLS: voxels of frontier's region padded by one on every side
DIFF_PAIRS_CHANGED = 0x0FBEFBE      # LA3DM_DIFF_PAIRS_CHANGED: the 20 (then, now) pairs with then != now, bit 5 * then + now
GAIN_MAX_CELLS = GAIN_MAX_RAYS = GAIN_MAX_WORDS = 1 << 28   # LA3DM_GAIN_MAX_*: voxels of gain's region, n * m rays, n * W set words
SCORE_MAX_CELLS, SCORE_MAX_POINTS, SCORE_MAX_POSES, SCORE_MAX_PAIRS, SCORE_MAX_RADIUS = 1 << 28, 1 << 20, 1 << 20, 1 << 32, 255   # LA3DM_SCORE_MAX_*
SCORE_HIT, SCORE_NEAR, SCORE_FAR, SCORE_OUTSIDE, SCORE_INVALID = range(5)   # LA3DM_SCORE_*: the columns of score_poses' counts
NEAREST_NONE, NEAREST_MAX_RADIUS = 0xFFFFFFFF, 255   # LA3DM_NEAREST_*: nearest found no obstacle within the radius; the largest radius
FOOTING_MAX_CELLS, FOOTING_MAX_HEADROOM, FOOTING_MAX_RADIUS, FOOTING_MAX_STEP = 1 << 28, 32, 8, 4   # LA3DM_FOOTING_MAX_*
SURFACE_MAX_CELLS, SURFACE_MAX_SMOOTH = 1 << 28, 4   # LA3DM_SURFACE_MAX_*
PATH_BLOCKED, PATH_LEFT, PATH_TRUNCATED, PATH_INVALID = 1, 2, 4, 8   # LA3DM_PATH_*: the bits of score_paths' flags
PATH_NONE = 0xFFFFFFFF              # LA3DM_PATH_NONE: score_paths' stop of a walk that did not stop
PATHS_MAX_STEPS, PATHS_MAX_WAY, PATHS_MAX_PATHS, PATHS_MAX_WAYPOINTS = 1 << 20, 1024, 1 << 20, 1 << 26   # LA3DM_PATHS_MAX_*
REACH_NONE = 0xFFFFFFFF             # LA3DM_REACH_NONE: reach found no walk to the voxel
REACH_MAX_CELLS, REACH_MAX_STEPS, REACH_MAX_SEEDS = 1 << 28, 1 << 16, 1 << 20   # LA3DM_REACH_MAX_*: padded voxels, max_steps, seeds
REACH_BATCH = 32                    # LA3DM_REACH_BATCH: level launches queued between two reads of the level counts
TRAVEL_NONE = 0xFFFFFFFF            # LA3DM_TRAVEL_NONE: travel found no walk to the voxel
TRAVEL_MAX_CELLS, TRAVEL_MAX_COST, TRAVEL_MAX_SEEDS, TRAVEL_MAX_ROUNDS = 1 << 28, 1 << 31, 1 << 20, 1 << 16   # LA3DM_TRAVEL_MAX_*
TRAVEL_MAX_MOVE = TRAVEL_MAX_PENALTY = 1 << 16
TRAVEL_BRICK, TRAVEL_INNER, TRAVEL_BATCH = 8, 16, 8   # LA3DM_TRAVEL_*: a brick's edge, iterations of one brick run, rounds queued between two reads of the counts
DRIVE_NONE = 0xFFFFFFFF             # LA3DM_DRIVE_NONE: a non-member, or a member drive found no walk to
DRIVE_MAX_CELLS, DRIVE_MAX_MEMBERS, DRIVE_MAX_SEEDS, DRIVE_MAX_ROUNDS = 1 << 28, 1 << 28, 1 << 20, 1 << 16   # LA3DM_DRIVE_MAX_*
DRIVE_MAX_STEP, DRIVE_MAX_SNAP = 4, 32   # voxels a move may climb or drop; voxels a seed or target may lie above its member
DRIVE_BRICK, DRIVE_INNER, DRIVE_BATCH = 8, 16, 8   # LA3DM_DRIVE_*: as travel's
DRIVE_SEED_CODE = 40                # drive's parent code of a seeded member: the offset (0, 0, 0)
CLUSTERS_NONE = 0xFFFFFFFF          # LA3DM_CLUSTERS_NONE: a non-member, or a member of a dropped cluster
CLUSTERS_MAX_CELLS, CLUSTERS_MAX_MEMBERS, CLUSTERS_MAX_ROUNDS = 1 << 28, 1 << 28, 1 << 16   # LA3DM_CLUSTERS_MAX_*
CLUSTERS_MAX_AXIS = CLUSTERS_MAX_TILE = 1 << 15
CLUSTERS_BRICK, CLUSTERS_INNER, CLUSTERS_BATCH = 8, 16, 8   # LA3DM_CLUSTERS_*: as travel's
_RAY_CLASS = dict(free=FREE, occupied=OCCUPIED, unknown=UNKNOWN, missing=MISSING, uncertain=4)


# -- the decisions the query methods share ---------------------------------------
def _class_mask(x):
    """a class name, an iterable of class names or an integer -> the bit mask (an unknown name: KeyError)"""
    if isinstance(x, (int, np.integer)):
        return int(x)
    return sum(1 << _RAY_CLASS[k] for k in ({x} if isinstance(x, str) else set(x)))


def _pair_mask(pairs):
    """diff's `pairs` -> the mask of (then, now) pairs, bit 5 * then + now"""
    if isinstance(pairs, str):
        if pairs != "changed":
            raise ValueError('diff: pairs is "changed", an integer mask or an iterable of (then, now) class names')
        return DIFF_PAIRS_CHANGED
    if isinstance(pairs, (int, np.integer)):
        return int(pairs)
    mask = 0
    for then, now in pairs:
        mask |= 1 << (5 * _RAY_CLASS[then] + _RAY_CLASS[now])
    return mask


def _want(who, fields, allowed):
    """`fields` (one name or several) as a tuple, every name out of `allowed`"""
    if isinstance(fields, str):
        fields = (fields,)
    bad = set(fields) - set(allowed)
    if bad:
        raise ValueError(f"{who}: unknown fields {sorted(bad)}")
    return tuple(fields)


def _fit(msg, values, bits=32):
    """ValueError(msg) unless every value fits an unsigned integer of `bits` bits"""
    for v in values:
        if not 0 <= int(v) < 1 << bits:
            raise ValueError(msg)


def _addr(a):
    """the address of an array for a C call; NULL for None and for an empty array"""
    return a.ctypes.data if a is not None and a.size else None


def _out(X, arrays, null_empty=()):
    """the out struct X with the address of arrays[k] in field k: NULL where the key is missing, and for the keys in
    `null_empty` also where the array is empty (elsewhere an empty array goes by its address: the C calls refuse a NULL
    mandatory output, e.g. raycast_many's steps or gain's gain, whatever the count)"""
    ptrs = []
    for k, _ in X._fields_:
        a = arrays.get(k)
        ptrs.append(None if a is None or (not a.size and k in null_empty) else a.ctypes.data)
    return X(*ptrs)


def _stream(stream):
    """a map stream (bytes or a uint8 array) as a flat uint8 array"""
    return np.ascontiguousarray(np.frombuffer(stream, np.uint8) if isinstance(stream, (bytes, bytearray, memoryview)) else stream,
                                np.uint8).reshape(-1)


def _indices(seeds, targets):
    """reach's and travel's flat index lists: seeds, targets (or None), the number of targets"""
    s = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
    t = None if targets is None else np.ascontiguousarray(targets, np.uint32).reshape(-1)
    return s, t, 0 if t is None else t.size


class PackedScan:
    """Host view of one prepared scan (numpy arrays aliasing the map's buffers)."""

    def __init__(self, s: _lib.BgkScan):
        self.c = s

        def arr(ptr, n, dt):
            if not ptr or n == 0:
                return np.zeros(0, dt)
            buf = (C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dt, count=n)

        self.train_xyzy = arr(s.train_xyzy, 4 * s.n_train_pts, np.float32).reshape(-1, 4)
        self.train_off = arr(s.train_off, s.n_train_blk + 1, np.uint32)
        self.nbr = arr(s.nbr, 7 * s.n_test_blk, np.int32).reshape(-1, 7)
        self.blk_center = arr(s.blk_center, 3 * s.n_test_blk, np.float32).reshape(-1, 3)
        self.leaf_off = arr(s.leaf_off, s.n_test_blk + 1, np.uint32)
        self.leaf_key = arr(s.leaf_key, s.n_leaf, np.uint32)
        self.alpha = arr(s.alpha, s.n_leaf, np.float32)
        self.beta = arr(s.beta, s.n_leaf, np.float32)
        self.state = arr(s.state, s.n_leaf, np.uint8)
        self.flags = s.flags
        self.n_test_blk = s.n_test_blk
        self.n_leaf = s.n_leaf
        self.n_train_pts = s.n_train_pts
        self.n_train_blk = s.n_train_blk


class BGKOctoMap:
    def __init__(self, resolution=0.1, block_depth=4, sf2=1.0, ell=1.0, free_thresh=0.3, occupied_thresh=0.7,
                 var_thresh=1.0, prior_A=1.0, prior_B=1.0, device=0):
        self._M = _lib.maplib()
        self._h = self._M.la3dm_map_create(resolution, block_depth, sf2, ell, free_thresh, occupied_thresh,
                                           var_thresh, prior_A, prior_B, device)
        if not self._h:
            raise RuntimeError(self._M.la3dm_map_last_error().decode())
        self.resolution = resolution
        self.block_depth = block_depth
        self.device = device

    _gp = False

    def set_device_resident(self, on=True):
        """Device-resident mode: the block pool lives in HBM and insert_pointcloud runs start to finish on the
        GPU (front end, partition, predict + fuse, write-back, prune); queries refresh a host mirror lazily."""
        self._chk(self._M.la3dm_map_set_device_resident(self._h, 1 if on else 0))
        return self

    def is_device_resident(self):
        return bool(self._M.la3dm_map_is_device_resident(self._h))

    def set_shard(self, rank, world, allgatherv):
        """Block-sharded insert_pointcloud over `world` replicas of this map, one process per GPU (every process
        inserts the same clouds): rank r predicts + fuses its contiguous range of the test blocks, then
        `allgatherv(segments, world, rank, stream)` is called once per pass — segments = [(base_ptr, offsets, nbytes), ...]
        (four: the scan's alpha, beta, state and leaf-key arrays; rank q owns bytes [offsets[q], offsets[q] + nbytes[q]) of each)
        — and must queue, on the HIP stream `stream` (an integer handle) or ordered against it, an in-place
        all-gather-v of every segment; nothing synchronises the host (la3dm_devmap_set_shard in include/la3dm_hip.h;
        la3dm_amd.sharding.torch_allgather builds one on torch.distributed).  world = 1 switches it off."""
        self._shard_error = None

        def _cb(user, segs, nseg, nranks, r, stream):
            try:
                seg_list = [(int(segs[i].base), [int(segs[i].offset[q]) for q in range(nranks)],
                             [int(segs[i].bytes[q]) for q in range(nranks)]) for i in range(nseg)]
                allgatherv(seg_list, int(nranks), int(r), int(stream or 0))
                return 0
            except Exception as e:           # never let an exception cross the C boundary
                self._shard_error = e
                return 1
        self._shard_cb = _lib.ALLGATHER_FN(_cb) if world > 1 else _lib.ALLGATHER_FN(0)
        self._chk(self._M.la3dm_map_set_shard(self._h, rank, world, self._shard_cb, None))
        return self

    def __del__(self):
        if getattr(self, "_h", None):
            self._M.la3dm_map_destroy(self._h)
            self._h = None

    def _chk(self, rc):
        if rc < 0:
            err, self._shard_error = getattr(self, "_shard_error", None), None
            if err is not None:          # the all-gather callback raised: that is the cause
                raise RuntimeError(self._M.la3dm_map_last_error().decode()) from err
            raise RuntimeError(self._M.la3dm_map_last_error().decode())
        return rc

    # -- reference API ------------------------------------------------------
    def get_resolution(self):
        return self._M.la3dm_map_resolution(self._h)

    def get_block_depth(self):
        return self._M.la3dm_map_block_depth(self._h)

    def set_resolution(self, resolution):
        """BGKOctoMap::set_resolution (reference src/bgkoctomap/bgkoctomap.cpp:66-72): empty maps only (RuntimeError otherwise)"""
        self._chk(self._M.la3dm_map_set_resolution(self._h, float(resolution)))
        self.resolution = self.get_resolution()
        return self

    def set_block_depth(self, block_depth):
        """BGKOctoMap::set_block_depth (reference src/bgkoctomap/bgkoctomap.cpp:74-80): empty maps only (RuntimeError otherwise)"""
        self._chk(self._M.la3dm_map_set_block_depth(self._h, int(block_depth)))
        self.block_depth = self.get_block_depth()
        return self

    def get_block_size(self):
        return self._M.la3dm_map_block_size(self._h)

    def insert_pointcloud(self, cloud, origin, ds_resolution, free_res=2.0, max_range=-1.0):
        """BGKOctoMap::insert_pointcloud(cloud, origin, ds_resolution, free_res, max_range)
        (include/bgkoctomap/bgkoctomap.h:82-84, src/bgkoctomap/bgkoctomap.cpp:214-366): ds_resolution < 0 skips the
        voxel-grid filter, max_range <= 0 the range gate; an empty training set is a silent no-op."""
        xyz = np.ascontiguousarray(cloud, np.float32).reshape(-1, 3)
        o = np.ascontiguousarray(origin, np.float32)
        self._chk(self._M.la3dm_map_insert_pointcloud(self._h, xyz, xyz.shape[0], o, ds_resolution, free_res,
                                                      max_range))

    def insert_pointcloud_device(self, d_xyz, n, origin, ds_resolution, free_res=2.0, max_range=-1.0):
        """insert_pointcloud for a cloud already in HBM: d_xyz = device address of n packed float32 xyz triples on the
        map's GPU (e.g. torch_tensor.data_ptr() of a contiguous (n, 3) float32 CUDA tensor); device-resident maps only.
        The insert runs on the library's own stream: the cloud must be complete before the call — synchronise the stream
        that produced it (torch.cuda.current_stream().synchronize()) or order the insert behind a hipEvent with
        la3dm_devmap_wait_event (include/la3dm_hip.h)."""
        o = np.ascontiguousarray(origin, np.float32)
        self._chk(self._M.la3dm_map_insert_pointcloud_device(self._h, int(d_xyz), int(n), o, ds_resolution, free_res, max_range))
        return self

    def insert_training_data(self, xyzy):
        """BGKOctoMap::insert_training_data(GPPointCloud) (bgkoctomap.h:86, bgkoctomap.cpp:82-212): rows x, y, z, label;
        every leaf of every test block is updated (no kbar gate)."""
        a = np.ascontiguousarray(xyzy, np.float32).reshape(-1, 4)
        self._chk(self._M.la3dm_map_insert_training_data(self._h, a, a.shape[0]))

    def get_bbox(self):
        """BGKOctoMap::get_bbox (bgkoctomap.h:89, bgkoctomap.cpp:368-381): block centres +- half a block"""
        lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._M.la3dm_map_get_bbox(self._h, lo, hi)
        return lo, hi

    def search(self, x, y, z):
        """BGKOctoMap::search(x, y, z) (bgkoctomap.h:315-319, bgkoctomap.cpp:554-567) -> (exists, alpha, beta, state)"""
        a, b, s = C.c_float(), C.c_float(), C.c_uint8()
        e = self._M.la3dm_map_search(self._h, x, y, z, C.byref(a), C.byref(b), C.byref(s))
        return bool(e), a.value, b.value, s.value

    def search_many(self, points):
        """search(x, y, z) for an (n, 3) array of points -> dict(exists, A, B, state); a device-resident map answers
        from the device pool (no host mirror refresh)"""
        q = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = q.shape[0]
        out = dict(exists=np.zeros(n, np.uint8), A=np.zeros(n, np.float32), B=np.zeros(n, np.float32),
                   state=np.zeros(n, np.uint8))
        self._chk(self._M.la3dm_map_search_many(self._h, q, n, *[out[k].ctypes.data for k in ("exists", "A", "B", "state")]))
        return out

    def raycast(self, start, end, cap=4096):
        """RayCaster(map, start, end) driven to its end: dict of p, block_key, node_key, valid, A, B, state per step."""
        s3, e3 = np.ascontiguousarray(start, np.float32), np.ascontiguousarray(end, np.float32)
        out = dict(p=np.zeros((cap, 3), np.float32), block_key=np.zeros(cap, np.int64), node_key=np.zeros(cap, np.int32),
                   valid=np.zeros(cap, np.uint8), A=np.zeros(cap, np.float32), B=np.zeros(cap, np.float32),
                   state=np.zeros(cap, np.uint8))
        n = self._M.la3dm_map_raycast(self._h, s3, e3, *[out[k].ctypes.data for k in
                                                          ("p", "block_key", "node_key", "valid", "A", "B", "state")], cap)
        n = min(int(n), cap)
        return {k: v[:n] for k, v in out.items()}

    def raycast_many(self, starts, ends, stop=("occupied",), max_steps=4096):
        """The client loop over a RayCaster for n segments starts[i] -> ends[i] at once: every ray is walked until it
        ends, produced `max_steps` rows (flags & RAY_TRUNCATED) or met a row whose class is in `stop` (flags & RAY_HIT).
        The class of a row is the state of the COVERING LEAF of its voxel (after prune() the raw finest-layer node of a
        collapsed region reads PRUNED; the answer lives in an ancestor) or MISSING where the block does not exist.
        stop: names out of free / occupied / unknown / missing (/ uncertain on a BGK-LV map), or an integer bit mask;
        () walks to the end and only counts.  Returns a dict of arrays: steps (rows), flags, and of the last row p,
        block_key, node_key, cls, leaf_depth, A, B; counts (n, 4) = rows per class FREE, OCCUPIED, UNKNOWN, MISSING.
        A device-resident map runs one HIP launch on the device pool (no host mirror refresh); a host-mode map runs
        the loop on the host, with bit-identical results."""
        s = np.ascontiguousarray(starts, np.float32).reshape(-1, 3)
        e = np.ascontiguousarray(ends, np.float32).reshape(-1, 3)
        if s.shape != e.shape:
            raise ValueError("raycast_many: starts and ends differ in shape")
        mask = _class_mask(stop)
        n = s.shape[0]
        rays = np.ascontiguousarray(np.hstack([s, e]))
        out = dict(steps=np.zeros(n, np.uint32), flags=np.zeros(n, np.uint8), p=np.zeros((n, 3), np.float32),
                   block_key=np.zeros(n, np.int64), node_key=np.zeros(n, np.int32), cls=np.zeros(n, np.uint8),
                   leaf_depth=np.zeros(n, np.uint8), A=np.zeros(n, np.float32), B=np.zeros(n, np.float32),
                   counts=np.zeros((n, 4), np.uint32))
        self._chk(self._M.la3dm_map_raycast_many(self._h, rays, n, mask, int(max_steps), C.byref(_out(_lib.RaycastOut, out))))
        return out

    @staticmethod
    def _region(lo, dims, served):
        """(lo and dims as C arrays, dims, their product, whether the C call is expected to serve the request: served(dims)
        and no zero dimension).  A request that is not served still goes to the C call, with one-element output arrays —
        the call refuses it before it looks at a buffer, and its text is the one that is raised"""
        lo3 = np.ascontiguousarray(lo, np.float32).reshape(-1)
        d = [int(v) for v in np.asarray(dims).reshape(-1)]
        if lo3.shape != (3,) or len(d) != 3 or min(d) < 0 or max(d) >= 2 ** 32:
            raise ValueError("lo must be 3 floats and dims 3 integers in [0, 2^32)")
        return lo3, np.array(d, np.uint32), d, d[0] * d[1] * d[2], bool(min(d) > 0 and served(d))

    def _region_call(self, fn, lo3, d3, *args):
        """fn(handle, lo, dims, *args, info), checked -> origin, block_key and cell of voxel (0, 0, 0)"""
        info = _lib.RegionInfo()
        self._chk(fn(self._h, lo3.ctypes.data, d3.ctypes.data, *args, C.byref(info)))
        return dict(origin=np.array(info.origin[:], np.float32), block_key=int(info.block_key),
                    cell=np.array(info.cell[:], np.int32))

    def box(self, lo, dims, fields=("cls", "leaf_depth", "A", "B")):
        """The voxels of an axis-aligned box as dense arrays of shape dims = (nx, ny, nz).  Voxel (0, 0, 0) is the voxel
        that holds the world point `lo` (resolved as the RayCaster resolves its start point); voxel (i, j, k) lies i, j, k
        cells of the finest-layer lattice further along x, y, z, across block borders.  Per voxel: cls = the state of
        its COVERING LEAF (FREE, OCCUPIED, UNKNOWN, MISSING where the block does not exist, 4 = UNCERTAIN on a BGK-LV
        map; never PRUNED — after prune() the raw node of a collapsed region reads PRUNED and search() reports that),
        leaf_depth = that leaf's layer (255: missing), A / B = its node values (m_ivar / ivar on a GP map; the default
        node: missing).  `fields` names the arrays wanted; cls always comes.  Also returned: origin = the centre of
        voxel (0, 0, 0) (the others: origin + (i, j, k) * resolution), block_key and cell of that voxel.  At most 2^30
        voxels.  A device-resident map runs one HIP launch on the device pool (no host mirror refresh); a host-mode map
        loops over its host blocks, with bit-identical results."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: d[0] * d[1] * d[2] <= 2 ** 30)
        shape = tuple(d) if ok else (1,)
        fields = _want("box", fields, ("cls", "leaf_depth", "A", "B"))
        out = {k: np.empty(shape, np.float32 if k in "AB" else np.uint8) for k in ("cls", "leaf_depth", "A", "B")
               if k == "cls" or k in fields}
        out.update(self._region_call(self._M.la3dm_map_box, lo3, d3, C.byref(_out(_lib.BoxOut, out))))
        return out

    def columns(self, lo, dims):
        """The box of box(lo, dims) reduced along z, without building it: per (x, y) column counts (nx, ny, 4) = voxels of
        class FREE, OCCUPIED, UNKNOWN (with UNCERTAIN), MISSING over k = 0 .. nz - 1 (they sum to nz), low_occ / top_occ
        (nx, ny) = the smallest / largest k whose class is OCCUPIED, -1 when there is none; plus origin, block_key, cell
        as box() returns them.  The 2-D occupancy grid / height map of a height band.  At most 2^30 columns, nz <= 2^16."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: d[0] * d[1] <= 2 ** 30 and d[2] <= 2 ** 16)
        shape = (d[0], d[1]) if ok else (1,)
        out = dict(counts=np.empty(shape + (4,), np.uint32), low_occ=np.empty(shape, np.int32), top_occ=np.empty(shape, np.int32))
        out.update(self._region_call(self._M.la3dm_map_columns, lo3, d3, C.byref(_out(_lib.ColumnsOut, out))))
        return out

    def distance_field(self, lo, dims, obstacles=("occupied",), radius=32, fields=("d2", "dist")):
        """The exact Euclidean distance transform of the region of box(lo, dims): per voxel the distance to the nearest
        obstacle INSIDE THE REGION, an obstacle being a voxel whose class (box's cls) is in `obstacles` — names out of
        free / occupied / unknown / missing (/ uncertain on a BGK-LV map) or an integer bit mask, as raycast_many's
        `stop`.  d2 (uint32) = the squared distance in voxel units, an integer, 0 on the obstacles and DF_FAR
        (0xFFFFFFFF) beyond radius^2 or where the region holds no obstacle; dist (float32) = sqrt(d2) * resolution in
        metres, +inf for FAR.  radius: 1 .. 1024 voxels.  Obstacles outside the region are not seen: pad the region by
        `radius` where that matters.  The distance inside obstacles is the call with the complementary classes.
        `fields` names the arrays wanted (at least one).  Also returned: origin, block_key, cell as box() returns them.
        At most 2^28 voxels.  A device-resident map runs the transform on the device pool (no host mirror refresh); a
        host-mode map runs it on the CPU, with bit-identical results."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: d[0] * d[1] * d[2] <= 2 ** 28)
        shape = tuple(d) if ok else (1,)
        fields = _want("distance_field", fields, ("d2", "dist"))
        mask = _class_mask(obstacles)
        _fit("distance_field: obstacles and radius must fit 32 bits", (mask, radius))
        out = {k: np.empty(shape, t) for k, t in (("d2", np.uint32), ("dist", np.float32)) if k in fields}
        out.update(self._region_call(self._M.la3dm_map_distance_field, lo3, d3, mask, int(radius), C.byref(_out(_lib.DistanceOut, out))))
        return out

    def frontier(self, lo, dims, open=("free",), unknown=("unknown", "missing"), connectivity=6, min_neighbours=1,
                 fields=("index", "nbrs"), cap=None):
        """The frontier of the region of box(lo, dims) as an ordered list: the voxels whose class (box's cls) is in `open`
        and that have at least `min_neighbours` neighbours whose class is in `unknown` — names out of free / occupied /
        unknown / missing (/ uncertain on a BGK-LV map) or an integer bit mask, as raycast_many's `stop`; the masks may
        overlap.  connectivity: 6 (faces), 18 (+ edges) or 26 (+ corners).  The neighbours one step outside the region are
        read from the map, so a frontier voxel on a face of the region is found.  Returns n = the number of frontier
        voxels, index (uint32) = their flat indices (i * ny + j) * nz + k in ascending order (np.unravel_index(index, dims)
        gives i, j, k), nbrs (uint8) = their scores (the number of such neighbours), and with "score" in `fields` the
        dense score (uint8, shape dims; 0 where the voxel is not open); plus origin, block_key, cell as box() returns
        them.  cap=None counts first and then fills exactly n entries; an integer cap fills the first min(n, cap) and n is
        still the total.  At most 2^28 voxels in the region padded by one.  A device-resident map runs the query on the
        device pool (no host mirror refresh); a host-mode map runs it on the CPU, with identical results."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: (d[0] + 2) * (d[1] + 2) * (d[2] + 2) <= 2 ** 28)
        fields = _want("frontier", fields, ("index", "nbrs", "score"))
        masks = [_class_mask(open), _class_mask(unknown)]
        _fit("frontier: open, unknown, connectivity and min_neighbours must fit 32 bits", masks + [connectivity, min_neighbours])
        if cap is not None:
            _fit("frontier: cap must fit 64 bits", [cap], bits=64)
        found = C.c_uint64(0)
        region = {}

        def call(k, arrays):
            o = _out(_lib.FrontierOut, arrays, null_empty=("index", "nbrs"))
            region.update(self._region_call(self._M.la3dm_map_frontier, lo3, d3, masks[0], masks[1], int(connectivity), int(min_neighbours),
                                            k, C.byref(o) if arrays else None, C.byref(found)))
            return int(found.value)

        out = {}
        if "score" in fields:
            out["score"] = np.empty(tuple(d) if ok else (1,), np.uint8)
        if cap is None:   # the two-call protocol: count (the dense score comes with this call), then fill exactly n
            k = call(0, out)
            filled = {}
        else:
            k = min(int(cap), cells if ok else 1)
            filled = dict(out)
        filled.update(index=np.empty(k, np.uint32), nbrs=np.empty(k, np.uint8))
        total = k
        if cap is not None or k:
            total = call(k, filled)
        m = min(total, k)
        out.update(index=filled["index"][:m], nbrs=filled["nbrs"][:m], n=total)
        out.update(region)
        return out

    def gain(self, lo, dims, origins, offsets, count=("unknown", "missing"), stop=("occupied",), max_steps=4096, fields=("gain",)):
        """The information gain of n candidate viewpoints: per viewpoint origins[v] the number of DISTINCT voxels of the
        region of box(lo, dims) that the m segments origins[v] -> origins[v] + offsets[d] walk over and whose class is in
        `count`.  Every segment is walked exactly as raycast_many(stop=stop, max_steps=max_steps) walks it; every row it
        produces, the stopping row included, marks its voxel if the voxel lies in the region and its class is in `count`.
        offsets (m, 3) are metres in the map frame, shared by all viewpoints: the caller's sensor pattern.  count / stop:
        names out of free / occupied / unknown / missing (/ uncertain on a BGK-LV map) or an integer bit mask, as
        frontier takes them; stop=() walks every ray to its end.  Returns a dict: gain (n,) uint32 and, when named in
        `fields`, started / hits (n,) = the rays of the viewpoint that produced a row / ended on a stop row, seen (n, W)
        uint32 = the sets themselves, bit f % 32 of word f // 32 for the flat index f = (i * ny + j) * nz + k, W =
        ceil(nx ny nz / 32); plus origin, block_key, cell as box() returns them.  At most 2^28 voxels, n * m <= 2^28 rays
        and n * W <= 2^28 words.  A device-resident map runs the query on the device pool (no host mirror refresh); a
        host-mode map runs it on the CPU, with identical results."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: d[0] * d[1] * d[2] <= GAIN_MAX_CELLS)
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(offsets, np.float32).reshape(-1, 3)
        fields = _want("gain", fields, ("gain", "started", "hits", "seen"))
        masks = [_class_mask(count), _class_mask(stop)]
        n, m, W = o.shape[0], f.shape[0], (cells + 31) // 32
        _fit("gain: count, stop, max_steps and the numbers of origins and offsets must fit 32 bits", masks + [max_steps, n, m])
        ok = ok and m > 0 and n * m <= GAIN_MAX_RAYS and n * W <= GAIN_MAX_WORDS
        out = {k: np.empty(n if ok else 1, np.uint32) for k in ("gain", "started", "hits") if k == "gain" or k in fields}
        if "seen" in fields:
            out["seen"] = np.empty((n, W) if ok else (1,), np.uint32)
        out.update(self._region_call(self._M.la3dm_map_gain, lo3, d3, _addr(o), n, _addr(f), m, masks[0], masks[1], int(max_steps),
                                     C.byref(_out(_lib.GainOut, out))))
        return out

    def score_poses(self, lo, dims, points, poses, obstacles=("occupied",), radius=16, fields=("sum_d2", "counts")):
        """Likelihood-field scoring of one scan under P candidate poses: every point of `points` (n, 3; sensor frame) is
        moved by every pose of `poses` (P, 3, 4) or (P, 12), row-major [R | t], in float32 — w[c] = ((R[c][0] x + R[c][1] y)
        + R[c][2] z) + t[c], every operation rounded on its own — its voxel resolved as search resolves it, and d2 =
        distance_field(lo, dims, obstacles, radius) gathered there.  Returns a dict: sum_d2 (P,) uint64 = per pose the sum
        of the finite d2, and, when named in `fields`, counts (P, 5) uint32 = its pairs of class HIT (d2 = 0), NEAR (d2
        finite), FAR (beyond radius), OUTSIDE (the voxel is not in the region), INVALID (a coordinate the lattice cannot
        hold: NaN, inf, |w / resolution| >= 2^30) — they sum to n; plus origin, block_key, cell as box() returns them.
        A score is the caller's to compose, e.g. sum_d2 + penalty * (far + outside).  obstacles: as distance_field takes
        them; radius: 1 .. 255 voxels.  Obstacles outside the region are not seen.  At most 2^28 voxels, 2^20 points, 2^20
        poses and 2^32 pairs.  A device-resident map runs the query on the device pool (no host mirror refresh); a
        host-mode map runs it on the CPU, with identical results."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: d[0] * d[1] * d[2] <= SCORE_MAX_CELLS)
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        T = np.ascontiguousarray(poses, np.float32)
        if T.ndim < 2 or T.shape[1:] not in ((3, 4), (12,)):
            raise ValueError("score_poses: poses must have the shape (P, 3, 4) or (P, 12)")
        T = T.reshape(-1, 12)
        fields = _want("score_poses", fields, ("sum_d2", "counts"))
        mask = _class_mask(obstacles)
        n, P = pts.shape[0], T.shape[0]
        _fit("score_poses: obstacles, radius and the numbers of points and poses must fit 32 bits", (mask, radius, n, P))
        ok = ok and n <= SCORE_MAX_POINTS and P <= SCORE_MAX_POSES and n * P <= SCORE_MAX_PAIRS
        out = dict(sum_d2=np.empty(P if ok else 1, np.uint64))
        if "counts" in fields:
            out["counts"] = np.empty((P, 5) if ok else (1, 5), np.uint32)
        out.update(self._region_call(self._M.la3dm_map_score_poses, lo3, d3, _addr(pts), n, _addr(T), P, mask, int(radius),
                                     C.byref(_out(_lib.ScoreOut, out))))
        return out

    def nearest(self, lo, dims, obstacles=("occupied",), radius=16, fields=("index", "d2")):
        """WHICH obstacle is the nearest: per voxel of the region of box(lo, dims) index (uint32, shape dims) = the flat index
        (i * ny + j) * nz + k of the nearest voxel of the region whose class is in `obstacles` — the smallest flat index among
        obstacles at the same distance, the voxel's own index on an obstacle, NEAREST_NONE beyond `radius` voxels — and d2
        (uint32) = exactly distance_field(lo, dims, obstacles, radius)'s d2.  np.unravel_index(index, dims) gives the
        obstacle's (i', j', k'); v - nearest(v) is the direction away from it.  obstacles: as distance_field takes them;
        radius: 1 .. 255 voxels.  Obstacles outside the region are not seen: pad the region by `radius` where that matters.
        `fields` names the arrays wanted (at least one).  Also returned: origin, block_key, cell as box() returns them.  At
        most 2^28 voxels.  A device-resident map runs the query on the device pool (no host mirror refresh); a host-mode map
        runs it on the CPU, with identical results."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: d[0] * d[1] * d[2] <= 1 << 28)
        fields = _want("nearest", fields, ("index", "d2"))
        mask = _class_mask(obstacles)
        _fit("nearest: obstacles and radius must fit 32 bits", (mask, radius))
        out = {k: np.empty(tuple(d) if ok else (1,), np.uint32) for k in ("index", "d2") if k in fields}
        out.update(self._region_call(self._M.la3dm_map_nearest, lo3, d3, mask, int(radius), C.byref(_out(_lib.NearestOut, out))))
        return out

    _NEAREST_POINTS_FIELDS = dict(cls=np.uint8, voxel=np.uint32, index=np.uint32, d2=np.uint32)

    def nearest_points(self, lo, dims, points, pose=None, obstacles=("occupied",), radius=16, fields=("cls", "voxel", "index", "d2")):
        """nearest() per point of a cloud — the correspondences of an ICP step.  Every point of `points` (n, 3) is moved by
        `pose` ((3, 4) or (12,), row-major [R | t], float32 and op by op as score_poses moves it; None: the points are taken
        as they are, in the map frame), its voxel resolved as search resolves it.  Returns a dict of (n,) arrays, those named
        in `fields`: cls uint8 = the point's class as score_poses counts it (SCORE_HIT: on an obstacle, SCORE_NEAR: one within
        `radius` voxels, SCORE_FAR, SCORE_OUTSIDE the region, SCORE_INVALID: a coordinate the lattice cannot hold); voxel =
        the flat index of the point's voxel (NEAREST_NONE for OUTSIDE and INVALID); index = nearest()'s index at that voxel
        (NEAREST_NONE for FAR, OUTSIDE, INVALID); d2 = its squared distance in voxels (DF_FAR likewise); plus origin,
        block_key, cell as box() returns them — origin + unravel_index(index, dims) * resolution is the obstacle's centre.
        obstacles, radius and the region's blind spot: as nearest().  At most 2^28 voxels and 2^20 points."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: d[0] * d[1] * d[2] <= 1 << 28)
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        T = None
        if pose is not None:
            T = np.ascontiguousarray(pose, np.float32)
            if T.shape not in ((3, 4), (12,)):
                raise ValueError("nearest_points: pose must have the shape (3, 4) or (12,)")
        fields = _want("nearest_points", fields, self._NEAREST_POINTS_FIELDS)
        mask = _class_mask(obstacles)
        n = pts.shape[0]
        _fit("nearest_points: obstacles, radius and the number of points must fit 32 bits", (mask, radius, n))
        ok = ok and n <= SCORE_MAX_POINTS
        out = {k: np.empty(n if ok else 1, t) for k, t in self._NEAREST_POINTS_FIELDS.items() if k in fields}
        out.update(self._region_call(self._M.la3dm_map_nearest_points, lo3, d3, _addr(pts), n, _addr(T), mask, int(radius),
                                     C.byref(_out(_lib.NearestPointsOut, out))))
        return out

    _FOOTING_FIELDS = dict(index=np.uint32, levels=np.uint32, lowest=np.int32, highest=np.int32)

    def footing(self, lo, dims, support=("occupied",), clear=("free",), headroom=2, radius=0, step=0, min_support=None,
                fields=("index",), cap=None):
        """Where a ground robot can stand in the region of box(lo, dims), as an ordered list and per column.  A voxel v is a
        foot voxel when the voxel directly below it has a class in `support`, the `headroom` voxels from v upwards have
        classes in `clear` (v stands), every cell of the disc of `radius` voxels round v is clear from `step` voxels above
        v's height up to the headroom (the body hits nothing it cannot climb over), and at least `min_support` cells of
        that disc have a standing place within `step` voxels of v's height (the footprint is carried).  support / clear:
        names out of free / occupied / unknown / missing (/ uncertain on a BGK-LV map) or an integer bit mask, as
        raycast_many's `stop`; they must not overlap.  headroom 1 .. 32, radius 0 .. 8, step 0 .. 4 and below headroom;
        min_support=None asks for every cell of the disc, footprint_cells(radius), a smaller value tolerates holes in a
        sparsely observed floor, 0 asks only for an unobstructed body.  Classes outside the region are read from the map:
        the answer for a voxel does not depend on where the region's faces are.  Returns n = the number of foot voxels and,
        as `fields` names them, index (uint32) = their flat indices (i * ny + j) * nz + k in ascending order — what
        clusters(members=...) takes —, levels (uint32, shape (nx, ny)) = the foot voxels per column, lowest / highest
        (int32) = their smallest / largest k, -1 where there is none; n_stand, n_body, n_foot, disc_cells = the voxels that
        pass each condition and the cells of the disc; plus origin, block_key, cell as box() returns them.  cap=None counts
        first and then fills exactly n entries; an integer cap fills the first min(n, cap) and n is still the total.  At
        most 2^28 voxels in the padded box (nx + 2 radius, ny + 2 radius, nz + headroom + 2 step).  A device-resident map
        runs the query on the device pool (no host mirror refresh); a host-mode map runs it on the CPU, with identical
        results."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: True)
        fields = _want("footing", fields, self._FOOTING_FIELDS)
        masks = [_class_mask(support), _class_mask(clear)]
        if min_support is None:
            min_support = footprint_cells(radius) if 0 <= int(radius) <= FOOTING_MAX_RADIUS else 0
        _fit("footing: support, clear, headroom, radius, step and min_support must fit 32 bits", masks + [headroom, radius, step, min_support])
        if cap is not None:
            _fit("footing: cap must fit 64 bits", [cap], bits=64)
        ok = ok and (d[0] + 2 * int(radius)) * (d[1] + 2 * int(radius)) * (d[2] + int(headroom) + 2 * int(step)) <= FOOTING_MAX_CELLS
        params = _lib.FootingParams(masks[0], masks[1], int(headroom), int(radius), int(step), int(min_support))
        found, stats = C.c_uint64(0), _lib.FootingStats()
        region = {}

        def call(k, arrays):
            o = _out(_lib.FootingOut, arrays, null_empty=("index",))
            region.update(self._region_call(self._M.la3dm_map_footing, lo3, d3, C.byref(params), k, C.byref(o) if arrays else None,
                                            C.byref(found), C.byref(stats)))
            return int(found.value)

        out = {k: np.empty((d[0], d[1]) if ok else (1,), t) for k, t in self._FOOTING_FIELDS.items() if k != "index" and k in fields}
        if cap is None:   # the two-call protocol: count (the dense arrays come with this call), then fill exactly n
            k = call(0, out)
            filled = {}
        else:
            k = min(int(cap), cells if ok else 1)
            filled = dict(out)
        filled.update(index=np.empty(k, np.uint32))
        total = k
        if cap is not None or (k and "index" in fields):
            total = call(k, filled)
        if "index" in fields:
            out["index"] = filled["index"][:min(total, k)]
        out.update(n=total, **stats.as_dict())
        out.update(region)
        return out

    _SURFACE_FIELDS = dict(index=np.uint32, faces=np.uint8, normal=np.int16, dense_faces=np.uint8)

    def surface(self, lo, dims, solid=("occupied",), open=("free",), smooth=0, fields=("index", "faces", "normal"), cap=None):
        """The exposed faces and integer normals of the region of box(lo, dims).  A voxel whose class is in `solid` has face
        d (0: -x, 1: +x, 2: -y, 3: +y, 4: -z, 5: +z) when its neighbour in that direction has a class in `open`; a surface
        voxel has at least one.  solid / open: names out of free / occupied / unknown / missing (/ uncertain on a BGK-LV map)
        or an integer bit mask, as raycast_many's `stop`; they must not overlap.  Classes outside the region are read from
        the map: the answer for a voxel does not depend on where the region's faces are.  Returns n = the number of surface
        voxels and, as `fields` names them, index (uint32) = their flat indices (i * ny + j) * nz + k in ascending order,
        faces (uint8) = their face masks, bit d for direction d, normal (int16, shape (n, 3)) = per listed voxel the sum of
        the face vectors of every voxel within `smooth` voxels on every axis (0 .. 4) — it points from solid into open space,
        is at most (2 smooth + 1)^3 in size per component and may be (0, 0, 0), which means "no normal"; normal needs index —,
        dense_faces (uint8, shape dims) = the face mask of every voxel of the region, 0 where it is not solid or not
        exposed; n_solid, n_surface, face_count = the solid voxels of the region, n, and the faces per direction (their sum
        times resolution^2 is the surface area); plus origin, block_key, cell as box() returns them.  cap=None counts first
        and then fills exactly n entries; an integer cap fills the first min(n, cap) and n is still the total.  At most 2^28
        voxels in the region padded by smooth + 1 voxels on every side.  A device-resident map runs the query on the device
        pool (no host mirror refresh); a host-mode map runs it on the CPU, with identical results."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: True)
        fields = _want("surface", fields, self._SURFACE_FIELDS)
        masks = [_class_mask(solid), _class_mask(open)]
        _fit("surface: solid, open and smooth must fit 32 bits", masks + [smooth])
        if cap is not None:
            _fit("surface: cap must fit 64 bits", [cap], bits=64)
        ok = ok and int(np.prod([v + 2 * (int(smooth) + 1) for v in d], dtype=object)) <= SURFACE_MAX_CELLS
        params = _lib.SurfaceParams(masks[0], masks[1], int(smooth))
        found, stats = C.c_uint64(0), _lib.SurfaceStats()
        region = {}
        listed = [k for k in ("index", "faces", "normal") if k in fields]

        def call(k, arrays):
            o = _out(_lib.SurfaceOut, arrays, null_empty=("index", "faces", "normal"))
            region.update(self._region_call(self._M.la3dm_map_surface, lo3, d3, C.byref(params), k, C.byref(o) if arrays else None,
                                            C.byref(found), C.byref(stats)))
            return int(found.value)

        out = {"dense_faces": np.empty(tuple(d) if ok else (1,), np.uint8)} if "dense_faces" in fields else {}
        if cap is None:   # the two-call protocol: count (the dense array comes with this call), then fill exactly n
            k = call(0, out)
            filled = {}
        else:
            k = min(int(cap), cells if ok else 1) if listed else 0
            filled = dict(out)
        filled.update({f: np.empty((k, 3) if f == "normal" else k, self._SURFACE_FIELDS[f]) for f in listed})
        total = k
        if cap is not None or (k and listed):
            total = call(k, filled)
        for f in listed:
            out[f] = filled[f][:min(total, k)]
        out.update(n=total, **stats.as_dict())
        out.update(region)
        return out

    _PATHS_FIELDS = dict(cost=np.uint64, steps=np.uint32, stop=np.uint32, min_d2=np.uint32, ways=np.uint32, flags=np.uint8)

    def score_paths(self, lo, dims, paths, obstacles=("occupied",), clearance=0, soft_radius=0, penalty=0, move_cost=(10, 14, 17),
                    max_steps=4096, fields=("cost", "steps", "stop", "min_d2", "ways", "flags")):
        """Cost and clearance of P candidate trajectories through the region of box(lo, dims).  `paths` is (P, W, 3): W
        waypoints per path in the world frame (a shorter path repeats its last waypoint).  Every waypoint is resolved to its
        voxel as search resolves it and every path walked voxel by voxel from waypoint to waypoint (a 26-connected walk; the
        integer rule is in include/la3dm_hip.h) against d2 = distance_field(lo, dims, obstacles, max(1, clearance,
        soft_radius)).  The walk stops at the first voxel that is outside the region (PATH_LEFT) or within `clearance` voxels
        of an obstacle (PATH_BLOCKED; clearance 0: the obstacle voxels themselves), and after max_steps moves
        (PATH_TRUNCATED); a path with a coordinate the lattice cannot hold (NaN, inf, |w / resolution| >= 2^30) is
        PATH_INVALID as a whole.  Returns a dict of (P,) arrays, those named in `fields` and always cost: cost uint64 = the
        moves (move_cost by the number of axes a move changes) plus travel's penalty of every voxel entered, up to the stop
        — the cost travel gives the same walk with the same clearance, soft_radius, penalty and move_cost; steps = voxels
        walked; stop = the ordinal of the stop or PATH_NONE; min_d2 = the least d2 on the walk (DF_FAR: none within the
        radius); ways = waypoints reached; flags uint8 = the PATH_* bits; plus origin, block_key, cell as box() returns
        them.  At most 2^28 voxels, 2^20 paths, 1024 waypoints a path and 2^26 waypoints.  A device-resident map runs the
        query on the device pool (no host mirror refresh); a host-mode map runs it on the CPU, with identical results."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: d[0] * d[1] * d[2] <= 1 << 28)
        W = np.ascontiguousarray(paths, np.float32)
        if W.ndim != 3 or W.shape[2] != 3:
            raise ValueError("score_paths: paths must have the shape (P, W, 3)")
        fields = _want("score_paths", fields, self._PATHS_FIELDS)
        mask = _class_mask(obstacles)
        mc = [int(v) for v in move_cost]
        P, n_way = W.shape[0], W.shape[1]
        msg = "score_paths: move_cost must have three entries, and every parameter and count must fit 32 bits"
        if len(mc) != 3:
            raise ValueError(msg)
        _fit(msg, [mask, clearance, soft_radius, penalty, max_steps, P, n_way] + mc)
        prm = _lib.PathsParams(mask, int(clearance), int(soft_radius), int(penalty), (C.c_uint32 * 3)(*mc), int(max_steps))
        ok = ok and 1 <= n_way <= PATHS_MAX_WAY and P <= PATHS_MAX_PATHS and P * n_way <= PATHS_MAX_WAYPOINTS
        out = {k: np.empty(P if ok else 1, t) for k, t in self._PATHS_FIELDS.items() if k == "cost" or k in fields}
        out.update(self._region_call(self._M.la3dm_map_score_paths, lo3, d3, _addr(W), P, n_way, C.byref(prm),
                                     C.byref(_out(_lib.PathsOut, out))))
        return out

    def reach(self, lo, dims, seeds, passable=("free",), obstacles=("occupied",), clearance=0, connectivity=6, max_steps=None,
              targets=None, fields=("steps",)):
        """Hop distances from seed voxels through the passable voxels of the region of box(lo, dims): can a goal be got to,
        and in how many moves.  A voxel is passable when its class (box's cls) is in `passable` and, with clearance > 0,
        distance_field(lo, dims, obstacles, radius=clearance) reports it FAR (obstacles outside the region are not seen).
        seeds: flat indices (i * ny + j) * nz + k; one that is out of range or not passable is ignored.  steps[v] = the
        least number of moves from any seed to v, each to a passable neighbour inside the region under `connectivity` (6,
        18 or 26; diagonal moves are not tested for corner cutting — use clearance >= 1 or connectivity 6 for that),
        REACH_NONE where there is no walk of at most max_steps moves (None: REACH_MAX_STEPS).  targets: flat indices, e.g.
        frontier's index; target_steps[t] = steps[targets[t]], REACH_NONE for one out of range.  passable / obstacles: names
        out of free / occupied / unknown / missing (/ uncertain on a BGK-LV map) or an integer bit mask, as frontier takes
        them.  Returns a dict: steps (uint32, shape dims) when named in `fields`, target_steps (uint32) when targets is given
        — fields=() with targets fetches the targets' steps alone — n_seeded (distinct passable seeds), n_reached (voxels
        with finite steps), levels (the largest finite step; == max_steps: the wave may have been cut); plus origin,
        block_key, cell as box() returns them.  At most 2^28 voxels in the region padded by one.  A device-resident map runs
        the wave on the device pool, one launch per level (no host mirror refresh); a host-mode map runs a queue BFS on the
        CPU, with identical results."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: (d[0] + 2) * (d[1] + 2) * (d[2] + 2) <= REACH_MAX_CELLS)
        fields = _want("reach", fields, ("steps",))
        masks = [_class_mask(passable), _class_mask(obstacles)]
        s, t, nt = _indices(seeds, targets)
        max_steps = REACH_MAX_STEPS if max_steps is None else int(max_steps)
        _fit("reach: passable, obstacles, clearance, connectivity, max_steps and the numbers of seeds and targets must fit 32 bits",
             masks + [clearance, connectivity, max_steps, s.size, nt])
        out = {}
        if "steps" in fields:
            out["steps"] = np.empty(tuple(d) if ok else (1,), np.uint32)
        if t is not None:
            out["target_steps"] = np.empty(nt, np.uint32)
        stats = _lib.ReachStats()
        region = self._region_call(self._M.la3dm_map_reach, lo3, d3, _addr(s), s.size, masks[0], masks[1], int(clearance), int(connectivity),
                                   max_steps, _addr(t), nt, C.byref(_out(_lib.ReachOut, out, null_empty=("target_steps",))), C.byref(stats))
        out.update(stats.as_dict(), **region)
        return out

    def travel(self, lo, dims, seeds, passable=("free",), obstacles=("occupied",), clearance=0, soft_radius=0, penalty=0,
               move_cost=(10, 14, 17), connectivity=26, max_cost=None, targets=None, fields=("cost",)):
        """Least path costs from seed voxels through the passable voxels of the region of box(lo, dims), and the parents to
        drive along.  A voxel is passable when its class (box's cls) is in `passable` and, with clearance > 0, it lies farther
        than `clearance` voxels from every voxel of the region with a class in `obstacles`.  A move along an offset with 1, 2
        or 3 non-zero components costs move_cost[0], [1] or [2] (10 / 14 / 17 is metres x 10 / resolution; 1 / 1 / 1 gives
        reach's steps); entering a voxel at squared distance d2 <= soft_radius^2 from an obstacle costs
        penalty * (soft_radius^2 - d2) // soft_radius^2 more.  seeds cost 0; one that is out of range or not passable is
        ignored.  cost[v] = the least cost of a walk inside the region from any seed to v under `connectivity` (6, 18 or 26),
        TRAVEL_NONE where there is none of at most max_cost (None: TRAVEL_MAX_COST).  parent[v] (uint8) = the code
        (di + 1) * 9 + (dj + 1) * 3 + (dk + 1) of the offset to the voxel a least-cost walk came from — the smallest such code
        — 13 at a seed and 255 where unreached: follow_parents(parent, dims, index) lists the path.  targets: flat indices,
        e.g. frontier's index; target_cost[t] = cost[targets[t]].  passable / obstacles: names or an integer bit mask, as reach
        takes them.  fields: any of "cost", "parent"; fields=() with targets fetches the targets' costs alone.  Returns a dict
        with those arrays, n_seeded, n_reached, max_cost (the largest finite cost), the device form's diagnostics rounds,
        brick_runs and capped (0 on a host-mode map), plus origin, block_key, cell as box() returns them.  A device-resident
        map relaxes 8 x 8 x 8 bricks of the region on the device pool (no host mirror refresh); a host-mode map runs Dijkstra
        on the CPU, with identical results."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: ((d[0] + 7) // 8) * ((d[1] + 7) // 8) * ((d[2] + 7) // 8) * 512 <= TRAVEL_MAX_CELLS)
        shape = tuple(d) if ok else (1,)
        fields = _want("travel", fields, ("cost", "parent"))
        masks = [_class_mask(passable), _class_mask(obstacles)]
        s, t, nt = _indices(seeds, targets)
        max_cost = TRAVEL_MAX_COST if max_cost is None else int(max_cost)
        moves = [int(v) for v in move_cost]
        if len(moves) != 3:
            raise ValueError("travel: move_cost must hold three values")
        words = masks + [int(clearance), int(soft_radius), int(penalty)] + moves + [int(connectivity), max_cost]
        _fit("travel: the masks, clearance, soft_radius, penalty, move_cost, connectivity, max_cost and the numbers of seeds and targets must fit 32 bits",
             words + [s.size, nt])
        p = _lib.TravelParams(words[0], words[1], words[2], words[3], words[4], (C.c_uint32 * 3)(*moves), words[8], words[9])
        out = {}
        if "cost" in fields:
            out["cost"] = np.empty(shape, np.uint32)
        if "parent" in fields:
            out["parent"] = np.empty(shape, np.uint8)
        if t is not None:
            out["target_cost"] = np.empty(nt, np.uint32)
        stats = _lib.TravelStats()
        region = self._region_call(self._M.la3dm_map_travel, lo3, d3, _addr(s), s.size, C.byref(p), _addr(t), nt,
                                   C.byref(_out(_lib.TravelOut, out, null_empty=("target_cost",))), C.byref(stats))
        out.update(stats.as_dict(), **region)
        return out

    def drive(self, lo, dims, seeds, members=None, footing=None, connectivity=8, step=1, snap=0, move_cost=(10, 14), climb_up=0,
              climb_down=0, max_cost=None, targets=None, fields=("cost",)):
        """Least costs of ground routes from seed voxels over the member voxels of the region of box(lo, dims), and the
        parents to drive along.  The members are the voxels of `members` (flat indices (i * ny + j) * nz + k, e.g. footing's
        index; one out of range is ignored, one listed twice counts once; no class is tested and the map is not read) or,
        with footing=dict(support=, clear=, headroom=, radius=, step=, min_support=) — footing()'s parameters —, exactly the
        voxels footing(lo, dims, **footing) lists: a device-resident map then feeds footing's kernels into the query
        without listing or downloading anything.  One of the two, not both.  A move goes from a member to a member at one
        of the `connectivity` (4 or 8) horizontal neighbours, up to `step` (0 .. 4) voxels higher or lower — never straight
        up or down — and costs move_cost[0] (straight) or move_cost[1] (diagonal) plus climb_up per voxel climbed or
        climb_down per voxel dropped.  seeds and targets are flat indices; each stands for the highest member of its column
        at most `snap` (0 .. 32) voxels below it, so the sensor's voxel can be passed as it is; a seed without one is
        ignored.  cost[v] = the least cost of a walk of members from any seed to v, DRIVE_NONE for a non-member and where
        there is none of at most max_cost (None: TRAVEL_MAX_COST).  parent[v] (uint8) = the code ((o_i + 1) * 3 + (o_j + 1))
        * 9 + (o_k + 4) of the offset to the member a least-cost walk came from — the smallest such code — 40 at a seed and
        255 where unreached: follow_drive_parents(parent, dims, index) lists the route.  fields: any of "cost", "parent",
        "of_member" (the cost per entry of `members`) and "target_index" (the member each target stands for, DRIVE_NONE
        without one); target_cost comes with `targets`, and fields=() with targets fetches the targets' answers alone.
        Returns a dict with those arrays, n_members, n_seeded, n_reached, max_cost (the largest finite cost), the device
        form's diagnostics rounds, brick_runs and capped (0 on a host-mode map), plus origin, block_key, cell as box()
        returns them.  A device-resident map relaxes 8 x 8 x 8 bricks of the region on the device (no host mirror refresh);
        a host-mode map runs Dijkstra on the CPU, with identical results."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: ((d[0] + 7) // 8) * ((d[1] + 7) // 8) * ((d[2] + 7) // 8) * 512 <= DRIVE_MAX_CELLS)
        fields = _want("drive", fields, ("cost", "parent", "of_member", "target_index"))
        s, t, nt = _indices(seeds, targets)
        lst = None if members is None else np.ascontiguousarray(members, np.uint32).reshape(-1)
        nm = 0 if lst is None else lst.size
        max_cost = TRAVEL_MAX_COST if max_cost is None else int(max_cost)
        moves = [int(v) for v in move_cost]
        if len(moves) != 2:
            raise ValueError("drive: move_cost must hold two values")
        words = [int(connectivity), int(step), int(snap)] + moves + [int(climb_up), int(climb_down), max_cost]
        msg = "drive: connectivity, step, snap, move_cost, climb_up, climb_down, max_cost, footing's parameters and the numbers of members, seeds and targets must fit 32 bits"
        _fit(msg, words + [nm, s.size, nt])
        fp = None
        if footing is not None:
            f = dict(support=("occupied",), clear=("free",), headroom=2, radius=0, step=0, min_support=None)
            bad = set(footing) - set(f)
            if bad:
                raise ValueError(f"drive: unknown footing parameters {sorted(bad)}")
            f.update(footing)
            if f["min_support"] is None:
                f["min_support"] = footprint_cells(f["radius"]) if 0 <= int(f["radius"]) <= FOOTING_MAX_RADIUS else 0
            fw = [_class_mask(f["support"]), _class_mask(f["clear"])] + [int(f[k]) for k in ("headroom", "radius", "step", "min_support")]
            _fit(msg, fw)
            fp = _lib.FootingParams(*fw)
            ok = ok and (d[0] + 2 * fw[3]) * (d[1] + 2 * fw[3]) * (d[2] + fw[2] + 2 * fw[4]) <= FOOTING_MAX_CELLS
        shape = tuple(d) if ok else (1,)
        # list mode with an empty list: the pointer still says which mode it is
        at = None if lst is None else (lst if nm else np.zeros(1, np.uint32)).ctypes.data
        p = _lib.DriveParams(at, C.pointer(fp) if fp is not None else None, nm, words[0], words[1], words[2], (C.c_uint32 * 2)(*moves),
                             words[5], words[6], words[7])
        out = {}
        if "cost" in fields:
            out["cost"] = np.empty(shape, np.uint32)
        if "parent" in fields:
            out["parent"] = np.empty(shape, np.uint8)
        if "of_member" in fields:
            out["of_member"] = np.empty(nm, np.uint32)
        if t is not None:
            out["target_cost"] = np.empty(nt, np.uint32)
            if "target_index" in fields:
                out["target_index"] = np.empty(nt, np.uint32)
        elif "target_index" in fields:
            raise ValueError("drive: target_index needs targets")
        stats = _lib.DriveStats()
        region = self._region_call(self._M.la3dm_map_drive, lo3, d3, _addr(s), s.size, C.byref(p), _addr(t), nt,
                                   C.byref(_out(_lib.DriveOut, out, null_empty=("of_member", "target_cost", "target_index"))), C.byref(stats))
        out.update(stats.as_dict(), **region)
        return out

    def clusters(self, lo, dims, members=None, member=("free",), connectivity=26, tile=0, min_size=1, cap=None, fields=("label",)):
        """The connected groups of the member voxels of the region of box(lo, dims).  A member is a voxel whose class (box's
        cls) is in `member` (names or an integer bit mask, as travel takes them) — every such voxel of the region, or with
        `members` (flat indices, e.g. frontier's index) only the listed ones; an index out of range is ignored and a voxel
        listed twice counts once.  Two members are adjacent under `connectivity` (6, 18 or 26) and, with tile > 0 (a multiple
        of 8), only inside the same tile of tile^3 voxels anchored at voxel (0, 0, 0).  Clusters with fewer than min_size
        members are dropped; the others are numbered in ascending order of `first`, their smallest flat index.  fields: any
        of "label" (uint32 per voxel, CLUSTERS_NONE for a non-member or a dropped cluster) and "of_member" (the same per
        entry of `members`).  cap: records wanted at most (None: every cluster; 0: count only).  Returns a dict with those
        arrays, the records of the first min(n, cap) clusters — first, size, lo and hi [., 3] (the bounding box, inclusive),
        sum [., 3] (uint64 sums of i, j, k: the client divides) and rep (the member nearest the rounded centroid, the
        smallest flat index among equals) — n (the number of kept clusters), n_members, n_clusters, n_dropped, largest, the
        device form's diagnostics rounds, brick_runs and capped (0 on a host-mode map), plus origin, block_key, cell as
        box() returns them.  A device-resident map relaxes 8 x 8 x 8 bricks of the region on the device pool (no host mirror
        refresh); a host-mode map flood-fills on the CPU, with identical results."""
        lo3, d3, d, cells, ok = self._region(lo, dims, lambda d: max(d) <= CLUSTERS_MAX_AXIS and ((d[0] + 7) // 8) * ((d[1] + 7) // 8) * ((d[2] + 7) // 8) * 512 <= CLUSTERS_MAX_CELLS)
        fields = _want("clusters", fields, ("label", "of_member"))
        mask = _class_mask(member)
        lst = None if members is None else np.ascontiguousarray(members, np.uint32).reshape(-1)
        nm = 0 if lst is None else lst.size
        room = (nm if lst is not None else (cells if ok else 1)) if cap is None else int(cap)   # (no more clusters than members)
        words = [mask, int(connectivity), int(tile), int(min_size), nm, room]
        _fit("clusters: the mask, connectivity, tile, min_size, cap and the number of members must fit 32 bits", words)
        p = _lib.ClustersParams(mask, 0 if lst is None else 1, words[1], words[2], words[3], nm, _addr(lst), room)
        out = {}
        if "label" in fields:
            out["label"] = np.empty(tuple(d) if ok else (1,), np.uint32)
        if "of_member" in fields:
            out["of_member"] = np.empty(nm, np.uint32)
        rec = dict(first=np.empty(room, np.uint32), size=np.empty(room, np.uint32), lo=np.empty((room, 3), np.uint32),
                   hi=np.empty((room, 3), np.uint32), sum=np.empty((room, 3), np.uint64), rep=np.empty(room, np.uint32))
        found, stats = C.c_uint32(0), _lib.ClustersStats()
        region = self._region_call(self._M.la3dm_map_clusters, lo3, d3, C.byref(p), C.byref(_out(_lib.ClustersOut, {**out, **rec}, null_empty=rec)),
                                   C.byref(found), C.byref(stats))
        m = min(int(found.value), room)
        out.update({k: v[:m].copy() for k, v in rec.items()})   # (the unused tail of the room is never touched)
        out.update(n=int(found.value), **stats.as_dict(), **region)
        return out

    def pack(self):
        """The map as the compact stream of its covering leaves (layout: include/la3dm_hip.h, la3dm_devmap_pack_host): a
        uint8 array of header, block keys, per-block leaf offsets and node masks, and state, A, B of the leaves.  A
        device-resident map compacts its pool on the GPU before it crosses PCIe (no host mirror refresh; blocks in pool
        order); a host-mode map writes the same stream from its blocks (ascending key).  Not in the stream: the last
        scan's training data, the statistics, the options and the shard configuration."""
        return self._sized(lambda *buf: self._M.la3dm_map_pack(self._h, *buf))

    def _sized(self, call):
        """a stream by the size-then-fill double call: call(buf, cap, size) with no buffer sizes it, then with one fills it"""
        size = C.c_uint64(0)
        self._chk(call(None, 0, C.byref(size)))
        buf = np.empty(int(size.value), np.uint8)
        self._chk(call(buf.ctypes.data, buf.size, C.byref(size)))
        return buf[:int(size.value)]

    def unpack(self, stream):
        """Load a stream of pack() (bytes or a uint8 array, of either writer) into this EMPTY map: same class, block_depth,
        resolution and default node, the other parameters may differ.  Validated first; a refused stream raises
        RuntimeError and leaves the map as it was."""
        buf = _stream(stream)
        self._chk(self._M.la3dm_map_unpack(self._h, _addr(buf), buf.size))
        return self

    def save(self, path):
        """pack() written to path + ".tmp" and renamed to path"""
        self._chk(self._M.la3dm_map_save(self._h, os.fsencode(path)))

    def load(self, path):
        """unpack() of the file at path"""
        self._chk(self._M.la3dm_map_load(self._h, os.fsencode(path)))
        return self

    def merge(self, stream_or_map):
        """Fuse a stream of pack() (bytes or a uint8 array) or another map of this map's class (packed first) into this
        map, which may hold blocks (contract: include/la3dm_hip.h, la3dm_devmap_merge_host).  Per finest cell of every
        block the stream names: kept where the incoming leaf is the default node, copied where this map's is, else the
        evidence sums are added and the state re-derived; the blocks are pruned and written in unpack()'s canonical form,
        new blocks appended in stream order.  BGKOctoMap and BGKLOctoMap only.  A device-resident map fuses on the GPU
        pool, a host-mode map on the CPU: the same bytes.  Validated first; a refused stream raises RuntimeError and
        leaves the map as it was.  Returns dict(n_blocks, n_created, cells_kept, cells_copied, cells_fused)."""
        if isinstance(stream_or_map, BGKOctoMap):
            if type(stream_or_map) is not type(self):
                raise TypeError(f"merge: a {type(stream_or_map).__name__} is not merged into a {type(self).__name__}")
            if stream_or_map is self:
                raise ValueError("merge: a map is not merged into itself")
            stream_or_map = stream_or_map.pack()
        buf = _stream(stream_or_map)
        stats = _lib.MergeStats()
        self._chk(self._M.la3dm_map_merge(self._h, _addr(buf), buf.size, C.byref(stats)))
        return stats.as_dict()

    def merge_file(self, path):
        """merge() of the file at path (a file save() wrote)"""
        stats = _lib.MergeStats()
        self._chk(self._M.la3dm_map_merge_file(self._h, os.fsencode(path), C.byref(stats)))
        return stats.as_dict()

    _DIFF_FIELDS = dict(block_key=(np.int64, 1), cell=(np.uint32, 1), code=(np.uint8, 1), centre=(np.float32, 3), A=(np.float32, 1),
                        B=(np.float32, 1))

    def _diff(self, fn, head, pairs, values, map_only, fields, cap):
        """what diff and diff_file share: the masks, the two-call protocol, the dict"""
        pair_mask, value_mask = _pair_mask(pairs), _class_mask(values)
        _fit("diff: pairs and values must fit 32 bits", (pair_mask, value_mask))
        fields = _want("diff", fields, self._DIFF_FIELDS)
        if cap is not None:
            _fit("diff: cap must fit 64 bits", [cap], bits=64)
        params = _lib.DiffParams(pair_mask, value_mask, 1 if map_only else 0)
        stats = _lib.DiffStats()
        found = C.c_uint64(0)
        if cap is None:   # the two-call protocol: count, then fill exactly n
            self._chk(fn(*head, C.byref(params), 0, None, C.byref(found), C.byref(stats)))
            k = int(found.value)
        else:
            k = min(int(cap), 2 ** 32 - 1)
        out = {f: np.empty((k, w) if w > 1 else k, t) for f, (t, w) in self._DIFF_FIELDS.items() if f in fields}
        if cap is not None or (k and out):
            self._chk(fn(*head, C.byref(params), k, C.byref(_out(_lib.DiffOut, out, null_empty=out)), C.byref(found), C.byref(stats)))
        m = min(int(found.value), k)
        out = {f: v[:m] for f, v in out.items()}
        counts = stats.as_dict()
        out.update(n=int(found.value), pairs=np.array(counts.pop("pairs"), np.uint64).reshape(5, 5),
                   value_changed=np.array(counts.pop("value_changed"), np.uint64), **counts)
        return out

    def diff(self, stream_or_map, pairs="changed", values=(), map_only=True, fields=("block_key", "cell", "code"), cap=None):
        """What changed: the finest cells whose class differs between this map (now) and a stream of pack() / pack_region() /
        evict() — bytes, a uint8 array, or another map of this map's class, packed first — (then); contract:
        include/la3dm_hip.h, la3dm_devmap_diff_host.  Compared are the blocks the stream names, in stream order, and with
        map_only the map's other blocks after them (pack()'s order).  The class is that of the cell's covering leaf: free 0,
        occupied 1, unknown 2, uncertain 4 (BGK-LV), missing 3 on the side that has no such block.  pairs selects (then, now)
        pairs: "changed" (every pair with then != now), an integer mask (bit 5 then + now) or an iterable of pairs of class
        names, e.g. [("free", "occupied"), ("missing", "occupied")]; values: class names (or a bit mask) for which cells of
        unchanged class whose A or B changed bit for bit are listed too.  Returns a dict: n = the number of selected cells;
        the arrays named in fields out of block_key, cell (the finest-layer index in the block), code (then | now << 4),
        centre (n, 3), A, B (the map's values now); pairs (5, 5) uint64 = the compared cells per [then, now];
        value_changed (5,) (all zero unless values is given); n_stream_blocks, n_map_only_blocks, n_missing_now.  cap=None
        counts first and then fills exactly n entries; an integer cap fills the first min(n, cap) and n is still the total.
        The map is not changed.  A device-resident map compares on the GPU pool (no host mirror refresh), a host-mode map
        on the CPU: the same list and counts.  A refused stream raises RuntimeError."""
        if isinstance(stream_or_map, BGKOctoMap):
            if type(stream_or_map) is not type(self):
                raise TypeError(f"diff: a {type(stream_or_map).__name__} is not compared with a {type(self).__name__}")
            stream_or_map = stream_or_map.pack()
        buf = _stream(stream_or_map)
        return self._diff(self._M.la3dm_map_diff, (self._h, _addr(buf), buf.size), pairs, values, map_only, fields, cap)

    def diff_file(self, path, pairs="changed", values=(), map_only=True, fields=("block_key", "cell", "code"), cap=None):
        """diff() against the file at path (a file save() or evict_file() wrote)"""
        return self._diff(self._M.la3dm_map_diff_file, (self._h, os.fsencode(path)), pairs, values, map_only, fields, cap)

    @staticmethod
    def _region_points(lo, hi):
        lo3, hi3 = np.ascontiguousarray(lo, np.float32).reshape(-1), np.ascontiguousarray(hi, np.float32).reshape(-1)
        if lo3.size != 3 or hi3.size != 3:
            raise ValueError("a region is given by two points of three coordinates")
        return lo3, hi3

    def pack_region(self, lo, hi, inside=True):
        """The stream of pack() with some of the blocks only (contract: include/la3dm_hip.h, la3dm_devmap_pack_region_host):
        the box of blocks from the block that holds the world point lo to the block that holds hi; inside=True selects the
        blocks in the box, False every other block.  The map is not changed; unpack(), merge() and pack_info() take the
        stream.  A device-resident map compacts the selected blocks on the GPU (pool slot order, no mirror refresh), a
        host-mode map writes them in ascending key order.  No block selected gives the header alone."""
        lo3, hi3 = self._region_points(lo, hi)
        args = (self._h, lo3.ctypes.data, hi3.ctypes.data, 1 if inside else 0)
        return self._sized(lambda *buf: self._M.la3dm_map_pack_region(*args, *buf))

    def erase_region(self, lo, hi, inside=True):
        """Remove the selected blocks (the region as in pack_region): their voxels read as missing through every query,
        block_count() drops, a later insert or merge may create blocks there again.  A device-resident map compacts its
        pool in place on the GPU — the surviving blocks of the tail fill the holes, everything else keeps its slot — and
        rebuilds its block table.  Returns dict(n_removed, n_moved, n_blocks); n_blocks is the count after the call."""
        lo3, hi3 = self._region_points(lo, hi)
        stats = _lib.EraseStats()
        self._chk(self._M.la3dm_map_erase_region(self._h, lo3.ctypes.data, hi3.ctypes.data, 1 if inside else 0, C.byref(stats)))
        return stats.as_dict()

    def evict(self, lo, hi, inside=True):
        """pack_region(), then erase_region() of the same region: the stream is complete on the host before the first block
        is removed, and a failure of the pack step leaves the map as it was.  Returns the stream as bytes; merge() of it
        brings the blocks back."""
        lo3, hi3 = self._region_points(lo, hi)
        args = (self._h, lo3.ctypes.data, hi3.ctypes.data, 1 if inside else 0)
        # (the sizing call removes nothing)
        return self._sized(lambda *buf: self._M.la3dm_map_evict(*args, *buf, None)).tobytes()

    def evict_file(self, path, lo, hi, inside=True):
        """evict() into a file: the stream is written to path + ".tmp" and renamed to path before the first block is removed
        (merge_file(path) brings the blocks back).  Returns erase_region()'s dict."""
        lo3, hi3 = self._region_points(lo, hi)
        stats = _lib.EraseStats()
        self._chk(self._M.la3dm_map_evict_file(self._h, os.fsencode(path), lo3.ctypes.data, hi3.ctypes.data, 1 if inside else 0, C.byref(stats)))
        return stats.as_dict()

    def mirror_syncs(self):
        """how often the host mirror of the device-resident map was refreshed (a download of every node of every block)"""
        return int(self._M.la3dm_map_mirror_syncs(self._h))

    def export_cells(self, state="occupied", original_size=True, min_z=0.0, max_z=0.0):
        """Cube lists of the map (the static node's publish loop + MarkerArrayPub::insert_point3d / heightMapColor,
        reference bgkoctomap_static_node.cpp:101-136, markerarray_pub.h:21-147, minus ROS): dict of cells (n, 4)
        {x, y, z, size}, rgba (n, 4), level (n,) = (int) log2(size / resolution).  state "occupied": coloured by
        height between min_z and max_z (equal: the map's bbox); "free": coloured by probability.  original_size
        False expands collapsed leaves (get_pruned_locs).  Device-resident maps are scanned on the GPU."""
        st = {"occupied": 1, "free": 0}[state]
        n = C.c_uint64(0)
        if self._M.la3dm_map_export_cells(self._h, st, int(bool(original_size)), min_z, max_z, None, None, None, 0, C.byref(n)) != 0:
            raise RuntimeError(self._M.la3dm_map_last_error().decode())
        k = int(n.value)
        out = dict(cells=np.zeros((k, 4), np.float32), rgba=np.zeros((k, 4), np.float32), level=np.zeros(k, np.int32))
        if k and self._M.la3dm_map_export_cells(self._h, st, int(bool(original_size)), min_z, max_z, out["cells"].ctypes.data,
                                                out["rgba"].ctypes.data, out["level"].ctypes.data, k, C.byref(n)) != 0:
            raise RuntimeError(self._M.la3dm_map_last_error().decode())
        return out

    def leaves(self):
        """All leaves (begin_leaf()..end_leaf()), blocks by ascending hash key, leaves in
        LeafIterator order: dict of block_key, node_key, loc, size, A, B, state, classified."""
        n = self._M.la3dm_map_leaf_count(self._h)
        out = dict(block_key=np.zeros(n, np.int64), node_key=np.zeros(n, np.int32), loc=np.zeros((n, 3), np.float32),
                   size=np.zeros(n, np.float32), A=np.zeros(n, np.float32), B=np.zeros(n, np.float32),
                   state=np.zeros(n, np.uint8), classified=np.zeros(n, np.uint8))
        m = self._M.la3dm_map_dump_leaves(self._h, *[out[k].ctypes.data for k in
                                                     ("block_key", "node_key", "loc", "size", "A", "B", "state",
                                                      "classified")], n)
        assert m <= n
        return {k: v[:m] for k, v in out.items()} if m < n else out   # (an LV map only reports touched blocks)

    def block_count(self):
        return self._M.la3dm_map_block_count(self._h)

    # -- split form ---------------------------------------------------------
    def prepare(self, cloud, origin, ds_resolution, free_res=2.0, max_range=-1.0):
        xyz = np.ascontiguousarray(cloud, np.float32).reshape(-1, 3)
        o = np.ascontiguousarray(origin, np.float32)
        return bool(self._chk(self._M.la3dm_map_prepare(self._h, xyz, xyz.shape[0], o, ds_resolution, free_res,
                                                        max_range)))

    def prepare_training_data(self, xyzy, ungated=False):
        a = np.ascontiguousarray(xyzy, np.float32).reshape(-1, 4)
        return bool(self._chk(self._M.la3dm_map_prepare_training_data(self._h, a, a.shape[0], int(ungated))))

    def packed(self):
        s = _lib.BgkScan()
        self._chk(self._M.la3dm_map_packed(self._h, C.byref(s)))
        return PackedScan(s)

    def commit(self):
        self._chk(self._M.la3dm_map_commit(self._h))

    def ctx(self):
        return self._M.la3dm_map_ctx(self._h)

    def set_option(self, name, value):
        rc = _lib.hip().la3dm_set_option(self.ctx(), name.encode(), int(value))
        if rc != 0:
            raise RuntimeError(_lib.hip().la3dm_last_error(self.ctx()).decode())

    def get_option(self, name):
        v = C.c_int()
        if _lib.hip().la3dm_get_option(self.ctx(), name.encode(), C.byref(v)) != 0:
            raise RuntimeError(f"la3dm_get_option: unknown option {name}")
        return v.value

    def scan_host(self, packed: PackedScan):
        cnt = _lib.BgkCounters()
        fn = _lib.hip().la3dm_gp_scan_host if self._gp else _lib.hip().la3dm_bgk_scan_host
        rc = fn(self.ctx(), C.byref(packed.c), C.byref(cnt))
        if rc != 0:
            raise RuntimeError(_lib.hip().la3dm_last_error(self.ctx()).decode())
        return cnt

    def stats(self):
        s = _lib.ScanStats()
        self._M.la3dm_map_stats(self._h, C.byref(s))
        return s.as_dict()

    def training_data(self):
        n = self._M.la3dm_map_training_size(self._h)
        a = np.zeros((n, 4), np.float32)
        if n:
            self._M.la3dm_map_training_data(self._h, a, n)
        return a

    def diag_eval(self, op, x):
        x = np.ascontiguousarray(x, np.float32)
        y = np.zeros_like(x)
        rc = _lib.hip().la3dm_diag_eval(self.ctx(), op, x.ctypes.data, x.size, y.ctypes.data)
        if rc != 0:
            raise RuntimeError(_lib.hip().la3dm_last_error(self.ctx()).decode())
        return y

    def diag_sweep(self, what, lo, hi):
        """count fp32 inputs in [lo, hi] (floats, same sign) where a kernel shortcut differs from IEEE"""
        lo_b = int(np.float32(lo).view(np.uint32))
        hi_b = int(np.float32(hi).view(np.uint32))
        if lo_b > hi_b:
            lo_b, hi_b = hi_b, lo_b
        out = C.c_uint64()
        rc = _lib.hip().la3dm_diag_sweep(self.ctx(), what, lo_b, hi_b, C.byref(out))
        if rc != 0:
            raise RuntimeError(_lib.hip().la3dm_last_error(self.ctx()).decode())
        return out.value

    # host bookkeeping primitives
    def block_to_hash_key(self, x, y, z):
        return self._M.la3dm_map_block_to_hash_key(self._h, x, y, z)

    def hash_key_to_block(self, key):
        o = np.zeros(3, np.float32)
        self._M.la3dm_map_hash_key_to_block(self._h, key, o)
        return o

    def get_extended_block(self, key):
        o = np.zeros(7, np.int64)
        self._M.la3dm_map_extended_block(self._h, key, o)
        return o

    def lut(self):
        n = self._M.la3dm_map_lut(self._h, None, 0)
        a = np.zeros((n, 3), np.float32)
        self._M.la3dm_map_lut(self._h, a.ctypes.data, n)
        return a


class GPOctoMap(BGKOctoMap):
    """Python mirror of la3dm::GPOctoMap (reference include/gpoctomap/gpoctomap.h): GP regression per block
    (Matern-3/2, Cholesky) + BCM fusion.  leaves()["A"/"B"] are the nodes' m_ivar / ivar."""
    _gp = True

    def __init__(self, resolution=0.1, block_depth=4, sf2=1.0, ell=1.0, noise=0.01, l=100.0, min_var=0.001,
                 max_var=1000.0, max_known_var=0.02, free_thresh=0.3, occupied_thresh=0.7, device=0):
        self._M = _lib.maplib()
        self._h = self._M.la3dm_map_create_gp(resolution, block_depth, sf2, ell, noise, l, min_var, max_var,
                                              max_known_var, free_thresh, occupied_thresh, device)
        if not self._h:
            raise RuntimeError(self._M.la3dm_map_last_error().decode())
        self.resolution = resolution
        self.block_depth = block_depth
        self.device = device


class BGKLOctoMap(BGKOctoMap):
    """Python mirror of la3dm::BGKLOctoMap (reference include/bgkloctomap/bgkloctomap.h): block-level BGK whose
    free-space evidence are the beams themselves (line segments)."""

    def __init__(self, resolution=0.1, block_depth=4, sf2=1.0, ell=1.0, free_thresh=0.3, occupied_thresh=0.7,
                 var_thresh=1.0, prior_A=1.0, prior_B=1.0, device=0):
        self._M = _lib.maplib()
        self._h = self._M.la3dm_map_create_l(resolution, block_depth, sf2, ell, free_thresh, occupied_thresh, var_thresh,
                                             prior_A, prior_B, device)
        if not self._h:
            raise RuntimeError(self._M.la3dm_map_last_error().decode())
        self.resolution = resolution
        self.block_depth = block_depth
        self.device = device

    def l_training(self):
        """(samples (n, 4) x,y,z,beam index or -1; beams (m, 6)) of the last scan"""
        nr = C.c_uint64()
        n = self._M.la3dm_map_l_training(self._h, None, 0, None, 0, C.byref(nr))
        idx, rays = np.zeros(n, np.int32), np.zeros((nr.value, 6), np.float32)
        self._M.la3dm_map_l_training(self._h, idx.ctypes.data, n, rays.ctypes.data, nr.value, C.byref(nr))
        xy = self.training_data()
        xy[:, 3] = idx
        return xy, rays


LV_STATS = ["n_hits", "n_rays", "n_samples", "n_bbox_blocks", "n_packed_blocks", "n_info_blocks", "voxels",
            "voxel_updates", "t_frontend", "t_partition", "t_device", "t_commit", "t_total"]


class BGKLVOctoMap(BGKOctoMap):
    """Python mirror of la3dm::BGKLVOctoMap (reference include/bgklvoctomap/bgklvoctomap.h): hits + free-space line
    segments, per-voxel inference, variance-aware node (UNCERTAIN = 3, PRUNED = 4 in leaves()["state"])."""

    def __init__(self, resolution=0.1, block_depth=4, sf2=1.0, ell=1.0, free_thresh=0.3, occupied_thresh=0.7,
                 var_thresh=1.0, prior_A=1.0, prior_B=1.0, original_size=True, min_W=0.1, device=0):
        self._M = _lib.maplib()
        self._h = self._M.la3dm_map_create_lv(resolution, block_depth, sf2, ell, free_thresh, occupied_thresh, var_thresh,
                                              prior_A, prior_B, int(original_size), min_W, device)
        if not self._h:
            raise RuntimeError(self._M.la3dm_map_last_error().decode())
        self.resolution = resolution
        self.block_depth = block_depth
        self.device = device

    def lv_stats(self):
        a = np.zeros(13, np.float64)
        self._M.la3dm_map_lv_stats(self._h, a)
        return dict(zip(LV_STATS, a.tolist()))

    def lv_training(self):
        nr = C.c_uint64()
        n = self._M.la3dm_map_lv_training(self._h, None, 0, None, 0, C.byref(nr))
        s, r = np.zeros((n, 4), np.float32), np.zeros((nr.value, 6), np.float32)
        self._M.la3dm_map_lv_training(self._h, s.ctypes.data, n, r.ctypes.data, nr.value, C.byref(nr))
        return s, r

    def lv_prepare(self, cloud, origin, ds_resolution, free_res=2.0, max_range=-1.0):
        xyz = np.ascontiguousarray(cloud, np.float32).reshape(-1, 3)
        o = np.ascontiguousarray(origin, np.float32)
        return bool(self._chk(self._M.la3dm_map_lv_prepare(self._h, xyz, xyz.shape[0], o, ds_resolution, free_res,
                                                           max_range)))

    def lv_packed(self):
        s = _lib.LvScan()
        self._chk(self._M.la3dm_map_lv_packed(self._h, C.byref(s)))
        return s

    def lv_commit(self):
        self._chk(self._M.la3dm_map_lv_commit(self._h))


PACK_CLASSES = ("BGKOctoMap", "GPOctoMap", "BGKLVOctoMap", "BGKLOctoMap")   # by the header's variant


def pack_info(stream_or_path):
    """The validated header of a map stream (bytes, a uint8 array, or the path of a saved map) as a dict: the fields of
    la3dm_pack_header (include/la3dm_hip.h) plus `cls`, the name of the map class.  No GPU is needed; a stream that fails
    validation raises RuntimeError."""
    if isinstance(stream_or_path, (str, os.PathLike)):
        stream_or_path = np.fromfile(stream_or_path, np.uint8)
    buf = _stream(stream_or_path)
    h = _lib.PackHeader()
    L = _lib.hip()
    if L.la3dm_pack_info(_addr(buf), buf.size, C.byref(h)) != 0:
        raise RuntimeError(L.la3dm_last_error(None).decode())
    out = {k: getattr(h, k) for k, _ in _lib.PackHeader._fields_ if k not in ("magic", "reserved")}
    out["magic"] = bytes(h.magic)
    out["cls"] = PACK_CLASSES[h.variant]
    return out


def load_map(path, device=0, device_resident=True):
    """The map saved at `path`: an object of the class the stream's header names, constructed with the header's parameters on
    `device` (-1: a host-mode map without a GPU), device-resident or not, with the stream loaded."""
    h = pack_info(path)
    f = lambda k: float(np.float32(h[k]))   # noqa: E731
    common = dict(resolution=f("resolution"), block_depth=int(h["block_depth"]), sf2=f("sf2"), ell=f("ell"),
                  free_thresh=f("free_thresh"), occupied_thresh=f("occupied_thresh"), device=device)
    if h["variant"] == 1:
        m = GPOctoMap(noise=f("noise"), l=f("l"), min_var=f("min_var"), max_var=f("max_var"), max_known_var=f("max_known_var"), **common)
    else:
        common.update(var_thresh=f("var_thresh"), prior_A=f("prior_A"), prior_B=f("prior_B"))
        if h["variant"] == 2:
            m = BGKLVOctoMap(original_size=bool(h["flags"] & 1), min_W=f("min_W"), **common)
        else:
            m = (BGKLOctoMap if h["variant"] == 3 else BGKOctoMap)(**common)
    if device >= 0 and m.is_device_resident() != bool(device_resident):
        m.set_device_resident(bool(device_resident))
    return m.load(path)


def poses_xyz_yaw(center, dxyz_dyaw):
    """Candidate poses for score_poses: row i of dxyz_dyaw = (dx, dy, dz, dyaw) gives the pose that rotates about `center`
    by dyaw (radians, about z) and then translates by (dx, dy, dz).  Returns (P, 3, 4) float32 [R | t].  Everything is
    computed in double and rounded to float32 once per entry — c = cos(dyaw), s = sin(dyaw) from libm (math.cos,
    math.sin), R = [[c, -s, 0], [s, c, 0], [0, 0, 1]], t = ((cx + dx) - (c * cx - s * cy), (cy + dy) - (s * cx + c * cy),
    dz) — so a C program that calls libm's cos and sin and does the same double arithmetic builds the same bits."""
    cx, cy = float(center[0]), float(center[1])
    rows = np.asarray(dxyz_dyaw, np.float64).reshape(-1, 4)
    out = np.zeros((rows.shape[0], 3, 4), np.float32)
    for i, (dx, dy, dz, dyaw) in enumerate(rows.tolist()):
        c, s = math.cos(dyaw), math.sin(dyaw)
        out[i] = [[c, -s, 0.0, (cx + dx) - (c * cx - s * cy)], [s, c, 0.0, (cy + dy) - (s * cx + c * cy)], [0.0, 0.0, 1.0, dz]]
    return out


def footprint_cells(radius):
    """N of footing: the cells (di, dj) of a disc of `radius` voxels without its centre, 0 < di^2 + dj^2 <= radius^2"""
    r = int(radius)
    if r < 0:
        raise ValueError("footprint_cells: radius must be >= 0")
    return sum(1 for di in range(-r, r + 1) for dj in range(-r, r + 1) if 0 < di * di + dj * dj <= r * r)


def surface_quads(index, faces, dims):
    """The exposed faces that surface() lists, as quads.  index, faces: surface's arrays; dims: the region's.  Returns
    (corners int32 [F, 4, 3], direction uint8 [F], voxel uint32 [F]): one quad per set bit of faces, in list order and then
    ascending direction d (0: -x, 1: +x, 2: -y, 3: +y, 4: -z, 5: +z); voxel = the flat index it belongs to.  Corners are in
    voxel-corner units of the region — the world position is origin + (corner - 0.5) * resolution — and run
    counter-clockwise seen from the open side: for a face along axis a with (b, c) = ((a + 1) % 3, (a + 2) % 3) the plane is
    v_a + 1 for the positive direction and v_a for the negative, the (b, c) offsets (0, 0), (1, 0), (1, 1), (0, 1) for the
    positive direction and in the reverse order for the negative.  Integers only."""
    index = np.ascontiguousarray(index, np.uint32).reshape(-1)
    faces = np.ascontiguousarray(faces, np.uint8).reshape(-1)
    nx, ny, nz = (int(v) for v in dims)
    if index.shape != faces.shape:
        raise ValueError("surface_quads: index and faces must have the same length")
    if index.size and int(index.max()) >= nx * ny * nz:
        raise ValueError("surface_quads: an index lies outside dims")
    bits = (faces[:, None] >> np.arange(6, dtype=np.uint8)[None, :]) & 1          # [n, 6]: list order, then ascending d
    entry, direction = np.nonzero(bits)
    voxel = index[entry]
    v = np.stack([voxel // (ny * nz), voxel // nz % ny, voxel % nz], 1).astype(np.int32)
    axis, positive = direction >> 1, (direction & 1).astype(np.int32)
    corners = np.repeat(v[:, None, :], 4, 1)                                      # [F, 4, 3]
    rows = np.arange(entry.size)
    ring = np.array(((0, 0), (1, 0), (1, 1), (0, 1)), np.int32)
    for t in range(4):
        off = np.where(positive[:, None] == 1, ring[t][None, :], ring[3 - t][None, :])
        corners[rows, t, axis] += positive
        corners[rows, t, (axis + 1) % 3] += off[:, 0]
        corners[rows, t, (axis + 2) % 3] += off[:, 1]
    return corners, direction.astype(np.uint8), voxel.astype(np.uint32)


def follow_parents(parent, dims, index):
    """The path from flat index `index` back to its seed through travel's `parent` array (any shape of prod(dims) codes): the
    flat indices, `index` first and the seed last.  Empty where `index` was not reached (code 255)."""
    par = np.asarray(parent).reshape(-1)
    ny, nz = int(dims[1]), int(dims[2])
    f, path = int(index), []
    while par[f] != 255:
        path.append(f)
        q = int(par[f])
        if q == 13:
            return np.array(path, np.int64)
        if len(path) > par.size:
            break
        f += ((q // 9 - 1) * ny + ((q // 3) % 3 - 1)) * nz + (q % 3 - 1)
    if path:
        raise ValueError("follow_parents: the parents do not lead to a seed")
    return np.zeros(0, np.int64)


def follow_drive_parents(parent, dims, index):
    """The route from flat index `index` back to its seed through drive's `parent` array (any shape of prod(dims) codes): the
    flat indices, `index` first and the seeded member last.  Empty where `index` was not reached (code 255)."""
    par = np.asarray(parent).reshape(-1)
    ny, nz = int(dims[1]), int(dims[2])
    f, path = int(index), []
    while par[f] != 255:
        path.append(f)
        q = int(par[f])
        if q == DRIVE_SEED_CODE:
            return np.array(path, np.int64)
        if q > 80 or len(path) > par.size:
            break
        f += ((q // 27 - 1) * ny + ((q // 9) % 3 - 1)) * nz + (q % 9 - 4)
    if path:
        raise ValueError("follow_drive_parents: the parents do not lead to a seed")
    return np.zeros(0, np.int64)
