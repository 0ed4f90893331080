"""The two pointer forms of every query on the device-resident map (la3dm_devmap_X_host / _device, csrc/devmap.hip) with
outputs left out: the host form stages device twins of the caller's arrays, and which twins exist and where they lie
depends on the outputs asked for.  On a bare la3dm_devmap, empty and after one scan, on a small and then a larger region
(so that the staging arenas grow between calls), every query is called in its host form with all outputs, with each
optional output alone besides the mandatory ones and with no optional output: every array returned equals the
all-outputs call bit for bit, and that call equals the device form on torch tensors.  Every host array is a view into a
larger buffer, one element off its alignment, between 16 guard elements of a sentinel on either side that no call may
touch; the device tensors carry the same guards.  A refused call between two served ones writes nothing."""
import ctypes as C

import numpy as np
import pytest

from conftest import pcd_path

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
INSERT = (0.1, 0.5, 8.0)      # ds_resolution, free_res, max_range of sim_structured
GUARD = 16
DIMS = ((5, 3, 7), (13, 11, 9))   # 105 and 1 287 voxels: neither a multiple of 4 or 16
FREE_M, OCC_M, OPEN_M = 0x1, 0x2, 0x1D   # classes FREE, OCCUPIED; every class but OCCUPIED
SENTINEL = {1: 0xA5, 4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}


class HostArray:
    """n elements one element into a buffer: [1 + GUARD sentinels | n | GUARD sentinels]"""

    def __init__(self, dtype, n, init=None):
        u = np.dtype(f"u{np.dtype(dtype).itemsize}")
        self.buf = np.full(1 + GUARD + n + GUARD, SENTINEL[u.itemsize], u)
        self.n, self.dtype = n, np.dtype(dtype)
        if init is not None:
            self.view()[:] = np.asarray(init, dtype).reshape(-1).view(u)
        self.ptr = self.buf.ctypes.data + (1 + GUARD) * u.itemsize
        assert self.ptr % 16 != 0

    def view(self):
        return self.buf[1 + GUARD:1 + GUARD + self.n]

    def bits(self):
        return self.view().copy()

    def guards_intact(self):
        s = SENTINEL[self.buf.itemsize]
        return bool((self.buf[:1 + GUARD] == s).all() and (self.buf[1 + GUARD + self.n:] == s).all())

    def untouched(self):
        return bool((self.buf == SENTINEL[self.buf.itemsize]).all())


class DeviceArray:
    """the same on a torch tensor: [GUARD sentinels | n | GUARD sentinels]"""

    def __init__(self, dtype, n, init=None):
        import torch
        u = np.dtype(f"u{np.dtype(dtype).itemsize}")
        host = np.full(GUARD + n + GUARD, SENTINEL[u.itemsize], u)
        if init is not None:
            host[GUARD:GUARD + n] = np.asarray(init, dtype).reshape(-1).view(u)
        self.t = torch.from_numpy(host.view(f"i{u.itemsize}")).to("cuda:0")
        torch.cuda.synchronize()
        self.n, self.u = n, u
        self.ptr = self.t.data_ptr() + GUARD * u.itemsize

    def _host(self):
        return self.t.cpu().numpy().view(self.u)

    def bits(self):
        return self._host()[GUARD:GUARD + self.n].copy()

    def guards_intact(self):
        h, s = self._host(), SENTINEL[self.u.itemsize]
        return bool((h[:GUARD] == s).all() and (h[GUARD + self.n:] == s).all())


class Query:
    """One call pattern of one query: `specs` name -> (dtype, elements) of every output array, `mandatory` the outputs no
    call may leave out (none_allowed: a call without any array is served too), `inputs` name -> array, and
    call(form, inputs' pointers, the pointers of the outputs asked for, dims pointer) -> (rc, scalars)."""

    def __init__(self, name, specs, mandatory, inputs, call, none_allowed=False):
        self.name, self.specs, self.inputs, self.call = name, specs, inputs, call
        optional = [k for k in specs if k not in mandatory]
        self.subsets = []   # all outputs first, then each optional one alone, then none of them
        for s in [tuple(specs)] + [tuple(mandatory) + (k,) for k in optional] + [tuple(mandatory)]:
            if (s or none_allowed) and s not in self.subsets:
                self.subsets.append(s)


def _queries(H, dm, lo, dims, rng):
    """the call patterns of the nine queries on the region (lo, dims)"""
    from la3dm_amd import _lib
    n = int(np.prod(dims))
    nx, ny, nz = dims
    lop = lo.ctypes.data
    u32, f32, u8, i32 = np.uint32, np.float32, np.uint8, np.int32
    centre = lo + np.array(dims, f32) * f32(0.05)
    out = []

    def struct(cls, ptrs):
        return cls(*[ptrs.get(k) for k, _ in cls._fields_])

    def info_of(info):
        return (info.block_key, tuple(info.cell), tuple(np.array(info.origin, f32).view(u32)))

    def stats_of(s):
        return tuple(getattr(s, k) for k, _ in s._fields_)

    # raycast: one ray per voxel of the region's size, from its centre
    rays = np.concatenate([np.tile(centre, (n, 1)), rng.uniform(-1, 1, (n, 3)).astype(f32)], axis=1).astype(f32)

    def raycast(form, i, o, dp, max_steps=64):
        fn = getattr(H, f"la3dm_devmap_raycast_{form}")
        return fn(dm, i["rays6"], n, OCC_M, max_steps, C.byref(struct(_lib.RaycastOut, o))), ()
    out.append(Query("raycast", dict(steps=(u32, n), flags=(u8, n), p=(f32, 3 * n), block_key=(np.int64, n), node_key=(i32, n), cls=(u8, n),
                                     leaf_depth=(u8, n), A=(f32, n), B=(f32, n), counts=(u32, 4 * n)), ("steps", "flags"), dict(rays6=rays), raycast))

    def region(name, cls):
        def call(form, i, o, dp):
            info = _lib.RegionInfo()
            rc = getattr(H, f"la3dm_devmap_{name}_{form}")(dm, lop, dp, C.byref(struct(cls, o)), C.byref(info))
            return rc, info_of(info)
        return call
    out.append(Query("box", dict(cls=(u8, n), leaf_depth=(u8, n), A=(f32, n), B=(f32, n)), ("cls",), {}, region("box", _lib.BoxOut)))
    nc = nx * ny
    out.append(Query("columns", dict(counts=(u32, 4 * nc), low_occ=(i32, nc), top_occ=(i32, nc)), ("counts",), {}, region("columns", _lib.ColumnsOut)))

    def distance(form, i, o, dp):
        info = _lib.RegionInfo()
        rc = getattr(H, f"la3dm_devmap_distance_{form}")(dm, lop, dp, OCC_M | 0x8, 3, C.byref(struct(_lib.DistanceOut, o)), C.byref(info))
        return rc, info_of(info)
    out.append(Query("distance", dict(d2=(u32, n), dist=(f32, n)), (), {}, distance))   # (either output alone; none is refused)

    for cap in (0, 3, n):
        def frontier(form, i, o, dp, cap=cap):
            info, found = _lib.RegionInfo(), C.c_uint64(0)
            rc = getattr(H, f"la3dm_devmap_frontier_{form}")(dm, lop, dp, FREE_M, 0xC, 6, 1, cap, C.byref(struct(_lib.FrontierOut, o)), C.byref(found),
                                                             C.byref(info))
            return rc, (found.value,) + info_of(info)
        out.append(Query(f"frontier cap {cap}", dict(index=(u32, cap), nbrs=(u8, cap), score=(u8, n)), ("index",) if cap else (), {}, frontier,
                         none_allowed=cap == 0))

    origins = (centre + rng.uniform(-0.1, 0.1, (2, 3))).astype(f32)
    offsets = rng.uniform(-1, 1, (5, 3)).astype(f32)
    for nv in (2, 0):
        def gain(form, i, o, dp, nv=nv):
            info = _lib.RegionInfo()
            rc = getattr(H, f"la3dm_devmap_gain_{form}")(dm, lop, dp, i["origins3"], nv, i["offsets3"], 5, 0xC, OCC_M, 64, C.byref(struct(_lib.GainOut, o)),
                                                         C.byref(info))
            return rc, info_of(info)
        W = (n + 31) // 32
        out.append(Query(f"gain n {nv}", dict(gain=(u32, 2), started=(u32, 2), hits=(u32, 2), seen=(u32, 2 * W)), ("gain",),
                         dict(origins3=origins, offsets3=offsets), gain))

    seeds, targets = np.array([0, n // 2], u32), np.array([1, n // 3, n - 1], u32)
    for nt in (3, 0):
        def reach(form, i, o, dp, nt=nt):
            info, stats = _lib.RegionInfo(), _lib.ReachStats()
            rc = getattr(H, f"la3dm_devmap_reach_{form}")(dm, lop, dp, i["seeds"], 2, OPEN_M, OCC_M, 1, 6, 64, i["targets"] if nt else None, nt,
                                                          C.byref(struct(_lib.ReachOut, o)), C.byref(stats), C.byref(info))
            return rc, stats_of(stats) + info_of(info)
        specs = dict(steps=(u32, n), target_steps=(u32, 3)) if nt else dict(steps=(u32, n))
        out.append(Query(f"reach targets {nt}", specs, ("target_steps",) if nt else ("steps",), dict(seeds=seeds, targets=targets), reach))

        def travel(form, i, o, dp, nt=nt):
            info, stats = _lib.RegionInfo(), _lib.TravelStats()
            p = _lib.TravelParams(OPEN_M, OCC_M, 0, 2, 4, (C.c_uint32 * 3)(1, 1, 1), 6, 1 << 31)
            rc = getattr(H, f"la3dm_devmap_travel_{form}")(dm, lop, dp, i["seeds"], 2, C.byref(p), i["targets"] if nt else None, nt,
                                                           C.byref(struct(_lib.TravelOut, o)), C.byref(stats), C.byref(info))
            return rc, stats_of(stats) + info_of(info)
        specs = dict(cost=(u32, n), target_cost=(u32, 3), parent=(u8, n)) if nt else dict(cost=(u32, n), parent=(u8, n))
        out.append(Query(f"travel targets {nt}", specs, ("target_cost",) if nt else ("cost",), dict(seeds=seeds, targets=targets), travel))

    members = np.array([0, 1, n // 2, n // 2 + 1, n - 1], u32)
    for cap, listed in ((0, False), (2, False), (2, True)):
        def clusters(form, i, o, dp, cap=cap, listed=listed):
            info, stats, found = _lib.RegionInfo(), _lib.ClustersStats(), C.c_uint32(0)
            p = _lib.ClustersParams(OPEN_M, 1 if listed else 0, 6, 0, 1, 5 if listed else 0, i["members"] if listed else None, cap)
            rc = getattr(H, f"la3dm_devmap_clusters_{form}")(dm, lop, dp, C.byref(p), C.byref(struct(_lib.ClustersOut, o)) if o else None,
                                                             C.byref(found), C.byref(stats), C.byref(info))
            return rc, (found.value,) + stats_of(stats) + info_of(info)
        specs = dict(label=(u32, n))
        if listed:
            specs["of_member"] = (u32, 5)
        specs.update(first=(u32, cap), size=(u32, cap), lo=(u32, 3 * cap), hi=(u32, 3 * cap), sum=(np.uint64, 3 * cap), rep=(u32, cap))
        out.append(Query(f"clusters cap {cap}{' listed' if listed else ''}", specs, ("first",) if cap else (), dict(members=members), clusters,
                         none_allowed=cap == 0))
    return out


@pytest.fixture(scope="module", params=["empty", "one scan"])
def devmap(request, built):
    import la3dm_amd
    from la3dm_amd import _lib
    H = _lib.hip()
    lender = la3dm_amd.BGKOctoMap(**la3dm_amd.BGK_YAML, device=0).set_device_resident(False)   # (lends its context)
    ctx = lender.ctx()
    dm = C.c_void_p()
    assert H.la3dm_devmap_create(ctx, C.byref(dm)) == OK
    xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", 1))
    if request.param == "one scan":
        o3 = (C.c_float * 3)(*[float(v) for v in origin])
        assert H.la3dm_devmap_insert_pointcloud_host(dm, np.ascontiguousarray(xyz, np.float32).ctypes.data, xyz.shape[0], 3, o3, *INSERT, None) == OK
    yield H, dm, ctx, np.asarray(origin, np.float32), request.param
    H.la3dm_devmap_destroy(dm)
    del lender


NAMES = ("raycast", "box", "columns", "distance", "frontier", "gain", "reach", "travel", "clusters")


@pytest.mark.parametrize("name", NAMES)
def test_outputs_left_out_and_both_forms(devmap, name):
    H, dm, ctx, origin, state = devmap
    err = lambda: H.la3dm_last_error(ctx).decode()   # noqa: E731
    rng = np.random.default_rng(7)
    for dims in DIMS:   # the small region first: the staging arenas grow at the second
        d3 = np.array(dims, np.uint32)
        zero = np.array((dims[0], 0, dims[2]), np.uint32)
        lo = (origin - np.array(dims, np.float32) * np.float32(0.05)).astype(np.float32)   # the sensor at the region's centre
        for q in [q for q in _queries(H, dm, lo, dims, rng) if q.name.split()[0] == name]:
            what = (state, dims, q.name)

            def run(form, subset, dp=d3.ctypes.data, **kw):
                arr = HostArray if form == "host" else DeviceArray
                ins = {k: arr(v.dtype, v.size, v) for k, v in q.inputs.items()}
                outs = {k: arr(*q.specs[k]) for k in q.specs}
                rc, scalars = q.call(form, {k: a.ptr for k, a in ins.items()}, {k: outs[k].ptr for k in subset}, dp, **kw)
                for k, a in list(ins.items()) + list(outs.items()):
                    assert a.guards_intact(), (what, form, subset, k)
                for k, a in ins.items():
                    assert (a.bits() == q.inputs[k].reshape(-1).view(a.bits().dtype)).all(), (what, form, subset, k)
                return rc, scalars, outs

            rc, scalars, full = run("host", q.subsets[0])
            assert rc == OK, (what, err())
            want = {k: a.bits() for k, a in full.items()}
            if state == "one scan" and q.name == "frontier cap 3":
                assert scalars[0] > 3, (what, scalars)   # the list is cut short: fewer entries copied than found
            for subset in q.subsets[1:]:
                rc, s2, got = run("host", subset)
                assert rc == OK, (what, subset, err())
                assert s2 == scalars, (what, subset, s2, scalars)
                for k, a in got.items():
                    if k in subset:
                        assert (a.bits() == want[k]).all(), (what, subset, k)
                    else:
                        assert a.untouched(), (what, subset, k)
            rc, s2, dev = run("device", q.subsets[0])
            assert rc == OK, (what, err())
            assert s2 == scalars, (what, s2, scalars)
            for k, a in dev.items():
                assert (a.bits() == want[k]).all(), (what, "device", k)
            # a refused call writes nothing, and the call after it answers as before
            if name == "raycast":
                rc, _, got = run("host", q.subsets[0], max_steps=0)
            else:
                rc, _, got = run("host", q.subsets[0], dp=zero.ctypes.data)
            assert rc == ERR_ARG and ("max_steps" if name == "raycast" else "dims must be >= 1") in err(), (what, rc, err())
            assert all(a.untouched() for a in got.values()), what
            rc, s2, again = run("host", q.subsets[0])
            assert rc == OK and s2 == scalars, (what, err())
            for k, a in again.items():
                assert (a.bits() == want[k]).all(), (what, "after a refusal", k)
