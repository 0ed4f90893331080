"""ctypes bindings of the two product libraries.

  libla3dm_hip.so   C ABI of the device hot path        (include/la3dm_hip.h)
  libla3dm_map.so   host-side BGKOctoMap, C view         (include/la3dm_map.h)

Both are built in-tree by la3dm_amd/csrc/Makefile.  There is no Python or CPU fallback:
if a library is missing or no HIP device is present, loading / map creation raises.
"""
import ctypes as C
import os

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
HIP_SO = os.path.join(_CSRC, "libla3dm_hip.so")
MAP_SO = os.path.join(_CSRC, "libla3dm_map.so")

class GatherSeg(C.Structure):
    """la3dm_gather_seg (include/la3dm_hip.h)"""
    _fields_ = [("base", C.c_void_p), ("offset", C.POINTER(C.c_uint64)), ("bytes", C.POINTER(C.c_uint64))]


# la3dm_allgatherv_fn: int fn(void *user, const la3dm_gather_seg *segs, uint32_t nseg, uint32_t world, uint32_t rank, void *stream)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(GatherSeg), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p)

LEAF_UPDATED = 0x80
SCAN_UPDATE_UNGATED = 0x1


class Params(C.Structure):
    _fields_ = [("resolution", C.c_float), ("block_depth", C.c_int32), ("sf2", C.c_float), ("ell", C.c_float),
                ("free_thresh", C.c_float), ("occupied_thresh", C.c_float), ("var_thresh", C.c_float),
                ("prior_A", C.c_float), ("prior_B", C.c_float), ("device", C.c_int32),
                ("lut_xyz", C.c_void_p), ("lut_count", C.c_uint32), ("variant", C.c_int32), ("noise", C.c_float),
                ("l", C.c_float), ("min_ivar", C.c_float), ("max_ivar", C.c_float), ("min_known_ivar", C.c_float), ("min_W", C.c_float)]


class BgkScan(C.Structure):
    _fields_ = [("train_xyzy", C.c_void_p), ("train_off", C.c_void_p), ("n_train_pts", C.c_uint32),
                ("n_train_blk", C.c_uint32), ("nbr", C.c_void_p), ("blk_center", C.c_void_p),
                ("leaf_off", C.c_void_p), ("n_test_blk", C.c_uint32), ("n_leaf", C.c_uint32),
                ("leaf_key", C.c_void_p), ("alpha", C.c_void_p), ("beta", C.c_void_p), ("state", C.c_void_p),
                ("flags", C.c_uint32), ("train_max_n", C.c_uint32), ("train_sum_n2", C.c_uint64)]


class LvScan(C.Structure):
    _fields_ = [("samples", C.c_void_p), ("sorted", C.c_void_p), ("n_samples", C.c_uint32), ("rays", C.c_void_p),
                ("n_rays", C.c_uint32), ("cell_off", C.c_void_p), ("cell_min", C.c_int32 * 3), ("cell_dim", C.c_int32 * 3),
                ("n_blk", C.c_uint32), ("blk_center", C.c_void_p), ("blk_cell0", C.c_void_p), ("alpha", C.c_void_p),
                ("beta", C.c_void_p), ("state", C.c_void_p)]


class BgkCounters(C.Structure):
    _fields_ = [("n_tiles", C.c_uint64), ("scratch_bytes", C.c_uint64)]


class _Stats(C.Structure):
    """what the statistics structures share"""

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ScanStats(_Stats):
    _fields_ = [(n, C.c_uint64) for n in ("n_hits", "n_frees", "n_bbox_blocks", "n_train_blocks", "n_test_blocks",
                                           "voxel_updates", "train_reads", "pair_evals", "n_tiles")] + \
               [(n, C.c_double) for n in ("t_frontend", "t_partition", "t_pack", "t_device", "t_commit", "t_prune",
                                          "t_total", "t_gather")]


class DevmapStats(_Stats):
    """la3dm_devmap_stats (include/la3dm_hip.h)"""
    _fields_ = [(k, C.c_uint64) for k in ("n_hits", "n_frees", "n_train_blocks", "n_test_blocks", "n_bbox_blocks",
                                          "voxel_updates", "train_reads", "pair_evals", "n_blocks")] + \
               [("n_passes", C.c_uint32)] + \
               [(k, C.c_double) for k in ("t_frontend", "t_partition", "t_pack", "t_kernel", "t_commit", "t_total", "t_gather")]


class RaycastOut(C.Structure):   # la3dm_raycast_out (include/la3dm_hip.h)
    _fields_ = [(k, C.c_void_p) for k in ("steps", "flags", "p", "block_key", "node_key", "cls", "leaf_depth", "A", "B",
                                          "counts")]


class BoxOut(C.Structure):       # la3dm_box_out
    _fields_ = [(k, C.c_void_p) for k in ("cls", "leaf_depth", "A", "B")]


class ColumnsOut(C.Structure):   # la3dm_columns_out
    _fields_ = [(k, C.c_void_p) for k in ("counts", "low_occ", "top_occ")]


class DistanceOut(C.Structure):  # la3dm_distance_out
    _fields_ = [(k, C.c_void_p) for k in ("d2", "dist")]


class FrontierOut(C.Structure):  # la3dm_frontier_out
    _fields_ = [(k, C.c_void_p) for k in ("index", "nbrs", "score")]


class GainOut(C.Structure):      # la3dm_gain_out
    _fields_ = [(k, C.c_void_p) for k in ("gain", "started", "hits", "seen")]


class ScoreOut(C.Structure):     # la3dm_score_out
    _fields_ = [(k, C.c_void_p) for k in ("sum_d2", "counts")]


class NearestOut(C.Structure):   # la3dm_nearest_out
    _fields_ = [(k, C.c_void_p) for k in ("index", "d2")]


class NearestPointsOut(C.Structure):   # la3dm_nearest_points_out
    _fields_ = [(k, C.c_void_p) for k in ("cls", "voxel", "index", "d2")]


class FootingParams(C.Structure):  # la3dm_footing_params
    _fields_ = [(k, C.c_uint32) for k in ("support_mask", "clear_mask", "headroom", "radius", "step", "min_support")]


class FootingOut(C.Structure):   # la3dm_footing_out
    _fields_ = [(k, C.c_void_p) for k in ("index", "levels", "lowest", "highest")]


class FootingStats(_Stats):   # la3dm_footing_stats
    _fields_ = [(k, C.c_uint32) for k in ("n_stand", "n_body", "n_foot", "disc_cells")]


class SurfaceParams(C.Structure):  # la3dm_surface_params
    _fields_ = [(k, C.c_uint32) for k in ("solid_mask", "open_mask", "smooth")]


class SurfaceOut(C.Structure):   # la3dm_surface_out
    _fields_ = [(k, C.c_void_p) for k in ("index", "faces", "normal", "dense_faces")]


class SurfaceStats(_Stats):   # la3dm_surface_stats
    _fields_ = [("n_solid", C.c_uint64), ("n_surface", C.c_uint64), ("faces", C.c_uint64 * 6)]

    def as_dict(self):
        return dict(n_solid=int(self.n_solid), n_surface=int(self.n_surface), face_count=tuple(int(v) for v in self.faces))


class PathsParams(C.Structure):  # la3dm_paths_params
    _fields_ = [("obstacle_mask", C.c_uint32), ("clearance", C.c_uint32), ("soft_radius", C.c_uint32), ("penalty", C.c_uint32),
                ("move_cost", C.c_uint32 * 3), ("max_steps", C.c_uint32)]


class PathsOut(C.Structure):     # la3dm_paths_out
    _fields_ = [(k, C.c_void_p) for k in ("cost", "steps", "stop", "min_d2", "ways", "flags")]


class ReachOut(C.Structure):     # la3dm_reach_out
    _fields_ = [(k, C.c_void_p) for k in ("steps", "target_steps")]


class ReachStats(_Stats):   # la3dm_reach_stats
    _fields_ = [(k, C.c_uint32) for k in ("n_seeded", "n_reached", "levels")]


class TravelParams(C.Structure):  # la3dm_travel_params
    _fields_ = [("pass_mask", C.c_uint32), ("obstacle_mask", C.c_uint32), ("clearance", C.c_uint32), ("soft_radius", C.c_uint32),
                ("penalty", C.c_uint32), ("move_cost", C.c_uint32 * 3), ("connectivity", C.c_uint32), ("max_cost", C.c_uint32)]


class TravelOut(C.Structure):    # la3dm_travel_out
    _fields_ = [(k, C.c_void_p) for k in ("cost", "target_cost", "parent")]


class TravelStats(_Stats):  # la3dm_travel_stats
    _fields_ = [(k, C.c_uint32) for k in ("n_seeded", "n_reached", "max_cost", "rounds", "brick_runs", "capped")]


class DriveParams(C.Structure):  # la3dm_drive_params
    _fields_ = [("members", C.c_void_p), ("footing", C.POINTER(FootingParams)), ("n_members", C.c_uint32), ("connectivity", C.c_uint32),
                ("step", C.c_uint32), ("snap", C.c_uint32), ("move_cost", C.c_uint32 * 2), ("climb_up", C.c_uint32),
                ("climb_down", C.c_uint32), ("max_cost", C.c_uint32)]


class DriveOut(C.Structure):     # la3dm_drive_out
    _fields_ = [(k, C.c_void_p) for k in ("cost", "parent", "of_member", "target_cost", "target_index")]


class DriveStats(_Stats):   # la3dm_drive_stats
    _fields_ = [(k, C.c_uint32) for k in ("n_members", "n_seeded", "n_reached", "max_cost", "rounds", "brick_runs", "capped")]


class ClustersParams(C.Structure):  # la3dm_clusters_params
    _fields_ = [(k, C.c_uint32) for k in ("member_mask", "from_list", "connectivity", "tile", "min_size", "n_members")] + \
               [("members", C.c_void_p), ("cap", C.c_uint32)]


class ClustersOut(C.Structure):    # la3dm_clusters_out
    _fields_ = [(k, C.c_void_p) for k in ("label", "of_member", "first", "size", "lo", "hi", "sum", "rep")]


class ClustersStats(_Stats):  # la3dm_clusters_stats
    _fields_ = [(k, C.c_uint32) for k in ("n_members", "n_clusters", "n_dropped", "largest", "rounds", "brick_runs", "capped")]


class RegionInfo(C.Structure):   # la3dm_region_info
    _fields_ = [("block_key", C.c_int64), ("cell", C.c_int32 * 3), ("origin", C.c_float * 3)]


class MergeStats(_Stats):   # la3dm_merge_stats
    _fields_ = [(k, C.c_uint64) for k in ("n_blocks", "n_created", "cells_kept", "cells_copied", "cells_fused")]


class DiffParams(C.Structure):   # la3dm_diff_params
    _fields_ = [(k, C.c_uint32) for k in ("pair_mask", "value_mask", "map_only")]


class DiffOut(C.Structure):      # la3dm_diff_out
    _fields_ = [(k, C.c_void_p) for k in ("block_key", "cell", "code", "centre", "A", "B")]


class DiffStats(_Stats):    # la3dm_diff_stats
    _fields_ = [(k, C.c_uint64) for k in ("n_stream_blocks", "n_map_only_blocks", "n_missing_now")] + \
               [("pairs", C.c_uint64 * 25), ("value_changed", C.c_uint64 * 5)]


class EraseStats(_Stats):   # la3dm_erase_stats
    _fields_ = [(k, C.c_uint64) for k in ("n_removed", "n_moved", "n_blocks")]


class PackHeader(C.Structure):   # la3dm_pack_header: the first 128 bytes of a map stream
    _fields_ = [("magic", C.c_char * 8)] + \
               [(k, C.c_uint32) for k in ("version", "header_bytes", "variant", "block_depth", "nodes_per_block", "flags")] + \
               [(k, C.c_uint64) for k in ("n_blocks", "n_leaves", "total_bytes")] + \
               [(k, C.c_float) for k in ("init_A", "init_B", "resolution", "sf2", "ell", "free_thresh", "occupied_thresh", "var_thresh",
                                         "prior_A", "prior_B", "noise", "l", "min_var", "max_var", "max_known_var", "min_W")] + \
               [("reserved", C.c_uint8 * 8)]


# -- the signatures: one table per library, name -> (restype, argtypes), from include/la3dm_hip.h and include/la3dm_map.h --
cint, u32, u64, i64, f32, vp, P = C.c_int, C.c_uint32, C.c_uint64, C.c_int64, C.c_float, C.c_void_p, C.POINTER
f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_INFO = P(RegionInfo)

# A query is served by la3dm_map_<view> and by la3dm_devmap_<stem>_host / _device, with one argument list after the handle:
# stem -> (view, the device map's pointer forms, that list)
QUERIES = {
    "raycast": ("raycast_many", ("host", "device"), [vp, u32, u32, u32, P(RaycastOut)]),
    "box": ("box", ("host", "device"), [vp, vp, P(BoxOut), _INFO]),
    "columns": ("columns", ("host", "device"), [vp, vp, P(ColumnsOut), _INFO]),
    "distance": ("distance_field", ("host", "device"), [vp, vp, u32, u32, P(DistanceOut), _INFO]),
    "frontier": ("frontier", ("host", "device"), [vp, vp] + [u32] * 4 + [u64, P(FrontierOut), P(u64), _INFO]),
    "gain": ("gain", ("host", "device"), [vp, vp, vp, u32, vp] + [u32] * 4 + [P(GainOut), _INFO]),
    "score_poses": ("score_poses", ("host", "device"), [vp, vp, vp, u32, vp] + [u32] * 3 + [P(ScoreOut), _INFO]),
    "score_paths": ("score_paths", ("host", "device"), [vp, vp, vp, u32, u32, P(PathsParams), P(PathsOut), _INFO]),
    "reach": ("reach", ("host", "device"), [vp, vp, vp] + [u32] * 6 + [vp, u32, P(ReachOut), P(ReachStats), _INFO]),
    "travel": ("travel", ("host", "device"), [vp, vp, vp, u32, P(TravelParams), vp, u32, P(TravelOut), P(TravelStats), _INFO]),
    "clusters": ("clusters", ("host", "device"), [vp, vp, P(ClustersParams), P(ClustersOut), P(u32), P(ClustersStats), _INFO]),
    "pack": ("pack", ("host",), [vp, u64, P(u64)]),
    "unpack": ("unpack", ("host",), [vp, u64]),
    "merge": ("merge", ("host",), [vp, u64, P(MergeStats)]),
    "diff": ("diff", ("host",), [vp, u64, P(DiffParams), u64, P(DiffOut), P(u64), P(DiffStats)]),
    "pack_region": ("pack_region", ("host",), [vp, vp, cint, vp, u64, P(u64)]),
    "erase_region": ("erase_region", ("host",), [vp, vp, cint, P(EraseStats)]),
}
# ... except at these entries, which take something else after the handle
QUERY_DIFFERS = {
    "la3dm_map_raycast_many": [f32p, u64, u32, u32, P(RaycastOut)],   # the rays as a numpy array, their number in 64 bits
    # the device map takes the box of block keys (int32 klo[3], khi[3]) that the map view derives from its two world points
    "la3dm_devmap_pack_region_host": [P(C.c_int32), P(C.c_int32), cint, vp, u64, P(u64)],
    "la3dm_devmap_erase_region_host": [P(C.c_int32), P(C.c_int32), cint, P(EraseStats)],
}


# nearest and nearest_points have the three forms of a query as well; they are declared entry by entry in the tables below:
# what follows the handle
_NEAREST = [vp, vp, u32, u32, P(NearestOut), _INFO]
_NEAREST_POINTS = [vp, vp, vp, u32, vp, u32, u32, P(NearestPointsOut), _INFO]
# ... and so has footing
_FOOTING = [vp, vp, P(FootingParams), u64, P(FootingOut), P(u64), P(FootingStats), _INFO]
_SURFACE = [vp, vp, P(SurfaceParams), u64, P(SurfaceOut), P(u64), P(SurfaceStats), _INFO]
# ... and drive: one row for its three forms
_DRIVE = {f"la3dm_{form}": (cint, [vp, vp, vp, vp, u32, P(DriveParams), vp, u32, P(DriveOut), P(DriveStats), _INFO])
          for form in ("map_drive", "devmap_drive_host", "devmap_drive_device")}


def _query_entries(of_map):
    """the queries' entries of one library's table"""
    out = {}
    for stem, (view, forms, args) in QUERIES.items():
        for n in [f"la3dm_map_{view}"] if of_map else [f"la3dm_devmap_{stem}_{f}" for f in forms]:
            out[n] = (cint, [vp] + QUERY_DIFFERS.get(n, args))
    return out


HIP_API = {
    "la3dm_device_count": (cint, []),
    "la3dm_version": (C.c_char_p, []),
    "la3dm_create": (cint, [P(Params), P(vp)]),
    "la3dm_destroy": (None, [vp]),
    "la3dm_last_error": (C.c_char_p, [vp]),
    "la3dm_set_option": (cint, [vp, C.c_char_p, cint]),
    "la3dm_get_option": (cint, [vp, C.c_char_p, P(cint)]),
    **{f"la3dm_{kind}_scan_{form}": (cint, [vp, P(scan)] + stream + [P(BgkCounters)])
       for kind, scan in (("bgk", BgkScan), ("bgkl", BgkScan), ("gp", BgkScan), ("bgklv", LvScan))
       for form, stream in (("host", []), ("device", [vp]))},
    "la3dm_kernel_times": (cint, [vp, vp, u32, P(u32)]),
    "la3dm_diag_eval": (cint, [vp, cint, vp, u32, vp]),
    "la3dm_diag_sweep": (cint, [vp, cint, u32, u32, P(u64)]),
    "la3dm_diag_mfma_chain": (cint, [vp, vp, vp, cint, P(u32)]),
    "la3dm_pack_info": (cint, [vp, u64, P(PackHeader)]),
    "la3dm_devmap_create": (cint, [vp, P(vp)]),
    "la3dm_devmap_destroy": (None, [vp]),
    "la3dm_devmap_insert_pointcloud_host": (cint, [vp, vp, u32, u32, vp, f32, f32, f32, P(DevmapStats)]),
    "la3dm_devmap_insert_pointcloud_device": (cint, [vp, vp, u32, vp, f32, f32, f32, P(DevmapStats)]),
    "la3dm_devmap_insert_training_data_host": (cint, [vp, vp, u32, P(DevmapStats)]),
    "la3dm_devmap_wait_event": (cint, [vp, vp]),
    "la3dm_devmap_set_shard": (cint, [vp, u32, u32, ALLGATHER_FN, vp]),
    "la3dm_devmap_lv_stats_get": (cint, [vp, vp]),   # (la3dm_devmap_lv_stats has no Structure here: nothing in Python reads it)
    "la3dm_devmap_lv_set_original_size": (cint, [vp, cint]),
    "la3dm_devmap_lv_training": (cint, [vp, vp, u32, vp, u32, P(u32), P(u32)]),
    "la3dm_devmap_block_count": (cint, [vp, P(u32), P(u32)]),
    "la3dm_devmap_download": (cint, [vp] * 5),
    "la3dm_devmap_training_data": (cint, [vp, vp, u32, P(u32)]),
    "la3dm_devmap_export_cells": (cint, [vp, cint, cint, f32, f32, vp, vp, vp, u64, P(u64)]),
    "la3dm_devmap_key_bounds": (cint, [vp, P(C.c_int32), P(C.c_int32)]),
    "la3dm_devmap_search_host": (cint, [vp, vp, u32] + [vp] * 4),
    "la3dm_devmap_diag_add_repeat": (cint, [vp] * 4 + [u32] + [vp] * 2),
    "la3dm_devmap_diag_scan": (cint, [vp, cint, vp, u32, vp, vp]),
    "la3dm_devmap_diag_sort": (cint, [vp, vp, vp, u32, cint, vp, vp]),
    "la3dm_devmap_nearest_host": (cint, [vp] + _NEAREST),
    "la3dm_devmap_nearest_device": (cint, [vp] + _NEAREST),
    "la3dm_devmap_nearest_points_host": (cint, [vp] + _NEAREST_POINTS),
    "la3dm_devmap_nearest_points_device": (cint, [vp] + _NEAREST_POINTS),
    "la3dm_devmap_footing_host": (cint, [vp] + _FOOTING),
    "la3dm_devmap_footing_device": (cint, [vp] + _FOOTING),
    "la3dm_devmap_surface_host": (cint, [vp] + _SURFACE),
    "la3dm_devmap_surface_device": (cint, [vp] + _SURFACE),
    **{n: sig for n, sig in _DRIVE.items() if n.startswith("la3dm_devmap_")},
    **_query_entries(of_map=False),
}

_CREATE = [f32, cint] + [f32] * 7 + [cint]       # resolution, block_depth, seven parameters, device
_CLOUD = [vp, f32p, u64, f32p, f32, f32, f32]    # xyz, n, origin, ds_resolution, free_res, max_range
MAP_API = {
    "la3dm_map_create": (vp, _CREATE),
    "la3dm_map_create_l": (vp, _CREATE),
    "la3dm_map_create_gp": (vp, [f32, cint] + [f32] * 9 + [cint]),
    "la3dm_map_create_lv": (vp, [f32, cint] + [f32] * 7 + [cint, f32, cint]),
    "la3dm_map_destroy": (None, [vp]),
    "la3dm_map_last_error": (C.c_char_p, []),
    "la3dm_map_l_training": (u64, [vp, vp, u64, vp, u64, P(u64)]),
    "la3dm_map_lv_training": (u64, [vp, vp, u64, vp, u64, P(u64)]),
    "la3dm_map_lv_stats": (cint, [vp, np.ctypeslib.ndpointer(np.float64)]),
    "la3dm_map_lv_prepare": (cint, _CLOUD),
    "la3dm_map_lv_packed": (cint, [vp, P(LvScan)]),
    "la3dm_map_lv_commit": (cint, [vp]),
    "la3dm_map_insert_pointcloud": (cint, _CLOUD),
    "la3dm_map_insert_pointcloud_device": (cint, [vp, vp, u64, f32p, f32, f32, f32]),
    "la3dm_map_insert_training_data": (cint, [vp, f32p, u64]),
    "la3dm_map_prepare": (cint, _CLOUD),
    "la3dm_map_prepare_training_data": (cint, [vp, f32p, u64, cint]),
    "la3dm_map_packed": (cint, [vp, P(BgkScan)]),
    "la3dm_map_commit": (cint, [vp]),
    "la3dm_map_ctx": (vp, [vp]),
    "la3dm_map_set_device_resident": (cint, [vp, cint]),
    "la3dm_map_is_device_resident": (cint, [vp]),
    "la3dm_map_set_shard": (cint, [vp, u32, u32, ALLGATHER_FN, vp]),
    "la3dm_map_mirror_syncs": (u64, [vp]),
    "la3dm_map_stats": (cint, [vp, P(ScanStats)]),
    "la3dm_map_training_size": (u64, [vp]),
    "la3dm_map_training_data": (cint, [vp, f32p, u64]),
    "la3dm_map_block_size": (f32, [vp]),
    "la3dm_map_resolution": (f32, [vp]),
    "la3dm_map_block_depth": (cint, [vp]),
    "la3dm_map_set_resolution": (cint, [vp, f32]),
    "la3dm_map_set_block_depth": (cint, [vp, cint]),
    "la3dm_map_block_count": (u64, [vp]),
    "la3dm_map_leaf_count": (u64, [vp]),
    "la3dm_map_dump_leaves": (u64, [vp] * 9 + [u64]),
    "la3dm_map_search": (cint, [vp, f32, f32, f32, P(f32), P(f32), P(C.c_uint8)]),
    "la3dm_map_search_many": (cint, [vp, f32p, u64] + [vp] * 4),
    "la3dm_map_raycast": (u64, [vp, f32p, f32p] + [vp] * 7 + [u64]),
    "la3dm_map_export_cells": (cint, [vp, cint, cint, f32, f32, vp, vp, vp, u64, P(u64)]),
    "la3dm_map_get_bbox": (cint, [vp, f32p, f32p]),
    "la3dm_map_block_grid": (None, [vp, f32p, f32p, np.ctypeslib.ndpointer(np.int32), P(C.c_int32), f32p]),
    "la3dm_map_block_to_hash_key": (i64, [vp, f32, f32, f32]),
    "la3dm_map_hash_key_to_block": (None, [vp, i64, f32p]),
    "la3dm_map_extended_block": (None, [vp, i64, np.ctypeslib.ndpointer(np.int64)]),
    "la3dm_map_lut": (u32, [vp, vp, u32]),
    "la3dm_map_save": (cint, [vp, C.c_char_p]),
    "la3dm_map_load": (cint, [vp, C.c_char_p]),
    # the file forms have no device-map counterpart: a path where the stream (or, for evict_file, the buffer) stands
    "la3dm_map_merge_file": (cint, [vp, C.c_char_p, P(MergeStats)]),
    "la3dm_map_diff_file": (cint, [vp, C.c_char_p] + QUERIES["diff"][2][2:]),
    "la3dm_map_evict": (cint, [vp] + QUERIES["pack_region"][2] + [P(EraseStats)]),
    "la3dm_map_evict_file": (cint, [vp, C.c_char_p, vp, vp, cint, P(EraseStats)]),
    "la3dm_map_nearest": (cint, [vp] + _NEAREST),
    "la3dm_map_nearest_points": (cint, [vp] + _NEAREST_POINTS),
    "la3dm_map_footing": (cint, [vp] + _FOOTING),
    "la3dm_map_surface": (cint, [vp] + _SURFACE),
    "la3dm_map_drive": _DRIVE["la3dm_map_drive"],
    **_query_entries(of_map=True),
}
HIP_SYMBOLS = list(HIP_API)
MAP_SYMBOLS = list(MAP_API)


def _load(path, table, **kw):
    """the library at `path` with the restype and argtypes of every entry of `table` set"""
    L = C.CDLL(path, **kw)
    for name, (restype, argtypes) in table.items():
        f = getattr(L, name)
        f.restype = restype
        f.argtypes = argtypes
    return L


_hip = None
_map = None


def hip():
    """libla3dm_hip.so (raises OSError if it has not been built)."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_SO):
            raise OSError(f"{HIP_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no fallback path)")
        _hip = _load(HIP_SO, HIP_API, mode=C.RTLD_GLOBAL)
    return _hip


def maplib():
    global _map
    if _map is None:
        hip()
        if not os.path.exists(MAP_SO):
            raise OSError(f"{MAP_SO} is missing: build it first (no fallback path)")
        _map = _load(MAP_SO, MAP_API)
    return _map
