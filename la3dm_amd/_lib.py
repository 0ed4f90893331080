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


class ScanStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_hits", "n_frees", "n_bbox_blocks", "n_train_blocks", "n_test_blocks",
                                           "voxel_updates", "train_reads", "pair_evals", "n_tiles")] + \
               [(n, C.c_double) for n in ("t_frontend", "t_partition", "t_pack", "t_device", "t_commit", "t_prune",
                                          "t_total", "t_gather")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DevmapStats(C.Structure):
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


class PathsParams(C.Structure):  # la3dm_paths_params
    _fields_ = [("obstacle_mask", C.c_uint32), ("clearance", C.c_uint32), ("soft_radius", C.c_uint32), ("penalty", C.c_uint32),
                ("move_cost", C.c_uint32 * 3), ("max_steps", C.c_uint32)]


class PathsOut(C.Structure):     # la3dm_paths_out
    _fields_ = [(k, C.c_void_p) for k in ("cost", "steps", "stop", "min_d2", "ways", "flags")]


class ReachOut(C.Structure):     # la3dm_reach_out
    _fields_ = [(k, C.c_void_p) for k in ("steps", "target_steps")]


class ReachStats(C.Structure):   # la3dm_reach_stats
    _fields_ = [(k, C.c_uint32) for k in ("n_seeded", "n_reached", "levels")]


class TravelParams(C.Structure):  # la3dm_travel_params
    _fields_ = [("pass_mask", C.c_uint32), ("obstacle_mask", C.c_uint32), ("clearance", C.c_uint32), ("soft_radius", C.c_uint32),
                ("penalty", C.c_uint32), ("move_cost", C.c_uint32 * 3), ("connectivity", C.c_uint32), ("max_cost", C.c_uint32)]


class TravelOut(C.Structure):    # la3dm_travel_out
    _fields_ = [(k, C.c_void_p) for k in ("cost", "target_cost", "parent")]


class TravelStats(C.Structure):  # la3dm_travel_stats
    _fields_ = [(k, C.c_uint32) for k in ("n_seeded", "n_reached", "max_cost", "rounds", "brick_runs", "capped")]


class ClustersParams(C.Structure):  # la3dm_clusters_params
    _fields_ = [(k, C.c_uint32) for k in ("member_mask", "from_list", "connectivity", "tile", "min_size", "n_members")] + \
               [("members", C.c_void_p), ("cap", C.c_uint32)]


class ClustersOut(C.Structure):    # la3dm_clusters_out
    _fields_ = [(k, C.c_void_p) for k in ("label", "of_member", "first", "size", "lo", "hi", "sum", "rep")]


class ClustersStats(C.Structure):  # la3dm_clusters_stats
    _fields_ = [(k, C.c_uint32) for k in ("n_members", "n_clusters", "n_dropped", "largest", "rounds", "brick_runs", "capped")]


class RegionInfo(C.Structure):   # la3dm_region_info
    _fields_ = [("block_key", C.c_int64), ("cell", C.c_int32 * 3), ("origin", C.c_float * 3)]


class MergeStats(C.Structure):   # la3dm_merge_stats
    _fields_ = [(k, C.c_uint64) for k in ("n_blocks", "n_created", "cells_kept", "cells_copied", "cells_fused")]


class DiffParams(C.Structure):   # la3dm_diff_params
    _fields_ = [(k, C.c_uint32) for k in ("pair_mask", "value_mask", "map_only")]


class DiffOut(C.Structure):      # la3dm_diff_out
    _fields_ = [(k, C.c_void_p) for k in ("block_key", "cell", "code", "centre", "A", "B")]


class DiffStats(C.Structure):    # la3dm_diff_stats
    _fields_ = [(k, C.c_uint64) for k in ("n_stream_blocks", "n_map_only_blocks", "n_missing_now")] + \
               [("pairs", C.c_uint64 * 25), ("value_changed", C.c_uint64 * 5)]


class EraseStats(C.Structure):   # la3dm_erase_stats
    _fields_ = [(k, C.c_uint64) for k in ("n_removed", "n_moved", "n_blocks")]


class PackHeader(C.Structure):   # la3dm_pack_header: the first 128 bytes of a map stream
    _fields_ = [("magic", C.c_char * 8)] + \
               [(k, C.c_uint32) for k in ("version", "header_bytes", "variant", "block_depth", "nodes_per_block", "flags")] + \
               [(k, C.c_uint64) for k in ("n_blocks", "n_leaves", "total_bytes")] + \
               [(k, C.c_float) for k in ("init_A", "init_B", "resolution", "sf2", "ell", "free_thresh", "occupied_thresh", "var_thresh",
                                         "prior_A", "prior_B", "noise", "l", "min_var", "max_var", "max_known_var", "min_W")] + \
               [("reserved", C.c_uint8 * 8)]


HIP_SYMBOLS = ["la3dm_device_count", "la3dm_version", "la3dm_create", "la3dm_destroy", "la3dm_last_error",
               "la3dm_set_option", "la3dm_get_option", "la3dm_bgk_scan_host", "la3dm_bgk_scan_device", "la3dm_gp_scan_host",
               "la3dm_gp_scan_device", "la3dm_bgklv_scan_host", "la3dm_bgklv_scan_device", "la3dm_kernel_times", "la3dm_diag_eval", "la3dm_diag_sweep",
               "la3dm_devmap_create", "la3dm_devmap_destroy", "la3dm_devmap_insert_pointcloud_host",
               "la3dm_devmap_insert_pointcloud_device", "la3dm_devmap_block_count", "la3dm_devmap_download",
               "la3dm_devmap_training_data", "la3dm_devmap_diag_add_repeat", "la3dm_bgkl_scan_host",
               "la3dm_bgkl_scan_device", "la3dm_diag_mfma_chain", "la3dm_devmap_search_host",
               "la3dm_devmap_export_cells", "la3dm_devmap_key_bounds",
               "la3dm_devmap_insert_training_data_host", "la3dm_devmap_set_shard", "la3dm_devmap_wait_event",
               "la3dm_devmap_lv_stats_get", "la3dm_devmap_lv_set_original_size", "la3dm_devmap_lv_training",
               "la3dm_devmap_diag_scan", "la3dm_devmap_diag_sort", "la3dm_devmap_raycast_host",
               "la3dm_devmap_raycast_device", "la3dm_devmap_box_host", "la3dm_devmap_box_device",
               "la3dm_devmap_columns_host", "la3dm_devmap_columns_device", "la3dm_devmap_distance_host",
               "la3dm_devmap_distance_device", "la3dm_devmap_frontier_host", "la3dm_devmap_frontier_device",
               "la3dm_devmap_gain_host", "la3dm_devmap_gain_device", "la3dm_devmap_score_poses_host",
               "la3dm_devmap_score_poses_device", "la3dm_devmap_score_paths_host", "la3dm_devmap_score_paths_device",
               "la3dm_devmap_reach_host",
               "la3dm_devmap_reach_device", "la3dm_devmap_travel_host", "la3dm_devmap_travel_device",
               "la3dm_devmap_clusters_host", "la3dm_devmap_clusters_device",
               "la3dm_devmap_pack_host", "la3dm_devmap_unpack_host", "la3dm_pack_info", "la3dm_devmap_merge_host",
               "la3dm_devmap_diff_host",
               "la3dm_devmap_pack_region_host", "la3dm_devmap_erase_region_host"]
MAP_SYMBOLS = ["la3dm_map_create", "la3dm_map_create_gp", "la3dm_map_create_lv", "la3dm_map_lv_training",
               "la3dm_map_lv_stats", "la3dm_map_lv_prepare", "la3dm_map_lv_packed", "la3dm_map_lv_commit", "la3dm_map_destroy", "la3dm_map_last_error", "la3dm_map_insert_pointcloud", "la3dm_map_insert_pointcloud_device",
               "la3dm_map_insert_training_data", "la3dm_map_prepare", "la3dm_map_prepare_training_data",
               "la3dm_map_packed", "la3dm_map_commit", "la3dm_map_ctx", "la3dm_map_stats", "la3dm_map_training_size",
               "la3dm_map_training_data", "la3dm_map_block_size", "la3dm_map_block_count", "la3dm_map_leaf_count",
               "la3dm_map_dump_leaves", "la3dm_map_search", "la3dm_map_get_bbox", "la3dm_map_block_to_hash_key",
               "la3dm_map_hash_key_to_block", "la3dm_map_extended_block", "la3dm_map_lut",
               "la3dm_map_set_device_resident", "la3dm_map_is_device_resident", "la3dm_map_raycast",
               "la3dm_map_block_grid", "la3dm_map_create_l", "la3dm_map_l_training",
               "la3dm_map_search_many", "la3dm_map_export_cells", "la3dm_map_set_shard", "la3dm_map_resolution",
               "la3dm_map_block_depth", "la3dm_map_set_resolution", "la3dm_map_set_block_depth",
               "la3dm_map_raycast_many", "la3dm_map_mirror_syncs", "la3dm_map_box", "la3dm_map_columns",
               "la3dm_map_distance_field", "la3dm_map_frontier", "la3dm_map_gain", "la3dm_map_score_poses", "la3dm_map_reach",
               "la3dm_map_score_paths",
               "la3dm_map_travel", "la3dm_map_clusters", "la3dm_map_pack", "la3dm_map_unpack", "la3dm_map_save",
               "la3dm_map_load", "la3dm_map_merge", "la3dm_map_merge_file", "la3dm_map_diff", "la3dm_map_diff_file", "la3dm_map_pack_region",
               "la3dm_map_erase_region", "la3dm_map_evict", "la3dm_map_evict_file"]

_hip = None
_map = None


def hip():
    """libla3dm_hip.so (raises OSError if it has not been built)."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_SO):
            raise OSError(f"{HIP_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no fallback path)")
        L = C.CDLL(HIP_SO, mode=C.RTLD_GLOBAL)
        L.la3dm_device_count.restype = C.c_int
        L.la3dm_version.restype = C.c_char_p
        L.la3dm_create.restype = C.c_int
        L.la3dm_create.argtypes = [C.POINTER(Params), C.POINTER(C.c_void_p)]
        L.la3dm_destroy.argtypes = [C.c_void_p]
        L.la3dm_last_error.restype = C.c_char_p
        L.la3dm_last_error.argtypes = [C.c_void_p]
        L.la3dm_set_option.restype = C.c_int
        L.la3dm_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.la3dm_get_option.restype = C.c_int
        L.la3dm_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
        L.la3dm_bgk_scan_host.restype = C.c_int
        L.la3dm_bgk_scan_host.argtypes = [C.c_void_p, C.POINTER(BgkScan), C.POINTER(BgkCounters)]
        L.la3dm_bgk_scan_device.restype = C.c_int
        L.la3dm_bgk_scan_device.argtypes = [C.c_void_p, C.POINTER(BgkScan), C.c_void_p, C.POINTER(BgkCounters)]
        L.la3dm_diag_mfma_chain.restype = C.c_int
        L.la3dm_diag_mfma_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]
        L.la3dm_bgkl_scan_host.restype = C.c_int
        L.la3dm_bgkl_scan_host.argtypes = [C.c_void_p, C.POINTER(BgkScan), C.POINTER(BgkCounters)]
        L.la3dm_bgkl_scan_device.restype = C.c_int
        L.la3dm_bgkl_scan_device.argtypes = [C.c_void_p, C.POINTER(BgkScan), C.c_void_p, C.POINTER(BgkCounters)]
        L.la3dm_gp_scan_host.restype = C.c_int
        L.la3dm_gp_scan_host.argtypes = [C.c_void_p, C.POINTER(BgkScan), C.POINTER(BgkCounters)]
        L.la3dm_gp_scan_device.restype = C.c_int
        L.la3dm_gp_scan_device.argtypes = [C.c_void_p, C.POINTER(BgkScan), C.c_void_p, C.POINTER(BgkCounters)]
        L.la3dm_bgklv_scan_host.restype = C.c_int
        L.la3dm_bgklv_scan_host.argtypes = [C.c_void_p, C.POINTER(LvScan), C.POINTER(BgkCounters)]
        L.la3dm_bgklv_scan_device.restype = C.c_int
        L.la3dm_bgklv_scan_device.argtypes = [C.c_void_p, C.POINTER(LvScan), C.c_void_p, C.POINTER(BgkCounters)]
        L.la3dm_kernel_times.restype = C.c_int
        L.la3dm_kernel_times.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.la3dm_diag_sweep.restype = C.c_int
        L.la3dm_diag_sweep.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        L.la3dm_diag_eval.restype = C.c_int
        L.la3dm_diag_eval.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
        L.la3dm_devmap_create.restype = C.c_int
        L.la3dm_devmap_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.la3dm_devmap_destroy.argtypes = [C.c_void_p]
        L.la3dm_devmap_insert_pointcloud_host.restype = C.c_int
        L.la3dm_devmap_insert_pointcloud_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                                          C.c_float, C.c_float, C.c_float, C.POINTER(DevmapStats)]
        L.la3dm_devmap_insert_pointcloud_device.restype = C.c_int
        L.la3dm_devmap_insert_pointcloud_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_float,
                                                            C.c_float, C.c_float, C.POINTER(DevmapStats)]
        L.la3dm_devmap_block_count.restype = C.c_int
        L.la3dm_devmap_block_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.la3dm_devmap_download.restype = C.c_int
        L.la3dm_devmap_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.la3dm_devmap_diag_add_repeat.restype = C.c_int
        L.la3dm_devmap_diag_scan.restype = C.c_int
        L.la3dm_devmap_diag_scan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.la3dm_devmap_diag_sort.restype = C.c_int
        L.la3dm_devmap_diag_sort.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
        L.la3dm_devmap_diag_add_repeat.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 2
        L.la3dm_devmap_search_host.restype = C.c_int
        L.la3dm_devmap_search_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
        L.la3dm_devmap_raycast_host.restype = C.c_int
        L.la3dm_devmap_raycast_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RaycastOut)]
        L.la3dm_devmap_raycast_device.restype = C.c_int
        L.la3dm_devmap_raycast_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RaycastOut)]
        for name, out in (("box", BoxOut), ("columns", ColumnsOut)):
            for form in ("host", "device"):
                f = getattr(L, f"la3dm_devmap_{name}_{form}")
                f.restype = C.c_int
                f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(out), C.POINTER(RegionInfo)]
        for form in ("host", "device"):
            f = getattr(L, f"la3dm_devmap_distance_{form}")
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DistanceOut), C.POINTER(RegionInfo)]
        for form in ("host", "device"):
            f = getattr(L, f"la3dm_devmap_frontier_{form}")
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_uint64, C.POINTER(FrontierOut),
                                                                                   C.POINTER(C.c_uint64), C.POINTER(RegionInfo)]
        for form in ("host", "device"):
            f = getattr(L, f"la3dm_devmap_gain_{form}")
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p] + [C.c_uint32] * 4 + \
                         [C.POINTER(GainOut), C.POINTER(RegionInfo)]
        for form in ("host", "device"):
            f = getattr(L, f"la3dm_devmap_score_poses_{form}")
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p] + [C.c_uint32] * 3 + \
                         [C.POINTER(ScoreOut), C.POINTER(RegionInfo)]
        for form in ("host", "device"):
            f = getattr(L, f"la3dm_devmap_score_paths_{form}")
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PathsParams),
                          C.POINTER(PathsOut), C.POINTER(RegionInfo)]
        for form in ("host", "device"):
            f = getattr(L, f"la3dm_devmap_reach_{form}")
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + \
                         [C.c_void_p, C.c_uint32, C.POINTER(ReachOut), C.POINTER(ReachStats), C.POINTER(RegionInfo)]
        for form in ("host", "device"):
            f = getattr(L, f"la3dm_devmap_travel_{form}")
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(TravelParams), C.c_void_p, C.c_uint32,
                          C.POINTER(TravelOut), C.POINTER(TravelStats), C.POINTER(RegionInfo)]
        for form in ("host", "device"):
            f = getattr(L, f"la3dm_devmap_clusters_{form}")
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ClustersParams), C.POINTER(ClustersOut), C.POINTER(C.c_uint32),
                          C.POINTER(ClustersStats), C.POINTER(RegionInfo)]
        L.la3dm_devmap_pack_host.restype = C.c_int
        L.la3dm_devmap_pack_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.la3dm_devmap_unpack_host.restype = C.c_int
        L.la3dm_devmap_unpack_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.la3dm_devmap_merge_host.restype = C.c_int
        L.la3dm_devmap_merge_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(MergeStats)]
        L.la3dm_devmap_diff_host.restype = C.c_int
        L.la3dm_devmap_diff_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(DiffParams), C.c_uint64, C.POINTER(DiffOut),
                                             C.POINTER(C.c_uint64), C.POINTER(DiffStats)]
        L.la3dm_devmap_pack_region_host.restype = C.c_int
        L.la3dm_devmap_pack_region_host.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_uint64,
                                                    C.POINTER(C.c_uint64)]
        L.la3dm_devmap_erase_region_host.restype = C.c_int
        L.la3dm_devmap_erase_region_host.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.POINTER(EraseStats)]
        L.la3dm_pack_info.restype = C.c_int
        L.la3dm_pack_info.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(PackHeader)]
        L.la3dm_devmap_training_data.restype = C.c_int
        L.la3dm_devmap_training_data.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        _hip = L
    return _hip


def maplib():
    global _map
    if _map is None:
        hip()
        if not os.path.exists(MAP_SO):
            raise OSError(f"{MAP_SO} is missing: build it first (no fallback path)")
        M = C.CDLL(MAP_SO)
        f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
        M.la3dm_map_create.restype = C.c_void_p
        M.la3dm_map_create.argtypes = [C.c_float, C.c_int] + [C.c_float] * 7 + [C.c_int]
        M.la3dm_map_create_l.restype = C.c_void_p
        M.la3dm_map_create_l.argtypes = [C.c_float, C.c_int] + [C.c_float] * 7 + [C.c_int]
        M.la3dm_map_l_training.restype = C.c_uint64
        M.la3dm_map_l_training.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        M.la3dm_map_create_gp.restype = C.c_void_p
        M.la3dm_map_create_gp.argtypes = [C.c_float, C.c_int] + [C.c_float] * 9 + [C.c_int]
        M.la3dm_map_create_lv.restype = C.c_void_p
        M.la3dm_map_create_lv.argtypes = [C.c_float, C.c_int] + [C.c_float] * 7 + [C.c_int, C.c_float, C.c_int]
        M.la3dm_map_lv_training.restype = C.c_uint64
        M.la3dm_map_lv_training.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        M.la3dm_map_lv_stats.argtypes = [C.c_void_p, np.ctypeslib.ndpointer(np.float64)]
        M.la3dm_map_lv_prepare.restype = C.c_int
        M.la3dm_map_lv_prepare.argtypes = [C.c_void_p, f32p, C.c_uint64, f32p, C.c_float, C.c_float, C.c_float]
        M.la3dm_map_lv_packed.restype = C.c_int
        M.la3dm_map_lv_packed.argtypes = [C.c_void_p, C.POINTER(LvScan)]
        M.la3dm_map_lv_commit.restype = C.c_int
        M.la3dm_map_lv_commit.argtypes = [C.c_void_p]
        M.la3dm_map_destroy.argtypes = [C.c_void_p]
        M.la3dm_map_block_grid.argtypes = [C.c_void_p, f32p, f32p, np.ctypeslib.ndpointer(np.int32), C.POINTER(C.c_int32), f32p]
        M.la3dm_map_search_many.restype = C.c_int
        M.la3dm_map_search_many.argtypes = [C.c_void_p, f32p, C.c_uint64] + [C.c_void_p] * 4
        M.la3dm_map_export_cells.restype = C.c_int
        M.la3dm_map_export_cells.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        M.la3dm_map_raycast_many.restype = C.c_int
        M.la3dm_map_raycast_many.argtypes = [C.c_void_p, f32p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(RaycastOut)]
        M.la3dm_map_box.restype = C.c_int
        M.la3dm_map_box.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BoxOut), C.POINTER(RegionInfo)]
        M.la3dm_map_columns.restype = C.c_int
        M.la3dm_map_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ColumnsOut), C.POINTER(RegionInfo)]
        M.la3dm_map_distance_field.restype = C.c_int
        M.la3dm_map_distance_field.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DistanceOut),
                                               C.POINTER(RegionInfo)]
        M.la3dm_map_frontier.restype = C.c_int
        M.la3dm_map_frontier.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_uint64, C.POINTER(FrontierOut),
                                                                                                  C.POINTER(C.c_uint64), C.POINTER(RegionInfo)]
        M.la3dm_map_gain.restype = C.c_int
        M.la3dm_map_gain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p] + [C.c_uint32] * 4 + \
                                    [C.POINTER(GainOut), C.POINTER(RegionInfo)]
        M.la3dm_map_score_poses.restype = C.c_int
        M.la3dm_map_score_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p] + [C.c_uint32] * 3 + \
                                           [C.POINTER(ScoreOut), C.POINTER(RegionInfo)]
        M.la3dm_map_score_paths.restype = C.c_int
        M.la3dm_map_score_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PathsParams),
                                           C.POINTER(PathsOut), C.POINTER(RegionInfo)]
        M.la3dm_map_reach.restype = C.c_int
        M.la3dm_map_reach.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + \
                                     [C.c_void_p, C.c_uint32, C.POINTER(ReachOut), C.POINTER(ReachStats), C.POINTER(RegionInfo)]
        M.la3dm_map_travel.restype = C.c_int
        M.la3dm_map_travel.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(TravelParams), C.c_void_p,
                                       C.c_uint32, C.POINTER(TravelOut), C.POINTER(TravelStats), C.POINTER(RegionInfo)]
        M.la3dm_map_clusters.restype = C.c_int
        M.la3dm_map_clusters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ClustersParams), C.POINTER(ClustersOut),
                                         C.POINTER(C.c_uint32), C.POINTER(ClustersStats), C.POINTER(RegionInfo)]
        M.la3dm_map_pack.restype = C.c_int
        M.la3dm_map_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        M.la3dm_map_unpack.restype = C.c_int
        M.la3dm_map_unpack.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        M.la3dm_map_save.restype = C.c_int
        M.la3dm_map_save.argtypes = [C.c_void_p, C.c_char_p]
        M.la3dm_map_load.restype = C.c_int
        M.la3dm_map_load.argtypes = [C.c_void_p, C.c_char_p]
        M.la3dm_map_merge.restype = C.c_int
        M.la3dm_map_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(MergeStats)]
        M.la3dm_map_merge_file.restype = C.c_int
        M.la3dm_map_merge_file.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(MergeStats)]
        M.la3dm_map_diff.restype = C.c_int
        M.la3dm_map_diff.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(DiffParams), C.c_uint64, C.POINTER(DiffOut),
                                     C.POINTER(C.c_uint64), C.POINTER(DiffStats)]
        M.la3dm_map_diff_file.restype = C.c_int
        M.la3dm_map_diff_file.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(DiffParams), C.c_uint64, C.POINTER(DiffOut),
                                          C.POINTER(C.c_uint64), C.POINTER(DiffStats)]
        M.la3dm_map_pack_region.restype = C.c_int
        M.la3dm_map_pack_region.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        M.la3dm_map_erase_region.restype = C.c_int
        M.la3dm_map_erase_region.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EraseStats)]
        M.la3dm_map_evict.restype = C.c_int
        M.la3dm_map_evict.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(EraseStats)]
        M.la3dm_map_evict_file.restype = C.c_int
        M.la3dm_map_evict_file.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EraseStats)]
        M.la3dm_map_mirror_syncs.restype = C.c_uint64
        M.la3dm_map_mirror_syncs.argtypes = [C.c_void_p]
        M.la3dm_map_raycast.restype = C.c_uint64
        M.la3dm_map_raycast.argtypes = [C.c_void_p, f32p, f32p] + [C.c_void_p] * 7 + [C.c_uint64]
        M.la3dm_map_set_shard.restype = C.c_int
        M.la3dm_map_set_shard.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, ALLGATHER_FN, C.c_void_p]
        M.la3dm_map_set_device_resident.restype = C.c_int
        M.la3dm_map_set_device_resident.argtypes = [C.c_void_p, C.c_int]
        M.la3dm_map_is_device_resident.restype = C.c_int
        M.la3dm_map_is_device_resident.argtypes = [C.c_void_p]
        M.la3dm_map_last_error.restype = C.c_char_p
        M.la3dm_map_insert_pointcloud_device.restype = C.c_int
        M.la3dm_map_insert_pointcloud_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, C.c_float, C.c_float, C.c_float]
        M.la3dm_map_insert_pointcloud.restype = C.c_int
        M.la3dm_map_insert_pointcloud.argtypes = [C.c_void_p, f32p, C.c_uint64, f32p, C.c_float, C.c_float, C.c_float]
        M.la3dm_map_insert_training_data.restype = C.c_int
        M.la3dm_map_insert_training_data.argtypes = [C.c_void_p, f32p, C.c_uint64]
        M.la3dm_map_prepare.restype = C.c_int
        M.la3dm_map_prepare.argtypes = [C.c_void_p, f32p, C.c_uint64, f32p, C.c_float, C.c_float, C.c_float]
        M.la3dm_map_prepare_training_data.restype = C.c_int
        M.la3dm_map_prepare_training_data.argtypes = [C.c_void_p, f32p, C.c_uint64, C.c_int]
        M.la3dm_map_packed.restype = C.c_int
        M.la3dm_map_packed.argtypes = [C.c_void_p, C.POINTER(BgkScan)]
        M.la3dm_map_commit.restype = C.c_int
        M.la3dm_map_commit.argtypes = [C.c_void_p]
        M.la3dm_map_ctx.restype = C.c_void_p
        M.la3dm_map_ctx.argtypes = [C.c_void_p]
        M.la3dm_map_stats.argtypes = [C.c_void_p, C.POINTER(ScanStats)]
        M.la3dm_map_training_size.restype = C.c_uint64
        M.la3dm_map_training_size.argtypes = [C.c_void_p]
        M.la3dm_map_training_data.argtypes = [C.c_void_p, f32p, C.c_uint64]
        M.la3dm_map_block_size.restype = C.c_float
        M.la3dm_map_block_size.argtypes = [C.c_void_p]
        M.la3dm_map_resolution.restype = C.c_float
        M.la3dm_map_resolution.argtypes = [C.c_void_p]
        M.la3dm_map_block_depth.argtypes = [C.c_void_p]
        M.la3dm_map_set_resolution.argtypes = [C.c_void_p, C.c_float]
        M.la3dm_map_set_block_depth.argtypes = [C.c_void_p, C.c_int]
        M.la3dm_map_block_count.restype = C.c_uint64
        M.la3dm_map_block_count.argtypes = [C.c_void_p]
        M.la3dm_map_leaf_count.restype = C.c_uint64
        M.la3dm_map_leaf_count.argtypes = [C.c_void_p]
        M.la3dm_map_dump_leaves.restype = C.c_uint64
        M.la3dm_map_dump_leaves.argtypes = [C.c_void_p] + [C.c_void_p] * 8 + [C.c_uint64]
        M.la3dm_map_search.restype = C.c_int
        M.la3dm_map_search.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float),
                                       C.POINTER(C.c_float), C.POINTER(C.c_uint8)]
        M.la3dm_map_get_bbox.argtypes = [C.c_void_p, f32p, f32p]
        M.la3dm_map_block_to_hash_key.restype = C.c_int64
        M.la3dm_map_block_to_hash_key.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float]
        M.la3dm_map_hash_key_to_block.argtypes = [C.c_void_p, C.c_int64, f32p]
        M.la3dm_map_extended_block.argtypes = [C.c_void_p, C.c_int64, np.ctypeslib.ndpointer(np.int64)]
        M.la3dm_map_lut.restype = C.c_uint32
        M.la3dm_map_lut.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        _map = M
    return _map
