/* la3dm_map.h — C binding of the host-side BGKOctoMap (la3dm_amd/csrc/host/bgkoctomap.h).
 *
 * The C++ class is the drop-in for the reference's la3dm::BGKOctoMap
 * (include/bgkoctomap/bgkoctomap.h:26-367); this flat C view exists for language
 * bindings (the Python tests and bench use it through ctypes).  Every function
 * returns 0 on success, negative on failure (la3dm_map_last_error()).
 */
#ifndef LA3DM_MAP_H
#define LA3DM_MAP_H
#include <stdint.h>
#include "la3dm_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct la3dm_map la3dm_map;

/* mirrors ScanStats */
typedef struct la3dm_scan_stats {
    uint64_t n_hits, n_frees, n_bbox_blocks, n_train_blocks, n_test_blocks;
    uint64_t voxel_updates, train_reads, pair_evals, n_tiles;
    double t_frontend, t_partition, t_pack, t_device, t_commit, t_prune, t_total;
    double t_gather; /* sharded device-resident insert with LA3DM_TIMING=1: the all-gather-v (otherwise part of t_device) */
} la3dm_scan_stats;

/* BGKOctoMap(resolution, block_depth, sf2, ell, free_thresh, occupied_thresh, var_thresh, prior_A, prior_B) */
la3dm_map *la3dm_map_create(float resolution, int block_depth, float sf2, float ell, float free_thresh,
                            float occupied_thresh, float var_thresh, float prior_A, float prior_B, int device);
/* GPOctoMap(resolution, block_depth, sf2, ell, noise, l, min_var, max_var, max_known_var, free_thresh, occupied_thresh)
 * (src/gpoctomap/gpoctomap.cpp:23-25); every other call below works on either map kind.  For a GP map the
 * leaf arrays A/B hold the node's m_ivar/ivar. */
la3dm_map *la3dm_map_create_gp(float resolution, int block_depth, float sf2, float ell, float noise, float l,
                               float min_var, float max_var, float max_known_var, float free_thresh,
                               float occupied_thresh, int device);
/* BGKLOctoMap(resolution, block_depth, sf2, ell, free_thresh, occupied_thresh, var_thresh, prior_A, prior_B)
 * (src/bgkloctomap/bgkloctomap.cpp:31-57): block-level BGK whose free-space evidence are beam segments. */
la3dm_map *la3dm_map_create_l(float resolution, int block_depth, float sf2, float ell, float free_thresh,
                              float occupied_thresh, float var_thresh, float prior_A, float prior_B, int device);
/* BGKLOctoMap only: beam index per training sample (-1 = hit) and beams (6 floats) of the last scan; returns the number
 * of samples (the samples themselves come from la3dm_map_training_data) */
uint64_t la3dm_map_l_training(const la3dm_map *m, int32_t *ray_idx, uint64_t cap, float *rays6, uint64_t cap_rays,
                              uint64_t *n_rays);
/* BGKLVOctoMap(resolution, block_depth, sf2, ell, free_thresh, occupied_thresh, var_thresh, prior_A, prior_B,
 * original_size, min_W) (src/bgklvoctomap/bgklvoctomap.cpp:33-43).  For an LV map la3dm_map_dump_leaves reports the
 * reference's LV state codes (UNCERTAIN = 3, PRUNED = 4), node_key = (depth << 28) + index, and only blocks that hold a
 * classified or collapsed leaf (the LV map allocates every block of each scan's bounding box). */
la3dm_map *la3dm_map_create_lv(float resolution, int block_depth, float sf2, float ell, float free_thresh,
                               float occupied_thresh, float var_thresh, float prior_A, float prior_B, int original_size,
                               float min_W, int device);
/* LV only: samples (x, y, z, ray) and segments (6 floats) of the last scan; counts via NULL pointers */
uint64_t la3dm_map_lv_training(const la3dm_map *m, float *samples4, uint64_t cap_samples, float *rays6, uint64_t cap_rays,
                               uint64_t *n_rays);
/* LV only: n_hits, n_rays, n_samples, n_bbox_blocks, n_packed_blocks, n_info_blocks, voxels, voxel_updates,
 * t_frontend, t_partition, t_device, t_commit, t_total */
int la3dm_map_lv_stats(const la3dm_map *m, double *out13);
/* LV only, split form: prepare -> la3dm_bgklv_scan_* on the packed arguments -> commit */
int la3dm_map_lv_prepare(la3dm_map *m, const float *xyz, uint64_t n, const float *origin3, float ds_resolution,
                         float free_res, float max_range);
int la3dm_map_lv_packed(la3dm_map *m, la3dm_lv_scan *out);
int la3dm_map_lv_commit(la3dm_map *m);
void la3dm_map_destroy(la3dm_map *m);
const char *la3dm_map_last_error(void);

/* insert_pointcloud(cloud, origin, ds_resolution, free_res, max_range); xyz packed, 3 floats per point */
int la3dm_map_insert_pointcloud(la3dm_map *m, const float *xyz, uint64_t n, const float *origin3, float ds_resolution,
                                float free_res, float max_range);
/* the same for a cloud that already lives in HBM on the map's device (n packed xyz triples); device-resident maps only */
int la3dm_map_insert_pointcloud_device(la3dm_map *m, const float *d_xyz, uint64_t n, const float *origin3, float ds_resolution,
                                       float free_resolution, float max_range);
/* insert_training_data(GPPointCloud): x,y,z,label per point */
int la3dm_map_insert_training_data(la3dm_map *m, const float *xyzy, uint64_t n);

/* split form: prepare -> (caller runs la3dm_bgk_scan_* on the packed scan) -> commit.
 * prepare returns 1 if there is work, 0 if the training set is empty. */
int la3dm_map_prepare(la3dm_map *m, const float *xyz, uint64_t n, const float *origin3, float ds_resolution,
                      float free_res, float max_range);
int la3dm_map_prepare_training_data(la3dm_map *m, const float *xyzy, uint64_t n, int ungated);
int la3dm_map_packed(la3dm_map *m, la3dm_bgk_scan *out);
int la3dm_map_commit(la3dm_map *m);
la3dm_ctx *la3dm_map_ctx(la3dm_map *m);

/* Device-resident mode (include/la3dm_hip.h, la3dm_devmap_*): the block pool lives in HBM, insert_pointcloud runs
 * start to finish on the GPU, the host blocks are a lazily refreshed mirror.  Switch while the map is empty.
 * insert_training_data and prepare/commit are refused in this mode. */
int la3dm_map_set_device_resident(la3dm_map *m, int on);
/* block-sharded insert_pointcloud over `world` replicas of the map, one per GPU (la3dm_devmap_set_shard, la3dm_hip.h);
 * the map must be device resident; world = 1 switches it off */
int la3dm_map_set_shard(la3dm_map *m, uint32_t rank, uint32_t world, la3dm_allgatherv_fn fn, void *user);
int la3dm_map_is_device_resident(const la3dm_map *m);

int la3dm_map_stats(const la3dm_map *m, la3dm_scan_stats *out);
uint64_t la3dm_map_training_size(const la3dm_map *m);
int la3dm_map_training_data(const la3dm_map *m, float *xyzy, uint64_t cap);

float la3dm_map_block_size(const la3dm_map *m);
float la3dm_map_resolution(const la3dm_map *m);
int la3dm_map_block_depth(const la3dm_map *m);
/* BGKOctoMap::set_resolution / set_block_depth (reference src/bgkoctomap/bgkoctomap.cpp:66-80, and the same pair of the
 * GP / BGK-L / BGK-LV classes): re-derive block size and voxel LUT, rebuild the device context.  Legal on an EMPTY map
 * only — the reference applies them under existing blocks and silently corrupts the map; here that is an error (-1,
 * la3dm_map_last_error).  Options set through la3dm_set_option return to their defaults. */
int la3dm_map_set_resolution(la3dm_map *m, float resolution);
int la3dm_map_set_block_depth(la3dm_map *m, int block_depth);
uint64_t la3dm_map_block_count(const la3dm_map *m);
uint64_t la3dm_map_leaf_count(const la3dm_map *m);
/* all leaves, blocks by ascending hash key, leaves in LeafIterator order */
uint64_t la3dm_map_dump_leaves(const la3dm_map *m, int64_t *block_key, int32_t *node_key, float *loc_xyz, float *size,
                               float *A, float *B, uint8_t *state, uint8_t *classified, uint64_t cap);
/* search(x, y, z): returns 1 if the block exists */
int la3dm_map_search(const la3dm_map *m, float x, float y, float z, float *A, float *B, uint8_t *state);
/* search for n points at once (packed xyz); device-resident maps answer from the device pool without a mirror refresh */
int la3dm_map_search_many(const la3dm_map *m, const float *xyz, uint64_t n, uint8_t *exists, float *A, float *B,
                          uint8_t *state);
/* BGKOctoMap::raycast_many: the client loop over a RayCaster for n segments at once (rays6: start xyz, end xyz per ray) —
 * walk until the end, max_steps rows, or a row whose class (state of the voxel's covering leaf, LA3DM_RAY_MISSING where
 * the block does not exist) is in stop_mask; semantics and `out` in include/la3dm_hip.h (la3dm_devmap_raycast_host).
 * Device-resident maps answer from the device pool without a mirror refresh, host-mode maps run the loop on the host;
 * the results are bit-identical. */
int la3dm_map_raycast_many(const la3dm_map *m, const float *rays6, uint64_t n, uint32_t stop_mask, uint32_t max_steps,
                           const la3dm_raycast_out *out);
/* BGKOctoMap::box / columns: the voxels of an axis-aligned box as dense arrays, and the same box reduced along z per
 * (x, y) column.  lo3: a world point inside voxel (0, 0, 0) of the region; dims3 = (nx, ny, nz), each >= 1; voxel (i, j, k)
 * is i, j, k cells of the finest-layer lattice further on, across block borders.  box: index (i * ny + j) * nz + k, the
 * state of the voxel's covering leaf (LA3DM_RAY_MISSING where the block does not exist), its layer and node values.
 * columns: index i * ny + j, voxels per class FREE, OCCUPIED, UNKNOWN, MISSING over k and the lowest / highest OCCUPIED k
 * (-1: none).  info (may be NULL): block key and cell of voxel (0, 0, 0) and its centre; the other centres are
 * origin + (i, j, k) * resolution.  Contract, limits and the output structs: include/la3dm_hip.h
 * (la3dm_devmap_box_host).  Device-resident maps answer from the device pool without a mirror refresh, host-mode maps loop
 * over the host blocks; the results are bit-identical. */
int la3dm_map_box(const la3dm_map *m, const float *lo3, const uint32_t *dims3, const la3dm_box_out *out, la3dm_region_info *info);
int la3dm_map_columns(const la3dm_map *m, const float *lo3, const uint32_t *dims3, const la3dm_columns_out *out,
                      la3dm_region_info *info);
/* BGKOctoMap::distance_field: the exact Euclidean distance transform of box's region.  A voxel is an obstacle when
 * obstacle_mask & (1u << cls) is set (cls as box reports it; the bits of raycast_many's stop_mask); d2 = the squared
 * distance, an integer in voxel units, to the nearest obstacle INSIDE THE REGION, LA3DM_DF_FAR beyond radius^2 (pad the
 * region by `radius` where that matters); dist = sqrtf(d2) * resolution, +inf for FAR.  At least one of out->d2, out->dist.
 * The distance inside obstacles is the call with the complementary mask.  Contract, limits and refusals:
 * include/la3dm_hip.h (la3dm_devmap_distance_host).  Device-resident maps run the transform on the device pool without a
 * mirror refresh, host-mode maps on the CPU; the results are bit-identical. */
int la3dm_map_distance_field(const la3dm_map *m, const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask, uint32_t radius,
                             const la3dm_distance_out *out, la3dm_region_info *info);
/* BGKOctoMap::frontier: the voxels of box's region whose class is in open_mask and that have at least min_neighbours
 * neighbours (connectivity 6, 18 or 26) whose class is in unknown_mask — cls as box reports it, the bits of raycast_many's
 * stop_mask — with the neighbours one step outside the region read from the map.  *n_found = their number, whatever cap is;
 * out->index = the flat indices (i * ny + j) * nz + k of the first min(*n_found, cap) in ascending order, out->nbrs = their
 * scores, out->score (dense, optional) = the score of every voxel.  cap = 0 with out NULL (or only out->score set) counts:
 * call once for *n_found, then with buffers of that size.  Contract, limits and refusals: include/la3dm_hip.h
 * (la3dm_devmap_frontier_host).  Device-resident maps run the query on the device pool without a mirror refresh, host-mode
 * maps on the CPU; the results are identical. */
int la3dm_map_frontier(const la3dm_map *m, const float *lo3, const uint32_t *dims3, uint32_t open_mask, uint32_t unknown_mask,
                       uint32_t connectivity, uint32_t min_neighbours, uint64_t cap, const la3dm_frontier_out *out,
                       uint64_t *n_found, la3dm_region_info *info);
/* BGKOctoMap::gain: per viewpoint origins3[v] the number of DISTINCT voxels of box's region that the segments origins3[v] ->
 * origins3[v] + offsets3[d], d < m, walk over — each exactly as raycast_many(stop_mask, max_steps) walks it — and whose class
 * is in count_mask: the expected information gain of a next-best-view planner with count_mask = UNKNOWN | MISSING.
 * out->gain (mandatory) [n]; out->started / out->hits [n] = the rays that produced a row / ended on a stop row; out->seen
 * [n * ceil(nx ny nz / 32)] = the sets, bit f = (i * ny + j) * nz + k.  Contract, limits and refusals: include/la3dm_hip.h
 * (la3dm_devmap_gain_host).  Device-resident maps run the query on the device pool without a mirror refresh, host-mode
 * maps on the CPU; the results are identical. */
int la3dm_map_gain(const la3dm_map *m, const float *lo3, const uint32_t *dims3, const float *origins3, uint32_t n,
                   const float *offsets3, uint32_t m_dirs, uint32_t count_mask, uint32_t stop_mask, uint32_t max_steps,
                   const la3dm_gain_out *out, la3dm_region_info *info);
/* BGKOctoMap::score_poses: likelihood-field scoring of one scan under many poses.  Every point of points3 (sensor frame) is
 * moved by every pose of poses12 (n_poses x 12 floats, row-major 3 x 4 [R | t]), its voxel resolved as search resolves it,
 * and d2 = distance_field(lo, dims, obstacle_mask, radius) gathered there.  out->sum_d2 (mandatory) [n_poses] = the sum of
 * the finite d2 per pose; out->counts [5 n_poses] = the pairs of class HIT, NEAR, FAR, OUTSIDE, INVALID.  Contract, limits
 * and refusals: include/la3dm_hip.h (la3dm_devmap_score_poses_host).  Device-resident maps run the query on the device
 * pool without a mirror refresh, host-mode maps on the CPU; the results are identical. */
int la3dm_map_score_poses(const la3dm_map *m, const float *lo3, const uint32_t *dims3, const float *points3, uint32_t n_points,
                          const float *poses12, uint32_t n_poses, uint32_t obstacle_mask, uint32_t radius, const la3dm_score_out *out,
                          la3dm_region_info *info);
/* BGKOctoMap::nearest: which obstacle is the nearest.  Per voxel of box's region out->index = the flat index of the nearest
 * voxel of the region whose class is in obstacle_mask (the smallest flat index among equals; LA3DM_NEAREST_NONE beyond
 * `radius` voxels) and out->d2 = distance_field's d2; either may be NULL, not both.  BGKOctoMap::nearest_points: the same
 * per point of points3, moved by the optional pose12 (row-major 3 x 4 [R | t]; NULL: the points as they are): out->cls =
 * score_poses' class of the point, out->voxel = its voxel, out->index = that voxel's nearest obstacle, out->d2 = the
 * squared distance — the correspondences of an ICP step.  Contract, limits and refusals: include/la3dm_hip.h
 * (la3dm_devmap_nearest_host).  Device-resident maps run the queries on the device pool without a mirror refresh,
 * host-mode maps on the CPU; the results are identical. */
int la3dm_map_nearest(const la3dm_map *m, const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask, uint32_t radius,
                      const la3dm_nearest_out *out, la3dm_region_info *info);
int la3dm_map_nearest_points(const la3dm_map *m, const float *lo3, const uint32_t *dims3, const float *points3, uint32_t n_points,
                             const float *pose12, uint32_t obstacle_mask, uint32_t radius, const la3dm_nearest_points_out *out,
                             la3dm_region_info *info);
/* BGKOctoMap::footing: where a ground robot can stand.  The voxels of box's region with a class of params->support_mask
 * directly below, params->headroom voxels of params->clear_mask classes from the voxel upwards, and a footprint of
 * params->radius voxels round them that is not blocked above params->step voxels and has ground within params->step
 * voxels of height under at least params->min_support of its cells.  *n_found = their number; out->index = the flat
 * indices of the first min(*n_found, cap) in ascending order; out->levels / lowest / highest (dense, per column, optional)
 * = the foot voxels of the column and their smallest / largest k (-1: none); stats (may be NULL) = the voxels that pass
 * each condition and the cells of the footprint.  cap = 0 only counts.  Contract, limits and refusals: include/la3dm_hip.h
 * (la3dm_devmap_footing_host).  Device-resident maps run the query on the device pool without a mirror refresh,
 * host-mode maps on the CPU; the results are identical. */
int la3dm_map_footing(const la3dm_map *m, const float *lo3, const uint32_t *dims3, const la3dm_footing_params *params, uint64_t cap,
                      const la3dm_footing_out *out, uint64_t *n_found, la3dm_footing_stats *stats, la3dm_region_info *info);
/* BGKOctoMap::surface: the exposed faces and integer normals of box's region.  A voxel whose class is in
 * params->solid_mask has face d (0: -x, 1: +x, 2: -y, 3: +y, 4: -z, 5: +z) when its neighbour in that direction has a class
 * in params->open_mask; a surface voxel has at least one.  *n_found = their number; out->index / faces / normal = the flat
 * indices of the first min(*n_found, cap) in ascending order, their face masks and their normals — the sum of the face
 * vectors of every voxel within params->smooth voxels (Chebyshev), three int16 pointing into open space, possibly zero —;
 * out->dense_faces (optional) = the face mask of every voxel of the region; stats (may be NULL) = the solid voxels, the
 * surface voxels and the faces per direction.  cap = 0 only counts.  Contract, limits and refusals: include/la3dm_hip.h
 * (la3dm_devmap_surface_host).  Device-resident maps run the query on the device pool without a mirror refresh, host-mode
 * maps on the CPU; the results are identical. */
int la3dm_map_surface(const la3dm_map *m, const float *lo3, const uint32_t *dims3, const la3dm_surface_params *params, uint64_t cap,
                      const la3dm_surface_out *out, uint64_t *n_found, la3dm_surface_stats *stats, la3dm_region_info *info);
/* BGKOctoMap::score_paths: cost and clearance of many candidate trajectories.  Every path of ways3 (n_paths x n_way x 3
 * floats, world frame; a shorter path repeats its last waypoint) is walked voxel by voxel through box's region against d2 =
 * distance_field(lo, dims, obstacle_mask, max(1, clearance, soft_radius)); out->cost (mandatory) [n_paths] = travel's cost
 * of the walk up to its stop; out->steps, stop, min_d2, ways, flags (LA3DM_PATH_*) [n_paths] are optional.  Contract, limits
 * and refusals: include/la3dm_hip.h (la3dm_devmap_score_paths_host).  Device-resident maps run the query on the device
 * pool without a mirror refresh, host-mode maps on the CPU; the results are identical. */
int la3dm_map_score_paths(const la3dm_map *m, const float *lo3, const uint32_t *dims3, const float *ways3, uint32_t n_paths,
                          uint32_t n_way, const la3dm_paths_params *params, const la3dm_paths_out *out, la3dm_region_info *info);
/* BGKOctoMap::reach: steps[v] = the least number of moves (connectivity 6, 18 or 26) from any of the seed voxels to v
 * through the passable voxels of box's region — class in pass_mask and, with clearance > 0, farther than clearance voxels
 * from every voxel of the region whose class is in obstacle_mask (distance_field's d2 == LA3DM_DF_FAR) — LA3DM_REACH_NONE
 * where no such walk of at most max_steps moves exists.  seeds and targets are flat indices (i * ny + j) * nz + k, e.g.
 * frontier's index list; out->target_steps[t] = steps[targets[t]].  stats (optional): seeded voxels, reached voxels, the
 * largest finite step.  Contract, limits and refusals: include/la3dm_hip.h (la3dm_devmap_reach_host).  Device-resident
 * maps run the wave on the device pool without a mirror refresh, host-mode maps a queue BFS on the CPU; the results are
 * identical. */
int la3dm_map_reach(const la3dm_map *m, const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds,
                    uint32_t pass_mask, uint32_t obstacle_mask, uint32_t clearance, uint32_t connectivity, uint32_t max_steps,
                    const uint32_t *targets, uint32_t n_targets, const la3dm_reach_out *out, la3dm_reach_stats *stats,
                    la3dm_region_info *info);
/* BGKOctoMap::travel: cost[v] = the least path cost from any of the seed voxels to v through the passable voxels of box's
 * region, with a cost per move by its number of non-zero components (params->move_cost), a penalty that falls from
 * params->penalty next to an obstacle to 0 at params->soft_radius, and reach's clearance; LA3DM_TRAVEL_NONE where no walk
 * of at most params->max_cost exists.  out->parent[v] = the code (di + 1) * 9 + (dj + 1) * 3 + (dk + 1) of the offset to the
 * voxel a least-cost walk came from, 13 at a seeded voxel, 255 where unreached; out->target_cost[t] = cost[targets[t]].
 * Contract, limits and refusals: include/la3dm_hip.h (la3dm_devmap_travel_host).  Device-resident maps relax bricks of
 * the region on the device pool without a mirror refresh, host-mode maps run Dijkstra on the CPU; the results are
 * identical. */
int la3dm_map_travel(const la3dm_map *m, const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds,
                     const la3dm_travel_params *params, const uint32_t *targets, uint32_t n_targets, const la3dm_travel_out *out,
                     la3dm_travel_stats *stats, la3dm_region_info *info);
/* BGKOctoMap::drive: cost[v] = the least cost of a ground route from any of the seed voxels to v over the member voxels of
 * box's region — those of the list params->members, or with params->footing set the voxels footing would list — by moves
 * to one of the 4 or 8 horizontal neighbours that climb or drop at most params->step voxels; LA3DM_DRIVE_NONE for a
 * non-member and where no walk of at most params->max_cost exists.  A seed or target stands for the highest member at
 * most params->snap voxels below it.  out->parent[v] = the code ((o_i + 1) * 3 + (o_j + 1)) * 9 + (o_k + 4) of the offset
 * to the member a least-cost walk came from, 40 at a seeded member, 255 where unreached; out->target_cost[t] and
 * out->target_index[t] = the cost at the member of targets[t] and that member.  Contract, limits and refusals:
 * include/la3dm_hip.h (la3dm_devmap_drive_host).  Device-resident maps relax bricks of the region on the device without a
 * mirror refresh, host-mode maps run their own footing and Dijkstra on the CPU; the results are identical. */
int la3dm_map_drive(const la3dm_map *m, const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds,
                    const la3dm_drive_params *params, const uint32_t *targets, uint32_t n_targets, const la3dm_drive_out *out,
                    la3dm_drive_stats *stats, la3dm_region_info *info);
/* BGKOctoMap::clusters: the connected groups of the member voxels of box's region — every voxel with a class in
 * params->member_mask, or those of the list params->members — under params->connectivity, confined to tiles of
 * params->tile voxels (0: untiled) and kept from params->min_size members up; numbered in ascending order of their
 * smallest flat index.  out->label = the number per voxel, out->of_member = per list entry (LA3DM_CLUSTERS_NONE elsewhere);
 * for the first params->cap clusters first, size, the bounding box lo / hi, the coordinate sums and rep, the member
 * nearest the rounded centroid.  *n_found = the number of kept clusters.  Contract, limits and refusals:
 * include/la3dm_hip.h (la3dm_devmap_clusters_host).  Device-resident maps relax bricks of the region on the device pool
 * without a mirror refresh, host-mode maps flood-fill on the CPU; the results are identical. */
int la3dm_map_clusters(const la3dm_map *m, const float *lo3, const uint32_t *dims3, const la3dm_clusters_params *params,
                       const la3dm_clusters_out *out, uint32_t *n_found, la3dm_clusters_stats *stats, la3dm_region_info *info);
/* BGKOctoMap::pack / unpack / save / load: the map as the compact stream of its covering leaves (layout, validation and
 * refusals: include/la3dm_hip.h, la3dm_devmap_pack_host).  pack: *size = the stream's bytes; buf NULL only sizes; cap < *size
 * is an error with *size set.  A device-resident map compacts its pool on the GPU (no mirror refresh), a host-mode map
 * writes the same stream from its blocks in ascending key order.  unpack: into an EMPTY map of the same class, block_depth,
 * resolution and default node; the stream is validated first and a refused one leaves the map as it was (-1,
 * la3dm_map_last_error).  save writes the stream to path + ".tmp" and renames it to path; load reads path and unpacks it.
 * Not in the stream: the last scan's training data, the statistics, the options and the shard configuration. */
int la3dm_map_pack(const la3dm_map *m, void *buf, uint64_t cap, uint64_t *size);
int la3dm_map_unpack(la3dm_map *m, const void *buf, uint64_t size);
int la3dm_map_save(const la3dm_map *m, const char *path);
int la3dm_map_load(la3dm_map *m, const char *path);
/* BGKOctoMap::merge / BGKLOctoMap::merge: a stream fused into a map that may hold blocks (the rule per finest cell — kept,
 * copied, fused —, the prune, the canonical form and the refusals: include/la3dm_hip.h, la3dm_devmap_merge_host).  A
 * device-resident map fuses on the GPU pool (its mirror is marked stale), a host-mode map runs csrc/host/merge_block.h over
 * its blocks; both leave the same bytes.  stats may be NULL.  merge_file reads path and merges it.  A refused stream leaves
 * the map as it was (-1, la3dm_map_last_error). */
int la3dm_map_merge(la3dm_map *m, const void *buf, uint64_t size, la3dm_merge_stats *stats);
int la3dm_map_merge_file(la3dm_map *m, const char *path, la3dm_merge_stats *stats);
/* BGKOctoMap::diff, all four classes: the finest cells whose class — or, with params->value_mask, whose A or B — differs
 * between the map (now) and a stream (then), as a list and as 5 x 5 pair counts (the compared blocks, the classes, the
 * selection, the outputs and the refusals: include/la3dm_hip.h, la3dm_devmap_diff_host).  The map is not changed.  A
 * device-resident map compares on the GPU pool (no mirror refresh, the mirror not marked stale), a host-mode map runs
 * csrc/host/diff_block.h over its blocks (map-only blocks in ascending key order); both give the same list and counts.
 * cap = 0 with out NULL only counts; stats may be NULL.  diff_file reads path and compares with it.  A refusal (-1,
 * la3dm_map_last_error) writes nothing. */
int la3dm_map_diff(const la3dm_map *m, const void *buf, uint64_t size, const la3dm_diff_params *params, uint64_t cap,
                   const la3dm_diff_out *out, uint64_t *n_found, la3dm_diff_stats *stats);
int la3dm_map_diff_file(const la3dm_map *m, const char *path, const la3dm_diff_params *params, uint64_t cap, const la3dm_diff_out *out,
                        uint64_t *n_found, la3dm_diff_stats *stats);
/* BGKOctoMap::pack_region / erase_region / evict / evict_file, all four classes: the map as a rolling window (the region,
 * the stream, the pool after an erase and the refusals: include/la3dm_hip.h, la3dm_devmap_pack_region_host).  The region is
 * given by two world points lo3, hi3: the box of blocks from the block that holds lo3 to the block that holds hi3
 * (block_to_hash_key of each point, on the host: klo from lo3, khi from hi3; klo > khi on an axis is refused); inside = 1 selects the blocks
 * in the box, 0 every other block.  pack_region follows la3dm_map_pack's buffer convention (buf = NULL sizes, cap < *size
 * is -1 with *size set) and does not change the map; a device-resident map writes the selected blocks in pool slot order, a
 * host-mode map in ascending key order.  erase_region removes the selected blocks (a device-resident map compacts its pool
 * on the GPU and drops the blocks from its mirror, which is marked stale; a host-mode map erases them from its container);
 * stats may be NULL.  evict = pack_region, then erase_region of the same region, composed on the host: the stream is in buf
 * — or, for evict_file, written to path + ".tmp" and renamed to path — BEFORE the first block is removed; if that step
 * fails (-1, la3dm_map_last_error) the map is as it was.  evict with buf = NULL only sizes and removes nothing.  What was
 * evicted can be merged back (la3dm_map_merge_file). */
int la3dm_map_pack_region(const la3dm_map *m, const float *lo3, const float *hi3, int inside, void *buf, uint64_t cap, uint64_t *size);
int la3dm_map_erase_region(la3dm_map *m, const float *lo3, const float *hi3, int inside, la3dm_erase_stats *stats);
int la3dm_map_evict(la3dm_map *m, const float *lo3, const float *hi3, int inside, void *buf, uint64_t cap, uint64_t *size,
                    la3dm_erase_stats *stats);
int la3dm_map_evict_file(la3dm_map *m, const char *path, const float *lo3, const float *hi3, int inside, la3dm_erase_stats *stats);
/* how often the host mirror of a device-resident map was refreshed (a download of every node of every block) */
uint64_t la3dm_map_mirror_syncs(const la3dm_map *m);
int la3dm_map_get_bbox(const la3dm_map *m, float *lim_min3, float *lim_max3);
/* Block(center).get_index(p) / get_node / get_point (reference bgkblock.cpp:131-150) */
void la3dm_map_block_grid(const la3dm_map *m, const float *center3, const float *p3, int32_t *idx3, int32_t *node_key,
                          float *point3);
/* BGKOctoMap::RayCaster(map, start, end) driven to its end (reference bgkoctomap.h:91-214): one row per next() call —
 * voxel centre, block key, node key, valid (block exists), a copy of the node.  Returns the number of steps
 * (rows beyond `cap` are counted but not written). */
uint64_t la3dm_map_raycast(const la3dm_map *m, const float *start3, const float *end3, float *p_xyz, int64_t *block_key,
                           int32_t *node_key, uint8_t *valid, float *A, float *B, uint8_t *state, uint64_t cap);

/* Cube lists of the map: the publish loop of the static node (reference bgkoctomap_static_node.cpp:101-136) with
 * MarkerArrayPub::insert_point3d / heightMapColor (markerarray_pub.h:21-147) minus ROS.  state 1 = OCCUPIED leaves
 * coloured by height between min_z and max_z (min_z == max_z: the map's bbox), 0 = FREE leaves coloured by
 * probability; original_size 0 expands collapsed leaves into base-resolution cells (get_pruned_locs).  cells / rgba:
 * 4 floats per cell {x, y, z, size} / {r, g, b, a}; level = (int) log2(size / resolution).  Device-resident maps are
 * scanned on the GPU.  Call with NULL buffers for *count, then with buffers of that capacity. */
int la3dm_map_export_cells(const la3dm_map *m, int state, int original_size, float min_z, float max_z, float *cells,
                           float *rgba, int32_t *level, uint64_t cap, uint64_t *count);

/* host bookkeeping primitives (known-answer tests) */
int64_t la3dm_map_block_to_hash_key(const la3dm_map *m, float x, float y, float z);
void la3dm_map_hash_key_to_block(const la3dm_map *m, int64_t key, float *out3);
void la3dm_map_extended_block(const la3dm_map *m, int64_t key, int64_t *out7);
uint32_t la3dm_map_lut(const la3dm_map *m, float *xyz, uint32_t cap_entries);

#ifdef __cplusplus
}
#endif
#endif
