// region_contract.h — what a valid region query is (include/la3dm_hip.h "Region"), once for the device library
// (devmap.hip) and the host map (bgkoctomap.cpp): the limits of each query, their order, their texts and the anchor
// arithmetic.  Host code, but for the inlines marked LA3DM_HD, which the device kernels compile as well (score_poses:
// csrc/devmap_score.h; score_paths: csrc/devmap_paths.h; nearest_points: csrc/devmap_nearest.h).  A check answers with the text of the refusal, without the caller's prefix, or with an empty
// string; how a refusal is reported (an error code and a stored text, an exception) is the caller's business.
#ifndef LA3DM_REGION_CONTRACT_H
#define LA3DM_REGION_CONTRACT_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/la3dm_hip.h"
#include "drive_cells.h"
#include "footing_cells.h"
#include "surface_cells.h"

#if defined(__HIPCC__)
#define LA3DM_HD __host__ __device__
#else
#define LA3DM_HD
#endif

namespace la3dm_region {

// The voxels a query reads outside its region, per axis: limit and block-field range are taken on the padded box.
struct Pad {
    uint32_t lo[3], hi[3];    // voxels below voxel (0, 0, 0) and above voxel (nx - 1, ny - 1, nz - 1)
    const char *range_text;   // refusal when the padded box leaves the block-field range
};
constexpr Pad kPadNone = {{0, 0, 0}, {0, 0, 0}, ""};
constexpr Pad kPadOne = {{1, 1, 1}, {1, 1, 1}, "dims: the block fields of the region padded by one voxel leave [0, 2^20)"};

struct Query {
    uint64_t max_cells;       // limit on the number of voxels (columns: of columns)
    const char *limit_text;
    bool columns;             // the limit counts columns, and nz has LA3DM_COLUMNS_MAX_NZ as a limit of its own
    Pad pad;                  // what the query reads past the region's faces
    const char *mandatory;    // refusal when the mandatory output is missing ("->" stands for the caller's member access)
    uint32_t brick = 0;       // > 0: the limit is taken on the region with every axis rounded up to a multiple of `brick`
};

constexpr Query kBox = {LA3DM_BOX_MAX_CELLS, "dims: more than LA3DM_BOX_MAX_CELLS (2^30) voxels", false, kPadNone, "out->cls must not be NULL"};
constexpr Query kColumns = {1ull << 30, "dims: more than 2^30 columns", true, kPadNone, "out->counts must not be NULL"};
constexpr Query kDistance = {LA3DM_DF_MAX_CELLS, "dims: more than LA3DM_DF_MAX_CELLS (2^28) voxels", false, kPadNone, "out: d2 or dist must not be NULL"};
constexpr Query kFrontier = {LA3DM_FR_MAX_CELLS, "dims: more than LA3DM_FR_MAX_CELLS (2^28) voxels in the padded region", false, kPadOne, ""};
constexpr Query kGain = {LA3DM_GAIN_MAX_CELLS, "dims: more than LA3DM_GAIN_MAX_CELLS (2^28) voxels", false, kPadNone, ""};
constexpr Query kReach = {LA3DM_REACH_MAX_CELLS, "dims: more than LA3DM_REACH_MAX_CELLS (2^28) voxels in the padded region", false, kPadOne, ""};
constexpr Query kTravel = {LA3DM_TRAVEL_MAX_CELLS, "dims: more than LA3DM_TRAVEL_MAX_CELLS (2^28) voxels in the region rounded up to whole bricks", false, kPadNone, "",
                           LA3DM_TRAVEL_BRICK};
// clusters: box's own limit here; the axis and brick limits follow the region's checks (clusters_region_check)
constexpr Query kClusters = {LA3DM_BOX_MAX_CELLS, "dims: more than LA3DM_BOX_MAX_CELLS (2^30) voxels", false, kPadNone, ""};
constexpr Query kScore = {LA3DM_SCORE_MAX_CELLS, "dims: more than LA3DM_SCORE_MAX_CELLS (2^28) voxels", false, kPadNone, ""};

struct Anchor {
    uint32_t g0[3];      // global voxel index of voxel (0, 0, 0): block field * lim + cell
    int32_t cell[3];     // cell of lo in its block
    float center[3];     // centre of that block
    int64_t block_key;
    uint64_t total;      // voxels of the region (columns: columns)
};

// One axis of the voxel that `search` and the RayCaster resolve for the coordinate w: the block field b
// (block_to_hash_key: the one double operation), the centre of that block (hash_key_to_block) and the cell inside it
// (Block::get_index: truncation, clamped), lim = 2^(block_depth - 1) cells per axis.  The global index is b * lim + cell.
// The caller has tested |w / resolution| < 2^30 (axis_in_range) before: no conversion below leaves its integer type.
struct AxisVoxel {
    long long b;
    float center;
    int cell;
};
LA3DM_HD inline bool axis_in_range(float w, float resolution) { return fabsf(w / resolution) < 1073741824.0f; }   // false for NaN and inf
LA3DM_HD inline AxisVoxel axis_voxel(float w, float resolution, float block_size, int lim) {
    AxisVoxel v;
    v.b = (long long)((double)w / (double)block_size + 524288.5);
    v.center = (float)(v.b - 524288) * block_size;
    const int t = (int)((w - v.center) / resolution + (float)(lim / 2));
    v.cell = t < 0 ? 0 : (t > lim - 1 ? lim - 1 : t);
    return v;
}

// Every check of a region in the contract's order — lo, dims, the limits and the block-field range before any buffer is
// looked at — and the anchor, the only floating-point work of a query.  `member` is "->" or ".": how the caller's texts
// name a member of out.
inline std::string resolve(const Query &q, const float *lo, const uint32_t *dims, float resolution, float block_size,
                           unsigned block_depth, bool has_out, bool has_mandatory, const char *member, Anchor &a) {
    if (!lo) return "lo is NULL";
    if (!dims) return "dims is NULL";
    for (int k = 0; k < 3; ++k)   // refused before any (int) conversion; false for NaN and inf
        if (!(std::fabs(lo[k] / resolution) < 1073741824.0f)) return "lo must be finite with |lo / resolution| < 2^30";
    for (int k = 0; k < 3; ++k)
        if (dims[k] == 0) return "dims must be >= 1 on every axis";
    const uint64_t ncol = (uint64_t)dims[0] * dims[1];
    uint64_t e[3];   // the extents the limit counts: padded, rounded up to whole bricks, or as they are
    for (int k = 0; k < 3; ++k)
        e[k] = q.brick ? ((uint64_t)dims[k] + q.brick - 1) / q.brick * q.brick : (uint64_t)dims[k] + q.pad.lo[k] + q.pad.hi[k];
    const uint64_t pcol = e[0] * e[1];
    if (q.columns) {
        if (ncol > q.max_cells) return q.limit_text;
        if (dims[2] > LA3DM_COLUMNS_MAX_NZ) return "dims: nz exceeds LA3DM_COLUMNS_MAX_NZ (2^16)";
    } else if (std::max(dims[0], std::max(dims[1], dims[2])) > q.max_cells || pcol > q.max_cells || pcol * e[2] > q.max_cells) {
        return q.limit_text;   // (an axis is tested first: the products of three such axes need not fit 64 bits)
    }
    a.total = q.columns ? ncol : ncol * dims[2];
    const long long lim = 1ll << (block_depth - 1), top = 1ll << 20;
    AxisVoxel v[3];
    for (int k = 0; k < 3; ++k) {   // (a key only holds fields that fit it: test them before one is built)
        v[k] = axis_voxel(lo[k], resolution, block_size, (int)lim);
        if (v[k].b < 0 || v[k].b >= top) return "lo: the block field leaves [0, 2^20)";
    }
    a.block_key = 0;
    for (int k = 0; k < 3; ++k) {
        a.center[k] = v[k].center;
        a.cell[k] = v[k].cell;
        const long long first = v[k].b * lim + a.cell[k], last = first + (long long)dims[k] - 1;
        if (last / lim >= top) return "dims: the region's block fields leave [0, 2^20)";
        if (first < (long long)q.pad.lo[k] || (last + (long long)q.pad.hi[k]) / lim >= top) return q.pad.range_text;
        a.g0[k] = (uint32_t)first;
        a.block_key = (a.block_key << 20) | v[k].b;
    }
    if (!has_out) return "out is NULL";
    if (!has_mandatory) {
        std::string text(q.mandatory);
        const size_t at = text.find("->");
        return at == std::string::npos ? text : text.replace(at, 2, member);
    }
    return "";
}

// the checks of distance_field's own arguments, before the region's
inline std::string distance_check(uint32_t obstacle_mask, uint32_t radius) {
    if (obstacle_mask == 0 || (obstacle_mask & ~0x1Fu)) return "obstacle_mask must hold at least one of the bits 0x1F and no other";
    if (radius == 0 || radius > LA3DM_DF_MAX_RADIUS) return "radius must lie in [1, LA3DM_DF_MAX_RADIUS (1024)]";
    return "";
}

// the checks of frontier's own arguments, before the region's
inline std::string frontier_check(uint32_t open_mask, uint32_t unknown_mask, uint32_t connectivity, uint32_t min_neighbours) {
    if (open_mask == 0 || (open_mask & ~0x1Fu)) return "open_mask must hold at least one of the bits 0x1F and no other";
    if (unknown_mask == 0 || (unknown_mask & ~0x1Fu)) return "unknown_mask must hold at least one of the bits 0x1F and no other";
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) return "connectivity must be 6, 18 or 26";
    if (min_neighbours == 0 || min_neighbours > connectivity) return "min_neighbours must lie in [1, connectivity]";
    return "";
}

// The neighbourhood of a connectivity (6, 18 or 26): the moves (di, dj, dk) in {-1, 0, 1}^3 with 1 to move_reach non-zero
// components — faces, then edges, then corners.
LA3DM_HD constexpr inline int move_reach(uint32_t connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3; }

// the checks of gain's own arguments, before the region's
inline std::string gain_check(uint32_t count_mask, uint32_t stop_mask, uint32_t max_steps, uint32_t n, uint32_t m) {
    if (count_mask == 0 || (count_mask & ~0x1Fu)) return "count_mask must hold at least one of the bits 0x1F and no other";
    if (stop_mask & ~0x1Fu) return "stop_mask must hold no bit above 0x1F";
    if (max_steps == 0 || max_steps > LA3DM_RAY_MAX_STEPS) return "max_steps must lie in [1, LA3DM_RAY_MAX_STEPS (2^20)]";
    if (m == 0) return "m must be >= 1";
    if ((uint64_t)n * m > LA3DM_GAIN_MAX_RAYS) return "n * m: more than LA3DM_GAIN_MAX_RAYS (2^28) rays";
    return "";
}

// ---- score_poses (contract: include/la3dm_hip.h, la3dm_devmap_score_poses_host) ----
// the checks of score_poses' own arguments, before the region's
inline std::string score_check(uint32_t obstacle_mask, uint32_t radius, uint32_t n_points, uint32_t n_poses) {
    if (obstacle_mask == 0 || (obstacle_mask & ~0x1Fu)) return "obstacle_mask must hold at least one of the bits 0x1F and no other";
    if (radius == 0 || radius > LA3DM_SCORE_MAX_RADIUS) return "radius must lie in [1, LA3DM_SCORE_MAX_RADIUS (255)]";
    if (n_points > LA3DM_SCORE_MAX_POINTS) return "n_points: more than LA3DM_SCORE_MAX_POINTS (2^20) points";
    if (n_poses > LA3DM_SCORE_MAX_POSES) return "n_poses: more than LA3DM_SCORE_MAX_POSES (2^20) poses";
    if ((uint64_t)n_points * n_poses > LA3DM_SCORE_MAX_PAIRS) return "n_points * n_poses: more than LA3DM_SCORE_MAX_PAIRS (2^32) pairs";
    return "";
}

// the checks that follow the region's: the buffers (`member` as in resolve)
inline std::string score_buffers(uint32_t n_points, uint32_t n_poses, bool has_points, bool has_poses, bool has_out, bool has_sum,
                                 const char *member) {
    if (n_poses == 0) return "";
    if (!has_poses) return "poses12 is NULL";
    if (!has_out) return "out is NULL";
    if (!has_sum) return std::string("out") + member + "sum_d2 must not be NULL";
    if (n_points > 0 && !has_points) return "points3 is NULL";
    return "";
}

// One coordinate of a point under a pose, row = the axis' four entries of [R | t]: three fp32 products and three fp32
// sums, each rounded on its own, in this order (both builds compile with -ffp-contract=off).
LA3DM_HD inline float pose_axis(const float *row, float x, float y, float z) { return ((row[0] * x + row[1] * y) + row[2] * z) + row[3]; }

// The class of a (pose, point) pair up to the cost volume: LA3DM_SCORE_INVALID, LA3DM_SCORE_OUTSIDE, or LA3DM_SCORE_HIT
// for a pair whose voxel lies in the region — f is then its flat index, and d2[f] decides between HIT, NEAR and FAR
// (score_class).  score_voxel is the transform followed by world_voxel, which takes the coordinate w in the map frame
// (nearest_points without a pose starts there).
LA3DM_HD inline uint32_t world_voxel(const float *w, float resolution, float block_size, int lim, const uint32_t *g0,
                                     const uint32_t *dims, uint32_t &f) {
    for (int c = 0; c < 3; ++c)
        if (!axis_in_range(w[c], resolution)) return LA3DM_SCORE_INVALID;
    uint32_t at[3];
    for (int c = 0; c < 3; ++c) {
        const AxisVoxel v = axis_voxel(w[c], resolution, block_size, lim);
        if (v.b < 0 || v.b >= (1ll << 20)) return LA3DM_SCORE_OUTSIDE;
        const long long d = v.b * lim + v.cell - (long long)g0[c];
        if (d < 0 || d >= (long long)dims[c]) return LA3DM_SCORE_OUTSIDE;
        at[c] = (uint32_t)d;
    }
    f = (at[0] * dims[1] + at[1]) * dims[2] + at[2];
    return LA3DM_SCORE_HIT;
}
LA3DM_HD inline uint32_t score_voxel(const float *pose12, float x, float y, float z, float resolution, float block_size, int lim,
                                     const uint32_t *g0, const uint32_t *dims, uint32_t &f) {
    float w[3];
    for (int c = 0; c < 3; ++c) w[c] = pose_axis(pose12 + 4 * c, x, y, z);
    return world_voxel(w, resolution, block_size, lim, g0, dims, f);
}
LA3DM_HD inline uint32_t score_class(uint32_t d2) { return d2 == 0 ? LA3DM_SCORE_HIT : (d2 != LA3DM_DF_FAR ? LA3DM_SCORE_NEAR : LA3DM_SCORE_FAR); }

// ---- nearest and nearest_points (contract: include/la3dm_hip.h, la3dm_devmap_nearest_host) ----
// nearest's limit, and its buffers as the region's last check; nearest_points' buffers follow the region's (nearest_buffers)
constexpr Query kNearest = {LA3DM_DF_MAX_CELLS, "dims: more than LA3DM_DF_MAX_CELLS (2^28) voxels", false, kPadNone, "out: index or d2 must not be NULL"};
constexpr Query kNearestPoints = {LA3DM_DF_MAX_CELLS, "dims: more than LA3DM_DF_MAX_CELLS (2^28) voxels", false, kPadNone, ""};

// the checks of the two queries' own arguments, before the region's (nearest: n_points = 0)
inline std::string nearest_check(uint32_t obstacle_mask, uint32_t radius, uint32_t n_points) {
    if (obstacle_mask == 0 || (obstacle_mask & ~0x1Fu)) return "obstacle_mask must hold at least one of the bits 0x1F and no other";
    if (radius == 0 || radius > LA3DM_NEAREST_MAX_RADIUS) return "radius must lie in [1, LA3DM_NEAREST_MAX_RADIUS (255)]";
    if (n_points > LA3DM_SCORE_MAX_POINTS) return "n_points: more than LA3DM_SCORE_MAX_POINTS (2^20) points";
    return "";
}

// nearest_points' checks that follow the region's: the buffers
inline std::string nearest_buffers(uint32_t n_points, bool has_points, bool has_out, bool has_any) {
    if (n_points == 0) return "";
    if (!has_points) return "points3 is NULL";
    if (!has_out) return "out is NULL";
    if (!has_any) return "out: cls, voxel, index or d2 must not be NULL";
    return "";
}

// words of one viewpoint's set
inline uint32_t gain_words(uint64_t total) { return (uint32_t)((total + 31) / 32); }

// the checks that follow the region's: the size of the sets, then the buffers (`member` as in resolve)
inline std::string gain_buffers(uint64_t total, uint32_t n, bool has_origins, bool has_offsets, bool has_out, bool has_gain,
                                const char *member) {
    if ((uint64_t)n * gain_words(total) > LA3DM_GAIN_MAX_WORDS) return "n * W: more than LA3DM_GAIN_MAX_WORDS (2^28) words of sets, W = ceil(nx ny nz / 32)";
    if (n == 0) return "";
    if (!has_origins) return "origins3 is NULL";
    if (!has_offsets) return "offsets3 is NULL";
    if (!has_out) return "out is NULL";
    if (!has_gain) return std::string("out") + member + "gain must not be NULL";
    return "";
}

// the checks of reach's own arguments and buffers, all before the region's (`member` as in resolve)
inline std::string reach_check(uint32_t pass_mask, uint32_t obstacle_mask, uint32_t clearance, uint32_t connectivity, uint32_t max_steps,
                               uint32_t n_seeds, uint32_t n_targets, bool has_seeds, bool has_targets, bool has_out, bool has_steps,
                               bool has_target_steps, const char *member) {
    if (pass_mask == 0 || (pass_mask & ~0x1Fu)) return "pass_mask must hold at least one of the bits 0x1F and no other";
    if (obstacle_mask & ~0x1Fu) return "obstacle_mask must hold no bit above 0x1F";
    if (clearance > 0 && obstacle_mask == 0) return "obstacle_mask must hold at least one of the bits 0x1F with clearance > 0";
    if (clearance > LA3DM_DF_MAX_RADIUS) return "clearance must not exceed LA3DM_DF_MAX_RADIUS (1024)";
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) return "connectivity must be 6, 18 or 26";
    if (max_steps == 0 || max_steps > LA3DM_REACH_MAX_STEPS) return "max_steps must lie in [1, LA3DM_REACH_MAX_STEPS (2^16)]";
    if (n_seeds > LA3DM_REACH_MAX_SEEDS) return "n_seeds: more than LA3DM_REACH_MAX_SEEDS (2^20) seeds";
    if (n_targets > (1u << 28)) return "n_targets: more than 2^28 targets";
    if (n_seeds > 0 && !has_seeds) return "seeds is NULL with n_seeds > 0";
    if (n_targets > 0 && !has_targets) return "targets is NULL with n_targets > 0";
    if (!has_out) return "out is NULL";
    const std::string out = std::string("out") + member;
    if (!has_steps && !has_target_steps) return out + "steps or " + out + "target_steps must not be NULL";
    if (has_target_steps && n_targets == 0) return out + "target_steps is set with n_targets = 0";
    if (!has_target_steps && n_targets > 0) return out + "target_steps must not be NULL with n_targets > 0";
    return "";
}

// the checks of travel's own arguments and buffers, all before the region's (`member` as in resolve)
inline std::string travel_check(const la3dm_travel_params *p, uint32_t n_seeds, uint32_t n_targets, bool has_seeds, bool has_targets,
                                bool has_out, bool has_cost, bool has_target_cost, const char *member) {
    if (!p) return "params is NULL";
    if (p->pass_mask == 0 || (p->pass_mask & ~0x1Fu)) return "pass_mask must hold at least one of the bits 0x1F and no other";
    if (p->obstacle_mask & ~0x1Fu) return "obstacle_mask must hold no bit above 0x1F";
    if ((p->clearance > 0 || p->soft_radius > 0) && p->obstacle_mask == 0)
        return "obstacle_mask must hold at least one of the bits 0x1F with clearance > 0 or soft_radius > 0";
    if (p->clearance > LA3DM_DF_MAX_RADIUS) return "clearance must not exceed LA3DM_DF_MAX_RADIUS (1024)";
    if (p->soft_radius > LA3DM_DF_MAX_RADIUS) return "soft_radius must not exceed LA3DM_DF_MAX_RADIUS (1024)";
    if (p->soft_radius > 0 && p->penalty == 0) return "penalty must be >= 1 with soft_radius > 0";
    if (p->penalty > LA3DM_TRAVEL_MAX_PENALTY) return "penalty must not exceed LA3DM_TRAVEL_MAX_PENALTY (2^16)";
    for (int k = 0; k < 3; ++k)
        if (p->move_cost[k] == 0 || p->move_cost[k] > LA3DM_TRAVEL_MAX_MOVE) return "move_cost: every entry must lie in [1, LA3DM_TRAVEL_MAX_MOVE (2^16)]";
    if (p->connectivity != 6 && p->connectivity != 18 && p->connectivity != 26) return "connectivity must be 6, 18 or 26";
    if (p->max_cost == 0 || p->max_cost > LA3DM_TRAVEL_MAX_COST) return "max_cost must lie in [1, LA3DM_TRAVEL_MAX_COST (2^31)]";
    if (n_seeds > LA3DM_TRAVEL_MAX_SEEDS) return "n_seeds: more than LA3DM_TRAVEL_MAX_SEEDS (2^20) seeds";
    if (n_targets > (1u << 28)) return "n_targets: more than 2^28 targets";
    if (n_seeds > 0 && !has_seeds) return "seeds is NULL with n_seeds > 0";
    if (n_targets > 0 && !has_targets) return "targets is NULL with n_targets > 0";
    if (!has_out) return "out is NULL";
    const std::string out = std::string("out") + member;
    if (!has_cost && !has_target_cost) return out + "cost or " + out + "target_cost must not be NULL";
    if (has_target_cost && n_targets == 0) return out + "target_cost is set with n_targets = 0";
    if (!has_target_cost && n_targets > 0) return out + "target_cost must not be NULL with n_targets > 0";
    return "";
}

// travel's entry word of a voxel whose class is in pass_mask: pen(v), or kTravelBlocked where the clearance closes it.
// d2 = distance_field's word (LA3DM_DF_FAR without a distance transform).  One definition for the host form; the device
// kernel (csrc/devmap_travel.h, tv_entry) is its twin.
constexpr uint32_t kTravelBlocked = 0xFFFFFFFFu;
// pen(v): falls linearly in the squared distance from just under `penalty` next to an obstacle to 0 at soft_radius
LA3DM_HD inline uint32_t travel_pen(uint32_t soft_radius, uint32_t penalty, uint32_t d2) {
    const uint32_t s2 = soft_radius * soft_radius;
    return s2 > 0 && d2 <= s2 ? (uint32_t)((uint64_t)penalty * (s2 - d2) / s2) : 0u;
}
inline uint32_t travel_entry(const la3dm_travel_params &p, uint32_t d2) {
    if (p.clearance > 0 && d2 != LA3DM_DF_FAR && d2 <= p.clearance * p.clearance) return kTravelBlocked;
    return travel_pen(p.soft_radius, p.penalty, d2);
}

// ---- score_paths (contract: include/la3dm_hip.h, la3dm_devmap_score_paths_host) ----
constexpr Query kPaths = {LA3DM_DF_MAX_CELLS, "dims: more than LA3DM_DF_MAX_CELLS (2^28) voxels", false, kPadNone, ""};

// the checks of score_paths' own arguments and buffers, all before the region's (`member` as in resolve)
inline std::string paths_check(const la3dm_paths_params *p, uint32_t n_paths, uint32_t n_way, bool has_ways, bool has_out, bool has_cost,
                               const char *member) {
    if (!p) return "params is NULL";
    if (p->obstacle_mask == 0 || (p->obstacle_mask & ~0x1Fu)) return "obstacle_mask must hold at least one of the bits 0x1F and no other";
    if (p->clearance > LA3DM_DF_MAX_RADIUS) return "clearance must not exceed LA3DM_DF_MAX_RADIUS (1024)";
    if (p->soft_radius > LA3DM_DF_MAX_RADIUS) return "soft_radius must not exceed LA3DM_DF_MAX_RADIUS (1024)";
    if (p->soft_radius > 0 && p->penalty == 0) return "penalty must be >= 1 with soft_radius > 0";
    if (p->penalty > LA3DM_TRAVEL_MAX_PENALTY) return "penalty must not exceed LA3DM_TRAVEL_MAX_PENALTY (2^16)";
    for (int k = 0; k < 3; ++k)
        if (p->move_cost[k] == 0 || p->move_cost[k] > LA3DM_TRAVEL_MAX_MOVE) return "move_cost: every entry must lie in [1, LA3DM_TRAVEL_MAX_MOVE (2^16)]";
    if (p->max_steps == 0 || p->max_steps > LA3DM_PATHS_MAX_STEPS) return "max_steps must lie in [1, LA3DM_PATHS_MAX_STEPS (2^20)]";
    if (n_way == 0 || n_way > LA3DM_PATHS_MAX_WAY) return "n_way must lie in [1, LA3DM_PATHS_MAX_WAY (1024)]";
    if (n_paths > LA3DM_PATHS_MAX_PATHS) return "n_paths: more than LA3DM_PATHS_MAX_PATHS (2^20) paths";
    if ((uint64_t)n_paths * n_way > LA3DM_PATHS_MAX_WAYPOINTS) return "n_paths * n_way: more than LA3DM_PATHS_MAX_WAYPOINTS (2^26) waypoints";
    if (n_paths == 0) return "";
    if (!has_ways) return "ways3 is NULL";
    if (!has_out) return "out is NULL";
    if (!has_cost) return std::string("out") + member + "cost must not be NULL";
    return "";
}

// the radius of score_paths' distance transform
inline uint32_t paths_radius(const la3dm_paths_params &p) { return std::max(1u, std::max(p.clearance, p.soft_radius)); }

// The voxel of a waypoint: G[c] = b * lim + cell per axis (axis_voxel), false where a coordinate fails the range test
// (the path is then INVALID).  For lim <= 32 (block_depth <= 6), -2^30 < G[c] < 2^30 + 2^25: every G fits 32 bits signed
// and every difference of two 33.
LA3DM_HD inline bool path_waypoint(const float *w3, float resolution, float block_size, int lim, long long *G) {
    for (int c = 0; c < 3; ++c)
        if (!axis_in_range(w3[c], resolution)) return false;
    for (int c = 0; c < 3; ++c) {
        const AxisVoxel v = axis_voxel(w3[c], resolution, block_size, lim);
        G[c] = v.b * lim + v.cell;
    }
    return true;
}

// the length of the segment from voxel A to voxel B: the largest |B[c] - A[c]|
LA3DM_HD inline long long path_segment(const long long *A, const long long *B) {
    long long n = 0;
    for (int c = 0; c < 3; ++c) {
        const long long d = B[c] - A[c], m = d < 0 ? -d : d;
        n = m > n ? m : n;
    }
    return n;
}

// One axis of the voxel at step s of a segment of length n >= 1 that starts at a and moves by d: a + floor((2 s d + n) /
// (2 n)).  0 <= s <= min(n, 2^20 + 1) and |d| <= n < 2^33 (path_waypoint's range): |2 s d + n| < 2^56, no overflow.
LA3DM_HD inline long long path_sample(long long a, long long d, long long n, long long s) {
    const long long num = 2 * s * d + n, den = 2 * n;
    long long q = num / den;
    if (num % den < 0) --q;   // floor, not truncation
    return a + q;
}

// the move from voxel u to voxel v of a walk: the number of their non-zero differences, 1 ... 3
LA3DM_HD inline uint32_t path_move(const long long *u, const long long *v) { return (uint32_t)(u[0] != v[0]) + (u[1] != v[1]) + (u[2] != v[2]); }

// The voxel v against the region: false where it is outside, else f = its flat index.
LA3DM_HD inline bool path_inside(const long long *v, const uint32_t *g0, const uint32_t *dims, uint32_t &f) {
    uint32_t at[3];
    for (int c = 0; c < 3; ++c) {
        const long long q = v[c] - (long long)g0[c];
        if (q < 0 || q >= (long long)dims[c]) return false;
        at[c] = (uint32_t)q;
    }
    f = (at[0] * dims[1] + at[1]) * dims[2] + at[2];
    return true;
}

// the entry of a voxel with distance word d2: blocked, or what entering it adds to the move
LA3DM_HD inline bool path_blocked(uint32_t clearance, uint32_t d2) { return d2 != LA3DM_DF_FAR && d2 <= clearance * clearance; }
LA3DM_HD inline uint32_t path_entry(const la3dm_paths_params &p, uint32_t nz, uint32_t d2) {
    const uint32_t move = nz == 1u ? p.move_cost[0] : (nz == 2u ? p.move_cost[1] : p.move_cost[2]);   // (no runtime-indexed array: registers)
    return move + travel_pen(p.soft_radius, p.penalty, d2);
}

// ---- footing (contract: include/la3dm_hip.h, la3dm_devmap_footing_host) ----
// the checks of footing's own arguments and of its list, all before the region's
inline std::string footing_check(const la3dm_footing_params *p, uint64_t cap, bool has_index, const char *member) {
    if (!p) return "params is NULL";
    if (p->support_mask == 0 || (p->support_mask & ~0x1Fu)) return "support_mask must hold at least one of the bits 0x1F and no other";
    if (p->clear_mask == 0 || (p->clear_mask & ~0x1Fu)) return "clear_mask must hold at least one of the bits 0x1F and no other";
    if (p->support_mask & p->clear_mask) return "support_mask and clear_mask must not overlap";
    if (p->headroom == 0 || p->headroom > LA3DM_FOOTING_MAX_HEADROOM) return "headroom must lie in [1, LA3DM_FOOTING_MAX_HEADROOM (32)]";
    if (p->radius > LA3DM_FOOTING_MAX_RADIUS) return "radius must not exceed LA3DM_FOOTING_MAX_RADIUS (8)";
    if (p->step > LA3DM_FOOTING_MAX_STEP || p->step >= p->headroom) return "step must not exceed LA3DM_FOOTING_MAX_STEP (4) and must be below headroom";
    if (p->min_support > la3dm_footing::disc_cells(p->radius)) return "min_support must not exceed the cells of the footprint, N";
    if (cap > 0 && !has_index) return std::string("out") + member + "index must not be NULL with cap > 0";
    return "";
}

// the region's checks of footing: limit and range on the padded box of these (checked) parameters
inline Query footing_query(const la3dm_footing_params &p) {
    return Query{LA3DM_FOOTING_MAX_CELLS,
                 "dims: more than LA3DM_FOOTING_MAX_CELLS (2^28) voxels in the padded box",
                 false,
                 Pad{{p.radius, p.radius, 1u + p.step}, {p.radius, p.radius, p.headroom - 1u + p.step}, "dims: the block fields of the padded box leave [0, 2^20)"},
                 ""};
}

inline la3dm_footing::Params footing_params(const la3dm_footing_params &p) {
    return la3dm_footing::Params{p.support_mask, p.clear_mask, p.headroom, p.radius, p.step, p.min_support};
}

// ---- surface (contract: include/la3dm_hip.h, la3dm_devmap_surface_host) ----
// the checks of surface's own arguments and of its list, all before the region's (`out` may be null)
inline std::string surface_check(const la3dm_surface_params *p, uint64_t cap, const la3dm_surface_out *out, const char *member) {
    if (!p) return "params is NULL";
    if (p->solid_mask == 0 || (p->solid_mask & ~0x1Fu)) return "solid_mask must hold at least one of the bits 0x1F and no other";
    if (p->open_mask == 0 || (p->open_mask & ~0x1Fu)) return "open_mask must hold at least one of the bits 0x1F and no other";
    if (p->solid_mask & p->open_mask) return "solid_mask and open_mask must not overlap";
    if (p->smooth > LA3DM_SURFACE_MAX_SMOOTH) return "smooth must not exceed LA3DM_SURFACE_MAX_SMOOTH (4)";
    if (out && out->normal && !out->index) return std::string("out") + member + "normal is set without out" + member + "index";
    if (cap > 0 && !(out && (out->index || out->faces))) return std::string("out") + member + "index or out" + member + "faces must not be NULL with cap > 0";
    return "";
}

// the region's checks of surface: limit and range on the box padded by smooth + 1 voxels on all six sides
inline Query surface_query(const la3dm_surface_params &p) {
    const uint32_t pad = p.smooth + 1u;
    return Query{LA3DM_SURFACE_MAX_CELLS,
                 "dims: more than LA3DM_SURFACE_MAX_CELLS (2^28) voxels in the padded box",
                 false,
                 Pad{{pad, pad, pad}, {pad, pad, pad}, "dims: the block fields of the padded box leave [0, 2^20)"},
                 ""};
}

inline la3dm_surface::Params surface_params(const la3dm_surface_params &p) { return la3dm_surface::Params{p.solid_mask, p.open_mask, p.smooth}; }

// ---- drive (contract: include/la3dm_hip.h, la3dm_devmap_drive_host) ----
static_assert(LA3DM_DRIVE_MAX_STEP == LA3DM_FOOTING_MAX_STEP && LA3DM_DRIVE_MAX_STEP == la3dm_drive::kMaxStep && LA3DM_DRIVE_NONE == la3dm_drive::kNone,
              "a move climbs what footing calls climbable; host/drive_cells.h states the two constants again");
constexpr Query kDrive = {LA3DM_DRIVE_MAX_CELLS, "dims: more than LA3DM_DRIVE_MAX_CELLS (2^28) voxels in the region rounded up to whole bricks", false, kPadNone, "",
                          LA3DM_DRIVE_BRICK};

// the checks of drive's own arguments and buffers, all before the region's (`member` as in resolve); footing mode goes on
// with footing_check(p->footing, 0, false, member)
inline std::string drive_check(const la3dm_drive_params *p, uint32_t n_seeds, uint32_t n_targets, bool has_seeds, bool has_targets,
                               const la3dm_drive_out *out, const char *member) {
    if (!p) return "params is NULL";
    if (p->connectivity != 4 && p->connectivity != 8) return "connectivity must be 4 or 8";
    if (p->step > LA3DM_DRIVE_MAX_STEP) return "step must not exceed LA3DM_DRIVE_MAX_STEP (4)";
    if (p->snap > LA3DM_DRIVE_MAX_SNAP) return "snap must not exceed LA3DM_DRIVE_MAX_SNAP (32)";
    for (int k = 0; k < 2; ++k)
        if (p->move_cost[k] == 0 || p->move_cost[k] > LA3DM_TRAVEL_MAX_MOVE) return "move_cost: both entries must lie in [1, LA3DM_TRAVEL_MAX_MOVE (2^16)]";
    if (p->climb_up > LA3DM_TRAVEL_MAX_MOVE) return "climb_up must not exceed LA3DM_TRAVEL_MAX_MOVE (2^16)";
    if (p->climb_down > LA3DM_TRAVEL_MAX_MOVE) return "climb_down must not exceed LA3DM_TRAVEL_MAX_MOVE (2^16)";
    if (p->max_cost == 0 || p->max_cost > LA3DM_TRAVEL_MAX_COST) return "max_cost must lie in [1, LA3DM_TRAVEL_MAX_COST (2^31)]";
    if (p->n_members > LA3DM_DRIVE_MAX_MEMBERS) return "n_members: more than LA3DM_DRIVE_MAX_MEMBERS (2^28) entries";
    if (n_seeds > LA3DM_DRIVE_MAX_SEEDS) return "n_seeds: more than LA3DM_DRIVE_MAX_SEEDS (2^20) seeds";
    if (n_targets > (1u << 28)) return "n_targets: more than 2^28 targets";
    if (n_seeds > 0 && !has_seeds) return "seeds is NULL with n_seeds > 0";
    if (n_targets > 0 && !has_targets) return "targets is NULL with n_targets > 0";
    if (p->n_members > 0 && !p->members) return "members is NULL with n_members > 0";
    if (p->footing && p->members) return "footing and members are both set: members must be NULL and n_members 0 in footing mode";
    if (!p->footing && !p->members) return "footing and members are both NULL: one of the two modes must be chosen";
    if (!out) return "out is NULL";
    const std::string o = std::string("out") + member;
    if (out->of_member && p->footing) return o + "of_member is set in footing mode";
    if (out->of_member && p->n_members == 0) return o + "of_member is set with n_members = 0";
    if (!out->cost && !out->of_member && !out->target_cost) return o + "cost, " + o + "of_member or " + o + "target_cost must not be NULL";
    if (out->target_cost && n_targets == 0) return o + "target_cost is set with n_targets = 0";
    if (out->target_index && n_targets == 0) return o + "target_index is set with n_targets = 0";
    if (!out->target_cost && n_targets > 0) return o + "target_cost must not be NULL with n_targets > 0";
    return "";
}

inline la3dm_drive::Params drive_params(const la3dm_drive_params &p) {
    return la3dm_drive::Params{p.connectivity, p.step, p.snap, {p.move_cost[0], p.move_cost[1]}, p.climb_up, p.climb_down, p.max_cost};
}

// the checks of clusters' own arguments and buffers, all before the region's; `out` may be null
inline std::string clusters_check(const la3dm_clusters_params *p, const la3dm_clusters_out *out) {
    if (!p) return "params is NULL";
    if (p->member_mask == 0 || (p->member_mask & ~0x1Fu)) return "member_mask must hold at least one of the bits 0x1F and no other";
    if (p->connectivity != 6 && p->connectivity != 18 && p->connectivity != 26) return "connectivity must be 6, 18 or 26";
    if (p->tile % LA3DM_CLUSTERS_BRICK != 0 || p->tile > LA3DM_CLUSTERS_MAX_TILE)
        return "tile must be 0 or a multiple of LA3DM_CLUSTERS_BRICK (8) of at most LA3DM_CLUSTERS_MAX_TILE (2^15)";
    if (p->min_size == 0) return "min_size must be >= 1";
    if (p->from_list > 1) return "from_list must be 0 or 1";
    if (p->n_members > LA3DM_CLUSTERS_MAX_MEMBERS) return "n_members: more than LA3DM_CLUSTERS_MAX_MEMBERS (2^28) entries";
    if (p->n_members > 0 && !p->members) return "members is NULL with n_members > 0";
    if (out && out->of_member && p->from_list == 0) return "of_member is set with from_list = 0";
    if (p->cap > 0 && !(out && (out->first || out->size || out->lo || out->hi || out->sum || out->rep)))
        return "cap > 0 with no record array (first, size, lo, hi, sum, rep)";
    return "";
}

// the limits of clusters that follow the region's checks
inline std::string clusters_region_check(const uint32_t *dims) {
    for (int k = 0; k < 3; ++k)
        if (dims[k] > LA3DM_CLUSTERS_MAX_AXIS) return "dims: an axis longer than LA3DM_CLUSTERS_MAX_AXIS (2^15)";
    uint64_t cells = 1;
    for (int k = 0; k < 3; ++k) cells *= ((uint64_t)dims[k] + LA3DM_CLUSTERS_BRICK - 1) / LA3DM_CLUSTERS_BRICK * LA3DM_CLUSTERS_BRICK;   // < 2^46
    if (cells > LA3DM_CLUSTERS_MAX_CELLS) return "dims: more than LA3DM_CLUSTERS_MAX_CELLS (2^28) voxels in the region rounded up to whole bricks";
    return "";
}

}  // namespace la3dm_region

#endif
