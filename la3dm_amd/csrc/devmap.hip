// devmap.hip — device-resident map: BGKOctoMap::insert_pointcloud start to finish on the GPU
// (C ABI: the la3dm_devmap_* entry points of include/la3dm_hip.h; kernels: devmap_kernels.h).
// The host only sizes launches (a handful of scalar read-backs per scan) and walks the float-stepped
// candidate loops of get_blocks_in_bbox (a few dozen iterations per axis).  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <cstring>   // (before rocPRIM: one of its iterator headers calls memset unqualified)

#include <rocprim/rocprim.hpp>

#include <string>
#include <vector>

#include "la3dm_ctx.h"
#include "devmap_kernels.h"
#include "devmap_scan.h"
#include "devmap_sort.h"
#include "devmap_lv_kernels.h"
#include "devmap_depth3.h"
#include "devmap_grid_keys.h"
#include "host/region_contract.h"
#include "devmap_raycast.h"
#include "devmap_region.h"
#include "devmap_distance.h"
#include "devmap_frontier.h"
#include "devmap_footing.h"
#include "devmap_surface.h"
#include "devmap_gain.h"
#include "devmap_score.h"
#include "devmap_nearest.h"
#include "devmap_paths.h"
#include "devmap_reach.h"
#include "devmap_travel.h"
#include "devmap_drive.h"
#include "devmap_clusters.h"
#include "devmap_pack.h"
#include "devmap_merge.h"
#include "devmap_diff.h"
#include "devmap_evict.h"
#include "host/pack_format.h"
#include "host/region_blocks.h"

using namespace la3dm_dev;

namespace {
double wall() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline uint32_t cdiv(uint64_t a, uint32_t b) { return (uint32_t)((a + b - 1) / b); }
inline uint32_t npb_of(int depth) {
    uint32_t n = 0;
    for (int d = 0; d < depth; ++d) n += 1u << (3 * d);
    return n;
}
}  // namespace

struct la3dm_devmap {
    la3dm_ctx *ctx = nullptr;
    uint32_t depth = 0, npb = 0, ncell = 0;
    float block_size = 0.f, init_A = 0.f, init_B = 0.f;
    // pool + table
    size_t cap_blocks = 0;
    uint32_t n_blocks = 0;
    bool insert_into_empty = false;  // this insert started on a map without blocks: every test block of its first pass is new, i.e. un-pruned
    float *A = nullptr, *B = nullptr;
    uint8_t *S = nullptr;
    long long *blk_key = nullptr;
    uint32_t tab_cap = 0;
    long long *tab_key = nullptr;
    uint32_t *tab_val = nullptr;
    // small fixed buffers
    uint32_t *d_cnt = nullptr, *h_cnt = nullptr;  // counters (device / pinned host)
    uint32_t *d_mm = nullptr;   // [0..5] encoded min / max, [6] arrival counter of the min/max launches
    float *d_bbox = nullptr, *h_bbox = nullptr;
    GridParams *d_gp = nullptr, *h_gp = nullptr;
    // arenas (grow only)
    Arena cloud, hits, keep, nfree, keep_off, free_off, frees_raw, frees_ds, xy;
    Arena k0, k1, v0, v1, flag, scan, seg_start, seg_key, cub_tmp, big, chunk_desc;
    Arena scan_status;            // devmap_scan.h: two arrays of per-tile status words, zero between launches
    size_t scan_tiles = 0, scan_dirty[2] = {0, 0};   // status entries in use per array
    uint32_t scan_seq = 0;
    Arena radix_state, radix_tmp; // devmap_sort.h: histograms + two status arrays (zero between sorts); ping-pong buffers
    size_t radix_tiles = 0;
    uint32_t radix_seq = 0;       // sorts so far: which of the two histograms is current
    std::vector<uint8_t> lv_axis_host;   // BGK-LV: staging of the per-axis candidate tables (kept until the next insert)
    bool test_sort = true;        // LA3DM_TEST_SORT=0: the test blocks stay in candidate order (no heaviest-first sort)
    bool own_sort = true;         // LA3DM_OWN_SORT=0: rocPRIM's radix sort instead (A/B)
    bool counters_clean = false;  // the last insert's final launch left the counter block as dm_begin would (dm_commit_prune)
    int spec_bits = 32;           // key digits (x 8 bits) the cloud's own voxel filter needed last time (voxel_grid)
    Arena train, grid, axis_tab, m_code, q_out;
    Arena df_work;                // distance field: 4 bytes per voxel (obstacle bits / z distances, then the partial sums)
    Arena fr_work;                // frontier: 1/2 byte per padded voxel (two bit streams, popcounts, prefixes: devmap_frontier.h)
    Arena ft_work;                // footing: 7/8 byte per padded voxel (five bit streams, popcounts, prefixes: devmap_footing.h)
    Arena sf_work;                // surface: 11/8 byte per padded voxel (eight bit streams, candidates, popcounts, prefixes: devmap_surface.h)
    Arena gain_work;              // gain: one bit per voxel and viewpoint (the sets: devmap_gain.h)
    Arena score_work;             // score_poses: d2 (4 bytes per voxel), then the chunks' partial records (devmap_score.h); score_paths: d2 (devmap_paths.h)
    Arena nt_work;                // nearest: the y keys (4 bytes per voxel), the z offsets (2), the obstacle bits; nearest_points: index and d2 as well (devmap_nearest.h)
    Arena reach_work;             // reach: four bit streams of the padded box, the level counts, 4 bytes per voxel (devmap_reach.h)
    Arena travel_work;            // travel: two brick-major cost buffers, the entry words, side / active per brick, the round counts, d2 (devmap_travel.h)
    Arena drive_work;             // drive: two brick-major cost buffers, the entry words, side / active per brick, the round counts (devmap_drive.h)
    Arena clusters_work;          // clusters: two brick-major label buffers, side / active per brick, the round counts, sizes, flags, numbers (devmap_clusters.h)
    Arena clusters_rec;           // clusters: the records of the clusters written (sums, keys, boxes, first, size, rep)
    Arena pack_stream, pack_counts;   // save / load: the stream as it leaves or enters the device; the blocks' leaf counts (devmap_pack.h)
    la3dm_pack_header pack_hdr;   // the header of the stream being packed (the source of an asynchronous copy)
    Arena c_flag, c_weight, c_scan, t_key0, t_key1, t_ent0, t_ent1, t_blockkey, t_center, t_nbr, t_slot, t_slot0;
    Arena nleaf, leaf_off, leaf_key, leaf_alpha, leaf_beta, leaf_state, leaf_node;
    Arena l_ray_idx, l_rays, l_rows, l_rows_off, l_rflag, l_rscan;  // BGKLOctoMap: beam of every sample, beam segments, training rows
    // BGKLVOctoMap (variant 2): beams, samples, segments, gather grid, packed blocks
    Arena lv_rng, lv_flags, lv_seg, lv_nsamp, lv_nray, lv_samp_off, lv_ray_off, lv_samples, lv_rays, lv_sorted, lv_cell_off;
    Arena lv_beam, lv_mask;
    Arena lv_hcell, lv_hcnt, lv_hoff, lv_hlist;
    Arena cell_cnt, slab_range;   // x-slab partition of a sharded insert: per-cell point counts; {first, last} grid cell of the own slab
    int shard_slab = getenv("LA3DM_SHARD_SLAB") ? atoi(getenv("LA3DM_SHARD_SLAB")) : 1;   // x-slab partition of a sharded insert (default); 0 = every rank builds the CSR of all training blocks (A/B)
    int depth3_batch = getenv("LA3DM_DEPTH3") ? atoi(getenv("LA3DM_DEPTH3")) : -1;   // block_depth 3: leaf lists and write-back + prune with 4 / 8 test blocks per wave (devmap_depth3.h); -1 = by the size of the test list, 0 = the general kernels (A/B)
    bool force_slab = getenv("LA3DM_FORCE_SLAB") && atoi(getenv("LA3DM_FORCE_SLAB")) == 1;   // (test / profiling hook: the x-slab form on an UNSHARDED map, its slab = the whole test list)   // ray shortening on the hit grid (devmap_lv_kernels.h, round 6)
    Arena lv_axis, lv_keys, lv_mult, lv_flag, lv_pos, lv_slot, lv_center, lv_cell0, lv_pslot, lv_pmult, lv_info, lv_prune;
    int32_t *d_lvmm = nullptr, *h_lvmm = nullptr;   // bucket bounds of the finite samples (+ their count)
    uint32_t lv_n_samples = 0, lv_n_rays = 0;
    bool lv_original_size = true;
    la3dm_devmap_lv_stats lv_stats;
    // block-sharded insert (la3dm_devmap_set_shard)
    int dbg_fail_rank = -1;       // LA3DM_INJECT_FRONT_END_FAILURE at la3dm_devmap_create (a test hook), else -1
    int dbg_fail_slab_rank = -1;  // LA3DM_INJECT_SLAB_FAILURE: that rank of a sharded map fails in build_slab_csr, i.e. AFTER the cut (test hook)
    int dbg_stuck_at = 0;         // LA3DM_INJECT_SCAN_STUCK = n at la3dm_devmap_create (a test hook): the n-th counter read-back of this
                                  // map reports the look-back loops' "stuck" bit as if a scan launch had found its state dirty
    uint32_t shard_rank = 0, shard_world = 1;
    la3dm_allgatherv_fn shard_fn = nullptr;
    void *shard_user = nullptr;
    Arena shard_w, shard_cumw, shard_bounds;
    uint32_t *h_shard = nullptr;  // pinned: bounds[world + 1] | leaf_bounds[world + 1]
    std::vector<uint64_t> shard_off[4], shard_bytes[4];   // the all-gather-v's segments (alpha, beta, state, leaf key), per rank
    Arena shard_hist, shard_nown, shard_own_off, shard_cnt, shard_frees;   // sharded sample filter (front_end)
    uint32_t shard_status_failed = 0xFFFFFFFFu;   // (the source of the slot's "failed" preset: lives as long as the map)
    std::vector<uint32_t> shard_hist_host, shard_cnt_host;
    uint32_t n_xy = 0;
    bool mailbox = true;      // read_counters through pinned host memory + a sequence number (LA3DM_MAILBOX=0: copy + sync)
    uint32_t mailbox_seq = 0;
    uint32_t scan_resident = kScanResident, radix_resident_wide = 256, radix_resident_big = 256;   // workgroups the chip holds at once (create)
    uint32_t mailbox_pending = 0;   // sequence number a queued kernel will publish itself (0: none — read_counters launches the publisher)
    bool poisoned = false;  // a failed insert whose block table could not be reconciled with the host's block count
    bool stage_timing = false;  // LA3DM_TIMING=1 at creation: extra synchronisations that split t_pack / t_kernel / t_commit
    la3dm_devmap_stats stats;
};

#define DM_TRY(expr) HIP_TRY(dm->ctx, expr)
#define DM_RESERVE(arena, bytes)                                                    \
    do {                                                                            \
        int rc_ = arena_reserve(dm->ctx, (arena), (bytes) ? (size_t)(bytes) : 16);  \
        if (rc_ != LA3DM_OK) return rc_;                                            \
    } while (0)

static int dm_fail(la3dm_devmap *dm, int code, const std::string &msg) {
    dm->ctx->err = msg;
    return code;
}

// Workgroups of a launch that ends in atomics on a handful of addresses (min/max words, arrival counters): a device-scope
// atomic on one address costs ~25 ns per workgroup, serialised — 512 workgroups spent 12 us on them, whatever the data.
constexpr uint32_t kMinmaxWgs = 128;
// dm_beam_write's workgroups: a thread walks n / (256 x workgroups) beams one after the other, each a chain of two dependent loads before its
// samples can be written (kept? -> the hit and its offsets), and every workgroup ends in twelve atomics of the two box reductions (~25 ns each,
// serialised per address).  Kernel trace (profiles/r06/wgs.txt), 128 / 256 / 512 / 1024 workgroups: configs[1]'s 92 k kept hits 25.9 / 30.2 / 35.0 /
// 33.9 us, configs[4]'s 417 k 75.8 / 62.6 / 66.4 / 84.6 us — 256 from 2^18 kept hits up, 128 below (LA3DM_BEAM_WGS: A/B)
static const uint32_t kBeamWgsEnv = getenv("LA3DM_BEAM_WGS") ? (uint32_t)std::max(1, atoi(getenv("LA3DM_BEAM_WGS"))) : 0u;
static inline uint32_t beam_wgs(uint32_t n_h) { return kBeamWgsEnv ? kBeamWgsEnv : (n_h >= (1u << 18) ? 2u * kMinmaxWgs : kMinmaxWgs); }

// ---- library plumbing: device-wide sort / scan (rocPRIM through hipCUB) ---------------------------------
template <size_t kMergeLimit>
static int sort_pairs_cfg(la3dm_devmap *dm, const uint32_t *k_in, uint32_t *k_out, const uint32_t *v_in, uint32_t *v_out,
                          uint32_t n, int end_bit, int begin_bit = 0) {
    hipStream_t st = dm->ctx->stream;
    size_t tmp = 0;
    using sort_config = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, kMergeLimit>;
    DM_TRY(rocprim::radix_sort_pairs<sort_config>(nullptr, tmp, k_in, k_out, v_in, v_out, (size_t)n, (unsigned)begin_bit, (unsigned)end_bit, st));
    DM_RESERVE(dm->cub_tmp, tmp);
    DM_TRY(rocprim::radix_sort_pairs<sort_config>(dm->cub_tmp.ptr, tmp, k_in, k_out, v_in, v_out, (size_t)n, (unsigned)begin_bit, (unsigned)end_bit, st));
    return LA3DM_OK;
}

// Stable sort of (key, value) pairs on the low `end_bit` key bits: devmap_sort.h (one histogram launch + one launch per
// 8 key bits; the input arrays are left as they are).  rocPRIM's sort (LA3DM_OWN_SORT=0) is kept for comparison: above
// 2^18 items its Onesweep costs three launches per pass, below that its merge sort log2(n / 1024) launch pairs.
// (sort_fusable: the own sort takes this key range, so a caller may hand its key producer to the histogram launch — sort_pairs_src)
static bool sort_fusable(la3dm_devmap *dm, int end_bit, int begin_bit = 0) {
    return dm->own_sort && end_bit <= 32 && end_bit > begin_bit && begin_bit >= 0;
}
struct SortJob {   // a sort between its histogram launch and its passes
    RadixState rs;
    uint32_t n_pass = 0, n_bound = 0;
    int begin_bit = 0;
};
// histogram launch of a sort of at most n_bound keys (the keys come from `src`: n_items items, devmap_sort.h)
template <class Src>
static int sort_begin_src(la3dm_devmap *dm, const Src &src, uint32_t n_items, uint32_t n_bound, int end_bit, int begin_bit, SortJob &job) {
    if (!sort_fusable(dm, end_bit, begin_bit)) return dm_fail(dm, LA3DM_ERR_ARG, "devmap: internal error: fused histogram on a key range the own sort does not take");
    hipStream_t st = dm->ctx->stream;
    const uint32_t n_pass = ((uint32_t)(end_bit - begin_bit) + 7u) / 8u, tiles = cdiv(n_bound, kRsTile);
    if (tiles > dm->radix_tiles) {
        const size_t want = std::max<size_t>(2 * (size_t)tiles, 1024);
        DM_TRY(hipStreamSynchronize(st));
        const size_t bytes = 2 * 4096 * kRsHistCopies + 64 + 2 * want * 1024 + 2 * (want / kRsGroup + 1) * 1024;
        DM_RESERVE(dm->radix_state, bytes);
        DM_TRY(hipMemsetAsync(dm->radix_state.ptr, 0, bytes, st));   // on the sorts' own stream
        dm->radix_tiles = want;
    }
    RadixState &rs = job.rs;   // layout: two histograms (this sort's, the next sort's), 16 spare words, two status arrays, two group arrays
    uint32_t *base = (uint32_t *)dm->radix_state.ptr;
    rs.hist = base + 1024 * kRsHistCopies * (dm->radix_seq & 1u);
    rs.hist_next = base + 1024 * kRsHistCopies * ((dm->radix_seq + 1u) & 1u);
    ++dm->radix_seq;
    rs.ticket = base + 2048 * kRsHistCopies;   // (the 16 spare words)
    rs.status[0] = base + 2048 * kRsHistCopies + 16;
    rs.status[1] = rs.status[0] + dm->radix_tiles * 256;
    rs.agg[0] = rs.status[1] + dm->radix_tiles * 256;
    rs.agg[1] = rs.agg[0] + (dm->radix_tiles / kRsGroup + 1) * 256;
    job.n_pass = n_pass;
    job.n_bound = n_bound;
    job.begin_bit = begin_bit;
    hipLaunchKernelGGL((dm_radix_hist_src<Src>), dim3(std::max<uint32_t>(std::min<uint32_t>(cdiv(n_items, 4 * kRsThreads), 512u), kRsHistCopies)), dim3(kRsThreads), 0, st, src, n_bound, n_items, n_pass, (uint32_t)begin_bit, rs);
    DM_TRY(hipGetLastError());
    return LA3DM_OK;
}
// the passes; n_dev != nullptr: the key count is read there by the launches (n_bound only sizes them)
static int sort_passes(la3dm_devmap *dm, const SortJob &job, const uint32_t *k_in, uint32_t *k_out, const uint32_t *v_in, uint32_t *v_out,
                       const uint32_t *n_dev = nullptr) {
    hipStream_t st = dm->ctx->stream;
    const uint32_t n = job.n_bound, n_pass = job.n_pass, tiles = cdiv(n, kRsTile);
    uint32_t *tk = nullptr, *tv = nullptr;
    if (n_pass > 1) {
        DM_RESERVE(dm->radix_tmp, 8ull * n);
        tk = (uint32_t *)dm->radix_tmp.ptr;
        tv = tk + n;
    }
    const uint32_t *sk = k_in, *sv = v_in;
    for (uint32_t p = 0; p < n_pass; ++p) {
        const bool to_out = ((n_pass - 1u - p) & 1u) == 0u;   // the last pass lands in the output arrays
        RadixArgs a;
        a.k_in = sk;
        a.v_in = sv;
        a.k_out = to_out ? k_out : tk;
        a.v_out = to_out ? v_out : tv;
        a.n = n;
        a.n_dev = n_dev;
        a.n_pass = n_pass;
        a.pass = p;
        a.begin_bit = (uint32_t)job.begin_bit;
        a.counters = dm->d_cnt;
        a.err_slot = (int)kCntError;
        if (tiles <= dm->radix_resident_wide) {   // every tile on the chip at once, sixteen waves each (devmap_sort.h)
            a.use_ticket = 0u;
            hipLaunchKernelGGL((dm_radix_pass<1024, 4>), dim3(tiles), dim3(1024), 0, st, a, job.rs);
        } else {   // 8192-item tiles, one workgroup per CU: every tile on the chip up to ~2 M items (the free samples' filter), through the ticket beyond
            const uint32_t t2 = cdiv(n, 2 * kRsTile);
            a.use_ticket = t2 > dm->radix_resident_big ? 1u : 0u;
            hipLaunchKernelGGL((dm_radix_pass<1024, 8>), dim3(std::min(t2, dm->radix_resident_big)), dim3(1024), 0, st, a, job.rs);
        }
        sk = a.k_out;
        sv = a.v_out;
    }
    DM_TRY(hipGetLastError());
    return LA3DM_OK;
}
template <class Src>
static int sort_pairs_src(la3dm_devmap *dm, const Src &src, uint32_t n_items, const uint32_t *k_in, uint32_t *k_out, const uint32_t *v_in,
                          uint32_t *v_out, uint32_t n, int end_bit, int begin_bit = 0) {
    if (n == 0) return LA3DM_OK;
    SortJob job;
    int rc = sort_begin_src(dm, src, n_items, n, end_bit, begin_bit, job);
    if (rc != LA3DM_OK) return rc;
    return sort_passes(dm, job, k_in, k_out, v_in, v_out);
}

static int sort_pairs(la3dm_devmap *dm, const uint32_t *k_in, uint32_t *k_out, const uint32_t *v_in, uint32_t *v_out,
                      uint32_t n, int end_bit, int begin_bit = 0) {
    if (n == 0) return LA3DM_OK;
    if (!sort_fusable(dm, end_bit, begin_bit))
        return sort_pairs_cfg<(1u << 18)>(dm, k_in, k_out, v_in, v_out, n, end_bit, begin_bit);
    return sort_pairs_src(dm, RsPlainKeys{k_in}, n, k_in, k_out, v_in, v_out, n, end_bit, begin_bit);
}

// The kernel about to be launched publishes the counter block itself (dm_publish_lane) under a fresh sequence number.
static void publish_with(la3dm_devmap *dm, volatile uint32_t *&mailbox, uint32_t &seq) {
    if (!dm->mailbox) return;   // (copy + synchronise mode: read_counters does it all)
    static const bool off = getenv("LA3DM_PUBLISH_IN_KERNEL") && atoi(getenv("LA3DM_PUBLISH_IN_KERNEL")) == 0;
    if (off) return;
    seq = dm->mailbox_pending = ++dm->mailbox_seq;
    mailbox = (volatile uint32_t *)dm->h_cnt;
}

// state of the single-launch scan (devmap_scan.h) for up to n elements
static int scan_state(la3dm_devmap *dm, uint32_t n, ScanState &ss) {
    const size_t tiles = ((size_t)n + kScanTile - 1) / kScanTile;
    if (tiles > dm->scan_tiles) {
        const size_t want = std::max<size_t>(2 * tiles, 4096);
        DM_TRY(hipStreamSynchronize(dm->ctx->stream));
        DM_RESERVE(dm->scan_status, 16 * want + 16);
        DM_TRY(hipMemsetAsync(dm->scan_status.ptr, 0, 16 * want + 16, dm->ctx->stream));   // on the scans' own stream
        dm->scan_tiles = want;
        dm->scan_dirty[0] = dm->scan_dirty[1] = 0;
    }
    // layout: 16 spare bytes, status array 0, status array 1.  The arrays alternate from launch to launch; a launch clears the
    // used part of the other array (written two launches ago), so the array a launch starts on is all zero.
    unsigned long long *base = (unsigned long long *)((uint8_t *)dm->scan_status.ptr + 16);
    const uint32_t cur = dm->scan_seq & 1u;
    ss.status = base + (size_t)cur * dm->scan_tiles;
    ss.other = base + (size_t)(cur ^ 1u) * dm->scan_tiles;
    ss.other_n = (uint32_t)dm->scan_dirty[cur ^ 1u];
    uint32_t *tickets = (uint32_t *)dm->scan_status.ptr;   // (the 16 spare bytes: one ticket per status array)
    ss.ticket = tiles > dm->scan_resident ? tickets + cur : nullptr;
    ss.ticket_other = tickets + (cur ^ 1u);
    dm->scan_dirty[cur ^ 1u] = 0;
    dm->scan_dirty[cur] = tiles;
    ++dm->scan_seq;
    return LA3DM_OK;
}

// out[i] = in[0] + ... + in[i-1]; total_slot >= 0: the sum of all n also goes to d_cnt[total_slot]
// publish: the launch also sends the counter block to the host's mailbox (the next read_counters only waits for it)
static int exclusive_scan(la3dm_devmap *dm, const uint32_t *in, uint32_t *out, uint32_t n, int total_slot = -1, bool publish = false) {
    if (n == 0) {
        if (total_slot >= 0) DM_TRY(hipMemsetAsync(dm->d_cnt + total_slot, 0, 4, dm->ctx->stream));
        return LA3DM_OK;
    }
    ScanState ss;
    int rc = scan_state(dm, n, ss);
    if (rc != LA3DM_OK) return rc;
    ScanArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in;
    a.out = out;
    a.n = n;
    a.counters = dm->d_cnt;
    a.total_slot = total_slot;
    a.zero_slot = -1;
    a.err_slot = (int)kCntError;
    if (publish && total_slot >= 0) publish_with(dm, a.mailbox, a.mailbox_seq);
    hipLaunchKernelGGL(dm_scan_lb<false>, dim3(std::min<uint32_t>(cdiv(n, kScanTile), dm->scan_resident)), dim3(kScanThreads), 0, dm->ctx->stream, a, ss);
    DM_TRY(hipGetLastError());
    return LA3DM_OK;
}

// what pack, pack_region, erase_region, unpack and merge answer on a poisoned map
constexpr const char *kPoisonedText = "the map is poisoned (a failed insert left its block table unreconciled)";

// A scan whose total the host needs before it can go on: the scan over n >= 1 elements, *total = out[n - 1] (callers close
// `in` with an entry of its own, so that is the sum of the rest) and the error word read back, one synchronisation.  A scan
// that found its state in use poisons the map.  also_bytes > 0: device bytes that travel with the same read-back.
static int scan_total(la3dm_devmap *dm, const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *total, void *also_dst = nullptr,
                      const void *also_src = nullptr, size_t also_bytes = 0) {
    hipStream_t st = dm->ctx->stream;
    int rc = exclusive_scan(dm, in, out, n);
    if (rc != LA3DM_OK) return rc;
    uint32_t err = 0;
    if (also_bytes) DM_TRY(hipMemcpyAsync(also_dst, also_src, also_bytes, hipMemcpyDeviceToHost, st));
    DM_TRY(hipMemcpyAsync(total, out + n - 1, 4, hipMemcpyDeviceToHost, st));
    DM_TRY(hipMemcpyAsync(&err, dm->d_cnt + kCntError, 4, hipMemcpyDeviceToHost, st));
    DM_TRY(hipStreamSynchronize(st));
    if (err & kScanErrStuck) {
        dm->poisoned = true;
        return dm_fail(dm, LA3DM_ERR_HIP, "devmap: a prefix-sum launch found its state in use (internal error)");
    }
    return LA3DM_OK;
}

// Segments of a sorted key array (invalid keys last), one launch: head flags, their exclusive scan, the segment starts
// (+ keys), d_cnt[seg_slot] = segments, d_cnt[valid_slot] = valid keys, seg_start[segments] = valid keys;
// zero_slot >= 0: d_cnt[zero_slot] = 0 on the way.
static int scan_heads(la3dm_devmap *dm, const uint32_t *keys, uint32_t n, uint32_t *flag, uint32_t *scan, uint32_t *seg_start,
                      uint32_t *seg_key, int seg_slot, int valid_slot, int zero_slot = -1, bool publish = false) {
    ScanState ss;
    int rc = scan_state(dm, n, ss);
    if (rc != LA3DM_OK) return rc;
    ScanArgs a;
    memset(&a, 0, sizeof(a));
    a.in = keys;
    a.out = scan;
    a.n = n;
    a.counters = dm->d_cnt;
    a.total_slot = -1;
    a.flag = flag;
    a.seg_start = seg_start;
    a.seg_key = seg_key;
    a.seg_slot = seg_slot;
    a.valid_slot = valid_slot;
    a.zero_slot = zero_slot;
    a.err_slot = (int)kCntError;
    if (publish) publish_with(dm, a.mailbox, a.mailbox_seq);
    hipLaunchKernelGGL(dm_scan_lb<true>, dim3(std::min<uint32_t>(cdiv(n, kScanTile), dm->scan_resident)), dim3(kScanThreads), 0, dm->ctx->stream, a, ss);
    DM_TRY(hipGetLastError());
    return LA3DM_OK;
}

static int read_counters(la3dm_devmap *dm) {
    hipStream_t st = dm->ctx->stream;
    if (!dm->mailbox) {
        DM_TRY(hipMemcpyAsync(dm->h_cnt, dm->d_cnt, sizeof(uint32_t) * kCntWords, hipMemcpyDeviceToHost, st));
        DM_TRY(hipStreamSynchronize(st));
        return LA3DM_OK;
    }
    uint32_t seq = dm->mailbox_pending;
    dm->mailbox_pending = 0;
    if (!seq) {
        seq = ++dm->mailbox_seq;
        hipLaunchKernelGGL(dm_publish_counters, dim3(1), dim3(64), 0, st, (const uint32_t *)dm->d_cnt, (volatile uint32_t *)dm->h_cnt, seq);
        DM_TRY(hipGetLastError());
    }
    volatile uint32_t *flag = dm->h_cnt + kCntWords;
    const double t0 = wall();
    for (uint32_t spin = 0; *flag != seq; ++spin) {
        if ((spin & 0x3FFu) == 0x3FFu && wall() - t0 > 2.0) {  // something is wrong (a fault upstream): let HIP report it
            DM_TRY(hipStreamSynchronize(st));
            if (*flag != seq) return dm_fail(dm, LA3DM_ERR_HIP, "devmap: the counter mailbox was not written");
            break;
        }
        __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);   // the counter words are read (non-volatile) after the flag
    if (dm->dbg_stuck_at > 0 && --dm->dbg_stuck_at == 0) dm->h_cnt[kCntError] |= kScanErrStuck;   // (test hook, tests/test_devmap_gpu.py)
    if (dm->h_cnt[kCntError] & (kScanErrStuck | kRsErrStuck)) {
        dm->poisoned = true;
        if (getenv("LA3DM_DEBUG_CNT")) {
            for (int w = 0; w < (int)kCntWords; ++w) fprintf(stderr, "cnt[%d]=%u ", w, dm->h_cnt[w]);
            fprintf(stderr, "\n");
        }
        return dm_fail(dm, LA3DM_ERR_HIP, "devmap: a prefix-sum launch found its state in use (internal error; flags " + std::to_string(dm->h_cnt[kCntError]) + ")");
    }
    return LA3DM_OK;
}

// after the beam-count kernels: a beam that would not terminate, or more samples than the 32-bit offsets can index
static int check_beam_counters(la3dm_devmap *dm) {
    if (dm->h_cnt[kCntError] & kErrBeam)
        return dm_fail(dm, LA3DM_ERR_ARG, "insert_pointcloud: a beam does not terminate (infinite range, or free_resolution too small "
                                          "against the range for fp32 stepping; set max_range / a larger free_resolution)");
    const uint64_t total = (uint64_t)dm->h_cnt[kCntBeamTotal] | ((uint64_t)dm->h_cnt[kCntBeamTotal + 1] << 32);
    if (total > 0x7FFFFFFFull)
        return dm_fail(dm, LA3DM_ERR_ARG, "insert_pointcloud: more than 2^31 beam samples in one scan (raise free_resolution or set max_range)");
    return LA3DM_OK;
}

// pcl::VoxelGrid centroid filter (bgkoctomap.cpp:419-431) on the device.  d_in: n packed xyz; the result is
// written to `out` (reserved here) and its point count returned.  One read-back (cell count).
// key_bits: number of low key bits that can differ between cells (32 = unknown); must satisfy
// cell count <= 2^key_bits - 1 so that the all-ones key of a non-finite point still sorts behind every cell.
// Round 5: key_bits = 0 — the caller does not know (the cloud's own filter: its grid is reduced on the device by this call): the
// sort runs on as many 8-bit digits as the LAST such call needed (dm->spec_bits; all four the first time), and the
// GridParams that come back with the cell count say whether that was enough; if not (the scene grew past 2^16 / 2^24 cells)
// the filter is simply run again on 32 bits — a constant top digit used to cost a copy pass (10 us) on every insert.
static const uint32_t kBigCellEnv = getenv("LA3DM_BIG_CELL") ? (uint32_t)std::max(8, atoi(getenv("LA3DM_BIG_CELL"))) : 0u;   // (A/B) cells above this many points: one wave each
static const uint32_t kBigCellWgs = getenv("LA3DM_BIG_WGS") ? (uint32_t)atoi(getenv("LA3DM_BIG_WGS")) : 2048u;   // waves (one per cell at a time) of dm_grid_centroids_big
static int voxel_grid(la3dm_devmap *dm, const float *d_in, uint32_t n, float leaf, Arena &out, uint32_t *n_out, int key_bits = 0,
                      bool params_ready = false) {
    hipStream_t st = dm->ctx->stream;
    *n_out = 0;
    if (n == 0) return LA3DM_OK;
    const bool speculate = key_bits == 0;
    if (speculate) key_bits = dm->spec_bits;
    const float inv = 1.0f / leaf;
    DM_RESERVE(dm->k0, 4ull * n);
    DM_RESERVE(dm->k1, 4ull * n);
    DM_RESERVE(dm->v0, 4ull * n);
    DM_RESERVE(dm->v1, 4ull * n);
    DM_RESERVE(dm->flag, 4ull * n);
    DM_RESERVE(dm->scan, 4ull * n);
    DM_RESERVE(dm->seg_start, 4ull * (n + 1));
    uint32_t *k0 = (uint32_t *)dm->k0.ptr, *k1 = (uint32_t *)dm->k1.ptr, *v0 = (uint32_t *)dm->v0.ptr, *v1 = (uint32_t *)dm->v1.ptr;
    uint32_t *flag = (uint32_t *)dm->flag.ptr, *scan = (uint32_t *)dm->scan.ptr, *seg_start = (uint32_t *)dm->seg_start.ptr;
    if (!params_ready) {   // (the producer of d_in may have reduced its box and left the GridParams already)
        MinmaxFin fin = {1, inv, dm->d_gp, nullptr, dm->d_cnt, dm->d_mm + 6, nullptr};
        hipLaunchKernelGGL(dm_minmax<3>, dim3(std::min<uint32_t>(cdiv(n, 1024), kMinmaxWgs)), dim3(256), 0, st, d_in, n, dm->d_mm, fin);
    }
    int rc;
    if (sort_fusable(dm, key_bits)) {   // the cell keys are written by the sort's histogram launch
        const GridCellsSrc src = {d_in, inv, dm->d_gp, k0, v0};
        rc = sort_pairs_src(dm, src, n, k0, k1, v0, v1, n, key_bits);
    } else {
        hipLaunchKernelGGL(dm_grid_cells, dim3(cdiv(n, 256)), dim3(256), 0, st, d_in, n, inv, dm->d_gp, k0, v0);
        rc = sort_pairs(dm, k0, k1, v0, v1, n, key_bits);
    }
    if (rc != LA3DM_OK) return rc;
    if (dm->ctx->opt_grid_order == 1) {
        // Verification mode (la3dm_set_option "grid_order" 1): the order of the points INSIDE a cell — the order of the fp32
        // centroid sums — as pcl::VoxelGrid leaves it: std::sort over {cell index, cloud index} comparing the cell index alone
        // (PCL 1.10 voxel_grid.hpp, call site src/bgkoctomap/bgkoctomap.cpp:419-431), i.e. whatever libstdc++'s introsort does with equal
        // keys.  That is a sequential algorithm: the keys go to the host, the host's own std::sort runs on them exactly as PCL's
        // does, the permutation comes back.  Slow by design (two synchronous copies and a host sort per filter call), never the
        // default; with "fast_trig" 3 the BGK family is then bit-identical to the restatement's set_modes(1, 1) — the arithmetic a
        // ROS Noetic build of the reference most plausibly runs (tests/test_likely_trig_gpu.py).
        std::vector<uint32_t> hk(n);
        DM_TRY(hipMemcpyAsync(hk.data(), k0, 4ull * n, hipMemcpyDeviceToHost, st));
        DM_TRY(hipStreamSynchronize(st));
        std::vector<std::pair<unsigned, unsigned>> iv;
        iv.reserve(n);
        for (uint32_t i = 0; i < n; ++i)
            if (hk[i] != kInvalidCell) iv.emplace_back((unsigned)hk[i], (unsigned)i);
        struct PclLess {
            bool operator()(const std::pair<unsigned, unsigned> &a, const std::pair<unsigned, unsigned> &b) const { return a.first < b.first; }
        };
        std::sort(iv.begin(), iv.end(), PclLess());
        for (size_t j = 0; j < iv.size(); ++j) hk[j] = iv[j].second;
        if (!iv.empty()) DM_TRY(hipMemcpyAsync(v1, hk.data(), 4ull * iv.size(), hipMemcpyHostToDevice, st));
        DM_TRY(hipStreamSynchronize(st));   // (hk is a local)
    }
    // (no head-flag / prefix arrays: their one reader, the chunk descriptors, asks the sorted keys instead — devmap_grid_keys.h;
    //  LA3DM_GRID_KEYS=0 keeps the round-5 form for A/B)
    static const bool kGridKeys = !(getenv("LA3DM_GRID_KEYS") && atoi(getenv("LA3DM_GRID_KEYS")) == 0);
    rc = scan_heads(dm, k1, n, kGridKeys ? nullptr : flag, kGridKeys ? nullptr : scan, seg_start, nullptr, (int)kCntGridSegs, (int)kCntGridValid,
                    (int)kCntBig, true);
    if (rc != LA3DM_OK) return rc;
    // The centroid kernels take the cell count from the counter block and are sized for the worst case (every point its
    // own cell), so they are queued before the host waits for the counters: the wait and the next launches' latency overlap
    // with them.  (A pass-through grid lets them write junk that the copy below replaces.)
    DM_RESERVE(out, 12ull * n);
    // cells with more than kBigCell points hold at least kBigCell + 1 of the n points each
    // (a filter of a few hundred thousand points is bound by its longest one-thread cells, a larger one by its gathers: measured)
    const uint32_t kBigCellMin = kBigCellEnv ? kBigCellEnv : (n <= (1u << 19) ? kBigCell / 2u : kBigCell);
    DM_RESERVE(dm->big, 16ull * (n / kBigCellMin + 1));   // {cell, first, end, -} per entry
    const uint32_t nchunk = n / kChunk;
    DM_RESERVE(dm->chunk_desc, 16ull * (nchunk + 1));
    if (kGridKeys)
        hipLaunchKernelGGL(dm_grid_centroids_keys, dim3(cdiv(n, 256) + cdiv(nchunk, 4)), dim3(256), 0, st, d_in, v1, seg_start, dm->d_cnt,
                           (int)kCntGridSegs, (int)kCntBig, (uint4 *)dm->big.ptr, (float *)out.ptr, cdiv(n, 256), (const uint32_t *)k1,
                           (int)kCntGridValid, nchunk, (uint4 *)dm->chunk_desc.ptr, kBigCellMin);
    else
        hipLaunchKernelGGL(dm_grid_centroids, dim3(cdiv(n, 256) + cdiv(nchunk, 4)), dim3(256), 0, st, d_in, v1, seg_start, dm->d_cnt,
                       (int)kCntGridSegs, (int)kCntBig, (uint4 *)dm->big.ptr, (float *)out.ptr, cdiv(n, 256), (const uint32_t *)flag,
                       (const uint32_t *)scan, (int)kCntGridValid, nchunk, (uint4 *)dm->chunk_desc.ptr, kBigCellMin);
    hipLaunchKernelGGL(dm_grid_centroids_big, dim3(kBigCellWgs), dim3(64), 0, st, d_in, v1, seg_start, dm->d_cnt, (int)kCntBig,
                       (const uint4 *)dm->big.ptr, (const uint4 *)dm->chunk_desc.ptr, (float *)out.ptr);
    rc = read_counters(dm);
    if (rc != LA3DM_OK) return rc;
    memcpy(dm->h_gp, dm->h_cnt + kCntGrid, sizeof(GridParams));
    if (dm->h_gp->passthrough) {  // index space overflows int32: PCL returns the cloud unfiltered
        DM_TRY(hipMemcpyAsync(out.ptr, d_in, 12ull * n, hipMemcpyDeviceToDevice, st));
        *n_out = n;
        return LA3DM_OK;
    }
    if (speculate && !dm->h_gp->empty) {
        // cells <= 2^bits - 1 keeps the all-ones key of a non-finite point behind every cell on `bits` key bits
        const uint64_t cells = (uint64_t)dm->h_gp->m2 * (uint64_t)dm->h_gp->span[2];
        int need = 1;
        while (need < 32 && ((1ull << need) - 1ull) < cells) ++need;
        const int need_digits = std::min(32, 8 * ((need + 7) / 8));
        dm->spec_bits = need_digits;
        if (need_digits > key_bits)   // too few digits were sorted: again, with the GridParams in place
            return voxel_grid(dm, d_in, n, leaf, out, n_out, 32, true);
    }
    *n_out = dm->h_cnt[kCntGridSegs];
    return LA3DM_OK;
}

static int grow_pool(la3dm_devmap *dm, size_t want_blocks) {
    if (want_blocks <= dm->cap_blocks) return LA3DM_OK;
    hipStream_t st = dm->ctx->stream;
    // a regrow copies the pool and synchronises: the first allocation leaves room for a few scans' worth of new blocks
    // (9 bytes per node: 164 k blocks of 73 nodes are 108 MB), later ones double
    // (node indices travel as 32-bit words — leaf_node, the write-back's slot * nodes-per-block: a pool ends at 2^32 nodes)
    const size_t cap_max = 0xFFFFFFFFull / dm->npb;
    if (want_blocks > cap_max) return dm_fail(dm, LA3DM_ERR_OOM, "devmap: the block pool would exceed 2^32 nodes");
    size_t cap = std::min(std::max<size_t>((dm->cap_blocks ? 2 : 4) * want_blocks, 4096), cap_max);
    float *A = nullptr, *B = nullptr;
    uint8_t *S = nullptr;
    long long *bk = nullptr;
    const size_t nn = cap * dm->npb;
    if (hipMalloc((void **)&A, 4 * nn) != hipSuccess || hipMalloc((void **)&B, 4 * nn) != hipSuccess ||
        hipMalloc((void **)&S, nn) != hipSuccess || hipMalloc((void **)&bk, 8 * cap) != hipSuccess) {
        if (A) (void)hipFree(A);
        if (B) (void)hipFree(B);
        if (S) (void)hipFree(S);
        if (bk) (void)hipFree(bk);
        return dm_fail(dm, LA3DM_ERR_OOM, "devmap: block pool allocation failed");
    }
    if (dm->n_blocks) {
        const size_t on = (size_t)dm->n_blocks * dm->npb;
        DM_TRY(hipMemcpyAsync(A, dm->A, 4 * on, hipMemcpyDeviceToDevice, st));
        DM_TRY(hipMemcpyAsync(B, dm->B, 4 * on, hipMemcpyDeviceToDevice, st));
        DM_TRY(hipMemcpyAsync(S, dm->S, on, hipMemcpyDeviceToDevice, st));
        DM_TRY(hipMemcpyAsync(bk, dm->blk_key, 8ull * dm->n_blocks, hipMemcpyDeviceToDevice, st));
        DM_TRY(hipStreamSynchronize(st));
    }
    if (dm->A) (void)hipFree(dm->A);
    if (dm->B) (void)hipFree(dm->B);
    if (dm->S) (void)hipFree(dm->S);
    if (dm->blk_key) (void)hipFree(dm->blk_key);
    dm->A = A;
    dm->B = B;
    dm->S = S;
    dm->blk_key = bk;
    dm->cap_blocks = cap;
    return LA3DM_OK;
}

// the block table (tab_key, tab_val; `cap` entries) built again from the keys of pool slots 0 .. n_blocks - 1
static int table_rebuild(la3dm_devmap *dm, long long *tab_key, uint32_t *tab_val, uint32_t cap, uint32_t n_blocks) {
    hipStream_t st = dm->ctx->stream;
    DM_TRY(hipMemsetAsync(tab_key, 0xFF, 8ull * cap, st));
    if (n_blocks) {
        hipLaunchKernelGGL(dm_table_rebuild, dim3(cdiv(n_blocks, 256)), dim3(256), 0, st, dm->blk_key, n_blocks, tab_key, tab_val, cap - 1);
        DM_TRY(hipGetLastError());
    }
    return LA3DM_OK;
}

// the pool as a kernel's argument (devmap_pool.h)
static PoolView pool_view(const la3dm_devmap *dm) {
    return PoolView{dm->tab_key, dm->tab_val, dm->tab_cap - 1, dm->A, dm->B, dm->S, dm->npb, dm->depth, dm->init_A, dm->init_B};
}

static int grow_table(la3dm_devmap *dm, size_t want_blocks) {
    if (dm->tab_cap >= 2 * want_blocks && dm->tab_cap) return LA3DM_OK;
    hipStream_t st = dm->ctx->stream;
    uint32_t cap = 1u << 16;
    while (cap < 4 * want_blocks) cap <<= 1;
    long long *tk = nullptr;
    uint32_t *tv = nullptr;
    if (hipMalloc((void **)&tk, 8ull * cap) != hipSuccess || hipMalloc((void **)&tv, 4ull * cap) != hipSuccess) {
        if (tk) (void)hipFree(tk);
        return dm_fail(dm, LA3DM_ERR_OOM, "devmap: block table allocation failed");
    }
    int rc = table_rebuild(dm, tk, tv, cap, dm->n_blocks);   // (into the new arrays, installed below)
    if (rc != LA3DM_OK) return rc;
    DM_TRY(hipStreamSynchronize(st));
    if (dm->tab_key) (void)hipFree(dm->tab_key);
    if (dm->tab_val) (void)hipFree(dm->tab_val);
    dm->tab_key = tk;
    dm->tab_val = tv;
    dm->tab_cap = cap;
    return LA3DM_OK;
}

// float-stepped candidate indices of one axis (get_blocks_in_bbox, bgkoctomap.cpp:486-495): the three nested
// loops restart the inner sequences identically, so the candidate list is the product of three sequences.
static std::vector<int> axis_sequence(float lo, float hi, float bs) {
    std::vector<int> seq;
    for (float v = lo - bs; v <= hi + 2 * bs; v += bs) {
        seq.push_back((int)(int64_t)((double)v / (double)bs + 524288.5));
        if (seq.size() > (1u << 20)) break;
    }
    return seq;
}

extern "C" {

int la3dm_devmap_create(la3dm_ctx *ctx, la3dm_devmap **out) {
    if (!ctx || !out) return LA3DM_ERR_ARG;
    *out = nullptr;
    if (ctx->p.variant < 0 || ctx->p.variant > 3) {
        ctx->err = "la3dm_devmap_create: the device-resident map supports variant 0 (BGK), 1 (GP), 2 (BGK-LV) and 3 (BGK-L)";
        return LA3DM_ERR_ARG;
    }
    if (ctx->p.block_depth > 5) {  // dm_prune stages 3 bytes per node of a block in LDS
        ctx->err = "la3dm_devmap_create: the device-resident map supports block_depth <= 5";
        return LA3DM_ERR_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    la3dm_devmap *dm = new la3dm_devmap;
    dm->ctx = ctx;
    if (const char *ev = getenv("LA3DM_INJECT_FRONT_END_FAILURE")) dm->dbg_fail_rank = atoi(ev);   // test hooks, read once
    if (const char *ev = getenv("LA3DM_INJECT_SLAB_FAILURE")) dm->dbg_fail_slab_rank = atoi(ev);
    if (const char *ev = getenv("LA3DM_INJECT_SCAN_STUCK")) dm->dbg_stuck_at = atoi(ev);
    ctx->n_devmaps++;   // (la3dm_devmap_destroy, also the failure paths' clean-up, counts it down)
    dm->depth = (uint32_t)ctx->p.block_depth;
    dm->npb = npb_of(ctx->p.block_depth);
    dm->ncell = 1u << (3 * (dm->depth - 1));
    dm->block_size = (float)pow(2, ctx->p.block_depth - 1) * ctx->p.resolution;  // bgkoctomap.cpp:36
    if (ctx->p.variant == 1) {  // GP nodes start at (0, min_ivar), gpoctree_node.cpp:15-17
        dm->init_A = 0.0f;
        dm->init_B = ctx->p.min_ivar;
    } else {
        dm->init_A = ctx->p.prior_A;
        dm->init_B = ctx->p.prior_B;
    }
    memset(&dm->stats, 0, sizeof(dm->stats));
    dm->stage_timing = getenv("LA3DM_TIMING") != nullptr;
    {
        const char *mb = getenv("LA3DM_MAILBOX");
        dm->mailbox = !(mb && mb[0] == '0');
        const char *os = getenv("LA3DM_OWN_SORT");
        dm->own_sort = !(os && os[0] == '0');
        const char *ts = getenv("LA3DM_TEST_SORT");
        dm->test_sort = !(ts && ts[0] == '0');
    }
    bool ok = hipMalloc((void **)&dm->d_cnt, sizeof(uint32_t) * kCntWords) == hipSuccess &&
              // the mailbox: coherent (the in-kernel publish must be visible while the kernel still runs, whatever
              // HIP_HOST_COHERENT says), mapped, and cleared — the first wait is for sequence number 1
              hipHostMalloc((void **)&dm->h_cnt, sizeof(uint32_t) * (kCntWords + 2), hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess &&
              (memset(dm->h_cnt, 0, sizeof(uint32_t) * (kCntWords + 2)), true) &&
              hipMalloc((void **)&dm->d_mm, sizeof(uint32_t) * kMmWords) == hipSuccess &&
              hipMalloc((void **)&dm->d_bbox, sizeof(float) * 8) == hipSuccess &&
              hipHostMalloc((void **)&dm->h_bbox, sizeof(float) * 8) == hipSuccess &&
              hipMalloc((void **)&dm->d_gp, sizeof(GridParams)) == hipSuccess &&
              hipHostMalloc((void **)&dm->h_gp, sizeof(GridParams)) == hipSuccess &&
              hipMemset(dm->d_cnt, 0, sizeof(uint32_t) * kCntWords) == hipSuccess &&
              (ctx->p.variant != 2 || (hipMalloc((void **)&dm->d_lvmm, 32) == hipSuccess && hipHostMalloc((void **)&dm->h_lvmm, 32) == hipSuccess));
    if (!ok) {
        ctx->err = "la3dm_devmap_create: allocation failed";
        la3dm_devmap_destroy(dm);
        return LA3DM_ERR_OOM;
    }
    {
        // The single-launch scan and the radix passes hand tiles to at most as many workgroups as the chip holds at once
        // (a workgroup waits for tiles of workgroups that started before it): the bound comes from the occupancy of the
        // kernels as compiled, not from a constant that a change of their register count would silently falsify.
        int cus = 0, b0 = 0, b1 = 0, b3 = 0, b4 = 0;   // (hipGetDeviceProperties would cost tens of ms here)
        ok = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && cus > 0 &&
             hipOccupancyMaxActiveBlocksPerMultiprocessor(&b0, dm_scan_lb<false>, (int)kScanThreads, 0) == hipSuccess &&
             hipOccupancyMaxActiveBlocksPerMultiprocessor(&b1, dm_scan_lb<true>, (int)kScanThreads, 0) == hipSuccess &&
             hipOccupancyMaxActiveBlocksPerMultiprocessor(&b3, dm_radix_pass<1024, 4>, 1024, 0) == hipSuccess &&
             hipOccupancyMaxActiveBlocksPerMultiprocessor(&b4, dm_radix_pass<1024, 8>, 1024, 0) == hipSuccess && b0 > 0 && b1 > 0 && b3 > 0 && b4 > 0;
        if (!ok) {
            ctx->err = "la3dm_devmap_create: occupancy query failed";
            la3dm_devmap_destroy(dm);
            return LA3DM_ERR_HIP;
        }
        dm->scan_resident = std::min<uint32_t>(kScanResident, (uint32_t)std::min(b0, b1) * (uint32_t)cus);
        dm->radix_resident_big = (uint32_t)cus;
        dm->radix_resident_wide = (uint32_t)cus;   // (one sixteen-wave workgroup per CU, whatever the occupancy allows: the shape is for tile latency)
        // test hook: a handful of workgroups per launch forces the multi-round (ticket) form of the scan / sort on small inputs
        if (const char *ev = getenv("LA3DM_SCAN_RESIDENT")) dm->scan_resident = std::max(1, std::min<int>(atoi(ev), (int)dm->scan_resident));
        if (const char *ev = getenv("LA3DM_RADIX_RESIDENT")) {
            const uint32_t cap = (uint32_t)std::max(1, atoi(ev));
            dm->radix_resident_wide = std::min(dm->radix_resident_wide, cap);
            dm->radix_resident_big = std::min(dm->radix_resident_big, cap);
        }
        if (const char *ev = getenv("LA3DM_RADIX_WIDE")) dm->radix_resident_wide = (uint32_t)std::max(0, atoi(ev));   // (A/B: 0 = 8192-item tiles only)
    }
    *out = dm;
    return LA3DM_OK;
}

void la3dm_devmap_destroy(la3dm_devmap *dm) {
    if (!dm) return;
    dm->ctx->n_devmaps--;
    (void)hipSetDevice(dm->ctx->device);
    Arena *all[] = {&dm->cloud, &dm->hits, &dm->keep, &dm->nfree, &dm->keep_off, &dm->free_off, &dm->frees_raw, &dm->frees_ds,
                    &dm->xy, &dm->k0, &dm->k1, &dm->v0, &dm->v1, &dm->flag, &dm->scan, &dm->seg_start, &dm->seg_key,
                    &dm->cub_tmp, &dm->scan_status, &dm->radix_state, &dm->radix_tmp, &dm->big, &dm->chunk_desc, &dm->train, &dm->grid, &dm->axis_tab, &dm->m_code, &dm->q_out, &dm->df_work, &dm->fr_work, &dm->ft_work, &dm->sf_work, &dm->gain_work, &dm->score_work, &dm->nt_work, &dm->reach_work, &dm->travel_work, &dm->drive_work, &dm->clusters_work, &dm->clusters_rec, &dm->pack_stream, &dm->pack_counts, &dm->c_flag, &dm->c_weight, &dm->c_scan, &dm->t_key0,
                    &dm->t_key1, &dm->t_ent0, &dm->t_ent1, &dm->t_blockkey, &dm->t_center, &dm->t_nbr, &dm->t_slot, &dm->t_slot0, &dm->nleaf,
                    &dm->leaf_off, &dm->leaf_key, &dm->leaf_alpha, &dm->leaf_beta, &dm->leaf_state, &dm->leaf_node,
                    &dm->l_ray_idx, &dm->l_rays, &dm->l_rows, &dm->l_rows_off, &dm->l_rflag, &dm->l_rscan,
                    &dm->shard_w, &dm->shard_cumw, &dm->shard_bounds, &dm->shard_hist, &dm->shard_nown, &dm->shard_own_off, &dm->shard_cnt, &dm->shard_frees,
                    &dm->lv_rng, &dm->lv_flags, &dm->lv_seg, &dm->lv_nsamp, &dm->lv_nray, &dm->lv_samp_off, &dm->lv_ray_off, &dm->lv_samples,
                    &dm->lv_rays, &dm->lv_sorted, &dm->lv_cell_off, &dm->lv_axis, &dm->lv_keys, &dm->lv_mult, &dm->lv_flag, &dm->lv_pos,
                    &dm->lv_slot, &dm->lv_center, &dm->lv_cell0, &dm->lv_pslot, &dm->lv_pmult, &dm->lv_info, &dm->lv_prune, &dm->lv_beam, &dm->lv_mask};
    for (Arena *a : all)
        if (a->ptr) (void)hipFree(a->ptr);
    if (dm->h_shard) (void)hipHostFree(dm->h_shard);
    if (dm->d_lvmm) (void)hipFree(dm->d_lvmm);
    if (dm->h_lvmm) (void)hipHostFree(dm->h_lvmm);
    void *dev[] = {dm->A, dm->B, dm->S, dm->blk_key, dm->tab_key, dm->tab_val, dm->d_cnt, dm->d_mm, dm->d_bbox, dm->d_gp};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    if (dm->h_cnt) (void)hipHostFree(dm->h_cnt);
    if (dm->h_bbox) (void)hipHostFree(dm->h_bbox);
    if (dm->h_gp) (void)hipHostFree(dm->h_gp);
    delete dm;
}

// bbox of the training set in dm->xy (bbox(), bgkoctomap.cpp:464-484) -> dm->h_bbox; get_blocks_in_bbox walks it on
// the host.  One synchronisation.
static int training_bbox(la3dm_devmap *dm, bool reduced = false) {
    hipStream_t st = dm->ctx->stream;
    const uint32_t npts = dm->n_xy;
    if (!reduced) {   // (the front end's own kernels may have reduced the box while writing the set)
        MinmaxFin fin = {2, 0.0f, nullptr, (const float *)dm->xy.ptr, dm->d_cnt, dm->d_mm + 6, nullptr};
        publish_with(dm, fin.mailbox, fin.mailbox_seq);
        hipLaunchKernelGGL(dm_minmax<4>, dim3(std::min<uint32_t>(cdiv(npts, 1024), kMinmaxWgs)), dim3(256), 0, st, (const float *)dm->xy.ptr,
                           npts, dm->d_mm, fin);
    }
    int rc = read_counters(dm);   // the box comes back with the counter block
    if (rc != LA3DM_OK) return rc;
    memcpy(dm->h_bbox, dm->h_cnt + kCntBbox, sizeof(float) * 6);
    return LA3DM_OK;
}

// Sharded sample filter: cut[q] = first layer of rank q (q = 0..world), contiguous ranges whose sample counts cross
// q / world of the total (mirrored by la3dm_amd/sharding.py layer_cuts for the CPU test).
static void shard_layer_cuts(const uint32_t *hist, uint32_t nlayer, uint32_t world, std::vector<uint32_t> &cut) {
    uint64_t total = 0;
    for (uint32_t j = 0; j < nlayer; ++j) total += hist[j];
    cut.assign(world + 1, nlayer);
    cut[0] = 0;
    uint64_t run = 0;
    uint32_t q = 1;
    for (uint32_t j = 0; j < nlayer && q < world; ++j) {
        // layer j starts at running count `run`: it opens rank q's range when the count has reached q / world of the total
        while (q < world && run * world >= total * q) cut[q++] = j;
        run += hist[j];
    }
    while (q < world) cut[q++] = nlayer;
}

// What the rank-local part of the front end leaves for its tail (and, in a sharded map, for the exchange in between).
struct FrontState {
    enum { kDone, kFilteredLocally, kShardedFilter } path = kDone;  // kDone: finished (no training set, or BGK-L's own path)
    uint32_t n_kept = 0, n_f = 0, n_f_own = 0;
    const float *d_frees = nullptr;
    float4 *xy = nullptr;
    uint32_t *mm_hits = nullptr;
};
// status word of a rank in the sharded front end's count exchange (values above any sample count)
constexpr uint32_t kShardStatusFailed = 0xFFFFFFFFu;    // a rank-local error: every rank gives the insert up
constexpr uint32_t kShardStatusNoFilter = 0xFFFFFFFEu;  // this insert does not shard its sample filter (decided alike everywhere)

// f1 (bgkoctomap.cpp:383-458): voxel grid over the hits, range gate + beam samples, voxel grid over the free samples;
// leaves the labelled training set in dm->xy (hits first), its size in dm->n_xy, and the scan's bbox in dm->h_bbox.
// front_end_local: everything a rank does on its own, up to (sharded map) its share of the filtered samples.
static int front_end_local(la3dm_devmap *dm, const float *d_xyz, uint32_t n, const float origin[3], float ds_resolution,
                           float free_resolution, float max_range, FrontState &F) {
    la3dm_ctx *ctx = dm->ctx;
    hipStream_t st = ctx->stream;
    la3dm_devmap_stats &S = dm->stats;
    int rc;
    // test hook (tests/test_sharded_insert_gpu.py): rank dbg_fail_rank of a sharded map fails here.  The environment variable is
    // read ONCE, when the map is created (not on every insert of the production path)
    if (dm->dbg_fail_rank >= 0 && dm->shard_world > 1 && dm->dbg_fail_rank == (int)dm->shard_rank)
        return dm_fail(dm, LA3DM_ERR_OOM, "devmap: injected rank-local front-end failure (LA3DM_INJECT_FRONT_END_FAILURE)");
    const float *d_hits = d_xyz;
    uint32_t n_h = n;
    int free_key_bits = 32;
    if (!(ds_resolution < 0)) {
        if ((rc = voxel_grid(dm, d_xyz, n, ds_resolution, dm->hits, &n_h)) != LA3DM_OK) return rc;
        d_hits = (const float *)dm->hits.ptr;
        // The free samples lie between the origin and a (downsampled) hit, i.e. inside the box of the raw hits and
        // the origin, give or take an ulp: their grid has at most (that box + one cell on every side) cells, which
        // bounds the significant bits of their sort keys (one Onesweep pass per 8 bits).
        const GridParams &g = *dm->h_gp;
        if (!g.passthrough && !g.empty) {
            const float inv = 1.0f / ds_resolution;
            double cells = 1.0;
            for (int a = 0; a < 3; ++a) {
                const double oc = floor((double)origin[a] * (double)inv);
                const double lo = std::min((double)g.lo[a], oc) - 1.0, hi = std::max((double)g.lo[a] + g.span[a] - 1.0, oc) + 1.0;
                cells *= hi - lo + 1.0;
            }
            int b = 1;
            while (b < 32 && (double)((1ull << b) - 1ull) < cells) ++b;
            free_key_bits = b;
        }
    }
    if (n_h == 0) return LA3DM_OK;
    DM_RESERVE(dm->keep, 4ull * n_h);
    DM_RESERVE(dm->nfree, 4ull * n_h);
    DM_RESERVE(dm->keep_off, 4ull * n_h);
    DM_RESERVE(dm->free_off, 4ull * n_h);
    BeamArgs ba = {origin[0], origin[1], origin[2], free_resolution, max_range};
    uint32_t *keep = (uint32_t *)dm->keep.ptr, *nfree = (uint32_t *)dm->nfree.ptr, *keep_off = (uint32_t *)dm->keep_off.ptr,
             *free_off = (uint32_t *)dm->free_off.ptr;
    if (ctx->p.variant == 3) {  // BGKLOctoMap: samples keep their beam, no second voxel filter
        hipLaunchKernelGGL(dm_l_beam_count, dim3(std::min<uint32_t>(cdiv(n_h, 256), kBeamCountWgs)), dim3(256), 0, st, d_hits, n_h, ba, keep, nfree, dm->d_cnt);
        if ((rc = exclusive_scan(dm, keep, keep_off, n_h, (int)kCntKept)) != LA3DM_OK) return rc;
        if ((rc = exclusive_scan(dm, nfree, free_off, n_h, (int)kCntFreeRaw, true)) != LA3DM_OK) return rc;
        if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
        if ((rc = check_beam_counters(dm)) != LA3DM_OK) return rc;
        const uint32_t n_beams = dm->h_cnt[kCntKept], n_samples = dm->h_cnt[kCntFreeRaw];
        if (n_beams == 0) return LA3DM_OK;
        DM_RESERVE(dm->xy, 16ull * n_samples);
        DM_RESERVE(dm->l_ray_idx, 4ull * n_samples);
        DM_RESERVE(dm->l_rays, 24ull * n_beams);
        hipLaunchKernelGGL(dm_l_beam_write, dim3(cdiv(n_h, 256)), dim3(256), 0, st, d_hits, n_h, ba, keep, keep_off, free_off,
                           (float4 *)dm->xy.ptr, (int32_t *)dm->l_ray_idx.ptr, (float *)dm->l_rays.ptr);
        dm->n_xy = n_samples;
        S.n_hits = n_beams;
        S.n_frees = n_samples - n_beams;
        return training_bbox(dm);
    }
    hipLaunchKernelGGL(dm_beam_count, dim3(std::min<uint32_t>(cdiv(n_h, 256), kBeamCountWgs)), dim3(256), 0, st, d_hits, n_h, ba, keep, nfree, dm->d_cnt);
    if ((rc = exclusive_scan(dm, keep, keep_off, n_h, (int)kCntKept)) != LA3DM_OK) return rc;
    if ((rc = exclusive_scan(dm, nfree, free_off, n_h, (int)kCntFreeRaw, true)) != LA3DM_OK) return rc;
    if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
    if ((rc = check_beam_counters(dm)) != LA3DM_OK) return rc;
    const uint32_t n_kept = dm->h_cnt[kCntKept], n_free_raw = dm->h_cnt[kCntFreeRaw];
    if (n_kept == 0) return LA3DM_OK;
    DM_RESERVE(dm->xy, 16ull * ((size_t)n_kept + n_free_raw));
    float4 *xy = (float4 *)dm->xy.ptr;
    // the beam kernel also reduces the box of the free samples (-> GridParams of the second voxel filter, finished by its
    // last workgroup) and the box of the kept hits (d_mm[8..13]); dm_append_frees then completes the training set's box
    uint32_t *mm_hits = dm->d_mm + 8;
    const float *d_frees = nullptr;
    uint32_t n_f = 0;
    // Block-sharded insert: the samples' voxel filter is divided over the ranks by z-layer of its grid (devmap_kernels.h,
    // "sharded sample filter"); every rank ends up with the same filtered list, in the single-GPU order.
    const GridParams &g1 = *dm->h_gp;   // (grid of the cloud's own filter: the box of the raw hits)
    if (dm->shard_world > 1 && ctx->opt_grid_order == 1 && !(ds_resolution < 0))
        return dm_fail(dm, LA3DM_ERR_ARG, "devmap: option grid_order 1 (pcl::VoxelGrid's own sort, a verification mode) runs on one GPU only");
    bool sharded_filter = dm->shard_world > 1 && !(ds_resolution < 0) && !g1.passthrough && !g1.empty;
    int zbase = 0;
    uint32_t nlayer = 0;
    if (sharded_filter) {
        // every sample lies between the origin and a filtered hit (a centroid of raw hits): its layer is inside
        // [min(origin, box) - 1, max(origin, box) + 1]
        const float inv = 1.0f / ds_resolution;
        const double oz = floor((double)origin[2] * (double)inv);
        const double lo = std::min((double)g1.lo[2], oz) - 1.0, hi = std::max((double)g1.lo[2] + g1.span[2] - 1.0, oz) + 1.0;
        if (hi - lo + 1.0 > (double)kShardLayers || fabs(lo) > 1e9 || fabs(hi) > 1e9) sharded_filter = false;   // (a very tall scan: unsharded filter)
        else {
            zbase = (int)lo;
            nlayer = (uint32_t)(hi - lo + 1.0);
        }
    }
    if (!sharded_filter) {
        DM_RESERVE(dm->frees_raw, 12ull * n_free_raw);
        {
            MinmaxFin fin = {1, ds_resolution < 0 ? 1.0f : 1.0f / ds_resolution, dm->d_gp, nullptr, dm->d_cnt, dm->d_mm + 6, nullptr};
            hipLaunchKernelGGL(dm_beam_write<false>, dim3(std::min<uint32_t>(cdiv(n_h, 256), beam_wgs(n_h))), dim3(256), 0, st, d_hits, n_h, ba, keep,
                               keep_off, free_off, xy, (float *)dm->frees_raw.ptr, dm->d_mm, fin, mm_hits, 0.0f, 0, 0);
        }
        d_frees = (const float *)dm->frees_raw.ptr;
        n_f = n_free_raw;
        if (!(ds_resolution < 0)) {
            if ((rc = voxel_grid(dm, d_frees, n_free_raw, ds_resolution, dm->frees_ds, &n_f, free_key_bits, true)) != LA3DM_OK) return rc;
            d_frees = (const float *)dm->frees_ds.ptr;
        }
    } else {
        const float inv = 1.0f / ds_resolution;
        const uint32_t world = dm->shard_world, rank = dm->shard_rank;
        // 1. samples per layer -> contiguous layer ranges of equal sample count
        DM_RESERVE(dm->shard_hist, 4ull * kShardLayers);
        DM_TRY(hipMemsetAsync(dm->shard_hist.ptr, 0, 4ull * nlayer, st));
        hipLaunchKernelGGL(dm_beam_hist, dim3(std::min<uint32_t>(cdiv(n_h, 256), kMinmaxWgs)), dim3(256), 0, st, d_hits, n_h, ba, keep, inv, zbase,
                           nlayer, (uint32_t *)dm->shard_hist.ptr, dm->d_cnt);
        dm->shard_hist_host.resize(nlayer);
        DM_TRY(hipMemcpyAsync(dm->shard_hist_host.data(), dm->shard_hist.ptr, 4ull * nlayer, hipMemcpyDeviceToHost, st));
        DM_TRY(hipStreamSynchronize(st));
        std::vector<uint32_t> cut;
        shard_layer_cuts(dm->shard_hist_host.data(), nlayer, world, cut);   // [world + 1] layer indices relative to zbase
        const int lo = zbase + (int)cut[rank], hi = zbase + (int)cut[rank + 1];
        if (getenv("LA3DM_DEBUG_SHARD"))
            fprintf(stderr, "la3dm sharded sample filter: rank %u of %u takes layers [%d, %d) of [%d, %d), %u raw samples in all\n", rank, world,
                    lo, hi, zbase, zbase + (int)nlayer, n_free_raw);
        // 2. own samples per beam -> offsets, total
        DM_RESERVE(dm->shard_nown, 4ull * n_h);
        DM_RESERVE(dm->shard_own_off, 4ull * n_h);
        uint32_t *nown = (uint32_t *)dm->shard_nown.ptr, *own_off = (uint32_t *)dm->shard_own_off.ptr;
        hipLaunchKernelGGL(dm_beam_count_own, dim3(cdiv(n_h, 256)), dim3(256), 0, st, d_hits, n_h, ba, keep, inv, lo, hi, nown);
        if ((rc = exclusive_scan(dm, nown, own_off, n_h, (int)kCntFreeRaw, true)) != LA3DM_OK) return rc;
        if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
        const uint32_t n_own = dm->h_cnt[kCntFreeRaw];
        // 3. kept hits -> xy, own samples -> frees_raw, the box of ALL samples -> the filter grid's (global) parameters
        DM_RESERVE(dm->frees_raw, 12ull * (n_own ? n_own : 1));
        DM_RESERVE(dm->shard_frees, 12ull * (n_free_raw ? n_free_raw : 1));  // the gathered list (<= every raw sample): sized HERE, so that a
                                                                             // rank that cannot hold it fails before the exchange, not inside it
        {
            MinmaxFin fin = {1, inv, dm->d_gp, nullptr, dm->d_cnt, dm->d_mm + 6, nullptr};
            hipLaunchKernelGGL(dm_beam_write<true>, dim3(std::min<uint32_t>(cdiv(n_h, 256), beam_wgs(n_h))), dim3(256), 0, st, d_hits, n_h, ba, keep,
                               keep_off, own_off, xy, (float *)dm->frees_raw.ptr, dm->d_mm, fin, mm_hits, inv, lo, hi);
        }
        // 4. this rank's cells.  (The grid's parameters come back with the filter's counters; a rank without samples fetches
        //    them on its own: whether the grid overflows int32 — PCL then returns its input unfiltered, which the layer
        //    split cannot reproduce — must be decided identically everywhere BEFORE the first collective.)
        uint32_t n_f_own = 0;
        if (n_own) {
            if ((rc = voxel_grid(dm, (const float *)dm->frees_raw.ptr, n_own, ds_resolution, dm->frees_ds, &n_f_own, free_key_bits, true)) != LA3DM_OK)
                return rc;
        } else {
            if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
            memcpy(dm->h_gp, dm->h_cnt + kCntGrid, sizeof(GridParams));
        }
        if (dm->h_gp->passthrough)
            return dm_fail(dm, LA3DM_ERR_ARG, "devmap: sharded insert: the samples' filter grid overflows int32 (PCL passes the cloud through); use one GPU");
        F.path = FrontState::kShardedFilter;
        F.n_kept = n_kept;
        F.n_f_own = n_f_own;
        F.xy = xy;
        F.mm_hits = mm_hits;
        return LA3DM_OK;
    }
    F.path = FrontState::kFilteredLocally;
    F.n_kept = n_kept;
    F.n_f = n_f;
    F.d_frees = d_frees;
    F.xy = xy;
    F.mm_hits = mm_hits;
    return LA3DM_OK;
}

static int front_end(la3dm_devmap *dm, const float *d_xyz, uint32_t n, const float origin[3], float ds_resolution,
                     float free_resolution, float max_range) {
    la3dm_ctx *ctx = dm->ctx;
    hipStream_t st = ctx->stream;
    la3dm_devmap_stats &S = dm->stats;
    FrontState F;
    // sharded map: this rank's slot of the status exchange reads "failed" from here until the local part has succeeded
    if (dm->shard_world > 1 && dm->shard_fn)
        (void)hipMemcpyAsync((uint32_t *)dm->shard_cnt.ptr + dm->shard_rank, &dm->shard_status_failed, 4, hipMemcpyHostToDevice, st);
    const int lrc = front_end_local(dm, d_xyz, n, origin, ds_resolution, free_resolution, max_range, F);
    if (dm->shard_world > 1 && dm->shard_fn) {
        // Sharded map: ONE status / count exchange per insert, entered by every rank whatever happened to it — a rank
        // that failed on its own (out of memory, a scan that tripped, ...) posts kShardStatusFailed and all ranks give
        // the insert up together instead of its peers waiting in a collective it never enters; an insert
        // that does not shard its filter (no voxel grid, a grid that overflows, a very tall scan, nothing to train on)
        // posts kShardStatusNoFilter.  4 bytes per rank.
        const uint32_t world = dm->shard_world, rank = dm->shard_rank;
        uint32_t status = lrc != LA3DM_OK ? kShardStatusFailed : F.path == FrontState::kShardedFilter ? F.n_f_own : kShardStatusNoFilter;
        const std::string local_err = ctx->err;
        // the exchange buffer exists since la3dm_devmap_set_shard, and this rank's slot reads "failed" (preset above, before the
        // local part) until the copy below has replaced it: a rank that cannot even stage its word is seen as failed by its peers instead of handing them a stale
        // count of the insert before
        int xrc = LA3DM_OK;
        if (hipMemcpyAsync((uint32_t *)dm->shard_cnt.ptr + rank, &status, 4, hipMemcpyHostToDevice, st) != hipSuccess) xrc = LA3DM_ERR_HIP;
        dm->shard_off[0].resize(world);
        dm->shard_bytes[0].resize(world);
        for (uint32_t q = 0; q < world; ++q) {
            dm->shard_off[0][q] = 4ull * q;
            dm->shard_bytes[0][q] = 4;
        }
        la3dm_gather_seg seg = {dm->shard_cnt.ptr, dm->shard_off[0].data(), dm->shard_bytes[0].data()};
        const int cbrc = dm->shard_fn(dm->shard_user, &seg, 1, world, rank, (void *)st);
        if (cbrc != 0 && lrc == LA3DM_OK)   // (a rank that had failed on its own keeps its own error)
            return dm_fail(dm, LA3DM_ERR_ARG, "devmap: the all-gather callback of the sharded insert failed (sample counts)");
        if (lrc != LA3DM_OK) {
            ctx->err = local_err;
            return lrc;
        }
        if (xrc != LA3DM_OK) return dm_fail(dm, xrc, "devmap: sharded insert: could not stage the status word");
        dm->shard_cnt_host.resize(world);
        DM_TRY(hipMemcpyAsync(dm->shard_cnt_host.data(), dm->shard_cnt.ptr, 4ull * world, hipMemcpyDeviceToHost, st));
        DM_TRY(hipStreamSynchronize(st));
        for (uint32_t q = 0; q < world; ++q)
            if (dm->shard_cnt_host[q] == kShardStatusFailed)
                return dm_fail(dm, LA3DM_ERR_PEER, "devmap: sharded insert: rank " + std::to_string(q) + " failed in its front end; the insert is given up on every rank");
        for (uint32_t q = 0; q < world; ++q)
            if ((dm->shard_cnt_host[q] == kShardStatusNoFilter) != (status == kShardStatusNoFilter))
                return dm_fail(dm, LA3DM_ERR_HIP, "devmap: sharded insert: the ranks disagree on whether this insert shards its sample filter");
    } else if (lrc != LA3DM_OK) {
        return lrc;
    }
    if (F.path == FrontState::kDone) return LA3DM_OK;
    const uint32_t n_kept = F.n_kept;
    float4 *xy = F.xy;
    uint32_t *mm_hits = F.mm_hits;
    const float *d_frees = F.d_frees;
    uint32_t n_f = F.n_f;
    if (F.path == FrontState::kShardedFilter) {
        // all-gather-v of the filtered points behind the count exchange above: every rank gets the whole list, rank
        // order = ascending cell index = the single-GPU order
        const uint32_t world = dm->shard_world, rank = dm->shard_rank, n_f_own = F.n_f_own;
        uint64_t total = 0, mine_at = 0;
        for (uint32_t q = 0; q < world; ++q) {
            if (q == rank) mine_at = total;
            dm->shard_off[0][q] = 12ull * total;
            dm->shard_bytes[0][q] = 12ull * dm->shard_cnt_host[q];
            total += dm->shard_cnt_host[q];
        }
        if (dm->shard_cnt_host[rank] != n_f_own || total > 0xFFFFFFF0ull)
            return dm_fail(dm, LA3DM_ERR_HIP, "devmap: sharded sample filter: inconsistent counts after the exchange");
        n_f = (uint32_t)total;
        if (n_f) {
            // (dm->shard_frees was sized for every raw sample by the local part: a rank that cannot hold the list has
            //  already said so in its status word)
            if (n_f_own)
                hipLaunchKernelGGL(dm_copy_f3, dim3(cdiv(3 * n_f_own, 256)), dim3(256), 0, st, (const float *)dm->frees_ds.ptr, 3 * n_f_own,
                                   (float *)dm->shard_frees.ptr + 3 * mine_at);
            la3dm_gather_seg seg2 = {dm->shard_frees.ptr, dm->shard_off[0].data(), dm->shard_bytes[0].data()};
            if (dm->shard_fn(dm->shard_user, &seg2, 1, world, rank, (void *)st) != 0)
                return dm_fail(dm, LA3DM_ERR_ARG, "devmap: the all-gather callback of the sharded insert failed (filtered samples)");
        }
        d_frees = (const float *)dm->shard_frees.ptr;
    }
    const float free_label = ctx->p.variant == 1 ? -1.0f : 0.0f;  // bgkoctomap.cpp:415 / gpoctomap.cpp:399
    bool box_reduced = false;
    if (n_f) {
        MinmaxFin fin = {2, 0.0f, nullptr, (const float *)xy, dm->d_cnt, dm->d_mm + 6, mm_hits};
        publish_with(dm, fin.mailbox, fin.mailbox_seq);   // training_bbox only waits
        hipLaunchKernelGGL(dm_append_frees, dim3(std::min<uint32_t>(cdiv(n_f, 256), kMinmaxWgs)), dim3(256), 0, st, d_frees, n_f, n_kept, free_label,
                           xy, dm->d_mm, fin);
        box_reduced = true;
    }
    const uint32_t npts = n_kept + n_f;
    dm->n_xy = npts;
    S.n_hits = n_kept;
    S.n_frees = n_f;

    return training_bbox(dm, box_reduced);
}

// Host-side facts of the scan in flight, shared by the partition and the passes.
struct ScanPlan {
    PartArgs pa;
    CandArgs ca;
    uint64_t ncid = 0;       // cells of the dense block-index grid
    uint32_t n_entries = 0;  // candidate list (product of the three axis sequences)
    uint32_t max_occ = 1;    // passes: how often the most repeated candidate key occurs
    uint32_t n_mem = 0;      // (block, point) membership pairs = gathered training rows
    uint32_t n_geo = 0;      // training blocks
    uint32_t *train_off = nullptr;
    uint32_t *rows_off = nullptr;  // BGKLOctoMap: CSR of the training rows over the training blocks
    uint32_t flags = 0;      // la3dm_bgk_scan.flags of the passes (LA3DM_SCAN_UPDATE_UNGATED for insert_training_data)
    bool slab = false;       // sharded, single pass: the CSR is built per rank, for its own x-slab, inside the pass (build_slab_csr)
    int cell_bits = 0;       // key bits of a grid cell index
};

// f2 (bgkoctomap.cpp:234-284, 486-552): candidate sequences of get_blocks_in_bbox, closed-box membership of every
// training point, CSR by block, dense block-index grid.
static int partition(la3dm_devmap *dm, ScanPlan &P) {
    la3dm_ctx *ctx = dm->ctx;
    hipStream_t st = ctx->stream;
    la3dm_devmap_stats &S = dm->stats;
    const uint32_t npts = dm->n_xy;
    const float4 *xy = (const float4 *)dm->xy.ptr;
    int rc;
    const float bs = dm->block_size, half = bs / 2.0f;
    std::vector<int> seq[3];
    int smin[3], smax[3];
    for (int a = 0; a < 3; ++a) {
        seq[a] = axis_sequence(dm->h_bbox[a], dm->h_bbox[3 + a], bs);
        if (seq[a].empty() || seq[a].size() > (1u << 20)) return dm_fail(dm, LA3DM_ERR_ARG, "devmap: degenerate training-set extent");
        smin[a] = smax[a] = seq[a][0];
        for (int v : seq[a]) {
            smin[a] = std::min(smin[a], v);
            smax[a] = std::max(smax[a], v);
        }
    }
    PartArgs &pa = P.pa;
    pa.bs = bs;
    pa.half = half;
    uint64_t ncid = 1;
    for (int a = 0; a < 3; ++a) {
        pa.g0[a] = smin[a] - 2;
        pa.gn[a] = smax[a] - smin[a] + 5;
        ncid *= (uint64_t)pa.gn[a];
    }
    if (ncid > (1ull << 27))
        return dm_fail(dm, LA3DM_ERR_ARG, "devmap: scan extent / block size needs more than 2^27 block cells (set max_range)");
    // axis tables: seq (int) | rank (u8) | mult (u8), three axes back to back
    std::vector<uint8_t> tab;
    size_t off_seq[3], off_rank[3], off_mult[3];
    uint32_t max_occ = 1;
    {
        size_t o = 0;
        for (int a = 0; a < 3; ++a) {
            off_seq[a] = o;
            o += 4 * seq[a].size();
        }
        for (int a = 0; a < 3; ++a) {
            off_rank[a] = o;
            o += seq[a].size();
        }
        for (int a = 0; a < 3; ++a) {
            off_mult[a] = o;
            o += (size_t)pa.gn[a];
        }
        tab.assign((o + 15) & ~(size_t)15, 0);
        for (int a = 0; a < 3; ++a) {
            memcpy(&tab[off_seq[a]], seq[a].data(), 4 * seq[a].size());
            uint8_t *mult = &tab[off_mult[a]], *rank = &tab[off_rank[a]];
            uint32_t mx = 0;
            for (size_t k = 0; k < seq[a].size(); ++k) {
                uint8_t &m = mult[seq[a][k] - pa.g0[a]];
                if (m == 255) return dm_fail(dm, LA3DM_ERR_ARG, "devmap: a candidate index repeats more than 255 times");
                rank[k] = m++;
                mx = std::max<uint32_t>(mx, m);
            }
            max_occ *= mx;
        }
    }
    DM_RESERVE(dm->axis_tab, tab.size());
    DM_TRY(hipMemcpyAsync(dm->axis_tab.ptr, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
    CandArgs &ca = P.ca;
    for (int a = 0; a < 3; ++a) {
        const uint8_t *base = (const uint8_t *)dm->axis_tab.ptr;
        pa.mult[a] = base + off_mult[a];
        ca.seq[a] = (const int *)(base + off_seq[a]);
        ca.rank[a] = base + off_rank[a];
        ca.nseq[a] = (int)seq[a].size();
    }
    ca.part = pa;
    const uint64_t n_entries64 = (uint64_t)seq[0].size() * seq[1].size() * seq[2].size();
    if (n_entries64 > (1ull << 30)) return dm_fail(dm, LA3DM_ERR_ARG, "devmap: candidate list too long");
    const uint32_t n_entries = (uint32_t)n_entries64;
    S.n_bbox_blocks = n_entries;

    // membership pairs (block, point), grouped by block with ascending point index inside a block
    DM_RESERVE(dm->flag, 4ull * npts);
    DM_RESERVE(dm->scan, 4ull * npts);
    uint32_t *m_cnt = (uint32_t *)dm->flag.ptr, *m_off = (uint32_t *)dm->scan.ptr;
    DM_RESERVE(dm->m_code, 16ull * npts);
    hipLaunchKernelGGL(dm_members_count, dim3(cdiv(npts, 256)), dim3(256), 0, st, xy, npts, pa, m_cnt,
                       (int4 *)dm->m_code.ptr);
    int bits = 1;
    while ((1ull << bits) < ncid) ++bits;
    P.cell_bits = bits;
    const bool want_slab = dm->shard_slab != 0;
    if (((dm->shard_world > 1 && dm->shard_fn && want_slab) || dm->force_slab) && max_occ == 1 && ctx->p.variant != 3) {
        // x-slab partition (devmap_kernels.h): only the per-cell point counts are formed for all blocks here; pairs, sort, CSR, rows
        // and neighbour tables follow inside the pass, once the cut is known, for the cells of this rank's slab (build_slab_csr)
        DM_RESERVE(dm->cell_cnt, 4ull * ncid);
        DM_RESERVE(dm->grid, 4ull * ncid);
        DM_TRY(hipMemsetAsync(dm->cell_cnt.ptr, 0, 4ull * ncid, st));
        hipLaunchKernelGGL(dm_members_hist, dim3(cdiv(npts, 256)), dim3(256), 0, st, (const int4 *)dm->m_code.ptr, npts, pa, (uint32_t *)dm->cell_cnt.ptr,
                           dm->d_cnt);
        hipLaunchKernelGGL(dm_cell_trained, dim3(std::min<uint32_t>(cdiv((uint32_t)ncid, 256), 64u)), dim3(256), 0, st, (const uint32_t *)dm->cell_cnt.ptr, (uint32_t)ncid, pa,
                           dm->d_cnt);
        DM_RESERVE(dm->c_flag, 4ull * n_entries);
        DM_RESERVE(dm->c_scan, 4ull * n_entries);
        P.slab = true;
        P.ncid = ncid;
        P.n_entries = n_entries;
        P.max_occ = max_occ;
        P.n_mem = 0;
        P.n_geo = 0;
        P.train_off = nullptr;
        return LA3DM_OK;
    }
    if ((rc = exclusive_scan(dm, m_cnt, m_off, npts, (int)kCntMembers, true)) != LA3DM_OK) return rc;
    if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
    const uint32_t n_mem = dm->h_cnt[kCntMembers];
    DM_RESERVE(dm->k0, 4ull * n_mem);
    DM_RESERVE(dm->k1, 4ull * n_mem);
    DM_RESERVE(dm->v0, 4ull * n_mem);
    DM_RESERVE(dm->v1, 4ull * n_mem);
    uint32_t *k0 = (uint32_t *)dm->k0.ptr, *k1 = (uint32_t *)dm->k1.ptr, *v0 = (uint32_t *)dm->v0.ptr, *v1 = (uint32_t *)dm->v1.ptr;
    DM_RESERVE(dm->grid, 4ull * ncid);
    if (n_mem && sort_fusable(dm, bits)) {   // the pairs are written by the sort's histogram launch
        const MembersSrc src = {(const int4 *)dm->m_code.ptr, pa, m_off, k0, v0, dm->d_cnt, (int32_t *)dm->grid.ptr, (uint32_t)ncid};
        if ((rc = sort_pairs_src(dm, src, npts, k0, k1, v0, v1, n_mem, bits)) != LA3DM_OK) return rc;
    } else {
        hipLaunchKernelGGL(dm_members_write, dim3(cdiv(npts, 256)), dim3(256), 0, st, (const int4 *)dm->m_code.ptr, npts, pa, m_off,
                           k0, v0, dm->d_cnt, (int32_t *)dm->grid.ptr, (uint32_t)ncid);
        if ((rc = sort_pairs(dm, k0, k1, v0, v1, n_mem, bits)) != LA3DM_OK) return rc;
    }
    DM_RESERVE(dm->c_flag, 4ull * std::max(n_mem, n_entries));
    DM_RESERVE(dm->c_scan, 4ull * std::max(n_mem, n_entries));
    DM_RESERVE(dm->seg_start, 4ull * (n_mem + 1));
    DM_RESERVE(dm->seg_key, 4ull * (n_mem + 1));
    uint32_t *sflag = (uint32_t *)dm->c_flag.ptr;
    uint32_t *train_off = (uint32_t *)dm->seg_start.ptr, *seg_key = (uint32_t *)dm->seg_key.ptr;
    // (the head flags have one reader — BGK-L's row flags; the prefix array none: left unwritten)
    if ((rc = scan_heads(dm, k1, n_mem, ctx->p.variant == 3 ? sflag : nullptr, nullptr, train_off, seg_key, (int)kCntGeo, (int)kCntGridValid)) != LA3DM_OK) return rc;
    if (ctx->p.variant == 3) {  // training rows: hits as degenerate segments, every beam once per block
        DM_RESERVE(dm->l_rflag, 4ull * n_mem);
        DM_RESERVE(dm->l_rscan, 4ull * n_mem);
        DM_RESERVE(dm->l_rows, 48ull * n_mem);   // 12 floats per row (LA3DM_SCAN_ROWS_PREPARED)
        DM_RESERVE(dm->l_rows_off, 4ull * ((size_t)n_mem + 2));
        uint32_t *rflag = (uint32_t *)dm->l_rflag.ptr, *rscan = (uint32_t *)dm->l_rscan.ptr;
        hipLaunchKernelGGL(dm_l_row_flags, dim3(cdiv(n_mem, 256)), dim3(256), 0, st, v1, sflag, n_mem,
                           (const int32_t *)dm->l_ray_idx.ptr, rflag);
        if ((rc = exclusive_scan(dm, rflag, rscan, n_mem)) != LA3DM_OK) return rc;
        hipLaunchKernelGGL(dm_l_rows_write, dim3(cdiv(n_mem, 256)), dim3(256), 0, st, v1, n_mem, rflag, rscan, xy,
                           (const int32_t *)dm->l_ray_idx.ptr, (const float *)dm->l_rays.ptr, (float4 *)dm->l_rows.ptr);
        hipLaunchKernelGGL(dm_l_rows_off, dim3(cdiv((size_t)n_mem + 1, 256)), dim3(256), 0, st, train_off, dm->d_cnt, rflag, rscan,
                           n_mem, (uint32_t *)dm->l_rows_off.ptr);
        P.rows_off = (uint32_t *)dm->l_rows_off.ptr;
    } else {
        DM_RESERVE(dm->train, 16ull * n_mem);
    }
    hipLaunchKernelGGL(dm_gather_geo, dim3(cdiv(n_mem, 256)), dim3(256), 0, st, xy, (const uint32_t *)v1, n_mem,
                       ctx->p.variant == 3 ? (float4 *)nullptr : (float4 *)dm->train.ptr, (const uint32_t *)seg_key, dm->d_cnt, pa,
                       (int32_t *)dm->grid.ptr);
    hipLaunchKernelGGL(dm_count_trained, dim3(std::min<uint32_t>(cdiv(n_mem, 256 * 4), 64u)), dim3(256), 0, st, (const uint32_t *)seg_key, pa, dm->d_cnt);
    // the segment count is only needed on the host by the GP launches; the BGK path reads it (and the error flag)
    // together with the test-block count of the first pass
    uint32_t n_geo = n_mem;
    if (ctx->p.variant == 1) {
        if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
        n_geo = dm->h_cnt[kCntGeo];
    }
    P.ncid = ncid;
    P.n_entries = n_entries;
    P.max_occ = max_occ;
    P.n_mem = n_mem;
    P.n_geo = n_geo;
    P.train_off = train_off;
    return LA3DM_OK;
}

// x-slab partition, second half (sharded single-pass inserts; devmap_kernels.h): the (block, point) pairs, their sort, the CSR, the
// training rows and the dense cell -> training-block index — for the grid cells of the own range [t0, t1) of the test list and its
// halo (the cells of those test blocks' extended blocks) only.  Training-block indices are local to the rank.
static int build_slab_csr(la3dm_devmap *dm, ScanPlan &P, const uint32_t *t_ent, uint32_t t0, uint32_t t1) {
    la3dm_ctx *ctx = dm->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t npts = dm->n_xy;
    const float4 *xy = (const float4 *)dm->xy.ptr;
    const PartArgs &pa = P.pa;
    const uint32_t ncid = (uint32_t)P.ncid;
    int rc;
    if (dm->dbg_fail_slab_rank >= 0 && dm->shard_world > 1 && dm->dbg_fail_slab_rank == (int)dm->shard_rank)
        return dm_fail(dm, LA3DM_ERR_OOM, "devmap: injected rank-local failure in the x-slab partition (LA3DM_INJECT_SLAB_FAILURE)");
    DM_RESERVE(dm->slab_range, 8);
    uint32_t *range = (uint32_t *)dm->slab_range.ptr;
    DM_TRY(hipMemsetAsync(range, 0xFF, 4, st));
    DM_TRY(hipMemsetAsync(range + 1, 0, 4, st));
    if (t1 > t0) hipLaunchKernelGGL(dm_slab_range, dim3(1), dim3(64), 0, st, P.ca, t_ent, t0, t1, range, dm->shard_world > 1 ? 0u : ncid);
    uint32_t *m_cnt = (uint32_t *)dm->flag.ptr, *m_off = (uint32_t *)dm->scan.ptr;   // (reserved by partition: 4 npts each)
    hipLaunchKernelGGL(dm_members_count_slab, dim3(cdiv(npts, 256)), dim3(256), 0, st, (const int4 *)dm->m_code.ptr, npts, pa, (const uint32_t *)range, m_cnt);
    if ((rc = exclusive_scan(dm, m_cnt, m_off, npts, (int)kCntMembers, true)) != LA3DM_OK) return rc;
    if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
    const uint32_t n_mem = dm->h_cnt[kCntMembers];
    const size_t pb = 4ull * std::max<uint32_t>(n_mem, 4u);
    DM_RESERVE(dm->k0, pb);
    DM_RESERVE(dm->k1, pb);
    DM_RESERVE(dm->v0, pb);
    DM_RESERVE(dm->v1, pb);
    uint32_t *k0 = (uint32_t *)dm->k0.ptr, *k1 = (uint32_t *)dm->k1.ptr, *v0 = (uint32_t *)dm->v0.ptr, *v1 = (uint32_t *)dm->v1.ptr;
    DM_RESERVE(dm->c_flag, pb);
    DM_RESERVE(dm->c_scan, pb);
    DM_RESERVE(dm->seg_start, 4ull * ((size_t)n_mem + 1));
    DM_RESERVE(dm->seg_key, 4ull * ((size_t)n_mem + 1));
    DM_RESERVE(dm->train, 16ull * std::max<uint32_t>(n_mem, 1u));
    uint32_t *train_off = (uint32_t *)dm->seg_start.ptr, *seg_key = (uint32_t *)dm->seg_key.ptr;
    if (n_mem) {
        const MembersSlabSrc src = {(const int4 *)dm->m_code.ptr, pa, m_off, range, k0, v0, (int32_t *)dm->grid.ptr, ncid};
        if (sort_fusable(dm, P.cell_bits)) {   // the pairs are written by the sort's histogram launch
            if ((rc = sort_pairs_src(dm, src, npts, k0, k1, v0, v1, n_mem, P.cell_bits)) != LA3DM_OK) return rc;
        } else {
            hipLaunchKernelGGL((dm_run_src<MembersSlabSrc>), dim3(cdiv(npts, 256)), dim3(256), 0, st, src, npts);
            if ((rc = sort_pairs(dm, k0, k1, v0, v1, n_mem, P.cell_bits)) != LA3DM_OK) return rc;
        }
        if ((rc = scan_heads(dm, k1, n_mem, nullptr, nullptr, train_off, seg_key, (int)kCntGeo, (int)kCntGridValid)) != LA3DM_OK)
            return rc;
        hipLaunchKernelGGL(dm_gather_geo, dim3(cdiv(n_mem, 256)), dim3(256), 0, st, xy, (const uint32_t *)v1, n_mem, (float4 *)dm->train.ptr,
                           (const uint32_t *)seg_key, dm->d_cnt, pa, (int32_t *)dm->grid.ptr);
    } else {   // a rank whose slab holds no training point: no block has a model
        DM_TRY(hipMemsetAsync(dm->grid.ptr, 0xFF, 4ull * ncid, st));
        DM_TRY(hipMemsetAsync(train_off, 0, 8, st));
    }
    P.n_mem = n_mem;
    P.n_geo = n_mem;
    P.train_off = train_off;
    if (ctx->p.variant == 1) {   // the GP launches are sized by the number of training blocks
        if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
        P.n_geo = n_mem ? dm->h_cnt[kCntGeo] : 0u;
    }
    if (getenv("LA3DM_DEBUG_SHARD"))
        fprintf(stderr, "la3dm x-slab partition: rank %u of %u builds the CSR of %u (block, point) pairs for test blocks [%u, %u)\n", dm->shard_rank,
                dm->shard_world, n_mem, t0, t1);
    return LA3DM_OK;
}

// block_depth 3: the leaf-list and write-back + prune launches with `batch` (4 or 8) test blocks per wave (devmap_depth3.h)
static void launch_leaves_d3(bool emit, uint32_t batch, uint32_t grid, hipStream_t st, const uint32_t *slot, const uint32_t *counters,
                             const uint8_t *S, const float *A, const float *B, uint32_t *nleaf, const uint32_t *leaf_off, uint32_t *leaf_key,
                             float *alpha, float *beta, uint32_t *leaf_node, const LeafExtra &lx) {
    if (emit && batch == 8)
        hipLaunchKernelGGL((dm_leaves_d3<true, 8>), dim3(grid), dim3(256), 0, st, slot, counters, S, A, B, nleaf, leaf_off, leaf_key, alpha, beta, leaf_node, lx);
    else if (emit)
        hipLaunchKernelGGL((dm_leaves_d3<true, 4>), dim3(grid), dim3(256), 0, st, slot, counters, S, A, B, nleaf, leaf_off, leaf_key, alpha, beta, leaf_node, lx);
    else if (batch == 8)
        hipLaunchKernelGGL((dm_leaves_d3<false, 8>), dim3(grid), dim3(256), 0, st, slot, counters, S, A, B, nleaf, leaf_off, leaf_key, alpha, beta, leaf_node, lx);
    else
        hipLaunchKernelGGL((dm_leaves_d3<false, 4>), dim3(grid), dim3(256), 0, st, slot, counters, S, A, B, nleaf, leaf_off, leaf_key, alpha, beta, leaf_node, lx);
}
static void launch_commit_prune_d3(uint32_t batch, hipStream_t st, const uint32_t *slot, uint32_t n_test, const uint32_t *leaf_off,
                                   const uint32_t *leaf_node, const uint32_t *leaf_key, const float *alpha, const float *beta,
                                   const uint8_t *state, float *A, float *B, uint8_t *S, uint32_t *counters, uint32_t *done,
                                   volatile uint32_t *mailbox, uint32_t mseq) {
    const dim3 grid(std::min(cdiv(cdiv(n_test, batch), 4), kCommitPruneWgs));
    const size_t lds = 4 * (size_t)batch * prune_lds_stride(kD3Npb);
    if (batch == 8)
        hipLaunchKernelGGL((dm_commit_prune_d3<8>), grid, dim3(256), lds, st, slot, n_test, leaf_off, leaf_node, leaf_key, alpha, beta, state, A, B, S,
                           counters, done, mailbox, mseq);
    else
        hipLaunchKernelGGL((dm_commit_prune_d3<4>), grid, dim3(256), lds, st, slot, n_test, leaf_off, leaf_node, leaf_key, alpha, beta, state, A, B, S,
                           counters, done, mailbox, mseq);
}

// One pass over the candidate list (bgkoctomap.cpp:286-353): test-block decision, find-or-create, leaves in
// LeafIterator order, predict + fuse, write-back, prune.  A pass holds every candidate key once; keys the float
// stepping of get_blocks_in_bbox repeats come back in later passes, as in the serial reference.
static int run_pass(la3dm_devmap *dm, ScanPlan &P, uint32_t pass, uint32_t *n_test0) {
    la3dm_ctx *ctx = dm->ctx;
    hipStream_t st = ctx->stream;
    la3dm_devmap_stats &S = dm->stats;
    CandArgs &ca = P.ca;
    const uint32_t n_entries = P.n_entries, max_occ = P.max_occ, ncell = dm->ncell;
    uint32_t n_mem = P.n_mem;
    uint32_t *train_off = P.train_off;   // (both set by build_slab_csr, further down, in the x-slab form of a sharded insert)
    uint32_t *c_flag = (uint32_t *)dm->c_flag.ptr, *c_weight = (uint32_t *)dm->c_weight.ptr, *c_scan = (uint32_t *)dm->c_scan.ptr;
    uint32_t &n_geo = P.n_geo;
    int rc;
    const double tp0 = wall();
    ca.pass = pass;
    if (P.slab)
        hipLaunchKernelGGL((dm_candidates<true>), dim3(cdiv(n_entries, 256)), dim3(256), 0, st, ca, (const int32_t *)dm->cell_cnt.ptr,
                           (const uint32_t *)nullptr, n_entries, c_flag, c_weight);
    else
        hipLaunchKernelGGL((dm_candidates<false>), dim3(cdiv(n_entries, 256)), dim3(256), 0, st, ca, (const int32_t *)dm->grid.ptr,
                           (const uint32_t *)train_off, n_entries, c_flag, c_weight);
    DM_RESERVE(dm->t_key0, 4ull * n_entries);
    DM_RESERVE(dm->t_ent0, 4ull * n_entries);
    // (the scan's total is the test-block count: it publishes the counters, the compaction runs while the host waits)
    if ((rc = exclusive_scan(dm, c_flag, c_scan, n_entries, (int)kCntTest, true)) != LA3DM_OK) return rc;
    // Heaviest test blocks first (the blocks are independent: order only balances the launch).  The compaction is the histogram
    // launch of that one-digit sort, and the pass behind it takes the list's length from the counter block: both are queued
    // before the host has read the length (round 5; compaction, read-back, histogram, pass were four steps in a row).
    const bool sharded = dm->shard_world > 1;
    const uint32_t world = dm->shard_world;
    const bool sorted_on_device = !sharded && dm->test_sort && sort_fusable(dm, 32, 24);
    if (sorted_on_device) {
        DM_RESERVE(dm->t_key1, 4ull * n_entries);
        DM_RESERVE(dm->t_ent1, 4ull * n_entries);
        const TestCompactSrc src = {c_flag, c_scan, c_weight, n_entries, (uint32_t *)dm->t_key0.ptr, (uint32_t *)dm->t_ent0.ptr, dm->d_cnt};
        SortJob job;
        if ((rc = sort_begin_src(dm, src, n_entries, n_entries, 32, 24, job)) != LA3DM_OK) return rc;   // the weight class
        if ((rc = sort_passes(dm, job, (const uint32_t *)dm->t_key0.ptr, (uint32_t *)dm->t_key1.ptr, (const uint32_t *)dm->t_ent0.ptr,
                              (uint32_t *)dm->t_ent1.ptr, dm->d_cnt + kCntTest)) != LA3DM_OK)
            return rc;
    } else {
        hipLaunchKernelGGL(dm_test_compact, dim3(cdiv(n_entries, 256)), dim3(256), 0, st, c_flag, c_scan, c_weight, n_entries,
                           (uint32_t *)dm->t_key0.ptr, (uint32_t *)dm->t_ent0.ptr, dm->d_cnt);
    }
    if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
    if (dm->h_cnt[kCntError])
        return dm_fail(dm, LA3DM_ERR_ARG, "devmap: internal error: training point outside the block index grid");
    if (ctx->p.variant != 1 && !P.slab) n_geo = dm->h_cnt[kCntGeo];
    S.n_train_blocks = dm->h_cnt[kCntTrained];
    const uint32_t n_test = dm->h_cnt[kCntTest];
    if (n_test == 0) return LA3DM_OK;
    S.n_test_blocks += n_test;
    S.n_passes = pass + 1;
    // the list the rest of the pass works on: sorted copies, or (sharded / LA3DM_TEST_SORT=0) the compacted list in candidate order
    const uint32_t *t_key = (const uint32_t *)dm->t_key1.ptr, *t_ent = (const uint32_t *)dm->t_ent1.ptr;
    if (sorted_on_device) {
        // (queued above)
    } else if (!sharded && dm->test_sort) {   // the library sort (LA3DM_OWN_SORT=0)
        DM_RESERVE(dm->t_key1, 4ull * n_test);
        DM_RESERVE(dm->t_ent1, 4ull * n_test);
        t_key = (const uint32_t *)dm->t_key1.ptr;
        t_ent = (const uint32_t *)dm->t_ent1.ptr;
        if (n_test <= kSortSmallMax) {
            uint32_t N = 2;
            while (N < n_test) N <<= 1;
            hipLaunchKernelGGL(dm_sort_small, dim3(1), dim3(1024), 0, st, (const uint32_t *)dm->t_key0.ptr, (const uint32_t *)dm->t_ent0.ptr,
                               n_test, N, (uint32_t *)dm->t_key1.ptr, (uint32_t *)dm->t_ent1.ptr);
        } else if ((rc = sort_pairs(dm, (uint32_t *)dm->t_key0.ptr, (uint32_t *)dm->t_key1.ptr, (uint32_t *)dm->t_ent0.ptr,
                                    (uint32_t *)dm->t_ent1.ptr, n_test, 32, 24)) != LA3DM_OK)   // the weight class
            return rc;
    } else {
        t_key = (const uint32_t *)dm->t_key0.ptr;
        t_ent = (const uint32_t *)dm->t_ent0.ptr;
    }
    if (sharded) {
        // block-sharded: the list stays in candidate order (block indices x-major: neighbouring test blocks, which share
        // training blocks, stay on one GPU's L2) and is cut into `world` contiguous ranges of equal weight
        DM_RESERVE(dm->shard_w, 4ull * n_test);
        DM_RESERVE(dm->shard_cumw, 4ull * n_test);
        DM_RESERVE(dm->shard_bounds, 8ull * (world + 1));
        // (a block's weight is capped so that the 32-bit running sum cannot wrap: n_test * cap < 2^31 — ADVICE r02)
        const uint32_t w_cap = std::max<uint32_t>(32u, (uint32_t)((1ull << 31) / n_test));
        hipLaunchKernelGGL(dm_shard_weight, dim3(cdiv(n_test, 256)), dim3(256), 0, st, t_key, n_test,
                           w_cap, (uint32_t *)dm->shard_w.ptr);
        if ((rc = exclusive_scan(dm, (const uint32_t *)dm->shard_w.ptr, (uint32_t *)dm->shard_cumw.ptr, n_test)) != LA3DM_OK) return rc;
        hipLaunchKernelGGL(dm_shard_bounds, dim3(1), dim3(1024), 0, st, (const uint32_t *)dm->shard_cumw.ptr,
                           (const uint32_t *)dm->shard_w.ptr, n_test, world, (uint32_t *)dm->shard_bounds.ptr);
    }
    DM_RESERVE(dm->t_blockkey, 8ull * n_test);
    DM_RESERVE(dm->t_center, 12ull * n_test);
    DM_RESERVE(dm->t_nbr, 28ull * n_test);
    DM_RESERVE(dm->t_slot, 4ull * n_test);
    // Every fallible reservation of the pack stage comes BEFORE the launch that creates blocks: dm_test_build
    // publishes new keys and bumps the device block count, and the new blocks' default nodes are only written by the
    // leaf-count launch behind it — nothing that can fail may sit between the two.
    DM_RESERVE(dm->nleaf, 4ull * (n_test + 1));
    DM_RESERVE(dm->leaf_off, 4ull * (n_test + 1));
    const size_t max_leaves = (size_t)n_test * ncell;
    DM_RESERVE(dm->leaf_key, 4 * max_leaves);
    DM_RESERVE(dm->leaf_alpha, 4 * max_leaves);
    DM_RESERVE(dm->leaf_beta, 4 * max_leaves);
    DM_RESERVE(dm->leaf_node, 4 * max_leaves);
    DM_RESERVE(dm->leaf_state, max_leaves);
    // blocks: find or create (bgkoctomap.cpp:298-305), in the launch that builds the test blocks' keys and neighbour tables
    if ((rc = grow_pool(dm, (size_t)dm->n_blocks + n_test)) != LA3DM_OK) return rc;
    if ((rc = grow_table(dm, (size_t)dm->n_blocks + n_test)) != LA3DM_OK) return rc;
    // (d_cnt[kCntBlocks] holds the pool's block count since dm_begin; the passes keep it current)
    {
        const TableArgs tb = {dm->tab_key, dm->tab_val, dm->tab_cap - 1, dm->d_cnt + kCntBlocks, dm->blk_key};
        hipLaunchKernelGGL(dm_test_build, dim3(cdiv(n_test, 256)), dim3(256), 0, st, ca, P.slab ? (const int32_t *)nullptr : (const int32_t *)dm->grid.ptr,
                           t_ent, dm->d_cnt, (long long *)dm->t_blockkey.ptr, (float *)dm->t_center.ptr,
                           (int32_t *)dm->t_nbr.ptr, tb, (uint32_t *)dm->t_slot.ptr);
    }
    // default nodes for the blocks this launch created — slots [old count, new count); the new count stays on the device (read
    // back with the pass's other counters) — are written by the leaf-count launch below (LeafExtra)
    // pack: leaves in LeafIterator order
    uint32_t *nleaf = (uint32_t *)dm->nleaf.ptr, *leaf_off = (uint32_t *)dm->leaf_off.ptr;
    LeafExtra lx;
    memset(&lx, 0, sizeof(lx));
    lx.old_blocks = dm->n_blocks;
    lx.a0 = dm->init_A;
    lx.b0 = dm->init_B;
    lx.A_w = dm->A;
    lx.B_w = dm->B;
    lx.S_w = dm->S;
    // test blocks per wave (devmap_depth3.h; measured at configs[4]'s 266 k test blocks: 8 beats 4 by 27 us, at configs[1]'s 42 k they are level)
    const int d3_env = dm->depth3_batch < 0 ? (n_test >= 65536u ? 8 : 4) : dm->depth3_batch;
    const uint32_t d3 = dm->depth == 3 && dm->npb == kD3Npb ? (d3_env >= 8 ? 8u : d3_env > 0 ? 4u : 0u) : 0u;
    if (d3)
        launch_leaves_d3(false, d3, cdiv(n_test, 4 * d3), st, (const uint32_t *)dm->t_slot.ptr, dm->d_cnt, (const uint8_t *)dm->S, (const float *)dm->A,
                         (const float *)dm->B, nleaf, nullptr, nullptr, nullptr, nullptr, nullptr, lx);
    else
        hipLaunchKernelGGL((dm_leaves<false>), dim3(cdiv(n_test, 4)), dim3(256), 0, st, (const uint32_t *)dm->t_slot.ptr, dm->d_cnt,
                           (const uint8_t *)dm->S, (const float *)dm->A, (const float *)dm->B, dm->npb, dm->depth, nleaf,
                           (const uint32_t *)nullptr, (uint32_t *)nullptr, (float *)nullptr, (float *)nullptr, (uint32_t *)nullptr, lx);
    if (ctx->p.variant == 3)
        hipLaunchKernelGGL(dm_l_test_stats, dim3(std::min(cdiv(n_test, 256), 32u)), dim3(256), 0, st, (const int32_t *)dm->t_nbr.ptr,
                           (const uint32_t *)P.rows_off, (const uint32_t *)nleaf, n_test, dm->d_cnt);
    if ((rc = exclusive_scan(dm, nleaf, leaf_off, n_test + 1, (int)kCntLeaves)) != LA3DM_OK) return rc;
    // Block-sharded, single pass (round 5, VERDICT r04 #4b): a rank lists the leaves of its OWN range of test blocks only; the
    // other ranks' leaves arrive through the all-gather-v with their keys (13 B per leaf instead of 9), and the write-back finds
    // their nodes from this replica's slot of the block.  The range cut needs the leaf offsets, so the one host wait of the
    // sharded path moves in front of the emitting launch.
    const bool own_emit = sharded && max_occ == 1;
    uint32_t t0s = 0, t1s = n_test;
    if (sharded) {
        uint32_t *lb = (uint32_t *)dm->shard_bounds.ptr + (world + 1);
        hipLaunchKernelGGL(dm_shard_leaf_bounds, dim3(1), dim3(1024), 0, st, (const uint32_t *)dm->shard_bounds.ptr,
                           (const uint32_t *)leaf_off, world, lb);
        DM_TRY(hipMemcpyAsync(dm->h_shard, dm->shard_bounds.ptr, 8ull * (world + 1), hipMemcpyDeviceToHost, st));
        DM_TRY(hipStreamSynchronize(st));   // (the one host wait of the sharded path: launch sizes depend on the cut)
        const uint32_t *hb = dm->h_shard, *hl = dm->h_shard + (world + 1);
        for (uint32_t q = 0; q < world; ++q)
            if (hb[q] > hb[q + 1] || hb[q + 1] > n_test || hl[q] > hl[q + 1])
                return dm_fail(dm, LA3DM_ERR_HIP, "devmap: internal error: the range cut of the sharded insert is not monotone");
        t0s = hb[dm->shard_rank];
        t1s = hb[dm->shard_rank + 1];
    }
    int rc_slab = LA3DM_OK;
    if (P.slab) {
        // the cut is known: pairs, sort, CSR and rows of the own slab, then the own range's neighbour tables.  A rank of a sharded
        // insert that fails here (out of memory for its pairs, ...) must still enter the leaf exchange its peers are about to wait
        // in: it skips its kernel, hands its range over as "no leaf updated" and reports afterwards (see the exchange below)
        rc_slab = build_slab_csr(dm, P, t_ent, t0s, t1s);
        if (rc_slab != LA3DM_OK && !sharded) return rc_slab;
        n_mem = P.n_mem;
        train_off = P.train_off;
        if (rc_slab == LA3DM_OK && t1s > t0s)
            hipLaunchKernelGGL(dm_test_nbr, dim3(cdiv(t1s - t0s, 256)), dim3(256), 0, st, ca, (const int32_t *)dm->grid.ptr, t_ent, t0s, t1s,
                               (int32_t *)dm->t_nbr.ptr);
    }
    {
        // the emitting launch carries the pass's work counters (train_reads, pair_evals) in a few workgroups of its own
        const uint32_t e0 = own_emit ? t0s : 0u, e1 = own_emit ? t1s : n_test;
        const uint32_t main_wgs = cdiv(e1 - e0, d3 ? 4 * d3 : 4), stat_wgs = ctx->p.variant == 3 ? 0u : std::min(cdiv(n_test, 256), 32u);
        lx.t_key = stat_wgs ? t_key : nullptr;
        lx.counters_w = dm->d_cnt;
        lx.main_wgs = main_wgs;
        lx.t_begin = e0;
        lx.t_end = e1;
        if ((main_wgs + stat_wgs) && d3)
            launch_leaves_d3(true, d3, main_wgs + stat_wgs, st, (const uint32_t *)dm->t_slot.ptr, dm->d_cnt, (const uint8_t *)dm->S, (const float *)dm->A,
                             (const float *)dm->B, nleaf, (const uint32_t *)leaf_off, (uint32_t *)dm->leaf_key.ptr, (float *)dm->leaf_alpha.ptr,
                             (float *)dm->leaf_beta.ptr, (uint32_t *)dm->leaf_node.ptr, lx);
        else if (main_wgs + stat_wgs)
            hipLaunchKernelGGL((dm_leaves<true>), dim3(main_wgs + stat_wgs), dim3(256), 0, st, (const uint32_t *)dm->t_slot.ptr, dm->d_cnt,
                               (const uint8_t *)dm->S, (const float *)dm->A, (const float *)dm->B, dm->npb, dm->depth, nleaf,
                               (const uint32_t *)leaf_off, (uint32_t *)dm->leaf_key.ptr, (float *)dm->leaf_alpha.ptr,
                               (float *)dm->leaf_beta.ptr, (uint32_t *)dm->leaf_node.ptr, lx);
    }
    double tp1 = tp0;
    if (dm->stage_timing) {
        DM_TRY(hipStreamSynchronize(st));
        tp1 = wall();
        S.t_pack += tp1 - tp0;
    }
    // E: predict + fuse
    la3dm_bgk_scan s;
    memset(&s, 0, sizeof(s));
    s.train_xyzy = (const float *)dm->train.ptr;
    s.train_off = train_off;
    s.n_train_pts = n_mem;
    if (ctx->p.variant == 3) {  // rows of 12 floats (prepared form); n_mem bounds their number
        s.train_xyzy = (const float *)dm->l_rows.ptr;
        s.train_off = P.rows_off;
    }
    s.n_train_blk = n_geo;
    s.nbr = (const int32_t *)dm->t_nbr.ptr;
    s.blk_center = (const float *)dm->t_center.ptr;
    s.leaf_off = leaf_off;
    s.n_test_blk = n_test;
    s.n_leaf = (uint32_t)std::min<size_t>(max_leaves, 0xFFFFFFFFu);
    s.leaf_key = (const uint32_t *)dm->leaf_key.ptr;
    s.alpha = (float *)dm->leaf_alpha.ptr;
    s.beta = (float *)dm->leaf_beta.ptr;
    s.state = (uint8_t *)dm->leaf_state.ptr;
    s.flags = P.flags;
    if (ctx->p.variant == 3) s.flags |= LA3DM_SCAN_ROWS_PREPARED;   // dm_l_rows_write wrote the 12-float form
    if (pass == 0 && dm->insert_into_empty) s.flags |= LA3DM_SCAN_FULL_BLOCKS;
    if (sharded) {
        // this rank's contiguous range of test blocks; leaf_off holds absolute leaf indices, so offsetting the per-block
        // arrays is all the kernel needs
        s.nbr += 7ull * t0s;
        s.blk_center += 3ull * t0s;
        s.leaf_off += t0s;
        s.n_test_blk = t1s - t0s;
    }
    rc = rc_slab;
    const std::string slab_err = rc_slab != LA3DM_OK ? ctx->err : std::string();
    if (s.n_test_blk && rc_slab == LA3DM_OK)
        rc = ctx->p.variant == 1   ? la3dm_gp_scan_device(ctx, &s, st, nullptr)
             : ctx->p.variant == 3 ? la3dm_bgkl_scan_device(ctx, &s, st, nullptr)
                                   : la3dm_bgk_scan_device(ctx, &s, st, nullptr);
    if (rc != LA3DM_OK && !sharded) return rc;
    double tg0 = tp1;
    if (sharded) {
        // ONE all-gather-v, in place on the leaf arrays (a rank's leaves are a contiguous index range of alpha, beta and
        // state: 9 B per leaf, no pack / unpack, no padding), queued on this stream by the callback; commit and prune
        // follow on the same stream on identical data everywhere.  A rank whose launch failed still enters the
        // collective (its peers would wait for ever otherwise) and reports afterwards.
        const int rc_kernel = rc;
        const uint32_t *hl = dm->h_shard + (world + 1);
        if (rc_kernel != LA3DM_OK && hl[dm->shard_rank + 1] > hl[dm->shard_rank]) {
            // this rank's range goes out as "update() ran on no leaf" (state 0: the write-back skips such leaves), so that every
            // replica — this one included — stays what it was for these blocks instead of committing whatever the arrays hold
            (void)hipMemsetAsync((uint8_t *)dm->leaf_state.ptr + hl[dm->shard_rank], 0, hl[dm->shard_rank + 1] - hl[dm->shard_rank], st);
        }
        for (int g = 0; g < 4; ++g) {
            dm->shard_off[g].resize(world);
            dm->shard_bytes[g].resize(world);
        }
        for (uint32_t q = 0; q < world; ++q) {
            const uint64_t f = hl[q], n_q = hl[q + 1] - hl[q];
            dm->shard_off[0][q] = dm->shard_off[1][q] = dm->shard_off[3][q] = 4 * f;
            dm->shard_bytes[0][q] = dm->shard_bytes[1][q] = dm->shard_bytes[3][q] = 4 * n_q;
            dm->shard_off[2][q] = f;
            dm->shard_bytes[2][q] = n_q;
        }
        la3dm_gather_seg segs[4] = {{dm->leaf_alpha.ptr, dm->shard_off[0].data(), dm->shard_bytes[0].data()},
                                    {dm->leaf_beta.ptr, dm->shard_off[1].data(), dm->shard_bytes[1].data()},
                                    {dm->leaf_state.ptr, dm->shard_off[2].data(), dm->shard_bytes[2].data()},
                                    {dm->leaf_key.ptr, dm->shard_off[3].data(), dm->shard_bytes[3].data()}};
        const uint32_t n_segs = own_emit ? 4u : 3u;   // (the keys travel only when the ranks did not list each other's leaves)
        if (dm->stage_timing) {
            DM_TRY(hipStreamSynchronize(st));
            tg0 = wall();
        }
        const int xrc = hl[world] ? dm->shard_fn(dm->shard_user, segs, n_segs, world, dm->shard_rank, (void *)st) : 0;
        if (rc_kernel != LA3DM_OK) {
            if (!slab_err.empty()) ctx->err = slab_err;
            return rc_kernel;
        }
        if (xrc != 0) return dm_fail(dm, LA3DM_ERR_ARG, "devmap: the all-gather callback of the sharded insert failed");
        if (dm->stage_timing) {
            DM_TRY(hipStreamSynchronize(st));
            S.t_gather += wall() - tg0;
        }
    }
    double tp2 = tp1;
    if (dm->stage_timing) {
        DM_TRY(hipStreamSynchronize(st));
        tp2 = wall();
        S.t_kernel += (sharded ? tg0 : tp2) - tp1;
    }
    // f3: write-back + prune
    // The reference prunes after ALL test blocks have been predicted (bgkoctomap.cpp:344-353): with repeated keys
    // the later passes must still see the un-pruned leaves, so the prune of pass 0 (which holds every distinct
    // test block) is deferred to the end of the pass loop.  A single-pass scan (the usual case) commits and prunes in ONE
    // launch, whose last workgroup also sends the counter block to the host (dm_commit_prune).
    bool reset_queued = false;   // dm_commit_prune leaves the counter block ready for the next insert
    if (max_occ == 1) {
        volatile uint32_t *mailbox = nullptr;
        uint32_t mseq = 0;
        publish_with(dm, mailbox, mseq);
        if (d3)
            launch_commit_prune_d3(d3, st, (const uint32_t *)dm->t_slot.ptr, n_test, (const uint32_t *)leaf_off, (const uint32_t *)dm->leaf_node.ptr,
                                   own_emit ? (const uint32_t *)dm->leaf_key.ptr : (const uint32_t *)nullptr, (const float *)dm->leaf_alpha.ptr,
                                   (const float *)dm->leaf_beta.ptr, (const uint8_t *)dm->leaf_state.ptr, dm->A, dm->B, dm->S, dm->d_cnt,
                                   dm->d_mm + kArriveBase, mailbox, mseq);
        else
            hipLaunchKernelGGL(dm_commit_prune, dim3(std::min(cdiv(n_test, 4), kCommitPruneWgs)), dim3(256), 4 * prune_lds_stride(dm->npb), st,
                           (const uint32_t *)dm->t_slot.ptr, n_test, (const uint32_t *)leaf_off, (const uint32_t *)dm->leaf_node.ptr,
                           own_emit ? (const uint32_t *)dm->leaf_key.ptr : (const uint32_t *)nullptr, (const float *)dm->leaf_alpha.ptr, (const float *)dm->leaf_beta.ptr, (const uint8_t *)dm->leaf_state.ptr,
                           dm->A, dm->B, dm->S, dm->npb, dm->depth, dm->d_cnt, dm->d_mm + kArriveBase, mailbox, mseq);
        reset_queued = mailbox != nullptr;
    } else {
        hipLaunchKernelGGL(dm_commit, dim3(cdiv(max_leaves, 256)), dim3(256), 0, st, dm->d_cnt, (const uint32_t *)dm->leaf_node.ptr,
                           (const float *)dm->leaf_alpha.ptr, (const float *)dm->leaf_beta.ptr,
                           (const uint8_t *)dm->leaf_state.ptr, dm->A, dm->B, dm->S);
        if (pass == 0) {
            DM_RESERVE(dm->t_slot0, 4ull * n_test);
            DM_TRY(hipMemcpyAsync(dm->t_slot0.ptr, dm->t_slot.ptr, 4ull * n_test, hipMemcpyDeviceToDevice, st));
            *n_test0 = n_test;
        }
    }
    if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
    dm->counters_clean = reset_queued;
    dm->n_blocks = dm->h_cnt[kCntBlocks];
    S.voxel_updates += dm->h_cnt[kCntLeaves];
    S.train_reads = (uint64_t)dm->h_cnt[kCntTrainReads] | ((uint64_t)dm->h_cnt[kCntTrainReads + 1] << 32);
    S.pair_evals = (uint64_t)dm->h_cnt[kCntPairEvals] | ((uint64_t)dm->h_cnt[kCntPairEvals + 1] << 32);
    if (dm->stage_timing) S.t_commit += wall() - tp2;
    return LA3DM_OK;
}

// Stages B..G on the training set in dm->xy (partition, passes, deferred prune); t0 = start of the call.
static int scan_training_set(la3dm_devmap *dm, uint32_t flags, double t0, la3dm_devmap_stats *stats_out) {
    hipStream_t st = dm->ctx->stream;
    la3dm_devmap_stats &S = dm->stats;
    int rc;
    bool no_bbox = false;  // a NaN coordinate in the first training point: the reference's bbox is NaN, no block is visited
    for (int a = 0; a < 6 && dm->n_xy; ++a) no_bbox |= dm->h_bbox[a] != dm->h_bbox[a];
    if (dm->n_xy == 0 || no_bbox) {  // empty cloud, every hit beyond max_range, or no candidate blocks
        S.t_total = wall() - t0;
        if (stats_out) *stats_out = S;
        return LA3DM_OK;
    }
    const double t1 = wall();
    S.t_frontend = t1 - t0;
    ScanPlan P;
    P.flags = flags;
    if ((rc = partition(dm, P)) != LA3DM_OK) return rc;
    S.t_partition = wall() - t1;
    DM_RESERVE(dm->c_weight, 4ull * P.n_entries);
    const uint32_t max_occ = P.max_occ;
    uint32_t n_test0 = 0;
    for (uint32_t pass = 0; pass < max_occ; ++pass)
        if ((rc = run_pass(dm, P, pass, &n_test0)) != LA3DM_OK) {
            // run_pass is not failure-atomic: dm_table_insert may already have published new keys and bumped the device
            // block counter when a later step (arena growth, a sort, the scan) fails.  Adopt the device counter so that the
            // table, the pool (the new blocks get their default nodes here if the pass had not written them) and the host agree again — the map stays usable, the
            // scan is lost, as if the reference had thrown after creating its blocks.  If even that fails: poison.
            const std::string why = dm->ctx->err;
            uint32_t dev_blocks = 0;
            if (hipStreamSynchronize(st) == hipSuccess &&
                hipMemcpy(&dev_blocks, dm->d_cnt + kCntBlocks, 4, hipMemcpyDeviceToHost) == hipSuccess && dev_blocks <= dm->cap_blocks) {
                if (dev_blocks > dm->n_blocks) {
                    // the slots [old, new) may not have been initialised yet (their default nodes are written by the leaf-count
                    // launch, which the failed pass may never have reached): write them now, then adopt the count
                    hipLaunchKernelGGL(dm_pool_init, dim3(cdiv((size_t)(dev_blocks - dm->n_blocks) * dm->npb, 256)), dim3(256), 0, st, dm->A,
                                       dm->B, dm->S, dm->n_blocks, (const uint32_t *)(dm->d_cnt + kCntBlocks), dm->npb, dm->init_A, dm->init_B);
                    if (hipStreamSynchronize(st) == hipSuccess)
                        dm->n_blocks = dev_blocks;
                    else
                        dm->poisoned = true;
                }
            } else {
                dm->poisoned = true;
            }
            dm->ctx->err = why;
            return rc;
        }
    if (max_occ > 1 && n_test0)
        hipLaunchKernelGGL(dm_prune, dim3(cdiv(n_test0, 4)), dim3(256), 4 * prune_lds_stride(dm->npb), st,
                           (const uint32_t *)dm->t_slot0.ptr, n_test0, dm->A, dm->B, dm->S, dm->npb, dm->depth);
    DM_TRY(hipGetLastError());
    if (max_occ > 1) DM_TRY(hipStreamSynchronize(st));  // (single pass: the pass's own read-back was the last sync)
    S.n_blocks = dm->n_blocks;
    S.t_total = wall() - t0;
    if (!dm->stage_timing) S.t_pack = S.t_total - S.t_frontend - S.t_partition;  // pack + kernel + commit, unsplit
    if (stats_out) *stats_out = S;
    return LA3DM_OK;
}

// Start of an insert: the counter block at its initial values — by dm_begin, unless the insert before left it so (round 5).
static void begin_insert(la3dm_devmap *dm) {
    if (dm->counters_clean && dm->mailbox) {
        dm->counters_clean = false;
        return;
    }
    dm->counters_clean = false;
    hipLaunchKernelGGL(dm_begin, dim3(1), dim3(64), 0, dm->ctx->stream, dm->d_cnt, dm->n_blocks, dm->d_mm, dm->d_mm + 6);
}

// BGKOctoMap::insert_training_data (bgkoctomap.cpp:82-212) on the pool: n labelled points {x, y, z, label} (host
// pointer) instead of a scan; every leaf of every test block is updated for every neighbour model (no kbar gate).
int la3dm_devmap_insert_training_data_host(la3dm_devmap *dm, const float *xyzy, uint32_t n, la3dm_devmap_stats *stats_out) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (!dm || (n && !xyzy)) return LA3DM_ERR_ARG;
    la3dm_ctx *ctx = dm->ctx;
    if (ctx->p.variant == 3) return dm_fail(dm, LA3DM_ERR_ARG, "la3dm_devmap_insert_training_data: a BGK-L map needs beams, not labelled points");
    DM_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    la3dm_devmap_stats &S = dm->stats;
    memset(&S, 0, sizeof(S));
    S.n_blocks = dm->n_blocks;
    dm->insert_into_empty = dm->n_blocks == 0;
    dm->n_xy = 0;
    const double t0 = wall();
    begin_insert(dm);
    if (n == 0) {  // bgkoctomap.cpp:83-84
        if (stats_out) *stats_out = S;
        return LA3DM_OK;
    }
    DM_RESERVE(dm->xy, 16ull * n);
    DM_TRY(hipMemcpyAsync(dm->xy.ptr, xyzy, 16ull * n, hipMemcpyHostToDevice, st));
    dm->n_xy = n;
    for (uint32_t i = 0; i < n; ++i) (xyzy[4 * (size_t)i + 3] > 0.5f ? S.n_hits : S.n_frees)++;
    int rc = training_bbox(dm);
    if (rc != LA3DM_OK) return rc;
    return scan_training_set(dm, LA3DM_SCAN_UPDATE_UNGATED, t0, stats_out);
}

// ---- BGKLVOctoMap::insert_pointcloud on the pool (src/bgklvoctomap/bgklvoctomap.cpp:89-285; kernels and the map of
// the stages in devmap_lv_kernels.h).  The pool stores the host's State enum (PRUNED 3, UNCERTAIN 4), so download,
// search and prune are the BGK ones.  Read-backs: hit-grid cell count, beam totals, sample bbox, bucket bounds,
// packed-block count, counters at the end.
static int lv_insert(la3dm_devmap *dm, const float *d_xyz, uint32_t n, const float origin[3], float ds_resolution,
                     float free_resolution, float max_range, double t0) {
    la3dm_ctx *ctx = dm->ctx;
    hipStream_t st = ctx->stream;
    la3dm_devmap_lv_stats &L = dm->lv_stats;
    memset(&L, 0, sizeof(L));
    dm->lv_n_samples = dm->lv_n_rays = 0;
    int rc;
    if (ds_resolution > ctx->p.resolution) ds_resolution = ctx->p.resolution;  // bgklvoctomap.cpp:95-96
    // hits: voxel-grid filter (or the cloud itself)
    const float *d_hits = d_xyz;
    uint32_t nh = n;
    if (!(ds_resolution < 0)) {
        if ((rc = voxel_grid(dm, d_xyz, n, ds_resolution, dm->hits, &nh)) != LA3DM_OK) return rc;
        d_hits = (const float *)dm->hits.ptr;
    }
    if (nh == 0) return LA3DM_OK;
    LvBeamArgs ba;
    ba.ox = origin[0]; ba.oy = origin[1]; ba.oz = origin[2];
    ba.max_range = max_range;
    ba.free_res = free_resolution;
    ba.offset = (double)ctx->p.ell * pow(2, 0.5);
    ba.influence = (double)ctx->p.ell;
    DM_RESERVE(dm->lv_rng, 8ull * nh);
    DM_RESERVE(dm->lv_flags, nh);
    DM_RESERVE(dm->lv_seg, 24ull * nh);
    DM_RESERVE(dm->lv_nsamp, 4ull * nh);
    DM_RESERVE(dm->lv_nray, 4ull * nh);
    DM_RESERVE(dm->lv_samp_off, 4ull * nh);
    DM_RESERVE(dm->lv_ray_off, 4ull * nh);
    uint32_t *nsamp = (uint32_t *)dm->lv_nsamp.ptr, *nray = (uint32_t *)dm->lv_nray.ptr;
    uint32_t *samp_off = (uint32_t *)dm->lv_samp_off.ptr, *ray_off = (uint32_t *)dm->lv_ray_off.ptr;
    hipLaunchKernelGGL(dm_lv_ranges, dim3(cdiv(nh, 256)), dim3(256), 0, st, d_hits, nh, ba, (double *)dm->lv_rng.ptr);
    // ray shortening (bgklvoctomap.cpp:313-423).  Small scans (configs[3]'s 3 500-point clouds): the dense form — membership of
    // the "nearby" gather for all (beam, hit) pairs at once as an nh x nh bit matrix, then the ordered walk over the set bits,
    // hit list in LDS.  Larger scans: the same sets from a uniform grid over the hits, O(N k) in time and memory (round 6).
    // LA3DM_LV_NEAR=dense | grid forces one of them (the tests compare the two).
    const char *near_env = getenv("LA3DM_LV_NEAR");
    const bool force_dense = near_env && !strcmp(near_env, "dense"), force_grid = near_env && !strcmp(near_env, "grid");
    if (force_dense && nh > 98304u)
        return dm_fail(dm, LA3DM_ERR_ARG, "devmap (BGK-LV): LA3DM_LV_NEAR=dense needs nh^2 / 8 bytes of mask: at most 98 304 hits");
    DM_RESERVE(dm->lv_beam, sizeof(LvBeam) * (size_t)nh);
    hipLaunchKernelGGL(dm_lv_beam_init, dim3(cdiv(nh, 256)), dim3(256), 0, st, d_hits, nh, ba, (LvBeam *)dm->lv_beam.ptr);
    static const uint32_t kGridMin = getenv("LA3DM_LV_GRID_MIN") ? (uint32_t)std::max(1, atoi(getenv("LA3DM_LV_GRID_MIN"))) : 8192u;   // (A/B: hits from which the grid form runs)
    if (force_dense || (!force_grid && nh < kGridMin)) {
        const uint32_t nw = cdiv(nh, 64);
        DM_RESERVE(dm->lv_mask, 8ull * nh * nw);
        // (beams per workgroup: small scans need the parallelism — a tile is walked in sequence —, large ones the reuse of the wave's 64 hits)
        const bool small_scan = nh < 16384u;
        const uint32_t near_tile = small_scan ? 32u : kLvNearTile;
        if (small_scan)
            hipLaunchKernelGGL(dm_lv_nearby<true>, dim3(nw, cdiv(nh, near_tile)), dim3(64), 0, st, d_hits, nh, ba, (const double *)dm->lv_rng.ptr,
                               (const LvBeam *)dm->lv_beam.ptr, (unsigned long long *)dm->lv_mask.ptr, near_tile);
        else
            hipLaunchKernelGGL(dm_lv_nearby<false>, dim3(nw, cdiv(nh, near_tile)), dim3(64), 0, st, d_hits, nh, ba, (const double *)dm->lv_rng.ptr,
                               (const LvBeam *)dm->lv_beam.ptr, (unsigned long long *)dm->lv_mask.ptr, near_tile);
        const int lds_hits = 12ull * nh <= 60000 ? 1 : 0;   // the hit list in LDS (2 workgroups per CU still fit)
        const uint32_t walk_threads = lds_hits ? 256u : 64u;   // (the staged hit list is shared by the workgroup's four waves)
        hipLaunchKernelGGL(dm_lv_beams_walk, dim3(cdiv(nh, walk_threads)), dim3(walk_threads), lds_hits ? 12 * nh : 0, st, d_hits, nh, ba,
                           (const LvBeam *)dm->lv_beam.ptr, (const unsigned long long *)dm->lv_mask.ptr, nw, (uint8_t *)dm->lv_flags.ptr,
                           (float *)dm->lv_seg.ptr, nsamp, nray, dm->d_cnt, lds_hits);
    } else {
        const double *rng = (const double *)dm->lv_rng.ptr;
        const LvBeam *beams = (const LvBeam *)dm->lv_beam.ptr;
        // 1. the grid: cells of edge `influence` around the sensor.  With a range gate every hit that can be nearby at all lies within
        //    max_range of the sensor, so the grid's extent is known here; without one, the bounds of the hits come from a reduction and
        //    one counter read-back
        int32_t hmm[7] = {0, 0, 0, 0, 0, 0, 1};
        const double reach = max_range > 0 ? ceil((double)max_range / ba.influence) + 1.0 : 0.0;
        if (max_range > 0 && reach < 1.0e6) {
            hmm[0] = hmm[1] = hmm[2] = -(int32_t)reach;
            hmm[3] = hmm[4] = hmm[5] = (int32_t)reach;
        } else {
            hipLaunchKernelGGL(dm_lv_hit_bounds, dim3(std::min<uint32_t>(cdiv(nh, 256), kMinmaxWgs)), dim3(256), 0, st, d_hits, nh, ba, rng, dm->d_cnt);
            if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
            if (dm->h_cnt[kCntError] & kErrLvExtent) return dm_fail(dm, LA3DM_ERR_ARG, "devmap (BGK-LV): hit coordinates beyond the ray-shortening grid's index range");
            memcpy(hmm, dm->h_cnt + kCntLvHmm, 28);
            if (hmm[6] == 0) hmm[0] = hmm[1] = hmm[2] = hmm[3] = hmm[4] = hmm[5] = 0;   // no hit in range: one empty cell
        }
        LvHitGrid G;
        uint64_t ncell = 0;
        for (int m = 1;; m *= 2) {   // coarser cells while the dense grid would need more than 2^24 of them
            ncell = 1;
            for (int a = 0; a < 3; ++a) {
                G.dim[a] = (int32_t)(((int64_t)hmm[3 + a] - hmm[a]) / m + 1);
                ncell *= (uint64_t)G.dim[a];
            }
            G.cell = ba.influence * m;
            if (ncell <= (1ull << 24)) break;
        }
        G.g0[0] = (double)ba.ox + (double)hmm[0] * ba.influence;
        G.g0[1] = (double)ba.oy + (double)hmm[1] * ba.influence;
        G.g0[2] = (double)ba.oz + (double)hmm[2] * ba.influence;
        DM_RESERVE(dm->lv_hcell, 4ull * nh);
        DM_RESERVE(dm->lv_hlist, 4ull * nh);
        DM_RESERVE(dm->lv_hcnt, 4ull * (ncell + 1));
        DM_RESERVE(dm->lv_hoff, 4ull * (ncell + 1));
        uint32_t *hcnt = (uint32_t *)dm->lv_hcnt.ptr, *hoff = (uint32_t *)dm->lv_hoff.ptr;
        DM_TRY(hipMemsetAsync(hcnt, 0, 4ull * (ncell + 1), st));
        hipLaunchKernelGGL(dm_lv_hgrid_count, dim3(cdiv(nh, 256)), dim3(256), 0, st, d_hits, nh, ba, rng, G, (uint32_t *)dm->lv_hcell.ptr, hcnt);
        if ((rc = exclusive_scan(dm, hcnt, hoff, (uint32_t)ncell + 1)) != LA3DM_OK) return rc;
        DM_TRY(hipMemsetAsync(hcnt, 0, 4ull * (ncell + 1), st));
        hipLaunchKernelGGL(dm_lv_hgrid_fill, dim3(cdiv(nh, 256)), dim3(256), 0, st, (const uint32_t *)dm->lv_hcell.ptr, nh, (const uint32_t *)hoff, hcnt,
                           (uint32_t *)dm->lv_hlist.ptr);
        // 2. every beam in one wave: capsule walk, nearby hits collected and sorted in LDS, the ordered shortening (dm_lv_beams_grid)
        hipLaunchKernelGGL(dm_lv_beams_grid, dim3(cdiv(nh, kLvGridWaves)), dim3(64 * kLvGridWaves), 0, st, d_hits, nh, ba, rng, beams, G,
                           (const uint32_t *)hoff, (const uint32_t *)dm->lv_hlist.ptr, (uint8_t *)dm->lv_flags.ptr, (float *)dm->lv_seg.ptr, nsamp, nray,
                           dm->d_cnt);
        hipLaunchKernelGGL(dm_lv_beam_totals, dim3(std::min<uint32_t>(cdiv(nh, 256), kMinmaxWgs)), dim3(256), 0, st, (const uint32_t *)nsamp,
                           (const uint8_t *)dm->lv_flags.ptr, nh, dm->d_cnt);
        if (getenv("LA3DM_DEBUG_LV")) fprintf(stderr, "la3dm BGK-LV ray shortening on the hit grid: %u hits, %d x %d x %d cells of %.3f m\n", nh, G.dim[0], G.dim[1], G.dim[2], G.cell);
    }
    if ((rc = exclusive_scan(dm, nsamp, samp_off, nh, (int)kCntFreeRaw)) != LA3DM_OK) return rc;
    if ((rc = exclusive_scan(dm, nray, ray_off, nh, (int)kCntKept, true)) != LA3DM_OK) return rc;
    if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
    if ((rc = check_beam_counters(dm)) != LA3DM_OK) return rc;
    const uint32_t ns = dm->h_cnt[kCntFreeRaw], n_rays = dm->h_cnt[kCntKept];
    L.n_rays = n_rays;
    L.n_samples = ns;
    if (ns == 0) return LA3DM_OK;
    DM_RESERVE(dm->lv_samples, 16ull * ns);
    DM_RESERVE(dm->lv_rays, 32ull * (n_rays ? n_rays : 1));
    float4 *samples = (float4 *)dm->lv_samples.ptr;
    hipLaunchKernelGGL(dm_lv_emit, dim3(cdiv(nh, 256)), dim3(256), 0, st, d_hits, nh, ba, (const uint8_t *)dm->lv_flags.ptr,
                       (const float *)dm->lv_seg.ptr, (const uint32_t *)samp_off, (const uint32_t *)ray_off, samples,
                       (float4 *)dm->lv_rays.ptr);
    dm->lv_n_samples = ns;
    dm->lv_n_rays = n_rays;
    L.n_hits = dm->h_cnt[kCntTrained];
    // bounding box of ALL samples (std::min / std::max chains from samples[0]: bgklvoctomap.cpp:105-112)
    {
        MinmaxFin fin = {2, 0.0f, nullptr, (const float *)samples, dm->d_cnt, dm->d_mm + 6, nullptr};
        hipLaunchKernelGGL(dm_minmax<4>, dim3(std::min<uint32_t>(cdiv(ns, 1024), kMinmaxWgs)), dim3(256), 0, st, (const float *)samples, ns, dm->d_mm, fin);
    }
    // bucket bounds of the finite samples
    const int depth = ctx->p.block_depth;
    const float bs = dm->block_size;
    const double g = depth >= 3 ? 4.0 * (double)ctx->p.resolution : (double)bs;
    const double half = 0.5 * (double)bs;
    // (the bounds live in the counter block — initialised by dm_begin, read back with it)
    hipLaunchKernelGGL(dm_lv_cell_bounds, dim3(std::min<uint32_t>(cdiv(ns, 256), kMinmaxWgs)), dim3(256), 0, st, (const float4 *)samples, ns, half, g,
                       (int32_t *)(dm->d_cnt + kCntLvmm), dm->d_cnt);
    if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
    memcpy(dm->h_bbox, dm->h_cnt + kCntBbox, sizeof(float) * 6);
    memcpy(dm->h_lvmm, dm->h_cnt + kCntLvmm, 28);
    if (dm->h_cnt[kCntError] & kErrLvExtent) return dm_fail(dm, LA3DM_ERR_ARG, "devmap (BGK-LV): sample coordinates beyond the gather grid's index range");
    for (int a = 0; a < 6; ++a)
        if (dm->h_bbox[a] != dm->h_bbox[a]) return LA3DM_OK;  // NaN box (first sample not finite): no candidate block, as on the host
    const uint32_t n_binned = (uint32_t)dm->h_lvmm[6];
    if (n_binned == 0) return LA3DM_OK;
    LvGridArgs ga;
    ga.g = g;
    ga.half = half;
    size_t ncell = 1;
    for (int a = 0; a < 3; ++a) {
        ga.cmin[a] = dm->h_lvmm[a];
        ga.cdim[a] = dm->h_lvmm[3 + a] - dm->h_lvmm[a] + 1;
        ncell *= (size_t)ga.cdim[a];
    }
    if (ncell > ((size_t)1 << 28)) return dm_fail(dm, LA3DM_ERR_ARG, "devmap (BGK-LV): scan extent too large for the dense gather grid");
    // candidate blocks: per-axis float-stepped sequences (host, a few dozen values), distinct indices + multiplicities
    std::vector<int32_t> ax_idx[3];
    std::vector<uint32_t> ax_mult[3];
    uint32_t max_mult = 1;
    size_t n_cand = 1, n_bbox = 1;
    for (int a = 0; a < 3; ++a) {
        std::vector<int> seq = axis_sequence(dm->h_bbox[a], dm->h_bbox[3 + a], bs);
        if (seq.empty() || seq.size() > (1u << 20)) return dm_fail(dm, LA3DM_ERR_ARG, "devmap: degenerate training-set extent");
        n_bbox *= seq.size();
        std::sort(seq.begin(), seq.end());
        uint32_t mm = 1;
        for (size_t i = 0; i < seq.size();) {
            size_t j = i;
            while (j < seq.size() && seq[j] == seq[i]) ++j;
            ax_idx[a].push_back(seq[i]);
            ax_mult[a].push_back((uint32_t)(j - i));
            mm = std::max(mm, (uint32_t)(j - i));
            i = j;
        }
        max_mult *= mm;
        n_cand *= ax_idx[a].size();
    }
    if (n_cand > (1u << 26)) return dm_fail(dm, LA3DM_ERR_ARG, "devmap (BGK-LV): more than 2^26 candidate blocks (set max_range)");
    L.n_bbox_blocks = n_bbox;
    // gather grid: stable sort of the samples by bucket, CSR over the dense grid
    DM_RESERVE(dm->k0, 4ull * ns);
    DM_RESERVE(dm->k1, 4ull * ns);
    DM_RESERVE(dm->v0, 4ull * ns);
    DM_RESERVE(dm->v1, 4ull * ns);
    DM_RESERVE(dm->lv_sorted, 16ull * ns);
    DM_RESERVE(dm->lv_cell_off, 4ull * (ncell + 1));
    uint32_t *k0 = (uint32_t *)dm->k0.ptr, *k1 = (uint32_t *)dm->k1.ptr, *v0 = (uint32_t *)dm->v0.ptr, *v1 = (uint32_t *)dm->v1.ptr;
    hipLaunchKernelGGL(dm_lv_cell_keys, dim3(cdiv(ns, 256)), dim3(256), 0, st, (const float4 *)samples, ns, ga, (uint32_t)ncell, k0, v0);
    int key_bits = 1;
    while (((size_t)1 << key_bits) <= ncell) ++key_bits;
    if ((rc = sort_pairs(dm, k0, k1, v0, v1, ns, key_bits)) != LA3DM_OK) return rc;
    hipLaunchKernelGGL(dm_lv_sorted, dim3(cdiv(ns, 256)), dim3(256), 0, st, (const float4 *)samples, (const uint32_t *)v1, ns, (float4 *)dm->lv_sorted.ptr);
    hipLaunchKernelGGL(dm_lv_cell_off, dim3(cdiv((uint32_t)ncell + 1, 256)), dim3(256), 0, st, (const uint32_t *)k1, ns, (uint32_t)ncell,
                       (uint32_t *)dm->lv_cell_off.ptr);
    // candidates: keys (ascending), multiplicities, "has a sample within reach"; every candidate block is created
    {
        size_t bytes = 0;
        for (int a = 0; a < 3; ++a) bytes += 8 * ax_idx[a].size();
        DM_RESERVE(dm->lv_axis, bytes);
    }
    LvCandArgs ca;
    {
        // one upload from a staging vector that lives as long as the map (no synchronisation for the host buffers' sake)
        size_t bytes = 0;
        for (int a = 0; a < 3; ++a) bytes += 8 * ax_idx[a].size();
        dm->lv_axis_host.resize(bytes);
        uint8_t *base = (uint8_t *)dm->lv_axis.ptr, *hb = dm->lv_axis_host.data();
        size_t o = 0;
        for (int a = 0; a < 3; ++a) {
            const size_t m = ax_idx[a].size();
            memcpy(hb + o, ax_idx[a].data(), 4 * m);
            ca.idx[a] = (const int32_t *)(base + o);
            o += 4 * m;
            memcpy(hb + o, ax_mult[a].data(), 4 * m);
            ca.mult[a] = (const uint32_t *)(base + o);
            o += 4 * m;
            ca.n[a] = (uint32_t)m;
            ca.cmin[a] = ga.cmin[a];
            ca.cdim[a] = ga.cdim[a];
        }
        DM_TRY(hipMemcpyAsync(base, hb, bytes, hipMemcpyHostToDevice, st));
    }
    ca.block_size = bs;
    ca.g = g;
    ca.reach = (int32_t)std::ceil((double)ctx->p.ell / g);
    ca.bpb = depth >= 3 ? (1 << (depth - 3)) : 1;
    const uint32_t nc = (uint32_t)n_cand;
    DM_RESERVE(dm->lv_keys, 8ull * nc);
    DM_RESERVE(dm->lv_mult, 4ull * nc);
    DM_RESERVE(dm->lv_flag, 4ull * nc);
    DM_RESERVE(dm->lv_pos, 4ull * nc);
    DM_RESERVE(dm->lv_slot, 4ull * nc);
    hipLaunchKernelGGL(dm_lv_candidates, dim3(cdiv(nc, 256)), dim3(256), 0, st, ca, nc, (const uint32_t *)dm->lv_cell_off.ptr,
                       (long long *)dm->lv_keys.ptr, (uint32_t *)dm->lv_mult.ptr, (uint32_t *)dm->lv_flag.ptr, dm->d_cnt);
    if ((rc = grow_pool(dm, (size_t)dm->n_blocks + nc)) != LA3DM_OK) return rc;
    if ((rc = grow_table(dm, (size_t)dm->n_blocks + nc)) != LA3DM_OK) return rc;
    hipLaunchKernelGGL(dm_table_insert, dim3(cdiv(nc, 256)), dim3(256), 0, st, (const long long *)dm->lv_keys.ptr, dm->d_cnt, dm->tab_key,
                       dm->tab_val, dm->tab_cap - 1, dm->d_cnt + kCntBlocks, dm->blk_key, (uint32_t *)dm->lv_slot.ptr);
    hipLaunchKernelGGL(dm_pool_init, dim3(cdiv((size_t)nc * dm->npb, 256)), dim3(256), 0, st, dm->A, dm->B, dm->S, dm->n_blocks,
                       (const uint32_t *)(dm->d_cnt + kCntBlocks), dm->npb, dm->init_A, dm->init_B);
    if ((rc = exclusive_scan(dm, (const uint32_t *)dm->lv_flag.ptr, (uint32_t *)dm->lv_pos.ptr, nc)) != LA3DM_OK) return rc;
    DM_RESERVE(dm->lv_center, 12ull * nc);
    DM_RESERVE(dm->lv_cell0, 12ull * nc);
    DM_RESERVE(dm->lv_pslot, 4ull * nc);
    DM_RESERVE(dm->lv_pmult, 4ull * nc);
    DM_RESERVE(dm->lv_info, 4ull * nc);
    DM_RESERVE(dm->lv_prune, 4ull * nc);
    hipLaunchKernelGGL(dm_lv_pack, dim3(cdiv(nc, 256)), dim3(256), 0, st, (const long long *)dm->lv_keys.ptr, (const uint32_t *)dm->lv_mult.ptr,
                       (const uint32_t *)dm->lv_flag.ptr, (const uint32_t *)dm->lv_pos.ptr, (const uint32_t *)dm->lv_slot.ptr, nc, bs, g,
                       (float *)dm->lv_center.ptr, (int32_t *)dm->lv_cell0.ptr, (uint32_t *)dm->lv_pslot.ptr, (uint32_t *)dm->lv_pmult.ptr,
                       dm->d_cnt, (uint32_t *)dm->lv_info.ptr);
    // (d_cnt[kCntLeaves] counts the voxel updates of all passes, d_cnt[kCntGeo] the blocks with information: zero since
    // dm_begin, nothing before this point of a BGK-LV insert touches them)
    // work plan of the voxel kernel for at most nc packed blocks (the kernel itself stops at the packed count, which is
    // still on the device): its totals come back with the counters below
    la3dm_lv_pool_scan ps;
    memset(&ps, 0, sizeof(ps));
    ps.n_samples = ns;
    ps.samples = (const float *)samples;
    ps.sorted = (const float *)dm->lv_sorted.ptr;
    ps.rays = (const float *)dm->lv_rays.ptr;
    ps.cell_off = (const uint32_t *)dm->lv_cell_off.ptr;
    for (int a = 0; a < 3; ++a) {
        ps.cell_min[a] = ga.cmin[a];
        ps.cell_dim[a] = ga.cdim[a];
    }
    ps.blk_center = (const float *)dm->lv_center.ptr;
    ps.blk_cell0 = (const int32_t *)dm->lv_cell0.ptr;
    ps.blk_slot = (const uint32_t *)dm->lv_pslot.ptr;
    ps.blk_mult = (const uint32_t *)dm->lv_pmult.ptr;
    ps.A = dm->A;
    ps.B = dm->B;
    ps.S = dm->S;
    ps.npb = dm->npb;
    ps.upd_counter = dm->d_cnt + kCntLeaves;
    ps.n_blk = ps.plan_n_blk = nc;
    ps.n_blk_dev = dm->d_cnt + kCntTest;
    if ((rc = la3dm_bgklv_pool_plan_device(ctx, &ps, dm->d_cnt + kCntLvPlan, st)) != LA3DM_OK) return rc;
    if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
    dm->n_blocks = dm->h_cnt[kCntBlocks];
    const uint32_t n_packed = dm->h_cnt[kCntTest];
    L.n_packed_blocks = n_packed;
    L.voxels = (uint64_t)n_packed << (3 * (depth - 1));
    const double t1 = wall();
    if (n_packed) {
        ps.n_blk = n_packed;
        for (int a = 0; a < 4; ++a) ps.plan_totals[a] = dm->h_cnt[kCntLvPlan + a];
        ps.plan_totals_dev = dm->d_cnt + kCntLvPlan;
        const uint32_t layer_n = 1u << (3 * (depth - 1)), layer_off = dm->npb - layer_n;
        for (uint32_t pass = 0; pass < max_mult; ++pass) {  // a key the float-stepped loop repeats is visited again, serially
            ps.pass = pass;
            if ((rc = la3dm_bgklv_pool_scan_device(ctx, &ps, st)) != LA3DM_OK) return rc;
            hipLaunchKernelGGL(dm_lv_finish, dim3(cdiv(n_packed, 4)), dim3(256), 0, st, (const uint32_t *)dm->lv_pslot.ptr,
                               (const uint32_t *)dm->lv_pmult.ptr, n_packed, pass, dm->S, dm->npb, layer_off, layer_n,
                               (uint32_t *)dm->lv_info.ptr);
        }
        hipLaunchKernelGGL(dm_lv_prune_list, dim3(cdiv(n_packed, 256)), dim3(256), 0, st, (const uint32_t *)dm->lv_pslot.ptr,
                           (const uint32_t *)dm->lv_info.ptr, n_packed, (uint32_t *)dm->lv_prune.ptr, dm->d_cnt);
        if (dm->lv_original_size)
            hipLaunchKernelGGL(dm_prune, dim3(cdiv(n_packed, 4)), dim3(256), 4 * prune_lds_stride(dm->npb), st,
                               (const uint32_t *)dm->lv_prune.ptr, n_packed, dm->A, dm->B, dm->S, dm->npb, dm->depth);
        DM_TRY(hipGetLastError());
        if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
        L.voxel_updates = dm->h_cnt[kCntLeaves];
        L.n_info_blocks = dm->h_cnt[kCntGeo];
    }
    L.n_blocks = dm->n_blocks;
    L.t_frontend = t1 - t0;
    L.t_total = wall() - t0;
    return LA3DM_OK;
}

// Argument checks shared by the insert entry points.  The beam sampler walks `for (d = fr; d < l; d += fr)` on the GPU
// (bgkoctomap.cpp:445-457): a free_resolution that is not a positive finite number would never terminate there (the
// reference would run out of memory on the host instead), so it is rejected here; so are NaN resolutions / ranges and a
// non-finite sensor origin.  Non-finite points of the cloud itself are dropped by the front end's range gate.
static int check_scan_args(la3dm_devmap *dm, const float origin[3], float ds_resolution, float free_resolution, float max_range) {
    if (dm->poisoned)
        return dm_fail(dm, LA3DM_ERR_HIP, "devmap: an earlier insert failed in a way that left the block table unusable; destroy the map");
    if (!(free_resolution > 0.0f) || !std::isfinite(free_resolution))
        return dm_fail(dm, LA3DM_ERR_ARG, "insert_pointcloud: free_resolution must be a positive finite number");
    if (ds_resolution != ds_resolution || std::isinf(ds_resolution) || ds_resolution == 0.0f)
        return dm_fail(dm, LA3DM_ERR_ARG, "insert_pointcloud: ds_resolution must be finite and non-zero (negative = no voxel filter)");
    if (max_range != max_range)
        return dm_fail(dm, LA3DM_ERR_ARG, "insert_pointcloud: max_range is NaN");
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(origin[i])) return dm_fail(dm, LA3DM_ERR_ARG, "insert_pointcloud: the sensor origin is not finite");
    return LA3DM_OK;
}

// after a failed BGK-LV insert: the candidate blocks may already be in the table (see scan_training_set)
static void lv_recover(la3dm_devmap *dm) {
    const std::string why = dm->ctx->err;
    uint32_t dev_blocks = 0;
    if (hipStreamSynchronize(dm->ctx->stream) == hipSuccess &&
        hipMemcpy(&dev_blocks, dm->d_cnt + kCntBlocks, 4, hipMemcpyDeviceToHost) == hipSuccess && dev_blocks <= dm->cap_blocks) {
        if (dev_blocks > dm->n_blocks) dm->n_blocks = dev_blocks;
    } else {
        dm->poisoned = true;
    }
    dm->ctx->err = why;
}

int la3dm_devmap_lv_stats_get(la3dm_devmap *dm, la3dm_devmap_lv_stats *out) {
    if (!dm || !out) return LA3DM_ERR_ARG;
    *out = dm->lv_stats;
    return LA3DM_OK;
}

int la3dm_devmap_lv_set_original_size(la3dm_devmap *dm, int original_size) {
    if (!dm) return LA3DM_ERR_ARG;
    dm->lv_original_size = original_size != 0;
    return LA3DM_OK;
}

int la3dm_devmap_lv_training(la3dm_devmap *dm, float *samples4, uint32_t cap_samples, float *rays6, uint32_t cap_rays,
                             uint32_t *n_samples, uint32_t *n_rays) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (!dm) return LA3DM_ERR_ARG;
    if (n_samples) *n_samples = dm->lv_n_samples;
    if (n_rays) *n_rays = dm->lv_n_rays;
    if (!samples4 && !rays6) return LA3DM_OK;
    if ((samples4 && cap_samples < dm->lv_n_samples) || (rays6 && cap_rays < dm->lv_n_rays)) return dm_fail(dm, LA3DM_ERR_ARG, "la3dm_devmap_lv_training: buffer too small");
    DM_TRY(hipSetDevice(dm->ctx->device));
    hipStream_t st = dm->ctx->stream;
    if (samples4 && dm->lv_n_samples)
        DM_TRY(hipMemcpyAsync(samples4, dm->lv_samples.ptr, 16ull * dm->lv_n_samples, hipMemcpyDeviceToHost, st));
    std::vector<float> r8;
    if (rays6 && dm->lv_n_rays) {
        r8.resize(8ull * dm->lv_n_rays);
        DM_TRY(hipMemcpyAsync(r8.data(), dm->lv_rays.ptr, 32ull * dm->lv_n_rays, hipMemcpyDeviceToHost, st));
    }
    DM_TRY(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < (rays6 ? dm->lv_n_rays : 0u); ++i) {
        rays6[6 * i] = r8[8 * i]; rays6[6 * i + 1] = r8[8 * i + 1]; rays6[6 * i + 2] = r8[8 * i + 2];
        rays6[6 * i + 3] = r8[8 * i + 4]; rays6[6 * i + 4] = r8[8 * i + 5]; rays6[6 * i + 5] = r8[8 * i + 6];
    }
    return LA3DM_OK;
}

int la3dm_devmap_wait_event(la3dm_devmap *dm, void *event) {
    if (!dm || !event) return LA3DM_ERR_ARG;
    DM_TRY(hipSetDevice(dm->ctx->device));
    DM_TRY(hipStreamWaitEvent(dm->ctx->stream, (hipEvent_t)event, 0));
    return LA3DM_OK;
}

int la3dm_devmap_set_shard(la3dm_devmap *dm, uint32_t rank, uint32_t world, la3dm_allgatherv_fn fn, void *user) {
    if (!dm) return LA3DM_ERR_ARG;
    if (world == 0 || world > 1023 || rank >= world || (world > 1 && !fn))
        return dm_fail(dm, LA3DM_ERR_ARG, "la3dm_devmap_set_shard: need rank < world <= 1023 and a callback when world > 1");
    if (world > 1 && dm->ctx->p.variant != 0 && dm->ctx->p.variant != 1)
        return dm_fail(dm, LA3DM_ERR_ARG, "la3dm_devmap_set_shard: block sharding is built for BGKOctoMap and GPOctoMap contexts");
    DM_TRY(hipSetDevice(dm->ctx->device));
    if (dm->h_shard) {
        (void)hipHostFree(dm->h_shard);
        dm->h_shard = nullptr;
    }
    if (world > 1) {
        DM_TRY(hipHostMalloc((void **)&dm->h_shard, 8ull * (world + 1)));
        // the status / count exchange buffer of every insert, every slot preset to "failed"
        int rc = arena_reserve(dm->ctx, dm->shard_cnt, 4ull * world);
        if (rc != LA3DM_OK) return dm_fail(dm, rc, "la3dm_devmap_set_shard: " + dm->ctx->err);
        DM_TRY(hipMemset(dm->shard_cnt.ptr, 0xFF, 4ull * world));
    }
    dm->shard_rank = rank;
    dm->shard_world = world;
    dm->shard_fn = world > 1 ? fn : nullptr;
    dm->shard_user = user;
    return LA3DM_OK;
}

int la3dm_devmap_insert_pointcloud_device(la3dm_devmap *dm, const float *d_xyz, uint32_t n, const float origin[3],
                                          float ds_resolution, float free_resolution, float max_range,
                                          la3dm_devmap_stats *stats_out) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (!dm || !origin || (n && !d_xyz)) return LA3DM_ERR_ARG;
    la3dm_ctx *ctx = dm->ctx;
    int rc;
    if ((rc = check_scan_args(dm, origin, ds_resolution, free_resolution, max_range)) != LA3DM_OK) return rc;
    DM_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    la3dm_devmap_stats &S = dm->stats;
    memset(&S, 0, sizeof(S));
    S.n_blocks = dm->n_blocks;
    dm->insert_into_empty = dm->n_blocks == 0;
    dm->n_xy = 0;
    const double t0 = wall();
    begin_insert(dm);
    if (ctx->p.variant == 2) {
        rc = lv_insert(dm, d_xyz, n, origin, ds_resolution, free_resolution, max_range, t0);
        if (rc != LA3DM_OK) lv_recover(dm);
        S.n_blocks = dm->n_blocks;
        if (stats_out) *stats_out = S;
        return rc;
    }

    if ((rc = front_end(dm, d_xyz, n, origin, ds_resolution, free_resolution, max_range)) != LA3DM_OK) return rc;
    return scan_training_set(dm, LA3DM_SCAN_LABELS_01, t0, stats_out);  // the front end labels hits 1.0f and free samples 0.0f
}

int la3dm_devmap_insert_pointcloud_host(la3dm_devmap *dm, const float *xyz, uint32_t n, uint32_t stride, const float origin[3],
                                        float ds_resolution, float free_resolution, float max_range,
                                        la3dm_devmap_stats *stats_out) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (!dm || (n && !xyz) || stride < 3) return LA3DM_ERR_ARG;
    DM_TRY(hipSetDevice(dm->ctx->device));
    DM_RESERVE(dm->cloud, 12ull * n);
    if (n) {
        if (stride == 3) {
            DM_TRY(hipMemcpyAsync(dm->cloud.ptr, xyz, 12ull * n, hipMemcpyHostToDevice, dm->ctx->stream));
        } else {
            DM_TRY(hipMemcpy2DAsync(dm->cloud.ptr, 12, xyz, 4ull * stride, 12, n, hipMemcpyHostToDevice, dm->ctx->stream));
        }
    }
    return la3dm_devmap_insert_pointcloud_device(dm, (const float *)dm->cloud.ptr, n, origin, ds_resolution, free_resolution,
                                                 max_range, stats_out);
}

int la3dm_devmap_block_count(la3dm_devmap *dm, uint32_t *n_blocks, uint32_t *nodes_per_block) {
    if (!dm) return LA3DM_ERR_ARG;
    if (n_blocks) *n_blocks = dm->n_blocks;
    if (nodes_per_block) *nodes_per_block = dm->npb;
    return LA3DM_OK;
}

int la3dm_devmap_download(la3dm_devmap *dm, int64_t *keys, float *A, float *B, uint8_t *S) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (!dm) return LA3DM_ERR_ARG;
    if (dm->n_blocks == 0) return LA3DM_OK;
    if (!keys || !A || !B || !S) return LA3DM_ERR_ARG;
    DM_TRY(hipSetDevice(dm->ctx->device));
    hipStream_t st = dm->ctx->stream;
    const size_t nn = (size_t)dm->n_blocks * dm->npb;
    DM_TRY(hipMemcpyAsync(keys, dm->blk_key, 8ull * dm->n_blocks, hipMemcpyDeviceToHost, st));
    DM_TRY(hipMemcpyAsync(A, dm->A, 4 * nn, hipMemcpyDeviceToHost, st));
    DM_TRY(hipMemcpyAsync(B, dm->B, 4 * nn, hipMemcpyDeviceToHost, st));
    DM_TRY(hipMemcpyAsync(S, dm->S, nn, hipMemcpyDeviceToHost, st));
    DM_TRY(hipStreamSynchronize(st));
    return LA3DM_OK;
}

// ---- what the queries' entry points share -----------------------------------------------------------------------
// Every query has a device-pointer and a host-pointer form with one body, X_query(dm, host, who, ...): the checks, the
// constant answer of an empty map (Fill), the staging of the caller's arrays (Stage), X_launch, the copies back.
#define DM_OK(expr)                        \
    do {                                   \
        int rc_ = (expr);                  \
        if (rc_ != LA3DM_OK) return rc_;   \
    } while (0)

extern "C++" {   // (member templates, inside the C ABI's block)
namespace {
struct RegionGeom {
    uint32_t g0[3], dims[3];
    uint64_t total;   // box: voxels; columns: columns
    la3dm_region_info info;
};

// The device twins of a query's arrays.  in() and out() register an array by the variable that holds the caller's pointer;
// reserve() sums the sizes, every array aligned to 16 bytes (the widest store of a query kernel), reserves `cloud` for
// the inputs and `q_out` for the outputs once each — an arena may move when it grows, hence after every registration —,
// points the variables at the twins and uploads the inputs; download() queues the copies of the outputs back.  A null
// pointer or a count of 0 gives a null twin and takes no room.  Device-pointer form (host = false): the caller's pointers
// are the device pointers, nothing is reserved or copied.
struct Stage {
    struct Item {
        void *slot;     // the registered variable (a pointer of any type)
        void *caller;   // what it held
        size_t bytes, elem;
        bool is_out;
    };
    la3dm_devmap *dm;
    bool host;
    int n_items = 0;
    Item item[16];
    Stage(la3dm_devmap *dm_, bool host_) : dm(dm_), host(host_) {}
    template <class T>
    int in(const T *&p, size_t count) { return add(&p, (void *)p, count, sizeof(T), false); }
    template <class T>
    int out(T *&p, size_t count) { return add(&p, p, count, sizeof(T), true); }
    int add(void *slot, void *caller, size_t count, size_t elem, bool is_out) {
        if (!host) return -1;
        assert(n_items < 16);
        item[n_items] = Item{slot, caller, caller ? count * elem : 0, elem, is_out};
        return n_items++;
    }
    // fewer elements to copy back than were given room, known only after the launch; i = what out() returned
    void count(int i, size_t n) {
        if (i >= 0) item[i].bytes = std::min(item[i].bytes, n * item[i].elem);
    }
    int reserve() {
        size_t total[2] = {0, 0};
        for (int i = 0; i < n_items; ++i) total[item[i].is_out] += (item[i].bytes + 15) & ~(size_t)15;
        if (total[0]) DM_RESERVE(dm->cloud, total[0]);
        if (total[1]) DM_RESERVE(dm->q_out, total[1]);
        size_t at[2] = {0, 0};
        for (int i = 0; i < n_items; ++i) {
            const Item &it = item[i];
            Arena &arena = it.is_out ? dm->q_out : dm->cloud;
            void *twin = it.bytes ? (char *)arena.ptr + at[it.is_out] : nullptr;
            at[it.is_out] += (it.bytes + 15) & ~(size_t)15;
            memcpy(it.slot, &twin, sizeof(twin));
            if (it.bytes && !it.is_out) DM_TRY(hipMemcpyAsync(twin, it.caller, it.bytes, hipMemcpyHostToDevice, dm->ctx->stream));
        }
        return LA3DM_OK;
    }
    int download() {
        for (int i = 0; i < n_items; ++i) {
            const Item &it = item[i];
            if (!it.is_out || !it.bytes) continue;
            void *twin;
            memcpy(&twin, it.slot, sizeof(twin));
            DM_TRY(hipMemcpyAsync(it.caller, twin, it.bytes, hipMemcpyDeviceToHost, dm->ctx->stream));
        }
        return LA3DM_OK;
    }
};

// The constant answer of an empty map, written without a launch: host memory directly, device memory by memsets on the
// map's stream.  A null array is left out.
struct Fill {
    la3dm_devmap *dm;
    bool host;
    int bytes(void *p, int value, size_t n) const {
        if (!p) return LA3DM_OK;
        if (host)
            memset(p, value, n);
        else
            DM_TRY(hipMemsetAsync(p, value, n, dm->ctx->stream));
        return LA3DM_OK;
    }
    int words(void *p, uint32_t value, size_t n) const {   // n 32-bit words
        if (!p) return LA3DM_OK;
        if (host)
            for (size_t i = 0; i < n; ++i) memcpy((char *)p + 4 * i, &value, 4);
        else
            DM_TRY(hipMemsetD32Async((hipDeviceptr_t)p, (int)value, n, dm->ctx->stream));
        return LA3DM_OK;
    }
    // p[i * stride] = value for i < n, in memory that holds zeros (device: byte by byte down the column of rows, the
    // non-zero bytes only)
    int strided(uint32_t *p, uint32_t value, size_t stride, size_t n) const {
        if (host) {
            for (size_t i = 0; i < n; ++i) p[i * stride] = value;
            return LA3DM_OK;
        }
        for (uint32_t byte = 0; byte < 4; ++byte)
            if ((value >> (8 * byte)) & 0xFFu)
                DM_TRY(hipMemset2DAsync((uint8_t *)p + byte, 4 * stride, (int)((value >> (8 * byte)) & 0xFFu), 1, n, dm->ctx->stream));
        return LA3DM_OK;
    }
};
inline uint32_t float_bits(float v) {
    uint32_t w;
    memcpy(&w, &v, 4);
    return w;
}
}  // namespace
}  // extern "C++"

// A refused call: LA3DM_ERR_ARG with "<who>: <refusal>" as the context's error; an empty refusal is none (LA3DM_OK).
static int refuse(la3dm_devmap *dm, const char *who, const std::string &refusal) {
    if (!dm) return LA3DM_ERR_ARG;
    return refusal.empty() ? LA3DM_OK : dm_fail(dm, LA3DM_ERR_ARG, std::string(who) + ": " + refusal);
}

// ---- save / load (contract: include/la3dm_hip.h; kernels: devmap_pack.h; format and validator: host/pack_format.h) ----
// The pool's covering leaves as the stream.  Launch chain: dm_pack_count (S only -> leaf counts + mask words), the one-launch
// scan over n_blocks + 1 counts straight into the stream's leaf_off section, one read-back of n_leaves, dm_pack_emit, one copy.
// The stream arena is reserved for the most leaves the blocks can have (every finest cell: 64 / 73 of the raw pool at
// block_depth 3) before the count is known, so nothing the count launch wrote has to move.
// pl = nullptr: stream block b is pool slot b (pack); else the nb selected slots of pack_region, whose flags and ranks lie in
// pack_counts already (nothing here may reserve that arena again): dm_evict_list writes the slot list and the keys.
namespace {
struct PackList {
    const uint32_t *flag, *rank;   // per pool slot (+ the closing entry)
    uint32_t *list, *counts;       // nb slots; nb + 1 leaf counts
    uint32_t n_pool;
};
}  // namespace

static int pack_blocks(la3dm_devmap *dm, const char *who, uint64_t nb, const PackList *pl, void *buf, uint64_t cap, uint64_t *size) {
    la3dm_ctx *ctx = dm->ctx;
    if (nb == 0) {   // no block is the header alone: no launch
        *size = la3dm_pack::kHeaderBytes;
        if (!buf) return LA3DM_OK;
        if (cap < *size) return refuse(dm, who, "the buffer is smaller than the stream");
        const la3dm_pack_header h = la3dm_pack::make_header(ctx->p, dm->lv_original_size, nullptr, 0, 0);
        memcpy(buf, &h, sizeof(h));
        return LA3DM_OK;
    }
    DM_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t npb = dm->npb;
    const la3dm_pack::Layout worst = la3dm_pack::layout(nb, nb * dm->ncell, npb);
    DM_RESERVE(dm->pack_stream, worst.total);
    if (!pl) DM_RESERVE(dm->pack_counts, 4ull * (nb + 1));
    uint8_t *arena = (uint8_t *)dm->pack_stream.ptr;
    uint32_t *counts = pl ? pl->counts : (uint32_t *)dm->pack_counts.ptr, *leaf_off = (uint32_t *)(arena + worst.leaf_off), *mask = (uint32_t *)(arena + worst.mask);
    const uint32_t *list = pl ? pl->list : nullptr;   // the kernels' switch: the listed slots, or the pool in order
    const auto count_kernel = pl ? dm_pack_count<true> : dm_pack_count<false>;
    const auto emit_kernel = pl ? dm_pack_emit<true> : dm_pack_emit<false>;
    if (pl) {
        hipLaunchKernelGGL(dm_evict_list, dim3(cdiv(pl->n_pool, 256)), dim3(256), 0, st, (const long long *)dm->blk_key, pl->n_pool, pl->flag, pl->rank,
                           pl->list, (long long *)(arena + worst.keys));
        DM_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(count_kernel, dim3(cdiv(nb + 1, kPackWaves)), dim3(64 * kPackWaves), kPackWaves * pack_lds_stride(npb), st,
                       (const uint8_t *)dm->S, (uint32_t)nb, npb, dm->depth, counts, mask, list);
    DM_TRY(hipGetLastError());
    uint32_t n_leaves = 0;
    DM_OK(scan_total(dm, counts, leaf_off, (uint32_t)nb + 1u, &n_leaves));
    if (n_leaves < nb || n_leaves > nb * dm->ncell) return dm_fail(dm, LA3DM_ERR_HIP, std::string(who) + ": the pool's leaves do not tile its blocks (internal error)");
    const la3dm_pack::Layout l = la3dm_pack::layout(nb, n_leaves, npb);
    *size = l.total;
    if (!buf) return LA3DM_OK;
    if (cap < l.total) return refuse(dm, who, "the buffer is smaller than the stream");
    dm->pack_hdr = la3dm_pack::make_header(ctx->p, dm->lv_original_size, nullptr, nb, n_leaves);
    DM_TRY(hipMemcpyAsync(arena, &dm->pack_hdr, sizeof(dm->pack_hdr), hipMemcpyHostToDevice, st));
    if (!pl) DM_TRY(hipMemcpyAsync(arena + l.keys, dm->blk_key, 8ull * nb, hipMemcpyDeviceToDevice, st));
    PackGaps gaps;
    const uint64_t ends[6][2] = {{l.keys + 8ull * nb, l.leaf_off}, {l.leaf_off + 4ull * (nb + 1), l.mask}, {l.mask + 4ull * nb * l.W, l.state},
                                 {l.state + n_leaves, l.A},         {l.A + 4ull * n_leaves, l.B},           {l.B + 4ull * n_leaves, l.total}};
    for (int g = 0; g < 6; ++g) {
        gaps.at[g] = ends[g][0];
        gaps.len[g] = (uint32_t)(ends[g][1] - ends[g][0]);
    }
    hipLaunchKernelGGL(emit_kernel, dim3(cdiv(nb, kPackWaves)), dim3(64 * kPackWaves), 0, st, (const float *)dm->A, (const float *)dm->B,
                       (const uint8_t *)dm->S, (uint32_t)nb, npb, (const uint32_t *)leaf_off, (const uint32_t *)mask, arena + l.state,
                       (float *)(arena + l.A), (float *)(arena + l.B), arena, gaps, list);
    DM_TRY(hipGetLastError());
    DM_TRY(hipMemcpyAsync(buf, arena, l.total, hipMemcpyDeviceToHost, st));
    DM_TRY(hipStreamSynchronize(st));
    return LA3DM_OK;
}

int la3dm_devmap_pack_host(la3dm_devmap *dm, void *buf, uint64_t cap, uint64_t *size) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (!dm || !size) return LA3DM_ERR_ARG;
    const char *who = "la3dm_devmap_pack_host";
    if (dm->poisoned) return refuse(dm, who, kPoisonedText);
    return pack_blocks(dm, who, dm->n_blocks, nullptr, buf, cap, size);
}

// ---- pack_region / erase_region (contract: include/la3dm_hip.h; kernels: devmap_evict.h; the region: host/region_blocks.h) ----
// What both start with: the checks, dm_evict_select over the pool's keys, the one-launch scan over n_blocks + 1 flags, one
// read-back of the number selected.  pack_counts holds flag[n + 1], rank[n + 1] and 2 n + 2 words for the caller's lists
// (reserved once: an arena may move when it grows).  *words = the first of those.
static int evict_select(la3dm_devmap *dm, const char *who, const int32_t *klo, const int32_t *khi, int inside, uint32_t **flag,
                        uint32_t **rank, uint32_t **words, uint32_t *n_sel) {
    EvictBox box;
    const std::string bad = la3dm_region_blocks::check(klo, khi, &box);
    if (!bad.empty()) return refuse(dm, who, bad);
    if (inside != 0 && inside != 1) return refuse(dm, who, "inside is neither 0 nor 1");
    box.inside = inside;
    if (dm->poisoned) return refuse(dm, who, kPoisonedText);
    *n_sel = 0;
    const uint32_t n = dm->n_blocks;
    if (n == 0) return LA3DM_OK;
    DM_TRY(hipSetDevice(dm->ctx->device));
    hipStream_t st = dm->ctx->stream;
    DM_RESERVE(dm->pack_counts, 4ull * (4ull * n + 4));
    *flag = (uint32_t *)dm->pack_counts.ptr;
    *rank = *flag + n + 1;
    *words = *rank + n + 1;
    hipLaunchKernelGGL(dm_evict_select, dim3(cdiv(n + 1, 256)), dim3(256), 0, st, (const long long *)dm->blk_key, n, box, *flag);
    DM_TRY(hipGetLastError());
    dm->counters_clean = false;   // (the scan may flag a dirty state in the counter block)
    DM_OK(scan_total(dm, *flag, *rank, n + 1u, n_sel));
    if (*n_sel > n) return dm_fail(dm, LA3DM_ERR_HIP, std::string(who) + ": more blocks selected than the pool has (internal error)");
    return LA3DM_OK;
}

// Launch chain: dm_evict_select, the scan, one read-back (blocks selected), dm_evict_list, then pack's own chain over the list
// (dm_pack_count, the scan, one read-back of n_leaves, dm_pack_emit, one copy).  The map is not written.
int la3dm_devmap_pack_region_host(la3dm_devmap *dm, const int32_t klo[3], const int32_t khi[3], int inside, void *buf, uint64_t cap,
                                  uint64_t *size) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (!dm || !size) return LA3DM_ERR_ARG;
    const char *who = "la3dm_devmap_pack_region_host";
    uint32_t *flag = nullptr, *rank = nullptr, *words = nullptr, n_sel = 0;
    DM_OK(evict_select(dm, who, klo, khi, inside, &flag, &rank, &words, &n_sel));
    const PackList pl = {flag, rank, words, words + dm->n_blocks, dm->n_blocks};
    return pack_blocks(dm, who, n_sel, &pl, buf, cap, size);
}

// Launch chain: dm_evict_select, the scan, one read-back (blocks removed); then dm_evict_plan (hole[] and tail[] from the same
// scan), dm_evict_move (one wave per pair, in place), the table cleared and dm_table_rebuild over n_new, one copy of the
// number moved.  Slots >= n_new are dead afterwards: whoever creates a block writes every node of it (dm_pool_init or the
// leaf-count launch for an insert, dm_merge_fuse for a merge, dm_unpack_expand for unpack), so nothing is cleared here.
int la3dm_devmap_erase_region_host(la3dm_devmap *dm, const int32_t klo[3], const int32_t khi[3], int inside, la3dm_erase_stats *stats) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (!dm) return LA3DM_ERR_ARG;
    const char *who = "la3dm_devmap_erase_region_host";
    if (stats) memset(stats, 0, sizeof(*stats));
    uint32_t *flag = nullptr, *rank = nullptr, *words = nullptr, n_removed = 0;
    DM_OK(evict_select(dm, who, klo, khi, inside, &flag, &rank, &words, &n_removed));
    if (n_removed == 0) {   // nothing selected: a no-op
        if (stats) stats->n_blocks = dm->n_blocks;
        return LA3DM_OK;
    }
    hipStream_t st = dm->ctx->stream;
    const uint32_t n = dm->n_blocks, n_new = n - n_removed, most = std::min(n_removed, n_new);
    uint32_t n_moved = 0;
    if (most) {
        uint32_t *hole = words, *tail = words + n;
        hipLaunchKernelGGL(dm_evict_plan, dim3(cdiv(n, 256)), dim3(256), 0, st, n, (const uint32_t *)flag, (const uint32_t *)rank, hole, tail);
        DM_TRY(hipGetLastError());
        hipLaunchKernelGGL(dm_evict_move, dim3(cdiv(most, kPackWaves)), dim3(64 * kPackWaves), 0, st, dm->A, dm->B, dm->S, dm->blk_key, dm->npb,
                           (const uint32_t *)(rank + n_new), (const uint32_t *)hole, (const uint32_t *)tail);
        DM_TRY(hipGetLastError());
        DM_TRY(hipMemcpyAsync(&n_moved, rank + n_new, 4, hipMemcpyDeviceToHost, st));
    }
    // from the first launch that writes the map on, the block count is the new one: a failure below leaves a map that says so
    dm->n_blocks = n_new;
    dm->counters_clean = false;
    if (dm->tab_cap) DM_OK(table_rebuild(dm, dm->tab_key, dm->tab_val, dm->tab_cap, n_new));
    DM_TRY(hipStreamSynchronize(st));
    if (stats) {
        stats->n_removed = n_removed;
        stats->n_moved = n_moved;
        stats->n_blocks = n_new;
    }
    return LA3DM_OK;
}

// Whether a stream may enter this map (unpack, merge): a poisoned map takes none, the stream must be well formed
// (host/pack_format.h) and its header must describe a map like this one.  *h = the stream's header.
static int admit_stream(la3dm_devmap *dm, const char *who, const void *buf, uint64_t size, la3dm_pack_header *h) {
    if (dm->poisoned) return refuse(dm, who, kPoisonedText);
    const std::string bad = la3dm_pack::validate(buf, size, h);
    if (!bad.empty()) return refuse(dm, who, bad);
    return refuse(dm, who, la3dm_pack::mismatch(*h, la3dm_pack::make_header(dm->ctx->p, dm->lv_original_size, nullptr, 0, 0)));
}

// The stream into an empty map: validate (host, before anything is allocated or launched), upload, dm_unpack_expand (the
// canonical pool), block keys, table rebuild; then the host-side facts an insert caches, as a finished insert leaves them —
// except the counter block, which the next insert's dm_begin sets up from n_blocks (counters_clean = false).
int la3dm_devmap_unpack_host(la3dm_devmap *dm, const void *buf, uint64_t size) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (!dm) return LA3DM_ERR_ARG;
    const char *who = "la3dm_devmap_unpack_host";
    la3dm_ctx *ctx = dm->ctx;
    if (dm->n_blocks != 0) return refuse(dm, who, "the map already holds blocks (a stream is loaded into an empty map)");
    la3dm_pack_header h;
    DM_OK(admit_stream(dm, who, buf, size, &h));
    const bool lv_original_size = h.variant == 2u ? (h.flags & LA3DM_PACK_FLAG_LV_ORIGINAL_SIZE) != 0 : dm->lv_original_size;
    if (h.n_blocks == 0) {
        dm->lv_original_size = lv_original_size;
        return LA3DM_OK;
    }
    DM_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t nb = h.n_blocks;
    const uint32_t npb = dm->npb;
    const la3dm_pack::Layout l = la3dm_pack::layout(nb, h.n_leaves, npb);
    DM_OK(grow_pool(dm, nb));
    DM_OK(grow_table(dm, nb));
    DM_RESERVE(dm->pack_stream, l.total);
    uint8_t *arena = (uint8_t *)dm->pack_stream.ptr;
    DM_TRY(hipMemcpyAsync(arena, buf, l.total, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dm_unpack_expand, dim3(cdiv(nb, kPackWaves)), dim3(64 * kPackWaves), kPackWaves * 8u * l.W, st, dm->A, dm->B, dm->S,
                       (uint32_t)nb, npb, dm->depth, (const uint32_t *)(arena + l.leaf_off), (const uint32_t *)(arena + l.mask),
                       (const uint8_t *)(arena + l.state), (const float *)(arena + l.A), (const float *)(arena + l.B), dm->init_A, dm->init_B);
    DM_TRY(hipGetLastError());
    DM_TRY(hipMemcpyAsync(dm->blk_key, arena + l.keys, 8ull * nb, hipMemcpyDeviceToDevice, st));
    DM_OK(table_rebuild(dm, dm->tab_key, dm->tab_val, dm->tab_cap, (uint32_t)nb));
    DM_TRY(hipStreamSynchronize(st));   // (buf is the caller's again)
    dm->n_blocks = (uint32_t)nb;
    dm->lv_original_size = lv_original_size;
    dm->insert_into_empty = false;
    dm->counters_clean = false;
    return LA3DM_OK;
}

// A stream fused into the live map (contract: include/la3dm_hip.h; kernels: devmap_merge.h).  Every refusal comes before the
// first allocation or launch, but one: whether the pool would pass 2^32 nodes is known only after dm_merge_find has counted
// the blocks to create — it writes scratch alone, and the refusal comes before grow_pool.
// Launch chain: one upload, dm_merge_find, the one-launch scan over the "new" flags, one read-back of the number created,
// grow_pool / grow_table, dm_merge_insert, dm_merge_fuse, one read-back of the three cell counters.
int la3dm_devmap_merge_host(la3dm_devmap *dm, const void *buf, uint64_t size, la3dm_merge_stats *stats) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (!dm) return LA3DM_ERR_ARG;
    const char *who = "la3dm_devmap_merge_host";
    la3dm_ctx *ctx = dm->ctx;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (ctx->p.variant != 0 && ctx->p.variant != 3)
        return refuse(dm, who, "merge is defined for BGKOctoMap (variant 0) and BGKLOctoMap (variant 3) maps; GPOctoMap and BGKLVOctoMap fuse by other rules");
    la3dm_pack_header h;
    DM_OK(admit_stream(dm, who, buf, size, &h));
    if (!merge_lds_fits(dm->depth))
        return refuse(dm, who, "block_depth " + std::to_string(dm->depth) + " needs " + std::to_string(kPackWaves * merge_lds_stride(dm->depth)) +
                                   " bytes of LDS per workgroup, a compute unit has " + std::to_string(kMergeLdsPerCu) + " (merge runs at block_depth 1 to 4)");
    if (h.n_blocks == 0) return LA3DM_OK;
    const uint64_t nb = h.n_blocks, cap_max = la3dm_pack::kPoolNodeLimit / dm->npb;
    const char *too_big = "the merged pool would pass 2^32 nodes";
    DM_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t npb = dm->npb, n_old = dm->n_blocks;
    const la3dm_pack::Layout l = la3dm_pack::layout(nb, h.n_leaves, npb);
    DM_RESERVE(dm->pack_stream, l.total);
    DM_RESERVE(dm->pack_counts, 4ull * (3 * nb + 2) + 8 + 8ull * kMergeCntWords);
    uint8_t *arena = (uint8_t *)dm->pack_stream.ptr;
    uint32_t *slot = (uint32_t *)dm->pack_counts.ptr, *flag = slot + nb, *off = flag + nb + 1;
    unsigned long long *cells = (unsigned long long *)(((uintptr_t)(off + nb + 1) + 7u) & ~(uintptr_t)7u);
    const long long *keys = (const long long *)(arena + l.keys);
    DM_TRY(hipMemcpyAsync(arena, buf, l.total, hipMemcpyHostToDevice, st));
    DM_TRY(hipMemsetAsync(cells, 0, 8ull * kMergeCntWords, st));
    hipLaunchKernelGGL(dm_merge_find, dim3(cdiv(nb + 1, 256)), dim3(256), 0, st, keys, (uint32_t)nb, pool_view(dm), n_old && dm->tab_cap ? 1u : 0u, slot, flag);
    DM_TRY(hipGetLastError());
    dm->counters_clean = false;   // (the scan may flag a dirty state in the counter block)
    uint32_t created = 0;
    DM_OK(scan_total(dm, flag, off, (uint32_t)nb + 1u, &created));   // (synchronised: buf is the caller's again)
    if (created > nb) return dm_fail(dm, LA3DM_ERR_HIP, "la3dm_devmap_merge_host: more blocks created than the stream has (internal error)");
    if ((uint64_t)n_old + created > cap_max) return refuse(dm, who, too_big);
    DM_OK(grow_pool(dm, (size_t)n_old + created));
    DM_OK(grow_table(dm, (size_t)n_old + created));
    if (created) {
        hipLaunchKernelGGL(dm_merge_insert, dim3(cdiv(nb, 256)), dim3(256), 0, st, keys, (uint32_t)nb, (const uint32_t *)flag, (const uint32_t *)off,
                           n_old, dm->tab_key, dm->tab_val, dm->tab_cap - 1, dm->blk_key, slot);
        DM_TRY(hipGetLastError());
    }
    MergeArgs ma;
    ma.A = dm->A;
    ma.B = dm->B;
    ma.S = dm->S;
    ma.n_blocks = (uint32_t)nb;
    ma.npb = npb;
    ma.block_depth = dm->depth;
    ma.slot = slot;
    ma.flag = flag;
    ma.leaf_off = (const uint32_t *)(arena + l.leaf_off);
    ma.mask = (const uint32_t *)(arena + l.mask);
    ma.i_state = arena + l.state;
    ma.i_A = (const float *)(arena + l.A);
    ma.i_B = (const float *)(arena + l.B);
    ma.a0 = dm->init_A;
    ma.b0 = dm->init_B;
    ma.free_thresh = ctx->p.free_thresh;
    ma.occupied_thresh = ctx->p.occupied_thresh;
    ma.var_thresh = ctx->p.var_thresh;
    ma.cells = cells;
    hipLaunchKernelGGL(dm_merge_fuse, dim3(cdiv(nb, kPackWaves)), dim3(64 * kPackWaves), kPackWaves * merge_lds_stride(dm->depth), st, ma);
    DM_TRY(hipGetLastError());
    std::vector<unsigned long long> slots(kMergeCntWords);
    DM_TRY(hipMemcpyAsync(slots.data(), cells, 8ull * kMergeCntWords, hipMemcpyDeviceToHost, st));
    DM_TRY(hipStreamSynchronize(st));
    unsigned long long h_cells[3] = {0, 0, 0};
    for (uint32_t s = 0; s < kMergeCntSlots; ++s)
        for (uint32_t k = 0; k < 3; ++k) h_cells[k] += slots[(size_t)(3u * s + k) * kMergeCntStride];
    dm->n_blocks = n_old + created;
    dm->insert_into_empty = false;
    dm->counters_clean = false;
    if (stats) {
        stats->n_blocks = nb;
        stats->n_created = created;
        stats->cells_kept = h_cells[0];
        stats->cells_copied = h_cells[1];
        stats->cells_fused = h_cells[2];
    }
    return LA3DM_OK;
}

// The cells whose class differs between the live map and a stream (contract: include/la3dm_hip.h; kernels: devmap_diff.h).
// Every refusal comes before the first allocation or launch, but one: whether more than 2^32 - 1 cells are selected is known
// only after dm_diff_count — it writes scratch alone, and nothing of the caller's is written before that check.
// Launch chain: one upload, dm_merge_find; with map_only dm_diff_mark, dm_diff_select, the one-launch scan, dm_diff_list (the
// number of map-only blocks stays on the device: the count launch covers n_stream + n_pool waves and reads it there);
// dm_diff_count, the scan over the counts, ONE read-back (the counters, the total, the scan's error word); with cap > 0 and a
// list asked for dm_diff_emit and ONE copy of the list.  Nothing of the map is written, on the device or on the host.
int la3dm_devmap_diff_host(la3dm_devmap *dm, const void *buf, uint64_t size, const la3dm_diff_params *params, uint64_t cap,
                           const la3dm_diff_out *out, uint64_t *n_found, la3dm_diff_stats *stats) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (!dm) return LA3DM_ERR_ARG;
    const char *who = "la3dm_devmap_diff_host";
    la3dm_ctx *ctx = dm->ctx;
    la3dm_pack_header h;
    DM_OK(admit_stream(dm, who, buf, size, &h));
    if (!params) return refuse(dm, who, "params is NULL");
    if (!n_found) return refuse(dm, who, "n_found is NULL");
    if (params->pair_mask >> 25) return refuse(dm, who, "pair_mask has bits above bit 24 (25 pairs, bit 5 * then + now)");
    if (params->value_mask >> 5) return refuse(dm, who, "value_mask has bits above bit 4 (5 classes)");
    if (cap > 0 && !out) return refuse(dm, who, "out is NULL with cap > 0");
    if (!diff_lds_fits(dm->depth))
        return refuse(dm, who, "block_depth " + std::to_string(dm->depth) + " needs " + std::to_string(kPackWaves * diff_lds_stride(dm->depth)) +
                                   " bytes of LDS per workgroup, a compute unit has " + std::to_string(kMergeLdsPerCu) + " (diff runs at block_depth 1 to 5)");
    la3dm_diff_out o;
    memset(&o, 0, sizeof(o));
    if (out) o = *out;
    const bool want_list = cap > 0 && (o.block_key || o.cell || o.code || o.centre || o.A || o.B);
    if (want_list && o.centre && dm->npb > ctx->lut_count) return refuse(dm, who, "the context's voxel LUT does not reach the finest layer");
    const uint64_t nb = h.n_blocks;
    const uint32_t n_pool = params->map_only ? dm->n_blocks : 0u, npb = dm->npb;
    if (nb + n_pool > 0xFFFFFFFEull) return refuse(dm, who, "more than 2^32 - 2 blocks to compare");
    la3dm_diff_stats S;
    memset(&S, 0, sizeof(S));
    if (nb + n_pool == 0) {   // nothing to compare: no launch
        *n_found = 0;
        if (stats) *stats = S;
        return LA3DM_OK;
    }
    DM_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t n_grid = (uint32_t)(nb + n_pool);
    const la3dm_pack::Layout l = la3dm_pack::layout(nb, h.n_leaves, npb);
    if (nb) DM_RESERVE(dm->pack_stream, l.total);
    // scratch: slot[nb], mark[n_pool], flag[n_pool + 1], rank[n_pool + 1], only[n_pool], counts[n_grid + 1], offset[n_grid + 1], the counters
    DM_RESERVE(dm->pack_counts, 4ull * (nb + 4ull * n_pool + 2 + 2ull * n_grid + 2) + 8 + 8ull * kDiffCntWords);
    uint8_t *arena = (uint8_t *)dm->pack_stream.ptr;
    uint32_t *slot = (uint32_t *)dm->pack_counts.ptr, *mark = slot + nb, *flag = mark + n_pool, *rank = flag + n_pool + 1, *only = rank + n_pool + 1;
    uint32_t *counts = only + n_pool, *offset = counts + n_grid + 1;
    unsigned long long *cnt = (unsigned long long *)(((uintptr_t)(offset + n_grid + 1) + 7u) & ~(uintptr_t)7u);
    DM_TRY(hipMemsetAsync(cnt, 0, 8ull * kDiffCntWords, st));
    if (nb) {
        DM_TRY(hipMemcpyAsync(arena, buf, l.total, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(dm_merge_find, dim3(cdiv(nb + 1, 256)), dim3(256), 0, st, (const long long *)(arena + l.keys), (uint32_t)nb, pool_view(dm),
                           dm->n_blocks && dm->tab_cap ? 1u : 0u, slot, counts);   // (its "new" flags land in counts, which dm_diff_count overwrites)
        DM_TRY(hipGetLastError());
    }
    dm->counters_clean = false;   // (the scans may flag a dirty state in the counter block)
    if (n_pool) {
        DM_TRY(hipMemsetAsync(mark, 0, 4ull * n_pool, st));
        if (nb) {
            hipLaunchKernelGGL(dm_diff_mark, dim3(cdiv(nb, 256)), dim3(256), 0, st, (const uint32_t *)slot, (uint32_t)nb, mark);
            DM_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(dm_diff_select, dim3(cdiv(n_pool + 1, 256)), dim3(256), 0, st, (const uint32_t *)mark, n_pool, flag);
        DM_TRY(hipGetLastError());
        DM_OK(exclusive_scan(dm, flag, rank, n_pool + 1u));
        hipLaunchKernelGGL(dm_diff_list, dim3(cdiv(n_pool, 256)), dim3(256), 0, st, n_pool, (const uint32_t *)flag, (const uint32_t *)rank, only);
        DM_TRY(hipGetLastError());
    }
    DiffArgs a;
    memset(&a, 0, sizeof(a));
    a.A = dm->A;
    a.B = dm->B;
    a.S = dm->S;
    a.blk_key = (const long long *)dm->blk_key;
    a.npb = npb;
    a.block_depth = dm->depth;
    a.n_stream = (uint32_t)nb;
    a.n_grid = n_grid;
    a.n_only = n_pool ? rank + n_pool : nullptr;
    a.slot = slot;
    a.only = only;
    if (nb) {   // (no stream block: no wave reads a section)
        a.keys = (const long long *)(arena + l.keys);
        a.leaf_off = (const uint32_t *)(arena + l.leaf_off);
        a.mask = (const uint32_t *)(arena + l.mask);
        a.i_state = arena + l.state;
        a.i_A = (const float *)(arena + l.A);
        a.i_B = (const float *)(arena + l.B);
    }
    a.a0 = dm->init_A;
    a.b0 = dm->init_B;
    a.pair_mask = params->pair_mask;
    a.value_mask = params->value_mask;
    a.counts = counts;
    a.cnt = cnt;
    const uint32_t lds = kPackWaves * diff_lds_stride(dm->depth);
    hipLaunchKernelGGL(params->value_mask ? dm_diff_count<true> : dm_diff_count<false>, dim3(cdiv(n_grid + 1, kPackWaves)), dim3(64 * kPackWaves), lds, st, a);
    DM_TRY(hipGetLastError());
    std::vector<unsigned long long> lines(kDiffCntWords);
    uint32_t total = 0;
    DM_OK(scan_total(dm, counts, offset, n_grid + 1u, &total, lines.data(), cnt, 8ull * kDiffCntWords));   // (synchronised: buf is the caller's again)
    unsigned long long sum[kDiffCnt];
    for (uint32_t k = 0; k < kDiffCnt; ++k) {
        sum[k] = 0;
        for (uint32_t s = 0; s < kDiffCntSlots; ++s) sum[k] += lines[(size_t)(kDiffCnt * s + k) * kMergeCntStride];
    }
    const unsigned long long selected = sum[kDiffCntSelected], n_only = sum[kDiffCntOnly];
    if (selected > 0xFFFFFFFFull) return refuse(dm, who, "more than 2^32 - 1 cells are selected (" + std::to_string(selected) + ")");
    if (selected != total || n_only > n_pool || sum[kDiffCntMissing] > nb)
        return dm_fail(dm, LA3DM_ERR_HIP, "la3dm_devmap_diff_host: the counters and the scan disagree (internal error)");
    const uint64_t m = std::min<uint64_t>(cap, selected);
    if (want_list && m) {
        Stage s(dm, true);
        s.out(o.block_key, m);
        s.out(o.cell, m);
        s.out(o.code, m);
        s.out(o.centre, 3 * m);
        s.out(o.A, m);
        s.out(o.B, m);
        DM_OK(s.reserve());
        a.n_grid = (uint32_t)(nb + n_only);
        a.offset = offset;
        a.cap = (uint32_t)m;
        a.lut = ctx->d_lut;
        a.block_size = dm->block_size;
        a.o_key = (long long *)o.block_key;
        a.o_cell = o.cell;
        a.o_code = o.code;
        a.o_centre = o.centre;
        a.o_A = o.A;
        a.o_B = o.B;
        hipLaunchKernelGGL(params->value_mask || o.A || o.B ? dm_diff_emit<true> : dm_diff_emit<false>, dim3(cdiv(a.n_grid, kPackWaves)),
                           dim3(64 * kPackWaves), lds, st, a);
        DM_TRY(hipGetLastError());
        DM_OK(s.download());
        DM_TRY(hipStreamSynchronize(st));
    }
    *n_found = selected;
    if (stats) {
        S.n_stream_blocks = nb;
        S.n_map_only_blocks = n_only;
        S.n_missing_now = sum[kDiffCntMissing];
        for (int k = 0; k < 25; ++k) S.pairs[k] = sum[k];
        for (int k = 0; k < 5; ++k) S.value_changed[k] = sum[25 + k];
        *stats = S;
    }
    return LA3DM_OK;
}

int la3dm_devmap_search_host(la3dm_devmap *dm, const float *xyz, uint32_t n, uint8_t *exists, float *A, float *B,
                             uint8_t *state) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (!dm || (n && (!xyz || !exists || !A || !B || !state))) return LA3DM_ERR_ARG;
    if (n == 0) return LA3DM_OK;
    DM_TRY(hipSetDevice(dm->ctx->device));
    hipStream_t st = dm->ctx->stream;
    if (dm->n_blocks == 0) {  // empty map: every query misses
        const Fill f{dm, true};
        DM_OK(f.bytes(exists, 0, n));
        DM_OK(f.words(A, float_bits(dm->init_A), n));
        DM_OK(f.words(B, float_bits(dm->init_B), n));
        return f.bytes(state, kStateUnknown, n);
    }
    Stage s(dm, true);
    s.in(xyz, 3ull * n);
    s.out(A, n);
    s.out(B, n);
    s.out(exists, n);
    s.out(state, n);
    DM_OK(s.reserve());
    hipLaunchKernelGGL(dm_search, dim3(cdiv(n, 256)), dim3(256), 0, st, xyz, n, dm->tab_key, dm->tab_val, dm->tab_cap - 1, dm->A, dm->B,
                       dm->S, dm->npb, dm->depth, dm->block_size, dm->ctx->p.resolution, dm->init_A, dm->init_B, exists, A, B, state);
    DM_OK(s.download());
    DM_TRY(hipStreamSynchronize(st));
    return LA3DM_OK;
}

// ---- batched ray casting (devmap_raycast.h) -----------------------------------------------------------------
static int raycast_check(la3dm_devmap *dm, const float *rays6, uint32_t n, uint32_t max_steps, const la3dm_raycast_out *out,
                         const char *who) {
    if (!dm) return LA3DM_ERR_ARG;
    dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (max_steps == 0 || max_steps > LA3DM_RAY_MAX_STEPS) return refuse(dm, who, "max_steps must be 1 ... 2^20");
    if (n == 0) return LA3DM_OK;
    if (!rays6) return refuse(dm, who, "rays6 is NULL");
    if (!out || !out->steps || !out->flags) return refuse(dm, who, "out, out->steps and out->flags must not be NULL");
    return LA3DM_OK;
}

static void raycast_launch(la3dm_devmap *dm, const float *d_rays6, uint32_t n, uint32_t stop_mask, uint32_t max_steps,
                           const la3dm_raycast_out &o) {
    RaycastArgs a;
    memset(&a, 0, sizeof(a));
    a.rays = d_rays6;
    a.n = n;
    a.stop_mask = stop_mask;
    a.max_steps = max_steps;
    a.pool = pool_view(dm);
    a.lut = dm->ctx->d_lut;
    a.block_size = dm->block_size;
    a.resolution = dm->ctx->p.resolution;
    a.steps = o.steps;
    a.flags = o.flags;
    a.p = o.p;
    a.block_key = (long long *)o.block_key;
    a.node_key = o.node_key;
    a.cls = o.cls;
    a.leaf_depth = o.leaf_depth;
    a.oA = o.A;
    a.oB = o.B;
    a.counts = o.counts;
    hipLaunchKernelGGL(dm_raycast, dim3(cdiv(n, 256)), dim3(256), 0, dm->ctx->stream, a);
}

// empty map: no ray starts
static int raycast_empty(const Fill &f, la3dm_devmap *dm, size_t n, const la3dm_raycast_out &o) {
    DM_OK(f.bytes(o.steps, 0, 4 * n));
    DM_OK(f.bytes(o.flags, 0, n));
    DM_OK(f.bytes(o.p, 0, 12 * n));
    DM_OK(f.bytes(o.block_key, 0, 8 * n));
    DM_OK(f.bytes(o.node_key, 0, 4 * n));
    DM_OK(f.bytes(o.cls, (int)LA3DM_RAY_MISSING, n));
    DM_OK(f.bytes(o.leaf_depth, 255, n));
    DM_OK(f.words(o.A, float_bits(dm->init_A), n));
    DM_OK(f.words(o.B, float_bits(dm->init_B), n));
    return f.bytes(o.counts, 0, 16 * n);
}

static int raycast_query(la3dm_devmap *dm, bool host, const char *who, const float *rays6, uint32_t n, uint32_t stop_mask,
                         uint32_t max_steps, const la3dm_raycast_out *out) {
    int rc = raycast_check(dm, rays6, n, max_steps, out, who);
    if (rc != LA3DM_OK || n == 0) return rc;
    DM_TRY(hipSetDevice(dm->ctx->device));
    la3dm_raycast_out o = *out;
    if (dm->n_blocks == 0) {
        DM_OK(raycast_empty(Fill{dm, host}, dm, n, o));
    } else {
        Stage s(dm, host);
        s.in(rays6, 6ull * n);
        s.out(o.steps, n);
        s.out(o.flags, n);
        s.out(o.p, 3ull * n);
        s.out(o.block_key, n);
        s.out(o.node_key, n);
        s.out(o.cls, n);
        s.out(o.leaf_depth, n);
        s.out(o.A, n);
        s.out(o.B, n);
        s.out(o.counts, 4ull * n);
        DM_OK(s.reserve());
        raycast_launch(dm, rays6, n, stop_mask, max_steps, o);
        DM_TRY(hipGetLastError());
        DM_OK(s.download());
    }
    DM_TRY(hipStreamSynchronize(dm->ctx->stream));
    return LA3DM_OK;
}

int la3dm_devmap_raycast_device(la3dm_devmap *dm, const float *d_rays6, uint32_t n, uint32_t stop_mask, uint32_t max_steps,
                                const la3dm_raycast_out *d_out) {
    return raycast_query(dm, false, "la3dm_devmap_raycast_device", d_rays6, n, stop_mask, max_steps, d_out);
}

int la3dm_devmap_raycast_host(la3dm_devmap *dm, const float *rays6, uint32_t n, uint32_t stop_mask, uint32_t max_steps,
                              const la3dm_raycast_out *out) {
    return raycast_query(dm, true, "la3dm_devmap_raycast_host", rays6, n, stop_mask, max_steps, out);
}

// ---- dense region reads (devmap_region.h) --------------------------------------------------------------------
// The region's checks and its anchor (host/region_contract.h, shared with the host twin BGKOctoMap::region_anchor), then
// info.origin, for which the one LUT entry of the anchor cell is fetched from the device.
static int region_resolve(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_region::Query &q, bool has_out,
                          bool has_mandatory, const char *who, RegionGeom &g) {
    if (!dm) return LA3DM_ERR_ARG;
    dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    la3dm_region::Anchor an;
    DM_OK(refuse(dm, who, la3dm_region::resolve(q, lo3, dims3, dm->ctx->p.resolution, dm->block_size, dm->depth, has_out, has_mandatory,
                                                "->", an)));
    for (int k = 0; k < 3; ++k) {
        g.g0[k] = an.g0[k];
        g.dims[k] = dims3[k];
        g.info.cell[k] = an.cell[k];
    }
    g.total = an.total;
    g.info.block_key = an.block_key;
    // origin = Block::get_point of the anchor cell: the LUT entry of its finest-layer node + the block centre
    const int dl = (int)dm->depth - 1;
    uint32_t index = 0;
    for (int level = dl - 1; level >= 0; --level)
        index = index * 8u + ((((an.cell[0] >> level) & 1u) << 2) | (((an.cell[1] >> level) & 1u) << 1) | ((an.cell[2] >> level) & 1u));
    const uint32_t entry = (0x249249u & ((1u << (3u * (uint32_t)dl)) - 1u)) + index;
    if (entry >= dm->ctx->lut_count) return refuse(dm, who, "the context's voxel LUT does not reach the finest layer");
    float4 o;
    DM_TRY(hipSetDevice(dm->ctx->device));
    DM_TRY(hipMemcpyAsync(&o, dm->ctx->d_lut + entry, sizeof(o), hipMemcpyDeviceToHost, dm->ctx->stream));
    DM_TRY(hipStreamSynchronize(dm->ctx->stream));
    g.info.origin[0] = o.x + an.center[0];
    g.info.origin[1] = o.y + an.center[1];
    g.info.origin[2] = o.z + an.center[2];
    return LA3DM_OK;
}

static RegionArgs region_args(la3dm_devmap *dm, const RegionGeom &g) {
    RegionArgs a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < 3; ++k) a.g0[k] = g.g0[k];
    a.nx = g.dims[0];
    a.ny = g.dims[1];
    a.nz = g.dims[2];
    a.total = (uint32_t)g.total;
    a.pool = pool_view(dm);
    return a;
}

static void box_launch(la3dm_devmap *dm, const RegionGeom &g, const la3dm_box_out &o) {
    RegionArgs a = region_args(dm, g);
    a.cls = o.cls;
    a.leaf_depth = o.leaf_depth;
    a.oA = o.A;
    a.oB = o.B;
    // four voxels per thread (word / float4 stores) when every output is aligned for them, else one
    const bool vec = ((uintptr_t)o.cls & 3u) == 0 && ((uintptr_t)o.leaf_depth & 3u) == 0 && ((uintptr_t)o.A & 15u) == 0 && ((uintptr_t)o.B & 15u) == 0;
    if (vec)
        hipLaunchKernelGGL(dm_box<4>, dim3(cdiv(cdiv(a.total, 4), 256)), dim3(256), 0, dm->ctx->stream, a);
    else
        hipLaunchKernelGGL(dm_box<1>, dim3(cdiv(a.total, 256)), dim3(256), 0, dm->ctx->stream, a);
}

static void columns_launch(la3dm_devmap *dm, const RegionGeom &g, const la3dm_columns_out &o) {
    RegionArgs a = region_args(dm, g);
    a.counts = o.counts;
    a.low_occ = o.low_occ;
    a.top_occ = o.top_occ;
    a.counts_vec = ((uintptr_t)o.counts & 15u) == 0 ? 1u : 0u;
    hipLaunchKernelGGL(dm_columns, dim3(cdiv(a.total, 256)), dim3(256), 0, dm->ctx->stream, a);
}

// empty map: every block is missing
static int box_empty(const Fill &f, la3dm_devmap *dm, size_t n, const la3dm_box_out &o) {
    DM_OK(f.bytes(o.cls, (int)LA3DM_RAY_MISSING, n));
    DM_OK(f.bytes(o.leaf_depth, 255, n));
    DM_OK(f.words(o.A, float_bits(dm->init_A), n));
    return f.words(o.B, float_bits(dm->init_B), n);
}

static int box_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3, const la3dm_box_out *out,
                     la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::kBox, out != nullptr, out && out->cls, who, g));
    la3dm_box_out o = *out;
    const size_t n = (size_t)g.total;
    if (dm->n_blocks == 0) {
        DM_OK(box_empty(Fill{dm, host}, dm, n, o));
    } else {
        Stage s(dm, host);   // (every twin aligned for the four-voxel stores)
        s.out(o.cls, n);
        s.out(o.leaf_depth, n);
        s.out(o.A, n);
        s.out(o.B, n);
        DM_OK(s.reserve());
        box_launch(dm, g, o);
        DM_TRY(hipGetLastError());
        DM_OK(s.download());
    }
    DM_TRY(hipStreamSynchronize(dm->ctx->stream));
    if (info) *info = g.info;
    return LA3DM_OK;
}

int la3dm_devmap_box_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_box_out *d_out,
                            la3dm_region_info *info) {
    return box_query(dm, false, "la3dm_devmap_box_device", lo3, dims3, d_out, info);
}

int la3dm_devmap_box_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_box_out *out,
                          la3dm_region_info *info) {
    return box_query(dm, true, "la3dm_devmap_box_host", lo3, dims3, out, info);
}

// empty map: {0, 0, 0, nz} per column (nz <= 2^16), no occupied voxel
static int columns_empty(const Fill &f, size_t n, uint32_t nz, const la3dm_columns_out &o) {
    DM_OK(f.bytes(o.counts, 0, 16 * n));
    DM_OK(f.strided(o.counts + 3, nz, 4, n));
    DM_OK(f.bytes(o.low_occ, 0xFF, 4 * n));
    return f.bytes(o.top_occ, 0xFF, 4 * n);
}

static int columns_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3,
                         const la3dm_columns_out *out, la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::kColumns, out != nullptr, out && out->counts, who, g));
    la3dm_columns_out o = *out;
    const size_t n = (size_t)g.total;
    if (dm->n_blocks == 0) {
        DM_OK(columns_empty(Fill{dm, host}, n, g.dims[2], o));
    } else {
        Stage s(dm, host);   // (per column, nothing that grows with nz)
        s.out(o.counts, 4 * n);
        s.out(o.low_occ, n);
        s.out(o.top_occ, n);
        DM_OK(s.reserve());
        columns_launch(dm, g, o);
        DM_TRY(hipGetLastError());
        DM_OK(s.download());
    }
    DM_TRY(hipStreamSynchronize(dm->ctx->stream));
    if (info) *info = g.info;
    return LA3DM_OK;
}

int la3dm_devmap_columns_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_columns_out *d_out,
                                la3dm_region_info *info) {
    return columns_query(dm, false, "la3dm_devmap_columns_device", lo3, dims3, d_out, info);
}

int la3dm_devmap_columns_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_columns_out *out,
                              la3dm_region_info *info) {
    return columns_query(dm, true, "la3dm_devmap_columns_host", lo3, dims3, out, info);
}

// ---- distance field of a region (devmap_distance.h) -------------------------------------------------------------

// a min-plus pass over 16-bit z distances or (wide) 32-bit partial sums: staged in LDS where the rows of a workgroup and
// their halo fit, else straight from global memory
static void df_pass_launch(hipStream_t st, bool wide, uint32_t grid, uint32_t rows, const DfPassArgs &p) {
    const uint32_t lds = rows * 64u * (wide ? 4u : 2u);
    const bool fits = lds <= kDfLdsBytes;
    void (*pass)(DfPassArgs) = wide ? (fits ? dm_df_pass<uint32_t, true> : dm_df_pass<uint32_t, false>)
                                    : (fits ? dm_df_pass<uint16_t, true> : dm_df_pass<uint16_t, false>);
    hipLaunchKernelGGL(pass, dim3(grid), dim3(256), fits ? lds : 0, st, p);
}

// The four stages on the map's stream.  Two buffers take turns: `work` (4 bytes per voxel, the devmap's) and `spare` (an
// output array, d2 or dist, free until the last pass fills it).  The last pass reads `work`, so the pass before it — y, or
// z where ny = 1 and the y pass is left out — writes there, and each earlier stage writes where its successor does not.
static void distance_launch(la3dm_devmap *dm, const RegionGeom &g, uint32_t obstacle_mask, uint32_t radius, void *work,
                            const la3dm_distance_out &o) {
    hipStream_t st = dm->ctx->stream;
    RegionArgs a = region_args(dm, g);
    void *spare = o.d2 ? (void *)o.d2 : (void *)o.dist;
    const bool y_pass = a.ny > 1;
    uint32_t *bits = (uint32_t *)(y_pass ? work : spare);   // ceil(total / 32) words <= 4 bytes per voxel
    uint16_t *fz = (uint16_t *)(y_pass ? spare : work);
    hipLaunchKernelGGL(dm_df_bits, dim3(cdiv(a.total, 256)), dim3(256), 0, st, a, obstacle_mask, bits);
    hipLaunchKernelGGL(dm_df_z, dim3(cdiv(a.total, 256)), dim3(256), 0, st, bits, fz, a.total, a.nz, radius);
    DfPassArgs p;
    memset(&p, 0, sizeof(p));
    p.radius = radius;
    p.r2 = radius * radius;
    p.resolution = dm->ctx->p.resolution;
    const uint32_t rows = kDfRows + 2u * radius;   // what a workgroup stages at most
    if (y_pass) {
        p.in = fz;
        p.out = (uint32_t *)work;
        p.L = a.ny;
        p.S = a.nz;
        p.n_lt = cdiv(p.L, kDfRows);
        p.n_ct = cdiv(p.S, 64);
        df_pass_launch(st, false, a.nx * p.n_lt * p.n_ct, rows, p);
    }
    p.in = work;
    p.out = nullptr;
    p.d2 = o.d2;
    p.dist = o.dist;
    p.last = 1;
    p.L = a.nx;
    p.S = a.ny * a.nz;
    p.n_lt = cdiv(p.L, kDfRows);
    p.n_ct = cdiv(p.S, 64);
    df_pass_launch(st, y_pass, p.n_lt * p.n_ct, rows, p);
}

// The obstacle field a query built on distance_field sees (reach, travel, score_poses, score_paths), decided here alone:
// radius 0 asks for no field, every voxel is FAR; an empty map has the uniform answer of distance_empty and no launch;
// otherwise the transform's chain runs into d2 — n words the caller has reserved in an arena of its own — with df_work
// as its working storage.
static int obstacle_field(la3dm_devmap *dm, const RegionGeom &g, uint32_t obstacle_mask, uint32_t radius, uint32_t *d2, ObstacleField &field) {
    field = ObstacleField{nullptr, LA3DM_DF_FAR};
    if (radius == 0) return LA3DM_OK;
    if (dm->n_blocks == 0) {
        if ((obstacle_mask >> LA3DM_RAY_MISSING) & 1u) field.fill = 0u;
        return LA3DM_OK;
    }
    DM_RESERVE(dm->df_work, 4ull * (size_t)g.total);
    distance_launch(dm, g, obstacle_mask, radius, dm->df_work.ptr, la3dm_distance_out{d2, nullptr});
    field.d2 = d2;
    return LA3DM_OK;
}

// empty map: every voxel is MISSING — all obstacles (0 everywhere) or none (FAR, +inf)
static int distance_empty(const Fill &f, size_t n, uint32_t obstacle_mask, const la3dm_distance_out &o) {
    const bool all = (obstacle_mask >> LA3DM_RAY_MISSING) & 1u;
    DM_OK(f.bytes(o.d2, all ? 0 : 0xFF, 4 * n));
    return f.words(o.dist, all ? 0u : 0x7F800000u, n);
}

static int distance_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask,
                          uint32_t radius, const la3dm_distance_out *out, la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(refuse(dm, who, la3dm_region::distance_check(obstacle_mask, radius)));
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::kDistance, out != nullptr, out && (out->d2 || out->dist), who, g));
    la3dm_distance_out o = *out;
    const size_t n = (size_t)g.total;
    if (dm->n_blocks == 0) {
        DM_OK(distance_empty(Fill{dm, host}, n, obstacle_mask, o));
    } else {
        Stage s(dm, host);
        s.out(o.d2, n);
        s.out(o.dist, n);
        DM_OK(s.reserve());
        DM_RESERVE(dm->df_work, 4ull * n);
        distance_launch(dm, g, obstacle_mask, radius, dm->df_work.ptr, o);
        DM_TRY(hipGetLastError());
        DM_OK(s.download());
    }
    DM_TRY(hipStreamSynchronize(dm->ctx->stream));
    if (info) *info = g.info;
    return LA3DM_OK;
}

int la3dm_devmap_distance_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask,
                                 uint32_t radius, const la3dm_distance_out *d_out, la3dm_region_info *info) {
    return distance_query(dm, false, "la3dm_devmap_distance_device", lo3, dims3, obstacle_mask, radius, d_out, info);
}

int la3dm_devmap_distance_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask,
                               uint32_t radius, const la3dm_distance_out *out, la3dm_region_info *info) {
    return distance_query(dm, true, "la3dm_devmap_distance_host", lo3, dims3, obstacle_mask, radius, out, info);
}

// ---- nearest and nearest_points: which obstacle is the nearest (devmap_nearest.h) ---------------------------------

// the parts of nt_work: per voxel the y keys, the z offsets and the obstacle bits; for nearest_points index and d2 as well
struct NtWork {
    uint32_t *keys;
    int16_t *az;
    uint32_t *bits;
    uint32_t *index, *d2;   // null for nearest, whose answer goes to the caller's arrays
};

static int nearest_reserve(la3dm_devmap *dm, size_t n, bool with_answer, NtWork &w) {
    const auto pad = [](size_t bytes) { return (bytes + 15) & ~(size_t)15; };
    const size_t keys = pad(4 * n), az = pad(2 * n), bits = pad(4 * ((n + 31) / 32)), answer = with_answer ? pad(4 * n) : 0;
    DM_RESERVE(dm->nt_work, keys + az + bits + 2 * answer);
    char *p = (char *)dm->nt_work.ptr;
    w.keys = (uint32_t *)p;
    w.az = (int16_t *)(p + keys);
    w.bits = (uint32_t *)(p + keys + az);
    w.index = with_answer ? (uint32_t *)(p + keys + az + bits) : nullptr;
    w.d2 = with_answer ? (uint32_t *)(p + keys + az + bits + answer) : nullptr;
    return LA3DM_OK;
}

// the y pass over 16-bit z offsets or the x pass over 32-bit keys: staged in LDS where the rows of a workgroup and their
// halo fit, else straight from global memory (y: radius <= 240, x: radius <= 112)
static void nt_pass_launch(hipStream_t st, bool x_pass, uint32_t grid, uint32_t rows, const NtPassArgs &p) {
    const uint32_t lds = rows * 64u * (x_pass ? 4u : 2u);
    const bool fits = lds <= kDfLdsBytes;
    void (*pass)(NtPassArgs) = x_pass ? (fits ? dm_nt_pass<uint32_t, true> : dm_nt_pass<uint32_t, false>)
                                      : (fits ? dm_nt_pass<int16_t, true> : dm_nt_pass<int16_t, false>);
    hipLaunchKernelGGL(pass, dim3(grid), dim3(256), fits ? lds : 0, st, p);
}

// The four launches on the map's stream: distance_field's bits, the z offsets, the y keys, the x pass with the chase into
// index and d2 (device memory, either may be null).
static void nearest_launch(la3dm_devmap *dm, const RegionGeom &g, uint32_t obstacle_mask, uint32_t radius, const NtWork &w, uint32_t *index,
                           uint32_t *d2) {
    hipStream_t st = dm->ctx->stream;
    const RegionArgs a = region_args(dm, g);
    hipLaunchKernelGGL(dm_df_bits, dim3(cdiv(a.total, 256)), dim3(256), 0, st, a, obstacle_mask, w.bits);
    hipLaunchKernelGGL(dm_nt_z, dim3(cdiv(a.total, 256)), dim3(256), 0, st, w.bits, w.az, a.total, a.nz, radius);
    NtPassArgs p;
    memset(&p, 0, sizeof(p));
    p.radius = radius;
    p.r2 = radius * radius;
    p.ny = a.ny;
    p.nz = a.nz;
    const uint32_t rows = kDfRows + 2u * radius;   // what a workgroup stages at most
    p.in = w.az;
    p.keys = w.keys;
    p.L = a.ny;
    p.S = a.nz;
    p.n_lt = cdiv(p.L, kDfRows);
    p.n_ct = cdiv(p.S, 64);
    nt_pass_launch(st, false, a.nx * p.n_lt * p.n_ct, rows, p);
    p.in = w.keys;
    p.keys = nullptr;
    p.az = w.az;
    p.index = index;
    p.d2 = d2;
    p.L = a.nx;
    p.S = a.ny * a.nz;
    p.n_lt = cdiv(p.L, kDfRows);
    p.n_ct = cdiv(p.S, 64);
    nt_pass_launch(st, true, p.n_lt * p.n_ct, rows, p);
}

static int nearest_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask,
                         uint32_t radius, const la3dm_nearest_out *out, la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(refuse(dm, who, la3dm_region::nearest_check(obstacle_mask, radius, 0)));
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::kNearest, out != nullptr, out && (out->index || out->d2), who, g));
    la3dm_nearest_out o = *out;
    const size_t n = (size_t)g.total;
    if (dm->n_blocks == 0) {   // every voxel is MISSING: each its own nearest obstacle, or none anywhere
        const Fill f{dm, host};
        const bool all = (obstacle_mask >> LA3DM_RAY_MISSING) & 1u;
        DM_OK(f.bytes(o.d2, all ? 0 : 0xFF, 4 * n));
        if (!all) {
            DM_OK(f.bytes(o.index, 0xFF, 4 * n));
        } else if (o.index && host) {
            for (size_t v = 0; v < n; ++v) o.index[v] = (uint32_t)v;
        } else if (o.index) {
            hipLaunchKernelGGL(dm_nt_iota, dim3(cdiv((uint32_t)n, 256)), dim3(256), 0, dm->ctx->stream, o.index, (uint32_t)n);
            DM_TRY(hipGetLastError());
        }
    } else {
        Stage s(dm, host);
        s.out(o.index, n);
        s.out(o.d2, n);
        DM_OK(s.reserve());
        NtWork w;
        DM_OK(nearest_reserve(dm, n, false, w));
        nearest_launch(dm, g, obstacle_mask, radius, w, o.index, o.d2);
        DM_TRY(hipGetLastError());
        DM_OK(s.download());
    }
    DM_TRY(hipStreamSynchronize(dm->ctx->stream));
    if (info) *info = g.info;
    return LA3DM_OK;
}

int la3dm_devmap_nearest_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask, uint32_t radius,
                                const la3dm_nearest_out *d_out, la3dm_region_info *info) {
    return nearest_query(dm, false, "la3dm_devmap_nearest_device", lo3, dims3, obstacle_mask, radius, d_out, info);
}

int la3dm_devmap_nearest_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask, uint32_t radius,
                              const la3dm_nearest_out *out, la3dm_region_info *info) {
    return nearest_query(dm, true, "la3dm_devmap_nearest_host", lo3, dims3, obstacle_mask, radius, out, info);
}

static int nearest_points_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3, const float *points3,
                                uint32_t n_points, const float *pose12, uint32_t obstacle_mask, uint32_t radius,
                                const la3dm_nearest_points_out *out, la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(refuse(dm, who, la3dm_region::nearest_check(obstacle_mask, radius, n_points)));
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::kNearestPoints, true, true, who, g));   // lo, dims, the limit and the range: before any buffer
    DM_OK(refuse(dm, who, la3dm_region::nearest_buffers(n_points, points3 != nullptr, out != nullptr,
                                                        out && (out->cls || out->voxel || out->index || out->d2))));
    if (info) *info = g.info;
    if (n_points == 0) return LA3DM_OK;
    la3dm_nearest_points_out o = *out;
    Stage s(dm, host);
    s.in(points3, 3ull * n_points);
    s.in(pose12, 12);
    s.out(o.cls, n_points);
    s.out(o.voxel, n_points);
    s.out(o.index, n_points);
    s.out(o.d2, n_points);
    DM_OK(s.reserve());
    NtPointsArgs a;
    memset(&a, 0, sizeof(a));
    a.points = points3;
    a.pose = pose12;
    a.n_points = n_points;
    a.resolution = dm->ctx->p.resolution;
    a.block_size = dm->block_size;
    a.lim = 1 << (dm->depth - 1);
    for (int k = 0; k < 3; ++k) {
        a.g0[k] = g.g0[k];
        a.dims[k] = g.dims[k];
    }
    if (dm->n_blocks == 0) {   // no transform to run: every voxel at distance 0 from itself, or FAR
        a.fill = ((obstacle_mask >> LA3DM_RAY_MISSING) & 1u) ? 0u : LA3DM_DF_FAR;
    } else {
        NtWork w;
        DM_OK(nearest_reserve(dm, (size_t)g.total, true, w));
        nearest_launch(dm, g, obstacle_mask, radius, w, w.index, w.d2);
        a.index = w.index;
        a.d2 = w.d2;
    }
    a.o_cls = o.cls;
    a.o_voxel = o.voxel;
    a.o_index = o.index;
    a.o_d2 = o.d2;
    hipLaunchKernelGGL(dm_nt_points, dim3(cdiv(n_points, 256)), dim3(256), 0, dm->ctx->stream, a);
    DM_TRY(hipGetLastError());
    DM_OK(s.download());
    DM_TRY(hipStreamSynchronize(dm->ctx->stream));
    return LA3DM_OK;
}

int la3dm_devmap_nearest_points_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *d_points3, uint32_t n_points,
                                       const float *d_pose12, uint32_t obstacle_mask, uint32_t radius, const la3dm_nearest_points_out *d_out,
                                       la3dm_region_info *info) {
    return nearest_points_query(dm, false, "la3dm_devmap_nearest_points_device", lo3, dims3, d_points3, n_points, d_pose12, obstacle_mask, radius,
                                d_out, info);
}

int la3dm_devmap_nearest_points_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *points3, uint32_t n_points,
                                     const float *pose12, uint32_t obstacle_mask, uint32_t radius, const la3dm_nearest_points_out *out,
                                     la3dm_region_info *info) {
    return nearest_points_query(dm, true, "la3dm_devmap_nearest_points_host", lo3, dims3, points3, n_points, pose12, obstacle_mask, radius, out,
                                info);
}

// ---- frontier of a region (devmap_frontier.h) -----------------------------------------------------------------

// the instantiation of a kernel template <int kConn> for a connectivity that the query's check has found to be 6, 18 or 26
#define DM_BY_CONNECTIVITY(kernel, connectivity) \
    ((connectivity) == 6 ? kernel<6> : (connectivity) == 18 ? kernel<18> : kernel<26>)

// Bits, stencil, scan and (cap > 0) emit on the map's stream; o's arrays are device memory.  d_total: where the launches
// leave the number of frontier voxels (a word of the query's working storage).
static int frontier_launch(la3dm_devmap *dm, const RegionGeom &g, uint32_t open_mask, uint32_t unknown_mask, uint32_t connectivity,
                           uint32_t min_neighbours, uint64_t cap, const la3dm_frontier_out &o, const uint32_t *&d_total) {
    hipStream_t st = dm->ctx->stream;
    RegionArgs a = region_args(dm, g);
    for (int k = 0; k < 3; ++k) a.g0[k] = g.g0[k] - 1u;   // (frontier_query's region check: g0 >= 1)
    a.nx = g.dims[0] + 2u;
    a.ny = g.dims[1] + 2u;
    a.nz = g.dims[2] + 2u;
    a.total = a.nx * a.ny * a.nz;   // <= LA3DM_FR_MAX_CELLS
    const uint32_t n_words = cdiv(a.total, 32);
    const size_t stride = ((size_t)n_words + 1 + 3) & ~(size_t)3;   // every array 16-byte aligned (the scan's vector path)
    DM_RESERVE(dm->fr_work, 16ull * stride);
    uint32_t *base = (uint32_t *)dm->fr_work.ptr;
    FrontierArgs f;
    memset(&f, 0, sizeof(f));
    f.nx = g.dims[0];
    f.ny = g.dims[1];
    f.nz = g.dims[2];
    f.PY = a.ny;
    f.PZ = a.nz;
    f.total = a.total;
    f.n_words = n_words;
    f.min_neighbours = min_neighbours;
    f.open = base;
    f.unknown = base + stride;
    f.count = base + 2 * stride;
    f.offset = base + 3 * stride;
    f.cap = cap;
    f.index = cap ? o.index : nullptr;
    f.nbrs = cap ? o.nbrs : nullptr;
    f.score = o.score;
    if (o.score) DM_TRY(hipMemsetAsync(o.score, 0, (size_t)g.total, st));
    hipLaunchKernelGGL(dm_fr_bits, dim3(cdiv(a.total, 256)), dim3(256), 0, st, a, open_mask, unknown_mask, f.open, base + stride);
    const dim3 wgrid(cdiv(n_words + 1, 256));
    hipLaunchKernelGGL(DM_BY_CONNECTIVITY(dm_fr_stencil, connectivity), wgrid, dim3(256), 0, st, f);
    DM_TRY(hipGetLastError());
    dm->counters_clean = false;   // (the scan may flag a dirty state in the counter block)
    int rc = exclusive_scan(dm, f.count, base + 3 * stride, n_words + 1);
    if (rc != LA3DM_OK) return rc;
    if (cap) {
        hipLaunchKernelGGL(DM_BY_CONNECTIVITY(dm_fr_emit, connectivity), wgrid, dim3(256), 0, st, f);
        DM_TRY(hipGetLastError());
    }
    d_total = f.offset + n_words;
    return LA3DM_OK;
}

// empty map: every voxel and its surroundings are MISSING — all voxels are frontier (the list 0, 1, 2, ... until cap) or
// none; the pool is not read
static int frontier_empty(const Fill &f, size_t n, uint32_t open_mask, uint32_t unknown_mask, uint32_t connectivity, uint64_t cap,
                          const la3dm_frontier_out &o, uint32_t &total) {
    const bool all = ((open_mask & unknown_mask) >> LA3DM_RAY_MISSING) & 1u;
    total = all ? (uint32_t)n : 0u;
    DM_OK(f.bytes(o.score, all ? (int)connectivity : 0, n));
    const uint32_t m = (uint32_t)std::min<uint64_t>(total, cap);
    if (m && f.host) {
        for (uint32_t t = 0; t < m; ++t) {
            o.index[t] = t;
            if (o.nbrs) o.nbrs[t] = (uint8_t)connectivity;
        }
    } else if (m) {
        la3dm_devmap *dm = f.dm;
        hipLaunchKernelGGL(dm_fr_all, dim3(cdiv(m, 256)), dim3(256), 0, dm->ctx->stream, o.index, o.nbrs, m, connectivity);
        DM_TRY(hipGetLastError());
    }
    return LA3DM_OK;
}

static int frontier_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3, uint32_t open_mask,
                          uint32_t unknown_mask, uint32_t connectivity, uint32_t min_neighbours, uint64_t cap,
                          const la3dm_frontier_out *out, uint64_t *n_found, la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(refuse(dm, who, la3dm_region::frontier_check(open_mask, unknown_mask, connectivity, min_neighbours)));
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::kFrontier, true, true, who, g));   // lo, dims, the limit and the range: before any buffer
    if (cap > 0 && !out) return refuse(dm, who, "out is NULL with cap > 0");
    if (cap > 0 && !out->index) return refuse(dm, who, "out->index must not be NULL with cap > 0");
    if (!n_found) return refuse(dm, who, "n_found is NULL");
    hipStream_t st = dm->ctx->stream;
    la3dm_frontier_out o;
    memset(&o, 0, sizeof(o));
    if (out) o = *out;
    const size_t n = (size_t)g.total;
    uint32_t total = 0;
    if (dm->n_blocks == 0) {
        DM_OK(frontier_empty(Fill{dm, host}, n, open_mask, unknown_mask, connectivity, cap, o, total));
        DM_TRY(hipStreamSynchronize(st));
    } else {
        // the list has at most one entry per voxel and no more than cap; only what was found is copied back
        const size_t room = (size_t)std::min<uint64_t>(cap, n);
        Stage s(dm, host);
        const int i_index = s.out(o.index, room), i_nbrs = s.out(o.nbrs, room);
        s.out(o.score, n);
        DM_OK(s.reserve());
        const uint32_t *d_total = nullptr;
        DM_OK(frontier_launch(dm, g, open_mask, unknown_mask, connectivity, min_neighbours, room, o, d_total));
        DM_TRY(hipMemcpyAsync(&total, d_total, 4, hipMemcpyDeviceToHost, st));
        DM_TRY(hipStreamSynchronize(st));
        s.count(i_index, total);
        s.count(i_nbrs, total);
        DM_OK(s.download());
        if (host) DM_TRY(hipStreamSynchronize(st));
    }
    *n_found = total;
    if (info) *info = g.info;
    return LA3DM_OK;
}

int la3dm_devmap_frontier_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, uint32_t open_mask,
                                 uint32_t unknown_mask, uint32_t connectivity, uint32_t min_neighbours, uint64_t cap,
                                 const la3dm_frontier_out *d_out, uint64_t *n_found, la3dm_region_info *info) {
    return frontier_query(dm, false, "la3dm_devmap_frontier_device", lo3, dims3, open_mask, unknown_mask, connectivity, min_neighbours, cap,
                          d_out, n_found, info);
}

int la3dm_devmap_frontier_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, uint32_t open_mask,
                               uint32_t unknown_mask, uint32_t connectivity, uint32_t min_neighbours, uint64_t cap,
                               const la3dm_frontier_out *out, uint64_t *n_found, la3dm_region_info *info) {
    return frontier_query(dm, true, "la3dm_devmap_frontier_host", lo3, dims3, open_mask, unknown_mask, connectivity, min_neighbours, cap, out,
                          n_found, info);
}

// ---- footing of a region (devmap_footing.h) --------------------------------------------------------------------

// Bits, derive and foot on the map's stream: footing's launches up to the foot words, which lie in f.stand afterwards (the
// popcounts in f.count, the partial counts in f.stats).  Fills f but for cap and the output arrays.  drive's footing mode
// stops here.
static int footing_words(la3dm_devmap *dm, const RegionGeom &g, const la3dm_footing_params &p, FootingArgs &f) {
    hipStream_t st = dm->ctx->stream;
    RegionArgs a = region_args(dm, g);
    a.g0[0] = g.g0[0] - p.radius;   // (footing_query's region check: g0 >= the pad below)
    a.g0[1] = g.g0[1] - p.radius;
    a.g0[2] = g.g0[2] - (1u + p.step);
    a.nx = g.dims[0] + 2u * p.radius;
    a.ny = g.dims[1] + 2u * p.radius;
    a.nz = g.dims[2] + p.headroom + 2u * p.step;
    a.total = a.nx * a.ny * a.nz;   // <= LA3DM_FOOTING_MAX_CELLS
    const uint32_t n_words = cdiv(a.total, 32);
    const size_t stride = ((size_t)n_words + 1 + 3) & ~(size_t)3;   // every array 16-byte aligned (the scan's vector path)
    DM_RESERVE(dm->ft_work, 4ull * (7 * stride + 3 * kFtWaves));
    uint32_t *base = (uint32_t *)dm->ft_work.ptr;
    memset(&f, 0, sizeof(f));
    f.nx = g.dims[0];
    f.ny = g.dims[1];
    f.nz = g.dims[2];
    f.PY = a.ny;
    f.PZ = a.nz;
    f.h = p.headroom;
    f.r = p.radius;
    f.s = p.step;
    f.c = p.min_support;
    f.total = a.total;
    f.n_words = n_words;
    f.support = base;
    f.clear = base + stride;
    f.stand = base + 2 * stride;
    f.near = base + 3 * stride;
    f.body = base + 4 * stride;
    f.count = base + 5 * stride;
    f.offset = base + 6 * stride;
    f.stats = base + 7 * stride;
    hipLaunchKernelGGL(dm_ft_bits, dim3(cdiv(a.total, 256)), dim3(256), 0, st, a, p.support_mask, p.clear_mask, base, base + stride);
    hipLaunchKernelGGL(dm_ft_derive, dim3(cdiv(n_words, 256)), dim3(256), 0, st, f);
    hipLaunchKernelGGL(dm_ft_foot, dim3(kFtWaves / 4), dim3(256), 0, st, f);   // four waves per workgroup
    DM_TRY(hipGetLastError());
    return LA3DM_OK;
}

// footing_words, scan, (cap > 0) emit and (a dense array) columns on the map's stream; o's arrays are device memory.
// d_stats: where the launches leave the kFtWaves partial counts of n_stand, n_body and n_foot (working storage).
static int footing_launch(la3dm_devmap *dm, const RegionGeom &g, const la3dm_footing_params &p, uint64_t cap, const la3dm_footing_out &o,
                          const uint32_t *&d_stats) {
    hipStream_t st = dm->ctx->stream;
    FootingArgs f;
    int rc = footing_words(dm, g, p, f);
    if (rc != LA3DM_OK) return rc;
    f.cap = cap;
    f.index = cap ? o.index : nullptr;
    f.levels = o.levels;
    f.lowest = o.lowest;
    f.highest = o.highest;
    const uint32_t n_words = f.n_words;
    const dim3 wgrid(cdiv(n_words + 1, 256));
    dm->counters_clean = false;   // (the scan may flag a dirty state in the counter block)
    rc = exclusive_scan(dm, f.count, const_cast<uint32_t *>(f.offset), n_words + 1);
    if (rc != LA3DM_OK) return rc;
    if (cap) hipLaunchKernelGGL(dm_ft_emit, wgrid, dim3(256), 0, st, f);
    if (o.levels || o.lowest || o.highest)
        hipLaunchKernelGGL(dm_ft_columns, dim3(cdiv((uint64_t)g.dims[0] * g.dims[1], 256)), dim3(256), 0, st, f);
    DM_TRY(hipGetLastError());
    d_stats = f.stats;
    return LA3DM_OK;
}

static int footing_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3,
                         const la3dm_footing_params *params, uint64_t cap, const la3dm_footing_out *out, uint64_t *n_found,
                         la3dm_footing_stats *stats, la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(refuse(dm, who, la3dm_region::footing_check(params, cap, out && out->index, "->")));
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::footing_query(*params), true, true, who, g));   // lo, dims, the limit and the range
    if (!n_found) return refuse(dm, who, "n_found is NULL");
    hipStream_t st = dm->ctx->stream;
    la3dm_footing_out o;
    memset(&o, 0, sizeof(o));
    if (out) o = *out;
    const size_t n = (size_t)g.total, n_col = (size_t)g.dims[0] * g.dims[1];
    uint32_t counts[3] = {0, 0, 0};
    if (dm->n_blocks == 0) {   // every voxel MISSING, and the masks do not overlap: nothing stands
        const Fill f{dm, host};
        DM_OK(f.bytes(o.levels, 0, 4 * n_col));
        DM_OK(f.bytes(o.lowest, 0xFF, 4 * n_col));
        DM_OK(f.bytes(o.highest, 0xFF, 4 * n_col));
        DM_TRY(hipStreamSynchronize(st));
    } else {
        // the list has at most one entry per voxel and no more than cap; only what was found is copied back
        const size_t room = (size_t)std::min<uint64_t>(cap, n);
        Stage s(dm, host);
        const int i_index = s.out(o.index, room);
        s.out(o.levels, n_col);
        s.out(o.lowest, n_col);
        s.out(o.highest, n_col);
        DM_OK(s.reserve());
        const uint32_t *d_stats = nullptr;
        DM_OK(footing_launch(dm, g, *params, room, o, d_stats));
        std::vector<uint32_t> partial(3 * kFtWaves);
        DM_TRY(hipMemcpyAsync(partial.data(), d_stats, 4 * partial.size(), hipMemcpyDeviceToHost, st));
        DM_TRY(hipStreamSynchronize(st));
        for (size_t t = 0; t < partial.size(); ++t) counts[t % 3] += partial[t];   // (each sum is at most the voxels of the region)
        s.count(i_index, counts[2]);
        DM_OK(s.download());
        if (host) DM_TRY(hipStreamSynchronize(st));
    }
    *n_found = counts[2];
    if (stats) *stats = la3dm_footing_stats{counts[0], counts[1], counts[2], la3dm_footing::disc_cells(params->radius)};
    if (info) *info = g.info;
    return LA3DM_OK;
}

int la3dm_devmap_footing_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_footing_params *params,
                                uint64_t cap, const la3dm_footing_out *d_out, uint64_t *n_found, la3dm_footing_stats *stats,
                                la3dm_region_info *info) {
    return footing_query(dm, false, "la3dm_devmap_footing_device", lo3, dims3, params, cap, d_out, n_found, stats, info);
}

int la3dm_devmap_footing_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_footing_params *params,
                              uint64_t cap, const la3dm_footing_out *out, uint64_t *n_found, la3dm_footing_stats *stats,
                              la3dm_region_info *info) {
    return footing_query(dm, true, "la3dm_devmap_footing_host", lo3, dims3, params, cap, out, n_found, stats, info);
}

// ---- surface of a region (devmap_surface.h) --------------------------------------------------------------------

// Bits, faces, scan, (cap > 0) emit, (smooth > 0 and a normal array) normals and (the dense array) dense on the map's stream;
// o's arrays are device memory.  d_stats: where the launches leave the kSfWaves partial counts (working storage).
static int surface_launch(la3dm_devmap *dm, const RegionGeom &g, const la3dm_surface_params &p, uint64_t cap, const la3dm_surface_out &o,
                          const uint32_t *&d_stats) {
    hipStream_t st = dm->ctx->stream;
    const uint32_t pad = p.smooth + 1u;
    RegionArgs a = region_args(dm, g);
    for (int k = 0; k < 3; ++k) a.g0[k] = g.g0[k] - pad;   // (surface_query's region check: g0 >= the pad below)
    a.nx = g.dims[0] + 2u * pad;
    a.ny = g.dims[1] + 2u * pad;
    a.nz = g.dims[2] + 2u * pad;
    a.total = a.nx * a.ny * a.nz;   // <= LA3DM_SURFACE_MAX_CELLS
    const uint32_t n_words = cdiv(a.total, 32);
    const size_t stride = ((size_t)n_words + 1 + 3) & ~(size_t)3;   // every array 16-byte aligned (the scan's vector path)
    DM_RESERVE(dm->sf_work, 4ull * (11 * stride + 8 * kSfWaves));
    uint32_t *base = (uint32_t *)dm->sf_work.ptr;
    SurfaceArgs f;
    memset(&f, 0, sizeof(f));
    f.nx = g.dims[0];
    f.ny = g.dims[1];
    f.nz = g.dims[2];
    f.PY = a.ny;
    f.PZ = a.nz;
    f.s = p.smooth;
    f.pad = pad;
    f.total = a.total;
    f.n_words = n_words;
    const bool normals = p.smooth > 0 && cap > 0 && o.normal != nullptr;
    f.store_faces = normals || o.dense_faces != nullptr;
    f.solid = base;
    f.open = base + stride;
    f.face = base + 2 * stride;
    f.stride = (uint32_t)stride;
    f.cand = base + 8 * stride;
    f.count = base + 9 * stride;
    f.offset = base + 10 * stride;
    f.stats = base + 11 * stride;
    f.cap = cap;
    f.index = cap ? o.index : nullptr;
    f.faces = cap ? o.faces : nullptr;
    f.normal = cap ? o.normal : nullptr;
    f.dense = o.dense_faces;
    hipLaunchKernelGGL(dm_ft_bits, dim3(cdiv(a.total, 256)), dim3(256), 0, st, a, p.solid_mask, p.open_mask, base, base + stride);
    hipLaunchKernelGGL(dm_sf_faces, dim3(kSfWaves / 4), dim3(256), 0, st, f);   // four waves per workgroup
    DM_TRY(hipGetLastError());
    dm->counters_clean = false;   // (the scan may flag a dirty state in the counter block)
    int rc = exclusive_scan(dm, f.count, base + 10 * stride, n_words + 1);
    if (rc != LA3DM_OK) return rc;
    if (cap) hipLaunchKernelGGL(dm_sf_emit, dim3(cdiv(n_words, 256)), dim3(256), 0, st, f);
    if (normals) hipLaunchKernelGGL(dm_sf_normals, dim3(kSfWaves / 4), dim3(256), 0, st, f);
    if (f.dense) hipLaunchKernelGGL(dm_sf_dense, dim3(cdiv(g.total, 256)), dim3(256), 0, st, f);
    DM_TRY(hipGetLastError());
    d_stats = f.stats;
    return LA3DM_OK;
}

static int surface_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3,
                         const la3dm_surface_params *params, uint64_t cap, const la3dm_surface_out *out, uint64_t *n_found,
                         la3dm_surface_stats *stats, la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(refuse(dm, who, la3dm_region::surface_check(params, cap, out, "->")));
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::surface_query(*params), true, true, who, g));   // lo, dims, the limit and the range
    if (!n_found) return refuse(dm, who, "n_found is NULL");
    hipStream_t st = dm->ctx->stream;
    la3dm_surface_out o;
    memset(&o, 0, sizeof(o));
    if (out) o = *out;
    const size_t n = (size_t)g.total;
    uint64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // solid, the six directions, surface voxels
    if (dm->n_blocks == 0) {   // every voxel MISSING, and the masks do not overlap: no face, and all or no voxel solid
        if ((params->solid_mask >> LA3DM_RAY_MISSING) & 1u) counts[0] = n;
        const Fill f{dm, host};
        DM_OK(f.bytes(o.dense_faces, 0, n));
        DM_TRY(hipStreamSynchronize(st));
    } else {
        // the list has at most one entry per voxel and no more than cap; only what was found is copied back
        const size_t room = (size_t)std::min<uint64_t>(cap, n);
        Stage s(dm, host);
        const int i_index = s.out(o.index, room);
        const int i_faces = s.out(o.faces, room);
        const int i_normal = s.out(o.normal, 3 * room);
        s.out(o.dense_faces, n);
        DM_OK(s.reserve());
        const uint32_t *d_stats = nullptr;
        DM_OK(surface_launch(dm, g, *params, room, o, d_stats));
        // (a one-workgroup launch that adds the partial counts on the device, so that 32 bytes come back, was measured: it
        // takes 8 us and the call gets no faster — DESIGN.md 3.24)
        std::vector<uint32_t> partial(8 * kSfWaves);
        DM_TRY(hipMemcpyAsync(partial.data(), d_stats, 4 * partial.size(), hipMemcpyDeviceToHost, st));
        DM_TRY(hipStreamSynchronize(st));
        for (size_t t = 0; t < partial.size(); ++t) counts[t % 8] += partial[t];   // (each sum is at most the voxels of the region)
        s.count(i_index, counts[7]);
        s.count(i_faces, counts[7]);
        s.count(i_normal, 3 * counts[7]);
        DM_OK(s.download());
        if (host) DM_TRY(hipStreamSynchronize(st));
    }
    *n_found = counts[7];
    if (stats) {
        stats->n_solid = counts[0];
        stats->n_surface = counts[7];
        for (int d = 0; d < 6; ++d) stats->faces[d] = counts[1 + d];
    }
    if (info) *info = g.info;
    return LA3DM_OK;
}

int la3dm_devmap_surface_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_surface_params *params,
                                uint64_t cap, const la3dm_surface_out *d_out, uint64_t *n_found, la3dm_surface_stats *stats,
                                la3dm_region_info *info) {
    return surface_query(dm, false, "la3dm_devmap_surface_device", lo3, dims3, params, cap, d_out, n_found, stats, info);
}

int la3dm_devmap_surface_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_surface_params *params,
                              uint64_t cap, const la3dm_surface_out *out, uint64_t *n_found, la3dm_surface_stats *stats,
                              la3dm_region_info *info) {
    return surface_query(dm, true, "la3dm_devmap_surface_host", lo3, dims3, params, cap, out, n_found, stats, info);
}

// ---- gain of candidate viewpoints (devmap_gain.h) ---------------------------------------------------------------

// Zeroing, mark and count on the map's stream; every pointer is device memory.  o.seen null: the sets live in the arena;
// `sets` returns where they are.
static int gain_launch(la3dm_devmap *dm, const RegionGeom &g, const float *d_origins3, uint32_t n, const float *d_offsets3,
                       uint32_t m, uint32_t count_mask, uint32_t stop_mask, uint32_t max_steps, const la3dm_gain_out &o,
                       const uint32_t *&sets) {
    hipStream_t st = dm->ctx->stream;
    const uint32_t W = la3dm_region::gain_words(g.total);
    const size_t words = (size_t)n * W;   // <= LA3DM_GAIN_MAX_WORDS
    uint32_t *seen = o.seen;
    if (!seen) {
        DM_RESERVE(dm->gain_work, 4ull * words);
        seen = (uint32_t *)dm->gain_work.ptr;
    }
    GainArgs a;
    memset(&a, 0, sizeof(a));
    a.origins = d_origins3;
    a.offsets = d_offsets3;
    a.n = n;
    a.m = m;
    a.chunks = cdiv(m, 256);
    a.count_mask = count_mask;
    a.stop_mask = stop_mask;
    a.max_steps = max_steps;
    a.block_size = dm->block_size;
    a.resolution = dm->ctx->p.resolution;
    a.pool = pool_view(dm);
    for (int k = 0; k < 3; ++k) a.g0[k] = g.g0[k];
    a.nx = g.dims[0];
    a.ny = g.dims[1];
    a.nz = g.dims[2];
    a.W = W;
    a.seen = seen;
    a.started = o.started;
    a.hits = o.hits;
    DM_TRY(hipMemsetAsync(seen, 0, 4ull * words, st));
    DM_TRY(hipMemsetAsync(o.gain, 0, 4ull * n, st));
    if (o.started) DM_TRY(hipMemsetAsync(o.started, 0, 4ull * n, st));
    if (o.hits) DM_TRY(hipMemsetAsync(o.hits, 0, 4ull * n, st));
    // (n chunks <= n m / 256 + n <= 2^20 + 2^28 workgroups, and n ceil(W / 256) <= 2^20 + 2^28: both fit the grid's x)
    hipLaunchKernelGGL(dm_gain_mark, dim3(n * a.chunks), dim3(256), 0, st, a);
    const uint32_t wchunks = cdiv(W, 256);
    hipLaunchKernelGGL(dm_gain_count, dim3(n * wchunks), dim3(256), 0, st, (const uint32_t *)seen, W, wchunks, o.gain);
    DM_TRY(hipGetLastError());
    sets = seen;
    return LA3DM_OK;
}

// empty map: no ray starts
static int gain_empty(const Fill &f, size_t n, size_t words, const la3dm_gain_out &o) {
    DM_OK(f.bytes(o.gain, 0, 4 * n));
    DM_OK(f.bytes(o.started, 0, 4 * n));
    DM_OK(f.bytes(o.hits, 0, 4 * n));
    return f.bytes(o.seen, 0, 4 * words);
}

static int gain_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3, const float *origins3,
                      uint32_t n, const float *offsets3, uint32_t m, uint32_t count_mask, uint32_t stop_mask, uint32_t max_steps,
                      const la3dm_gain_out *out, la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(refuse(dm, who, la3dm_region::gain_check(count_mask, stop_mask, max_steps, n, m)));
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::kGain, true, true, who, g));   // lo, dims, the limit and the range: before any buffer
    DM_OK(refuse(dm, who, la3dm_region::gain_buffers(g.total, n, origins3 != nullptr, offsets3 != nullptr, out != nullptr, out && out->gain, "->")));
    if (info) *info = g.info;
    if (n == 0) return LA3DM_OK;
    hipStream_t st = dm->ctx->stream;
    la3dm_gain_out o = *out;
    const size_t words = (size_t)n * la3dm_region::gain_words(g.total);
    if (dm->n_blocks == 0) {
        DM_OK(gain_empty(Fill{dm, host}, n, words, o));
    } else {
        // host pointers: the sets stay in their own arena (gain_launch) and are copied from there
        uint32_t *h_seen = host ? o.seen : nullptr;
        if (host) o.seen = nullptr;
        Stage s(dm, host);
        s.in(origins3, 3ull * n);
        s.in(offsets3, 3ull * m);
        s.out(o.gain, n);
        s.out(o.started, n);
        s.out(o.hits, n);
        DM_OK(s.reserve());
        const uint32_t *sets = nullptr;
        DM_OK(gain_launch(dm, g, origins3, n, offsets3, m, count_mask, stop_mask, max_steps, o, sets));
        DM_OK(s.download());
        if (h_seen) DM_TRY(hipMemcpyAsync(h_seen, sets, 4ull * words, hipMemcpyDeviceToHost, st));
    }
    DM_TRY(hipStreamSynchronize(st));
    return LA3DM_OK;
}

int la3dm_devmap_gain_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *d_origins3, uint32_t n,
                             const float *d_offsets3, uint32_t m, uint32_t count_mask, uint32_t stop_mask, uint32_t max_steps,
                             const la3dm_gain_out *d_out, la3dm_region_info *info) {
    return gain_query(dm, false, "la3dm_devmap_gain_device", lo3, dims3, d_origins3, n, d_offsets3, m, count_mask, stop_mask, max_steps, d_out,
                      info);
}

int la3dm_devmap_gain_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *origins3, uint32_t n,
                           const float *offsets3, uint32_t m, uint32_t count_mask, uint32_t stop_mask, uint32_t max_steps,
                           const la3dm_gain_out *out, la3dm_region_info *info) {
    return gain_query(dm, true, "la3dm_devmap_gain_host", lo3, dims3, origins3, n, offsets3, m, count_mask, stop_mask, max_steps, out, info);
}

// ---- score_poses: one scan under many poses against the distance field of a region (devmap_score.h) ----------------

// Stage 1 (the obstacle field, into working storage) and stage 2 on the map's stream; every pointer is device memory.
static int score_launch(la3dm_devmap *dm, const RegionGeom &g, const float *d_points3, uint32_t n_points, const float *d_poses12,
                        uint32_t n_poses, uint32_t obstacle_mask, uint32_t radius, const la3dm_score_out &o) {
    hipStream_t st = dm->ctx->stream;
    const size_t n = (size_t)g.total;
    ScoreArgs a;
    memset(&a, 0, sizeof(a));
    a.points = d_points3;
    a.poses = d_poses12;
    a.n_points = n_points;
    a.n_poses = n_poses;
    // Few poses: the cloud is cut into chunks until about four workgroups per compute unit exist, 256 points a chunk at
    // least; the chunks' records are then added by dm_score_fold.
    a.chunks = std::max(1u, std::min(cdiv(1024, n_poses), cdiv(n_points, 256)));
    a.per_chunk = cdiv(cdiv(n_points, a.chunks), 256) * 256u;
    a.resolution = dm->ctx->p.resolution;
    a.block_size = dm->block_size;
    a.lim = 1 << (dm->depth - 1);
    for (int k = 0; k < 3; ++k) {
        a.g0[k] = g.g0[k];
        a.dims[k] = g.dims[k];
    }
    const size_t d2_bytes = (4 * n + 15) & ~(size_t)15;
    DM_RESERVE(dm->score_work, d2_bytes + (a.chunks > 1 ? 4ull * kScoreWords * n_poses * a.chunks : 0));
    a.partial = (uint32_t *)((char *)dm->score_work.ptr + d2_bytes);
    a.sum_d2 = (uint32_t *)o.sum_d2;
    a.counts = o.counts;
    DM_OK(obstacle_field(dm, g, obstacle_mask, radius, (uint32_t *)dm->score_work.ptr, a.cost));
    // (n_poses chunks <= 2^20 + 1024 workgroups)
    hipLaunchKernelGGL(dm_score_pairs, dim3(n_poses * a.chunks), dim3(256), 0, st, a);
    if (a.chunks > 1) hipLaunchKernelGGL(dm_score_fold, dim3(n_poses), dim3(64), 0, st, a);
    DM_TRY(hipGetLastError());
    return LA3DM_OK;
}

static int score_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3, const float *points3,
                       uint32_t n_points, const float *poses12, uint32_t n_poses, uint32_t obstacle_mask, uint32_t radius,
                       const la3dm_score_out *out, la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(refuse(dm, who, la3dm_region::score_check(obstacle_mask, radius, n_points, n_poses)));
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::kScore, true, true, who, g));   // lo, dims, the limit and the range: before any buffer
    DM_OK(refuse(dm, who, la3dm_region::score_buffers(n_points, n_poses, points3 != nullptr, poses12 != nullptr, out != nullptr,
                                                      out && out->sum_d2, "->")));
    if (info) *info = g.info;
    if (n_poses == 0) return LA3DM_OK;
    hipStream_t st = dm->ctx->stream;
    la3dm_score_out o = *out;
    if (n_points == 0) {   // no pair: zeros, no launch
        const Fill f{dm, host};
        DM_OK(f.bytes(o.sum_d2, 0, 8ull * n_poses));
        DM_OK(f.bytes(o.counts, 0, 20ull * n_poses));
    } else {
        Stage s(dm, host);
        s.in(points3, 3ull * n_points);
        s.in(poses12, 12ull * n_poses);
        s.out(o.sum_d2, n_poses);
        s.out(o.counts, 5ull * n_poses);
        DM_OK(s.reserve());
        DM_OK(score_launch(dm, g, points3, n_points, poses12, n_poses, obstacle_mask, radius, o));
        DM_OK(s.download());
    }
    DM_TRY(hipStreamSynchronize(st));
    return LA3DM_OK;
}

int la3dm_devmap_score_poses_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *d_points3, uint32_t n_points,
                                    const float *d_poses12, uint32_t n_poses, uint32_t obstacle_mask, uint32_t radius,
                                    const la3dm_score_out *d_out, la3dm_region_info *info) {
    return score_query(dm, false, "la3dm_devmap_score_poses_device", lo3, dims3, d_points3, n_points, d_poses12, n_poses, obstacle_mask, radius,
                       d_out, info);
}

int la3dm_devmap_score_poses_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *points3, uint32_t n_points,
                                  const float *poses12, uint32_t n_poses, uint32_t obstacle_mask, uint32_t radius,
                                  const la3dm_score_out *out, la3dm_region_info *info) {
    return score_query(dm, true, "la3dm_devmap_score_poses_host", lo3, dims3, points3, n_points, poses12, n_poses, obstacle_mask, radius, out,
                       info);
}

// ---- score_paths: many polylines walked through the distance field of a region (devmap_paths.h) --------------------

// Stage 1 (the obstacle field, into score_poses' arena) and stage 2 on the map's stream; every pointer is device memory.
static int paths_launch(la3dm_devmap *dm, const RegionGeom &g, const float *d_ways3, uint32_t n_paths, uint32_t n_way,
                        const la3dm_paths_params &p, const la3dm_paths_out &o) {
    hipStream_t st = dm->ctx->stream;
    PathsArgs a;
    memset(&a, 0, sizeof(a));
    a.ways = d_ways3;
    a.n_paths = n_paths;
    a.n_way = n_way;
    a.resolution = dm->ctx->p.resolution;
    a.block_size = dm->block_size;
    a.lim = 1 << (dm->depth - 1);
    for (int k = 0; k < 3; ++k) {
        a.g0[k] = g.g0[k];
        a.dims[k] = g.dims[k];
    }
    a.p = p;
    a.cost = (uint32_t *)o.cost;
    a.steps = o.steps;
    a.stop = o.stop;
    a.min_d2 = o.min_d2;
    a.reached = o.ways;
    a.flags = o.flags;
    if (dm->n_blocks) DM_RESERVE(dm->score_work, 4ull * (size_t)g.total);   // (an empty map has no transform to hold)
    DM_OK(obstacle_field(dm, g, p.obstacle_mask, la3dm_region::paths_radius(p), (uint32_t *)dm->score_work.ptr, a.field));
    // (at most 2^18 workgroups; 16 bytes of LDS per waypoint and wave: at most 64 KB)
    hipLaunchKernelGGL(dm_paths_walk, dim3(cdiv(n_paths, kPathsWaves)), dim3(64 * kPathsWaves), 16ull * kPathsWaves * n_way, st, a);
    DM_TRY(hipGetLastError());
    return LA3DM_OK;
}

static int paths_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3, const float *ways3,
                       uint32_t n_paths, uint32_t n_way, const la3dm_paths_params *params, const la3dm_paths_out *out,
                       la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(refuse(dm, who, la3dm_region::paths_check(params, n_paths, n_way, ways3 != nullptr, out != nullptr, out && out->cost, "->")));
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::kPaths, true, true, who, g));   // lo, dims, the limit and the range: before any buffer
    if (info) *info = g.info;
    if (n_paths == 0) return LA3DM_OK;
    la3dm_paths_out o = *out;
    Stage s(dm, host);
    s.in(ways3, 3ull * n_paths * n_way);
    s.out(o.cost, n_paths);
    s.out(o.steps, n_paths);
    s.out(o.stop, n_paths);
    s.out(o.min_d2, n_paths);
    s.out(o.ways, n_paths);
    s.out(o.flags, n_paths);
    DM_OK(s.reserve());
    DM_OK(paths_launch(dm, g, ways3, n_paths, n_way, *params, o));
    DM_OK(s.download());
    DM_TRY(hipStreamSynchronize(dm->ctx->stream));
    return LA3DM_OK;
}

int la3dm_devmap_score_paths_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *d_ways3, uint32_t n_paths,
                                    uint32_t n_way, const la3dm_paths_params *params, const la3dm_paths_out *d_out,
                                    la3dm_region_info *info) {
    return paths_query(dm, false, "la3dm_devmap_score_paths_device", lo3, dims3, d_ways3, n_paths, n_way, params, d_out, info);
}

int la3dm_devmap_score_paths_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *ways3, uint32_t n_paths,
                                  uint32_t n_way, const la3dm_paths_params *params, const la3dm_paths_out *out, la3dm_region_info *info) {
    return paths_query(dm, true, "la3dm_devmap_score_paths_host", lo3, dims3, ways3, n_paths, n_way, params, out, info);
}

// ---- reach: hop distance from seeds through the passable voxels of a region (devmap_reach.h) -------------------------

// The whole query on the map's stream; every pointer but `stats` is device memory.  The working storage is initialised
// here on every call.  d_steps: where the dense steps are — o.steps, or the query's working storage when the caller gave
// no array for them.  The level launches are queued LA3DM_REACH_BATCH at a time; the counts of a batch are then read, and
// the first level that reached nothing ends the loop (the levels queued behind it saw an empty front).
static int reach_launch(la3dm_devmap *dm, const RegionGeom &g, const uint32_t *d_seeds, uint32_t n_seeds, uint32_t pass_mask,
                        uint32_t obstacle_mask, uint32_t clearance, uint32_t connectivity, uint32_t max_steps,
                        const uint32_t *d_targets, uint32_t n_targets, const la3dm_reach_out &o, la3dm_reach_stats &stats,
                        const uint32_t *&d_steps) {
    hipStream_t st = dm->ctx->stream;
    const size_t n = (size_t)g.total;
    ReachArgs a;
    memset(&a, 0, sizeof(a));
    a.nx = g.dims[0];
    a.ny = g.dims[1];
    a.nz = g.dims[2];
    a.PY = a.ny + 2u;
    a.PZ = a.nz + 2u;
    a.total = (a.nx + 2u) * a.PY * a.PZ;   // <= LA3DM_REACH_MAX_CELLS
    a.n_words = cdiv(a.total, 32);
    a.n_cells = (uint32_t)n;
    const size_t stride = ((size_t)a.n_words + 3) & ~(size_t)3, n_count = ((size_t)max_steps + 1 + 3) & ~(size_t)3;
    // layout: pass | reached | front 0 | front 1 | counts | cells.  `cells` (4 bytes per voxel) is d2 while dm_rc_bits reads
    // it and the steps from the fill behind that launch on, where the caller gave no array for them: the order of the
    // stream is what keeps the two uses apart.
    DM_RESERVE(dm->reach_work, 4ull * (4 * stride + n_count + n));
    uint32_t *base = (uint32_t *)dm->reach_work.ptr;
    uint32_t *pass = base, *front[2] = {base + 2 * stride, base + 3 * stride}, *cells = base + 4 * stride + n_count;
    a.pass = pass;
    a.reached = base + stride;
    a.count = base + 4 * stride;
    const bool empty = dm->n_blocks == 0;   // every voxel MISSING: the pool is not read
    ObstacleField field;   // a voxel passes where its word is FAR: everywhere without a clearance
    DM_OK(obstacle_field(dm, g, obstacle_mask, clearance, cells, field));
    DM_TRY(hipMemsetAsync(a.reached, 0, 4ull * (3 * stride + n_count), st));   // reached, both fronts, the counts
    RegionArgs r = region_args(dm, g);
    hipLaunchKernelGGL(dm_rc_bits, dim3(cdiv(a.total, 256)), dim3(256), 0, st, r, a, pass_mask, empty ? 0u : 1u, field, pass);
    DM_TRY(hipGetLastError());
    a.steps = o.steps ? o.steps : cells;   // (cells held d2 until dm_rc_bits read it)
    DM_TRY(hipMemsetAsync(a.steps, 0xFF, 4ull * n, st));
    stats.n_seeded = stats.n_reached = stats.levels = 0;
    if (n_seeds) {
        hipLaunchKernelGGL(dm_rc_seed, dim3(cdiv(n_seeds, 256)), dim3(256), 0, st, a, d_seeds, n_seeds, front[0]);
        DM_TRY(hipGetLastError());
        const auto level_kernel = DM_BY_CONNECTIVITY(dm_rc_level, connectivity);
        const dim3 wgrid(cdiv(a.n_words, 256));
        uint32_t h_count[LA3DM_REACH_BATCH + 1];
        uint32_t level = 1, turn = 0;
        bool ended = false;
        while (!ended && level <= max_steps) {   // at most max_steps / LA3DM_REACH_BATCH + 1 trips
            const uint32_t next = (uint32_t)std::min<uint64_t>((uint64_t)level + LA3DM_REACH_BATCH, (uint64_t)max_steps + 1);
            for (uint32_t l = level; l < next; ++l, turn ^= 1u)
                hipLaunchKernelGGL(level_kernel, wgrid, dim3(256), 0, st, a, (const uint32_t *)front[turn], front[turn ^ 1u], l);
            DM_TRY(hipGetLastError());
            const uint32_t from = level == 1 ? 0u : level;   // (the first batch brings n_seeded along)
            DM_TRY(hipMemcpyAsync(h_count, a.count + from, 4ull * (next - from), hipMemcpyDeviceToHost, st));
            DM_TRY(hipStreamSynchronize(st));
            if (level == 1) stats.n_seeded = stats.n_reached = h_count[0];
            for (uint32_t l = level; l < next && !ended; ++l) {
                const uint32_t c = h_count[l - from];
                if (c == 0) {
                    ended = true;
                } else {
                    stats.n_reached += c;
                    stats.levels = l;
                }
            }
            level = next;
        }
    }
    if (n_targets) {
        hipLaunchKernelGGL(dm_rc_gather, dim3(cdiv(n_targets, 256)), dim3(256), 0, st, (const uint32_t *)a.steps, a.n_cells, d_targets,
                           n_targets, o.target_steps);
        DM_TRY(hipGetLastError());
    }
    d_steps = a.steps;
    return LA3DM_OK;
}

static int reach_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3, const uint32_t *seeds,
                       uint32_t n_seeds, uint32_t pass_mask, uint32_t obstacle_mask, uint32_t clearance, uint32_t connectivity,
                       uint32_t max_steps, const uint32_t *targets, uint32_t n_targets, const la3dm_reach_out *out, la3dm_reach_stats *stats,
                       la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(refuse(dm, who, la3dm_region::reach_check(pass_mask, obstacle_mask, clearance, connectivity, max_steps, n_seeds, n_targets,
                                                    seeds != nullptr, targets != nullptr, out != nullptr, out && out->steps,
                                                    out && out->target_steps, "->")));
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::kReach, true, true, who, g));
    hipStream_t st = dm->ctx->stream;
    la3dm_reach_out o = *out;
    // host pointers: the dense steps stay in the working storage (reach_launch) and are copied from there
    uint32_t *h_steps = host ? o.steps : nullptr;
    if (host) o.steps = nullptr;
    Stage s(dm, host);
    s.in(seeds, n_seeds);
    s.in(targets, n_targets);
    s.out(o.target_steps, n_targets);
    DM_OK(s.reserve());
    la3dm_reach_stats rs;
    const uint32_t *d_steps = nullptr;
    DM_OK(reach_launch(dm, g, seeds, n_seeds, pass_mask, obstacle_mask, clearance, connectivity, max_steps, targets, n_targets, o, rs, d_steps));
    DM_OK(s.download());
    if (h_steps) DM_TRY(hipMemcpyAsync(h_steps, d_steps, 4ull * (size_t)g.total, hipMemcpyDeviceToHost, st));
    DM_TRY(hipStreamSynchronize(st));
    if (stats) *stats = rs;
    if (info) *info = g.info;
    return LA3DM_OK;
}

int la3dm_devmap_reach_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const uint32_t *d_seeds, uint32_t n_seeds,
                              uint32_t pass_mask, uint32_t obstacle_mask, uint32_t clearance, uint32_t connectivity,
                              uint32_t max_steps, const uint32_t *d_targets, uint32_t n_targets, const la3dm_reach_out *d_out,
                              la3dm_reach_stats *stats, la3dm_region_info *info) {
    return reach_query(dm, false, "la3dm_devmap_reach_device", lo3, dims3, d_seeds, n_seeds, pass_mask, obstacle_mask, clearance, connectivity,
                       max_steps, d_targets, n_targets, d_out, stats, info);
}

int la3dm_devmap_reach_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds,
                            uint32_t pass_mask, uint32_t obstacle_mask, uint32_t clearance, uint32_t connectivity,
                            uint32_t max_steps, const uint32_t *targets, uint32_t n_targets, const la3dm_reach_out *out,
                            la3dm_reach_stats *stats, la3dm_region_info *info) {
    return reach_query(dm, true, "la3dm_devmap_reach_host", lo3, dims3, seeds, n_seeds, pass_mask, obstacle_mask, clearance, connectivity,
                       max_steps, targets, n_targets, out, stats, info);
}

// ---- the host side of the brick scheme that travel and clusters share (devmap_brick.h) ---------------------------------
constexpr uint32_t kBrickCountRing = 1024;   // rounds whose counts the working storage holds before they are cleared again
static_assert(kBrickCountRing % LA3DM_TRAVEL_BATCH == 0 && kBrickCountRing % LA3DM_CLUSTERS_BATCH == 0 && kBrickCountRing % LA3DM_DRIVE_BATCH == 0,
              "a batch never straddles the ring's end");

// Fills the grid of region g and lays a query's working storage out in `work`:
//   value 0 | value 1 | `more_cells` further arrays of a word per cell | side 0 | side 1 | active 0 | active 1 | counts |
//   totals (4 words) | `own_words` words of the query's own
// `own` = where those last begin.  Nothing is cleared here: side .. totals are the words [b.side[0], own).
static int brick_layout(la3dm_devmap *dm, Arena &work, const RegionGeom &g, size_t more_cells, size_t own_words, BrickGrid &b, uint32_t *&totals,
                        uint32_t *&own) {
    b.nx = g.dims[0];
    b.ny = g.dims[1];
    b.nz = g.dims[2];
    b.BX = cdiv(b.nx, 8);
    b.BY = cdiv(b.ny, 8);
    b.BZ = cdiv(b.nz, 8);
    b.n_bricks = b.BX * b.BY * b.BZ;   // * 512 <= LA3DM_TRAVEL_MAX_CELLS, LA3DM_CLUSTERS_MAX_CELLS
    b.n_cells = (uint32_t)g.total;
    const size_t cells = (size_t)b.n_bricks * 512, per_brick = ((size_t)b.n_bricks + 3) & ~(size_t)3;
    const size_t n_small = 4 * per_brick + (size_t)kBrickCountRing * kBrickCountWords + 4;
    DM_RESERVE(work, 4ull * ((2 + more_cells) * cells + n_small + own_words));
    uint32_t *base = (uint32_t *)work.ptr, *small = base + (2 + more_cells) * cells;
    b.val[0] = base;
    b.val[1] = base + cells;
    b.side[0] = small;
    b.side[1] = small + per_brick;
    b.active[0] = small + 2 * per_brick;
    b.active[1] = small + 3 * per_brick;
    b.count = small + 4 * per_brick;
    totals = b.count + (size_t)kBrickCountRing * kBrickCountWords;
    own = small + n_small;
    return LA3DM_OK;
}

// The rounds of a query on the map's stream, kBatch at a time: launch(turn, slot) queues one round kernel.  The counts of
// a batch are then read, and the first round in which no voxel changed ends the loop (the rounds queued behind it found
// every brick inactive and only copied `side`).  `queued` = rounds launched: side[queued & 1] is the array the last of
// them wrote.  Ends in a synchronise.
extern "C++" {   // (a template, inside the C ABI's block)
template <uint32_t kBatch, class Launch>
static int brick_rounds(la3dm_devmap *dm, const BrickGrid &b, Launch launch, uint32_t max_rounds, const char *limit_text, uint32_t &queued,
                        uint32_t &rounds, uint32_t &brick_runs, uint32_t &capped) {
    hipStream_t st = dm->ctx->stream;
    uint32_t h_count[kBatch * kBrickCountWords];
    bool ended = false;
    while (!ended) {   // at most max_rounds / kBatch trips
        if (queued >= max_rounds) return dm_fail(dm, LA3DM_ERR_LIMIT, limit_text);
        const uint32_t slot = queued % kBrickCountRing;
        if (slot == 0 && queued) DM_TRY(hipMemsetAsync(b.count, 0, 4ull * kBrickCountRing * kBrickCountWords, st));
        for (uint32_t q = 0; q < kBatch; ++q) launch((queued + q) & 1u, slot + q);
        DM_TRY(hipGetLastError());
        DM_TRY(hipMemcpyAsync(h_count, b.count + (size_t)slot * kBrickCountWords, sizeof(h_count), hipMemcpyDeviceToHost, st));
        DM_TRY(hipStreamSynchronize(st));
        queued += kBatch;
        for (uint32_t q = 0; q < kBatch && !ended; ++q) {
            const uint32_t *c = h_count + q * kBrickCountWords;
            brick_runs += c[1];
            capped += c[2];
            if (c[0] == 0)
                ended = true;
            else
                ++rounds;
        }
    }
    return LA3DM_OK;
}
}  // extern "C++"

// ---- travel: least path cost from seeds through the passable voxels of a region, with parents (devmap_travel.h) -------

// The whole query on the map's stream; every pointer but `stats` is device memory.  The working storage is initialised
// here on every call.  The rounds are queued LA3DM_TRAVEL_BATCH at a time (brick_rounds).  o.cost and o.parent may be
// null: dm_tv_finish then only accumulates the totals.
static int travel_launch(la3dm_devmap *dm, const RegionGeom &g, const uint32_t *d_seeds, uint32_t n_seeds, const la3dm_travel_params &p,
                         const uint32_t *d_targets, uint32_t n_targets, const la3dm_travel_out &o, la3dm_travel_stats &stats) {
    hipStream_t st = dm->ctx->stream;
    const size_t n = (size_t)g.total;
    TravelArgs a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < 3; ++k) a.move[k] = p.move_cost[k];
    a.max_cost = p.max_cost;
    const uint32_t R = std::max(p.clearance, p.soft_radius);
    const bool empty = dm->n_blocks == 0;   // every voxel MISSING: the pool is not read
    const bool transform = R > 0 && !empty;
    // layout: cost 0 | cost 1 | E | side .. totals | d2
    uint32_t *own;
    int rc = brick_layout(dm, dm->travel_work, g, 1, transform ? n : 0, a.g, a.totals, own);
    if (rc != LA3DM_OK) return rc;
    a.E = a.g.val[1] + (size_t)a.g.n_bricks * 512;
    ObstacleField field;
    DM_OK(obstacle_field(dm, g, p.obstacle_mask, R, own, field));
    DM_TRY(hipMemsetAsync(a.g.side[0], 0, 4ull * (own - a.g.side[0]), st));
    RegionArgs r = region_args(dm, g);
    hipLaunchKernelGGL(dm_tv_enter, dim3(a.g.n_bricks * 2u), dim3(256), 0, st, r, a, p.pass_mask, empty ? 0u : 1u, field, p.clearance,
                       p.soft_radius * p.soft_radius, p.penalty);
    DM_TRY(hipGetLastError());
    memset(&stats, 0, sizeof(stats));
    uint32_t queued = 0;
    if (n_seeds) {
        hipLaunchKernelGGL(dm_tv_seed, dim3(cdiv(n_seeds, 256)), dim3(256), 0, st, a, d_seeds, n_seeds,
                           la3dm_region::move_reach(p.connectivity));
        DM_TRY(hipGetLastError());
        const auto round_kernel = DM_BY_CONNECTIVITY(dm_tv_round, p.connectivity);
        rc = brick_rounds<LA3DM_TRAVEL_BATCH>(
            dm, a.g, [&](uint32_t turn, uint32_t slot) { hipLaunchKernelGGL(round_kernel, dim3(a.g.n_bricks), dim3(512), 0, st, a, turn, slot); },
            LA3DM_TRAVEL_MAX_ROUNDS, "la3dm_devmap_travel: no fixed point after LA3DM_TRAVEL_MAX_ROUNDS (2^16) rounds; the outputs are unspecified",
            queued, stats.rounds, stats.brick_runs, stats.capped);
        if (rc != LA3DM_OK) return rc;
    }
    const uint32_t *side = a.g.side[queued & 1u];
    hipLaunchKernelGGL(DM_BY_CONNECTIVITY(dm_tv_finish, p.connectivity), dim3(cdiv(a.g.n_cells, 256)), dim3(256), 0, st, a, side, o.cost, o.parent);
    DM_TRY(hipGetLastError());
    if (n_targets) {
        hipLaunchKernelGGL(dm_tv_gather, dim3(cdiv(n_targets, 256)), dim3(256), 0, st, a, side, d_targets, n_targets, o.target_cost);
        DM_TRY(hipGetLastError());
    }
    uint32_t totals[3];
    DM_TRY(hipMemcpyAsync(totals, a.totals, sizeof(totals), hipMemcpyDeviceToHost, st));
    DM_TRY(hipStreamSynchronize(st));
    stats.n_seeded = totals[0];
    stats.n_reached = totals[1];
    stats.max_cost = totals[2];
    return LA3DM_OK;
}

static int travel_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3, const uint32_t *seeds,
                        uint32_t n_seeds, const la3dm_travel_params *params, const uint32_t *targets, uint32_t n_targets,
                        const la3dm_travel_out *out, la3dm_travel_stats *stats, la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(refuse(dm, who, la3dm_region::travel_check(params, n_seeds, n_targets, seeds != nullptr, targets != nullptr, out != nullptr,
                                                     out && out->cost, out && out->target_cost, "->")));
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::kTravel, true, true, who, g));
    la3dm_travel_out o = *out;
    const size_t n = (size_t)g.total;
    Stage s(dm, host);
    s.in(seeds, n_seeds);
    s.in(targets, n_targets);
    s.out(o.cost, n);
    s.out(o.target_cost, n_targets);
    s.out(o.parent, n);
    DM_OK(s.reserve());
    la3dm_travel_stats ts;
    DM_OK(travel_launch(dm, g, seeds, n_seeds, *params, targets, n_targets, o, ts));   // (ends in a synchronise)
    DM_OK(s.download());
    if (host) DM_TRY(hipStreamSynchronize(dm->ctx->stream));
    if (stats) *stats = ts;
    if (info) *info = g.info;
    return LA3DM_OK;
}

int la3dm_devmap_travel_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const uint32_t *d_seeds, uint32_t n_seeds,
                               const la3dm_travel_params *params, const uint32_t *d_targets, uint32_t n_targets,
                               const la3dm_travel_out *d_out, la3dm_travel_stats *stats, la3dm_region_info *info) {
    return travel_query(dm, false, "la3dm_devmap_travel_device", lo3, dims3, d_seeds, n_seeds, params, d_targets, n_targets, d_out, stats, info);
}

int la3dm_devmap_travel_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds,
                             const la3dm_travel_params *params, const uint32_t *targets, uint32_t n_targets, const la3dm_travel_out *out,
                             la3dm_travel_stats *stats, la3dm_region_info *info) {
    return travel_query(dm, true, "la3dm_devmap_travel_host", lo3, dims3, seeds, n_seeds, params, targets, n_targets, out, stats, info);
}

// ---- drive: least cost of a ground route over the member voxels of a region, with parents (devmap_drive.h) -------------

// the instantiation of a kernel template <int kConn, int kStep> for a connectivity and a step that the query's check has
// found to be 4 or 8 and 0 ... 4
#define DM_DR_BY_STEP(kernel, conn, step) \
    ((step) == 0 ? kernel<conn, 0> : (step) == 1 ? kernel<conn, 1> : (step) == 2 ? kernel<conn, 2> : (step) == 3 ? kernel<conn, 3> : kernel<conn, 4>)
#define DM_BY_DRIVE(kernel, connectivity, step) ((connectivity) == 4 ? DM_DR_BY_STEP(kernel, 4, step) : DM_DR_BY_STEP(kernel, 8, step))

// The whole query on the map's stream; every pointer but `stats` and p.footing is device memory.  The working storage is
// initialised here on every call.  The rounds are queued LA3DM_DRIVE_BATCH at a time (brick_rounds).  o.cost and o.parent
// may be null: dm_dr_finish then only accumulates the totals.
static int drive_launch(la3dm_devmap *dm, const RegionGeom &g, const uint32_t *d_seeds, uint32_t n_seeds, const la3dm_drive_params &p,
                        const uint32_t *d_targets, uint32_t n_targets, const la3dm_drive_out &o, la3dm_drive_stats &stats) {
    hipStream_t st = dm->ctx->stream;
    DriveArgs a;
    memset(&a, 0, sizeof(a));
    a.move[0] = p.move_cost[0];
    a.move[1] = p.move_cost[1];
    a.up = p.climb_up;
    a.down = p.climb_down;
    a.max_cost = p.max_cost;
    a.snap = p.snap;
    // layout: cost 0 | cost 1 | E | side .. totals
    uint32_t *own;
    int rc = brick_layout(dm, dm->drive_work, g, 1, 0, a.g, a.totals, own);
    if (rc != LA3DM_OK) return rc;
    a.E = a.g.val[1] + (size_t)a.g.n_bricks * 512;
    DM_TRY(hipMemsetAsync(a.g.side[0], 0, 4ull * (own - a.g.side[0]), st));
    hipLaunchKernelGGL(dm_dr_clear, dim3(a.g.n_bricks * 2u), dim3(256), 0, st, a);
    if (p.footing) {
        if (dm->n_blocks) {   // (an empty map: every voxel MISSING, nothing stands, the pool is not read)
            FootingArgs f;
            rc = footing_words(dm, g, *p.footing, f);
            if (rc != LA3DM_OK) return rc;
            hipLaunchKernelGGL(dm_dr_foot, dim3(cdiv(a.g.n_cells, 256)), dim3(256), 0, st, a, f.stand, f.PY, f.PZ, f.r, f.s);
        }
    } else if (p.n_members) {
        hipLaunchKernelGGL(dm_dr_members, dim3(cdiv(p.n_members, 256)), dim3(256), 0, st, a, p.members, p.n_members);
    }
    DM_TRY(hipGetLastError());
    memset(&stats, 0, sizeof(stats));
    uint32_t queued = 0;
    if (n_seeds) {
        hipLaunchKernelGGL(DM_BY_DRIVE(dm_dr_seed, p.connectivity, p.step), dim3(cdiv(n_seeds, 256)), dim3(256), 0, st, a, d_seeds, n_seeds);
        DM_TRY(hipGetLastError());
        const auto round_kernel = DM_BY_DRIVE(dm_dr_round, p.connectivity, p.step);
        rc = brick_rounds<LA3DM_DRIVE_BATCH>(
            dm, a.g, [&](uint32_t turn, uint32_t slot) { hipLaunchKernelGGL(round_kernel, dim3(a.g.n_bricks), dim3(512), 0, st, a, turn, slot); },
            LA3DM_DRIVE_MAX_ROUNDS, "la3dm_devmap_drive: no fixed point after LA3DM_DRIVE_MAX_ROUNDS (2^16) rounds; the outputs are unspecified",
            queued, stats.rounds, stats.brick_runs, stats.capped);
        if (rc != LA3DM_OK) return rc;
    }
    const uint32_t *side = a.g.side[queued & 1u];
    hipLaunchKernelGGL(DM_BY_DRIVE(dm_dr_finish, p.connectivity, p.step), dim3(cdiv(a.g.n_cells, 256)), dim3(256), 0, st, a, side, o.cost, o.parent);
    DM_TRY(hipGetLastError());
    const uint32_t n_list = o.of_member ? p.n_members : 0u;
    if (n_targets + n_list) {
        hipLaunchKernelGGL(dm_dr_gather, dim3(cdiv(n_targets + n_list, 256)), dim3(256), 0, st, a, side, d_targets, n_targets, o.target_cost,
                           o.target_index, p.members, n_list, o.of_member);
        DM_TRY(hipGetLastError());
    }
    uint32_t totals[4];
    DM_TRY(hipMemcpyAsync(totals, a.totals, sizeof(totals), hipMemcpyDeviceToHost, st));
    DM_TRY(hipStreamSynchronize(st));
    stats.n_seeded = totals[0];
    stats.n_reached = totals[1];
    stats.max_cost = totals[2];
    stats.n_members = totals[3];
    return LA3DM_OK;
}

static int drive_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3, const uint32_t *seeds,
                       uint32_t n_seeds, const la3dm_drive_params *params, const uint32_t *targets, uint32_t n_targets,
                       const la3dm_drive_out *out, la3dm_drive_stats *stats, la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(refuse(dm, who, la3dm_region::drive_check(params, n_seeds, n_targets, seeds != nullptr, targets != nullptr, out, "->")));
    if (params->footing) DM_OK(refuse(dm, who, la3dm_region::footing_check(params->footing, 0, false, "->")));
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::kDrive, true, true, who, g));
    if (params->footing) DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::footing_query(*params->footing), true, true, who, g));   // the padded box
    la3dm_drive_out o = *out;
    la3dm_drive_params p = *params;
    const size_t n = (size_t)g.total;
    Stage s(dm, host);
    s.in(seeds, n_seeds);
    s.in(targets, n_targets);
    s.in(p.members, p.n_members);
    s.out(o.cost, n);
    s.out(o.parent, n);
    s.out(o.of_member, p.n_members);
    s.out(o.target_cost, n_targets);
    s.out(o.target_index, n_targets);
    DM_OK(s.reserve());
    la3dm_drive_stats ds;
    DM_OK(drive_launch(dm, g, seeds, n_seeds, p, targets, n_targets, o, ds));   // (ends in a synchronise)
    DM_OK(s.download());
    if (host) DM_TRY(hipStreamSynchronize(dm->ctx->stream));
    if (stats) *stats = ds;
    if (info) *info = g.info;
    return LA3DM_OK;
}

int la3dm_devmap_drive_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const uint32_t *d_seeds, uint32_t n_seeds,
                              const la3dm_drive_params *params, const uint32_t *d_targets, uint32_t n_targets,
                              const la3dm_drive_out *d_out, la3dm_drive_stats *stats, la3dm_region_info *info) {
    return drive_query(dm, false, "la3dm_devmap_drive_device", lo3, dims3, d_seeds, n_seeds, params, d_targets, n_targets, d_out, stats, info);
}

int la3dm_devmap_drive_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds,
                            const la3dm_drive_params *params, const uint32_t *targets, uint32_t n_targets, const la3dm_drive_out *out,
                            la3dm_drive_stats *stats, la3dm_region_info *info) {
    return drive_query(dm, true, "la3dm_devmap_drive_host", lo3, dims3, seeds, n_seeds, params, targets, n_targets, out, stats, info);
}

// ---- clusters: connected groups of a region's member voxels, optionally tiled (devmap_clusters.h) ----------------------

// The whole query on the map's stream; every pointer of p and o is device memory.  The working storage is initialised
// here on every call.  The rounds are queued LA3DM_CLUSTERS_BATCH at a time (brick_rounds).  n and the totals are read
// before the records, whose storage is
// sized by min(n, cap).  `rec` = where the records lie in the working storage (rec.m of them) for a caller that copies
// them itself; o's record arrays may all be null.
static int clusters_launch(la3dm_devmap *dm, const RegionGeom &g, const la3dm_clusters_params &p, const la3dm_clusters_out &o,
                           uint32_t &n_found, la3dm_clusters_stats &stats, ClustersRec &rec) {
    hipStream_t st = dm->ctx->stream;
    ClustersArgs a;
    memset(&a, 0, sizeof(a));
    a.tb = p.tile ? p.tile / LA3DM_CLUSTERS_BRICK : kClNoTile;
    a.min_size = p.min_size;
    const size_t per_voxel = ((size_t)g.total + 1 + 3) & ~(size_t)3;   // every array 16-byte aligned (the scan's vector path)
    // layout: label 0 | label 1 | side .. totals | size | flag | number
    int rc = brick_layout(dm, dm->clusters_work, g, 0, 3 * per_voxel, a.g, a.totals, a.size);
    if (rc != LA3DM_OK) return rc;
    a.flag = a.size + per_voxel;
    a.number = a.flag + per_voxel;
    const uint32_t n_bricks = a.g.n_bricks, n_cells = a.g.n_cells;
    DM_TRY(hipMemsetAsync(a.g.side[0], 0, 4ull * (a.flag - a.g.side[0]), st));   // (the sizes too)
    const uint32_t probe = dm->n_blocks == 0 ? 0u : 1u;   // an empty map: every voxel MISSING, the pool is not read
    RegionArgs r = region_args(dm, g);
    if (p.from_list) {
        DM_TRY(hipMemsetAsync(a.g.val[0], 0xFF, 4ull * n_bricks * 512, st));
        if (p.n_members) hipLaunchKernelGGL(dm_cl_list, dim3(cdiv(p.n_members, 256)), dim3(256), 0, st, r, a, p.member_mask, probe, p.members, p.n_members);
    } else {
        hipLaunchKernelGGL(dm_cl_enter, dim3(n_bricks * 2u), dim3(256), 0, st, r, a, p.member_mask, probe);
    }
    DM_TRY(hipGetLastError());
    memset(&stats, 0, sizeof(stats));
    rec.m = 0;
    uint32_t queued = 0;
    if (!p.from_list || p.n_members) {
        const auto round_kernel = DM_BY_CONNECTIVITY(dm_cl_round, p.connectivity);
        rc = brick_rounds<LA3DM_CLUSTERS_BATCH>(
            dm, a.g, [&](uint32_t turn, uint32_t slot) { hipLaunchKernelGGL(round_kernel, dim3(n_bricks), dim3(512), 0, st, a, turn, slot); },
            LA3DM_CLUSTERS_MAX_ROUNDS, "la3dm_devmap_clusters: no fixed point after LA3DM_CLUSTERS_MAX_ROUNDS (2^16) rounds; the outputs are unspecified",
            queued, stats.rounds, stats.brick_runs, stats.capped);
        if (rc != LA3DM_OK) return rc;
    }
    const uint32_t *side = a.g.side[queued & 1u];
    hipLaunchKernelGGL(dm_cl_sizes, dim3(n_bricks), dim3(512), 0, st, a, side);
    hipLaunchKernelGGL(dm_cl_flags, dim3(cdiv(n_cells + 1u, 256)), dim3(256), 0, st, a, side);
    DM_TRY(hipGetLastError());
    dm->counters_clean = false;   // (the scan may flag a dirty state in the counter block)
    rc = exclusive_scan(dm, a.flag, a.number, n_cells + 1u);
    if (rc != LA3DM_OK) return rc;
    if (o.label) hipLaunchKernelGGL(dm_cl_label, dim3(cdiv(n_cells, 256)), dim3(256), 0, st, a, side, o.label);
    if (o.of_member && p.n_members)
        hipLaunchKernelGGL(dm_cl_gather, dim3(cdiv(p.n_members, 256)), dim3(256), 0, st, a, side, p.members, p.n_members, o.of_member);
    DM_TRY(hipGetLastError());
    uint32_t totals[3], n = 0;
    DM_TRY(hipMemcpyAsync(totals, a.totals, sizeof(totals), hipMemcpyDeviceToHost, st));
    DM_TRY(hipMemcpyAsync(&n, a.number + n_cells, 4, hipMemcpyDeviceToHost, st));
    DM_TRY(hipStreamSynchronize(st));
    stats.n_members = totals[0];
    stats.n_dropped = totals[1];
    stats.largest = totals[2];
    stats.n_clusters = n_found = n;
    const uint32_t m = std::min(n, p.cap);
    if (m == 0) return LA3DM_OK;
    // layout: sum [3 m] | key [m] (64-bit words) | lo [3 m] | hi [3 m] | first | size | rep [m]
    DM_RESERVE(dm->clusters_rec, 68ull * m);
    rec.m = m;
    rec.sum = (unsigned long long *)dm->clusters_rec.ptr;
    rec.key = rec.sum + 3ull * m;
    rec.lo = (uint32_t *)(rec.key + m);
    rec.hi = rec.lo + 3ull * m;
    rec.first = rec.hi + 3ull * m;
    rec.size = rec.first + m;
    rec.rep = rec.size + m;
    hipLaunchKernelGGL(dm_cl_rec_init, dim3(cdiv(m, 256)), dim3(256), 0, st, rec);
    hipLaunchKernelGGL(dm_cl_records, dim3(n_bricks), dim3(512), 0, st, a, side, rec);
    hipLaunchKernelGGL(dm_cl_rep, dim3(n_bricks), dim3(512), 0, st, a, side, rec);
    hipLaunchKernelGGL(dm_cl_emit, dim3(cdiv(m, 256)), dim3(256), 0, st, rec, o.first, o.size, o.lo, o.hi, (unsigned long long *)o.sum, o.rep);
    DM_TRY(hipGetLastError());
    return LA3DM_OK;
}

static int clusters_query(la3dm_devmap *dm, bool host, const char *who, const float *lo3, const uint32_t *dims3,
                          const la3dm_clusters_params *params, const la3dm_clusters_out *out, uint32_t *n_found, la3dm_clusters_stats *stats,
                          la3dm_region_info *info) {
    RegionGeom g;
    DM_OK(refuse(dm, who, la3dm_region::clusters_check(params, out)));
    DM_OK(region_resolve(dm, lo3, dims3, la3dm_region::kClusters, true, true, who, g));
    DM_OK(refuse(dm, who, la3dm_region::clusters_region_check(dims3)));
    hipStream_t st = dm->ctx->stream;
    la3dm_clusters_out o;
    memset(&o, 0, sizeof(o));
    if (out) o = *out;
    la3dm_clusters_params p = *params;
    if (!p.from_list) p.n_members = 0;   // (checked, not used)
    // host pointers: the records are copied straight from the working storage (clusters_launch), not emitted
    const la3dm_clusters_out h = o;
    if (host) {
        o.first = o.size = o.lo = o.hi = o.rep = nullptr;
        o.sum = nullptr;
    }
    Stage s(dm, host);
    s.in(p.members, p.n_members);
    s.out(o.label, (size_t)g.total);
    s.out(o.of_member, p.n_members);
    DM_OK(s.reserve());
    la3dm_clusters_stats cs;
    ClustersRec rec;
    uint32_t found = 0;
    DM_OK(clusters_launch(dm, g, p, o, found, cs, rec));
    DM_OK(s.download());
    if (host && rec.m) {
        const size_t m = rec.m;
        if (h.first) DM_TRY(hipMemcpyAsync(h.first, rec.first, 4ull * m, hipMemcpyDeviceToHost, st));
        if (h.size) DM_TRY(hipMemcpyAsync(h.size, rec.size, 4ull * m, hipMemcpyDeviceToHost, st));
        if (h.lo) DM_TRY(hipMemcpyAsync(h.lo, rec.lo, 12ull * m, hipMemcpyDeviceToHost, st));
        if (h.hi) DM_TRY(hipMemcpyAsync(h.hi, rec.hi, 12ull * m, hipMemcpyDeviceToHost, st));
        if (h.sum) DM_TRY(hipMemcpyAsync(h.sum, rec.sum, 24ull * m, hipMemcpyDeviceToHost, st));
        if (h.rep) DM_TRY(hipMemcpyAsync(h.rep, rec.rep, 4ull * m, hipMemcpyDeviceToHost, st));
    }
    DM_TRY(hipStreamSynchronize(st));
    if (n_found) *n_found = found;
    if (stats) *stats = cs;
    if (info) *info = g.info;
    return LA3DM_OK;
}

int la3dm_devmap_clusters_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_clusters_params *params,
                                 const la3dm_clusters_out *d_out, uint32_t *n_found, la3dm_clusters_stats *stats,
                                 la3dm_region_info *info) {
    return clusters_query(dm, false, "la3dm_devmap_clusters_device", lo3, dims3, params, d_out, n_found, stats, info);
}

int la3dm_devmap_clusters_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_clusters_params *params,
                               const la3dm_clusters_out *out, uint32_t *n_found, la3dm_clusters_stats *stats, la3dm_region_info *info) {
    return clusters_query(dm, true, "la3dm_devmap_clusters_host", lo3, dims3, params, out, n_found, stats, info);
}

int la3dm_devmap_key_bounds(la3dm_devmap *dm, int32_t lo[3], int32_t hi[3]) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (!dm || !lo || !hi) return LA3DM_ERR_ARG;
    if (dm->n_blocks == 0) return dm_fail(dm, LA3DM_ERR_ARG, "la3dm_devmap_key_bounds: the map holds no blocks");
    DM_TRY(hipSetDevice(dm->ctx->device));
    hipStream_t st = dm->ctx->stream;
    DM_RESERVE(dm->q_out, 64);
    uint32_t *mm = (uint32_t *)dm->q_out.ptr;
    DM_TRY(hipMemsetAsync(mm, 0xFF, 12, st));
    DM_TRY(hipMemsetAsync(mm + 3, 0, 12, st));
    hipLaunchKernelGGL(dm_key_bounds, dim3(std::min(cdiv(dm->n_blocks, 256), 64u)), dim3(256), 0, st, dm->blk_key, dm->n_blocks, mm);
    uint32_t h[6];
    DM_TRY(hipMemcpyAsync(h, mm, 24, hipMemcpyDeviceToHost, st));
    DM_TRY(hipStreamSynchronize(st));
    for (int a = 0; a < 3; ++a) {
        lo[a] = (int32_t)h[a];
        hi[a] = (int32_t)h[3 + a];
    }
    return LA3DM_OK;
}

int la3dm_devmap_export_cells(la3dm_devmap *dm, int state, int original_size, float min_z, float max_z, float *cells,
                              float *rgba, int32_t *level, uint64_t cap, uint64_t *count) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (dm) dm->counters_clean = false;   // (this entry point's scans / sorts write counter slots; only an insert's own last launch leaves the block clean)
    if (!dm || !count || (state != 0 && state != 1)) return LA3DM_ERR_ARG;
    *count = 0;
    if (dm->n_blocks == 0) return LA3DM_OK;
    DM_TRY(hipSetDevice(dm->ctx->device));
    hipStream_t st = dm->ctx->stream;
    const la3dm_params &p = dm->ctx->p;
    ExportArgs a;
    memset(&a, 0, sizeof(a));
    a.blk_key = dm->blk_key;
    a.S = dm->S;
    a.A = dm->A;
    a.B = dm->B;
    a.lut = dm->ctx->d_lut;
    a.n_blocks = dm->n_blocks;
    a.npb = dm->npb;
    a.depth = dm->depth;
    a.want_state = state;
    a.original = original_size ? 1 : 0;
    a.variant = p.variant;
    a.coloured = min_z < max_z ? 1 : 0;
    a.block_size = dm->block_size;
    a.resolution = p.resolution;
    a.min_z = min_z;
    a.max_z = max_z;
    a.gp_l = p.l;
    a.gp_max_ivar = p.max_ivar;
    for (uint32_t d = 0; d < dm->depth && d < 8; ++d) {
        a.size_of_depth[d] = float(dm->block_size / pow(2, d));                       // Block::get_size, bgkblock.h:69-73
        a.level_of_depth[d] = (int)log2(a.size_of_depth[d] / p.resolution);            // markerarray_pub.h:112-114
    }
    DM_RESERVE(dm->c_scan, 8ull * (dm->n_blocks + 1));
    uint32_t *cnt = (uint32_t *)dm->c_scan.ptr, *off = cnt + dm->n_blocks + 1;
    a.blk_cnt = cnt;
    a.blk_off = off;
    DM_TRY(hipMemsetAsync(cnt + dm->n_blocks, 0, 4, st));
    hipLaunchKernelGGL(dm_export<false>, dim3(cdiv(dm->n_blocks, 4)), dim3(256), 0, st, a);
    int rc = exclusive_scan(dm, cnt, off, dm->n_blocks + 1);
    if (rc != LA3DM_OK) return rc;
    uint32_t total = 0;
    DM_TRY(hipMemcpyAsync(&total, off + dm->n_blocks, 4, hipMemcpyDeviceToHost, st));
    DM_TRY(hipStreamSynchronize(st));
    *count = total;
    if (!cells && !rgba && !level) return LA3DM_OK;  // size query
    if (!cells || !rgba || !level || cap < total) return dm_fail(dm, LA3DM_ERR_ARG, "la3dm_devmap_export_cells: buffers too small");
    if (total == 0) return LA3DM_OK;
    DM_RESERVE(dm->q_out, 36ull * total + 64);
    a.cells = (float4 *)dm->q_out.ptr;
    a.rgba = a.cells + total;
    a.level = (int32_t *)(a.rgba + total);
    hipLaunchKernelGGL(dm_export<true>, dim3(cdiv(dm->n_blocks, 4)), dim3(256), 0, st, a);
    DM_TRY(hipGetLastError());
    DM_TRY(hipMemcpyAsync(cells, a.cells, 16ull * total, hipMemcpyDeviceToHost, st));
    DM_TRY(hipMemcpyAsync(rgba, a.rgba, 16ull * total, hipMemcpyDeviceToHost, st));
    DM_TRY(hipMemcpyAsync(level, a.level, 4ull * total, hipMemcpyDeviceToHost, st));
    DM_TRY(hipStreamSynchronize(st));
    return LA3DM_OK;
}

int la3dm_devmap_diag_add_repeat(la3dm_ctx *ctx, const float *s, const float *x, const uint32_t *m, uint32_t n,
                                 float *out_fast, float *out_loop) {
    if (!ctx || !s || !x || !m || !out_fast || !out_loop) return LA3DM_ERR_ARG;
    if (n == 0) return LA3DM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void *d = nullptr;
    HIP_TRY(ctx, hipMalloc(&d, 20ull * n));
    float *ds = (float *)d, *dx = ds + n, *df = dx + n, *dl = df + n;
    uint32_t *dmm = (uint32_t *)(dl + n);
    hipError_t e = hipMemcpy(ds, s, 4ull * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dx, x, 4ull * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dmm, m, 4ull * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(dm_diag_add_repeat, dim3(cdiv(n, 64)), dim3(64), 0, ctx->stream, ds, dx, dmm, n, df, dl);
        e = hipStreamSynchronize(ctx->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(out_fast, df, 4ull * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_loop, dl, 4ull * n, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) {
        ctx->err = std::string("la3dm_devmap_diag_add_repeat: ") + hipGetErrorString(e);
        return LA3DM_ERR_HIP;
    }
    return LA3DM_OK;
}

// Test hooks for the front end's own primitives (devmap_scan.h, devmap_sort.h), on the map's stream and state.
// mode 0: out[i] = sum of in[0..i), aux[0] = total.  mode 1: in = sorted keys (0xFFFFFFFF = invalid, last): out = exclusive
// scan of the head flags, aux = {segments, valid keys, seg_start[0..segments]} (aux holds n + 3 words).
int la3dm_devmap_diag_scan(la3dm_devmap *dm, int mode, const uint32_t *in, uint32_t n, uint32_t *out, uint32_t *aux) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (dm) dm->counters_clean = false;   // (this entry point's scans / sorts write counter slots; only an insert's own last launch leaves the block clean)
    if (!dm || !in || !out || !aux || n == 0 || (mode != 0 && mode != 1)) return LA3DM_ERR_ARG;
    DM_TRY(hipSetDevice(dm->ctx->device));
    hipStream_t st = dm->ctx->stream;
    DM_RESERVE(dm->k0, 4ull * n);
    DM_RESERVE(dm->k1, 4ull * n);
    DM_RESERVE(dm->seg_start, 4ull * (n + 1));
    DM_TRY(hipMemcpyAsync(dm->k0.ptr, in, 4ull * n, hipMemcpyHostToDevice, st));
    int rc;
    // (publishing launches, as in insert_pointcloud: the mailbox may arrive before the copy below has finished — hence the
    // synchronisation after read_counters)
    if (mode == 0) rc = exclusive_scan(dm, (const uint32_t *)dm->k0.ptr, (uint32_t *)dm->k1.ptr, n, (int)kCntMembers, true);
    else rc = scan_heads(dm, (const uint32_t *)dm->k0.ptr, n, nullptr, (uint32_t *)dm->k1.ptr, (uint32_t *)dm->seg_start.ptr, nullptr,
                         (int)kCntGridSegs, (int)kCntGridValid, -1, true);
    if (rc != LA3DM_OK) return rc;
    DM_TRY(hipMemcpyAsync(out, dm->k1.ptr, 4ull * n, hipMemcpyDeviceToHost, st));
    if ((rc = read_counters(dm)) != LA3DM_OK) return rc;
    DM_TRY(hipStreamSynchronize(st));
    if (mode == 0) {
        aux[0] = dm->h_cnt[kCntMembers];
    } else {
        aux[0] = dm->h_cnt[kCntGridSegs];
        aux[1] = dm->h_cnt[kCntGridValid];
        DM_TRY(hipMemcpy(aux + 2, dm->seg_start.ptr, 4ull * (aux[0] + 1), hipMemcpyDeviceToHost));
    }
    return LA3DM_OK;
}

// stable sort of (keys, vals) on the low `bits` key bits through sort_pairs (the in-house radix sort unless LA3DM_OWN_SORT=0)
int la3dm_devmap_diag_sort(la3dm_devmap *dm, const uint32_t *keys, const uint32_t *vals, uint32_t n, int bits, uint32_t *keys_out,
                           uint32_t *vals_out) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (dm) dm->counters_clean = false;   // (this entry point's scans / sorts write counter slots; only an insert's own last launch leaves the block clean)
    if (!dm || !keys || !vals || !keys_out || !vals_out || n == 0 || bits < 1 || bits > 32) return LA3DM_ERR_ARG;
    DM_TRY(hipSetDevice(dm->ctx->device));
    hipStream_t st = dm->ctx->stream;
    DM_RESERVE(dm->k0, 4ull * n);
    DM_RESERVE(dm->k1, 4ull * n);
    DM_RESERVE(dm->v0, 4ull * n);
    DM_RESERVE(dm->v1, 4ull * n);
    DM_TRY(hipMemcpyAsync(dm->k0.ptr, keys, 4ull * n, hipMemcpyHostToDevice, st));
    DM_TRY(hipMemcpyAsync(dm->v0.ptr, vals, 4ull * n, hipMemcpyHostToDevice, st));
    int rc = sort_pairs(dm, (const uint32_t *)dm->k0.ptr, (uint32_t *)dm->k1.ptr, (const uint32_t *)dm->v0.ptr, (uint32_t *)dm->v1.ptr, n, bits);
    if (rc != LA3DM_OK) return rc;
    DM_TRY(hipMemcpyAsync(keys_out, dm->k1.ptr, 4ull * n, hipMemcpyDeviceToHost, st));
    DM_TRY(hipMemcpyAsync(vals_out, dm->v1.ptr, 4ull * n, hipMemcpyDeviceToHost, st));
    if ((rc = read_counters(dm)) != LA3DM_OK) return rc;   // (carries the "stuck" error bit of the look-back loops)
    DM_TRY(hipStreamSynchronize(st));
#ifdef LA3DM_RS_TRACE
    {   // per pass: the phases of the first, a middle and the last tile, relative to the pass's earliest entry stamp (us)
        std::vector<unsigned long long> tr(4 * 1024 * 8);
        DM_TRY(hipMemcpyFromSymbol(tr.data(), HIP_SYMBOL(la3dm_dev::g_rs_trace), 8ull * tr.size()));
        const uint32_t tiles = std::min(1024u, (n + la3dm_dev::kRsTile - 1) / la3dm_dev::kRsTile), passes = (uint32_t)(bits + 7) / 8;
        for (uint32_t p = 0; p < passes; ++p) {
            unsigned long long t0 = ~0ull, t1 = 0;
            for (uint32_t t = 0; t < tiles; ++t) t0 = std::min(t0, tr[(p * 1024 + t) * 8]), t1 = std::max(t1, tr[(p * 1024 + t) * 8 + 7]);
            fprintf(stderr, "rs_trace pass %u: %u tiles, first entry -> last end %.2f us\n", p, tiles, (t1 - t0) * 0.01);
            for (uint32_t t : {0u, tiles / 4, tiles / 2, 3 * tiles / 4, tiles - 1}) {
                fprintf(stderr, "  tile %4u:", t);
                for (int k = 0; k < 8; ++k) fprintf(stderr, " %6.2f", (double)(long long)(tr[(p * 1024 + t) * 8 + k] - t0) * 0.01);
                fprintf(stderr, "\n");
            }
        }
    }
#endif
    return LA3DM_OK;
}

int la3dm_devmap_training_data(la3dm_devmap *dm, float *xyzy, uint32_t cap, uint32_t *n) {
    if (dm) dm->mailbox_pending = 0;   // (left behind by a call that failed between a publishing launch and its read_counters)
    if (!dm || !n) return LA3DM_ERR_ARG;
    *n = dm->n_xy;
    if (!xyzy || cap < dm->n_xy) return dm->n_xy ? LA3DM_ERR_ARG : LA3DM_OK;
    if (dm->n_xy == 0) return LA3DM_OK;
    DM_TRY(hipSetDevice(dm->ctx->device));
    DM_TRY(hipMemcpyAsync(xyzy, dm->xy.ptr, 16ull * dm->n_xy, hipMemcpyDeviceToHost, dm->ctx->stream));
    DM_TRY(hipStreamSynchronize(dm->ctx->stream));
    return LA3DM_OK;
}

}  // extern "C"
