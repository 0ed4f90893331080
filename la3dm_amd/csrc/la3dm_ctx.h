// la3dm_ctx.h — internal: the device context shared by the translation units of libla3dm_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/la3dm_hip.h"

struct Arena {
    void *ptr = nullptr;
    size_t cap = 0;
};

struct la3dm_ctx {
    la3dm_params p;
    int device = 0;
    hipStream_t stream = nullptr;  // used by the host-pointer entry points
    float4 *d_lut = nullptr;
    uint32_t lut_count = 0;
    std::string err;
    int n_devmaps = 0;     // live la3dm_devmap objects that point at this context (la3dm_destroy refuses while > 0)
    int opt_bgk_sum = 1;   // BGK accumulate mode: 1 (default) = order-free double accumulators (bgk_predict_fuse_r: the correctly rounded
                           // sums, |dp| <= ~4e-7 from the reference's fp32 chains), 0 = the reference's fp32 summation order
                           // (bgk_predict_fuse_v5, bit-identical to the CPU restatement); env LA3DM_BGK_SUM sets the default
    int opt_bgk_tables = 1;  // bgk_sum = 1 only: 1 (default) = bgk_predict_fuse_t (per-axis distance tables for aligned 4x4x4 tiles, the
                             // other tiles through the general path in the same launch), 0 = bgk_predict_fuse_r for every tile
    int opt_bgk_one_launch = 1;  // bgk_sum = 1, tables, block_depth 3, a scan of full blocks only: 1 (default) = one launch, bgk_predict_fuse_t1 on the caller's
                                 // unscaled points (bgk_scan1_kernels.h), 0 = bgk_prepare + bgk_predict_fuse_t<.., false>; env LA3DM_BGK_ONE_LAUNCH sets the default
    int opt_bgk_scan1_generic = 0;  // the one launch: 0 (default) = the production instance of the kernel (bgk_scan1_tile<0, true>) where la3dm_bgk_scan_device finds its
                                    // conditions, 1 = the generic instance always (A/B, tests); env LA3DM_BGK_SCAN1_GENERIC sets the default
    int last_scan1_instance = 0;    // what the last la3dm_bgk_scan_device call launched: 0 not the one launch, 1 its generic instance, 2 its production instance (la3dm_get_option "bgk_scan1_instance")
    float inv_ell = 0.0f;   // RN(1 / ell), or 0 when x / ell must stay an IEEE division (bgk_kernels.h div_by_ell)
    int opt_fast_trig = 0;  // 0 correctly rounded (f64 kernels), 1 f32 polynomial, 2 OCML, 3 Eigen 3.3.7 psin / pcos without FMA (the likely reference build)
    int opt_gp_mode = 0;    // GPOctoMap: 0 = FMA chains in ascending order (VALU and matrix cores alike: the parity configuration), 1 = the order of an
                            // x86-64 / SSE2 build of Eigen 3.3.7 on the VALU (gp_eigen_kernels.h; blocks of up to 128 points); env LA3DM_GP_MODE
    int opt_bgk_tile_desc = 1;   // block_depth >= 4, bgk_sum 1: per-tile neighbour descriptors without the face neighbours out of the tile's reach (bgk_prepare); 0 = block-wide descriptors (A/B)
    int opt_grid_order = 0;  // device-resident map's voxel-grid filters: 0 = ascending cloud index inside a cell (the parity configuration), 1 = the order
                             // pcl::VoxelGrid's unstable std::sort leaves (host sort of the downloaded keys: verification mode, slow by design)
    int opt_time_kernel = 0;
    int opt_waves = 1;  // waves per workgroup (variant 3)
    int opt_remap = 2;
    int opt_l_dense_add = 1;      // BGK-L split tiles: 1 = expansion for all items at once + two-wave ordered add, 0 = producer / consumer workgroup
    int opt_l_split_rows = 1024;  // BGK-L: tiles with more rows than this are split over waves (< 0: never); measured on the 200 k-ray scan, round 5 (order-free sums, row cull): 8192 1.67 ms, 4096 1.63, 2048 1.30, 1024 1.27, 512 1.27 (round 2, ordered: 2048 was the optimum)
    int opt_lds_pad = 0;  // profiling only: extra dynamic LDS bytes on the BGK predict launch (lowers the waves a CU holds)
    int opt_ablate = 0;  // profiling only: 1 skip kernel evaluation, 2 skip the candidate tests
    struct EvPair {
        hipEvent_t first = nullptr, second = nullptr;
        unsigned flags = 0;  // what hipEventCreateWithFlags was given
    };
    std::vector<EvPair> ev_pool;  // start / stop events of the dominant kernel, one pair per *_scan_device call timed by events (KernelTimer below)
    size_t ev_used = 0;
    // stamp records of the calls timed from inside the kernel (bgk_predict_fuse_t1s; stamps_acquire below): chunks of
    // kStampChunkRecords records that never move, all zero except the records handed out since the last drain
    std::vector<unsigned long long *> stamp_chunks;
    size_t stamp_used = 0;
    std::vector<hipStream_t> stamp_streams;  // the streams those launches went to (what a drain waits for)
    std::vector<uint8_t> timed_form;         // one entry per timed call since the last drain, oldest first: 0 = the next event pair, 1 = the next stamp record
    int wall_clock_khz = 0;                  // hipDeviceAttributeWallClockRate, read once in la3dm_create (0: not available, stamped launches fall back to events)
    // scratch (device-pointer path)
    Arena pts_scaled, nbr_range, blk_desc, label_seq;
    Arena nbr_finite, blk_poison;  // la3dm_bgk_scan_device, two launches: the neighbour table without neighbours that hold a point at no finite distance; one flag per test block
    uint32_t scan_seq = 0;  // la3dm_bgk_scan_device calls so far (BgkArgs::seq)
    Arena gp_loff, gp_totals, gp_order, gp_L, gp_alpha, gp_v;
    Arena l_task_item, l_split_list, l_nb_first, l_part, l_counters, l_item_desc, l_rowrec, l_batch_off, l_item_hits, l_bdesc, l_vals, l_rowx, l_dense, l_labmask, l_part64;
    Arena lv_samples, lv_sorted, lv_rays, lv_cell, lv_center, lv_cell0, lv_alpha, lv_beta, lv_state;
    Arena lvp_sub_task, lvp_task, lvp_totals, lvp_rows, lvp_sub_out, lvp_cand;  // BGK-LV work plan + row scratch of split cubes
    // staging (host-pointer path)
    Arena h_train, h_train_off, h_nbr, h_center, h_leaf_off, h_leaf_key, h_alpha, h_beta, h_state, h_diag_in,
        h_diag_out;
};

#define HIP_TRY(ctx, expr)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                          \
            return LA3DM_ERR_HIP;                                                                   \
        }                                                                                           \
    } while (0)

static inline int arena_reserve(la3dm_ctx *ctx, Arena &a, size_t bytes) {
    if (bytes <= a.cap) return LA3DM_OK;
    if (a.ptr) {
        HIP_TRY(ctx, hipFree(a.ptr));
        a.ptr = nullptr;
        a.cap = 0;
    }
    // 50 % head room: a regrow is a device-wide free + malloc (hundreds of us); above 1 GB an eighth (the BGK-L split
    // scratch is 64 KB per item: tens of GB on a large scan — ADVICE r02)
    size_t want = bytes + (bytes > (1ull << 30) ? bytes / 8 : bytes / 2) + 256;
    hipError_t e = hipMalloc(&a.ptr, want);
    if (e != hipSuccess) {
        ctx->err = std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e);
        a.ptr = nullptr;
        return LA3DM_ERR_OOM;
    }
    a.cap = want;
    return LA3DM_OK;
}

// ---- kernel timing (option "time_kernel"): the time of one *_scan_device call's dominant kernel ----
// Three forms; la3dm_kernel_times returns them in call order whatever the mix (la3dm_ctx::timed_form).
// Marker form (timer_begin / timer_end round any number of launches): each is a hipEventRecord, a packet of its own on the
// stream.
// Dispatch-bound form (one launch): timer_acquire(.., true), then start and stop are handed to hipExtLaunchKernelGGL.  The
// stop event is then the completion of the kernel's own dispatch packet, no packet of its own; the start event is still a
// marker ahead of the kernel with the HIP 7.2 runtime (profiles/step_gap: 3.9 us per step on configs[1], against 7.5 us for
// the two markers; a launch with the stop event alone costs nothing, but hipEventElapsedTime of that event with itself is 0,
// so it gives no kernel time).  "time_kernel" 1 uses it for every single launch but the one-launch BGK scan, "time_kernel" 2
// for that one too (the two clocks side by side in one process; also what 1 means where the device reports no wall-clock rate).
// Stamped form (the one-launch BGK scan at "time_kernel" 1): a plain hipLaunchKernelGGL of bgk_predict_fuse_t1s, which reads
// the device's wall clock as each wave enters and leaves and writes the stamps into a record of the context's pool
// (stamps_acquire) — no event, no packet but the kernel's own, no stream operation per launch.  The time is first wave in to
// last wave out: (greatest exit stamp - least entry stamp) / hipDeviceAttributeWallClockRate.  It leaves out what an event or
// a kernel trace includes on either side, the command processor's dispatch set-up and the end-of-kernel cache write-back: on
// small grids it reads 1.1 - 1.5 us below the event pair.  On configs[1] it reads 0.5 us ABOVE it (59.74 against 59.26 us),
// because the stamped instance is itself about 2 us slower than the plain one: 35 more VALU-class instructions per tile, most of
// them scalars parked in VGPR lanes, in a kernel whose VALU is 95 % busy (profiles/kernel_stamps/README.md).
struct KernelTimer {
    hipEvent_t start = nullptr, stop = nullptr;  // both null: "time_kernel" is 0, nothing to do
    explicit operator bool() const { return start != nullptr; }
};

// the next pair of the context's pool (la3dm_kernel_times reads them oldest first and resets the pool); t stays empty when
// "time_kernel" is 0
static inline int timer_acquire(la3dm_ctx *ctx, KernelTimer &t, bool dispatch_bound) {
    t = KernelTimer();
    if (!ctx->opt_time_kernel) return LA3DM_OK;
    // Dispatch-bound pairs are created with hipEventDisableSystemFence: the host reads nothing on the strength of these
    // events — la3dm_kernel_times takes their timestamps only, and results reach the host through the stream synchronisation
    // or copy that follows the scan anyway — so the kernel keeps the fence scope of a plain launch.
    const unsigned flags = dispatch_bound ? hipEventDisableSystemFence : hipEventDefault;
    if (ctx->ev_used == ctx->ev_pool.size()) ctx->ev_pool.emplace_back();
    la3dm_ctx::EvPair &p = ctx->ev_pool[ctx->ev_used];
    if (p.first && p.flags != flags) {  // a pair left by the other form
        HIP_TRY(ctx, hipEventDestroy(p.first));
        p.first = nullptr;
    }
    if (p.second && p.flags != flags) {
        HIP_TRY(ctx, hipEventDestroy(p.second));
        p.second = nullptr;
    }
    p.flags = flags;
    if (!p.first) HIP_TRY(ctx, hipEventCreateWithFlags(&p.first, flags));
    if (!p.second) HIP_TRY(ctx, hipEventCreateWithFlags(&p.second, flags));
    ++ctx->ev_used;
    ctx->timed_form.push_back(0);
    t.start = p.first;
    t.stop = p.second;
    return LA3DM_OK;
}

// ---- the stamp pool ----
// A record is kStampRecordWords 8-byte words (bgk_scan1_kernels.h: 64 entry slots side by side, then 64 exit slots on a
// 128-byte line each), zero when it is handed out.  The pool is zeroed in bulk — a chunk when it is created, the used records
// when they are drained — never per launch: a memset or copy per launch would put back on the stream the packet the stamped
// form exists to remove.  Growing adds a chunk (one hipMalloc and one memset per kStampChunkRecords launches between two
// drains, the first of them when "time_kernel" is set); the chunks before it stay where launches in flight write them.
constexpr size_t kStampEntrySlots = 64, kStampExitSlots = 64, kStampExitStrideWords = 16;
constexpr size_t kStampRecordWords = kStampEntrySlots + kStampExitSlots * kStampExitStrideWords, kStampChunkRecords = 1024;   // 8.5 KiB, 8.5 MiB

// zero records [0, n) of the pool, from the context's own stream, and wait for it
static inline int stamps_zero(la3dm_ctx *ctx, size_t n) {
    for (size_t c = 0; c * kStampChunkRecords < n; ++c) {
        const size_t recs = std::min(n - c * kStampChunkRecords, kStampChunkRecords);
        HIP_TRY(ctx, hipMemsetAsync(ctx->stamp_chunks[c], 0, recs * kStampRecordWords * 8, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return LA3DM_OK;
}

// chunks for `records` records (grow only).  Blocks the host until a new chunk is zero; touches no caller stream.
static inline int stamps_reserve(la3dm_ctx *ctx, size_t records) {
    while (ctx->stamp_chunks.size() * kStampChunkRecords < records) {
        void *p = nullptr;
        const size_t bytes = kStampChunkRecords * kStampRecordWords * 8;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            ctx->err = std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e);
            return LA3DM_ERR_OOM;
        }
        ctx->stamp_chunks.push_back((unsigned long long *)p);
        HIP_TRY(ctx, hipMemsetAsync(p, 0, bytes, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return LA3DM_OK;
}

// the next record of the pool for a launch on `stream`
static inline int stamps_acquire(la3dm_ctx *ctx, unsigned long long *&rec, hipStream_t stream) {
    int rc = stamps_reserve(ctx, ctx->stamp_used + 1);
    if (rc != LA3DM_OK) return rc;
    rec = ctx->stamp_chunks[ctx->stamp_used / kStampChunkRecords] + (ctx->stamp_used % kStampChunkRecords) * kStampRecordWords;
    ++ctx->stamp_used;
    ctx->timed_form.push_back(1);
    if (std::find(ctx->stamp_streams.begin(), ctx->stamp_streams.end(), stream) == ctx->stamp_streams.end()) ctx->stamp_streams.push_back(stream);
    return LA3DM_OK;
}

// wait for the stamped launches since the last drain; host != nullptr: their records, oldest first
static inline int stamps_collect(la3dm_ctx *ctx, std::vector<unsigned long long> *host) {
    for (hipStream_t s : ctx->stamp_streams) HIP_TRY(ctx, hipStreamSynchronize(s));
    if (!host) return LA3DM_OK;
    host->resize(ctx->stamp_used * kStampRecordWords);
    for (size_t c = 0; c * kStampChunkRecords < ctx->stamp_used; ++c) {
        const size_t recs = std::min(ctx->stamp_used - c * kStampChunkRecords, kStampChunkRecords);
        HIP_TRY(ctx, hipMemcpy(host->data() + c * kStampChunkRecords * kStampRecordWords, ctx->stamp_chunks[c], recs * kStampRecordWords * 8, hipMemcpyDeviceToHost));
    }
    return LA3DM_OK;
}

// forget every timed call since the last drain: the event pairs go back to their pool, the used stamp records to zero (the
// caller has waited for the launches that write them: stamps_collect)
static inline int timing_reset(la3dm_ctx *ctx) {
    if (ctx->stamp_used) {
        int rc = stamps_zero(ctx, ctx->stamp_used);
        if (rc != LA3DM_OK) return rc;
    }
    ctx->stamp_used = 0;
    ctx->stamp_streams.clear();
    ctx->ev_used = 0;
    ctx->timed_form.clear();
    return LA3DM_OK;
}

// milliseconds from first wave in to last wave out of one record (NaN: no wave wrote it)
static inline float stamps_ms(const unsigned long long *rec, int wall_clock_khz) {
    unsigned long long t_in = ~0ull, t_out = 0;
    for (size_t i = 0; i < kStampEntrySlots; ++i)
        if (rec[i] != 0 && rec[i] < t_in) t_in = rec[i];   // (a grid of fewer than 64 workgroups leaves entry slots at zero)
    for (size_t i = 0; i < kStampExitSlots; ++i) t_out = std::max(t_out, rec[kStampEntrySlots + kStampExitStrideWords * i]);
    if (t_in == ~0ull || t_out < t_in) return __builtin_nanf("");
    return (float)((double)(t_out - t_in) / (double)wall_clock_khz);
}
static inline int timer_begin(la3dm_ctx *ctx, KernelTimer &t, hipStream_t stream) {
    int rc = timer_acquire(ctx, t, false);
    if (rc != LA3DM_OK) return rc;
    if (t) HIP_TRY(ctx, hipEventRecord(t.start, stream));
    return LA3DM_OK;
}
static inline int timer_end(la3dm_ctx *ctx, const KernelTimer &t, hipStream_t stream) {
    if (t) HIP_TRY(ctx, hipEventRecord(t.stop, stream));
    return LA3DM_OK;
}


// ---- internal (devmap.hip -> la3dm_hip.hip): the BGKLV voxel kernel run in place on the device-resident block pool ----
struct la3dm_lv_pool_scan {
    const float *samples, *sorted, *rays;  // as la3dm_lv_scan (device pointers)
    const uint32_t *cell_off;
    int32_t cell_min[3], cell_dim[3];
    uint32_t n_blk;
    const float *blk_center;
    const int32_t *blk_cell0;
    const uint32_t *blk_slot, *blk_mult;   // pool slot and candidate-key multiplicity of every packed block
    float *A, *B;                          // the pool
    uint8_t *S;
    uint32_t npb, pass;
    uint32_t *upd_counter;                 // += nodes updated
    uint32_t n_samples;
    uint32_t plan_n_blk;                   // block count the plan arrays were laid out for (>= n_blk)
    const uint32_t *n_blk_dev;             // plan only: the packed block count, still on the device (nullptr: n_blk)
    uint32_t plan_totals[4];               // read back from the plan: workgroups of split cubes, scratch rows, split cubes,
                                           // workgroups of the other cubes
    uint32_t *plan_totals_dev;             // where the plan left them on the device (the voxel kernel reads [0])
};
// plan once per scan (totals_dev: 3 words the caller reads back into plan_totals), then one scan per pass
int la3dm_bgklv_pool_plan_device(la3dm_ctx *ctx, const la3dm_lv_pool_scan *s, uint32_t *totals_dev, hipStream_t stream);
int la3dm_bgklv_pool_scan_device(la3dm_ctx *ctx, const la3dm_lv_pool_scan *s, hipStream_t stream);
