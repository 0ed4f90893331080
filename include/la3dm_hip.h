/* la3dm_hip.h — C ABI of the MI355X (gfx950) occupancy-inference hot path.
 *
 * This is the drop-in boundary for la3dm's per-scan inference + fusion:
 * everything between "training points gathered per block" and "leaf (alpha, beta,
 * state) updated" runs behind these entry points as hand-written HIP kernels.
 * Plain pointers and sizes only — no C++/torch types.
 *
 * Reference interfaces replaced (paths relative to RobustFieldAutonomyLab/la3dm):
 *   BGK3f::train(x, y) / BGK3f::predict(xs, ybar, kbar)
 *                                   include/bgkoctomap/bgkinference.h:28-44, 52-79, 113-126
 *   the 7-neighbour predict/update loop of BGKOctoMap::insert_pointcloud
 *                                   src/bgkoctomap/bgkoctomap.cpp:293-336
 *   Occupancy::update(ybar, kbar)   src/bgkoctomap/bgkoctree_node.cpp:31-44
 *   Block::get_loc (LUT + centre)   include/bgkoctomap/bgkblock.h:64-66
 * The reference-side binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Threading: one ctx per map, calls on one ctx are serialized by the caller (the
 * reference's insert_pointcloud is single-caller too).  All functions return
 * LA3DM_OK (0) or a negative error code and never throw; la3dm_last_error() gives
 * the text.  There is NO CPU fallback: without a HIP device la3dm_create fails with
 * LA3DM_ERR_NODEVICE.
 */
#ifndef LA3DM_HIP_H
#define LA3DM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct la3dm_ctx la3dm_ctx;

enum {
    LA3DM_OK = 0,
    LA3DM_ERR_ARG = -1,      /* null / inconsistent argument */
    LA3DM_ERR_HIP = -2,      /* a HIP runtime call failed */
    LA3DM_ERR_NODEVICE = -3, /* no usable HIP device */
    LA3DM_ERR_OOM = -4,      /* device arena allocation failed */
    LA3DM_ERR_PEER = -5,     /* block-sharded insert: another rank failed in its rank-local work; every rank gives the insert up */
    LA3DM_ERR_LIMIT = -6     /* a bounded loop of a query ran out before its answer was complete (travel: LA3DM_TRAVEL_MAX_ROUNDS; clusters: LA3DM_CLUSTERS_MAX_ROUNDS) */
};

/* Occupancy state codes, include/bgkoctomap/bgkoctree_node.h:10-12 */
enum { LA3DM_FREE = 0, LA3DM_OCCUPIED = 1, LA3DM_UNKNOWN = 2, LA3DM_PRUNED = 3 };
/* OR-ed into the per-leaf state byte when Occupancy::update ran for that leaf
 * in this scan (the reference sets node.classified = true there). A leaf whose
 * byte has this bit clear was not touched: its alpha/beta/state are unchanged. */
#define LA3DM_LEAF_UPDATED 0x80u

/* la3dm_bgk_scan.flags */
#define LA3DM_SCAN_UPDATE_UNGATED 0x1u /* insert_training_data semantics: update even when kbar == 0
                                          (src/bgkoctomap/bgkoctomap.cpp:179-185) */
#define LA3DM_SCAN_LABELS_01 0x2u      /* the caller guarantees that every training label is exactly 0.0f or 1.0f (what
                                          get_training_data produces, bgkoctomap.cpp:383-458): bgk_sum = 1 may then run the
                                          table kernel on the un-pruned blocks.  Without it the general kernel runs (and
                                          detects other labels itself). */
#define LA3DM_SCAN_FULL_BLOCKS 0x4u    /* the caller guarantees that every test block of the call holds all its
                                          8^(block_depth-1) finest-level leaves (nothing pruned: e.g. every block was
                                          created by this scan).  Only a hint for the kernel choice of bgk_sum = 1; a
                                          block that breaks the promise is left untouched. */

#define LA3DM_SCAN_ROWS_PREPARED 0x8u  /* la3dm_bgkl_scan_device only: train_xyzy holds the rows in the kernels' own 12-float form
                                          {x0 y0 z0 x1 | y1 z1 label [segment shorter than 0.1 mm ? 1 : 0] | lx ly lz |l|^2} (what
                                          the library otherwise derives from the 8-float rows in a launch of its own, the same fp32
                                          expressions as point_to_line_dist, bgklinference.h:104-118) — the device-resident map
                                          writes its rows in that form directly */

/* Map-wide constants: the statics BGKOctoMap's constructor sets
 * (src/bgkoctomap/bgkoctomap.cpp:31-56) plus the voxel look-up table
 * Block::key_loc_map (src/bgkoctomap/bgkblock.cpp:7-32) flattened depth-major:
 * entry (depth d, index i) at ((8^d - 1) / 7 + i), 3 floats each. */
typedef struct la3dm_params {
    float resolution;
    int32_t block_depth;
    float sf2;
    float ell;
    float free_thresh;
    float occupied_thresh;
    float var_thresh;
    float prior_A;
    float prior_B;
    int32_t device;       /* HIP device ordinal */
    const float *lut_xyz; /* host pointer, lut_count * 3 floats; copied */
    uint32_t lut_count;   /* sum_{d<block_depth} 8^d */
    /* variant: 0 = BGKOctoMap (fields above), 1 = GPOctoMap: the statics of
     * src/gpoctomap/gpoctomap.cpp:29-46 (var_thresh, prior_A/B unused; leaf arrays alpha/beta then
     * carry the node's m_ivar/ivar, src/gpoctomap/gpoctree_node.h:34) */
    int32_t variant;
    float noise;          /* GP noise variance */
    float l;              /* logistic length scale */
    float min_ivar;       /* 1 / max_var */
    float max_ivar;       /* 1 / min_var */
    float min_known_ivar; /* 1 / max_known_var */
    /* variant 2 = BGKLVOctoMap (src/bgklvoctomap/bgklvoctomap.cpp:33-62): fields of variant 0 plus */
    float min_W;          /* minimum total weight, src/bgklvoctomap/bgklvoctree_node.cpp:29-47 */
} la3dm_params;

/* One scan's worth of work for the BGK kernel.
 *  - training points are grouped by training block (CSR): block b owns points
 *    [train_off[b], train_off[b+1]); each point is (x, y, z, label) fp32, label 1 = hit,
 *    0 = free-beam sample  (bgkoctomap.cpp:265-277).
 *  - test block t has centre blk_center[3t..], leaves [leaf_off[t], leaf_off[t+1]) in
 *    OcTree::LeafIterator order, and up to 7 neighbour training blocks nbr[7t..7t+6] in
 *    ExtendedBlock order self,+x,-x,+y,-y,+z,-z  (-1 = no trained model there).
 *  - leaf_key[l] = (depth << 16) + index  (OcTreeHashKey, bgkoctree.cpp:9-11).
 *  - alpha/beta are in/out (m_A, m_B); state is out (see LA3DM_LEAF_UPDATED).
 * A test block must appear at most once per call (the caller runs repeated keys as
 * separate calls, preserving the reference's serial semantics).
 * A training point at no finite distance (a NaN coordinate, a coordinate so large that the squared distance
 * overflows) makes ybar / kbar of its training block NaN at every leaf, as in the reference: a gated scan rejects that
 * neighbour's update (bgk_sum 0) or, with one sum over all seven neighbours, the leaf's only update (bgk_sum 1); an ungated
 * scan leaves alpha = beta = NaN. */
typedef struct la3dm_bgk_scan {
    const float *train_xyzy;   /* [n_train_pts * 4] */
    const uint32_t *train_off; /* [n_train_blk + 1] */
    uint32_t n_train_pts;
    uint32_t n_train_blk;
    const int32_t *nbr;        /* [n_test_blk * 7] */
    const float *blk_center;   /* [n_test_blk * 3] */
    const uint32_t *leaf_off;  /* [n_test_blk + 1], absolute indices into the leaf arrays */
    uint32_t n_test_blk;
    uint32_t n_leaf;           /* length of the leaf arrays */
    const uint32_t *leaf_key;  /* [n_leaf] */
    float *alpha;              /* [n_leaf] in/out */
    float *beta;               /* [n_leaf] in/out */
    uint8_t *state;            /* [n_leaf] out */
    uint32_t flags;
    /* optional hints for la3dm_gp_scan_* (0 = unknown: the library computes them on the device and
     * synchronises once): largest training block and sum over training blocks of N_b^2 */
    uint32_t train_max_n;
    uint64_t train_sum_n2;
} la3dm_bgk_scan;

/* Per-call work counters (filled by the *_scan_* calls when `out` is non-null). */
typedef struct la3dm_bgk_counters {
    uint64_t n_tiles;          /* 64-leaf tiles launched */
    uint64_t scratch_bytes;    /* device scratch used by this call */
} la3dm_bgk_counters;

int la3dm_device_count(void);
const char *la3dm_version(void);

int la3dm_create(const la3dm_params *params, la3dm_ctx **out);
void la3dm_destroy(la3dm_ctx *ctx);
const char *la3dm_last_error(const la3dm_ctx *ctx); /* ctx may be NULL: last create error */

/* Options: "bgk_sum" — the sum mode of the BGK family's kernels (BGKOctoMap; since round 5 also BGKLOctoMap and
 * BGKLVOctoMap, where 1 = each neighbour's / voxel's two sums formed in double from the same fp32 terms and rounded to fp32
 * once, the gates and node updates unchanged, and 0 = the reference's fp32 running sums in row / gather order).  For the BGK
 * predict + fuse kernel:
 *   1 (default; env LA3DM_BGK_SUM sets the default of new contexts) = order-free: every leaf's sum(k), sum(k y) in double
 *     accumulators over all 7 neighbours, alpha / beta rounded once.  Within ~4e-7 of the reference's fp32 chains on p;
 *     NOT the reference's summation order; what bench.py's headline is quoted on (and labelled so).  Two kernels share
 *     the mode: bgk_predict_fuse_t ("bgk_tables" 1, the default; env LA3DM_BGK_TABLES) — per-axis distance tables for the
 *     tiles of un-pruned blocks, the general path for the others in the same launch; needs LA3DM_SCAN_LABELS_01 — and
 *     bgk_predict_fuse_r ("bgk_tables" 0, and every scan without that flag).  Same pairs, same kernel values, same sums.
 *     "bgk_one_launch" 1 (default; env LA3DM_BGK_ONE_LAUNCH) = a table scan whose blocks are all full (LA3DM_SCAN_FULL_BLOCKS, verified from
 *     the leaf count) at block_depth 3 — the first scan into an empty map — runs as ONE launch: bgk_predict_fuse_t1 reads the caller's
 *     unscaled points and the nbr / train_off arrays itself, no scaled copy of the points and no scratch (scratch_bytes 0);
 *     0 = the prescale launch + bgk_predict_fuse_t, as every other scan.  Bit-identical results.
 *     "bgk_scan1_generic" 0 (default; env LA3DM_BGK_SCAN1_GENERIC) = that one launch runs the instance of the kernel with its scan compiled in
 *     (depth 3, sf2 == 1, x / ell by the reciprocal, default remap, gated, no profiling switch) wherever those conditions hold, the generic
 *     instance elsewhere; 1 = the generic instance always (A/B switch).  Bit-identical results.  la3dm_get_option "bgk_scan1_instance" (read-only)
 *     says what the last la3dm_bgk_scan_device call launched: 2 the production instance, 1 the generic one, 0 not the one launch.
 *     "bgk_tile_desc" 1 (default) = at block_depth >= 4 every 64-leaf tile of a full block gets its own neighbour descriptor
 *     without the face neighbours its voxel cube cannot reach (only while ell <= 4 * resolution; 0 = block-wide descriptors; same results).
 *   0 = the reference's fp32 summation order (bgk_predict_fuse_v5): bit-identical to the CPU restatement, the regression
 *     mode of the parity suites.
 * "gp_mode" (GPOctoMap; env LA3DM_GP_MODE) 0 = every inner product an fp32 FMA chain in ascending order, on the VALU and the matrix
 * cores alike (default: the parity configuration), 1 = the order of operations of an x86-64 / SSE2 build of Eigen 3.3.7 on the VALU
 * (no FMA, packet sums, llt_inplace blocking, panels of 8 with reciprocal diagonals, packet exp: la3dm_amd/csrc/gp_eigen_kernels.h),
 * bit-identical to the restatement's oracle.set_gp_mode(1); training blocks of up to 128 points (block_depth 3), else LA3DM_ERR_ARG.
 * "grid_order" (the maps' voxel-grid filters, device-resident and host-orchestrated) 0 = ascending cloud index inside a cell (default), 1 = what pcl::VoxelGrid's own
 * std::sort on the cell index alone leaves (src/bgkoctomap/bgkoctomap.cpp:419-431): the keys are sorted on the HOST by libstdc++ —
 * a verification mode, slow by design, single GPU; with "fast_trig" 3 (and "gp_mode" 1) the device path is bit-identical to the
 * restatement's oracle.set_modes(1, 1): the configuration a ROS Noetic build of the reference most plausibly runs.
 * "fast_trig" 0 = correctly rounded sin/cos (default: the parity configuration), 1 = f32 polynomial, 2 = OCML (BGK kernels
 * only), 3 = Eigen 3.3.7's psin / pcos without FMA — the arithmetic a ROS Noetic build of the reference most plausibly runs
 * (include/bgkoctomap/bgkinference.h:115-116), for the BGK, BGK-L and BGK-LV kernels, bit-identical to the restatement's
 * oracle.set_modes(1, 0); "waves_per_wg" 1/2/4 (bgk_sum 0),
 * "remap" 0-2, "ablate" 0-31 and "lds_pad" (profiling: extra dynamic LDS bytes on the BGK predict launch); values outside
 * these sets are rejected with LA3DM_ERR_ARG;
 * "time_kernel" see la3dm_kernel_times; "bgkl_split_rows" (variant 3): tiles whose seven neighbours hold more
 * rows than this take the split path (default 1024 — env LA3DM_BGKL_SPLIT_ROWS sets another default —, -1 = never, values outside
 * -1 .. 2^24 are rejected; results do not depend on it); "bgkl_dense_add" 1 (default) =
 * the split tiles' rows are expanded for all items at once (64 KB more scratch per item) and added by a copy-only replay,
 * 0 = the replay expands them itself (results do not depend on it; bgk_sum 0 only — the order-free mode has no replay). */
int la3dm_set_option(la3dm_ctx *ctx, const char *name, int value);
/* current value of an option that has one ("bgk_sum", "bgk_tables", "bgk_one_launch", "bgk_scan1_generic", "bgk_tile_desc", "fast_trig", "gp_mode", "grid_order", "waves_per_wg", "remap");
 * read-only, not an option la3dm_set_option knows: "bgk_scan1_instance" = what the last la3dm_bgk_scan_device call launched (2 / 1 / 0, see "bgk_scan1_generic") */
int la3dm_get_option(const la3dm_ctx *ctx, const char *name, int *value);

/* All pointers in *scan are HOST pointers. Synchronous: H2D, kernels, D2H. */
int la3dm_bgk_scan_host(la3dm_ctx *ctx, const la3dm_bgk_scan *scan, la3dm_bgk_counters *out);

/* All pointers in *scan are DEVICE pointers (on params.device). Asynchronous on
 * `stream` (a hipStream_t passed as void*, NULL = the default stream). The ctx's
 * scratch arena is reused by the next call, so calls must be stream-ordered. */
int la3dm_bgk_scan_device(la3dm_ctx *ctx, const la3dm_bgk_scan *scan, void *stream, la3dm_bgk_counters *out);

/* GPOctoMap (variant 1).  Same scan layout; labels are +1 (hit) / -1 (free)
 * (src/gpoctomap/gpoctomap.cpp:399); alpha/beta are the leaves' m_ivar/ivar.  Replaces
 * GPR3f::train (include/gpoctomap/gpregressor.h:42-51: Matern-3/2 K + noise I, LLT, alpha) for every
 * training block, GPR3f::predict (:80-92: m = Ks^T alpha, v = L^-1 Ks, var = sf2 - diag(v^T v)) for
 * every (test block, neighbour), and the unconditional BCM Occupancy::update
 * (src/gpoctomap/gpoctree_node.cpp:36-49) in ExtendedBlock order.  A neighbour whose training block holds no
 * points (train_off[b] == train_off[b + 1]) is skipped like -1: no model, no update. */
int la3dm_gp_scan_host(la3dm_ctx *ctx, const la3dm_bgk_scan *scan, la3dm_bgk_counters *out);
int la3dm_gp_scan_device(la3dm_ctx *ctx, const la3dm_bgk_scan *scan, void *stream, la3dm_bgk_counters *out);

/* BGKLVOctoMap (variant 2): per-voxel inference against hit points and free-space line segments.
 * Replaces, for every base-resolution leaf of every block, the body of the leaf loop of
 * BGKLVOctoMap::insert_pointcloud (src/bgklvoctomap/bgklvoctomap.cpp:155-244): the +-ell box query, the
 * one-row-per-ray de-duplication, BGKLV3f::predict (include/bgklvoctomap/bgklvinference.h:76-157: point-to-
 * segment distance, r = min(d/ell, 1), sparse kernel without the < 0 clamp), the kbar > 0.001 gate and the LV
 * Occupancy::update (src/bgklvoctomap/bgklvoctree_node.cpp:29-77).
 *
 *  - samples: every training sample in original order, (x, y, z, ray) with ray = -1 for a hit, else the index
 *    of its segment (bgklvoctomap.cpp:303-423 builds them); a ray's samples are contiguous, first = segment start.
 *    PRECONDITION: along a ray every coordinate of its samples is monotone (non-decreasing or non-increasing, as stored in
 *    fp32) — true of samples taken along a straight segment.  The samples of a ray inside a voxel's box are then one
 *    contiguous run, and the kernel finds the run's first sample (the one that adds the ray's row) by looking at the ray's
 *    first sample and at the previous sample only; samples that wander in and out of a box would add a row per entry.
 *  - sorted: the same samples bucketed on a grid of edge g aligned with the blocks (bucket = floor((v +
 *    block_size/2) / g), g = 4 * resolution for block_depth >= 3 else block_size), buckets x-fastest over
 *    [cell_min, cell_min + cell_dim), ascending original index inside a bucket; w = original index (int bits).
 *  - rays: 8 floats per segment: start xyz, index of its first sample (int bits), end xyz, 0.
 *  - blocks: centre, bucket coordinates of the block's lowest bucket, and dense per-node arrays of the
 *    FINEST layer only (8^(block_depth-1) nodes per block, octree index order): alpha, beta in/out; state in:
 *    LV code of the node (4 = pruned / not a base-resolution leaf: skipped); state out: LA3DM_LEAF_UPDATED |
 *    new state when update() ran, LA3DM_LV_HAS_INFO when the voxel's box held any sample.  Every state byte is rewritten:
 *    a node that came in as 4 comes back as 0, like any node that was not updated and saw no sample (alpha, beta untouched). */
#define LA3DM_LV_HAS_INFO 0x40u
enum { LA3DM_LV_FREE = 0, LA3DM_LV_OCCUPIED = 1, LA3DM_LV_UNKNOWN = 2, LA3DM_LV_UNCERTAIN = 3, LA3DM_LV_PRUNED = 4 };
typedef struct la3dm_lv_scan {
    const float *samples;     /* [n_samples * 4] */
    const float *sorted;      /* [n_samples * 4] */
    uint32_t n_samples;
    const float *rays;        /* [n_rays * 8] */
    uint32_t n_rays;
    const uint32_t *cell_off; /* [cell_dim[0]*cell_dim[1]*cell_dim[2] + 1] */
    int32_t cell_min[3];
    int32_t cell_dim[3];
    uint32_t n_blk;
    const float *blk_center;  /* [n_blk * 3] */
    const int32_t *blk_cell0; /* [n_blk * 3] */
    float *alpha;             /* [n_blk * 8^(depth-1)] in/out */
    float *beta;
    uint8_t *state;           /* in/out */
} la3dm_lv_scan;
int la3dm_bgklv_scan_host(la3dm_ctx *ctx, const la3dm_lv_scan *scan, la3dm_bgk_counters *out);
int la3dm_bgklv_scan_device(la3dm_ctx *ctx, const la3dm_lv_scan *scan, void *stream, la3dm_bgk_counters *out);

/* Kernel timing.  After la3dm_set_option(ctx, "time_kernel", 1) every *_scan_device call
 * times its dominant kernel with a pair of HIP events on the launch stream.
 * la3dm_bgk_scan_device (one launch: bgk_predict_fuse_*; bgk_prepare is not in the figure)
 * hands the pair to the launch itself (hipExtLaunchKernelGGL): the stop event is bound to the
 * kernel's own dispatch packet and costs nothing on the stream; the start event is, with the
 * HIP 7.2 runtime, still one marker packet ahead of the kernel (measured: DESIGN section 5,
 * profiles/step_gap).  The GP and BGK-LV scans, whose dominant step is several launches, record
 * one event before and one after them (two marker packets on the stream).
 * The one-launch BGK scan (bgk_predict_fuse_t1: block_depth 3, full blocks) uses no event at
 * "time_kernel" 1: a plain launch of an instance of the kernel that reads the device's wall clock
 * as each wave enters and leaves and keeps the stamps in a record owned by the context, so a timed
 * step puts nothing but the kernel on the stream.  Its figure is FIRST WAVE IN TO LAST WAVE OUT: it
 * leaves out the dispatch set-up before the first wave and the end-of-kernel cache write-back after
 * the last, which an event pair or a kernel trace includes (1.1 - 1.5 us on small grids); the stamped
 * instance is itself about 2 us slower on the 200 k-ray scan, where its figure reads 0.5 us above the
 * event pair's (profiles/kernel_stamps).  "time_kernel" 2 times that scan with the event pair as well
 * (every other scan: the same as 1); so does 1 on a device that reports no wall-clock rate.
 * This call waits for the timed launches, writes the elapsed milliseconds of each scan call since
 * the last call (oldest first whichever way each was timed, at most cap; *n_out = how many there
 * were) and resets the list.  Setting "time_kernel" drops what was timed and not read. */
int la3dm_kernel_times(la3dm_ctx *ctx, float *ms, uint32_t cap, uint32_t *n_out);

/* Diagnostics used by the parity tests: evaluate one primitive of the device
 * arithmetic elementwise on host arrays.  op: 0 sqrt(x)  1 sin(x)  2 cos(x)
 * 3 sparse kernel k(r) with the ctx's sf2 (clamped)  4 x / ell  5 k(r) unclamped
 * 9 / 10 the correctly rounded sin / cos of the kernels  12 / 13 node state of the pairs (alpha, beta) =
 * (in[2 j], in[2 j + 1]) with the ctx's thresholds, by the kernels' approximate-quotient form / by the IEEE
 * divisions of bgkoctree_node.cpp:36-43 (out[2 j] = state). */
int la3dm_diag_eval(la3dm_ctx *ctx, int op, const float *in, uint32_t n, float *out);


/* Exhaustive device-side sweep over every fp32 bit pattern in [lo_bits, hi_bits]: counts the
 * inputs where a shortcut of the kernel differs from the IEEE result.  what: 0  x/3 by
 * reciprocal+FMA correction, 1  x/(2*pi') likewise, 2  lean sqrt vs correctly rounded sqrt,
 * 3  sin/cos (f64 kernels rounded to f32) vs the f64 library functions rounded to f32,
 * 7  +-x / ell by the context's reciprocal + correction vs the IEEE division (always equal when the context fell back
 *    to the division), 8  k(sqrt(x)) > 0 with the context's sf2 (the FIFO kernel's hit threshold 0x3f77c08d claims: none
 *    in [0x3f77c08d, 0x3f7fffff]),  10  the GP kernels' exp(x) for x in [-87, -0] vs the f64 library exp rounded to f32. */
int la3dm_diag_sweep(la3dm_ctx *ctx, int what, uint32_t lo_bits, uint32_t hi_bits, uint64_t *mismatches);

/* Test hook for the property the GP kernels' matrix-core paths rely on: D = A B (A 32 x K row-major, B K x 32
 * row-major, K even, host pointers) through v_mfma_f32_32x32x2_f32 versus fmaf chains over k ascending, compared
 * on the device; *mismatches = number of outputs whose bits differ (0 on gfx950). */
int la3dm_diag_mfma_chain(la3dm_ctx *ctx, const float *A, const float *B, int K, uint32_t *mismatches);

/* BGKLOctoMap (params.variant = 3): block-level BGK with free-space line segments.  Replaces
 * BGKLInference::train/predict (include/bgkloctomap/bgklinference.h:44-88: point_to_line_dist :104-140,
 * covSparseLine :186-200) + the update loop gated on kbar > 0.001 (src/bgkloctomap/bgkloctomap.cpp:206-231).
 * Same la3dm_bgk_scan layout, except that train_xyzy holds ROWS OF 8 FLOATS {x0,y0,z0, x1,y1,z1, label, 0}
 * (hits = degenerate segments with label 1; one row per beam and block with label 0), n_train_pts = number of
 * rows and train_off is the CSR over training blocks in rows.  The device form enqueues on `stream`; it waits for
 * the stream once (item count) to size the scratch of the split path — set "bgkl_split_rows" < 0 for a call that never
 * blocks. */
int la3dm_bgkl_scan_host(la3dm_ctx *ctx, const la3dm_bgk_scan *s, la3dm_bgk_counters *out);
int la3dm_bgkl_scan_device(la3dm_ctx *ctx, const la3dm_bgk_scan *s, void *stream, la3dm_bgk_counters *out);

/* ------------------------------------------------------------------------------------------------
 * Device-resident map: the block pool (alpha, beta, state of every node of
 * every block) lives in HBM and BGKOctoMap::insert_pointcloud (src/bgkoctomap/bgkoctomap.cpp:214-366)
 * runs start to finish on the GPU:
 *   f1  get_training_data (:383-417), beam_sample (:433-458), downsample (:419-431, pcl::VoxelGrid)
 *   f2  bbox / get_blocks_in_bbox (:464-495), closed-box gather (:497-552, rtree.h:1519-1532),
 *       ExtendedBlock (bgkblock.cpp:85-130), block creation (:298-305)
 *   E   la3dm_bgk_scan_device / la3dm_gp_scan_device / la3dm_bgkl_scan_device (above)
 *   f3  leaf enumeration (bgkoctree.h:62-147), node write-back, OcTree::prune (bgkoctree.cpp:101-148)
 * Only the cloud goes in; the host reads nodes back on demand (la3dm_devmap_download).  Results are
 * bit-identical to the host-orchestrated path.  Works for variant 0 (BGK), 1 (GP), 3 (BGK-L: the front end of
 * src/bgkloctomap/bgkloctomap.cpp:300-381 and the training rows of :141-170 take the place of f1 / the gather) and 2
 * (BGK-LV, see la3dm_devmap_lv_stats below) contexts. */
typedef struct la3dm_devmap la3dm_devmap;

typedef struct la3dm_devmap_stats {
    uint64_t n_hits, n_frees;          /* training set after the front end */
    uint64_t n_train_blocks;           /* blocks that hold training points */
    uint64_t n_test_blocks;            /* test blocks (all passes) */
    uint64_t n_bbox_blocks;            /* entries of the candidate list */
    uint64_t voxel_updates;            /* U: leaves of the test blocks */
    uint64_t train_reads;              /* sum over test blocks of their 7-neighbourhood training points */
    uint64_t pair_evals;               /* sum over test blocks of neighbourhood points x leaves (P) */
    uint64_t n_blocks;                 /* blocks in the pool after the scan */
    uint32_t n_passes;                 /* 1 + repeats of a key in the candidate list */
    double t_frontend, t_partition, t_pack, t_kernel, t_commit, t_total; /* seconds, host clock at sync points */
    double t_gather;                   /* sharded insert with LA3DM_TIMING=1: the all-gather-v (else inside t_kernel) */
} la3dm_devmap_stats;

/* The devmap keeps a pointer to `ctx`: destroy the devmap BEFORE the context (la3dm_destroy refuses — keeps the context
 * alive and reports on stderr — while a devmap still points at it). */
int la3dm_devmap_create(la3dm_ctx *ctx, la3dm_devmap **out);
void la3dm_devmap_destroy(la3dm_devmap *dm);
/* cloud: n points, `stride` floats apart (>= 3), host memory */
int la3dm_devmap_insert_pointcloud_host(la3dm_devmap *dm, const float *xyz, uint32_t n, uint32_t stride,
                                        const float origin[3], float ds_resolution, float free_resolution,
                                        float max_range, la3dm_devmap_stats *stats);
/* cloud: n packed xyz triples in device memory; runs on the context's OWN (non-blocking) stream and returns after the last
 * kernel has been enqueued and the few scalar read-backs the launch sizes depend on.  That stream is not ordered against
 * the stream that produced d_xyz: either the cloud is complete before the call (synchronise the producer), or record a
 * hipEvent_t on the producing stream and hand it to la3dm_devmap_wait_event first — the insert then starts behind it. */
int la3dm_devmap_wait_event(la3dm_devmap *dm, void *event /* hipEvent_t */);
int la3dm_devmap_insert_pointcloud_device(la3dm_devmap *dm, const float *d_xyz, uint32_t n, const float origin[3],
                                          float ds_resolution, float free_resolution, float max_range,
                                          la3dm_devmap_stats *stats);
/* BGKOctoMap::insert_training_data (src/bgkoctomap/bgkoctomap.cpp:82-212) on the pool: n labelled points
 * {x, y, z, label} (host pointer) take the place of the front end's output; every leaf of every test block is updated
 * for every neighbour model (LA3DM_SCAN_UPDATE_UNGATED), then the test blocks are pruned. */
int la3dm_devmap_insert_training_data_host(la3dm_devmap *dm, const float *xyzy, uint32_t n, la3dm_devmap_stats *stats);
/* BGKLVOctoMap (variant 2) on the device-resident pool: la3dm_devmap_insert_pointcloud_{host,device} run
 * BGKLVOctoMap::insert_pointcloud (src/bgklvoctomap/bgklvoctomap.cpp:89-285) start to finish on the GPU — voxel filter of
 * the hits, ray shortening and the downward-ray filter (:303-423), free segments and their samples (:439-462), the
 * candidate blocks of the bounding box (all created, :105-135), the gather grid that stands in for the R-tree, the
 * per-voxel kernel in place on the pool (once per repeat of a candidate key), prune of the blocks that had information
 * (:262-273, only with original_size).  The pool stores the host enum of the states (PRUNED 3, UNCERTAIN 4), so
 * la3dm_devmap_download / _search_host / _key_bounds serve this variant unchanged. */
typedef struct la3dm_devmap_lv_stats {
    uint64_t n_hits;           /* hit samples */
    uint64_t n_rays;           /* free segments */
    uint64_t n_samples;        /* hit + segment samples */
    uint64_t n_bbox_blocks;    /* entries of the candidate list */
    uint64_t n_packed_blocks;  /* blocks with a sample within reach */
    uint64_t voxels;           /* base-resolution voxels of the packed blocks */
    uint64_t voxel_updates;    /* Occupancy::update calls (all passes) */
    uint64_t n_info_blocks;    /* blocks that had information (pruned afterwards) */
    uint64_t n_blocks;         /* blocks in the pool after the scan */
    double t_frontend, t_total; /* seconds; t_frontend = everything before the first voxel kernel */
} la3dm_devmap_lv_stats;
int la3dm_devmap_lv_stats_get(la3dm_devmap *dm, la3dm_devmap_lv_stats *out);
/* BGKLVOctoMap's constructor argument original_size (prune after the scan): default 1 */
int la3dm_devmap_lv_set_original_size(la3dm_devmap *dm, int original_size);
/* samples {x, y, z, ray (-1 = hit)} and segments {start xyz, end xyz} of the last scan (host buffers; NULL = counts only) */
int la3dm_devmap_lv_training(la3dm_devmap *dm, float *samples4, uint32_t cap_samples, float *rays6, uint32_t cap_rays,
                             uint32_t *n_samples, uint32_t *n_rays);

/* Block-sharded insert_pointcloud (BASELINE configs[4]): `world` replicas of the map, one per GPU / process,
 * every one is handed the same cloud; front end and partition run redundantly, the test-block list is cut into `world`
 * contiguous ranges of equal weight in candidate order, rank r predicts + fuses range r only, then ONE all-gather-v
 * reassembles the updated leaves on every rank, and commit + prune run everywhere: after the call all replicas are
 * identical to a single-GPU map, bit for bit.
 * The exchange is IN PLACE on the scan's leaf arrays (alpha, beta: 4 B per leaf, state: 1 B per leaf, and — single-pass scans,
 * where a rank lists the leaves of its own range only and the write-back finds a foreign leaf's node from its key and this
 * replica's slot of the block — the leaf keys: 4 B per leaf; a rank's leaves are a contiguous index range of each): no pack /
 * unpack copies, no padding — the payload is exactly 13 B per leaf of the scan (9 B in a multi-pass scan).
 * The library has no communication dependency: `fn` is called once per pass with nseg = 4 (or 3) segments; for segment s, rank q
 * owns bytes [offset[q], offset[q] + bytes[q]) of the DEVICE buffer `base` (filled for q = rank by work already queued
 * on `stream`), and fn must queue on `stream` — or order against it — an all-gather-v that fills every other rank's
 * bytes, e.g. between ncclGroupStart / ncclGroupEnd one ncclBroadcast(base + offset[q], base + offset[q], bytes[q],
 * ncclUint8, q, comm, stream) per rank and segment.  Nothing synchronises the host: the library queues commit and prune
 * behind the call on the same stream.  fn returns 0 on success.  A rank whose own kernel launch failed still calls fn (its
 * bytes are then not meaningful) so that no peer waits in the collective for ever, and reports the error afterwards.
 * Besides that per-pass call the front end calls fn once per insert with ONE segment of 4 bytes per rank (the rank's
 * status / count word: a rank that failed on its own posts a failure word and every rank returns — LA3DM_ERR_PEER on
 * the healthy ones) and, when the insert shards its sample filter, once more with one segment of 12 bytes per sample.
 * world = 1 switches sharding off.  Variants 0 (BGK) and 1 (GP). */
typedef struct la3dm_gather_seg {
    void *base;              /* device pointer */
    const uint64_t *offset;  /* [world] byte offset of rank q's range */
    const uint64_t *bytes;   /* [world] byte count of rank q's range */
} la3dm_gather_seg;
typedef int (*la3dm_allgatherv_fn)(void *user, const la3dm_gather_seg *segs, uint32_t nseg, uint32_t world, uint32_t rank,
                                   void *stream);
int la3dm_devmap_set_shard(la3dm_devmap *dm, uint32_t rank, uint32_t world, la3dm_allgatherv_fn fn, void *user);
int la3dm_devmap_block_count(la3dm_devmap *dm, uint32_t *n_blocks, uint32_t *nodes_per_block);
/* keys[n_blocks]; A, B, S [n_blocks * nodes_per_block], node order = depth-major (8^d - 1)/7 + index;
 * S: bits 0-2 State (FREE 0, OCCUPIED 1, UNKNOWN 2, PRUNED 3), bit 7 = classified */
int la3dm_devmap_download(la3dm_devmap *dm, int64_t *keys, float *A, float *B, uint8_t *S);
/* Save and load: the map as a compact stream of its COVERING LEAVES (csrc/devmap_pack.h; the format's host code — layout,
 * validator, host writer — is csrc/host/pack_format.h, shared with the host-mode map).
 *
 *   A covering leaf is a node that is not PRUNED and is either on the finest layer or has child 0 PRUNED — OcTree::is_leaf,
 *   the image of covering_leaf over the finest cells.  The leaves of a block tile it; everything else in the pool is dead:
 *   PRUNED children keep stale values nothing reads, the nodes above the leaves never leave their defaults.
 *
 *   The stream.  Little-endian; every section starts at a multiple of 16 bytes; padding bytes are zero, so two packs of
 *   one pool are byte-identical.
 *     header, 128 bytes = la3dm_pack_header:
 *         0  char magic[8] = "LA3DMAP\0"          8  u32 version = 1          12  u32 header_bytes = 128
 *        16  u32 variant (0 BGK, 1 GP, 2 BGK-LV, 3 BGK-L)   20  u32 block_depth   24  u32 nodes_per_block = (8^block_depth - 1) / 7
 *        28  u32 flags (bit 0: BGK-LV original_size; the other bits 0)
 *        32  u64 n_blocks       40  u64 n_leaves       48  u64 total_bytes (the whole stream, header included)
 *        56  f32 init_A, init_B: the values of a node never written — prior_A, prior_B; GP: 0, min_ivar = 1 / max_var
 *        64  f32 resolution, sf2, ell, free_thresh, occupied_thresh, var_thresh, prior_A, prior_B, noise, l, min_var, max_var,
 *            max_known_var, min_W — what the map class was constructed with, 0 where the class has no such argument (GP:
 *            var_thresh, prior_A, prior_B; noise .. max_known_var on the others; min_W except on BGK-LV).  The raw entry
 *            points below only know the context's inverses and write min_var = 1 / max_ivar, max_var = 1 / min_ivar,
 *            max_known_var = 1 / min_known_ivar; the map classes write their constructor arguments.
 *       120  8 reserved bytes, zero
 *     then, each at the next multiple of 16:
 *       keys     i64[n_blocks]        block hash keys (x << 40 | y << 20 | z, 20 bits each), distinct, any order
 *       leaf_off u32[n_blocks + 1]    exclusive prefix of the blocks' leaf counts; leaf_off[n_blocks] = n_leaves
 *       mask     u32[n_blocks * W]    W = ceil(nodes_per_block / 32); bit n % 32 of word n / 32 of a block's W words is set when
 *                                     node n (la3dm_devmap_download's depth-major numbering) is a covering leaf; bits at or
 *                                     past nodes_per_block are clear
 *       state    u8[n_leaves]         the pool's S byte unchanged (bits 0-2 State, bit 7 classified)
 *       A        f32[n_leaves]        a block's leaves in ascending node number, block b's at [leaf_off[b], leaf_off[b + 1]);
 *       B        f32[n_leaves]        values are copied bit for bit
 *     Block order is the writer's: pool slot order from the device pool, ascending key from a host-mode map.  An empty map
 *     is the header alone.  Per block the stream holds 12 + 4 W + 9 L bytes (L leaves, L <= 8^(block_depth - 1)) against the
 *     8 + 9 nodes_per_block of la3dm_devmap_download: never more from block_depth 2 up.
 *     NOT in the stream: the last scan's training data, the statistics, the options (la3dm_set_option) and the shard
 *     configuration.
 *
 *   la3dm_devmap_pack_host: count kernel (S only -> leaf counts and mask words, the wave's ballots), the map's one-launch
 *     scan over the counts, one read-back of n_leaves, emit kernel (state, A, B of the leaves to leaf_off[b] + rank), one
 *     copy of the stream and one synchronisation.  buf = NULL: *size only.  cap < *size: LA3DM_ERR_ARG, *size set.  Changes
 *     nothing in the pool.  A poisoned map is refused.
 *   la3dm_devmap_unpack_host: the stream is validated on the host BEFORE the first allocation or launch (magic, version,
 *     sizes, section extents, n_blocks * nodes_per_block < 2^32, distinct keys of 60 bits, leaf_off against the mask
 *     popcounts, no mask bit past the end, no leaf under a leaf, the leaves tile the block, leaf states not PRUNED and known
 *     to the variant with bits 3-6 clear, zero padding), then compared with the context: variant, block_depth,
 *     nodes_per_block and, by bit pattern, resolution, init_A, init_B must agree — the other header floats are
 *     informational, a loaded map may be continued with another ell.  The map must hold no blocks.  One expand kernel
 *     writes every node of every block once — the CANONICAL pool: a leaf takes its (A, B, state); a node under a leaf
 *     (init_A, init_B, PRUNED); every other node (init_A, init_B, UNKNOWN) — then the block table is rebuilt.  No insert and
 *     no query reads more of a dead node than its State; la3dm_devmap_search_host at a collapsed voxel reports PRUNED with
 *     the default values where the original pool had the values from before the collapse.
 *   la3dm_pack_info: the validation alone (no GPU, dm-free), *out = the header.
 *   A refusal returns LA3DM_ERR_ARG, leaves the map exactly as it was, and its text is la3dm_last_error(ctx) — for
 *   la3dm_pack_info, which has no context, la3dm_last_error(NULL). */
typedef struct la3dm_pack_header {
    char magic[8];
    uint32_t version, header_bytes, variant, block_depth, nodes_per_block, flags;
    uint64_t n_blocks, n_leaves, total_bytes;
    float init_A, init_B;
    float resolution, sf2, ell, free_thresh, occupied_thresh, var_thresh, prior_A, prior_B, noise, l, min_var, max_var,
        max_known_var, min_W;
    uint8_t reserved[8];
} la3dm_pack_header;
#define LA3DM_PACK_VERSION 1u
#define LA3DM_PACK_FLAG_LV_ORIGINAL_SIZE 0x1u
int la3dm_devmap_pack_host(la3dm_devmap *dm, void *buf, uint64_t cap, uint64_t *size);
int la3dm_devmap_unpack_host(la3dm_devmap *dm, const void *buf, uint64_t size);
int la3dm_pack_info(const void *buf, uint64_t size, la3dm_pack_header *out);
/* Merge: a map stream fused into a LIVE map on the GPU (csrc/devmap_merge.h; the rule per block on flat arrays, which the
 * host-mode map runs, is csrc/host/merge_block.h — both give the same bytes).  For maps of class BGKOctoMap (variant 0) and
 * BGKLOctoMap (variant 3), whose nodes are a pair of evidence sums over a shared prior.
 *
 *   The stream is validated and compared with the context exactly as la3dm_devmap_unpack_host does.  The map may hold any
 *   number of blocks.  For every block key k of the stream:
 *     - a block the map lacks is created, conceptually all-default (every node init_A, init_B, UNKNOWN, no prune);
 *     - for every finest-layer cell c, with (A2, B2, S2) the stream's covering leaf of c and (A1, B1, S1) the map's (S = the
 *       whole byte, bit 7 included), the cell becomes
 *         kept    (A1, B1, S1)            if A2, B2 are init_A, init_B bit for bit: the incoming leaf carries no evidence
 *         copied  (A2, B2, S2) verbatim   else if A1, B1 are init_A, init_B bit for bit
 *         fused   A = A1 + (A2 - init_A), B = B1 + (B2 - init_B) in fp32 in that association; state = Occupancy::update's
 *                 rule with IEEE divisions — var = (A B) / ((s s)(s + 1)), s = A + B; var > var_thresh: UNKNOWN; else
 *                 p = A / s > occupied_thresh: OCCUPIED, p < free_thresh: FREE, else UNKNOWN — with bit 7 set;
 *     - the block is pruned by OcTree::prune's rule, bottom up: eight siblings that are all leaves of one state other than
 *       UNKNOWN collapse into their parent, which takes child 0's A, B and WHOLE S byte (an untouched coarse leaf that is
 *       expanded and collapsed again comes back bit-identical; nothing depends on dead nodes' stale bytes);
 *     - the block is written in unpack's canonical form, every node once: leaves their values, nodes under a leaf
 *       (init_A, init_B, PRUNED), nodes above the leaves (init_A, init_B, UNKNOWN).
 *   Blocks the stream does not name are neither read nor written.  New blocks take pool slots n_blocks, n_blocks + 1, ... in
 *   STREAM ORDER; apart from those slot numbers the result does not depend on the order of the stream's blocks, so replicas
 *   that merge one stream stay identical and two packs of the result are byte-identical.  NaN payload bits of a fused
 *   sum are not part of the contract.
 *
 *   Refusals — LA3DM_ERR_ARG, the text through la3dm_last_error, the map exactly as it was: a stream the validator
 *   rejects; a mismatch with the context; a GPOctoMap or BGKLVOctoMap map (ivar clamping and UNCERTAIN make their fusion
 *   another rule); a poisoned map; a block_depth whose staging does not fit a compute unit's LDS (5: block_depth 1 to 4
 *   run); a pool that would pass 2^32 nodes.  All but the last come before the first allocation or launch; the last is
 *   known once the find launch has counted the blocks to create, before the pool is touched.
 *   Launch chain: one upload, dm_merge_find (table probe per stream block), the map's one-launch scan over the "new" flags,
 *   one read-back of the number created, grow_pool / grow_table, dm_merge_insert (keys of the new blocks), dm_merge_fuse (one
 *   wave per block: both trees climbed per finest cell, prune in LDS, every node written once), one read-back of the cell
 *   counters.  An empty stream (the header alone) is a no-op with zero stats.  Afterwards the host-side facts are as unpack
 *   leaves them; a following insert works on the merged pool. */
typedef struct la3dm_merge_stats {
    uint64_t n_blocks;   /* blocks of the stream */
    uint64_t n_created;
    uint64_t cells_kept, cells_copied, cells_fused;
} la3dm_merge_stats;
int la3dm_devmap_merge_host(la3dm_devmap *dm, const void *buf, uint64_t size, la3dm_merge_stats *stats /* may be NULL */);
/* Diff: the finest-layer cells whose class differs between the live map (NOW) and a map stream (THEN), on the GPU
 * (csrc/devmap_diff.h; the rule per block on flat arrays, which the host-mode map runs, is csrc/host/diff_block.h — both
 * give the same lists and counts).  merge's read-only sibling; all four map classes.
 *
 *   The stream is a pack / pack_region / evict of this or another map.  It is validated and compared with the context
 *   exactly as la3dm_devmap_unpack_host and merge do: variant, block_depth, nodes_per_block and, by bit pattern, resolution,
 *   init_A, init_B.  The map is never modified.
 *   COMPARED BLOCKS.  Every block the stream names, in STREAM ORDER.  With params->map_only != 0 also every block the map
 *     holds that the stream does not name, after the stream's, in the order pack would write them: ascending pool slot on
 *     the device pool, ascending key on a host-mode map.  No other block is read.
 *   PER FINEST-LAYER CELL c of a compared block (c = the finest-layer index as Block::get_node builds it, 0 .. 8^(block_depth
 *     - 1) - 1): then = the class of the stream's covering leaf of c, now = the class of the map's covering leaf of c.  The
 *     class is S & 7 of that leaf as box reports it — FREE 0, OCCUPIED 1, UNKNOWN 2, and 4 for an UNCERTAIN leaf of a BGK-LV
 *     map — and LA3DM_RAY_MISSING (3) on the side that has no such block (a covering leaf is never PRUNED, so 3 is
 *     unambiguous).  The cell is VALUE-CHANGED when then == now and A or B of the two covering leaves differ bit for bit.
 *   STATS (optional, always complete whatever cap is): n_stream_blocks; n_map_only_blocks (0 when map_only is 0);
 *     n_missing_now = the stream blocks the map lacks; pairs[5 * then + now] = the compared cells with that pair;
 *     value_changed[cls] = the value-changed cells of that class — counted, for all five classes, when params->value_mask
 *     is not 0; with value_mask 0 no A or B is read and the five counts are 0.
 *   SELECTION.  A cell is listed when bit 5 * then + now of params->pair_mask is set, or when it is value-changed and bit
 *     now of params->value_mask is set.  LA3DM_DIFF_PAIRS_CHANGED = the 20 off-diagonal pairs.  The list follows the block
 *     order above and, within a block, ascending c.  *n_found = the number selected, whatever cap is; the first
 *     min(*n_found, cap) entries are written, nothing past them.  cap = 0 with out NULL only counts (frontier's convention).
 *   OUTPUTS (la3dm_diff_out, every pointer optional, host memory): block_key; cell = c; code = then | now << 4; centre = the
 *     cell's centre as la3dm_devmap_export_cells / la3dm_map_dump_leaves compute a finest leaf's location: the LUT entry of
 *     node layer_base(block_depth - 1) + c plus axis_center of the key's field, in fp32, those two operands in that order;
 *     A, B = the NOW covering leaf's values, init_A, init_B where now is MISSING.
 *   An empty stream with map_only 0 is a no-op (*n_found = 0, zero stats, no launch); an empty map compares every stream
 *     block against MISSING.
 *   Refusals — LA3DM_ERR_ARG, the text through la3dm_last_error, NOTHING written (not *n_found, not stats, no buffer): a
 *     stream the validator rejects; a mismatch with the context; a poisoned map; params or n_found NULL; pair_mask bits
 *     above bit 24 or value_mask bits above bit 4; cap > 0 with out NULL; a block_depth whose four waves' staging — the
 *     mask words, their prefixes and the block's S bytes per wave — does not fit a compute unit's LDS (that is block_depth 6,
 *     which la3dm_devmap_create does not accept today: every depth a device map can have, 1 to 5, runs); more compared blocks than 2^32 - 2; more than 2^32 - 1 selected cells, which is known once they are counted.
 *   Launch chain: one upload of the stream, dm_merge_find (the pool slot per stream block); with map_only a scatter of
 *     marks, a select over the pool's slots, the map's one-launch scan and a list of the unmarked slots; dm_diff_count (one
 *     wave per compared block: both trees climbed per finest cell, 64 cells at a time, the counters from ballots), the scan
 *     over the blocks' counts, ONE read-back of the counters and *n_found; with cap > 0 dm_diff_emit and ONE copy of the
 *     list.  No download of the pool, no host pass over cells; the host mirror is neither refreshed nor marked stale.
 *     Measured on a 44 k-block map: 2.2 ms to count, 2.3 ms with the list of 91 k changed cells, of which
 *     the launches are 0.1 ms and the host-side validation and upload of the stream the rest; pack() alone takes 0.8 ms,
 *     pack() plus a host pass over both streams 28 ms. */
#define LA3DM_DIFF_PAIRS_CHANGED 0x0FBEFBEu
typedef struct la3dm_diff_params {
    uint32_t pair_mask;    /* bit 5 * then + now */
    uint32_t value_mask;   /* bit now */
    uint32_t map_only;     /* != 0: the map's blocks the stream does not name are compared too (then = MISSING) */
} la3dm_diff_params;
typedef struct la3dm_diff_out {
    int64_t *block_key;   /* [cap] or NULL */
    uint32_t *cell;       /* [cap] or NULL */
    uint8_t *code;        /* [cap] or NULL */
    float *centre;        /* [3 cap] or NULL */
    float *A, *B;         /* [cap] or NULL */
} la3dm_diff_out;
typedef struct la3dm_diff_stats {
    uint64_t n_stream_blocks, n_map_only_blocks, n_missing_now;
    uint64_t pairs[25];
    uint64_t value_changed[5];
} la3dm_diff_stats;
int la3dm_devmap_diff_host(la3dm_devmap *dm, const void *buf, uint64_t size, const la3dm_diff_params *params, uint64_t cap,
                           const la3dm_diff_out *out /* may be NULL with cap 0 */, uint64_t *n_found,
                           la3dm_diff_stats *stats /* may be NULL */);
/* The map as a rolling window: the stream of SOME blocks, and blocks leaving the map (csrc/devmap_evict.h; the region test,
 * shared with the host-mode map: csrc/host/region_blocks.h).  All four map classes, every block_depth pack accepts.
 *
 *   THE REGION is a closed box of blocks in integer block-key coordinates, klo[a] <= k[a] <= khi[a] on the axes a = x, y, z,
 *   where k[a] is the 20-bit field of the block's hash key on that axis (x: bits 59..40, y: 39..20, z: 19..0 — the numbers
 *   la3dm_devmap_key_bounds reports; the block that holds a world point has the fields of block_to_hash_key of that point).
 *   inside = 1 selects the blocks in the box, inside = 0 every OTHER block (erase all but the box round the robot).
 *   klo[a] > khi[a] on any axis, a null bound and an inside other than 0 or 1 are refused (LA3DM_ERR_ARG, the text through
 *   la3dm_last_error, the map exactly as it was); so is a poisoned map.  Bounds outside 0 .. 2^20 - 1 are no error.
 *
 *   PACK_REGION writes the version-1 stream of la3dm_devmap_pack_host, unchanged in format, that holds the selected blocks
 *   only: la3dm_pack_info, unpack and merge accept it.  The blocks come in ascending pool slot (pack's rule), and each
 *   block's mask words and leaf bytes are bit for bit what la3dm_devmap_pack_host writes for that block.  The map is not
 *   changed.  buf = NULL only sizes (*size); cap < *size is LA3DM_ERR_ARG with *size set; no block selected gives the header
 *   alone (128 bytes).
 *
 *   ERASE_REGION removes the selected blocks: their voxels read as missing through every query, the block count drops, a
 *   later insert or merge may create blocks there again.  THE POOL AFTERWARDS, with n_old blocks before and n_removed
 *   selected: n_new = n_old - n_removed.  A surviving block in a slot < n_new keeps its slot.  Let the holes be the removed
 *   slots < n_new in ascending order, h_0 < h_1 < ..., and the tail survivors the surviving slots >= n_new in ascending order,
 *   t_0 < t_1 < ... — there are equally many; the block in t_i moves to h_i, every node of it (A, B and the state byte, dead
 *   nodes included) and its key.  That is the fewest blocks that can move; sources and destinations are disjoint, so the move
 *   runs in place; it is deterministic, so replicas that erase one region stay identical.  Blocks that do not move are neither
 *   read nor written, apart from their keys.  The block table is rebuilt for the n_new blocks.  Slots >= n_new are dead: their
 *   bytes are not part of the map, and whoever creates a block later writes every node of it.  Nothing selected is a no-op;
 *   everything selected leaves an empty map that behaves like a new one.  The last scan's training data, the options, the
 *   shard settings, the pool's allocation and the table's capacity are untouched.  stats (may be NULL): blocks removed, blocks
 *   moved (the number of holes), and the block count after the call; all zero after a refusal.
 *   Launch chains.  Both: dm_evict_select (one lane per block), the map's one-launch scan over n_blocks + 1 flags, one
 *   read-back of the number selected.  pack_region: dm_evict_list (slot list + keys), then pack's chain over the list
 *   (dm_pack_count, the scan, one read-back of n_leaves, dm_pack_emit, one copy).  erase_region: dm_evict_plan (holes and tail
 *   survivors from the same scan), dm_evict_move (one wave per pair), the table cleared, dm_table_rebuild, one copy of the
 *   number moved. */
typedef struct la3dm_erase_stats {
    uint64_t n_removed;
    uint64_t n_moved;
    uint64_t n_blocks;   /* after the call */
} la3dm_erase_stats;
int la3dm_devmap_pack_region_host(la3dm_devmap *dm, const int32_t klo[3], const int32_t khi[3], int inside, void *buf, uint64_t cap,
                                  uint64_t *size);
int la3dm_devmap_erase_region_host(la3dm_devmap *dm, const int32_t klo[3], const int32_t khi[3], int inside,
                                   la3dm_erase_stats *stats /* may be NULL */);
/* BGKOctoMap::search(x, y, z) (include/bgkoctomap/bgkoctomap.h:315-319) for n query points (host pointers, packed xyz),
 * answered from the device pool without refreshing a host mirror: exists[i] = the block exists; A/B/state = the
 * finest-layer node that holds the point (a default node when the block is missing). */
int la3dm_devmap_search_host(la3dm_devmap *dm, const float *xyz, uint32_t n, uint8_t *exists, float *A, float *B,
                             uint8_t *state);
/* Batched ray casting on the device pool: the client loop over BGKOctoMap::RayCaster (include/bgkoctomap/bgkoctomap.h:91-214)
 * for n segments at once, one ray per GPU lane.  rays6: start xyz, end xyz per ray.  Per ray
 *     steps = 0; counts = {0}; flags = 0
 *     RayCaster rc(map, start, end)           -- the unchanged voxel walk; starts only inside an existing block
 *     while (!rc.end()) {
 *         if (steps == max_steps) { flags |= LA3DM_RAY_TRUNCATED; break; }
 *         valid = rc.next(p, node, block_key, node_key); ++steps
 *         cls = valid ? state of the COVERING LEAF of node_key in that block : LA3DM_RAY_MISSING
 *         ++counts[cls]; last = this row
 *         if (stop_mask & (1u << cls)) { flags |= LA3DM_RAY_HIT; break; }
 *     }
 * Covering leaf: climb from the finest-layer node while its state is PRUNED (prune() leaves the eight children of a
 * collapsed group PRUNED; the answer lives in an ancestor).  leaf_depth = the layer where the climb ends (block_depth - 1
 * when nothing was pruned); A, B are that node's.  cls: FREE 0, OCCUPIED 1, UNKNOWN 2, LA3DM_RAY_MISSING 3 (the block does
 * not exist: A, B = the map's default node, leaf_depth 255); a BGK-LV map's UNCERTAIN leaves report 4 and are counted with
 * UNKNOWN in counts[2].  A ray that never starts (its start block does not exist, or the map is empty) has steps = 0,
 * flags = 0, cls = LA3DM_RAY_MISSING, leaf_depth 255, default A / B, everything else 0.  A ray with a non-finite
 * coordinate or |coordinate / resolution| >= 2^30 is refused on its own: flags = LA3DM_RAY_INVALID, the other outputs as
 * for a ray that never starts.  stop_mask 0 walks to the end and only counts.  max_steps: 1 ... LA3DM_RAY_MAX_STEPS.
 * Every pointer of `out` except steps and flags may be NULL.  The result is bit-identical to the host loop. */
#define LA3DM_RAY_HIT 1u
#define LA3DM_RAY_TRUNCATED 2u
#define LA3DM_RAY_INVALID 4u
#define LA3DM_RAY_MISSING 3u
#define LA3DM_RAY_MAX_STEPS (1u << 20)
typedef struct la3dm_raycast_out {
    uint32_t *steps;     /* [n] rows produced */
    uint8_t *flags;      /* [n] LA3DM_RAY_* */
    float *p;            /* [3n] last row: voxel centre (dead-reckoned position inside a missing block) */
    int64_t *block_key;  /* [n] */
    int32_t *node_key;   /* [n] finest-layer key of the last row, as next() reports it */
    uint8_t *cls;        /* [n] */
    uint8_t *leaf_depth; /* [n] */
    float *A, *B;        /* [n] */
    uint32_t *counts;    /* [4n] rows per class: FREE, OCCUPIED, UNKNOWN, MISSING */
} la3dm_raycast_out;
/* host pointers: upload, one launch, download, synchronise — on the map's stream */
int la3dm_devmap_raycast_host(la3dm_devmap *dm, const float *rays6, uint32_t n, uint32_t stop_mask, uint32_t max_steps,
                              const la3dm_raycast_out *out);
/* device pointers (rays and outputs already in HBM on the map's device); returns when the results are complete */
int la3dm_devmap_raycast_device(la3dm_devmap *dm, const float *d_rays6, uint32_t n, uint32_t stop_mask, uint32_t max_steps,
                                const la3dm_raycast_out *d_out);
/* Dense region reads on the device pool: an axis-aligned box of voxels as arrays (box), and the same box reduced along
 * z per (x, y) column (columns).  The region: lo[3] (a world point) and dims[3] = (nx, ny, nz), each >= 1.
 *   Anchor.  Voxel (0, 0, 0) is the voxel that holds lo the way the RayCaster resolves its start point: per axis the block
 *     field b = (int64)(lo / block_size + 524288.5) in double (block_to_hash_key) and the cell
 *     c = clamp((int)((lo - (b - 524288) * block_size) / resolution + lim / 2), 0, lim - 1) in float (Block::get_index,
 *     truncation), lim = 2^(block_depth - 1).  These are the only floating-point operations of the query.
 *   Lattice.  With the global index g0 = b * lim + c per axis, voxel (i, j, k) has the global index g = g0 + (i, j, k):
 *     block field g / lim, cell g % lim, block key (bx << 40) | (by << 20) | bz, finest-layer node as Block::get_node
 *     builds it (child bit 4 = +x, 2 = +y, 1 = +z per level).  Integers only.  The region need not be aligned to blocks.
 *   Refused as a whole (LA3DM_ERR_ARG, a text that names the argument, nothing written): a non-finite lo or
 *     |lo / resolution| >= 2^30, a zero dimension, a region whose block fields leave [0, 2^20), more than
 *     LA3DM_BOX_MAX_CELLS voxels (box), more than 2^30 columns or nz > LA3DM_COLUMNS_MAX_NZ (columns), a NULL lo, dims,
 *     out or mandatory output.  The limits are checked before any buffer is touched.
 *   info (optional, host memory in both forms): the anchor's block key and cell, and origin = the centre of voxel
 *     (0, 0, 0) as Block::get_point gives it (LUT entry + block centre, whether or not the block exists).  The centre of
 *     voxel (i, j, k) is origin + (i, j, k) * resolution up to fp32 rounding.
 * box: voxel (i, j, k) at index (i * ny + j) * nz + k (C order of shape (nx, ny, nz)).  cls (mandatory) = state of the
 *   COVERING LEAF as in raycast_many: FREE 0, OCCUPIED 1, UNKNOWN 2, LA3DM_RAY_MISSING 3 where the block does not exist,
 *   4 for an UNCERTAIN leaf of a BGK-LV map; leaf_depth = its layer, 255 for a missing block; A, B = its node values
 *   (m_ivar / ivar on a GP map), the map's default node for a missing block.  An empty map answers all-MISSING without a
 *   launch.
 * columns: column (i, j) at index i * ny + j, over k = 0 ... nz - 1 of the same lattice.  counts (mandatory, 4 per
 *   column): voxels of class FREE, OCCUPIED, UNKNOWN (+ UNCERTAIN), MISSING — they sum to nz; low_occ / top_occ: smallest /
 *   largest k whose class is OCCUPIED, -1 when there is none.  columns(lo, dims) is the reduction of box(lo, dims).cls
 *   along its last axis; it reads the pool itself and allocates nothing that grows with nx * ny * nz.
 * The results are bit-identical to the host form (BGKOctoMap::box / columns on a host-mode map). */
#define LA3DM_BOX_MAX_CELLS (1u << 30)
#define LA3DM_COLUMNS_MAX_NZ (1u << 16)
typedef struct la3dm_region_info {
    int64_t block_key;   /* block of voxel (0, 0, 0) */
    int32_t cell[3];     /* its cell inside that block */
    float origin[3];     /* its centre */
} la3dm_region_info;
typedef struct la3dm_box_out {
    uint8_t *cls;        /* [nx ny nz] */
    uint8_t *leaf_depth; /* [nx ny nz] or NULL */
    float *A, *B;        /* [nx ny nz] or NULL */
} la3dm_box_out;
typedef struct la3dm_columns_out {
    uint32_t *counts;    /* [4 nx ny] FREE, OCCUPIED, UNKNOWN, MISSING */
    int32_t *low_occ;    /* [nx ny] or NULL */
    int32_t *top_occ;    /* [nx ny] or NULL */
} la3dm_columns_out;
/* host pointers: one launch, download, synchronise — on the map's stream */
int la3dm_devmap_box_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_box_out *out,
                          la3dm_region_info *info);
int la3dm_devmap_columns_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_columns_out *out,
                              la3dm_region_info *info);
/* device pointers (outputs already in HBM on the map's device; lo3, dims3 and info stay host-side); return when the
 * results are complete */
int la3dm_devmap_box_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_box_out *d_out,
                            la3dm_region_info *info);
int la3dm_devmap_columns_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_columns_out *d_out,
                                la3dm_region_info *info);
/* Distance field of a region: the exact Euclidean distance transform of box(lo, dims).  The region (anchor, lattice,
 * info, index (i * ny + j) * nz + k) is box's.
 *   Obstacles.  Voxel (i, j, k) is an obstacle when obstacle_mask & (1u << cls) is set, cls being what box reports for
 *     it (FREE 0, OCCUPIED 1, UNKNOWN 2, MISSING 3, a BGK-LV map's UNCERTAIN 4): the bit convention of raycast_many's
 *     stop_mask.
 *   Definition.  D(v) = the minimum over the obstacles o INSIDE THE REGION of |v - o|^2, an integer in voxel units.
 *     d2[v] = D(v) if D(v) <= radius^2, else LA3DM_DF_FAR (a region without obstacles: FAR everywhere).
 *     dist[v] = sqrtf((float)d2[v]) * resolution — one correctly rounded fp32 square root, one fp32 multiply — and +inf
 *     for FAR.  Every finite d2 is below 2^24, hence exact in fp32.
 *   Obstacles outside the region are not seen: a caller who needs the distances of a region to be true up to `radius`
 *     pads the region by `radius` voxels on every side.  The distance INSIDE obstacles (to the nearest voxel that is
 *     none) is the same call with the complementary mask (0x1F & ~obstacle_mask); there is no signed form.
 *   Refused as a whole (LA3DM_ERR_ARG, a text that names the argument, no buffer touched, no scratch reserved): what box
 *     refuses for lo and dims; an obstacle_mask of 0 or with bits above 0x1F; a radius of 0 or above
 *     LA3DM_DF_MAX_RADIUS; more than LA3DM_DF_MAX_CELLS voxels; a NULL out or an out with both arrays NULL.
 *   An empty map (every voxel MISSING) answers all 0 if the mask holds bit 3 and all FAR / +inf otherwise, without a launch.
 *   Working storage: 4 bytes per voxel in a grow-only arena of the devmap (released with it), next to the outputs.
 * The results are bit-identical to the host form (BGKOctoMap::distance_field on a host-mode map). */
#define LA3DM_DF_FAR        0xFFFFFFFFu
#define LA3DM_DF_MAX_RADIUS 1024u
#define LA3DM_DF_MAX_CELLS  (1u << 28)
typedef struct la3dm_distance_out {
    uint32_t *d2;   /* [nx ny nz] or NULL */
    float *dist;    /* [nx ny nz] or NULL; at least one of the two */
} la3dm_distance_out;
/* host pointers: the launches, download, synchronise — on the map's stream */
int la3dm_devmap_distance_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask,
                               uint32_t radius, const la3dm_distance_out *out, la3dm_region_info *info);
/* device pointers (outputs already in HBM on the map's device, 4-byte aligned; lo3, dims3 and info stay host-side);
 * returns when the results are complete.  An output array doubles as working storage until the last pass fills it. */
int la3dm_devmap_distance_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask,
                                 uint32_t radius, const la3dm_distance_out *d_out, la3dm_region_info *info);
/* Frontier of a region: the voxels of box(lo, dims) that are open and border unexplored space, as an ordered list.
 *   Region and lattice.  The region, anchor, lattice, info and flat index f = (i * ny + j) * nz + k are box's.
 *   Classes.  cls(v) is what box reports for voxel v, the class of the covering leaf: FREE 0, OCCUPIED 1, UNKNOWN 2,
 *     MISSING 3, a BGK-LV map's UNCERTAIN 4.
 *   Reading past the faces.  The lattice does not stop at the region's faces: cls of a voxel one step outside the region
 *     is read from the map exactly as box would read it at that lattice position.  In this the query differs from
 *     distance_field: a frontier voxel on a face of the region is still found, and the answers of two boxes that tile a
 *     third merge into the third's.
 *   Neighbourhood.  The neighbours of v are v + (di, dj, dk), (di, dj, dk) in {-1, 0, 1}^3 without 0, chosen by
 *     connectivity: 6 = the offsets with |di| + |dj| + |dk| = 1, 18 = those with a sum <= 2, 26 = all of them.
 *   Score.  c(v) = the number of neighbours w of v with unknown_mask & (1u << cls(w)) set;
 *     score[v] = c(v) if open_mask & (1u << cls(v)) is set, else 0.
 *   Frontier.  v is a frontier voxel when score[v] >= min_neighbours.  *n_found = the number of frontier voxels of the
 *     region, whatever cap is; index[t], t < min(*n_found, cap), = the flat index of the t-th frontier voxel in ascending
 *     order of f; nbrs[t] = score[index[t]].  Entries at t >= *n_found are not written.  score (dense, optional) does not
 *     depend on cap.
 *   Count-only call.  cap = 0 with out NULL (or with only out->score set) returns *n_found (and score): the two-call
 *     protocol of la3dm_devmap_export_cells.
 *   Refused as a whole (LA3DM_ERR_ARG, a text that names the argument, no buffer touched, nothing reserved): an
 *     open_mask or unknown_mask of 0 or with bits above 0x1F (overlapping masks are legal); a connectivity other than 6,
 *     18, 26; min_neighbours of 0 or above connectivity; what box refuses for lo and dims; (nx + 2)(ny + 2)(nz + 2) >
 *     LA3DM_FR_MAX_CELLS; a region that, padded by one voxel on every side, fails box's block-field range check; cap > 0
 *     with out or out->index NULL; n_found NULL.  The limits are checked before any buffer is looked at.
 *   An empty map (every voxel and its surroundings MISSING) answers from the definition without reading the pool: every
 *     voxel with score = connectivity if both masks hold bit 3, no voxel otherwise.
 *   Everything is integer arithmetic on classes: the results equal the host form (BGKOctoMap::frontier on a host-mode
 *     map) exactly.
 *   Working storage: two bit streams, one popcount and one prefix per 32 voxels of the padded box — 1/2 byte per padded
 *     voxel — in a grow-only arena of the devmap (released with it; a smaller request after a larger one allocates
 *     nothing).  No per-voxel byte is kept: a dense score is written only where the caller asks for it. */
#define LA3DM_FR_MAX_CELLS (1u << 28)
typedef struct la3dm_frontier_out {
    uint32_t *index;   /* [cap] or NULL */
    uint8_t  *nbrs;    /* [cap] or NULL */
    uint8_t  *score;   /* [nx ny nz] or NULL, independent of cap */
} la3dm_frontier_out;
/* host pointers: the launches, download of min(*n_found, cap) entries, synchronise — on the map's stream */
int la3dm_devmap_frontier_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, uint32_t open_mask,
                               uint32_t unknown_mask, uint32_t connectivity, uint32_t min_neighbours, uint64_t cap,
                               const la3dm_frontier_out *out, uint64_t *n_found, la3dm_region_info *info);
/* device pointers (out's arrays already in HBM on the map's device, index 4-byte aligned; lo3, dims3, n_found and info
 * stay host-side); returns when the results are complete */
int la3dm_devmap_frontier_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, uint32_t open_mask,
                                 uint32_t unknown_mask, uint32_t connectivity, uint32_t min_neighbours, uint64_t cap,
                                 const la3dm_frontier_out *d_out, uint64_t *n_found, la3dm_region_info *info);
/* Gain of candidate viewpoints: per viewpoint the number of DISTINCT voxels of a region that a fan of rays from it walks
 * over and whose class is in count_mask — the expected information gain of a next-best-view planner when count_mask
 * selects the unobserved classes.  (Summing raycast_many's counts over the rays of a viewpoint counts a voxel once per
 * ray that crosses it; the rays of a fan overlap near their origin.)
 *   Region and lattice.  The region, anchor, lattice, info and flat index f = (i * ny + j) * nz + k are box's.
 *   Rays.  n viewpoints origins3 (packed xyz) and m directions offsets3 (packed xyz, metres in the map frame, shared by
 *     all viewpoints: the caller's sensor pattern) give n * m segments: start = origins[v], end[c] = origins[v][c] +
 *     offsets[d][c], one fp32 add per coordinate — the only floating-point operation the query adds to raycast_many's.
 *   Walk.  Every segment is walked exactly as raycast_many(start, end, stop_mask, max_steps) walks it: the same validity
 *     test on the six coordinates (an invalid ray contributes nothing), the same never-starts rule, the same rows, the
 *     same stopping row and the same truncation.
 *   Marking.  Every row produced is a candidate, the stopping row included.  Its lattice position is, per axis, the
 *     20-bit field of its block key times lim plus the cell of its node key, as RayCaster::next reports them (rows in
 *     missing blocks included).  If that position lies in the region and count_mask & (1u << cls) is set — cls the class
 *     of the row: FREE 0, OCCUPIED 1, UNKNOWN 2, MISSING 3, a BGK-LV map's UNCERTAIN 4; what box reports there — bit f
 *     of the viewpoint's set is set.
 *   Outputs.  gain[v] = the popcount of viewpoint v's set.  seen[v * W + f / 32] bit f % 32 = the set itself, W =
 *     ceil(nx ny nz / 32); the bits at f >= nx ny nz are 0.  started[v] / hits[v] = the rays of the viewpoint with
 *     steps > 0 / that ended on a stop row (LA3DM_RAY_HIT).
 *   Refused as a whole (LA3DM_ERR_ARG, a text that names the argument, no buffer touched, nothing reserved), in this
 *     order: a count_mask of 0 or with bits above 0x1F; a stop_mask with bits above 0x1F (0 is legal: every ray walks to
 *     its end); max_steps outside 1 ... LA3DM_RAY_MAX_STEPS; m = 0; n * m > LA3DM_GAIN_MAX_RAYS; what box refuses for
 *     lo and dims; more than LA3DM_GAIN_MAX_CELLS voxels; n * W > LA3DM_GAIN_MAX_WORDS; with n > 0 a NULL origins3,
 *     offsets3, out or out->gain.
 *   n = 0 is served and writes nothing.  An empty map (no ray starts) answers all-zero without a launch.
 *   Working storage: the sets, n * W words, in a grow-only arena of the devmap (released with it; a smaller request
 *     after a larger one allocates nothing).  When out->seen is given to the device-pointer form it is the working
 *     storage and the arena is not used.
 *   Everything after the walk is integer arithmetic: the results equal the host form (BGKOctoMap::gain on a host-mode
 *     map) exactly. */
#define LA3DM_GAIN_MAX_CELLS (1u << 28)
#define LA3DM_GAIN_MAX_RAYS  (1u << 28)
#define LA3DM_GAIN_MAX_WORDS (1u << 28)
typedef struct la3dm_gain_out {
    uint32_t *gain;     /* [n]   mandatory: distinct marked voxels per viewpoint */
    uint32_t *started;  /* [n]   or NULL: rays of the viewpoint with steps > 0 */
    uint32_t *hits;     /* [n]   or NULL: rays that ended on a stop row (LA3DM_RAY_HIT) */
    uint32_t *seen;     /* [n W] or NULL: the sets themselves, W = ceil(nx ny nz / 32) */
} la3dm_gain_out;
/* host pointers: upload of the origins and offsets, the launches, download, synchronise — on the map's stream */
int la3dm_devmap_gain_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *origins3, uint32_t n,
                           const float *offsets3, uint32_t m, uint32_t count_mask, uint32_t stop_mask, uint32_t max_steps,
                           const la3dm_gain_out *out, la3dm_region_info *info);
/* device pointers (origins3, offsets3 and out's arrays already in HBM on the map's device, 4-byte aligned; lo3, dims3 and
 * info stay host-side); returns when the results are complete */
int la3dm_devmap_gain_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *d_origins3, uint32_t n,
                             const float *d_offsets3, uint32_t m, uint32_t count_mask, uint32_t stop_mask, uint32_t max_steps,
                             const la3dm_gain_out *d_out, la3dm_region_info *info);
/* Score poses: likelihood-field scoring of one scan under many candidate poses — which pose fits the map best.  Every
 * point of the cloud is moved by every pose, its voxel resolved as search resolves it, and the squared distance from
 * that voxel to the nearest obstacle gathered from distance_field's answer; per pose the distances are summed and the
 * pairs counted by class.
 *   Region and lattice.  The region, anchor, lattice, info and flat index f = (i * ny + j) * nz + k are box's.
 *   Cost volume.  d2 = distance_field(lo, dims, obstacle_mask, radius) over the same region, unchanged, with its blind
 *     spot: obstacles outside the region are not seen.  radius lies in 1 ... LA3DM_SCORE_MAX_RADIUS (255), so every
 *     finite d2 is <= 65 025 and fits 16 bits.
 *   Inputs.  points3: n_points packed xyz in the sensor frame.  poses12: n_poses x 12 floats, row-major 3 x 4 [R | t].
 *     Nothing checks that R is a rotation.
 *   Transform.  Per axis c, w[c] = ((R[c][0] * x + R[c][1] * y) + R[c][2] * z) + t[c]: three fp32 products and three fp32
 *     sums, each rounded on its own, in this order — the only floating-point work of the query besides the anchor's.
 *   Classes of a (pose, point) pair, tested in this order:
 *     LA3DM_SCORE_INVALID  some axis fails fabsf(w / resolution) < 2^30, the region's test for lo (false for NaN and inf,
 *                          whether they come from the point or from the pose);
 *     LA3DM_SCORE_OUTSIDE  per axis the global index is built with the anchor's own arithmetic,
 *                            b = (int64)((double)w / (double)block_size + 524288.5),
 *                            center = (float)(b - 524288) * block_size,
 *                            cell = clamp((int)((w - center) / resolution + (float)(lim / 2)), 0, lim - 1),
 *                            g = b * lim + cell,
 *                          the voxel search resolves for w; the pair is OUTSIDE when some b is outside [0, 2^20) or some
 *                          g - g0 is outside [0, n) of its axis;
 *     otherwise, f the flat index of (g - g0): LA3DM_SCORE_HIT if d2[f] == 0, LA3DM_SCORE_NEAR if d2[f] is finite,
 *                          LA3DM_SCORE_FAR if d2[f] == LA3DM_DF_FAR.
 *   Outputs per pose p.  sum_d2[p] (mandatory) = the sum of d2[f] over the pose's HIT and NEAR pairs; counts[5 p + c]
 *     (optional) = its pairs of class c, in the order HIT, NEAR, FAR, OUTSIDE, INVALID: they sum to n_points.  The caller
 *     composes a score, e.g. sum_d2 + penalty * (far + outside).
 *   Refused as a whole (LA3DM_ERR_ARG, a text that names the argument, no buffer touched, nothing reserved), in this
 *     order: an obstacle_mask of 0 or with bits above 0x1F; a radius outside 1 ... LA3DM_SCORE_MAX_RADIUS; n_points >
 *     LA3DM_SCORE_MAX_POINTS; n_poses > LA3DM_SCORE_MAX_POSES; n_points * n_poses > LA3DM_SCORE_MAX_PAIRS; what box
 *     refuses for lo and dims; more than LA3DM_SCORE_MAX_CELLS voxels; with n_poses > 0 a NULL poses12, out or
 *     out->sum_d2 and, with n_points > 0 as well, a NULL points3.
 *   n_poses = 0 is served and writes nothing; n_points = 0 writes zeros.  An empty map answers from the definition without
 *     a launch that reads the pool: every voxel is MISSING, so d2 is 0 everywhere if the mask holds bit 3 and FAR
 *     everywhere otherwise; the classes of the pairs still depend on the transform.
 *   Working storage: distance_field's 4 bytes per voxel and as many again for d2, in grow-only arenas of the devmap
 *     (released with it; a smaller request after a larger one allocates nothing).
 *   All sums are integers: the results equal the host form (BGKOctoMap::score_poses on a host-mode map) exactly. */
#define LA3DM_SCORE_MAX_RADIUS 255u
#define LA3DM_SCORE_MAX_POINTS (1u << 20)
#define LA3DM_SCORE_MAX_POSES  (1u << 20)
#define LA3DM_SCORE_MAX_PAIRS  (1ull << 32)
#define LA3DM_SCORE_MAX_CELLS  (1u << 28)
#define LA3DM_SCORE_HIT     0u
#define LA3DM_SCORE_NEAR    1u
#define LA3DM_SCORE_FAR     2u
#define LA3DM_SCORE_OUTSIDE 3u
#define LA3DM_SCORE_INVALID 4u
typedef struct la3dm_score_out {
    uint64_t *sum_d2;   /* [n_poses]   mandatory: sum of d2 over the pose's HIT and NEAR pairs */
    uint32_t *counts;   /* [5 n_poses] or NULL: pairs of class HIT, NEAR, FAR, OUTSIDE, INVALID */
} la3dm_score_out;
/* host pointers: upload of the points and poses, the launches, download, synchronise — on the map's stream */
int la3dm_devmap_score_poses_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *points3,
                                  uint32_t n_points, const float *poses12, uint32_t n_poses, uint32_t obstacle_mask,
                                  uint32_t radius, const la3dm_score_out *out, la3dm_region_info *info);
/* device pointers (points3, poses12 and out's arrays already in HBM on the map's device, 4-byte aligned — sum_d2 too;
 * lo3, dims3 and info stay host-side); returns when the results are complete */
int la3dm_devmap_score_poses_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *d_points3,
                                    uint32_t n_points, const float *d_poses12, uint32_t n_poses, uint32_t obstacle_mask,
                                    uint32_t radius, const la3dm_score_out *d_out, la3dm_region_info *info);
/* Nearest: WHICH obstacle voxel is the nearest — the feature transform of a region, dense (nearest) and per point of a
 * cloud (nearest_points: the correspondences of an ICP step; v - nearest(v) is the direction away from the obstacle).
 *   Region and lattice.  The region, anchor, lattice, info and flat index f = (i * ny + j) * nz + k are box's.
 *   Obstacles are distance_field's: voxel v is an obstacle when obstacle_mask & (1u << cls(v)) is set, bits 0 to 4.
 *   Definition.  D(v) = the minimum over the obstacles o INSIDE THE REGION of |v - o|^2, distance_field's D with its blind
 *     spot: obstacles outside the region are not seen; pad the region by `radius` where that matters.
 *   nearest, per voxel v.  index[v] = the SMALLEST FLAT INDEX among the obstacles at squared distance D(v) when D(v) <=
 *     radius^2, else LA3DM_NEAREST_NONE; an obstacle voxel answers its own index.  The smallest flat index is the
 *     lexicographically smallest (i', j', k'): one reproducible answer on the medial axis, and a tie-break that is
 *     separable (smaller k' in the z stage, smaller j' in the y pass, smaller i' in the x pass).  d2[v] is exactly what
 *     distance_field(lo, dims, obstacle_mask, radius) holds in d2, LA3DM_DF_FAR included.  Either array may be NULL, not
 *     both.
 *   nearest_points, per point q of points3 (n_points packed xyz).  With pose12 (one row-major 3 x 4 [R | t]) w =
 *     score_poses' transform of q, per axis c ((R[c][0] * x + R[c][1] * y) + R[c][2] * z) + t[c] in fp32, every operation
 *     rounded on its own; with pose12 == NULL w is the point's three floats verbatim, no arithmetic.  The class of the
 *     point is score_poses' class of the pair, by the same tests in the same order: LA3DM_SCORE_INVALID, LA3DM_SCORE_OUTSIDE,
 *     then HIT / NEAR / FAR from d2 at the voxel search resolves for w.  Outputs, each [n_points], each optional, at least
 *     one: cls (the class), voxel (the flat index of the point's voxel; NONE for OUTSIDE and INVALID), index (nearest's
 *     index[voxel]; NONE for FAR, OUTSIDE and INVALID), d2 (nearest's d2[voxel]; LA3DM_DF_FAR for FAR, OUTSIDE and INVALID).
 *   radius lies in 1 ... LA3DM_NEAREST_MAX_RADIUS (255, as for score_poses): every partial sum of the transform stays
 *     below 2^18 and an axis offset fits 9 bits.
 *   Refused as a whole (LA3DM_ERR_ARG, a text that names the argument, no buffer touched, nothing reserved), in this
 *     order: an obstacle_mask of 0 or with bits above 0x1F; a radius outside 1 ... LA3DM_NEAREST_MAX_RADIUS; n_points >
 *     LA3DM_SCORE_MAX_POINTS (nearest_points); what box refuses for lo and dims; more than LA3DM_DF_MAX_CELLS voxels; then
 *     the buffers — nearest: a NULL out, an out with both arrays NULL; nearest_points with n_points > 0: a NULL points3, a
 *     NULL out, an out with all four arrays NULL.
 *   nearest_points with n_points = 0 is served and writes nothing.  An empty map answers from the definition without a
 *     launch that reads the pool: every voxel is MISSING, so with mask bit 3 index[v] = v and d2 = 0, otherwise NONE and FAR.
 *   Working storage: per voxel 4 bytes of y-pass keys, 2 bytes of z offsets and one obstacle bit, for nearest_points also
 *     index and d2 (8 bytes), in a grow-only arena of the devmap (released with it; a smaller request after a larger one
 *     allocates nothing).
 *   Everything is integers after the transform: the results equal the host form (BGKOctoMap::nearest and ::nearest_points
 *   on a host-mode map) exactly. */
#define LA3DM_NEAREST_NONE       0xFFFFFFFFu
#define LA3DM_NEAREST_MAX_RADIUS 255u
typedef struct la3dm_nearest_out {
    uint32_t *index;   /* [nx ny nz] or NULL: flat index of the nearest obstacle, LA3DM_NEAREST_NONE beyond the radius */
    uint32_t *d2;      /* [nx ny nz] or NULL: distance_field's d2; at least one of the two */
} la3dm_nearest_out;
typedef struct la3dm_nearest_points_out {   /* each [n_points] or NULL; at least one */
    uint8_t *cls;      /* LA3DM_SCORE_HIT ... LA3DM_SCORE_INVALID */
    uint32_t *voxel;   /* flat index of the point's voxel; LA3DM_NEAREST_NONE for OUTSIDE and INVALID */
    uint32_t *index;   /* index[voxel]; LA3DM_NEAREST_NONE for FAR, OUTSIDE and INVALID */
    uint32_t *d2;      /* d2[voxel]; LA3DM_DF_FAR for FAR, OUTSIDE and INVALID */
} la3dm_nearest_points_out;
/* host pointers: upload of the points and the pose, the launches, download, synchronise — on the map's stream */
int la3dm_devmap_nearest_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask,
                              uint32_t radius, const la3dm_nearest_out *out, la3dm_region_info *info);
int la3dm_devmap_nearest_points_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *points3,
                                     uint32_t n_points, const float *pose12, uint32_t obstacle_mask, uint32_t radius,
                                     const la3dm_nearest_points_out *out, la3dm_region_info *info);
/* device pointers (points3, pose12 and out's arrays already in HBM on the map's device; the 32-bit arrays 4-byte aligned;
 * lo3, dims3 and info stay host-side); return when the results are complete */
int la3dm_devmap_nearest_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask,
                                uint32_t radius, const la3dm_nearest_out *d_out, la3dm_region_info *info);
int la3dm_devmap_nearest_points_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *d_points3,
                                       uint32_t n_points, const float *d_pose12, uint32_t obstacle_mask, uint32_t radius,
                                       const la3dm_nearest_points_out *d_out, la3dm_region_info *info);
/* Reach: the hop distance from seed voxels through the passable voxels of a region — can a goal be got to, and in how
 * many moves.  A breadth-first wave, one launch per level.
 *   Region and lattice.  The region, anchor, lattice, info and flat index f = (i * ny + j) * nz + k are box's; cls(v)
 *     is what box reports for voxel v (FREE 0, OCCUPIED 1, UNKNOWN 2, MISSING 3, a BGK-LV map's UNCERTAIN 4).
 *   Passable.  v is passable iff pass_mask & (1u << cls(v)) is set and (clearance == 0 or distance_field(lo, dims,
 *     obstacle_mask, radius = clearance) reports d2[v] == LA3DM_DF_FAR): distance_field's definition over the same region.
 *     Obstacles outside the region are not seen; a caller pads the region where that matters.  obstacle_mask is ignored
 *     when clearance is 0.
 *   Seeds.  seeds[s] is a flat index.  A seed that is out of range (>= nx ny nz) or not passable is ignored; n_seeded =
 *     the number of DISTINCT passable voxels among the seeds.  n_seeds = 0 is served: everything is unreachable.
 *   Steps.  steps[v] = the least number of moves from any seeded voxel to v, each move to a neighbour under connectivity
 *     (frontier's offset sets: 6 = |di| + |dj| + |dk| = 1, 18 = a sum <= 2, 26 = all of {-1, 0, 1}^3 without 0) that is
 *     passable and inside the region.  A seeded voxel has steps 0.  steps[v] = LA3DM_REACH_NONE when v is not passable,
 *     when no such walk exists, or when the walk needs more than max_steps moves.
 *   Corner cutting.  A diagonal move (connectivity 18, 26) is NOT tested for the voxels it squeezes between: two passable
 *     voxels that touch by an edge or a corner are neighbours even when the voxels they share faces with are not
 *     passable.  A caller who minds that uses clearance >= 1 or connectivity 6.
 *   Targets.  target_steps[t] = steps[targets[t]], and LA3DM_REACH_NONE for an index out of range (>= nx ny nz).
 *   Stats (always a host struct, may be NULL): n_seeded; n_reached = the voxels with finite steps, seeds included;
 *     levels = the largest finite step (0 without a reached voxel).  levels == max_steps tells the caller that the wave
 *     may have been cut.
 *   Refused as a whole (LA3DM_ERR_ARG, a text that names the argument, nothing written), before the region's own
 *     checks: a pass_mask of 0 or with bits above 0x1F; with clearance > 0 an obstacle_mask of 0, and in any case one
 *     with bits above 0x1F; clearance > LA3DM_DF_MAX_RADIUS; a connectivity other than 6, 18, 26; max_steps outside
 *     1 ... LA3DM_REACH_MAX_STEPS; n_seeds > LA3DM_REACH_MAX_SEEDS; n_targets > 2^28; a NULL seeds or targets with a
 *     non-zero count; a NULL out, or an out with neither steps nor target_steps; target_steps set with n_targets = 0 or
 *     unset with n_targets > 0.  Then what box refuses for lo and dims, and as for frontier (nx + 2)(ny + 2)(nz + 2) >
 *     LA3DM_REACH_MAX_CELLS or a region that, padded by one voxel on every side, fails box's block-field range check.
 *   An empty map (every voxel MISSING) is answered all the same: an open box when pass_mask holds bit 3 (no obstacle
 *     unless obstacle_mask holds it too), nothing reached otherwise.
 *   Integers throughout, and the answer is unique: the results equal the host form (BGKOctoMap::reach on a host-mode
 *     map) exactly.
 *   Working storage, in a grow-only arena of the devmap (released with it; re-initialised on every call; a second call
 *     at the same or a smaller size allocates nothing): four bit streams over the padded box (passable, reached and two fronts that take
 *     turns: 1/2 byte per padded voxel), max_steps + 1 level counts, and 4 bytes per voxel that hold d2 (clearance > 0) and then the steps (when
 *     out->steps is not given to the device form).
 *   The host queues LA3DM_REACH_BATCH level launches, reads that batch's counts and stops at the first level that
 *     reached nothing; levels queued behind it see an empty front and write nothing. */
#define LA3DM_REACH_NONE      0xFFFFFFFFu
#define LA3DM_REACH_MAX_CELLS (1u << 28)
#define LA3DM_REACH_MAX_STEPS (1u << 16)
#define LA3DM_REACH_MAX_SEEDS (1u << 20)
#define LA3DM_REACH_BATCH     32
typedef struct la3dm_reach_out {
    uint32_t *steps;         /* [nx ny nz] or NULL */
    uint32_t *target_steps;  /* [n_targets] or NULL; at least one of the two */
} la3dm_reach_out;
typedef struct la3dm_reach_stats {
    uint32_t n_seeded;   /* distinct passable voxels among the seeds */
    uint32_t n_reached;  /* voxels with finite steps, seeds included */
    uint32_t levels;     /* the largest finite step */
} la3dm_reach_stats;
/* host pointers: upload of the seeds and targets, the launches, download of what was asked for (with target_steps alone:
 * n_targets words), synchronise — on the map's stream */
int la3dm_devmap_reach_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds,
                            uint32_t pass_mask, uint32_t obstacle_mask, uint32_t clearance, uint32_t connectivity,
                            uint32_t max_steps, const uint32_t *targets, uint32_t n_targets, const la3dm_reach_out *out,
                            la3dm_reach_stats *stats, la3dm_region_info *info);
/* device pointers (seeds, targets and out's arrays already in HBM on the map's device, 4-byte aligned; lo3, dims3, stats
 * and info stay host-side); returns when the results are complete */
int la3dm_devmap_reach_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const uint32_t *d_seeds, uint32_t n_seeds,
                              uint32_t pass_mask, uint32_t obstacle_mask, uint32_t clearance, uint32_t connectivity,
                              uint32_t max_steps, const uint32_t *d_targets, uint32_t n_targets, const la3dm_reach_out *d_out,
                              la3dm_reach_stats *stats, la3dm_region_info *info);
/* Travel: the least path cost from seed voxels through the passable voxels of a region, with weighted moves, a soft
 * penalty near obstacles and a parent per voxel to drive along — reach with costs.
 *   Region and lattice.  The region, anchor, lattice, info and flat index f = (i * ny + j) * nz + k are box's; cls(v)
 *     is what box reports for voxel v (FREE 0, OCCUPIED 1, UNKNOWN 2, MISSING 3, a BGK-LV map's UNCERTAIN 4).
 *   Distance.  Only when clearance > 0 or soft_radius > 0: R = max(clearance, soft_radius) and d2 = distance_field(lo,
 *     dims, obstacle_mask, radius = R) over the same region.  Obstacles outside the region are not seen, as for reach.
 *     obstacle_mask is ignored when R = 0.
 *   Passable.  v is passable iff pass_mask & (1u << cls(v)) is set and (clearance == 0 or d2[v] == LA3DM_DF_FAR or
 *     d2[v] > clearance^2).  With soft_radius = 0 this is reach's rule.
 *   Penalty.  pen(v) = floor(penalty * (S2 - d2[v]) / S2) with S2 = soft_radius^2 where soft_radius > 0 and d2[v] <= S2,
 *     and 0 elsewhere: a 64-bit product and a floor division; it falls linearly in the squared distance from just under
 *     `penalty` next to an obstacle to 0 at soft_radius.
 *   Moves.  connectivity is 6, 18 or 26 with frontier's offset sets.  A move along an offset with 1, 2 or 3 non-zero
 *     components costs move_cost[0], move_cost[1] or move_cost[2]: 10 / 14 / 17 approximates metres x 10 / resolution,
 *     1 / 1 / 1 makes cost equal reach's steps.  Diagonal moves are not tested for corner cutting, as for reach.
 *   Cost.  Entering passable v from passable u costs the move + pen(v).  A seeded voxel costs 0: its own penalty is not
 *     charged.  cost[v] = the minimum over all walks inside the region from any seeded voxel, LA3DM_TRAVEL_NONE where v
 *     is not passable, where no walk exists, or where the least cost exceeds max_cost.  (Candidates above max_cost are
 *     dropped while relaxing; every prefix of a least-cost walk is cheaper than the walk, so no cost <= max_cost changes.)
 *   Seeds and targets.  As reach's: a seed that is out of range (>= nx ny nz) or not passable is ignored, n_seeded counts
 *     the DISTINCT passable voxels among the seeds, n_seeds = 0 is served.  target_cost[t] = cost[targets[t]], and
 *     LA3DM_TRAVEL_NONE for an index out of range.
 *   Parent (optional, dense uint8).  An offset (di, dj, dk) has the code q = (di + 1) * 9 + (dj + 1) * 3 + (dk + 1).  A
 *     seeded voxel gets 13, an unreached voxel 255, any other reached v the smallest q such that the connectivity allows
 *     the offset, u = v + offset lies in the region, cost[u] is finite and cost[u] + move + pen(v) == cost[v].  Such a q
 *     exists and is a function of `cost` alone; following parents strictly lowers the cost and ends at a seeded voxel.
 *   Stats (always a host struct, may be NULL).  Contract: n_seeded, n_reached (voxels with a finite cost, seeds
 *     included), max_cost (the largest finite cost, 0 when nothing is reached).  Diagnostics of the device form, all 0 in
 *     the host form and no part of device == host: rounds (launches of the round kernel in which a voxel changed),
 *     brick_runs (brick relaxations run), capped (those that stopped at LA3DM_TRAVEL_INNER iterations).
 *   Refused as a whole (LA3DM_ERR_ARG, a text that names the argument, nothing written, nothing reserved), before the
 *     region's own checks: a NULL params; a pass_mask of 0 or with bits above 0x1F; an obstacle_mask with bits above 0x1F,
 *     or 0 with R > 0; clearance or soft_radius > LA3DM_DF_MAX_RADIUS; soft_radius > 0 with penalty 0; penalty >
 *     LA3DM_TRAVEL_MAX_PENALTY; a move_cost of 0 or > LA3DM_TRAVEL_MAX_MOVE; a connectivity other than 6, 18, 26;
 *     max_cost outside 1 ... LA3DM_TRAVEL_MAX_COST; n_seeds > LA3DM_TRAVEL_MAX_SEEDS; n_targets > 2^28; a NULL seeds or
 *     targets with a non-zero count; a NULL out, or an out with neither cost nor target_cost (parent alone is not
 *     enough); target_cost set with n_targets = 0 or unset with n_targets > 0.  Then what box refuses for lo and dims, and
 *     a region whose axes, each rounded up to a multiple of LA3DM_TRAVEL_BRICK, hold more than LA3DM_TRAVEL_MAX_CELLS
 *     voxels.  No sum overflows 32 bits: a candidate is at most 2^31 + 2^17.
 *   Non-convergence.  A call that needs more than LA3DM_TRAVEL_MAX_ROUNDS rounds fails with LA3DM_ERR_LIMIT and a text
 *     that says so; the outputs are then unspecified.
 *   An empty map (every voxel MISSING) is answered from the definition without reading the pool, as reach does.
 *   Integers throughout, and the answer is unique: the results equal the host form (BGKOctoMap::travel on a host-mode
 *     map: box's classes, the host distance transform, Dijkstra with a binary heap, then the parent pass) exactly.
 *   Device form (csrc/devmap_travel.h on csrc/devmap_brick.h): min-plus relaxation to its fixed point, which is unique whatever the order of the
 *     relaxations.  The cost lives in bricks of LA3DM_TRAVEL_BRICK^3 voxels; one workgroup relaxes one brick in LDS until
 *     nothing changes (at most LA3DM_TRAVEL_INNER iterations) before anything is written back, so a round moves the wave
 *     by a brick.  The host queues LA3DM_TRAVEL_BATCH rounds, reads that batch's counts and stops at the first round in
 *     which no voxel changed.  Working storage, in a grow-only arena of the devmap (released with it, re-initialised on
 *     every call; a second call at the same or a smaller size allocates nothing): 12 bytes per voxel of the region
 *     rounded up to whole bricks (two cost buffers, the entry words), 16 bytes per brick and the round counts; with
 *     R > 0 also 4 bytes per voxel for d2 and distance_field's own working storage. */
#define LA3DM_TRAVEL_NONE        0xFFFFFFFFu
#define LA3DM_TRAVEL_MAX_CELLS   (1u << 28)
#define LA3DM_TRAVEL_MAX_COST    (1u << 31)
#define LA3DM_TRAVEL_MAX_MOVE    (1u << 16)
#define LA3DM_TRAVEL_MAX_PENALTY (1u << 16)
#define LA3DM_TRAVEL_MAX_SEEDS   (1u << 20)
#define LA3DM_TRAVEL_MAX_ROUNDS  (1u << 16)
#define LA3DM_TRAVEL_BRICK       8
#define LA3DM_TRAVEL_INNER       16
#define LA3DM_TRAVEL_BATCH       8
typedef struct la3dm_travel_params {
    uint32_t pass_mask, obstacle_mask;
    uint32_t clearance;      /* voxels; 0: none */
    uint32_t soft_radius;    /* voxels; 0: no penalty */
    uint32_t penalty;        /* cost units at distance 0 */
    uint32_t move_cost[3];   /* moves with 1, 2, 3 non-zero components */
    uint32_t connectivity;   /* 6, 18, 26 */
    uint32_t max_cost;       /* 1 ... LA3DM_TRAVEL_MAX_COST */
} la3dm_travel_params;
typedef struct la3dm_travel_out {
    uint32_t *cost;         /* [nx ny nz] or NULL */
    uint32_t *target_cost;  /* [n_targets] or NULL; at least one of the two */
    uint8_t *parent;        /* [nx ny nz] or NULL */
} la3dm_travel_out;
typedef struct la3dm_travel_stats {
    uint32_t n_seeded;    /* distinct passable voxels among the seeds */
    uint32_t n_reached;   /* voxels with a finite cost, seeds included */
    uint32_t max_cost;    /* the largest finite cost */
    uint32_t rounds, brick_runs, capped;   /* diagnostics of the device form */
} la3dm_travel_stats;
/* host pointers: upload of the seeds and targets, the launches, download of what was asked for, synchronise — on the
 * map's stream */
int la3dm_devmap_travel_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds,
                             const la3dm_travel_params *params, const uint32_t *targets, uint32_t n_targets,
                             const la3dm_travel_out *out, la3dm_travel_stats *stats, la3dm_region_info *info);
/* device pointers (seeds, targets and out's arrays already in HBM on the map's device, cost and target_cost 4-byte
 * aligned; lo3, dims3, params, stats and info stay host-side); returns when the results are complete */
int la3dm_devmap_travel_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const uint32_t *d_seeds, uint32_t n_seeds,
                               const la3dm_travel_params *params, const uint32_t *d_targets, uint32_t n_targets,
                               const la3dm_travel_out *d_out, la3dm_travel_stats *stats, la3dm_region_info *info);
/* Score paths: cost and clearance of many candidate trajectories — the local planner's question.  Every path is a
 * polyline of waypoints; it is walked voxel by voxel through the region, the walk stops where it leaves the region or
 * comes too close to an obstacle, and what was walked is charged in travel's units, so that a walk costs here what it
 * costs there.
 *   Region and lattice.  The region, anchor, lattice, info and flat index f = (i * ny + j) * nz + k are box's.
 *   Distance.  R = max(1, clearance, soft_radius) and d2 = distance_field(lo, dims, obstacle_mask, radius = R) over the
 *     same region, unchanged, with its blind spot: obstacles outside the region are not seen.
 *   Inputs.  ways3: n_paths x n_way x 3 floats, world frame, the same n_way >= 1 for every path of a call; a shorter
 *     path is padded by repeating its last waypoint.  params: obstacle_mask, clearance, soft_radius, penalty and
 *     move_cost[3] mean what they mean in la3dm_travel_params; max_steps bounds the walk.
 *   Waypoint voxels.  Per waypoint and axis c the coordinate w is tested as the region tests lo, fabsf(w / resolution) <
 *     2^30 (false for NaN and inf), and resolved with the anchor's own arithmetic (score_poses: b, center, cell), G[c] =
 *     b * lim + cell as a 64-bit integer.  b is not restricted to [0, 2^20): such a voxel is simply outside the region.
 *     If any coordinate of any waypoint of a path fails the range test the whole path is LA3DM_PATH_INVALID, wherever the
 *     waypoint lies, also beyond a later stop: flags = INVALID, cost 0, steps 0, stop LA3DM_PATH_NONE, min_d2
 *     LA3DM_DF_FAR, ways 0.  This is the only floating-point work of the query besides the anchor's.
 *   The walk (integers).  For segment k = 1 ... n_way - 1: d = G[k] - G[k - 1], n_k = max_c |d[c]|, off[0] = 0, off[k] =
 *     off[k - 1] + n_k, T = off[n_way - 1].  The voxel of ordinal 0 is G[0]; for off[k - 1] < o <= off[k], with s = o -
 *     off[k - 1], v_o[c] = G[k - 1][c] + floor((2 s d[c] + n_k) / (2 n_k)): a floor division (the numerator can be
 *     negative) in 64 bits.  A segment with n_k = 0 contributes no voxel.  Hence: consecutive voxels differ by at most 1
 *     per axis and in at least one axis (the axis of n_k moves by exactly 1), so the walk is a 26-connected walk in
 *     travel's sense; v at s = n_k is G[k]; and the walk of the reversed waypoint list is the reversed walk (floor((2 (n
 *     - s) (-d) + n) / (2 n)) = -d + floor((2 s d + n) / (2 n))).
 *   Stop.  E = min(T, max_steps).  stop = the smallest ordinal in [0, E] whose voxel is outside the region
 *     (LA3DM_PATH_LEFT) or blocked, d2 != LA3DM_DF_FAR and d2 <= clearance^2 (LA3DM_PATH_BLOCKED); with clearance 0 that
 *     is the obstacle voxel itself.  (travel_entry leaves class tests to pass_mask; here the obstacle classes block.)
 *     LA3DM_PATH_TRUNCATED is set iff there is no stop and T > max_steps.  L = stop if there is one, else E + 1.
 *   Outputs per path.  cost (mandatory, 64 bits) = the sum over o = 1 ... L - 1 of move_cost[nz(o) - 1] + pen(d2[v_o]),
 *     nz(o) the number of non-zero components of v_o - v_(o-1) and pen travel's formula; voxel 0 is not charged, as
 *     travel's seed is not.  steps = L.  stop = the ordinal, or LA3DM_PATH_NONE.  min_d2 = the minimum of d2[v_o] over o
 *     < L, LA3DM_DF_FAR if none.  ways = the number of waypoints k with off[k] < L: how many waypoints the robot reaches.
 *     flags (uint8) = the LA3DM_PATH_* bits.  All outputs but cost are optional.
 *   Refused as a whole (LA3DM_ERR_ARG, a text that names the argument, nothing written, nothing reserved), in this
 *     order: a NULL params; an obstacle_mask of 0 or with bits above 0x1F; clearance or soft_radius > LA3DM_DF_MAX_RADIUS;
 *     soft_radius > 0 with penalty 0; penalty > LA3DM_TRAVEL_MAX_PENALTY; a move_cost of 0 or > LA3DM_TRAVEL_MAX_MOVE;
 *     max_steps outside 1 ... LA3DM_PATHS_MAX_STEPS; n_way outside 1 ... LA3DM_PATHS_MAX_WAY; n_paths >
 *     LA3DM_PATHS_MAX_PATHS; n_paths * n_way > LA3DM_PATHS_MAX_WAYPOINTS; with n_paths > 0 a NULL ways3, out or
 *     out->cost.  Then what box refuses for lo and dims, and more than LA3DM_DF_MAX_CELLS voxels.
 *   n_paths = 0 is served and writes nothing.  An empty map answers from the definition without a launch that reads the
 *     pool: every voxel is MISSING, so d2 is 0 everywhere if the mask holds bit 3 and FAR everywhere otherwise.
 *   No sum overflows: a path charges at most 2^20 steps of at most 2^17 each.
 *   Working storage: distance_field's 4 bytes per voxel and as many again for d2, in grow-only arenas of the devmap
 *     (score_poses' own; released with it; a smaller request after a larger one allocates nothing).
 *   Everything after the waypoint voxels is integers: the results equal the host form (BGKOctoMap::score_paths on a
 *     host-mode map, a plain loop) exactly.
 *   Device form (csrc/devmap_paths.h): one wave per path, four paths per workgroup; the waypoint voxels and the offsets
 *     (saturated at max_steps + 1) live in LDS, lanes take ordinals in ascending chunks of 64. */
#define LA3DM_PATHS_MAX_STEPS     (1u << 20)
#define LA3DM_PATHS_MAX_WAY       1024u
#define LA3DM_PATHS_MAX_PATHS     (1u << 20)
#define LA3DM_PATHS_MAX_WAYPOINTS (1u << 26)
#define LA3DM_PATH_BLOCKED   1u
#define LA3DM_PATH_LEFT      2u
#define LA3DM_PATH_TRUNCATED 4u
#define LA3DM_PATH_INVALID   8u
#define LA3DM_PATH_NONE      0xFFFFFFFFu
typedef struct la3dm_paths_params {
    uint32_t obstacle_mask;
    uint32_t clearance;      /* voxels; 0: only the obstacle voxels themselves block */
    uint32_t soft_radius;    /* voxels; 0: no penalty */
    uint32_t penalty;        /* cost units at distance 0 */
    uint32_t move_cost[3];   /* moves with 1, 2, 3 non-zero components */
    uint32_t max_steps;      /* 1 ... LA3DM_PATHS_MAX_STEPS */
} la3dm_paths_params;
typedef struct la3dm_paths_out {
    uint64_t *cost;     /* [n_paths] mandatory */
    uint32_t *steps;    /* [n_paths] or NULL: L, the voxels walked */
    uint32_t *stop;     /* [n_paths] or NULL: the ordinal of the stop, or LA3DM_PATH_NONE */
    uint32_t *min_d2;   /* [n_paths] or NULL */
    uint32_t *ways;     /* [n_paths] or NULL: waypoints reached */
    uint8_t *flags;     /* [n_paths] or NULL: LA3DM_PATH_* */
} la3dm_paths_out;
/* host pointers: upload of the waypoints, the launches, download, synchronise — on the map's stream */
int la3dm_devmap_score_paths_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *ways3, uint32_t n_paths,
                                  uint32_t n_way, const la3dm_paths_params *params, const la3dm_paths_out *out,
                                  la3dm_region_info *info);
/* device pointers (ways3 and out's arrays already in HBM on the map's device, 4-byte aligned — cost too; flags any
 * alignment; lo3, dims3, params and info stay host-side); returns when the results are complete */
int la3dm_devmap_score_paths_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const float *d_ways3, uint32_t n_paths,
                                    uint32_t n_way, const la3dm_paths_params *params, const la3dm_paths_out *d_out,
                                    la3dm_region_info *info);
/* Clusters: the connected groups of a region's member voxels, optionally confined to tiles and cut at a minimum size —
 * a dense label and one record per cluster (first voxel, size, bounding box, coordinate sums, a representative member).
 *   Region and lattice.  The region, anchor, lattice, info and flat index f = (i * ny + j) * nz + k are box's; cls(v)
 *     is what box reports for voxel v.
 *   Members.  member_mask holds the bits of stop_mask: non-zero, no bit above 0x1F.  from_list = 0: every voxel v of the
 *     region with member_mask & (1u << cls(v)) set is a member; members and n_members are then only checked, not used.
 *     from_list = 1: only the voxels listed in members[n_members] (flat indices, e.g. frontier's index) whose class is in
 *     member_mask are members; an index >= nx ny nz is ignored, a voxel listed twice counts once, n_members = 0 is served
 *     and gives no clusters.
 *   Adjacency.  connectivity is 6, 18 or 26 with frontier's offset sets, inside the region.  tile = 0: no tiling.
 *     Otherwise tile is a multiple of LA3DM_CLUSTERS_BRICK and at most LA3DM_CLUSTERS_MAX_TILE, and two voxels are
 *     adjacent only if i / tile, j / tile and k / tile agree (tiles are anchored at voxel (0, 0, 0) of the region).  A
 *     cluster is a maximal set of members connected through adjacent members.
 *   Minimum size.  min_size >= 1; a cluster with fewer members is dropped.
 *   Numbering.  The kept clusters are numbered 0 ... n - 1 in ascending order of `first`, their smallest flat index.
 *     *n_found = n whatever cap is (n_found may be NULL).
 *   Outputs (out may be NULL, and so may each array).  label[nx ny nz]: the number of the voxel's cluster,
 *     LA3DM_CLUSTERS_NONE for a non-member or a member of a dropped cluster.  of_member[n_members] (from_list = 1 only):
 *     the same per list entry, NONE for an ignored entry.  Records for c < min(n, cap): first[c], size[c]; lo[3c ...],
 *     hi[3c ...]: the bounding box in voxels of the region, inclusive; sum[3c ...]: the 64-bit sums of i, j and k over
 *     the members (the client divides); rep[c]: a member to drive to or look from — with c_a = (2 sum_a + size) /
 *     (2 size) in integer division, the member of the cluster with the smallest (i - c_0)^2 + (j - c_1)^2 + (k - c_2)^2,
 *     the smallest flat index among equals.  The rounded centroid need not be a member; rep always is.  cap = 0 with no
 *     record array counts, as frontier does.
 *   Stats (always a host struct, may be NULL).  Contract: n_members (distinct members), n_clusters (= n), n_dropped
 *     (clusters below min_size), largest (the largest size of a kept cluster, 0 when there is none).  Diagnostics of the
 *     device form, all 0 in the host form and no part of device == host: rounds (launches of the round kernel in which
 *     a voxel changed), brick_runs (brick relaxations run), capped (those that stopped at LA3DM_CLUSTERS_INNER
 *     iterations).
 *   Refused as a whole (LA3DM_ERR_ARG, a text that names the argument, nothing written, nothing reserved), in this
 *     order: a NULL params; a member_mask of 0 or with bits above 0x1F; a connectivity other than 6, 18, 26; a tile that
 *     is no multiple of LA3DM_CLUSTERS_BRICK or exceeds LA3DM_CLUSTERS_MAX_TILE; min_size 0; from_list > 1; n_members >
 *     LA3DM_CLUSTERS_MAX_MEMBERS; a NULL members with n_members > 0; of_member set with from_list = 0; cap > 0 with no
 *     record array.  Then what box refuses for lo and dims; an axis longer than LA3DM_CLUSTERS_MAX_AXIS (the squared
 *     distance of rep then fits 32 bits); a region whose axes, each rounded up to a multiple of LA3DM_CLUSTERS_BRICK,
 *     hold more than LA3DM_CLUSTERS_MAX_CELLS voxels.
 *   Non-convergence.  A call that needs more than LA3DM_CLUSTERS_MAX_ROUNDS rounds fails with LA3DM_ERR_LIMIT and a
 *     text that says so; the outputs are then unspecified.
 *   An empty map (every voxel MISSING) is served without reading the pool: member_mask = MISSING makes every voxel, or
 *     every listed voxel, a member.
 *   Integers throughout, and the answer is unique: the results equal the host form (BGKOctoMap::clusters on a host-mode
 *     map: box's classes, a flood fill from every unlabelled member in ascending flat order, the records in one pass,
 *     rep in a second) exactly.
 *   Device form (csrc/devmap_clusters.h on csrc/devmap_brick.h): travel's scheme with min in place of min-plus.  The label of a member starts
 *     as its own flat index; the fixed point of "take the smallest label among yourself and your adjacent members" is
 *     the cluster's `first`, whatever the order of the relaxations.  The labels live in bricks of LA3DM_CLUSTERS_BRICK^3
 *     voxels; one workgroup relaxes one brick in LDS until nothing changes (at most LA3DM_CLUSTERS_INNER iterations);
 *     the host queues LA3DM_CLUSTERS_BATCH rounds, reads that batch's counts and stops at the first round in which no
 *     voxel changed.  Sizes, the kept flags, the map's one-launch scan over them for the numbering, the labels and the
 *     records follow; sizes, boxes, sums and rep are reduced per wave and cluster before one atomic per group is issued.
 *     Working storage, in two grow-only arenas of the devmap (released with it, re-initialised on every call; a second
 *     call at the same or a smaller size allocates nothing): 8 bytes per voxel of the region rounded up to whole bricks
 *     (two label buffers), 12 bytes per voxel of the region (sizes, flags, numbers), 16 bytes per brick, the round
 *     counts, and 68 bytes per record written. */
#define LA3DM_CLUSTERS_NONE        0xFFFFFFFFu
#define LA3DM_CLUSTERS_MAX_CELLS   (1u << 28)
#define LA3DM_CLUSTERS_MAX_AXIS    (1u << 15)
#define LA3DM_CLUSTERS_MAX_TILE    (1u << 15)
#define LA3DM_CLUSTERS_MAX_MEMBERS (1u << 28)
#define LA3DM_CLUSTERS_MAX_ROUNDS  (1u << 16)
#define LA3DM_CLUSTERS_BRICK       8
#define LA3DM_CLUSTERS_INNER       16
#define LA3DM_CLUSTERS_BATCH       8
typedef struct la3dm_clusters_params {
    uint32_t member_mask;
    uint32_t from_list;       /* 0: every voxel of the region by its class; 1: the listed voxels only */
    uint32_t connectivity;    /* 6, 18, 26 */
    uint32_t tile;            /* 0: none; else a multiple of LA3DM_CLUSTERS_BRICK */
    uint32_t min_size;        /* >= 1 */
    uint32_t n_members;
    const uint32_t *members;  /* [n_members] flat indices (host or device memory, as the entry point says) */
    uint32_t cap;             /* records wanted at most */
} la3dm_clusters_params;
typedef struct la3dm_clusters_out {
    uint32_t *label;       /* [nx ny nz] or NULL */
    uint32_t *of_member;   /* [n_members] or NULL */
    uint32_t *first;       /* [cap] or NULL */
    uint32_t *size;        /* [cap] or NULL */
    uint32_t *lo, *hi;     /* [3 cap] or NULL */
    uint64_t *sum;         /* [3 cap] or NULL */
    uint32_t *rep;         /* [cap] or NULL */
} la3dm_clusters_out;
typedef struct la3dm_clusters_stats {
    uint32_t n_members;    /* distinct members */
    uint32_t n_clusters;   /* kept clusters: n */
    uint32_t n_dropped;    /* clusters below min_size */
    uint32_t largest;      /* the largest size of a kept cluster */
    uint32_t rounds, brick_runs, capped;   /* diagnostics of the device form */
} la3dm_clusters_stats;
/* host pointers (params->members included): upload of the list, the launches, download of what was asked for,
 * synchronise — on the map's stream */
int la3dm_devmap_clusters_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_clusters_params *params,
                               const la3dm_clusters_out *out, uint32_t *n_found, la3dm_clusters_stats *stats, la3dm_region_info *info);
/* device pointers (params->members and out's arrays already in HBM on the map's device, sum 8-byte aligned, the others
 * 4-byte; lo3, dims3, params, n_found, stats and info stay host-side); returns when the results are complete */
int la3dm_devmap_clusters_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_clusters_params *params,
                                 const la3dm_clusters_out *d_out, uint32_t *n_found, la3dm_clusters_stats *stats,
                                 la3dm_region_info *info);
/* Footing: where a ground robot can stand in a region of the map — the voxels with ground directly below, room for the
 * body above, and a footprint round them that is carried, not blocked, and climbable — as an ordered list and per column.
 *   Region and lattice.  The region, anchor, lattice, info and flat index f = (i * ny + j) * nz + k are box's; k grows
 *     along +z of the map frame.
 *   Classes.  cls(g) is what box would report for lattice voxel g, inside or outside the region: FREE 0, OCCUPIED 1,
 *     UNKNOWN 2, MISSING 3, a BGK-LV map's UNCERTAIN 4.  Classes outside the region are read from the map, as frontier
 *     reads its one-voxel halo: the answer for a voxel does not depend on where the region's faces are.
 *   Parameters (la3dm_footing_params).  support_mask and clear_mask hold the bits of stop_mask; headroom h, radius r,
 *     step s, min_support c.
 *   Definition.  ez = (0, 0, 1); disc = {(di, dj) : 0 < di^2 + dj^2 <= r^2}, N = |disc| (N = 0 for r = 0).
 *     stand(g) <=> cls(g - ez) in support_mask and cls(g + t ez) in clear_mask for every t in [0, h): ground below, and
 *       room for the body.
 *     near(g)  <=> stand(g + dk ez) for some |dk| <= s: there is ground within a climbable height of g.
 *     body(g)  <=> cls(g + t ez) in clear_mask for every t in [s, h): nothing in the body's way above the height the
 *       robot can climb over.
 *     foot(v), v in the region, <=> stand(v); body(v + (di, dj, 0)) for every (di, dj) in disc; and
 *       #{(di, dj) in disc : near(v + (di, dj, 0))} >= c.
 *     A cylinder of radius r and height h with a ground clearance of s voxels that stands at v hits nothing and has
 *     ground under at least c of its N footprint cells.  c = N is the strict footprint, a smaller c tolerates the holes of
 *     a sparsely observed floor, c = 0 asks only for an unobstructed body.
 *   Outputs.  *n_found = the number of foot voxels, whatever cap is.  out->index[cap]: the flat indices of the first
 *     min(n, cap) foot voxels in ascending order; entries past them are not written.  Dense, per column i * ny + j, and
 *     independent of cap: out->levels (uint32) = the foot voxels of the column, out->lowest / out->highest (int32) = their
 *     smallest / largest k, -1 where there are none.  cap = 0 with out NULL, or with only dense arrays set, counts.
 *     stats (a host struct, may be NULL): n_stand = the voxels of the region with stand, n_body = those with stand and the
 *     body condition, n_foot, disc_cells = N.  On an empty map n = 0, levels = 0, lowest = highest = -1.
 *   Refused as a whole (LA3DM_ERR_ARG, a text that names the argument, nothing written, nothing reserved), in this
 *     order: a NULL params; a mask that is 0 or has bits above 0x1F; masks that overlap; headroom outside [1,
 *     LA3DM_FOOTING_MAX_HEADROOM]; radius above LA3DM_FOOTING_MAX_RADIUS; step above LA3DM_FOOTING_MAX_STEP or step >=
 *     headroom; min_support > N; cap > 0 without out->index; what box refuses for lo and dims; a padded box that is too
 *     large or leaves the block-field range — the padded box (nx + 2r, ny + 2r, nz + h + 2s) extends r in x and y, 1 + s
 *     below and h - 1 + s above; it is refused when it holds more than LA3DM_FOOTING_MAX_CELLS voxels or when its block
 *     fields leave [0, 2^20); last a NULL n_found.
 *   Integer arithmetic on classes throughout: the results equal the host form (BGKOctoMap::footing on a host-mode map,
 *     host/footing_cells.h over the classes of the padded box) exactly.
 *   Device form (csrc/devmap_footing.h): bit streams over the padded box, 32 voxels per word with k fastest — one pool
 *     probe per padded voxel gives the support and the clear stream, a word pass derives stand, near and body from shifted
 *     windows, a second one ANDs the body windows over the disc and counts the near windows in a bit-sliced counter for
 *     the words that hold a stand bit, the map's scan and an emit kernel give the list, one lane per column the dense
 *     arrays.  No atomic is used.  Working storage: seven words per 32 padded voxels — 7/8 byte per padded voxel — and
 *     24 KB of partial counts, in a grow-only arena of the devmap (released with it). */
#define LA3DM_FOOTING_MAX_CELLS    (1u << 28)
#define LA3DM_FOOTING_MAX_HEADROOM 32
#define LA3DM_FOOTING_MAX_RADIUS   8
#define LA3DM_FOOTING_MAX_STEP     4
typedef struct la3dm_footing_params {
    uint32_t support_mask;   /* classes that carry: the voxel below */
    uint32_t clear_mask;     /* classes the body may occupy */
    uint32_t headroom;       /* h: voxels of free height, 1 .. LA3DM_FOOTING_MAX_HEADROOM */
    uint32_t radius;         /* r: footprint radius in voxels, 0 .. LA3DM_FOOTING_MAX_RADIUS */
    uint32_t step;           /* s: climbable height in voxels, 0 .. LA3DM_FOOTING_MAX_STEP, < headroom */
    uint32_t min_support;    /* c: footprint cells that must be carried, 0 .. N */
} la3dm_footing_params;
typedef struct la3dm_footing_out {
    uint32_t *index;      /* [cap] or NULL */
    uint32_t *levels;     /* [nx ny] or NULL, independent of cap */
    int32_t  *lowest;     /* [nx ny] or NULL */
    int32_t  *highest;    /* [nx ny] or NULL */
} la3dm_footing_out;
typedef struct la3dm_footing_stats {
    uint32_t n_stand;      /* voxels of the region with stand */
    uint32_t n_body;       /* ... and the body condition over the disc */
    uint32_t n_foot;       /* foot voxels: n */
    uint32_t disc_cells;   /* N */
} la3dm_footing_stats;
/* host pointers: the launches, download of min(*n_found, cap) entries and the dense arrays, synchronise — on the map's
 * stream */
int la3dm_devmap_footing_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_footing_params *params,
                              uint64_t cap, const la3dm_footing_out *out, uint64_t *n_found, la3dm_footing_stats *stats,
                              la3dm_region_info *info);
/* device pointers (out's arrays already in HBM on the map's device, 4-byte aligned; lo3, dims3, params, n_found, stats
 * and info stay host-side); returns when the results are complete */
int la3dm_devmap_footing_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_footing_params *params,
                                uint64_t cap, const la3dm_footing_out *d_out, uint64_t *n_found, la3dm_footing_stats *stats,
                                la3dm_region_info *info);
/* Surface: the exposed faces of the solid voxels of a region and an integer normal estimated from them, as an ordered
 * list and (the faces) per voxel.
 *   Region and lattice.  The region, anchor, lattice, info and flat index f = (i * ny + j) * nz + k are box's.
 *   Classes.  cls(g) is what box would report for lattice voxel g, inside or outside the region: FREE 0, OCCUPIED 1,
 *     UNKNOWN 2, MISSING 3, a BGK-LV map's UNCERTAIN 4.  Classes past the region's faces are read from the map, as frontier
 *     and footing read theirs: the answer for a voxel does not depend on where the region's faces are.
 *   Parameters (la3dm_surface_params).  solid_mask and open_mask hold the bits of stop_mask; smooth s, 0 ..
 *     LA3DM_SURFACE_MAX_SMOOTH.
 *   Definition.  The six directions are d = 0: -x, 1: +x, 2: -y, 3: +y, 4: -z, 5: +z, with unit vectors e_d.
 *     F_d(u)    = 1 when cls(u) is in solid_mask and cls(u + e_d) is in open_mask, else 0, for every voxel u of the
 *       lattice, inside the region or not.
 *     faces(u)  = sum over d of F_d(u) << d.
 *     A surface voxel is a voxel of the region with faces != 0.
 *     normal(v) = the sum over all u with |u - v|_inf <= s of (F_1 - F_0, F_3 - F_2, F_5 - F_4)(u): three int16, each at
 *       most (2 s + 1)^3 = 729 in size.  It points from solid into open space; with s = 0 it is the voxel's own face
 *       vector.  The sum of the face vectors of a voxelised patch is the area vector of the patch, so the windowed sum is
 *       an unbiased normal up to the window's rim.  It may be (0, 0, 0) — a one-voxel pillar, a table top seen from both
 *       sides —: callers treat that as "no normal".
 *   Outputs.  *n_found = the number of surface voxels, whatever cap is.  out->index[cap] (uint32): the flat indices of the
 *     first min(n, cap) surface voxels in ascending order; out->faces[cap] (uint8) and out->normal[3 cap] (int16) = the
 *     same entries' face masks and normals; entries past them are not written.  out->dense_faces[nx ny nz] (uint8,
 *     independent of cap) = faces of every voxel of the region, 0 where the voxel is not solid or not exposed: what a
 *     caller gathers at nearest's index.  cap = 0 with out NULL, or with only dense_faces set, counts.  stats (a host
 *     struct, may be NULL): n_solid = the voxels of the region with a class in solid_mask, n_surface = n, faces[d] = the
 *     voxels of the region with F_d; the surface area is their sum times resolution^2.  On an empty map n = 0,
 *     dense_faces = 0 and n_solid = nx ny nz when MISSING is in solid_mask, 0 when it is not.
 *   Refused as a whole (LA3DM_ERR_ARG, a text that names the argument, nothing written, nothing reserved), in this
 *     order: a NULL params; a mask that is 0 or has bits above 0x1F; masks that overlap; smooth above
 *     LA3DM_SURFACE_MAX_SMOOTH; out->normal without out->index; cap > 0 with neither out->index nor out->faces; what box
 *     refuses for lo and dims; a padded box that is too large or leaves the block-field range — the working box is the
 *     region padded by p = s + 1 voxels on all six sides, (nx + 2 p, ny + 2 p, nz + 2 p); it is refused when it holds more
 *     than LA3DM_SURFACE_MAX_CELLS voxels or when its block fields leave [0, 2^20); last a NULL n_found.
 *   Integer arithmetic on classes throughout: the results equal the host form (BGKOctoMap::surface on a host-mode map,
 *     host/surface_cells.h over the classes of the padded box) exactly.
 *   Device form (csrc/devmap_surface.h): bit streams over the padded box, 32 voxels per word with k fastest — one pool
 *     probe per padded voxel gives the solid and the open stream, a word pass the six face streams, the candidate words
 *     and the counts, the map's scan and an emit kernel the list; with s > 0 a wave per candidate word sums the face
 *     windows of the (2 s + 1)^2 columns round it in bit-sliced counters.  No atomic is used.  Working storage: eleven words
 *     per 32 padded voxels — 11/8 byte per padded voxel — and 64 KB of partial counts, in a grow-only arena of the devmap
 *     (released with it). */
#define LA3DM_SURFACE_MAX_CELLS  (1u << 28)
#define LA3DM_SURFACE_MAX_SMOOTH 4
typedef struct la3dm_surface_params {
    uint32_t solid_mask;   /* classes that make a voxel solid */
    uint32_t open_mask;    /* classes a face may look into */
    uint32_t smooth;       /* s: half width of the normal's window in voxels, 0 .. LA3DM_SURFACE_MAX_SMOOTH */
} la3dm_surface_params;
typedef struct la3dm_surface_out {
    uint32_t *index;         /* [cap] or NULL */
    uint8_t  *faces;         /* [cap] or NULL */
    int16_t  *normal;        /* [3 cap] or NULL; needs index */
    uint8_t  *dense_faces;   /* [nx ny nz] or NULL, independent of cap */
} la3dm_surface_out;
typedef struct la3dm_surface_stats {
    uint64_t n_solid;      /* voxels of the region with a class in solid_mask */
    uint64_t n_surface;    /* surface voxels: n */
    uint64_t faces[6];     /* exposed faces per direction -x, +x, -y, +y, -z, +z */
} la3dm_surface_stats;
/* host pointers: the launches, download of min(*n_found, cap) entries and the dense array, synchronise — on the map's
 * stream */
int la3dm_devmap_surface_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_surface_params *params,
                              uint64_t cap, const la3dm_surface_out *out, uint64_t *n_found, la3dm_surface_stats *stats,
                              la3dm_region_info *info);
/* device pointers (out's arrays already in HBM on the map's device, index 4-byte and normal 2-byte aligned; lo3, dims3,
 * params, n_found, stats and info stay host-side); returns when the results are complete */
int la3dm_devmap_surface_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const la3dm_surface_params *params,
                                uint64_t cap, const la3dm_surface_out *d_out, uint64_t *n_found, la3dm_surface_stats *stats,
                                la3dm_region_info *info);
/* Drive: the least cost of a ground route from seed voxels over a set of MEMBER voxels of a region — the voxels footing
 * finds —, with moves that climb or drop up to `step` voxels, and a parent per voxel to drive along.  travel routes a
 * flying point through a class mask; drive routes a ground robot over the places where it can stand.
 *   Region and lattice.  The region, anchor, lattice, info and flat index f = (i * ny + j) * nz + k are box's; k grows
 *     along +z of the map frame.
 *   Members, list mode (params->footing NULL, params->members not NULL).  members[n_members] are flat indices, e.g.
 *     footing's index.  clusters' rule for from_list = 1: an index >= nx ny nz is ignored, a voxel listed twice counts
 *     once, n_members = 0 is served (members must still point somewhere: a NULL members with a NULL footing is no mode at
 *     all).  There is no class test: the list is the truth, the pool is never read, and an empty map is served like any
 *     other.
 *   Members, footing mode (params->footing not NULL; members NULL, n_members 0).  The members are exactly the voxels that
 *     footing(lo, dims, *params->footing) would list.  params->footing is a host pointer in both pointer forms.  On an
 *     empty map there is no member.
 *   Moves.  A move goes from member u to member v = u + (a, b, c) with (a, b) != (0, 0), |a|, |b| <= 1 and |c| <= step,
 *     step in 0 ... LA3DM_DRIVE_MAX_STEP.  connectivity is 4 (|a| + |b| = 1) or 8.  There is no purely vertical move: a
 *     floor and a table top in one column are joined only by a ramp of members.  Diagonal moves are not tested for corner
 *     cutting, as for travel.  The move costs move_cost[|a| + |b| - 1] + (c > 0 ? climb_up * c : climb_down * -c);
 *     move_cost[0], move_cost[1] in 1 ... LA3DM_TRAVEL_MAX_MOVE, climb_up, climb_down in 0 ... LA3DM_TRAVEL_MAX_MOVE.  Every
 *     move costs at least 1, so the least costs are unique.
 *   Cost.  cost[v] = the minimum over all walks of members from any seeded member to v; a seeded member costs 0.
 *     LA3DM_DRIVE_NONE for a non-member, for a member no walk reaches, and where the least cost exceeds max_cost (1 ...
 *     2^31).  (Candidates above max_cost are dropped while relaxing; every prefix of a least-cost walk is no dearer than the
 *     walk, so no cost <= max_cost changes.)  No sum overflows 32 bits: a candidate is at most 2^31 + 2^16 + 4 * 2^16.
 *   Seeds, targets, snap.  seeds and targets are flat indices.  snap in 0 ... LA3DM_DRIVE_MAX_SNAP.  A seed or target (i,
 *     j, k) stands for the member (i, j, k') with the largest k' in [max(0, k - snap), k]: the sensor's voxel can be passed
 *     as it is.  With an index out of range (>= nx ny nz), or with no such member, a seed is ignored and a target gets
 *     LA3DM_DRIVE_NONE.  n_seeded counts the DISTINCT seeded members; n_seeds = 0 is served.  target_cost[t] = the cost at
 *     the snapped member, target_index[t] (optional) = that member's flat index, or LA3DM_DRIVE_NONE.
 *   Parent (optional, dense uint8).  The offset o = u - v from v back to u has the code q = ((o_i + 1) * 3 + (o_j + 1)) *
 *     9 + (o_k + 4), 0 ... 80.  A seeded member gets 40, a non-member or an unreached voxel 255, any other reached v the
 *     smallest q such that the move u -> v is allowed, u lies in the region and is a member, cost[u] is finite and cost[u] +
 *     move(u -> v) == cost[v].  Such a q exists and is a function of `cost` and the member set alone; following parents
 *     strictly lowers the cost and ends at a seeded member.
 *   Outputs (la3dm_drive_out).  cost [nx ny nz]; parent [nx ny nz]; of_member [n_members] = the cost per list entry,
 *     LA3DM_DRIVE_NONE for an ignored entry, list mode only; target_cost and target_index [n_targets].  At least one of
 *     cost, of_member, target_cost must be set.
 *   Stats (always a host struct, may be NULL).  Contract: n_members (distinct members in the region), n_seeded, n_reached
 *     (members with a finite cost, seeds included), max_cost (the largest finite cost, 0 when nothing is reached).
 *     Diagnostics of the device form, all 0 in the host form and no part of device == host: rounds, brick_runs, capped, as
 *     travel's.
 *   Refused as a whole (LA3DM_ERR_ARG, a text that names the argument, nothing written, nothing reserved), in this order:
 *     a NULL params; a connectivity other than 4 or 8; step > LA3DM_DRIVE_MAX_STEP; snap > LA3DM_DRIVE_MAX_SNAP; a
 *     move_cost of 0 or > LA3DM_TRAVEL_MAX_MOVE; climb_up or climb_down > LA3DM_TRAVEL_MAX_MOVE; max_cost outside 1 ...
 *     LA3DM_TRAVEL_MAX_COST; n_members > LA3DM_DRIVE_MAX_MEMBERS; n_seeds > LA3DM_DRIVE_MAX_SEEDS; n_targets > 2^28; a NULL
 *     seeds, targets or members with a non-zero count; both modes at once (footing and members), or neither; a NULL out;
 *     of_member set in footing mode or with n_members = 0; an out with none of cost, of_member and target_cost (parent or
 *     target_index alone is not enough); target_cost or target_index set with n_targets = 0, or target_cost unset with
 *     n_targets > 0.  Footing mode then refuses what footing refuses for *params->footing, in footing's order and with its
 *     texts.  Then what box refuses for lo and dims, and a region whose axes, each rounded up to a multiple of
 *     LA3DM_DRIVE_BRICK, hold more than LA3DM_DRIVE_MAX_CELLS voxels; in footing mode last footing's padded box that is too
 *     large or leaves the block-field range.
 *   Non-convergence.  A call that needs more than LA3DM_DRIVE_MAX_ROUNDS rounds fails with LA3DM_ERR_LIMIT and a text
 *     that says so; the outputs are then unspecified.
 *   Integers throughout, and the answer is unique: the results equal the host form (host/drive_cells.h — Dijkstra with a
 *     binary heap, then the parent pass — which BGKOctoMap::drive calls on a host-mode map, in footing mode after its own
 *     footing) exactly.
 *   Device form (csrc/devmap_drive.h on csrc/devmap_brick.h's grid and round driver): travel's scheme.  The round kernel
 *     relaxes a brick in a 10 x 10 x 16 LDS tile that holds LA3DM_DRIVE_MAX_STEP levels below and above the brick.  In
 *     footing mode footing's launches run up to the foot words and one kernel turns the foot bits of the region's voxels
 *     into entry words: nothing is listed, scanned or downloaded.  Working storage, in a grow-only arena of the devmap
 *     (released with it, re-initialised on every call): 12 bytes per voxel of the region rounded up to whole bricks, 16
 *     bytes per brick and the round counts; in footing mode also footing's own working storage. */
#define LA3DM_DRIVE_NONE        0xFFFFFFFFu
#define LA3DM_DRIVE_MAX_CELLS   (1u << 28)
#define LA3DM_DRIVE_MAX_MEMBERS (1u << 28)
#define LA3DM_DRIVE_MAX_SEEDS   (1u << 20)
#define LA3DM_DRIVE_MAX_STEP    4
#define LA3DM_DRIVE_MAX_SNAP    32
#define LA3DM_DRIVE_MAX_ROUNDS  (1u << 16)
#define LA3DM_DRIVE_BRICK       8
#define LA3DM_DRIVE_INNER       16
#define LA3DM_DRIVE_BATCH       8
typedef struct la3dm_drive_params {
    const uint32_t *members;                 /* list mode: [n_members] flat indices (device form: device memory); else NULL */
    const la3dm_footing_params *footing;     /* footing mode: a host struct; else NULL */
    uint32_t n_members;
    uint32_t connectivity;   /* 4 or 8 */
    uint32_t step;           /* voxels a move may climb or drop, 0 ... LA3DM_DRIVE_MAX_STEP */
    uint32_t snap;           /* voxels a seed or target may lie above its member, 0 ... LA3DM_DRIVE_MAX_SNAP */
    uint32_t move_cost[2];   /* moves with |a| + |b| = 1, 2 */
    uint32_t climb_up;       /* per voxel climbed */
    uint32_t climb_down;     /* per voxel dropped */
    uint32_t max_cost;       /* 1 ... LA3DM_TRAVEL_MAX_COST */
} la3dm_drive_params;
typedef struct la3dm_drive_out {
    uint32_t *cost;          /* [nx ny nz] or NULL */
    uint8_t *parent;         /* [nx ny nz] or NULL */
    uint32_t *of_member;     /* [n_members] or NULL; list mode only */
    uint32_t *target_cost;   /* [n_targets] or NULL */
    uint32_t *target_index;  /* [n_targets] or NULL */
} la3dm_drive_out;
typedef struct la3dm_drive_stats {
    uint32_t n_members;   /* distinct members in the region */
    uint32_t n_seeded;    /* distinct seeded members */
    uint32_t n_reached;   /* members with a finite cost, seeds included */
    uint32_t max_cost;    /* the largest finite cost */
    uint32_t rounds, brick_runs, capped;   /* diagnostics of the device form */
} la3dm_drive_stats;
/* host pointers (params->members included): upload of the list, the seeds and the targets, the launches, download of what
 * was asked for, synchronise — on the map's stream */
int la3dm_devmap_drive_host(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds,
                            const la3dm_drive_params *params, const uint32_t *targets, uint32_t n_targets,
                            const la3dm_drive_out *out, la3dm_drive_stats *stats, la3dm_region_info *info);
/* device pointers (seeds, targets, params->members and out's arrays already in HBM on the map's device, the word arrays
 * 4-byte aligned; lo3, dims3, params, params->footing, stats and info stay host-side); returns when the results are
 * complete */
int la3dm_devmap_drive_device(la3dm_devmap *dm, const float *lo3, const uint32_t *dims3, const uint32_t *d_seeds, uint32_t n_seeds,
                              const la3dm_drive_params *params, const uint32_t *d_targets, uint32_t n_targets,
                              const la3dm_drive_out *d_out, la3dm_drive_stats *stats, la3dm_region_info *info);
/* Leaf export =the publish loop of the static node (src/bgkoctomap/bgkoctomap_static_node.cpp:101-136) with the
 * cube-list bookkeeping of MarkerArrayPub (include/common/markerarray_pub.h:104-147) minus ROS, run on the pool:
 * state 1 = OCCUPIED leaves coloured by height (heightMapColor when min_z < max_z, else the marker default),
 * state 0 = FREE leaves coloured by probability.  original_size 0 expands a collapsed leaf into the
 * base-resolution cells of get_pruned_locs (bgkoctomap.h:269-287).  cells/rgba: 4 floats per cell {x, y, z, size} /
 * {r, g, b, a}; level = (int) log2(size / resolution) = index of the CUBE_LIST marker.  Order: pool blocks, leaves
 * in LeafIterator order.  Call with cells = rgba = level = NULL to get *count, then with buffers (host pointers). */
int la3dm_devmap_export_cells(la3dm_devmap *dm, int state, int original_size, float min_z, float max_z, float *cells,
                              float *rgba, int32_t *level, uint64_t cap, uint64_t *count);
/* smallest / largest block index per axis (the 20-bit fields of BlockHashKey): get_bbox
 * (src/bgkoctomap/bgkoctomap.cpp:368-381) without a download */
int la3dm_devmap_key_bounds(la3dm_devmap *dm, int32_t lo[3], int32_t hi[3]);
/* training set (x, y, z, label) of the last scan, for parity tests; *n = number of points */
int la3dm_devmap_training_data(la3dm_devmap *dm, float *xyzy, uint32_t cap, uint32_t *n);
/* test hook (host pointers, n entries): out_fast = the closed-form sum of m[i] copies of x[i] onto s[i] that
 * the voxel-grid kernel uses for runs of identical samples, out_loop = the plain sequential fp32 loop */
int la3dm_devmap_diag_add_repeat(la3dm_ctx *ctx, const float *s, const float *x, const uint32_t *m, uint32_t n,
                                 float *out_fast, float *out_loop);
/* Test hooks for the device-resident front end's own scan / sort primitives (la3dm_amd/csrc/devmap_scan.h,
 * devmap_sort.h), run on the map's stream and self-cleaning state; host arrays in and out.
 * scan, mode 0: out[i] = in[0] + ... + in[i-1], aux[0] = total.
 * scan, mode 1: in = keys sorted ascending, 0xFFFFFFFF = invalid (last); out = exclusive scan of the head flags,
 *               aux = {segments, valid keys, seg_start[0 .. segments]} (room for n + 3 words).
 * sort: stable, on the low `bits` bits of the keys. */
int la3dm_devmap_diag_scan(la3dm_devmap *dm, int mode, const uint32_t *in, uint32_t n, uint32_t *out, uint32_t *aux);
int la3dm_devmap_diag_sort(la3dm_devmap *dm, const uint32_t *keys, const uint32_t *vals, uint32_t n, int bits,
                           uint32_t *keys_out, uint32_t *vals_out);

#ifdef __cplusplus
}
#endif
#endif /* LA3DM_HIP_H */
