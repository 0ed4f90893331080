// devmap_diff.h — the device side of diff (contract: include/la3dm_hip.h, la3dm_devmap_diff_host; the rule per block on
// flat arrays and the host-mode map's form of it: host/diff_block.h): the finest cells whose class — or, on request, whose
// values — differ between the live pool (NOW) and a validated map stream (THEN).  merge's read-only sibling: nothing here
// writes the pool.  Included by devmap.hip only.
//   dm_merge_find    (devmap_merge.h, as it stands) the pool slot per stream block, or kNoSlot.
//   dm_diff_mark     (map_only) one lane per stream block: mark[slot] = 1 for the slots found (mark[] zeroed before).
//   dm_diff_select   (map_only) one lane per pool slot: flag = 1 where the slot is unmarked; flag[n_pool] = 0 closes the list,
//                    so the map's one-launch scan gives every unmarked slot its rank and, last, their number — which stays
//                    on the device: the count launch covers n_stream + n_pool waves and reads it there.
//   dm_diff_list     (map_only) one lane per pool slot: an unmarked slot goes to only[rank] — ascending slot, pack's order.
//   dm_diff_count    one wave per compared block, four waves per workgroup.  In LDS per wave: the stream block's mask words
//                    with their exclusive popcount prefixes (as dm_merge_fuse / dm_unpack_expand) and the map block's S
//                    bytes.  The finest cells are walked 64 at a time in ascending c: the stream side climbs to the first
//                    set mask bit, the map side calls pool_leaf_class; ten ballots (then == t, now == n) give the 25 pair
//                    counts of the chunk, which lane 5 t + n keeps — one counter per lane, no register array indexed at run
//                    time; the value-changed counts go to lanes 25 .. 29 the same way.  The block's number of selected
//                    cells goes to counts[b] (the scan makes the list offsets of it), and the counters reach memory as one
//                    atomic per wave and non-zero counter, on kDiffCntSlots lines per counter (one line would serialise:
//                    kMergeCntSlots' argument), summed by the host after its one read-back.
//   dm_diff_emit     the same walk; the entries of a chunk go to offset[b] + running base + prefix popcount of the selection
//                    ballot: no atomics, ascending c.  Entries at or past cap are not written.
//   kValues: A and B of the two covering leaves are gathered only when value_mask or an A / B output needs them; the
//   class-only form reads the pool's S, the stream's mask words and the stream's state bytes alone.
//   A stream block the map lacks (slot kNoSlot) reads nothing from the pool; a map-only block reads no stream section.
// LDS: diff_lds_stride(block_depth) bytes per wave — 0.7 KB at block_depth 4, 5.7 KB at 5, 45.7 KB at 6, whose four waves
// would take 183 KB of a CU's 160 KB: la3dm_devmap_diff_host REFUSES that depth (diff_lds_fits), which la3dm_devmap_create
// does not accept today either; block_depth 1 .. 5, every depth a device map can have, run.
#ifndef LA3DM_DEVMAP_DIFF_H
#define LA3DM_DEVMAP_DIFF_H

#include "devmap_merge.h"

namespace la3dm_dev {

// counters: 25 pairs (5 then + now), 5 value-changed (25 + now), cells selected, stream blocks the map lacks, map-only blocks
constexpr uint32_t kDiffCnt = 33, kDiffCntSelected = 30, kDiffCntMissing = 31, kDiffCntOnly = 32;
// counter k of slot s lives on a line of its own, word (kDiffCnt s + k) kMergeCntStride; a workgroup adds to slot
// blockIdx.x % kDiffCntSlots (16 slots: 33 counters x 16 lines are 66 KB to clear and to read back)
constexpr uint32_t kDiffCntSlots = 16, kDiffCntWords = kDiffCnt * kDiffCntSlots * kMergeCntStride;
constexpr uint32_t kDiffDead = 7;   // the class of a lane past the block's last cell: no ballot counts it

// dynamic LDS per wave: 2 W mask / prefix words, the block's S bytes
__host__ __device__ inline uint32_t diff_lds_stride(uint32_t block_depth) {
    const uint32_t npb = (uint32_t)(((1ull << (3u * block_depth)) - 1u) / 7u);
    const uint32_t W = (npb + 31u) >> 5, nS = (npb + 3u) & ~3u;
    return (8u * W + nS + 15u) & ~15u;
}
__host__ __device__ inline bool diff_lds_fits(uint32_t block_depth) {
    return (uint64_t)kPackWaves * diff_lds_stride(block_depth) <= kMergeLdsPerCu;
}

__global__ __launch_bounds__(256) void dm_diff_mark(const uint32_t *__restrict__ slot, uint32_t n_stream, uint32_t *mark) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_stream) return;
    const uint32_t s = slot[b];
    if (s != kNoSlot) mark[s] = 1u;   // (the keys of a validated stream are distinct: one writer per slot)
}

__global__ __launch_bounds__(256) void dm_diff_select(const uint32_t *__restrict__ mark, uint32_t n_pool, uint32_t *flag) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s == n_pool) flag[n_pool] = 0u;   // (the grid covers n_pool + 1 lanes)
    if (s >= n_pool) return;
    flag[s] = mark[s] ? 0u : 1u;
}

__global__ __launch_bounds__(256) void dm_diff_list(uint32_t n_pool, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank,
                                                   uint32_t *only) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_pool || !flag[s]) return;
    only[rank[s]] = s;
}

struct DiffArgs {
    const float *A, *B;   // the pool, read only
    const uint8_t *S;
    const long long *blk_key;
    uint32_t npb, block_depth;
    uint32_t n_stream;                // blocks of the stream
    uint32_t n_grid;                  // count: waves that may hold a block; emit: compared blocks
    const uint32_t *n_only;           // count: the number of map-only blocks, on the device (null: none)
    const uint32_t *slot, *only;      // per stream block: pool slot or kNoSlot; the map-only slots
    const long long *keys;            // the stream's sections
    const uint32_t *leaf_off, *mask;
    const uint8_t *i_state;
    const float *i_A, *i_B;
    float a0, b0;                     // the default node
    uint32_t pair_mask, value_mask;
    uint32_t *counts;                 // count: selected cells per compared block, n_grid + 1 entries
    unsigned long long *cnt;          // count: kDiffCntWords words, zero at launch
    const uint32_t *offset;           // emit: the scan of counts
    uint32_t cap;
    const float4 *lut;
    float block_size;
    long long *o_key;                 // emit: the list, every array optional
    uint32_t *o_cell;
    uint8_t *o_code;
    float *o_centre, *o_A, *o_B;
};

// One compared block as a wave sees it: which sides exist, where they lie, and the staged LDS.
struct DiffBlock {
    bool has_stream, has_map;
    uint32_t dl, ncell, fine, first;
    size_t base;        // the map block's first node in the pool
    long long key;
    const uint32_t *sW, *sP;
    const uint8_t *dS;
};

// Which block wave `b` compares, and its staging.  `mine` = the wave's LDS.
__device__ __forceinline__ void diff_stage(const DiffArgs &a, uint32_t b, uint32_t lane, uint8_t *mine, DiffBlock &k) {
    const uint32_t npb = a.npb, W = (npb + 31u) >> 5;
    k.dl = a.block_depth - 1u;
    k.ncell = 1u << (3u * k.dl);
    k.fine = dm_layer_base(k.dl);
    k.has_stream = b < a.n_stream;
    uint32_t s;
    if (k.has_stream) {
        s = a.slot[b];
        k.key = a.keys[b];
        k.first = a.leaf_off[b];
    } else {
        s = a.only[b - a.n_stream];
        k.key = a.blk_key[s];
        k.first = 0u;
    }
    k.has_map = s != kNoSlot;
    k.base = k.has_map ? (size_t)s * npb : 0u;
    uint32_t *sW = (uint32_t *)mine, *sP = sW + W;
    uint8_t *dS = (uint8_t *)(sP + W);
    if (k.has_stream) {   // the words and the exclusive prefix of their popcounts
        const uint32_t *mb = a.mask + (size_t)b * W;
        uint32_t run = 0;
        for (uint32_t w0 = 0; w0 < W; w0 += 64) {
            const uint32_t w = w0 + lane;
            const uint32_t word = w < W ? mb[w] : 0u;
            uint32_t incl = (uint32_t)__popc(word);
#pragma unroll
            for (int sh = 1; sh < 64; sh <<= 1) {
                const uint32_t o = (uint32_t)__shfl_up((int)incl, sh, 64);
                if ((int)lane >= sh) incl += o;
            }
            if (w < W) {
                sW[w] = word;
                sP[w] = run + incl - (uint32_t)__popc(word);
            }
            run += (uint32_t)__shfl((int)incl, 63, 64);
        }
    }
    if (k.has_map)
        for (uint32_t i = lane; i < npb; i += 64) dS[i] = a.S[k.base + i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    k.sW = sW;
    k.sP = sP;
    k.dS = dS;
}

// Finest cell c of the block (c >= ncell: a dead lane, both classes kDiffDead): the two classes, whether the cell is
// value-changed, and the NOW leaf's values (kValues; the default node where the map lacks the block).
template <bool kValues>
__device__ __forceinline__ void diff_cell(const DiffArgs &a, const DiffBlock &k, uint32_t c, uint32_t &then, uint32_t &now, bool &vchg,
                                          float &a1, float &b1) {
    then = now = kDiffDead;
    vchg = false;
    a1 = a.a0;
    b1 = a.b0;
    if (c >= k.ncell) return;
    uint32_t r = 0;
    if (k.has_stream) {   // the stream's covering leaf: the first set mask bit on the way up (a validated stream tiles the block)
        uint32_t d = k.dl, i = c, n2 = k.fine + c;
        while (d > 0 && !((k.sW[n2 >> 5] >> (n2 & 31u)) & 1u)) {
            --d;
            i >>= 3;
            n2 = dm_layer_base(d) + i;
        }
        const uint32_t word = k.sW[n2 >> 5], bit = n2 & 31u;
        r = k.first + k.sP[n2 >> 5] + (uint32_t)__popc(word & ((1u << bit) - 1u));
        then = a.i_state[r] & 7u;
    } else {
        then = kClsMissing;
    }
    if (k.has_map) {
        uint32_t d1, i1;
        now = pool_leaf_class(k.dS, k.dl, c, d1, i1);
        if (kValues) {
            const uint32_t n1 = dm_layer_base(d1) + i1;
            a1 = a.A[k.base + n1];
            b1 = a.B[k.base + n1];
        }
    } else {
        now = kClsMissing;
    }
    if (kValues && a.value_mask && k.has_stream && k.has_map && then == now)
        vchg = __float_as_uint(a.i_A[r]) != __float_as_uint(a1) || __float_as_uint(a.i_B[r]) != __float_as_uint(b1);
}

__device__ __forceinline__ bool diff_selected(const DiffArgs &a, uint32_t then, uint32_t now, bool vchg) {
    if (then == kDiffDead) return false;
    return ((a.pair_mask >> (5u * then + now)) & 1u) || (vchg && ((a.value_mask >> now) & 1u));
}

// Dynamic LDS: kPackWaves x diff_lds_stride(block_depth) bytes.  The grid covers n_grid + 1 waves.
template <bool kValues>
__global__ __launch_bounds__(64 * kPackWaves) void dm_diff_count(DiffArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t dm_diff_smem[];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * kPackWaves + wv;
    if (b > a.n_grid) return;
    const uint32_t n_only = a.n_only ? *a.n_only : 0u;
    if (b >= a.n_stream + n_only) {   // the closing entry, and the waves past the last map-only block
        if (lane == 0) a.counts[b] = 0u;
        return;
    }
    DiffBlock k;
    diff_stage(a, b, lane, dm_diff_smem + (size_t)wv * diff_lds_stride(a.block_depth), k);
    uint32_t acc = 0, total = 0;   // acc: counter `lane` of this block
    for (uint32_t c0 = 0; c0 < k.ncell; c0 += 64) {
        uint32_t then, now;
        bool vchg;
        float a1, b1;
        diff_cell<kValues>(a, k, c0 + lane, then, now, vchg, a1, b1);
        unsigned long long bt[5], bn[5];
#pragma unroll
        for (uint32_t t = 0; t < 5; ++t) {
            bt[t] = __ballot(then == t);
            bn[t] = __ballot(now == t);
        }
#pragma unroll
        for (uint32_t t = 0; t < 5; ++t)
#pragma unroll
            for (uint32_t n = 0; n < 5; ++n) {
                const uint32_t pairs = (uint32_t)__popcll(bt[t] & bn[n]);
                if (lane == 5u * t + n) acc += pairs;
            }
        if (kValues) {
            const unsigned long long bv = __ballot(vchg);
#pragma unroll
            for (uint32_t n = 0; n < 5; ++n) {
                const uint32_t changed = (uint32_t)__popcll(bv & bn[n]);
                if (lane == 25u + n) acc += changed;
            }
        }
        total += (uint32_t)__popcll(__ballot(diff_selected(a, then, now, vchg)));
    }
    if (lane == 0) a.counts[b] = total;
    if (lane == kDiffCntSelected) acc = total;
    if (lane == kDiffCntMissing) acc = k.has_map ? 0u : 1u;
    if (lane == kDiffCntOnly) acc = k.has_stream ? 0u : 1u;
    // one atomic per wave and non-zero counter, every counter of a slot on a line of its own
    if (lane < kDiffCnt && acc)
        atomicAdd(a.cnt + ((size_t)(blockIdx.x % kDiffCntSlots) * kDiffCnt + lane) * kMergeCntStride, (unsigned long long)acc);
}

// Dynamic LDS: kPackWaves x diff_lds_stride(block_depth) bytes.  The grid covers the n_grid compared blocks.
template <bool kValues>
__global__ __launch_bounds__(64 * kPackWaves) void dm_diff_emit(DiffArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t dm_diff_smem[];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * kPackWaves + wv;
    if (b >= a.n_grid) return;
    uint32_t out = a.offset[b];
    if (out >= a.cap || a.offset[b + 1u] == out) return;   // nothing of this block is listed
    DiffBlock k;
    diff_stage(a, b, lane, dm_diff_smem + (size_t)wv * diff_lds_stride(a.block_depth), k);
    const float bs = a.block_size;
    const float cx = axis_center(k.key >> 40, bs), cy = axis_center((k.key >> 20) & 0xFFFFF, bs), cz = axis_center(k.key & 0xFFFFF, bs);
    for (uint32_t c0 = 0; c0 < k.ncell && out < a.cap; c0 += 64) {
        const uint32_t c = c0 + lane;
        uint32_t then, now;
        bool vchg;
        float a1, b1;
        diff_cell<kValues>(a, k, c, then, now, vchg, a1, b1);
        const bool sel = diff_selected(a, then, now, vchg);
        const unsigned long long vote = __ballot(sel);
        const uint32_t r = out + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
        if (sel && r < a.cap) {
            if (a.o_key) a.o_key[r] = k.key;
            if (a.o_cell) a.o_cell[r] = c;
            if (a.o_code) a.o_code[r] = (uint8_t)(then | (now << 4));
            if (a.o_centre) {
                const float4 o = a.lut[k.fine + c];
                a.o_centre[3u * (size_t)r] = o.x + cx;
                a.o_centre[3u * (size_t)r + 1u] = o.y + cy;
                a.o_centre[3u * (size_t)r + 2u] = o.z + cz;
            }
            if (kValues) {
                if (a.o_A) a.o_A[r] = a1;
                if (a.o_B) a.o_B[r] = b1;
            }
        }
        out += (uint32_t)__popcll(vote);
    }
}

}  // namespace la3dm_dev

#endif
