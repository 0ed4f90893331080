// devmap_merge.h — the device side of merge (contract: include/la3dm_hip.h, la3dm_devmap_merge_host; the rule per block on
// flat arrays and the host-mode map's form of it: host/merge_block.h): a validated map stream fused into the live pool.
// Included by devmap.hip only.
//   dm_merge_find    one lane per stream block: the table probe (pool_find_block) -> the block's slot, or kNoSlot and a
//                    "new" flag; flag[n_blocks] = 0 closes the list, so the map's one-launch scan over n_blocks + 1 flags
//                    gives every new block its offset and, as its last output, the number created.  Nothing is written
//                    to the map.
//   dm_merge_insert  (after grow_pool / grow_table on the host) one lane per stream block: a new block takes slot
//                    n_old + offset — stream order — and publishes its key in blk_key and the table (the keys of a
//                    validated stream are distinct and absent from the table: a CAS on the empty key, no find).
//   dm_merge_fuse    one wave per stream block, four waves per workgroup.  In LDS per wave: the stream's mask words with
//                    their exclusive popcount prefixes (as dm_unpack_expand), the destination block's S bytes (a created
//                    block: all UNKNOWN, nothing read from the pool), the result's A, B per finest cell, the result tree's
//                    S bytes and, per node, the finest cell its values come from.  The finest cells are walked 64 at a
//                    time: both trees are climbed to the covering leaves, the rule (kept / copied / fused) applied, the
//                    cell's result kept in LDS; the three counters come from ballots and reach memory as one atomic per
//                    wave and counter (on kMergeCntSlots lines per counter, summed by the host).  Then OcTree::prune's
//                    rule bottom up in LDS — the parent takes child 0's WHOLE S byte and its source cell, so a collapsed
//                    chain is resolved to its bottom cell as it forms — and every node of the block is written once,
//                    coalesced, in unpack's canonical form.  No global atomics on the data path, no register array
//                    indexed at run time.
// LDS: merge_lds_stride(block_depth) bytes per wave — 6.6 KB at block_depth 4, 52.7 KB at 5.  Four waves at block_depth 5
// would take 211 KB of a CU's 160 KB: la3dm_devmap_merge_host REFUSES a block_depth whose four waves do not fit
// (merge_lds_fits), with a text that says so; block_depth 1 .. 4 run.
#ifndef LA3DM_DEVMAP_MERGE_H
#define LA3DM_DEVMAP_MERGE_H

#include "devmap_pack.h"

namespace la3dm_dev {

constexpr uint32_t kMergeLdsPerCu = 160u * 1024u;
// The cell counters: atomics on one 128-byte line serialise like atomics on one word, and a merge of 44 k blocks would queue
// 132 k of them on a single line.  Counter k of slot s lives on a line of its own, word (3 s + k) kMergeCntStride; a
// workgroup adds to slot blockIdx.x % kMergeCntSlots and the host sums the slots after its one read-back.
constexpr uint32_t kMergeCntSlots = 64, kMergeCntStride = 16, kMergeCntWords = 3u * kMergeCntSlots * kMergeCntStride;
// dm_merge_fuse's dynamic LDS per wave: 2 W mask / prefix words, A and B per finest cell, dS and T per node (bytes),
// src per node (16 bits)
__host__ __device__ inline uint32_t merge_lds_stride(uint32_t block_depth) {
    const uint32_t npb = (uint32_t)(((1ull << (3u * block_depth)) - 1u) / 7u), ncell = 1u << (3u * (block_depth - 1u));
    const uint32_t W = (npb + 31u) >> 5, nS = (npb + 3u) & ~3u;
    return (8u * W + 8u * ncell + 2u * nS + 2u * nS + 15u) & ~15u;
}
__host__ __device__ inline bool merge_lds_fits(uint32_t block_depth) {
    return (uint64_t)kPackWaves * merge_lds_stride(block_depth) <= kMergeLdsPerCu;
}

__global__ __launch_bounds__(256) void dm_merge_find(const long long *__restrict__ keys, uint32_t n_blocks, PoolView pool,
                                                    uint32_t has_table, uint32_t *slot, uint32_t *flag) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == n_blocks) flag[n_blocks] = 0u;   // (the grid covers n_blocks + 1 lanes)
    if (b >= n_blocks) return;
    const uint32_t s = has_table ? pool_find_block(pool, keys[b]) : kNoSlot;
    slot[b] = s;
    flag[b] = s == kNoSlot ? 1u : 0u;
}

__global__ __launch_bounds__(256) void dm_merge_insert(const long long *__restrict__ keys, uint32_t n_blocks,
                                                      const uint32_t *__restrict__ flag, const uint32_t *__restrict__ off, uint32_t n_old,
                                                      long long *tab_key, uint32_t *tab_val, uint32_t mask, long long *blk_key,
                                                      uint32_t *slot) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks || !flag[b]) return;
    const uint32_t s = n_old + off[b];
    const long long k = keys[b];
    blk_key[s] = k;
    slot[b] = s;
    uint32_t h = hash_key64(k, mask);
    for (uint32_t probe = 0; probe <= mask; ++probe) {   // (the table holds at most half its slots: an empty one is near)
        const long long prev = (long long)atomicCAS((unsigned long long *)&tab_key[h], (unsigned long long)kEmptyKey, (unsigned long long)k);
        if (prev == kEmptyKey) {
            tab_val[h] = s;
            return;
        }
        h = (h + 1) & mask;
    }
}

struct MergeArgs {
    float *A, *B;   // the pool
    uint8_t *S;
    uint32_t n_blocks, npb, block_depth;   // blocks of the stream
    const uint32_t *slot, *flag;           // per stream block: pool slot; 1 = created by this merge
    const uint32_t *leaf_off, *mask;       // the stream's sections
    const uint8_t *i_state;
    const float *i_A, *i_B;
    float a0, b0;                          // the default node
    float free_thresh, occupied_thresh, var_thresh;
    unsigned long long *cells;             // kept, copied, fused: kMergeCntWords words, zero at launch
};

// Occupancy::update's state: the exact-division form (classify(), bgk_kernels.h; host twin: la3dm_merge::classify)
__device__ __forceinline__ uint8_t merge_classify(float A, float B, const MergeArgs &a) {
    const float s = A + B;
    const float var = (A * B) / ((s * s) * (s + 1.0f));
    if (var > a.var_thresh) return 2;
    const float p = A / s;
    return p > a.occupied_thresh ? 1 : (p < a.free_thresh ? 0 : 2);
}

// Dynamic LDS: kPackWaves x merge_lds_stride(block_depth) bytes.
__global__ __launch_bounds__(64 * kPackWaves) void dm_merge_fuse(MergeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t dm_merge_smem[];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * kPackWaves + wv;
    if (b >= a.n_blocks) return;
    const uint32_t npb = a.npb, dl = a.block_depth - 1u, W = (npb + 31u) >> 5, ncell = 1u << (3u * dl), nS = (npb + 3u) & ~3u;
    const uint32_t fine = dm_layer_base(dl);
    uint8_t *mine = dm_merge_smem + (size_t)wv * merge_lds_stride(a.block_depth);
    uint32_t *sW = (uint32_t *)mine, *sP = sW + W;
    float *cA = (float *)(sP + W), *cB = cA + ncell;
    uint16_t *src = (uint16_t *)(cB + ncell);
    uint8_t *dS = (uint8_t *)(src + nS), *T = dS + nS;

    const uint32_t *mb = a.mask + (size_t)b * W;
    uint32_t run = 0;
    for (uint32_t w0 = 0; w0 < W; w0 += 64) {   // the words and the exclusive prefix of their popcounts
        const uint32_t w = w0 + lane;
        const uint32_t word = w < W ? mb[w] : 0u;
        uint32_t incl = (uint32_t)__popc(word);
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, s, 64);
            if ((int)lane >= s) incl += o;
        }
        if (w < W) {
            sW[w] = word;
            sP[w] = run + incl - (uint32_t)__popc(word);
        }
        run += (uint32_t)__shfl((int)incl, 63, 64);
    }
    const bool created = a.flag[b] != 0u;
    const size_t base = (size_t)a.slot[b] * npb;
    for (uint32_t i = lane; i < npb; i += 64) {
        dS[i] = created ? kStateUnknown : a.S[base + i];
        T[i] = kStateUnknown;   // a node above the leaves stays UNKNOWN and never passes for a leaf in the prune
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    const uint32_t first = a.leaf_off[b];
    const uint32_t a0 = __float_as_uint(a.a0), b0 = __float_as_uint(a.b0);
    uint32_t n_kept = 0, n_copied = 0, n_fused = 0;
    for (uint32_t c0 = 0; c0 < ncell; c0 += 64) {
        const uint32_t c = c0 + lane;
        const bool live = c < ncell;
        bool kept = false, copied = false, fused = false;
        if (live) {
            // the stream's covering leaf: the first set mask bit on the way up (a validated stream tiles the block)
            uint32_t d = dl, i = c, n2 = fine + c;
            while (d > 0 && !((sW[n2 >> 5] >> (n2 & 31u)) & 1u)) {
                --d;
                i >>= 3;
                n2 = dm_layer_base(d) + i;
            }
            const uint32_t word = sW[n2 >> 5], bit = n2 & 31u;
            const uint32_t r = first + sP[n2 >> 5] + (uint32_t)__popc(word & ((1u << bit) - 1u));
            const float a2 = a.i_A[r], b2 = a.i_B[r];
            float a1 = a.a0, b1 = a.b0;
            uint8_t s1 = kStateUnknown;
            if (!created) {
                uint32_t d1, i1;
                (void)pool_leaf_class(dS, dl, c, d1, i1);
                const uint32_t n1 = dm_layer_base(d1) + i1;
                a1 = a.A[base + n1];
                b1 = a.B[base + n1];
                s1 = dS[n1];
            }
            if (__float_as_uint(a2) == a0 && __float_as_uint(b2) == b0) {
                kept = true;
            } else if (__float_as_uint(a1) == a0 && __float_as_uint(b1) == b0) {
                copied = true;
                a1 = a2;
                b1 = b2;
                s1 = a.i_state[r];
            } else {
                fused = true;
                a1 = a1 + (a2 - a.a0);
                b1 = b1 + (b2 - a.b0);
                s1 = (uint8_t)(merge_classify(a1, b1, a) | kClassifiedBit);
            }
            cA[c] = a1;
            cB[c] = b1;
            T[fine + c] = s1;
            src[fine + c] = (uint16_t)c;
        }
        n_kept += (uint32_t)__popcll(__ballot(kept));
        n_copied += (uint32_t)__popcll(__ballot(copied));
        n_fused += (uint32_t)__popcll(__ballot(fused));
    }
    if (lane == 0) {   // one atomic per wave and counter, spread over kMergeCntSlots lines per counter
        unsigned long long *cnt = a.cells + (size_t)(blockIdx.x % kMergeCntSlots) * 3u * kMergeCntStride;
        if (n_kept) atomicAdd(cnt, (unsigned long long)n_kept);
        if (n_copied) atomicAdd(cnt + kMergeCntStride, (unsigned long long)n_copied);
        if (n_fused) atomicAdd(cnt + 2u * kMergeCntStride, (unsigned long long)n_fused);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    for (uint32_t d = dl; d > 0; --d) {   // OcTree::prune's rule; the parent takes child 0's whole byte and source cell
        const uint32_t lb = dm_layer_base(d), pb = dm_layer_base(d - 1u), ngroup = 1u << (3u * (d - 1u));
        for (uint32_t g = lane; g < ngroup; g += 64) {
            const uint32_t g0 = lb + 8u * g;
            const uint8_t t0 = T[g0], st0 = t0 & 7u;
            if (st0 == kStatePruned || st0 == kStateUnknown) continue;
            bool same = true;
#pragma unroll
            for (int k = 1; k < 8; ++k) same &= (T[g0 + k] & 7u) == st0;
            if (!same) continue;
            T[pb + g] = t0;
            src[pb + g] = src[g0];
#pragma unroll
            for (int k = 0; k < 8; ++k) T[g0 + k] = kStatePruned;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }

    for (uint32_t n = lane; n < npb; n += 64) {   // canonical form, every node once
        const uint8_t t = T[n], st = t & 7u;
        const bool leaf = st != kStatePruned && (n >= fine || st != kStateUnknown);
        float va = a.a0, vb = a.b0;
        if (leaf) {
            const uint32_t sc = src[n];
            va = cA[sc];
            vb = cB[sc];
        }
        a.A[base + n] = va;
        a.B[base + n] = vb;
        a.S[base + n] = leaf ? t : (st == kStatePruned ? kStatePruned : kStateUnknown);
    }
}

}  // namespace la3dm_dev

#endif
