// devmap_pack.h — the device side of save / load (contract and stream layout: include/la3dm_hip.h, la3dm_devmap_pack_host;
// host code of the format: host/pack_format.h): the pool's covering leaves compacted into the stream before it crosses PCIe,
// and the stream expanded into the canonical pool.  Included by devmap.hip only.
//
// All three kernels: one wave per block, four waves per workgroup, a block's nodes taken 64 at a time in download's depth-major
// numbering, so that the wave's ballot over "node n is a covering leaf" IS two words of the block's mask.
//   dm_pack_count   reads S only (staged in LDS: the leaf test of node (d, i) reads its child 0, node (d + 1, 8 i)) and writes
//                   the block's mask words and leaf count; counts[n_blocks] = 0 closes the list for the scan, whose output over
//                   n_blocks + 1 items is the stream's leaf_off section as it stands
//   dm_pack_emit    re-reads the mask words (the ballots) and gathers state, A, B of the set nodes to leaf_off[b] + rank, rank =
//                   the prefix popcount inside the 64-node chunk + the popcount of the chunks before it (a running base in a
//                   scalar): no atomics, no register array indexed at run time.  Workgroup 0 also zeroes the stream's padding.
//   Both take the pool slot of stream block b behind a template flag: pack reads slot b, pack_region (devmap_evict.h) the
//   slot its list names; the mask words, counts and leaves are indexed by the STREAM block either way.
//   dm_unpack_expand loads the block's mask words and their exclusive popcount prefixes into LDS and writes every node of the
//                   block exactly once, coalesced: a set node takes its leaf's values, a node with a set ancestor (init, PRUNED),
//                   every other node (init, UNKNOWN).  It only ever sees a stream that host/pack_format.h validated.
#ifndef LA3DM_DEVMAP_PACK_H
#define LA3DM_DEVMAP_PACK_H

#include "devmap_pool.h"

namespace la3dm_dev {

constexpr uint32_t kPackWaves = 4;   // waves (= blocks) per workgroup
__host__ __device__ inline uint32_t pack_lds_stride(uint32_t npb) { return (npb + 15u) & ~15u; }   // dm_pack_count: bytes per wave

// layer of node n in the depth-major order (n < nodes per block, at most 6 layers)
__device__ __forceinline__ uint32_t pack_layer_of(uint32_t n, uint32_t dl) {
    uint32_t d = 0;
    while (d < dl && n >= dm_layer_base(d + 1u)) ++d;
    return d;
}

// Dynamic LDS: kPackWaves x pack_lds_stride(npb) bytes.
// kList (pack_region, devmap_evict.h): stream block b is pool slot list[b]; else (pack) it is slot b and list is not read.
template <bool kList>
__global__ __launch_bounds__(64 * kPackWaves) void dm_pack_count(const uint8_t *__restrict__ S, uint32_t n_blocks, uint32_t npb,
                                                                 uint32_t block_depth, uint32_t *counts, uint32_t *mask,
                                                                 const uint32_t *__restrict__ list) {
    extern __shared__ __attribute__((aligned(16))) uint8_t dm_pack_smem[];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * kPackWaves + wv;
    if (b == n_blocks && lane == 0) counts[n_blocks] = 0u;   // (the grid covers n_blocks + 1 waves)
    if (b >= n_blocks) return;
    uint8_t *sS = dm_pack_smem + wv * pack_lds_stride(npb);
    const uint8_t *Sb = S + (size_t)(kList ? list[b] : b) * npb;
    for (uint32_t i = lane; i < npb; i += 64) sS[i] = Sb[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t dl = block_depth - 1u, W = (npb + 31u) >> 5;
    uint32_t *mb = mask + (size_t)b * W;
    uint32_t total = 0;
    for (uint32_t n0 = 0; n0 < npb; n0 += 64) {
        const uint32_t n = n0 + lane;
        bool leaf = false;
        if (n < npb && (sS[n] & 7u) != kStatePruned) {
            const uint32_t d = pack_layer_of(n, dl);
            leaf = d == dl || (sS[dm_layer_base(d + 1u) + 8u * (n - dm_layer_base(d))] & 7u) == kStatePruned;
        }
        const unsigned long long vote = __ballot(leaf);
        const uint32_t word = (n0 >> 5) + (lane >> 5);
        if ((lane & 31u) == 0u && word < W) mb[word] = lane ? (uint32_t)(vote >> 32) : (uint32_t)vote;
        total += (uint32_t)__popcll(vote);
    }
    if (lane == 0) counts[b] = total;
}

struct PackGaps {   // the stream's padding: gap g is the bytes [at[g], at[g] + len[g]), len < 16
    uint64_t at[6];
    uint32_t len[6];
};

template <bool kList>
__global__ __launch_bounds__(64 * kPackWaves) void dm_pack_emit(const float *__restrict__ A, const float *__restrict__ B,
                                                                const uint8_t *__restrict__ S, uint32_t n_blocks, uint32_t npb,
                                                                const uint32_t *__restrict__ leaf_off, const uint32_t *__restrict__ mask,
                                                                uint8_t *o_state, float *o_A, float *o_B, uint8_t *stream, PackGaps gaps,
                                                                const uint32_t *__restrict__ list) {
    if (blockIdx.x == 0 && threadIdx.x < 6u * 16u) {
        const uint32_t g = threadIdx.x >> 4, i = threadIdx.x & 15u;
        if (i < gaps.len[g]) stream[gaps.at[g] + i] = 0;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * kPackWaves + (threadIdx.x >> 6);
    if (b >= n_blocks) return;
    const uint32_t W = (npb + 31u) >> 5;
    const uint32_t *mb = mask + (size_t)b * W;
    const size_t base = (size_t)(kList ? list[b] : b) * npb;
    uint32_t out = leaf_off[b];
    for (uint32_t n0 = 0; n0 < npb; n0 += 64) {
        const uint32_t w0 = n0 >> 5;
        const unsigned long long vote = (unsigned long long)mb[w0] | (w0 + 1u < W ? (unsigned long long)mb[w0 + 1u] << 32 : 0ull);
        if ((vote >> lane) & 1ull) {
            const uint32_t r = out + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
            const size_t node = base + n0 + lane;
            o_state[r] = S[node];
            o_A[r] = A[node];
            o_B[r] = B[node];
        }
        out += (uint32_t)__popcll(vote);
    }
}

// Dynamic LDS: kPackWaves x 2 W words.
__global__ __launch_bounds__(64 * kPackWaves) void dm_unpack_expand(float *A, float *B, uint8_t *S, uint32_t n_blocks, uint32_t npb,
                                                                    uint32_t block_depth, const uint32_t *__restrict__ leaf_off,
                                                                    const uint32_t *__restrict__ mask, const uint8_t *__restrict__ i_state,
                                                                    const float *__restrict__ i_A, const float *__restrict__ i_B, float a0,
                                                                    float b0) {
    extern __shared__ __attribute__((aligned(16))) uint8_t dm_pack_smem[];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * kPackWaves + wv;
    if (b >= n_blocks) return;
    const uint32_t dl = block_depth - 1u, W = (npb + 31u) >> 5;
    uint32_t *sW = (uint32_t *)dm_pack_smem + (size_t)wv * 2u * W, *sP = sW + W;
    const uint32_t *mb = mask + (size_t)b * W;
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
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const size_t base = (size_t)b * npb;
    const uint32_t first = leaf_off[b];
    for (uint32_t n = lane; n < npb; n += 64) {
        const uint32_t word = sW[n >> 5], bit = n & 31u;
        float a = a0, bb = b0;
        uint8_t st = kStateUnknown;
        if ((word >> bit) & 1u) {
            const uint32_t r = first + sP[n >> 5] + (uint32_t)__popc(word & ((1u << bit) - 1u));
            a = i_A[r];
            bb = i_B[r];
            st = i_state[r];
        } else {
            uint32_t d = pack_layer_of(n, dl), i = n - dm_layer_base(d);
            while (d > 0) {
                --d;
                i >>= 3;
                const uint32_t an = dm_layer_base(d) + i;
                if ((sW[an >> 5] >> (an & 31u)) & 1u) {
                    st = kStatePruned;
                    break;
                }
            }
        }
        A[base + n] = a;
        B[base + n] = bb;
        S[base + n] = st;
    }
}

}  // namespace la3dm_dev

#endif
