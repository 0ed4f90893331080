// devmap_evict.h — the device side of pack_region and erase_region (contract: include/la3dm_hip.h,
// la3dm_devmap_pack_region_host / la3dm_devmap_erase_region_host; the region test: host/region_blocks.h, the same
// function on both sides).  Included by devmap.hip only.
//   dm_evict_select  one lane per pool block: blk_key against the box -> a 0 / 1 flag; flag[n_blocks] = 0 closes the list,
//                    so the map's one-launch scan over n_blocks + 1 flags gives every selected block its rank r(b) = the
//                    number of selected slots before b and, as its last output, the number selected.
//   dm_evict_list    (pack_region) one lane per pool block: a selected block writes its slot to list[r(b)] and its key to
//                    the stream's key section.  dm_pack_count<true> / dm_pack_emit<true> (devmap_pack.h) then run over the
//                    list: stream block b is pool slot list[b].
//   dm_evict_plan    (erase_region) one lane per pool block, from the one scan: with n_new = n_blocks - r(n_blocks), a
//                    removed slot b < n_new is hole number r(b); a surviving slot b >= n_new is tail survivor number
//                    (b - n_new) - (r(b) - r(n_new)).  Both lists are ascending by construction and equally long, r(n_new).
//   dm_evict_move    one wave per (tail[i] -> hole[i]) pair, four waves per workgroup: npb dwords of A and of B, lanes on
//                    consecutive dwords (a block's rows start at slot * npb * 4 bytes: dword aligned, nothing wider is — npb
//                    is odd); npb bytes of S, lanes on consecutive BYTES: a row starts at slot * npb bytes, any alignment,
//                    source and destination differently, and byte accesses neither need an aligned head / tail nor touch a
//                    neighbouring block (S is 1 / 9 of the bytes moved); the key by lane 0.  Sources (>= n_new) and
//                    destinations (< n_new) are disjoint: in place, no staging.  No atomics, no LDS, no register array.
#ifndef LA3DM_DEVMAP_EVICT_H
#define LA3DM_DEVMAP_EVICT_H

#include "devmap_pack.h"
#include "host/region_blocks.h"

namespace la3dm_dev {

using EvictBox = la3dm_region_blocks::Box;

__global__ __launch_bounds__(256) void dm_evict_select(const long long *__restrict__ blk_key, uint32_t n_blocks, EvictBox box,
                                                      uint32_t *flag) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == n_blocks) flag[n_blocks] = 0u;   // (the grid covers n_blocks + 1 lanes)
    if (b >= n_blocks) return;
    flag[b] = la3dm_region_blocks::selected(blk_key[b], box) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void dm_evict_list(const long long *__restrict__ blk_key, uint32_t n_blocks,
                                                    const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank,
                                                    uint32_t *list, long long *keys) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks || !flag[b]) return;
    const uint32_t r = rank[b];
    list[r] = b;
    keys[r] = blk_key[b];
}

// hole[] and tail[] have room for min(n_removed, n_new) entries each (the host sizes them after its read-back)
__global__ __launch_bounds__(256) void dm_evict_plan(uint32_t n_blocks, const uint32_t *__restrict__ flag,
                                                    const uint32_t *__restrict__ rank, uint32_t *hole, uint32_t *tail) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks) return;
    const uint32_t n_new = n_blocks - rank[n_blocks];
    const uint32_t r = rank[b];
    if (b < n_new) {
        if (flag[b]) hole[r] = b;
    } else if (!flag[b]) {
        tail[(b - n_new) - (r - rank[n_new])] = b;
    }
}

// The grid covers min(n_removed, n_new) waves, the most pairs there can be; the number there are, r(n_new), is read here
// (the host learns it with the call's last copy, not with a read-back of its own in the middle of the chain).
__global__ __launch_bounds__(64 * kPackWaves) void dm_evict_move(float *A, float *B, uint8_t *S, long long *blk_key, uint32_t npb,
                                                                 const uint32_t *__restrict__ n_pairs, const uint32_t *__restrict__ hole,
                                                                 const uint32_t *__restrict__ tail) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * kPackWaves + (threadIdx.x >> 6);
    if (i >= *n_pairs) return;
    const uint32_t dst = hole[i], src = tail[i];
    const size_t d0 = (size_t)dst * npb, s0 = (size_t)src * npb;
    for (uint32_t n = lane; n < npb; n += 64) {
        A[d0 + n] = A[s0 + n];
        B[d0 + n] = B[s0 + n];
        S[d0 + n] = S[s0 + n];
    }
    if (lane == 0) blk_key[dst] = blk_key[src];
}

}  // namespace la3dm_dev

#endif
