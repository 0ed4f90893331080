// devmap_frontier.h — frontier of a map region on the device-resident block pool: the voxels whose class is in the open
// mask and that have at least min_neighbours neighbours (6 / 18 / 26 connectivity) whose class is in the unknown mask, as
// an ordered list (la3dm_devmap_frontier_*, include/la3dm_hip.h; host twin and definition: BGKOctoMap::frontier,
// host/bgkoctomap.cpp).  Integer arithmetic on classes throughout: the result equals the host form bit for bit.
//
// Everything runs on the PADDED box (PX, PY, PZ) = (nx + 2, ny + 2, nz + 2), whose voxel (0, 0, 0) lies one step below
// the region's on every axis: a neighbour of padded index p is p + di PY PZ + dj PZ + dk, with no test at the faces, and
// the classes one step outside the region are read from the map as box would read them there.
//
// dm_fr_bits     one probe per padded voxel as dm_df_bits does it, two ballots: the OPEN stream (class in open_mask and
//                the voxel inside the region — pad cells never open) and the UNKNOWN stream (class in unknown_mask, pad
//                cells included).  1/8 byte per padded voxel each; the class itself is never stored.
// dm_fr_stencil  one lane per 32-voxel word of the open stream.  A word of zeros ends there (44 % of the words on the
//                one-scan map of DESIGN.md 3.10; more where free space is mostly enclosed by known space).  Otherwise
//                per offset of the connectivity the 32-bit window of the unknown stream at that bit offset (two words,
//                one funnel shift) is added into a bit-sliced counter (bit b of plane q = bit q of the count of voxel b):
//                all 32 voxels are counted at once.  The planes are compared with min_neighbours, the open word is
//                replaced IN PLACE by the frontier word, and its popcount goes to the compaction's input.  With `score`
//                the lane also scatters the counts of its open voxels into the dense output (zeroed before).
// (scan)         devmap.hip's exclusive_scan over n_words + 1 popcounts (the last is 0): the prefix of the extra element
//                is the total, a word of the query's own — no slot of the map's counter block is used.
// dm_fr_emit     one lane per word; each set bit becomes the unpadded flat index at its place in the list, until cap.
//                With `nbrs` the lane counts its word again (the same code as the stencil) instead of reading a stored
//                score: the query keeps no per-voxel byte.
//
// Working storage: open / frontier words, unknown words, popcounts and prefixes — 4 x 4 bytes per 32 padded voxels, 1/2
// byte per padded voxel.
//
// Every loop is bounded by an argument or by the table size / depth: the offsets, 32 bits of a word, the probe count.
#ifndef LA3DM_DEVMAP_FRONTIER_H
#define LA3DM_DEVMAP_FRONTIER_H

#include "devmap_region.h"
#include "host/region_contract.h"

namespace la3dm_dev {

struct FrontierArgs {
    uint32_t nx, ny, nz;          // the region
    uint32_t PY, PZ;              // padded extents along y and z
    uint32_t total;               // padded voxels PX PY PZ <= 2^28
    uint32_t n_words;             // ceil(total / 32)
    uint32_t min_neighbours;
    uint32_t *open;               // [n_words] open stream, the frontier words after dm_fr_stencil
    const uint32_t *unknown;      // [n_words]
    uint32_t *count;              // [n_words + 1] popcount per frontier word, then 0
    const uint32_t *offset;       // [n_words + 1] their exclusive prefixes; the last is the total
    uint64_t cap;
    uint32_t *index;              // [cap]
    uint8_t *nbrs;                // [cap] or null
    uint8_t *score;               // [nx ny nz] or null
};

// ---- stage 1: the two bit streams --------------------------------------------------------------------------------
// `a` describes the padded box (g0 one below the region's, dims + 2).  The grid covers whole waves: lanes beyond
// a.total vote 0, so the bits past the end of the last word are clear.
__global__ __launch_bounds__(256) void dm_fr_bits(RegionArgs a, uint32_t open_mask, uint32_t unknown_mask, uint32_t *open,
                                                  uint32_t *unknown) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;   // total <= 2^28: no overflow
    uint32_t cls = kClsMissing;
    const bool in = p < a.total;
    bool inner = false;
    if (in) {
        const uint32_t k = p % a.nz, row = p / a.nz;
        const uint32_t i = row / a.ny, j = row % a.ny;
        inner = k >= 1u && k + 1u < a.nz && j >= 1u && j + 1u < a.ny && i >= 1u && i + 1u < a.nx;
        cls = pool_class_at(a.pool, a.g0[0] + i, a.g0[1] + j, a.g0[2] + k);
    }
    pool_store_ballot(open, p, a.total, inner && ((open_mask >> cls) & 1u));
    pool_store_ballot(unknown, p, a.total, in && ((unknown_mask >> cls) & 1u));
}

// ---- the stencil of one word --------------------------------------------------------------------------------------
constexpr uint32_t kFrPlanes = 5;   // counts up to 26

// bits [b, b + 32) of the unknown stream; words outside the stream read 0 (only pad cells can ask for them)
__device__ __forceinline__ uint32_t fr_window(const uint32_t *__restrict__ u, uint32_t n_words, int b) {
    const int w = b >> 5;   // floor, also for b < 0
    const uint32_t lo = (uint32_t)w < n_words ? u[w] : 0u, hi = (uint32_t)(w + 1) < n_words ? u[w + 1] : 0u;
    return (uint32_t)(((((unsigned long long)hi) << 32) | lo) >> ((uint32_t)b & 31u));
}

// planes[q] bit b = bit q of the number of neighbours (connectivity kConn) of padded voxel 32 w + b in the unknown stream
template <int kConn>
__device__ __forceinline__ void fr_count(const FrontierArgs &a, uint32_t w, uint32_t planes[kFrPlanes]) {
#pragma unroll
    for (uint32_t q = 0; q < kFrPlanes; ++q) planes[q] = 0u;
    const int base = (int)(w << 5), sy = (int)a.PZ, sx = (int)(a.PY * a.PZ);
#pragma unroll
    for (int di = -1; di <= 1; ++di)
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
            for (int dk = -1; dk <= 1; ++dk) {
                const int manhattan = (di ? 1 : 0) + (dj ? 1 : 0) + (dk ? 1 : 0);
                if (manhattan == 0 || manhattan > la3dm_region::move_reach(kConn)) continue;
                uint32_t carry = fr_window(a.unknown, a.n_words, base + di * sx + dj * sy + dk);
#pragma unroll
                for (uint32_t q = 0; q < kFrPlanes; ++q) {   // a chain of half adders
                    const uint32_t t = planes[q] & carry;
                    planes[q] ^= carry;
                    carry = t;
                }
            }
}

// bit b set where the bit-sliced count of voxel b is >= m (m < 32)
__device__ __forceinline__ uint32_t fr_at_least(const uint32_t planes[kFrPlanes], uint32_t m) {
    uint32_t ge = 0u, eq = 0xFFFFFFFFu;
#pragma unroll
    for (int q = (int)kFrPlanes - 1; q >= 0; --q) {
        if ((m >> q) & 1u) {
            eq &= planes[q];
        } else {
            ge |= eq & planes[q];
            eq &= ~planes[q];
        }
    }
    return ge | eq;
}

__device__ __forceinline__ uint32_t fr_count_of(const uint32_t planes[kFrPlanes], uint32_t b) {
    uint32_t c = 0u;
#pragma unroll
    for (uint32_t q = 0; q < kFrPlanes; ++q) c |= ((planes[q] >> b) & 1u) << q;
    return c;
}

// flat index in the region of an inner padded voxel p
__device__ __forceinline__ uint32_t fr_unpadded(const FrontierArgs &a, uint32_t p) {
    const uint32_t k = p % a.PZ, row = p / a.PZ;
    const uint32_t j = row % a.PY, i = row / a.PY;
    return ((i - 1u) * a.ny + (j - 1u)) * a.nz + (k - 1u);
}

// ---- stage 2: stencil ----------------------------------------------------------------------------------------------
template <int kConn>
__global__ __launch_bounds__(256) void dm_fr_stencil(FrontierArgs a) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w > a.n_words) return;
    if (w == a.n_words) {   // the extra element of the scan: its prefix is the total
        a.count[w] = 0u;
        return;
    }
    const uint32_t open = a.open[w];
    if (open == 0u) {
        a.count[w] = 0u;
        return;
    }
    uint32_t planes[kFrPlanes];
    fr_count<kConn>(a, w, planes);
    const uint32_t front = open & fr_at_least(planes, a.min_neighbours);
    a.open[w] = front;
    a.count[w] = (uint32_t)__builtin_popcount(front);
    if (a.score) {
        uint32_t rest = open;
        while (rest) {   // at most 32 trips
            const uint32_t b = (uint32_t)__builtin_ctz(rest);
            rest &= rest - 1u;
            const uint32_t c = fr_count_of(planes, b);
            if (c) a.score[fr_unpadded(a, (w << 5) + b)] = (uint8_t)c;
        }
    }
}

// ---- stage 3: emit ---------------------------------------------------------------------------------------------------
template <int kConn>
__global__ __launch_bounds__(256) void dm_fr_emit(FrontierArgs a) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= a.n_words) return;
    uint32_t rest = a.open[w];
    if (rest == 0u) return;
    unsigned long long t = a.offset[w];
    if (t >= a.cap) return;
    uint32_t planes[kFrPlanes];
    if (a.nbrs) fr_count<kConn>(a, w, planes);
    while (rest && t < a.cap) {   // at most 32 trips
        const uint32_t b = (uint32_t)__builtin_ctz(rest);
        rest &= rest - 1u;
        a.index[t] = fr_unpadded(a, (w << 5) + b);
        if (a.nbrs) a.nbrs[t] = (uint8_t)fr_count_of(planes, b);
        ++t;
    }
}

// ---- the empty map with MISSING in both masks: every voxel is a frontier voxel, the list is 0, 1, 2, ... ---------------
__global__ __launch_bounds__(256) void dm_fr_all(uint32_t *index, uint8_t *nbrs, uint32_t n, uint32_t connectivity) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    index[t] = t;
    if (nbrs) nbrs[t] = (uint8_t)connectivity;
}

}  // namespace la3dm_dev

#endif
