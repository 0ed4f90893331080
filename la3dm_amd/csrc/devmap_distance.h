// devmap_distance.h — exact Euclidean distance transform of a map region on the device-resident block pool
// (la3dm_devmap_distance_*, include/la3dm_hip.h; host twin and definition: BGKOctoMap::distance_field,
// host/bgkoctomap.cpp).  Squared distances in voxel units are integers, so every stage is integer arithmetic and the
// result equals the host form bit for bit.
//
// The transform is separable.  D(v) = min over obstacles o of |v - o|^2 splits into a 1-D distance along z followed by
// min-plus passes along y and x; a window of +-radius per pass loses nothing (if D(v) <= radius^2 every axis offset to the
// minimiser is <= radius, anything larger is FAR at the end).  A z distance saturates at radius + 1: a partial sum that
// holds a saturated term exceeds radius^2 and can only end as FAR.
//
// dm_df_bits   one obstacle bit per voxel, straight from the pool (the class of the covering leaf is never stored): a
//              thread resolves one voxel of the flat (i, j, k) index as dm_box does, the wave's ballot is written as two
//              32-bit words.  1/8 byte per voxel.
// dm_df_z      per voxel the distance to the nearest set bit of its own z line within +-radius, by count-trailing /
//              count-leading zeros over at most radius / 32 + 2 words per side; written as 16 bits.
// dm_df_pass   one min-plus pass along an axis of length L whose elements lie `S` apart (y: L = ny, S = nz, one such
//              plane per i; x: L = nx, S = ny nz).  Lanes run along the S contiguous elements (k fastest), so global loads
//              and stores of a wave are 64 consecutive elements and LDS accesses of consecutive lanes hit consecutive
//              words.  A workgroup owns kDfRows consecutive rows of the line x 64 lanes; with kLds it stages those rows
//              plus a halo of `radius` rows on either side (clipped to the line) in LDS, otherwise — a halo that does
//              not fit kDfLdsBytes — it reads the neighbours from global memory / L2.  A wave takes its 8 rows together:
//              all lanes step the same offset d, the 16 reads of an offset are independent (indices clamped, no branch),
//              and a lane stops once d^2 >= the largest best of its 8 rows.  The last pass writes d2 and / or dist itself.
//
// Every loop is bounded by an argument or by the table size / depth: dims, radius, the probe count, the climb.
#ifndef LA3DM_DEVMAP_DISTANCE_H
#define LA3DM_DEVMAP_DISTANCE_H

#include "devmap_region.h"

namespace la3dm_dev {

constexpr uint32_t kDfRows = 32;              // rows of a line per workgroup
constexpr uint32_t kDfWaveRows = kDfRows / 4; // consecutive rows per wave, all in flight together
constexpr uint32_t kDfLdsBytes = 64u << 10;   // staging limit of dm_df_pass<.., true>

// The obstacle field a query on top of distance_field sees (reach, travel, score_poses, score_paths), as a kernel argument:
// the transform's d2 words by flat voxel index, or — d2 null — the same word `fill` at every voxel.  That is LA3DM_DF_FAR
// where the query asked for no transform (radius 0), and the empty map's uniform answer, 0 or FAR, of which no transform
// runs.  Built in one place, obstacle_field (devmap.hip).
struct ObstacleField {
    const uint32_t *d2;   // [nx ny nz] or null
    uint32_t fill;
    __device__ __forceinline__ uint32_t at(uint32_t f) const { return d2 ? d2[f] : fill; }
};

// ---- stage 1: obstacle bits ------------------------------------------------------------------------------------
// a.total voxels -> ceil(total / 32) words; bit f of the stream = voxel f is an obstacle.  The grid covers whole waves:
// lanes beyond `total` vote 0, so the bits past the end of the last word are clear.
__global__ __launch_bounds__(256) void dm_df_bits(RegionArgs a, uint32_t obstacle_mask, uint32_t *bits) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;   // total <= 2^28: no overflow
    uint32_t cls = kClsMissing;
    if (f < a.total) {
        const uint32_t k = f % a.nz, row = f / a.nz;
        cls = pool_class_at(a.pool, a.g0[0] + row / a.ny, a.g0[1] + row % a.ny, a.g0[2] + k);
    }
    pool_store_ballot(bits, f, a.total, f < a.total && ((obstacle_mask >> cls) & 1u));
}

// ---- stage 2: distance along z ---------------------------------------------------------------------------------
// fz[f] = min(|k - k'| : voxel (i, j, k') of the same line is an obstacle, |k - k'| <= radius), radius + 1 if none
__global__ __launch_bounds__(256) void dm_df_z(const uint32_t *__restrict__ bits, uint16_t *__restrict__ fz, uint32_t total,
                                               uint32_t nz, uint32_t radius) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= total) return;
    const uint32_t k = f % nz;
    const uint32_t lo = f - min(k, radius), hi = f + min(nz - 1u - k, radius);   // the window, clipped to the line
    uint32_t best = radius + 1u;
    uint32_t w = f >> 5, word = bits[w] & (0xFFFFFFFFu << (f & 31u));
    for (;;) {   // upwards: at most radius / 32 + 2 words
        if (word) {
            const uint32_t p = (w << 5) + (uint32_t)__builtin_ctz(word);
            if (p <= hi) best = p - f;
            break;
        }
        if (++w > (hi >> 5)) break;
        word = bits[w];
    }
    w = f >> 5;
    word = bits[w] & (0xFFFFFFFFu >> (31u - (f & 31u)));
    for (;;) {   // downwards
        if (word) {
            const uint32_t p = (w << 5) + 31u - (uint32_t)__builtin_clz(word);
            if (p >= lo) best = min(best, f - p);
            break;
        }
        if (w == (lo >> 5)) break;
        word = bits[--w];
    }
    fz[f] = (uint16_t)best;
}

// ---- stages 3 and 4: min-plus passes along y and x ---------------------------------------------------------------
struct DfPassArgs {
    const void *in;       // uint16 z distances (squared on read) or uint32 partial sums
    uint32_t *out;        // partial sums (not the last pass)
    uint32_t *d2;         // the last pass: either may be null
    float *dist;
    uint32_t L, S;        // line length, distance between its elements (= contiguous elements per row)
    uint32_t n_lt, n_ct;  // tiles per line, tiles per row
    uint32_t radius, r2;
    uint32_t last;
    float resolution;
};

template <typename TIn>
__device__ __forceinline__ uint32_t df_term(TIn v) {
    return sizeof(TIn) == 2 ? (uint32_t)v * (uint32_t)v : (uint32_t)v;
}

template <typename TIn, bool kLds>
__global__ __launch_bounds__(256) void dm_df_pass(DfPassArgs a) {
    extern __shared__ __align__(16) unsigned char df_lds[];
    TIn *tile = (TIn *)df_lds;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t ct = blockIdx.x % a.n_ct, rest = blockIdx.x / a.n_ct;
    const uint32_t lt = rest % a.n_lt, plane = rest / a.n_lt;
    const uint32_t c = ct * 64u + lane;
    const bool in = c < a.S;
    const uint32_t l0 = lt * kDfRows, l1 = min(l0 + kDfRows, a.L);
    const uint32_t first = l0 - min(l0, a.radius), end = min(l1 + a.radius, a.L);   // the staged rows [first, end)
    const TIn *src = (const TIn *)a.in + (size_t)plane * a.L * a.S + c;            // element (plane, 0, c)
    if (kLds) {
        for (uint32_t row = first + wave; row < end; row += 4u)
            if (in) tile[(row - first) * 64u + lane] = src[(size_t)row * a.S];
        __syncthreads();
    }
    const uint32_t lw = l0 + wave * kDfWaveRows;   // the wave's rows [lw, lw + kDfWaveRows) of the tile, taken together
    if (!in || lw >= l1) return;
    const auto term = [&](uint32_t row) -> uint32_t {
        return df_term<TIn>(kLds ? tile[(row - first) * 64u + lane] : src[(size_t)row * a.S]);
    };
    // A row index past the tile is clamped to its last row: computed again, stored by nobody.  A neighbour index off the
    // line is replaced by the row itself, whose term + d^2 cannot lower `best` (best <= the row's own term): no branch.
    uint32_t rr[kDfWaveRows], best[kDfWaveRows], worst = 0;
#pragma unroll
    for (uint32_t r = 0; r < kDfWaveRows; ++r) {
        rr[r] = min(lw + r, l1 - 1u);
        best[r] = term(rr[r]);
        worst = max(worst, best[r]);
    }
    for (uint32_t d = 1; d <= a.radius && d * d < worst; ++d) {   // the reads of an offset are independent: in flight together
        uint32_t lo_t[kDfWaveRows], hi_t[kDfWaveRows];
#pragma unroll
        for (uint32_t r = 0; r < kDfWaveRows; ++r) {
            lo_t[r] = term(rr[r] >= d ? rr[r] - d : rr[r]);
            hi_t[r] = term(rr[r] + d < a.L ? rr[r] + d : rr[r]);
        }
        worst = 0;
#pragma unroll
        for (uint32_t r = 0; r < kDfWaveRows; ++r) {
            best[r] = min(best[r], min(lo_t[r], hi_t[r]) + d * d);
            worst = max(worst, best[r]);
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < kDfWaveRows; ++r) {
        if (lw + r >= l1) break;
        const size_t o = ((size_t)plane * a.L + lw + r) * a.S + c;
        if (!a.last) {
            a.out[o] = best[r];
            continue;
        }
        const bool far = best[r] > a.r2;
        if (a.d2) a.d2[o] = far ? LA3DM_DF_FAR : best[r];
        // the correctly rounded fp32 root: the double root of an integer below 2^24 lies further than 2^-49 (relative) from
        // every midpoint of two floats, so rounding it once more gives what sqrtf gives on the host
        if (a.dist) a.dist[o] = far ? __builtin_inff() : (float)sqrt((double)best[r]) * a.resolution;
    }
}

}  // namespace la3dm_dev

#endif
