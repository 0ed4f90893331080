// devmap_nearest.h — the feature transform of a map region on the device-resident block pool: which obstacle voxel is
// the nearest, per voxel (la3dm_devmap_nearest_*) and per point of a cloud (la3dm_devmap_nearest_points_*; contract:
// include/la3dm_hip.h; host twin and definition: BGKOctoMap::nearest / ::nearest_points, host/bgkoctomap.cpp over
// host/nearest_lines.h).  distance_field's separable stages (devmap_distance.h), each of which now keeps its argmin; the
// key arithmetic is nearest_lines.h's, compiled here as it is for the host form.  Everything is integers, so the result
// equals the host form exactly.
//
// dm_df_bits    distance_field's kernel, launched as it is: one obstacle bit per voxel.
// dm_nt_z       dm_df_z with the sign kept: per voxel the signed 16-bit offset k' - k to the nearest set bit of its own z
//               line within +-radius by count-trailing / count-leading zeros over the bit words, the lower k' on a tie;
//               radius + 1 where there is none (the saturated offset: its square is distance_field's saturated term).
// dm_nt_pass    one min-plus pass over the packed key (sum << 9) | (offset + 256), in the lane layout of dm_df_pass: 64
//               consecutive elements per wave, kDfRows rows of the line per workgroup, rows plus a halo of `radius` staged
//               in LDS where they fit kDfLdsBytes, a wave's 8 rows in flight together.  The plain min of two keys is the
//               tie-break (smaller sum, then smaller offset = smaller j' or i'): no branch.  A lane stops once d^2 exceeds
//               the largest best SUM of its rows — not at d^2 == sum, where dm_df_pass stops: with a term of 0 on the low
//               side that offset still wins the tie.  The clamp for a neighbour off the line (the row itself) cannot win:
//               its sum is the row's own term plus d^2.  <int16_t> is the y pass (z offsets in, keys out; ny = 1 runs it
//               over lines of length 1: one launch more, one code path fewer); <uint32_t> is the x pass and the last: it
//               follows i' = i + ax(i, j, k), j' = j + ay(i', j, k), k' = k + az(i', j', k) — two dependent gathers, the y
//               key and the z offset — and writes index and d2.
// dm_nt_points  one lane per point: the transform (or none), world_voxel, two gathers from nearest's answer in working
//               storage.  No atomic, no LDS.  index = null stands for the empty map: every voxel has the distance `fill`
//               (0: it is its own nearest obstacle; FAR: none), and the pool is not read.
// dm_nt_iota    index[v] = v: the empty map's answer to nearest with MISSING among the obstacles, device-pointer form.
//
// Every loop is bounded by an argument: dims, radius, the word count of a line's window.
#ifndef LA3DM_DEVMAP_NEAREST_H
#define LA3DM_DEVMAP_NEAREST_H

#include "devmap_distance.h"
#include "host/nearest_lines.h"
#include "host/region_contract.h"

namespace la3dm_dev {

// ---- z: the signed offset along z ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dm_nt_z(const uint32_t *__restrict__ bits, int16_t *__restrict__ az, uint32_t total, uint32_t nz,
                                               uint32_t radius) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= total) return;
    const uint32_t k = f % nz;
    const uint32_t lo = f - min(k, radius), hi = f + min(nz - 1u - k, radius);   // the window, clipped to the line
    uint32_t up = radius + 1u, down = radius + 1u;
    uint32_t w = f >> 5, word = bits[w] & (0xFFFFFFFFu << (f & 31u));
    for (;;) {   // upwards: at most radius / 32 + 2 words
        if (word) {
            const uint32_t p = (w << 5) + (uint32_t)__builtin_ctz(word);
            if (p <= hi) up = p - f;
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
            if (p >= lo) down = f - p;
            break;
        }
        if (w == (lo >> 5)) break;
        word = bits[--w];
    }
    // the lower k' on a tie; both saturated: none
    az[f] = (int16_t)(down <= up ? (down > radius ? (int)(radius + 1u) : -(int)down) : (int)up);
}

// ---- y and x: min-plus passes over packed keys ---------------------------------------------------------------------
struct NtPassArgs {
    const void *in;         // y pass: int16 z offsets; x pass: uint32 y keys
    uint32_t *keys;         // y pass: the keys out
    const int16_t *az;      // x pass: the z offsets, for the chase
    uint32_t *index, *d2;   // x pass: the outputs, either may be null
    uint32_t L, S;          // line length, distance between its elements (= contiguous elements per row)
    uint32_t n_lt, n_ct;    // tiles per line, tiles per row
    uint32_t radius, r2;
    uint32_t ny, nz;
};

template <typename TIn>
__device__ __forceinline__ uint32_t nt_term(TIn v) {
    return sizeof(TIn) == 2 ? la3dm_nearest::offset_term((int16_t)v) : la3dm_nearest::key_sum((uint32_t)v);
}

template <typename TIn, bool kLds>
__global__ __launch_bounds__(256) void dm_nt_pass(NtPassArgs a) {
    namespace nt = la3dm_nearest;
    constexpr bool kLast = sizeof(TIn) == 4;
    extern __shared__ __align__(16) unsigned char nt_lds[];
    TIn *tile = (TIn *)nt_lds;
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
        return nt_term<TIn>(kLds ? tile[(row - first) * 64u + lane] : src[(size_t)row * a.S]);
    };
    // A row index past the tile is clamped to its last row: computed again, stored by nobody.  A neighbour index off the
    // line is replaced by the row itself, whose sum (its own term + d^2) exceeds the best sum: it cannot win.
    uint32_t rr[kDfWaveRows], best[kDfWaveRows], worst = 0;
#pragma unroll
    for (uint32_t r = 0; r < kDfWaveRows; ++r) {
        rr[r] = min(lw + r, l1 - 1u);
        best[r] = nt::key_of(term(rr[r]), 0);
        worst = max(worst, best[r]);
    }
    for (uint32_t d = 1; d <= a.radius && d * d <= nt::key_sum(worst); ++d) {   // the reads of an offset are independent: in flight together
        uint32_t lo_t[kDfWaveRows], hi_t[kDfWaveRows];
#pragma unroll
        for (uint32_t r = 0; r < kDfWaveRows; ++r) {
            lo_t[r] = term(rr[r] >= d ? rr[r] - d : rr[r]);
            hi_t[r] = term(rr[r] + d < a.L ? rr[r] + d : rr[r]);
        }
        worst = 0;
#pragma unroll
        for (uint32_t r = 0; r < kDfWaveRows; ++r) {
            best[r] = min(best[r], min(nt::key_of(lo_t[r] + d * d, -(int)d), nt::key_of(hi_t[r] + d * d, (int)d)));
            worst = max(worst, best[r]);
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < kDfWaveRows; ++r) {
        if (lw + r >= l1) break;
        const uint32_t l = lw + r;
        const size_t o = ((size_t)plane * a.L + l) * a.S + c;
        if (!kLast) {
            a.keys[o] = best[r];
            continue;
        }
        // the x pass: plane = 0, l = i, c = j nz + k
        const uint32_t sum = nt::key_sum(best[r]);
        const bool far = sum > a.r2;
        if (a.d2) a.d2[o] = far ? LA3DM_DF_FAR : sum;
        if (!a.index) continue;
        uint32_t at = LA3DM_NEAREST_NONE;
        if (!far) {
            // (the offsets lead to voxels of the region by construction; the clamps keep a gather inside the arrays whatever
            // the keys hold)
            const uint32_t j = c / a.nz, k = c - j * a.nz;
            const uint32_t i2 = min((uint32_t)((int)l + nt::key_offset(best[r])), a.L - 1u);
            const uint32_t ykey = (uint32_t)src[(size_t)i2 * a.S];
            const uint32_t j2 = min((uint32_t)((int)j + nt::key_offset(ykey)), a.ny - 1u);
            const uint32_t line = (i2 * a.ny + j2) * a.nz;
            at = line + min((uint32_t)((int)k + (int)a.az[line + k]), a.nz - 1u);
        }
        a.index[o] = at;
    }
}

// ---- nearest_points -----------------------------------------------------------------------------------------------
struct NtPointsArgs {
    const float *points;     // 3 per point
    const float *pose;       // 12 floats or null: the points as they are
    uint32_t n_points;
    float resolution, block_size;
    int lim;                 // cells of a block per axis
    uint32_t g0[3], dims[3];
    const uint32_t *index;   // [nx ny nz] nearest's answer, or null: the empty map, d2 = `fill` everywhere
    const uint32_t *d2;
    uint32_t fill;
    uint8_t *o_cls;          // the outputs, each [n_points] or null
    uint32_t *o_voxel, *o_index, *o_d2;
};

__global__ __launch_bounds__(256) void dm_nt_points(NtPointsArgs a) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;   // n_points <= 2^20: no overflow
    if (p >= a.n_points) return;
    const float *q = a.points + 3 * (size_t)p;
    const float w[3] = {q[0], q[1], q[2]};
    uint32_t f = 0, cls;
    if (a.pose) {   // wave-uniform
        float T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = a.pose[k];
        cls = la3dm_region::score_voxel(T, w[0], w[1], w[2], a.resolution, a.block_size, a.lim, a.g0, a.dims, f);
    } else {
        cls = la3dm_region::world_voxel(w, a.resolution, a.block_size, a.lim, a.g0, a.dims, f);
    }
    const bool inside = cls == LA3DM_SCORE_HIT;
    uint32_t at = LA3DM_NEAREST_NONE, d2 = LA3DM_DF_FAR;
    if (inside) {
        d2 = a.index ? a.d2[f] : a.fill;
        at = a.index ? a.index[f] : (a.fill == 0u ? f : LA3DM_NEAREST_NONE);
        cls = la3dm_region::score_class(d2);
    }
    if (a.o_cls) a.o_cls[p] = (uint8_t)cls;
    if (a.o_voxel) a.o_voxel[p] = inside ? f : LA3DM_NEAREST_NONE;
    if (a.o_index) a.o_index[p] = at;
    if (a.o_d2) a.o_d2[p] = d2;
}

__global__ __launch_bounds__(256) void dm_nt_iota(uint32_t *index, uint32_t total) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f < total) index[f] = f;
}

}  // namespace la3dm_dev

#endif
