// devmap_footing.h — footing of a map region on the device-resident block pool: the voxels on which a ground robot can
// stand — ground below, headroom above, a footprint that is carried, not blocked and climbable — as an ordered list and
// per column (la3dm_devmap_footing_*, include/la3dm_hip.h; host twin and definition: host/footing_cells.h, called by
// BGKOctoMap::footing).  Integer arithmetic on classes throughout: the result equals the host form exactly.
//
// Everything runs on bit streams over the PADDED box (PX, PY, PZ) = (nx + 2r, ny + 2r, nz + h + 2s), 32 voxels per word,
// z fastest: region voxel (i, j, k) is padded voxel (i + r, j + r, k + 1 + s), bit p = (pi PY + pj) PZ + pz.  A vertical
// neighbour of bit p is bit p + dk — a shift —, a horizontal one bit p + di PY PZ + dj PZ — a word offset and a funnel
// shift (ft_window, devmap_frontier.h's fr_window).  A window that runs past the end of a padded column reads the next
// column's cells: stand is right only at pz in [1, PZ - h], near and body only at the region's own pz in [1 + s, nz + s].
// No bit outside those ranges is ever used: near reads stand at pz -+ s, which stays inside [1, nz + 2s] = [1, PZ - h], and
// the last pass keeps only the bits of the region's interior (ft_interior) of the stand words it starts from.
//
// dm_ft_bits     one probe per padded voxel (pool_class_at), two ballots: the SUPPORT stream and the CLEAR stream.  The
//                only pass that touches the pool.
// dm_ft_derive   one lane per word.  run(c, n) = the AND of n consecutive windows of the clear stream, by doubling; stand =
//                support one bit below AND run(clear, h), for the lane's word and the two beside it, so that near = the OR
//                of the stand windows at -s .. +s needs no second launch; body = run(clear from bit s, h - s).  Stores
//                stand masked to the region's interior (the candidates), near and body.
// dm_ft_foot     a fixed number of waves, each over a strided share of the candidate words.  A word of zeros costs a load
//                (nearly all on a scanned map: the floor is a thin sheet).  For a word that holds a standing voxel the 64
//                lanes take one cell each of the square round the disc: the AND of the body windows over the disc, with
//                an early-out at 0; then the near windows added into bit-sliced counters (bit b of plane q = bit q of the count of voxel b), the lanes'
//                counters summed in a butterfly of full adders into kFtPlanes planes (8 hold N <= 196) and compared with
//                min_support.  The candidate word is replaced IN PLACE by the foot word; its popcount goes to the
//                compaction's input; a wave stores its three counts (stand, body, foot) once, and the host adds them up.
// (scan)         devmap.hip's exclusive_scan over n_words + 1 popcounts: the prefix of the extra element is the total.
// dm_ft_emit     one lane per word; each set bit becomes the region's flat index at its place in the list, until cap.
// dm_ft_columns  one lane per column of the region: its nz bits are contiguous in the stream; levels, lowest and highest
//                are popcount, ctz and clz over the words they overlap.
//
// Working storage: support, clear, candidates / foot, near, body, popcounts, prefixes — 7 words per 32 padded voxels — and
// 3 kFtWaves words of partial counts.
//
// The rules of this code base, followed here: no array indexed at run time (the planes are a fixed array whose every
// index is a constant after unrolling); every loop is bounded by an argument (h, r, s, nz) or a constant (32 bits of a
// word, 17 column pieces of a word, 5 rounds of 64 footprint cells, 64 words of a wave's round); no atomic at all — the
// per-wave counts are stored, not added —; no slot of the map's counter block; no mirror refresh.
#ifndef LA3DM_DEVMAP_FOOTING_H
#define LA3DM_DEVMAP_FOOTING_H

#include "devmap_region.h"

namespace la3dm_dev {

struct FootingArgs {
    uint32_t nx, ny, nz;          // the region
    uint32_t PY, PZ;              // padded extents along y and z
    uint32_t h, r, s, c;          // headroom, radius, step, min_support
    uint32_t total;               // padded voxels PX PY PZ <= 2^28
    uint32_t n_words;             // ceil(total / 32)
    const uint32_t *support;      // [n_words]
    const uint32_t *clear;        // [n_words]
    uint32_t *stand;              // [n_words] candidates, the foot words after dm_ft_foot
    uint32_t *near;               // [n_words]
    uint32_t *body;               // [n_words]
    uint32_t *count;              // [n_words + 1] popcount per foot word, then 0
    const uint32_t *offset;       // [n_words + 1] their exclusive prefixes; the last is the total
    uint32_t *stats;              // [3 kFtWaves] n_stand, n_body, n_foot per wave of dm_ft_foot
    uint64_t cap;
    uint32_t *index;              // [cap]
    uint32_t *levels;             // [nx ny] or null
    int32_t *lowest, *highest;    // [nx ny] or null
};

// ---- stage 1: the two bit streams ---------------------------------------------------------------------------------
// `a` describes the padded box.  The grid covers whole waves: lanes beyond a.total vote 0, so the bits past the end of
// the last word are clear.
__global__ __launch_bounds__(256) void dm_ft_bits(RegionArgs a, uint32_t support_mask, uint32_t clear_mask, uint32_t *support,
                                                  uint32_t *clear) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;   // total <= 2^28: no overflow
    uint32_t cls = kClsMissing;
    const bool in = p < a.total;
    if (in) {
        const uint32_t k = p % a.nz, row = p / a.nz;
        const uint32_t i = row / a.ny, j = row % a.ny;
        cls = pool_class_at(a.pool, a.g0[0] + i, a.g0[1] + j, a.g0[2] + k);
    }
    pool_store_ballot(support, p, a.total, in && ((support_mask >> cls) & 1u));
    pool_store_ballot(clear, p, a.total, in && ((clear_mask >> cls) & 1u));
}

// ---- words and windows ---------------------------------------------------------------------------------------------
// word w of a stream; words outside it read 0
__device__ __forceinline__ uint32_t ft_word(const uint32_t *__restrict__ u, uint32_t n_words, int w) {
    return (uint32_t)w < n_words ? u[w] : 0u;
}

// bits [b, b + 32) of a stream
__device__ __forceinline__ uint32_t ft_window(const uint32_t *__restrict__ u, uint32_t n_words, int b) {
    const int w = b >> 5;   // floor, also for b < 0
    const uint32_t lo = ft_word(u, n_words, w), hi = ft_word(u, n_words, w + 1);
    return (uint32_t)(((((unsigned long long)hi) << 32) | lo) >> ((uint32_t)b & 31u));
}

// bit b of the result, b < 32 = the AND of bits b .. b + n - 1 of c, 1 <= n <= 32 (b + n - 1 <= 62: bit 63 is not read)
__device__ __forceinline__ uint32_t ft_run(unsigned long long c, uint32_t n) {
    uint32_t len = 1u;
#pragma unroll
    for (int t = 0; t < 5; ++t)   // doubling: runs of 2, 4, 8, 16, 32 while they fit n
        if (2u * len <= n) {
            c &= c >> len;
            len *= 2u;
        }
    c &= c >> (n - len);   // n - len < len <= 32
    return (uint32_t)c;
}

// stand of the 32 voxels of word w (right at pz in [1, PZ - h])
__device__ __forceinline__ uint32_t ft_stand(const FootingArgs &a, int w) {
    const uint32_t below = (ft_word(a.support, a.n_words, w) << 1) | (ft_word(a.support, a.n_words, w - 1) >> 31);
    if (below == 0u) return 0u;
    const unsigned long long c = (((unsigned long long)ft_word(a.clear, a.n_words, w + 1)) << 32) | ft_word(a.clear, a.n_words, w);
    return below & ft_run(c, a.h);
}

// the bits of word w of a stream over a padded box (., PY, PZ) that belong to the region (nx, ny, nz) which starts pad_xy
// voxels inside the box in x and y and pad_z in z: pz in [pad_z, nz + pad_z), pj in [pad_xy, ny + pad_xy), pi in [pad_xy,
// nx + pad_xy).  A word overlaps at most 32 / PZ + 2 <= 17 padded columns (PZ >= 2).  (devmap_surface.h uses it as well.)
__device__ __forceinline__ uint32_t ft_interior_bits(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t PY, uint32_t PZ, uint32_t pad_xy,
                                                     uint32_t pad_z, uint32_t w) {
    uint32_t mask = 0u;
    const uint32_t first = w << 5;
    uint32_t col = first / PZ, z0 = first % PZ;   // the column of bit 0 and where in it the bit lies
    int at = -(int)z0;                            // the bit of the word at which column `col` starts
#pragma unroll 1
    for (int piece = 0; piece < 17; ++piece) {
        if (at >= 32) break;
        const uint32_t pi = col / PY, pj = col % PY;
        if (pi >= pad_xy && pi < nx + pad_xy && pj >= pad_xy && pj < ny + pad_xy) {
            const int lo = at + (int)pad_z, hi = lo + (int)nz;   // bits [lo, hi) of the word
            const int from = lo < 0 ? 0 : lo, to = hi > 32 ? 32 : hi;
            if (from < to) mask |= (to - from == 32 ? 0xFFFFFFFFu : ((1u << (to - from)) - 1u) << from);
        }
        ++col;
        at += (int)PZ;
    }
    return mask;
}

// footing's own interior: pz in [1 + s, nz + s], pj in [r, ny + r), pi in [r, nx + r)
__device__ __forceinline__ uint32_t ft_interior(const FootingArgs &a, uint32_t w) {
    return ft_interior_bits(a.nx, a.ny, a.nz, a.PY, a.PZ, a.r, 1u + a.s, w);
}

// the sum of v over the wave, in lane 0
__device__ __forceinline__ uint32_t ft_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// ---- stage 2: stand, near, body -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dm_ft_derive(FootingArgs a) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= a.n_words) return;
    const int iw = (int)w;
    const uint32_t mid = ft_stand(a, iw);
    uint32_t near = mid;
    if (a.s) {
        const uint32_t left = ft_stand(a, iw - 1), right = ft_stand(a, iw + 1);
#pragma unroll 1
        for (uint32_t dk = 1; dk <= a.s; ++dk)   // s <= 4
            near |= (mid << dk) | (left >> (32u - dk)) | (mid >> dk) | (right << (32u - dk));
    }
    const unsigned long long c = (((unsigned long long)ft_word(a.clear, a.n_words, iw + 1)) << 32) | a.clear[w];
    a.near[w] = near;
    a.body[w] = ft_run(c >> a.s, a.h - a.s);
    a.stand[w] = mid ? mid & ft_interior(a, w) : 0u;
}

// ---- stage 3: the footprint -------------------------------------------------------------------------------------------
constexpr uint32_t kFtPlanes = 8;   // counts up to 255 >= N(8) = 196

// bit b set where the bit-sliced count of voxel b is >= m (m < 256)
__device__ __forceinline__ uint32_t ft_at_least(const uint32_t planes[kFtPlanes], uint32_t m) {
    uint32_t ge = 0u, eq = 0xFFFFFFFFu;
#pragma unroll
    for (int q = (int)kFtPlanes - 1; q >= 0; --q) {
        if ((m >> q) & 1u) {
            eq &= planes[q];
        } else {
            ge |= eq & planes[q];
            eq &= ~planes[q];
        }
    }
    return ge | eq;
}

// planes += the planes of lane ^ d, bit-sliced: both terms fit kP planes, the sum kP + 1 (at most kN, the planes there
// are: N < 256 here; devmap_surface.h sums up to 729 in 10)
template <int kP, int kN = (int)kFtPlanes>
__device__ __forceinline__ void ft_fold(uint32_t *planes, int d) {
    uint32_t carry = 0u;
#pragma unroll
    for (int q = 0; q < kN; ++q) {
        if (q < kP) {   // a full adder per plane
            const uint32_t other = __shfl_xor(planes[q], d, 64);
            const uint32_t x = planes[q] ^ other;
            const uint32_t both = planes[q] & other;
            planes[q] = x ^ carry;
            carry = both | (carry & x);
        } else if (q == kP) {
            planes[q] = carry;
        }
    }
}

// kFtWaves waves, whatever the region; word w belongs to wave w % kFtWaves, so the words of a patch of floor — neighbours
// in the stream — go to different waves.  A wave loads 64 of its words at a time, one per lane, and takes those that hold
// a standing voxel one after the other, its 64 lanes one cell each of the (2r + 1)^2 square round the voxel (at most 289
// cells: 5 rounds): the windows of a word are loaded side by side.  It ends with one store of its three counts; the
// host adds the kFtWaves partial counts.  Three other forms were measured and dropped: one lane per
// word reads its 2 N windows one after the other; one wave per 16 consecutive words takes the words of a patch of floor
// one after the other; one wave per word needs an atomic per word for the counts.
constexpr uint32_t kFtWaves = 2048;

__global__ __launch_bounds__(256) void dm_ft_foot(FootingArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6);   // the wave, < kFtWaves
    const int sy = (int)a.PZ, sx = (int)(a.PY * a.PZ), r = (int)a.r, r2 = r * r, side = 2 * r + 1, cells = side * side;
    uint32_t n_stand = 0u, n_body = 0u, n_foot = 0u;
#pragma unroll 1
    for (uint32_t w0 = g; w0 <= a.n_words; w0 += 64u * kFtWaves) {   // everything in here but `mine` is uniform over the wave
        const uint32_t w = w0 + lane * kFtWaves;
        uint32_t mine = w < a.n_words ? a.stand[w] : 0u;
        n_stand += (uint32_t)__builtin_popcount(mine);
        unsigned long long todo = __ballot(mine != 0u);
        while (todo) {   // at most 64 trips
            const int t = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            uint32_t cand = __shfl(mine, t, 64);
            const int base = (int)((w0 + (uint32_t)t * kFtWaves) << 5);
            uint32_t clear = 0xFFFFFFFFu;   // the AND of this lane's body windows
#pragma unroll 1
            for (int q0 = 0; q0 < cells; q0 += 64) {   // at most 5 rounds
                const int q = q0 + (int)lane, di = q / side - r, dj = q % side - r;
                if (q < cells && (di | dj) != 0 && di * di + dj * dj <= r2) clear &= ft_window(a.body, a.n_words, base + di * sx + dj * sy);
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) clear &= __shfl_xor(clear, d, 64);
            cand &= clear;
            if ((int)lane == t) n_body += (uint32_t)__builtin_popcount(cand);
            if (cand && a.c) {   // the early-out at 0, and min_support = 0 asks for no count
                uint32_t planes[kFtPlanes];
#pragma unroll
                for (uint32_t q = 0; q < kFtPlanes; ++q) planes[q] = 0u;
#pragma unroll 1
                for (int q0 = 0; q0 < cells; q0 += 64) {
                    const int q = q0 + (int)lane, di = q / side - r, dj = q % side - r;
                    uint32_t carry = 0u;
                    if (q < cells && (di | dj) != 0 && di * di + dj * dj <= r2) carry = ft_window(a.near, a.n_words, base + di * sx + dj * sy);
#pragma unroll
                    for (uint32_t p = 0; p < 3u; ++p) {   // a chain of half adders: a lane adds at most 5 windows
                        const uint32_t both = planes[p] & carry;
                        planes[p] ^= carry;
                        carry = both;
                    }
                }
                ft_fold<3>(planes, 1);   // the lanes' counts summed in a butterfly: every lane ends with the total
                ft_fold<4>(planes, 2);
                ft_fold<5>(planes, 4);
                ft_fold<6>(planes, 8);
                ft_fold<7>(planes, 16);
                ft_fold<8>(planes, 32);
                cand &= ft_at_least(planes, a.c);
            }
            if ((int)lane == t) mine = cand;
        }
        const uint32_t found = (uint32_t)__builtin_popcount(mine);
        n_foot += found;
        if (w < a.n_words) a.stand[w] = mine;
        if (w <= a.n_words) a.count[w] = found;   // (the extra element of the scan is 0: its prefix is the total)
    }
    const uint32_t t_stand = ft_wave_sum(n_stand), t_body = ft_wave_sum(n_body), t_foot = ft_wave_sum(n_foot);
    if (lane == 0u) {
        a.stats[3u * g + 0u] = t_stand;
        a.stats[3u * g + 1u] = t_body;
        a.stats[3u * g + 2u] = t_foot;
    }
}

// ---- stage 4: emit -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dm_ft_emit(FootingArgs a) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= a.n_words) return;
    uint32_t rest = a.stand[w];
    if (rest == 0u) return;
    unsigned long long t = a.offset[w];
    while (rest && t < a.cap) {   // at most 32 trips
        const uint32_t b = (uint32_t)__builtin_ctz(rest);
        rest &= rest - 1u;
        const uint32_t p = (w << 5) + b;   // an interior bit
        const uint32_t pz = p % a.PZ, row = p / a.PZ;
        const uint32_t pj = row % a.PY, pi = row / a.PY;
        a.index[t] = ((pi - a.r) * a.ny + (pj - a.r)) * a.nz + (pz - 1u - a.s);
        ++t;
    }
}

// ---- stage 5: the columns ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dm_ft_columns(FootingArgs a) {
    const uint32_t col = blockIdx.x * 256u + threadIdx.x;
    if (col >= a.nx * a.ny) return;
    const uint32_t i = col / a.ny, j = col % a.ny;
    const uint32_t p0 = ((i + a.r) * a.PY + (j + a.r)) * a.PZ + 1u + a.s, p1 = p0 + a.nz;   // the column's bits [p0, p1)
    uint32_t levels = 0u;
    int32_t low = -1, top = -1;
    const uint32_t w1 = (p1 - 1u) >> 5;
#pragma unroll 1
    for (uint32_t w = p0 >> 5; w <= w1; ++w) {   // at most nz / 32 + 2 words
        const uint32_t first = w << 5;
        const uint32_t from = p0 > first ? p0 - first : 0u, to = p1 < first + 32u ? p1 - first : 32u;
        const uint32_t mask = (to - from == 32u ? 0xFFFFFFFFu : ((1u << (to - from)) - 1u) << from);
        const uint32_t bits = a.stand[w] & mask;
        if (bits == 0u) continue;
        levels += (uint32_t)__builtin_popcount(bits);
        if (low < 0) low = (int32_t)(first + (uint32_t)__builtin_ctz(bits) - p0);
        top = (int32_t)(first + 31u - (uint32_t)__builtin_clz(bits) - p0);
    }
    if (a.levels) a.levels[col] = levels;
    if (a.lowest) a.lowest[col] = low;
    if (a.highest) a.highest[col] = top;
}

}  // namespace la3dm_dev

#endif
