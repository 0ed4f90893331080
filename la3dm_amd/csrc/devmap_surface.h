// devmap_surface.h — surface of a map region on the device-resident block pool: the exposed faces of the solid voxels and
// an integer normal summed from them, as an ordered list and (the faces) per voxel (la3dm_devmap_surface_*,
// include/la3dm_hip.h; host twin and definition: host/surface_cells.h, called by BGKOctoMap::surface).  Integer arithmetic
// on classes throughout: the result equals the host form exactly.
//
// Everything runs on bit streams over the PADDED box (PX, PY, PZ) = (nx + 2p, ny + 2p, nz + 2p), p = smooth + 1, 32 voxels
// per word, z fastest: region voxel (i, j, k) is padded voxel (i + p, j + p, k + p), bit (pi PY + pj) PZ + pz.  A neighbour
// of bit b is bit b + di PY PZ + dj PZ + dk — a word offset and a funnel shift (ft_window).  A window that runs past the end
// of a padded column reads the next column's cells: a face word is right for the padded voxels one layer inside the box,
// and those are all that is ever used — the candidates are masked to the region, and the normal of a region voxel reads
// the faces of voxels at most smooth = p - 1 away.
//
// dm_ft_bits     footing's: one probe per padded voxel (pool_class_at), two ballots: the SOLID stream and the OPEN stream.
//                The only pass that touches the pool.
// dm_sf_faces    a fixed number of waves, a lane per word: the six face words = SOLID & the OPEN window at bit offsets
//                -+ PY PZ, -+ PZ, -+ 1; stored as six streams when the normals pass or the dense array needs them.  Their OR,
//                masked to the region (ft_interior_bits), is the candidate word; its popcount goes to the compaction's
//                input.  A wave stores its eight counts (solid, six directions, candidates) once, and the host adds them up.
// (scan)         devmap.hip's exclusive_scan over n_words + 1 popcounts: the prefix of the extra element is the total.
// dm_sf_emit     one lane per word; each set bit writes index and face mask at its place in the list, until cap — the face
//                words formed again, as frontier's emit counts again —, and with smooth = 0 the normal, which is the
//                voxel's own face vector.
// dm_sf_normals  (smooth > 0) a fixed number of waves, each over a strided share of the candidate words; a word of zeros
//                costs a load.  For a word that holds a surface voxel the lanes take the (2s + 1)^2 columns of the window
//                (at most 81: two rounds of 64), one axis at a time: a lane loads 64 bits of the axis' two face streams at
//                its columns from s bits below the word — twelve loads issued together —, adds the 2s + 1 shifted windows
//                into bit-sliced counters (bit b of plane q = bit q of the count of voxel b), the lanes' counters are
//                summed in a butterfly of full adders (footing's ft_fold) into 10 planes (729 < 1024), and the lanes of
//                the set bits store plus - minus.  A direction with no face in the whole window — most of them next to a
//                floor — skips its butterfly.  79 VGPRs, 6 waves per SIMD; the grid is two waves per SIMD.
// dm_sf_dense    one lane per voxel of the region: bit d of the byte from face stream d.
//
// Working storage: solid, open, six face streams, candidates, popcounts, prefixes — 11 words per 32 padded voxels — and
// 8 kSfWaves words of partial counts.
//
// The rules of this code base, followed here: no array indexed at run time (face words and planes are fixed arrays whose
// every index is a constant after unrolling); every loop is bounded by an argument (s) or a constant (32 bits of a word,
// 2 rounds of 64 columns, 64 words of a wave's round); no atomic at all; no slot of the map's counter block; no mirror
// refresh.
#ifndef LA3DM_DEVMAP_SURFACE_H
#define LA3DM_DEVMAP_SURFACE_H

#include "devmap_footing.h"

namespace la3dm_dev {

struct SurfaceArgs {
    uint32_t nx, ny, nz;          // the region
    uint32_t PY, PZ;              // padded extents along y and z
    uint32_t s, pad;              // smooth; pad = s + 1
    uint32_t total;               // padded voxels PX PY PZ <= 2^28
    uint32_t n_words;             // ceil(total / 32)
    uint32_t store_faces;         // the six face streams are wanted
    const uint32_t *solid;        // [n_words]
    const uint32_t *open;         // [n_words]
    uint32_t *face;               // six streams, `stride` words apart
    uint32_t stride;
    uint32_t *cand;               // [n_words] candidate words
    uint32_t *count;              // [n_words + 1] their popcounts, then 0
    const uint32_t *offset;       // [n_words + 1] their exclusive prefixes; the last is the total
    uint32_t *stats;              // [8 kSfWaves] solid, the six directions and the candidates per wave of dm_sf_faces
    uint64_t cap;
    uint32_t *index;              // [cap] or null
    uint8_t *faces;               // [cap] or null
    int16_t *normal;              // [3 cap] or null
    uint8_t *dense;               // [nx ny nz] or null
};

constexpr uint32_t kSfWaves = 2048;
constexpr int kSfPlanes = 10;   // counts up to 1023 >= 729

// the six face words of word w: f[d] bit b = F_d of padded voxel 32 w + b
__device__ __forceinline__ void sf_face_words(const SurfaceArgs &a, uint32_t w, uint32_t solid, uint32_t f[6]) {
    const int base = (int)(w << 5), sy = (int)a.PZ, sx = (int)(a.PY * a.PZ);   // base + 4 sx < 5 * 2^28: fits
    f[0] = solid & ft_window(a.open, a.n_words, base - sx);
    f[1] = solid & ft_window(a.open, a.n_words, base + sx);
    f[2] = solid & ft_window(a.open, a.n_words, base - sy);
    f[3] = solid & ft_window(a.open, a.n_words, base + sy);
    f[4] = solid & ft_window(a.open, a.n_words, base - 1);
    f[5] = solid & ft_window(a.open, a.n_words, base + 1);
}

// flat index in the region of a padded voxel of its interior
__device__ __forceinline__ uint32_t sf_unpadded(const SurfaceArgs &a, uint32_t p) {
    const uint32_t pz = p % a.PZ, row = p / a.PZ;
    const uint32_t pj = row % a.PY, pi = row / a.PY;
    return ((pi - a.pad) * a.ny + (pj - a.pad)) * a.nz + (pz - a.pad);
}

// ---- stage 2: faces, candidates, counts ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dm_sf_faces(SurfaceArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6);   // the wave, < kSfWaves
    uint32_t n_solid = 0u, n_cand = 0u, n0 = 0u, n1 = 0u, n2 = 0u, n3 = 0u, n4 = 0u, n5 = 0u;
#pragma unroll 1
    for (uint32_t w = g * 64u + lane; w <= a.n_words; w += 64u * kSfWaves) {
        uint32_t f[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        uint32_t cand = 0u;
        const uint32_t solid = w < a.n_words ? a.solid[w] : 0u;
        if (solid) {
            sf_face_words(a, w, solid, f);
            const uint32_t inner = ft_interior_bits(a.nx, a.ny, a.nz, a.PY, a.PZ, a.pad, a.pad, w);
            cand = (f[0] | f[1] | f[2] | f[3] | f[4] | f[5]) & inner;
            n_solid += (uint32_t)__builtin_popcount(solid & inner);
            n0 += (uint32_t)__builtin_popcount(f[0] & inner);
            n1 += (uint32_t)__builtin_popcount(f[1] & inner);
            n2 += (uint32_t)__builtin_popcount(f[2] & inner);
            n3 += (uint32_t)__builtin_popcount(f[3] & inner);
            n4 += (uint32_t)__builtin_popcount(f[4] & inner);
            n5 += (uint32_t)__builtin_popcount(f[5] & inner);
        }
        if (w < a.n_words) {
            a.cand[w] = cand;
            if (a.store_faces) {
#pragma unroll
                for (uint32_t d = 0; d < 6u; ++d) a.face[d * a.stride + w] = f[d];
            }
        }
        n_cand += (uint32_t)__builtin_popcount(cand);
        a.count[w] = (uint32_t)__builtin_popcount(cand);   // (the extra element of the scan is 0: its prefix is the total)
    }
    const uint32_t t_solid = ft_wave_sum(n_solid), t0 = ft_wave_sum(n0), t1 = ft_wave_sum(n1), t2 = ft_wave_sum(n2), t3 = ft_wave_sum(n3),
                   t4 = ft_wave_sum(n4), t5 = ft_wave_sum(n5), t_cand = ft_wave_sum(n_cand);
    if (lane == 0u) {
        uint32_t *o = a.stats + 8u * g;
        o[0] = t_solid;
        o[1] = t0;
        o[2] = t1;
        o[3] = t2;
        o[4] = t3;
        o[5] = t4;
        o[6] = t5;
        o[7] = t_cand;
    }
}

// ---- stage 3: emit -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dm_sf_emit(SurfaceArgs a) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= a.n_words) return;
    uint32_t rest = a.cand[w];
    if (rest == 0u) return;
    unsigned long long t = a.offset[w];
    if (t >= a.cap) return;
    uint32_t f[6];
    sf_face_words(a, w, a.solid[w], f);
    const bool own_normal = a.normal != nullptr && a.s == 0u;
    while (rest && t < a.cap) {   // at most 32 trips
        const uint32_t b = (uint32_t)__builtin_ctz(rest);
        rest &= rest - 1u;
        uint32_t byte = 0u;
#pragma unroll
        for (uint32_t d = 0; d < 6u; ++d) byte |= ((f[d] >> b) & 1u) << d;
        if (a.index) a.index[t] = sf_unpadded(a, (w << 5) + b);
        if (a.faces) a.faces[t] = (uint8_t)byte;
        if (own_normal) {
            a.normal[3ull * t + 0ull] = (int16_t)((int)((byte >> 1) & 1u) - (int)(byte & 1u));
            a.normal[3ull * t + 1ull] = (int16_t)((int)((byte >> 3) & 1u) - (int)((byte >> 2) & 1u));
            a.normal[3ull * t + 2ull] = (int16_t)((int)((byte >> 5) & 1u) - (int)((byte >> 4) & 1u));
        }
        ++t;
    }
}

// ---- stage 4: the windowed normals (smooth > 0) -----------------------------------------------------------------------
// the count of voxel b < 32 from the planes
__device__ __forceinline__ int sf_count_of(const uint32_t planes[kSfPlanes], uint32_t b) {
    uint32_t c = 0u;
#pragma unroll
    for (int q = 0; q < kSfPlanes; ++q) c |= ((planes[q] >> b) & 1u) << q;
    return (int)c;
}

// word w of a stream by a load that is never skipped — at a safe address where w lies outside — so that the loads of a
// whole round can be in flight together
__device__ __forceinline__ uint32_t sf_word(const uint32_t *__restrict__ u, uint32_t n_words, int w) {
    const bool in = (uint32_t)w < n_words;
    const uint32_t v = u[in ? (uint32_t)w : 0u];
    return in ? v : 0u;
}

// bits from .. from + 63 of a stream (from may be negative or past the end: zeros there)
__device__ __forceinline__ unsigned long long sf_window64(const uint32_t *__restrict__ u, uint32_t n_words, int from) {
    const int w = from >> 5;   // floor, also for from < 0
    const uint32_t sh = (uint32_t)from & 31u;
    const uint32_t x0 = sf_word(u, n_words, w), x1 = sf_word(u, n_words, w + 1), x2 = sf_word(u, n_words, w + 2);
    const unsigned long long lo = ((((unsigned long long)x1) << 32) | x0) >> sh;
    return sh ? lo | (((unsigned long long)x2) << (64u - sh)) : lo;
}

// planes += c0 + c1, bit-sliced, in the 5 low planes (the count stays below 32): a full adder, then half adders
__device__ __forceinline__ void sf_add2(uint32_t planes[kSfPlanes], uint32_t c0, uint32_t c1) {
    const uint32_t x = planes[0] ^ c0;
    uint32_t carry = (planes[0] & c0) | (x & c1);
    planes[0] = x ^ c1;
#pragma unroll
    for (int p = 1; p < 5; ++p) {
        const uint32_t both = planes[p] & carry;
        planes[p] ^= carry;
        carry = both;
    }
}

// the lanes' bit-sliced counts (at most 18 each, 5 planes) summed over the wave: the count of voxel lane & 31, in every lane
__device__ __forceinline__ int sf_wave_count(uint32_t planes[kSfPlanes], uint32_t lane) {
    ft_fold<5, kSfPlanes>(planes, 1);   // 64 lanes x 18 would not fit 10 planes, but the 81 columns hold 729 at most
    ft_fold<6, kSfPlanes>(planes, 2);
    ft_fold<7, kSfPlanes>(planes, 4);
    ft_fold<8, kSfPlanes>(planes, 8);
    ft_fold<9, kSfPlanes>(planes, 16);
    ft_fold<10, kSfPlanes>(planes, 32);
    return sf_count_of(planes, lane & 31u);
}

// the count of voxel lane & 31 from the lanes' two 64-bit column windows x0, x1 (those of the two rounds): the 2s + 1 shifts
// of each added into 5 planes (at most 18 a lane), the lanes summed.  All 64 lanes call it; a direction with no face in
// the whole window — most of them next to a floor — skips the butterfly.
__device__ __forceinline__ int sf_column_count(unsigned long long x0, unsigned long long x1, int side, uint32_t lane) {
    if (__ballot((x0 | x1) != 0ull) == 0ull) return 0;   // uniform
    uint32_t planes[kSfPlanes];
#pragma unroll
    for (int q = 0; q < kSfPlanes; ++q) planes[q] = 0u;
#pragma unroll 1
    for (int dk = 0; dk < side; ++dk) sf_add2(planes, (uint32_t)(x0 >> dk), (uint32_t)(x1 >> dk));
    return sf_wave_count(planes, lane);
}

// kSfWaves waves, whatever the region; word w belongs to wave w % kSfWaves, as in footing's dm_ft_foot, so the words of a
// patch of surface — neighbours in the stream — go to different waves.  Per candidate word one axis at a time: the lanes
// take the (2s + 1)^2 columns in two rounds of 64, and the twelve loads of an axis — two streams, two rounds, three words —
// are issued together (a lane without a column loads bit 0's words and masks them).  Three other forms were measured and
// dropped: the six streams one after the other, each with its own loads, took 23 to 68 us where this one
// takes 20 to 47; the three axes unrolled gained nothing; the planes of both directions live together (84 VGPRs) were no
// faster; one lane per word took 90 to 600.
__global__ __launch_bounds__(256) void dm_sf_normals(SurfaceArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6);   // the wave, < kSfWaves
    const int s = (int)a.s, side = 2 * s + 1, cells = side * side, sy = (int)a.PZ, sx = (int)(a.PY * a.PZ);
    // this lane's columns in the two rounds, as bit offsets from the word (0 and masked where it has none)
    const int q0 = (int)lane, q1 = 64 + (int)lane;
    const bool has0 = q0 < cells, has1 = q1 < cells;
    const int off0 = has0 ? (q0 / side - s) * sx + (q0 % side - s) * sy - s : 0;
    const int off1 = has1 ? (q1 / side - s) * sx + (q1 % side - s) * sy - s : 0;
    const unsigned long long keep0 = has0 ? ~0ull : 0ull, keep1 = has1 ? ~0ull : 0ull;
#pragma unroll 1
    for (uint32_t w0 = g; w0 < a.n_words; w0 += 64u * kSfWaves) {   // everything in here but `mine` and `at` is uniform over the wave
        const uint32_t w = w0 + lane * kSfWaves;
        const uint32_t mine = w < a.n_words ? a.cand[w] : 0u;
        const uint32_t at = mine ? a.offset[w] : 0u;
        unsigned long long todo = __ballot(mine != 0u && at < a.cap);
        while (todo) {   // at most 64 trips
            const int t = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const uint32_t cand = __shfl(mine, t, 64);
            const unsigned long long first = __shfl(at, t, 64);
            const int base = (int)((w0 + (uint32_t)t * kSfWaves) << 5);
            const uint32_t b = lane & 31u;
            const bool listed = lane < 32u && ((cand >> b) & 1u);
            const unsigned long long place = first + (unsigned long long)__builtin_popcount(cand & ((1u << b) - 1u));
#pragma unroll 1
            for (uint32_t axis = 0; axis < 3u; ++axis) {
                const uint32_t *minus_stream = a.face + (size_t)(2u * axis) * a.stride, *plus_stream = minus_stream + a.stride;
                const unsigned long long m0 = sf_window64(minus_stream, a.n_words, base + off0) & keep0;
                const unsigned long long m1 = sf_window64(minus_stream, a.n_words, base + off1) & keep1;
                const unsigned long long p0 = sf_window64(plus_stream, a.n_words, base + off0) & keep0;
                const unsigned long long p1 = sf_window64(plus_stream, a.n_words, base + off1) & keep1;
                const int n_minus = sf_column_count(m0, m1, side, lane), n_plus = sf_column_count(p0, p1, side, lane);
                if (listed && place < a.cap) a.normal[3ull * place + axis] = (int16_t)(n_plus - n_minus);
            }
        }
    }
}

// ---- stage 5: the dense face masks ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dm_sf_dense(SurfaceArgs a) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;   // nx ny nz <= 2^28
    if (f >= a.nx * a.ny * a.nz) return;
    const uint32_t k = f % a.nz, row = f / a.nz;
    const uint32_t j = row % a.ny, i = row / a.ny;
    const uint32_t p = ((i + a.pad) * a.PY + (j + a.pad)) * a.PZ + (k + a.pad);
    const uint32_t w = p >> 5, b = p & 31u;
    uint32_t byte = 0u;
#pragma unroll
    for (uint32_t d = 0; d < 6u; ++d) byte |= ((a.face[d * a.stride + w] >> b) & 1u) << d;
    a.dense[f] = (uint8_t)byte;
}

}  // namespace la3dm_dev

#endif
