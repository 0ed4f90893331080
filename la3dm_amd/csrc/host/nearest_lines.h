// nearest_lines.h — the line passes of the feature transform behind nearest and nearest_points (contract:
// include/la3dm_hip.h, la3dm_devmap_nearest_host): distance_field's three separable stages, each of which keeps its
// argmin.  The host form (BGKOctoMap::nearest, host/bgkoctomap.cpp) is built from these and is the definition; the device
// kernels (csrc/devmap_nearest.h) share the key arithmetic.  Compiles alone (tools/check/nearest_lines.cpp drives the
// passes under ASan and UBSan).
//
// z      per voxel the signed offset k' - k to the nearest obstacle of its own z line within +-radius, the smaller k' on a
//        tie; radius + 1 where there is none — the saturated offset: its square is the saturated term of distance_field,
//        a sum that holds it exceeds radius^2, and it is never followed.
// y, x   min-plus over the packed key (sum << 9) | (offset + 256): the plain minimum of two keys is the smaller sum and,
//        among equal sums, the smaller offset, i.e. the smaller j' (i').  radius <= 255: a term is at most 256^2, a sum
//        below 2^18, an offset fits 9 bits, a key 27.
// chase  i' = i + ax(i, j, k), j' = j + ay(i', j, k), k' = k + az(i', j', k): the smallest flat index among the global
//        minimisers.  All minimisers in plane i' share one in-plane distance, so the per-plane lexicographic choice is the
//        global one; minimisers with D <= radius^2 have every axis offset <= radius, so the windows lose none.
#ifndef LA3DM_NEAREST_LINES_H
#define LA3DM_NEAREST_LINES_H

#include <algorithm>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define LA3DM_NT_HD __host__ __device__
#else
#define LA3DM_NT_HD
#endif

namespace la3dm_nearest {

constexpr uint32_t kOffsetBits = 9, kOffsetZero = 256;

LA3DM_NT_HD inline uint32_t key_of(uint32_t sum, int offset) { return (sum << kOffsetBits) | (uint32_t)(offset + (int)kOffsetZero); }
LA3DM_NT_HD inline uint32_t key_sum(uint32_t key) { return key >> kOffsetBits; }
LA3DM_NT_HD inline int key_offset(uint32_t key) { return (int)(key & ((1u << kOffsetBits) - 1u)) - (int)kOffsetZero; }
// the term of a z offset: its square ((radius + 1)^2 where the line holds no obstacle within the radius)
LA3DM_NT_HD inline uint32_t offset_term(int16_t off) { return (uint32_t)((int)off * (int)off); }

// z: obstacle[k] != 0 marks the obstacles of a line of n voxels; a sweep up and a sweep down
inline void line_z(const uint8_t *obstacle, size_t n, uint32_t radius, int16_t *off) {
    const uint32_t sat = radius + 1u;
    uint32_t run = sat;
    for (size_t k = 0; k < n; ++k) {   // the distance to the nearest obstacle at or below k
        run = obstacle[k] ? 0u : std::min(run + 1u, sat);
        off[k] = (int16_t)run;
    }
    run = sat;
    for (size_t k = n; k-- > 0;) {     // ... at or above k; the one below wins a tie
        run = obstacle[k] ? 0u : std::min(run + 1u, sat);
        const uint32_t below = (uint32_t)off[k];
        off[k] = below <= run ? (below == sat ? (int16_t)sat : (int16_t)(-(int)below)) : (int16_t)run;
    }
}

// y, x: key(l) = min over |d| <= radius with 0 <= l + d < L of key_of(term(l + d) + d^2, d), handed to out(l, key).  An
// offset with d^2 == the best sum can still win — with a term of 0 on the low side — so the bound is <= where
// distance_field's is <.
template <class Term, class Out>
inline void line_pass(size_t L, uint32_t radius, Term term, Out out) {
    for (size_t l = 0; l < L; ++l) {
        uint32_t best = key_of(term(l), 0);
        for (uint32_t d = 1; d <= radius && d * d <= key_sum(best); ++d) {
            if (l >= d) best = std::min(best, key_of(term(l - d) + d * d, -(int)d));
            if (l + d < L) best = std::min(best, key_of(term(l + d) + d * d, (int)d));
        }
        out(l, best);
    }
}

}  // namespace la3dm_nearest

#endif
