// devmap_reach.h — hop distance from seed voxels through the passable voxels of a map region on the device-resident block
// pool: a breadth-first wave, one launch per level (la3dm_devmap_reach_*, include/la3dm_hip.h; host twin and definition:
// BGKOctoMap::reach, host/bgkoctomap.cpp).  Integers throughout and a unique answer: the result equals the host form bit
// for bit.
//
// Everything runs on the PADDED box (PX, PY, PZ) = (nx + 2, ny + 2, nz + 2) as frontier's kernels do, but the pad is never
// read from the map: pad cells are never passable, their bits are 0 in every stream, so a neighbour of padded index p is
// p + di PY PZ + dj PZ + dk with no test at the faces and the wave cannot leave the region.
//
// dm_rc_bits    one probe per padded voxel of the region's interior and one ballot: the PASS stream (class in pass_mask,
//               and the word FAR at the unpadded index of the ObstacleField, devmap_distance.h: distance_field's d2 at
//               radius = clearance, computed before, or FAR everywhere without a clearance).
// dm_rc_seed    one lane per seed: range test, pass bit, then an atomic OR into the REACHED and the FRONT word.  The old
//               value of the reached word tells whether the voxel is new: only then steps = 0 is written and the seed
//               counted, so n_seeded counts a voxel once however often it is listed.
// dm_rc_level   one lane per 32-voxel word.  p = pass & ~reached; a word without such a voxel writes an empty front word
//               and is done.  Otherwise the 32-bit windows of the previous front at the connectivity's bit offsets
//               (fr_window: two words, one funnel shift) are ORed and cut with p: the voxels of this level.  They join
//               reached, become the word of the next front, get `level` as their steps, and their number goes — summed
//               over the wave first, one atomic per wave — into count[level].
// dm_rc_gather  one lane per target: steps at the target, NONE for an index out of range.
//
// Invariant.  Within a launch front_in is only read.  reached[w], front_out[w] and the steps of the voxels of word w are
// written by the lane of word w alone.  The only atomics are the seed kernel's and the per-wave add into count[level].
// There is no grid-wide barrier, no cooperative launch and no spin: one level is one launch, and the host reads a batch
// of counts to learn where the wave ended.  A level queued behind the last one finds an empty front and writes nothing
// but empty front words.
//
// Working storage: pass, reached and two fronts that take turns — 4 x 4 bytes per 32 padded voxels, 1/2 byte per padded
// voxel — plus max_steps + 1 counts and 4 bytes per voxel (d2, then the steps where the caller gave no array for them).
//
// Every loop is bounded by an argument or a constant: the offsets, 32 bits of a word, the probe count, 6 shuffle steps.
#ifndef LA3DM_DEVMAP_REACH_H
#define LA3DM_DEVMAP_REACH_H

#include "devmap_distance.h"
#include "devmap_frontier.h"
#include "host/region_contract.h"

namespace la3dm_dev {

struct ReachArgs {
    uint32_t nx, ny, nz;          // the region
    uint32_t PY, PZ;              // padded extents along y and z
    uint32_t total;               // padded voxels PX PY PZ <= 2^28
    uint32_t n_words;             // ceil(total / 32)
    uint32_t n_cells;             // nx ny nz
    const uint32_t *pass;         // [n_words]
    uint32_t *reached;            // [n_words]
    uint32_t *steps;              // [n_cells], LA3DM_REACH_NONE before the wave
    uint32_t *count;              // [max_steps + 1]: n_seeded, then the voxels of every level
};

constexpr uint32_t kReachNone = LA3DM_REACH_NONE;

// padded index of the voxel with flat index f of the region
__device__ __forceinline__ uint32_t rc_padded(const ReachArgs &a, uint32_t f) {
    const uint32_t k = f % a.nz, row = f / a.nz;
    const uint32_t j = row % a.ny, i = row / a.ny;
    return ((i + 1u) * a.PY + (j + 1u)) * a.PZ + (k + 1u);
}

// flat index in the region of an inner padded voxel p
__device__ __forceinline__ uint32_t rc_unpadded(const ReachArgs &a, uint32_t p) {
    const uint32_t k = p % a.PZ, row = p / a.PZ;
    const uint32_t j = row % a.PY, i = row / a.PY;
    return ((i - 1u) * a.ny + (j - 1u)) * a.nz + (k - 1u);
}

// ---- stage 1: the pass stream ------------------------------------------------------------------------------------
// `r` describes the UNPADDED region (g0, dims, pool).  The grid covers whole waves of the padded box: lanes beyond
// a.total vote 0, so the bits past the end of the last word are clear.  `probe` = 0: the map has no block, every voxel is
// MISSING and the table is not read.  `field` (ObstacleField, devmap_distance.h): a voxel within the clearance of an
// obstacle has a word other than FAR there and does not pass; without a clearance every word is FAR.
__global__ __launch_bounds__(256) void dm_rc_bits(RegionArgs r, ReachArgs a, uint32_t pass_mask, uint32_t probe, ObstacleField field,
                                                  uint32_t *pass) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;   // total <= 2^28: no overflow
    bool ok = false;
    if (p < a.total) {
        const uint32_t k = p % a.PZ, row = p / a.PZ;
        const uint32_t j = row % a.PY, i = row / a.PY;
        if (k >= 1u && k <= a.nz && j >= 1u && j <= a.ny && i >= 1u && i <= a.nx) {   // pad cells are never passable and not probed
            const uint32_t cls = probe ? pool_class_at(r.pool, r.g0[0] + i - 1u, r.g0[1] + j - 1u, r.g0[2] + k - 1u) : kClsMissing;
            ok = (pass_mask >> cls) & 1u;
            if (ok) ok = field.at(((i - 1u) * a.ny + (j - 1u)) * a.nz + (k - 1u)) == LA3DM_DF_FAR;
        }
    }
    pool_store_ballot(pass, p, a.total, ok);
}

// ---- stage 2: the seeds ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dm_rc_seed(ReachArgs a, const uint32_t *seeds, uint32_t n_seeds, uint32_t *front) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_seeds) return;
    const uint32_t f = seeds[t];
    if (f >= a.n_cells) return;
    const uint32_t p = rc_padded(a, f), w = p >> 5, bit = 1u << (p & 31u);   // p < total: w < n_words
    if (!(a.pass[w] & bit)) return;
    const uint32_t old = atomicOr(&a.reached[w], bit);
    atomicOr(&front[w], bit);
    if (old & bit) return;   // listed before
    a.steps[f] = 0u;
    atomicAdd(&a.count[0], 1u);
}

// ---- stage 3: one level ------------------------------------------------------------------------------------------------
template <int kConn>
__global__ __launch_bounds__(256) void dm_rc_level(ReachArgs a, const uint32_t *__restrict__ front_in, uint32_t *__restrict__ front_out,
                                                   uint32_t level) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    uint32_t fresh = 0u;
    if (w < a.n_words) {
        const uint32_t reached = a.reached[w];
        const uint32_t p = a.pass[w] & ~reached;
        if (p) {
            const int base = (int)(w << 5), sy = (int)a.PZ, sx = (int)(a.PY * a.PZ);
#pragma unroll
            for (int di = -1; di <= 1; ++di)
#pragma unroll
                for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
                    for (int dk = -1; dk <= 1; ++dk) {
                        const int manhattan = (di ? 1 : 0) + (dj ? 1 : 0) + (dk ? 1 : 0);
                        if (manhattan == 0 || manhattan > la3dm_region::move_reach(kConn)) continue;
                        fresh |= fr_window(front_in, a.n_words, base + di * sx + dj * sy + dk);
                    }
            fresh &= p;
        }
        front_out[w] = fresh;
        if (fresh) {
            a.reached[w] = reached | fresh;
            uint32_t rest = fresh;
            while (rest) {   // at most 32 trips
                const uint32_t b = (uint32_t)__builtin_ctz(rest);
                rest &= rest - 1u;
                a.steps[rc_unpadded(a, (w << 5) + b)] = level;   // (fresh is a subset of pass: inner voxels only)
            }
        }
    }
    // the wave's popcount, one atomic per wave; every lane of the wave arrives here
    if (__ballot(fresh != 0u) == 0ull) return;
    uint32_t n = (uint32_t)__builtin_popcount(fresh);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63u) == 0u) atomicAdd(&a.count[level], n);
}

// ---- stage 4: the steps at the targets -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dm_rc_gather(const uint32_t *steps, uint32_t n_cells, const uint32_t *targets, uint32_t n_targets,
                                                    uint32_t *target_steps) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_targets) return;
    const uint32_t f = targets[t];
    target_steps[t] = f < n_cells ? steps[f] : kReachNone;
}

}  // namespace la3dm_dev

#endif
