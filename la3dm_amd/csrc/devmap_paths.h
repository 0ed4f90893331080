// devmap_paths.h — cost and clearance of many candidate trajectories on the device-resident map
// (la3dm_devmap_score_paths_*, include/la3dm_hip.h; host twin and definition: BGKOctoMap::score_paths,
// host/bgkoctomap.cpp).  Stage 1 is distance_field's launch chain (devmap_distance.h) into working storage; the kernel
// below is stage 2.  The waypoint voxel, the walk sample, the move class and the entry are host/region_contract.h's
// inlines, compiled here as they are for the host form; everything after the waypoint voxels is integers, so any order of
// the sums gives the same answer.
//
// dm_paths_walk    one wave per path, kPathsWaves paths per workgroup.
//                  1. Lanes resolve the path's waypoints, 64 a trip, into LDS: three 32-bit words per waypoint (for
//                     block_depth <= 6 every G fits 32 bits signed: region_contract.h, path_waypoint) and one for the offset.
//                  2. The segment lengths n_k go through a prefix scan by shuffles, 64 a trip with a carry, into the LDS
//                     offsets.  Lengths and sums saturate at max_steps + 1, so 32 bits suffice; no output changes, because
//                     only ordinals <= max_steps are walked and only offsets < L <= max_steps + 1 are counted.
//                  3. Lanes take ordinals in ascending chunks of 64.  A lane finds its segment by binary search in the
//                     offsets (at most 10 trips), samples its voxel, takes its predecessor's from the lane below (lane 0:
//                     from the chunk before), tests the region and gathers d2.  A ballot finds the first stop of the chunk;
//                     lanes at or beyond it add nothing, and the wave leaves the loop.
//                  4. The 64-bit sum, the minimum and the waypoint count are folded by shuffles; lane 0 writes.
//                  LDS: 16 bytes per waypoint and wave, sized by the launch (at most 64 KB at n_way = 1024; 2 KB at 32), so
//                  a planner-sized call is not held back by it.  No atomic.  Every loop is bounded by an argument: n_way,
//                  max_steps, or the 10 halvings of the search.  The barriers stand in loops whose trip count depends on
//                  n_way alone, so every wave of a workgroup — also one past the last path, and one whose path is INVALID —
//                  meets each of them.
//
// cost is written as two 32-bit words: a device pointer need only be 4-byte aligned.  The distance word of a voxel is read
// through ObstacleField (devmap_distance.h): on the empty map it has no array, every voxel has its `fill`, and the pool
// is not read.
#ifndef LA3DM_DEVMAP_PATHS_H
#define LA3DM_DEVMAP_PATHS_H

#include "devmap_distance.h"
#include "host/region_contract.h"

namespace la3dm_dev {

constexpr uint32_t kPathsWaves = 4;   // paths per workgroup

struct PathsArgs {
    const float *ways;      // 3 n_way per path
    uint32_t n_paths, n_way;
    float resolution, block_size;
    int lim;                // cells of a block per axis
    uint32_t g0[3], dims[3];
    la3dm_paths_params p;
    ObstacleField field;    // the d2 word of a voxel (devmap_distance.h)
    uint32_t *cost;         // [2 n_paths]: low word, high word
    uint32_t *steps, *stop, *min_d2, *reached;   // [n_paths] or null
    uint8_t *flags;         // [n_paths] or null
};

__global__ __launch_bounds__(64 * kPathsWaves) void dm_paths_walk(PathsArgs a) {
    extern __shared__ uint32_t paths_lds[];   // per wave: gx, gy, gz, off, n_way words each
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t path = blockIdx.x * kPathsWaves + wave;
    const bool live = path < a.n_paths;
    const uint32_t nw = a.n_way;
    int32_t *gx = (int32_t *)(paths_lds + 4 * (size_t)wave * nw), *gy = gx + nw, *gz = gy + nw;
    uint32_t *off = (uint32_t *)(gz + nw);

    // 1. the waypoint voxels
    bool bad = false;
    for (uint32_t k = lane; k < nw; k += 64u) {   // at most n_way / 64 + 1 trips
        long long g[3] = {0, 0, 0};
        if (live) {
            const float *w = a.ways + 3 * ((size_t)path * nw + k);
            const float w3[3] = {w[0], w[1], w[2]};
            bad = !la3dm_region::path_waypoint(w3, a.resolution, a.block_size, a.lim, g) || bad;
        }
        gx[k] = (int32_t)g[0];
        gy[k] = (int32_t)g[1];
        gz[k] = (int32_t)g[2];
    }
    __syncthreads();

    // 2. the offsets, saturated at cap
    const uint32_t cap = a.p.max_steps + 1u;
    uint32_t carry = 0;
    if (lane == 0u) off[0] = 0u;
    for (uint32_t base = 1; base < nw; base += 64u) {   // at most n_way / 64 + 1 trips
        const uint32_t k = base + lane;
        uint32_t x = 0;
        if (k < nw) {
            const long long A[3] = {gx[k - 1], gy[k - 1], gz[k - 1]}, B[3] = {gx[k], gy[k], gz[k]};
            const long long n = la3dm_region::path_segment(A, B);
            x = n < (long long)cap ? (uint32_t)n : cap;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {   // (64 lengths of at most 2^20 + 1 and the carry: below 2^27)
            const uint32_t y = __shfl_up(x, d);
            if ((int)lane >= d) x += y;
        }
        x = min(x + carry, cap);
        if (k < nw) off[k] = x;
        carry = __shfl(x, 63);
    }
    __syncthreads();
    if (!live) return;   // (no barrier below)

    const uint32_t T = off[nw - 1u];                    // saturated: T > max_steps iff T == cap
    const uint32_t E = min(T, a.p.max_steps);
    uint32_t stop = LA3DM_PATH_NONE, flags = 0, L = 0, mn = LA3DM_DF_FAR, reached = 0;
    unsigned long long sum = 0;
    if (__ballot(bad) != 0ull) {
        flags = LA3DM_PATH_INVALID;
    } else {
        // 3. the walk
        int32_t tail[3] = {0, 0, 0};   // the voxel of the ordinal before this chunk
        for (uint32_t base = 0; base <= E; base += 64u) {   // at most max_steps / 64 + 1 trips
            const uint32_t o = base + lane;
            const bool act = o <= E;
            int32_t v[3] = {gx[0], gy[0], gz[0]};
            if (act && o > 0u) {
                uint32_t lo = 1, hi = nw - 1u;   // the smallest k with off[k] >= o: o <= E <= off[n_way - 1]
                while (lo < hi) {                // at most 10 trips
                    const uint32_t mid = (lo + hi) >> 1;
                    if (off[mid] >= o)
                        hi = mid;
                    else
                        lo = mid + 1u;
                }
                const long long A[3] = {gx[lo - 1u], gy[lo - 1u], gz[lo - 1u]}, B[3] = {gx[lo], gy[lo], gz[lo]};
                const long long n = la3dm_region::path_segment(A, B), s = (long long)(o - off[lo - 1u]);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = (int32_t)la3dm_region::path_sample(A[c], B[c] - A[c], n, s);
            }
            int32_t u[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                u[c] = __shfl_up(v[c], 1);
                if (lane == 0u) u[c] = tail[c];
                tail[c] = __shfl(v[c], 63);
            }
            bool halt = false, left = false;
            uint32_t word = LA3DM_DF_FAR, charge = 0;
            if (act) {
                const long long U[3] = {u[0], u[1], u[2]}, V[3] = {v[0], v[1], v[2]};
                uint32_t f = 0;
                if (!la3dm_region::path_inside(V, a.g0, a.dims, f)) {
                    halt = left = true;
                } else {
                    word = a.field.at(f);
                    if (la3dm_region::path_blocked(a.p.clearance, word))
                        halt = true;
                    else if (o > 0u)
                        charge = la3dm_region::path_entry(a.p, la3dm_region::path_move(U, V), word);
                }
            }
            const unsigned long long halts = __ballot(halt);
            const uint32_t first = halts ? (uint32_t)__ffsll((long long)halts) - 1u : 64u;
            if (act && lane < first) {
                sum += charge;
                mn = min(mn, word);
            }
            if (halts) {
                stop = base + first;
                flags = __shfl((int)left, (int)first) ? LA3DM_PATH_LEFT : LA3DM_PATH_BLOCKED;
                break;
            }
        }
        if (stop == LA3DM_PATH_NONE && T > a.p.max_steps) flags = LA3DM_PATH_TRUNCATED;
        L = stop != LA3DM_PATH_NONE ? stop : E + 1u;
        // 4. the waypoints reached, and the folds
        for (uint32_t k = lane; k < nw; k += 64u) reached += off[k] < L ? 1u : 0u;   // at most n_way / 64 + 1 trips
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            reached += __shfl_xor(reached, d);
            mn = min(mn, (uint32_t)__shfl_xor(mn, d));
            const uint32_t olo = __shfl_xor((uint32_t)sum, d), ohi = __shfl_xor((uint32_t)(sum >> 32), d);
            sum += ((unsigned long long)ohi << 32) | olo;
        }
    }
    if (lane != 0u) return;
    a.cost[2 * (size_t)path] = (uint32_t)sum;
    a.cost[2 * (size_t)path + 1] = (uint32_t)(sum >> 32);
    if (a.steps) a.steps[path] = L;
    if (a.stop) a.stop[path] = stop;
    if (a.min_d2) a.min_d2[path] = mn;
    if (a.reached) a.reached[path] = reached;
    if (a.flags) a.flags[path] = (uint8_t)flags;
}

}  // namespace la3dm_dev

#endif
