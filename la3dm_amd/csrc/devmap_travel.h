// devmap_travel.h — least path cost from seed voxels through the passable voxels of a map region on the device-resident
// block pool, with a parent per voxel (la3dm_devmap_travel_*, include/la3dm_hip.h; host twin and definition:
// BGKOctoMap::travel, host/bgkoctomap.cpp).  Integers throughout and a unique answer: the result equals the host form
// bit for bit.
//
// The scheme is devmap_brick.h's (bricks, two buffers, rounds, the LDS tile, Invariant and Termination); the value is the
// cost, and the rule is min-plus relaxation with positive integer weights, whose fixed point is unique whatever order the
// relaxations run in.  Every stored cost is the cost of a real walk, so at the fixed point the Bellman equations hold
// everywhere and the costs are the least ones.  Cells outside the region are blocked.
//
// dm_tv_enter   one lane per cell of the bricks: the pool probe (pool_class_at), the class test and the d2 tests; writes
//               the entry word E = pen(v), or kTvBlocked (not passable, or outside the region), and NONE into buffer 0.
// dm_tv_seed    one lane per seed: range test, entry word, atomicMin of the cost to 0; the old value tells whether the
//               voxel is new: only then it is counted; marks its brick active, and the neighbour bricks that touch it.
// dm_tv_round   the hot kernel: brick_round with TravelRule, at most LA3DM_TRAVEL_INNER iterations per run.  A lane keeps
//               its own E word in a register; a cost above max_cost is not stored.
// dm_tv_finish  one lane per voxel of the region: reads the brick-major cost through `side`, writes the dense cost and
//               the parent code, accumulates n_reached and max_cost, one atomic each per wave.
// dm_tv_gather  one lane per target: the cost at the target, NONE for an index out of range.
//
// Beside the round's atomics (devmap_brick.h) there are the seed kernel's and finish's two per wave.  Every loop is
// bounded by a constant (the seed kernel's 27 offsets, finish's 27 and 6 shuffle steps), and no array is indexed at run
// time: nothing lives in scratch.
#ifndef LA3DM_DEVMAP_TRAVEL_H
#define LA3DM_DEVMAP_TRAVEL_H

#include "devmap_brick.h"
#include "devmap_distance.h"

namespace la3dm_dev {

static_assert(LA3DM_TRAVEL_BRICK == 8 && LA3DM_TRAVEL_NONE == kBrickNone, "devmap_brick.h: bricks of 8 x 8 x 8, NONE the largest word");
constexpr uint32_t kTvNone = LA3DM_TRAVEL_NONE, kTvBlocked = 0xFFFFFFFFu;

struct TravelArgs {
    BrickGrid g;                  // val = the cost
    uint32_t *E;                  // [n_bricks * 512] entry words
    uint32_t *totals;             // n_seeded, n_reached, max_cost
    uint32_t move[3];             // cost of a move with 1, 2, 3 non-zero components
    uint32_t max_cost;
};

// twin of la3dm_region::travel_entry (host/region_contract.h)
__device__ __forceinline__ uint32_t tv_entry(uint32_t d2, uint32_t clearance, uint32_t s2, uint32_t penalty) {
    if (clearance > 0u && d2 != LA3DM_DF_FAR && d2 <= clearance * clearance) return kTvBlocked;
    return s2 > 0u && d2 <= s2 ? (uint32_t)((unsigned long long)penalty * (s2 - d2) / s2) : 0u;
}

// ---- stage 1: the entry words ------------------------------------------------------------------------------------------
// `r` describes the region (g0, dims, pool).  `probe` = 0: the map has no block, every voxel is MISSING and the table is
// not read.  `field`: the d2 word of every voxel (ObstacleField, devmap_distance.h).
__global__ __launch_bounds__(256) void dm_tv_enter(RegionArgs r, TravelArgs a, uint32_t pass_mask, uint32_t probe, ObstacleField field,
                                                   uint32_t clearance, uint32_t s2, uint32_t penalty) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;   // n_bricks * 512 <= 2^28: no overflow; the grid covers the cells exactly
    uint32_t i, j, k;
    brick_coords(a.g, c >> 9, c & 511u, i, j, k);
    uint32_t e = kTvBlocked;
    if (i < a.g.nx && j < a.g.ny && k < a.g.nz) {
        const uint32_t cls = probe ? pool_class_at(r.pool, r.g0[0] + i, r.g0[1] + j, r.g0[2] + k) : kClsMissing;
        if ((pass_mask >> cls) & 1u) e = tv_entry(field.at((i * a.g.ny + j) * a.g.nz + k), clearance, s2, penalty);
    }
    a.E[c] = e;
    a.g.val[0][c] = kTvNone;
}

// ---- stage 2: the seeds ------------------------------------------------------------------------------------------------
// `far` = the most non-zero components of a move (1, 2, 3 at connectivity 6, 18, 26).  A seed on a face of its brick is
// a neighbour of voxels of the next brick, and no round will ever see the seed itself change: the bricks that touch it
// are marked here.
__global__ __launch_bounds__(256) void dm_tv_seed(TravelArgs a, const uint32_t *seeds, uint32_t n_seeds, int far) {
    const BrickGrid &g = a.g;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_seeds) return;
    const uint32_t f = seeds[t];
    if (f >= g.n_cells) return;
    uint32_t b;
    const uint32_t c = brick_cell_of_flat(g, f, b);
    if (a.E[c] == kTvBlocked) return;
    if (atomicMin(&g.val[0][c], 0u) == 0u) return;   // listed before
    atomicAdd(&a.totals[0], 1u);
    const uint32_t li = (c >> 6) & 7u, lj = (c >> 3) & 7u, lk = c & 7u;
    const uint32_t bk = b % g.BZ, brow = b / g.BZ, bj = brow % g.BY, bi = brow / g.BY;
    for (int di = -1; di <= 1; ++di)
        for (int dj = -1; dj <= 1; ++dj)
            for (int dk = -1; dk <= 1; ++dk) {   // the seed's own brick (0, 0, 0) and the bricks that touch the seed
                if ((di ? 1 : 0) + (dj ? 1 : 0) + (dk ? 1 : 0) > far) continue;
                if (!brick_touches(di, dj, dk, li, lj, lk)) continue;
                const uint32_t qi = bi + (uint32_t)di, qj = bj + (uint32_t)dj, qk = bk + (uint32_t)dk;   // (bi - 1 wraps above BX)
                if (qi < g.BX && qj < g.BY && qk < g.BZ) atomicOr(&g.active[0][(qi * g.BY + qj) * g.BZ + qk], 1u);
            }
}

// ---- stage 3: one round ------------------------------------------------------------------------------------------------
// The rule of brick_round: a voxel that is not blocked takes the least of u + move + pen(v) over its neighbours u that
// hold a cost, if that is below its own and at most max_cost.  Every brick is joined to every neighbour.
struct TravelRule {
    const uint32_t *E;
    uint32_t move1, move2, move3, max_cost;
    uint32_t e;                   // the lane's own entry word
    __device__ __forceinline__ void brick(uint32_t, uint32_t, uint32_t) {}
    __device__ __forceinline__ bool open(uint32_t cell, uint32_t) {
        e = E[cell];
        return e != kTvBlocked;
    }
    __device__ __forceinline__ bool joined(uint32_t, uint32_t, uint32_t) const { return true; }
    __device__ __forceinline__ uint32_t relax(uint32_t best, uint32_t u, int m) const {
        const uint32_t cand = u + (m == 1 ? move1 : m == 2 ? move2 : move3) + e;   // u <= max_cost <= 2^31, move + e < 2^17: no overflow for a finite u
        return u != kTvNone && cand < best ? cand : best;
    }
    __device__ __forceinline__ bool keep(uint32_t best) const { return best <= max_cost; }
};

template <int kConn>
__global__ __launch_bounds__(512) void dm_tv_round(TravelArgs a, uint32_t turn, uint32_t round) {
    brick_round<kConn, LA3DM_TRAVEL_INNER>(a.g, turn, round, TravelRule{a.E, a.move[0], a.move[1], a.move[2], a.max_cost, 0u});
}

// ---- stage 4: dense cost, parents, totals ------------------------------------------------------------------------------
// `side`: the array the last queued round wrote.  cost and parent may be null.  The parent of a reached voxel that is no
// seed is the smallest code q whose offset the connectivity allows, that stays in the region, and whose voxel u has a
// finite cost with cost[u] + move + pen(v) == cost[v]: the loops run in the order of q.
template <int kConn>
__global__ __launch_bounds__(256) void dm_tv_finish(TravelArgs a, const uint32_t *__restrict__ side, uint32_t *cost, uint8_t *parent) {
    const BrickGrid &g = a.g;
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    uint32_t c = kTvNone;
    if (f < g.n_cells) {
        const uint32_t k = f % g.nz, row = f / g.nz, j = row % g.ny, i = row / g.ny;
        uint32_t b;
        const uint32_t cell = brick_cell(g, i, j, k, b);
        c = brick_pick(g.val, side[b] & 1u)[cell];
        if (cost) cost[f] = c;
        if (parent) {
            uint32_t code = c == kTvNone ? 255u : 13u;
            if (c != kTvNone && c != 0u) {
                const uint32_t e = a.E[cell];
                bool found = false;
#pragma unroll
                for (int di = -1; di <= 1; ++di)
#pragma unroll
                    for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
                        for (int dk = -1; dk <= 1; ++dk) {
                            if (!brick_allowed<kConn>(di, dj, dk)) continue;
                            const uint32_t ui = i + (uint32_t)di, uj = j + (uint32_t)dj, uk = k + (uint32_t)dk;   // (0 - 1 wraps above nx)
                            if (found || ui >= g.nx || uj >= g.ny || uk >= g.nz) continue;
                            uint32_t ub;
                            const uint32_t ucell = brick_cell(g, ui, uj, uk, ub);
                            const uint32_t u = brick_pick(g.val, side[ub] & 1u)[ucell];
                            if (u != kTvNone && u + a.move[(di ? 1 : 0) + (dj ? 1 : 0) + (dk ? 1 : 0) - 1] + e == c) {
                                code = (uint32_t)((di + 1) * 9 + (dj + 1) * 3 + (dk + 1));
                                found = true;
                            }
                        }
            }
            parent[f] = (uint8_t)code;
        }
    }
    // the wave's totals, one atomic each per wave; every lane of the wave arrives here
    if (__ballot(c != kTvNone) == 0ull) return;
    uint32_t n = c != kTvNone ? 1u : 0u, most = c != kTvNone ? c : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n += __shfl_xor(n, o);
        most = max(most, __shfl_xor(most, o));
    }
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(&a.totals[1], n);
        atomicMax(&a.totals[2], most);
    }
}

// ---- stage 5: the cost at the targets ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dm_tv_gather(TravelArgs a, const uint32_t *__restrict__ side, const uint32_t *targets, uint32_t n_targets,
                                                    uint32_t *target_cost) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_targets) return;
    const uint32_t f = targets[t];
    uint32_t c = kTvNone;
    if (f < a.g.n_cells) {
        uint32_t b;
        const uint32_t cell = brick_cell_of_flat(a.g, f, b);
        c = brick_pick(a.g.val, side[b] & 1u)[cell];
    }
    target_cost[t] = c;
}

}  // namespace la3dm_dev

#endif
