// devmap_travel.h — least path cost from seed voxels through the passable voxels of a map region on the device-resident
// block pool, with a parent per voxel (la3dm_devmap_travel_*, include/la3dm_hip.h; host twin and definition:
// BGKOctoMap::travel, host/bgkoctomap.cpp).  Integers throughout and a unique answer: the result equals the host form
// bit for bit.
//
// The fixed point of min-plus relaxation with positive integer weights is unique whatever order the relaxations run in,
// so a workgroup may relax a brick of voxels to its LOCAL fixed point in LDS before anything is written back; a global
// round then moves the wave by a brick, not by a voxel.
//
// The cost is kept BRICK-MAJOR: the region is rounded up to whole bricks of 8 x 8 x 8 voxels, brick b = (bi BY + bj) BZ
// + bk holds the 512 consecutive words b * 512 + (li * 8 + lj) * 8 + lk, and cells outside the region are blocked.  There
// are two cost buffers; side[b] names the one that holds brick b's current costs.  One workgroup owns one brick.
//
// dm_tv_enter   one lane per cell of the bricks: the pool probe (pool_class_at), the class test and the d2 tests; writes
//               the entry word E = pen(v), or kTvBlocked (not passable, or outside the region), and NONE into buffer 0.
// dm_tv_seed    one lane per seed: range test, entry word, atomicMin of the cost to 0; the old value tells whether the
//               voxel is new: only then it is counted; marks its brick active, and the neighbour bricks that touch it.
// dm_tv_round   the hot kernel: one workgroup of 512 lanes per brick, for every brick.  Reads side_in[b] and
//               active_in[b], then clears active_in[b].  An inactive brick copies its side to side_out[b] and leaves.  An
//               active brick loads its 512 costs from buffer side_in[b] and the one-voxel halo from its up to 26
//               neighbour bricks, each from the buffer THAT brick's side_in names, into a 10 x 10 x 10 tile in LDS (its
//               own E word stays in a register), and relaxes there — Jacobi: every lane reads its neighbours, a barrier
//               (__syncthreads_or of "changed"), every changed lane writes, a barrier — until no lane changes or
//               LA3DM_TRAVEL_INNER iterations have run.  If nothing changed: side_out[b] = side_in[b] and nothing else is
//               written.  Otherwise the 512 costs go to the OTHER buffer, side_out[b] flips, active_out is ORed for every
//               neighbour brick that touches a changed voxel (and for the brick itself where the cap stopped it), and the
//               changed voxels are added to count[round].
// dm_tv_finish  one lane per voxel of the region: reads the brick-major cost through `side`, writes the dense cost and
//               the parent code, accumulates n_reached and max_cost, one atomic each per wave.
// dm_tv_gather  one lane per target: the cost at the target, NONE for an index out of range.
//
// LDS tile.  ds_read_b32 banks are (address / 4) % 32 and the two 32-lane halves of a wave conflict among themselves
// only.  Strides (x, y, z) = (168, 16, 1) and a lane order whose low five bits are lk (3 bits), lj & 1, li & 1 put the
// four 8-word z runs of a half wave at 0, 16, 168 = 8 and 184 = 24 (mod 32): every bank once.  A neighbour read adds the
// same constant to every lane's address, so it is conflict-free too.  10 x 168 words = 6720 bytes.
//
// Invariant.  Within a launch of dm_tv_round, side_in, both roles of `active` and buffer side_in[b] of every brick are
// only read — but for each owner clearing its own active_in word, which no other workgroup reads.  Only the owner of b
// writes buffer 1 - side_in[b] of b and side_out[b].  No word is read by one workgroup and written by another in the
// same launch.  The only atomics are the seed kernel's, the ORs into active_out, the per-workgroup adds into
// count[round] (changed voxels, brick runs, capped runs: three lanes, one instruction) and finish's two per wave.  There
// is no grid barrier, no cooperative launch and no spin.
// Termination.  Every stored value is the cost of a real walk (a minimum over candidates built from stored values).  An
// inactive brick ended its last run at a local fixed point and has seen no neighbour change since.  So count[round] ==
// 0 — no voxel changed, hence no brick was marked — means the Bellman equations hold everywhere, and the costs are the
// least ones.  Rounds queued behind that one find every brick inactive and only copy `side`.
//
// Every loop is bounded by a constant: the offsets (27 in the seed kernel), the tile's 1000 cells, LA3DM_TRAVEL_INNER, 6 shuffle steps.  No
// array is indexed at run time: nothing lives in scratch.
#ifndef LA3DM_DEVMAP_TRAVEL_H
#define LA3DM_DEVMAP_TRAVEL_H

#include "devmap_pool.h"
#include "devmap_region.h"

namespace la3dm_dev {

constexpr uint32_t kTvNone = LA3DM_TRAVEL_NONE, kTvBlocked = 0xFFFFFFFFu;
constexpr int kTvSY = 16, kTvSX = 168, kTvTile = 10 * kTvSX;   // LDS strides of the 10 x 10 x 10 tile (see above)
constexpr uint32_t kTvCountWords = 4;   // per round: changed voxels, brick runs, capped runs, -

struct TravelArgs {
    uint32_t nx, ny, nz;
    uint32_t BX, BY, BZ;          // bricks per axis
    uint32_t n_bricks;            // BX BY BZ <= 2^19
    uint32_t n_cells;             // nx ny nz
    uint32_t move[3];             // cost of a move with 1, 2, 3 non-zero components
    uint32_t max_cost;
    uint32_t *cost[2];            // [n_bricks * 512] each, brick-major
    uint32_t *E;                  // [n_bricks * 512] entry words
    uint32_t *side[2];            // [n_bricks] each: which buffer holds the brick (the two arrays take turns)
    uint32_t *active[2];          // [n_bricks] each
    uint32_t *count;              // [rounds][kTvCountWords]
    uint32_t *totals;             // n_seeded, n_reached, max_cost
};

// brick-major cell of voxel (i, j, k) of the region
__device__ __forceinline__ uint32_t tv_cell(const TravelArgs &a, uint32_t i, uint32_t j, uint32_t k, uint32_t &brick) {
    brick = ((i >> 3) * a.BY + (j >> 3)) * a.BZ + (k >> 3);
    return (brick << 9) | ((i & 7u) << 6) | ((j & 7u) << 3) | (k & 7u);
}

__device__ __forceinline__ uint32_t tv_cell_of_flat(const TravelArgs &a, uint32_t f, uint32_t &brick) {
    const uint32_t k = f % a.nz, row = f / a.nz;
    return tv_cell(a, row / a.ny, row % a.ny, k, brick);
}

// one of a pair by a run-time index, as a select: an array indexed at run time would live in scratch
template <class T>
__device__ __forceinline__ T tv_pick(T const (&pair)[2], uint32_t which) {
    return which ? pair[1] : pair[0];
}

// twin of la3dm_region::travel_entry (host/region_contract.h)
__device__ __forceinline__ uint32_t tv_entry(uint32_t d2, uint32_t clearance, uint32_t s2, uint32_t penalty) {
    if (clearance > 0u && d2 != LA3DM_DF_FAR && d2 <= clearance * clearance) return kTvBlocked;
    return s2 > 0u && d2 <= s2 ? (uint32_t)((unsigned long long)penalty * (s2 - d2) / s2) : 0u;
}

template <int kConn>
__device__ __forceinline__ constexpr bool tv_allowed(int di, int dj, int dk) {
    const int m = (di ? 1 : 0) + (dj ? 1 : 0) + (dk ? 1 : 0);
    return m >= 1 && m <= (kConn == 6 ? 1 : kConn == 18 ? 2 : 3);
}

// ---- stage 1: the entry words ------------------------------------------------------------------------------------------
// `r` describes the region (g0, dims, pool).  `probe` = 0: the map has no block, every voxel is MISSING and the table is
// not read.  d2 null: every voxel has d2 = d2_fill (no distance transform, or the empty map's uniform answer).
__global__ __launch_bounds__(256) void dm_tv_enter(RegionArgs r, TravelArgs a, uint32_t pass_mask, uint32_t probe, const uint32_t *d2,
                                                   uint32_t d2_fill, uint32_t clearance, uint32_t s2, uint32_t penalty) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;   // n_bricks * 512 <= 2^28: no overflow; the grid covers the cells exactly
    const uint32_t b = c >> 9, bk = b % a.BZ, brow = b / a.BZ;
    const uint32_t i = (brow / a.BY) * 8u + ((c >> 6) & 7u), j = (brow % a.BY) * 8u + ((c >> 3) & 7u), k = bk * 8u + (c & 7u);
    uint32_t e = kTvBlocked;
    if (i < a.nx && j < a.ny && k < a.nz) {
        const uint32_t cls = probe ? pool_class_at(r.pool, r.g0[0] + i, r.g0[1] + j, r.g0[2] + k) : kClsMissing;
        if ((pass_mask >> cls) & 1u) e = tv_entry(d2 ? d2[(i * a.ny + j) * a.nz + k] : d2_fill, clearance, s2, penalty);
    }
    a.E[c] = e;
    a.cost[0][c] = kTvNone;
}

// ---- stage 2: the seeds ------------------------------------------------------------------------------------------------
// `far` = the most non-zero components of a move (1, 2, 3 at connectivity 6, 18, 26).  A seed on a face of its brick is
// a neighbour of voxels of the next brick, and no round will ever see the seed itself change: the bricks that touch it
// are marked here.
__global__ __launch_bounds__(256) void dm_tv_seed(TravelArgs a, const uint32_t *seeds, uint32_t n_seeds, int far) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_seeds) return;
    const uint32_t f = seeds[t];
    if (f >= a.n_cells) return;
    uint32_t b;
    const uint32_t c = tv_cell_of_flat(a, f, b);
    if (a.E[c] == kTvBlocked) return;
    if (atomicMin(&a.cost[0][c], 0u) == 0u) return;   // listed before
    atomicAdd(&a.totals[0], 1u);
    const uint32_t li = (c >> 6) & 7u, lj = (c >> 3) & 7u, lk = c & 7u;
    const uint32_t bk = b % a.BZ, brow = b / a.BZ, bj = brow % a.BY, bi = brow / a.BY;
    for (int di = -1; di <= 1; ++di)
        for (int dj = -1; dj <= 1; ++dj)
            for (int dk = -1; dk <= 1; ++dk) {   // the seed's own brick (0, 0, 0) and the bricks that touch the seed
                if ((di ? 1 : 0) + (dj ? 1 : 0) + (dk ? 1 : 0) > far) continue;
                const bool touches = (di == 0 || li == (di < 0 ? 0u : 7u)) && (dj == 0 || lj == (dj < 0 ? 0u : 7u)) &&
                                     (dk == 0 || lk == (dk < 0 ? 0u : 7u));
                const uint32_t qi = bi + (uint32_t)di, qj = bj + (uint32_t)dj, qk = bk + (uint32_t)dk;   // (bi - 1 wraps above BX)
                if (touches && qi < a.BX && qj < a.BY && qk < a.BZ) atomicOr(&a.active[0][(qi * a.BY + qj) * a.BZ + qk], 1u);
            }
}

// ---- stage 3: one round ------------------------------------------------------------------------------------------------
// `turn` = round & 1: side[turn] and active[turn] are this round's inputs, the other two its outputs.
template <int kConn>
__global__ __launch_bounds__(512) void dm_tv_round(TravelArgs a, uint32_t turn, uint32_t round) {
    __shared__ uint32_t tile[kTvTile];
    __shared__ uint32_t wave_mask[8], wave_count[8];
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    const uint32_t *__restrict__ side_in = tv_pick(a.side, turn);
    uint32_t *side_out = tv_pick(a.side, turn ^ 1u), *active_in = tv_pick(a.active, turn), *active_out = tv_pick(a.active, turn ^ 1u);
    const uint32_t s = side_in[b] & 1u, act = active_in[b];
    __syncthreads();                      // every lane has read active_in[b] before its owner clears it
    if (t == 0u && act) active_in[b] = 0u;
    if (!act) {                           // (uniform over the workgroup)
        if (t == 0u) side_out[b] = s;
        return;
    }
    const uint32_t bk = b % a.BZ, brow = b / a.BZ, bj = brow % a.BY, bi = brow / a.BY;
    // lane order: bits 0-2 lk, 3 lj & 1, 4 li & 1, 5-6 lj >> 1, 7-8 li >> 1 (the LDS banks, see above)
    const uint32_t lk = t & 7u, lj = ((t >> 3) & 1u) | (((t >> 5) & 3u) << 1), li = ((t >> 4) & 1u) | (((t >> 7) & 3u) << 1);
    const uint32_t cell = (b << 9) | (li << 6) | (lj << 3) | lk;
    const int own = (int)((li + 1u) * kTvSX + (lj + 1u) * kTvSY + lk + 1u);
    const uint32_t e = a.E[cell];
    uint32_t my = tv_pick(a.cost, s)[cell];
    tile[own] = my;
    // the halo: the tile's 1000 cells over the 512 lanes, two trips; interior cells are skipped
    for (uint32_t h = t; h < 1000u; h += 512u) {
        const uint32_t tk = h % 10u, tj = (h / 10u) % 10u, ti = h / 100u;
        const int oi = ti == 0u ? -1 : ti == 9u ? 1 : 0, oj = tj == 0u ? -1 : tj == 9u ? 1 : 0, ok = tk == 0u ? -1 : tk == 9u ? 1 : 0;
        if (oi == 0 && oj == 0 && ok == 0) continue;
        uint32_t v = kTvNone;
        const uint32_t qi = bi + (uint32_t)oi, qj = bj + (uint32_t)oj, qk = bk + (uint32_t)ok;   // (bi - 1 wraps above BX)
        if (tv_allowed<kConn>(oi, oj, ok) && qi < a.BX && qj < a.BY && qk < a.BZ) {
            const uint32_t q = (qi * a.BY + qj) * a.BZ + qk;
            v = tv_pick(a.cost, side_in[q] & 1u)[(q << 9) | (((ti + 7u) & 7u) << 6) | (((tj + 7u) & 7u) << 3) | ((tk + 7u) & 7u)];
        }
        tile[ti * kTvSX + tj * kTvSY + tk] = v;
    }
    __syncthreads();
    const bool open = e != kTvBlocked;
    bool ever = false;
    int any = 0;
#pragma unroll 1
    for (int it = 0; it < LA3DM_TRAVEL_INNER; ++it) {
        uint32_t best = my;
        if (open) {
#pragma unroll
            for (int di = -1; di <= 1; ++di)
#pragma unroll
                for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
                    for (int dk = -1; dk <= 1; ++dk) {
                        if (!tv_allowed<kConn>(di, dj, dk)) continue;
                        const uint32_t u = tile[own + di * kTvSX + dj * kTvSY + dk];
                        const uint32_t step = a.move[(di ? 1 : 0) + (dj ? 1 : 0) + (dk ? 1 : 0) - 1] + e;   // (a constant index after unrolling)
                        const uint32_t cand = u + step;   // u <= max_cost <= 2^31, step < 2^17: no overflow for a finite u
                        if (u != kTvNone && cand < best) best = cand;
                    }
        }
        const bool changed = best < my && best <= a.max_cost;
        any = __syncthreads_or(changed ? 1 : 0);   // (also: every lane has read before any lane writes)
        if (!any) break;
        if (changed) {
            my = best;
            tile[own] = best;
            ever = true;
        }
        __syncthreads();
    }
    // what the workgroup changed: the neighbour bricks that touch a changed voxel (bit q of the offset's code), the count
    uint32_t mask = 0u;
    if (ever) {
#pragma unroll
        for (int di = -1; di <= 1; ++di)
#pragma unroll
            for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
                for (int dk = -1; dk <= 1; ++dk) {
                    if (!tv_allowed<kConn>(di, dj, dk)) continue;
                    const bool touches = (di == 0 || li == (di < 0 ? 0u : 7u)) && (dj == 0 || lj == (dj < 0 ? 0u : 7u)) &&
                                         (dk == 0 || lk == (dk < 0 ? 0u : 7u));
                    if (touches) mask |= 1u << ((di + 1) * 9 + (dj + 1) * 3 + (dk + 1));
                }
    }
    uint32_t n = ever ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mask |= __shfl_xor(mask, o);
        n += __shfl_xor(n, o);
    }
    if ((t & 63u) == 0u) {
        wave_mask[t >> 6] = mask;
        wave_count[t >> 6] = n;
    }
    __syncthreads();
    uint32_t all_mask = 0u, all_n = 0u;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        all_mask |= wave_mask[w];
        all_n += wave_count[w];
    }
    const bool capped = any != 0;          // the last of LA3DM_TRAVEL_INNER iterations still changed a voxel
    if (t < 3u) {
        const uint32_t add = t == 0u ? all_n : t == 1u ? 1u : (capped ? 1u : 0u);
        if (add) atomicAdd(&a.count[round * kTvCountWords + t], add);
    }
    if (all_n == 0u) {                     // (uniform) a local fixed point already: nothing is written
        if (t == 0u) side_out[b] = s;
        return;
    }
    tv_pick(a.cost, s ^ 1u)[cell] = my;
    if (t == 0u) side_out[b] = s ^ 1u;
    if (t < 27u) {
        const int di = (int)(t / 9u) - 1, dj = (int)((t / 3u) % 3u) - 1, dk = (int)(t % 3u) - 1;
        const uint32_t qi = bi + (uint32_t)di, qj = bj + (uint32_t)dj, qk = bk + (uint32_t)dk;
        const bool wanted = t == 13u ? capped : ((all_mask >> t) & 1u) != 0u;
        if (wanted && qi < a.BX && qj < a.BY && qk < a.BZ) atomicOr(&active_out[(qi * a.BY + qj) * a.BZ + qk], 1u);
    }
}

// ---- stage 4: dense cost, parents, totals ------------------------------------------------------------------------------
// `side`: the array the last queued round wrote.  cost and parent may be null.  The parent of a reached voxel that is no
// seed is the smallest code q whose offset the connectivity allows, that stays in the region, and whose voxel u has a
// finite cost with cost[u] + move + pen(v) == cost[v]: the loops run in the order of q.
template <int kConn>
__global__ __launch_bounds__(256) void dm_tv_finish(TravelArgs a, const uint32_t *__restrict__ side, uint32_t *cost, uint8_t *parent) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    uint32_t c = kTvNone;
    if (f < a.n_cells) {
        const uint32_t k = f % a.nz, row = f / a.nz, j = row % a.ny, i = row / a.ny;
        uint32_t b;
        const uint32_t cell = tv_cell(a, i, j, k, b);
        c = tv_pick(a.cost, side[b] & 1u)[cell];
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
                            if (!tv_allowed<kConn>(di, dj, dk)) continue;
                            const uint32_t ui = i + (uint32_t)di, uj = j + (uint32_t)dj, uk = k + (uint32_t)dk;   // (0 - 1 wraps above nx)
                            if (found || ui >= a.nx || uj >= a.ny || uk >= a.nz) continue;
                            uint32_t ub;
                            const uint32_t ucell = tv_cell(a, ui, uj, uk, ub);
                            const uint32_t u = tv_pick(a.cost, side[ub] & 1u)[ucell];
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
    if (f < a.n_cells) {
        uint32_t b;
        const uint32_t cell = tv_cell_of_flat(a, f, b);
        c = tv_pick(a.cost, side[b] & 1u)[cell];
    }
    target_cost[t] = c;
}

}  // namespace la3dm_dev

#endif
