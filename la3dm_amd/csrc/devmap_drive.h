// devmap_drive.h — least cost of a ground route from seed voxels over the MEMBER voxels of a map region, with a parent
// per voxel (la3dm_devmap_drive_*, include/la3dm_hip.h; host twin and definition: host/drive_cells.h, called by
// BGKOctoMap::drive).  Integers throughout and a unique answer: the result equals the host form bit for bit.
//
// The scheme is devmap_brick.h's (bricks, two buffers, side / active words, rounds, Invariant and Termination) and the
// host side is its brick_layout and brick_rounds; the value is the cost and the rule min-plus relaxation with positive
// integer weights, as travel's.  What differs is the MOVE: from member u to member v = u + (a, b, c), (a, b) != (0, 0),
// |a|, |b| <= 1, |c| <= step <= 4.  brick_round's tile holds one voxel round the brick and its loop runs over {-1, 0, 1}^3,
// so drive has a sibling of it, drive_round, which differs in three places:
//
// LDS tile.  10 x 10 x 16 words: x and y from -1 to 8 of the brick, z from -4 to 11, own cell (li + 1, lj + 1, lk + 4).
//   The strides stay (168, 16, 1) — the largest index is 9 * 168 + 9 * 16 + 15 = 1671 < 1680 = kBrickTile — so
//   devmap_brick.h's bank argument carries over: with the same lane order the four 8-word z runs of a half wave start at
//   4, 20, 172 = 12 and 188 = 28 (mod 32), that is banks 4 - 11, 20 - 27, 12 - 19 and 28 - 31, 0 - 3: every bank once; the
//   shift of the own cell by 4 rotates the banks and nothing else.  A neighbour read adds one constant to every lane's
//   address.  The halo is the tile's 1600 cells less the brick's 512, from the up to 26 neighbour bricks: lk 4 .. 7 of the
//   brick below, lk 0 .. 3 of the brick above, all rows and columns; four trips of the 512 lanes.  Levels beyond `step`
//   and, at connectivity 4, the corner columns are never read by the loop below: they are filled with NONE, not loaded.
// Relaxation.  The 4 or 8 horizontal offsets times 2 step + 1 levels, unrolled: kConn and kStep are template arguments (10
//   instantiations).  A voxel takes u + move_cost[|a| + |b| - 1] + (the voxel lies above u ? climb_up : climb_down) * |c|
//   from a neighbour that holds a cost u; a non-member never holds one, so only the lane's own entry word is looked at.
// Waking.  A brick must run again whenever one of its voxels is within one move of a changed voxel.  Changed voxel (li,
//   lj, 7) with a member at (li + 1, lj, 9) wakes the brick above although li + 1 <= 7: the bricks straight above and below
//   are neighbours as soon as step >= 1, and the test along z is lk < step / lk >= 8 - step (drive_touches), not the face
//   test of brick_touches.  Along x and y it is the face test.  Waking too much costs a run; waking too little is a wrong
//   answer.  The seed kernel marks by the same rule.
//
// dm_dr_clear    one lane per cell of the bricks: E = blocked, cost = NONE in buffer 0.
// dm_dr_members  list mode: one lane per list entry; range test, then a plain store of E = 0 (a voxel listed twice is
//                stored twice: the same word).
// dm_dr_foot     footing mode: one lane per voxel of the region; E = 0 where the voxel's bit is set in footing's foot words
//                (devmap_footing.h: bit ((i + r) PY + j + r) PZ + k + 1 + s of the stream).
// dm_dr_seed     one lane per seed: range test, the snap loop of at most 33 reads of E, atomicMin of the cost to 0; the
//                old value tells whether the member is new: only then it is counted and its bricks are marked.
// dm_dr_round    the hot kernel: drive_round, at most LA3DM_DRIVE_INNER iterations per run.
// dm_dr_finish   one lane per voxel of the region: dense cost and the parent, searched in the order of its code; n_members
//                (E == 0), n_reached and max_cost, one atomic each per wave.
// dm_dr_gather   one lane per target (the snap loop again) and per list entry (of_member).
//
// Every loop is bounded by a constant (the unrolled offsets, 33 snap reads, 1600 tile cells, kInner, 6 shuffle steps) and
// no array is indexed at run time: nothing lives in scratch.
#ifndef LA3DM_DEVMAP_DRIVE_H
#define LA3DM_DEVMAP_DRIVE_H

#include "devmap_brick.h"
#include "devmap_footing.h"

namespace la3dm_dev {

static_assert(LA3DM_DRIVE_BRICK == 8 && LA3DM_DRIVE_NONE == kBrickNone, "devmap_brick.h: bricks of 8 x 8 x 8, NONE the largest word");
static_assert(LA3DM_DRIVE_MAX_STEP == 4 && 9 * kBrickSX + 9 * kBrickSY + 8 + 2 * LA3DM_DRIVE_MAX_STEP <= kBrickTile, "the 10 x 10 x 16 tile");
constexpr uint32_t kDrNone = LA3DM_DRIVE_NONE, kDrBlocked = 0xFFFFFFFFu, kDrMember = 0u;
constexpr int kDrZ = LA3DM_DRIVE_MAX_STEP;   // levels of halo below and above the brick

struct DriveArgs {
    BrickGrid g;                  // val = the cost
    uint32_t *E;                  // [n_bricks * 512] entry words: kDrMember or kDrBlocked
    uint32_t *totals;             // n_seeded, n_reached, max_cost, n_members
    uint32_t move[2];             // cost of a move with |a| + |b| = 1, 2
    uint32_t up, down;            // per voxel climbed, dropped
    uint32_t max_cost;
    uint32_t snap;
};

template <int kConn>
__device__ __forceinline__ constexpr bool drive_flat_allowed(int a, int b) {
    const int m = (a ? 1 : 0) + (b ? 1 : 0);
    return m >= 1 && m <= (kConn == 4 ? 1 : 2);
}

// what a voxel pays to be entered from the neighbour at offset (a, b, c) FROM it: the move runs the other way, so the voxel
// lies above the neighbour where c < 0
__device__ __forceinline__ uint32_t drive_move(const DriveArgs &a, int da, int db, int dc) {
    const uint32_t flat = (da ? 1 : 0) + (db ? 1 : 0) == 1 ? a.move[0] : a.move[1];
    return flat + (dc < 0 ? a.up * (uint32_t)(-dc) : a.down * (uint32_t)dc);
}

// may a voxel of the neighbour brick at (di, dj, dk) lie within one move of voxel (li, lj, lk) of this brick?
template <int kConn, int kStep>
__device__ __forceinline__ constexpr bool drive_touches(int di, int dj, int dk, uint32_t li, uint32_t lj, uint32_t lk) {
    if (di == 0 && dj == 0 && dk == 0) return false;
    if (kConn == 4 && di != 0 && dj != 0) return false;
    if (kStep == 0 && dk != 0) return false;
    return (di == 0 || li == (di < 0 ? 0u : 7u)) && (dj == 0 || lj == (dj < 0 ? 0u : 7u)) &&
           (dk == 0 || (dk < 0 ? lk < (uint32_t)kStep : lk >= 8u - (uint32_t)kStep));
}

// ---- stage 1: the entry words ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dm_dr_clear(DriveArgs a) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;   // n_bricks * 512 <= 2^28: no overflow; the grid covers the cells exactly
    a.E[c] = kDrBlocked;
    a.g.val[0][c] = kDrNone;
}

__global__ __launch_bounds__(256) void dm_dr_members(DriveArgs a, const uint32_t *__restrict__ members, uint32_t n_members) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_members) return;
    const uint32_t f = members[t];
    if (f >= a.g.n_cells) return;
    uint32_t b;
    a.E[brick_cell_of_flat(a.g, f, b)] = kDrMember;
}

// `foot`: footing's foot words over its padded box (PY, PZ, r, s as FootingArgs has them)
__global__ __launch_bounds__(256) void dm_dr_foot(DriveArgs a, const uint32_t *__restrict__ foot, uint32_t PY, uint32_t PZ, uint32_t r, uint32_t s) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= a.g.n_cells) return;
    const uint32_t k = f % a.g.nz, row = f / a.g.nz, j = row % a.g.ny, i = row / a.g.ny;
    const uint32_t p = ((i + r) * PY + (j + r)) * PZ + k + 1u + s;   // < the padded box's voxels <= 2^28
    if (((foot[p >> 5] >> (p & 31u)) & 1u) == 0u) return;
    uint32_t b;
    a.E[brick_cell(a.g, i, j, k, b)] = kDrMember;
}

// the member that flat index f stands for: (i, j, k') with the largest k' in [max(0, k - snap), k].  false where f is out of
// range or there is none; else cell = its brick-major cell, b its brick, fm its flat index.
__device__ __forceinline__ bool drive_snap(const DriveArgs &a, uint32_t f, uint32_t &cell, uint32_t &b, uint32_t &fm) {
    if (f >= a.g.n_cells) return false;
    const uint32_t k = f % a.g.nz, row = f / a.g.nz, j = row % a.g.ny, i = row / a.g.ny;
    const uint32_t reach = k < a.snap ? k : a.snap;
#pragma unroll 1
    for (uint32_t t = 0; t <= reach; ++t) {   // at most LA3DM_DRIVE_MAX_SNAP + 1 trips
        cell = brick_cell(a.g, i, j, k - t, b);
        if (a.E[cell] == kDrMember) {
            fm = f - t;
            return true;
        }
    }
    return false;
}

// ---- stage 2: the seeds ------------------------------------------------------------------------------------------------
// No round will ever see a seed itself change: its own brick and the bricks within one move of it are marked here.
template <int kConn, int kStep>
__global__ __launch_bounds__(256) void dm_dr_seed(DriveArgs a, const uint32_t *__restrict__ seeds, uint32_t n_seeds) {
    const BrickGrid &g = a.g;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_seeds) return;
    uint32_t c, b, fm;
    if (!drive_snap(a, seeds[t], c, b, fm)) return;
    if (atomicMin(&g.val[0][c], 0u) == 0u) return;   // seeded before
    atomicAdd(&a.totals[0], 1u);
    const uint32_t li = (c >> 6) & 7u, lj = (c >> 3) & 7u, lk = c & 7u;
    const uint32_t bk = b % g.BZ, brow = b / g.BZ, bj = brow % g.BY, bi = brow / g.BY;
#pragma unroll
    for (int di = -1; di <= 1; ++di)
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
            for (int dk = -1; dk <= 1; ++dk) {
                if (!((di | dj | dk) == 0 || drive_touches<kConn, kStep>(di, dj, dk, li, lj, lk))) continue;
                const uint32_t qi = bi + (uint32_t)di, qj = bj + (uint32_t)dj, qk = bk + (uint32_t)dk;   // (bi - 1 wraps above BX)
                if (qi < g.BX && qj < g.BY && qk < g.BZ) atomicOr(&g.active[0][(qi * g.BY + qj) * g.BZ + qk], 1u);
            }
}

// ---- stage 3: one round ------------------------------------------------------------------------------------------------
// The sibling of brick_round (devmap_brick.h), whose protocol on side, active and count it keeps word for word.  The
// arguments are taken BY VALUE for brick_round's reason.
template <int kConn, int kStep, int kInner>
__device__ __forceinline__ void drive_round(const DriveArgs a, uint32_t turn, uint32_t round) {
    __shared__ uint32_t tile[kBrickTile];
    __shared__ uint32_t wave_mask[8], wave_count[8];
    const BrickGrid g = a.g;
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    const uint32_t *__restrict__ side_in = brick_pick(g.side, turn);
    uint32_t *side_out = brick_pick(g.side, turn ^ 1u), *active_in = brick_pick(g.active, turn), *active_out = brick_pick(g.active, turn ^ 1u);
    const uint32_t s = side_in[b] & 1u, act = active_in[b];
    __syncthreads();                      // every lane has read active_in[b] before its owner clears it
    if (t == 0u && act) active_in[b] = 0u;
    if (!act) {                           // (uniform over the workgroup)
        if (t == 0u) side_out[b] = s;
        return;
    }
    const uint32_t bk = b % g.BZ, brow = b / g.BZ, bj = brow % g.BY, bi = brow / g.BY;
    // lane order: bits 0-2 lk, 3 lj & 1, 4 li & 1, 5-6 lj >> 1, 7-8 li >> 1 (the LDS banks, see above)
    const uint32_t lk = t & 7u, lj = ((t >> 3) & 1u) | (((t >> 5) & 3u) << 1), li = ((t >> 4) & 1u) | (((t >> 7) & 3u) << 1);
    const uint32_t cell = (b << 9) | (li << 6) | (lj << 3) | lk;
    const int own = (int)((li + 1u) * kBrickSX + (lj + 1u) * kBrickSY + lk + (uint32_t)kDrZ);
    uint32_t my = brick_pick(g.val, s)[cell];
    const bool open = a.E[cell] == kDrMember;
    tile[own] = my;
    // the halo: the tile's 1600 cells over the 512 lanes, four trips; interior cells are skipped
#pragma unroll 1
    for (uint32_t h = t; h < 1600u; h += 512u) {
        const uint32_t tz = h & 15u, tj = (h >> 4) % 10u, ti = h / 160u;
        const int oi = ti == 0u ? -1 : ti == 9u ? 1 : 0, oj = tj == 0u ? -1 : tj == 9u ? 1 : 0;
        const int ok = tz < (uint32_t)kDrZ ? -1 : tz >= 8u + (uint32_t)kDrZ ? 1 : 0;
        if (oi == 0 && oj == 0 && ok == 0) continue;
        uint32_t v = kDrNone;
        const uint32_t qi = bi + (uint32_t)oi, qj = bj + (uint32_t)oj, qk = bk + (uint32_t)ok;   // (bi - 1 wraps above BX)
        const bool read = (kConn == 8 || oi == 0 || oj == 0) && tz >= (uint32_t)(kDrZ - kStep) && tz < (uint32_t)(8 + kDrZ + kStep);
        if (read && qi < g.BX && qj < g.BY && qk < g.BZ) {
            const uint32_t q = (qi * g.BY + qj) * g.BZ + qk;
            v = brick_pick(g.val, side_in[q] & 1u)[(q << 9) | (((ti + 7u) & 7u) << 6) | (((tj + 7u) & 7u) << 3) | ((tz + 8u - (uint32_t)kDrZ) & 7u)];
        }
        tile[ti * kBrickSX + tj * kBrickSY + tz] = v;
    }
    __syncthreads();
    bool ever = false;
    int any = 0;
#pragma unroll 1
    for (int it = 0; it < kInner; ++it) {
        uint32_t best = my;
        if (open) {
#pragma unroll
            for (int da = -1; da <= 1; ++da)
#pragma unroll
                for (int db = -1; db <= 1; ++db)
#pragma unroll
                    for (int dc = -kStep; dc <= kStep; ++dc) {
                        if (!drive_flat_allowed<kConn>(da, db)) continue;
                        const uint32_t u = tile[own + da * kBrickSX + db * kBrickSY + dc];
                        const uint32_t cand = u + drive_move(a, da, db, dc);   // u <= max_cost <= 2^31, the move <= 5 * 2^16: no overflow for a finite u
                        best = u != kDrNone && cand < best ? cand : best;
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
    // what the workgroup changed: the neighbour bricks within one move of a changed voxel (bit q of the offset's code), the count
    uint32_t mask = 0u;
    if (ever) {
#pragma unroll
        for (int di = -1; di <= 1; ++di)
#pragma unroll
            for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
                for (int dk = -1; dk <= 1; ++dk)
                    if (drive_touches<kConn, kStep>(di, dj, dk, li, lj, lk)) mask |= 1u << ((di + 1) * 9 + (dj + 1) * 3 + (dk + 1));
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
    const bool capped = any != 0;          // the last of kInner iterations still changed a voxel
    if (t < 3u) {
        const uint32_t add = t == 0u ? all_n : t == 1u ? 1u : (capped ? 1u : 0u);
        if (add) atomicAdd(&g.count[round * kBrickCountWords + t], add);
    }
    if (all_n == 0u) {                     // (uniform) a local fixed point already: nothing is written
        if (t == 0u) side_out[b] = s;
        return;
    }
    brick_pick(g.val, s ^ 1u)[cell] = my;
    if (t == 0u) side_out[b] = s ^ 1u;
    if (t < 27u) {
        const int di = (int)(t / 9u) - 1, dj = (int)((t / 3u) % 3u) - 1, dk = (int)(t % 3u) - 1;
        const uint32_t qi = bi + (uint32_t)di, qj = bj + (uint32_t)dj, qk = bk + (uint32_t)dk;
        const bool wanted = t == 13u ? capped : ((all_mask >> t) & 1u) != 0u;
        if (wanted && qi < g.BX && qj < g.BY && qk < g.BZ) atomicOr(&active_out[(qi * g.BY + qj) * g.BZ + qk], 1u);
    }
}

template <int kConn, int kStep>
__global__ __launch_bounds__(512) void dm_dr_round(DriveArgs a, uint32_t turn, uint32_t round) {
    drive_round<kConn, kStep, LA3DM_DRIVE_INNER>(a, turn, round);
}

// ---- stage 4: dense cost, parents, totals ------------------------------------------------------------------------------
// `side`: the array the last queued round wrote.  cost and parent may be null.  The parent of a reached member that is no
// seed: the loops run over the offsets o = u - v in the order of their code q, and the move u -> v is -o.
template <int kConn, int kStep>
__global__ __launch_bounds__(256) void dm_dr_finish(DriveArgs a, const uint32_t *__restrict__ side, uint32_t *cost, uint8_t *parent) {
    const BrickGrid &g = a.g;
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    uint32_t c = kDrNone;
    bool member = false;
    if (f < g.n_cells) {
        const uint32_t k = f % g.nz, row = f / g.nz, j = row % g.ny, i = row / g.ny;
        uint32_t b;
        const uint32_t cell = brick_cell(g, i, j, k, b);
        c = brick_pick(g.val, side[b] & 1u)[cell];
        member = a.E[cell] == kDrMember;
        if (cost) cost[f] = c;
        if (parent) {
            uint32_t code = c == kDrNone ? 255u : 40u;
            if (c != kDrNone && c != 0u) {
                bool found = false;
#pragma unroll
                for (int da = -1; da <= 1; ++da)
#pragma unroll
                    for (int db = -1; db <= 1; ++db)
#pragma unroll
                        for (int dc = -kStep; dc <= kStep; ++dc) {
                            if (!drive_flat_allowed<kConn>(da, db)) continue;
                            const uint32_t ui = i + (uint32_t)da, uj = j + (uint32_t)db, uk = k + (uint32_t)dc;   // (0 - 1 wraps above nx)
                            if (found || ui >= g.nx || uj >= g.ny || uk >= g.nz) continue;
                            uint32_t ub;
                            const uint32_t ucell = brick_cell(g, ui, uj, uk, ub);
                            const uint32_t u = brick_pick(g.val, side[ub] & 1u)[ucell];
                            if (u != kDrNone && u + drive_move(a, da, db, dc) == c) {   // (a finite cost: a member)
                                code = (uint32_t)(((da + 1) * 3 + (db + 1)) * 9 + (dc + kDrZ));
                                found = true;
                            }
                        }
            }
            parent[f] = (uint8_t)code;
        }
    }
    // the wave's totals, one atomic each per wave; every lane of the wave arrives here
    if (__ballot(member) == 0ull) return;
    uint32_t m = member ? 1u : 0u, n = c != kDrNone ? 1u : 0u, most = c != kDrNone ? c : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m += __shfl_xor(m, o);
        n += __shfl_xor(n, o);
        most = max(most, __shfl_xor(most, o));
    }
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(&a.totals[3], m);
        if (n) {
            atomicAdd(&a.totals[1], n);
            atomicMax(&a.totals[2], most);
        }
    }
}

// ---- stage 5: the targets and the list entries ----------------------------------------------------------------------
// lanes [0, n_targets): the targets; lanes [n_targets, n_targets + n_members): of_member (members = null: none)
__global__ __launch_bounds__(256) void dm_dr_gather(DriveArgs a, const uint32_t *__restrict__ side, const uint32_t *__restrict__ targets,
                                                    uint32_t n_targets, uint32_t *target_cost, uint32_t *target_index,
                                                    const uint32_t *__restrict__ members, uint32_t n_members, uint32_t *of_member) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;   // n_targets + n_members <= 2^29
    if (t < n_targets) {
        uint32_t cell, b, fm = kDrNone, c = kDrNone;
        if (drive_snap(a, targets[t], cell, b, fm)) c = brick_pick(a.g.val, side[b] & 1u)[cell];
        if (target_cost) target_cost[t] = c;
        if (target_index) target_index[t] = fm;
    } else if (t - n_targets < n_members) {
        const uint32_t f = members[t - n_targets];
        uint32_t c = kDrNone;
        if (f < a.g.n_cells) {
            uint32_t b;
            const uint32_t cell = brick_cell_of_flat(a.g, f, b);
            c = brick_pick(a.g.val, side[b] & 1u)[cell];
        }
        of_member[t - n_targets] = c;
    }
}

}  // namespace la3dm_dev

#endif
