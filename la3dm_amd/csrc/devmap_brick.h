// devmap_brick.h — relaxation to a fixed point over a map region cut into bricks: the scheme that travel
// (devmap_travel.h) and clusters (devmap_clusters.h) share.  A query keeps one 32-bit VALUE per voxel (a cost, a label)
// and a RULE that lowers the value of a voxel from the values of its neighbours.  The rule must be monotone (values only
// fall) and have a fixed point that is unique whatever order the relaxations run in; then a workgroup may relax a brick
// of voxels to its LOCAL fixed point in LDS before anything is written back, and a global round moves the wave by a
// brick, not by a voxel.  NONE = 0xFFFFFFFF is the value of a voxel that has none.
//
// The values are kept BRICK-MAJOR: the region is rounded up to whole bricks of 8 x 8 x 8 voxels, brick b = (bi BY + bj)
// BZ + bk holds the 512 consecutive words b * 512 + (li * 8 + lj) * 8 + lk, and cells outside the region never open.
// There are two value buffers; side[b] names the one that holds brick b's current values.  One workgroup owns one brick.
//
// brick_round   the body of a query's hot kernel: one workgroup of 512 lanes per brick, for every brick.  Reads
//               side_in[b] and active_in[b], then clears active_in[b].  An inactive brick copies its side to side_out[b]
//               and leaves.  An active brick loads its 512 values from buffer side_in[b] and the one-voxel halo from its
//               up to 26 neighbour bricks, each from the buffer THAT brick's side_in names, into a 10 x 10 x 10 tile in
//               LDS, and relaxes there — Jacobi: every lane reads its neighbours, a barrier (__syncthreads_or of
//               "changed"), every changed lane writes, a barrier — until no lane changes or kInner iterations have run.
//               If nothing changed: side_out[b] = side_in[b] and nothing else is written.  Otherwise the 512 values go to
//               the OTHER buffer, side_out[b] flips, active_out is ORed for every neighbour brick the rule joins to this
//               one that touches a changed voxel (and for the brick itself where the cap stopped it), and the changed
//               voxels are added to count[round].
//
// A Rule is a small struct whose members are all inlined (TravelRule, ClustersRule):
//   void     brick(bi, bj, bk)     once per active brick, before anything else
//   bool     open(cell, my)        may this lane's voxel take a value from a neighbour?  (may load what relax needs)
//   bool     joined(qi, qj, qk)    is neighbour brick q (inside the grid) connected to this one?  Asked for the halo load
//                                  and for the activation alike: a brick that is not read is not woken
//   uint32_t relax(best, u, m)     the better of `best` and the candidate through a neighbour that holds u, over a move
//                                  with m = 1, 2, 3 non-zero components (a constant after unrolling)
//   bool     keep(best)            may a lower value `best` be stored?
//
// LDS tile.  ds_read_b32 banks are (address / 4) % 32 and the two 32-lane halves of a wave conflict among themselves
// only.  Strides (x, y, z) = (168, 16, 1) and a lane order whose low five bits are lk (3 bits), lj & 1, li & 1 put the
// four 8-word z runs of a half wave at 0, 16, 168 = 8 and 184 = 24 (mod 32): every bank once.  A neighbour read adds the
// same constant to every lane's address, so it is conflict-free too.  10 x 168 words = 6720 bytes.
//
// Invariant.  Within a launch of a round kernel, side_in, both roles of `active` and buffer side_in[b] of every brick
// are only read — but for each owner clearing its own active_in word, which no other workgroup reads.  Only the owner
// of b writes buffer 1 - side_in[b] of b and side_out[b].  No word is read by one workgroup and written by another in
// the same launch.  The round's only atomics are the ORs into active_out and the per-workgroup adds into count[round]
// (changed voxels, brick runs, capped runs: three lanes, one instruction).  There is no grid barrier, no cooperative
// launch and no spin.
// Termination.  Every stored value is one the rule built from stored values, and values only fall.  An inactive brick
// ended its last run at a local fixed point and has seen no neighbour change since.  So count[round] == 0 — no voxel
// changed, hence no brick was marked — means the rule's equations hold everywhere: the values are the fixed point.
// Rounds queued behind that one find every brick inactive and only copy `side`.
//
// Every loop is bounded by a constant: 27 offsets, the tile's 1000 cells, kInner, 6 shuffle steps.  No array is indexed
// at run time: nothing lives in scratch.
#ifndef LA3DM_DEVMAP_BRICK_H
#define LA3DM_DEVMAP_BRICK_H

#include "devmap_pool.h"
#include "devmap_region.h"
#include "host/region_contract.h"

namespace la3dm_dev {

constexpr uint32_t kBrickNone = 0xFFFFFFFFu;
constexpr int kBrickSY = 16, kBrickSX = 168, kBrickTile = 10 * kBrickSX;   // LDS strides of the 10 x 10 x 10 tile (see above)
constexpr uint32_t kBrickCountWords = 4;   // per round: changed voxels, brick runs, capped runs, -

struct BrickGrid {
    uint32_t nx, ny, nz;
    uint32_t BX, BY, BZ;          // bricks per axis
    uint32_t n_bricks;            // BX BY BZ <= 2^19
    uint32_t n_cells;             // nx ny nz
    uint32_t *val[2];             // [n_bricks * 512] each, brick-major
    uint32_t *side[2];            // [n_bricks] each: which buffer holds the brick (the two arrays take turns)
    uint32_t *active[2];          // [n_bricks] each
    uint32_t *count;              // [rounds][kBrickCountWords]
};

// brick-major cell of voxel (i, j, k) of the region
__device__ __forceinline__ uint32_t brick_cell(const BrickGrid &g, uint32_t i, uint32_t j, uint32_t k, uint32_t &brick) {
    brick = ((i >> 3) * g.BY + (j >> 3)) * g.BZ + (k >> 3);
    return (brick << 9) | ((i & 7u) << 6) | ((j & 7u) << 3) | (k & 7u);
}

__device__ __forceinline__ uint32_t brick_cell_of_flat(const BrickGrid &g, uint32_t f, uint32_t &brick) {
    const uint32_t k = f % g.nz, row = f / g.nz;
    return brick_cell(g, row / g.ny, row % g.ny, k, brick);
}

// voxel (i, j, k) of cell `local` < 512 of brick b, that is of brick-major cell b * 512 + local; it may lie outside the region
__device__ __forceinline__ void brick_coords(const BrickGrid &g, uint32_t b, uint32_t local, uint32_t &i, uint32_t &j, uint32_t &k) {
    const uint32_t brow = b / g.BZ;
    i = (brow / g.BY) * 8u + (local >> 6);
    j = (brow % g.BY) * 8u + ((local >> 3) & 7u);
    k = (b % g.BZ) * 8u + (local & 7u);
}

// one of a pair by a run-time index, as a select of the two VALUES: an array indexed at run time would live in scratch,
// and a select of the two addresses becomes an indexed load from the kernel's arguments, one more trip to memory
template <class T>
__device__ __forceinline__ T brick_pick(T const (&pair)[2], uint32_t which) {
    return which ? pair[1] : pair[0];
}

template <int kConn>
__device__ __forceinline__ constexpr bool brick_allowed(int di, int dj, int dk) {
    const int m = (di ? 1 : 0) + (dj ? 1 : 0) + (dk ? 1 : 0);
    return m >= 1 && m <= la3dm_region::move_reach(kConn);
}

// does voxel (li, lj, lk) of a brick lie on the face, edge or corner towards the neighbour brick at (di, dj, dk)?
__device__ __forceinline__ constexpr bool brick_touches(int di, int dj, int dk, uint32_t li, uint32_t lj, uint32_t lk) {
    return (di == 0 || li == (di < 0 ? 0u : 7u)) && (dj == 0 || lj == (dj < 0 ? 0u : 7u)) && (dk == 0 || lk == (dk < 0 ? 0u : 7u));
}

// One round of one brick.  `turn` = round & 1: side[turn] and active[turn] are this round's inputs, the other two its
// outputs.  Called by every lane of a workgroup of 512, once per kernel.  The grid is taken BY VALUE: through a reference
// to the kernel's argument the compiler turns brick_pick in the halo loop into an indexed load from the argument segment —
// one more dependent trip to memory per halo cell (seen in the ISA: one more global_load in each of the six kernels).
template <int kConn, int kInner, class Rule>
__device__ __forceinline__ void brick_round(const BrickGrid g, uint32_t turn, uint32_t round, Rule rule) {
    __shared__ uint32_t tile[kBrickTile];
    __shared__ uint32_t wave_mask[8], wave_count[8];
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
    rule.brick(bi, bj, bk);
    // lane order: bits 0-2 lk, 3 lj & 1, 4 li & 1, 5-6 lj >> 1, 7-8 li >> 1 (the LDS banks, see above)
    const uint32_t lk = t & 7u, lj = ((t >> 3) & 1u) | (((t >> 5) & 3u) << 1), li = ((t >> 4) & 1u) | (((t >> 7) & 3u) << 1);
    const uint32_t cell = (b << 9) | (li << 6) | (lj << 3) | lk;
    const int own = (int)((li + 1u) * kBrickSX + (lj + 1u) * kBrickSY + lk + 1u);
    uint32_t my = brick_pick(g.val, s)[cell];
    const bool open = rule.open(cell, my);
    tile[own] = my;
    // the halo: the tile's 1000 cells over the 512 lanes, two trips; interior cells are skipped
    for (uint32_t h = t; h < 1000u; h += 512u) {
        const uint32_t tk = h % 10u, tj = (h / 10u) % 10u, ti = h / 100u;
        const int oi = ti == 0u ? -1 : ti == 9u ? 1 : 0, oj = tj == 0u ? -1 : tj == 9u ? 1 : 0, ok = tk == 0u ? -1 : tk == 9u ? 1 : 0;
        if (oi == 0 && oj == 0 && ok == 0) continue;
        uint32_t v = kBrickNone;
        const uint32_t qi = bi + (uint32_t)oi, qj = bj + (uint32_t)oj, qk = bk + (uint32_t)ok;   // (bi - 1 wraps above BX)
        if (brick_allowed<kConn>(oi, oj, ok) && qi < g.BX && qj < g.BY && qk < g.BZ && rule.joined(qi, qj, qk)) {
            const uint32_t q = (qi * g.BY + qj) * g.BZ + qk;
            v = brick_pick(g.val, side_in[q] & 1u)[(q << 9) | (((ti + 7u) & 7u) << 6) | (((tj + 7u) & 7u) << 3) | ((tk + 7u) & 7u)];
        }
        tile[ti * kBrickSX + tj * kBrickSY + tk] = v;
    }
    __syncthreads();
    bool ever = false;
    int any = 0;
#pragma unroll 1
    for (int it = 0; it < kInner; ++it) {
        uint32_t best = my;
        if (open) {
#pragma unroll
            for (int di = -1; di <= 1; ++di)
#pragma unroll
                for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
                    for (int dk = -1; dk <= 1; ++dk) {
                        if (!brick_allowed<kConn>(di, dj, dk)) continue;
                        best = rule.relax(best, tile[own + di * kBrickSX + dj * kBrickSY + dk], (di ? 1 : 0) + (dj ? 1 : 0) + (dk ? 1 : 0));
                    }
        }
        const bool changed = best < my && rule.keep(best);
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
                for (int dk = -1; dk <= 1; ++dk)
                    if (brick_allowed<kConn>(di, dj, dk) && brick_touches(di, dj, dk, li, lj, lk)) mask |= 1u << ((di + 1) * 9 + (dj + 1) * 3 + (dk + 1));
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
        if (wanted && qi < g.BX && qj < g.BY && qk < g.BZ && rule.joined(qi, qj, qk)) atomicOr(&active_out[(qi * g.BY + qj) * g.BZ + qk], 1u);
    }
}

}  // namespace la3dm_dev

#endif
