// devmap_clusters.h — connected groups of a region's member voxels on the device-resident block pool, optionally
// confined to tiles and cut at a minimum size: a dense label and a record per cluster (la3dm_devmap_clusters_*,
// include/la3dm_hip.h; host twin and definition: BGKOctoMap::clusters, host/bgkoctomap.cpp).  Integers throughout and
// a unique answer: the result equals the host form bit for bit.
//
// travel's scheme (devmap_travel.h) with min in place of min-plus.  The label of a member starts as its own flat
// index f = (i ny + j) nz + k; a non-member holds NONE = 0xFFFFFFFF, the identity of min.  The fixed point of "take the
// smallest label among yourself and your adjacent members" gives every member the smallest flat index of its cluster
// — its `first` — whatever order the relaxations run in, so a workgroup may relax a brick to its LOCAL fixed point in
// LDS before anything is written back.
//
// The labels are kept BRICK-MAJOR as travel's costs are (tv_cell): the region is rounded up to whole bricks of 8 x 8 x 8
// voxels, cells outside the region are non-members, there are two label buffers and side[b] names the one that holds
// brick b.  A tile is a whole number of bricks (tile % 8 == 0, `tb` bricks per axis), so a brick never straddles one:
// a halo cell of a brick in another tile reads as a non-member, and such a brick is never activated from here.
//
// dm_cl_enter    from_list 0.  One lane per cell of the bricks: the pool probe (pool_class_at), the mask; label = own
//                flat index or NONE into buffer 0; a wave that holds a member marks its brick active (a plain store of 1).
// dm_cl_list     from_list 1, after buffer 0 was cleared to NONE.  One lane per list entry: range test, class test, then
//                the voxel's own index is stored — idempotent, so an entry listed twice needs no atomic — and 1 into the
//                brick's active word.
// dm_cl_round    the hot kernel: one workgroup of 512 lanes per brick, for every brick; dm_tv_round with min.  An inactive
//                brick copies its side and leaves.  An active one loads its labels and the one-voxel halo into a 10 x 10
//                x 10 tile in LDS (travel's strides: no bank conflict), runs Jacobi until no lane changes or
//                LA3DM_CLUSTERS_INNER iterations have run, writes the other buffer if a voxel changed, ORs active_out for
//                the neighbour bricks of its tile that touch a changed voxel (and for itself where the cap stopped it)
//                and adds to count[round].
// dm_cl_sizes    one workgroup per brick: size[root] += the lanes of a wave that share the root, one atomic per group.
// dm_cl_flags    one lane per voxel: root (label == own index), flag = root with size >= min_size; n_members, n_dropped
//                and largest from the roots, reduced per wave.  The map's one-launch scan (devmap_scan.h) over the flags
//                then numbers the kept roots in ascending order of their index.
// dm_cl_label    one lane per voxel: label = number[root] where the root is kept, else NONE.
// dm_cl_gather   one lane per list entry: the same for of_member.
// dm_cl_rec_init, dm_cl_records, dm_cl_rep, dm_cl_emit   the records of clusters c < min(n, cap): see "Accumulators".
//
// Accumulators.  An atomic on one address costs about 29 ns, serialised, and an untiled cluster may hold most of the
// members: adding a box and three sums voxel by voxel would be a chain of milliseconds.  The lanes of a wave are 64
// consecutive cells of a brick (one li, 8 lj, 8 lk), which almost always share a root; so every accumulating kernel
// first groups its wave by cluster — the lowest pending lane names a cluster, a ballot finds the lanes that share it,
// six xor-shuffle steps reduce their values — and only the group's first lane issues the atomics: one per wave, cluster
// and word.  rep is a second pass once the sums are final: key = squared distance to the rounded centroid << 32 | flat
// index (an axis is at most 2^15 long: 3 x 2^30 fits 32 bits), a wave-and-cluster minimum, one 64-bit atomicMin.
//
// Invariant.  Within a launch of dm_cl_round, side_in, both roles of `active` and buffer side_in[b] of every brick are
// only read — but for each owner clearing its own active_in word, which no other workgroup reads.  Only the owner of b
// writes buffer 1 - side_in[b] of b and side_out[b].  In the finish every launch reads words that earlier launches
// completed and accumulates, by atomics alone, into words it does not read (dm_cl_sizes: size; dm_cl_flags: totals;
// dm_cl_records: lo, hi, sum — first and size have one writer, the root's lane; dm_cl_rep: key).  No word is read by one
// workgroup and written by another in the same launch.  There is no grid barrier, no cooperative launch and no spin
// in this file (the scan is the map's own).
// Termination.  Labels only fall, and every stored label is the index of a member connected to the voxel.  An inactive
// brick ended its last run at a local fixed point and has seen no neighbour change since, so count[round] == 0 means
// every member holds the minimum of its neighbourhood: the cluster's smallest index.
//
// Every loop is bounded by a constant: 27 offsets, the tile's 1000 cells, LA3DM_CLUSTERS_INNER, 6 shuffle steps, 64
// groups of a wave.  No array is indexed at run time: nothing lives in scratch.
#ifndef LA3DM_DEVMAP_CLUSTERS_H
#define LA3DM_DEVMAP_CLUSTERS_H

#include "devmap_pool.h"
#include "devmap_region.h"
#include "devmap_travel.h"   // tv_pick, tv_allowed, the tile's strides

namespace la3dm_dev {

constexpr uint32_t kClNone = LA3DM_CLUSTERS_NONE;
constexpr uint32_t kClCountWords = 4;   // per round: changed voxels, brick runs, capped runs, -
constexpr uint32_t kClNoTile = 1u << 20;   // `tb` of an untiled query: more bricks than an axis holds

struct ClustersArgs {
    uint32_t nx, ny, nz;
    uint32_t BX, BY, BZ;          // bricks per axis
    uint32_t n_bricks;            // BX BY BZ <= 2^19
    uint32_t n_cells;             // nx ny nz
    uint32_t tb;                  // bricks per tile and axis (kClNoTile: untiled)
    uint32_t min_size;
    uint32_t *lab[2];             // [n_bricks * 512] each, brick-major
    uint32_t *side[2];            // [n_bricks] each: which buffer holds the brick (the two arrays take turns)
    uint32_t *active[2];          // [n_bricks] each
    uint32_t *count;              // [rounds][kClCountWords]
    uint32_t *totals;             // n_members, n_dropped, largest
    uint32_t *size;               // [n_cells] members of the cluster whose root is voxel f
    uint32_t *flag;               // [n_cells + 1] kept root
    uint32_t *number;             // [n_cells + 1] exclusive prefix of flag: the cluster's number; [n_cells] = n
};

// the records of the clusters c < m, in the working storage (dm_cl_emit copies what the caller asked for)
struct ClustersRec {
    uint32_t m;
    unsigned long long *sum;      // [3 m]
    unsigned long long *key;      // [m] squared distance << 32 | flat index, the minimum over the members
    uint32_t *lo, *hi;            // [3 m]
    uint32_t *first, *size, *rep; // [m]
};

// brick-major cell of voxel (i, j, k) of the region: travel's layout
__device__ __forceinline__ uint32_t cl_cell(const ClustersArgs &a, uint32_t i, uint32_t j, uint32_t k, uint32_t &brick) {
    brick = ((i >> 3) * a.BY + (j >> 3)) * a.BZ + (k >> 3);
    return (brick << 9) | ((i & 7u) << 6) | ((j & 7u) << 3) | (k & 7u);
}

// the final label of voxel f < n_cells
__device__ __forceinline__ uint32_t cl_label_of_flat(const ClustersArgs &a, const uint32_t *__restrict__ side, uint32_t f) {
    const uint32_t k = f % a.nz, row = f / a.nz;
    uint32_t b;
    const uint32_t cell = cl_cell(a, row / a.ny, row % a.ny, k, b);
    return tv_pick(a.lab, side[b] & 1u)[cell];
}

// The next group of a wave: the lowest pending lane names `key`, `mine` = the pending lanes that share it, `leader` = that
// lowest lane, `count` = the lanes of the group.  False when no lane is pending.  Every lane of the wave calls it.
__device__ __forceinline__ bool cl_group(bool pending, uint32_t key, bool &mine, bool &leader, uint32_t &count) {
    const unsigned long long todo = __ballot(pending);
    if (todo == 0ull) return false;
    const int lead = __builtin_ctzll(todo);
    mine = pending && key == (uint32_t)__shfl((int)key, lead);
    count = (uint32_t)__popcll(__ballot(mine));
    leader = (int)(threadIdx.x & 63u) == lead;
    return true;
}

// ---- stage 1: the members ----------------------------------------------------------------------------------------------
// `probe` = 0: the map has no block, every voxel is MISSING and the table is not read.
__global__ __launch_bounds__(256) void dm_cl_enter(RegionArgs r, ClustersArgs a, uint32_t member_mask, uint32_t probe) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;   // n_bricks * 512 <= 2^28: no overflow; the grid covers the cells exactly
    const uint32_t b = c >> 9, bk = b % a.BZ, brow = b / a.BZ;
    const uint32_t i = (brow / a.BY) * 8u + ((c >> 6) & 7u), j = (brow % a.BY) * 8u + ((c >> 3) & 7u), k = bk * 8u + (c & 7u);
    uint32_t v = kClNone;
    if (i < a.nx && j < a.ny && k < a.nz) {
        const uint32_t cls = probe ? pool_class_at(r.pool, r.g0[0] + i, r.g0[1] + j, r.g0[2] + k) : kClsMissing;
        if ((member_mask >> cls) & 1u) v = (i * a.ny + j) * a.nz + k;
    }
    a.lab[0][c] = v;
    if (__ballot(v != kClNone) != 0ull && (threadIdx.x & 63u) == 0u) a.active[0][b] = 1u;   // (a wave lies in one brick)
}

__global__ __launch_bounds__(256) void dm_cl_list(RegionArgs r, ClustersArgs a, uint32_t member_mask, uint32_t probe, const uint32_t *members,
                                                  uint32_t n_members) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_members) return;
    const uint32_t f = members[t];
    if (f >= a.n_cells) return;
    const uint32_t k = f % a.nz, row = f / a.nz, j = row % a.ny, i = row / a.ny;
    const uint32_t cls = probe ? pool_class_at(r.pool, r.g0[0] + i, r.g0[1] + j, r.g0[2] + k) : kClsMissing;
    if (!((member_mask >> cls) & 1u)) return;
    uint32_t b;
    const uint32_t cell = cl_cell(a, i, j, k, b);
    a.lab[0][cell] = f;      // (the same word from every lane that lists the voxel)
    a.active[0][b] = 1u;
}

// ---- stage 2: one round ------------------------------------------------------------------------------------------------
// `turn` = round & 1: side[turn] and active[turn] are this round's inputs, the other two its outputs.
template <int kConn>
__global__ __launch_bounds__(512) void dm_cl_round(ClustersArgs a, uint32_t turn, uint32_t round) {
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
    const uint32_t ti0 = bi / a.tb, tj0 = bj / a.tb, tk0 = bk / a.tb;   // the brick's tile
    // lane order: bits 0-2 lk, 3 lj & 1, 4 li & 1, 5-6 lj >> 1, 7-8 li >> 1 (the LDS banks, devmap_travel.h)
    const uint32_t lk = t & 7u, lj = ((t >> 3) & 1u) | (((t >> 5) & 3u) << 1), li = ((t >> 4) & 1u) | (((t >> 7) & 3u) << 1);
    const uint32_t cell = (b << 9) | (li << 6) | (lj << 3) | lk;
    const int own = (int)((li + 1u) * kTvSX + (lj + 1u) * kTvSY + lk + 1u);
    uint32_t my = tv_pick(a.lab, s)[cell];
    tile[own] = my;
    // the halo: the tile's 1000 cells over the 512 lanes, two trips; interior cells are skipped
    for (uint32_t h = t; h < 1000u; h += 512u) {
        const uint32_t tk = h % 10u, tj = (h / 10u) % 10u, ti = h / 100u;
        const int oi = ti == 0u ? -1 : ti == 9u ? 1 : 0, oj = tj == 0u ? -1 : tj == 9u ? 1 : 0, ok = tk == 0u ? -1 : tk == 9u ? 1 : 0;
        if (oi == 0 && oj == 0 && ok == 0) continue;
        uint32_t v = kClNone;
        const uint32_t qi = bi + (uint32_t)oi, qj = bj + (uint32_t)oj, qk = bk + (uint32_t)ok;   // (bi - 1 wraps above BX)
        if (tv_allowed<kConn>(oi, oj, ok) && qi < a.BX && qj < a.BY && qk < a.BZ && qi / a.tb == ti0 && qj / a.tb == tj0 && qk / a.tb == tk0) {
            const uint32_t q = (qi * a.BY + qj) * a.BZ + qk;
            v = tv_pick(a.lab, side_in[q] & 1u)[(q << 9) | (((ti + 7u) & 7u) << 6) | (((tj + 7u) & 7u) << 3) | ((tk + 7u) & 7u)];
        }
        tile[ti * kTvSX + tj * kTvSY + tk] = v;
    }
    __syncthreads();
    const bool open = my != kClNone;
    bool ever = false;
    int any = 0;
#pragma unroll 1
    for (int it = 0; it < LA3DM_CLUSTERS_INNER; ++it) {
        uint32_t best = my;
        if (open) {
#pragma unroll
            for (int di = -1; di <= 1; ++di)
#pragma unroll
                for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
                    for (int dk = -1; dk <= 1; ++dk) {
                        if (!tv_allowed<kConn>(di, dj, dk)) continue;
                        best = min(best, tile[own + di * kTvSX + dj * kTvSY + dk]);   // (a non-member holds NONE, the largest word)
                    }
        }
        const bool changed = best < my;
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
    const bool capped = any != 0;          // the last of LA3DM_CLUSTERS_INNER iterations still changed a voxel
    if (t < 3u) {
        const uint32_t add = t == 0u ? all_n : t == 1u ? 1u : (capped ? 1u : 0u);
        if (add) atomicAdd(&a.count[round * kClCountWords + t], add);
    }
    if (all_n == 0u) {                     // (uniform) a local fixed point already: nothing is written
        if (t == 0u) side_out[b] = s;
        return;
    }
    tv_pick(a.lab, s ^ 1u)[cell] = my;
    if (t == 0u) side_out[b] = s ^ 1u;
    if (t < 27u) {
        const int di = (int)(t / 9u) - 1, dj = (int)((t / 3u) % 3u) - 1, dk = (int)(t % 3u) - 1;
        const uint32_t qi = bi + (uint32_t)di, qj = bj + (uint32_t)dj, qk = bk + (uint32_t)dk;
        const bool wanted = t == 13u ? capped : ((all_mask >> t) & 1u) != 0u;
        if (wanted && qi < a.BX && qj < a.BY && qk < a.BZ && qi / a.tb == ti0 && qj / a.tb == tj0 && qk / a.tb == tk0)
            atomicOr(&active_out[(qi * a.BY + qj) * a.BZ + qk], 1u);
    }
}

// ---- stage 3: sizes, kept roots, labels --------------------------------------------------------------------------------
// `side`: the array the last queued round wrote (array 0 when no round ran).
__global__ __launch_bounds__(512) void dm_cl_sizes(ClustersArgs a, const uint32_t *__restrict__ side) {
    const uint32_t b = blockIdx.x;
    const uint32_t root = tv_pick(a.lab, side[b] & 1u)[(b << 9) | threadIdx.x];
    bool pending = root != kClNone;
#pragma unroll 1
    for (int g = 0; g < 64; ++g) {   // at most 64 roots in a wave
        bool mine, leader;
        uint32_t count;
        if (!cl_group(pending, root, mine, leader, count)) break;
        if (leader) atomicAdd(&a.size[root], count);
        if (mine) pending = false;
    }
}

// one lane per word of flag: n_cells + 1 of them, the last one 0 (the scan leaves n behind it)
__global__ __launch_bounds__(256) void dm_cl_flags(ClustersArgs a, const uint32_t *__restrict__ side) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    uint32_t sz = 0u;   // the size of the cluster whose root this voxel is
    if (f < a.n_cells && cl_label_of_flat(a, side, f) == f) sz = a.size[f];
    const bool keep = sz >= a.min_size;   // (min_size >= 1: no root, no flag)
    if (f <= a.n_cells) a.flag[f] = keep ? 1u : 0u;
    if (__ballot(sz != 0u) == 0ull) return;   // the wave's totals, one atomic each per wave that holds a root
    uint32_t members = sz, dropped = sz != 0u && !keep ? 1u : 0u, largest = keep ? sz : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        members += __shfl_xor(members, o);
        dropped += __shfl_xor(dropped, o);
        largest = max(largest, __shfl_xor(largest, o));
    }
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(&a.totals[0], members);
        if (dropped) atomicAdd(&a.totals[1], dropped);
        if (largest) atomicMax(&a.totals[2], largest);
    }
}

// the number of the kept cluster whose root is `root`, NONE for NONE or a dropped one
__device__ __forceinline__ uint32_t cl_number(const ClustersArgs &a, uint32_t root) {
    return root != kClNone && a.flag[root] ? a.number[root] : kClNone;
}

__global__ __launch_bounds__(256) void dm_cl_label(ClustersArgs a, const uint32_t *__restrict__ side, uint32_t *label) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f < a.n_cells) label[f] = cl_number(a, cl_label_of_flat(a, side, f));
}

__global__ __launch_bounds__(256) void dm_cl_gather(ClustersArgs a, const uint32_t *__restrict__ side, const uint32_t *members, uint32_t n_members,
                                                    uint32_t *of_member) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_members) return;
    const uint32_t f = members[t];
    of_member[t] = f < a.n_cells ? cl_number(a, cl_label_of_flat(a, side, f)) : kClNone;   // (a listed non-member holds NONE)
}

// ---- stage 4: the records of the clusters c < m ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dm_cl_rec_init(ClustersRec r) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= r.m) return;
    r.key[c] = ~0ull;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        r.sum[3u * c + x] = 0ull;
        r.lo[3u * c + x] = 0xFFFFFFFFu;
        r.hi[3u * c + x] = 0u;
    }
}

// One workgroup per brick, lane t = cell t of the brick: a wave is one li with 8 lj x 8 lk, so i is the wave's own.
__global__ __launch_bounds__(512) void dm_cl_records(ClustersArgs a, const uint32_t *__restrict__ side, ClustersRec r) {
    const uint32_t b = blockIdx.x, t = threadIdx.x, bk = b % a.BZ, brow = b / a.BZ;
    const uint32_t i = (brow / a.BY) * 8u + (t >> 6), j = (brow % a.BY) * 8u + ((t >> 3) & 7u), k = bk * 8u + (t & 7u);
    const uint32_t root = tv_pick(a.lab, side[b] & 1u)[(b << 9) | t];
    const uint32_t c = cl_number(a, root);
    bool pending = c < r.m;   // (NONE is no record)
    if (pending && root == (i * a.ny + j) * a.nz + k) {   // the root's own lane: the only writer of these two
        r.first[c] = root;
        r.size[c] = a.size[root];
    }
#pragma unroll 1
    for (int g = 0; g < 64; ++g) {   // at most 64 clusters in a wave
        bool mine, leader;
        uint32_t count;
        if (!cl_group(pending, c, mine, leader, count)) break;
        uint32_t jlo = mine ? j : 0xFFFFFFFFu, jhi = mine ? j : 0u, jsum = mine ? j : 0u;
        uint32_t klo = mine ? k : 0xFFFFFFFFu, khi = mine ? k : 0u, ksum = mine ? k : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            jlo = min(jlo, __shfl_xor(jlo, o));
            jhi = max(jhi, __shfl_xor(jhi, o));
            jsum += __shfl_xor(jsum, o);      // (64 lanes x 2^15: no overflow)
            klo = min(klo, __shfl_xor(klo, o));
            khi = max(khi, __shfl_xor(khi, o));
            ksum += __shfl_xor(ksum, o);
        }
        if (leader) {
            atomicMin(&r.lo[3u * c], i);
            atomicMin(&r.lo[3u * c + 1u], jlo);
            atomicMin(&r.lo[3u * c + 2u], klo);
            atomicMax(&r.hi[3u * c], i);
            atomicMax(&r.hi[3u * c + 1u], jhi);
            atomicMax(&r.hi[3u * c + 2u], khi);
            atomicAdd(&r.sum[3u * c], (unsigned long long)i * count);
            atomicAdd(&r.sum[3u * c + 1u], (unsigned long long)jsum);
            atomicAdd(&r.sum[3u * c + 2u], (unsigned long long)ksum);
        }
        if (mine) pending = false;
    }
}

// rep: the sums and sizes are final (an earlier launch).  c_a = (2 sum_a + size) / (2 size); the key orders by squared
// distance, then by flat index.
__global__ __launch_bounds__(512) void dm_cl_rep(ClustersArgs a, const uint32_t *__restrict__ side, ClustersRec r) {
    const uint32_t b = blockIdx.x, t = threadIdx.x, bk = b % a.BZ, brow = b / a.BZ;
    const uint32_t i = (brow / a.BY) * 8u + (t >> 6), j = (brow % a.BY) * 8u + ((t >> 3) & 7u), k = bk * 8u + (t & 7u);
    const uint32_t c = cl_number(a, tv_pick(a.lab, side[b] & 1u)[(b << 9) | t]);
    bool pending = c < r.m;
    unsigned long long key = ~0ull;
    if (pending) {
        const unsigned long long sz = r.size[c];
        const uint32_t ci = (uint32_t)((2ull * r.sum[3u * c] + sz) / (2ull * sz)), cj = (uint32_t)((2ull * r.sum[3u * c + 1u] + sz) / (2ull * sz)),
                       ck = (uint32_t)((2ull * r.sum[3u * c + 2u] + sz) / (2ull * sz));
        const uint32_t di = i - ci, dj = j - cj, dk = k - ck;   // (the squares of the wrapped differences are the squares)
        key = ((unsigned long long)(di * di + dj * dj + dk * dk) << 32) | ((i * a.ny + j) * a.nz + k);
    }
#pragma unroll 1
    for (int g = 0; g < 64; ++g) {
        bool mine, leader;
        uint32_t count;
        if (!cl_group(pending, c, mine, leader, count)) break;
        unsigned long long best = mine ? key : ~0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o);
            best = other < best ? other : best;
        }
        if (leader) atomicMin(&r.key[c], best);
        if (mine) pending = false;
    }
}

// one lane per record: rep from its key, and the caller's arrays (any of them may be null)
__global__ __launch_bounds__(256) void dm_cl_emit(ClustersRec r, uint32_t *first, uint32_t *size, uint32_t *lo, uint32_t *hi, unsigned long long *sum,
                                                  uint32_t *rep) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= r.m) return;
    const uint32_t v = (uint32_t)r.key[c];
    r.rep[c] = v;
    if (rep) rep[c] = v;
    if (first) first[c] = r.first[c];
    if (size) size[c] = r.size[c];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        if (lo) lo[3u * c + x] = r.lo[3u * c + x];
        if (hi) hi[3u * c + x] = r.hi[3u * c + x];
        if (sum) sum[3u * c + x] = r.sum[3u * c + x];
    }
}

}  // namespace la3dm_dev

#endif
