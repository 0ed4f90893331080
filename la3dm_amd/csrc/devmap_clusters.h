// devmap_clusters.h — connected groups of a region's member voxels on the device-resident block pool, optionally
// confined to tiles and cut at a minimum size: a dense label and a record per cluster (la3dm_devmap_clusters_*,
// include/la3dm_hip.h; host twin and definition: BGKOctoMap::clusters, host/bgkoctomap.cpp).  Integers throughout and
// a unique answer: the result equals the host form bit for bit.
//
// The scheme is devmap_brick.h's (bricks, two buffers, rounds, the LDS tile, Invariant and Termination); the value is the
// label, and the rule is min.  The label of a member starts as its own flat index f = (i ny + j) nz + k; a non-member
// holds NONE = 0xFFFFFFFF, the identity of min.  The fixed point of "take the smallest label among yourself and your
// adjacent members" gives every member the smallest flat index of its cluster — its `first` — whatever order the
// relaxations run in: labels only fall, and every stored label is the index of a member connected to the voxel.
//
// Cells outside the region are non-members.  A tile is a whole number of bricks (tile % 8 == 0, `tb` bricks per axis),
// so a brick never straddles one: a halo cell of a brick in another tile reads as a non-member, and such a brick is
// never activated from here.
//
// dm_cl_enter    from_list 0.  One lane per cell of the bricks: the pool probe (pool_class_at), the mask; label = own
//                flat index or NONE into buffer 0; a wave that holds a member marks its brick active (a plain store of 1).
// dm_cl_list     from_list 1, after buffer 0 was cleared to NONE.  One lane per list entry: range test, class test, then
//                the voxel's own index is stored — idempotent, so an entry listed twice needs no atomic — and 1 into the
//                brick's active word.
// dm_cl_round    the hot kernel: brick_round with ClustersRule, at most LA3DM_CLUSTERS_INNER iterations per run.  Only
//                the bricks of one tile are joined.
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
// The finish.  Every launch after the rounds reads words that earlier launches completed and accumulates, by atomics
// alone, into words it does not read (dm_cl_sizes: size; dm_cl_flags: totals; dm_cl_records: lo, hi, sum — first and
// size have one writer, the root's lane; dm_cl_rep: key).  No word is read by one workgroup and written by another in
// the same launch.  There is no grid barrier, no cooperative launch and no spin in this file (the scan is the map's own).
//
// Every loop is bounded by a constant: 6 shuffle steps, 64 groups of a wave.  No array is indexed at run time: nothing
// lives in scratch.
#ifndef LA3DM_DEVMAP_CLUSTERS_H
#define LA3DM_DEVMAP_CLUSTERS_H

#include "devmap_brick.h"

namespace la3dm_dev {

static_assert(LA3DM_CLUSTERS_BRICK == 8 && LA3DM_CLUSTERS_NONE == kBrickNone, "devmap_brick.h: bricks of 8 x 8 x 8, NONE the largest word");
constexpr uint32_t kClNone = LA3DM_CLUSTERS_NONE;
constexpr uint32_t kClNoTile = 1u << 20;   // `tb` of an untiled query: more bricks than an axis holds

struct ClustersArgs {
    BrickGrid g;                  // val = the label
    uint32_t tb;                  // bricks per tile and axis (kClNoTile: untiled)
    uint32_t min_size;
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

// the final label of voxel f < n_cells
__device__ __forceinline__ uint32_t cl_label_of_flat(const ClustersArgs &a, const uint32_t *__restrict__ side, uint32_t f) {
    uint32_t b;
    const uint32_t cell = brick_cell_of_flat(a.g, f, b);
    return brick_pick(a.g.val, side[b] & 1u)[cell];
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
    uint32_t i, j, k;
    brick_coords(a.g, c >> 9, c & 511u, i, j, k);
    uint32_t v = kClNone;
    if (i < a.g.nx && j < a.g.ny && k < a.g.nz) {
        const uint32_t cls = probe ? pool_class_at(r.pool, r.g0[0] + i, r.g0[1] + j, r.g0[2] + k) : kClsMissing;
        if ((member_mask >> cls) & 1u) v = (i * a.g.ny + j) * a.g.nz + k;
    }
    a.g.val[0][c] = v;
    if (__ballot(v != kClNone) != 0ull && (threadIdx.x & 63u) == 0u) a.g.active[0][c >> 9] = 1u;   // (a wave lies in one brick)
}

__global__ __launch_bounds__(256) void dm_cl_list(RegionArgs r, ClustersArgs a, uint32_t member_mask, uint32_t probe, const uint32_t *members,
                                                  uint32_t n_members) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_members) return;
    const uint32_t f = members[t];
    if (f >= a.g.n_cells) return;
    const uint32_t k = f % a.g.nz, row = f / a.g.nz, j = row % a.g.ny, i = row / a.g.ny;
    const uint32_t cls = probe ? pool_class_at(r.pool, r.g0[0] + i, r.g0[1] + j, r.g0[2] + k) : kClsMissing;
    if (!((member_mask >> cls) & 1u)) return;
    uint32_t b;
    const uint32_t cell = brick_cell(a.g, i, j, k, b);
    a.g.val[0][cell] = f;      // (the same word from every lane that lists the voxel)
    a.g.active[0][b] = 1u;
}

// ---- stage 2: one round ------------------------------------------------------------------------------------------------
// The rule of brick_round: a member takes the smallest label of its neighbours (a non-member holds NONE, the largest
// word).  Only the bricks of one tile are joined.
struct ClustersRule {
    uint32_t tb;
    uint32_t ti0, tj0, tk0;       // the brick's tile
    __device__ __forceinline__ void brick(uint32_t bi, uint32_t bj, uint32_t bk) {
        ti0 = bi / tb;
        tj0 = bj / tb;
        tk0 = bk / tb;
    }
    __device__ __forceinline__ bool open(uint32_t, uint32_t my) const { return my != kClNone; }
    __device__ __forceinline__ bool joined(uint32_t qi, uint32_t qj, uint32_t qk) const { return qi / tb == ti0 && qj / tb == tj0 && qk / tb == tk0; }
    __device__ __forceinline__ uint32_t relax(uint32_t best, uint32_t u, int) const { return min(best, u); }
    __device__ __forceinline__ bool keep(uint32_t) const { return true; }
};

template <int kConn>
__global__ __launch_bounds__(512) void dm_cl_round(ClustersArgs a, uint32_t turn, uint32_t round) {
    brick_round<kConn, LA3DM_CLUSTERS_INNER>(a.g, turn, round, ClustersRule{a.tb, 0u, 0u, 0u});
}

// ---- stage 3: sizes, kept roots, labels --------------------------------------------------------------------------------
// `side`: the array the last queued round wrote (array 0 when no round ran).
__global__ __launch_bounds__(512) void dm_cl_sizes(ClustersArgs a, const uint32_t *__restrict__ side) {
    const uint32_t b = blockIdx.x;
    const uint32_t root = brick_pick(a.g.val, side[b] & 1u)[(b << 9) | threadIdx.x];
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
    if (f < a.g.n_cells && cl_label_of_flat(a, side, f) == f) sz = a.size[f];
    const bool keep = sz >= a.min_size;   // (min_size >= 1: no root, no flag)
    if (f <= a.g.n_cells) a.flag[f] = keep ? 1u : 0u;
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
    if (f < a.g.n_cells) label[f] = cl_number(a, cl_label_of_flat(a, side, f));
}

__global__ __launch_bounds__(256) void dm_cl_gather(ClustersArgs a, const uint32_t *__restrict__ side, const uint32_t *members, uint32_t n_members,
                                                    uint32_t *of_member) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_members) return;
    const uint32_t f = members[t];
    of_member[t] = f < a.g.n_cells ? cl_number(a, cl_label_of_flat(a, side, f)) : kClNone;   // (a listed non-member holds NONE)
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
    const uint32_t b = blockIdx.x, t = threadIdx.x, cell = (b << 9) | t;
    uint32_t i, j, k;
    brick_coords(a.g, b, t, i, j, k);
    const uint32_t root = brick_pick(a.g.val, side[b] & 1u)[cell];
    const uint32_t c = cl_number(a, root);
    bool pending = c < r.m;   // (NONE is no record)
    if (pending && root == (i * a.g.ny + j) * a.g.nz + k) {   // the root's own lane: the only writer of these two
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
    const uint32_t b = blockIdx.x, t = threadIdx.x, cell = (b << 9) | t;
    uint32_t i, j, k;
    brick_coords(a.g, b, t, i, j, k);
    const uint32_t c = cl_number(a, brick_pick(a.g.val, side[b] & 1u)[cell]);
    bool pending = c < r.m;
    unsigned long long key = ~0ull;
    if (pending) {
        const unsigned long long sz = r.size[c];
        const uint32_t ci = (uint32_t)((2ull * r.sum[3u * c] + sz) / (2ull * sz)), cj = (uint32_t)((2ull * r.sum[3u * c + 1u] + sz) / (2ull * sz)),
                       ck = (uint32_t)((2ull * r.sum[3u * c + 2u] + sz) / (2ull * sz));
        const uint32_t di = i - ci, dj = j - cj, dk = k - ck;   // (the squares of the wrapped differences are the squares)
        key = ((unsigned long long)(di * di + dj * dj + dk * dk) << 32) | ((i * a.g.ny + j) * a.g.nz + k);
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
