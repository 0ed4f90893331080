// devmap_region.h — dense region reads on the device-resident block pool (la3dm_devmap_box_* / la3dm_devmap_columns_*,
// include/la3dm_hip.h; host twin and definition: BGKOctoMap::box / columns, host/bgkoctomap.cpp).
//
// The host resolves the anchor (the only floating-point work of the query) and hands the kernels the global voxel index
// g0 of voxel (0, 0, 0); everything below is integer arithmetic on g = g0 + (i, j, k): block field g >> dl, cell
// g & (lim - 1), dl = block_depth - 1.  A block field is below 2^20 and lim at most 2^5, so g fits 32 bits.
//
// dm_box<V>   output order: a thread owns V consecutive voxels of the flat (i, j, k) index (k fastest), so a wave writes
//             64 V consecutive bytes of cls / leaf_depth and 256 V of A and of B.  The block table is probed when the
//             block key changes along the thread's run; the lanes of a wave that sit in the same block ask for the
//             same table entry (one cache line, the requests of a wave merge in the L1).  A missing block reads nothing
//             but the table.  V = 4 stores words / float4 and needs outputs aligned to 4 / 16 bytes; V = 1 has no such
//             need and is what an unaligned device pointer gets.
// dm_columns  one lane per column (i, j), lanes along j; the lane walks k block by block: one probe per block of the
//             column, then the lim state bytes of its z run (finest-layer indices cell_xy + {0, 1, 8, 9, 64, 65, ...}: a
//             span of 10 B at depth 3, 74 B at depth 4 — one 128-byte line, two where the block's slab straddles one)
//             plus one byte per PRUNED level climbed.  Nothing is written but the column's own counts and bounds.
//
// Every loop is bounded by an argument or by the table size / depth: V, dims, lim, the probe count, the climb.
#ifndef LA3DM_DEVMAP_REGION_H
#define LA3DM_DEVMAP_REGION_H

#include "devmap_pool.h"

namespace la3dm_dev {

struct RegionArgs {
    uint32_t g0[3];      // global voxel index of voxel (0, 0, 0)
    uint32_t nx, ny, nz;
    uint32_t total;      // box: nx ny nz; columns: nx ny
    PoolView pool;
    // box outputs (all but cls may be null)
    uint8_t *cls, *leaf_depth;
    float *oA, *oB;
    // columns outputs (all but counts may be null)
    uint32_t *counts;
    int32_t *low_occ, *top_occ;
    uint32_t counts_vec;   // counts is 16-byte aligned: one uint4 store per column
};

constexpr uint32_t kRegionFree = 0u, kRegionOccupied = 1u;   // State::FREE, State::OCCUPIED

template <int V>
__global__ __launch_bounds__(256) void dm_box(RegionArgs a) {
    const uint32_t first = (blockIdx.x * 256u + threadIdx.x) * (uint32_t)V;   // total <= 2^30: no overflow
    if (first >= a.total) return;
    const uint32_t dl = a.pool.depth - 1u, cm = (1u << dl) - 1u;
    uint32_t k = first % a.nz;
    const uint32_t row = first / a.nz;
    uint32_t j = row % a.ny, i = row / a.ny;
    uint32_t cls[V], dep[V];
    float vA[V], vB[V];
    long long last_key = -2;   // (no key: keys are >= 0, the table's empty mark is -1)
    uint32_t slot = kNoSlot;
#pragma unroll
    for (int v = 0; v < V; ++v) {   // V is a template argument: the four arrays are registers
        cls[v] = kClsMissing;
        dep[v] = 255u;
        vA[v] = a.pool.a0;
        vB[v] = a.pool.b0;
        if (first + (uint32_t)v < a.total) {
            const uint32_t gx = a.g0[0] + i, gy = a.g0[1] + j, gz = a.g0[2] + k;
            const long long key = pool_block_key(gx, gy, gz, dl);
            if (key != last_key) {
                slot = pool_find_block(a.pool, key);
                last_key = key;
            }
            if (slot != kNoSlot) {
                const uint32_t cell = pool_cell_index((int)(gx & cm), (int)(gy & cm), (int)(gz & cm), (int)dl);
                uint32_t d, n;
                covering_leaf(a.pool.S + (size_t)slot * a.pool.npb, dl, cell, d, n);
                const size_t node = (size_t)slot * a.pool.npb + dm_layer_base(d) + n;
                cls[v] = a.pool.S[node] & 7u;
                dep[v] = d;
                if (a.oA) vA[v] = a.pool.A[node];
                if (a.oB) vB[v] = a.pool.B[node];
            }
            if (++k == a.nz) {
                k = 0;
                if (++j == a.ny) {
                    j = 0;
                    ++i;
                }
            }
        }
    }
    if (V == 4 && first + 4u <= a.total) {   // (the host chose V = 4 only for aligned outputs; first is a multiple of 4)
        *(uint32_t *)(a.cls + first) = cls[0] | (cls[V > 1 ? 1 : 0] << 8) | (cls[V > 2 ? 2 : 0] << 16) | (cls[V > 3 ? 3 : 0] << 24);
        if (a.leaf_depth)
            *(uint32_t *)(a.leaf_depth + first) = dep[0] | (dep[V > 1 ? 1 : 0] << 8) | (dep[V > 2 ? 2 : 0] << 16) | (dep[V > 3 ? 3 : 0] << 24);
        if (a.oA) *(float4 *)(a.oA + first) = make_float4(vA[0], vA[V > 1 ? 1 : 0], vA[V > 2 ? 2 : 0], vA[V > 3 ? 3 : 0]);
        if (a.oB) *(float4 *)(a.oB + first) = make_float4(vB[0], vB[V > 1 ? 1 : 0], vB[V > 2 ? 2 : 0], vB[V > 3 ? 3 : 0]);
        return;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const uint32_t o = first + (uint32_t)v;
        if (o < a.total) {
            a.cls[o] = (uint8_t)cls[v];
            if (a.leaf_depth) a.leaf_depth[o] = (uint8_t)dep[v];
            if (a.oA) a.oA[o] = vA[v];
            if (a.oB) a.oB[o] = vB[v];
        }
    }
}

__global__ __launch_bounds__(256) void dm_columns(RegionArgs a) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= a.total) return;
    const uint32_t dl = a.pool.depth - 1u, lim = 1u << dl, cm = lim - 1u;
    const uint32_t j = c % a.ny, i = c / a.ny;
    const uint32_t gx = a.g0[0] + i, gy = a.g0[1] + j;
    const uint32_t cell_xy = pool_cell_index((int)(gx & cm), (int)(gy & cm), 0, (int)dl);
    uint32_t n_free = 0, n_occ = 0, n_unk = 0;
    int32_t low = -1, top = -1;
    uint32_t k = 0;
    while (k < a.nz) {   // one trip per block of the column: at most nz / lim + 2
        const uint32_t gz = a.g0[2] + k, cz0 = gz & cm;
        const uint32_t run = min(lim - cz0, a.nz - k);
        const uint32_t slot = pool_find_block(a.pool, pool_block_key(gx, gy, gz, dl));
        if (slot != kNoSlot) {   // (a missing block is counted by what is left of nz at the end)
            const uint8_t *Sb = a.pool.S + (size_t)slot * a.pool.npb;
            for (uint32_t u = 0; u < run; ++u) {
                uint32_t d, n;
                const uint32_t st = pool_leaf_class(Sb, dl, cell_xy | pool_cell_index(0, 0, (int)(cz0 + u), (int)dl), d, n);
                n_free += st == kRegionFree ? 1u : 0u;
                n_occ += st == kRegionOccupied ? 1u : 0u;
                n_unk += (st != kRegionFree && st != kRegionOccupied) ? 1u : 0u;   // UNKNOWN, and a BGK-LV map's UNCERTAIN
                if (st == kRegionOccupied) {
                    low = low < 0 ? (int32_t)(k + u) : low;
                    top = (int32_t)(k + u);
                }
            }
        }
        k += run;
    }
    const uint32_t n_miss = a.nz - n_free - n_occ - n_unk;
    if (a.counts_vec) {
        *(uint4 *)(a.counts + 4 * (size_t)c) = make_uint4(n_free, n_occ, n_unk, n_miss);
    } else {
        uint32_t *o = a.counts + 4 * (size_t)c;
        o[0] = n_free;
        o[1] = n_occ;
        o[2] = n_unk;
        o[3] = n_miss;
    }
    if (a.low_occ) a.low_occ[c] = low;
    if (a.top_occ) a.top_occ[c] = top;
}

}  // namespace la3dm_dev

#endif
