// devmap_raycast.h — batched ray casting on the device-resident block pool (la3dm_devmap_raycast_*, include/la3dm_hip.h).
//
// One ray per lane drives the reference's voxel walk (BGKOctoMap::RayCaster, include/bgkoctomap/bgkoctomap.h:91-214; host
// twin: host/bgkoctomap.cpp RayCaster + BGKOctoMap::raycast_many, which is the definition this kernel reproduces bit for
// bit): an integer DDA over the voxel indices of the two end points, the reference's case order, its diagonal double
// step and its "no case applies" repeat, the fp32 block-centre re-hash when a face is crossed and dead reckoning inside
// missing blocks.  What a row IS comes from the covering leaf of its voxel (pool_leaf_class, devmap_pool.h).
//
// Memory traffic per step: one state byte (plus one per PRUNED level climbed); the block-table probe (8 B key and 4 B
// slot per entry tried) only when a block face is crossed; the LUT entry (16 B) of the voxel; A / B once, for the last row.
// Every loop is bounded by an argument: the walk by max_steps, the probe by the table size, the climb by the depth.
#ifndef LA3DM_DEVMAP_RAYCAST_H
#define LA3DM_DEVMAP_RAYCAST_H

#include "devmap_pool.h"

namespace la3dm_dev {

struct RaycastArgs {
    const float *rays;   // 6 per ray: start xyz, end xyz
    uint32_t n, stop_mask, max_steps;
    const float4 *lut;   // voxel offsets, depth-major (the context's LUT)
    float block_size, resolution;
    PoolView pool;
    // outputs (all but steps / flags may be null)
    uint32_t *steps;
    uint8_t *flags;
    float *p;
    long long *block_key;
    int32_t *node_key;
    uint8_t *cls, *leaf_depth;
    float *oA, *oB;
    uint32_t *counts;
};

constexpr uint32_t kRayHit = 1u, kRayTruncated = 2u, kRayInvalid = 4u;
static_assert(LA3DM_RAY_MAX_STEPS <= (1u << 20), "dm_raycast packs its per-class row counts in 21-bit fields");

// element `k` (runtime) of a 3-array that lives in registers: selects, never a runtime-indexed array (scratch)
#define RAY_SEL3(v, k) ((k) == 0 ? (v)[0] : ((k) == 1 ? (v)[1] : (v)[2]))
#define RAY_PUT3(v, k, x)                  \
    do {                                   \
        const auto x_ = (x);               \
        (v)[0] = (k) == 0 ? x_ : (v)[0];   \
        (v)[1] = (k) == 1 ? x_ : (v)[1];   \
        (v)[2] = (k) == 2 ? x_ : (v)[2];   \
    } while (0)

__global__ __launch_bounds__(256, 8) void dm_raycast(RaycastArgs a) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    const float res = a.resolution, bs = a.block_size;
    float q[6];
    bool ok = true;   // refused before any (int) conversion
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        q[k] = a.rays[6 * (size_t)r + k];
        ok &= fabsf(q[k] / res) < 1073741824.0f;   // false for NaN and inf
    }
    const int dl = (int)a.pool.depth - 1, lim = 1 << dl;
    const uint32_t fine_base = dm_layer_base((uint32_t)dl);
    uint32_t steps = 0, flags = ok ? 0u : kRayInvalid;
    unsigned long long cnt = 0;   // rows of class 0, 1, 2 in 21-bit fields (a ray has at most 2^20 rows); class 3 = the rest
    // block of the start point
    int bi[3] = {0, 0, 0};
    long long key = 0;
    uint32_t slot = kNoSlot;
    if (ok) {
        const long long i0 = axis_index(q[0], bs), i1 = axis_index(q[1], bs), i2 = axis_index(q[2], bs);
        key = (i0 << 40) | (i1 << 20) | i2;
        slot = pool_find_block(a.pool, key);
    }
    float cur[3] = {0.f, 0.f, 0.f};   // current_p
    uint32_t idx = 0;                 // voxel index inside the block, 8 bits per axis (x lowest)
    if (slot != kNoSlot) {
        // centre of the block as the host block holds it (hash_key_to_block of its key); recomputed from the key where
        // a row needs it, which is cheaper than three registers carried round the loop
        const float pc[3] = {axis_center(key >> 40, bs), axis_center((key >> 20) & 0xFFFFF, bs), axis_center(key & 0xFFFFF, bs)};
        float wc[3] = {pc[0], pc[1], pc[2]};   // the walk's own block centre: += block size per face crossed, then re-hashed
        int dd[3], d2[3];
        uint32_t inc = 0;             // step sign + 1, 2 bits per axis
        int n = 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            // every axis of the key comes from the walk's centre from here on (block_to_hash_key(block_center) in enter_block;
            // a biased index is below 2^31 for every coordinate the validity test lets through)
            bi[k] = (int)axis_index(wc[k], bs);
            cur[k] = q[k];
            const int t = (int)((q[k] - pc[k]) / res + (float)(lim / 2));   // Block::get_index: truncation, clamped
            idx |= (uint32_t)max(0, min(t, lim - 1)) << (8 * k);
            const int v0 = (int)(q[k] / res), v1 = (int)(q[3 + k] / res);
            const int d = abs(v1 - v0);
            inc |= (v1 > v0 ? 2u : (v1 == v0 ? 1u : 0u)) << (2 * k);
            n += d;
            dd[k] = d;
            d2[k] = 2 * d;
        }
        int err_xy = dd[0] - dd[1], err_xz = dd[0] - dd[2], err_yz = dd[1] - dd[2];
        for (;;) {   // n > 0 here; every trip is one row, and a.max_steps rows end the loop whatever the map holds
            // ---- the row (RayCaster::next up to `p = current_p`): its class is all the loop needs
            uint32_t cls = kClsMissing;
            if (slot != kNoSlot) {
                const uint32_t cell = pool_cell_index(idx & 0xFF, (idx >> 8) & 0xFF, (idx >> 16) & 0xFF, dl);
                const float4 o = a.lut[fine_base + cell];
                cur[0] = o.x + axis_center(key >> 40, bs);
                cur[1] = o.y + axis_center((key >> 20) & 0xFFFFF, bs);
                cur[2] = o.z + axis_center(key & 0xFFFFF, bs);
                uint32_t d, i;
                cls = pool_leaf_class(a.pool.S + (size_t)slot * a.pool.npb, (uint32_t)dl, cell, d, i);
            }
            ++steps;
            const uint32_t field = cls > 3u ? 2u : cls;   // (a BGK-LV map's UNCERTAIN leaves count with UNKNOWN)
            cnt += field < 3u ? 1ull << (21u * field) : 0ull;
            if (a.stop_mask & (1u << cls)) {
                flags |= kRayHit;
                break;
            }
            // ---- advance (the rest of next()): same case order as the reference; no case = the voxel repeats
            int ax0 = -1, ax1 = -1;
            if (err_xy > 0 && err_xz > 0) {
                ax0 = 0;
                err_xy -= d2[1];
                err_xz -= d2[2];
            } else if (err_xy < 0 && err_yz > 0) {
                ax0 = 1;
                err_xy += d2[0];
                err_yz -= d2[2];
            } else if (err_yz < 0 && err_xz < 0) {
                ax0 = 2;
                err_xz += d2[0];
                err_yz += d2[1];
            } else if (err_xy == 0) {   // diagonal move in the xy plane: two voxel steps at once
                ax0 = 0;
                ax1 = 1;
                n -= 2;
            }
            --n;
            // The row just made is the last one if the walk is over or the budget is spent: the position is then left
            // where that row put it (the host's next() moves on, but nothing reads what it moved to).
            if (n <= 0) break;
            if (steps == a.max_steps) {
                flags |= kRayTruncated;
                break;
            }
#pragma unroll 1
            for (int pass = 0; pass < 2; ++pass) {   // RayCaster's step(axis), once or (diagonal) twice
                const int ax = pass == 0 ? ax0 : ax1;
                if (ax < 0) continue;
                const int ic = (int)((inc >> (2 * ax)) & 3u) - 1;
                const int ni = (int)((idx >> (8 * ax)) & 0xFFu) + ic;
                const bool leaves = ni >= lim || ni < 0;
                idx = (idx & ~(0xFFu << (8 * ax))) | ((uint32_t)(leaves ? (ic > 0 ? 0 : lim - 1) : ni) << (8 * ax));
                RAY_PUT3(cur, ax, RAY_SEL3(cur, ax) + (float)ic * res);
                if (leaves) {   // enter_block: through the face of this axis
                    const float w = RAY_SEL3(wc, ax) + (float)ic * bs;
                    RAY_PUT3(wc, ax, w);
                    RAY_PUT3(bi, ax, (int)axis_index(w, bs));
                    key = ((long long)bi[0] << 40) | ((long long)bi[1] << 20) | (long long)bi[2];
                    slot = pool_find_block(a.pool, key);
                }
            }
        }
    }
    // ---- the last row again, in full: key, covering leaf and its node (the loop kept only the position and the counts)
    uint32_t cls = kClsMissing, leaf_d = 255u, node_key = 0;
    float A = a.pool.a0, B = a.pool.b0;
    if (steps == 0) {
        key = 0;   // never started (or refused)
    } else {
        const uint32_t cell = pool_cell_index(idx & 0xFF, (idx >> 8) & 0xFF, (idx >> 16) & 0xFF, dl);
        node_key = ((uint32_t)dl << 16) + cell;
        if (slot != kNoSlot) {
            uint32_t d, i;
            covering_leaf(a.pool.S + (size_t)slot * a.pool.npb, (uint32_t)dl, cell, d, i);
            const size_t node = (size_t)slot * a.pool.npb + dm_layer_base(d) + i;
            cls = a.pool.S[node] & 7u;
            leaf_d = d;
            if (a.oA) A = a.pool.A[node];
            if (a.oB) B = a.pool.B[node];
        }
    }
    a.steps[r] = steps;
    a.flags[r] = (uint8_t)flags;
    if (a.p) {
        a.p[3 * (size_t)r] = cur[0];
        a.p[3 * (size_t)r + 1] = cur[1];
        a.p[3 * (size_t)r + 2] = cur[2];
    }
    if (a.block_key) a.block_key[r] = key;
    if (a.node_key) a.node_key[r] = (int32_t)node_key;
    if (a.cls) a.cls[r] = (uint8_t)cls;
    if (a.leaf_depth) a.leaf_depth[r] = (uint8_t)leaf_d;
    if (a.oA) a.oA[r] = A;
    if (a.oB) a.oB[r] = B;
    if (a.counts) {
        const uint32_t c0 = (uint32_t)cnt & 0x1FFFFFu, c1 = (uint32_t)(cnt >> 21) & 0x1FFFFFu, c2 = (uint32_t)(cnt >> 42) & 0x1FFFFFu;
        uint32_t *c = a.counts + 4 * (size_t)r;
        c[0] = c0;
        c[1] = c1;
        c[2] = c2;
        c[3] = steps - c0 - c1 - c2;
    }
}
#undef RAY_SEL3
#undef RAY_PUT3

}  // namespace la3dm_dev

#endif
