// devmap_gain.h — information gain of candidate viewpoints on the device-resident block pool: per viewpoint the number of
// DISTINCT voxels of a map region that a fan of rays from it walks over and whose class is in the count mask
// (la3dm_devmap_gain_*, include/la3dm_hip.h; host twin and definition: BGKOctoMap::gain, host/bgkoctomap.cpp).  The only
// floating-point operation the query adds to raycast_many's is the fp32 add origin + offset per coordinate; everything
// after the walk is integers: the result equals the host form bit for bit.
//
// (memset)       the sets — n x W words, W = ceil(nx ny nz / 32) — and the per-viewpoint counters are zeroed on the map's
//                stream before the launches.
// dm_gain_mark   one ray per lane, one viewpoint per workgroup (grid = n x ceil(m / 256), flattened): the lanes of a
//                workgroup share the start block, so their early rows hit the same table entries, state bytes and set
//                words.  The walk is dm_raycast's (devmap_raycast.h), restated; the loop keeps only the class of a row.
//                Each row turns (block key, cell) into the region index with integer subtracts and an unsigned compare,
//                reads the word of its bit and issues a no-return atomic OR only when the bit is still clear — a stale
//                read (the L1 is not coherent with the atomics) only costs a redundant atomic.  started / hits: a wave
//                ballot, one atomic add per wave.
// dm_gain_count  one lane per word of a set (grid = n x ceil(W / 256), flattened): popcount, wave reduction, one atomic
//                add per wave into gain[v].
//
// Every loop is bounded by an argument: the walk by max_steps, the probe by the table size, the climb by the depth.  No
// workgroup waits for another.
#ifndef LA3DM_DEVMAP_GAIN_H
#define LA3DM_DEVMAP_GAIN_H

#include "devmap_raycast.h"

namespace la3dm_dev {

struct GainArgs {
    const float *origins;   // 3 per viewpoint
    const float *offsets;   // 3 per direction, shared by the viewpoints
    uint32_t n, m;          // viewpoints, directions
    uint32_t chunks;        // ceil(m / 256): workgroups per viewpoint
    uint32_t count_mask, stop_mask, max_steps;
    float block_size, resolution;
    PoolView pool;
    uint32_t g0[3];         // global voxel index of the region's voxel (0, 0, 0)
    uint32_t nx, ny, nz;
    uint32_t W;             // words per set
    uint32_t *seen;         // [n W], zero before the launch
    uint32_t *started;      // [n] or null, zero before the launch
    uint32_t *hits;         // [n] or null, zero before the launch
};

// element `k` (runtime) of a 3-array that lives in registers: selects, never a runtime-indexed array (scratch)
#define GAIN_SEL3(v, k) ((k) == 0 ? (v)[0] : ((k) == 1 ? (v)[1] : (v)[2]))
#define GAIN_PUT3(v, k, x)                 \
    do {                                   \
        const auto x_ = (x);               \
        (v)[0] = (k) == 0 ? x_ : (v)[0];   \
        (v)[1] = (k) == 1 ? x_ : (v)[1];   \
        (v)[2] = (k) == 2 ? x_ : (v)[2];   \
    } while (0)

// The walk below is the twin of dm_raycast's (devmap_raycast.h): the same validity test, the same start block, the same
// DDA with the reference's case order, diagonal double step and repeat, the same re-hash of the walk's own block centre
// at a face and the same stop and truncation.  A change to one must be made to the other; tests/test_gain_gpu.py holds
// the two together through the host form, whose gain loops the very RayCaster raycast_many loops.
__global__ __launch_bounds__(256) void dm_gain_mark(GainArgs a) {
    const uint32_t v = blockIdx.x / a.chunks;                                   // the workgroup's viewpoint
    const uint32_t dir = (blockIdx.x - v * a.chunks) * 256u + threadIdx.x;      // the lane's direction
    const bool live = dir < a.m;
    const float res = a.resolution, bs = a.block_size;
    float q[6];
    bool ok = live;   // refused before any (int) conversion
    if (live) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            q[k] = a.origins[3 * (size_t)v + k];
            q[3 + k] = q[k] + a.offsets[3 * (size_t)dir + k];   // the query's one floating-point operation of its own
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) ok &= fabsf(q[k] / res) < 1073741824.0f;   // false for NaN and inf
    }
    const int dl = (int)a.pool.depth - 1, lim = 1 << dl;
    uint32_t steps = 0;
    bool hit = false;
    long long key = 0;
    uint32_t slot = kNoSlot;
    if (ok) {
        const long long i0 = axis_index(q[0], bs), i1 = axis_index(q[1], bs), i2 = axis_index(q[2], bs);
        key = (i0 << 40) | (i1 << 20) | i2;
        slot = pool_find_block(a.pool, key);
    }
    if (slot != kNoSlot) {
        uint32_t *const set = a.seen + (size_t)v * a.W;
        const float pc[3] = {axis_center(key >> 40, bs), axis_center((key >> 20) & 0xFFFFF, bs), axis_center(key & 0xFFFFF, bs)};
        float wc[3] = {pc[0], pc[1], pc[2]};   // the walk's own block centre: += block size per face crossed, then re-hashed
        int bi[3] = {0, 0, 0};
        int dd[3], d2[3];
        uint32_t idx = 0;             // voxel index inside the block, 8 bits per axis (x lowest)
        uint32_t inc = 0;             // step sign + 1, 2 bits per axis
        int n = 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            bi[k] = (int)axis_index(wc[k], bs);
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
            // ---- the row: its class
            uint32_t cls = kClsMissing;
            if (slot != kNoSlot) {
                const uint32_t cell = pool_cell_index(idx & 0xFF, (idx >> 8) & 0xFF, (idx >> 16) & 0xFF, dl);
                uint32_t d, i;
                cls = pool_leaf_class(a.pool.S + (size_t)slot * a.pool.npb, (uint32_t)dl, cell, d, i);
            }
            ++steps;
            // ---- mark: lattice position = block-key fields * lim + cell, minus the region's g0 (wrapping: a position
            // below g0 becomes a huge index and fails the compare)
            if ((a.count_mask >> cls) & 1u) {
                const uint32_t i = ((uint32_t)(key >> 40) & 0xFFFFFu) * (uint32_t)lim + (idx & 0xFFu) - a.g0[0];
                const uint32_t j = ((uint32_t)(key >> 20) & 0xFFFFFu) * (uint32_t)lim + ((idx >> 8) & 0xFFu) - a.g0[1];
                const uint32_t k = ((uint32_t)key & 0xFFFFFu) * (uint32_t)lim + ((idx >> 16) & 0xFFu) - a.g0[2];
                if (i < a.nx && j < a.ny && k < a.nz) {
                    const uint32_t f = (i * a.ny + j) * a.nz + k, bit = 1u << (f & 31u);
                    uint32_t *const w = set + (f >> 5);
                    // (result unused: the no-return form.  The unconditional atomic was measured 14 % slower: DESIGN.md 3.11)
                    if (!(*w & bit)) __hip_atomic_fetch_or(w, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if (a.stop_mask & (1u << cls)) {
                hit = true;
                break;
            }
            // ---- advance: same case order as the reference; no case = the voxel repeats
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
            if (n <= 0) break;
            if (steps == a.max_steps) break;   // truncated
#pragma unroll 1
            for (int pass = 0; pass < 2; ++pass) {   // RayCaster's step(axis), once or (diagonal) twice
                const int ax = pass == 0 ? ax0 : ax1;
                if (ax < 0) continue;
                const int ic = (int)((inc >> (2 * ax)) & 3u) - 1;
                const int ni = (int)((idx >> (8 * ax)) & 0xFFu) + ic;
                const bool leaves = ni >= lim || ni < 0;
                idx = (idx & ~(0xFFu << (8 * ax))) | ((uint32_t)(leaves ? (ic > 0 ? 0 : lim - 1) : ni) << (8 * ax));
                if (leaves) {   // enter_block: through the face of this axis
                    const float w = GAIN_SEL3(wc, ax) + (float)ic * bs;
                    GAIN_PUT3(wc, ax, w);
                    GAIN_PUT3(bi, ax, (int)axis_index(w, bs));
                    key = ((long long)bi[0] << 40) | ((long long)bi[1] << 20) | (long long)bi[2];
                    slot = pool_find_block(a.pool, key);
                }
            }
        }
    }
    // ---- rays per viewpoint: every lane of the wave is here (none returned early), one atomic add per wave
    if (a.started) {
        const unsigned long long vote = __ballot(steps > 0);
        if ((threadIdx.x & 63u) == 0u && vote) atomicAdd(a.started + v, (uint32_t)__popcll(vote));
    }
    if (a.hits) {
        const unsigned long long vote = __ballot(hit);
        if ((threadIdx.x & 63u) == 0u && vote) atomicAdd(a.hits + v, (uint32_t)__popcll(vote));
    }
}
#undef GAIN_SEL3
#undef GAIN_PUT3

// gain[v] += popcount of the words of set v; chunks = ceil(W / 256) workgroups per viewpoint; gain is zero before
__global__ __launch_bounds__(256) void dm_gain_count(const uint32_t *__restrict__ seen, uint32_t W, uint32_t chunks, uint32_t *gain) {
    const uint32_t v = blockIdx.x / chunks;
    const uint32_t w = (blockIdx.x - v * chunks) * 256u + threadIdx.x;
    uint32_t c = w < W ? (uint32_t)__popc(seen[(size_t)v * W + w]) : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63u) == 0u && c) atomicAdd(gain + v, c);
}

}  // namespace la3dm_dev

#endif
