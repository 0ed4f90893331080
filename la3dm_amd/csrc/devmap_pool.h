// devmap_pool.h — how a query kernel reads the device-resident block pool: the pool's fields as one kernel argument and
// the one way from a global voxel index to the class of its covering leaf (block key, table probe, cell index, climb).
// Used by dm_raycast, dm_box, dm_columns, dm_df_bits and dm_fr_bits; host twin: covering_leaf_at, host/bgkoctomap.cpp.
#ifndef LA3DM_DEVMAP_POOL_H
#define LA3DM_DEVMAP_POOL_H

#include "../../include/la3dm_hip.h"
#include "devmap_kernels.h"

namespace la3dm_dev {

struct PoolView {
    const long long *tab_key;
    const uint32_t *tab_val;
    uint32_t mask;       // table size - 1
    const float *A, *B;
    const uint8_t *S;
    uint32_t npb, depth;
    float a0, b0;        // A, B of a voxel whose block is missing
};

constexpr uint32_t kNoSlot = 0xFFFFFFFFu, kClsMissing = LA3DM_RAY_MISSING;

// pool slot of a block key, kNoSlot when the map has no such block; at most one trip round the table
__device__ __forceinline__ uint32_t pool_find_block(const PoolView &p, long long key) {
    uint32_t h = hash_key64(key, p.mask);
    for (uint32_t probe = 0; probe <= p.mask; ++probe) {
        const long long cur = p.tab_key[h];
        const uint32_t val = p.tab_val[h];   // asked for together with the key: one round trip per probe, not two
        if (cur == key) return val;
        if (cur == kEmptyKey) break;
        h = (h + 1) & p.mask;
    }
    return kNoSlot;
}

// key of the block that holds global voxel (gx, gy, gz); dl = block_depth - 1
__device__ __forceinline__ long long pool_block_key(uint32_t gx, uint32_t gy, uint32_t gz, uint32_t dl) {
    return ((long long)(gx >> dl) << 40) | ((long long)(gy >> dl) << 20) | (long long)(gz >> dl);
}

// Block::get_node: finest-layer index of cell (x, y, z); child bit 4 = +x, 2 = +y, 1 = +z per level
__device__ __forceinline__ uint32_t pool_cell_index(int x, int y, int z, int levels) {
    uint32_t index = 0;
    for (int level = levels - 1; level >= 0; --level)
        index = index * 8u + (uint32_t)((((x >> level) & 1) << 2) | (((y >> level) & 1) << 1) | ((z >> level) & 1));
    return index;
}

// covering_leaf with the state kept: class of the leaf that covers finest-layer cell c of the block whose states are Sb,
// its layer d and index n; one byte read per PRUNED level climbed
__device__ __forceinline__ uint32_t pool_leaf_class(const uint8_t *__restrict__ Sb, uint32_t dl, uint32_t c, uint32_t &d, uint32_t &n) {
    d = dl;
    n = c;
    uint32_t st = Sb[dm_layer_base(d) + n] & 7u;
    while (d > 0 && st == kStatePruned) {
        --d;
        n >>= 3;
        st = Sb[dm_layer_base(d) + n] & 7u;
    }
    return st;
}

// class at global voxel (gx, gy, gz): that of its covering leaf, kClsMissing where the map has no block there
__device__ __forceinline__ uint32_t pool_class_at(const PoolView &p, uint32_t gx, uint32_t gy, uint32_t gz) {
    const uint32_t dl = p.depth - 1u, cm = (1u << dl) - 1u;
    const uint32_t slot = pool_find_block(p, pool_block_key(gx, gy, gz, dl));
    if (slot == kNoSlot) return kClsMissing;
    uint32_t d, n;
    return pool_leaf_class(p.S + (size_t)slot * p.npb, dl, pool_cell_index((int)(gx & cm), (int)(gy & cm), (int)(gz & cm), (int)dl), d, n);
}

// Bit f of the stream `bits` = `set`, for the 64 consecutive f of a wave (f of lane 0 a multiple of 64): the wave's ballot
// as two 32-bit words.  Every lane of the wave calls it; lanes with f >= total pass set = false, so the bits past the
// end of the last word are clear, and a word that starts at or past total is not written.
__device__ __forceinline__ void pool_store_ballot(uint32_t *bits, uint32_t f, uint32_t total, bool set) {
    const unsigned long long vote = __ballot(set);
    const uint32_t lane = threadIdx.x & 63u;
    if (f < total && (lane & 31u) == 0u) bits[f >> 5] = lane ? (uint32_t)(vote >> 32) : (uint32_t)vote;
}

}  // namespace la3dm_dev

#endif
