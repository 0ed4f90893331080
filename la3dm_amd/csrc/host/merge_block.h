// merge_block.h — the per-block rule of merge (contract: include/la3dm_hip.h, la3dm_devmap_merge_host) on flat (A, B, S)
// arrays in la3dm_devmap_download's depth-major node numbering: the covering-leaf lookup, the three cases per finest
// cell, the prune and the canonical write.  Plain C++, no HIP: the host-mode map runs it over its blocks
// (host/bgkoctomap.cpp), tools/check/merge_block.cpp runs it under a sanitizer, and dm_merge_fuse (devmap_merge.h) is its
// device twin — the two give the same bytes.
#ifndef LA3DM_MERGE_BLOCK_H
#define LA3DM_MERGE_BLOCK_H

#include <cstdint>
#include <cstring>
#include <vector>

namespace la3dm_merge {

constexpr uint8_t kPruned = 3, kUnknown = 2, kClassified = 0x80u;

struct Rule {
    uint32_t block_depth;
    float init_A, init_B;                               // the default node: "no evidence", compared bit for bit
    float free_thresh, occupied_thresh, var_thresh;     // Occupancy::update's classification of a fused cell
};
struct Counts {
    uint64_t kept = 0, copied = 0, fused = 0;
};

inline uint32_t layer_base(uint32_t d) { return 0x249249u & ((1u << (3u * d)) - 1u); }
inline uint32_t bits_of(float v) {
    uint32_t w;
    std::memcpy(&w, &v, 4);
    return w;
}

// node number of the covering leaf of finest cell c: climb while PRUNED
inline uint32_t cover(const uint8_t *S, uint32_t dl, uint32_t c) {
    uint32_t d = dl, i = c;
    while (d > 0 && (S[layer_base(d) + i] & 7u) == kPruned) {
        --d;
        i >>= 3;
    }
    return layer_base(d) + i;
}

// Occupancy::update's state of (A, B): the exact-division form (bgk_kernels.h, classify())
inline uint8_t classify(float A, float B, const Rule &r) {
    const float s = A + B;
    const float den = (s * s) * (s + 1.0f);
    const float var = (A * B) / den;
    if (var > r.var_thresh) return 2;
    const float p = A / s;
    return p > r.occupied_thresh ? 1 : (p < r.free_thresh ? 0 : 2);
}

// One block.  (A1, B1, S1): the map's block, npb nodes, read and then overwritten with the result in canonical form; of a
// block the map lacks (created = true: conceptually all-default) they are only written.  (A2, B2, S2): the stream's block
// as expand_block gives it (any pool whose covering leaves are the stream's).
inline void merge_block(const Rule &r, bool created, float *A1, float *B1, uint8_t *S1, const float *A2, const float *B2,
                        const uint8_t *S2, Counts &n) {
    const uint32_t dl = r.block_depth - 1u, npb = layer_base(r.block_depth), ncell = 1u << (3u * dl), fine = layer_base(dl);
    const uint32_t a0 = bits_of(r.init_A), b0 = bits_of(r.init_B);
    std::vector<float> cA(ncell), cB(ncell);
    std::vector<uint8_t> T(npb, kUnknown);   // the result tree's states: finest cells, then what the prune makes of them
    std::vector<uint32_t> src(npb);          // the finest cell a leaf takes its values from
    for (uint32_t c = 0; c < ncell; ++c) {
        const uint32_t n2 = cover(S2, dl, c);
        float a1 = r.init_A, b1 = r.init_B;
        uint8_t s1 = kUnknown;
        if (!created) {
            const uint32_t n1 = cover(S1, dl, c);
            a1 = A1[n1];
            b1 = B1[n1];
            s1 = S1[n1];
        }
        const float a2 = A2[n2], b2 = B2[n2];
        if (bits_of(a2) == a0 && bits_of(b2) == b0) {   // kept: the incoming leaf carries no evidence
            ++n.kept;
        } else if (bits_of(a1) == a0 && bits_of(b1) == b0) {   // copied verbatim
            a1 = a2;
            b1 = b2;
            s1 = S2[n2];
            ++n.copied;
        } else {   // fused
            a1 = a1 + (a2 - r.init_A);
            b1 = b1 + (b2 - r.init_B);
            s1 = (uint8_t)(classify(a1, b1, r) | kClassified);
            ++n.fused;
        }
        cA[c] = a1;
        cB[c] = b1;
        T[fine + c] = s1;
        src[fine + c] = c;
    }
    // OcTree::prune's rule, bottom up; the parent takes child 0's values and whole S byte.  A node above the leaves stays
    // UNKNOWN (2) in T and so never passes for a leaf; on the finest layer every node is one.
    for (uint32_t d = dl; d > 0; --d) {
        const uint32_t lb = layer_base(d), pb = layer_base(d - 1u), ngroup = 1u << (3u * (d - 1u));
        for (uint32_t g = 0; g < ngroup; ++g) {
            const uint32_t c0 = lb + 8u * g;
            const uint8_t st0 = T[c0] & 7u;
            if (st0 == kPruned || st0 == kUnknown) continue;
            bool same = true;
            for (uint32_t c = 1; c < 8; ++c) same = same && (T[c0 + c] & 7u) == st0;
            if (!same) continue;
            T[pb + g] = T[c0];
            src[pb + g] = src[c0];
            for (uint32_t c = 0; c < 8; ++c) T[c0 + c] = kPruned;
        }
    }
    // canonical write, every node once: under a collapsed group the deeper layers are PRUNED already (a collapsing child is
    // a leaf, so its own children were collapsed before it)
    for (uint32_t d = 0; d <= dl; ++d)
        for (uint32_t i = 0; i < (1u << (3u * d)); ++i) {
            const uint32_t nd = layer_base(d) + i;
            const uint8_t st = T[nd] & 7u;
            const bool leaf = st != kPruned && (d == dl || st != kUnknown);
            A1[nd] = leaf ? cA[src[nd]] : r.init_A;
            B1[nd] = leaf ? cB[src[nd]] : r.init_B;
            S1[nd] = leaf ? T[nd] : (st == kPruned ? kPruned : kUnknown);
        }
}

}  // namespace la3dm_merge

#endif
