// diff_block.h — the per-block rule of diff (contract: include/la3dm_hip.h, la3dm_devmap_diff_host) on flat arrays: the
// stream block as the stream holds it (mask words, first leaf, the state / A / B sections) against the map block's (S, A, B)
// in la3dm_devmap_download's depth-major node numbering, either side absent.  Per finest cell the two covering leaves, the
// 5 x 5 pair count, the value-changed count and the selected entries in ascending cell order.  Plain C++, no HIP: the
// host-mode map runs it over its blocks (host/bgkoctomap.cpp), tools/check/diff_block.cpp runs it under a sanitizer, and
// dm_diff_count / dm_diff_emit (devmap_diff.h) are its device twins — the same counts and the same list.
#ifndef LA3DM_DIFF_BLOCK_H
#define LA3DM_DIFF_BLOCK_H

#include <cstdint>
#include <cstring>
#include <vector>

namespace la3dm_diff {

constexpr uint32_t kPruned = 3, kMissing = 3;   // PRUNED is never a covering leaf's state: 3 as a class says "no such block"

struct Rule {
    uint32_t block_depth;
    float init_A, init_B;   // A, B reported where the map lacks the block
    uint32_t pair_mask;     // bit 5 * then + now
    uint32_t value_mask;    // bit now; 0: no A or B is compared
};
struct Counts {
    uint64_t pairs[25] = {};
    uint64_t value_changed[5] = {};
    uint64_t selected = 0;
};
// the stream's block: its W mask words, leaf_off[b], and the stream's whole state / A / B sections (bytes: a stream in
// memory need not be aligned)
struct StreamBlock {
    const uint8_t *mask;
    uint32_t first;
    const uint8_t *state, *A, *B;
};
struct MapBlock {
    const uint8_t *S;   // npb nodes each
    const float *A, *B;
};
// the selected cells, appended while fewer than cap are held (Counts::selected counts them all)
struct List {
    uint64_t cap = 0;
    std::vector<uint32_t> cell;
    std::vector<uint8_t> code;
    std::vector<float> A, B;
};

inline uint32_t layer_base(uint32_t d) { return 0x249249u & ((1u << (3u * d)) - 1u); }
inline uint32_t word_at(const uint8_t *p, uint64_t i) {
    uint32_t w;
    std::memcpy(&w, p + 4u * i, 4);
    return w;
}

// One compared block; then == nullptr: a block the stream does not name, now == nullptr: a block the map lacks (not both).
inline void diff_block(const Rule &r, const StreamBlock *then, const MapBlock *now, Counts &n, List &out) {
    const uint32_t dl = r.block_depth - 1u, npb = layer_base(r.block_depth), ncell = 1u << (3u * dl), fine = layer_base(dl);
    const uint32_t W = (npb + 31u) >> 5;
    std::vector<uint32_t> word(W), before(W);   // the mask words and the exclusive prefix of their popcounts
    if (then) {
        uint32_t run = 0;
        for (uint32_t w = 0; w < W; ++w) {
            word[w] = word_at(then->mask, w);
            before[w] = run;
            run += (uint32_t)__builtin_popcount(word[w]);
        }
    }
    for (uint32_t c = 0; c < ncell; ++c) {
        uint32_t cls_then = kMissing, cls_now = kMissing, a_then = 0, b_then = 0;
        float a_now = r.init_A, b_now = r.init_B;
        if (then) {   // the first set mask bit on the way up (a validated stream tiles the block)
            uint32_t d = dl, i = c, n2 = fine + c;
            while (d > 0 && !((word[n2 >> 5] >> (n2 & 31u)) & 1u)) {
                --d;
                i >>= 3;
                n2 = layer_base(d) + i;
            }
            const uint64_t at = (uint64_t)then->first + before[n2 >> 5] + (uint32_t)__builtin_popcount(word[n2 >> 5] & ((1u << (n2 & 31u)) - 1u));
            cls_then = then->state[at] & 7u;
            a_then = word_at(then->A, at);
            b_then = word_at(then->B, at);
        }
        if (now) {   // climb while PRUNED
            uint32_t d = dl, i = c;
            while (d > 0 && (now->S[layer_base(d) + i] & 7u) == kPruned) {
                --d;
                i >>= 3;
            }
            const uint32_t n1 = layer_base(d) + i;
            cls_now = now->S[n1] & 7u;
            a_now = now->A[n1];
            b_now = now->B[n1];
        }
        if (cls_then > 4u || cls_now > 4u) continue;   // (no validated stream and no pool holds such a state)
        ++n.pairs[5u * cls_then + cls_now];
        bool changed = false;
        if (r.value_mask && then && now && cls_then == cls_now) {
            uint32_t a_bits, b_bits;
            std::memcpy(&a_bits, &a_now, 4);
            std::memcpy(&b_bits, &b_now, 4);
            changed = a_bits != a_then || b_bits != b_then;
            if (changed) ++n.value_changed[cls_now];
        }
        if (!(((r.pair_mask >> (5u * cls_then + cls_now)) & 1u) || (changed && ((r.value_mask >> cls_now) & 1u)))) continue;
        ++n.selected;
        if (out.cell.size() >= out.cap) continue;
        out.cell.push_back(c);
        out.code.push_back((uint8_t)(cls_then | (cls_now << 4)));
        out.A.push_back(a_now);
        out.B.push_back(b_now);
    }
}

}  // namespace la3dm_diff

#endif
