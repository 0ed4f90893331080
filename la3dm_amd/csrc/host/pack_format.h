// pack_format.h — the host code of the map stream (contract: include/la3dm_hip.h, la3dm_devmap_pack_host): the section
// layout, the header of a context, the validator of untrusted bytes, and the writer / expander over flat per-block node
// arrays that the host-mode map uses.  Plain C++, no HIP: it is compiled into libla3dm_hip.so (devmap.hip, la3dm_hip.hip),
// into libla3dm_map.so (host/bgkoctomap.cpp) and into tools/check/pack_validate.cpp, which runs it under a sanitizer.
#ifndef LA3DM_PACK_FORMAT_H
#define LA3DM_PACK_FORMAT_H

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../../include/la3dm_hip.h"

namespace la3dm_pack {

constexpr uint32_t kHeaderBytes = 128, kStatePruned = 3, kStateUncertain = 4;
constexpr uint64_t kPoolNodeLimit = 0xFFFFFFFFull;   // grow_pool: node indices travel as 32-bit words
static_assert(sizeof(la3dm_pack_header) == kHeaderBytes, "the header struct is the first 128 bytes of the stream");

inline uint64_t align16(uint64_t v) { return (v + 15u) & ~(uint64_t)15u; }
inline uint32_t npb_of(uint32_t depth) { return (uint32_t)(((1ull << (3u * depth)) - 1u) / 7u); }
inline uint32_t layer_base(uint32_t d) { return 0x249249u & ((1u << (3u * d)) - 1u); }
inline uint32_t float_bits(float v) {
    uint32_t w;
    std::memcpy(&w, &v, 4);
    return w;
}

struct Layout {
    uint32_t W;   // mask words per block
    uint64_t keys, leaf_off, mask, state, A, B, total;   // byte offsets of the sections, the stream's size
};
// sections of a stream of n_blocks blocks and n_leaves leaves (n_blocks * npb <= 2^32: nothing here overflows)
inline Layout layout(uint64_t n_blocks, uint64_t n_leaves, uint32_t npb) {
    Layout l;
    l.W = (npb + 31u) / 32u;
    l.keys = kHeaderBytes;
    if (n_blocks == 0) {   // an empty map is the header alone
        l.leaf_off = l.mask = l.state = l.A = l.B = l.total = kHeaderBytes;
        return l;
    }
    l.leaf_off = align16(l.keys + 8u * n_blocks);
    l.mask = align16(l.leaf_off + 4u * (n_blocks + 1u));
    l.state = align16(l.mask + 4u * n_blocks * l.W);
    l.A = align16(l.state + n_leaves);
    l.B = align16(l.A + 4u * n_leaves);
    l.total = align16(l.B + 4u * n_leaves);
    return l;
}

// the header of a map with these parameters; exact_gp (may be null) = {min_var, max_var, max_known_var} as the map class
// was constructed with, else the inverses of the context's values
inline la3dm_pack_header make_header(const la3dm_params &p, bool lv_original_size, const float *exact_gp, uint64_t n_blocks,
                                     uint64_t n_leaves) {
    la3dm_pack_header h;
    std::memset(&h, 0, sizeof(h));
    std::memcpy(h.magic, "LA3DMAP", 8);
    h.version = LA3DM_PACK_VERSION;
    h.header_bytes = kHeaderBytes;
    h.variant = (uint32_t)p.variant;
    h.block_depth = (uint32_t)p.block_depth;
    h.nodes_per_block = npb_of((uint32_t)p.block_depth);
    h.flags = p.variant == 2 && lv_original_size ? LA3DM_PACK_FLAG_LV_ORIGINAL_SIZE : 0u;
    h.n_blocks = n_blocks;
    h.n_leaves = n_leaves;
    h.total_bytes = layout(n_blocks, n_leaves, h.nodes_per_block).total;
    h.init_A = p.variant == 1 ? 0.0f : p.prior_A;   // la3dm_devmap_create
    h.init_B = p.variant == 1 ? p.min_ivar : p.prior_B;
    h.resolution = p.resolution;
    h.sf2 = p.sf2;
    h.ell = p.ell;
    h.free_thresh = p.free_thresh;
    h.occupied_thresh = p.occupied_thresh;
    if (p.variant != 1) {
        h.var_thresh = p.var_thresh;
        h.prior_A = p.prior_A;
        h.prior_B = p.prior_B;
    } else {
        h.noise = p.noise;
        h.l = p.l;
        h.min_var = exact_gp ? exact_gp[0] : 1.0f / p.max_ivar;
        h.max_var = exact_gp ? exact_gp[1] : 1.0f / p.min_ivar;
        h.max_known_var = exact_gp ? exact_gp[2] : 1.0f / p.min_known_ivar;
    }
    if (p.variant == 2) h.min_W = p.min_W;
    return h;
}

// the mask and leaf_off checks of blocks [b0, b1) of a stream whose header and section extents were checked; "" = none fails
inline std::string check_blocks(const uint8_t *p, const la3dm_pack_header &h, const Layout &l, uint64_t b0, uint64_t b1) {
    const uint32_t npb = h.nodes_per_block, dl = h.block_depth - 1u;
    const uint64_t ncell = 1ull << (3u * dl);
    const uint8_t *lo = p + l.leaf_off, *mk = p + l.mask;
    std::vector<uint32_t> w(l.W);
    for (uint64_t b = b0; b < b1; ++b) {
        uint32_t prev, next;
        std::memcpy(&prev, lo + 4u * b, 4);
        std::memcpy(&next, lo + 4u * (b + 1u), 4);
        if (next < prev) return "leaf_off decreases at block " + std::to_string(b);
        std::memcpy(w.data(), mk + 4u * b * l.W, 4u * l.W);
        if ((npb & 31u) && (w[l.W - 1u] >> (npb & 31u))) return "mask bit at or past nodes_per_block in block " + std::to_string(b);
        uint32_t pop = 0;
        uint64_t cover = 0;
        for (uint32_t d = 0; d <= dl; ++d) {
            const uint32_t base = layer_base(d), cnt = 1u << (3u * d);
            for (uint32_t i = 0; i < cnt; ++i) {
                const uint32_t n = base + i;
                if (!((w[n >> 5] >> (n & 31u)) & 1u)) continue;
                ++pop;
                cover += 1ull << (3u * (dl - d));
                for (uint32_t ad = d, ai = i; ad > 0;) {   // every ancestor must be clear
                    --ad;
                    ai >>= 3;
                    const uint32_t a = layer_base(ad) + ai;
                    if ((w[a >> 5] >> (a & 31u)) & 1u) return "a leaf under a leaf in block " + std::to_string(b) + " (node " + std::to_string(n) + ")";
                }
            }
        }
        if (next - prev != pop)
            return "leaf_off of block " + std::to_string(b) + " gives " + std::to_string(next - prev) + " leaves, its mask " + std::to_string(pop);
        if (cover != ncell) return "the leaves of block " + std::to_string(b) + " do not tile it (a hole in the tiling)";
    }
    return "";
}

// Everything the contract lists, in its order; "" = a valid stream (then *out, when given, is its header).  Reads no byte
// at or past buf + size and derives no index from the stream before that index was checked.
inline std::string validate(const void *buf, uint64_t size, la3dm_pack_header *out) {
    if (!buf) return "null stream";
    if (size < kHeaderBytes) return "truncated: " + std::to_string(size) + " bytes are less than the header's 128";
    const uint8_t *p = (const uint8_t *)buf;
    la3dm_pack_header h;
    std::memcpy(&h, p, kHeaderBytes);
    if (std::memcmp(h.magic, "LA3DMAP", 8) != 0) return "wrong magic: not a map stream";
    if (h.version != LA3DM_PACK_VERSION) return "unsupported version " + std::to_string(h.version);
    if (h.header_bytes != kHeaderBytes) return "header_bytes is " + std::to_string(h.header_bytes) + ", not 128";
    if (h.total_bytes != size)
        return "total_bytes is " + std::to_string(h.total_bytes) + " but the stream has " + std::to_string(size) + " bytes";
    if (h.variant > 3u) return "unknown variant " + std::to_string(h.variant);
    if (h.block_depth < 1u || h.block_depth > 6u) return "block_depth " + std::to_string(h.block_depth) + " is outside 1..6";
    const uint32_t npb = npb_of(h.block_depth), dl = h.block_depth - 1u;
    if (h.nodes_per_block != npb) return "nodes_per_block does not belong to block_depth";
    if (h.flags & ~(h.variant == 2u ? LA3DM_PACK_FLAG_LV_ORIGINAL_SIZE : 0u)) return "unknown flag bits";
    for (uint8_t r : h.reserved)
        if (r) return "non-zero reserved bytes in the header";
    if (h.n_blocks > kPoolNodeLimit / npb) return "n_blocks x nodes_per_block exceeds the pool's limit of 2^32 nodes";
    const uint64_t ncell = 1ull << (3u * dl);
    if (h.n_leaves > h.n_blocks * ncell) return "n_leaves exceeds n_blocks x 8^(block_depth - 1)";
    const Layout l = layout(h.n_blocks, h.n_leaves, npb);
    if (l.total != size) return "the sections of the header's counts take " + std::to_string(l.total) + " bytes, the stream has " + std::to_string(size);
    if (h.n_blocks == 0) {
        if (out) *out = h;
        return "";
    }
    const uint64_t nb = h.n_blocks;
    // padding: the gaps between the ends of the sections' payloads and the next section
    const uint64_t ends[6][2] = {{l.keys + 8u * nb, l.leaf_off}, {l.leaf_off + 4u * (nb + 1u), l.mask}, {l.mask + 4u * nb * l.W, l.state},
                                 {l.state + h.n_leaves, l.A},    {l.A + 4u * h.n_leaves, l.B},          {l.B + 4u * h.n_leaves, l.total}};
    for (const auto &e : ends)
        for (uint64_t i = e[0]; i < e[1]; ++i)
            if (p[i]) return "non-zero padding byte at offset " + std::to_string(i);
    // keys: 60 bits, distinct
    std::vector<int64_t> keys(nb);
    std::memcpy(keys.data(), p + l.keys, 8u * nb);
    for (uint64_t b = 0; b < nb; ++b)
        if (keys[b] < 0 || (keys[b] >> 60) != 0) return "key of block " + std::to_string(b) + " has a field out of range (bits above bit 59)";
    std::sort(keys.begin(), keys.end());
    for (uint64_t b = 1; b < nb; ++b)
        if (keys[b] == keys[b - 1]) return "duplicate block key " + std::to_string(keys[b]);
    // per block: mask bits in range, popcount = the leaf_off difference, no leaf under a leaf, the leaves tile the block
    uint32_t first, last;
    std::memcpy(&first, p + l.leaf_off, 4);
    std::memcpy(&last, p + l.leaf_off + 4u * nb, 4);
    if (first != 0u) return "leaf_off[0] is not 0";
    // (blocks are independent: a large stream is checked by a few threads, and the refusal reported is that of the lowest block)
    const unsigned hw = std::thread::hardware_concurrency();
    const uint64_t n_threads = nb * npb < (1u << 18) ? 1u : std::min<uint64_t>(std::max(1u, std::min(hw, 8u)), nb);
    std::vector<std::string> why(n_threads);
    std::vector<std::thread> pool;
    uint64_t started = 1;
    try {
        for (; started < n_threads; ++started)
            pool.emplace_back([&, started] { why[started] = check_blocks(p, h, l, nb * started / n_threads, nb * (started + 1) / n_threads); });
    } catch (const std::system_error &) {   // no more threads to be had: this one does the rest
    }
    why[0] = check_blocks(p, h, l, 0, nb / n_threads);
    for (std::thread &t : pool) t.join();
    for (uint64_t t = started; t < n_threads; ++t) why[t] = check_blocks(p, h, l, nb * t / n_threads, nb * (t + 1) / n_threads);
    for (const std::string &w : why)
        if (!w.empty()) return w;
    if ((uint64_t)last != h.n_leaves) return "leaf_off[n_blocks] is not n_leaves";
    // leaf states, eight at a time; the slow loop only words a refusal
    const uint8_t *st = p + l.state;
    const uint64_t k01 = 0x0101010101010101ull;
    uint64_t bad_bits = 0, i8 = 0;
    for (; i8 + 8 <= h.n_leaves; i8 += 8) {
        uint64_t w8;
        std::memcpy(&w8, st + i8, 8);
        const uint64_t b0 = w8 & k01, b1 = (w8 >> 1) & k01, b2 = (w8 >> 2) & k01;
        // bits 3-6; PRUNED (3) and 7; 5 and 6; UNCERTAIN (4) where the variant has none
        bad_bits |= (w8 & 0x7878787878787878ull) | (b0 & b1) | (b2 & (b0 | b1)) | (h.variant == 2u ? 0ull : b2);
    }
    for (uint64_t i = bad_bits ? 0 : i8; i < h.n_leaves; ++i) {
        const uint32_t sv = st[i] & 7u;
        if (st[i] & 0x78u) return "state byte of leaf " + std::to_string(i) + " has bits 3-6 set";
        if (sv == kStatePruned) return "PRUNED as the state of leaf " + std::to_string(i);
        if (sv > 2u && !(sv == kStateUncertain && h.variant == 2u)) return "state " + std::to_string(sv) + " of leaf " + std::to_string(i) + " is unknown to the variant";
    }
    if (out) *out = h;
    return "";
}

// what the loading map must agree with, floats by bit pattern; "" = it does
inline std::string mismatch(const la3dm_pack_header &h, const la3dm_pack_header &mine) {
    if (h.variant != mine.variant) return "the stream's variant " + std::to_string(h.variant) + " is not the map's " + std::to_string(mine.variant);
    if (h.block_depth != mine.block_depth)
        return "the stream's block_depth " + std::to_string(h.block_depth) + " is not the map's " + std::to_string(mine.block_depth);
    if (h.nodes_per_block != mine.nodes_per_block) return "the stream's nodes_per_block is not the map's";
    if (float_bits(h.resolution) != float_bits(mine.resolution)) return "the stream's resolution is not the map's";
    if (float_bits(h.init_A) != float_bits(mine.init_A) || float_bits(h.init_B) != float_bits(mine.init_B))
        return "the stream's default node (prior_A, prior_B; GP: 0, 1 / max_var) is not the map's";
    return "";
}

// covering leaf: not PRUNED, and on the finest layer or with child 0 PRUNED (S = one block's state bytes)
inline bool is_leaf(const uint8_t *S, uint32_t d, uint32_t i, uint32_t dl) {
    if ((S[layer_base(d) + i] & 7u) == kStatePruned) return false;
    return d == dl || (S[layer_base(d + 1u) + 8u * i] & 7u) == kStatePruned;
}

// The stream of n_blocks blocks given in order: node(b, A, B, S) fills block b's npb values in depth-major order.
template <class NodeFn>
inline std::vector<uint8_t> write(const la3dm_pack_header &proto, const std::vector<int64_t> &keys, NodeFn node) {
    const uint32_t npb = proto.nodes_per_block, dl = proto.block_depth - 1u, W = (npb + 31u) / 32u;
    const uint64_t nb = keys.size();
    std::vector<float> A(npb), B(npb);
    std::vector<uint8_t> S(npb), st;
    std::vector<float> la, lb;
    std::vector<uint32_t> off(nb + 1u, 0u), mask(nb * W, 0u);
    for (uint64_t b = 0; b < nb; ++b) {
        node(b, A.data(), B.data(), S.data());
        for (uint32_t d = 0; d <= dl; ++d)
            for (uint32_t i = 0; i < (1u << (3u * d)); ++i) {
                if (!is_leaf(S.data(), d, i, dl)) continue;
                const uint32_t n = layer_base(d) + i;
                mask[b * W + (n >> 5)] |= 1u << (n & 31u);
                st.push_back(S[n]);
                la.push_back(A[n]);
                lb.push_back(B[n]);
            }
        off[b + 1u] = (uint32_t)st.size();
    }
    la3dm_pack_header h = proto;
    h.n_blocks = nb;
    h.n_leaves = st.size();
    const Layout l = layout(nb, st.size(), npb);
    h.total_bytes = l.total;
    std::vector<uint8_t> out(l.total, 0);
    std::memcpy(out.data(), &h, kHeaderBytes);
    if (nb) {
        std::memcpy(out.data() + l.keys, keys.data(), 8u * nb);
        std::memcpy(out.data() + l.leaf_off, off.data(), 4u * (nb + 1u));
        std::memcpy(out.data() + l.mask, mask.data(), 4u * nb * W);
        if (!st.empty()) {
            std::memcpy(out.data() + l.state, st.data(), st.size());
            std::memcpy(out.data() + l.A, la.data(), 4u * la.size());
            std::memcpy(out.data() + l.B, lb.data(), 4u * lb.size());
        }
    }
    return out;
}

// the canonical nodes of block b of a VALIDATED stream: a leaf takes its values, a node under a leaf (init, PRUNED), every
// other node (init, UNKNOWN)
inline void expand_block(const uint8_t *stream, const la3dm_pack_header &h, const Layout &l, uint64_t b, float *A, float *B, uint8_t *S) {
    const uint32_t npb = h.nodes_per_block, dl = h.block_depth - 1u;
    uint32_t first;
    std::memcpy(&first, stream + l.leaf_off + 4u * b, 4);
    const uint8_t *mk = stream + l.mask + 4u * b * l.W;
    uint32_t rank = 0;
    for (uint32_t d = 0; d <= dl; ++d)
        for (uint32_t i = 0; i < (1u << (3u * d)); ++i) {
            const uint32_t n = layer_base(d) + i;
            uint32_t word;
            std::memcpy(&word, mk + 4u * (n >> 5), 4);
            if ((word >> (n & 31u)) & 1u) {
                const uint64_t at = (uint64_t)first + rank++;
                S[n] = stream[l.state + at];
                std::memcpy(&A[n], stream + l.A + 4u * at, 4);
                std::memcpy(&B[n], stream + l.B + 4u * at, 4);
                continue;
            }
            A[n] = h.init_A;
            B[n] = h.init_B;
            // under a leaf: the parent is a leaf or is itself under one (layers are visited top down)
            const uint32_t par = d ? layer_base(d - 1u) + (i >> 3) : 0u;
            uint32_t pw = 0;
            if (d) std::memcpy(&pw, mk + 4u * (par >> 5), 4);
            const bool under = d && (((pw >> (par & 31u)) & 1u) || (S[par] & 7u) == kStatePruned);
            S[n] = (uint8_t)(under ? kStatePruned : 2u);
        }
    (void)npb;
}

}  // namespace la3dm_pack

#endif
