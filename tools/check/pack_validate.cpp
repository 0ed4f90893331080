// pack_validate.cpp — the map stream's validator (la3dm_amd/csrc/host/pack_format.h) on untrusted bytes, as a stand-alone
// CPU program meant to be built with a sanitizer:
//
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all tools/check/pack_validate.cpp \
//       -o tools/check/pack_validate && tools/check/pack_validate
//
// It writes valid streams with the format's own host writer (random tilings at block_depth 1 .. 5), checks that they are
// accepted and that expand(write(pool)) is the pool, then feeds the validator the defects of the tests' corrupt table —
// wrong magic / version, truncated, too long, duplicate and out-of-range keys, leaf_off off by one, a mask bit past the end,
// a leaf under a leaf, a hole in the tiling, PRUNED as a leaf state, non-zero padding — and, beyond the table, every prefix
// of a stream, every single-byte change of its header and index sections with the sizes left alone, and headers whose
// counts promise far more than the bytes that follow.  Every stream goes to the validator in a heap buffer of exactly its
// size, so a read past the end is a sanitizer report.  Prints one line per group and exits 0 when every corrupt stream was
// refused and every valid one accepted.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

#include "../../la3dm_amd/csrc/host/pack_format.h"

namespace P = la3dm_pack;

static int g_fail = 0;

// the validator on an exact-size heap copy
static std::string check(const std::vector<uint8_t> &s, la3dm_pack_header *h = nullptr) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[s.size() ? s.size() : 1]);
    if (!s.empty()) std::memcpy(exact.get(), s.data(), s.size());
    return P::validate(exact.get(), s.size(), h);
}
static void refused(const char *name, const std::vector<uint8_t> &s, const char *frag) {
    const std::string r = check(s);
    if (r.empty() || r.find(frag) == std::string::npos) {
        std::printf("FAIL %-28s: expected a refusal with \"%s\", got \"%s\"\n", name, frag, r.c_str());
        ++g_fail;
    }
}

static la3dm_pack_header proto(uint32_t depth, uint32_t variant) {
    la3dm_params p;
    std::memset(&p, 0, sizeof(p));
    p.resolution = 0.1f;
    p.block_depth = (int32_t)depth;
    p.sf2 = 1.0f;
    p.ell = 0.2f;
    p.free_thresh = 0.3f;
    p.occupied_thresh = 0.7f;
    p.var_thresh = 100.0f;
    p.prior_A = 0.5f;
    p.prior_B = 0.25f;
    p.variant = (int32_t)variant;
    p.min_W = 0.001f;
    return P::make_header(p, true, nullptr, 0, 0);
}

struct Pool {
    uint32_t depth, npb;
    std::vector<int64_t> keys;
    std::vector<float> A, B;
    std::vector<uint8_t> S;
};

// canonical pool of random tilings: top down, a node not under a leaf becomes one with probability p or on the finest layer
static Pool random_pool(std::mt19937 &rng, uint32_t depth, uint32_t nb, double p, uint32_t variant) {
    Pool q;
    q.depth = depth;
    q.npb = P::npb_of(depth);
    std::uniform_real_distribution<double> u(0, 1);
    for (uint32_t b = 0; b < nb; ++b) q.keys.push_back(((int64_t)(1000 + 7 * b) << 40) | ((int64_t)(rng() & 0xFFFFF) << 20) | (int64_t)(rng() & 0xFFFFF));
    const la3dm_pack_header defaults = proto(depth, variant);   // dead nodes hold the variant's default node
    q.A.assign((size_t)nb * q.npb, defaults.init_A);
    q.B.assign((size_t)nb * q.npb, defaults.init_B);
    q.S.assign((size_t)nb * q.npb, 2);
    const uint32_t dl = depth - 1;
    for (uint32_t b = 0; b < nb; ++b) {
        uint8_t *S = &q.S[(size_t)b * q.npb];
        std::vector<uint8_t> role(q.npb, 0);   // 0 above, 1 leaf, 2 under a leaf
        for (uint32_t d = 0; d <= dl; ++d)
            for (uint32_t i = 0; i < (1u << (3 * d)); ++i) {
                const uint32_t n = P::layer_base(d) + i;
                const uint8_t up = d ? role[P::layer_base(d - 1) + (i >> 3)] : 0;
                role[n] = up ? 2 : ((d == dl || (b != 0 && u(rng) < p)) ? 1 : 0);
                if (role[n] == 2) S[n] = P::kStatePruned;
                if (role[n] == 1) {
                    const uint8_t states[4] = {0, 1, 2, 4};
                    S[n] = (uint8_t)(states[rng() % (variant == 2 ? 4 : 3)] | ((rng() & 1) ? 0x80 : 0));
                    const uint32_t bits[2] = {(uint32_t)rng(), (uint32_t)rng()};
                    std::memcpy(&q.A[(size_t)b * q.npb + n], &bits[0], 4);
                    std::memcpy(&q.B[(size_t)b * q.npb + n], &bits[1], 4);
                }
            }
    }
    return q;
}

static std::vector<uint8_t> stream_of(const Pool &q, uint32_t variant) {
    return P::write(proto(q.depth, variant), q.keys, [&](uint64_t b, float *A, float *B, uint8_t *S) {
        std::memcpy(A, &q.A[b * q.npb], 4 * q.npb);
        std::memcpy(B, &q.B[b * q.npb], 4 * q.npb);
        std::memcpy(S, &q.S[b * q.npb], q.npb);
    });
}

template <class T>
static void put(std::vector<uint8_t> &s, uint64_t at, T v) {
    std::memcpy(&s[at], &v, sizeof(T));
}
template <class T>
static T get(const std::vector<uint8_t> &s, uint64_t at) {
    T v;
    std::memcpy(&v, &s[at], sizeof(T));
    return v;
}

int main() {
    std::mt19937 rng(12345);
    // 1. valid streams: accepted, and expand(write(pool)) == pool
    size_t n_valid = 0;
    for (uint32_t depth = 1; depth <= 5; ++depth)
        for (uint32_t variant = 0; variant < 4; ++variant)
            for (uint32_t nb : {0u, 1u, 3u, 6u}) {
                const Pool q = random_pool(rng, depth, nb, 0.3, variant);
                const std::vector<uint8_t> s = stream_of(q, variant);
                la3dm_pack_header h;
                const std::string r = check(s, &h);
                if (!r.empty()) {
                    std::printf("FAIL valid stream (depth %u, variant %u, %u blocks) refused: %s\n", depth, variant, nb, r.c_str());
                    ++g_fail;
                    continue;
                }
                const P::Layout l = P::layout(h.n_blocks, h.n_leaves, h.nodes_per_block);
                std::vector<float> A(q.npb), B(q.npb);
                std::vector<uint8_t> S(q.npb);
                for (uint32_t b = 0; b < nb; ++b) {
                    P::expand_block(s.data(), h, l, b, A.data(), B.data(), S.data());
                    if (std::memcmp(S.data(), &q.S[(size_t)b * q.npb], q.npb) || std::memcmp(A.data(), &q.A[(size_t)b * q.npb], 4 * q.npb) ||
                        std::memcmp(B.data(), &q.B[(size_t)b * q.npb], 4 * q.npb)) {
                        std::printf("FAIL round trip (depth %u, variant %u, block %u)\n", depth, variant, b);
                        ++g_fail;
                    }
                }
                ++n_valid;
            }
    std::printf("valid streams: %zu accepted and expanded back to their pools\n", n_valid);

    // 2. the corrupt table, on a depth-3 stream of 3 blocks whose block 1 has one collapsed group of the finest layer
    Pool q = random_pool(rng, 3, 3, 0.0, 0);
    {
        uint8_t *S = &q.S[q.npb];   // block 1: group 5 of layer 2 collapsed into node (1, 5)
        S[P::layer_base(1) + 5] = 0x81;
        for (uint32_t c = 0; c < 8; ++c) S[P::layer_base(2) + 40 + c] = P::kStatePruned;
    }
    const std::vector<uint8_t> valid = stream_of(q, 0);
    la3dm_pack_header h;
    if (!check(valid, &h).empty()) {
        std::printf("FAIL the table's base stream is refused: %s\n", check(valid).c_str());
        return 1;
    }
    const P::Layout l = P::layout(h.n_blocks, h.n_leaves, h.nodes_per_block);
    std::vector<uint8_t> s;
    s = valid, s[6] = 'Q', refused("wrong magic", s, "magic");
    s = valid, put<uint32_t>(s, 8, 2), refused("wrong version", s, "version");
    s = valid, put<uint32_t>(s, 12, 64), refused("wrong header_bytes", s, "header_bytes");
    s = valid, s.resize(s.size() - 16), refused("truncated", s, "total_bytes");
    s = valid, s.resize(100), refused("truncated inside the header", s, "truncated");
    s = valid, s.push_back(0), refused("one byte too long", s, "total_bytes");
    s = valid, put<int64_t>(s, l.keys + 16, q.keys[0]), refused("duplicate key", s, "duplicate");
    s = valid, put<int64_t>(s, l.keys + 8, q.keys[1] | (1ll << 60)), refused("key field out of range", s, "out of range");
    s = valid, put<int64_t>(s, l.keys + 8, -1), refused("negative key", s, "out of range");
    s = valid, put<uint32_t>(s, l.leaf_off + 4, get<uint32_t>(valid, l.leaf_off + 4) + 1), refused("leaf_off off by one", s, "leaf_off");
    s = valid, put<uint32_t>(s, l.leaf_off, 1), refused("leaf_off[0] not 0", s, "leaf_off");
    s = valid, put<uint32_t>(s, l.leaf_off + 8, 0), refused("leaf_off decreases", s, "leaf_off");
    {
        const uint64_t at = l.mask + 4 * (l.W - 1);
        s = valid, put<uint32_t>(s, at, get<uint32_t>(valid, at) | (1u << (h.nodes_per_block % 32))), refused("mask bit past the end", s, "past");
    }
    {
        const uint32_t child = P::layer_base(2) + 40;
        const uint64_t at = l.mask + 4 * (l.W + child / 32);
        s = valid, put<uint32_t>(s, at, get<uint32_t>(valid, at) | (1u << (child % 32))), refused("a leaf under a leaf", s, "under a leaf");
    }
    {
        Pool hole = q;   // a finest leaf of block 2 turned PRUNED without a parent to cover it: the writer leaves it out
        hole.S[2 * (size_t)q.npb + q.npb - 1] = P::kStatePruned;
        refused("a hole in the tiling", stream_of(hole, 0), "tile");
    }
    s = valid, s[l.state] = P::kStatePruned, refused("PRUNED as a leaf state", s, "PRUNED");
    s = valid, s[l.state + 1] = 0x41, refused("state bits 3-6", s, "bits 3-6");
    s = valid, s[l.state + 2] = 4, refused("a state the variant lacks", s, "unknown to the variant");
    s = valid, s[l.leaf_off - 1] = 1, refused("non-zero padding", s, "padding");
    s = valid, s[127] = 1, refused("non-zero reserved byte", s, "reserved");
    s = valid, put<uint32_t>(s, 16, 9), refused("unknown variant", s, "variant");
    s = valid, put<uint32_t>(s, 20, 0), refused("block_depth 0", s, "block_depth");
    s = valid, put<uint32_t>(s, 20, 40), refused("block_depth 40", s, "block_depth");
    s = valid, put<uint32_t>(s, 24, 585), refused("nodes_per_block of another depth", s, "nodes_per_block");
    s = valid, put<uint64_t>(s, 32, ~0ull), refused("n_blocks 2^64 - 1", s, "limit");
    s = valid, put<uint64_t>(s, 32, 1ull << 31), refused("n_blocks 2^31", s, "limit");
    s = valid, put<uint64_t>(s, 32, 50000000), refused("n_blocks beyond the bytes", s, "sections");
    s = valid, put<uint64_t>(s, 40, ~0ull), refused("n_leaves 2^64 - 1", s, "n_leaves");
    s = valid, put<uint64_t>(s, 40, h.n_leaves + 4), refused("n_leaves beyond the bytes", s, "sections");
    std::printf("corrupt table: %s\n", g_fail ? "FAILED" : "every row refused with its message");

    // 2b. a stream large enough for the validator's threads (blocks x nodes >= 2^18): accepted; a defect in a late block and
    // one in the last leaf state are found
    {
        const Pool big = random_pool(rng, 3, 4000, 0.2, 2);
        const std::vector<uint8_t> v = stream_of(big, 2);
        la3dm_pack_header hb;
        if (!check(v, &hb).empty()) {
            std::printf("FAIL the large stream is refused: %s\n", check(v).c_str());
            ++g_fail;
        }
        const P::Layout lb = P::layout(hb.n_blocks, hb.n_leaves, hb.nodes_per_block);
        s = v, put<uint32_t>(s, lb.mask + 4 * (lb.W * 3900), 0), refused("large: a cleared mask word", s, "block 3900");
        s = v, s[lb.state + hb.n_leaves - 1] = 7, refused("large: the last leaf state", s, "unknown to the variant");
        s = v, s[lb.state + hb.n_leaves - 9] = 3, refused("large: PRUNED near the end", s, "PRUNED");
        std::printf("large stream: %llu blocks, %llu leaves\n", (unsigned long long)hb.n_blocks, (unsigned long long)hb.n_leaves);
    }

    // 3. every prefix is refused (the full length is the valid stream)
    size_t n = 0;
    for (size_t len = 0; len < valid.size(); ++len, ++n) {
        s.assign(valid.begin(), valid.begin() + (std::ptrdiff_t)len);
        if (check(s).empty()) {
            std::printf("FAIL prefix of %zu bytes accepted\n", len);
            ++g_fail;
        }
    }
    std::printf("prefixes: %zu refused\n", n);

    // 4. every byte of the header and the index sections (keys, leaf_off, mask) changed three ways: the validator must
    // return (accepting is fine where the change is harmless, e.g. an informational float) without reading out of bounds
    size_t accepted = 0, total = 0;
    for (uint64_t at = 0; at < l.state; ++at)
        for (uint8_t x : {(uint8_t)0x01, (uint8_t)0x80, (uint8_t)0xFF}) {
            s = valid;
            s[at] ^= x;
            accepted += check(s).empty();
            ++total;
        }
    std::printf("single-byte changes: %zu streams validated, %zu of them still valid\n", total, accepted);
    if (g_fail) {
        std::printf("%d FAILURES\n", g_fail);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
