// merge_block.cpp — the per-block rule of merge (la3dm_amd/csrc/host/merge_block.h) on hand-built blocks, as a stand-alone
// CPU program meant to be built with a sanitizer:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/check/merge_block.cpp \
//       -o tools/check/merge_block && tools/check/merge_block
//
// Every block lives in heap arrays of exactly nodes-per-block elements, so a read or write past a block is a sanitizer
// report.  The cases: a single node (block_depth 1) fused; an all-default source (everything kept, a coarse destination leaf
// comes back bit-identical); a created block (copied verbatim, odd state bytes included); one cell fused under a coarse
// leaf (the leaf splits, the seven siblings and the seven other groups keep its bytes); a fuse that makes every cell agree
// (the two-level chain collapses to the root with cell 0's values); and random tilings at block_depth 2 .. 5, where the
// counters add up to the block's cells, the result is in canonical form and merging an all-default block into it changes
// nothing.  Prints one line per case and exits 0 when all hold.
#include <cstdio>
#include <memory>
#include <random>

#include "../../la3dm_amd/csrc/host/merge_block.h"

namespace M = la3dm_merge;

static int g_fail = 0;
static void expect(bool ok, const char *what) {
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++g_fail;
}

struct Blk {   // exact-size heap arrays
    uint32_t npb;
    std::unique_ptr<float[]> A, B;
    std::unique_ptr<uint8_t[]> S;
    explicit Blk(uint32_t n) : npb(n), A(new float[n]), B(new float[n]), S(new uint8_t[n]) {}
    Blk(const Blk &o) : Blk(o.npb) {
        std::memcpy(A.get(), o.A.get(), 4u * npb);
        std::memcpy(B.get(), o.B.get(), 4u * npb);
        std::memcpy(S.get(), o.S.get(), npb);
    }
    bool same(const Blk &o) const {
        return std::memcmp(A.get(), o.A.get(), 4u * npb) == 0 && std::memcmp(B.get(), o.B.get(), 4u * npb) == 0 && std::memcmp(S.get(), o.S.get(), npb) == 0;
    }
};

static M::Rule rule(uint32_t depth) { return M::Rule{depth, 0.001f, 0.001f, 0.3f, 0.7f, 100.0f}; }

// canonical block over a tiling: top down, a node not under a leaf becomes a leaf where leaf_at(d, i) says so or on the
// finest layer; a leaf's values come from value(d, i, A, B, S)
template <class LeafAt, class Value>
static Blk canonical(const M::Rule &r, LeafAt leaf_at, Value value) {
    const uint32_t dl = r.block_depth - 1u;
    Blk q(M::layer_base(r.block_depth));
    for (uint32_t d = 0; d <= dl; ++d)
        for (uint32_t i = 0; i < (1u << (3u * d)); ++i) {
            const uint32_t n = M::layer_base(d) + i;
            const uint32_t par = d ? M::layer_base(d - 1u) + (i >> 3) : 0u;
            const bool under = d && ((q.S[par] & 7u) == M::kPruned || (q.S[par] & 0x40u));   // bit 6: scratch mark "is a leaf"
            q.A[n] = r.init_A;
            q.B[n] = r.init_B;
            q.S[n] = under ? M::kPruned : M::kUnknown;
            if (!under && (d == dl || leaf_at(d, i))) {
                value(d, i, q.A[n], q.B[n], q.S[n]);
                q.S[n] |= 0x40u;
            }
        }
    for (uint32_t n = 0; n < q.npb; ++n) q.S[n] &= (uint8_t)~0x40u;
    return q;
}

static Blk all_default(const M::Rule &r) {
    return canonical(r, [](uint32_t, uint32_t) { return false; }, [&](uint32_t, uint32_t, float &a, float &b, uint8_t &s) {
        a = r.init_A;
        b = r.init_B;
        s = M::kUnknown;
    });
}

static bool is_canonical(const M::Rule &r, const Blk &q) {
    const uint32_t dl = r.block_depth - 1u;
    for (uint32_t d = 0; d <= dl; ++d)
        for (uint32_t i = 0; i < (1u << (3u * d)); ++i) {
            const uint32_t n = M::layer_base(d) + i;
            const uint8_t st = q.S[n] & 7u;
            const bool par_dead = d && ((q.S[M::layer_base(d - 1u) + (i >> 3)] & 7u) == M::kPruned);
            if (par_dead && st != M::kPruned) return false;
            const bool leaf = st != M::kPruned && (d == dl || (q.S[M::layer_base(d + 1u) + 8u * i] & 7u) == M::kPruned);
            if (!leaf && (M::bits_of(q.A[n]) != M::bits_of(r.init_A) || M::bits_of(q.B[n]) != M::bits_of(r.init_B))) return false;
            if (!leaf && q.S[n] != M::kPruned && q.S[n] != M::kUnknown) return false;
        }
    return true;
}

int main() {
    {   // block_depth 1: one node, fused
        const M::Rule r = rule(1);
        Blk d = canonical(r, [](uint32_t, uint32_t) { return true; }, [](uint32_t, uint32_t, float &a, float &b, uint8_t &s) { a = 3.0f; b = 1.0f; s = 0x81; });
        Blk s = canonical(r, [](uint32_t, uint32_t) { return true; }, [](uint32_t, uint32_t, float &a, float &b, uint8_t &st) { a = 1.0f; b = 9.0f; st = 0x00; });
        M::Counts n;
        M::merge_block(r, false, d.A.get(), d.B.get(), d.S.get(), s.A.get(), s.B.get(), s.S.get(), n);
        const float A = 3.0f + (1.0f - 0.001f), B = 1.0f + (9.0f - 0.001f);
        expect(n.fused == 1 && n.kept == 0 && n.copied == 0 && d.A[0] == A && d.B[0] == B && d.S[0] == 0x80, "block_depth 1: one node fused, p = 0.29 -> FREE, classified");
    }
    {   // all-default source: kept; a coarse FREE destination leaf (root) expands and comes back bit-identical
        const M::Rule r = rule(3);
        Blk d = canonical(r, [](uint32_t dd, uint32_t) { return dd == 0; }, [](uint32_t, uint32_t, float &a, float &b, uint8_t &s) { a = 0.5f; b = 7.0f; s = 0x00; });
        const Blk before(d), s = all_default(r);
        M::Counts n;
        M::merge_block(r, false, d.A.get(), d.B.get(), d.S.get(), s.A.get(), s.B.get(), s.S.get(), n);
        expect(n.kept == 64 && n.copied + n.fused == 0 && d.same(before), "all-default source: 64 cells kept, the root leaf comes back bit-identical");
    }
    {   // created block: copied verbatim, odd state bytes and all; an UNKNOWN group does not collapse
        const M::Rule r = rule(2);
        Blk s = canonical(r, [](uint32_t, uint32_t) { return false; }, [](uint32_t, uint32_t i, float &a, float &b, uint8_t &st) {
            a = 1.0f + (float)i;
            b = 2.0f;
            st = (uint8_t)((i & 1u ? 0x80u : 0u) | (i % 3u));
        });
        Blk d(s.npb);   // uninitialised on purpose: a created block is only written
        M::Counts n;
        M::merge_block(r, true, d.A.get(), d.B.get(), d.S.get(), s.A.get(), s.B.get(), s.S.get(), n);
        expect(n.copied == 8 && d.same(s), "created block: 8 cells copied verbatim");
    }
    {   // one cell fused under a coarse leaf: it splits; seven siblings and seven groups keep the coarse leaf's bytes
        const M::Rule r = rule(3);
        Blk d = canonical(r, [](uint32_t dd, uint32_t) { return dd == 0; }, [](uint32_t, uint32_t, float &a, float &b, uint8_t &s) { a = 0.5f; b = 7.0f; s = 0x00; });
        Blk s = canonical(r, [](uint32_t, uint32_t) { return false; }, [&](uint32_t, uint32_t i, float &a, float &b, uint8_t &st) {
            a = i == 19 ? 50.0f : r.init_A;   // cell 19 turns OCCUPIED
            b = r.init_B;
            st = i == 19 ? 0x81 : M::kUnknown;
        });
        M::Counts n;
        M::merge_block(r, false, d.A.get(), d.B.get(), d.S.get(), s.A.get(), s.B.get(), s.S.get(), n);
        bool ok = n.kept == 63 && n.fused == 1 && is_canonical(r, d) && d.S[0] == M::kUnknown;
        for (uint32_t g = 0; g < 8; ++g) {   // layer 1: group 2 (cells 16 .. 23) is split, the others are leaves again
            const uint32_t n1 = 1 + g;
            ok = ok && (g == 2 ? d.S[n1] == M::kUnknown : (d.S[n1] == 0x00 && d.A[n1] == 0.5f && d.B[n1] == 7.0f));
        }
        for (uint32_t c = 16; c < 24; ++c) {
            const uint32_t n2 = 9 + c;
            ok = ok && (c == 19 ? (d.S[n2] == 0x81 && d.A[n2] == 0.5f + (50.0f - 0.001f)) : (d.S[n2] == 0x00 && d.A[n2] == 0.5f && d.B[n2] == 7.0f));
        }
        expect(ok, "one cell fused under the root leaf: the leaf splits, 63 cells keep its bytes");
    }
    {   // a fuse that makes all 64 cells agree: the two-level chain collapses to the root with cell 0's values
        const M::Rule r = rule(3);
        Blk d = canonical(r, [](uint32_t, uint32_t) { return false; }, [](uint32_t, uint32_t i, float &a, float &b, uint8_t &s) {
            a = 1.0f + (float)i;   // OCCUPIED cells, but cell 63 is FREE
            b = i == 63 ? 1000.0f : 0.01f;
            s = i == 63 ? 0x80 : 0x81;
        });
        Blk s = canonical(r, [](uint32_t, uint32_t) { return false; }, [&](uint32_t, uint32_t i, float &a, float &b, uint8_t &st) {
            a = i == 63 ? 9000.0f : r.init_A;
            b = r.init_B;
            st = i == 63 ? 0x81 : M::kUnknown;
        });
        M::Counts n;
        M::merge_block(r, false, d.A.get(), d.B.get(), d.S.get(), s.A.get(), s.B.get(), s.S.get(), n);
        bool ok = n.kept == 63 && n.fused == 1 && is_canonical(r, d) && d.S[0] == 0x81 && d.A[0] == 1.0f && d.B[0] == 0.01f;
        for (uint32_t k = 1; k < d.npb; ++k) ok = ok && d.S[k] == M::kPruned;
        expect(ok, "a fuse that makes 64 cells agree: collapsed to the root, cell 0's values");
    }
    std::mt19937 rng(11);
    for (uint32_t depth = 2; depth <= 5; ++depth) {   // random tilings on both sides
        const M::Rule r = rule(depth);
        bool ok = true;
        for (int rep = 0; rep < 6; ++rep) {
            auto coin = [&](uint32_t, uint32_t) { return rng() % 4u == 0u; };
            auto val = [&](uint32_t, uint32_t, float &a, float &b, uint8_t &s) {
                const uint32_t k = rng() % 4u;
                a = k == 0 ? r.init_A : 0.001f + (float)(rng() % 1000u) * 0.01f;
                b = k == 0 ? r.init_B : 0.001f + (float)(rng() % 1000u) * 0.01f;
                s = (uint8_t)((rng() % 3u) | (rng() & 0x80u));
            };
            Blk d = canonical(r, coin, val), s = canonical(r, coin, val);
            M::Counts n;
            M::merge_block(r, false, d.A.get(), d.B.get(), d.S.get(), s.A.get(), s.B.get(), s.S.get(), n);
            ok = ok && n.kept + n.copied + n.fused == (1ull << (3u * (depth - 1u))) && is_canonical(r, d);
            const Blk once(d), none = all_default(r);
            M::merge_block(r, false, d.A.get(), d.B.get(), d.S.get(), none.A.get(), none.B.get(), none.S.get(), n);
            // (a coarse UNKNOWN leaf is no prune result: expanded it stays expanded — its cells keep its bytes)
            M::Counts n2;
            const Blk twice(d);
            M::merge_block(r, false, d.A.get(), d.B.get(), d.S.get(), none.A.get(), none.B.get(), none.S.get(), n2);
            ok = ok && d.same(twice) && is_canonical(r, once);
        }
        char what[96];
        std::snprintf(what, sizeof(what), "block_depth %u: random tilings, counters add up, canonical, a default merge is stable", depth);
        expect(ok, what);
    }
    std::printf("%s\n", g_fail ? "merge_block: FAILED" : "merge_block: all cases hold");
    return g_fail ? 1 : 0;
}
