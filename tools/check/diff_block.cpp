// diff_block.cpp — a stand-alone check of la3dm_amd/csrc/host/diff_block.h (the per-block rule of diff, contract:
// include/la3dm_hip.h, la3dm_devmap_diff_host) on hand-built blocks: each side a single root leaf, all finest cells, a
// random tiling, or absent.  Every array is heap memory of its exact size, so a read past an end is a sanitizer report.
// The expected answer comes from the construction itself (which leaf owns which finest cell), not from a climb.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/check/diff_block.cpp -o diff_block && ./diff_block
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <random>
#include <vector>

#include "../../la3dm_amd/csrc/host/diff_block.h"

namespace D = la3dm_diff;

static int g_fail = 0;
static void expect(bool ok, const char *what) {
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++g_fail;
}

struct Leaf {
    uint32_t node;
    uint8_t state;
    float A, B;
};
// a tiling of one block: its leaves in ascending node number and, per finest cell, the leaf that covers it
struct Tree {
    uint32_t depth;
    std::vector<Leaf> leaves;
    std::vector<uint32_t> owner;
};

static Tree build(uint32_t depth, const std::function<bool(uint32_t, uint32_t)> &collapse, const std::function<Leaf(uint32_t)> &value) {
    Tree t;
    t.depth = depth;
    const uint32_t dl = depth - 1u;
    t.owner.assign(1u << (3u * dl), 0u);
    std::vector<std::pair<uint32_t, uint32_t>> found;   // (node, first cell << 8 | layer)
    std::function<void(uint32_t, uint32_t)> walk = [&](uint32_t d, uint32_t i) {
        if (d == dl || collapse(d, i)) {
            found.push_back({D::layer_base(d) + i, (i << (3u * (dl - d))) << 8 | d});
            return;
        }
        for (uint32_t c = 0; c < 8; ++c) walk(d + 1u, 8u * i + c);
    };
    walk(0, 0);
    std::sort(found.begin(), found.end());
    for (uint32_t k = 0; k < found.size(); ++k) {
        Leaf l = value(found[k].first);
        l.node = found[k].first;
        t.leaves.push_back(l);
        const uint32_t d = found[k].second & 0xFFu, c0 = found[k].second >> 8;
        for (uint32_t c = 0; c < (1u << (3u * (dl - d))); ++c) t.owner[c0 + c] = k;
    }
    return t;
}

// the stream's form of a tree: mask words and the three leaf sections, behind `first` leaves of other blocks
struct AsStream {
    std::unique_ptr<uint8_t[]> mask, state, A, B;
    D::StreamBlock view;
    AsStream(const Tree &t, uint32_t first) {
        const uint32_t npb = D::layer_base(t.depth), W = (npb + 31u) >> 5, nl = first + (uint32_t)t.leaves.size();
        std::vector<uint32_t> w(W, 0u);
        for (const Leaf &l : t.leaves) w[l.node >> 5] |= 1u << (l.node & 31u);
        mask.reset(new uint8_t[4u * W]);
        std::memcpy(mask.get(), w.data(), 4u * W);
        state.reset(new uint8_t[nl]);
        A.reset(new uint8_t[4u * nl]);
        B.reset(new uint8_t[4u * nl]);
        std::memset(state.get(), 1, nl);   // the other blocks' leaves: OCCUPIED, (77, 78)
        for (uint32_t k = 0; k < nl; ++k) {
            const float a = 77.0f, b = 78.0f;
            std::memcpy(A.get() + 4u * k, &a, 4);
            std::memcpy(B.get() + 4u * k, &b, 4);
        }
        for (uint32_t k = 0; k < t.leaves.size(); ++k) {
            state[first + k] = t.leaves[k].state;
            std::memcpy(A.get() + 4u * (first + k), &t.leaves[k].A, 4);
            std::memcpy(B.get() + 4u * (first + k), &t.leaves[k].B, 4);
        }
        view = {mask.get(), first, state.get(), A.get(), B.get()};
    }
};

// the pool's form: leaves their values, nodes under a leaf PRUNED with stale values, nodes above UNKNOWN
struct AsMap {
    std::unique_ptr<uint8_t[]> S;
    std::unique_ptr<float[]> A, B;
    D::MapBlock view;
    explicit AsMap(const Tree &t) {
        const uint32_t npb = D::layer_base(t.depth), dl = t.depth - 1u;
        S.reset(new uint8_t[npb]);
        A.reset(new float[npb]);
        B.reset(new float[npb]);
        for (uint32_t n = 0; n < npb; ++n) {
            S[n] = 2;
            A[n] = B[n] = -5.0f;   // dead values: nothing may report them
        }
        for (const Leaf &l : t.leaves) {
            S[l.node] = l.state;
            A[l.node] = l.A;
            B[l.node] = l.B;
            uint32_t d = 0;
            while (d < dl && l.node >= D::layer_base(d + 1u)) ++d;
            uint32_t lo = l.node - D::layer_base(d), n_at = 1;
            for (uint32_t dd = d + 1u; dd <= dl; ++dd) {
                lo *= 8u;
                n_at *= 8u;
                for (uint32_t k = 0; k < n_at; ++k) S[D::layer_base(dd) + lo + k] = (uint8_t)(D::kPruned | 0x80u);
            }
        }
        view = {S.get(), A.get(), B.get()};
    }
};

static uint32_t bits(float v) {
    uint32_t w;
    std::memcpy(&w, &v, 4);
    return w;
}

// diff_block against the answer the two constructions give; then / now may be null
static bool check(const D::Rule &r, const Tree *then, const Tree *now, uint32_t first, uint64_t cap) {
    const uint32_t ncell = 1u << (3u * (r.block_depth - 1u));
    D::Counts want;
    D::List list_want;
    for (uint32_t c = 0; c < ncell; ++c) {
        const Leaf *lt = then ? &then->leaves[then->owner[c]] : nullptr, *ln = now ? &now->leaves[now->owner[c]] : nullptr;
        const uint32_t t = lt ? lt->state & 7u : 3u, n = ln ? ln->state & 7u : 3u;
        ++want.pairs[5u * t + n];
        const bool changed = r.value_mask && lt && ln && t == n && (bits(lt->A) != bits(ln->A) || bits(lt->B) != bits(ln->B));
        if (changed) ++want.value_changed[n];
        if (!(((r.pair_mask >> (5u * t + n)) & 1u) || (changed && ((r.value_mask >> n) & 1u)))) continue;
        ++want.selected;
        if (list_want.cell.size() >= cap) continue;
        list_want.cell.push_back(c);
        list_want.code.push_back((uint8_t)(t | n << 4));
        list_want.A.push_back(ln ? ln->A : r.init_A);
        list_want.B.push_back(ln ? ln->B : r.init_B);
    }
    std::unique_ptr<AsStream> s(then ? new AsStream(*then, first) : nullptr);
    std::unique_ptr<AsMap> m(now ? new AsMap(*now) : nullptr);
    D::Counts got;
    D::List list;
    list.cap = cap;
    D::diff_block(r, s ? &s->view : nullptr, m ? &m->view : nullptr, got, list);
    bool ok = got.selected == want.selected && !std::memcmp(got.pairs, want.pairs, sizeof(got.pairs)) &&
              !std::memcmp(got.value_changed, want.value_changed, sizeof(got.value_changed));
    ok = ok && list.cell == list_want.cell && list.code == list_want.code && list.A.size() == list_want.A.size();
    for (size_t k = 0; ok && k < list.A.size(); ++k) ok = bits(list.A[k]) == bits(list_want.A[k]) && bits(list.B[k]) == bits(list_want.B[k]);
    return ok;
}

int main() {
    std::mt19937 rng(17);
    const uint32_t changed = 0x0FBEFBEu, every = 0x1FFFFFFu;
    const auto never = [](uint32_t, uint32_t) { return false; };
    const auto root = [](uint32_t d, uint32_t) { return d == 0; };
    const auto coin = [&](uint32_t, uint32_t) { return rng() % 4u == 0u; };
    const auto value = [&](uint32_t) {
        const uint8_t states[4] = {0, 1, 2, 4};
        return Leaf{0, (uint8_t)(states[rng() % 4u] | (rng() & 0x80u)), 0.001f + (float)(rng() % 8u), 0.001f + (float)(rng() % 8u)};
    };
    for (uint32_t depth = 1; depth <= 5; ++depth) {
        bool ok = true;
        for (int rep = 0; rep < 4; ++rep) {
            const Tree fine = build(depth, never, value), coarse = build(depth, root, value), mixed = build(depth, coin, value),
                       other = build(depth, coin, value);
            const Tree *side[4] = {&fine, &coarse, &mixed, nullptr};
            for (const Tree *then : side)
                for (const Tree *now : side) {
                    if (!then && !now) continue;
                    for (const uint32_t vm : {0u, 0x1Fu, 1u << 1})
                        for (const uint64_t cap : {(uint64_t)0, (uint64_t)3, ~(uint64_t)0}) {
                            ok = ok && check(D::Rule{depth, 0.001f, 0.001f, changed, vm}, then, now, (uint32_t)(rng() % 5u), cap);
                            ok = ok && check(D::Rule{depth, 0.001f, 0.001f, 1u << (5u * 0u + 1u), vm}, then, now, 0, cap);
                        }
                }
            ok = ok && check(D::Rule{depth, 0.001f, 0.001f, every, 0x1Fu}, &mixed, &other, 2, ~(uint64_t)0);
            // a tree against itself: nothing changed, every pair on the diagonal
            D::Counts n;
            D::List list;
            list.cap = ~(uint64_t)0;
            const AsStream s(mixed, 1);
            const AsMap m(mixed);
            D::diff_block(D::Rule{depth, 0.001f, 0.001f, changed, 0x1Fu}, &s.view, &m.view, n, list);
            uint64_t diagonal = 0;
            for (uint32_t k = 0; k < 5; ++k) diagonal += n.pairs[6u * k];
            ok = ok && n.selected == 0 && list.cell.empty() && diagonal == (1ull << (3u * (depth - 1u)));
        }
        char what[112];
        std::snprintf(what, sizeof(what), "block_depth %u: fine, coarse, mixed and absent sides; masks, caps, a tree against itself", depth);
        expect(ok, what);
    }
    {   // same class, B one bit apart in one leaf: value-changed for that leaf's cells only
        const Tree t = build(3, never, [](uint32_t) { return Leaf{0, 0x81, 2.0f, 3.0f}; });
        Tree u = t;
        uint32_t b = bits(u.leaves[19].B) ^ 1u;
        std::memcpy(&u.leaves[19].B, &b, 4);
        const AsStream s(t, 0);
        const AsMap m(u);
        D::Counts n;
        D::List list;
        list.cap = 8;
        D::diff_block(D::Rule{3, 0.001f, 0.001f, 0u, 1u << 1}, &s.view, &m.view, n, list);
        expect(n.selected == 1 && n.value_changed[1] == 1 && n.pairs[6] == 64 && list.cell.size() == 1 && list.cell[0] == 19 && list.code[0] == 0x11 &&
                   bits(list.B[0]) == b,
               "one bit of B in one leaf: one value-changed cell, listed with the map's values");
    }
    std::printf("%s\n", g_fail ? "diff_block: FAILED" : "diff_block: all cases hold");
    return g_fail ? 1 : 0;
}
