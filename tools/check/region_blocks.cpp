// region_blocks.cpp — the region of pack_region / erase_region (la3dm_amd/csrc/host/region_blocks.h) and the host writer of
// the map stream (la3dm_amd/csrc/host/pack_format.h) on a SUBSET of a map's blocks, as a stand-alone CPU program meant to be
// built with a sanitizer:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/check/region_blocks.cpp \
//       -o tools/check/region_blocks -lpthread && tools/check/region_blocks
//
// Every array lives on the heap at its exact size, so a read or write past one is a sanitizer report.  The cases: the key
// fields and the closed box at its six faces and at the ends of the 20-bit range; inside against outside (a partition of any
// key list); klo > khi and null bounds refused; the box between two corner keys; and, for block_depth 1 .. 4, the
// writer over the selected keys of a random pool: the sub-stream validates, names exactly the selected keys in order, and
// every block expands to the nodes it was written from.  Prints one line per case and exits 0 when all hold.
#include <cstdio>
#include <memory>
#include <random>

#include "../../la3dm_amd/csrc/host/pack_format.h"
#include "../../la3dm_amd/csrc/host/region_blocks.h"

namespace R = la3dm_region_blocks;
namespace K = la3dm_pack;

static int g_fail = 0;
static void expect(bool ok, const char *what) {
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++g_fail;
}

static int64_t key_of(int64_t x, int64_t y, int64_t z) { return (x << 40) | (y << 20) | z; }

static R::Box box_of(int32_t x0, int32_t y0, int32_t z0, int32_t x1, int32_t y1, int32_t z1, int inside) {
    R::Box b;
    const int32_t lo[3] = {x0, y0, z0}, hi[3] = {x1, y1, z1};
    const std::string bad = R::check(lo, hi, &b);
    if (!bad.empty()) std::printf("FAIL unexpected refusal: %s\n", bad.c_str()), ++g_fail;
    b.inside = inside;
    return b;
}

static void fields_and_faces() {
    const int64_t k = key_of(0xFFFFF, 0, 0x12345);
    expect(R::field(k, 0) == 0xFFFFF && R::field(k, 1) == 0 && R::field(k, 2) == 0x12345, "the three 20-bit fields");
    const R::Box b = box_of(10, 20, 30, 12, 20, 35, 1);
    bool ok = true;
    for (int x = 8; x <= 14; ++x)
        for (int y = 18; y <= 22; ++y)
            for (int z = 28; z <= 37; ++z) {
                const bool want = x >= 10 && x <= 12 && y == 20 && z >= 30 && z <= 35;
                R::Box out = b;
                out.inside = 0;
                ok = ok && R::selected(key_of(x, y, z), b) == want && R::selected(key_of(x, y, z), out) == !want;
            }
    expect(ok, "a closed box: every face included, inside = 0 is the complement");
    const R::Box all = box_of(0, 0, 0, R::kFieldMax, R::kFieldMax, R::kFieldMax, 1);
    expect(R::selected(key_of(0, 0, 0), all) && R::selected(key_of(R::kFieldMax, R::kFieldMax, R::kFieldMax), all), "the ends of the 20-bit range");
    const R::Box wide = box_of(-5, -5, -5, 1 << 21, 1 << 21, 1 << 21, 1);
    expect(R::selected(key_of(0, 7, R::kFieldMax), wide), "bounds outside the range select what is inside them");
}

static void refusals() {
    const int32_t lo[3] = {5, 5, 5}, hi[3] = {5, 4, 5};
    R::Box b;
    expect(R::check(lo, hi, &b).find("klo > khi on axis 1") != std::string::npos, "klo > khi on one axis is refused and names the axis");
    expect(!R::check(nullptr, hi, &b).empty() && !R::check(lo, nullptr, &b).empty(), "null bounds are refused");
    expect(R::check(lo, lo, nullptr).empty(), "a one-block box is a region (and out may be null)");
    R::Box c;
    expect(R::from_corner_keys(key_of(3, 2, 7), key_of(9, 8, 7), true, &c).empty() && c.lo[0] == 3 && c.hi[0] == 9 && c.lo[1] == 2 && c.hi[1] == 8 &&
               c.lo[2] == 7 && c.hi[2] == 7 && c.inside == 1,
           "the box between two corner keys");
    expect(R::from_corner_keys(key_of(3, 9, 7), key_of(9, 8, 7), false, &c).find("axis 1") != std::string::npos, "corner keys the wrong way round are refused");
}

struct Pool {   // exact-size heap arrays of a random canonical pool
    uint32_t npb;
    std::vector<int64_t> keys;
    std::unique_ptr<float[]> A, B;
    std::unique_ptr<uint8_t[]> S;
};

static Pool random_pool(uint32_t depth, uint32_t nb, std::mt19937 &rng) {
    Pool p;
    p.npb = K::npb_of(depth);
    p.A.reset(new float[(size_t)nb * p.npb]);
    p.B.reset(new float[(size_t)nb * p.npb]);
    p.S.reset(new uint8_t[(size_t)nb * p.npb]);
    const uint32_t dl = depth - 1u;
    for (uint32_t b = 0; b < nb; ++b) {
        p.keys.push_back(key_of(100 + (int64_t)(rng() % 8), 200 + b, rng() & 0xFFFFF));
        float *A = p.A.get() + (size_t)b * p.npb, *B = p.B.get() + (size_t)b * p.npb;
        uint8_t *S = p.S.get() + (size_t)b * p.npb;
        for (uint32_t d = 0; d <= dl; ++d)
            for (uint32_t i = 0; i < (1u << (3u * d)); ++i) {
                const uint32_t n = K::layer_base(d) + i, par = d ? K::layer_base(d - 1u) + (i >> 3) : 0u;
                const bool under = d && ((S[par] & 7u) == K::kStatePruned || (S[par] & 0x40u));   // bit 6: scratch mark "is a leaf"
                const bool leaf = !under && (d == dl || rng() % 5 == 0);
                A[n] = leaf ? (float)(rng() % 1000) * 0.25f : 0.001f;
                B[n] = leaf ? (float)(rng() % 1000) * 0.5f : 0.001f;
                S[n] = (uint8_t)(under ? K::kStatePruned : leaf ? ((rng() % 3) | ((rng() & 1u) << 7) | 0x40u) : 2u);
            }
        for (uint32_t n = 0; n < p.npb; ++n) S[n] &= (uint8_t)~0x40u;
    }
    return p;
}

static void writer_on_a_subset(uint32_t depth, std::mt19937 &rng) {
    const uint32_t nb = 23;
    const Pool p = random_pool(depth, nb, rng);
    la3dm_params prm;
    std::memset(&prm, 0, sizeof(prm));
    prm.variant = 0;
    prm.block_depth = (int)depth;
    prm.resolution = 0.1f;
    prm.prior_A = prm.prior_B = 0.001f;
    const la3dm_pack_header proto = K::make_header(prm, true, nullptr, 0, 0);
    bool ok = true;
    for (int inside = 0; inside <= 1; ++inside) {
        const R::Box box = box_of(102, 205, 0, 105, 219, R::kFieldMax, inside);
        std::vector<int64_t> keys = R::select(p.keys, box);
        std::sort(keys.begin(), keys.end());
        const auto slot_of = [&](int64_t k) { return (size_t)(std::find(p.keys.begin(), p.keys.end(), k) - p.keys.begin()); };
        const std::vector<uint8_t> stream = K::write(proto, keys, [&](uint64_t b, float *A, float *B, uint8_t *S) {
            const size_t s = slot_of(keys[b]);
            std::memcpy(A, p.A.get() + s * p.npb, 4u * p.npb);
            std::memcpy(B, p.B.get() + s * p.npb, 4u * p.npb);
            std::memcpy(S, p.S.get() + s * p.npb, p.npb);
        });
        std::unique_ptr<uint8_t[]> exact(new uint8_t[stream.size()]);   // (the validator on an exact-size copy)
        std::memcpy(exact.get(), stream.data(), stream.size());
        la3dm_pack_header h;
        const std::string bad = K::validate(exact.get(), stream.size(), &h);
        ok = ok && bad.empty() && h.n_blocks == keys.size();
        if (!bad.empty()) std::printf("     validator: %s\n", bad.c_str());
        size_t n_sel = 0;
        for (int64_t k : p.keys) n_sel += R::selected(k, box) ? 1u : 0u;
        ok = ok && n_sel == keys.size() && (inside ? n_sel > 0 && n_sel < nb : true);
        if (!bad.empty() || keys.empty()) continue;
        const K::Layout l = K::layout(h.n_blocks, h.n_leaves, h.nodes_per_block);
        std::unique_ptr<float[]> A(new float[p.npb]), B(new float[p.npb]);
        std::unique_ptr<uint8_t[]> S(new uint8_t[p.npb]);
        for (uint64_t b = 0; b < h.n_blocks; ++b) {
            int64_t key;
            std::memcpy(&key, exact.get() + l.keys + 8 * b, 8);
            ok = ok && key == keys[b];
            K::expand_block(exact.get(), h, l, b, A.get(), B.get(), S.get());
            const size_t s = slot_of(keys[b]);
            ok = ok && std::memcmp(A.get(), p.A.get() + s * p.npb, 4u * p.npb) == 0 && std::memcmp(B.get(), p.B.get() + s * p.npb, 4u * p.npb) == 0 &&
                 std::memcmp(S.get(), p.S.get() + s * p.npb, p.npb) == 0;
        }
    }
    const std::string what = "block_depth " + std::to_string(depth) + ": the writer over the selected keys, inside and outside: valid, the keys in order, every block expands to its nodes";
    expect(ok, what.c_str());
    const R::Box none = box_of(1, 1, 1, 2, 2, 2, 1);
    const std::vector<uint8_t> empty = K::write(proto, R::select(p.keys, none), [](uint64_t, float *, float *, uint8_t *) {});
    expect(empty.size() == K::kHeaderBytes && K::validate(empty.data(), empty.size(), nullptr).empty(), "no block selected: the header alone");
}

int main() {
    std::mt19937 rng(20);
    fields_and_faces();
    refusals();
    for (uint32_t depth = 1; depth <= 4; ++depth) writer_on_a_subset(depth, rng);
    std::printf(g_fail ? "%d case(s) FAILED\n" : "all cases hold\n", g_fail);
    return g_fail ? 1 : 0;
}
