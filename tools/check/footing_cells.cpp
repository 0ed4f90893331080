// footing_cells.cpp — the pure part of footing (la3dm_amd/csrc/host/footing_cells.h: classes of the padded box in; foot
// voxels, list, columns and counts out) against the definition, as a stand-alone CPU program meant to be built with a
// sanitizer:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/check/footing_cells.cpp \
//       -o tools/check/footing_cells && tools/check/footing_cells
//
// Every array lives on the heap at its exact size, so a window that leaves the padded box is a report.  The brute force
// below is the contract's definition voxel by voxel — stand, near, body and foot as predicates on a class lookup that
// aborts outside the padded box —, with no run lengths and no shared intermediate.  The cases: the hand-built scene of the
// tests (floor, kerb, two-voxel step, table, pillar, hole, a missing block) with its recorded counts; random classes on the
// shapes whose columns end with and straddle 32 and 64 voxels; every limit value (h = 32, r = 8, s = 4, c = N = 196, s =
// h - 1, nz = 1); cap = 0, below n, n and above n.  Prints one line per case and exits 0 when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../la3dm_amd/csrc/host/footing_cells.h"

namespace ft = la3dm_footing;

static int g_fail = 0;
static void expect(bool ok, const char *what) {
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++g_fail;
}

struct Box {
    uint32_t dims[3];
    ft::Params p;
    size_t P[3];
    std::unique_ptr<uint8_t[]> cls;   // [PX PY PZ], exact size
    Box(uint32_t nx, uint32_t ny, uint32_t nz, const ft::Params &q) : p(q) {
        dims[0] = nx;
        dims[1] = ny;
        dims[2] = nz;
        ft::padded_dims(dims, p, P);
        cls.reset(new uint8_t[P[0] * P[1] * P[2]]);
        std::memset(cls.get(), 3, P[0] * P[1] * P[2]);   // MISSING
    }
    // class of the region's voxel (i, j, k), any of which may lie in the pads
    uint8_t &at(long i, long j, long k) const {
        const long pi = i + (long)p.radius, pj = j + (long)p.radius, pk = k + 1 + (long)p.step;
        if (pi < 0 || pj < 0 || pk < 0 || pi >= (long)P[0] || pj >= (long)P[1] || pk >= (long)P[2]) {
            std::printf("FAIL the definition asked for a voxel outside the padded box\n");
            std::abort();
        }
        return cls[((size_t)pi * P[1] + (size_t)pj) * P[2] + (size_t)pk];
    }
    bool in(uint32_t mask, long i, long j, long k) const { return (mask >> at(i, j, k)) & 1u; }
    bool stand(long i, long j, long k) const {
        if (!in(p.support_mask, i, j, k - 1)) return false;
        for (long t = 0; t < (long)p.headroom; ++t)
            if (!in(p.clear_mask, i, j, k + t)) return false;
        return true;
    }
    bool near(long i, long j, long k) const {
        for (long dk = -(long)p.step; dk <= (long)p.step; ++dk)
            if (stand(i, j, k + dk)) return true;
        return false;
    }
    bool body(long i, long j, long k) const {
        for (long t = (long)p.step; t < (long)p.headroom; ++t)
            if (!in(p.clear_mask, i, j, k + t)) return false;
        return true;
    }
};

struct Answer {
    std::vector<uint8_t> foot;
    std::vector<uint32_t> index, levels;
    std::vector<int32_t> lowest, highest;
    ft::Counts n;
};

static Answer brute(const Box &b) {
    const long nx = b.dims[0], ny = b.dims[1], nz = b.dims[2], r = (long)b.p.radius;
    Answer a;
    a.foot.assign((size_t)(nx * ny * nz), 0);
    a.levels.assign((size_t)(nx * ny), 0);
    a.lowest.assign((size_t)(nx * ny), -1);
    a.highest.assign((size_t)(nx * ny), -1);
    a.n = ft::Counts{0, 0, 0};
    for (long i = 0; i < nx; ++i)
        for (long j = 0; j < ny; ++j)
            for (long k = 0; k < nz; ++k) {
                if (!b.stand(i, j, k)) continue;
                ++a.n.n_stand;
                bool free_body = true;
                uint32_t carried = 0;
                for (long di = -r; di <= r; ++di)
                    for (long dj = -r; dj <= r; ++dj) {
                        if ((di == 0 && dj == 0) || di * di + dj * dj > r * r) continue;
                        free_body = free_body && b.body(i + di, j + dj, k);
                        carried += b.near(i + di, j + dj, k) ? 1u : 0u;
                    }
                if (!free_body) continue;
                ++a.n.n_body;
                if (carried < b.p.min_support) continue;
                ++a.n.n_foot;
                const size_t col = (size_t)(i * ny + j), f = col * (size_t)nz + (size_t)k;
                a.foot[f] = 1;
                a.index.push_back((uint32_t)f);
                ++a.levels[col];
                if (a.lowest[col] < 0) a.lowest[col] = (int32_t)k;
                a.highest[col] = (int32_t)k;
            }
    return a;
}

// cells() into exact-size heap arrays at the given cap, against the brute force
static bool same(const Box &b, const Answer &want, uint64_t cap) {
    const size_t n = (size_t)b.dims[0] * b.dims[1] * b.dims[2], n_col = (size_t)b.dims[0] * b.dims[1];
    std::unique_ptr<uint8_t[]> foot(new uint8_t[n]);
    std::unique_ptr<uint32_t[]> index(new uint32_t[cap ? cap : 1]), levels(new uint32_t[n_col]);
    std::unique_ptr<int32_t[]> lowest(new int32_t[n_col]), highest(new int32_t[n_col]);
    for (uint64_t t = 0; t < (cap ? cap : 1); ++t) index[t] = 0xDEADBEEFu;
    const ft::Counts got = ft::cells(b.cls.get(), b.dims, b.p, foot.get(), cap, cap ? index.get() : nullptr, levels.get(), lowest.get(), highest.get());
    bool ok = got.n_stand == want.n.n_stand && got.n_body == want.n.n_body && got.n_foot == want.n.n_foot;
    ok = ok && std::memcmp(foot.get(), want.foot.data(), n) == 0;
    for (size_t c = 0; c < n_col; ++c) ok = ok && levels[c] == want.levels[c] && lowest[c] == want.lowest[c] && highest[c] == want.highest[c];
    for (uint64_t t = 0; t < cap; ++t) ok = ok && index[t] == (t < want.index.size() ? want.index[t] : 0xDEADBEEFu);
    // the optional outputs left out: the same counts
    const ft::Counts bare = ft::cells(b.cls.get(), b.dims, b.p, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
    return ok && bare.n_foot == want.n.n_foot && bare.n_stand == want.n.n_stand && bare.n_body == want.n.n_body;
}

static bool all_caps(const Box &b, const Answer &want) {
    const uint64_t n = want.index.size();
    bool ok = true;
    for (uint64_t cap : {(uint64_t)0, (uint64_t)1, n / 2, n, n + 7}) ok = ok && same(b, want, cap);
    return ok;
}

// ---- the hand-built scene: (24, 24, 16), the issue's assignments in their order ------------------------------------
static void fill_scene(Box &b) {
    enum { FREE = 0, OCC = 1, UNK = 2, MISS = 3 };
    for (long i = 0; i < 24; ++i)
        for (long j = 0; j < 24; ++j) {
            for (long k = 0; k < 16; ++k) b.at(i, j, k) = FREE;
            b.at(i, j, 0) = UNK;
            b.at(i, j, 1) = OCC;
            if (i >= 12) b.at(i, j, 2) = OCC;
            if (i >= 18) b.at(i, j, 3) = b.at(i, j, 4) = OCC;
            if (i >= 2 && i < 6 && j >= 2 && j < 6) b.at(i, j, 5) = OCC;
            if (i == 9 && j == 9)
                for (long k = 2; k < 11; ++k) b.at(i, j, k) = OCC;
            if (i >= 2 && i < 5 && j >= 14 && j < 17) b.at(i, j, 1) = UNK;
            if (i >= 16 && j >= 16)
                for (long k = 8; k < 16; ++k) b.at(i, j, k) = MISS;
        }
}

static void scene() {
    struct Row {
        uint32_t clear, h, r, s, c;
        long stand, body, foot;   // -1: not recorded
    };
    const Row rows[] = {{1, 2, 0, 0, 0, 583, -1, 583},   {1, 4, 0, 0, 0, 519, -1, -1},    {1, 4, 2, 1, 0, 519, 290, 290},
                        {1, 4, 2, 1, 6, 519, 290, 285},  {1, 4, 2, 1, 12, 519, 290, 229}, {1, 4, 3, 2, 0, -1, -1, 245},
                        {1, 4, 3, 2, 14, -1, -1, 239},   {1, 4, 3, 2, 28, -1, -1, 187},   {0xD, 4, 2, 1, 12, 567, 471, 245}};
    bool ok = true, counts = true;
    for (const Row &q : rows) {
        Box b(24, 24, 16, ft::Params{2u, q.clear, q.h, q.r, q.s, q.c});
        fill_scene(b);
        const Answer want = brute(b);
        counts = counts && (q.stand < 0 || (long)want.n.n_stand == q.stand) && (q.body < 0 || (long)want.n.n_body == q.body) &&
                 (q.foot < 0 || (long)want.n.n_foot == q.foot);
        ok = ok && all_caps(b, want);
    }
    expect(counts, "scene: the definition gives the recorded counts (583; 519; 290 / 285 / 229; 245 / 239 / 187; 567, 471, 245)");
    expect(ok, "scene: cells == the definition at every recorded parameter set and cap");
}

// dense: mostly FREE, some of every class; else (for a tall body) a blocked voxel in 256 and an unseen one in 32
static void random_fill(Box &b, std::mt19937 &rng, int floor_every, bool dense = true) {
    const size_t n = b.P[0] * b.P[1] * b.P[2];
    for (size_t v = 0; v < n; ++v) {
        const uint32_t x = rng() % (dense ? 16u : 256u);
        if (dense)
            b.cls[v] = (uint8_t)(x < 9 ? 0 : x < 12 ? 1 : x < 14 ? 2 : x < 15 ? 3 : 4);
        else
            b.cls[v] = (uint8_t)(x == 0 ? 1 : x < 5 ? 2 : x < 9 ? 3 : 0);
    }
    for (size_t col = 0; col < b.P[0] * b.P[1]; ++col)   // sheets of ground, so that something stands
        for (size_t z = (size_t)(col % 3); z < b.P[2]; z += (size_t)floor_every) b.cls[col * b.P[2] + z] = 1;
}

static void word_shapes() {
    std::mt19937 rng(11);
    const uint32_t shapes[][3] = {{1, 1, 1},  {1, 1, 31}, {1, 1, 32}, {1, 1, 33}, {1, 1, 63}, {1, 1, 64}, {1, 1, 65},
                                  {2, 2, 64}, {33, 1, 1}, {5, 64, 1}, {3, 5, 7},  {1, 1, 41}};
    const uint32_t hrs[][3] = {{1, 0, 0}, {2, 0, 0}, {4, 2, 1}, {3, 1, 2}, {2, 3, 1}};
    bool ok = true;
    uint64_t found = 0;
    for (const auto &sh : shapes)
        for (const auto &q : hrs)
            for (uint32_t clear : {0x1u, 0xDu, 0x1Du}) {
                const uint32_t N = ft::disc_cells(q[1]);
                for (uint32_t c : {0u, N / 2u, N}) {
                    Box b(sh[0], sh[1], sh[2], ft::Params{2u, clear, q[0], q[1], q[2], c});
                    random_fill(b, rng, 6);
                    const Answer want = brute(b);
                    found += want.n.n_foot;
                    ok = ok && all_caps(b, want);
                }
            }
    std::printf("     (%llu foot voxels over the word shapes)\n", (unsigned long long)found);
    expect(ok && found > 200, "word shapes: cells == the definition on columns that end with and straddle 32 and 64 voxels");
}

static void limits() {
    std::mt19937 rng(5);
    bool ok = ft::disc_cells(0) == 0 && ft::disc_cells(1) == 4 && ft::disc_cells(2) == 12 && ft::disc_cells(3) == 28 && ft::disc_cells(8) == 196;
    expect(ok, "disc_cells: 0, 4, 12, 28 and 196 cells at radius 0, 1, 2, 3 and 8");
    ok = true;
    uint64_t found = 0;
    const uint32_t sets[][5] = {{32, 8, 4, 196, 40}, {32, 8, 4, 98, 40}, {32, 0, 4, 0, 40}, {5, 8, 4, 0, 8}, {1, 8, 0, 196, 3},
                                {2, 1, 1, 4, 4},     {32, 0, 0, 0, 40},  {5, 2, 4, 12, 9}};
    for (const auto &q : sets)
        for (const auto &sh : {std::vector<uint32_t>{1, 1, 1}, std::vector<uint32_t>{4, 3, 1}, std::vector<uint32_t>{6, 7, 45}}) {
            Box b(sh[0], sh[1], sh[2], ft::Params{2u, 0xDu, q[0], q[1], q[2], q[3]});
            random_fill(b, rng, (int)q[4], false);
            const Answer want = brute(b);
            found += want.n.n_foot;
            ok = ok && all_caps(b, want);
        }
    std::printf("     (%llu foot voxels at the limit values)\n", (unsigned long long)found);
    expect(ok && found > 0, "limits: h = 32, r = 8, s = 4, c = N = 196, s = h - 1, h = 1 and nz = 1 against the definition");
}

int main() {
    scene();
    word_shapes();
    limits();
    std::printf("%s\n", g_fail ? "FAILED" : "all ok");
    return g_fail ? 1 : 0;
}
