// surface_cells.cpp — the pure part of surface (la3dm_amd/csrc/host/surface_cells.h: classes of the padded box in; surface
// voxels, list, face masks, normals, dense faces and counts out) against the definition, as a stand-alone CPU program meant
// to be built with a sanitizer:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/check/surface_cells.cpp \
//       -o tools/check/surface_cells && tools/check/surface_cells
//
// Every array lives on the heap at its exact size, so a window that leaves the padded box is a report.  The brute force
// below is the contract's definition voxel by voxel — F_d as a predicate on a class lookup that aborts outside the padded
// box, the normal as a triple loop over the window —, with no separable pass and no shared intermediate.  The cases: the
// hand-built scene of the tests (floor, kerb, two-voxel step, table, pillar, hole, a missing block) with its recorded
// counts; random classes on thin axes and on the shapes whose padded columns end with and straddle 32 and 64 voxels; every
// smooth from 0 to 4; cap = 0, below n, n and above n; list arrays left out one by one.  Prints one line per case and
// exits 0 when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../la3dm_amd/csrc/host/surface_cells.h"

namespace sf = la3dm_surface;

static int g_fail = 0;
static void expect(bool ok, const char *what) {
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++g_fail;
}

struct Box {
    uint32_t dims[3];
    sf::Params p;
    size_t P[3];
    std::unique_ptr<uint8_t[]> cls;   // [PX PY PZ], exact size
    Box(uint32_t nx, uint32_t ny, uint32_t nz, const sf::Params &q) : p(q) {
        dims[0] = nx;
        dims[1] = ny;
        dims[2] = nz;
        sf::padded_dims(dims, p, P);
        cls.reset(new uint8_t[P[0] * P[1] * P[2]]);
        std::memset(cls.get(), 3, P[0] * P[1] * P[2]);   // MISSING
    }
    // class of the region's voxel (i, j, k), any of which may lie in the pads
    uint8_t &at(long i, long j, long k) const {
        const long pad = (long)p.smooth + 1, pi = i + pad, pj = j + pad, pk = k + pad;
        if (pi < 0 || pj < 0 || pk < 0 || pi >= (long)P[0] || pj >= (long)P[1] || pk >= (long)P[2]) {
            std::printf("FAIL the definition asked for a voxel outside the padded box\n");
            std::abort();
        }
        return cls[((size_t)pi * P[1] + (size_t)pj) * P[2] + (size_t)pk];
    }
    bool in(uint32_t mask, long i, long j, long k) const { return (mask >> at(i, j, k)) & 1u; }
    int F(int d, long i, long j, long k) const {
        const long e[3] = {d >> 1 == 0 ? ((d & 1) ? 1 : -1) : 0, d >> 1 == 1 ? ((d & 1) ? 1 : -1) : 0, d >> 1 == 2 ? ((d & 1) ? 1 : -1) : 0};
        return in(p.solid_mask, i, j, k) && in(p.open_mask, i + e[0], j + e[1], k + e[2]) ? 1 : 0;
    }
    uint8_t faces(long i, long j, long k) const {
        uint8_t f = 0;
        for (int d = 0; d < 6; ++d) f |= (uint8_t)(F(d, i, j, k) << d);
        return f;
    }
    void normal(long i, long j, long k, int out[3]) const {
        const long s = (long)p.smooth;
        out[0] = out[1] = out[2] = 0;
        for (long di = -s; di <= s; ++di)
            for (long dj = -s; dj <= s; ++dj)
                for (long dk = -s; dk <= s; ++dk)
                    for (int a = 0; a < 3; ++a) out[a] += F(2 * a + 1, i + di, j + dj, k + dk) - F(2 * a, i + di, j + dj, k + dk);
    }
};

// the host form at this cap, with the arrays `use` names (bit 0 index, 1 faces, 2 normal, 3 dense), against the brute force
static bool same(const Box &b, uint64_t cap, unsigned use, sf::Counts *counts_out = nullptr) {
    const size_t n_vox = (size_t)b.dims[0] * b.dims[1] * b.dims[2];
    std::vector<uint32_t> want_index;
    std::vector<uint8_t> want_faces, want_dense(n_vox);
    std::vector<int16_t> want_normal;
    sf::Counts want = {0, 0, {0, 0, 0, 0, 0, 0}};
    for (long i = 0; i < (long)b.dims[0]; ++i)
        for (long j = 0; j < (long)b.dims[1]; ++j)
            for (long k = 0; k < (long)b.dims[2]; ++k) {
                const size_t f = ((size_t)i * b.dims[1] + (size_t)j) * b.dims[2] + (size_t)k;
                const uint8_t m = b.faces(i, j, k);
                want_dense[f] = m;
                want.n_solid += b.in(b.p.solid_mask, i, j, k);
                for (int d = 0; d < 6; ++d) want.faces[d] += (m >> d) & 1u;
                if (!m) continue;
                ++want.n_surface;
                int nrm[3];
                b.normal(i, j, k, nrm);
                want_index.push_back((uint32_t)f);
                want_faces.push_back(m);
                for (int a = 0; a < 3; ++a) want_normal.push_back((int16_t)nrm[a]);
            }
    // exact-size outputs with a sentinel past min(n, cap)
    const size_t room = (size_t)cap;
    std::unique_ptr<uint32_t[]> index(new uint32_t[room]);
    std::unique_ptr<uint8_t[]> faces(new uint8_t[room]), dense(new uint8_t[n_vox]);
    std::unique_ptr<int16_t[]> normal(new int16_t[3 * room]);
    for (size_t t = 0; t < room; ++t) {
        index[t] = 0xDEADBEEFu;
        faces[t] = 0xEE;
        normal[3 * t] = normal[3 * t + 1] = normal[3 * t + 2] = 0x7EEE;
    }
    std::memset(dense.get(), 0xCD, n_vox);
    const sf::Counts got = sf::cells(b.cls.get(), b.dims, b.p, cap, (use & 1u) ? index.get() : nullptr, (use & 2u) ? faces.get() : nullptr,
                                     (use & 4u) ? normal.get() : nullptr, (use & 8u) ? dense.get() : nullptr);
    if (counts_out) *counts_out = got;
    bool ok = got.n_solid == want.n_solid && got.n_surface == want.n_surface;
    for (int d = 0; d < 6; ++d) ok = ok && got.faces[d] == want.faces[d];
    const size_t filled = std::min<size_t>(room, (size_t)want.n_surface);
    for (size_t t = 0; t < room; ++t) {
        const bool in = t < filled;
        ok = ok && index[t] == ((use & 1u) && in ? want_index[t] : 0xDEADBEEFu);
        ok = ok && faces[t] == ((use & 2u) && in ? want_faces[t] : 0xEE);
        for (size_t a = 0; a < 3; ++a) ok = ok && normal[3 * t + a] == ((use & 4u) && (use & 1u) && in ? want_normal[3 * t + a] : 0x7EEE);
    }
    for (size_t f = 0; f < n_vox; ++f) ok = ok && dense[f] == ((use & 8u) ? want_dense[f] : 0xCD);
    return ok;
}

static void scene(Box &b) {   // the tests' hand-built scene over 24 x 24 x 16, MISSING outside it and in one block
    for (long i = 0; i < 24; ++i)
        for (long j = 0; j < 24; ++j)
            for (long k = 0; k < 16; ++k) {
                uint8_t c = 0;
                if (k == 0) c = 2;
                if (k == 1) c = 1;
                if (i >= 12 && k == 2) c = 1;
                if (i >= 18 && (k == 3 || k == 4)) c = 1;
                if (i >= 2 && i < 6 && j >= 2 && j < 6 && k == 5) c = 1;
                if (i == 9 && j == 9 && k >= 2 && k < 11) c = 1;
                if (i >= 2 && i < 5 && j >= 14 && j < 17 && k == 1) c = 2;
                if (i >= 16 && j >= 16 && k >= 8) c = 3;
                b.at(i, j, k) = c;
            }
}

int main() {
    char what[256];
    // ---- the scene with its recorded counts, every smooth
    const uint64_t rec[4][9] = {{1u << 1, 1u << 0, 615, 1168, 85, 13, 13, 13, 16}, {1u << 1, 0xD, 970, 1168, 112, 112, 64, 64, 583},
                                {0x6, 1u << 0, 624, 1753, 85, 13, 13, 13, 16}, {1u << 1, 0xC, 681, 1168, 27, 99, 51, 51, 567}};
    const uint64_t rec_up[4] = {583, 583, 592, 0};
    for (uint32_t s = 0; s <= 4; ++s)
        for (int r = 0; r < 4; ++r) {
            Box b(24, 24, 16, sf::Params{(uint32_t)rec[r][0], (uint32_t)rec[r][1], s});
            scene(b);
            sf::Counts c;
            const bool ok = same(b, 2000, 15u, &c);
            std::snprintf(what, sizeof(what), "scene solid %#x open %#x smooth %u: n %llu solid %llu", (unsigned)rec[r][0], (unsigned)rec[r][1], s,
                          (unsigned long long)c.n_surface, (unsigned long long)c.n_solid);
            expect(ok && c.n_surface == rec[r][2] && c.n_solid == rec[r][3] && c.faces[0] == rec[r][4] && c.faces[1] == rec[r][5] && c.faces[2] == rec[r][6] &&
                       c.faces[3] == rec[r][7] && c.faces[4] == rec[r][8] && c.faces[5] == rec_up[r],
                   what);
        }
    // ---- random classes: thin axes, padded columns of 31 .. 33 and 63 .. 65 voxels, every smooth, the caps, the arrays left out
    std::mt19937 rng(20261021u);
    const uint32_t shapes[][3] = {{1, 1, 1}, {1, 1, 41}, {33, 1, 1}, {1, 17, 1}, {5, 64, 1}, {3, 5, 7}, {2, 2, 64}, {9, 1, 6}, {1, 9, 6}};
    for (uint32_t s = 0; s <= 4; ++s) {
        std::vector<std::vector<uint32_t>> all;
        for (const auto &sh : shapes) all.push_back({sh[0], sh[1], sh[2]});
        for (uint32_t pz : {31u, 32u, 33u, 63u, 64u, 65u}) all.push_back({2, 3, pz - 2 * (s + 1)});
        for (const auto &sh : all) {
            const sf::Params masks[3] = {{1u << 1, 1u << 0, s}, {0x12, 0xD, s}, {0x6, 0x9, s}};
            for (const sf::Params &p : masks) {
                Box b(sh[0], sh[1], sh[2], p);
                const size_t total = b.P[0] * b.P[1] * b.P[2];
                const uint32_t solid_share = 2 + rng() % 6;
                for (size_t u = 0; u < total; ++u) b.cls[u] = rng() % 10 < solid_share ? 1 : (uint8_t)(rng() % 5);
                sf::Counts c;
                bool ok = same(b, (uint64_t)sh[0] * sh[1] * sh[2] + 7, 15u, &c);
                const uint64_t n = c.n_surface;
                const uint64_t caps[4] = {0, n ? n - 1 : 0, n, n + 1};
                for (uint64_t cap : caps) ok = ok && same(b, cap, 15u);
                for (unsigned use : {0u, 1u, 2u, 3u, 5u, 8u, 9u, 10u, 13u}) ok = ok && same(b, n / 2 + 1, use);
                std::snprintf(what, sizeof(what), "random %u x %u x %u smooth %u solid %#x open %#x: n %llu", sh[0], sh[1], sh[2], s, p.solid_mask, p.open_mask,
                              (unsigned long long)n);
                expect(ok, what);
            }
        }
    }
    std::printf("%s\n", g_fail ? "FAILED" : "all ok");
    return g_fail ? 1 : 0;
}
