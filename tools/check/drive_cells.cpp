// drive_cells.cpp — the pure part of drive (la3dm_amd/csrc/host/drive_cells.h: member bytes, seeds and targets in; costs,
// parents and the answers at the targets out) against the definition, as a stand-alone CPU program meant to be built with
// a sanitizer:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/check/drive_cells.cpp \
//       -o tools/check/drive_cells && tools/check/drive_cells
//
// Every array lives on the heap at its exact size, so a neighbour or a snap read that leaves the region is a report.  The
// brute force below is the contract's definition voxel by voxel: 64-bit costs relaxed over every voxel and every allowed
// offset until nothing changes (no heap, no early cut), the cut at max_cost afterwards, the parents as the first code q in
// ascending order that satisfies the contract's four conditions, snap as a downward scan.  The cases: the hand-built sets of
// the tests (flat floor, stairs that rise 1 .. 5, the brick-border links, floor and shelf with and without the ramp, the
// serpentine), random member sets at both connectivities and every step with up != down, and every limit value (step 4,
// snap 32, move and climb 2^16, max_cost 1 and 2^31, a region of one voxel, no seed, no member).  Prints one line per case
// and exits 0 when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../la3dm_amd/csrc/host/drive_cells.h"

namespace dr = la3dm_drive;

static int g_fail = 0;
static void expect(bool ok, const std::string &what) {
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what.c_str());
    if (!ok) ++g_fail;
}

struct Set {
    uint32_t dims[3];
    size_t n;
    std::unique_ptr<uint8_t[]> member;   // [nx ny nz], exact size
    Set(uint32_t nx, uint32_t ny, uint32_t nz) : n((size_t)nx * ny * nz), member(new uint8_t[(size_t)nx * ny * nz]) {
        dims[0] = nx;
        dims[1] = ny;
        dims[2] = nz;
        std::memset(member.get(), 0, n);
    }
    uint32_t flat(uint32_t i, uint32_t j, uint32_t k) const { return (i * dims[1] + j) * dims[2] + k; }
    void add(uint32_t i, uint32_t j, uint32_t k) { member[flat(i, j, k)] = 1; }
    bool inside(long i, long j, long k) const { return i >= 0 && j >= 0 && k >= 0 && i < (long)dims[0] && j < (long)dims[1] && k < (long)dims[2]; }
    bool is(long i, long j, long k) const { return inside(i, j, k) && member[flat((uint32_t)i, (uint32_t)j, (uint32_t)k)]; }
};

// the contract, term by term
static bool move_allowed(const dr::Params &p, int a, int b, int c) {
    if (a == 0 && b == 0) return false;
    if (std::abs(a) > 1 || std::abs(b) > 1 || std::abs(c) > (int)p.step) return false;
    return p.connectivity == 8 || std::abs(a) + std::abs(b) == 1;
}
static long long move_cost(const dr::Params &p, int a, int b, int c) {
    return (long long)p.move_cost[std::abs(a) + std::abs(b) - 1] + (c > 0 ? (long long)p.climb_up * c : (long long)p.climb_down * -c);
}
static long long snap_of(const Set &s, uint32_t snap, uint32_t f) {   // -1: none
    if (f >= s.n) return -1;
    const long k = (long)(f % s.dims[2]);
    for (long t = 0; t <= (long)snap && k - t >= 0; ++t)
        if (s.member[f - (uint32_t)t]) return (long long)f - t;
    return -1;
}

static bool check(const Set &s, const std::vector<uint32_t> &seeds, const std::vector<uint32_t> &targets, const dr::Params &p, const std::string &what,
                  dr::Counts *counts = nullptr, std::vector<uint32_t> *cost_out = nullptr) {
    const long long none = -1;
    std::vector<long long> cost(s.n, none);
    std::vector<uint8_t> seeded(s.n, 0);
    for (const uint32_t f : seeds) {
        const long long m = snap_of(s, p.snap, f);
        if (m >= 0) {
            seeded[(size_t)m] = 1;
            cost[(size_t)m] = 0;
        }
    }
    const long nz = s.dims[2], ny = s.dims[1];
    for (bool changed = true; changed;) {
        changed = false;
        for (size_t f = 0; f < s.n; ++f) {
            if (cost[f] == none) continue;
            const long k = (long)(f % nz), j = (long)((f / nz) % ny), i = (long)(f / ((size_t)nz * ny));
            for (int a = -1; a <= 1; ++a)
                for (int b = -1; b <= 1; ++b)
                    for (int c = -dr::kMaxStep; c <= dr::kMaxStep; ++c) {
                        if (!move_allowed(p, a, b, c) || !s.is(i + a, j + b, k + c)) continue;
                        const size_t v = s.flat((uint32_t)(i + a), (uint32_t)(j + b), (uint32_t)(k + c));
                        const long long cand = cost[f] + move_cost(p, a, b, c);
                        if (cost[v] == none || cand < cost[v]) {
                            cost[v] = cand;
                            changed = true;
                        }
                    }
        }
    }
    for (size_t f = 0; f < s.n; ++f)
        if (cost[f] > (long long)p.max_cost) cost[f] = none;
    // the code under test, every output on the heap at its exact size
    std::unique_ptr<uint32_t[]> got_cost(new uint32_t[s.n]), got_tc(new uint32_t[targets.size()]), got_ti(new uint32_t[targets.size()]);
    std::unique_ptr<uint8_t[]> got_parent(new uint8_t[s.n]);
    std::unique_ptr<uint32_t[]> sd(new uint32_t[seeds.size()]), tg(new uint32_t[targets.size()]), list(new uint32_t[s.n + 2]), om(new uint32_t[s.n + 2]);
    std::copy(seeds.begin(), seeds.end(), sd.get());
    std::copy(targets.begin(), targets.end(), tg.get());
    for (size_t f = 0; f < s.n + 2; ++f) list[f] = (uint32_t)(s.n + 1 - f);   // every voxel, two strays, descending
    const dr::Counts c = dr::cells(s.dims, s.member.get(), sd.get(), (uint32_t)seeds.size(), tg.get(), (uint32_t)targets.size(), list.get(),
                                   (uint32_t)(s.n + 2), p, got_cost.get(), got_parent.get(), om.get(), got_tc.get(), got_ti.get());
    bool ok = true;
    uint32_t n_members = 0, n_seeded = 0, n_reached = 0, most = 0;
    for (size_t f = 0; f < s.n; ++f) {
        const uint32_t want = cost[f] == none ? dr::kNone : (uint32_t)cost[f];
        ok = ok && got_cost[f] == want;
        n_members += s.member[f] ? 1u : 0u;
        n_seeded += seeded[f];
        if (cost[f] != none) {
            ++n_reached;
            most = std::max(most, want);
        }
        // the parent from the definition
        uint8_t q = cost[f] == none ? 255 : 40;
        if (cost[f] != none && !seeded[f]) {
            const long k = (long)(f % nz), j = (long)((f / nz) % ny), i = (long)(f / ((size_t)nz * ny));
            bool found = false;
            for (int code = 0; code <= 80 && !found; ++code) {
                const int oi = code / 27 - 1, oj = (code / 9) % 3 - 1, ok_ = code % 9 - 4;   // o = u - v
                if (!move_allowed(p, -oi, -oj, -ok_) || !s.is(i + oi, j + oj, k + ok_)) continue;
                const size_t u = s.flat((uint32_t)(i + oi), (uint32_t)(j + oj), (uint32_t)(k + ok_));
                if (cost[u] != none && cost[u] + move_cost(p, -oi, -oj, -ok_) == cost[f]) {
                    q = (uint8_t)code;
                    found = true;
                }
            }
            ok = ok && found;
        }
        ok = ok && got_parent[f] == q;
    }
    for (size_t f = 0; f < s.n + 2; ++f) ok = ok && om[f] == (list[f] < s.n ? got_cost[list[f]] : dr::kNone);
    for (size_t t = 0; t < targets.size(); ++t) {
        const long long m = snap_of(s, p.snap, targets[t]);
        ok = ok && got_ti[t] == (m < 0 ? dr::kNone : (uint32_t)m) && got_tc[t] == (m < 0 ? dr::kNone : got_cost[(size_t)m]);
    }
    ok = ok && c.n_members == n_members && c.n_seeded == n_seeded && c.n_reached == n_reached && c.max_cost == most;
    // every optional output left out: the counts are the same
    const dr::Counts c2 = dr::cells(s.dims, s.member.get(), sd.get(), (uint32_t)seeds.size(), nullptr, 0, nullptr, 0, p, nullptr, nullptr, nullptr, nullptr, nullptr);
    ok = ok && c2.n_reached == c.n_reached && c2.max_cost == c.max_cost && c2.n_seeded == c.n_seeded;
    expect(ok, what + ": members " + std::to_string(n_members) + " seeded " + std::to_string(n_seeded) + " reached " + std::to_string(n_reached) +
                   " max_cost " + std::to_string(most));
    if (counts) *counts = c;
    if (cost_out) cost_out->assign(got_cost.get(), got_cost.get() + s.n);
    return ok;
}

static dr::Params params(uint32_t conn, uint32_t step, uint32_t snap = 0, uint32_t m0 = 10, uint32_t m1 = 14, uint32_t up = 0, uint32_t down = 0,
                         uint32_t max_cost = 1u << 31) {
    return dr::Params{conn, step, snap, {m0, m1}, up, down, max_cost};
}

int main() {
    // the flat floor: 17 x 17 x 9, k = 3
    {
        Set s(17, 17, 9);
        for (uint32_t i = 0; i < 17; ++i)
            for (uint32_t j = 0; j < 17; ++j) s.add(i, j, 3);
        for (const uint32_t conn : {4u, 8u}) {
            std::vector<uint32_t> cost;
            check(s, {s.flat(8, 8, 3)}, {s.flat(16, 0, 3), s.flat(0, 0, 4), (uint32_t)s.n}, params(conn, 0), "flat floor, connectivity " + std::to_string(conn), nullptr, &cost);
            expect(cost[s.flat(16, 0, 3)] == (conn == 4 ? 160u : 112u) && cost[s.flat(8, 0, 3)] == 80u, "  octile / Manhattan distance");
        }
        check(s, {s.flat(8, 8, 5)}, {s.flat(8, 8, 8)}, params(8, 0, 2), "flat floor, a seed two above it with snap 2");
        check(s, {s.flat(8, 8, 6)}, {s.flat(8, 8, 8)}, params(8, 0, 2), "flat floor, a seed three above it with snap 2");
        check(s, {s.flat(8, 8, 3)}, {}, params(8, 0, 0, 10, 14, 0, 0, 27), "flat floor, max_cost 27");
        check(s, {}, {s.flat(1, 1, 3)}, params(8, 1), "flat floor, no seed");
    }
    // stairs that rise 1 .. 5 a column: climbed iff rise <= step; up != down; both ways
    for (uint32_t rise = 1; rise <= 5; ++rise) {
        Set s(5, 3, 4 * rise + 1);
        for (uint32_t i = 0; i < 5; ++i) s.add(i, 1, i * rise);
        for (uint32_t step = 0; step <= 4; ++step) {
            dr::Counts c;
            std::vector<uint32_t> cost;
            check(s, {s.flat(0, 1, 0)}, {s.flat(4, 1, 4 * rise)}, params(4, step, 0, 10, 14, 7, 3), "stairs up, rise " + std::to_string(rise) + " step " + std::to_string(step), &c, &cost);
            expect(cost[s.flat(4, 1, 4 * rise)] == (rise <= step ? 4 * (10 + 7 * rise) : dr::kNone), "  reached iff rise <= step, at climb_up a voxel");
            check(s, {s.flat(4, 1, 4 * rise)}, {s.flat(0, 1, 0)}, params(8, step, 0, 10, 14, 7, 3), "stairs down, rise " + std::to_string(rise) + " step " + std::to_string(step), &c, &cost);
            expect(cost[s.flat(0, 1, 0)] == (rise <= step ? 4 * (10 + 3 * rise) : dr::kNone), "  reached iff rise <= step, at climb_down a voxel");
        }
    }
    // the brick-border links
    {
        const uint32_t links[6][8] = {{3, 3, 7, 4, 3, 9, 2, 4}, {3, 3, 8, 4, 3, 4, 4, 4}, {7, 7, 7, 8, 8, 11, 4, 8}, {7, 3, 0, 8, 3, 0, 0, 4}, {0, 8, 3, 1, 7, 7, 4, 8}, {7, 7, 7, 8, 7, 7, 1, 4}};
        for (const auto &l : links) {
            Set s(17, 17, 16);
            s.add(l[0], l[1], l[2]);
            s.add(l[3], l[4], l[5]);
            dr::Counts c;
            check(s, {s.flat(l[0], l[1], l[2])}, {s.flat(l[3], l[4], l[5])}, params(l[7], l[6], 0, 10, 14, 2, 1), "link forwards", &c);
            expect(c.n_reached == 2, "  joined");
            check(s, {s.flat(l[3], l[4], l[5])}, {s.flat(l[0], l[1], l[2])}, params(l[7], l[6], 0, 10, 14, 2, 1), "link backwards", &c);
            expect(c.n_reached == 2, "  joined");
        }
    }
    // floor and shelf in one column
    for (const bool ramp : {false, true}) {
        Set s(9, 9, 8);
        for (uint32_t i = 0; i < 9; ++i)
            for (uint32_t j = 0; j < 9; ++j) {
                s.add(i, j, 2);
                if (i >= 4) s.add(i, j, 6);
            }
        if (ramp) s.add(3, 0, 4);
        dr::Counts c;
        check(s, {s.flat(0, 4, 2)}, {s.flat(6, 4, 6), s.flat(6, 4, 7)}, params(8, 2, 5, 10, 14, 3, 0), ramp ? "floor and shelf with the ramp" : "floor and shelf", &c);
        expect(c.n_reached == (ramp ? 81u + 45u + 1u : 81u), ramp ? "  joined by the ramp" : "  not joined");
    }
    // the serpentine in one brick
    {
        Set s(8, 8, 8);
        for (uint32_t i = 0; i < 8; ++i)
            for (uint32_t j = 0; j < 8; j += 2) s.add(i, j, 0);
        s.add(7, 1, 0);
        s.add(0, 3, 0);
        s.add(7, 5, 0);
        std::vector<uint32_t> cost;
        check(s, {s.flat(0, 0, 0)}, {s.flat(0, 6, 0)}, params(4, 0, 0, 3, 5), "serpentine", nullptr, &cost);
        expect(cost[s.flat(0, 6, 0)] == 3u * 34u, "  34 moves");
    }
    // random member sets
    std::mt19937 rng(12345);
    for (int round = 0; round < 6; ++round) {
        Set s(11 + (uint32_t)round, 9, 13);
        for (size_t f = 0; f < s.n; ++f) s.member[f] = rng() % 100 < (round % 2 ? 55u : 30u);
        std::vector<uint32_t> seeds, targets;
        for (int t = 0; t < 4; ++t) seeds.push_back((uint32_t)(rng() % (s.n + 3)));
        for (int t = 0; t < 40; ++t) targets.push_back((uint32_t)(rng() % (s.n + 3)));
        for (const uint32_t conn : {4u, 8u})
            for (uint32_t step = 0; step <= 4; ++step)
                check(s, seeds, targets, params(conn, step, (uint32_t)round, 10, 14, 6, 1),
                      "random " + std::to_string(round) + " connectivity " + std::to_string(conn) + " step " + std::to_string(step));
    }
    // the limit values
    {
        Set s(9, 8, 40);
        for (size_t f = 0; f < s.n; ++f) s.member[f] = rng() % 100 < 50u;
        check(s, {s.flat(4, 4, 39), 0u}, {s.flat(8, 7, 39), s.flat(0, 0, 32)}, params(8, 4, 32, 1u << 16, 1u << 16, 1u << 16, 1u << 16, 1u << 31), "every limit value");
        check(s, {s.flat(4, 4, 39), 0u}, {s.flat(8, 7, 39)}, params(8, 4, 32, 1, 1, 0, 0, 1), "max_cost 1");
        Set one(1, 1, 1);
        check(one, {0u}, {0u, 1u}, params(8, 4, 32), "one voxel, no member");
        one.add(0, 0, 0);
        check(one, {0u, 0u}, {0u, 1u}, params(4, 0, 0), "one voxel, a member seeded twice");
        Set row(1, 64, 1);
        for (uint32_t j = 0; j < 64; ++j) row.add(0, j, 0);
        check(row, {row.flat(0, 63, 0)}, {0u}, params(4, 4, 32), "one row");
    }
    std::printf("%s\n", g_fail ? "FAILED" : "all cases hold");
    return g_fail ? 1 : 0;
}
