// paths_walk.cpp — the integer walk of score_paths (la3dm_amd/csrc/host/region_contract.h: path_waypoint, path_segment,
// path_sample, path_move, path_inside, path_blocked, path_entry) at the ends of its range, as a stand-alone CPU program meant
// to be built with a sanitizer:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/check/paths_walk.cpp \
//       -o tools/check/paths_walk && tools/check/paths_walk
//
// Signed overflow in the walk arithmetic is what it is there to exclude; every array lives on the heap at its exact size,
// so a read past one is a report as well.  The cases: the range test at its edge; waypoints with |w / resolution| just
// under 2^30 at block_depth 1 .. 6 and three resolutions, their G inside the range path_waypoint states; the floor
// division against a floating-point floor on every small segment; on 20 000 random segments the three properties of the
// contract (a 26-connected walk, the last voxel is the waypoint's, the reversed segment gives the reversed walk); segments
// between opposite corners of the lattice sampled over the first and last 2^20 + 1 steps a call may take; and a path of
// 1024 waypoints that alternates between the corners, walked as the host form walks it for 2^20 steps against a small
// region.  Prints one line per case and exits 0 when all hold.
#include <cmath>
#include <cstdio>
#include <memory>
#include <random>

#include "../../la3dm_amd/csrc/host/region_contract.h"

namespace R = la3dm_region;

static int g_fail = 0;
static void expect(bool ok, const char *what) {
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++g_fail;
}

static void range_edge() {
    bool ok = true;
    for (float res : {0.05f, 0.1f, 1.0f}) {
        const float edge = 1073741824.0f * res, under = std::nextafter(edge, 0.0f);
        ok = ok && R::axis_in_range(under, res) && R::axis_in_range(-under, res) && R::axis_in_range(0.0f, res);
        ok = ok && !R::axis_in_range(std::nextafter(edge, 2 * edge), res) && !R::axis_in_range(NAN, res) && !R::axis_in_range(INFINITY, res) &&
             !R::axis_in_range(-INFINITY, res);
    }
    expect(ok, "range test: just under 2^30 passes; above it, NaN and inf fail");
}

// the largest coordinate that passes the range test
static float widest(float res) {
    float w = 1073741824.0f * res;
    while (!R::axis_in_range(w, res)) w = std::nextafter(w, 0.0f);
    return w;
}

static void extreme_waypoints() {
    bool ok = true;
    long long lowest = 0, highest = 0;
    for (int depth = 1; depth <= 6; ++depth)
        for (float res : {0.05f, 0.1f, 1.0f}) {
            const int lim = 1 << (depth - 1);
            const float bs = (float)lim * res, w = widest(res);
            for (int corner = 0; corner < 8; ++corner) {
                const float p[3] = {corner & 1 ? w : -w, corner & 2 ? w : -w, corner & 4 ? w : -w};
                long long G[3];
                ok = ok && R::path_waypoint(p, res, bs, lim, G);
                for (int c = 0; c < 3; ++c) {
                    ok = ok && G[c] > -(1ll << 30) && G[c] < (1ll << 30) + (1ll << 25);
                    lowest = std::min(lowest, G[c]);
                    highest = std::max(highest, G[c]);
                }
            }
            const float bad[3] = {0.0f, std::nextafter(1073741824.0f * res, INFINITY), 0.0f};
            long long G[3] = {7, 7, 7};
            ok = ok && !R::path_waypoint(bad, res, bs, lim, G) && G[0] == 7;
        }
    std::printf("     G over the corners: %lld ... %lld\n", lowest, highest);
    expect(ok, "waypoints with |w / resolution| just under 2^30, block_depth 1 .. 6: every G in (-2^30, 2^30 + 2^25)");
}

static void floor_division() {
    bool ok = true;
    for (long long n = 1; n <= 12; ++n)
        for (long long d = -n; d <= n; ++d)
            for (long long s = 0; s <= n; ++s)
                ok = ok && R::path_sample(100, d, n, s) == 100 + (long long)std::floor((2.0 * s * d + n) / (2.0 * n));
    expect(ok, "path_sample is a floor division for every |d| <= n <= 12");
}

// the walk of one segment into a heap array of exactly n + 1 voxels
static std::unique_ptr<long long[]> segment_walk(const long long *A, const long long *B, long long n) {
    std::unique_ptr<long long[]> v(new long long[3 * (size_t)(n + 1)]);
    for (int c = 0; c < 3; ++c) v[c] = A[c];
    for (long long s = 1; s <= n; ++s)
        for (int c = 0; c < 3; ++c) v[3 * s + c] = R::path_sample(A[c], B[c] - A[c], n, s);
    return v;
}

static void random_segments() {
    std::mt19937_64 rng(20000);
    bool connected = true, ends = true, reversed = true;
    for (int i = 0; i < 20000; ++i) {
        const long long span = i % 3 == 0 ? 6 : (i % 3 == 1 ? 300 : 5000);
        std::uniform_int_distribution<long long> at(-(1ll << 30) + 1, (1ll << 30)), by(-span, span);
        long long A[3], B[3];
        for (int c = 0; c < 3; ++c) {
            A[c] = at(rng);
            B[c] = A[c] + by(rng);
        }
        const long long n = R::path_segment(A, B);
        if (n == 0) continue;
        const auto f = segment_walk(A, B, n), b = segment_walk(B, A, n);
        for (long long s = 1; s <= n; ++s) {
            const uint32_t nz = R::path_move(&f[3 * (s - 1)], &f[3 * s]);
            connected = connected && nz >= 1 && nz <= 3;
            for (int c = 0; c < 3; ++c) connected = connected && std::llabs(f[3 * s + c] - f[3 * (s - 1) + c]) <= 1;
        }
        for (int c = 0; c < 3; ++c) ends = ends && f[3 * n + c] == B[c] && f[c] == A[c];
        for (long long s = 0; s <= n; ++s)
            for (int c = 0; c < 3; ++c) reversed = reversed && f[3 * s + c] == b[3 * (n - s) + c];
    }
    expect(connected, "20 000 random segments: consecutive voxels differ by at most 1 per axis and in 1 .. 3 axes");
    expect(ends, "20 000 random segments: the walk starts at one waypoint's voxel and ends at the other's");
    expect(reversed, "20 000 random segments: the reversed segment gives the reversed walk");
}

static void opposite_corners() {
    bool ok = true;
    const long long kMost = (1ll << 20) + 1;   // the most steps a call takes in one segment
    for (int depth : {1, 3, 6})
        for (float res : {0.05f, 0.1f}) {
            const int lim = 1 << (depth - 1);
            const float bs = (float)lim * res, w = widest(res);
            for (int corner = 0; corner < 8; ++corner) {
                const float p[3] = {corner & 1 ? w : -w, corner & 2 ? w : -w, corner & 4 ? w : -w}, q[3] = {-p[0], -p[1], w};
                long long A[3], B[3];
                ok = ok && R::path_waypoint(p, res, bs, lim, A) && R::path_waypoint(q, res, bs, lim, B);
                const long long n = R::path_segment(A, B);
                ok = ok && n > (1ll << 30) && n < (1ll << 33);
                long long prev[3] = {A[0], A[1], A[2]};
                for (long long s = 1; s <= kMost; s += (s < 4096 || s > kMost - 4096) ? 1 : 997) {
                    long long v[3];
                    for (int c = 0; c < 3; ++c) v[c] = R::path_sample(A[c], B[c] - A[c], n, s);
                    for (int c = 0; c < 3; ++c) ok = ok && std::llabs(v[c] - A[c]) <= s;
                    if (s <= 4096) {
                        const uint32_t nz = R::path_move(prev, v);
                        ok = ok && nz >= 1 && nz <= 3;
                        for (int c = 0; c < 3; ++c) prev[c] = v[c];
                    }
                }
            }
        }
    expect(ok, "opposite corners of the lattice: 2^30 < n < 2^33, the first 2^20 + 1 steps sampled without overflow");
}

static void long_path() {
    const uint32_t n_way = LA3DM_PATHS_MAX_WAY, max_steps = LA3DM_PATHS_MAX_STEPS;
    const float res = 0.1f;
    const int lim = 4;
    const float bs = (float)lim * res, w = widest(res);
    std::unique_ptr<float[]> ways(new float[3 * (size_t)n_way]);
    for (uint32_t k = 0; k < n_way; ++k) {   // the first two waypoints inside the region, the rest from corner to corner
        const float far = (k & 1) ? w : -w;
        ways[3 * k] = k < 2 ? 0.05f + 0.3f * (float)k : far;
        ways[3 * k + 1] = k < 2 ? 0.05f : -far;
        ways[3 * k + 2] = k < 2 ? 0.05f : far;
    }
    std::unique_ptr<long long[]> G(new long long[3 * (size_t)n_way]);
    bool ok = true;
    for (uint32_t k = 0; k < n_way; ++k) ok = ok && R::path_waypoint(&ways[3 * k], res, bs, lim, &G[3 * k]);
    unsigned long long T = 0;
    for (uint32_t k = 1; k < n_way; ++k) T += (unsigned long long)R::path_segment(&G[3 * (k - 1)], &G[3 * k]);
    ok = ok && T > (1ull << 40) && T < (1ull << 42);   // 1021 segments of about 2^31 voxels
    // a region of 4 x 3 x 2 voxels anchored at the first waypoint's voxel, no obstacle in it
    const uint32_t g0[3] = {(uint32_t)G[0], (uint32_t)G[1], (uint32_t)G[2]}, dims[3] = {4, 3, 2};
    std::unique_ptr<uint32_t[]> d2(new uint32_t[24]);
    for (int f = 0; f < 24; ++f) d2[f] = LA3DM_DF_FAR;
    la3dm_paths_params p = {1u << 1, 0, 3, 9, {10, 14, 17}, max_steps};
    unsigned long long cost = 0, visited = 0, left_at = 0;
    long long last[3] = {G[0], G[1], G[2]};
    unsigned long long o = 0;
    for (uint32_t k = 1; k < n_way && o < max_steps; ++k) {
        const long long *A = &G[3 * (k - 1)], *B = &G[3 * k];
        const long long n = R::path_segment(A, B);
        for (long long s = 1; s <= n && o < max_steps; ++s) {
            ++o;
            long long v[3];
            for (int c = 0; c < 3; ++c) v[c] = R::path_sample(A[c], B[c] - A[c], n, s);
            uint32_t f = 0;
            if (R::path_inside(v, g0, dims, f)) {
                ok = ok && f < 24 && !R::path_blocked(p.clearance, d2[f]);
                cost += R::path_entry(p, R::path_move(last, v), d2[f]);
                ++visited;
            } else if (left_at == 0) {
                left_at = o;
            }
            for (int c = 0; c < 3; ++c) last[c] = v[c];
        }
    }
    std::printf("     T = %llu, walked %llu steps, %llu inside the region (cost %llu), left it at ordinal %llu\n", T, o, visited, cost, left_at);
    expect(ok && o == max_steps && visited == 3 && cost == 30 && left_at == 4, "1024 waypoints from corner to corner: 2^20 steps walked, the offsets fit 64 bits");
}

int main() {
    range_edge();
    extreme_waypoints();
    floor_division();
    random_segments();
    opposite_corners();
    long_path();
    std::printf(g_fail ? "%d case(s) FAILED\n" : "all cases hold\n", g_fail);
    return g_fail ? 1 : 0;
}
