// nearest_lines.cpp — the line passes of nearest (la3dm_amd/csrc/host/nearest_lines.h: line_z, line_pass, the packed key)
// against the definition, as a stand-alone CPU program meant to be built with a sanitizer:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/check/nearest_lines.cpp \
//       -o tools/check/nearest_lines && tools/check/nearest_lines
//
// Every array lives on the heap at its exact size, so an offset that leaves its line is a report.  The cases: the key
// arithmetic at its ends (sum 2^18 - 1, offsets -255 and 255); line_z on lines of length 1, lines shorter than the radius
// and at radius 255, against a scan of the line; the three passes composed as the host form composes them (z, y, x and the
// chase) on boxes with an axis of length 1, axes shorter than the radius and radius 255, against a brute force that takes
// the FIRST minimum over the obstacles in ascending flat index — every index and d2 equal, tied voxels counted.  Prints one
// line per case and exits 0 when all hold.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

#include "../../la3dm_amd/csrc/host/nearest_lines.h"

namespace nt = la3dm_nearest;

constexpr uint32_t kNone = 0xFFFFFFFFu;

static int g_fail = 0;
static void expect(bool ok, const char *what) {
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++g_fail;
}

static void key_ends() {
    bool ok = true;
    for (uint32_t sum : {0u, 1u, 65025u, 65536u, (1u << 18) - 1u})
        for (int off : {-255, -1, 0, 1, 255})
            ok = ok && nt::key_sum(nt::key_of(sum, off)) == sum && nt::key_offset(nt::key_of(sum, off)) == off;
    ok = ok && nt::key_of(5, -3) < nt::key_of(5, 2) && nt::key_of(4, 200) < nt::key_of(5, -200);
    ok = ok && nt::offset_term(256) == 65536u && nt::offset_term(-255) == 65025u;
    expect(ok, "keys: sum and offset come back at the ends of their ranges; the smaller sum, then the smaller offset, is the smaller key");
}

static void z_lines() {
    std::mt19937 rng(7);
    bool ok = true;
    size_t lines = 0;
    for (size_t n : {1u, 2u, 3u, 31u, 64u, 300u})
        for (uint32_t radius : {1u, 2u, 40u, 255u})
            for (double density : {0.0, 0.03, 0.3, 1.0})
                for (int rep = 0; rep < 8; ++rep, ++lines) {
                    std::unique_ptr<uint8_t[]> obs(new uint8_t[n]);
                    std::unique_ptr<int16_t[]> off(new int16_t[n]);
                    for (size_t k = 0; k < n; ++k) obs[k] = std::uniform_real_distribution<double>(0, 1)(rng) < density;
                    nt::line_z(obs.get(), n, radius, off.get());
                    for (size_t k = 0; k < n; ++k) {
                        int want = (int)radius + 1;
                        for (size_t q = 0; q < n; ++q) {   // ascending k': the first of equals stays
                            const int d = (int)q - (int)k;
                            if (obs[q] && std::abs(d) <= (int)radius && std::abs(d) < std::abs(want)) want = d;
                        }
                        ok = ok && off[k] == want;
                    }
                }
    std::printf("     %zu lines\n", lines);
    expect(ok, "line_z: lengths 1 .. 300, radii 1 .. 255: the nearest obstacle within the radius, the lower one on a tie, radius + 1 where none");
}

// the host form's composition of the passes on a box of nx x ny x nz flags
static void transform(const uint8_t *obs, size_t nx, size_t ny, size_t nz, uint32_t radius, uint32_t *index, uint32_t *d2) {
    const size_t n = nx * ny * nz, S = ny * nz;
    std::unique_ptr<int16_t[]> az(new int16_t[n]);
    std::unique_ptr<uint32_t[]> ky(new uint32_t[n]);
    for (size_t line = 0; line < nx * ny; ++line) nt::line_z(obs + line * nz, nz, radius, az.get() + line * nz);
    for (size_t i = 0; i < nx; ++i)
        for (size_t k = 0; k < nz; ++k)
            nt::line_pass(
                ny, radius, [&](size_t j) { return nt::offset_term(az[(i * ny + j) * nz + k]); },
                [&](size_t j, uint32_t key) { ky[(i * ny + j) * nz + k] = key; });
    for (size_t c = 0; c < S; ++c)
        nt::line_pass(
            nx, radius, [&](size_t i) { return nt::key_sum(ky[i * S + c]); },
            [&](size_t i, uint32_t key) {
                const uint32_t sum = nt::key_sum(key);
                if (sum > radius * radius) {
                    index[i * S + c] = d2[i * S + c] = kNone;
                    return;
                }
                const size_t j = c / nz, k = c % nz;
                const size_t i2 = (size_t)((ptrdiff_t)i + nt::key_offset(key));
                const size_t j2 = (size_t)((ptrdiff_t)j + nt::key_offset(ky[i2 * S + c]));
                const size_t k2 = (size_t)((ptrdiff_t)k + az[(i2 * ny + j2) * nz + k]);
                index[i * S + c] = (uint32_t)((i2 * ny + j2) * nz + k2);
                d2[i * S + c] = sum;
            });
}

static void boxes() {
    std::mt19937 rng(11);
    const size_t shapes[][3] = {{1, 1, 1}, {1, 1, 9}, {6, 1, 1}, {1, 7, 1}, {2, 7, 1}, {3, 5, 7}, {7, 6, 5}, {9, 9, 3}, {4, 1, 6}, {12, 11, 10}};
    bool ok = true;
    size_t tied = 0, none = 0, voxels = 0;
    for (const auto &s : shapes)
        for (uint32_t radius : {1u, 2u, 3u, 255u})
            for (double density : {0.0, 0.03, 0.15, 0.6}) {
                const size_t nx = s[0], ny = s[1], nz = s[2], n = nx * ny * nz;
                std::unique_ptr<uint8_t[]> obs(new uint8_t[n]);
                std::unique_ptr<uint32_t[]> index(new uint32_t[n]), d2(new uint32_t[n]);
                for (size_t f = 0; f < n; ++f) obs[f] = std::uniform_real_distribution<double>(0, 1)(rng) < density;
                transform(obs.get(), nx, ny, nz, radius, index.get(), d2.get());
                for (size_t f = 0; f < n; ++f, ++voxels) {
                    const long i = (long)(f / (ny * nz)), j = (long)(f / nz % ny), k = (long)(f % nz);
                    uint32_t best = kNone, at = kNone, ties = 0;
                    for (size_t o = 0; o < n; ++o) {
                        if (!obs[o]) continue;
                        const long di = (long)(o / (ny * nz)) - i, dj = (long)(o / nz % ny) - j, dk = (long)(o % nz) - k;
                        const uint32_t d = (uint32_t)(di * di + dj * dj + dk * dk);
                        if (d < best) {
                            best = d;
                            at = (uint32_t)o;
                            ties = 1;
                        } else if (d == best) {
                            ++ties;
                        }
                    }
                    if (best > radius * radius) best = at = kNone;
                    tied += at != kNone && ties > 1;
                    none += at == kNone;
                    ok = ok && index[f] == at && d2[f] == best;
                }
            }
    std::printf("     %zu voxels, %zu with more than one nearest obstacle, %zu with none within the radius\n", voxels, tied, none);
    expect(ok && tied > 100 && none > 100, "boxes with axes of length 1 and shorter than the radius, radii 1, 2, 3, 255: index and d2 equal the brute force");
}

int main() {
    key_ends();
    z_lines();
    boxes();
    std::printf(g_fail ? "%d case(s) FAILED\n" : "all cases hold\n", g_fail);
    return g_fail ? 1 : 0;
}
