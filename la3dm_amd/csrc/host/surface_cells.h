// surface_cells.h — the pure part of surface (contract: include/la3dm_hip.h, la3dm_devmap_surface_host): the classes of
// the padded box go in; the surface voxels, their ordered list with face masks and normals, the dense face masks and the
// counts come out.  The host form (BGKOctoMap::surface, host/bgkoctomap.cpp) reads the classes and calls `cells`: that is
// the definition, and the device kernels (csrc/devmap_surface.h) reproduce it exactly.  std only; compiles alone
// (tools/check/surface_cells.cpp drives it under ASan and UBSan).
//
// The padded box (PX, PY, PZ) = (nx + 2p, ny + 2p, nz + 2p), p = smooth + 1, starts p voxels before the region on every
// axis: region voxel (i, j, k) is padded voxel (i + p, j + p, k + p), index (pi PY + pj) PZ + pz.  The face mask of a padded
// voxel needs its six neighbours: it is formed for the padded voxels one layer inside the box, which are all the normal's
// window reaches (|u - v|_inf <= smooth = p - 1).  The window sum is separable: along z, then y, then x.
#ifndef LA3DM_SURFACE_CELLS_H
#define LA3DM_SURFACE_CELLS_H

#include <cstddef>
#include <cstdint>
#include <vector>

namespace la3dm_surface {

struct Params {   // la3dm_surface_params, field by field
    uint32_t solid_mask, open_mask, smooth;
};

struct Counts {
    uint64_t n_solid, n_surface, faces[6];
};

// the padded extents of a region of dims
inline void padded_dims(const uint32_t dims[3], const Params &p, size_t P[3]) {
    for (int a = 0; a < 3; ++a) P[a] = (size_t)dims[a] + 2u * (p.smooth + 1u);
}

// one pass of the window sum along the axis of stride `step`: out[u] = the sum of in[u + t step], |t| <= s, for the padded
// voxels of [lo, hi) per axis
inline void window_pass(const std::vector<int16_t> &in, std::vector<int16_t> &out, const size_t P[3], const size_t lo[3],
                        const size_t hi[3], ptrdiff_t step, ptrdiff_t s) {
#pragma omp parallel for schedule(static)
    for (size_t pi = lo[0]; pi < hi[0]; ++pi)
        for (size_t pj = lo[1]; pj < hi[1]; ++pj)
            for (size_t pz = lo[2]; pz < hi[2]; ++pz) {
                const ptrdiff_t u = (ptrdiff_t)((pi * P[1] + pj) * P[2] + pz);
                int sum = 0;
                for (ptrdiff_t t = -s; t <= s; ++t) sum += in[(size_t)(u + t * step)];
                out[(size_t)u] = (int16_t)sum;   // at most (2 s + 1)^3 = 729 in size
            }
}

// pcls[PX PY PZ]: the classes of the padded box.  index[cap], faces[cap], normal[3 cap], dense_faces[nx ny nz]: each may
// be null.  The arguments have passed the contract's checks (smooth <= 4).
inline Counts cells(const uint8_t *pcls, const uint32_t dims[3], const Params &p, uint64_t cap, uint32_t *index, uint8_t *faces,
                    int16_t *normal, uint8_t *dense_faces) {
    const size_t nx = dims[0], ny = dims[1], nz = dims[2], pad = (size_t)p.smooth + 1;
    size_t P[3];
    padded_dims(dims, p, P);
    const size_t PY = P[1], PZ = P[2], total = P[0] * PY * PZ;
    const ptrdiff_t step[3] = {(ptrdiff_t)(PY * PZ), (ptrdiff_t)PZ, 1};
    // the face masks of the padded voxels that have all six neighbours in the box
    std::vector<uint8_t> fb(total, 0);
#pragma omp parallel for schedule(static)
    for (size_t pi = 1; pi < P[0] - 1; ++pi)
        for (size_t pj = 1; pj + 1 < PY; ++pj)
            for (size_t pz = 1; pz + 1 < PZ; ++pz) {
                const ptrdiff_t u = (ptrdiff_t)((pi * PY + pj) * PZ + pz);
                if (!((p.solid_mask >> pcls[u]) & 1u)) continue;
                uint8_t f = 0;
                for (int d = 0; d < 6; ++d) {
                    const ptrdiff_t v = u + ((d & 1) ? step[d >> 1] : -step[d >> 1]);
                    f |= (uint8_t)(((p.open_mask >> pcls[v]) & 1u) << d);
                }
                fb[(size_t)u] = f;
            }
    // the window sums, one component at a time: z, y, x, each pass over no more voxels than the next one reads
    std::vector<int16_t> sum[3];
    const bool want_normal = normal != nullptr && index != nullptr && cap > 0;
    if (want_normal && p.smooth > 0) {
        const ptrdiff_t s = (ptrdiff_t)p.smooth;
        std::vector<int16_t> a(total), b(total);
        for (int c = 0; c < 3; ++c) {
#pragma omp parallel for schedule(static)
            for (size_t u = 0; u < total; ++u) a[u] = (int16_t)((int)((fb[u] >> (2 * c + 1)) & 1) - (int)((fb[u] >> (2 * c)) & 1));
            const size_t lo_z[3] = {1, 1, pad}, hi_z[3] = {P[0] - 1, PY - 1, pad + nz};
            window_pass(a, b, P, lo_z, hi_z, step[2], s);
            const size_t lo_y[3] = {1, pad, pad}, hi_y[3] = {P[0] - 1, pad + ny, pad + nz};
            window_pass(b, a, P, lo_y, hi_y, step[1], s);
            const size_t lo_x[3] = {pad, pad, pad}, hi_x[3] = {pad + nx, pad + ny, pad + nz};
            sum[c].assign(total, 0);
            window_pass(a, sum[c], P, lo_x, hi_x, step[0], s);
        }
    }
    // the region in flat order: counts per column, their prefixes, then the list
    const size_t n_col = nx * ny;
    std::vector<uint64_t> col_start(n_col + 1, 0), col_solid(n_col, 0);
    std::vector<uint64_t> col_faces(6 * n_col, 0);
#pragma omp parallel for schedule(static)
    for (size_t col = 0; col < n_col; ++col) {
        const size_t base = ((col / ny + pad) * PY + (col % ny + pad)) * PZ + pad;
        uint64_t found = 0;
        for (size_t k = 0; k < nz; ++k) {
            const uint8_t f = fb[base + k];
            col_solid[col] += (p.solid_mask >> pcls[base + k]) & 1u;
            for (int d = 0; d < 6; ++d) col_faces[6 * col + (size_t)d] += (f >> d) & 1u;
            found += f != 0;
            if (dense_faces) dense_faces[col * nz + k] = f;
        }
        col_start[col + 1] = found;
    }
    Counts n = {0, 0, {0, 0, 0, 0, 0, 0}};
    for (size_t col = 0; col < n_col; ++col) {
        n.n_solid += col_solid[col];
        for (size_t d = 0; d < 6; ++d) n.faces[d] += col_faces[6 * col + d];
        col_start[col + 1] += col_start[col];
    }
    n.n_surface = col_start[n_col];
    if (cap > 0 && (index != nullptr || faces != nullptr)) {
#pragma omp parallel for schedule(static)
        for (size_t col = 0; col < n_col; ++col) {
            const size_t base = ((col / ny + pad) * PY + (col % ny + pad)) * PZ + pad;
            uint64_t t = col_start[col];
            for (size_t k = 0; k < nz && t < cap; ++k) {
                const uint8_t f = fb[base + k];
                if (f == 0) continue;
                if (index) index[t] = (uint32_t)(col * nz + k);
                if (faces) faces[t] = f;
                if (want_normal)
                    for (int c = 0; c < 3; ++c)
                        normal[3 * t + (uint64_t)c] = p.smooth > 0 ? sum[c][base + k] : (int16_t)((int)((f >> (2 * c + 1)) & 1) - (int)((f >> (2 * c)) & 1));
                ++t;
            }
        }
    }
    return n;
}

}  // namespace la3dm_surface

#endif
