// footing_cells.h — the pure part of footing (contract: include/la3dm_hip.h, la3dm_devmap_footing_host): the classes of
// the padded box go in; the foot voxels, their ordered list and the column arrays come out.  The host form
// (BGKOctoMap::footing, host/bgkoctomap.cpp) reads the classes and calls `cells`: that is the definition, and the device
// kernels (csrc/devmap_footing.h) reproduce it exactly.  std only; compiles alone (tools/check/footing_cells.cpp drives it
// under ASan and UBSan).
//
// The padded box (PX, PY, PZ) = (nx + 2r, ny + 2r, nz + h + 2s) starts r voxels before the region in x and y and 1 + s
// below it: region voxel (i, j, k) is padded voxel (i + r, j + r, k + 1 + s), index (pi PY + pj) PZ + pz.  Per padded column,
// up[z] = the number of voxels from z upwards, at most h, whose class is in clear_mask; then
//   stand(z) = support(z - 1) and up[z] >= h          for z in [1, PZ - h], the only z at which it is asked for,
//   near(z)  = stand(z + dk) for some |dk| <= s       for z in [1 + s, nz + s], the region's own z,
//   body(z)  = up[z + s] >= h - s                     for the same z.
#ifndef LA3DM_FOOTING_CELLS_H
#define LA3DM_FOOTING_CELLS_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace la3dm_footing {

struct Params {   // la3dm_footing_params, field by field
    uint32_t support_mask, clear_mask, headroom, radius, step, min_support;
};

struct Counts {
    uint64_t n_stand, n_body, n_foot;
};

// N: the cells of the footprint without its centre
constexpr inline uint32_t disc_cells(uint32_t r) {
    uint32_t n = 0;
    for (int di = -(int)r; di <= (int)r; ++di)
        for (int dj = -(int)r; dj <= (int)r; ++dj) n += (di || dj) && (uint32_t)(di * di + dj * dj) <= r * r ? 1u : 0u;
    return n;
}

// the padded extents of a region of dims
inline void padded_dims(const uint32_t dims[3], const Params &p, size_t P[3]) {
    P[0] = (size_t)dims[0] + 2u * p.radius;
    P[1] = (size_t)dims[1] + 2u * p.radius;
    P[2] = (size_t)dims[2] + p.headroom + 2u * p.step;
}

// pcls[PX PY PZ]: the classes of the padded box.  foot[nx ny nz] (0 / 1), index[cap], levels / lowest / highest[nx ny]:
// each may be null.  The arguments have passed the contract's checks (1 <= h, s < h, c <= N).
inline Counts cells(const uint8_t *pcls, const uint32_t dims[3], const Params &p, uint8_t *foot, uint64_t cap, uint32_t *index,
                    uint32_t *levels, int32_t *lowest, int32_t *highest) {
    const size_t nx = dims[0], ny = dims[1], nz = dims[2];
    const size_t h = p.headroom, r = p.radius, s = p.step;
    size_t P[3];
    padded_dims(dims, p, P);
    const size_t PY = P[1], PZ = P[2], n_pcol = P[0] * PY;
    std::vector<uint8_t> stand(n_pcol * PZ, 0), near(n_pcol * PZ, 0), body(n_pcol * PZ, 0);
#pragma omp parallel
    {
        std::vector<uint32_t> up(PZ + 1);
#pragma omp for schedule(static)
        for (size_t col = 0; col < n_pcol; ++col) {
            const uint8_t *c = pcls + col * PZ;
            uint8_t *st = stand.data() + col * PZ, *nr = near.data() + col * PZ, *bd = body.data() + col * PZ;
            up[PZ] = 0;
            for (size_t z = PZ; z-- > 0;) up[z] = ((p.clear_mask >> c[z]) & 1u) ? std::min<uint32_t>(up[z + 1] + 1u, (uint32_t)h) : 0u;
            for (size_t z = 1; z + h <= PZ; ++z) st[z] = ((p.support_mask >> c[z - 1]) & 1u) && up[z] >= h;
            for (size_t z = 1 + s; z <= nz + s; ++z) {
                uint8_t any = 0;
                for (size_t q = z - s; q <= z + s; ++q) any |= st[q];   // 1 <= q <= nz + 2s = PZ - h
                nr[z] = any;
                bd[z] = up[z + s] >= h - s;
            }
        }
    }
    std::vector<ptrdiff_t> disc;   // the footprint's offsets in the padded arrays
    for (ptrdiff_t di = -(ptrdiff_t)r; di <= (ptrdiff_t)r; ++di)
        for (ptrdiff_t dj = -(ptrdiff_t)r; dj <= (ptrdiff_t)r; ++dj)
            if ((di || dj) && (size_t)(di * di + dj * dj) <= r * r) disc.push_back((di * (ptrdiff_t)PY + dj) * (ptrdiff_t)PZ);
    const size_t n_col = nx * ny;
    std::vector<uint8_t> own_foot;
    if (foot == nullptr) {
        own_foot.resize(n_col * nz);
        foot = own_foot.data();
    }
    std::vector<uint64_t> col_start(n_col + 1, 0), col_stand(n_col, 0), col_body(n_col, 0);
#pragma omp parallel for schedule(static)
    for (size_t col = 0; col < n_col; ++col) {
        const size_t i = col / ny, j = col % ny;
        const size_t base = ((i + r) * PY + (j + r)) * PZ + 1 + s;
        uint32_t found = 0;
        int32_t low = -1, top = -1;
        for (size_t k = 0; k < nz; ++k) {
            const ptrdiff_t at = (ptrdiff_t)(base + k);
            uint8_t is_foot = 0;
            if (stand[(size_t)at]) {
                ++col_stand[col];
                bool free_body = true;
                for (size_t d = 0; d < disc.size() && free_body; ++d) free_body = body[(size_t)(at + disc[d])] != 0;
                if (free_body) {
                    ++col_body[col];
                    uint32_t carried = 0;
                    for (const ptrdiff_t o : disc) carried += near[(size_t)(at + o)];
                    is_foot = carried >= p.min_support;
                }
            }
            foot[col * nz + k] = is_foot;
            if (is_foot) {
                ++found;
                if (low < 0) low = (int32_t)k;
                top = (int32_t)k;
            }
        }
        col_start[col + 1] = found;
        if (levels) levels[col] = found;
        if (lowest) lowest[col] = low;
        if (highest) highest[col] = top;
    }
    Counts n = {0, 0, 0};
    for (size_t col = 0; col < n_col; ++col) {
        n.n_stand += col_stand[col];
        n.n_body += col_body[col];
        col_start[col + 1] += col_start[col];
    }
    n.n_foot = col_start[n_col];
    if (index != nullptr && cap > 0) {
#pragma omp parallel for schedule(static)
        for (size_t col = 0; col < n_col; ++col) {
            uint64_t t = col_start[col];
            for (size_t k = 0; k < nz && t < cap; ++k)
                if (foot[col * nz + k]) index[t++] = (uint32_t)(col * nz + k);
        }
    }
    return n;
}

}  // namespace la3dm_footing

#endif
