// surface_mesh.cpp — the skin of the map as quads, and what its normals do for scan matching, on the map the static node
// builds (examples/static_map.cpp's insert loop).  Queries on the device pool, no host mirror:
//
//   surface          the exposed faces of the OCCUPIED voxels of the box round the sensor against FREE, with the integer
//                    normal summed over a window of smooth = 2 voxels; the faces become quads (one per set bit of the face
//                    mask, counter-clockwise seen from the open side), written as an ASCII PLY when a path is given.
//   score_poses      localize's 9 x 9 x 9 grid round the identity: the start pose of the two alignments is its best candidate.
//   nearest_points   per point of the scan, moved by the current pose: the flat index of the nearest OCCUPIED voxel.
//
//   surface_mesh <dir> <prefix> <scan_num> [resolution block_depth sf2 ell free_res ds_res max_range
//                                           free_thresh occupied_thresh var_thresh prior_A prior_B device [out.ply]]
// device: the GPU (default 0); -1 = a host-mode map without a GPU (it cannot insert scans: scan_num 0, the empty map).
// The map, the cloud and the box (128 x 128 x 32 voxels, radius 16) are align's.  A vertex of the PLY is origin + (corner -
// 0.5) * resolution, corner in voxel-corner units of the region.  Two alignments of 6 steps each start from the grid's best
// candidate: align's point-to-voxel step (the planar rigid fit to the voxel centres), and a point-to-plane step — the
// normal of the nearest voxel looked up by binary search of surface's index; where the voxel has a normal n (unit, from the
// integer one), the residual is n . (p - q), linearised in (yaw, tx, ty) and solved in closed form from the 3 x 3 normal
// equations; where it has none (not a surface voxel, or (0, 0, 0)), the two planar point-to-point residuals.  Both print
// the planar rms distance to the voxel centres, so the two can be compared; nothing is asserted about where the poses end.
// prints:  surface_mesh 128 x 128 x 32 from <origin>: surface voxels <n> solid <n> faces -x <n> +x <n> -y <n> +y <n> -z <n> +z <n>
//                       area_m2 <a> zero_normals <share> floor <share> quads <n> ply <path|none>
//          start <number> dx <m> dy <m> dyaw <rad> score <n>
//          iter <k> voxel rms_xy_m <m> | plane rms_xy_m <m> rms_plane_m <m> with_normal <n> of <n>             k = 0 .. 6
//          surface_mesh done: points <n> mirror_syncs <n> device_resident <0|1>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <algorithm>
#include <vector>

#include "../la3dm_amd/csrc/host/bgkoctomap.h"

// PCD v0.7, "DATA ascii" or "DATA binary" (what pcl::io::loadPCDFile is used for in the reference node): the
// fields x, y, z are located through FIELDS / SIZE / COUNT, VIEWPOINT tx ty tz ... gives the sensor origin.
static bool load_pcd(const std::string &path, la3dm::point3f &origin, la3dm::BGKOctoMap::PointCloud &cloud) {
    std::ifstream in(path, std::ios::binary);
    if (!in) return false;
    std::vector<std::string> fields;
    std::vector<size_t> sizes, counts;
    size_t points = 0;
    std::string line, kind;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string key, tok;
        ss >> key;
        if (key == "FIELDS") while (ss >> tok) fields.push_back(tok);
        else if (key == "SIZE") while (ss >> tok) sizes.push_back((size_t)std::stoul(tok));
        else if (key == "COUNT") while (ss >> tok) counts.push_back((size_t)std::stoul(tok));
        else if (key == "POINTS") ss >> points;
        else if (key == "VIEWPOINT") {
            float x = 0, y = 0, z = 0;
            ss >> x >> y >> z;
            origin = la3dm::point3f(x, y, z);
        } else if (key == "DATA") {
            ss >> kind;
            break;
        }
    }
    if (fields.empty() || sizes.size() != fields.size()) return false;
    if (counts.size() != fields.size()) counts.assign(fields.size(), 1);
    size_t off[3] = {0, 0, 0}, idx[3] = {0, 0, 0}, stride = 0;
    bool have[3] = {false, false, false};
    for (size_t f = 0; f < fields.size(); ++f) {
        for (int a = 0; a < 3; ++a)
            if (fields[f] == std::string(1, "xyz"[a]) && sizes[f] == 4) {
                off[a] = stride;
                idx[a] = f;
                have[a] = true;
            }
        stride += sizes[f] * counts[f];
    }
    if (!have[0] || !have[1] || !have[2]) return false;
    cloud.clear();
    cloud.reserve(points);
    if (kind == "binary") {
        std::vector<char> rec(stride);
        for (size_t i = 0; i < points && in.read(rec.data(), (std::streamsize)stride); ++i) {
            float v[3];
            for (int a = 0; a < 3; ++a) std::memcpy(&v[a], rec.data() + off[a], 4);
            cloud.emplace_back(v[0], v[1], v[2]);
        }
    } else if (kind == "ascii") {
        while (cloud.size() < points && std::getline(in, line)) {
            std::istringstream ss(line);
            std::vector<float> row;
            float t;
            while (ss >> t) row.push_back(t);
            if (row.size() > std::max(idx[0], std::max(idx[1], idx[2]))) cloud.emplace_back(row[idx[0]], row[idx[1]], row[idx[2]]);
        }
    } else {
        return false;
    }
    return cloud.size() == points;
}

// one alignment step's correspondences and residuals under pose T; plane = use the normals where there are any
struct Fit {
    double rms_xy = 0, rms_plane = 0;
    size_t used = 0, with_normal = 0;
    double U[12];   // the next pose
};

int main(int argc, char **argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s dir prefix scan_num [resolution block_depth sf2 ell free_res ds_res max_range ... device [out.ply]]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[2];
    const int scan_num = std::atoi(argv[3]);
    float v[13] = {0.1f, 3, 1.0f, 0.2f, 0.5f, 0.1f, 8.0f, 0.3f, 0.7f, 100.0f, 0.001f, 0.001f, 0};  // bgkoctomap.yaml + sim_structured.yaml, device
    for (int i = 0; i < 13 && 4 + i < argc; ++i) v[i] = (float)std::atof(argv[4 + i]);
    const std::string ply = argc > 17 ? argv[17] : "";
    try {
        la3dm::BGKOctoMap map(v[0], (unsigned short)v[1], v[2], v[3], v[7], v[8], v[9], v[10], v[11], (int)v[12]);
        la3dm::point3f origin(0, 0, 0);
        la3dm::BGKOctoMap::PointCloud cloud;
        for (int scan_id = 1; scan_id <= scan_num + 1; ++scan_id) {   // the last one is aligned, not inserted
            const std::string filename = dir + "/" + prefix + "_" + std::to_string(scan_id) + ".pcd";
            if (!load_pcd(filename, origin, cloud)) {
                std::fprintf(stderr, "cannot read %s\n", filename.c_str());
                return 1;
            }
            if (scan_id <= scan_num) map.insert_pointcloud(cloud, origin, v[5], v[4], v[6]);
        }
        const uint32_t dims[3] = {128, 128, 32}, radius = 16, occupied_m = 1u << 1, free_m = 1u << 0, side = 9, steps = 6;
        const float lo[3] = {origin.x() - 6.4f, origin.y() - 6.4f, origin.z() - 1.6f};
        const double res = v[0];
        // ---- the surface: count, then fill exactly n
        const la3dm_surface_params sp = {occupied_m, free_m, 2};
        la3dm_surface_out out = la3dm_surface_out();
        la3dm_surface_stats st;
        la3dm_region_info info;
        uint64_t n_surface = 0;
        map.surface(lo, dims, &sp, 0, out, &n_surface, &st, &info);
        std::vector<uint32_t> s_index(n_surface);
        std::vector<uint8_t> s_faces(n_surface);
        std::vector<int16_t> s_normal(3 * n_surface);
        if (n_surface) {
            out.index = s_index.data();
            out.faces = s_faces.data();
            out.normal = s_normal.data();
            map.surface(lo, dims, &sp, n_surface, out, &n_surface, &st, &info);
        }
        uint64_t zero = 0, floor_up = 0, n_faces = 0;
        for (uint64_t t = 0; t < n_surface; ++t) {
            const int nx = s_normal[3 * t], ny = s_normal[3 * t + 1], nz = s_normal[3 * t + 2];
            zero += nx == 0 && ny == 0 && nz == 0;
            floor_up += nz > 0 && nz >= std::abs(nx) && nz >= std::abs(ny);
        }
        for (int d = 0; d < 6; ++d) n_faces += st.faces[d];
        // ---- the quads: list order, then ascending direction
        std::vector<int32_t> corners;   // 4 x 3 per quad, voxel-corner units
        for (uint64_t t = 0; t < n_surface; ++t) {
            const uint32_t f = s_index[t];
            const int32_t vox[3] = {(int32_t)(f / (dims[1] * dims[2])), (int32_t)(f / dims[2] % dims[1]), (int32_t)(f % dims[2])};
            for (int d = 0; d < 6; ++d) {
                if (!((s_faces[t] >> d) & 1)) continue;
                const int a = d >> 1, b = (a + 1) % 3, c = (a + 2) % 3, positive = d & 1;
                const int ring[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
                for (int k = 0; k < 4; ++k) {
                    const int *o = ring[positive ? k : 3 - k];
                    int32_t p[3] = {vox[0], vox[1], vox[2]};
                    p[a] += positive;
                    p[b] += o[0];
                    p[c] += o[1];
                    corners.insert(corners.end(), p, p + 3);
                }
            }
        }
        const size_t n_quads = corners.size() / 12;
        if (!ply.empty()) {
            std::ofstream f(ply);
            f << "ply\nformat ascii 1.0\nelement vertex " << 4 * n_quads << "\nproperty float x\nproperty float y\nproperty float z\nelement face " << n_quads
              << "\nproperty list uchar int vertex_index\nend_header\n";
            for (size_t k = 0; k < corners.size(); k += 3)
                f << info.origin[0] + (corners[k] - 0.5) * res << " " << info.origin[1] + (corners[k + 1] - 0.5) * res << " "
                  << info.origin[2] + (corners[k + 2] - 0.5) * res << "\n";
            for (size_t q = 0; q < n_quads; ++q) f << "4 " << 4 * q << " " << 4 * q + 1 << " " << 4 * q + 2 << " " << 4 * q + 3 << "\n";
        }
        std::printf("surface_mesh %u x %u x %u from %g %g %g: surface voxels %llu solid %llu faces -x %llu +x %llu -y %llu +y %llu -z %llu +z %llu "
                    "area_m2 %.2f zero_normals %.4f floor %.4f quads %zu ply %s\n",
                    dims[0], dims[1], dims[2], info.origin[0], info.origin[1], info.origin[2], (unsigned long long)n_surface, (unsigned long long)st.n_solid,
                    (unsigned long long)st.faces[0], (unsigned long long)st.faces[1], (unsigned long long)st.faces[2], (unsigned long long)st.faces[3],
                    (unsigned long long)st.faces[4], (unsigned long long)st.faces[5], (double)n_faces * res * res,
                    n_surface ? (double)zero / (double)n_surface : 0.0, n_surface ? (double)floor_up / (double)n_surface : 0.0, n_quads,
                    ply.empty() ? "none" : ply.c_str());
        // ---- the start of both alignments: the best candidate of localize's grid
        std::vector<float> points;
        for (const la3dm::point3f &p : cloud) {
            const float q[3] = {p.x(), p.y(), p.z()};
            points.insert(points.end(), q, q + 3);
        }
        const uint32_t n = (uint32_t)(points.size() / 3);
        const double cx = origin.x(), cy = origin.y();
        std::vector<float> poses;
        std::vector<double> grid;
        for (uint32_t i = 0; i < side; ++i)
            for (uint32_t j = 0; j < side; ++j)
                for (uint32_t k = 0; k < side; ++k) {
                    const double dx = 0.1 * ((int)i - 4), dy = 0.1 * ((int)j - 4), dyaw = 0.02 * ((int)k - 4);
                    const double c = std::cos(dyaw), s = std::sin(dyaw);
                    const double T[12] = {c, -s, 0.0, (cx + dx) - (c * cx - s * cy), s, c, 0.0, (cy + dy) - (s * cx + c * cy), 0.0, 0.0, 1.0, 0.0};
                    for (double t : T) poses.push_back((float)t);
                    const double g[3] = {dx, dy, dyaw};
                    grid.insert(grid.end(), g, g + 3);
                }
        const uint32_t n_poses = side * side * side;
        std::vector<uint64_t> sum(n_poses);
        std::vector<uint32_t> counts(5 * (size_t)n_poses);
        la3dm_score_out so;
        so.sum_d2 = sum.data();
        so.counts = counts.data();
        map.score_poses(lo, dims, points.data(), n, poses.data(), n_poses, occupied_m, radius, so, &info);
        const auto score = [&](uint32_t p) -> unsigned long long {
            return sum[p] + (unsigned long long)(radius * radius) * (counts[5 * p + LA3DM_SCORE_FAR] + counts[5 * p + LA3DM_SCORE_OUTSIDE]);
        };
        uint32_t best = 0;
        for (uint32_t p = 1; p < n_poses; ++p)
            if (score(p) < score(best)) best = p;
        std::printf("start %u dx %g dy %g dyaw %g score %llu\n", best, grid[3 * best], grid[3 * best + 1], grid[3 * best + 2], score(best));
        // ---- one step of either kind from pose T
        std::vector<uint8_t> cls(n);
        std::vector<uint32_t> index(n), d2(n);
        la3dm_nearest_points_out no;
        no.cls = cls.data();
        no.voxel = nullptr;
        no.index = index.data();
        no.d2 = d2.data();
        const auto step = [&](const float *T, bool plane) {
            Fit fit;
            map.nearest_points(lo, dims, points.data(), n, T, occupied_m, radius, no, &info);
            double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, rhs[3] = {0, 0, 0};   // unknowns (yaw, tx, ty), linearised at yaw = 0
            double pm[2] = {0, 0}, qm[2] = {0, 0}, e_xy = 0, e_plane = 0;
            std::vector<double> P, Q;
            for (uint32_t p = 0; p < n; ++p) {
                if (cls[p] > LA3DM_SCORE_NEAR) continue;
                const float *q = &points[3 * (size_t)p];
                const uint32_t f = index[p], i2 = f / (dims[1] * dims[2]), j2 = f / dims[2] % dims[1], k2 = f % dims[2];
                const double w[3] = {(double)T[0] * q[0] + (double)T[1] * q[1] + (double)T[2] * q[2] + (double)T[3],
                                     (double)T[4] * q[0] + (double)T[5] * q[1] + (double)T[6] * q[2] + (double)T[7],
                                     (double)T[8] * q[0] + (double)T[9] * q[1] + (double)T[10] * q[2] + (double)T[11]};
                const double t[3] = {info.origin[0] + i2 * res, info.origin[1] + j2 * res, info.origin[2] + k2 * res};
                const double d[3] = {w[0] - t[0], w[1] - t[1], w[2] - t[2]};
                e_xy += d[0] * d[0] + d[1] * d[1];
                ++fit.used;
                P.insert(P.end(), w, w + 2);
                Q.insert(Q.end(), t, t + 2);
                for (int a = 0; a < 2; ++a) {
                    pm[a] += w[a];
                    qm[a] += t[a];
                }
                double nrm[3] = {0, 0, 0};
                const auto at = std::lower_bound(s_index.begin(), s_index.end(), f);
                if (at != s_index.end() && *at == f) {
                    const size_t e = (size_t)(at - s_index.begin());
                    const double len = std::sqrt((double)s_normal[3 * e] * s_normal[3 * e] + (double)s_normal[3 * e + 1] * s_normal[3 * e + 1] +
                                                 (double)s_normal[3 * e + 2] * s_normal[3 * e + 2]);
                    if (len > 0)
                        for (int a = 0; a < 3; ++a) nrm[a] = s_normal[3 * e + (size_t)a] / len;
                }
                const bool has = nrm[0] != 0 || nrm[1] != 0 || nrm[2] != 0;
                fit.with_normal += has;
                // rows g . (yaw, tx, ty) = -r0: the moved point is w + yaw (-w_y, w_x, 0) + (tx, ty, 0)
                const double rows[2][3] = {{has ? nrm[0] : 1.0, has ? nrm[1] : 0.0, has ? nrm[2] : 0.0}, {0.0, 1.0, 0.0}};
                for (int r = 0; r < (has ? 1 : 2); ++r) {
                    const double *m = rows[r];
                    const double r0 = m[0] * d[0] + m[1] * d[1] + (has ? m[2] * d[2] : 0.0);
                    const double g[3] = {-m[0] * w[1] + m[1] * w[0], m[0], m[1]};
                    if (has) e_plane += r0 * r0;
                    for (int a = 0; a < 3; ++a) {
                        rhs[a] -= g[a] * r0;
                        for (int b = 0; b < 3; ++b) A[a][b] += g[a] * g[b];
                    }
                }
            }
            fit.rms_xy = fit.used ? std::sqrt(e_xy / (double)fit.used) : 0.0;
            fit.rms_plane = fit.with_normal ? std::sqrt(e_plane / (double)fit.with_normal) : 0.0;
            double yaw = 0, tx = 0, ty = 0;
            const size_t m = fit.used;
            if (m >= 3 && !plane) {   // align's planar rigid fit to the voxel centres
                for (int a = 0; a < 2; ++a) {
                    pm[a] /= (double)m;
                    qm[a] /= (double)m;
                }
                double Sc = 0, Ss = 0;
                for (size_t p = 0; p < m; ++p) {
                    const double px = P[2 * p] - pm[0], py = P[2 * p + 1] - pm[1], qx = Q[2 * p] - qm[0], qy = Q[2 * p + 1] - qm[1];
                    Sc += px * qx + py * qy;
                    Ss += px * qy - py * qx;
                }
                yaw = std::atan2(Ss, Sc);
                tx = qm[0] - (std::cos(yaw) * pm[0] - std::sin(yaw) * pm[1]);
                ty = qm[1] - (std::sin(yaw) * pm[0] + std::cos(yaw) * pm[1]);
            } else if (m >= 3) {   // Cramer's rule on the 3 x 3 normal equations; a singular system leaves the pose alone
                const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                                   A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
                if (std::fabs(det) > 1e-12) {
                    double x[3];
                    for (int c = 0; c < 3; ++c) {
                        double B[3][3];
                        for (int a = 0; a < 3; ++a)
                            for (int b = 0; b < 3; ++b) B[a][b] = b == c ? rhs[a] : A[a][b];
                        x[c] = (B[0][0] * (B[1][1] * B[2][2] - B[1][2] * B[2][1]) - B[0][1] * (B[1][0] * B[2][2] - B[1][2] * B[2][0]) +
                                B[0][2] * (B[1][0] * B[2][1] - B[1][1] * B[2][0])) / det;
                    }
                    // the linearised rotation turns about the frame's origin: [R(yaw) | (tx, ty)] with the same first-order motion
                    yaw = x[0];
                    tx = x[1];
                    ty = x[2];
                }
            }
            const double c = std::cos(yaw), s = std::sin(yaw);
            for (int col = 0; col < 4; ++col) {
                fit.U[col] = c * T[col] - s * T[4 + col];
                fit.U[4 + col] = s * T[col] + c * T[4 + col];
                fit.U[8 + col] = T[8 + col];
            }
            fit.U[3] += tx;
            fit.U[7] += ty;
            return fit;
        };
        float Tv[12], Tp[12];
        std::memcpy(Tv, &poses[12 * (size_t)best], sizeof(Tv));
        std::memcpy(Tp, Tv, sizeof(Tp));
        for (uint32_t it = 0; it <= steps; ++it) {
            const Fit fv = step(Tv, false), fp = step(Tp, true);
            std::printf("iter %u voxel rms_xy_m %.6f | plane rms_xy_m %.6f rms_plane_m %.6f with_normal %zu of %zu\n", it, fv.rms_xy, fp.rms_xy, fp.rms_plane,
                        fp.with_normal, fp.used);
            for (int k = 0; k < 12; ++k) {
                Tv[k] = (float)fv.U[k];
                Tp[k] = (float)fp.U[k];
            }
        }
        std::printf("surface_mesh done: points %u mirror_syncs %llu device_resident %d\n", n, (unsigned long long)map.mirror_syncs(),
                    map.is_device_resident() ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
