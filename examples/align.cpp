// align.cpp — refine the pose where localize stops: a few point-to-voxel ICP steps from the best candidate of localize's
// pose grid, on the map the static node builds (examples/static_map.cpp's insert loop).  Two queries on the device pool, no
// host mirror, no distance field downloaded:
//
//   score_poses      localize's 9 x 9 x 9 grid round the identity: the start pose is its best candidate.
//   nearest_points   per point of the scan, moved by the current pose: its class (HIT, NEAR, FAR, OUTSIDE, INVALID), the
//                    flat index of the nearest OCCUPIED voxel of the box and the squared distance to it in voxels — the
//                    correspondences of the step.
//
//   align <dir> <prefix> <scan_num> [resolution block_depth sf2 ell free_res ds_res max_range
//                                    free_thresh occupied_thresh var_thresh prior_A prior_B device]
// device: the GPU (default 0); -1 = a host-mode map without a GPU (it cannot insert scans: scan_num 0, the empty map).
// The map, the cloud, the box (128 x 128 x 32 voxels, radius 16) and the candidates are localize's.  Each of the 6 steps:
// nearest_points with the current pose; over the HIT and NEAR points, the moved point p (double, from the float pose) and
// the centre q of its `index` voxel (origin + (i', j', k') * resolution); the planar rigid fit in closed form — centred
// sums Sc = sum (p - pm) . (q - qm), Ss = sum (p - pm) x (q - qm) over x and y, yaw = atan2(Ss, Sc), t = qm - R(yaw) pm —
// and the pose update T <- [R(yaw) | t] T, computed in double and rounded to float once per entry.  z is left alone.
// A step minimises the planar distance to the voxel centres (rms_xy_m), not the sum of the integer d2 that the grid search
// has already minimised over its 729 candidates, so that sum need not fall.  Nothing is asserted about where the pose ends:
// the program prints what happens.
// prints:  start <number> dx <m> dy <m> dyaw <rad> score <n>          the grid's best candidate (the first of equals)
//          iter <k> sum_d2 <n> hit <n> near <n> far <n> outside <n> invalid <n> rms_xy_m <m> pose <12 floats as %a>   k = 0 .. 6
//                                                                      (the sums and counts of the pose printed on the line)
//          align 128 x 128 x 32 from <origin of voxel 0>: start_sum <n> end_sum <n> least_sum <n> rises <n> points <n>
//                                                                      mirror_syncs <n> device_resident <0|1>
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

int main(int argc, char **argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s dir prefix scan_num [resolution block_depth sf2 ell free_res ds_res max_range ... device]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[2];
    const int scan_num = std::atoi(argv[3]);
    float v[13] = {0.1f, 3, 1.0f, 0.2f, 0.5f, 0.1f, 8.0f, 0.3f, 0.7f, 100.0f, 0.001f, 0.001f, 0};  // bgkoctomap.yaml + sim_structured.yaml, device
    for (int i = 0; i < 13 && 4 + i < argc; ++i) v[i] = (float)std::atof(argv[4 + i]);
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
        const uint32_t dims[3] = {128, 128, 32}, radius = 16, occupied_m = 1u << 1, side = 9, steps = 6;
        const float lo[3] = {origin.x() - 6.4f, origin.y() - 6.4f, origin.z() - 1.6f};
        std::vector<float> points;
        for (const la3dm::point3f &p : cloud) {
            const float q[3] = {p.x(), p.y(), p.z()};
            points.insert(points.end(), q, q + 3);
        }
        const uint32_t n = (uint32_t)(points.size() / 3);
        // ---- the start: the best candidate of localize's grid
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
        la3dm_region_info info;
        map.score_poses(lo, dims, points.data(), n, poses.data(), n_poses, occupied_m, radius, so, &info);
        const auto score = [&](uint32_t p) -> unsigned long long {
            return sum[p] + (unsigned long long)(radius * radius) * (counts[5 * p + LA3DM_SCORE_FAR] + counts[5 * p + LA3DM_SCORE_OUTSIDE]);
        };
        uint32_t best = 0;
        for (uint32_t p = 1; p < n_poses; ++p)
            if (score(p) < score(best)) best = p;
        std::printf("start %u dx %g dy %g dyaw %g score %llu\n", best, grid[3 * best], grid[3 * best + 1], grid[3 * best + 2], score(best));
        // ---- the steps
        float T[12];
        std::memcpy(T, &poses[12 * (size_t)best], sizeof(T));
        std::vector<uint8_t> cls(n);
        std::vector<uint32_t> index(n), d2(n);
        la3dm_nearest_points_out no;
        no.cls = cls.data();
        no.voxel = nullptr;
        no.index = index.data();
        no.d2 = d2.data();
        const double res = v[0];
        unsigned long long first_sum = 0, last_sum = 0, least_sum = 0, rises = 0;
        for (uint32_t it = 0; it <= steps; ++it) {
            map.nearest_points(lo, dims, points.data(), n, T, occupied_m, radius, no, &info);
            unsigned long long total = 0, c5[5] = {0, 0, 0, 0, 0};
            double pm[2] = {0, 0}, qm[2] = {0, 0};
            std::vector<double> P, Q;   // the moved points and their targets, x and y
            for (uint32_t p = 0; p < n; ++p) {
                ++c5[cls[p]];
                if (cls[p] > LA3DM_SCORE_NEAR) continue;
                total += d2[p];
                const float *q = &points[3 * (size_t)p];
                const uint32_t f = index[p], i2 = f / (dims[1] * dims[2]), j2 = f / dims[2] % dims[1];
                const double w[2] = {(double)T[0] * q[0] + (double)T[1] * q[1] + (double)T[2] * q[2] + (double)T[3],
                                     (double)T[4] * q[0] + (double)T[5] * q[1] + (double)T[6] * q[2] + (double)T[7]};
                const double t[2] = {info.origin[0] + i2 * res, info.origin[1] + j2 * res};
                P.insert(P.end(), w, w + 2);
                Q.insert(Q.end(), t, t + 2);
                for (int a = 0; a < 2; ++a) {
                    pm[a] += w[a];
                    qm[a] += t[a];
                }
            }
            double fit = 0;   // what a step minimises: the planar distance from a moved point to the centre of its obstacle voxel
            for (size_t p = 0; p < P.size(); ++p) fit += (P[p] - Q[p]) * (P[p] - Q[p]);
            std::printf("iter %u sum_d2 %llu hit %llu near %llu far %llu outside %llu invalid %llu rms_xy_m %.6f pose", it, total, c5[0], c5[1], c5[2], c5[3],
                        c5[4], P.empty() ? 0.0 : std::sqrt(fit / (double)(P.size() / 2)));
            for (float t : T) std::printf(" %a", (double)t);
            std::printf("\n");
            if (it == 0) first_sum = least_sum = total;
            rises += it > 0 && total > last_sum;
            least_sum = std::min(least_sum, total);
            last_sum = total;
            const size_t m = P.size() / 2;
            if (it == steps || m < 3) continue;
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
            const double yaw = std::atan2(Ss, Sc), c = std::cos(yaw), s = std::sin(yaw);
            const double tx = qm[0] - (c * pm[0] - s * pm[1]), ty = qm[1] - (s * pm[0] + c * pm[1]);
            double U[12];   // [R(yaw) | t] T
            for (int col = 0; col < 4; ++col) {
                U[col] = c * T[col] - s * T[4 + col];
                U[4 + col] = s * T[col] + c * T[4 + col];
                U[8 + col] = T[8 + col];
            }
            U[3] += tx;
            U[7] += ty;
            for (int k = 0; k < 12; ++k) T[k] = (float)U[k];
        }
        std::printf("align %u x %u x %u from %g %g %g: start_sum %llu end_sum %llu least_sum %llu rises %llu points %u mirror_syncs %llu device_resident %d\n",
                    dims[0], dims[1], dims[2], info.origin[0], info.origin[1], info.origin[2], first_sum, last_sum, least_sum, rises, n,
                    (unsigned long long)map.mirror_syncs(), map.is_device_resident() ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
