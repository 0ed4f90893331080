// localize.cpp — where is the sensor: the next scan scored against the map under a grid of candidate poses round the pose
// it is believed to have been taken from, on the map the static node builds (examples/static_map.cpp's insert loop).  One
// query on the device pool, no host mirror, no distance field downloaded:
//
//   score_poses   per candidate pose the sum of the squared distances (voxel units) from every point of the scan, moved
//                 by the pose, to the nearest OCCUPIED voxel of the box, and the pairs per class: HIT, NEAR, FAR (beyond
//                 the radius), OUTSIDE the box, INVALID.  The likelihood-field score of a scan matcher.
//
//   localize <dir> <prefix> <scan_num> [resolution block_depth sf2 ell free_res ds_res max_range
//                                       free_thresh occupied_thresh var_thresh prior_A prior_B device]
// device: the GPU (default 0); -1 = a host-mode map without a GPU (it cannot insert scans: scan_num 0, the empty map).
// The map: scans 1 ... scan_num.  The cloud scored: scan scan_num + 1 as the file holds it (map frame), so the identity is
// the pose it was taken from.  The box: 128 x 128 x 32 voxels whose voxel (0, 0, 0) holds that scan's origin - (6.4, 6.4,
// 1.6); radius 16 voxels.  Candidates: 9 x 9 x 9 poses, number (i * 9 + j) * 9 + k = rotate about the scan's origin by
// dyaw = 0.02 (k - 4) rad, then translate by dx = 0.1 (i - 4), dy = 0.1 (j - 4) m; the identity is number 364.  The pose
// entries are computed in double with libm's cos and sin and rounded to float once (la3dm_amd.poses_xyz_yaw builds the
// same bits).  Score = sum_d2 + 256 (far + outside): a pair without an obstacle within the radius costs radius^2.
// prints:  best <number> dx <m> dy <m> dyaw <rad> score <n> sum_d2 <n> counts <hit> <near> <far> <outside> <invalid>
//                                                                      the candidate with the least score (the first of equals)
//          identity <number> score <n> sum_d2 <n> counts <hit> <near> <far> <outside> <invalid>
//          localize 128 x 128 x 32 from <origin of voxel 0>: poses <n> points <n> mirror_syncs <n> device_resident <0|1>
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
        for (int scan_id = 1; scan_id <= scan_num + 1; ++scan_id) {   // the last one is scored, not inserted
            const std::string filename = dir + "/" + prefix + "_" + std::to_string(scan_id) + ".pcd";
            if (!load_pcd(filename, origin, cloud)) {
                std::fprintf(stderr, "cannot read %s\n", filename.c_str());
                return 1;
            }
            if (scan_id <= scan_num) map.insert_pointcloud(cloud, origin, v[5], v[4], v[6]);
        }
        const uint32_t dims[3] = {128, 128, 32}, radius = 16, occupied_m = 1u << 1, side = 9;
        const float lo[3] = {origin.x() - 6.4f, origin.y() - 6.4f, origin.z() - 1.6f};
        std::vector<float> points;
        for (const la3dm::point3f &p : cloud) {
            const float q[3] = {p.x(), p.y(), p.z()};
            points.insert(points.end(), q, q + 3);
        }
        // ---- the candidates
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
        const uint32_t n_poses = side * side * side, identity = (4 * side + 4) * side + 4;
        // ---- the score
        std::vector<uint64_t> sum(n_poses);
        std::vector<uint32_t> counts(5 * (size_t)n_poses);
        la3dm_score_out so;
        so.sum_d2 = sum.data();
        so.counts = counts.data();
        la3dm_region_info info;
        map.score_poses(lo, dims, points.data(), (uint32_t)(points.size() / 3), poses.data(), n_poses, occupied_m, radius, so, &info);
        const auto score = [&](uint32_t p) -> unsigned long long {
            return sum[p] + (unsigned long long)(radius * radius) * (counts[5 * p + LA3DM_SCORE_FAR] + counts[5 * p + LA3DM_SCORE_OUTSIDE]);
        };
        uint32_t best = 0;
        for (uint32_t p = 1; p < n_poses; ++p)
            if (score(p) < score(best)) best = p;
        const uint32_t *cb = &counts[5 * best], *ci = &counts[5 * identity];
        std::printf("best %u dx %g dy %g dyaw %g score %llu sum_d2 %llu counts %u %u %u %u %u\n", best, grid[3 * best], grid[3 * best + 1],
                    grid[3 * best + 2], score(best), (unsigned long long)sum[best], cb[0], cb[1], cb[2], cb[3], cb[4]);
        std::printf("identity %u score %llu sum_d2 %llu counts %u %u %u %u %u\n", identity, score(identity), (unsigned long long)sum[identity],
                    ci[0], ci[1], ci[2], ci[3], ci[4]);
        std::printf("localize %u x %u x %u from %g %g %g: poses %u points %llu mirror_syncs %llu device_resident %d\n", dims[0], dims[1], dims[2],
                    info.origin[0], info.origin[1], info.origin[2], n_poses, (unsigned long long)(points.size() / 3),
                    (unsigned long long)map.mirror_syncs(), map.is_device_resident() ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
