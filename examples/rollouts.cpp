// rollouts.cpp — which way to drive: a fan of candidate arcs from the sensor's position, scored in one call against the
// map the static node builds (examples/static_map.cpp's insert loop).  One query on the device pool, no host mirror, no
// distance field downloaded:
//
//   score_paths   per arc the cost of its walk through the box in travel's units (10 / 14 / 17 a move, a penalty near
//                 obstacles), the voxels walked, where it stopped (BLOCKED by an OCCUPIED voxel, LEFT
//                 the box) and its least squared distance to an obstacle.  The rollout scores of a sampling local planner.
//
//   rollouts <dir> <prefix> <scan_num> [resolution block_depth sf2 ell free_res ds_res max_range
//                                       free_thresh occupied_thresh var_thresh prior_A prior_B device]
// device: the GPU (default 0); -1 = a host-mode map without a GPU (it cannot insert scans: scan_num 0, the empty map).
// The map: scans 1 ... scan_num.  The start: the origin of scan scan_num + 1 lifted by 0.3 m (the sensor of this data set
// sits one voxel above the floor, where every arc would be blocked before its first move).  The box: 128 x 128 x 32 voxels whose voxel
// (0, 0, 0) holds that origin - (6.4, 6.4, 1.6).  The arcs: 8 headings x 41 curvatures, number j * 41 + i with heading
// theta = j pi / 4 and curvature kappa = 0.05 (i - 20) per metre, 32 waypoints each at arc lengths s = 4 k / 31 m:
// dx = sin(kappa s) / kappa, dy = (1 - cos(kappa s)) / kappa (dx = s, dy = 0 for kappa = 0), turned by theta and added to
// the origin, in double with libm's sin and cos and rounded to float once (tests/test_paths_gpu.py builds the same bits).
// clearance 0 (the OCCUPIED voxels themselves block), soft_radius 3, penalty 20, moves 10 / 14 / 17, at most 4096 steps.
// prints:  best <number> heading <j> curvature <1/m> cost <n> steps <n> min_d2 <n>     the cheapest arc with flags 0 (the
//                                                                      first of equals), or  best none
//          blocked <n> steps min <n> max <n> sum <n>                   how far the BLOCKED arcs get (voxels walked)
//          left <n> truncated <n> invalid <n> clean <n>
//          rollouts 128 x 128 x 32 from <origin of voxel 0>: paths <n> waypoints <n> mirror_syncs <n> device_resident <0|1>
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
        for (int scan_id = 1; scan_id <= scan_num + 1; ++scan_id) {   // the last one gives the start, it is not inserted
            const std::string filename = dir + "/" + prefix + "_" + std::to_string(scan_id) + ".pcd";
            if (!load_pcd(filename, origin, cloud)) {
                std::fprintf(stderr, "cannot read %s\n", filename.c_str());
                return 1;
            }
            if (scan_id <= scan_num) map.insert_pointcloud(cloud, origin, v[5], v[4], v[6]);
        }
        const uint32_t dims[3] = {128, 128, 32}, n_head = 8, n_curv = 41, n_way = 32, n_paths = n_head * n_curv;
        const float lo[3] = {origin.x() - 6.4f, origin.y() - 6.4f, origin.z() - 1.6f};
        // ---- the arcs
        const double ox = origin.x(), oy = origin.y(), pi = 3.14159265358979323846;
        std::vector<float> ways;
        for (uint32_t j = 0; j < n_head; ++j)
            for (uint32_t i = 0; i < n_curv; ++i)
                for (uint32_t k = 0; k < n_way; ++k) {
                    const double theta = j * pi / 4, kappa = 0.05 * ((int)i - 20), s = 4.0 * k / 31;
                    const double dx = i == 20 ? s : std::sin(kappa * s) / kappa, dy = i == 20 ? 0.0 : (1.0 - std::cos(kappa * s)) / kappa;
                    const double c = std::cos(theta), sn = std::sin(theta);
                    ways.push_back((float)(ox + (c * dx - sn * dy)));
                    ways.push_back((float)(oy + (sn * dx + c * dy)));
                    ways.push_back(origin.z() + 0.3f);
                }
        // ---- the scores
        la3dm_paths_params prm;
        std::memset(&prm, 0, sizeof(prm));
        prm.obstacle_mask = 1u << 1;
        prm.clearance = 0;
        prm.soft_radius = 3;
        prm.penalty = 20;
        prm.move_cost[0] = 10;
        prm.move_cost[1] = 14;
        prm.move_cost[2] = 17;
        prm.max_steps = 4096;
        std::vector<uint64_t> cost(n_paths);
        std::vector<uint32_t> steps(n_paths), min_d2(n_paths);
        std::vector<uint8_t> flags(n_paths);
        la3dm_paths_out po;
        std::memset(&po, 0, sizeof(po));
        po.cost = cost.data();
        po.steps = steps.data();
        po.min_d2 = min_d2.data();
        po.flags = flags.data();
        la3dm_region_info info;
        map.score_paths(lo, dims, ways.data(), n_paths, n_way, &prm, po, &info);
        long best = -1;
        uint32_t n_blocked = 0, n_left = 0, n_trunc = 0, n_invalid = 0, n_clean = 0, s_min = 0xFFFFFFFFu, s_max = 0;
        unsigned long long s_sum = 0;
        for (uint32_t p = 0; p < n_paths; ++p) {
            if (flags[p] == 0) {
                ++n_clean;
                if (best < 0 || cost[p] < cost[(size_t)best]) best = (long)p;
            } else if (flags[p] & LA3DM_PATH_BLOCKED) {
                ++n_blocked;
                s_min = std::min(s_min, steps[p]);
                s_max = std::max(s_max, steps[p]);
                s_sum += steps[p];
            } else if (flags[p] & LA3DM_PATH_LEFT) {
                ++n_left;
            } else if (flags[p] & LA3DM_PATH_TRUNCATED) {
                ++n_trunc;
            } else {
                ++n_invalid;
            }
        }
        if (best < 0)
            std::printf("best none\n");
        else
            std::printf("best %ld heading %ld curvature %g cost %llu steps %u min_d2 %u\n", best, best / n_curv, 0.05 * ((int)(best % n_curv) - 20),
                        (unsigned long long)cost[(size_t)best], steps[(size_t)best], min_d2[(size_t)best]);
        std::printf("blocked %u steps min %u max %u sum %llu\n", n_blocked, n_blocked ? s_min : 0u, s_max, s_sum);
        std::printf("left %u truncated %u invalid %u clean %u\n", n_left, n_trunc, n_invalid, n_clean);
        std::printf("rollouts %u x %u x %u from %g %g %g: paths %u waypoints %u mirror_syncs %llu device_resident %d\n", dims[0], dims[1], dims[2],
                    info.origin[0], info.origin[1], info.origin[2], n_paths, n_way, (unsigned long long)map.mirror_syncs(),
                    map.is_device_resident() ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
