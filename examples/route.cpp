// route.cpp — which exploration goal is cheapest to drive to, and along which voxels: the frontier of a height band round
// the robot (examples/frontier.cpp), then la3dm::BGKOctoMap::travel from the sensor's voxel with the frontier's index list
// as targets, and the path to the cheapest goal followed through the parents.  On a device-resident map everything is
// answered from the device pool: no host mirror is downloaded, no class array is fetched, no Dijkstra runs on the CPU.
//
// travel(lo, dims, seeds, params, targets) gives every voxel the least cost of a walk from the seeds through the passable
// voxels of the region — here FREE voxels farther than 1 voxel from every OCCUPIED voxel of the region — where an axis
// move costs 10, a move along two axes 14, along three 17, and entering a voxel within 4 voxels of an obstacle costs up to
// 40 more, so the path keeps off the walls where it can.  parent[v] is the code (di + 1) * 9 + (dj + 1) * 3 + (dk + 1) of
// the offset to the voxel the walk came from, 13 at the seed.
//
//   route <dir> <prefix> <scan_num> [resolution block_depth sf2 ell free_res ds_res max_range
//                                    free_thresh occupied_thresh var_thresh prior_A prior_B device]
// device: the GPU (default 0); -1 = a host-mode map without a GPU (it cannot insert scans: scan_num 0, the empty map).
// The box: 128 x 128 x 16 voxels whose voxel (0, 0, 0) holds the last sensor origin - (6.4, 6.4, 0.8); frontier with
// connectivity 6 and min_neighbours 1; travel with connectivity 26.
// prints:  goal <x> <y> <z> cost <n>       the (at most) five reachable goals with the least cost, as world points
//          path <n> voxels length <metres> least_d2 <squared voxels | far>     the first goal's path: its voxels, its length, and
//                                          the least squared distance to an obstacle along it (far: beyond 4 voxels everywhere)
//          route 128 x 128 x 16 from <origin of voxel 0>: found <n> reachable <n> max_cost <n> mirror_syncs <n> device_resident <0|1>
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
        for (int scan_id = 1; scan_id <= scan_num; ++scan_id) {
            la3dm::BGKOctoMap::PointCloud cloud;
            const std::string filename = dir + "/" + prefix + "_" + std::to_string(scan_id) + ".pcd";
            if (!load_pcd(filename, origin, cloud)) {
                std::fprintf(stderr, "cannot read %s\n", filename.c_str());
                return 1;
            }
            map.insert_pointcloud(cloud, origin, v[5], v[4], v[6]);
        }
        const uint32_t dims[3] = {128, 128, 16};
        const size_t n = (size_t)dims[0] * dims[1] * dims[2];
        const float lo[3] = {origin.x() - 6.4f, origin.y() - 6.4f, origin.z() - 0.8f};
        const float res = v[0];
        const uint32_t free_mask = 1u << 0, occupied = 1u << 1, unknown = (1u << 2) | (1u << 3);   // FREE; OCCUPIED; UNKNOWN | MISSING
        la3dm_region_info info;
        uint64_t found = 0;
        la3dm_frontier_out fo;
        fo.index = nullptr;
        fo.nbrs = nullptr;
        fo.score = nullptr;
        map.frontier(lo, dims, free_mask, unknown, 6, 1, 0, fo, &found, &info);   // count
        std::vector<uint32_t> index(found);
        if (found) {
            fo.index = index.data();
            map.frontier(lo, dims, free_mask, unknown, 6, 1, found, fo, &found, nullptr);
        }
        // the seed: the voxel of the region that holds the sensor
        uint32_t s[3];
        const float o3[3] = {origin.x(), origin.y(), origin.z()};
        for (int a = 0; a < 3; ++a) {
            const long c = std::lround((o3[a] - info.origin[a]) / res);
            s[a] = (uint32_t)std::max(0l, std::min(c, (long)dims[a] - 1));
        }
        const uint32_t seed = (s[0] * dims[1] + s[1]) * dims[2] + s[2];
        la3dm_travel_params tp;
        tp.pass_mask = free_mask;
        tp.obstacle_mask = occupied;
        tp.clearance = 1;
        tp.soft_radius = 4;
        tp.penalty = 40;
        tp.move_cost[0] = 10;
        tp.move_cost[1] = 14;
        tp.move_cost[2] = 17;
        tp.connectivity = 26;
        tp.max_cost = LA3DM_TRAVEL_MAX_COST;
        std::vector<uint32_t> cost(found);
        std::vector<uint8_t> parent;
        la3dm_travel_stats stats;
        std::memset(&stats, 0, sizeof(stats));
        if (found) {   // (without a goal there is nothing to ask)
            parent.resize(n);
            la3dm_travel_out to;
            to.cost = nullptr;
            to.target_cost = cost.data();
            to.parent = parent.data();
            map.travel(lo, dims, &seed, 1, tp, index.data(), (uint32_t)found, to, &stats, nullptr);
        }
        struct Goal {
            uint32_t cost, f;
        };
        std::vector<Goal> goals;
        for (size_t t = 0; t < index.size(); ++t)
            if (cost[t] != LA3DM_TRAVEL_NONE) goals.push_back(Goal{cost[t], index[t]});
        std::stable_sort(goals.begin(), goals.end(), [](const Goal &a, const Goal &b) { return a.cost < b.cost; });
        for (size_t t = 0; t < goals.size() && t < 5; ++t) {
            const uint32_t f = goals[t].f, k = f % dims[2], j = (f / dims[2]) % dims[1], i = f / (dims[2] * dims[1]);
            std::printf("goal %g %g %g cost %u\n", info.origin[0] + (float)i * res, info.origin[1] + (float)j * res,
                        info.origin[2] + (float)k * res, goals[t].cost);
        }
        if (!goals.empty()) {
            // the first goal's path: every parent names the offset to the voxel before; the walk ends at the seed (13)
            std::vector<uint32_t> d2(n);
            la3dm_distance_out dd;
            dd.d2 = d2.data();
            dd.dist = nullptr;
            map.distance_field(lo, dims, occupied, tp.soft_radius, dd, nullptr);
            uint32_t f = goals[0].f, least = LA3DM_DF_FAR;
            size_t voxels = 1;
            double length = 0.0;
            least = std::min(least, d2[f]);
            while (parent[f] != 13) {   // at most n trips: the cost falls with every one
                const int q = parent[f], di = q / 9 - 1, dj = (q / 3) % 3 - 1, dk = q % 3 - 1;
                if (q == 255 || voxels > n) throw std::runtime_error("route: the parents do not lead to the seed");
                f = (uint32_t)((int64_t)f + ((int64_t)di * dims[1] + dj) * dims[2] + dk);
                length += std::sqrt((double)(di * di + dj * dj + dk * dk)) * res;
                least = std::min(least, d2[f]);
                ++voxels;
            }
            if (least == LA3DM_DF_FAR)
                std::printf("path %zu voxels length %.3f least_d2 far\n", voxels, length);
            else
                std::printf("path %zu voxels length %.3f least_d2 %u\n", voxels, length, least);
        }
        std::printf("route %u x %u x %u from %g %g %g: found %llu reachable %llu max_cost %u mirror_syncs %llu device_resident %d\n", dims[0],
                    dims[1], dims[2], info.origin[0], info.origin[1], info.origin[2], (unsigned long long)found,
                    (unsigned long long)goals.size(), stats.max_cost, (unsigned long long)map.mirror_syncs(),
                    map.is_device_resident() ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
