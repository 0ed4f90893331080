// ground_route.cpp — examples/ground_goals.cpp continued: which exploration goal is the cheapest to DRIVE to, and along which
// route.  la3dm::BGKOctoMap::drive in footing mode takes footing's parameters and routes over exactly the voxels footing
// would list — on a device-resident map footing's kernels feed the query on the device, nothing is listed, scanned or
// downloaded in between.  The seed is the sensor's voxel as it is: `snap` lowers it to the standing place under the sensor.
// The targets are the frontier voxels (examples/frontier.cpp); those that are no foot voxels answer LA3DM_DRIVE_NONE, as do
// those on ground the robot cannot get to.  A move goes to one of the 8 horizontal neighbours and climbs or drops at most
// `step` voxels — 10 / 14 cost units, 5 more per voxel climbed, 2 per voxel dropped — and the parents give the route back
// from the goal to the robot.  examples/route.cpp does the same for a robot that flies.
//
//   ground_route <dir> <prefix> <scan_num> [resolution block_depth sf2 ell free_res ds_res max_range
//                                           free_thresh occupied_thresh var_thresh prior_A prior_B device]
// device: the GPU (default 0); -1 = a host-mode map without a GPU (it cannot insert scans: scan_num 0, the empty map).
// The box: 128 x 128 x 32 voxels whose voxel (0, 0, 0) holds the last sensor origin - (6.4, 6.4, 2.0).
// prints:  drive: members <n> seeded <n> reached <n> max_cost <n> rounds <n>
//          goal <i j k> cost <c> of <n> goals on reachable ground (<n> frontier voxels)     or: no goal on reachable ground
//          route <n> voxels: <i j k> ... (from the robot to the goal, every 8th voxel and the last)
//          ground_route 128 x 128 x 32 from <origin of voxel 0>: mirror_syncs <n> device_resident <0|1>
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
        const uint32_t dims[3] = {128, 128, 32};
        const size_t n = (size_t)dims[0] * dims[1] * dims[2];
        const float lo[3] = {origin.x() - 6.4f, origin.y() - 6.4f, origin.z() - 2.0f};
        const float res = v[0];
        const uint32_t free_mask = 1u << 0, occupied = 1u << 1, unseen = (1u << 2) | (1u << 3);   // FREE; OCCUPIED; UNKNOWN | MISSING
        la3dm_region_info info;
        // the exploration goals: free voxels that border unexplored space
        uint64_t n_front = 0;
        la3dm_frontier_out fo;
        fo.index = nullptr;
        fo.nbrs = nullptr;
        fo.score = nullptr;
        map.frontier(lo, dims, free_mask, unseen, 6, 1, 0, fo, &n_front, &info);   // count
        std::vector<uint32_t> front(n_front);
        if (n_front) {
            fo.index = front.data();
            map.frontier(lo, dims, free_mask, unseen, 6, 1, n_front, fo, &n_front, nullptr);
        }
        // the sensor's voxel, as it is: snap finds the ground under it
        uint32_t s[3];
        const float o3[3] = {origin.x(), origin.y(), origin.z()};
        for (int a = 0; a < 3; ++a) {
            const long c = std::lround((o3[a] - info.origin[a]) / res);
            s[a] = (uint32_t)std::max(0l, std::min(c, (long)dims[a] - 1));
        }
        const uint32_t seed = (s[0] * dims[1] + s[1]) * dims[2] + s[2];
        la3dm_footing_params fp;
        fp.support_mask = occupied;
        fp.clear_mask = free_mask | unseen;
        fp.headroom = 4;   // a body 0.4 m tall
        fp.radius = 2;     // ... and 0.5 m wide
        fp.step = 1;       // ... that climbs one voxel
        fp.min_support = 6;   // half the footprint carried: the floor of a scanned map has holes
        la3dm_drive_params dp;
        std::memset(&dp, 0, sizeof(dp));
        dp.footing = &fp;   // footing mode: no list
        dp.connectivity = 8;
        dp.step = fp.step;
        dp.snap = LA3DM_DRIVE_MAX_SNAP;
        dp.move_cost[0] = 10;
        dp.move_cost[1] = 14;
        dp.climb_up = 5;
        dp.climb_down = 2;
        dp.max_cost = LA3DM_TRAVEL_MAX_COST;
        std::vector<uint8_t> parent(n);
        std::vector<uint32_t> goal_cost(front.size());
        la3dm_drive_out out;
        std::memset(&out, 0, sizeof(out));
        out.parent = parent.data();
        std::vector<uint32_t> cost;
        if (front.empty()) {   // (no target: the dense cost is the mandatory output then)
            cost.resize(n);
            out.cost = cost.data();
        } else {
            out.target_cost = goal_cost.data();
        }
        la3dm_drive_stats ds;
        std::memset(&ds, 0, sizeof(ds));
        // snap lowers the seed to the ground under the sensor; it would lower a target as well, and a goal is a frontier voxel
        // at which the robot itself can stand: the parent of a target that is no reached member is 255, and that one is skipped
        map.drive(lo, dims, &seed, 1, &dp, front.empty() ? nullptr : front.data(), (uint32_t)front.size(), &out, &ds, nullptr);
        std::printf("drive: members %u seeded %u reached %u max_cost %u rounds %u\n", ds.n_members, ds.n_seeded, ds.n_reached, ds.max_cost, ds.rounds);
        uint32_t best = LA3DM_DRIVE_NONE, goal = 0;
        uint64_t n_goals = 0;
        for (size_t t = 0; t < front.size(); ++t) {
            if (parent[front[t]] == 255 || goal_cost[t] == LA3DM_DRIVE_NONE) continue;   // the frontier voxel itself must be a reached member
            ++n_goals;
            if (goal_cost[t] < best) {
                best = goal_cost[t];
                goal = front[t];
            }
        }
        if (best == LA3DM_DRIVE_NONE) {
            std::printf("no goal on reachable ground (%llu frontier voxels)\n", (unsigned long long)n_front);
        } else {
            const auto ijk = [&](uint32_t f, uint32_t *c) {
                c[2] = f % dims[2];
                c[1] = (f / dims[2]) % dims[1];
                c[0] = f / (dims[2] * dims[1]);
            };
            uint32_t c[3];
            ijk(goal, c);
            std::printf("goal %u %u %u cost %u of %llu goals on reachable ground (%llu frontier voxels)\n", c[0], c[1], c[2], best,
                        (unsigned long long)n_goals, (unsigned long long)n_front);
            std::vector<uint32_t> route;   // from the goal back to the robot
            for (uint32_t f = goal; route.size() <= n; ) {
                route.push_back(f);
                const int q = parent[f];
                if (q == 40) break;   // the seeded member
                f = (uint32_t)((int64_t)f + ((int64_t)(q / 27 - 1) * dims[1] + ((q / 9) % 3 - 1)) * dims[2] + (q % 9 - 4));
            }
            std::printf("route %zu voxels:", route.size());
            for (size_t t = route.size(); t-- > 0;)
                if ((route.size() - 1 - t) % 8 == 0 || t == 0) {
                    ijk(route[t], c);
                    std::printf(" %u %u %u", c[0], c[1], c[2]);
                }
            std::printf("\n");
        }
        std::printf("ground_route %u x %u x %u from %g %g %g: mirror_syncs %llu device_resident %d\n", dims[0], dims[1], dims[2], info.origin[0],
                    info.origin[1], info.origin[2], (unsigned long long)map.mirror_syncs(), map.is_device_resident() ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
