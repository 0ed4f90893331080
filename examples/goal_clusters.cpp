// goal_clusters.cpp — where the exploration goals are, one voxel each: the frontier of a height band round the robot
// (examples/frontier.cpp), the goals kept that lie farther than 2 voxels from every obstacle (distance_field),
// la3dm::BGKOctoMap::clusters over the kept list, and the clusters' representatives as the targets of travel
// (examples/route.cpp).  On a device-resident map everything is answered from the device pool: no host mirror is
// downloaded, no class array is fetched, no labelling runs on the CPU.
//
// Untiled, the frontier of a room is one sheet and plain connected components answer "is this set connected".  Confined
// to tiles of 8 voxels, with connectivity 26 and at least 8 members, the clusters are the goals: each has a bounded
// extent, and rep[c] — the member nearest the cluster's rounded centroid — is a voxel to drive to or look from.
//
//   goal_clusters <dir> <prefix> <scan_num> [resolution block_depth sf2 ell free_res ds_res max_range
//                                            free_thresh occupied_thresh var_thresh prior_A prior_B device]
// device: the GPU (default 0); -1 = a host-mode map without a GPU (it cannot insert scans: scan_num 0, the empty map).
// The box: 128 x 128 x 16 voxels whose voxel (0, 0, 0) holds the last sensor origin - (6.4, 6.4, 0.8).
// prints:  cluster <c> size <n> rep <x> <y> <z> cost <n | none>     the (at most) five reachable clusters with the least cost
//          goal_clusters 128 x 128 x 16 from <origin of voxel 0>: found <n> kept <n> clusters <n> dropped <n> largest <n>
//                                          reachable <n> mirror_syncs <n> device_resident <0|1>
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
        // the goals farther than 2 voxels from every obstacle of the region
        const uint32_t keep_off = 2;
        std::vector<uint32_t> d2(n), kept;
        la3dm_distance_out dd;
        dd.d2 = d2.data();
        dd.dist = nullptr;
        map.distance_field(lo, dims, occupied, keep_off, dd, nullptr);
        for (uint32_t f : index)
            if (d2[f] == LA3DM_DF_FAR) kept.push_back(f);
        // the clusters of the kept goals: count, then fetch the records
        la3dm_clusters_params cp;
        std::memset(&cp, 0, sizeof(cp));
        cp.member_mask = free_mask;
        cp.from_list = 1;
        cp.connectivity = 26;
        cp.tile = 8;
        cp.min_size = 8;
        cp.members = kept.data();
        cp.n_members = (uint32_t)kept.size();
        uint32_t n_clusters = 0;
        la3dm_clusters_stats cs;
        std::memset(&cs, 0, sizeof(cs));
        map.clusters(lo, dims, cp, nullptr, &n_clusters, &cs, nullptr);
        std::vector<uint32_t> size(n_clusters), rep(n_clusters), cost(n_clusters);
        if (n_clusters) {
            la3dm_clusters_out co;
            std::memset(&co, 0, sizeof(co));
            co.size = size.data();
            co.rep = rep.data();
            cp.cap = n_clusters;
            map.clusters(lo, dims, cp, &co, &n_clusters, &cs, nullptr);
        }
        // the representatives as the targets of travel from the sensor's voxel
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
        if (n_clusters) {   // (without a goal there is nothing to ask)
            la3dm_travel_out to;
            to.cost = nullptr;
            to.target_cost = cost.data();
            to.parent = nullptr;
            map.travel(lo, dims, &seed, 1, tp, rep.data(), n_clusters, to, nullptr, nullptr);
        }
        struct Goal {
            uint32_t cost, c;
        };
        std::vector<Goal> goals;
        for (uint32_t c = 0; c < n_clusters; ++c)
            if (cost[c] != LA3DM_TRAVEL_NONE) goals.push_back(Goal{cost[c], c});
        std::stable_sort(goals.begin(), goals.end(), [](const Goal &a, const Goal &b) { return a.cost < b.cost; });
        for (size_t t = 0; t < goals.size() && t < 5; ++t) {
            const uint32_t c = goals[t].c, f = rep[c], k = f % dims[2], j = (f / dims[2]) % dims[1], i = f / (dims[2] * dims[1]);
            std::printf("cluster %u size %u rep %g %g %g cost %u\n", c, size[c], info.origin[0] + (float)i * res, info.origin[1] + (float)j * res,
                        info.origin[2] + (float)k * res, goals[t].cost);
        }
        std::printf("goal_clusters %u x %u x %u from %g %g %g: found %llu kept %llu clusters %u dropped %u largest %u reachable %llu mirror_syncs %llu device_resident %d\n",
                    dims[0], dims[1], dims[2], info.origin[0], info.origin[1], info.origin[2], (unsigned long long)found,
                    (unsigned long long)kept.size(), n_clusters, cs.n_dropped, cs.largest, (unsigned long long)goals.size(),
                    (unsigned long long)map.mirror_syncs(), map.is_device_resident() ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
