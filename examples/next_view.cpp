// next_view.cpp — which exploration goal to drive to: the frontier voxels round the robot that are far enough from obstacles,
// scored by how much unobserved space a sensor placed there would see, from the map the static node builds
// (examples/static_map.cpp's insert loop).  Three queries on the device pool, no host mirror, no class array downloaded:
//
//   frontier        the goals: FREE voxels with an UNKNOWN or MISSING face neighbour (examples/frontier.cpp);
//   distance_field  their clearance to the nearest OCCUPIED voxel: goals closer than the robot radius are dropped;
//   gain            per kept candidate the number of DISTINCT UNKNOWN or MISSING voxels of the box that a fixed fan of
//                   rays from it walks over before an OCCUPIED voxel stops them — the expected information gain of a
//                   next-best-view planner.  Summing raycast_many's per-ray counts instead would count the voxels near
//                   the viewpoint once per ray.
//
//   next_view <dir> <prefix> <scan_num> [resolution block_depth sf2 ell free_res ds_res max_range
//                                        free_thresh occupied_thresh var_thresh prior_A prior_B device]
// device: the GPU (default 0); -1 = a host-mode map without a GPU (it cannot insert scans: scan_num 0, the empty map).
// The box: 128 x 128 x 16 voxels whose voxel (0, 0, 0) holds the last sensor origin - (6.4, 6.4, 0.8); connectivity 6,
// min_neighbours 1; clearance radius 8 voxels; robot radius 0.3 m.  Candidates: every s-th kept goal in ascending order
// of the flat index, s = ceil(kept / 512).  The fan: 384 offsets on the surface of a cube of half side 3 m, 8 x 8 per
// face at (-2.625 + 0.75 i, -2.625 + 0.75 j) — every coordinate exact in fp32, so any client reproduces it.
// prints:  best <x> <y> <z> index <flat index> gain <n>       the candidate with the largest gain (the first of equals)
//          next_view 128 x 128 x 16 from <origin of voxel 0>: found <n> kept <n> candidates <n> sum_gain <n>
//                    mirror_syncs <n> device_resident <0|1>
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
        const uint32_t dims[3] = {128, 128, 16}, radius = 8;
        const float lo[3] = {origin.x() - 6.4f, origin.y() - 6.4f, origin.z() - 0.8f};
        const float robot_radius = 0.3f, res = v[0];
        const uint32_t free_m = 1u << 0, occupied_m = 1u << 1, unseen_m = (1u << 2) | (1u << 3);   // UNKNOWN | MISSING
        // ---- the goals (examples/frontier.cpp)
        la3dm_region_info info;
        uint64_t found = 0;
        la3dm_frontier_out fo;
        fo.index = nullptr;
        fo.nbrs = nullptr;
        fo.score = nullptr;
        map.frontier(lo, dims, free_m, unseen_m, 6, 1, 0, fo, &found, &info);   // count
        std::vector<uint32_t> index(found);
        if (found) {
            fo.index = index.data();
            map.frontier(lo, dims, free_m, unseen_m, 6, 1, found, fo, &found, nullptr);
        }
        // ---- the ones a robot can stand on
        std::vector<float> clearance((size_t)dims[0] * dims[1] * dims[2]);
        la3dm_distance_out df;
        df.d2 = nullptr;
        df.dist = clearance.data();
        map.distance_field(lo, dims, occupied_m, radius, df, nullptr);
        std::vector<uint32_t> kept;
        for (size_t t = 0; t < index.size(); ++t)
            if (!(clearance[index[t]] < robot_radius)) kept.push_back(index[t]);
        const size_t stride = (kept.size() + 511) / 512;
        std::vector<uint32_t> cand;
        for (size_t t = 0; t < kept.size(); t += stride) cand.push_back(kept[t]);
        std::vector<float> origins(3 * cand.size());
        for (size_t t = 0; t < cand.size(); ++t) {
            const uint32_t f = cand[t], k = f % dims[2], j = (f / dims[2]) % dims[1], i = f / (dims[2] * dims[1]);
            origins[3 * t] = info.origin[0] + (float)i * res;
            origins[3 * t + 1] = info.origin[1] + (float)j * res;
            origins[3 * t + 2] = info.origin[2] + (float)k * res;
        }
        // ---- the fan
        std::vector<float> offsets;
        for (int axis = 0; axis < 3; ++axis)
            for (int side = -1; side <= 1; side += 2)
                for (int i = 0; i < 8; ++i)
                    for (int j = 0; j < 8; ++j) {
                        float p[3];
                        p[axis] = 3.0f * (float)side;
                        p[(axis + 1) % 3] = -2.625f + 0.75f * (float)i;
                        p[(axis + 2) % 3] = -2.625f + 0.75f * (float)j;
                        offsets.insert(offsets.end(), p, p + 3);
                    }
        // ---- the score
        std::vector<uint32_t> gain(cand.size());
        la3dm_gain_out go;
        go.gain = gain.data();
        go.started = nullptr;
        go.hits = nullptr;
        go.seen = nullptr;
        map.gain(lo, dims, origins.data(), (uint32_t)cand.size(), offsets.data(), (uint32_t)(offsets.size() / 3), unseen_m, occupied_m,
                 4096, go, nullptr);
        unsigned long long sum = 0;
        size_t best = 0;
        for (size_t t = 0; t < cand.size(); ++t) {
            sum += gain[t];
            if (gain[t] > gain[best]) best = t;
        }
        if (!cand.empty())
            std::printf("best %g %g %g index %u gain %u\n", origins[3 * best], origins[3 * best + 1], origins[3 * best + 2], cand[best], gain[best]);
        std::printf("next_view %u x %u x %u from %g %g %g: found %llu kept %llu candidates %llu sum_gain %llu mirror_syncs %llu device_resident %d\n",
                    dims[0], dims[1], dims[2], info.origin[0], info.origin[1], info.origin[2], (unsigned long long)found,
                    (unsigned long long)kept.size(), (unsigned long long)cand.size(), sum, (unsigned long long)map.mirror_syncs(),
                    map.is_device_resident() ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
