// occupancy_grid.cpp — the 2-D occupancy grid / height map of a box round the robot, from the map the static node builds
// (examples/static_map.cpp's insert loop), answered by la3dm::BGKOctoMap::columns straight from the device pool: no host
// mirror is downloaded and the box itself is never built.
//
// An octree mapping server publishes, next to its markers, the map projected down the z axis: per (x, y) cell whether
// anything is occupied in a height band, whether the cell is known free, and how high the top occupied voxel is.
// columns(lo, dims) gives exactly that per column of the finest-layer lattice: the voxels per class (of the covering
// leaf, so collapsed regions count as what they are) and the lowest / highest occupied k.
//
//   occupancy_grid <dir> <prefix> <scan_num> [resolution block_depth sf2 ell free_res ds_res max_range
//                                             free_thresh occupied_thresh var_thresh prior_A prior_B]
// The box: 128 x 128 x 32 voxels whose voxel (0, 0, 0) holds the last sensor origin - (6.4, 6.4, 1.6).
// prints:  grid 128 x 128 x 32 from <origin of voxel 0>: occupied <n> free_only <n> unknown <n> top_occ_max <k> mirror_syncs <n> device_resident <0|1>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
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
        std::fprintf(stderr, "usage: %s dir prefix scan_num [resolution block_depth sf2 ell free_res ds_res max_range ...]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[2];
    const int scan_num = std::atoi(argv[3]);
    float v[12] = {0.1f, 3, 1.0f, 0.2f, 0.5f, 0.1f, 8.0f, 0.3f, 0.7f, 100.0f, 0.001f, 0.001f};  // bgkoctomap.yaml + sim_structured.yaml
    for (int i = 0; i < 12 && 4 + i < argc; ++i) v[i] = (float)std::atof(argv[4 + i]);
    try {
        la3dm::BGKOctoMap map(v[0], (unsigned short)v[1], v[2], v[3], v[7], v[8], v[9], v[10], v[11]);
        la3dm::point3f origin;
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
        const float lo[3] = {origin.x() - 6.4f, origin.y() - 6.4f, origin.z() - 1.6f};
        const size_t ncol = (size_t)dims[0] * dims[1];
        std::vector<uint32_t> counts(4 * ncol);
        std::vector<int32_t> top(ncol);
        la3dm_columns_out out;
        out.counts = counts.data();
        out.low_occ = nullptr;   // not asked for
        out.top_occ = top.data();
        la3dm_region_info info;
        map.columns(lo, dims, out, &info);
        // the three values of a nav_msgs/OccupancyGrid cell: occupied (100), free (0), unknown (-1)
        uint64_t occupied = 0, free_only = 0, unknown = 0;
        int32_t top_max = -1;
        for (size_t c = 0; c < ncol; ++c) {
            if (counts[4 * c + 1] > 0) ++occupied;
            else if (counts[4 * c] > 0) ++free_only;
            else ++unknown;
            top_max = std::max(top_max, top[c]);
        }
        std::printf("grid %u x %u x %u from %g %g %g: occupied %llu free_only %llu unknown %llu top_occ_max %d mirror_syncs %llu device_resident %d\n",
                    dims[0], dims[1], dims[2], info.origin[0], info.origin[1], info.origin[2], (unsigned long long)occupied,
                    (unsigned long long)free_only, (unsigned long long)unknown, (int)top_max,
                    (unsigned long long)map.mirror_syncs(), map.is_device_resident() ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
