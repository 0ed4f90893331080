// resume_map.cpp — a map that outlives its process: build the map the static node builds (examples/static_map.cpp's insert
// loop), save() it, load() the file into a second object and ask both for the frontier of the same region.
//
// save() writes the compact stream of the map's covering leaves (layout: include/la3dm_hip.h, la3dm_devmap_pack_host): a
// device-resident map compacts its pool on the GPU before anything crosses PCIe, and load() expands the stream on the GPU
// again — no scan is re-inserted, no host mirror is downloaded.  What does not travel: the last scan's training data, the
// statistics, the options and the shard configuration.
//
//   resume_map <dir> <prefix> <scan_num> [resolution block_depth sf2 ell free_res ds_res max_range
//                                         free_thresh occupied_thresh var_thresh prior_A prior_B device [file]]
// device: the GPU (default 0); -1 = a host-mode map without a GPU (it cannot insert scans: scan_num 0, the empty map).
// file: where the map is saved (default resume_map.la3dm in the working directory; removed afterwards).
// The box: 128 x 128 x 16 voxels whose voxel (0, 0, 0) holds the last sensor origin - (6.4, 6.4, 0.8); connectivity 6.
// prints:  resume_map: <n> blocks, stream <n> bytes, raw pool <n> bytes; frontier <n> / <n>: lists agree|DIFFER;
//          mirror_syncs <n> <n> device_resident <0|1>
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

// the frontier list of the region: FREE voxels with an UNKNOWN or MISSING face neighbour (count, then fill)
static std::vector<uint32_t> frontier_list(const la3dm::BGKOctoMap &map, const float *lo, const uint32_t *dims) {
    const uint32_t open = 1u << 0, unknown = (1u << 2) | (1u << 3);
    uint64_t found = 0;
    la3dm_frontier_out out;
    out.index = nullptr;
    out.nbrs = nullptr;
    out.score = nullptr;
    map.frontier(lo, dims, open, unknown, 6, 1, 0, out, &found, nullptr);
    std::vector<uint32_t> index(found);
    if (found) {
        out.index = index.data();
        map.frontier(lo, dims, open, unknown, 6, 1, found, out, &found, nullptr);
    }
    return index;
}

int main(int argc, char **argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s dir prefix scan_num [resolution block_depth sf2 ell free_res ds_res max_range ... device [file]]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[2];
    const int scan_num = std::atoi(argv[3]);
    float v[13] = {0.1f, 3, 1.0f, 0.2f, 0.5f, 0.1f, 8.0f, 0.3f, 0.7f, 100.0f, 0.001f, 0.001f, 0};  // bgkoctomap.yaml + sim_structured.yaml, device
    for (int i = 0; i < 13 && 4 + i < argc; ++i) v[i] = (float)std::atof(argv[4 + i]);
    const std::string file = argc > 17 ? argv[17] : "resume_map.la3dm";
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
        map.save(file);
        // "tomorrow": a second object with the same parameters (la3dm_amd.load_map reads them from the file's header)
        la3dm::BGKOctoMap again(v[0], (unsigned short)v[1], v[2], v[3], v[7], v[8], v[9], v[10], v[11], (int)v[12]);
        again.load(file);
        const std::vector<uint8_t> stream = again.pack();
        la3dm_pack_header h;
        std::memcpy(&h, stream.data(), sizeof(h));
        std::remove(file.c_str());
        const uint32_t dims[3] = {128, 128, 16};
        const float lo[3] = {origin.x() - 6.4f, origin.y() - 6.4f, origin.z() - 0.8f};
        const std::vector<uint32_t> a = frontier_list(map, lo, dims), b = frontier_list(again, lo, dims);
        const bool agree = a == b && stream == map.pack();
        std::printf("resume_map: %llu blocks, stream %llu bytes, raw pool %llu bytes; frontier %zu / %zu: lists %s; mirror_syncs %llu %llu "
                    "device_resident %d\n",
                    (unsigned long long)h.n_blocks, (unsigned long long)h.total_bytes,
                    (unsigned long long)(h.n_blocks * (8ull + 9ull * h.nodes_per_block)), a.size(), b.size(), agree ? "agree" : "DIFFER",
                    (unsigned long long)map.mirror_syncs(), (unsigned long long)again.mirror_syncs(), again.is_device_resident() ? 1 : 0);
        return agree ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
