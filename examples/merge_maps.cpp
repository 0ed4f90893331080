// merge_maps.cpp — two robots, one map: the scans of a sequence are split into two disjoint halves (odd and even scan
// numbers), each half builds a map of its own, the second map is packed and merged into the first, and the first is asked
// for the frontier of the same region before and after.
//
// merge() (contract: include/la3dm_hip.h, la3dm_devmap_merge_host) fuses the stream of the other map's covering leaves into
// the live pool on the GPU: per finest cell the incoming evidence is kept out (none), copied (this map had none) or added
// to this map's sums and the state re-derived; the blocks are pruned and new blocks appended.  Nothing is downloaded, no
// scan is inserted again.
//
//   merge_maps <dir> <prefix> <scan_num> [resolution block_depth sf2 ell free_res ds_res max_range
//                                         free_thresh occupied_thresh var_thresh prior_A prior_B device]
// device: the GPU (default 0); -1 = host-mode maps without a GPU (they cannot insert scans: scan_num 0, two empty maps).
// The box: 128 x 128 x 16 voxels whose voxel (0, 0, 0) holds the last sensor origin - (6.4, 6.4, 0.8); connectivity 6.
// prints:  merge_maps: <n> + <n> blocks -> <n> (<n> created); cells kept <n> copied <n> fused <n>; frontier <n> -> <n>;
//          mirror_syncs <n> device_resident <0|1>
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
    try {
        // two robots with the same map parameters; robot 0 takes the odd scans, robot 1 the even ones
        la3dm::BGKOctoMap mine(v[0], (unsigned short)v[1], v[2], v[3], v[7], v[8], v[9], v[10], v[11], (int)v[12]);
        la3dm::BGKOctoMap theirs(v[0], (unsigned short)v[1], v[2], v[3], v[7], v[8], v[9], v[10], v[11], (int)v[12]);
        la3dm::point3f origin(0, 0, 0);
        for (int scan_id = 1; scan_id <= scan_num; ++scan_id) {
            la3dm::BGKOctoMap::PointCloud cloud;
            const std::string filename = dir + "/" + prefix + "_" + std::to_string(scan_id) + ".pcd";
            if (!load_pcd(filename, origin, cloud)) {
                std::fprintf(stderr, "cannot read %s\n", filename.c_str());
                return 1;
            }
            (scan_id % 2 ? mine : theirs).insert_pointcloud(cloud, origin, v[5], v[4], v[6]);
        }
        const uint32_t dims[3] = {128, 128, 16};
        const float lo[3] = {origin.x() - 6.4f, origin.y() - 6.4f, origin.z() - 0.8f};
        const std::vector<uint32_t> before = frontier_list(mine, lo, dims);
        la3dm_pack_header h0, h1, h2;
        const std::vector<uint8_t> s0 = mine.pack(), s1 = theirs.pack();   // what robot 1 sends
        const la3dm_merge_stats st = mine.merge(s1.data(), s1.size());
        const std::vector<uint8_t> s2 = mine.pack();
        std::memcpy(&h0, s0.data(), sizeof(h0));
        std::memcpy(&h1, s1.data(), sizeof(h1));
        std::memcpy(&h2, s2.data(), sizeof(h2));
        const std::vector<uint32_t> after = frontier_list(mine, lo, dims);
        const bool ok = st.n_blocks == h1.n_blocks && h2.n_blocks == h0.n_blocks + st.n_created &&
                        st.cells_kept + st.cells_copied + st.cells_fused == (h1.n_blocks << (3u * (h1.block_depth - 1u)));
        std::printf("merge_maps: %llu + %llu blocks -> %llu (%llu created); cells kept %llu copied %llu fused %llu; frontier %zu -> %zu; "
                    "mirror_syncs %llu device_resident %d%s\n",
                    (unsigned long long)h0.n_blocks, (unsigned long long)h1.n_blocks, (unsigned long long)h2.n_blocks,
                    (unsigned long long)st.n_created, (unsigned long long)st.cells_kept, (unsigned long long)st.cells_copied,
                    (unsigned long long)st.cells_fused, before.size(), after.size(), (unsigned long long)mine.mirror_syncs(),
                    mine.is_device_resident() ? 1 : 0, ok ? "" : " INCONSISTENT");
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
