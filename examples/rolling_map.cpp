// rolling_map.cpp — the map as a rolling window: scans along a path go into a map that, after every scan, evicts every
// block outside a box round the sensor into a numbered file (evict_file: the stream is written and renamed before the first
// block leaves the pool), so the blocks held on the GPU stay bounded however long the drive.  At the end the files are merged
// back (merge_file) and the result is compared with a second map that took the same scans and never evicted: the block count
// and the frontier of a box round the last sensor origin.
//
// evict (contract: include/la3dm_hip.h, la3dm_devmap_pack_region_host) is pack_region, then erase_region of the same region:
// the selected blocks are compacted into a stream on the GPU, then the pool is compacted in place (the tail's survivors fill
// the holes) and the block table rebuilt.  merge creates the blocks the map lacks, which closes the loop.
//
//   rolling_map <dir> <prefix> <scan_num> <out_dir> [half_extent resolution block_depth sf2 ell free_res ds_res max_range
//                                                    free_thresh occupied_thresh var_thresh prior_A prior_B device]
// half_extent: half the side of the kept box in metres (default 4.0).  device: the GPU (default 0); -1 = host-mode maps without
// a GPU (they cannot insert scans: scan_num 0, two empty maps).
// prints one line per scan:  scan <i>: <n> blocks held, <n> evicted (<n> moved) to <file>; the whole map holds <n>
// and last:  rolling_map: held at most <n> of <n> blocks; <n> files merged back (<n> created) -> <n> blocks; frontier <n> vs <n>
//            equal <0|1>; device_resident <0|1>
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
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s dir prefix scan_num out_dir [half_extent resolution block_depth sf2 ell free_res ds_res max_range ... device]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[2], out_dir = argv[4];
    const int scan_num = std::atoi(argv[3]);
    float v[14] = {4.0f, 0.1f, 3, 1.0f, 0.2f, 0.5f, 0.1f, 8.0f, 0.3f, 0.7f, 100.0f, 0.001f, 0.001f, 0};  // half_extent, bgkoctomap.yaml + sim_structured.yaml, device
    for (int i = 0; i < 14 && 5 + i < argc; ++i) v[i] = (float)std::atof(argv[5 + i]);
    try {
        la3dm::BGKOctoMap rolling(v[1], (unsigned short)v[2], v[3], v[4], v[8], v[9], v[10], v[11], v[12], (int)v[13]);
        la3dm::BGKOctoMap whole(v[1], (unsigned short)v[2], v[3], v[4], v[8], v[9], v[10], v[11], v[12], (int)v[13]);
        la3dm::point3f origin(0, 0, 0);
        std::vector<std::string> files;
        size_t most_held = 0;
        for (int scan_id = 1; scan_id <= scan_num; ++scan_id) {
            la3dm::BGKOctoMap::PointCloud cloud;
            const std::string filename = dir + "/" + prefix + "_" + std::to_string(scan_id) + ".pcd";
            if (!load_pcd(filename, origin, cloud)) {
                std::fprintf(stderr, "cannot read %s\n", filename.c_str());
                return 1;
            }
            rolling.insert_pointcloud(cloud, origin, v[6], v[5], v[7]);
            whole.insert_pointcloud(cloud, origin, v[6], v[5], v[7]);
            // everything but the box round the sensor leaves the map for a file of its own
            const float lo[3] = {origin.x() - v[0], origin.y() - v[0], origin.z() - v[0]};
            const float hi[3] = {origin.x() + v[0], origin.y() + v[0], origin.z() + v[0]};
            const std::string file = out_dir + "/evicted_" + std::to_string(scan_id) + ".la3dm";
            const la3dm_erase_stats st = rolling.evict_file(file, lo, hi, false);
            files.push_back(file);
            most_held = std::max<size_t>(most_held, (size_t)st.n_blocks);
            std::printf("scan %d: %llu blocks held, %llu evicted (%llu moved) to %s; the whole map holds %zu\n", scan_id,
                        (unsigned long long)st.n_blocks, (unsigned long long)st.n_removed, (unsigned long long)st.n_moved, file.c_str(),
                        whole.block_count());
        }
        uint64_t created = 0;
        for (const std::string &file : files) created += rolling.merge_file(file).n_created;
        const uint32_t dims[3] = {128, 128, 16};
        const float lo[3] = {origin.x() - 6.4f, origin.y() - 6.4f, origin.z() - 0.8f};
        const std::vector<uint32_t> a = frontier_list(rolling, lo, dims), b = frontier_list(whole, lo, dims);
        const size_t n_rolling = rolling.block_count(), n_whole = whole.block_count();
        const bool equal = a == b;
        std::printf("rolling_map: held at most %zu of %zu blocks; %zu files merged back (%llu created) -> %zu blocks; frontier %zu vs %zu "
                    "equal %d; device_resident %d\n",
                    most_held, n_whole, files.size(), (unsigned long long)created, n_rolling, a.size(), b.size(), equal ? 1 : 0,
                    rolling.is_device_resident() ? 1 : 0);
        return n_rolling == n_whole && equal ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
