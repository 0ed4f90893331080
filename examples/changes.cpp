// changes.cpp — what changed: a publisher that sends the cells a few scans changed instead of the whole map.  The first
// half of a sequence is inserted and the map packed (the snapshot a subscriber holds); the second half is inserted and the
// live map is compared with the snapshot.
//
// diff() (contract: include/la3dm_hip.h, la3dm_devmap_diff_host) compares the live pool with the stream on the GPU: per
// finest cell of every block either side holds, the class then and the class now; the selected cells come back as a list
// (block key, cell, then | now << 4, centre) and every (then, now) pair is counted.  Nothing is downloaded and the map is
// not changed.  Then the map is compared with its own fresh pack: no cell differs.
//
//   changes <dir> <prefix> <scan_num> [resolution block_depth sf2 ell free_res ds_res max_range
//                                      free_thresh occupied_thresh var_thresh prior_A prior_B device]
// device: the GPU (default 0); -1 = a host-mode map without a GPU (it cannot insert scans: scan_num 0, an empty map).
// prints:  changes: <n> -> <n> blocks; cells newly occupied <n> no longer occupied <n> newly observed <n> changed <n>;
//          self diff <n>; mirror_syncs <n> device_resident <0|1>
//          then up to five lines "  newly occupied at x y z"
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
        std::fprintf(stderr, "usage: %s dir prefix scan_num [resolution block_depth sf2 ell free_res ds_res max_range ... device]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[2];
    const int scan_num = std::atoi(argv[3]);
    float v[13] = {0.1f, 3, 1.0f, 0.2f, 0.5f, 0.1f, 8.0f, 0.3f, 0.7f, 100.0f, 0.001f, 0.001f, 0};  // bgkoctomap.yaml + sim_structured.yaml, device
    for (int i = 0; i < 13 && 4 + i < argc; ++i) v[i] = (float)std::atof(argv[4 + i]);
    try {
        la3dm::BGKOctoMap map(v[0], (unsigned short)v[1], v[2], v[3], v[7], v[8], v[9], v[10], v[11], (int)v[12]);
        std::vector<uint8_t> snapshot = map.pack();
        for (int scan_id = 1; scan_id <= scan_num; ++scan_id) {
            la3dm::BGKOctoMap::PointCloud cloud;
            la3dm::point3f origin(0, 0, 0);
            const std::string filename = dir + "/" + prefix + "_" + std::to_string(scan_id) + ".pcd";
            if (!load_pcd(filename, origin, cloud)) {
                std::fprintf(stderr, "cannot read %s\n", filename.c_str());
                return 1;
            }
            map.insert_pointcloud(cloud, origin, v[5], v[4], v[6]);
            if (scan_id == scan_num / 2) snapshot = map.pack();   // what the subscriber holds
        }
        la3dm_pack_header then;
        std::memcpy(&then, snapshot.data(), sizeof(then));
        // every changed pair is counted; listed are the cells that became OCCUPIED (class 1) from any other class
        const auto pair = [](uint32_t t, uint32_t n) { return 1u << (5u * t + n); };
        la3dm_diff_params p;
        p.pair_mask = pair(0, 1) | pair(2, 1) | pair(3, 1);
        p.value_mask = 0;
        p.map_only = 1;
        la3dm_diff_stats st;
        uint64_t found = 0;
        map.diff(snapshot.data(), snapshot.size(), p, 0, nullptr, &found, &st);   // count, then fill
        std::vector<float> centre(3 * found);
        la3dm_diff_out out;
        std::memset(&out, 0, sizeof(out));
        out.centre = centre.data();
        if (found) map.diff(snapshot.data(), snapshot.size(), p, found, &out, &found, nullptr);
        uint64_t newly_occupied = 0, no_longer = 0, newly_observed = 0, changed = 0;
        for (uint32_t t = 0; t < 5; ++t)
            for (uint32_t n = 0; n < 5; ++n) {
                const uint64_t cells = st.pairs[5 * t + n];
                if (t != n) changed += cells;
                if (n == 1 && t != 1) newly_occupied += cells;
                if (t == 1 && n != 1) no_longer += cells;
                if ((t == 2 || t == 3) && n <= 1) newly_observed += cells;
            }
        // the map against its own fresh pack: every pair on the diagonal
        const std::vector<uint8_t> fresh = map.pack();
        la3dm_pack_header now;
        std::memcpy(&now, fresh.data(), sizeof(now));
        p.pair_mask = LA3DM_DIFF_PAIRS_CHANGED;
        p.value_mask = 0x1Fu;
        uint64_t self = 0;
        map.diff(fresh.data(), fresh.size(), p, 0, nullptr, &self, nullptr);
        const bool ok = found == newly_occupied && self == 0 && st.n_stream_blocks == then.n_blocks &&
                        st.n_stream_blocks + st.n_map_only_blocks == now.n_blocks + st.n_missing_now;
        std::printf("changes: %llu -> %llu blocks; cells newly occupied %llu no longer occupied %llu newly observed %llu changed %llu; "
                    "self diff %llu; mirror_syncs %llu device_resident %d%s\n",
                    (unsigned long long)then.n_blocks, (unsigned long long)now.n_blocks, (unsigned long long)newly_occupied,
                    (unsigned long long)no_longer, (unsigned long long)newly_observed, (unsigned long long)changed, (unsigned long long)self,
                    (unsigned long long)map.mirror_syncs(), map.is_device_resident() ? 1 : 0, ok ? "" : " INCONSISTENT");
        for (uint64_t t = 0; t < std::min<uint64_t>(found, 5); ++t)
            std::printf("  newly occupied at %.3f %.3f %.3f\n", centre[3 * t], centre[3 * t + 1], centre[3 * t + 2]);
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
