// ground_goals.cpp — the exploration goals a ground robot can use: la3dm::BGKOctoMap::footing round the sensor says where
// the robot can stand (ground below, headroom above, a footprint that is carried and not blocked), clusters over footing's
// list joins the standing places into patches the robot can drive across (connectivity 26: one step sideways and at most one
// voxel up or down), the patch under the sensor is the ground it stands on, and the frontier voxels (examples/frontier.cpp)
// that are foot voxels of that patch are the goals it can reach on the ground; those on any patch are the goals it could
// use once the ground in between has been seen.  On a device-resident map everything is answered from the device pool: no
// host mirror is downloaded, no class array is fetched, no stencil runs on the CPU.
//
// The clear mask is optimistic (FREE | UNKNOWN | MISSING): space nobody has seen does not block the body.  min_support = N
// asks for ground under every cell of the footprint, N / 2 tolerates the holes of a sparsely observed floor, 0 asks only
// for an unobstructed body; the example prints all three.
//
//   ground_goals <dir> <prefix> <scan_num> [resolution block_depth sf2 ell free_res ds_res max_range
//                                           free_thresh occupied_thresh var_thresh prior_A prior_B device]
// device: the GPU (default 0); -1 = a host-mode map without a GPU (it cannot insert scans: scan_num 0, the empty map).
// The box: 128 x 128 x 32 voxels whose voxel (0, 0, 0) holds the last sensor origin - (6.4, 6.4, 2.0).
// prints:  support <c> of <N>: stand <n> body <n> foot <n> patches <n> patch <size | none> goals <n> on any patch <n>
//          for c = N, N / 2, 0: the voxels that pass each condition, the patches, the size of the patch under the sensor, the
//          frontier voxels that are foot voxels of that patch and of any patch
//          ground_goals 128 x 128 x 32 from <origin of voxel 0>: frontier <n> mirror_syncs <n> device_resident <0|1>
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
        // the sensor's voxel
        uint32_t s[3];
        const float o3[3] = {origin.x(), origin.y(), origin.z()};
        for (int a = 0; a < 3; ++a) {
            const long c = std::lround((o3[a] - info.origin[a]) / res);
            s[a] = (uint32_t)std::max(0l, std::min(c, (long)dims[a] - 1));
        }
        la3dm_footing_params fp;
        fp.support_mask = occupied;
        fp.clear_mask = free_mask | unseen;
        fp.headroom = 4;   // a body 0.4 m tall
        fp.radius = 2;     // ... and 0.5 m wide
        fp.step = 1;       // ... that climbs one voxel
        la3dm_footing_stats fs;
        std::memset(&fs, 0, sizeof(fs));
        uint64_t n_foot = 0;
        la3dm_footing_out none;
        std::memset(&none, 0, sizeof(none));
        fp.min_support = 0;
        map.footing(lo, dims, &fp, 0, none, &n_foot, &fs, nullptr);   // N, by a count-only call
        const uint32_t N = fs.disc_cells;
        std::vector<uint32_t> label(n);
        const uint32_t supports[3] = {N, N / 2, 0};
        for (const uint32_t c : supports) {
            fp.min_support = c;
            map.footing(lo, dims, &fp, 0, none, &n_foot, &fs, nullptr);   // count
            std::vector<uint32_t> foot(n_foot);
            if (n_foot) {
                la3dm_footing_out out = none;
                out.index = foot.data();
                map.footing(lo, dims, &fp, n_foot, out, &n_foot, &fs, nullptr);
            }
            // the patches: standing places one step apart, at most one voxel up or down
            la3dm_clusters_params cp;
            std::memset(&cp, 0, sizeof(cp));
            cp.member_mask = fp.clear_mask;   // (a foot voxel's class is in the clear mask by definition)
            cp.from_list = 1;
            cp.connectivity = 26;
            cp.min_size = 1;
            cp.members = foot.data();
            cp.n_members = (uint32_t)foot.size();
            uint32_t n_patches = 0;
            la3dm_clusters_stats cs;
            std::memset(&cs, 0, sizeof(cs));
            la3dm_clusters_out co;
            std::memset(&co, 0, sizeof(co));
            co.label = label.data();
            map.clusters(lo, dims, cp, &co, &n_patches, &cs, nullptr);
            // the patch under the sensor: the patch of the foot voxel nearest the sensor's voxel (the first of equals)
            uint32_t patch = LA3DM_CLUSTERS_NONE;
            uint64_t best = std::numeric_limits<uint64_t>::max();
            for (const uint32_t f : foot) {
                const uint32_t k = f % dims[2], j = (f / dims[2]) % dims[1], i = f / (dims[2] * dims[1]);
                const int64_t di = (int64_t)i - s[0], dj = (int64_t)j - s[1], dk = (int64_t)k - s[2];
                const uint64_t d = (uint64_t)(di * di + dj * dj + dk * dk);
                if (d < best) {
                    best = d;
                    patch = label[f];
                }
            }
            uint64_t patch_size = 0, goals = 0, goals_any = 0;
            for (const uint32_t f : front) goals_any += label[f] != LA3DM_CLUSTERS_NONE ? 1u : 0u;   // (a non-member's label is NONE)
            if (patch != LA3DM_CLUSTERS_NONE) {
                for (const uint32_t f : foot) patch_size += label[f] == patch ? 1u : 0u;
                for (const uint32_t f : front) goals += label[f] == patch ? 1u : 0u;
            }
            std::printf("support %u of %u: stand %u body %u foot %llu patches %u patch ", c, N, fs.n_stand, fs.n_body, (unsigned long long)n_foot,
                        n_patches);
            if (patch != LA3DM_CLUSTERS_NONE)
                std::printf("%llu", (unsigned long long)patch_size);
            else
                std::printf("none");
            std::printf(" goals %llu on any patch %llu\n", (unsigned long long)goals, (unsigned long long)goals_any);
        }
        std::printf("ground_goals %u x %u x %u from %g %g %g: frontier %llu mirror_syncs %llu device_resident %d\n", dims[0], dims[1], dims[2],
                    info.origin[0], info.origin[1], info.origin[2], (unsigned long long)n_front, (unsigned long long)map.mirror_syncs(),
                    map.is_device_resident() ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
