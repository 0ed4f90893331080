// raycast.cpp — ray queries on the map the static node builds (examples/static_map.cpp's insert loop), answered by
// la3dm::BGKOctoMap::raycast_many straight from the device pool: no host mirror is downloaded.
//
// The reference's static node keeps a ray test as a comment (src/bgkloctomap/bgkloctomap_static_node.cpp:119-131): a RayCaster
// from (1, 1, 0.3) to (6, 7, 8) whose rows a client inspects one by one.  Here that ray and a fan of 4 096 rays from
// the last sensor origin go through raycast_many, which drives the same walk per ray, stops at the first OCCUPIED
// covering leaf (a collapsed region's raw voxels read PRUNED; the covering leaf is where their answer lives) and
// reports the last row and the rows per class.
//
//   raycast <dir> <prefix> <scan_num> [resolution block_depth sf2 ell free_res ds_res max_range
//                                      free_thresh occupied_thresh var_thresh prior_A prior_B]
// prints:  ray (1, 1, 0.3) -> (6, 7, 8): steps <n> flags <f> cls <c> leaf_depth <d> at <x y z> rows free <n> occupied <n> unknown <n> missing <n>
//          fan 4096 rays from <origin>: hits <n> total_steps <n> unknown_or_missing_rows <n> mirror_syncs <n>
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

// The fan: a 64 x 16 grid on each of the four vertical faces of a box round the origin, 8 m to a face.  Every offset
// is a binary fraction, so the end points are the same floats wherever they are computed.
static void fan_rays(const la3dm::point3f &o, std::vector<float> &rays6) {
    rays6.resize(6 * 4096);
    for (int i = 0; i < 4096; ++i) {
        const int a = i & 63, b = (i >> 6) & 15, f = i >> 10;
        const float u = ((float)a - 31.5f) * 0.25f, w = ((float)b - 7.5f) * 0.25f;
        const float dx = f == 0 ? 8.0f : (f == 1 ? -8.0f : u), dy = f == 2 ? 8.0f : (f == 3 ? -8.0f : u);
        float *r = &rays6[6 * (size_t)i];
        r[0] = o.x(); r[1] = o.y(); r[2] = o.z();
        r[3] = o.x() + dx; r[4] = o.y() + dy; r[5] = o.z() + w;
    }
}

struct RayResults {
    std::vector<uint32_t> steps, counts;
    std::vector<uint8_t> flags, cls, leaf_depth;
    std::vector<float> p;
    la3dm_raycast_out out;
    explicit RayResults(size_t n) : steps(n), counts(4 * n), flags(n), cls(n), leaf_depth(n), p(3 * n) {
        std::memset(&out, 0, sizeof(out));   // block_key, node_key, A, B are not asked for
        out.steps = steps.data();
        out.flags = flags.data();
        out.p = p.data();
        out.cls = cls.data();
        out.leaf_depth = leaf_depth.data();
        out.counts = counts.data();
    }
};

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
        const uint32_t stop = 1u << (unsigned)la3dm::State::OCCUPIED, max_steps = 4096;
        const float one[6] = {1.0f, 1.0f, 0.3f, 6.0f, 7.0f, 8.0f};
        RayResults r1(1);
        map.raycast_many(one, 1, stop, max_steps, r1.out);
        std::printf("ray (1, 1, 0.3) -> (6, 7, 8): steps %u flags %u cls %u leaf_depth %u at %g %g %g rows free %u occupied %u unknown %u missing %u\n",
                    r1.steps[0], (unsigned)r1.flags[0], (unsigned)r1.cls[0], (unsigned)r1.leaf_depth[0], r1.p[0], r1.p[1], r1.p[2],
                    r1.counts[0], r1.counts[1], r1.counts[2], r1.counts[3]);
        std::vector<float> rays;
        fan_rays(origin, rays);
        RayResults rf(4096);
        map.raycast_many(rays.data(), 4096, stop, max_steps, rf.out);
        uint64_t hits = 0, total = 0, unseen = 0;
        for (size_t i = 0; i < 4096; ++i) {
            hits += (rf.flags[i] & LA3DM_RAY_HIT) != 0;
            total += rf.steps[i];
            unseen += rf.counts[4 * i + 2] + rf.counts[4 * i + 3];
        }
        std::printf("fan 4096 rays from %g %g %g: hits %llu total_steps %llu unknown_or_missing_rows %llu mirror_syncs %llu device_resident %d\n",
                    origin.x(), origin.y(), origin.z(), (unsigned long long)hits, (unsigned long long)total,
                    (unsigned long long)unseen, (unsigned long long)map.mirror_syncs(), map.is_device_resident() ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
