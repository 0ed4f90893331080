// drive_cells.h — the pure part of drive (contract: include/la3dm_hip.h, la3dm_devmap_drive_host): the member set of a
// region, the seeds and the targets go in; the least costs, the parents and the answers at the targets come out.  The host
// form (BGKOctoMap::drive, host/bgkoctomap.cpp) builds the member bytes — from the list, or from its own footing — and
// calls `cells`: that is the definition, and the device kernels (csrc/devmap_drive.h) reproduce it exactly.  std only;
// compiles alone (tools/check/drive_cells.cpp drives it under ASan and UBSan).
//
// Dijkstra with a binary heap over the members — a candidate above max_cost is dropped where it is made, which changes no
// cost <= max_cost because every prefix of a least-cost walk is no dearer than the walk —, then one pass over the voxels
// for the parents, which are a function of the costs and the member set alone.
#ifndef LA3DM_DRIVE_CELLS_H
#define LA3DM_DRIVE_CELLS_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

namespace la3dm_drive {

constexpr uint32_t kNone = 0xFFFFFFFFu;   // LA3DM_DRIVE_NONE
constexpr int kMaxStep = 4;               // LA3DM_DRIVE_MAX_STEP

struct Params {   // la3dm_drive_params without its pointers, field by field
    uint32_t connectivity, step, snap, move_cost[2], climb_up, climb_down, max_cost;
};

struct Counts {
    uint32_t n_members, n_seeded, n_reached, max_cost;
};

// is the offset (a, b, c) a move?
inline bool allowed(const Params &p, int a, int b, int c) {
    const int flat = (a ? 1 : 0) + (b ? 1 : 0);
    return flat >= 1 && flat <= (p.connectivity == 4 ? 1 : 2) && c >= -(int)p.step && c <= (int)p.step;
}

// what the allowed move along (a, b, c) costs: <= 2^16 + 4 * 2^16
inline uint32_t move(const Params &p, int a, int b, int c) {
    return p.move_cost[(a ? 1 : 0) + (b ? 1 : 0) - 1] + (c > 0 ? p.climb_up * (uint32_t)c : p.climb_down * (uint32_t)(-c));
}

// the code of the offset o = u - v
inline uint8_t code(int oi, int oj, int ok) { return (uint8_t)(((oi + 1) * 3 + (oj + 1)) * 9 + (ok + kMaxStep)); }

// the member that flat index f stands for: (i, j, k') with the largest k' in [max(0, k - snap), k]; kNone where f is out of
// range or there is none
inline uint32_t snapped(const uint32_t dims[3], const uint8_t *member, uint32_t snap, uint32_t f) {
    const uint64_t n = (uint64_t)dims[0] * dims[1] * dims[2];
    if (f >= n) return kNone;
    const uint32_t k = f % dims[2], low = k > snap ? k - snap : 0u;
    for (uint32_t t = 0; t <= k - low; ++t)
        if (member[f - t]) return f - t;
    return kNone;
}

// member: one byte per voxel of the region, non-zero = member.  cost, parent (dense), of_member [n_list] (the cost at
// list[t], kNone for an entry >= nx ny nz), target_cost and target_index [n_targets] may each be null.
inline Counts cells(const uint32_t dims[3], const uint8_t *member, const uint32_t *seeds, uint32_t n_seeds, const uint32_t *targets,
                    uint32_t n_targets, const uint32_t *list, uint32_t n_list, const Params &p, uint32_t *cost, uint8_t *parent,
                    uint32_t *of_member, uint32_t *target_cost, uint32_t *target_index) {
    const uint32_t nx = dims[0], ny = dims[1], nz = dims[2];
    const size_t n = (size_t)nx * ny * nz;
    std::vector<uint32_t> own_cost;
    if (cost == nullptr) {
        own_cost.resize(n);
        cost = own_cost.data();
    }
    std::fill(cost, cost + n, kNone);
    Counts s = {0, 0, 0, 0};
    for (size_t f = 0; f < n; ++f) s.n_members += member[f] ? 1u : 0u;
    typedef std::pair<uint32_t, uint32_t> Item;   // (cost, flat index)
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    for (uint32_t t = 0; t < n_seeds; ++t) {
        const uint32_t f = snapped(dims, member, p.snap, seeds[t]);
        if (f == kNone || cost[f] == 0) continue;   // out of range, no member, seeded before
        cost[f] = 0;
        ++s.n_seeded;
        heap.push(Item(0u, f));
    }
    // voxel (i, j, k) + (a, b, c), or n where it leaves the region
    const auto neighbour = [&](uint32_t i, uint32_t j, uint32_t k, int a, int b, int c) -> size_t {
        const uint32_t ui = i + (uint32_t)a, uj = j + (uint32_t)b, uk = k + (uint32_t)c;   // (0 - 1 wraps above nx)
        return ui < nx && uj < ny && uk < nz ? ((size_t)ui * ny + uj) * nz + uk : n;
    };
    const int st = (int)p.step;
    while (!heap.empty()) {
        const Item top = heap.top();
        heap.pop();
        const uint32_t f = top.second;
        if (top.first != cost[f]) continue;   // a stale entry
        const uint32_t k = f % nz, j = (f / nz) % ny, i = f / (nz * ny);
        for (int a = -1; a <= 1; ++a)
            for (int b = -1; b <= 1; ++b)
                for (int c = -st; c <= st; ++c) {
                    if (!allowed(p, a, b, c)) continue;
                    const size_t v = neighbour(i, j, k, a, b, c);
                    if (v == n || !member[v]) continue;
                    const uint32_t cand = top.first + move(p, a, b, c);   // <= 2^31 + 5 * 2^16
                    if (cand > p.max_cost || cand >= cost[v]) continue;
                    cost[v] = cand;
                    heap.push(Item(cand, (uint32_t)v));
                }
    }
    for (size_t f = 0; f < n; ++f) {
        if (cost[f] != kNone) {
            ++s.n_reached;
            s.max_cost = std::max(s.max_cost, cost[f]);
        }
        if (parent == nullptr) continue;
        uint8_t q = cost[f] == kNone ? 255 : code(0, 0, 0);
        if (cost[f] != kNone && cost[f] != 0) {
            const uint32_t k = (uint32_t)(f % nz), j = (uint32_t)((f / nz) % ny), i = (uint32_t)(f / ((size_t)nz * ny));
            bool found = false;
            for (int a = -1; a <= 1 && !found; ++a)   // the offsets o = u - v in the order of their code
                for (int b = -1; b <= 1 && !found; ++b)
                    for (int c = -st; c <= st && !found; ++c) {
                        if (!allowed(p, -a, -b, -c)) continue;
                        const size_t u = neighbour(i, j, k, a, b, c);
                        if (u != n && cost[u] != kNone && cost[u] + move(p, -a, -b, -c) == cost[f]) {   // (a finite cost: a member)
                            q = code(a, b, c);
                            found = true;
                        }
                    }
        }
        parent[f] = q;
    }
    if (of_member)
        for (uint32_t t = 0; t < n_list; ++t) of_member[t] = list[t] < n ? cost[list[t]] : kNone;
    for (uint32_t t = 0; t < n_targets; ++t) {
        const uint32_t f = snapped(dims, member, p.snap, targets[t]);
        if (target_cost) target_cost[t] = f == kNone ? kNone : cost[f];
        if (target_index) target_index[t] = f;
    }
    return s;
}

}  // namespace la3dm_drive

#endif
