// region_blocks.h — a region of blocks for pack_region / erase_region / evict (contract: include/la3dm_hip.h,
// la3dm_devmap_pack_region_host): a closed box klo <= k <= khi over the three 20-bit fields of the block hash key, and the
// flag `inside` that selects the blocks in the box (1) or every other block (0).  Plain C++ without dependencies: compiled
// into libla3dm_hip.so (devmap.hip: the argument checks; devmap_evict.h: the same test per lane), into libla3dm_map.so
// (host/bgkoctomap.cpp: the host-mode map and the mirror of a device-resident one) and into tools/check/region_blocks.cpp,
// which runs it under a sanitizer.
#ifndef LA3DM_REGION_BLOCKS_H
#define LA3DM_REGION_BLOCKS_H

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define LA3DM_RB_HD __host__ __device__
#else
#define LA3DM_RB_HD
#endif

namespace la3dm_region_blocks {

constexpr int32_t kFieldMax = 0xFFFFF;   // a key field has 20 bits

struct Box {
    int32_t lo[3], hi[3];   // x, y, z: key bits 59..40, 39..20, 19..0 (as la3dm_devmap_key_bounds reports them)
    int32_t inside;         // 1: the blocks in the box; 0: every other block
};

LA3DM_RB_HD inline int32_t field(long long key, int axis) { return (int32_t)((key >> (20 * (2 - axis))) & 0xFFFFF); }

LA3DM_RB_HD inline bool in_box(long long key, const Box &b) {
    bool in = true;
    for (int a = 0; a < 3; ++a) {
        const int32_t f = field(key, a);
        in = in && f >= b.lo[a] && f <= b.hi[a];
    }
    return in;
}

LA3DM_RB_HD inline bool selected(long long key, const Box &b) { return in_box(key, b) == (b.inside != 0); }

// "" = a region; else the refusal.  klo > khi on an axis is refused; a bound outside the 20-bit range is not (no key is there).
inline std::string check(const int32_t *klo, const int32_t *khi, Box *out) {
    if (!klo || !khi) return "null region bounds";
    for (int a = 0; a < 3; ++a)
        if (klo[a] > khi[a])
            return "klo > khi on axis " + std::to_string(a) + " (" + std::to_string(klo[a]) + " > " + std::to_string(khi[a]) + "): an empty box is not a region";
    if (out)
        for (int a = 0; a < 3; ++a) {
            out->lo[a] = klo[a];
            out->hi[a] = khi[a];
        }
    return "";
}

// the box from the block with key ka to the block with key kb (block_to_hash_key of two world points); "" or check's refusal
inline std::string from_corner_keys(long long ka, long long kb, bool inside, Box *out) {
    int32_t lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = field(ka, a);
        hi[a] = field(kb, a);
    }
    out->inside = inside ? 1 : 0;
    return check(lo, hi, out);
}

// the selected keys of a list, in the list's order
inline std::vector<int64_t> select(const std::vector<int64_t> &keys, const Box &b) {
    std::vector<int64_t> out;
    for (int64_t k : keys)
        if (selected(k, b)) out.push_back(k);
    return out;
}

}  // namespace la3dm_region_blocks

#endif
