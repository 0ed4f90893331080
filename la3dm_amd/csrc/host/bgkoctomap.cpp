// bgkoctomap.cpp — host side of the MI355X BGKOctoMap: node/octree/block bookkeeping,
// training-set front end, block partition (counting sort + closed-box rule), scan packing,
// commit + prune.  Kernel evaluation and fusion happen on the GPU via include/la3dm_hip.h.
//
// Reference behaviour followed (file:line relative to RobustFieldAutonomyLab/la3dm):
//   constructor / statics              src/bgkoctomap/bgkoctomap.cpp:31-56
//   insert_pointcloud stages A..G      src/bgkoctomap/bgkoctomap.cpp:214-366
//   get_training_data / beam_sample    src/bgkoctomap/bgkoctomap.cpp:383-458
//   bbox / get_blocks_in_bbox          src/bgkoctomap/bgkoctomap.cpp:464-495
//   closed-box gather                  src/bgkoctomap/bgkoctomap.cpp:497-552, include/common/rtree.h:1519-1532
//   hashing / LUT / extended block     src/bgkoctomap/bgkblock.cpp:7-32, 73-130
//   OcTree leaves / prune              src/bgkoctomap/bgkoctree.cpp:72-148, include/bgkoctomap/bgkoctree.h:62-147
//   Occupancy                          src/bgkoctomap/bgkoctree_node.cpp:15-44
#include "bgkoctomap.h"
#include "region_contract.h"
#include "nearest_lines.h"
#include "diff_block.h"
#include "merge_block.h"
#include "region_blocks.h"
#include "pack_format.h"

#include <algorithm>
#include <parallel/algorithm>
#include <omp.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <new>
#include <queue>
#include <stdexcept>
#include <string>

namespace la3dm {

namespace {
constexpr int kHostThreads = 16;  // OpenMP team of the host-side loops (start-up and spin-wait cost grow with the team)
double wall() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline uint32_t layer_base(unsigned depth) { return 0x249249u & ((1u << (3u * depth)) - 1u); }
}  // namespace

// ------------------------------------------------------------------ Occupancy
float Occupancy::sf2 = 1.0f;
float Occupancy::ell = 1.0f;
float Occupancy::free_thresh = 0.3f;
float Occupancy::occupied_thresh = 0.7f;
float Occupancy::var_thresh = 1000.0f;
float Occupancy::prior_A = 0.5f;
float Occupancy::prior_B = 0.5f;
int Occupancy::variant = 0;
float Occupancy::init_A = 0.5f;
float Occupancy::init_B = 0.5f;
float Occupancy::noise = 0.01f;
float Occupancy::l = 100.f;
float Occupancy::max_ivar = 1000.0f;
float Occupancy::min_ivar = 0.001f;
float Occupancy::min_known_ivar = 10.0f;

float Occupancy::min_W = 0.1f;
bool Occupancy::original_size = true;

float Occupancy::get_var() const {
    if (variant == 1) return 1.0f / m_B;
    if (variant == 2) {  // bgklvoctree_node.cpp:49-63
        const float prob = get_prob();
        const float W = (m_A + m_B < min_W) ? min_W : m_A + m_B;
        return (float)(m_A / W * pow(1 - prob, 2) + (W - m_A - m_B) / W * pow(0.5 - prob, 2) + m_B / W * pow(prob, 2));
    }
    return (m_A * m_B) / ((m_A + m_B) * (m_A + m_B) * (m_A + m_B + 1.0f));
}

float Occupancy::get_prob() const {
    if (variant == 2) {  // bgklvoctree_node.cpp:29-47
        const float W = (m_A + m_B < min_W) ? min_W : m_A + m_B;
        if (m_A > m_B) return (float)(m_A / (W - m_B) + (W - m_A - m_B) * 0.5 / (W - m_B));
        return (float)(0.5 * (W - m_B - m_A) / (W - m_A));
    }
    if (variant == 1) return 1.0f / (1.0f + (float)exp((double)(-l * m_A / max_ivar)));  // gpoctree_node.cpp:31-34
    return m_A / (m_A + m_B);
}

void Occupancy::classify() {
    if (variant == 1) {  // gpoctree_node.cpp:40-48
        if (m_B < min_known_ivar) {
            state = State::UNKNOWN;
            return;
        }
        m_B = m_B > max_ivar ? max_ivar : m_B;
        const float p = get_prob();
        state = p > occupied_thresh ? State::OCCUPIED : (p < free_thresh ? State::FREE : State::UNKNOWN);
        return;
    }
    if (get_var() > var_thresh) {
        state = variant == 2 ? State::UNCERTAIN : State::UNKNOWN;
        return;
    }
    float p = get_prob();
    state = p > occupied_thresh ? State::OCCUPIED : (p < free_thresh ? State::FREE : State::UNKNOWN);
}

Occupancy::Occupancy(float A, float B) : classified(false) {
    if (variant == 1) {  // Occupancy(m, var), gpoctree_node.cpp:19-29
        m_A = A / B;
        m_B = 1.0f / B;
    } else {
        m_A = prior_A + A;
        m_B = prior_B + B;
    }
    classify();
}

std::ofstream &operator<<(std::ofstream &os, const Occupancy &oc) {
    os.write((const char *)&oc.m_A, sizeof(oc.m_A));
    os.write((const char *)&oc.m_B, sizeof(oc.m_B));
    return os;
}
std::ifstream &operator>>(std::ifstream &is, Occupancy &oc) {
    float A, B;
    is.read((char *)&A, sizeof(A));
    is.read((char *)&B, sizeof(B));
    oc = OcTreeNode(A, B);
    return is;
}
std::ostream &operator<<(std::ostream &os, const Occupancy &oc) { return os << '(' << oc.m_A << ' ' << oc.m_B << ' ' << oc.get_prob() << ')'; }

void Occupancy::update(float ybar, float kbar) {
    classified = true;
    if (variant == 1) {  // BCM: update(new_m, new_var), gpoctree_node.cpp:36-39
        m_B = (float)((double)m_B + (1.0 / (double)kbar - (double)sf2));
        m_A += ybar / kbar;
    } else {
        m_A += ybar;
        m_B += kbar - ybar;
    }
    classify();
}

// --------------------------------------------------------------------- OcTree
unsigned short OcTree::max_depth = 0;

OcTree::OcTree() : node_arr(nullptr), slab(nullptr), ever_pruned(false) {
    if (max_depth == 0) return;
    size_t total = layer_base(max_depth);
    slab = new OcTreeNode[total]();
    node_arr = new OcTreeNode *[max_depth];
    for (unsigned d = 0; d < max_depth; ++d) node_arr[d] = slab + layer_base(d);
}

OcTree::~OcTree() {
    delete[] node_arr;
    delete[] slab;
}

bool OcTree::is_leaf(unsigned short depth, unsigned short index) const {
    if (node_arr == nullptr || node_arr[depth] == nullptr) return false;
    if (node_arr[depth][index].get_state() == State::PRUNED) return false;
    if (depth + 1 >= max_depth) return true;
    return node_arr[depth + 1] == nullptr || node_arr[depth + 1][index * 8].get_state() == State::PRUNED;
}

void OcTree::load_nodes(const float *A, const float *B, const uint8_t *S, size_t n) {
    if (slab == nullptr || n != layer_base(max_depth)) throw std::runtime_error("OcTree::load_nodes: node count mismatch");
    bool pruned = false;
    for (size_t i = 0; i < n; ++i) {
        OcTreeNode &nd = slab[i];
        nd.m_A = A[i];
        nd.m_B = B[i];
        nd.state = (State)(S[i] & 7u);
        nd.classified = (S[i] & 0x80u) != 0;
        pruned |= nd.state == State::PRUNED;
    }
    for (unsigned d = 0; d < max_depth; ++d) node_arr[d] = slab + layer_base(d);  // layers are never retired here
    ever_pruned = pruned;
}

bool OcTree::is_leaf(OcTreeHashKey key) const { return is_leaf((unsigned short)(key >> 16), (unsigned short)(key & 0xFFFF)); }

bool OcTree::search(OcTreeHashKey key) const {
    unsigned d = key >> 16, i = key & 0xFFFF;
    return node_arr != nullptr && node_arr[d] != nullptr && node_arr[d][i].get_state() != State::PRUNED;
}

// Nodes stay addressable after their layer was retired by prune() (the reference frees the layer and would read
// freed memory here): the slab keeps them, with state PRUNED.
OcTreeNode &OcTree::operator[](OcTreeHashKey key) const { return slab[layer_base((unsigned)(key >> 16)) + (key & 0xFFFF)]; }

// Bottom-up collapse of sibling groups that share one non-UNKNOWN state; the parent becomes a
// copy of child 0 (not an average) and a layer with nothing left to collapse is retired.
bool OcTree::prune() {
    if (node_arr == nullptr) return false;
    bool any = false;
    for (int depth = max_depth - 1; depth > 0; --depth) {
        OcTreeNode *layer = node_arr[depth];
        if (layer == nullptr) continue;
        OcTreeNode *parents = node_arr[depth - 1];
        const unsigned n = 1u << (3 * depth);
        bool retire = true;
        for (unsigned g = 0; g < n; g += 8) {
            const State s0 = layer[g].get_state();
            if (s0 == State::PRUNED) continue;
            if (s0 == State::UNKNOWN) {
                retire = false;
                continue;
            }
            bool same = true;
            for (unsigned c = 1; c < 8; ++c) same &= (layer[g + c].get_state() == s0);
            if (!same) {
                retire = false;
                continue;
            }
            parents[g >> 3] = layer[g];
            for (unsigned c = 0; c < 8; ++c) layer[g + c].prune();
            any = true;
        }
        if (retire) node_arr[depth] = nullptr;
    }
    if (any) ever_pruned = true;
    return any;
}

OcTree::LeafIterator::LeafIterator(const OcTree *t) : tree(t != nullptr && t->node_arr != nullptr ? t : nullptr), top(0) {
    if (tree == nullptr) return;
    stack[top++] = node_to_hash_key(0, 0);
    settle();
    if (top == 0) tree = nullptr;
}

void OcTree::LeafIterator::settle() {
    while (top > 0 && !tree->is_leaf(stack[top - 1])) {
        const OcTreeHashKey k = stack[--top];
        const unsigned d = k >> 16, i = k & 0xFFFF;
        if (d + 1 >= OcTree::max_depth) continue;  // pruned node at the last layer
        for (unsigned c = 0; c < 8; ++c) stack[top++] = node_to_hash_key(d + 1, i * 8 + c);
    }
}

OcTree::LeafIterator &OcTree::LeafIterator::operator++() {
    if (top > 0) {
        --top;
        settle();
    }
    if (top == 0) tree = nullptr;
    return *this;
}

void OcTree::collect_leaves(std::vector<uint32_t> &keys) const {
    if (node_arr == nullptr) return;
    if (!ever_pruned) {  // untouched tree: the whole finest layer, highest index first
        const unsigned d = max_depth - 1, n = 1u << (3 * d);
        for (unsigned i = n; i-- > 0;) keys.push_back((d << 16) + i);
        return;
    }
    for (LeafIterator it(this); it != LeafIterator(); ++it) keys.push_back((uint32_t)it.get_hash_key());
}

// ---------------------------------------------------------------------- Block
float Block::resolution = 0.1f;
float Block::size = 0.8f;
std::vector<point3f> Block::key_loc_map;

std::vector<point3f> init_key_loc_map(float resolution, unsigned short max_depth) {
    // Layer by layer; the child offsets are formed in double and rounded once, exactly as
    // the reference's breadth-first construction does (bgkblock.cpp:14-28).
    std::vector<point3f> lut(layer_base(max_depth));
    if (max_depth == 0) return lut;
    lut[0] = point3f(0.0f, 0.0f, 0.0f);
    for (unsigned d = 0; d + 1 < max_depth; ++d) {
        const float half_size = (float)(resolution * pow(2, max_depth - d - 1) * 0.5f);
        const unsigned n = 1u << (3 * d);
        for (unsigned i = 0; i < n; ++i) {
            const point3f c = lut[layer_base(d) + i];
            for (unsigned k = 0; k < 8; ++k)
                lut[layer_base(d + 1) + 8 * i + k] =
                    point3f((float)(c.x() + half_size * (k & 4 ? 0.5 : -0.5)), (float)(c.y() + half_size * (k & 2 ? 0.5 : -0.5)),
                            (float)(c.z() + half_size * (k & 1 ? 0.5 : -0.5)));
        }
    }
    return lut;
}

BlockHashKey block_to_hash_key(point3f c) { return block_to_hash_key(c.x(), c.y(), c.z()); }

BlockHashKey block_to_hash_key(float x, float y, float z) {
    const double s = (double)Block::size;
    return (int64_t(x / s + 524288.5) << 40) | (int64_t(y / s + 524288.5) << 20) | int64_t(z / s + 524288.5);
}

point3f hash_key_to_block(BlockHashKey key) {
    return point3f(((key >> 40) - 524288) * Block::size, (((key >> 20) & 0xFFFFF) - 524288) * Block::size,
                   ((key & 0xFFFFF) - 524288) * Block::size);
}

static ExtendedBlock extended_from(float x, float y, float z, BlockHashKey self, float s) {
    ExtendedBlock e;
    e[0] = self;
    e[1] = block_to_hash_key(s + x, 0 + y, 0 + z);
    e[2] = block_to_hash_key(-s + x, 0 + y, 0 + z);
    e[3] = block_to_hash_key(0 + x, s + y, 0 + z);
    e[4] = block_to_hash_key(0 + x, -s + y, 0 + z);
    e[5] = block_to_hash_key(0 + x, 0 + y, s + z);
    e[6] = block_to_hash_key(0 + x, 0 + y, -s + z);
    return e;
}

ExtendedBlock get_extended_block(BlockHashKey key) {
    const point3f c = hash_key_to_block(key);
    return extended_from(c.x(), c.y(), c.z(), key, Block::size);
}

ExtendedBlock Block::get_extended_block() const {
    return extended_from(center.x(), center.y(), center.z(), block_to_hash_key(center.x(), center.y(), center.z()), size);
}

OcTreeNode &Block::search(point3f p) const {
    // finest-layer voxel containing p; child bit 4 -> +x, 2 -> +y, 1 -> +z at every level
    const int cells = 1 << (max_depth - 1);
    auto cell = [&](float v, float c) {
        int i = (int)std::floor((v - c) / resolution + cells / 2.0f);
        return std::max(0, std::min(i, cells - 1));
    };
    const int ix = cell(p.x(), center.x()), iy = cell(p.y(), center.y()), iz = cell(p.z(), center.z());
    unsigned index = 0;
    for (int level = max_depth - 2; level >= 0; --level)
        index = index * 8 + ((((ix >> level) & 1) << 2) | (((iy >> level) & 1) << 1) | ((iz >> level) & 1));
    return slab[layer_base(max_depth - 1) + index];  // also valid when prune() retired the finest layer
}

void Block::get_index(const point3f &p, unsigned short &x, unsigned short &y, unsigned short &z) const {
    const int cells = cell_num();
    auto cell = [&](float v, float c) {
        const int i = (int)((v - c) / resolution + cells / 2);
        return (unsigned short)std::max(0, std::min(i, cells - 1));
    };
    x = cell(p.x(), center.x());
    y = cell(p.y(), center.y());
    z = cell(p.z(), center.z());
}

OcTreeHashKey Block::get_node(unsigned short x, unsigned short y, unsigned short z) {
    unsigned index = 0;
    for (int level = max_depth - 2; level >= 0; --level)
        index = index * 8 + ((((x >> level) & 1u) << 2) | (((y >> level) & 1u) << 1) | ((z >> level) & 1u));
    return node_to_hash_key((unsigned short)(max_depth - 1), (unsigned short)index);
}

// ------------------------------------------------------------------ RayCaster
BGKOctoMap::RayCaster::RayCaster(const BGKOctoMap *m, const point3f &start, const point3f &end_)
    : map(m), block(nullptr), n(0), lim(1 << (m->block_depth - 1)) {
    m->bind();
    key = block_to_hash_key(start);
    block = map->search(key);
    if (block == nullptr) return;  // the walk only starts inside an existing block
    unsigned short x, y, z;
    block->get_index(start, x, y, z);
    idx[0] = x;
    idx[1] = y;
    idx[2] = z;
    block_center = block->get_center();
    current_p = start;
    const float res = map->resolution;
    const int a0[3] = {(int)(start.x() / res), (int)(start.y() / res), (int)(start.z() / res)};
    const int a1[3] = {(int)(end_.x() / res), (int)(end_.y() / res), (int)(end_.z() / res)};
    int d[3];
    for (int a = 0; a < 3; ++a) {
        d[a] = std::abs(a1[a] - a0[a]);
        inc[a] = a1[a] > a0[a] ? 1 : (a1[a] == a0[a] ? 0 : -1);
    }
    n = 1 + d[0] + d[1] + d[2];
    err_xy = d[0] - d[1];
    err_xz = d[0] - d[2];
    err_yz = d[1] - d[2];
    for (int a = 0; a < 3; ++a) d2[a] = 2 * d[a];
}

// leave the block through the face of `axis`: neighbour centre = centre +- size on that axis, re-hashed
void BGKOctoMap::RayCaster::enter_block(int axis, int step) {
    block_center(axis) += step * map->block_size;
    key = block_to_hash_key(block_center);
    block = map->search(key);
    idx[axis] = step > 0 ? 0 : lim - 1;
}

bool BGKOctoMap::RayCaster::next(point3f &p, OcTreeNode &node, BlockHashKey &block_key, OcTreeHashKey &node_key) {
    node_key = Block::get_node((unsigned short)idx[0], (unsigned short)idx[1], (unsigned short)idx[2]);
    block_key = key;
    const bool valid = block != nullptr;
    if (valid) {
        node = (*block)[node_key];
        current_p = block->get_point((unsigned short)idx[0], (unsigned short)idx[1], (unsigned short)idx[2]);
    }
    p = current_p;
    const float res = map->resolution;
    auto step = [&](int axis) {
        idx[axis] += inc[axis];
        current_p(axis) += inc[axis] * res;
        if (idx[axis] >= lim || idx[axis] < 0) enter_block(axis, inc[axis]);
    };
    // same case order as the reference; when no case applies the walk repeats the voxel (n still counts down)
    if (err_xy > 0 && err_xz > 0) {
        step(0);
        err_xy -= d2[1];
        err_xz -= d2[2];
    } else if (err_xy < 0 && err_yz > 0) {
        step(1);
        err_xy += d2[0];
        err_yz -= d2[2];
    } else if (err_yz < 0 && err_xz < 0) {
        step(2);
        err_xz += d2[0];
        err_yz += d2[1];
    } else if (err_xy == 0) {  // diagonal move in the xy plane: two voxel steps at once
        step(0);
        step(1);
        n -= 2;
    }
    --n;
    return valid;
}

// ----------------------------------------------------------------- BGKOctoMap
BGKOctoMap::BGKOctoMap() : BGKOctoMap(0.1f, 4, 1.0, 1.0, 0.3f, 0.7f, 1.0f, 1.0f, 1.0f) {}

BGKOctoMap::BGKOctoMap(float resolution_, unsigned short block_depth_, float sf2, float ell, float free_thresh,
                       float occupied_thresh, float var_thresh, float prior_A, float prior_B, int device)
    : BGKOctoMap(0, resolution_, block_depth_, sf2, ell, free_thresh, occupied_thresh, var_thresh, prior_A, prior_B,
                 nullptr, device) {}

GPOctoMap::GPOctoMap(float resolution_, unsigned short block_depth_, float sf2, float ell, float noise, float l,
                     float min_var, float max_var, float max_known_var, float free_thresh, float occupied_thresh,
                     int device)
    : BGKOctoMap(1, resolution_, block_depth_, sf2, ell, free_thresh, occupied_thresh, 0.0f, 0.0f, 0.0f,
                 [&] {
                     static thread_local GPParams g;
                     g = GPParams{noise, l, min_var, max_var, max_known_var, 0.1f, true};
                     return &g;
                 }(),
                 device) {}

BGKOctoMap::BGKOctoMap(int variant_, float resolution_, unsigned short block_depth_, float sf2, float ell,
                       float free_thresh, float occupied_thresh, float var_thresh, float prior_A, float prior_B,
                       const GPParams *gp, int device)
    : resolution(resolution_), block_size((float)pow(2, block_depth_ - 1) * resolution_), block_depth(block_depth_),
      ctx(nullptr), scan_flags(0), variant(variant_), train_max_n(0), train_sum_n2(0) {
    ctor_gp = gp != nullptr ? *gp : GPParams{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, true};
    Block::resolution = resolution;
    Block::size = block_size;
    Block::key_loc_map = init_key_loc_map(resolution, block_depth);
    OcTree::max_depth = block_depth;
    OcTreeNode::sf2 = sf2;
    OcTreeNode::ell = ell;
    OcTreeNode::free_thresh = free_thresh;
    OcTreeNode::occupied_thresh = occupied_thresh;
    OcTreeNode::var_thresh = var_thresh;
    OcTreeNode::prior_A = prior_A;
    OcTreeNode::prior_B = prior_B;
    OcTreeNode::variant = variant == 3 ? 0 : variant;  // BGKLOctoMap shares the BGK node (bgkloctree_node.cpp)
    OcTreeNode::init_A = prior_A;
    OcTreeNode::init_B = prior_B;
    if (variant == 2) {  // src/bgklvoctomap/bgklvoctomap.cpp:60-61
        OcTreeNode::min_W = gp->min_W;
        OcTreeNode::original_size = gp->original_size;
    }
    if (variant == 1) {  // src/gpoctomap/gpoctomap.cpp:37-44
        OcTreeNode::noise = gp->noise;
        OcTreeNode::l = gp->l;
        OcTreeNode::min_ivar = 1.0f / gp->max_var;
        OcTreeNode::max_ivar = 1.0f / gp->min_var;
        OcTreeNode::min_known_ivar = 1.0f / gp->max_known_var;
        OcTreeNode::init_A = 0.0f;
        OcTreeNode::init_B = OcTreeNode::min_ivar;
    }

    capture_statics();

    la3dm_params &p = create_params;
    std::memset(&p, 0, sizeof(p));
    p.variant = variant;
    p.noise = OcTreeNode::noise;
    p.l = OcTreeNode::l;
    p.min_ivar = OcTreeNode::min_ivar;
    p.max_ivar = OcTreeNode::max_ivar;
    p.min_known_ivar = OcTreeNode::min_known_ivar;
    p.min_W = OcTreeNode::min_W;
    p.sf2 = sf2;
    p.ell = ell;
    p.free_thresh = free_thresh;
    p.occupied_thresh = occupied_thresh;
    p.var_thresh = var_thresh;
    p.prior_A = prior_A;
    p.prior_B = prior_B;
    p.device = device;
    create_context();
}

void BGKOctoMap::create_context() {
    la3dm_params &p = create_params;
    p.resolution = resolution;
    p.block_depth = block_depth;
    p.lut_xyz = &Block::key_loc_map[0].x();
    p.lut_count = (uint32_t)Block::key_loc_map.size();
    static_assert(sizeof(point3f) == 12, "LUT is handed to the device as packed xyz");
    if (p.device < 0) return;  // bookkeeping-only map (tests of the host logic): inserting throws
    int rc = la3dm_create(&p, &ctx);
    if (rc != LA3DM_OK)
        throw std::runtime_error(std::string("BGKOctoMap: GPU context creation failed: ") + la3dm_last_error(nullptr));
    // Device-resident by default where it exists (BGK and GP maps, block_depth <= 5): insert_pointcloud then runs
    // start to finish on the GPU (insert_training_data too).  The split prepare()/commit() form moves the map back to
    // the host-orchestrated mode on its own (ensure_host_mode).  LA3DM_DEVICE_RESIDENT=0 keeps the host mode.
    const char *env = getenv("LA3DM_DEVICE_RESIDENT");
    if (variant >= 0 && variant <= 3 && block_depth <= 5 && !(env && env[0] == '0')) {
        if (la3dm_devmap_create(ctx, &dmap) != LA3DM_OK) dmap = nullptr;
    }
}

void BGKOctoMap::set_resolution(float r) { reconfigure(r, block_depth); }
void BGKOctoMap::set_block_depth(unsigned short d) { reconfigure(resolution, d); }

// reference bgkoctomap.cpp:66-80: resolution / block_depth, Block::resolution, Block::size, Block::key_loc_map,
// OcTree::max_depth — on an empty map (see the header)
void BGKOctoMap::reconfigure(float r, unsigned short d) {
    bind();
    if (!(r > 0.0f) || !std::isfinite(r)) throw std::invalid_argument("set_resolution: resolution must be positive and finite");
    if (d < 1 || d > 6) throw std::invalid_argument("set_block_depth: block_depth must be in 1..6 (16-bit in-block keys)");
    bool empty = block_arr.empty();
    if (dmap != nullptr) {
        uint32_t nb = 0, npb = 0;
        if (la3dm_devmap_block_count(dmap, &nb, &npb) != LA3DM_OK || nb != 0) empty = false;
    }
    if (!empty)
        throw std::logic_error("set_resolution / set_block_depth: the map already holds blocks (the reference re-derives the "
                               "block size and the voxel LUT under them and corrupts the map; build a new map instead)");
    const bool was_resident = dmap != nullptr;
    la3dm_devmap_destroy(dmap);
    dmap = nullptr;
    la3dm_destroy(ctx);
    ctx = nullptr;
    resolution = r;
    block_depth = d;
    block_size = (float)pow(2, block_depth - 1) * resolution;
    Block::resolution = resolution;
    Block::size = block_size;
    Block::key_loc_map = init_key_loc_map(resolution, block_depth);
    OcTree::max_depth = block_depth;
    capture_statics();
    passes.clear();
    create_context();
    if (!was_resident && dmap != nullptr) {  // the map had been moved to the host-orchestrated mode: keep it there
        la3dm_devmap_destroy(dmap);
        dmap = nullptr;
    }
    // the new device map starts unsharded: a block-sharded map stays one
    if (dmap != nullptr && shard_cfg.world > 1 &&
        la3dm_devmap_set_shard(dmap, shard_cfg.rank, shard_cfg.world, shard_cfg.fn, shard_cfg.user) != LA3DM_OK)
        throw std::runtime_error(la3dm_last_error(ctx));
}

const BGKOctoMap *BGKOctoMap::bound = nullptr;

void BGKOctoMap::capture_statics() {
    mine.resolution = Block::resolution;
    mine.size = Block::size;
    mine.key_loc_map = Block::key_loc_map;
    mine.max_depth = OcTree::max_depth;
    mine.sf2 = OcTreeNode::sf2;
    mine.ell = OcTreeNode::ell;
    mine.free_thresh = OcTreeNode::free_thresh;
    mine.occupied_thresh = OcTreeNode::occupied_thresh;
    mine.var_thresh = OcTreeNode::var_thresh;
    mine.prior_A = OcTreeNode::prior_A;
    mine.prior_B = OcTreeNode::prior_B;
    mine.init_A = OcTreeNode::init_A;
    mine.init_B = OcTreeNode::init_B;
    mine.min_W = OcTreeNode::min_W;
    mine.noise = OcTreeNode::noise;
    mine.l = OcTreeNode::l;
    mine.min_ivar = OcTreeNode::min_ivar;
    mine.max_ivar = OcTreeNode::max_ivar;
    mine.min_known_ivar = OcTreeNode::min_known_ivar;
    mine.variant = OcTreeNode::variant;
    mine.original_size = OcTreeNode::original_size;
    bound = this;
}

// re-install this map's parameters into the process-global statics (no-op while this map is the bound one)
void BGKOctoMap::bind() const {
    if (bound == this) return;
    Block::resolution = mine.resolution;
    Block::size = mine.size;
    Block::key_loc_map = mine.key_loc_map;
    OcTree::max_depth = mine.max_depth;
    OcTreeNode::sf2 = mine.sf2;
    OcTreeNode::ell = mine.ell;
    OcTreeNode::free_thresh = mine.free_thresh;
    OcTreeNode::occupied_thresh = mine.occupied_thresh;
    OcTreeNode::var_thresh = mine.var_thresh;
    OcTreeNode::prior_A = mine.prior_A;
    OcTreeNode::prior_B = mine.prior_B;
    OcTreeNode::init_A = mine.init_A;
    OcTreeNode::init_B = mine.init_B;
    OcTreeNode::min_W = mine.min_W;
    OcTreeNode::noise = mine.noise;
    OcTreeNode::l = mine.l;
    OcTreeNode::min_ivar = mine.min_ivar;
    OcTreeNode::max_ivar = mine.max_ivar;
    OcTreeNode::min_known_ivar = mine.min_known_ivar;
    OcTreeNode::variant = mine.variant;
    OcTreeNode::original_size = mine.original_size;
    bound = this;
}

void BGKOctoMap::ensure_host_mode() {
    if (dmap != nullptr) set_device_resident(false);
}

BGKOctoMap::~BGKOctoMap() {
    bind();  // the blocks' destructors read the layer count
    for (auto &kv : block_arr) delete kv.second;
    bound = nullptr;
    la3dm_devmap_destroy(dmap);
    la3dm_destroy(ctx);
}

// ------------------------------------------------------------- device-resident mode
void BGKOctoMap::set_device_resident(bool on) {
    bind();
    if (on == (dmap != nullptr)) return;
    if (!on) {
        sync_mirror();
        la3dm_devmap_destroy(dmap);
        dmap = nullptr;
        return;
    }
    if (ctx == nullptr) throw std::runtime_error("BGKOctoMap::set_device_resident: the map has no GPU context");
    if (!block_arr.empty())
        throw std::runtime_error("BGKOctoMap::set_device_resident: a map that already holds host blocks stays host-orchestrated");
    if (la3dm_devmap_create(ctx, &dmap) != LA3DM_OK)
        throw std::runtime_error(std::string("BGKOctoMap::set_device_resident: ") + la3dm_last_error(ctx));
}

// Refresh the host mirror from the device pool: every block's nodes are overwritten with the device
// state (alpha, beta, state, classified); PRUNED children keep their collapsed parents' leaf role.
void BGKOctoMap::sync_mirror() const {
    bind();
    if (dmap == nullptr || !mirror_dirty) return;
    uint32_t nb = 0, npb = 0;
    if (la3dm_devmap_block_count(dmap, &nb, &npb) != LA3DM_OK)
        throw std::runtime_error(std::string("BGKOctoMap::sync_mirror: ") + la3dm_last_error(ctx));
    std::vector<int64_t> keys(nb);
    std::vector<float> A((size_t)nb * npb), B((size_t)nb * npb);
    std::vector<uint8_t> S((size_t)nb * npb);
    if (nb && la3dm_devmap_download(dmap, keys.data(), A.data(), B.data(), S.data()) != LA3DM_OK)
        throw std::runtime_error(std::string("BGKOctoMap::sync_mirror: ") + la3dm_last_error(ctx));
    for (uint32_t b = 0; b < nb; ++b) {
        auto it = block_arr.find(keys[b]);
        if (it == block_arr.end()) it = block_arr.emplace(keys[b], new Block(hash_key_to_block(keys[b]))).first;
        it->second->load_nodes(&A[(size_t)b * npb], &B[(size_t)b * npb], &S[(size_t)b * npb], npb);
    }
    mirror_dirty = false;
    ++mirror_sync_count;
}

// ---- save / load (include/la3dm_hip.h, la3dm_devmap_pack_host; the format's host code: pack_format.h) ----
namespace {
la3dm_params stream_params(const la3dm_params &created, float resolution, unsigned short block_depth) {
    la3dm_params p = created;
    p.resolution = resolution;
    p.block_depth = block_depth;
    return p;
}
}  // namespace

// pack / pack_region: box = nullptr is every block
std::vector<uint8_t> BGKOctoMap::pack_blocks(const la3dm_region_blocks::Box *box, const char *who) const {
    bind();
    const float gp3[3] = {ctor_gp.min_var, ctor_gp.max_var, ctor_gp.max_known_var};
    const float *exact = variant == 1 ? gp3 : nullptr;
    if (dmap != nullptr) {   // compacted on the GPU; the mirror is not touched
        uint64_t size = 0;
        const auto call = [&](void *buf, uint64_t cap) {
            return box ? la3dm_devmap_pack_region_host(dmap, box->lo, box->hi, box->inside, buf, cap, &size) : la3dm_devmap_pack_host(dmap, buf, cap, &size);
        };
        if (call(nullptr, 0) != LA3DM_OK) throw std::runtime_error(std::string(who) + ": " + la3dm_last_error(ctx));
        std::vector<uint8_t> out(size);
        if (call(out.data(), size) != LA3DM_OK) throw std::runtime_error(std::string(who) + ": " + la3dm_last_error(ctx));
        if (exact) std::memcpy(out.data() + offsetof(la3dm_pack_header, min_var), exact, sizeof(gp3));   // (the context only knows the inverses)
        return out;
    }
    const la3dm_pack_header proto =
        la3dm_pack::make_header(stream_params(create_params, resolution, block_depth), mine.original_size, exact, 0, 0);
    std::vector<int64_t> keys;
    keys.reserve(block_arr.size());
    for (const auto &kv : block_arr) keys.push_back(kv.first);
    if (box) keys = la3dm_region_blocks::select(keys, *box);
    std::sort(keys.begin(), keys.end());
    return la3dm_pack::write(proto, keys, [&](uint64_t b, float *A, float *B, uint8_t *S) {
        const OcTreeNode *slab = block_arr.find(keys[b])->second->slab;   // (retired layers keep their PRUNED nodes in the slab)
        for (uint32_t n = 0; n < proto.nodes_per_block; ++n) {
            A[n] = slab[n].m_A;
            B[n] = slab[n].m_B;
            S[n] = (uint8_t)((uint8_t)slab[n].state | (slab[n].classified ? 0x80u : 0u));
        }
    });
}

std::vector<uint8_t> BGKOctoMap::pack() const { return pack_blocks(nullptr, "BGKOctoMap::pack"); }

uint64_t BGKOctoMap::packed_size() const {
    bind();
    if (dmap == nullptr) return pack().size();
    uint64_t size = 0;
    if (la3dm_devmap_pack_host(dmap, nullptr, 0, &size) != LA3DM_OK)
        throw std::runtime_error(std::string("BGKOctoMap::pack: ") + la3dm_last_error(ctx));
    return size;
}

void BGKOctoMap::unpack(const void *stream, size_t size) {
    bind();
    la3dm_pack_header h;
    if (dmap != nullptr) {
        if (la3dm_devmap_unpack_host(dmap, stream, size) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::unpack: ") + la3dm_last_error(ctx));
        std::memcpy(&h, stream, sizeof(h));
        for (auto &kv : block_arr) delete kv.second;
        block_arr.clear();
        mirror_dirty = true;
    } else {
        if (!block_arr.empty())
            throw std::runtime_error("BGKOctoMap::unpack: the map already holds blocks (a stream is loaded into an empty map)");
        std::string bad = la3dm_pack::validate(stream, size, &h);
        if (bad.empty())
            bad = la3dm_pack::mismatch(h, la3dm_pack::make_header(stream_params(create_params, resolution, block_depth), mine.original_size, nullptr, 0, 0));
        if (!bad.empty()) throw std::runtime_error("BGKOctoMap::unpack: " + bad);
        const la3dm_pack::Layout l = la3dm_pack::layout(h.n_blocks, h.n_leaves, h.nodes_per_block);
        std::vector<float> A(h.nodes_per_block), B(h.nodes_per_block);
        std::vector<uint8_t> S(h.nodes_per_block);
        for (uint64_t b = 0; b < h.n_blocks; ++b) {
            int64_t key;
            std::memcpy(&key, (const uint8_t *)stream + l.keys + 8 * b, 8);
            la3dm_pack::expand_block((const uint8_t *)stream, h, l, b, A.data(), B.data(), S.data());
            Block *blk = new Block(hash_key_to_block(key));
            blk->load_nodes(A.data(), B.data(), S.data(), h.nodes_per_block);
            block_arr.emplace(key, blk);
        }
    }
    if (h.variant == 2u) {   // BGK-LV: whether export_cells keeps collapsed leaves at their size travels with the map
        mine.original_size = (h.flags & LA3DM_PACK_FLAG_LV_ORIGINAL_SIZE) != 0;
        OcTreeNode::original_size = mine.original_size;
    }
}

namespace {
// bytes to path + ".tmp", renamed to path
void write_renamed(const std::vector<uint8_t> &bytes, const std::string &path, const std::string &who) {
    const std::string tmp = path + ".tmp";
    {
        std::ofstream out(tmp, std::ios::binary | std::ios::trunc);
        if (!out) throw std::runtime_error(who + ": cannot open " + tmp);
        out.write((const char *)bytes.data(), (std::streamsize)bytes.size());
        out.flush();
        if (!out) throw std::runtime_error(who + ": cannot write " + tmp);
    }
    if (std::rename(tmp.c_str(), path.c_str()) != 0) throw std::runtime_error(who + ": cannot rename " + tmp + " to " + path);
}
}  // namespace

void BGKOctoMap::save(const std::string &path) const { write_renamed(pack(), path, "BGKOctoMap::save"); }

void BGKOctoMap::load(const std::string &path) {
    std::ifstream in(path, std::ios::binary | std::ios::ate);
    if (!in) throw std::runtime_error("BGKOctoMap::load: cannot open " + path);
    const std::streamsize size = in.tellg();
    std::vector<uint8_t> bytes((size_t)std::max<std::streamsize>(size, 0));
    in.seekg(0);
    if (!bytes.empty() && !in.read((char *)bytes.data(), size)) throw std::runtime_error("BGKOctoMap::load: cannot read " + path);
    unpack(bytes.data(), bytes.size());
}

// ---- merge (include/la3dm_hip.h, la3dm_devmap_merge_host; the rule per block: merge_block.h) ----
la3dm_merge_stats BGKOctoMap::merge(const void *stream, size_t size) {
    bind();
    la3dm_merge_stats stats;
    std::memset(&stats, 0, sizeof(stats));
    if (dmap != nullptr) {
        if (la3dm_devmap_merge_host(dmap, stream, size, &stats) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::merge: ") + la3dm_last_error(ctx));
        mirror_dirty = true;
        return stats;
    }
    if (variant != 0 && variant != 3)
        throw std::runtime_error("BGKOctoMap::merge: merge is defined for BGKOctoMap (variant 0) and BGKLOctoMap (variant 3) maps; GPOctoMap and BGKLVOctoMap fuse by other rules");
    la3dm_pack_header h;
    const la3dm_pack_header my = la3dm_pack::make_header(stream_params(create_params, resolution, block_depth), mine.original_size, nullptr, 0, 0);
    std::string bad = la3dm_pack::validate(stream, size, &h);
    if (bad.empty()) bad = la3dm_pack::mismatch(h, my);
    if (bad.empty() && (block_arr.size() + h.n_blocks) * (uint64_t)h.nodes_per_block > la3dm_pack::kPoolNodeLimit) {
        uint64_t created = 0;   // (only a stream this large is looked through twice)
        const la3dm_pack::Layout lk = la3dm_pack::layout(h.n_blocks, h.n_leaves, h.nodes_per_block);
        for (uint64_t b = 0; b < h.n_blocks; ++b) {
            int64_t key;
            std::memcpy(&key, (const uint8_t *)stream + lk.keys + 8 * b, 8);
            created += block_arr.find(key) == block_arr.end();
        }
        if ((block_arr.size() + created) * (uint64_t)h.nodes_per_block > la3dm_pack::kPoolNodeLimit) bad = "the merged pool would pass 2^32 nodes";
    }
    if (!bad.empty()) throw std::runtime_error("BGKOctoMap::merge: " + bad);
    const la3dm_pack::Layout l = la3dm_pack::layout(h.n_blocks, h.n_leaves, h.nodes_per_block);
    const uint32_t npb = h.nodes_per_block;
    const la3dm_merge::Rule rule = {h.block_depth,           my.init_A, my.init_B, create_params.free_thresh, create_params.occupied_thresh,
                                    create_params.var_thresh};
    la3dm_merge::Counts cells;
    std::vector<float> A1(npb), B1(npb), A2(npb), B2(npb);
    std::vector<uint8_t> S1(npb), S2(npb);
    for (uint64_t b = 0; b < h.n_blocks; ++b) {
        int64_t key;
        std::memcpy(&key, (const uint8_t *)stream + l.keys + 8 * b, 8);
        la3dm_pack::expand_block((const uint8_t *)stream, h, l, b, A2.data(), B2.data(), S2.data());
        auto it = block_arr.find(key);
        const bool created = it == block_arr.end();
        if (created) {
            it = block_arr.emplace(key, new Block(hash_key_to_block(key))).first;
            ++stats.n_created;
        } else {
            const OcTreeNode *slab = it->second->slab;
            for (uint32_t n = 0; n < npb; ++n) {
                A1[n] = slab[n].m_A;
                B1[n] = slab[n].m_B;
                S1[n] = (uint8_t)((uint8_t)slab[n].state | (slab[n].classified ? 0x80u : 0u));
            }
        }
        la3dm_merge::merge_block(rule, created, A1.data(), B1.data(), S1.data(), A2.data(), B2.data(), S2.data(), cells);
        it->second->load_nodes(A1.data(), B1.data(), S1.data(), npb);
    }
    stats.n_blocks = h.n_blocks;
    stats.cells_kept = cells.kept;
    stats.cells_copied = cells.copied;
    stats.cells_fused = cells.fused;
    return stats;
}

la3dm_merge_stats BGKOctoMap::merge(const BGKOctoMap &other) {
    if (&other == this) throw std::runtime_error("BGKOctoMap::merge: a map is not merged into itself");
    const std::vector<uint8_t> bytes = other.pack();   // (binds the other map; merge() binds this one again)
    return merge(bytes.data(), bytes.size());
}

la3dm_merge_stats BGKOctoMap::merge_file(const std::string &path) {
    std::ifstream in(path, std::ios::binary | std::ios::ate);
    if (!in) throw std::runtime_error("BGKOctoMap::merge_file: cannot open " + path);
    const std::streamsize size = in.tellg();
    std::vector<uint8_t> bytes((size_t)std::max<std::streamsize>(size, 0));
    in.seekg(0);
    if (!bytes.empty() && !in.read((char *)bytes.data(), size)) throw std::runtime_error("BGKOctoMap::merge_file: cannot read " + path);
    return merge(bytes.data(), bytes.size());
}

// ---- diff (include/la3dm_hip.h, la3dm_devmap_diff_host; the rule per block: diff_block.h) ----
void BGKOctoMap::diff(const void *stream, size_t size, const la3dm_diff_params &p, uint64_t cap, const la3dm_diff_out *out,
                      uint64_t *n_found, la3dm_diff_stats *stats) const {
    bind();
    if (dmap != nullptr) {   // on the pool; the mirror is not touched
        if (la3dm_devmap_diff_host(dmap, stream, size, &p, cap, out, n_found, stats) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::diff: ") + la3dm_last_error(ctx));
        return;
    }
    la3dm_pack_header h;
    const la3dm_pack_header my = la3dm_pack::make_header(stream_params(create_params, resolution, block_depth), mine.original_size, nullptr, 0, 0);
    std::string bad = la3dm_pack::validate(stream, size, &h);
    if (bad.empty()) bad = la3dm_pack::mismatch(h, my);
    if (bad.empty() && n_found == nullptr) bad = "n_found is NULL";
    if (bad.empty() && (p.pair_mask >> 25)) bad = "pair_mask has bits above bit 24 (25 pairs, bit 5 * then + now)";
    if (bad.empty() && (p.value_mask >> 5)) bad = "value_mask has bits above bit 4 (5 classes)";
    if (bad.empty() && cap > 0 && out == nullptr) bad = "out is NULL with cap > 0";
    if (!bad.empty()) throw std::runtime_error("BGKOctoMap::diff: " + bad);
    const la3dm_pack::Layout l = la3dm_pack::layout(h.n_blocks, h.n_leaves, h.nodes_per_block);
    const uint8_t *bytes = (const uint8_t *)stream;
    const uint32_t npb = h.nodes_per_block, fine = la3dm_diff::layer_base(h.block_depth - 1u);
    const la3dm_diff::Rule rule = {h.block_depth, my.init_A, my.init_B, p.pair_mask, p.value_mask};
    la3dm_diff::Counts cells;
    la3dm_diff::List list;
    list.cap = cap;
    std::vector<int64_t> key_of;   // per listed entry
    std::vector<float> A(npb), B(npb);
    std::vector<uint8_t> S(npb);
    la3dm_diff_stats st;
    std::memset(&st, 0, sizeof(st));
    const auto compare = [&](int64_t key, const la3dm_diff::StreamBlock *then, const Block *blk) {
        la3dm_diff::MapBlock now = {S.data(), A.data(), B.data()};
        if (blk != nullptr)
            for (uint32_t n = 0; n < npb; ++n) {
                A[n] = blk->slab[n].m_A;
                B[n] = blk->slab[n].m_B;
                S[n] = (uint8_t)((uint8_t)blk->slab[n].state | (blk->slab[n].classified ? 0x80u : 0u));
            }
        la3dm_diff::diff_block(rule, then, blk != nullptr ? &now : nullptr, cells, list);
        key_of.resize(list.cell.size(), key);
    };
    std::vector<int64_t> named(h.n_blocks);
    for (uint64_t b = 0; b < h.n_blocks; ++b) {
        std::memcpy(&named[b], bytes + l.keys + 8 * b, 8);
        const la3dm_diff::StreamBlock then = {bytes + l.mask + 4ull * b * l.W, la3dm_diff::word_at(bytes + l.leaf_off, b), bytes + l.state, bytes + l.A,
                                              bytes + l.B};
        const auto it = block_arr.find(named[b]);
        st.n_missing_now += it == block_arr.end();
        compare(named[b], &then, it == block_arr.end() ? nullptr : it->second);
    }
    if (p.map_only) {   // the map's other blocks, in the order pack() writes them
        std::sort(named.begin(), named.end());
        std::vector<int64_t> rest;
        for (const auto &kv : block_arr)
            if (!std::binary_search(named.begin(), named.end(), kv.first)) rest.push_back(kv.first);
        std::sort(rest.begin(), rest.end());
        for (const int64_t key : rest) compare(key, nullptr, block_arr.find(key)->second);
        st.n_map_only_blocks = rest.size();
    }
    if (cells.selected > 0xFFFFFFFFull)
        throw std::runtime_error("BGKOctoMap::diff: more than 2^32 - 1 cells are selected (" + std::to_string(cells.selected) + ")");
    const size_t m = list.cell.size();
    if (out != nullptr && m) {
        if (out->block_key) std::memcpy(out->block_key, key_of.data(), 8 * m);
        if (out->cell) std::memcpy(out->cell, list.cell.data(), 4 * m);
        if (out->code) std::memcpy(out->code, list.code.data(), m);
        if (out->A) std::memcpy(out->A, list.A.data(), 4 * m);
        if (out->B) std::memcpy(out->B, list.B.data(), 4 * m);
        if (out->centre)   // Block::get_loc of the finest node: the LUT entry + the block's centre
            for (size_t t = 0; t < m; ++t) {
                const point3f c = Block::key_loc_map[fine + list.cell[t]] + hash_key_to_block(key_of[t]);
                out->centre[3 * t] = c.x();
                out->centre[3 * t + 1] = c.y();
                out->centre[3 * t + 2] = c.z();
            }
    }
    *n_found = cells.selected;
    if (stats != nullptr) {
        st.n_stream_blocks = h.n_blocks;
        std::memcpy(st.pairs, cells.pairs, sizeof(st.pairs));
        std::memcpy(st.value_changed, cells.value_changed, sizeof(st.value_changed));
        *stats = st;
    }
}

void BGKOctoMap::diff(const BGKOctoMap &then, const la3dm_diff_params &p, uint64_t cap, const la3dm_diff_out *out, uint64_t *n_found,
                      la3dm_diff_stats *stats) const {
    const std::vector<uint8_t> bytes = then.pack();   // (binds the other map; diff() binds this one again)
    diff(bytes.data(), bytes.size(), p, cap, out, n_found, stats);
}

void BGKOctoMap::diff_file(const std::string &path, const la3dm_diff_params &p, uint64_t cap, const la3dm_diff_out *out, uint64_t *n_found,
                           la3dm_diff_stats *stats) const {
    std::ifstream in(path, std::ios::binary | std::ios::ate);
    if (!in) throw std::runtime_error("BGKOctoMap::diff_file: cannot open " + path);
    const std::streamsize size = in.tellg();
    std::vector<uint8_t> bytes((size_t)std::max<std::streamsize>(size, 0));
    in.seekg(0);
    if (!bytes.empty() && !in.read((char *)bytes.data(), size)) throw std::runtime_error("BGKOctoMap::diff_file: cannot read " + path);
    diff(bytes.data(), bytes.size(), p, cap, out, n_found, stats);
}

// ---- pack_region / erase_region / evict (include/la3dm_hip.h, la3dm_devmap_pack_region_host; the region: region_blocks.h) ----
la3dm_region_blocks::Box BGKOctoMap::region_box(const float *lo3, const float *hi3, bool inside, const char *who) const {
    bind();   // (block_to_hash_key divides by this map's block size)
    if (lo3 == nullptr || hi3 == nullptr) throw std::invalid_argument(std::string(who) + ": a region point is NULL");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(lo3[a]) || !std::isfinite(hi3[a])) throw std::invalid_argument(std::string(who) + ": a region point is not finite");
    la3dm_region_blocks::Box box;
    const std::string bad = la3dm_region_blocks::from_corner_keys(block_to_hash_key(lo3[0], lo3[1], lo3[2]), block_to_hash_key(hi3[0], hi3[1], hi3[2]), inside, &box);
    if (!bad.empty()) throw std::invalid_argument(std::string(who) + ": " + bad);
    return box;
}

std::vector<uint8_t> BGKOctoMap::pack_region(const float *lo3, const float *hi3, bool inside) const {
    const la3dm_region_blocks::Box box = region_box(lo3, hi3, inside, "BGKOctoMap::pack_region");
    return pack_blocks(&box, "BGKOctoMap::pack_region");
}

la3dm_erase_stats BGKOctoMap::erase_region(const float *lo3, const float *hi3, bool inside) {
    const la3dm_region_blocks::Box box = region_box(lo3, hi3, inside, "BGKOctoMap::erase_region");
    la3dm_erase_stats stats;
    std::memset(&stats, 0, sizeof(stats));
    if (dmap != nullptr && la3dm_devmap_erase_region_host(dmap, box.lo, box.hi, box.inside, &stats) != LA3DM_OK)
        throw std::runtime_error(std::string("BGKOctoMap::erase_region: ") + la3dm_last_error(ctx));
    // the container: the map itself in host mode; the mirror of a device-resident map, which sync_mirror only ever adds to
    uint64_t erased = 0;
    for (auto it = block_arr.begin(); it != block_arr.end();) {
        if (la3dm_region_blocks::selected(it->first, box)) {
            delete it->second;
            it = block_arr.erase(it);
            ++erased;
        } else {
            ++it;
        }
    }
    if (dmap != nullptr) {
        if (stats.n_removed) mirror_dirty = true;
        return stats;
    }
    stats.n_removed = erased;
    stats.n_blocks = block_arr.size();   // (n_moved: a host-mode map has no pool slots)
    return stats;
}

std::vector<uint8_t> BGKOctoMap::evict(const float *lo3, const float *hi3, bool inside, la3dm_erase_stats *stats) {
    std::vector<uint8_t> bytes = pack_region(lo3, hi3, inside);   // (on the host before the first block is removed)
    const la3dm_erase_stats s = erase_region(lo3, hi3, inside);
    if (stats) *stats = s;
    return bytes;
}

la3dm_erase_stats BGKOctoMap::evict_file(const std::string &path, const float *lo3, const float *hi3, bool inside) {
    write_renamed(pack_region(lo3, hi3, inside), path, "BGKOctoMap::evict_file");
    return erase_region(lo3, hi3, inside);
}

std::vector<float> BGKOctoMap::device_training_data() const {
    std::vector<float> out;
    if (dmap == nullptr) return out;
    uint32_t n = 0;
    la3dm_devmap_training_data(dmap, nullptr, 0, &n);
    out.resize(4 * (size_t)n);
    if (n && la3dm_devmap_training_data(dmap, out.data(), n, &n) != LA3DM_OK)
        throw std::runtime_error(std::string("BGKOctoMap::device_training_data: ") + la3dm_last_error(ctx));
    return out;
}

Block *BGKOctoMap::search(BlockHashKey key) const {
    sync_mirror();
    auto it = block_arr.find(key);
    return it == block_arr.end() ? nullptr : it->second;
}

OcTreeNode BGKOctoMap::search(point3f p) const {
    bind();
    Block *b = search(block_to_hash_key(p));
    return b == nullptr ? OcTreeNode() : OcTreeNode(b->search(p));
}

void BGKOctoMap::search_many(const float *xyz, size_t n, uint8_t *exists, float *A, float *B, uint8_t *state) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_search_host(dmap, xyz, (uint32_t)n, exists, A, B, state) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::search_many: ") + la3dm_last_error(ctx));
        return;
    }
    for (size_t i = 0; i < n; ++i) {
        const point3f p(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
        exists[i] = search(block_to_hash_key(p)) != nullptr;
        const OcTreeNode nd = search(p);
        A[i] = nd.m_A;
        B[i] = nd.m_B;
        state[i] = (uint8_t)nd.get_state();
    }
}

// The reference leaves this loop to its clients (a planner walks a RayCaster until it meets an OCCUPIED node); what is
// added is the covering leaf — after prune() the raw finest-layer node of a collapsed region reads PRUNED — and the
// batch.  The host form below is the definition; the device kernel (csrc/devmap_raycast.h) reproduces it bit for bit.
void BGKOctoMap::raycast_many(const float *rays6, size_t n, uint32_t stop_mask, uint32_t max_steps,
                              const la3dm_raycast_out &out) const {
    bind();
    if (max_steps == 0 || max_steps > LA3DM_RAY_MAX_STEPS)
        throw std::invalid_argument("BGKOctoMap::raycast_many: max_steps must be 1 ... 2^20");
    if (n > 0xFFFFFFFFull) throw std::invalid_argument("BGKOctoMap::raycast_many: more than 2^32 - 1 rays");
    if (n == 0) return;
    if (rays6 == nullptr || out.steps == nullptr || out.flags == nullptr)
        throw std::invalid_argument("BGKOctoMap::raycast_many: rays, steps and flags must not be NULL");
    if (dmap != nullptr) {
        if (la3dm_devmap_raycast_host(dmap, rays6, (uint32_t)n, stop_mask, max_steps, &out) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::raycast_many: ") + la3dm_last_error(ctx));
        return;
    }
    const OcTreeNode dflt;
    const unsigned dl = block_depth - 1u;
    for (size_t r = 0; r < n; ++r) {
        const float *q = rays6 + 6 * r;
        uint32_t steps = 0, counts[4] = {0, 0, 0, 0};
        uint8_t flags = 0, cls = LA3DM_RAY_MISSING, leaf_depth = 255;
        point3f p;
        BlockHashKey bk = 0;
        OcTreeHashKey nk = 0;
        float A = dflt.m_A, B = dflt.m_B;
        bool ok = true;  // refused before any (int) conversion: (int)(x / resolution) is undefined out there
        for (int a = 0; a < 6; ++a) ok &= std::fabs(q[a] / resolution) < 1073741824.0f;   // false for NaN and inf
        if (!ok) {
            flags = LA3DM_RAY_INVALID;
        } else {
            RayCaster rc(this, point3f(q[0], q[1], q[2]), point3f(q[3], q[4], q[5]));
            while (!rc.end()) {
                if (steps == max_steps) {
                    flags |= LA3DM_RAY_TRUNCATED;
                    break;
                }
                OcTreeNode nd;
                const bool valid = rc.next(p, nd, bk, nk);
                ++steps;
                if (valid) {
                    const Block *b = block_arr.find(bk)->second;
                    unsigned d = dl, i = (unsigned)(nk & 0xFFFF);
                    while (d > 0 && b->slab[layer_base(d) + i].state == State::PRUNED) {
                        --d;
                        i >>= 3;
                    }
                    const OcTreeNode &leaf = b->slab[layer_base(d) + i];
                    cls = (uint8_t)leaf.state;
                    leaf_depth = (uint8_t)d;
                    A = leaf.m_A;
                    B = leaf.m_B;
                } else {
                    cls = LA3DM_RAY_MISSING;
                    leaf_depth = 255;
                    A = dflt.m_A;
                    B = dflt.m_B;
                }
                ++counts[cls < 4 ? cls : 2];   // (a BGK-LV map's UNCERTAIN leaves count with UNKNOWN)
                if (stop_mask & (1u << cls)) {
                    flags |= LA3DM_RAY_HIT;
                    break;
                }
            }
        }
        out.steps[r] = steps;
        out.flags[r] = flags;
        if (out.p)
            for (unsigned a = 0; a < 3; ++a) out.p[3 * r + a] = p(a);
        if (out.block_key) out.block_key[r] = bk;
        if (out.node_key) out.node_key[r] = nk;
        if (out.cls) out.cls[r] = cls;
        if (out.leaf_depth) out.leaf_depth[r] = leaf_depth;
        if (out.A) out.A[r] = A;
        if (out.B) out.B[r] = B;
        if (out.counts)
            for (unsigned c = 0; c < 4; ++c) out.counts[4 * r + c] = counts[c];
    }
}

// ---- dense region reads: box / columns.  The host forms below are the definition; the device kernels
// (csrc/devmap_region.h) reproduce them bit for bit.
void BGKOctoMap::region_anchor(const float *lo3, const uint32_t *dims3, const la3dm_region::Query &q, bool has_mandatory,
                               const char *who, uint32_t g0[3], la3dm_region_info &info) const {
    la3dm_region::Anchor an;
    const std::string refusal = la3dm_region::resolve(q, lo3, dims3, resolution, block_size, block_depth, true, has_mandatory, ".", an);
    if (!refusal.empty()) throw std::invalid_argument(std::string("BGKOctoMap::") + who + ": " + refusal);
    const Block anchor(hash_key_to_block(an.block_key));
    const point3f o = anchor.get_point((unsigned short)an.cell[0], (unsigned short)an.cell[1], (unsigned short)an.cell[2]);
    for (int k = 0; k < 3; ++k) {
        g0[k] = an.g0[k];
        info.cell[k] = an.cell[k];
        info.origin[k] = o(k);
    }
    info.block_key = an.block_key;
}

// (have, b) is the caller's cache of the last block looked up (have = -1 before the first call): a run along z asks the
// block table once per block.  d = the leaf's layer, untouched where the block is missing.
const OcTreeNode *BGKOctoMap::covering_leaf_at(uint32_t gx, uint32_t gy, uint32_t gz, BlockHashKey &have, const Block *&b, unsigned &d) const {
    const unsigned dl = block_depth - 1u;
    const BlockHashKey key = ((BlockHashKey)(gx >> dl) << 40) | ((BlockHashKey)(gy >> dl) << 20) | (BlockHashKey)(gz >> dl);
    if (key != have) {
        auto it = block_arr.find(key);
        b = it == block_arr.end() ? nullptr : it->second;
        have = key;
    }
    if (b == nullptr) return nullptr;
    const uint32_t cm = (1u << dl) - 1u;
    unsigned n = (unsigned)(Block::get_node((unsigned short)(gx & cm), (unsigned short)(gy & cm), (unsigned short)(gz & cm)) & 0xFFFF);
    for (d = dl; d > 0 && b->slab[layer_base(d) + n].state == State::PRUNED; --d) n >>= 3;
    return &b->slab[layer_base(d) + n];
}

void BGKOctoMap::box(const float *lo3, const uint32_t *dims3, const la3dm_box_out &out, la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_box_host(dmap, lo3, dims3, &out, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::box: ") + la3dm_last_error(ctx));
        return;
    }
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::kBox, out.cls != nullptr, "box", g0, inf);
    if (info) *info = inf;
    const OcTreeNode dflt;
    const size_t ny = dims3[1], nz = dims3[2];
    for (uint32_t i = 0; i < dims3[0]; ++i)
        for (uint32_t j = 0; j < dims3[1]; ++j) {
            const Block *b = nullptr;
            BlockHashKey have = -1;
            for (uint32_t k = 0; k < dims3[2]; ++k) {
                unsigned d = 255;
                const OcTreeNode *leaf = covering_leaf_at(g0[0] + i, g0[1] + j, g0[2] + k, have, b, d);
                const size_t o = ((size_t)i * ny + j) * nz + k;
                out.cls[o] = leaf ? (uint8_t)leaf->state : (uint8_t)LA3DM_RAY_MISSING;
                if (out.leaf_depth) out.leaf_depth[o] = (uint8_t)d;
                if (out.A) out.A[o] = (leaf ? leaf : &dflt)->m_A;
                if (out.B) out.B[o] = (leaf ? leaf : &dflt)->m_B;
            }
        }
}

void BGKOctoMap::columns(const float *lo3, const uint32_t *dims3, const la3dm_columns_out &out, la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_columns_host(dmap, lo3, dims3, &out, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::columns: ") + la3dm_last_error(ctx));
        return;
    }
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::kColumns, out.counts != nullptr, "columns", g0, inf);
    if (info) *info = inf;
    for (uint32_t i = 0; i < dims3[0]; ++i)
        for (uint32_t j = 0; j < dims3[1]; ++j) {
            uint32_t counts[4] = {0, 0, 0, 0};
            int32_t low = -1, top = -1;
            const Block *b = nullptr;
            BlockHashKey have = -1;
            for (uint32_t k = 0; k < dims3[2]; ++k) {
                unsigned d;
                const OcTreeNode *leaf = covering_leaf_at(g0[0] + i, g0[1] + j, g0[2] + k, have, b, d);
                const unsigned cls = leaf ? (unsigned)leaf->state : (unsigned)LA3DM_RAY_MISSING;
                ++counts[cls < 4 ? cls : 2];   // (a BGK-LV map's UNCERTAIN leaves count with UNKNOWN)
                if (cls == (unsigned)State::OCCUPIED) {
                    if (low < 0) low = (int32_t)k;
                    top = (int32_t)k;
                }
            }
            const size_t c = (size_t)i * dims3[1] + j;
            for (unsigned q = 0; q < 4; ++q) out.counts[4 * c + q] = counts[q];
            if (out.low_occ) out.low_occ[c] = low;
            if (out.top_occ) out.top_occ[c] = top;
        }
}

// ---- distance field of a region.  The host form below is the definition; the device kernels (csrc/devmap_distance.h)
// reproduce it bit for bit.  Separable and exact: the distance along z to the nearest obstacle of the line (saturated at
// radius + 1, squared), then min-plus passes along y and x over a window of +-radius — if D(v) <= radius^2 every axis
// offset to the minimiser is <= radius, and a sum that holds a saturated term exceeds radius^2 and ends as FAR.
namespace {
// out[l] = min over |d| <= radius of in[l + d] + d^2 along lines of length L whose elements lie S apart
void df_min_plus(const uint32_t *in, uint32_t *out, size_t planes, size_t L, size_t S, uint32_t radius) {
#pragma omp parallel for collapse(2) schedule(static)
    for (size_t p = 0; p < planes; ++p)
        for (size_t l = 0; l < L; ++l) {
            const uint32_t *line = in + p * L * S;
            for (size_t c = 0; c < S; ++c) {
                uint32_t best = line[l * S + c];
                for (uint32_t d = 1; d <= radius && d * d < best; ++d) {
                    if (l >= d) best = std::min(best, line[(l - d) * S + c] + d * d);
                    if (l + d < L) best = std::min(best, line[(l + d) * S + c] + d * d);
                }
                out[(p * L + l) * S + c] = best;
            }
        }
}

// the classes of a region's voxels, as box reads them
std::vector<uint8_t> region_classes(const BGKOctoMap &map, const float *lo3, const uint32_t *dims3) {
    std::vector<uint8_t> cls((size_t)dims3[0] * dims3[1] * dims3[2]);
    map.box(lo3, dims3, la3dm_box_out{cls.data(), nullptr, nullptr, nullptr}, nullptr);
    return cls;
}

// the obstacle field of a region: distance_field's d2 words
std::vector<uint32_t> region_d2(const BGKOctoMap &map, const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask, uint32_t radius) {
    std::vector<uint32_t> d2((size_t)dims3[0] * dims3[1] * dims3[2]);
    map.distance_field(lo3, dims3, obstacle_mask, radius, la3dm_distance_out{d2.data(), nullptr}, nullptr);
    return d2;
}

// The moves of a connectivity in ascending order of their code (di + 1) * 9 + (dj + 1) * 3 + (dk + 1): the order in which
// every host form tries its neighbours, and so the order its ties are broken in.  len = the non-zero components.
struct Move {
    int d[3], len;
    uint32_t code;
    ptrdiff_t offset(ptrdiff_t sx, ptrdiff_t sy) const { return d[0] * sx + d[1] * sy + d[2]; }   // in an array with these strides
};
std::vector<Move> connectivity_moves(uint32_t connectivity) {
    std::vector<Move> moves;
    for (int di = -1; di <= 1; ++di)
        for (int dj = -1; dj <= 1; ++dj)
            for (int dk = -1; dk <= 1; ++dk) {
                const int len = std::abs(di) + std::abs(dj) + std::abs(dk);
                if (len >= 1 && len <= la3dm_region::move_reach(connectivity))
                    moves.push_back(Move{{di, dj, dk}, len, (uint32_t)((di + 1) * 9 + (dj + 1) * 3 + (dk + 1))});
            }
    return moves;
}
}  // namespace

void BGKOctoMap::distance_field(const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask, uint32_t radius,
                                const la3dm_distance_out &out, la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_distance_host(dmap, lo3, dims3, obstacle_mask, radius, &out, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::distance_field: ") + la3dm_last_error(ctx));
        return;
    }
    const std::string refusal = la3dm_region::distance_check(obstacle_mask, radius);
    if (!refusal.empty()) throw std::invalid_argument("BGKOctoMap::distance_field: " + refusal);
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::kDistance, out.d2 != nullptr || out.dist != nullptr, "distance_field", g0, inf);
    if (info) *info = inf;
    const size_t nx = dims3[0], ny = dims3[1], nz = dims3[2], n = nx * ny * nz;
    const std::vector<uint8_t> cls = region_classes(*this, lo3, dims3);
    std::vector<uint32_t> f(n), g(n);
    const uint32_t sat = radius + 1u;
#pragma omp parallel for schedule(static)
    for (size_t line = 0; line < nx * ny; ++line) {   // z: a sweep up and a sweep down the line
        const uint8_t *c = cls.data() + line * nz;
        uint32_t *p = f.data() + line * nz;
        uint32_t run = sat;
        for (size_t k = 0; k < nz; ++k) {
            run = ((obstacle_mask >> c[k]) & 1u) ? 0u : std::min(run + 1u, sat);
            p[k] = run;
        }
        run = sat;
        for (size_t k = nz; k-- > 0;) {
            run = ((obstacle_mask >> c[k]) & 1u) ? 0u : std::min(run + 1u, sat);
            p[k] = std::min(p[k], run);
        }
        for (size_t k = 0; k < nz; ++k) p[k] *= p[k];
    }
    df_min_plus(f.data(), g.data(), nx, ny, nz, radius);        // y
    df_min_plus(g.data(), f.data(), 1, nx, ny * nz, radius);    // x
    const uint32_t r2 = radius * radius;
    const float res = resolution;
    for (size_t v = 0; v < n; ++v) {
        const bool far = f[v] > r2;
        if (out.d2) out.d2[v] = far ? LA3DM_DF_FAR : f[v];
        if (out.dist) out.dist[v] = far ? std::numeric_limits<float>::infinity() : sqrtf((float)f[v]) * res;
    }
}

// ---- nearest and nearest_points: the feature transform of a region.  The host form below is the definition; the device
// kernels (csrc/devmap_nearest.h) reproduce it exactly.  distance_field's three stages, each keeping its argmin with the
// smaller coordinate on a tie (host/nearest_lines.h, where the tie-break argument stands); the last stage follows the
// three offsets to the obstacle.
namespace {
// index and / or d2 (either may be null) of every voxel of a region with the classes cls
void feature_transform(const std::vector<uint8_t> &cls, const uint32_t *dims3, uint32_t obstacle_mask, uint32_t radius, uint32_t *index,
                       uint32_t *d2) {
    namespace nt = la3dm_nearest;
    const size_t nx = dims3[0], ny = dims3[1], nz = dims3[2], n = nx * ny * nz;
    std::vector<int16_t> az(n);
    std::vector<uint32_t> ky(n);
#pragma omp parallel
    {
        std::vector<uint8_t> obstacle(nz);
#pragma omp for schedule(static)
        for (size_t line = 0; line < nx * ny; ++line) {   // z
            for (size_t k = 0; k < nz; ++k) obstacle[k] = (uint8_t)((obstacle_mask >> cls[line * nz + k]) & 1u);
            nt::line_z(obstacle.data(), nz, radius, az.data() + line * nz);
        }
    }
#pragma omp parallel for collapse(2) schedule(static)
    for (size_t i = 0; i < nx; ++i)   // y: the lines (i, *, k)
        for (size_t k = 0; k < nz; ++k) {
            const int16_t *in = az.data() + i * ny * nz + k;
            uint32_t *out = ky.data() + i * ny * nz + k;
            nt::line_pass(
                ny, radius, [&](size_t j) { return nt::offset_term(in[j * nz]); }, [&](size_t j, uint32_t key) { out[j * nz] = key; });
        }
    const uint32_t r2 = radius * radius;
    const size_t S = ny * nz;
#pragma omp parallel for schedule(static)
    for (size_t c = 0; c < S; ++c) {   // x: the lines (*, j, k), and the chase
        const size_t j = c / nz, k = c % nz;
        nt::line_pass(
            nx, radius, [&](size_t i) { return nt::key_sum(ky[i * S + c]); },
            [&](size_t i, uint32_t key) {
                const uint32_t sum = nt::key_sum(key);
                const bool far = sum > r2;
                if (d2) d2[i * S + c] = far ? LA3DM_DF_FAR : sum;
                if (!index) return;
                if (far) {
                    index[i * S + c] = LA3DM_NEAREST_NONE;
                    return;
                }
                const size_t i2 = (size_t)((ptrdiff_t)i + nt::key_offset(key));
                const size_t j2 = (size_t)((ptrdiff_t)j + nt::key_offset(ky[i2 * S + c]));
                const size_t k2 = (size_t)((ptrdiff_t)k + az[(i2 * ny + j2) * nz + k]);
                index[i * S + c] = (uint32_t)((i2 * ny + j2) * nz + k2);
            });
    }
}
}  // namespace

void BGKOctoMap::nearest(const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask, uint32_t radius, const la3dm_nearest_out &out,
                         la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_nearest_host(dmap, lo3, dims3, obstacle_mask, radius, &out, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::nearest: ") + la3dm_last_error(ctx));
        return;
    }
    const std::string refusal = la3dm_region::nearest_check(obstacle_mask, radius, 0);
    if (!refusal.empty()) throw std::invalid_argument("BGKOctoMap::nearest: " + refusal);
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::kNearest, out.index != nullptr || out.d2 != nullptr, "nearest", g0, inf);
    if (info) *info = inf;
    feature_transform(region_classes(*this, lo3, dims3), dims3, obstacle_mask, radius, out.index, out.d2);
}

// a loop over world_voxel — after score_voxel's transform where a pose is given — and two gathers
void BGKOctoMap::nearest_points(const float *lo3, const uint32_t *dims3, const float *points3, uint32_t n_points, const float *pose12,
                                uint32_t obstacle_mask, uint32_t radius, const la3dm_nearest_points_out &out, la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_nearest_points_host(dmap, lo3, dims3, points3, n_points, pose12, obstacle_mask, radius, &out, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::nearest_points: ") + la3dm_last_error(ctx));
        return;
    }
    const std::string w = "BGKOctoMap::nearest_points";
    std::string refusal = la3dm_region::nearest_check(obstacle_mask, radius, n_points);
    if (!refusal.empty()) throw std::invalid_argument(w + ": " + refusal);
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::kNearestPoints, true, "nearest_points", g0, inf);
    refusal = la3dm_region::nearest_buffers(n_points, points3 != nullptr, true, out.cls || out.voxel || out.index || out.d2);
    if (!refusal.empty()) throw std::invalid_argument(w + ": " + refusal);
    if (info) *info = inf;
    if (n_points == 0) return;
    const size_t n = (size_t)dims3[0] * dims3[1] * dims3[2];
    std::vector<uint32_t> index(n), d2(n);
    feature_transform(region_classes(*this, lo3, dims3), dims3, obstacle_mask, radius, index.data(), d2.data());
    const int lim = 1 << (block_depth - 1);
#pragma omp parallel for schedule(static)
    for (uint32_t p = 0; p < n_points; ++p) {
        const float *q = points3 + 3 * (size_t)p;
        uint32_t f = 0;
        uint32_t cls = pose12 ? la3dm_region::score_voxel(pose12, q[0], q[1], q[2], resolution, block_size, lim, g0, dims3, f)
                              : la3dm_region::world_voxel(q, resolution, block_size, lim, g0, dims3, f);
        const bool inside = cls == LA3DM_SCORE_HIT;
        if (inside) cls = la3dm_region::score_class(d2[f]);
        if (out.cls) out.cls[p] = (uint8_t)cls;
        if (out.voxel) out.voxel[p] = inside ? f : LA3DM_NEAREST_NONE;
        if (out.index) out.index[p] = inside ? index[f] : LA3DM_NEAREST_NONE;
        if (out.d2) out.d2[p] = inside ? d2[f] : LA3DM_DF_FAR;
    }
}

// ---- frontier of a region.  The host form below is the definition; the device kernels (csrc/devmap_frontier.h)
// reproduce it bit for bit.  The classes of the region padded by one voxel on every side are read as box reads them (the
// lattice does not stop at the region's faces); a voxel's score is the number of its neighbours whose class is in
// unknown_mask if its own class is in open_mask, else 0.
void BGKOctoMap::frontier(const float *lo3, const uint32_t *dims3, uint32_t open_mask, uint32_t unknown_mask, uint32_t connectivity,
                          uint32_t min_neighbours, uint64_t cap, const la3dm_frontier_out &out, uint64_t *n_found,
                          la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_frontier_host(dmap, lo3, dims3, open_mask, unknown_mask, connectivity, min_neighbours, cap, &out, n_found, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::frontier: ") + la3dm_last_error(ctx));
        return;
    }
    const std::string w = "BGKOctoMap::frontier";
    const std::string refusal = la3dm_region::frontier_check(open_mask, unknown_mask, connectivity, min_neighbours);
    if (!refusal.empty()) throw std::invalid_argument(w + ": " + refusal);
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::kFrontier, true, "frontier", g0, inf);
    if (cap > 0 && out.index == nullptr) throw std::invalid_argument(w + ": out.index must not be NULL with cap > 0");
    if (n_found == nullptr) throw std::invalid_argument(w + ": n_found is NULL");
    if (info) *info = inf;
    const size_t nx = dims3[0], ny = dims3[1], nz = dims3[2];
    const size_t PY = ny + 2, PZ = nz + 2, P = (nx + 2) * PY * PZ;
    // classes of the padded box: box's loop at the lattice positions g0 - 1 + (i, j, k)
    std::vector<uint8_t> cls(P);
#pragma omp parallel for schedule(static)
    for (size_t row = 0; row < (nx + 2) * PY; ++row) {
        const uint32_t gx = g0[0] - 1u + (uint32_t)(row / PY), gy = g0[1] - 1u + (uint32_t)(row % PY);
        const Block *b = nullptr;
        BlockHashKey have = -1;
        for (size_t k = 0; k < PZ; ++k) {
            unsigned d;
            const OcTreeNode *leaf = covering_leaf_at(gx, gy, g0[2] - 1u + (uint32_t)k, have, b, d);
            cls[row * PZ + k] = leaf ? (uint8_t)leaf->state : (uint8_t)LA3DM_RAY_MISSING;
        }
    }
    std::vector<ptrdiff_t> offs;
    for (const Move &m : connectivity_moves(connectivity)) offs.push_back(m.offset((ptrdiff_t)(PY * PZ), (ptrdiff_t)PZ));
    // per (i, j) row of the region: its scores and how many of them reach min_neighbours; then the rows' places in the list
    std::vector<uint8_t> own_score;
    uint8_t *score = out.score;
    if (score == nullptr) {
        own_score.resize(nx * ny * nz);
        score = own_score.data();
    }
    std::vector<uint64_t> row_start(nx * ny + 1, 0);
#pragma omp parallel for schedule(static)
    for (size_t row = 0; row < nx * ny; ++row) {
        const size_t i = row / ny, j = row % ny;
        const uint8_t *c = cls.data() + ((i + 1) * PY + (j + 1)) * PZ + 1;
        uint64_t found = 0;
        for (size_t k = 0; k < nz; ++k) {
            uint32_t sc = 0;
            if ((open_mask >> c[k]) & 1u)
                for (const ptrdiff_t o : offs) sc += (unknown_mask >> c[(ptrdiff_t)k + o]) & 1u;
            score[row * nz + k] = (uint8_t)sc;
            found += sc >= min_neighbours ? 1u : 0u;
        }
        row_start[row + 1] = found;
    }
    for (size_t row = 0; row < nx * ny; ++row) row_start[row + 1] += row_start[row];
    *n_found = row_start[nx * ny];
#pragma omp parallel for schedule(static)
    for (size_t row = 0; row < nx * ny; ++row) {
        uint64_t t = row_start[row];
        for (size_t k = 0; k < nz && t < cap; ++k) {
            const uint8_t sc = score[row * nz + k];
            if (sc < min_neighbours) continue;
            out.index[t] = (uint32_t)(row * nz + k);
            if (out.nbrs) out.nbrs[t] = sc;
            ++t;
        }
    }
}

// ---- footing of a region.  The host form is the definition; the device kernels (csrc/devmap_footing.h) reproduce it
// exactly.  The classes of the padded box — r voxels round the region in x and y, 1 + s below, h - 1 + s above — are read
// as box reads them (the lattice does not stop at the region's faces); host/footing_cells.h does the rest.
void BGKOctoMap::footing(const float *lo3, const uint32_t *dims3, const la3dm_footing_params *p, uint64_t cap, const la3dm_footing_out &out,
                         uint64_t *n_found, la3dm_footing_stats *stats, la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_footing_host(dmap, lo3, dims3, p, cap, &out, n_found, stats, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::footing: ") + la3dm_last_error(ctx));
        return;
    }
    const std::string w = "BGKOctoMap::footing";
    const std::string refusal = la3dm_region::footing_check(p, cap, out.index != nullptr, ".");
    if (!refusal.empty()) throw std::invalid_argument(w + ": " + refusal);
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::footing_query(*p), true, "footing", g0, inf);
    if (n_found == nullptr) throw std::invalid_argument(w + ": n_found is NULL");
    if (info) *info = inf;
    const la3dm_footing::Params fp = la3dm_region::footing_params(*p);
    size_t P[3];
    la3dm_footing::padded_dims(dims3, fp, P);
    const uint32_t below[3] = {p->radius, p->radius, 1u + p->step};
    // classes of the padded box: box's loop at the lattice positions g0 - below + (i, j, k)
    std::vector<uint8_t> cls(P[0] * P[1] * P[2]);
#pragma omp parallel for schedule(static)
    for (size_t row = 0; row < P[0] * P[1]; ++row) {
        const uint32_t gx = g0[0] - below[0] + (uint32_t)(row / P[1]), gy = g0[1] - below[1] + (uint32_t)(row % P[1]);
        const Block *b = nullptr;
        BlockHashKey have = -1;
        for (size_t k = 0; k < P[2]; ++k) {
            unsigned d;
            const OcTreeNode *leaf = covering_leaf_at(gx, gy, g0[2] - below[2] + (uint32_t)k, have, b, d);
            cls[row * P[2] + k] = leaf ? (uint8_t)leaf->state : (uint8_t)LA3DM_RAY_MISSING;
        }
    }
    const la3dm_footing::Counts n = la3dm_footing::cells(cls.data(), dims3, fp, nullptr, cap, out.index, out.levels, out.lowest, out.highest);
    *n_found = n.n_foot;
    if (stats) *stats = la3dm_footing_stats{(uint32_t)n.n_stand, (uint32_t)n.n_body, (uint32_t)n.n_foot, la3dm_footing::disc_cells(p->radius)};
}

// ---- surface of a region.  The host form is the definition; the device kernels (csrc/devmap_surface.h) reproduce it
// exactly.  The classes of the padded box — smooth + 1 voxels round the region on every side — are read as box reads them
// (the lattice does not stop at the region's faces); host/surface_cells.h does the rest.
void BGKOctoMap::surface(const float *lo3, const uint32_t *dims3, const la3dm_surface_params *p, uint64_t cap, const la3dm_surface_out &out,
                         uint64_t *n_found, la3dm_surface_stats *stats, la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_surface_host(dmap, lo3, dims3, p, cap, &out, n_found, stats, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::surface: ") + la3dm_last_error(ctx));
        return;
    }
    const std::string w = "BGKOctoMap::surface";
    const std::string refusal = la3dm_region::surface_check(p, cap, &out, ".");
    if (!refusal.empty()) throw std::invalid_argument(w + ": " + refusal);
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::surface_query(*p), true, "surface", g0, inf);
    if (n_found == nullptr) throw std::invalid_argument(w + ": n_found is NULL");
    if (info) *info = inf;
    const la3dm_surface::Params sp = la3dm_region::surface_params(*p);
    size_t P[3];
    la3dm_surface::padded_dims(dims3, sp, P);
    const uint32_t below = p->smooth + 1u;
    // classes of the padded box: box's loop at the lattice positions g0 - below + (i, j, k)
    std::vector<uint8_t> cls(P[0] * P[1] * P[2]);
#pragma omp parallel for schedule(static)
    for (size_t row = 0; row < P[0] * P[1]; ++row) {
        const uint32_t gx = g0[0] - below + (uint32_t)(row / P[1]), gy = g0[1] - below + (uint32_t)(row % P[1]);
        const Block *b = nullptr;
        BlockHashKey have = -1;
        for (size_t k = 0; k < P[2]; ++k) {
            unsigned d;
            const OcTreeNode *leaf = covering_leaf_at(gx, gy, g0[2] - below + (uint32_t)k, have, b, d);
            cls[row * P[2] + k] = leaf ? (uint8_t)leaf->state : (uint8_t)LA3DM_RAY_MISSING;
        }
    }
    const la3dm_surface::Counts n = la3dm_surface::cells(cls.data(), dims3, sp, cap, out.index, out.faces, out.normal, out.dense_faces);
    *n_found = n.n_surface;
    if (stats) {
        stats->n_solid = n.n_solid;
        stats->n_surface = n.n_surface;
        for (int d = 0; d < 6; ++d) stats->faces[d] = n.faces[d];
    }
}

// ---- reach over a region.  The host form below is the definition; the device kernels (csrc/devmap_reach.h) reproduce
// it bit for bit.  A queue BFS over the passable voxels of the box padded by one voxel that is never passable, so a
// neighbour is an index offset with no test at the faces.
void BGKOctoMap::reach(const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds, uint32_t pass_mask,
                       uint32_t obstacle_mask, uint32_t clearance, uint32_t connectivity, uint32_t max_steps, const uint32_t *targets,
                       uint32_t n_targets, const la3dm_reach_out &out, la3dm_reach_stats *stats, la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_reach_host(dmap, lo3, dims3, seeds, n_seeds, pass_mask, obstacle_mask, clearance, connectivity, max_steps,
                                    targets, n_targets, &out, stats, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::reach: ") + la3dm_last_error(ctx));
        return;
    }
    const std::string refusal = la3dm_region::reach_check(pass_mask, obstacle_mask, clearance, connectivity, max_steps, n_seeds, n_targets,
                                                          seeds != nullptr, targets != nullptr, true, out.steps != nullptr,
                                                          out.target_steps != nullptr, ".");
    if (!refusal.empty()) throw std::invalid_argument("BGKOctoMap::reach: " + refusal);
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::kReach, true, "reach", g0, inf);
    if (info) *info = inf;
    const size_t nx = dims3[0], ny = dims3[1], nz = dims3[2], n = nx * ny * nz;
    const size_t PY = ny + 2, PZ = nz + 2;
    const std::vector<uint8_t> cls = region_classes(*this, lo3, dims3);
    std::vector<uint32_t> d2;
    if (clearance > 0) d2 = region_d2(*this, lo3, dims3, obstacle_mask, clearance);
    // open[p] = 1: padded voxel p is passable and not reached yet
    std::vector<uint8_t> open((nx + 2) * PY * PZ, 0);
    const auto padded = [&](size_t f) { return ((f / (ny * nz) + 1) * PY + (f / nz) % ny + 1) * PZ + f % nz + 1; };
    const auto unpadded = [&](size_t p) { return ((p / (PY * PZ) - 1) * ny + (p / PZ) % PY - 1) * nz + p % PZ - 1; };
    for (size_t f = 0; f < n; ++f)
        open[padded(f)] = ((pass_mask >> cls[f]) & 1u) && (clearance == 0 || d2[f] == LA3DM_DF_FAR) ? 1 : 0;
    std::vector<ptrdiff_t> offs;
    for (const Move &m : connectivity_moves(connectivity)) offs.push_back(m.offset((ptrdiff_t)(PY * PZ), (ptrdiff_t)PZ));
    std::vector<uint32_t> own_steps;
    uint32_t *steps = out.steps;
    if (steps == nullptr) {
        own_steps.resize(n);
        steps = own_steps.data();
    }
    std::fill(steps, steps + n, LA3DM_REACH_NONE);
    la3dm_reach_stats s = {0, 0, 0};
    std::vector<size_t> wave, next;
    for (uint32_t t = 0; t < n_seeds; ++t) {
        if (seeds[t] >= n) continue;
        const size_t p = padded(seeds[t]);
        if (!open[p]) continue;   // not passable, or listed before
        open[p] = 0;
        steps[seeds[t]] = 0;
        wave.push_back(p);
    }
    s.n_seeded = s.n_reached = (uint32_t)wave.size();
    for (uint32_t level = 1; level <= max_steps && !wave.empty(); ++level) {
        next.clear();
        for (const size_t p : wave)
            for (const ptrdiff_t o : offs) {
                const size_t q = (size_t)((ptrdiff_t)p + o);
                if (!open[q]) continue;
                open[q] = 0;
                steps[unpadded(q)] = level;
                next.push_back(q);
            }
        if (!next.empty()) {
            s.levels = level;
            s.n_reached += (uint32_t)next.size();
        }
        wave.swap(next);
    }
    for (uint32_t t = 0; t < n_targets; ++t) out.target_steps[t] = targets[t] < n ? steps[targets[t]] : LA3DM_REACH_NONE;
    if (stats) *stats = s;
}

// ---- travel over a region.  The host form below is the definition; the device kernels (csrc/devmap_travel.h) reproduce
// it bit for bit.  box's classes and the host distance transform give every voxel its entry word (pen(v), or blocked);
// Dijkstra with a binary heap gives the costs — a candidate above max_cost is dropped where it is made, which changes no
// cost <= max_cost because every prefix of a least-cost walk is cheaper than the walk — and a pass over the voxels the
// parents, which are a function of the costs alone.
void BGKOctoMap::travel(const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds, const la3dm_travel_params &p,
                        const uint32_t *targets, uint32_t n_targets, const la3dm_travel_out &out, la3dm_travel_stats *stats,
                        la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_travel_host(dmap, lo3, dims3, seeds, n_seeds, &p, targets, n_targets, &out, stats, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::travel: ") + la3dm_last_error(ctx));
        return;
    }
    const std::string refusal = la3dm_region::travel_check(&p, n_seeds, n_targets, seeds != nullptr, targets != nullptr, true,
                                                           out.cost != nullptr, out.target_cost != nullptr, ".");
    if (!refusal.empty()) throw std::invalid_argument("BGKOctoMap::travel: " + refusal);
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::kTravel, true, "travel", g0, inf);
    if (info) *info = inf;
    const uint32_t nx = dims3[0], ny = dims3[1], nz = dims3[2];
    const size_t n = (size_t)nx * ny * nz;
    const std::vector<uint8_t> cls = region_classes(*this, lo3, dims3);
    const uint32_t R = std::max(p.clearance, p.soft_radius);
    std::vector<uint32_t> d2;
    if (R > 0) d2 = region_d2(*this, lo3, dims3, p.obstacle_mask, R);
    std::vector<uint32_t> entry(n);   // pen(v), or blocked
    for (size_t f = 0; f < n; ++f)
        entry[f] = ((p.pass_mask >> cls[f]) & 1u) ? la3dm_region::travel_entry(p, R > 0 ? d2[f] : LA3DM_DF_FAR) : la3dm_region::kTravelBlocked;
    const std::vector<Move> moves = connectivity_moves(p.connectivity);   // in the order of the code q
    std::vector<uint32_t> own_cost;
    uint32_t *cost = out.cost;
    if (cost == nullptr) {
        own_cost.resize(n);
        cost = own_cost.data();
    }
    std::fill(cost, cost + n, LA3DM_TRAVEL_NONE);
    la3dm_travel_stats s;
    std::memset(&s, 0, sizeof(s));
    typedef std::pair<uint32_t, uint32_t> Item;   // (cost, flat index)
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    for (uint32_t t = 0; t < n_seeds; ++t) {
        const uint32_t f = seeds[t];
        if (f >= n || entry[f] == la3dm_region::kTravelBlocked || cost[f] == 0) continue;   // out of range, not passable, listed before
        cost[f] = 0;
        ++s.n_seeded;
        heap.push(Item(0u, f));
    }
    // neighbour u of voxel (i, j, k) along m, or n where it leaves the region
    const auto neighbour = [&](uint32_t i, uint32_t j, uint32_t k, const Move &m) -> size_t {
        const uint32_t ui = i + (uint32_t)m.d[0], uj = j + (uint32_t)m.d[1], uk = k + (uint32_t)m.d[2];   // (0 - 1 wraps above nx)
        return ui < nx && uj < ny && uk < nz ? ((size_t)ui * ny + uj) * nz + uk : n;
    };
    while (!heap.empty()) {
        const Item top = heap.top();
        heap.pop();
        const uint32_t f = top.second;
        if (top.first != cost[f]) continue;   // a stale entry
        const uint32_t k = f % nz, j = (f / nz) % ny, i = f / (nz * ny);
        for (const Move &m : moves) {
            const size_t v = neighbour(i, j, k, m);
            if (v == n || entry[v] == la3dm_region::kTravelBlocked) continue;
            const uint32_t cand = top.first + p.move_cost[m.len - 1] + entry[v];   // <= 2^31 + 2^17
            if (cand > p.max_cost || cand >= cost[v]) continue;
            cost[v] = cand;
            heap.push(Item(cand, (uint32_t)v));
        }
    }
    for (size_t f = 0; f < n; ++f) {
        if (cost[f] != LA3DM_TRAVEL_NONE) {
            ++s.n_reached;
            s.max_cost = std::max(s.max_cost, cost[f]);
        }
        if (out.parent == nullptr) continue;
        uint8_t code = cost[f] == LA3DM_TRAVEL_NONE ? 255 : 13;
        if (cost[f] != LA3DM_TRAVEL_NONE && cost[f] != 0) {
            const uint32_t k = (uint32_t)(f % nz), j = (uint32_t)((f / nz) % ny), i = (uint32_t)(f / ((size_t)nz * ny));
            for (const Move &m : moves) {
                const size_t u = neighbour(i, j, k, m);
                if (u != n && cost[u] != LA3DM_TRAVEL_NONE && cost[u] + p.move_cost[m.len - 1] + entry[f] == cost[f]) {
                    code = (uint8_t)m.code;
                    break;
                }
            }
        }
        out.parent[f] = code;
    }
    for (uint32_t t = 0; t < n_targets; ++t) out.target_cost[t] = targets[t] < n ? cost[targets[t]] : LA3DM_TRAVEL_NONE;
    if (stats) *stats = s;
}

// ---- drive over a region.  host/drive_cells.h is the definition; the device kernels (csrc/devmap_drive.h) reproduce it
// bit for bit.  Here the member bytes are built: from the list, or from this map's own footing over the same region.
void BGKOctoMap::drive(const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds, const la3dm_drive_params *p,
                       const uint32_t *targets, uint32_t n_targets, const la3dm_drive_out *out, la3dm_drive_stats *stats,
                       la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_drive_host(dmap, lo3, dims3, seeds, n_seeds, p, targets, n_targets, out, stats, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::drive: ") + la3dm_last_error(ctx));
        return;
    }
    const std::string w = "BGKOctoMap::drive: ";
    std::string refusal = la3dm_region::drive_check(p, n_seeds, n_targets, seeds != nullptr, targets != nullptr, out, ".");
    if (refusal.empty() && p->footing) refusal = la3dm_region::footing_check(p->footing, 0, false, ".");
    if (!refusal.empty()) throw std::invalid_argument(w + refusal);
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::kDrive, true, "drive", g0, inf);
    if (p->footing) region_anchor(lo3, dims3, la3dm_region::footing_query(*p->footing), true, "drive", g0, inf);   // the padded box
    const size_t n = (size_t)dims3[0] * dims3[1] * dims3[2];
    std::vector<uint8_t> member(n, 0);
    if (p->footing) {
        std::vector<uint32_t> index(n);
        uint64_t found = 0;
        la3dm_footing_out fo = la3dm_footing_out();
        fo.index = index.data();
        footing(lo3, dims3, p->footing, n, fo, &found);
        for (uint64_t t = 0; t < found; ++t) member[index[t]] = 1;
    } else {
        for (uint32_t t = 0; t < p->n_members; ++t)
            if (p->members[t] < n) member[p->members[t]] = 1;
    }
    const la3dm_drive::Counts c = la3dm_drive::cells(dims3, member.data(), seeds, n_seeds, targets, n_targets, p->members, p->n_members,
                                                     la3dm_region::drive_params(*p), out->cost, out->parent, out->of_member, out->target_cost,
                                                     out->target_index);
    if (info) *info = inf;
    if (stats) *stats = la3dm_drive_stats{c.n_members, c.n_seeded, c.n_reached, c.max_cost, 0, 0, 0};
}

// ---- clusters of a region.  The host form below is the definition; the device kernels (csrc/devmap_clusters.h) reproduce
// it bit for bit.  box's classes (and the list) give the members; a flood fill from every unlabelled member in ascending
// flat order numbers the clusters by their smallest index; the kept ones are renumbered in that order; one pass over the
// voxels gives the records and a second one rep, once the sums are final.
void BGKOctoMap::clusters(const float *lo3, const uint32_t *dims3, const la3dm_clusters_params &p, const la3dm_clusters_out *out,
                          uint32_t *n_found, la3dm_clusters_stats *stats, la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_clusters_host(dmap, lo3, dims3, &p, out, n_found, stats, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::clusters: ") + la3dm_last_error(ctx));
        return;
    }
    std::string refusal = la3dm_region::clusters_check(&p, out);
    if (!refusal.empty()) throw std::invalid_argument("BGKOctoMap::clusters: " + refusal);
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::kClusters, true, "clusters", g0, inf);
    refusal = la3dm_region::clusters_region_check(dims3);
    if (!refusal.empty()) throw std::invalid_argument("BGKOctoMap::clusters: " + refusal);
    if (info) *info = inf;
    la3dm_clusters_out o;
    std::memset(&o, 0, sizeof(o));
    if (out) o = *out;
    const uint32_t nx = dims3[0], ny = dims3[1], nz = dims3[2];
    const size_t n = (size_t)nx * ny * nz;
    const std::vector<uint8_t> cls = region_classes(*this, lo3, dims3);
    const uint32_t n_list = p.from_list ? p.n_members : 0;
    std::vector<uint8_t> member(n, 0);
    if (p.from_list) {
        for (uint32_t t = 0; t < n_list; ++t)
            if (p.members[t] < n && ((p.member_mask >> cls[p.members[t]]) & 1u)) member[p.members[t]] = 1;
    } else {
        for (size_t f = 0; f < n; ++f) member[f] = (p.member_mask >> cls[f]) & 1u;
    }
    const std::vector<Move> moves = connectivity_moves(p.connectivity);
    const uint32_t tile = p.tile ? p.tile : 0xFFFFFFFFu;   // (untiled: every voxel in tile 0)
    // the flood fill: comp[f] = the cluster's number among ALL clusters, in ascending order of their smallest index
    std::vector<uint32_t> comp(n, LA3DM_CLUSTERS_NONE), sizes, stack;
    la3dm_clusters_stats s;
    std::memset(&s, 0, sizeof(s));
    for (size_t f0 = 0; f0 < n; ++f0) {
        if (!member[f0] || comp[f0] != LA3DM_CLUSTERS_NONE) continue;
        const uint32_t c = (uint32_t)sizes.size();
        uint32_t count = 0;
        comp[f0] = c;
        stack.push_back((uint32_t)f0);
        while (!stack.empty()) {
            const uint32_t f = stack.back();
            stack.pop_back();
            ++count;
            const uint32_t k = f % nz, j = (f / nz) % ny, i = f / (nz * ny);
            for (const Move &mv : moves) {
                const uint32_t ui = i + (uint32_t)mv.d[0], uj = j + (uint32_t)mv.d[1], uk = k + (uint32_t)mv.d[2];   // (0 - 1 wraps above nx)
                if (ui >= nx || uj >= ny || uk >= nz || ui / tile != i / tile || uj / tile != j / tile || uk / tile != k / tile) continue;
                const size_t u = ((size_t)ui * ny + uj) * nz + uk;
                if (!member[u] || comp[u] != LA3DM_CLUSTERS_NONE) continue;
                comp[u] = c;
                stack.push_back((uint32_t)u);
            }
        }
        sizes.push_back(count);
        s.n_members += count;
    }
    std::vector<uint32_t> number(sizes.size());
    for (size_t c = 0; c < sizes.size(); ++c) {
        const bool keep = sizes[c] >= p.min_size;
        number[c] = keep ? s.n_clusters++ : LA3DM_CLUSTERS_NONE;
        if (keep)
            s.largest = std::max(s.largest, sizes[c]);
        else
            ++s.n_dropped;
    }
    const uint32_t m = std::min(s.n_clusters, p.cap);
    std::vector<uint64_t> sum(3 * (size_t)m, 0), key(m, ~0ull);
    std::vector<uint32_t> size_of(m, 0);
    for (uint32_t c = 0; c < m; ++c)
        for (int a = 0; a < 3; ++a) {
            if (o.lo) o.lo[3 * c + a] = 0xFFFFFFFFu;
            if (o.hi) o.hi[3 * c + a] = 0;
        }
    for (size_t f = 0; f < n; ++f) {
        const uint32_t c = comp[f] == LA3DM_CLUSTERS_NONE ? LA3DM_CLUSTERS_NONE : number[comp[f]];
        if (o.label) o.label[f] = c;
        if (c >= m) continue;   // (NONE is no record)
        const uint32_t v[3] = {(uint32_t)(f / ((size_t)nz * ny)), (uint32_t)((f / nz) % ny), (uint32_t)(f % nz)};
        if (size_of[c]++ == 0 && o.first) o.first[c] = (uint32_t)f;   // ascending f: the first member seen is the smallest index
        for (int a = 0; a < 3; ++a) {
            sum[3 * c + a] += v[a];
            if (o.lo) o.lo[3 * c + a] = std::min(o.lo[3 * c + a], v[a]);
            if (o.hi) o.hi[3 * c + a] = std::max(o.hi[3 * c + a], v[a]);
        }
    }
    if (o.rep)
        for (size_t f = 0; f < n; ++f) {   // ascending f and a strict comparison: ties go to the smallest index
            const uint32_t c = comp[f] == LA3DM_CLUSTERS_NONE ? LA3DM_CLUSTERS_NONE : number[comp[f]];
            if (c >= m) continue;
            const int64_t v[3] = {(int64_t)(f / ((size_t)nz * ny)), (int64_t)((f / nz) % ny), (int64_t)(f % nz)};
            uint64_t d = 0;
            for (int a = 0; a < 3; ++a) {
                const int64_t ca = (int64_t)((2 * sum[3 * c + a] + size_of[c]) / (2ull * size_of[c]));
                d += (uint64_t)((v[a] - ca) * (v[a] - ca));
            }
            const uint64_t cand = (d << 32) | (uint64_t)f;
            if (cand < key[c]) key[c] = cand;
        }
    for (uint32_t c = 0; c < m; ++c) {
        if (o.size) o.size[c] = size_of[c];
        if (o.rep) o.rep[c] = (uint32_t)key[c];
        if (o.sum)
            for (int a = 0; a < 3; ++a) o.sum[3 * c + a] = sum[3 * c + a];
    }
    for (uint32_t t = 0; t < n_list && o.of_member; ++t) {
        const uint32_t f = p.members[t];
        o.of_member[t] = f < n && comp[f] != LA3DM_CLUSTERS_NONE ? number[comp[f]] : LA3DM_CLUSTERS_NONE;
    }
    if (n_found) *n_found = s.n_clusters;
    if (stats) *stats = s;
}

// ---- gain of candidate viewpoints.  The host form below is the definition; the device kernels (csrc/devmap_gain.h)
// reproduce it bit for bit.  Per segment the loop is raycast_many's, row for row; what is added is the mark: the row's
// lattice position (block-key fields * lim + the cell of its node key) against the region, and one bit per voxel and
// viewpoint.
void BGKOctoMap::gain(const float *lo3, const uint32_t *dims3, const float *origins3, uint32_t n, const float *offsets3, uint32_t m,
                      uint32_t count_mask, uint32_t stop_mask, uint32_t max_steps, const la3dm_gain_out &out,
                      la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_gain_host(dmap, lo3, dims3, origins3, n, offsets3, m, count_mask, stop_mask, max_steps, &out, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::gain: ") + la3dm_last_error(ctx));
        return;
    }
    const std::string w = "BGKOctoMap::gain";
    std::string refusal = la3dm_region::gain_check(count_mask, stop_mask, max_steps, n, m);
    if (!refusal.empty()) throw std::invalid_argument(w + ": " + refusal);
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::kGain, true, "gain", g0, inf);
    const uint64_t total = (uint64_t)dims3[0] * dims3[1] * dims3[2];
    refusal = la3dm_region::gain_buffers(total, n, origins3 != nullptr, offsets3 != nullptr, true, out.gain != nullptr, ".");
    if (!refusal.empty()) throw std::invalid_argument(w + ": " + refusal);
    if (info) *info = inf;
    if (n == 0) return;
    const size_t W = la3dm_region::gain_words(total);
    std::vector<uint32_t> own_sets;
    uint32_t *sets = out.seen;
    if (sets == nullptr) {
        own_sets.resize((size_t)n * W);
        sets = own_sets.data();
    }
    std::fill(sets, sets + (size_t)n * W, 0u);
    const unsigned dl = block_depth - 1u;
    const uint32_t lim = 1u << dl, nx = dims3[0], ny = dims3[1], nz = dims3[2];
    for (uint32_t v = 0; v < n; ++v) {
        uint32_t *set = sets + (size_t)v * W;
        uint32_t started = 0, hits = 0;
        const float *o = origins3 + 3 * (size_t)v;
        for (uint32_t d = 0; d < m; ++d) {
            const float *off = offsets3 + 3 * (size_t)d;
            const float q[6] = {o[0], o[1], o[2], o[0] + off[0], o[1] + off[1], o[2] + off[2]};
            bool ok = true;  // raycast_many's validity test
            for (int a = 0; a < 6; ++a) ok &= std::fabs(q[a] / resolution) < 1073741824.0f;   // false for NaN and inf
            if (!ok) continue;
            uint32_t steps = 0;
            RayCaster rc(this, point3f(q[0], q[1], q[2]), point3f(q[3], q[4], q[5]));
            while (!rc.end()) {
                if (steps == max_steps) break;   // truncated
                point3f p;
                OcTreeNode nd;
                BlockHashKey bk = 0;
                OcTreeHashKey nk = 0;
                const bool valid = rc.next(p, nd, bk, nk);
                ++steps;
                uint32_t cls = LA3DM_RAY_MISSING;
                if (valid) {   // the covering leaf, as raycast_many finds it
                    const Block *b = block_arr.find(bk)->second;
                    unsigned ld = dl, i = (unsigned)(nk & 0xFFFF);
                    while (ld > 0 && b->slab[layer_base(ld) + i].state == State::PRUNED) {
                        --ld;
                        i >>= 3;
                    }
                    cls = (uint32_t)b->slab[layer_base(ld) + i].state;
                }
                if ((count_mask >> cls) & 1u) {
                    // the cell of the node key: its digits base 8 (bit 4 = x, 2 = y, 1 = z), the coarsest level first
                    uint32_t c[3] = {0, 0, 0};
                    for (unsigned level = 0; level < dl; ++level) {
                        const uint32_t digit = ((uint32_t)nk >> (3 * level)) & 7u;
                        c[0] |= ((digit >> 2) & 1u) << level;
                        c[1] |= ((digit >> 1) & 1u) << level;
                        c[2] |= (digit & 1u) << level;
                    }
                    // (wrapping: a position below g0 becomes a huge index and fails the compare)
                    const uint32_t i = ((uint32_t)(bk >> 40) & 0xFFFFFu) * lim + c[0] - g0[0];
                    const uint32_t j = ((uint32_t)(bk >> 20) & 0xFFFFFu) * lim + c[1] - g0[1];
                    const uint32_t k = ((uint32_t)bk & 0xFFFFFu) * lim + c[2] - g0[2];
                    if (i < nx && j < ny && k < nz) {
                        const uint32_t f = (i * ny + j) * nz + k;
                        set[f >> 5] |= 1u << (f & 31u);
                    }
                }
                if (stop_mask & (1u << cls)) {
                    ++hits;
                    break;
                }
            }
            started += steps > 0 ? 1u : 0u;
        }
        uint32_t gain = 0;
        for (size_t t = 0; t < W; ++t) gain += (uint32_t)__builtin_popcount(set[t]);
        out.gain[v] = gain;
        if (out.started) out.started[v] = started;
        if (out.hits) out.hits[v] = hits;
    }
}

// ---- score_poses.  The host form below is the definition; the device kernels (csrc/devmap_score.h) compile the same
// transform and point-to-voxel inlines (region_contract.h) and reproduce it exactly: everything after them is integers.
void BGKOctoMap::score_poses(const float *lo3, const uint32_t *dims3, const float *points3, uint32_t n_points, const float *poses12,
                             uint32_t n_poses, uint32_t obstacle_mask, uint32_t radius, const la3dm_score_out &out,
                             la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_score_poses_host(dmap, lo3, dims3, points3, n_points, poses12, n_poses, obstacle_mask, radius, &out, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::score_poses: ") + la3dm_last_error(ctx));
        return;
    }
    const std::string w = "BGKOctoMap::score_poses";
    std::string refusal = la3dm_region::score_check(obstacle_mask, radius, n_points, n_poses);
    if (!refusal.empty()) throw std::invalid_argument(w + ": " + refusal);
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::kScore, true, "score_poses", g0, inf);
    refusal = la3dm_region::score_buffers(n_points, n_poses, points3 != nullptr, poses12 != nullptr, true, out.sum_d2 != nullptr, ".");
    if (!refusal.empty()) throw std::invalid_argument(w + ": " + refusal);
    if (info) *info = inf;
    if (n_poses == 0) return;
    std::vector<uint32_t> d2;
    if (n_points > 0) d2 = region_d2(*this, lo3, dims3, obstacle_mask, radius);
    const int lim = 1 << (block_depth - 1);
#pragma omp parallel for schedule(static)
    for (uint32_t p = 0; p < n_poses; ++p) {
        uint32_t c[5] = {0, 0, 0, 0, 0};
        uint64_t sum = 0;
        for (uint32_t i = 0; i < n_points; ++i) {
            const float *q = points3 + 3 * (size_t)i;
            uint32_t f = 0;
            uint32_t cls = la3dm_region::score_voxel(poses12 + 12 * (size_t)p, q[0], q[1], q[2], resolution, block_size, lim, g0, dims3, f);
            if (cls == LA3DM_SCORE_HIT) {
                cls = la3dm_region::score_class(d2[f]);
                if (cls != LA3DM_SCORE_FAR) sum += d2[f];
            }
            ++c[cls];
        }
        out.sum_d2[p] = sum;
        if (out.counts)
            for (int k = 0; k < 5; ++k) out.counts[5 * (size_t)p + k] = c[k];
    }
}

// ---- score_paths.  The host form below is the definition; the device kernel (csrc/devmap_paths.h) compiles the same
// waypoint, walk, move and entry inlines (region_contract.h) and reproduces it exactly: everything after the waypoint
// voxels is integers.
void BGKOctoMap::score_paths(const float *lo3, const uint32_t *dims3, const float *ways3, uint32_t n_paths, uint32_t n_way,
                             const la3dm_paths_params *params, const la3dm_paths_out &out, la3dm_region_info *info) const {
    bind();
    if (dmap != nullptr) {
        if (la3dm_devmap_score_paths_host(dmap, lo3, dims3, ways3, n_paths, n_way, params, &out, info) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::score_paths: ") + la3dm_last_error(ctx));
        return;
    }
    const std::string w = "BGKOctoMap::score_paths";
    const std::string refusal = la3dm_region::paths_check(params, n_paths, n_way, ways3 != nullptr, true, out.cost != nullptr, ".");
    if (!refusal.empty()) throw std::invalid_argument(w + ": " + refusal);
    uint32_t g0[3];
    la3dm_region_info inf;
    region_anchor(lo3, dims3, la3dm_region::kPaths, true, "score_paths", g0, inf);
    if (info) *info = inf;
    if (n_paths == 0) return;
    const la3dm_paths_params &p = *params;
    const std::vector<uint32_t> d2 = region_d2(*this, lo3, dims3, p.obstacle_mask, la3dm_region::paths_radius(p));
    const int lim = 1 << (block_depth - 1);
#pragma omp parallel for schedule(dynamic, 16)
    for (uint32_t path = 0; path < n_paths; ++path) {
        const float *W = ways3 + 3 * (size_t)path * n_way;
        std::vector<long long> G(3 * (size_t)n_way);
        bool valid = true;
        for (uint32_t k = 0; k < n_way; ++k) valid = la3dm_region::path_waypoint(W + 3 * k, resolution, block_size, lim, &G[3 * k]) && valid;
        uint64_t cost = 0, o = 0;   // o: the ordinal of the voxel at hand
        uint32_t L = 0, stop = LA3DM_PATH_NONE, min_d2 = LA3DM_DF_FAR, ways = 0, flags = valid ? 0u : LA3DM_PATH_INVALID;
        // the voxel v of ordinal o, entered by a move with nz components (0: the first): true where the walk stops
        auto visit = [&](const long long *v, uint32_t nz) {
            uint32_t f = 0;
            if (!la3dm_region::path_inside(v, g0, dims3, f)) {
                flags |= LA3DM_PATH_LEFT;
            } else if (la3dm_region::path_blocked(p.clearance, d2[f])) {
                flags |= LA3DM_PATH_BLOCKED;
            } else {
                if (nz > 0) cost += la3dm_region::path_entry(p, nz, d2[f]);
                min_d2 = std::min(min_d2, d2[f]);
                ++L;
                return false;
            }
            stop = (uint32_t)o;
            return true;
        };
        if (valid) {
            bool stopped = visit(&G[0], 0);
            if (!stopped) ways = 1;
            long long last[3] = {G[0], G[1], G[2]};
            for (uint32_t k = 1; k < n_way && !stopped && !(flags & LA3DM_PATH_TRUNCATED); ++k) {
                const long long *A = &G[3 * (k - 1)], *B = &G[3 * k];
                const long long n = la3dm_region::path_segment(A, B);
                for (long long s = 1; s <= n && !stopped; ++s) {
                    if (o == p.max_steps) {   // T > max_steps, and no stop in [0, E]
                        flags |= LA3DM_PATH_TRUNCATED;
                        break;
                    }
                    ++o;
                    long long v[3];
                    for (int c = 0; c < 3; ++c) v[c] = la3dm_region::path_sample(A[c], B[c] - A[c], n, s);
                    stopped = visit(v, la3dm_region::path_move(last, v));
                    for (int c = 0; c < 3; ++c) last[c] = v[c];
                }
                if (!stopped && !(flags & LA3DM_PATH_TRUNCATED)) ++ways;   // off[k] < L: waypoint k is reached
            }
        }
        out.cost[path] = cost;
        if (out.steps) out.steps[path] = L;
        if (out.stop) out.stop[path] = stop;
        if (out.min_d2) out.min_d2[path] = min_d2;
        if (out.ways) out.ways[path] = ways;
        if (out.flags) out.flags[path] = (uint8_t)flags;
    }
}

namespace {
// heightMapColor, include/common/markerarray_pub.h:21-76 (s = v = 1)
void height_map_color(double h, float *rgba) {
    h -= floor(h);
    h *= 6;
    const int i = (int)floor(h);
    double f = h - i;
    if (!(i & 1)) f = 1 - f;
    const double v = 1.0, m = 0.0, n = 1.0 - f;
    double r, g, b;
    switch (i) {
    case 6:
    case 0: r = v; g = n; b = m; break;
    case 1: r = n; g = v; b = m; break;
    case 2: r = m; g = v; b = n; break;
    case 3: r = m; g = n; b = v; break;
    case 4: r = n; g = m; b = v; break;
    case 5: r = v; g = m; b = n; break;
    default: r = 1; g = 0.5; b = 0.5; break;
    }
    rgba[0] = (float)r;
    rgba[1] = (float)g;
    rgba[2] = (float)b;
    rgba[3] = 1.0f;
}
}  // namespace

size_t BGKOctoMap::export_cells(State state, bool original_size, float min_z, float max_z, Cells &out) const {
    bind();
    if (state != State::OCCUPIED && state != State::FREE)
        throw std::runtime_error("BGKOctoMap::export_cells: state must be OCCUPIED or FREE");
    out.xyz_size.clear();
    out.rgba.clear();
    out.level.clear();
    if (min_z == max_z) {  // bgkoctomap_static_node.cpp:103-108
        point3f lo, hi;
        get_bbox(lo, hi);
        min_z = lo.z();
        max_z = hi.z();
    }
    if (dmap != nullptr) {
        uint64_t n = 0;
        if (la3dm_devmap_export_cells(dmap, (int)state, original_size ? 1 : 0, min_z, max_z, nullptr, nullptr, nullptr, 0, &n) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::export_cells: ") + la3dm_last_error(ctx));
        out.xyz_size.resize(4 * n);
        out.rgba.resize(4 * n);
        out.level.resize(n);
        if (n && la3dm_devmap_export_cells(dmap, (int)state, original_size ? 1 : 0, min_z, max_z, out.xyz_size.data(), out.rgba.data(),
                                           out.level.data(), n, &n) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::export_cells: ") + la3dm_last_error(ctx));
        return (size_t)n;
    }
    auto push = [&](float x, float y, float z, float size, const OcTreeNode &nd) {
        out.xyz_size.insert(out.xyz_size.end(), {x, y, z, size});
        out.level.push_back(size > 0 ? (int)log2(size / resolution) : 0);  // markerarray_pub.h:110-114
        float c[4] = {0.0f, 0.0f, 1.0f, 1.0f};                             // the marker's default colour
        if (state == State::OCCUPIED) {
            if (min_z < max_z) {
                const double h = (1.0 - std::min(std::max((z - min_z) / (max_z - min_z), 0.0f), 1.0f)) * 0.8;
                height_map_color(h, c);
            }
        } else {
            const float prob = nd.get_prob();
            if (prob < 0.5f) {
                c[0] = c[1] = c[2] = 0.8f;
            } else {
                height_map_color(std::min(2.0 - 2.0 * prob, 0.6), c);
            }
        }
        out.rgba.insert(out.rgba.end(), c, c + 4);
    };
    for (auto it = begin_leaf(); it != end_leaf(); ++it) {
        if (it.get_node().get_state() != state) continue;
        if (original_size) {
            const point3f p = it.get_loc();
            push(p.x(), p.y(), p.z(), it.get_size(), it.get_node());
        } else {
            for (const point3f &p : it.get_pruned_locs()) push(p.x(), p.y(), p.z(), resolution, it.get_node());
        }
    }
    return out.level.size();
}

void BGKOctoMap::get_bbox(point3f &lim_min, point3f &lim_max) const {
    bind();
    if (dmap != nullptr) {  // index box of the pool's keys; centre = (index - 524288) * size is monotone in the index
        lim_min = point3f(0, 0, 0);
        lim_max = point3f(0, 0, 0);
        uint32_t nb = 0, npb = 0;
        if (la3dm_devmap_block_count(dmap, &nb, &npb) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::get_bbox: ") + la3dm_last_error(ctx));
        if (nb == 0) return;
        int32_t lo[3], hi[3];
        if (la3dm_devmap_key_bounds(dmap, lo, hi) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::get_bbox: ") + la3dm_last_error(ctx));
        const BlockHashKey klo = ((int64_t)lo[0] << 40) | ((int64_t)lo[1] << 20) | (int64_t)lo[2];
        const BlockHashKey khi = ((int64_t)hi[0] << 40) | ((int64_t)hi[1] << 20) | (int64_t)hi[2];
        lim_min = hash_key_to_block(klo);
        lim_max = hash_key_to_block(khi);
        lim_min -= point3f(block_size, block_size, block_size) * 0.5;
        lim_max += point3f(block_size, block_size, block_size) * 0.5;
        return;
    }
    sync_mirror();
    lim_min = point3f(0, 0, 0);
    lim_max = point3f(0, 0, 0);
    bool first = true;
    for (auto &kv : block_arr) {
        const point3f c = kv.second->get_center();
        if (first) {
            lim_min = lim_max = c;
            first = false;
            continue;
        }
        for (unsigned a = 0; a < 3; ++a) {
            lim_min(a) = std::min(lim_min(a), c(a));
            lim_max(a) = std::max(lim_max(a), c(a));
        }
    }
    if (!first) {
        lim_min -= point3f(block_size, block_size, block_size) * 0.5;
        lim_max += point3f(block_size, block_size, block_size) * 0.5;
    }
}

BGKOctoMap::LeafIterator::LeafIterator(const BGKOctoMap *map)
    : block_it(map->block_arr.cbegin()), end_block(map->block_arr.cend()) {
    // skip nothing: every block has at least one leaf
    if (block_it != end_block) {
        leaf_it = block_it->second->begin_leaf();
        end_leaf = block_it->second->end_leaf();
    }
}

BGKOctoMap::LeafIterator &BGKOctoMap::LeafIterator::operator++() {
    ++leaf_it;
    if (leaf_it == end_leaf) {
        ++block_it;
        if (block_it != end_block) {
            leaf_it = block_it->second->begin_leaf();
            end_leaf = block_it->second->end_leaf();
        }
    }
    return *this;
}

std::vector<point3f> BGKOctoMap::LeafIterator::get_pruned_locs() const {
    // base-resolution voxel centres covered by a (possibly collapsed) leaf
    std::vector<point3f> out;
    const point3f c = get_loc();
    const float size = get_size();
    const float x0 = c.x() - size * 0.5 + Block::resolution * 0.5;
    const float y0 = c.y() - size * 0.5 + Block::resolution * 0.5;
    const float z0 = c.z() - size * 0.5 + Block::resolution * 0.5;
    const float x1 = c.x() + size * 0.5, y1 = c.y() + size * 0.5, z1 = c.z() + size * 0.5;
    for (float x = x0; x < x1; x += Block::resolution)
        for (float y = y0; y < y1; y += Block::resolution)
            for (float z = z0; z < z1; z += Block::resolution) out.emplace_back(x, y, z);
    return out;
}

// ---------------------------------------------------------------- front end (stage A)
namespace {

// Voxel-grid centroid filter with the semantics of pcl::VoxelGrid<PointXYZ> (PCL is not a
// dependency of this build): cell = floor(p * (1/leaf)) - floor(min * (1/leaf)), output cells in
// ascending linear index, centroid = fp32 sum in cloud order / (float)count.
bool grid_order_option(la3dm_ctx *ctx) {
    int v = 0;
    return ctx && la3dm_get_option(ctx, "grid_order", &v) == 0 && v == 1;
}

void voxel_grid_filter(const float *in, size_t n, float leaf, std::vector<float> &out, bool pcl_order = false) {
    out.clear();
    if (n == 0) return;
    const float inv = 1.0f / leaf;
    float mn[3] = {std::numeric_limits<float>::max(), std::numeric_limits<float>::max(), std::numeric_limits<float>::max()};
    float mx[3] = {-mn[0], -mn[1], -mn[2]};
    for (size_t i = 0; i < n; ++i) {
        const float *p = in + 3 * i;
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
        for (int a = 0; a < 3; ++a) {
            mn[a] = std::min(mn[a], p[a]);
            mx[a] = std::max(mx[a], p[a]);
        }
    }
    const int64_t ex = (int64_t)((mx[0] - mn[0]) * inv) + 1, ey = (int64_t)((mx[1] - mn[1]) * inv) + 1,
                  ez = (int64_t)((mx[2] - mn[2]) * inv) + 1;
    if (ex * ey * ez > (int64_t)std::numeric_limits<int32_t>::max()) {  // PCL gives the input back
        out.assign(in, in + 3 * n);
        return;
    }
    int lo[3], span[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = (int)std::floor(mn[a] * inv);
        span[a] = (int)std::floor(mx[a] * inv) - lo[a] + 1;
    }
    const int m1 = span[0], m2 = span[0] * span[1];
    const size_t ncell = (size_t)span[0] * span[1] * span[2];
    if (pcl_order) {
        // option "grid_order" 1 (verification mode, include/la3dm_hip.h): the order of the points inside a cell as pcl::VoxelGrid's own
        // std::sort leaves it — {cell, cloud index} pairs compared on the cell alone (src/bgkoctomap/bgkoctomap.cpp:419-431)
        std::vector<std::pair<unsigned, unsigned>> iv;
        iv.reserve(n);
        for (size_t i = 0; i < n; ++i) {
            const float *p = in + 3 * i;
            if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
            const int c0 = (int)(std::floor(p[0] * inv) - (float)lo[0]);
            const int c1 = (int)(std::floor(p[1] * inv) - (float)lo[1]);
            const int c2 = (int)(std::floor(p[2] * inv) - (float)lo[2]);
            iv.emplace_back((unsigned)(c0 + c1 * m1 + c2 * m2), (unsigned)i);
        }
        struct PclLess {
            bool operator()(const std::pair<unsigned, unsigned> &a, const std::pair<unsigned, unsigned> &b) const { return a.first < b.first; }
        };
        std::sort(iv.begin(), iv.end(), PclLess());
        for (size_t i = 0; i < iv.size();) {
            size_t j = i;
            float sx = 0.f, sy = 0.f, sz = 0.f;
            for (; j < iv.size() && iv[j].first == iv[i].first; ++j) {
                const float *p = in + 3 * (size_t)iv[j].second;
                sx += p[0];
                sy += p[1];
                sz += p[2];
            }
            const float cnt = (float)(j - i);
            out.push_back(sx / cnt);
            out.push_back(sy / cnt);
            out.push_back(sz / cnt);
            i = j;
        }
        return;
    }
    if (ncell <= ((size_t)1 << 24)) {
        // dense accumulation: one pass in cloud order (the same per-cell summation order as sorting by
        // (cell, index)), then the occupied cells in ascending index
        struct Acc {
            float x, y, z;
            uint32_t n;
        };
        // zero pages on demand (calloc): only the touched part of the grid is ever paged in
        Acc *acc = static_cast<Acc *>(std::calloc(ncell, sizeof(Acc)));
        if (acc == nullptr) throw std::bad_alloc();
        // pass 1 (streaming, parallel): cell of every point.  pass 2: every thread of a small team owns a contiguous
        // range of cells and walks the whole cell list in cloud order, accumulating only its own cells — each cell
        // still sums its points in cloud order (one owner), and the owners' touched lists, each sorted, concatenate
        // to the ascending cell order.  The accumulation target is prefetched a few points ahead (the cloud arrives in
        // ray order: every access is a cache miss).
        std::vector<uint32_t> cells(n);
        const int team = n > 200000 ? kHostThreads : 1;
#pragma omp parallel for num_threads(team) schedule(static)
        for (long ii = 0; ii < (long)n; ++ii) {
            const size_t i = (size_t)ii;
            const float *p = in + 3 * i;
            if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) {
                cells[i] = 0xFFFFFFFFu;
                continue;
            }
            const int c0 = (int)(std::floor(p[0] * inv) - (float)lo[0]);
            const int c1 = (int)(std::floor(p[1] * inv) - (float)lo[1]);
            const int c2 = (int)(std::floor(p[2] * inv) - (float)lo[2]);
            cells[i] = (uint32_t)(c0 + c1 * m1 + c2 * m2);
        }
        std::vector<std::vector<uint32_t>> touched(team);
        std::vector<size_t> first(team + 1, 0);
#pragma omp parallel num_threads(team)
        {
            const int t = omp_get_thread_num(), nt = omp_get_num_threads();  // the runtime may grant fewer threads
            const uint32_t c_lo = (uint32_t)((uint64_t)ncell * t / nt), c_hi = (uint32_t)((uint64_t)ncell * (t + 1) / nt);
            std::vector<uint32_t> &mine = touched[t];
            constexpr size_t kAhead = 24;
            for (size_t i = 0; i < n; ++i) {
                if (i + kAhead < n) {
                    const uint32_t ca = cells[i + kAhead];
                    if (ca >= c_lo && ca < c_hi) __builtin_prefetch(&acc[ca], 1, 1);
                }
                const uint32_t cell = cells[i];
                if (cell < c_lo || cell >= c_hi) continue;  // (0xFFFFFFFF = non-finite point: owned by nobody)
                const float *p = in + 3 * i;
                Acc &a = acc[cell];
                if (a.n == 0) mine.push_back(cell);
                a.x += p[0];
                a.y += p[1];
                a.z += p[2];
                ++a.n;
            }
            std::sort(mine.begin(), mine.end());
        }
        for (int t = 0; t < team; ++t) first[t + 1] = first[t] + touched[t].size();
        out.resize(3 * first[team]);
#pragma omp parallel for num_threads(team) schedule(static)
        for (int t = 0; t < team; ++t) {
            size_t o = 3 * first[t];
            for (uint32_t cell : touched[t]) {
                const Acc &a = acc[cell];
                const float cnt = (float)a.n;
                out[o++] = a.x / cnt;
                out[o++] = a.y / cnt;
                out[o++] = a.z / cnt;
            }
        }
        std::free(acc);
        return;
    }
    std::vector<uint64_t> order;
    order.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        const float *p = in + 3 * i;
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
        const int c0 = (int)(std::floor(p[0] * inv) - (float)lo[0]);
        const int c1 = (int)(std::floor(p[1] * inv) - (float)lo[1]);
        const int c2 = (int)(std::floor(p[2] * inv) - (float)lo[2]);
        const uint32_t cell = (uint32_t)(c0 + c1 * m1 + c2 * m2);
        order.push_back(((uint64_t)cell << 32) | (uint32_t)i);
    }
    std::sort(order.begin(), order.end());
    size_t i = 0;
    while (i < order.size()) {
        const uint32_t cell = (uint32_t)(order[i] >> 32);
        float sx = 0.f, sy = 0.f, sz = 0.f;
        size_t j = i;
        for (; j < order.size() && (uint32_t)(order[j] >> 32) == cell; ++j) {
            const float *p = in + 3 * (uint32_t)order[j];
            sx += p[0];
            sy += p[1];
            sz += p[2];
        }
        const float cnt = (float)(j - i);
        out.push_back(sx / cnt);
        out.push_back(sy / cnt);
        out.push_back(sz / cnt);
        i = j;
    }
}

}  // namespace

void BGKOctoMap::get_training_data(const float *xyz, size_t n, size_t stride, const point3f &origin, float ds_resolution,
                                   float free_resolution, float max_range) {
    std::vector<float> packed(3 * n);
    for (size_t i = 0; i < n; ++i) {
        packed[3 * i] = xyz[stride * i];
        packed[3 * i + 1] = xyz[stride * i + 1];
        packed[3 * i + 2] = xyz[stride * i + 2];
    }
    std::vector<float> hits;
    const double tt0 = wall();
    const bool pcl_order = grid_order_option(ctx);
    if (ds_resolution < 0) hits.swap(packed); else voxel_grid_filter(packed.data(), n, ds_resolution, hits, pcl_order);
    const double tt1 = wall();

    xy.clear();
    std::vector<float> frees;
    const float x0 = origin.x(), y0 = origin.y(), z0 = origin.z();
    const size_t nh = hits.size() / 3;
    xy.reserve(4 * nh);
    frees.reserve(3 * nh * 8);
    size_t kept = 0;
    for (size_t i = 0; i < nh; ++i) {
        const float x = hits[3 * i], y = hits[3 * i + 1], z = hits[3 * i + 2];
        if (max_range > 0) {
            const double l = (point3f(x, y, z) - origin).norm();
            if (l > max_range) continue;
        }
        xy.push_back(x);
        xy.push_back(y);
        xy.push_back(z);
        xy.push_back(1.0f);
        ++kept;
        // free-space samples along the beam: the origin itself, then every free_resolution,
        // then one sample free_resolution short of the hit
        const float l = (float)sqrt((x - x0) * (x - x0) + (y - y0) * (y - y0) + (z - z0) * (z - z0));
        const float nx = (x - x0) / l, ny = (y - y0) / l, nz = (z - z0) / l;
        size_t w = frees.size();
        const size_t room = 3 * ((l < 1.0e9f ? (size_t)(l / free_resolution) : 0) + 4);  // (false for a NaN range too)
        frees.resize(w + room);
        float *f = frees.data();
        f[w++] = x0;
        f[w++] = y0;
        f[w++] = z0;
        for (float d = free_resolution; d < l; d += free_resolution) {
            if (w + 6 > frees.size()) {  // (float stepping can take one more step than l / free_resolution)
                frees.resize(frees.size() + 64);
                f = frees.data();
            }
            f[w++] = x0 + nx * d;
            f[w++] = y0 + ny * d;
            f[w++] = z0 + nz * d;
        }
        if (l > free_resolution) {
            const float d = l - free_resolution;
            f[w++] = x0 + nx * d;
            f[w++] = y0 + ny * d;
            f[w++] = z0 + nz * d;
        }
        frees.resize(w);
    }
    std::vector<float> sampled;
    const double tt2 = wall();
    if (ds_resolution < 0) sampled.swap(frees); else voxel_grid_filter(frees.data(), frees.size() / 3, ds_resolution, sampled, pcl_order);
    if (getenv("LA3DM_TIMING"))
        fprintf(stderr, "[la3dm] front end: grid(hits) %.4f beam %.4f grid(frees, %zu pts) %.4f\n", tt1 - tt0, tt2 - tt1,
                frees.size() / 3, wall() - tt2);
    const size_t nf = sampled.size() / 3;
    xy.reserve(xy.size() + 4 * nf);
    const float free_label = variant == 1 ? -1.0f : 0.0f;  // bgkoctomap.cpp:415 / gpoctomap.cpp:399
    for (size_t i = 0; i < nf; ++i) xy.insert(xy.end(), {sampled[3 * i], sampled[3 * i + 1], sampled[3 * i + 2], free_label});
    stats.n_hits = kept;
    stats.n_frees = nf;
}

// BGKLOctoMap front end (src/bgkloctomap/bgkloctomap.cpp:300-343, beam_sample :359-381): hits are re-projected as
// origin + n * l, free samples step down from l - free_resolution while d > 0 and are not voxel-filtered, every sample
// of a beam (the origin sample first) remembers its beam; the beam itself is origin -> origin + n * (l - free_resolution).
void BGKOctoMap::get_training_data_l(const float *xyz, size_t n, size_t stride, const point3f &origin, float ds_resolution,
                                     float free_resolution, float max_range) {
    std::vector<float> packed(3 * n);
    for (size_t i = 0; i < n; ++i) {
        packed[3 * i] = xyz[stride * i];
        packed[3 * i + 1] = xyz[stride * i + 1];
        packed[3 * i + 2] = xyz[stride * i + 2];
    }
    std::vector<float> hits;
    if (ds_resolution < 0) hits.swap(packed); else voxel_grid_filter(packed.data(), n, ds_resolution, hits, grid_order_option(ctx));
    const float x0 = origin.x(), y0 = origin.y(), z0 = origin.z();
    const size_t nh = hits.size() / 3;
    // pass 1: range gate and sample count per hit (the float-stepped while loop, kept verbatim); pass 2: fill
    std::vector<uint32_t> first(nh + 1, 0u);  // first xy entry of hit i; kept hits only contribute
    std::vector<uint8_t> kept(nh, 0);
    auto end_point = [&](size_t i, float &ex, float &ey, float &ez, float &nx, float &ny, float &nz, float &l) {
        const float x = hits[3 * i], y = hits[3 * i + 1], z = hits[3 * i + 2];
        l = (float)sqrt((x - x0) * (x - x0) + (y - y0) * (y - y0) + (z - z0) * (z - z0));
        nx = (x - x0) / l;
        ny = (y - y0) / l;
        nz = (z - z0) / l;
        ex = x0 + nx * l;
        ey = y0 + ny * l;
        ez = z0 + nz * l;
    };
#pragma omp parallel for num_threads(kHostThreads) schedule(static)
    for (long i = 0; i < (long)nh; ++i) {
        const float x = hits[3 * i], y = hits[3 * i + 1], z = hits[3 * i + 2];
        if (max_range > 0) {
            const double lr = (point3f(x, y, z) - origin).norm();
            if (lr > max_range) continue;
        }
        kept[i] = 1;
        float ex, ey, ez, nx, ny, nz, l;
        end_point((size_t)i, ex, ey, ez, nx, ny, nz, l);
        const float l2 = (float)sqrt((ex - x0) * (ex - x0) + (ey - y0) * (ey - y0) + (ez - z0) * (ez - z0));
        uint32_t c = 2;  // the re-projected hit and the origin sample
        for (float d = l2 - free_resolution; d > 0.0; d -= free_resolution) ++c;
        first[i + 1] = c;
    }
    std::vector<int32_t> beam(nh, -1);
    int32_t idx = 0;
    for (size_t i = 0; i < nh; ++i) {
        first[i + 1] += first[i];
        if (kept[i]) beam[i] = idx++;
    }
    xy.resize(4 * (size_t)first[nh]);
    l_ray_idx.resize(first[nh]);
    l_rays.resize(6 * (size_t)idx);
#pragma omp parallel for num_threads(kHostThreads) schedule(static)
    for (long i = 0; i < (long)nh; ++i) {
        if (!kept[i]) continue;
        float ex, ey, ez, nx, ny, nz, l;
        end_point((size_t)i, ex, ey, ez, nx, ny, nz, l);
        const int32_t id = beam[i];
        size_t w = first[i];
        auto put = [&](float a, float b, float c, float lab, int32_t ray) {
            float *o = &xy[4 * w];
            o[0] = a;
            o[1] = b;
            o[2] = c;
            o[3] = lab;
            l_ray_idx[w++] = ray;
        };
        put(ex, ey, ez, 1.0f, -1);
        put(x0, y0, z0, 0.0f, id);
        {   // beam_sample from the re-projected end point
            const float l2 = (float)sqrt((ex - x0) * (ex - x0) + (ey - y0) * (ey - y0) + (ez - z0) * (ez - z0));
            const float mx = (ex - x0) / l2, my = (ey - y0) / l2, mz = (ez - z0) / l2;
            float d = l2 - free_resolution;
            while (d > 0.0) {
                put(x0 + mx * d, y0 + my * d, z0 + mz * d, 0.0f, id);
                d -= free_resolution;
            }
        }
        l = l - free_resolution;
        const float ray[6] = {x0, y0, z0, x0 + nx * l, y0 + ny * l, z0 + nz * l};
        std::memcpy(&l_rays[6 * (size_t)id], ray, sizeof(ray));
    }
    stats.n_hits = (uint64_t)idx;
    stats.n_frees = xy.size() / 4 - (uint64_t)idx;
}

// Training rows of every block (bgkloctomap.cpp:141-170): members in CSR order; a hit becomes a degenerate segment with
// label 1, a free sample contributes its beam once per block (at the position of the beam's first sample) with label 0.
void BGKOctoMap::build_rows_l() {
    // Members of a block are in ascending source order and the samples of one beam are consecutive in `xy`, so the
    // entries of a beam are adjacent inside a block: "once per block" = "differs from the previous entry's beam".
    const long nblk = (long)train_off.size() - 1;
    rows_off.assign((size_t)std::max(nblk, 0L) + 1, 0u);
    auto emits = [&](uint32_t k, uint32_t k0) {
        const int32_t r = l_ray_idx[train_src[k]];
        return r < 0 || k == k0 || l_ray_idx[train_src[k - 1]] != r;
    };
#pragma omp parallel for num_threads(kHostThreads) schedule(dynamic, 256)
    for (long b = 0; b < nblk; ++b) {
        uint32_t c = 0;
        for (uint32_t k = train_off[b]; k < train_off[b + 1]; ++k) c += emits(k, train_off[b]) ? 1u : 0u;
        rows_off[b + 1] = c;
    }
    for (long b = 0; b < nblk; ++b) rows_off[b + 1] += rows_off[b];
    train_rows.resize(8 * (size_t)rows_off[(size_t)std::max(nblk, 0L)]);
#pragma omp parallel for num_threads(kHostThreads) schedule(dynamic, 256)
    for (long b = 0; b < nblk; ++b) {
        float *o = train_rows.data() + 8 * (size_t)rows_off[b];
        for (uint32_t k = train_off[b]; k < train_off[b + 1]; ++k) {
            if (!emits(k, train_off[b])) continue;
            const uint32_t src = train_src[k];
            const int32_t r = l_ray_idx[src];
            if (r < 0) {
                const float *p = &xy[4 * (size_t)src];
                const float row[8] = {p[0], p[1], p[2], p[0], p[1], p[2], 1.0f, 0.0f};
                std::memcpy(o, row, sizeof(row));
            } else {
                const float *q = &l_rays[6 * (size_t)r];
                const float row[8] = {q[0], q[1], q[2], q[3], q[4], q[5], 0.0f, 0.0f};
                std::memcpy(o, row, sizeof(row));
            }
            o += 8;
        }
    }
    // work counters in rows (what the oracle counts for this variant)
    stats.train_reads = stats.pair_evals = 0;
    for (const Pass &ps : passes)
        for (size_t t = 0; t < ps.blocks.size(); ++t) {
            uint64_t nr = 0;
            for (int q = 0; q < 7; ++q) {
                const int32_t tb = ps.nbr[7 * t + q];
                if (tb >= 0) nr += rows_off[tb + 1] - rows_off[tb];
            }
            stats.train_reads += nr;
            stats.pair_evals += nr * (ps.leaf_off[t + 1] - ps.leaf_off[t]);
        }
}

// ------------------------------------------------- partition + pack (stages B..E host part)
namespace {
struct AxisCand {
    int64_t idx[3];
    int n;
};
// block indices (with the +524288 bias) whose CLOSED fp32 box [c-h, c+h] holds v on one axis
inline AxisCand axis_candidates(float v, float size, float h) {
    AxisCand r;
    r.n = 0;
    const int64_t i0 = int64_t(v / (double)size + 524288.5);
    for (int64_t i = i0 - 1; i <= i0 + 1; ++i) {
        const float c = (i - 524288) * size;
        if (c - h <= v && v <= c + h) r.idx[r.n++] = i;
    }
    return r;
}
}  // namespace

bool BGKOctoMap::partition_and_pack(bool ungated) {
    scan_flags = ungated ? LA3DM_SCAN_UPDATE_UNGATED : 0u;
    passes.clear();
    prune_list.clear();
    train_xyzy.clear();
    train_src.clear();
    train_off.assign(1, 0u);
    const size_t npts = xy.size() / 4;
    if (npts == 0) return false;
    const double t0 = wall();
    const float bs = block_size;
    const float h = bs / 2.0f;

    // bounding box of the training set, candidate block list (float-stepped, repeats kept)
    float lo[3] = {xy[0], xy[1], xy[2]}, hi[3] = {xy[0], xy[1], xy[2]};
    {
        float l0 = lo[0], l1 = lo[1], l2 = lo[2], h0 = hi[0], h1 = hi[1], h2 = hi[2];
#pragma omp parallel for num_threads(npts > 100000 ? kHostThreads : 1) schedule(static) reduction(min : l0, l1, l2) reduction(max : h0, h1, h2)
        for (long i = 1; i < (long)npts; ++i) {
            const float *p = &xy[4 * (size_t)i];
            l0 = std::min(l0, p[0]);
            l1 = std::min(l1, p[1]);
            l2 = std::min(l2, p[2]);
            h0 = std::max(h0, p[0]);
            h1 = std::max(h1, p[1]);
            h2 = std::max(h2, p[2]);
        }
        lo[0] = l0; lo[1] = l1; lo[2] = l2;
        hi[0] = h0; hi[1] = h1; hi[2] = h2;
        // The reference's reduction uses `<`, which a NaN never wins: NaN coordinates are ignored, except in the first
        // point, which seeds the reduction and never loses — that axis' limits are NaN and no candidate block is made.
        for (int a = 0; a < 3; ++a)
            if (xy[a] != xy[a]) lo[a] = hi[a] = xy[a];
    }
    std::vector<BlockHashKey> bbox_keys;
    for (float x = lo[0] - bs; x <= hi[0] + 2 * bs; x += bs)
        for (float y = lo[1] - bs; y <= hi[1] + 2 * bs; y += bs)
            for (float z = lo[2] - bs; z <= hi[2] + 2 * bs; z += bs) bbox_keys.push_back(block_to_hash_key(x, y, z));
    stats.n_bbox_blocks = bbox_keys.size();
    std::unordered_map<BlockHashKey, int32_t> in_bbox;  // key -> training-block index (or -1)
    in_bbox.reserve(bbox_keys.size() * 2);
    for (BlockHashKey k : bbox_keys) in_bbox.emplace(k, -1);

    // membership: every (block, point) pair with the point in the block's closed box
    struct Member {
        BlockHashKey key;
        uint32_t pt;
    };
    std::vector<Member> members;
    {
        // contiguous point ranges per thread, concatenated in range order: the list is the serial loop's list
        const int team = npts > 100000 ? kHostThreads : 1;
        std::vector<std::vector<Member>> part((size_t)team);
#pragma omp parallel for num_threads(team) schedule(static, 1)
        for (int t = 0; t < team; ++t) {
            const size_t i0 = npts * (size_t)t / (size_t)team, i1 = npts * (size_t)(t + 1) / (size_t)team;
            std::vector<Member> &out = part[(size_t)t];
            out.reserve((i1 - i0) + (i1 - i0) / 8);
            for (size_t i = i0; i < i1; ++i) {
                const AxisCand ax = axis_candidates(xy[4 * i], bs, h), ay = axis_candidates(xy[4 * i + 1], bs, h),
                               az = axis_candidates(xy[4 * i + 2], bs, h);
                for (int a = 0; a < ax.n; ++a)
                    for (int b = 0; b < ay.n; ++b)
                        for (int c = 0; c < az.n; ++c)
                            out.push_back(Member{(ax.idx[a] << 40) | (ay.idx[b] << 20) | az.idx[c], (uint32_t)i});
            }
        }
        std::vector<size_t> off((size_t)team + 1, 0);
        for (int t = 0; t < team; ++t) off[(size_t)t + 1] = off[(size_t)t] + part[(size_t)t].size();
        members.resize(off[(size_t)team]);
#pragma omp parallel for num_threads(team) schedule(static, 1)
        for (int t = 0; t < team; ++t)
            if (!part[(size_t)t].empty())
                std::memcpy(members.data() + off[(size_t)t], part[(size_t)t].data(), part[(size_t)t].size() * sizeof(Member));
    }
    // group by block; inside a block keep ascending point index.  (libstdc++ parallel mode, a small team: the sort is
    // the largest single item of the host partition; a stable sort has one result whatever the thread count.)
    if (members.size() > 100000)
        __gnu_parallel::stable_sort(members.begin(), members.end(), [](const Member &a, const Member &b) { return a.key < b.key; },
                                    __gnu_parallel::default_parallel_tag(kHostThreads));
    else
        std::stable_sort(members.begin(), members.end(), [](const Member &a, const Member &b) { return a.key < b.key; });

    // "geo" blocks = every block that geometrically holds points (what an R-tree query sees);
    // trained blocks = geo blocks that are also in the candidate list.
    std::unordered_map<BlockHashKey, char> geo;
    uint32_t n_train_blk = 0;
    {
        std::vector<size_t> start;  // first member of every block group (+ end)
        for (size_t i = 0; i < members.size(); ++i)
            if (i == 0 || members[i].key != members[i - 1].key) start.push_back(i);
        start.push_back(members.size());
        geo.reserve(start.size() * 2 + 16);
        std::vector<size_t> tgroup;  // groups that are training blocks, in key order
        for (size_t g = 0; g + 1 < start.size(); ++g) {
            const BlockHashKey key = members[start[g]].key;
            geo.emplace(key, 1);
            auto it = in_bbox.find(key);
            if (it == in_bbox.end()) continue;
            it->second = (int32_t)n_train_blk++;
            tgroup.push_back(g);
            train_off.push_back(train_off.back() + (uint32_t)(start[g + 1] - start[g]));
        }
        train_xyzy.resize(4 * (size_t)train_off.back());
        if (variant == 3) train_src.resize(train_off.back());
#pragma omp parallel for num_threads(kHostThreads) schedule(dynamic, 256)
        for (long b = 0; b < (long)tgroup.size(); ++b) {
            const size_t g = tgroup[(size_t)b];
            size_t w = train_off[(size_t)b];
            for (size_t k = start[g]; k < start[g + 1]; ++k, ++w) {
                std::memcpy(&train_xyzy[4 * w], &xy[4 * (size_t)members[k].pt], 4 * sizeof(float));
                if (variant == 3) train_src[w] = members[k].pt;
            }
        }
    }
    stats.n_train_blocks = n_train_blk;
    train_max_n = 0;
    train_sum_n2 = 0;
    for (size_t b = 0; b + 1 < train_off.size(); ++b) {
        const uint64_t nb = train_off[b + 1] - train_off[b];
        train_max_n = std::max<uint32_t>(train_max_n, (uint32_t)nb);
        train_sum_n2 += nb * nb;
    }

    // test blocks: candidate blocks whose extended block holds any point; list order kept
    std::unordered_map<BlockHashKey, uint32_t> times_seen;
    std::vector<std::pair<BlockHashKey, uint32_t>> test;  // (key, occurrence number)
    for (BlockHashKey k : bbox_keys) {
        const ExtendedBlock e = get_extended_block(k);
        bool any = false;
        for (int q = 0; q < 7 && !any; ++q) any = geo.find(e[q]) != geo.end();
        if (!any) continue;
        test.emplace_back(k, times_seen[k]++);
        prune_list.push_back(k);
    }
    stats.n_test_blocks = test.size();
    // Device-side load balance: hand the GPU the heaviest test blocks first (longest-
    // processing-time order, weight = training points in the 7-neighbourhood).  The blocks are
    // independent, so the order only changes the layout of the packed arrays, not the results.
    {
        auto weight = [&](BlockHashKey k) {
            const ExtendedBlock e = get_extended_block(k);
            uint32_t w = 0;
            for (int q = 0; q < 7; ++q) {
                auto it = in_bbox.find(e[q]);
                if (it != in_bbox.end() && it->second >= 0) w += train_off[it->second + 1] - train_off[it->second];
            }
            return w;
        };
        std::vector<std::pair<uint32_t, uint32_t>> order(test.size());  // (weight, position)
        for (size_t i = 0; i < test.size(); ++i) order[i] = {weight(test[i].first), (uint32_t)i};
        std::stable_sort(order.begin(), order.end(),
                         [](const std::pair<uint32_t, uint32_t> &a, const std::pair<uint32_t, uint32_t> &b) { return a.first > b.first; });
        std::vector<std::pair<BlockHashKey, uint32_t>> sorted(test.size());
        for (size_t i = 0; i < test.size(); ++i) sorted[i] = test[order[i].second];
        test.swap(sorted);
    }
    const double t1 = wall();
    stats.t_partition = t1 - t0;

    uint32_t max_occ = 0;
    for (auto &t : test) max_occ = std::max(max_occ, t.second);
    passes.resize(test.empty() ? 0 : max_occ + 1);
    stats.voxel_updates = stats.train_reads = stats.pair_evals = 0;
    // find or create the blocks (bgkoctomap.cpp:298-305): look-ups and insertions in list order on one thread, the
    // constructors of the missing ones (a node slab each) on the team
    const long ntest = (long)test.size();
    std::vector<Block *> tblk((size_t)ntest, nullptr);
    {
        std::vector<long> missing;
        std::unordered_map<BlockHashKey, long> first_missing;
        for (long t = 0; t < ntest; ++t) {
            auto bit = block_arr.find(test[(size_t)t].first);
            if (bit != block_arr.end()) tblk[(size_t)t] = bit->second;
            else if (first_missing.emplace(test[(size_t)t].first, t).second) missing.push_back(t);
        }
#pragma omp parallel for num_threads(kHostThreads) schedule(static)
        for (long k = 0; k < (long)missing.size(); ++k) {
            const long t = missing[(size_t)k];
            tblk[(size_t)t] = new Block(hash_key_to_block(test[(size_t)t].first));
        }
        for (long t : missing) block_arr.emplace(test[(size_t)t].first, tblk[(size_t)t]);
        for (long t = 0; t < ntest; ++t)
            if (tblk[(size_t)t] == nullptr) tblk[(size_t)t] = tblk[(size_t)first_missing[test[(size_t)t].first]];
    }
    // position of every test block inside its pass, then neighbour table / centre / leaf count on the team
    std::vector<uint32_t> pos((size_t)ntest), nleaf((size_t)ntest);
    for (long t = 0; t < ntest; ++t) {
        Pass &ps = passes[test[(size_t)t].second];
        pos[(size_t)t] = (uint32_t)ps.blocks.size();
        ps.keys.push_back(test[(size_t)t].first);
        ps.blocks.push_back(tblk[(size_t)t]);
    }
    for (Pass &ps : passes) {
        ps.center.resize(3 * ps.blocks.size());
        ps.nbr.resize(7 * ps.blocks.size());
        ps.leaf_off.assign(ps.blocks.size() + 1, 0u);
    }
    uint64_t sum_reads = 0, sum_pairs = 0, sum_leaves = 0;
#pragma omp parallel num_threads(kHostThreads) reduction(+ : sum_reads, sum_pairs, sum_leaves)
    {
        std::vector<uint32_t> scratch;
#pragma omp for schedule(static)
        for (long t = 0; t < ntest; ++t) {
            Pass &ps = passes[test[(size_t)t].second];
            const uint32_t b = pos[(size_t)t];
            Block *blk = tblk[(size_t)t];
            const point3f c = blk->get_center();
            ps.center[3 * (size_t)b] = c.x();
            ps.center[3 * (size_t)b + 1] = c.y();
            ps.center[3 * (size_t)b + 2] = c.z();
            const ExtendedBlock e = blk->get_extended_block();
            uint64_t npts_nb = 0;
            for (int q = 0; q < 7; ++q) {
                auto it = in_bbox.find(e[q]);
                const int32_t tb = it == in_bbox.end() ? -1 : it->second;
                ps.nbr[7 * (size_t)b + q] = tb;
                if (tb >= 0) npts_nb += train_off[tb + 1] - train_off[tb];
            }
            scratch.clear();
            blk->collect_leaves(scratch);
            nleaf[(size_t)t] = (uint32_t)scratch.size();
            ps.leaf_off[(size_t)b + 1] = (uint32_t)scratch.size();
            sum_leaves += scratch.size();
            sum_reads += npts_nb;
            sum_pairs += npts_nb * scratch.size();
        }
    }
    stats.voxel_updates = sum_leaves;
    stats.train_reads = sum_reads;
    stats.pair_evals = sum_pairs;
    for (Pass &ps : passes) {
        for (size_t b = 0; b < ps.blocks.size(); ++b) ps.leaf_off[b + 1] += ps.leaf_off[b];
        ps.leaf_key.resize(ps.leaf_off.back());
    }
#pragma omp parallel num_threads(kHostThreads)
    {
        std::vector<uint32_t> scratch;
#pragma omp for schedule(static)
        for (long t = 0; t < ntest; ++t) {
            Pass &ps = passes[test[(size_t)t].second];
            scratch.clear();
            tblk[(size_t)t]->collect_leaves(scratch);
            std::memcpy(ps.leaf_key.data() + ps.leaf_off[pos[(size_t)t]], scratch.data(), scratch.size() * sizeof(uint32_t));
        }
    }
    for (Pass &ps : passes) {
        const size_t nl = ps.leaf_key.size();
        ps.alpha.resize(nl);
        ps.beta.resize(nl);
        ps.state.assign(nl, 0);
#pragma omp parallel for num_threads(kHostThreads) schedule(static)
        for (long b = 0; b < (long)ps.blocks.size(); ++b)
            for (size_t l = ps.leaf_off[b]; l < ps.leaf_off[b + 1]; ++l) {
                const OcTreeNode &nd = (*ps.blocks[b])[(OcTreeHashKey)ps.leaf_key[l]];
                ps.alpha[l] = nd.m_A;
                ps.beta[l] = nd.m_B;
            }
    }
    stats.t_pack = wall() - t1;
    return !passes.empty();
}

int BGKOctoMap::run_scan(la3dm_bgk_scan *s, la3dm_bgk_counters *c) {
    if (variant == 3) return la3dm_bgkl_scan_host(ctx, s, c);
    return variant == 1 ? la3dm_gp_scan_host(ctx, s, c) : la3dm_bgk_scan_host(ctx, s, c);
}

la3dm_bgk_scan BGKOctoMap::packed(size_t pass) {
    bind();
    la3dm_bgk_scan s;
    std::memset(&s, 0, sizeof(s));
    Pass &ps = passes.at(pass);
    s.train_xyzy = train_xyzy.data();
    s.train_off = train_off.data();
    s.n_train_pts = (uint32_t)(train_xyzy.size() / 4);
    s.n_train_blk = (uint32_t)(train_off.size() - 1);
    s.nbr = ps.nbr.data();
    s.blk_center = ps.center.data();
    s.leaf_off = ps.leaf_off.data();
    s.n_test_blk = (uint32_t)ps.blocks.size();
    s.n_leaf = (uint32_t)ps.leaf_key.size();
    s.leaf_key = ps.leaf_key.data();
    s.alpha = ps.alpha.data();
    s.beta = ps.beta.data();
    s.state = ps.state.data();
    s.flags = scan_flags;
    if ((uint64_t)s.n_leaf == ((uint64_t)s.n_test_blk << (3 * (block_depth - 1)))) s.flags |= LA3DM_SCAN_FULL_BLOCKS;  // no test block of this pass is pruned
    s.train_max_n = train_max_n;
    s.train_sum_n2 = train_sum_n2;
    if (variant == 3) {  // BGKLOctoMap: segment rows (8 floats) instead of points
        s.train_xyzy = train_rows.data();
        s.train_off = rows_off.data();
        s.n_train_pts = (uint32_t)(train_rows.size() / 8);
    }
    return s;
}

void BGKOctoMap::refresh_pass(size_t p) {
    Pass &ps = passes[p];
#pragma omp parallel for num_threads(kHostThreads) schedule(static)
    for (long b = 0; b < (long)ps.blocks.size(); ++b)
        for (size_t l = ps.leaf_off[b]; l < ps.leaf_off[b + 1]; ++l) {
            const OcTreeNode &nd = (*ps.blocks[b])[(OcTreeHashKey)ps.leaf_key[l]];
            ps.alpha[l] = nd.m_A;
            ps.beta[l] = nd.m_B;
        }
}

void BGKOctoMap::write_nodes(size_t p) {
    Pass &ps = passes[p];
#pragma omp parallel for num_threads(kHostThreads) schedule(static)
    for (long b = 0; b < (long)ps.blocks.size(); ++b)
        for (size_t l = ps.leaf_off[b]; l < ps.leaf_off[b + 1]; ++l) {
            const uint8_t st = ps.state[l];
            if (!(st & LA3DM_LEAF_UPDATED)) continue;
            OcTreeNode &nd = (*ps.blocks[b])[(OcTreeHashKey)ps.leaf_key[l]];
            nd.classified = true;
            nd.m_A = ps.alpha[l];
            nd.m_B = ps.beta[l];
            nd.state = (State)(st & 3u);
        }
}

// Pass 0 (all distinct test blocks) has been run by the caller; repeated keys of the
// candidate list (a float-stepping artefact, normally none) are replayed here one pass
// after the other so that they see the previous pass's posterior, as the serial reference does.
void BGKOctoMap::commit() {
    bind();
    const double t0 = wall();
    if (!passes.empty()) write_nodes(0);
    for (size_t p = 1; p < passes.size(); ++p) {
        refresh_pass(p);
        la3dm_bgk_scan s = packed(p);
        if (ctx == nullptr) throw std::runtime_error("BGKOctoMap::commit: no device context");
        if (run_scan(&s, nullptr) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::commit: ") + la3dm_last_error(ctx));
        write_nodes(p);
    }
    const double t1 = wall();
    stats.t_commit = t1 - t0;
    // the blocks of pass 0 are the distinct test blocks (prune_list only repeats some of them; prune is idempotent)
    if (!passes.empty()) {
        std::vector<Block *> &blks = passes[0].blocks;
#pragma omp parallel for num_threads(kHostThreads) schedule(static)
        for (long b = 0; b < (long)blks.size(); ++b) blks[b]->prune();
    }
    stats.t_prune = wall() - t1;
}

void BGKOctoMap::set_shard(uint32_t rank, uint32_t world, la3dm_allgatherv_fn fn, void *user) {
    if (dmap == nullptr) throw std::runtime_error("set_shard: the map is not in device-resident mode");
    if (la3dm_devmap_set_shard(dmap, rank, world, fn, user) != LA3DM_OK) throw std::runtime_error(la3dm_last_error(ctx));
    shard_cfg = {rank, world, fn, user};   // (reconfigure() rebuilds the device map and applies it again)
}

bool BGKOctoMap::prepare(const float *xyz, size_t n, size_t stride, const point3f &origin, float ds_resolution,
                         float free_res, float max_range) {
    bind();
    ensure_host_mode();
    stats = ScanStats();
    const double t0 = wall();
    if (variant == 3) {
        get_training_data_l(xyz, n, stride, origin, ds_resolution, free_res, max_range);
        stats.t_frontend = wall() - t0;
        const bool work = partition_and_pack(false);
        build_rows_l();
        return work;
    }
    get_training_data(xyz, n, stride, origin, ds_resolution, free_res, max_range);
    stats.t_frontend = wall() - t0;
    const bool work = partition_and_pack(false);
    scan_flags |= LA3DM_SCAN_LABELS_01;  // hits are labelled 1.0f, free samples 0.0f
    return work;
}

bool BGKOctoMap::prepare_training_data(const float *xyzy, size_t n, bool ungated) {
    bind();
    ensure_host_mode();
    stats = ScanStats();
    xy.assign(xyzy, xyzy + 4 * n);
    for (size_t i = 0; i < n; ++i) (xyzy[4 * i + 3] > 0.5f ? stats.n_hits : stats.n_frees)++;
    return partition_and_pack(ungated);
}

void BGKOctoMap::take_device_stats(const la3dm_devmap_stats &ds) {
    stats = ScanStats();
    stats.n_hits = ds.n_hits;
    stats.n_frees = ds.n_frees;
    stats.n_bbox_blocks = ds.n_bbox_blocks;
    stats.n_train_blocks = ds.n_train_blocks;
    stats.n_test_blocks = ds.n_test_blocks;
    stats.voxel_updates = ds.voxel_updates;
    stats.train_reads = ds.train_reads;
    stats.pair_evals = ds.pair_evals;
    stats.t_frontend = ds.t_frontend;
    stats.t_partition = ds.t_partition;
    stats.t_pack = ds.t_pack;
    stats.t_device = ds.t_kernel;
    stats.t_commit = ds.t_commit;
    stats.t_gather = ds.t_gather;
}

void BGKOctoMap::insert_pointcloud(const float *xyz, size_t n, size_t stride, const point3f &origin, float ds_resolution,
                                   float free_res, float max_range) {
    bind();
    const double t0 = wall();
    if (ctx == nullptr) throw std::runtime_error("BGKOctoMap::insert_pointcloud: no device context (there is no CPU path)");
    if (dmap != nullptr) {  // device-resident mode: the whole scan runs on the GPU
        const float o[3] = {origin.x(), origin.y(), origin.z()};
        la3dm_devmap_stats ds;
        if (la3dm_devmap_insert_pointcloud_host(dmap, xyz, (uint32_t)n, (uint32_t)stride, o, ds_resolution, free_res, max_range,
                                                &ds) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::insert_pointcloud: ") + la3dm_last_error(ctx));
        take_device_stats(ds);
        stats.t_total = wall() - t0;
        mirror_dirty = true;
        return;
    }
    if (!prepare(xyz, n, stride, origin, ds_resolution, free_res, max_range)) return;
    const double t1 = wall();
    {
        la3dm_bgk_scan s = packed(0);
        la3dm_bgk_counters c;
        if (run_scan(&s, &c) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::insert_pointcloud: ") + la3dm_last_error(ctx));
        stats.n_tiles += c.n_tiles;
    }
    stats.t_device = wall() - t1;
    commit();
    stats.t_total = wall() - t0;
}

void BGKOctoMap::insert_pointcloud_device(const float *d_xyz, size_t n, const point3f &origin, float ds_resolution, float free_res,
                                          float max_range) {
    bind();
    const double t0 = wall();
    if (dmap == nullptr) throw std::runtime_error("BGKOctoMap::insert_pointcloud_device: the map is not device resident");
    const float o[3] = {origin.x(), origin.y(), origin.z()};
    la3dm_devmap_stats ds;
    if (la3dm_devmap_insert_pointcloud_device(dmap, d_xyz, (uint32_t)n, o, ds_resolution, free_res, max_range, &ds) != LA3DM_OK)
        throw std::runtime_error(std::string("BGKOctoMap::insert_pointcloud_device: ") + la3dm_last_error(ctx));
    take_device_stats(ds);
    stats.t_total = wall() - t0;
    mirror_dirty = true;
}

void BGKOctoMap::insert_training_data(const GPPointCloud &cloud) {
    bind();
    const double t0 = wall();
    if (ctx == nullptr) throw std::runtime_error("BGKOctoMap::insert_training_data: no device context (there is no CPU path)");
    std::vector<float> flat;
    flat.reserve(cloud.size() * 4);
    for (const GPPointType &p : cloud) flat.insert(flat.end(), {p.first.x(), p.first.y(), p.first.z(), p.second});
    if (dmap != nullptr && variant != 3) {  // device-resident mode (a BGK-L map has no beams for a labelled set)
        la3dm_devmap_stats ds;
        if (la3dm_devmap_insert_training_data_host(dmap, flat.data(), (uint32_t)cloud.size(), &ds) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::insert_training_data: ") + la3dm_last_error(ctx));
        take_device_stats(ds);
        stats.t_total = wall() - t0;
        mirror_dirty = true;
        return;
    }
    if (!prepare_training_data(flat.data(), cloud.size(), true)) return;
    const double t1 = wall();
    {
        la3dm_bgk_scan s = packed(0);
        if (run_scan(&s, nullptr) != LA3DM_OK)
            throw std::runtime_error(std::string("BGKOctoMap::insert_training_data: ") + la3dm_last_error(ctx));
    }
    stats.t_device = wall() - t1;
    commit();
    stats.t_total = wall() - t0;
}

}  // namespace la3dm

extern "C" void la3dm_node_ab(const void *node, float *A, float *B) {
    const la3dm::Occupancy *n = static_cast<const la3dm::Occupancy *>(node);
    *A = n->m_A;
    *B = n->m_B;
}
