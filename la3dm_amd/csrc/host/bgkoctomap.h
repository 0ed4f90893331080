// bgkoctomap.h — host side of the MI355X BGKOctoMap.
//
// Same public surface and data layout as the reference's BGKOctoMap family
// (include/bgkoctomap/{bgkoctomap,bgkblock,bgkoctree,bgkoctree_node}.h,
// include/common/point3f.h) so that the ROS nodes' call sequence
// (src/bgkoctomap/bgkoctomap_static_node.cpp:86-139) works unchanged:
//
//     la3dm::BGKOctoMap map(resolution, block_depth, sf2, ell, free_thresh,
//                           occupied_thresh, var_thresh, prior_A, prior_B);
//     map.insert_pointcloud(cloud, origin, ds_resolution, free_res, max_range);
//     for (auto it = map.begin_leaf(); it != map.end_leaf(); ++it) { it.get_loc(); it.get_node()...}
//
// What is different underneath: block hashing, neighbour gather (a counting sort by
// block instead of an R-tree) and octree bookkeeping stay on the host in this file's
// implementation; kernel evaluation and the alpha/beta fusion run on the GPU through
// the C ABI of include/la3dm_hip.h.  There is no CPU inference path: constructing a
// map without a HIP device throws std::runtime_error.
#ifndef LA3DM_AMD_BGKOCTOMAP_H
#define LA3DM_AMD_BGKOCTOMAP_H

#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <fstream>
#include <ostream>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../../include/la3dm_hip.h"

namespace la3dm_region {
struct Query;   // region_contract.h
}
namespace la3dm_region_blocks {
struct Box;   // region_blocks.h
}

extern "C" void la3dm_node_ab(const void *node, float *A, float *B);  // (m_A, m_B) of an Occupancy

namespace la3dm {

/// 3 floats; the scalar type of every coordinate (reference: include/common/point3f.h).
class point3f {
public:
    point3f() : d{0.f, 0.f, 0.f} {}
    point3f(float x, float y, float z) : d{x, y, z} {}
    float &x() { return d[0]; }
    float &y() { return d[1]; }
    float &z() { return d[2]; }
    const float &x() const { return d[0]; }
    const float &y() const { return d[1]; }
    const float &z() const { return d[2]; }
    float &operator()(unsigned i) { return d[i]; }
    const float &operator()(unsigned i) const { return d[i]; }
    point3f operator+(const point3f &o) const { return point3f(d[0] + o.d[0], d[1] + o.d[1], d[2] + o.d[2]); }
    point3f operator-(const point3f &o) const { return point3f(d[0] - o.d[0], d[1] - o.d[1], d[2] - o.d[2]); }
    point3f operator*(float s) const { return point3f(d[0] * s, d[1] * s, d[2] * s); }
    void operator+=(const point3f &o) { d[0] += o.d[0]; d[1] += o.d[1]; d[2] += o.d[2]; }
    void operator-=(const point3f &o) { d[0] -= o.d[0]; d[1] -= o.d[1]; d[2] -= o.d[2]; }
    bool operator==(const point3f &o) const { return d[0] == o.d[0] && d[1] == o.d[1] && d[2] == o.d[2]; }
    /// double sqrt of a float sum, as the reference (point3f.h:207-214)
    double norm() const { return std::sqrt((double)(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])); }

private:
    float d[3];
};

typedef int OcTreeHashKey;     // (depth << 16) + index
typedef int64_t BlockHashKey;  // 3 x 20-bit block indices
typedef std::array<BlockHashKey, 7> ExtendedBlock;  // self,+x,-x,+y,-y,+z,-z

/// UNCERTAIN is used by the BGKLV variant only (reference bgklvoctree_node.h:11-13 numbers it 3 and PRUNED 4; the
/// C view and the device use those codes for LV maps, this enum is symbolic).
enum class State : char { FREE, OCCUPIED, UNKNOWN, PRUNED, UNCERTAIN };

inline OcTreeHashKey node_to_hash_key(unsigned short depth, unsigned short index) { return (depth << 16) + index; }
inline void hash_key_to_node(OcTreeHashKey key, unsigned short &depth, unsigned short &index) {
    depth = (unsigned short)(key >> 16);
    index = (unsigned short)(key & 0xFFFF);
}

/// Beta posterior of one voxel. 16 bytes: classified@0, m_A@4, m_B@8, state@12
/// (reference: include/bgkoctomap/bgkoctree_node.h:76-81).
class Occupancy {
    friend class BGKOctoMap;
    friend class BGKLVOctoMap;
    friend class OcTree;
    friend void ::la3dm_node_ab(const void *node, float *A, float *B);

public:
    /// BGK: (prior_A, prior_B); GP: (m_ivar, ivar) = (0, min_ivar)  (gpoctree_node.h:34)
    Occupancy() : classified(false), m_A(init_A), m_B(init_B), state(State::UNKNOWN) {}
    Occupancy(float A, float B);
    // like the reference, copying does not carry `classified`
    Occupancy(const Occupancy &o) : m_A(o.m_A), m_B(o.m_B), state(o.state) {}
    Occupancy &operator=(const Occupancy &o) {
        m_A = o.m_A;
        m_B = o.m_B;
        state = o.state;
        return *this;
    }

    /// Host twin of the device-side update (kept for API parity; the map itself
    /// never calls it — the GPU does the updates).
    void update(float ybar, float kbar);

    float get_prob() const;
    float get_var() const;
    State get_state() const { return state; }
    void prune() { state = State::PRUNED; }
    bool operator==(const Occupancy &rhs) const {
        return state != State::UNKNOWN && state != State::UNCERTAIN && state == rhs.state;
    }

    /// The reference node's stream operators (src/bgkoctomap/bgkoctree_node.cpp:46-62; unused by its own nodes): the binary
    /// pair writes m_A, m_B as 8 raw bytes and reads them back THROUGH the (A, B) constructor — which adds the priors again,
    /// as the reference does —; the text form is "(m_A m_B prob)".
    friend std::ofstream &operator<<(std::ofstream &os, const Occupancy &oc);
    friend std::ifstream &operator>>(std::ifstream &is, Occupancy &oc);
    friend std::ostream &operator<<(std::ostream &os, const Occupancy &oc);

    bool classified;

private:
    void classify();
    float m_A;
    float m_B;
    State state;

    static float sf2, ell, prior_A, prior_B, free_thresh, occupied_thresh, var_thresh;
    // GPOctoMap statics (src/gpoctomap/gpoctree_node.cpp:7-17); for GP nodes m_A holds m_ivar, m_B holds ivar
    static int variant;  // 0 BGK, 1 GP, 2 BGKLV
    static float min_W;  // BGKLV (bgklvoctree_node.cpp:15)
    static bool original_size;
    static float init_A, init_B, noise, l, max_ivar, min_ivar, min_known_ivar;
};
typedef Occupancy OcTreeNode;
static_assert(sizeof(Occupancy) == 16, "node layout must match the reference (16 bytes)");

/// Fixed-depth test-data octree of one block: layer d holds 8^d nodes, child c of node i
/// is node 8i+c of the next layer (c&4 -> +x, c&2 -> +y, c&1 -> +z).
class OcTree {
    friend class BGKOctoMap;
    friend class BGKLVOctoMap;

public:
    OcTree();
    ~OcTree();
    OcTree(const OcTree &) = delete;
    OcTree &operator=(const OcTree &) = delete;

    bool prune();
    /// overwrite every node from flat (alpha, beta, state|classified<<7) arrays in depth-major node order
    void load_nodes(const float *A, const float *B, const uint8_t *S, size_t n);
    bool is_leaf(OcTreeHashKey key) const;
    bool is_leaf(unsigned short depth, unsigned short index) const;
    bool search(OcTreeHashKey key) const;
    OcTreeNode &operator[](OcTreeHashKey key) const;

    /// Leaves in the reference's LeafIterator order (depth-first, children 7..0).
    class LeafIterator {
    public:
        LeafIterator() : tree(nullptr), top(0) {}
        explicit LeafIterator(const OcTree *t);
        bool operator==(const LeafIterator &o) const {
            return tree == o.tree && top == o.top && (top == 0 || stack[top - 1] == o.stack[o.top - 1]);
        }
        bool operator!=(const LeafIterator &o) const { return !(*this == o); }
        LeafIterator &operator++();
        LeafIterator operator++(int) {
            LeafIterator r(*this);
            ++(*this);
            return r;
        }
        OcTreeNode &operator*() const { return (*tree)[get_hash_key()]; }
        OcTreeNode &get_node() const { return operator*(); }
        OcTreeHashKey get_hash_key() const { return stack[top - 1]; }

    private:
        void settle();
        const OcTree *tree;
        int top;
        OcTreeHashKey stack[7 * 6 + 2];  // depth <= 6: at most 7 siblings pending per level
    };
    LeafIterator begin_leaf() const { return LeafIterator(this); }
    LeafIterator end_leaf() const { return LeafIterator(); }

    /// Append the leaf keys in LeafIterator order (bulk form used by the packer).
    void collect_leaves(std::vector<uint32_t> &keys) const;

protected:
    OcTreeNode **node_arr;  // node_arr[d] == nullptr once a layer is fully collapsed
    OcTreeNode *slab;       // all layers in one allocation
    bool ever_pruned;
    static unsigned short max_depth;
};

BlockHashKey block_to_hash_key(point3f center);
BlockHashKey block_to_hash_key(float x, float y, float z);
point3f hash_key_to_block(BlockHashKey key);
ExtendedBlock get_extended_block(BlockHashKey key);

/// Voxel LUT, flat and depth-major: entry (d, i) at (8^d - 1)/7 + i
/// (replaces the reference's unordered_map Block::key_loc_map; same values).
std::vector<point3f> init_key_loc_map(float resolution, unsigned short max_depth);

class Block : public OcTree {
    friend class BGKOctoMap;
    friend class BGKLVOctoMap;
    friend BlockHashKey block_to_hash_key(float x, float y, float z);
    friend point3f hash_key_to_block(BlockHashKey key);
    friend ExtendedBlock get_extended_block(BlockHashKey key);

public:
    Block() : OcTree(), center(0.f, 0.f, 0.f) {}
    explicit Block(point3f c) : OcTree(), center(c) {}

    static const point3f &lut(OcTreeHashKey key) {
        return key_loc_map[(0x249249u & ((1u << (3u * (unsigned)(key >> 16))) - 1u)) + (unsigned)(key & 0xFFFF)];
    }
    point3f get_loc(const LeafIterator &it) const { return lut(it.get_hash_key()) + center; }
    float get_size(const LeafIterator &it) const { return float(size / pow(2, it.get_hash_key() >> 16)); }
    point3f get_center() const { return center; }
    point3f get_lim_min() const { return center - point3f(size / 2.0f, size / 2.0f, size / 2.0f); }
    point3f get_lim_max() const { return center + point3f(size / 2.0f, size / 2.0f, size / 2.0f); }
    ExtendedBlock get_extended_block() const;
    /// voxel containing p (index clamped into the block), at the finest layer
    OcTreeNode &search(point3f p) const;
    // ---- finest-layer grid view of a block (reference bgkblock.cpp:131-147, index_map :34-67) ----
    /// voxels per block edge.  (The reference keeps a static cell_num that is initialised once from the default
    /// statics — 8 — and never updated by the map constructor, so its grid view is only meaningful at
    /// block_depth 4; this is the value it has there.)
    static unsigned short cell_num() { return (unsigned short)(1u << (max_depth - 1)); }
    /// grid cell of p, clamped into the block; truncation toward zero as in the reference
    void get_index(const point3f &p, unsigned short &x, unsigned short &y, unsigned short &z) const;
    /// finest-layer node of grid cell (x, y, z): per level the child bit 4 is +x, 2 is +y, 1 is +z
    static OcTreeHashKey get_node(unsigned short x, unsigned short y, unsigned short z);
    point3f get_point(unsigned short x, unsigned short y, unsigned short z) const { return lut(get_node(x, y, z)) + center; }
    OcTreeNode &search(float x, float y, float z) const { return search(point3f(x, y, z)); }

private:
    static std::vector<point3f> key_loc_map;
    static float resolution;
    static float size;
    point3f center;
};

struct ScanStats {
    uint64_t n_hits = 0, n_frees = 0, n_bbox_blocks = 0, n_train_blocks = 0, n_test_blocks = 0;
    uint64_t voxel_updates = 0;  // U
    uint64_t train_reads = 0;    // sum_t sum_{b in E(t)} N_b
    uint64_t pair_evals = 0;     // P
    uint64_t n_tiles = 0;
    double t_frontend = 0, t_partition = 0, t_pack = 0, t_device = 0, t_commit = 0, t_prune = 0, t_total = 0;
    double t_gather = 0;   // sharded device-resident insert with LA3DM_TIMING=1: the all-gather-v of the leaves
};

class BGKOctoMap {
public:
    typedef std::vector<point3f> PointCloud;
    typedef std::pair<point3f, float> GPPointType;
    typedef std::vector<GPPointType> GPPointCloud;

    BGKOctoMap();
    virtual ~BGKOctoMap();
    /// Same argument order as the reference constructor (bgkoctomap.h:50-58); `device`
    /// is the HIP device ordinal (a negative ordinal builds a bookkeeping-only map without a
    /// GPU context — prepare()/packed()/commit() work, insert_* throw; used to test host logic).
    BGKOctoMap(float resolution, unsigned short block_depth, float sf2, float ell, float free_thresh,
               float occupied_thresh, float var_thresh, float prior_A, float prior_B, int device = 0);
    BGKOctoMap(const BGKOctoMap &) = delete;
    BGKOctoMap &operator=(const BGKOctoMap &) = delete;

protected:
    struct GPParams {  // variant-specific constructor arguments (GP: first five; BGKLV: last two)
        float noise, l, min_var, max_var, max_known_var;
        float min_W;
        bool original_size;
    };
    /// shared constructor: variant 0 = BGK (gp == nullptr), 1 = GP
    BGKOctoMap(int variant, float resolution, unsigned short block_depth, float sf2, float ell, float free_thresh,
               float occupied_thresh, float var_thresh, float prior_A, float prior_B, const GPParams *gp, int device);

public:
    float get_resolution() const { return resolution; }
    float get_block_depth() const { return block_depth; }
    float get_block_size() const { return block_size; }
    /// reference bgkoctomap.cpp:66-80 (the same pair in gpoctomap.cpp:55-69, bgkloctomap.cpp:67-81, bgklvoctomap.cpp:73-87):
    /// re-derive the block size and the voxel LUT for a new resolution / block depth.  The reference does this under
    /// whatever blocks the map already holds (their octrees keep the old depth, their centres the old block size — a
    /// filled map is silently corrupted); here it is legal on an EMPTY map only and throws std::logic_error otherwise.
    /// The device context (LUT, kernels' block depth) and the device-resident pool are rebuilt; options set through
    /// la3dm_set_option return to their defaults.
    void set_resolution(float resolution);
    void set_block_depth(unsigned short max_depth);

    /// One scan. xyz: n points, `stride` floats between consecutive points (3 for packed
    /// xyz, 4 for PCL's PointXYZ).  Mirrors insert_pointcloud(const PCLPointCloud&, ...)
    /// (bgkoctomap.h:82-84): ds_resolution < 0 disables the voxel-grid filter,
    /// max_range <= 0 disables the range gate. Empty training set => silent return.
    virtual void insert_pointcloud(const float *xyz, size_t n, size_t stride, const point3f &origin, float ds_resolution,
                                   float free_res = 2.0f, float max_range = -1);
    void insert_pointcloud(const PointCloud &cloud, const point3f &origin, float ds_resolution, float free_res = 2.0f,
                           float max_range = -1) {
        insert_pointcloud(cloud.empty() ? nullptr : &cloud[0].x(), cloud.size(), 3, origin, ds_resolution, free_res,
                          max_range);
    }
#if defined(LA3DM_WITH_PCL)
    template <class PCLCloud>
    void insert_pointcloud(const PCLCloud &cloud, const point3f &origin, float ds_resolution, float free_res = 2.0f,
                           float max_range = -1) {
        insert_pointcloud(cloud.empty() ? nullptr : &cloud.points[0].x, cloud.size(),
                          sizeof(cloud.points[0]) / sizeof(float), origin, ds_resolution, free_res, max_range);
    }
#endif
    /// Pre-labelled training points (y = 1 hit, 0 free); updates are not gated on kbar
    /// (reference bgkoctomap.cpp:82-212, without its null dereference).
    void insert_training_data(const GPPointCloud &xy);
    /// insert_pointcloud for a cloud that already lives in HBM (n packed xyz triples on the map's device): the
    /// device-resident mode only; nothing crosses PCIe but the scalars that size the launches.
    void insert_pointcloud_device(const float *d_xyz, size_t n, const point3f &origin, float ds_resolution,
                                  float free_res = 2.0f, float max_range = -1);

    void get_bbox(point3f &lim_min, point3f &lim_max) const;

    // ---- split form of insert_pointcloud, used by the benchmark and the multi-GPU
    // driver: prepare() runs the front end, the block partition and packs the scan into
    // flat host arrays (valid until the next prepare); the caller runs the kernel
    // (la3dm_bgk_scan_host / _device on any shard of the test blocks) and hands the
    // updated leaf arrays back to commit(), which writes the nodes and prunes.
    /// returns false when there is nothing to do (empty training set)
    bool prepare(const float *xyz, size_t n, size_t stride, const point3f &origin, float ds_resolution, float free_res,
                 float max_range);
    bool prepare_training_data(const float *xyzy, size_t n, bool ungated);
    /// the packed scan (host pointers into this map's buffers): pass 0 = every distinct
    /// test block. (Repeated keys of get_blocks_in_bbox — normally none — form further
    /// passes that commit() replays itself.)
    size_t num_passes() const { return passes.size(); }
    la3dm_bgk_scan packed(size_t pass = 0);
    /// write the updated leaves of pass 0 back into the nodes, replay passes >= 1, prune
    void commit();
    la3dm_ctx *device_ctx() const { return ctx; }
    const ScanStats &last_stats() const { return stats; }

    // ---- device-resident mode: the block pool lives in HBM and a scan runs start
    // to finish on the GPU (front end, partition, predict + fuse, write-back, prune — include/la3dm_hip.h,
    // la3dm_devmap_*).  The host blocks become a mirror that is refreshed lazily, the first time a query
    // (search, begin_leaf, block_count) follows a scan; get_bbox, search_many and export_cells are answered from
    // the pool without a refresh.  This is the DEFAULT for BGK, GP and BGK-L maps with a GPU context (block_depth <= 5;
    // LA3DM_DEVICE_RESIDENT=0 disables it); insert_pointcloud and insert_training_data both run on the pool.  The
    // split prepare()/commit() form is host-orchestrated: calling it moves the map to the host mode for good (the
    // pool is downloaded once).  Results are bit-identical in both modes.
    void set_device_resident(bool on);
    void ensure_host_mode();
    bool is_device_resident() const { return dmap != nullptr; }
    /// Block-sharded insert_pointcloud across `world` GPUs (one process per GPU, every process holds a replica of the map
    /// and inserts the same clouds): see la3dm_devmap_set_shard in include/la3dm_hip.h.  Needs the device-resident mode.
    void set_shard(uint32_t rank, uint32_t world, la3dm_allgatherv_fn fn, void *user);
    void sync_mirror() const;
    void take_device_stats(const la3dm_devmap_stats &ds);
    /// training set (x, y, z, label) the device front end produced for the last scan
    std::vector<float> device_training_data() const;
    const std::vector<float> &last_training_data() const { return xy; }  // x,y,z,label

    /// Voxel walk along the segment start -> end at the base resolution (reference bgkoctomap.h:91-214):
    /// an integer DDA on the voxel indices of the two end points with one error term per axis pair, crossing
    /// into neighbour blocks (which may be missing: next() then reports valid = false).  Starts only if the
    /// block that holds `start` exists.
    class RayCaster {
    public:
        RayCaster(const BGKOctoMap *map, const point3f &start, const point3f &end);
        bool end() const { return n <= 0; }
        /// current voxel: centre (or the dead-reckoned position when its block is missing), a copy of its
        /// node, block and node key; then advance.  Returns whether the block exists.
        bool next(point3f &p, OcTreeNode &node, BlockHashKey &block_key, OcTreeHashKey &node_key);

    private:
        void enter_block(int axis, int inc);
        const BGKOctoMap *map;
        Block *block;
        point3f block_center, current_p;
        int idx[3], inc[3], d2[3];   // voxel index inside the block, step sign, 2 * |delta| per axis
        int err_xy, err_xz, err_yz, n, lim;
        BlockHashKey key;
    };

    class LeafIterator {
    public:
        explicit LeafIterator(const BGKOctoMap *map);
        LeafIterator(std::unordered_map<BlockHashKey, Block *>::const_iterator bit, OcTree::LeafIterator lit)
            : block_it(bit), end_block(bit), leaf_it(lit), end_leaf(lit) {}
        bool operator==(const LeafIterator &o) const { return block_it == o.block_it && leaf_it == o.leaf_it; }
        bool operator!=(const LeafIterator &o) const { return !(*this == o); }
        LeafIterator &operator++();
        OcTreeNode &operator*() const { return *leaf_it; }
        OcTreeNode &get_node() const { return *leaf_it; }
        point3f get_loc() const { return block_it->second->get_loc(leaf_it); }
        float get_size() const { return block_it->second->get_size(leaf_it); }
        BlockHashKey get_block_key() const { return block_it->first; }
        OcTreeHashKey get_node_key() const { return leaf_it.get_hash_key(); }
        std::vector<point3f> get_pruned_locs() const;

    private:
        std::unordered_map<BlockHashKey, Block *>::const_iterator block_it, end_block;
        OcTree::LeafIterator leaf_it, end_leaf;
    };
    LeafIterator begin_leaf() const {
        bind();
        sync_mirror();
        return LeafIterator(this);
    }
    LeafIterator end_leaf() const { return LeafIterator(block_arr.cend(), OcTree::LeafIterator()); }

    OcTreeNode search(point3f p) const;
    OcTreeNode search(float x, float y, float z) const { return search(point3f(x, y, z)); }
    Block *search(BlockHashKey key) const;
    /// search(x, y, z) for n points at once (packed xyz).  In device-resident mode the answers come straight from the
    /// device pool (no mirror refresh); otherwise from the host blocks.  exists[i] = the block exists.
    void search_many(const float *xyz, size_t n, uint8_t *exists, float *A, float *B, uint8_t *state) const;
    /// The client loop over a RayCaster, for n segments at once (rays6: start xyz, end xyz per ray).  Per ray: walk with
    /// next() until the walk ends, `max_steps` rows were produced (flags |= LA3DM_RAY_TRUNCATED) or a row's class is in
    /// `stop_mask` (flags |= LA3DM_RAY_HIT; bit c of the mask = class c).  The class of a row is the state of the COVERING
    /// LEAF of its voxel — after prune() the eight children of a collapsed group read PRUNED and the answer lives in an
    /// ancestor — or LA3DM_RAY_MISSING where the block does not exist.  out (include/la3dm_hip.h): the last row, the number
    /// of rows and the rows per class.  A device-resident map answers from the device pool (no mirror refresh); a
    /// host-mode map runs this very loop over its own RayCaster.  Both give the same bits.
    void raycast_many(const float *rays6, size_t n, uint32_t stop_mask, uint32_t max_steps, const la3dm_raycast_out &out) const;
    /// Dense region reads (contract: include/la3dm_hip.h, la3dm_devmap_box_host).  The region is the nx x ny x nz voxels of
    /// the finest-layer lattice whose voxel (0, 0, 0) holds `lo` the way the RayCaster resolves its start point
    /// (block_to_hash_key + Block::get_index); voxel (i, j, k) is the one i, j, k cells further along x, y, z, across
    /// block borders, in integer arithmetic.  box: per voxel, index (i * ny + j) * nz + k, the state of the COVERING LEAF
    /// (FREE 0, OCCUPIED 1, UNKNOWN 2, LA3DM_RAY_MISSING where the block does not exist, 4 = UNCERTAIN on a BGK-LV map),
    /// its layer (255: missing) and its node values (the default node: missing).  columns: per column (i, j), index
    /// i * ny + j, the voxels per class FREE, OCCUPIED, UNKNOWN (+ UNCERTAIN), MISSING over k, and the smallest / largest k
    /// whose class is OCCUPIED (-1: none) — the reduction of box's cls along z, computed without the box.  `info` (may
    /// be null): the anchor's block key and cell and the centre of voxel (0, 0, 0) (Block::get_point).  Bad arguments throw
    /// std::invalid_argument.  A device-resident map answers from the device pool (no mirror refresh); a host-mode map
    /// loops over its host blocks: that form is the definition, and both give the same bits.
    void box(const float *lo3, const uint32_t *dims3, const la3dm_box_out &out, la3dm_region_info *info = nullptr) const;
    void columns(const float *lo3, const uint32_t *dims3, const la3dm_columns_out &out, la3dm_region_info *info = nullptr) const;
    /// Distance field of box's region (contract: include/la3dm_hip.h, la3dm_devmap_distance_host): per voxel the squared
    /// Euclidean distance, an integer in voxel units, to the nearest voxel of the region whose class (box's cls) has its bit
    /// in `obstacle_mask` — d2, LA3DM_DF_FAR beyond radius^2 — and dist = sqrtf(d2) * resolution, +inf for FAR.  Obstacles
    /// outside the region are not seen (pad the region by `radius`); the distance inside obstacles is the call with the
    /// complementary mask.  Bad arguments throw std::invalid_argument.  A device-resident map runs the transform on the
    /// device pool (no mirror refresh); a host-mode map runs an exact separable transform (windowed min-plus) over the host
    /// form of box's classes: that form is the definition, and both give the same bits.
    void distance_field(const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask, uint32_t radius,
                        const la3dm_distance_out &out, la3dm_region_info *info = nullptr) const;
    /// Frontier of box's region (contract: include/la3dm_hip.h, la3dm_devmap_frontier_host): the voxels whose class (box's
    /// cls) is in `open_mask` and that have at least `min_neighbours` neighbours (connectivity 6, 18 or 26) whose class is in
    /// `unknown_mask`, neighbours one step outside the region included.  *n_found = their number; out.index = the flat
    /// indices of the first min(*n_found, cap) in ascending order, out.nbrs = their scores, out.score (dense, optional) = the
    /// score of every voxel.  cap = 0 only counts.  Bad arguments throw std::invalid_argument.  A device-resident map runs
    /// the query on the device pool (no mirror refresh); a host-mode map loops over the classes of the padded box: that form
    /// is the definition, and both give the same integers.
    void frontier(const float *lo3, const uint32_t *dims3, uint32_t open_mask, uint32_t unknown_mask, uint32_t connectivity,
                  uint32_t min_neighbours, uint64_t cap, const la3dm_frontier_out &out, uint64_t *n_found,
                  la3dm_region_info *info = nullptr) const;
    /// Footing over box's region (contract: include/la3dm_hip.h, la3dm_devmap_footing_host): where a ground robot can stand —
    /// the voxels with a class of p->support_mask directly below and p->headroom voxels of p->clear_mask classes from the
    /// voxel upwards, round which every cell of a disc of p->radius voxels is clear above p->step voxels and at least
    /// p->min_support cells have such a standing place within p->step voxels of height.  Classes past the region's faces
    /// are read from the map.  *n_found = their number; out.index = the flat indices of the first min(*n_found, cap) in
    /// ascending order; out.levels / lowest / highest (dense, per column, optional) = the foot voxels of the column and
    /// their smallest / largest k; stats (may be null) = the voxels that pass each condition and the cells of the disc.
    /// Bad arguments throw std::invalid_argument.  A device-resident map runs the query on the device pool (no mirror
    /// refresh); a host-mode map reads the classes of the padded box and calls host/footing_cells.h: that form is the
    /// definition, and both give the same integers.
    void footing(const float *lo3, const uint32_t *dims3, const la3dm_footing_params *p, uint64_t cap, const la3dm_footing_out &out,
                 uint64_t *n_found, la3dm_footing_stats *stats = nullptr, la3dm_region_info *info = nullptr) const;
    /// Surface over box's region (contract: include/la3dm_hip.h, la3dm_devmap_surface_host): the exposed faces and integer
    /// normals of its solid voxels.  A voxel with a class in p->solid_mask has face d (0: -x, 1: +x, 2: -y, 3: +y, 4: -z,
    /// 5: +z) when its neighbour in that direction has a class in p->open_mask; classes past the region's faces are read
    /// from the map.  *n_found = the voxels with a face; out.index / faces / normal = the flat indices of the first
    /// min(*n_found, cap) in ascending order, their face masks and their normals (the sum of the face vectors of every voxel
    /// within p->smooth voxels, three int16, possibly zero); out.dense_faces (optional) = the face mask of every voxel;
    /// stats (may be null) = the solid voxels, the surface voxels and the faces per direction.  Bad arguments throw
    /// std::invalid_argument.  A device-resident map runs the query on the device pool (no mirror refresh); a host-mode map
    /// reads the classes of the padded box and calls host/surface_cells.h: that form is the definition, and both give the
    /// same integers.
    void surface(const float *lo3, const uint32_t *dims3, const la3dm_surface_params *p, uint64_t cap, const la3dm_surface_out &out,
                 uint64_t *n_found, la3dm_surface_stats *stats = nullptr, la3dm_region_info *info = nullptr) const;
    /// Gain of candidate viewpoints over box's region (contract: include/la3dm_hip.h, la3dm_devmap_gain_host): the n * m
    /// segments origins[v] -> origins[v] + offsets[d] are walked exactly as raycast_many(stop_mask, max_steps) walks them;
    /// every row whose class is in `count_mask` and whose voxel lies in the region sets that voxel's bit in viewpoint v's
    /// set.  out.gain[v] = the number of DISTINCT voxels marked — the expected information gain when count_mask selects the
    /// unobserved classes — out.seen the sets, out.started / out.hits the rays per viewpoint that produced a row / ended on a
    /// stop row.  Bad arguments throw std::invalid_argument.  A device-resident map runs the query on the device pool (no
    /// mirror refresh); a host-mode map loops its own RayCaster: that form is the definition, and both give the same
    /// integers.
    void gain(const float *lo3, const uint32_t *dims3, const float *origins3, uint32_t n, const float *offsets3, uint32_t m,
              uint32_t count_mask, uint32_t stop_mask, uint32_t max_steps, const la3dm_gain_out &out,
              la3dm_region_info *info = nullptr) const;
    /// Likelihood-field scoring of one scan under many poses (contract: include/la3dm_hip.h, la3dm_devmap_score_poses_host):
    /// every point of points3 (sensor frame) is moved by every pose of poses12 (row-major 3 x 4 [R | t], fp32, op by op as
    /// the contract spells it), its voxel resolved as search resolves it, and d2 = distance_field(lo, dims, obstacle_mask,
    /// radius) gathered there.  out.sum_d2[p] = the sum of the finite d2 of pose p; out.counts[5 p + c] = its pairs of class
    /// HIT (d2 = 0), NEAR (finite), FAR, OUTSIDE (the voxel is not in the region), INVALID (a coordinate the lattice cannot
    /// hold).  Bad arguments throw std::invalid_argument.  A device-resident map runs the query on the device pool (no
    /// mirror refresh); a host-mode map runs its own distance_field and a plain loop: that form is the definition, and both
    /// give the same integers.
    void score_poses(const float *lo3, const uint32_t *dims3, const float *points3, uint32_t n_points, const float *poses12,
                     uint32_t n_poses, uint32_t obstacle_mask, uint32_t radius, const la3dm_score_out &out,
                     la3dm_region_info *info = nullptr) const;
    /// Which obstacle is the nearest (contract: include/la3dm_hip.h, la3dm_devmap_nearest_host): per voxel of box's region
    /// out.index = the flat index of the nearest voxel of the region whose class is in obstacle_mask — the smallest flat
    /// index among equals, LA3DM_NEAREST_NONE beyond `radius` (1 .. 255) voxels — and out.d2 = distance_field's d2; either
    /// may be null, not both.  Bad arguments throw std::invalid_argument.  A device-resident map runs the query on the
    /// device pool (no mirror refresh); a host-mode map runs distance_field's three stages with their argmins
    /// (host/nearest_lines.h): that form is the definition, and both give the same integers.
    void nearest(const float *lo3, const uint32_t *dims3, uint32_t obstacle_mask, uint32_t radius, const la3dm_nearest_out &out,
                 la3dm_region_info *info = nullptr) const;
    /// nearest per point of a cloud — the correspondences of an ICP step: every point of points3 is moved by pose12 (row-major
    /// 3 x 4 [R | t], score_poses' transform; null: the points as they are, no arithmetic), its voxel resolved as search
    /// resolves it; out.cls = score_poses' class of the point, out.voxel = the voxel's flat index, out.index = nearest's
    /// index there, out.d2 = the squared distance (NONE / FAR where the contract says so).  Every array may be null, not all.
    void nearest_points(const float *lo3, const uint32_t *dims3, const float *points3, uint32_t n_points, const float *pose12,
                        uint32_t obstacle_mask, uint32_t radius, const la3dm_nearest_points_out &out, la3dm_region_info *info = nullptr) const;
    /// Cost and clearance of many candidate trajectories (contract: include/la3dm_hip.h, la3dm_devmap_score_paths_host):
    /// every path of ways3 (n_paths x n_way x 3 floats, world frame) is walked voxel by voxel from waypoint to waypoint
    /// through box's region against d2 = distance_field(lo, dims, obstacle_mask, max(1, clearance, soft_radius)); the walk
    /// stops where it leaves the region (LA3DM_PATH_LEFT) or meets a voxel within `clearance` of an obstacle
    /// (LA3DM_PATH_BLOCKED), and after max_steps moves (LA3DM_PATH_TRUNCATED).  out.cost[p] = travel's cost of the walk up to
    /// the stop; steps, stop, min_d2, ways (waypoints reached) and flags are optional.  Bad arguments throw
    /// std::invalid_argument.  A device-resident map runs the query on the device pool (no mirror refresh); a host-mode
    /// map runs its own distance_field and a plain loop: that form is the definition, and both give the same integers.
    void score_paths(const float *lo3, const uint32_t *dims3, const float *ways3, uint32_t n_paths, uint32_t n_way,
                     const la3dm_paths_params *params, const la3dm_paths_out &out, la3dm_region_info *info = nullptr) const;
    /// Reach over box's region (contract: include/la3dm_hip.h, la3dm_devmap_reach_host): steps[v] = the least number of
    /// moves (connectivity 6, 18 or 26) from any seed to v through passable voxels of the region — class (box's cls) in
    /// `pass_mask` and, with clearance > 0, distance_field(obstacle_mask, radius = clearance) FAR — LA3DM_REACH_NONE where
    /// there is no such walk of at most max_steps moves.  seeds / targets are flat indices; out.target_steps = the steps at
    /// the targets; stats (may be null) = seeded and reached voxels and the largest finite step.  Diagonal moves are not
    /// tested for corner cutting.  Bad arguments throw std::invalid_argument.  A device-resident map runs a level-per-launch
    /// wave on the device pool (no mirror refresh); a host-mode map runs a queue BFS over box's classes and its own distance
    /// transform: that form is the definition, and both give the same integers.
    void reach(const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds, uint32_t pass_mask,
               uint32_t obstacle_mask, uint32_t clearance, uint32_t connectivity, uint32_t max_steps, const uint32_t *targets,
               uint32_t n_targets, const la3dm_reach_out &out, la3dm_reach_stats *stats = nullptr,
               la3dm_region_info *info = nullptr) const;
    /// Travel over box's region (contract: include/la3dm_hip.h, la3dm_devmap_travel_host): cost[v] = the least path cost
    /// from any seed to v through passable voxels — class in p.pass_mask and farther than p.clearance voxels from every
    /// voxel with a class in p.obstacle_mask — where a move costs p.move_cost by its number of non-zero components plus the
    /// entered voxel's penalty, which falls from p.penalty next to an obstacle to 0 at p.soft_radius; LA3DM_TRAVEL_NONE
    /// where no walk of at most p.max_cost exists.  out.parent (may be null) = the code of the offset to the voxel a
    /// least-cost walk came from, 13 at a seed, 255 where unreached; out.target_cost = the costs at the targets; stats (may
    /// be null) = seeded and reached voxels, the largest finite cost, and the device form's diagnostics.  Bad arguments
    /// throw std::invalid_argument.  A device-resident map relaxes bricks of the region on the device pool (no mirror
    /// refresh); a host-mode map runs Dijkstra over box's classes and its own distance transform: that form is the
    /// definition, and both give the same integers.
    void travel(const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds, const la3dm_travel_params &p,
                const uint32_t *targets, uint32_t n_targets, const la3dm_travel_out &out, la3dm_travel_stats *stats = nullptr,
                la3dm_region_info *info = nullptr) const;
    /// Drive over box's region (contract: include/la3dm_hip.h, la3dm_devmap_drive_host): cost[v] = the least cost of a
    /// ground route from any seed to v over the MEMBER voxels — those of the list p.members or, with p.footing set, the
    /// voxels footing(lo, dims, *p.footing) lists — by moves to one of the 4 or 8 horizontal neighbours that climb or
    /// drop at most p.step voxels and cost p.move_cost plus p.climb_up / p.climb_down per voxel of height;
    /// LA3DM_DRIVE_NONE for a non-member and where no walk of at most p.max_cost exists.  A seed or target stands for the
    /// highest member at most p.snap voxels below it.  out.parent (may be null) = the code of the offset to the member a
    /// least-cost walk came from, 40 at a seed, 255 where unreached; out.of_member = the cost per list entry;
    /// out.target_cost / out.target_index = the cost at the targets' members and those members; stats (may be null) = the
    /// members, the seeded and reached ones, the largest finite cost, and the device form's diagnostics.  Bad arguments
    /// throw std::invalid_argument.  A device-resident map relaxes bricks of the region on the device (no mirror refresh;
    /// in footing mode footing's kernels feed it without a list); a host-mode map runs its own footing and
    /// host/drive_cells.h: that form is the definition, and both give the same integers.
    void drive(const float *lo3, const uint32_t *dims3, const uint32_t *seeds, uint32_t n_seeds, const la3dm_drive_params *p,
               const uint32_t *targets, uint32_t n_targets, const la3dm_drive_out *out, la3dm_drive_stats *stats = nullptr,
               la3dm_region_info *info = nullptr) const;
    /// Clusters over box's region (contract: include/la3dm_hip.h, la3dm_devmap_clusters_host): the maximal sets of members
    /// — voxels with a class in p.member_mask, all of them or those of the list p.members — connected under p.connectivity
    /// inside tiles of p.tile voxels (0: untiled); those with fewer than p.min_size members are dropped, the others
    /// numbered in ascending order of their smallest flat index.  out (may be null, and so may each array) = the dense
    /// label, the label per list entry and, for the first p.cap clusters, first, size, bounding box, coordinate sums and
    /// rep, the member nearest the rounded centroid; *n_found = the number of kept clusters.  Bad arguments throw
    /// std::invalid_argument.  A device-resident map relaxes bricks of the region on the device pool (no mirror
    /// refresh); a host-mode map flood-fills box's classes: that form is the definition, and both give the same integers.
    void clusters(const float *lo3, const uint32_t *dims3, const la3dm_clusters_params &p, const la3dm_clusters_out *out,
                  uint32_t *n_found = nullptr, la3dm_clusters_stats *stats = nullptr, la3dm_region_info *info = nullptr) const;
    /// Save and load (stream layout and contract: include/la3dm_hip.h, la3dm_devmap_pack_host): the map as the compact stream
    /// of its covering leaves — block keys, one mask bit per node, and state, A, B of the leaves; not the last scan's training
    /// data, the statistics, the options or the shard configuration.  pack() of a device-resident map compacts the pool on
    /// the GPU before it crosses PCIe (blocks in pool slot order; no mirror refresh); a host-mode map, device = -1 included,
    /// writes the same stream from its blocks (ascending key).  unpack() loads a stream of either writer into an EMPTY map
    /// of the same class, block_depth, resolution and default node (the other parameters are informational: a loaded map may
    /// be continued with another ell): every node that is not a leaf becomes (default values, PRUNED under a leaf, UNKNOWN
    /// above).  A device-resident map expands the stream on the GPU; its mirror is emptied and marked stale.  The stream is
    /// validated before anything is touched; a refusal throws std::runtime_error and leaves the map as it was.  save() writes
    /// pack() to path + ".tmp" and renames it to path; load() reads the file and calls unpack().
    std::vector<uint8_t> pack() const;
    uint64_t packed_size() const;   ///< pack().size(); on a device-resident map without the gather and the copy
    void unpack(const void *stream, size_t size);
    void save(const std::string &path) const;
    void load(const std::string &path);
    /// Merge (contract: include/la3dm_hip.h, la3dm_devmap_merge_host): a stream — or another map of the same class, packed
    /// first — fused into this map, which may hold blocks.  Per finest cell of every block the stream names: kept where the
    /// incoming leaf is the default node, copied where this map's is, else the evidence sums added and the state re-derived;
    /// then the block is pruned and written in unpack's canonical form.  BGKOctoMap and BGKLOctoMap only.  A
    /// device-resident map fuses on the GPU pool (mirror marked stale), a host-mode map runs host/merge_block.h over its
    /// blocks: the same bytes.  The stream is validated before anything is touched; a refusal throws std::runtime_error.
    la3dm_merge_stats merge(const void *stream, size_t size);
    la3dm_merge_stats merge(const BGKOctoMap &other);
    la3dm_merge_stats merge_file(const std::string &path);
    /// Diff (contract: include/la3dm_hip.h, la3dm_devmap_diff_host), all four classes: the finest cells whose class — or,
    /// with p.value_mask, whose A or B — differs between this map (now) and a stream, or another map of the same class
    /// packed first (then): the blocks the stream names in stream order, with p.map_only then the map's other blocks in
    /// pack()'s order; the selected cells as a list (the first min(*n_found, cap) entries; cap 0 with out null only counts)
    /// and the 5 x 5 pair counts in stats (may be null).  The map is not changed: a device-resident map compares on the GPU
    /// pool (no mirror refresh, the mirror not marked stale), a host-mode map runs host/diff_block.h over its blocks — the
    /// same list and counts.  A refusal throws std::runtime_error before anything is written.
    void diff(const void *stream, size_t size, const la3dm_diff_params &p, uint64_t cap, const la3dm_diff_out *out, uint64_t *n_found,
              la3dm_diff_stats *stats = nullptr) const;
    void diff(const BGKOctoMap &then, const la3dm_diff_params &p, uint64_t cap, const la3dm_diff_out *out, uint64_t *n_found,
              la3dm_diff_stats *stats = nullptr) const;
    void diff_file(const std::string &path, const la3dm_diff_params &p, uint64_t cap, const la3dm_diff_out *out, uint64_t *n_found,
                   la3dm_diff_stats *stats = nullptr) const;
    /// The map as a rolling window (contract: include/la3dm_hip.h, la3dm_devmap_pack_region_host), all four classes.  The
    /// region is the box of blocks from the block that holds lo3 to the block that holds hi3 (block_to_hash_key, on the
    /// host; a box whose first block lies past its second on an axis is refused); inside selects the blocks in the box, !inside every other block.  pack_region: the
    /// stream of the selected blocks only, the map unchanged (device-resident: compacted on the GPU in pool slot order,
    /// no mirror refresh; host-mode: ascending key).  erase_region: the selected blocks leave the map (device-resident: the
    /// pool compacted by the hole / tail rule and the table rebuilt on the GPU, the blocks dropped from the mirror, which is
    /// marked stale; host-mode: erased from the container).  evict: pack_region, then erase_region — the stream is complete on
    /// the host, and for evict_file written to path + ".tmp" and renamed to path, before the first block is removed; a
    /// failure of that step throws and leaves the map as it was.  Null points and refusals throw.
    std::vector<uint8_t> pack_region(const float *lo3, const float *hi3, bool inside) const;
    la3dm_erase_stats erase_region(const float *lo3, const float *hi3, bool inside);
    std::vector<uint8_t> evict(const float *lo3, const float *hi3, bool inside, la3dm_erase_stats *stats = nullptr);
    la3dm_erase_stats evict_file(const std::string &path, const float *lo3, const float *hi3, bool inside);

protected:
    std::vector<uint8_t> pack_blocks(const la3dm_region_blocks::Box *box, const char *who) const;
    la3dm_region_blocks::Box region_box(const float *lo3, const float *hi3, bool inside, const char *who) const;

public:
    /// how often the host mirror was refreshed from the device pool (sync_mirror that found it stale)
    uint64_t mirror_syncs() const { return mirror_sync_count; }
    size_t block_count() const {
        bind();
        sync_mirror();
        return block_arr.size();
    }
    int get_variant() const { return variant; }

    /// Cube lists of the map = the publish loop of the static node (src/bgkoctomap/bgkoctomap_static_node.cpp:101-136)
    /// with MarkerArrayPub::insert_point3d / heightMapColor (include/common/markerarray_pub.h:21-147) minus ROS.
    /// `state` OCCUPIED: cells coloured by height between min_z and max_z (min_z == max_z: the map's bbox, as the node
    /// does); FREE: coloured by probability.  original_size false expands collapsed leaves (get_pruned_locs).
    /// level[i] = (int) log2(size / resolution) = the CUBE_LIST marker the cell goes to.  In device-resident mode the
    /// pool is scanned on the GPU (no mirror refresh).  Returns the number of cells.
    struct Cells {
        std::vector<float> xyz_size;  // 4 per cell
        std::vector<float> rgba;      // 4 per cell
        std::vector<int32_t> level;
    };
    size_t export_cells(State state, bool original_size, float min_z, float max_z, Cells &out) const;

protected:
    void get_training_data(const float *xyz, size_t n, size_t stride, const point3f &origin, float ds_resolution,
                           float free_resolution, float max_range);
    bool partition_and_pack(bool ungated);
    void refresh_pass(size_t p);
    void write_nodes(size_t p);

    // The reference keeps its map parameters in process-global statics (Block::resolution / size / key_loc_map,
    // OcTree::max_depth, every OcTreeNode threshold: bgkoctomap.cpp:31-56) and so do the node / block classes here.
    // Each map therefore remembers its own set and re-installs it (bind()) at the top of every public entry point, so
    // several maps with different variants, depths or resolutions can be alive in one process.  Like the reference the
    // maps of a process must be driven from one thread at a time, and a LeafIterator / RayCaster must be used up
    // before another map is touched.
    struct BoundStatics {
        float resolution, size;
        std::vector<point3f> key_loc_map;
        unsigned short max_depth;
        float sf2, ell, free_thresh, occupied_thresh, var_thresh, prior_A, prior_B, init_A, init_B, min_W;
        float noise, l, min_ivar, max_ivar, min_known_ivar;
        int variant;
        bool original_size;
    };
    BoundStatics mine;
    static const BGKOctoMap *bound;
    void capture_statics();

public:
    /// make this map's parameters the process-global ones (every public entry point does it; call it yourself before
    /// using the static helpers block_to_hash_key / hash_key_to_block / get_extended_block with a particular map in mind)
    void bind() const;

protected:

    float resolution;
    float block_size;
    unsigned short block_depth;
    mutable std::unordered_map<BlockHashKey, Block *> block_arr;
    la3dm_ctx *ctx;
    la3dm_devmap *dmap = nullptr;
    mutable bool mirror_dirty = false;
    mutable uint64_t mirror_sync_count = 0;
    /// checks of a region query in the contract's order (region_contract.h) + its anchor: global voxel index g0 of voxel
    /// (0, 0, 0), info
    void region_anchor(const float *lo3, const uint32_t *dims3, const la3dm_region::Query &q, bool has_mandatory, const char *who,
                       uint32_t g0[3], la3dm_region_info &info) const;
    /// leaf that covers global voxel (gx, gy, gz), null where the map has no block there
    const OcTreeNode *covering_leaf_at(uint32_t gx, uint32_t gy, uint32_t gz, BlockHashKey &have, const Block *&b, unsigned &d) const;
    la3dm_params create_params;   // what the context was created with (lut_xyz is re-pointed on use)
    GPParams ctor_gp;             // the variant-specific constructor arguments as given (the stream's header carries them)
    void create_context();        // la3dm_create + the device-resident pool from create_params and the current statics
    void reconfigure(float resolution, unsigned short depth);
    struct ShardCfg {
        uint32_t rank = 0, world = 1;
        la3dm_allgatherv_fn fn = nullptr;
        void *user = nullptr;
    } shard_cfg;   // what set_shard() installed (re-applied to the device map reconfigure() builds)

    // per-scan buffers (capacity reused across scans)
    std::vector<float> xy;               // training set: x,y,z,label
    std::vector<float> train_xyzy;       // grouped by training block
    std::vector<uint32_t> train_off;
    struct Pass {
        std::vector<BlockHashKey> keys;
        std::vector<Block *> blocks;
        std::vector<int32_t> nbr;
        std::vector<float> center;
        std::vector<uint32_t> leaf_off, leaf_key;
        std::vector<float> alpha, beta;
        std::vector<uint8_t> state;
    };
    std::vector<Pass> passes;
    std::vector<BlockHashKey> prune_list;  // test_blocks in list order (with repeats)
    uint32_t scan_flags;
    ScanStats stats;
    int variant;
    uint32_t train_max_n;
    uint64_t train_sum_n2;
    int run_scan(la3dm_bgk_scan *s, la3dm_bgk_counters *c);

    // ---- variant 3 (BGKLOctoMap): training samples keep their beam, training blocks hold segment rows ----
    void get_training_data_l(const float *xyz, size_t n, size_t stride, const point3f &origin, float ds_resolution,
                             float free_resolution, float max_range);
    void build_rows_l();
    std::vector<int32_t> l_ray_idx;     // per training sample: -1 = hit, else index into l_rays
    std::vector<float> l_rays;          // 6 floats per beam: origin -> hit shortened by free_resolution
    std::vector<uint32_t> train_src;    // training sample index of every CSR member
    std::vector<float> train_rows;      // 8 floats per row {x0,y0,z0,x1,y1,z1,label,0}
    std::vector<uint32_t> rows_off;     // CSR over training blocks

public:
    const std::vector<int32_t> &last_ray_index() const { return l_ray_idx; }
    const std::vector<float> &last_rays() const { return l_rays; }
};

/// BGKLOctoMap: block-level BGK whose free-space evidence are the beams themselves (line segments) instead of
/// down-sampled free points (reference include/bgkloctomap/bgkloctomap.h, src/bgkloctomap/bgkloctomap.cpp:31-57).
/// Same node type and constructor argument order as BGKOctoMap.
class BGKLOctoMap : public BGKOctoMap {
public:
    BGKLOctoMap() : BGKLOctoMap(0.1f, 4, 1.0, 1.0, 0.3f, 0.7f, 1.0f, 1.0f, 1.0f) {}
    BGKLOctoMap(float resolution, unsigned short block_depth, float sf2, float ell, float free_thresh, float occupied_thresh,
                float var_thresh, float prior_A, float prior_B, int device = 0)
        : BGKOctoMap(3, resolution, block_depth, sf2, ell, free_thresh, occupied_thresh, var_thresh, prior_A, prior_B, nullptr,
                     device) {}
};

/// BGKLVOctoMap: variance-aware BGK with free-space line segments and per-voxel inference
/// (reference include/bgklvoctomap/bgklvoctomap.h; constructor order src/bgklvoctomap/bgklvoctomap.cpp:33-43).
/// Every block of the scan's bounding box is allocated, every base-resolution leaf is inferred on the GPU.
class BGKLVOctoMap : public BGKOctoMap {
public:
    BGKLVOctoMap() : BGKLVOctoMap(0.1f, 4, 1.0, 1.0, 0.3f, 0.7f, 1.0f, 1.0f, 1.0f, true, 0.1f) {}
    BGKLVOctoMap(float resolution, unsigned short block_depth, float sf2, float ell, float free_thresh, float occupied_thresh,
                 float var_thresh, float prior_A, float prior_B, bool original_size, float min_W, int device = 0);
    void insert_pointcloud(const float *xyz, size_t n, size_t stride, const point3f &origin, float ds_resolution,
                           float free_res = 2.0f, float max_range = -1) override;
    using BGKOctoMap::insert_pointcloud;

    struct LVStats {
        uint64_t n_hits = 0, n_rays = 0, n_samples = 0, n_bbox_blocks = 0, n_packed_blocks = 0, n_info_blocks = 0,
                 voxels = 0, voxel_updates = 0;
        double t_frontend = 0, t_partition = 0, t_device = 0, t_commit = 0, t_total = 0;
    };
    const LVStats &lv_stats() const { return lvst; }
    /// training samples (x, y, z, ray index or -1) and segments (6 floats) of the last scan
    const std::vector<float> &lv_samples() const {
        fetch_device_training();
        return samples;
    }
    const std::vector<float> &lv_rays() const {
        fetch_device_training();
        return rays6;
    }
    /// split form used by the benchmark: prepare_lv packs (returns false if nothing to do), packed_lv exposes the
    /// device-call arguments (host pointers), commit_lv writes the nodes and prunes (the split form runs the first visit
    /// of every block only; insert_pointcloud also runs the repeats of the float-stepped candidate list)
    bool prepare_lv(const float *xyz, size_t n, size_t stride, const point3f &origin, float ds_resolution, float free_res,
                    float max_range);
    la3dm_lv_scan packed_lv();
    void commit_lv();
    void finish_lv();

private:
    void training_data_lv(const float *xyz, size_t n, size_t stride, const point3f &origin, float ds_resolution,
                          float free_resolution, float max_range);
    void fetch_device_training() const;   // device-resident mode: samples / segments of the last scan come from the GPU on demand
    mutable bool device_training_stale = false;
    mutable std::vector<float> samples;   // x, y, z, ray
    std::vector<float> sorted;    // x, y, z, original index bits
    std::vector<float> rays8;
    mutable std::vector<float> rays6;
    std::vector<uint32_t> cell_off;
    int32_t cell_min[3], cell_dim[3];
    std::vector<float> lv_center, lv_alpha, lv_beta;
    std::vector<int32_t> lv_cell0;
    std::vector<uint8_t> lv_state;
    std::vector<Block *> lv_blocks;
    // A block index the float-stepped candidate loop produces k times is visited k times by the reference (the same
    // samples, serially): lv_mult[b] = k; pass p re-packs and re-runs the blocks with k > p (lv_all_* keep the full
    // list, lv_blocks / lv_center / lv_cell0 hold the current pass), the prune follows the last pass.
    std::vector<Block *> lv_all_blocks;
    std::vector<float> lv_all_center;
    std::vector<int32_t> lv_all_cell0;
    std::vector<uint32_t> lv_mult;
    std::vector<uint8_t> lv_info;   // per entry of lv_all_blocks: some voxel had samples in its box (any pass)
    std::vector<uint32_t> lv_pass_index;  // lv_blocks[i] == lv_all_blocks[lv_pass_index[i]]
    uint32_t lv_max_mult = 0;
    bool select_pass_lv(uint32_t pass);
    LVStats lvst;
};

/// GPOctoMap: same skeleton, GP regression per block + BCM fusion (reference include/gpoctomap/gpoctomap.h).
/// Constructor argument order as the reference (src/gpoctomap/gpoctomap.cpp:23-25).
class GPOctoMap : public BGKOctoMap {
public:
    GPOctoMap() : GPOctoMap(0.1f, 4, 1.0, 1.0, 0.01, 100, 0.001f, 1000.0f, 0.02f, 0.3f, 0.7f) {}
    GPOctoMap(float resolution, unsigned short block_depth, float sf2, float ell, float noise, float l, float min_var,
              float max_var, float max_known_var, float free_thresh, float occupied_thresh, int device = 0);
};

}  // namespace la3dm
#endif
