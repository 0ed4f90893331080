// la3dm_oracle.cpp — CPU restatement of la3dm's per-scan BGK occupancy-inference path.
//
// *** TEST INFRASTRUCTURE ONLY. ***  This file is the parity oracle for the HIP
// implementation in la3dm_amd/csrc.  Only tests/, __graft_entry__.smoke() and
// bench.py's cpu_baseline leg may load it.  Nothing in the product path links,
// imports or calls it.
//
// It restates, in strict fp32 (build with -ffp-contract=off, no -ffast-math), the
// reference algorithm of RobustFieldAutonomyLab/la3dm.  Every function cites the
// reference file:line it follows (paths relative to the reference checkout).
//
// PARITY PINNING STATUS
//  * Block hashing, voxel LUT, leaf enumeration order, Occupancy::update, prune and
//    the R-tree closed-box inclusion rule are PINNED: tests compare this file with
//    the reference's own std-only sources compiled in place (oracle/_ref, built by
//    oracle/Makefile) and with golden vectors captured from them (tests/golden).
//  * The kernel arithmetic (include/bgkoctomap/bgkinference.h) runs on Eigen and the
//    front-end filter on pcl::VoxelGrid.  Neither library is vendored by the
//    reference (Eigen arrives through PCL; both unpinned, README targets ROS
//    Noetic => Eigen 3.3.7 / PCL 1.10) and neither is installed here, and the
//    reference ships no tests or golden vectors.  For those two boundaries this
//    oracle restates the published algorithms and is  **parity unpinned**.
//  * The ORDER in which a block's training points reach Ks*y differs by design: ascending index here, R-tree
//    traversal order in the reference.  tests/test_oracle.py measures the effect with the reference's real tree
//    (rtree.h in oracle/_ref): the fused posterior moves by <= 2e-7 (tolerance 1e-5) — the order only permutes fp32 sums.
//
// Conventions: all arithmetic that the reference does in float is done in float
// here, every float->double promotion the reference performs is reproduced.

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <queue>
#include <unordered_map>
#include <utility>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

namespace {

// include/bgkoctomap/bgkoctree_node.h:10-12
enum : uint8_t { ST_FREE = 0, ST_OCCUPIED = 1, ST_UNKNOWN = 2, ST_PRUNED = 3 };

struct Params {
    float resolution;
    int block_depth;
    float sf2, ell;
    float free_thresh, occupied_thresh, var_thresh;
    float prior_A, prior_B;
    float block_size;  // src/bgkoctomap/bgkoctomap.cpp:41
    // GPOctoMap (variant 1): src/gpoctomap/gpoctomap.cpp:23-46
    int variant;       // 0 = BGKOctoMap, 1 = GPOctoMap
    float noise, l, min_ivar, max_ivar, min_known_ivar;
};

// include/bgkoctomap/bgkoctree_node.h:76-81 (classified, m_A, m_B, state)
struct Node {
    uint8_t classified;
    float A, B;
    uint8_t state;
};

struct V3 {
    float x, y, z;
};

// ---------------------------------------------------------------------------
// Node: src/bgkoctomap/bgkoctree_node.cpp:27-44, include/.../bgkoctree_node.h:60
// ---------------------------------------------------------------------------
inline float node_var(const Node &n) {
    // (m_A * m_B) / ((m_A + m_B) * (m_A + m_B) * (m_A + m_B + 1.0f))
    float s = n.A + n.B;
    float num = n.A * n.B;
    float den = (s * s) * (s + 1.0f);
    return num / den;
}
inline float node_prob(const Node &n) { return n.A / (n.A + n.B); }

inline void node_update(const Params &p, Node &n, float ybar, float kbar) {
    n.classified = 1;
    n.A += ybar;
    n.B += kbar - ybar;
    float var = node_var(n);
    if (var > p.var_thresh)
        n.state = ST_UNKNOWN;
    else {
        float pr = node_prob(n);
        n.state = pr > p.occupied_thresh ? ST_OCCUPIED : (pr < p.free_thresh ? ST_FREE : ST_UNKNOWN);
    }
}

// GP node (variant 1): A holds m_ivar, B holds ivar.  src/gpoctomap/gpoctree_node.cpp:31-49.
// exp() is evaluated in double; `ivar += 1.0 / new_var - sf2` is a double expression.
inline float gp_node_prob(const Params &p, const Node &n) {
    return 1.0f / (1.0f + (float)exp((double)(-p.l * n.A / p.max_ivar)));
}
inline void gp_node_update(const Params &p, Node &n, float new_m, float new_var) {
    n.classified = 1;
    n.B = (float)((double)n.B + (1.0 / (double)new_var - (double)p.sf2));
    n.A += new_m / new_var;
    if (n.B < p.min_known_ivar)
        n.state = ST_UNKNOWN;
    else {
        n.B = n.B > p.max_ivar ? p.max_ivar : n.B;
        float pr = gp_node_prob(p, n);
        n.state = pr > p.occupied_thresh ? ST_OCCUPIED : (pr < p.free_thresh ? ST_FREE : ST_UNKNOWN);
    }
}

// ---------------------------------------------------------------------------
// Block hashing: src/bgkoctomap/bgkblock.cpp:73-101
// ---------------------------------------------------------------------------
inline int64_t block_to_hash_key(const Params &p, float x, float y, float z) {
    double s = (double)p.block_size;
    return (int64_t(x / s + 524288.5) << 40) | (int64_t(y / s + 524288.5) << 20) | (int64_t(z / s + 524288.5));
}
inline V3 hash_key_to_block(const Params &p, int64_t key) {
    V3 c;
    c.x = ((key >> 40) - 524288) * p.block_size;  // int64 -> float, float multiply
    c.y = (((key >> 20) & 0xFFFFF) - 524288) * p.block_size;
    c.z = ((key & 0xFFFFF) - 524288) * p.block_size;
    return c;
}
// order: self,+x,-x,+y,-y,+z,-z  (bgkblock.cpp:85-101 and 114-130)
inline void extended_block_from_center(const Params &p, V3 c, int64_t key0, int64_t out[7]) {
    out[0] = key0;
    for (int i = 0; i < 6; ++i) {
        float ex = (i / 2 == 0) ? (i % 2 == 0 ? p.block_size : -p.block_size) : 0;
        float ey = (i / 2 == 1) ? (i % 2 == 0 ? p.block_size : -p.block_size) : 0;
        float ez = (i / 2 == 2) ? (i % 2 == 0 ? p.block_size : -p.block_size) : 0;
        out[i + 1] = block_to_hash_key(p, ex + c.x, ey + c.y, ez + c.z);
    }
}

// ---------------------------------------------------------------------------
// Voxel LUT: src/bgkoctomap/bgkblock.cpp:7-32 (BFS, f64 intermediates)
// lut[depth][index]
// ---------------------------------------------------------------------------
std::vector<std::vector<V3>> build_lut(float resolution, int max_depth) {
    std::vector<std::vector<V3>> lut(max_depth);
    std::queue<V3> q;
    q.push(V3{0.0f, 0.0f, 0.0f});
    for (int depth = 0; depth < max_depth; ++depth) {
        size_t q_size = q.size();
        float half_size = (float)(resolution * pow(2, max_depth - depth - 1) * 0.5f);
        for (size_t index = 0; index < q_size; ++index) {
            V3 center = q.front();
            q.pop();
            lut[depth].push_back(center);
            if (depth == max_depth - 1) continue;
            for (int i = 0; i < 8; ++i) {
                float x = (float)(center.x + half_size * (i & 4 ? 0.5 : -0.5));
                float y = (float)(center.y + half_size * (i & 2 ? 0.5 : -0.5));
                float z = (float)(center.z + half_size * (i & 1 ? 0.5 : -0.5));
                q.push(V3{x, y, z});
            }
        }
    }
    return lut;
}

// ---------------------------------------------------------------------------
// OcTree / Block: src/bgkoctomap/bgkoctree.cpp:18-27,72-82,101-148,
//                 include/bgkoctomap/bgkoctree.h:62-147
// ---------------------------------------------------------------------------
struct Block {
    V3 center;
    std::vector<std::vector<Node>> layer;  // empty vector == deleted layer
    std::vector<char> alive;
};

Block *block_new(const Params &p, V3 center) {
    Block *b = new Block;
    b->center = center;
    b->layer.resize(p.block_depth);
    b->alive.assign(p.block_depth, 1);
    size_t n = 1;
    for (int d = 0; d < p.block_depth; ++d, n *= 8) {
        Node def{0, p.prior_A, p.prior_B, ST_UNKNOWN};  // bgkoctree_node.h:34
        if (p.variant == 1) def = Node{0, 0.0f, p.min_ivar, ST_UNKNOWN};  // gpoctree_node.h:34
        b->layer[d].assign(n, def);
    }
    return b;
}

inline bool is_leaf(const Params &p, const Block &b, int depth, int index) {
    if (b.alive[depth] && b.layer[depth][index].state != ST_PRUNED) {
        if (depth + 1 < p.block_depth) {
            if (!b.alive[depth + 1] || b.layer[depth + 1][index * 8].state == ST_PRUNED) return true;
        } else
            return true;
    }
    return false;
}

// Leaf order of OcTree::LeafIterator: explicit stack, children pushed 0..7, popped 7..0.
void enumerate_leaves(const Params &p, const Block &b, std::vector<int> &keys) {
    keys.clear();
    std::vector<std::pair<int, int>> st;
    st.emplace_back(0, 0);
    while (!st.empty()) {
        auto top = st.back();
        if (is_leaf(p, b, top.first, top.second)) {
            keys.push_back((top.first << 16) + top.second);
            st.pop_back();
        } else {
            st.pop_back();
            // single_inc(): expands unconditionally; guard the array bound the
            // reference never reaches (a non-leaf at the last depth is PRUNED and
            // is only reachable below a collapsed parent, which is a leaf).
            if (top.first + 1 < p.block_depth)
                for (int i = 0; i < 8; ++i) st.emplace_back(top.first + 1, top.second * 8 + i);
        }
    }
}

bool block_prune(const Params &p, Block &b) {
    bool pruned = false;
    for (int depth = p.block_depth - 1; depth > 0; --depth) {
        if (!b.alive[depth]) continue;
        std::vector<Node> &layer = b.layer[depth];
        std::vector<Node> &parent = b.layer[depth - 1];
        bool empty_layer = true;
        size_t n = layer.size();
        for (size_t index = 0; index < n; index += 8) {
            uint8_t state = layer[index].state;
            if (state == ST_UNKNOWN) {
                empty_layer = false;
                continue;
            }
            if (state == ST_PRUNED) continue;
            bool collapsible = true;
            for (int i = 1; i < 8; ++i)
                if (layer[index + i].state != state) collapsible = false;
            if (collapsible) {
                // Occupancy::operator= copies m_A, m_B, state but NOT classified
                // (bgkoctree_node.h:40-45)
                Node &par = parent[index / 8];
                par.A = layer[index].A;
                par.B = layer[index].B;
                par.state = layer[index].state;
                for (int i = 0; i < 8; ++i) layer[index + i].state = ST_PRUNED;
                pruned = true;
            } else
                empty_layer = false;
        }
        if (empty_layer) {
            b.alive[depth] = 0;
            std::vector<Node>().swap(b.layer[depth]);
        }
    }
    return pruned;
}

// ---------------------------------------------------------------------------
// Sparse kernel: include/bgkoctomap/bgkinference.h:113-126 (elementwise, fp32)
// r is the distance of the ell-prescaled coordinates.
//
// cos()/sin() of a float Eigen array are third-party (Eigen packet psin/pcos for
// full packets, libm for the tail; version and SIMD level unpinned).  They are
// restated as the CORRECTLY ROUNDED single-precision functions: the double libm
// value rounded once to float (differs from the exactly rounded result only when
// the true value lies within ~1e-16 relative of a rounding tie).  This is
// independent of which cosf/sinf variant glibc's ifunc selects on the host.
// ---------------------------------------------------------------------------
}  // namespace

// ---- sensitivity switches (tests/test_oracle.py::test_eigen_packet_trig_and_pcl_sort_order_move_p_by) ----------------
// The two boundaries where this oracle restates third-party code the image does not have can be restated in more than
// one plausible way.  Default (0, 0): correctly rounded sinf/cosf, ascending cloud index inside a voxel-grid cell — what
// the HIP path is bit-identical to.  Alternative (1, 1): what a ROS Noetic build of the reference most likely executes:
//   trig 1       Eigen 3.3.7's SSE packet psin / pcos (Eigen/src/Core/arch/SSE/MathFunctions.h, the Cephes-derived
//                sse_mathfun algorithm: scale by 4/pi, truncate, j = (j + 1) & ~1, three-term Cody-Waite reduction with
//                separate multiply and add, degree-3 polynomials in z = x^2, no FMA) for EVERY element (Eigen uses libm
//                for the last size % 4 elements of an array only);
//   grid sort 1  pcl::VoxelGrid's std::sort over {idx, cloud_point_index} with operator< on idx alone (PCL 1.10
//                voxel_grid.hpp): libstdc++'s introsort, so the order of the points inside a cell — the order of the fp32
//                centroid sum — is whatever that unstable sort leaves.
// Neither library is present, so the alternative is as unpinned as the default; the point of having both is to MEASURE
// how far the choice moves the occupancy probability.
int g_orc_trig_mode = 0;
int g_orc_grid_sort_mode = 0;
extern "C" void orc_set_modes(int trig, int grid_sort) {
    g_orc_trig_mode = trig;
    g_orc_grid_sort_mode = grid_sort;
}
// Summation switch of the BGK update loop (variant 0; since round 5 also BGKLOctoMap, see bgkl_predict, and BGKLVOctoMap,
// la3dm_oracle_lv.cpp), the counterpart of the device's order-free accumulate mode
// (la3dm_set_option "bgk_sum" 1, bgk_kernels.h bgk_predict_fuse_r):
//   0  the reference: fp32 running sums per neighbour in training-point order (bgkinference.h:76-78), one
//      Occupancy::update per neighbour with kbar > 0 (bgkoctomap.cpp:314-335) — default, what every parity test uses;
//   1  the same pairs and the same fp32 kernel values k and products k * y, summed in DOUBLE over all 7 neighbours, and
//      alpha + sum(k y), beta + (sum(k) - sum(k y)) rounded to fp32 once; update() runs when sum(k) > 0 (k >= 0, so that
//      is "some neighbour had kbar > 0").  A double sum of a few thousand fp32 terms does not depend on their order
//      (up to 2^-53 relative), so this is the value the reference's fp32 chains approximate.
int g_orc_sum_mode = 0;
extern "C" void orc_set_sum_mode(int mode) { g_orc_sum_mode = mode; }
// GP sensitivity switch (orc_set_gp_mode): 0 = the restatement every parity test uses (FMA chains in ascending k);
// 1 = an emulation of what an x86-64 / SSE2 (ROS Noetic) build of Eigen 3.3.7 most plausibly does — see gp_train_eigen.
int g_orc_gp_mode = 0;
extern "C" void orc_set_gp_mode(int mode) { g_orc_gp_mode = mode; }

namespace orc_eigen337 {
static inline float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static inline uint32_t to_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline void reduce(float &x, float &y, int32_t &j) {
    x = std::fabs(x);
    y = x * 1.27323954473516f;        // cephes_FOPI = 4 / pi
    j = (int32_t)y;                   // _mm_cvttps_epi32
    j = (j + 1) & ~1;
    y = (float)j;
}
static inline float poly(float x, bool use_sin) {
    const float z = x * x;
    if (!use_sin) {
        float y = 2.443315711809948E-005f;
        y = y * z + -1.388731625493765E-003f;   // pmadd without FMA: rounded multiply, rounded add
        y = y * z + 4.166664568298827E-002f;
        y = y * z;
        y = y * z;
        y = y - z * 0.5f;
        return y + 1.0f;
    }
    float y2 = -1.9515295891E-4f;
    y2 = y2 * z + 8.3321608736E-3f;
    y2 = y2 * z + -1.6666654611E-1f;
    y2 = y2 * z;
    y2 = y2 * x;
    return y2 + x;
}
float psin(float x0) {
    uint32_t sign = to_bits(x0) & 0x80000000u;
    float x, y;
    int32_t j;
    x = x0;
    reduce(x, y, j);
    sign ^= ((uint32_t)(j & 4)) << 29;
    const bool use_sin = (j & 2) == 0;
    x = x + y * -0.78515625f;
    x = x + y * -2.4187564849853515625e-4f;
    x = x + y * -3.77489497744594108e-8f;
    return from_bits(to_bits(poly(x, use_sin)) ^ sign);
}
float pcos(float x0) {
    float x = x0, y;
    int32_t j;
    reduce(x, y, j);
    j -= 2;
    const uint32_t sign = ((uint32_t)(~j & 4)) << 29;
    const bool use_sin = (j & 2) == 0;
    x = x + y * -0.78515625f;
    x = x + y * -2.4187564849853515625e-4f;
    x = x + y * -3.77489497744594108e-8f;
    return from_bits(to_bits(poly(x, use_sin)) ^ sign);
}
// pexp<Packet4f> of Eigen 3.3.7 (arch/SSE/MathFunctions.h, the Cephes expf), one lane, SSE2 path (no _mm_floor_ps,
// pmadd = rounded multiply then rounded add)
float pexp(float x0) {
    float x = std::min(x0, 88.3762626647950f);
    x = std::max(x, -88.3762626647949f);
    float fx = x * 1.44269504088896341f + 0.5f;
    float tmp = (float)(int32_t)fx;          // _mm_cvttps_epi32 + _mm_cvtepi32_ps
    if (tmp > fx) tmp = tmp - 1.0f;          // floor
    fx = tmp;
    tmp = fx * 0.693359375f;
    float z = fx * -2.12194440e-4f;
    x = x - tmp;
    x = x - z;
    z = x * x;
    float y = 1.9875691500E-4f;
    y = y * x + 1.3981999507E-3f;
    y = y * x + 8.3334519073E-3f;
    y = y * x + 4.1665795894E-2f;
    y = y * x + 1.6666665459E-1f;
    y = y * x + 5.0000001201E-1f;
    y = y * z + x;
    y = y + 1.0f;
    const int32_t e = ((int32_t)fx + 0x7f) << 23;
    return std::max(y * from_bits((uint32_t)e), x0);
}
}  // namespace orc_eigen337

namespace {
inline float cr_cosf(float t) { return g_orc_trig_mode ? orc_eigen337::pcos(t) : (float)cos((double)t); }
inline float cr_sinf(float t) { return g_orc_trig_mode ? orc_eigen337::psin(t) : (float)sin((double)t); }

inline float cov_sparse_elem(float r, float sf2) {
    float t = (r * 2.0f) * 3.1415926f;
    float a = ((2.0f + cr_cosf(t)) * (1.0f - r)) / 3.0f;
    float b = cr_sinf(t) / (2.0f * 3.1415926f);
    float k = (a + b) * sf2;
    if (k < 0.0) k = 0.0f;
    return k;
}

// BGKInference::predict, bgkinference.h:73-79 with dist :88-93.
// xs: M test points, x: N training points (both un-scaled); division by ell per
// coordinate first (:114), difference, dx^2 + (dy^2 + dz^2), sqrt.
void bgk_predict(float sf2, float ell, const float *xs, int M, const float *x, const float *y, int N, float *ybar,
                 float *kbar) {
    std::vector<float> xsn((size_t)M * 3), xn((size_t)N * 3);
    for (int i = 0; i < M * 3; ++i) xsn[i] = xs[i] / ell;
    for (int i = 0; i < N * 3; ++i) xn[i] = x[i] / ell;
    for (int i = 0; i < M; ++i) {
        float yb = 0.0f, kb = 0.0f;
        for (int j = 0; j < N; ++j) {
            float dx = xn[3 * j + 0] - xsn[3 * i + 0];
            float dy = xn[3 * j + 1] - xsn[3 * i + 1];
            float dz = xn[3 * j + 2] - xsn[3 * i + 2];
            float d2 = dx * dx + (dy * dy + dz * dz);
            float r = sqrtf(d2);
            float k = cov_sparse_elem(r, sf2);
            yb += k * y[j];  // Ks * y
            kb += k;         // Ks.rowwise().sum()
        }
        ybar[i] = yb;
        kbar[i] = kb;
    }
}

// sum mode 1 (see orc_set_sum_mode): the same k and k * y, added to double accumulators
void bgk_predict_acc(float sf2, float ell, const float *xs, int M, const float *x, const float *y, int N, double *ysum,
                     double *ksum) {
    std::vector<float> xsn((size_t)M * 3), xn((size_t)N * 3);
    for (int i = 0; i < M * 3; ++i) xsn[i] = xs[i] / ell;
    for (int i = 0; i < N * 3; ++i) xn[i] = x[i] / ell;
    for (int i = 0; i < M; ++i) {
        double yb = 0.0, kb = 0.0;
        for (int j = 0; j < N; ++j) {
            float dx = xn[3 * j + 0] - xsn[3 * i + 0];
            float dy = xn[3 * j + 1] - xsn[3 * i + 1];
            float dz = xn[3 * j + 2] - xsn[3 * i + 2];
            float d2 = dx * dx + (dy * dy + dz * dz);
            float r = sqrtf(d2);
            float k = cov_sparse_elem(r, sf2);
            float ky = k * y[j];
            yb += (double)ky;
            kb += (double)k;
        }
        ysum[i] += yb;
        ksum[i] += kb;
    }
}

// ---------------------------------------------------------------------------
// GPRegressor<3,float>: include/gpoctomap/gpregressor.h:42-51 (train), :80-92 (predict),
// :114-117 (covMaterniso3).  Eigen internals (LLT, triangular solve, GEMV, packet exp) are
// third-party and unpinned => PARITY UNPINNED for this block; restated with every inner
// product as an fp32 FMA chain in ascending index order (the order an MFMA f32 tile
// accumulates in) and exp() as the correctly rounded single-precision function.
// ---------------------------------------------------------------------------
inline float cr_expf(float x) { return (float)exp((double)x); }

inline float matern3(const float *a, const float *b, float sf2) {  // a, b already scaled by 1.73205/ell
    float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    float d = sqrtf(dx * dx + (dy * dy + dz * dz));
    return ((1 + d) * cr_expf(-d)) * sf2;
}

struct GPModel {
    int N;
    std::vector<float> xn;     // scaled training points
    std::vector<float> alpha;  // K^-1 y
    std::vector<float> L;      // lower Cholesky factor, row-major N x N
    std::vector<double> xn64, alpha64, L64;  // the same in double (GP mode 2 only)
};

void gp_train_eigen(const Params &p, const float *x, const float *y, int N, GPModel &g);
void gp_train_f64(const Params &p, const float *x, const float *y, int N, GPModel &g);
void gp_train(const Params &p, const float *x, const float *y, int N, GPModel &g) {
    if (g_orc_gp_mode == 1) {
        gp_train_eigen(p, x, y, N, g);
        return;
    }
    if (g_orc_gp_mode == 2) {
        gp_train_f64(p, x, y, N, g);
        return;
    }
    g.N = N;
    g.xn.resize((size_t)N * 3);
    const float s = (float)(1.73205 / p.ell);  // double quotient narrowed before the product (:115)
    for (int i = 0; i < N * 3; ++i) g.xn[i] = s * x[i];
    std::vector<float> K((size_t)N * N);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) K[(size_t)i * N + j] = matern3(&g.xn[3 * i], &g.xn[3 * j], p.sf2);
    for (int i = 0; i < N; ++i) K[(size_t)i * N + i] = K[(size_t)i * N + i] + p.noise;  // K + noise * I (:46)
    // LLT (:47): column by column, each entry an FMA chain over k ascending
    g.L.assign((size_t)N * N, 0.0f);
    float *L = g.L.data();
    for (int j = 0; j < N; ++j) {
        float acc = K[(size_t)j * N + j];
        for (int k = 0; k < j; ++k) acc = fmaf(-L[(size_t)j * N + k], L[(size_t)j * N + k], acc);
        const float d = sqrtf(acc);
        L[(size_t)j * N + j] = d;
        for (int i = j + 1; i < N; ++i) {
            float a2 = K[(size_t)i * N + j];
            for (int k = 0; k < j; ++k) a2 = fmaf(-L[(size_t)i * N + k], L[(size_t)j * N + k], a2);
            L[(size_t)i * N + j] = a2 / d;
        }
    }
    // alpha = llt.solve(y) (:48): forward with L (k ascending), backward with L^T (k descending)
    std::vector<float> z(N);
    for (int j = 0; j < N; ++j) {
        float acc = y[j];
        for (int k = 0; k < j; ++k) acc = fmaf(-L[(size_t)j * N + k], z[k], acc);
        z[j] = acc / L[(size_t)j * N + j];
    }
    g.alpha.resize(N);
    for (int j = N - 1; j >= 0; --j) {
        float acc = z[j];
        for (int k = N - 1; k > j; --k) acc = fmaf(-L[(size_t)k * N + j], g.alpha[k], acc);
        g.alpha[j] = acc / L[(size_t)j * N + j];
    }
}

// ---------------------------------------------------------------------------
// GP mode 1: the order of operations of Eigen 3.3.7 on x86-64 without FMA (SSE2 packets of 4 floats), as far as it is
// determined by the library's algorithms rather than by run-time pointer alignment.  A SENSITIVITY PROBE (how far do
// alpha, m and var move when the arithmetic is Eigen's and not an FMA chain), not a pin — Eigen is absent here.
//   * no FMA anywhere: a product is rounded, then added (pmadd without EIGEN_HAS_SINGLE_INSTRUCTION_MADD);
//   * inner products (squaredNorm, GEMV rows, Ks^T alpha) in packet order: two 4-lane accumulators over the aligned
//     part (Redux.h LinearVectorizedTraversal), p0 + p1, predux = (s0 + s2) + (s1 + s3), the tail added one by one;
//   * LLT (Cholesky/LLT.h llt_inplace<Lower>): unblocked below 32 rows; otherwise panels of
//     bs = clamp((n / 8 / 16) * 16, 8, 128) columns — unblocked factor of A11, A21 <- A21 A11^-T, A22 -= A21 A21^T
//     with the rank update accumulated from ZERO over the panel's columns and subtracted once (GEBP: C += alpha * acc);
//   * triangular solves (TriangularSolverMatrix.h, row-major L): panels of 8 rows; inside a panel
//     x_i = (b_i - sum_{k in panel, k < i} l_ik x_k) * (1 / l_ii) with the sum from zero and the RECIPROCAL of the
//     diagonal; the rows below a panel get b -= L21 x as one from-zero accumulation per panel;
//   * exp() as the SSE packet pexp (orc_eigen337::pexp) for every element.
// ---------------------------------------------------------------------------
inline float dot_sse(const float *a, const float *b, int n) {
    const int n4 = n & ~3, n8 = n & ~7;
    float res = 0.0f;
    if (n4) {
        float p0[4], p1[4];
        for (int l = 0; l < 4; ++l) p0[l] = a[l] * b[l];
        if (n4 > 4) {
            for (int l = 0; l < 4; ++l) p1[l] = a[4 + l] * b[4 + l];
            for (int i = 8; i < n8; i += 8)
                for (int l = 0; l < 4; ++l) {
                    p0[l] = p0[l] + a[i + l] * b[i + l];
                    p1[l] = p1[l] + a[i + 4 + l] * b[i + 4 + l];
                }
            for (int l = 0; l < 4; ++l) p0[l] = p0[l] + p1[l];
            if (n4 > n8)
                for (int l = 0; l < 4; ++l) p0[l] = p0[l] + a[n8 + l] * b[n8 + l];
        }
        res = (p0[0] + p0[2]) + (p0[1] + p0[3]);
    }
    for (int i = n4; i < n; ++i) res = res + a[i] * b[i];
    return res;
}
// llt_inplace<float, Lower>::unblocked on the n x n block at (o, o) of the row-major N x N matrix A (lower triangle)
void llt_unblocked_eigen(float *A, int N, int o, int n) {
    std::vector<float> col;
    for (int k = 0; k < n; ++k) {
        float *rk = A + (size_t)(o + k) * N + o;
        float x = rk[k];
        if (k > 0) x = x - dot_sse(rk, rk, k);                       // A10.squaredNorm()
        x = sqrtf(x);
        rk[k] = x;
        for (int i = k + 1; i < n; ++i) {                              // A21 -= A20 * A10^T ; A21 /= x
            float *ri = A + (size_t)(o + i) * N + o;
            float v = ri[k];
            if (k > 0) v = v - dot_sse(ri, rk, k);
            ri[k] = v / x;
        }
    }
}
// rows [r0, r1) of A21 (columns [o, o + bs)) <- A21 * A11^-T, A11 the factored bs x bs block at (o, o): per row a
// forward substitution in panels of 8 columns (sum from zero inside the panel, reciprocal of the diagonal; the
// columns right of a panel get their update as one from-zero accumulation)
void trsm_right_eigen(float *A, int N, int o, int bs, int r0, int r1) {
    for (int i = r0; i < r1; ++i) {
        float *ri = A + (size_t)i * N + o;
        for (int p0 = 0; p0 < bs; p0 += 8) {
            const int pw = std::min(8, bs - p0);
            for (int k = 0; k < pw; ++k) {
                const float *lk = A + (size_t)(o + p0 + k) * N + o;
                float b = 0.0f;
                for (int q = 0; q < k; ++q) b = b + lk[p0 + q] * ri[p0 + q];
                ri[p0 + k] = (ri[p0 + k] - b) * (1.0f / lk[p0 + k]);
            }
            for (int c = p0 + pw; c < bs; ++c) {
                const float *lc = A + (size_t)(o + c) * N + o;
                float acc = 0.0f;
                for (int q = 0; q < pw; ++q) acc = acc + ri[p0 + q] * lc[p0 + q];
                ri[c] = ri[c] - acc;
            }
        }
    }
}
void llt_eigen(float *A, int N) {
    if (N < 32) {
        llt_unblocked_eigen(A, N, 0, N);
        return;
    }
    int bs = N / 8;
    bs = (bs / 16) * 16;
    bs = std::min(std::max(bs, 8), 128);
    for (int k = 0; k < N; k += bs) {
        const int b = std::min(bs, N - k), rs = N - k - b;
        llt_unblocked_eigen(A, N, k, b);
        if (rs > 0) {
            trsm_right_eigen(A, N, k, b, k + b, N);
            for (int i = k + b; i < N; ++i)                             // A22 -= A21 * A21^T (lower part)
                for (int j = k + b; j <= i; ++j) {
                    const float *ai = A + (size_t)i * N + k, *aj = A + (size_t)j * N + k;
                    float acc = 0.0f;
                    for (int q = 0; q < b; ++q) acc = acc + ai[q] * aj[q];
                    A[(size_t)i * N + j] = A[(size_t)i * N + j] - acc;
                }
        }
    }
}
// x <- L^-1 x (forward) for one right-hand side, panels of 8 rows (see the header of this block)
void trsv_lower_eigen(const float *L, int N, float *x) {
    for (int p0 = 0; p0 < N; p0 += 8) {
        const int pw = std::min(8, N - p0);
        for (int k = 0; k < pw; ++k) {
            const float *lk = L + (size_t)(p0 + k) * N;
            float b = 0.0f;
            for (int q = 0; q < k; ++q) b = b + lk[p0 + q] * x[p0 + q];
            x[p0 + k] = (x[p0 + k] - b) * (1.0f / lk[p0 + k]);
        }
        for (int i = p0 + pw; i < N; ++i) {
            const float *li = L + (size_t)i * N;
            float acc = 0.0f;
            for (int q = 0; q < pw; ++q) acc = acc + li[p0 + q] * x[p0 + q];
            x[i] = x[i] - acc;
        }
    }
}
// x <- L^-T x (backward), the mirror image: panels of 8 from the bottom
void trsv_upper_eigen(const float *L, int N, float *x) {
    for (int p1 = N; p1 > 0; p1 -= 8) {
        const int pw = std::min(8, p1), p0 = p1 - pw;
        for (int k = pw - 1; k >= 0; --k) {
            float b = 0.0f;
            for (int q = pw - 1; q > k; --q) b = b + L[(size_t)(p0 + q) * N + p0 + k] * x[p0 + q];
            x[p0 + k] = (x[p0 + k] - b) * (1.0f / L[(size_t)(p0 + k) * N + p0 + k]);
        }
        for (int i = 0; i < p0; ++i) {
            float acc = 0.0f;
            for (int q = 0; q < pw; ++q) acc = acc + L[(size_t)(p0 + q) * N + i] * x[p0 + q];
            x[i] = x[i] - acc;
        }
    }
}
inline float matern3_eigen(const float *a, const float *b, float sf2) {
    float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    float d = sqrtf(dx * dx + (dy * dy + dz * dz));
    return ((1 + d) * orc_eigen337::pexp(-d)) * sf2;
}
void gp_train_eigen(const Params &p, const float *x, const float *y, int N, GPModel &g) {
    g.N = N;
    g.xn.resize((size_t)N * 3);
    const float s = (float)(1.73205 / p.ell);
    for (int i = 0; i < N * 3; ++i) g.xn[i] = s * x[i];
    g.L.assign((size_t)N * N, 0.0f);
    float *L = g.L.data();
    for (int i = 0; i < N; ++i)
        for (int j = 0; j <= i; ++j) L[(size_t)i * N + j] = matern3_eigen(&g.xn[3 * i], &g.xn[3 * j], p.sf2);
    for (int i = 0; i < N; ++i) L[(size_t)i * N + i] = L[(size_t)i * N + i] + p.noise;
    llt_eigen(L, N);
    g.alpha.assign(y, y + N);
    trsv_lower_eigen(L, N, g.alpha.data());
    trsv_upper_eigen(L, N, g.alpha.data());
}
void gp_predict_eigen(const Params &p, const GPModel &g, const float *xs, int M, float *m, float *var) {
    const int N = g.N;
    const float s = (float)(1.73205 / p.ell);
    std::vector<float> v(N);
    for (int j = 0; j < M; ++j) {
        const float t[3] = {s * xs[3 * j], s * xs[3 * j + 1], s * xs[3 * j + 2]};
        for (int k = 0; k < N; ++k) v[k] = matern3_eigen(&g.xn[3 * k], t, p.sf2);
        m[j] = dot_sse(v.data(), g.alpha.data(), N);                    // (Ks^T alpha)(j)
        trsv_lower_eigen(g.L.data(), N, v.data());
        var[j] = p.sf2 - dot_sse(v.data(), v.data(), N);               // Kss - (v^T v).diagonal()
    }
}

// GP mode 2: the same regressor evaluated in double precision throughout (inputs and outputs stay fp32) — the yardstick
// that tells how much of a difference between two fp32 evaluations is rounding noise of the ill-conditioned solve
// (noise 0.01 on a Matern kernel of nearby points) rather than a defect of either.
inline double matern3_64(const double *a, const double *b, double sf2) {
    const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    const double d = sqrt(dx * dx + (dy * dy + dz * dz));
    return ((1 + d) * exp(-d)) * sf2;
}
void gp_train_f64(const Params &p, const float *x, const float *y, int N, GPModel &g) {
    g.N = N;
    const double s = (double)(float)(1.73205 / p.ell);
    struct { std::vector<double> &xn, &alpha, &L; } h{g.xn64, g.alpha64, g.L64};
    h.xn.resize((size_t)N * 3);
    for (int i = 0; i < N * 3; ++i) h.xn[i] = s * (double)x[i];
    h.L.assign((size_t)N * N, 0.0);
    double *L = h.L.data();
    for (int j = 0; j < N; ++j) {
        double acc = matern3_64(&h.xn[3 * j], &h.xn[3 * j], p.sf2) + (double)p.noise;
        for (int k = 0; k < j; ++k) acc -= L[(size_t)j * N + k] * L[(size_t)j * N + k];
        const double d = sqrt(acc);
        L[(size_t)j * N + j] = d;
        for (int i = j + 1; i < N; ++i) {
            double a2 = matern3_64(&h.xn[3 * i], &h.xn[3 * j], p.sf2);
            for (int k = 0; k < j; ++k) a2 -= L[(size_t)i * N + k] * L[(size_t)j * N + k];
            L[(size_t)i * N + j] = a2 / d;
        }
    }
    std::vector<double> z(N);
    for (int j = 0; j < N; ++j) {
        double acc = y[j];
        for (int k = 0; k < j; ++k) acc -= L[(size_t)j * N + k] * z[k];
        z[j] = acc / L[(size_t)j * N + j];
    }
    h.alpha.resize(N);
    for (int j = N - 1; j >= 0; --j) {
        double acc = z[j];
        for (int k = N - 1; k > j; --k) acc -= L[(size_t)k * N + j] * h.alpha[k];
        h.alpha[j] = acc / L[(size_t)j * N + j];
    }
    g.xn.assign(h.xn.begin(), h.xn.end());
    g.alpha.assign(h.alpha.begin(), h.alpha.end());
    g.L.assign(h.L.begin(), h.L.end());
}
void gp_predict_f64(const Params &p, const GPModel &g, const float *xs, int M, float *m, float *var) {
    struct { const std::vector<double> &xn, &alpha, &L; } h{g.xn64, g.alpha64, g.L64};
    const int N = g.N;
    const double s = (double)(float)(1.73205 / p.ell);
    std::vector<double> v(N);
    for (int j = 0; j < M; ++j) {
        const double t[3] = {s * xs[3 * j], s * xs[3 * j + 1], s * xs[3 * j + 2]};
        double mj = 0.0, ss = 0.0;
        for (int k = 0; k < N; ++k) {
            const double ks = matern3_64(&h.xn[3 * k], t, p.sf2);
            mj += ks * h.alpha[k];
            double acc = ks;
            for (int i = 0; i < k; ++i) acc -= h.L[(size_t)k * N + i] * v[i];
            v[k] = acc / h.L[(size_t)k * N + k];
            ss += v[k] * v[k];
        }
        m[j] = (float)mj;
        var[j] = (float)((double)p.sf2 - ss);
    }
}

void gp_predict(const Params &p, const GPModel &g, const float *xs, int M, float *m, float *var) {
    if (g_orc_gp_mode == 1) {
        gp_predict_eigen(p, g, xs, M, m, var);
        return;
    }
    if (g_orc_gp_mode == 2) {
        gp_predict_f64(p, g, xs, M, m, var);
        return;
    }
    const int N = g.N;
    const float s = (float)(1.73205 / p.ell);
    std::vector<float> v(N);
    for (int j = 0; j < M; ++j) {
        const float t[3] = {s * xs[3 * j], s * xs[3 * j + 1], s * xs[3 * j + 2]};
        float mj = 0.0f, ss = 0.0f;
        for (int k = 0; k < N; ++k) {
            const float ks = matern3(&g.xn[3 * k], t, p.sf2);     // Ks(k, j), dist(x, xs)
            mj = fmaf(ks, g.alpha[k], mj);                          // m = Ks^T alpha (:85)
            float acc = ks;                                          // v = L^-1 Ks (:87)
            for (int i = 0; i < k; ++i) acc = fmaf(-g.L[(size_t)k * N + i], v[i], acc);
            v[k] = acc / g.L[(size_t)k * N + k];
            ss = fmaf(v[k], v[k], ss);                               // (v^T v).diagonal() (:90)
        }
        m[j] = mj;
        var[j] = p.sf2 - ss;
    }
}

// ---------------------------------------------------------------------------
// pcl::VoxelGrid<PointXYZ>::applyFilter restated (PCL 1.10 filters/impl/voxel_grid.hpp;
// third-party, absent from /root/reference, version unpinned => parity unpinned).
// downsample_all_data_=true, min_points_per_voxel_=0, no field filter.
// Call site: src/bgkoctomap/bgkoctomap.cpp:419-431.
// ---------------------------------------------------------------------------
void voxel_grid(const std::vector<V3> &in, float leaf, std::vector<V3> &out) {
    out.clear();
    if (in.empty()) return;
    float inv = 1.0f / leaf;  // inverse_leaf_size_ = Ones / leaf_size_
    float mn[3] = {std::numeric_limits<float>::max(), std::numeric_limits<float>::max(),
                   std::numeric_limits<float>::max()};
    float mx[3] = {-mn[0], -mn[0], -mn[0]};
    for (const V3 &p : in) {
        if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z)) continue;
        mn[0] = std::min(mn[0], p.x); mn[1] = std::min(mn[1], p.y); mn[2] = std::min(mn[2], p.z);
        mx[0] = std::max(mx[0], p.x); mx[1] = std::max(mx[1], p.y); mx[2] = std::max(mx[2], p.z);
    }
    int64_t dx = (int64_t)((mx[0] - mn[0]) * inv) + 1;
    int64_t dy = (int64_t)((mx[1] - mn[1]) * inv) + 1;
    int64_t dz = (int64_t)((mx[2] - mn[2]) * inv) + 1;
    if (dx * dy * dz > (int64_t)std::numeric_limits<int32_t>::max()) {
        out = in;  // "Leaf size is too small ... Integer indices would overflow."
        return;
    }
    int min_b[3], max_b[3], div_b[3], mul[3];
    for (int a = 0; a < 3; ++a) {
        min_b[a] = (int)std::floor(mn[a] * inv);
        max_b[a] = (int)std::floor(mx[a] * inv);
        div_b[a] = max_b[a] - min_b[a] + 1;
    }
    mul[0] = 1; mul[1] = div_b[0]; mul[2] = div_b[0] * div_b[1];
    std::vector<std::pair<unsigned, unsigned>> iv;
    iv.reserve(in.size());
    for (size_t i = 0; i < in.size(); ++i) {
        const V3 &p = in[i];
        if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z)) continue;
        int i0 = (int)(std::floor(p.x * inv) - (float)min_b[0]);
        int i1 = (int)(std::floor(p.y * inv) - (float)min_b[1]);
        int i2 = (int)(std::floor(p.z * inv) - (float)min_b[2]);
        int idx = i0 * mul[0] + i1 * mul[1] + i2 * mul[2];
        iv.emplace_back((unsigned)idx, (unsigned)i);
    }
    // std::sort in PCL is not stable; equal-cell order is implementation defined.
    // Restated as ascending cloud index inside a cell — or, with the sensitivity switch, as what libstdc++'s introsort
    // leaves when it compares idx only, like pcl::VoxelGrid's cloud_point_index_idx::operator<.
    if (g_orc_grid_sort_mode) {
        struct PclLess {
            bool operator()(const std::pair<unsigned, unsigned> &a, const std::pair<unsigned, unsigned> &b) const { return a.first < b.first; }
        };
        std::sort(iv.begin(), iv.end(), PclLess());
    } else {
        std::sort(iv.begin(), iv.end());
    }
    size_t i = 0;
    while (i < iv.size()) {
        size_t j = i + 1;
        while (j < iv.size() && iv[j].first == iv[i].first) ++j;
        // CentroidPoint / AccumulatorXYZ: float sums, divide by (float)n
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
        for (size_t k = i; k < j; ++k) {
            const V3 &p = in[iv[k].second];
            sx += p.x; sy += p.y; sz += p.z;
        }
        float n = (float)(j - i);
        out.push_back(V3{sx / n, sy / n, sz / n});
        i = j;
    }
}

// src/bgkoctomap/bgkoctomap.cpp:433-458
void beam_sample(V3 hit, V3 origin, float free_resolution, std::vector<V3> &frees) {
    frees.clear();
    float x0 = origin.x, y0 = origin.y, z0 = origin.z;
    float x = hit.x, y = hit.y, z = hit.z;
    float l = (float)sqrt((x - x0) * (x - x0) + (y - y0) * (y - y0) + (z - z0) * (z - z0));
    float nx = (x - x0) / l, ny = (y - y0) / l, nz = (z - z0) / l;
    float d = free_resolution;
    while (d < l) {
        frees.push_back(V3{x0 + nx * d, y0 + ny * d, z0 + nz * d});
        d += free_resolution;
    }
    if (l > free_resolution)
        frees.push_back(V3{x0 + nx * (l - free_resolution), y0 + ny * (l - free_resolution),
                           z0 + nz * (l - free_resolution)});
}

struct XY {
    V3 p;
    float y;
};

// src/bgkoctomap/bgkoctomap.cpp:383-417
void get_training_data(const std::vector<V3> &cloud, V3 origin, float ds_resolution, float free_resolution,
                       float max_range, std::vector<XY> &xy, size_t *n_hits, size_t *n_frees, float free_label = 0.0f) {
    std::vector<V3> sampled_hits;
    if (ds_resolution < 0) sampled_hits = cloud; else voxel_grid(cloud, ds_resolution, sampled_hits);
    std::vector<V3> frees, frees_n;
    xy.clear();
    for (const V3 &p : sampled_hits) {
        if (max_range > 0) {
            float ddx = p.x - origin.x, ddy = p.y - origin.y, ddz = p.z - origin.z;
            // point3f::norm(): double sqrt of a float sum (point3f.h:207-214)
            double l = sqrt((double)(ddx * ddx + ddy * ddy + ddz * ddz));
            if (l > max_range) continue;
        }
        xy.push_back(XY{p, 1.0f});
        beam_sample(p, origin, free_resolution, frees_n);
        frees.push_back(origin);
        for (const V3 &f : frees_n) frees.push_back(f);
    }
    if (n_hits) *n_hits = xy.size();
    std::vector<V3> sampled_frees;
    if (ds_resolution < 0) sampled_frees = frees; else voxel_grid(frees, ds_resolution, sampled_frees);
    for (const V3 &f : sampled_frees) xy.push_back(XY{f, free_label});  // 0 (bgkoctomap.cpp:415), -1 (gpoctomap.cpp:399)
    if (n_frees) *n_frees = sampled_frees.size();
}

// ---------------------------------------------------------------------------
// BGKLOctoMap (block-level BGK with free-space line segments; variant 3 here)
//   get_training_data / beam_sample   src/bgkloctomap/bgkloctomap.cpp:300-343, 359-381
//   point_to_line_dist / covSparseLine include/bgkloctomap/bgklinference.h:104-140, 186-200
// ---------------------------------------------------------------------------
struct Seg {
    V3 a, b;
};
struct LData {
    std::vector<int> ray_idx;  // per training sample: -1 = hit, else index into rays
    std::vector<Seg> rays;     // origin -> hit shortened by free_resolution
};

// Hits are re-projected as origin + n * l; free samples step DOWN from l - free_resolution while d > 0 and are
// NOT voxel-filtered; every sample of a beam (and the origin sample that precedes them) carries the beam's index.
void get_training_data_l(const std::vector<V3> &cloud, V3 origin, float ds_resolution, float free_resolution, float max_range,
                         std::vector<XY> &xy, LData &ld) {
    std::vector<V3> sampled_hits;
    if (ds_resolution < 0) sampled_hits = cloud; else voxel_grid(cloud, ds_resolution, sampled_hits);
    xy.clear();
    ld.ray_idx.clear();
    ld.rays.clear();
    int idx = 0;
    for (const V3 &p : sampled_hits) {
        if (max_range > 0) {
            float ddx = p.x - origin.x, ddy = p.y - origin.y, ddz = p.z - origin.z;
            double l = sqrt((double)(ddx * ddx + ddy * ddy + ddz * ddz));
            if (l > max_range) continue;
        }
        float l = (float)sqrt((p.x - origin.x) * (p.x - origin.x) + (p.y - origin.y) * (p.y - origin.y) +
                              (p.z - origin.z) * (p.z - origin.z));
        const float nx = (p.x - origin.x) / l, ny = (p.y - origin.y) / l, nz = (p.z - origin.z) / l;
        const V3 occ{origin.x + nx * l, origin.y + ny * l, origin.z + nz * l};
        xy.push_back(XY{occ, 1.0f});
        ld.ray_idx.push_back(-1);
        // beam_sample(occ_endpt, origin, ...): its own l and n from the re-projected end point
        {
            xy.push_back(XY{origin, 0.0f});
            ld.ray_idx.push_back(idx);
            const float l2 = (float)sqrt((occ.x - origin.x) * (occ.x - origin.x) + (occ.y - origin.y) * (occ.y - origin.y) +
                                         (occ.z - origin.z) * (occ.z - origin.z));
            const float mx = (occ.x - origin.x) / l2, my = (occ.y - origin.y) / l2, mz = (occ.z - origin.z) / l2;
            float d = l2 - free_resolution;
            while (d > 0.0) {
                xy.push_back(XY{V3{origin.x + mx * d, origin.y + my * d, origin.z + mz * d}, 0.0f});
                ld.ray_idx.push_back(idx);
                d -= free_resolution;
            }
        }
        l = l - free_resolution;
        ld.rays.push_back(Seg{origin, V3{origin.x + nx * l, origin.y + ny * l, origin.z + nz * l}});
        ++idx;
    }
}

// point_to_line_dist for one (point, segment) pair: point3f arithmetic in float, norms and dots through double,
// b = c1 / c2 in double narrowed to float by point3f::operator*(float) (bgklinference.h:104-140)
inline float seg_dist_l(V3 p, V3 p0, V3 p1) {
    auto sub = [](V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; };
    auto norm = [](V3 a) { return sqrt((double)(a.x * a.x + a.y * a.y + a.z * a.z)); };
    auto dot = [](V3 a, V3 b) { return (double)(a.x * b.x + a.y * b.y + a.z * b.z); };
    const V3 line_vec = sub(p1, p0);
    const float line_len = (float)norm(line_vec);
    const V3 pnt_vec = sub(p, p0);
    if (line_len < 0.0001f) return (float)norm(sub(p, p0));
    const double c1 = dot(pnt_vec, line_vec), c2 = dot(line_vec, line_vec);
    if (c1 <= 0) return (float)norm(sub(p, p0));
    if (c2 <= c1) return (float)norm(sub(p, p1));
    const float b = (float)(c1 / c2);
    const V3 nearest{p0.x + line_vec.x * b, p0.y + line_vec.y * b, p0.z + line_vec.z * b};
    return (float)norm(sub(p, nearest));
}

// BGKLInference::predict (bgklinference.h:80-88): rows = 6-float segments, labels y
void bgkl_predict(float sf2, float ell, const float *xs, int M, const Seg *rows, const float *y, int N, float *ybar,
                  float *kbar) {
    for (int i = 0; i < M; ++i) {
        const V3 q{xs[3 * i], xs[3 * i + 1], xs[3 * i + 2]};
        if (g_orc_sum_mode == 1) {
            // sum mode 1 (orc_set_sum_mode; the device's "bgk_sum" 1 for BGKLOctoMap): the same fp32 k and k * y of every row,
            // summed in DOUBLE, each of the neighbour's two sums rounded to fp32 once — the correctly rounded value of what the
            // fp32 chains below approximate, whatever the order of the rows.  The per-neighbour gate kbar > 0.001f
            // (bgkloctomap.cpp:226-227) and the fp32 update per neighbour stay as they are.
            double dy = 0.0, dk = 0.0;
            for (int j = 0; j < N; ++j) {
                const float r = seg_dist_l(q, rows[j].a, rows[j].b) / ell;
                const float k = cov_sparse_elem(r, sf2);
                const float ky = k * y[j];
                dy += (double)ky;
                dk += (double)k;
            }
            ybar[i] = (float)dy;
            kbar[i] = (float)dk;
            continue;
        }
        float sy = 0.0f, sk = 0.0f;
        for (int j = 0; j < N; ++j) {
            const float r = seg_dist_l(q, rows[j].a, rows[j].b) / ell;  // Kxz /= ell
            const float k = cov_sparse_elem(r, sf2);                     // formula + `< 0 -> 0` clean-up
            sy += k * y[j];
            sk += k;
        }
        ybar[i] = sy;
        kbar[i] = sk;
    }
}

// ---------------------------------------------------------------------------
// Map
// ---------------------------------------------------------------------------
struct Stats {
    double n_hits, n_frees, n_bbox_blocks, n_train_blocks, n_test_blocks;
    double voxel_updates;   // U: sum over test blocks of leaf count
    double update_calls;    // node.update invocations
    double pair_evals;      // P
    double train_reads;     // sum_t sum_{b in E(t)} N_b
    double t_frontend, t_partition, t_predict, t_prune, t_total;
};

struct Map {
    Params p;
    std::vector<std::vector<V3>> lut;
    std::unordered_map<int64_t, Block *> blocks;
    Stats st;
    ~Map() {
        for (auto &kv : blocks) delete kv.second;
    }
};

// Closed-box membership (src/bgkoctomap/bgkoctomap.cpp:497-503 + rtree.h:1519-1532):
// p in block iff  c-h <= p <= c+h  per axis, all in fp32.
inline bool in_closed_box(const Params &p, V3 c, V3 q) {
    float h = p.block_size / 2.0f;
    float lo, hi;
    lo = c.x - h; hi = c.x + h; if (lo > q.x || q.x > hi) return false;
    lo = c.y - h; hi = c.y + h; if (lo > q.y || q.y > hi) return false;
    lo = c.z - h; hi = c.z + h; if (lo > q.z || q.z > hi) return false;
    return true;
}

// Spatial index standing in for the reference's per-scan R-tree
// (include/common/rtree.h): same query results (closed boxes), returned in
// ascending training-point index (the R-tree's traversal order is not restated —
// it only permutes fp32 sums).
struct PointIndex {
    const Params *p;
    const std::vector<XY> *xy;
    std::unordered_map<int64_t, std::vector<int>> cell;  // primary cell -> point ids
    static int64_t ckey(int64_t ix, int64_t iy, int64_t iz) { return (ix << 40) | (iy << 20) | iz; }
    void build(const Params &pp, const std::vector<XY> &pts) {
        p = &pp; xy = &pts;
        for (size_t i = 0; i < pts.size(); ++i) {
            int64_t k = block_to_hash_key(pp, pts[i].p.x, pts[i].p.y, pts[i].p.z);
            cell[k].push_back((int)i);
        }
    }
    // gather ids inside the closed box of block `key`; if first_only, stop at one.
    int query(int64_t key, std::vector<int> *out, bool first_only) const {
        V3 c = hash_key_to_block(*p, key);
        int64_t ix = key >> 40, iy = (key >> 20) & 0xFFFFF, iz = key & 0xFFFFF;
        int found = 0;
        for (int64_t a = -1; a <= 1; ++a)
            for (int64_t b = -1; b <= 1; ++b)
                for (int64_t d = -1; d <= 1; ++d) {
                    auto it = cell.find(ckey(ix + a, iy + b, iz + d));
                    if (it == cell.end()) continue;
                    for (int id : it->second)
                        if (in_closed_box(*p, c, (*xy)[id].p)) {
                            ++found;
                            if (out) out->push_back(id);
                            if (first_only) return found;
                        }
                }
        if (out) std::sort(out->begin(), out->end());
        return found;
    }
};

double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Stages B..G of BGKOctoMap::insert_pointcloud, src/bgkoctomap/bgkoctomap.cpp:229-366; with `ungated` the same
// stages as BGKOctoMap::insert_training_data runs them (:82-212): node.update for every leaf of a test block and
// every neighbour model, whatever kbar is (:179-185).
void insert_xy(Map &m, const std::vector<XY> &xy, const LData *ld = nullptr, bool ungated = false) {
    const Params &p = m.p;
    Stats &st = m.st;
    if (xy.empty()) return;  // :230-232
    double t0 = now_s();

    // bbox(): :464-484
    V3 lo = xy[0].p, hi = xy[0].p;
    for (const XY &q : xy) {
        lo.x = std::min(lo.x, q.p.x); lo.y = std::min(lo.y, q.p.y); lo.z = std::min(lo.z, q.p.z);
        hi.x = std::max(hi.x, q.p.x); hi.y = std::max(hi.y, q.p.y); hi.z = std::max(hi.z, q.p.z);
    }
    // get_blocks_in_bbox(): :486-495 — float-stepped triple loop, duplicates kept.
    std::vector<int64_t> blocks;
    const float bs = p.block_size;
    for (float x = lo.x - bs; x <= hi.x + 2 * bs; x += bs)
        for (float y = lo.y - bs; y <= hi.y + 2 * bs; y += bs)
            for (float z = lo.z - bs; z <= hi.z + 2 * bs; z += bs) blocks.push_back(block_to_hash_key(p, x, y, z));
    st.n_bbox_blocks = (double)blocks.size();

    PointIndex index;  // :240-243 rtree.Insert
    index.build(p, xy);

    // TRAIN :250-284 (serial order; `test_blocks` keeps duplicates of `blocks`)
    std::vector<int64_t> test_blocks;
    std::unordered_map<int64_t, std::vector<int>> bgk_arr;  // key -> training point ids
    for (size_t i = 0; i < blocks.size(); ++i) {
        int64_t key = blocks[i];
        int64_t eb[7];
        extended_block_from_center(p, hash_key_to_block(p, key), key, eb);  // get_extended_block(key)
        bool has = false;
        for (int k = 0; k < 7 && !has; ++k) has = index.query(eb[k], nullptr, true) > 0;
        if (has) test_blocks.push_back(key);
        std::vector<int> ids;
        index.query(key, &ids, false);
        if (ids.empty()) continue;
        bgk_arr.emplace(key, std::move(ids));  // emplace: first insertion wins
    }
    st.n_train_blocks = (double)bgk_arr.size();
    st.n_test_blocks = (double)test_blocks.size();
    // GPOctoMap: gpr->train per training block (gpoctomap.cpp:253-275)
    std::unordered_map<int64_t, GPModel> gp_arr;
    if (p.variant == 1) {
        std::vector<int64_t> tkeys;
        for (auto &kv : bgk_arr) {
            tkeys.push_back(kv.first);
            gp_arr.emplace(kv.first, GPModel());
        }
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic)
#endif
        for (long ti = 0; ti < (long)tkeys.size(); ++ti) {
            const std::vector<int> &ids = bgk_arr[tkeys[ti]];
            std::vector<float> bx(ids.size() * 3), by(ids.size());
            for (size_t n = 0; n < ids.size(); ++n) {
                bx[3 * n] = xy[ids[n]].p.x; bx[3 * n + 1] = xy[ids[n]].p.y; bx[3 * n + 2] = xy[ids[n]].p.z;
                by[n] = xy[ids[n]].y;
            }
            gp_train(p, bx.data(), by.data(), (int)ids.size(), gp_arr.find(tkeys[ti])->second);
        }
    }
    // BGKLOctoMap: per training block, hits become degenerate segments (label 1) and every beam that has a sample
    // in the block contributes its segment once, at the position of its first sample (bgkloctomap.cpp:141-170)
    std::unordered_map<int64_t, std::pair<std::vector<Seg>, std::vector<float>>> bgkl_arr;
    if (p.variant == 3) {
        std::vector<int> stamp(ld->rays.size(), -1);
        int serial = 0;
        for (auto &kv : bgk_arr) {
            auto &rows = bgkl_arr[kv.first];
            for (int id : kv.second) {
                const int r = ld->ray_idx[id];
                if (r < 0) {
                    rows.first.push_back(Seg{xy[id].p, xy[id].p});
                    rows.second.push_back(1.0f);
                } else if (stamp[r] != serial) {
                    stamp[r] = serial;
                    rows.first.push_back(ld->rays[r]);
                    rows.second.push_back(0.0f);
                }
            }
            ++serial;
        }
    }
    double t1 = now_s();
    st.t_partition = t1 - t0;

    // Blocks are created serially first (the reference does it inside an omp
    // critical; creation order does not affect results).
    for (int64_t key : test_blocks)
        if (m.blocks.find(key) == m.blocks.end()) m.blocks.emplace(key, block_new(p, hash_key_to_block(p, key)));

    // PREDICT :293-336
    double U = 0, calls = 0, pairs = 0, reads = 0;
    // duplicates in test_blocks must be processed one after the other; group them.
    // (With OpenMP the reference would race on them; serial semantics are kept.)
    std::vector<char> is_dup(test_blocks.size(), 0);
    {
        std::unordered_map<int64_t, int> seen;
        for (size_t i = 0; i < test_blocks.size(); ++i) is_dup[i] = seen[test_blocks[i]]++ > 0;
    }
    auto predict_one = [&](long ti, double &U_, double &calls_, double &pairs_, double &reads_) {
        int64_t key = test_blocks[ti];
        Block *block = m.blocks.find(key)->second;
        std::vector<int> leaf_keys;
        enumerate_leaves(p, *block, leaf_keys);
        int M = (int)leaf_keys.size();
        std::vector<float> xs((size_t)M * 3);
        for (int j = 0; j < M; ++j) {
            const V3 &o = m.lut[leaf_keys[j] >> 16][leaf_keys[j] & 0xFFFF];
            xs[3 * j + 0] = o.x + block->center.x;  // Block::get_loc, bgkblock.h:64-66
            xs[3 * j + 1] = o.y + block->center.y;
            xs[3 * j + 2] = o.z + block->center.z;
        }
        U_ += M;
        int64_t eb[7];
        extended_block_from_center(p, block->center,
                                   block_to_hash_key(p, block->center.x, block->center.y, block->center.z), eb);
        std::vector<float> bx, by, ybar(M), kbar(M);
        const bool sum64 = g_orc_sum_mode == 1 && p.variant == 0;
        std::vector<double> ysum(sum64 ? M : 0, 0.0), ksum(sum64 ? M : 0, 0.0);
        for (int k = 0; k < 7; ++k) {
            auto it = bgk_arr.find(eb[k]);
            if (it == bgk_arr.end()) continue;
            if (p.variant == 3) {  // BGKLOctoMap: bgkloctomap.cpp:206-231, gate kbar > 0.001
                const auto &rows = bgkl_arr.find(eb[k])->second;
                const int NR = (int)rows.second.size();
                pairs_ += (double)M * NR;
                reads_ += NR;
                bgkl_predict(p.sf2, p.ell, xs.data(), M, rows.first.data(), rows.second.data(), NR, ybar.data(), kbar.data());
                for (int j = 0; j < M; ++j)
                    if (kbar[j] > 0.001f) {
                        node_update(p, block->layer[leaf_keys[j] >> 16][leaf_keys[j] & 0xFFFF], ybar[j], kbar[j]);
                        calls_ += 1;
                    }
                continue;
            }
            const std::vector<int> &ids = it->second;
            int N = (int)ids.size();
            bx.resize((size_t)N * 3); by.resize(N);
            for (int n = 0; n < N; ++n) {
                bx[3 * n] = xy[ids[n]].p.x; bx[3 * n + 1] = xy[ids[n]].p.y; bx[3 * n + 2] = xy[ids[n]].p.z;
                by[n] = xy[ids[n]].y;
            }
            pairs_ += (double)M * N;
            reads_ += N;
            if (p.variant == 1) {  // GPOctoMap: gpoctomap.cpp:306-319, unconditional BCM update
                gp_predict(p, gp_arr.find(eb[k])->second, xs.data(), M, ybar.data(), kbar.data());
                for (int j = 0; j < M; ++j) {
                    gp_node_update(p, block->layer[leaf_keys[j] >> 16][leaf_keys[j] & 0xFFFF], ybar[j], kbar[j]);
                    calls_ += 1;
                }
                continue;
            }
            if (sum64) {
                bgk_predict_acc(p.sf2, p.ell, xs.data(), M, bx.data(), by.data(), N, ysum.data(), ksum.data());
                continue;
            }
            bgk_predict(p.sf2, p.ell, xs.data(), M, bx.data(), by.data(), N, ybar.data(), kbar.data());
            for (int j = 0; j < M; ++j) {
                Node &node = block->layer[leaf_keys[j] >> 16][leaf_keys[j] & 0xFFFF];
                if (kbar[j] > 0.0 || ungated) {  // :331-333
                    node_update(p, node, ybar[j], kbar[j]);
                    calls_ += 1;
                }
            }
        }
        if (sum64)
            for (int j = 0; j < M; ++j) {
                Node &node = block->layer[leaf_keys[j] >> 16][leaf_keys[j] & 0xFFFF];
                if (ksum[j] > 0.0 || ungated) {
                    const float A1 = (float)((double)node.A + ysum[j]);
                    const float B1 = (float)((double)node.B + (ksum[j] - ysum[j]));
                    node.A = A1;
                    node.B = B1;
                    node_update(p, node, 0.0f, 0.0f);  // + 0 leaves A, B as they are; state and classified as in update()
                    calls_ += 1;
                }
            }
    };
    // first occurrences: independent blocks, parallel like the reference's omp loop
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic) reduction(+ : U, calls, pairs, reads)
#endif
    for (long ti = 0; ti < (long)test_blocks.size(); ++ti)
        if (!is_dup[ti]) predict_one(ti, U, calls, pairs, reads);
    // repeated keys (float-stepping artefact of get_blocks_in_bbox): serial, in list order
    for (long ti = 0; ti < (long)test_blocks.size(); ++ti)
        if (is_dup[ti]) predict_one(ti, U, calls, pairs, reads);
    st.voxel_updates = U; st.update_calls = calls; st.pair_evals = pairs; st.train_reads = reads;
    double t2 = now_s();
    st.t_predict = t2 - t1;

    // PRUNE :344-353
    for (int64_t key : test_blocks) {
        auto it = m.blocks.find(key);
        if (it == m.blocks.end()) continue;
        block_prune(p, *it->second);
    }
    st.t_prune = now_s() - t2;
}

}  // namespace

// ===========================================================================
// C interface (ctypes)
// ===========================================================================
extern "C" {

void *orc_map_create(float resolution, int block_depth, float sf2, float ell, float free_thresh, float occupied_thresh,
                     float var_thresh, float prior_A, float prior_B) {
    Map *m = new Map;
    m->p = Params{resolution, block_depth, sf2, ell, free_thresh, occupied_thresh, var_thresh, prior_A, prior_B,
                  (float)pow(2, block_depth - 1) * resolution,  // bgkoctomap.cpp:41
                  0, 0.f, 0.f, 0.f, 0.f, 0.f};
    m->lut = build_lut(resolution, block_depth);
    std::memset(&m->st, 0, sizeof(Stats));
    return m;
}
// GPOctoMap(resolution, block_depth, sf2, ell, noise, l, min_var, max_var, max_known_var, free_thresh,
// occupied_thresh): src/gpoctomap/gpoctomap.cpp:23-46
void *orc_gp_map_create(float resolution, int block_depth, float sf2, float ell, float noise, float l, float min_var,
                        float max_var, float max_known_var, float free_thresh, float occupied_thresh) {
    Map *m = new Map;
    m->p = Params{resolution, block_depth, sf2, ell, free_thresh, occupied_thresh, 0.f, 0.f, 0.f,
                  (float)pow(2, block_depth - 1) * resolution,
                  1, noise, l, 1.0f / max_var, 1.0f / min_var, 1.0f / max_known_var};
    m->lut = build_lut(resolution, block_depth);
    std::memset(&m->st, 0, sizeof(Stats));
    return m;
}
// BGKLOctoMap(resolution, block_depth, sf2, ell, free_thresh, occupied_thresh, var_thresh, prior_A, prior_B):
// src/bgkloctomap/bgkloctomap.cpp:31-57 (same node as BGKOctoMap, bgkloctree_node.cpp)
void *orc_l_map_create(float resolution, int block_depth, float sf2, float ell, float free_thresh, float occupied_thresh,
                       float var_thresh, float prior_A, float prior_B) {
    Map *m = (Map *)orc_map_create(resolution, block_depth, sf2, ell, free_thresh, occupied_thresh, var_thresh, prior_A, prior_B);
    m->p.variant = 3;
    return m;
}
void orc_map_destroy(void *h) { delete (Map *)h; }
// GPRegressor train + predict on one block (known-answer tests)
void orc_gp_train_predict(void *h, const float *x, const float *y, int N, const float *xs, int M, float *alpha,
                          float *L, float *m, float *var) {
    Map *mp = (Map *)h;
    GPModel g;
    gp_train(mp->p, x, y, N, g);
    if (alpha) std::memcpy(alpha, g.alpha.data(), sizeof(float) * N);
    if (L) std::memcpy(L, g.L.data(), sizeof(float) * (size_t)N * N);
    if (M) gp_predict(mp->p, g, xs, M, m, var);
}
void orc_gp_node_update(void *h, float *m_ivar, float *ivar, uint8_t *state, float new_m, float new_var) {
    Node n{0, *m_ivar, *ivar, *state};
    gp_node_update(((Map *)h)->p, n, new_m, new_var);
    *m_ivar = n.A; *ivar = n.B; *state = n.state;
}
float orc_gp_node_prob(void *h, float m_ivar) { return gp_node_prob(((Map *)h)->p, Node{0, m_ivar, 0.f, 0}); }
float orc_block_size(void *h) { return ((Map *)h)->p.block_size; }

int64_t orc_block_to_hash_key(void *h, float x, float y, float z) { return block_to_hash_key(((Map *)h)->p, x, y, z); }
void orc_hash_key_to_block(void *h, int64_t key, float *out3) {
    V3 c = hash_key_to_block(((Map *)h)->p, key);
    out3[0] = c.x; out3[1] = c.y; out3[2] = c.z;
}
void orc_get_extended_block(void *h, int64_t key, int64_t *out7) {
    Map *m = (Map *)h;
    extended_block_from_center(m->p, hash_key_to_block(m->p, key), key, out7);
}
int orc_lut_count(void *h, int depth) { return (int)((Map *)h)->lut[depth].size(); }
void orc_lut(void *h, int depth, int index, float *out3) {
    const V3 &v = ((Map *)h)->lut[depth][index];
    out3[0] = v.x; out3[1] = v.y; out3[2] = v.z;
}

// sin / cos of the active trig mode (orc_set_modes), array form: what = 0 sin, 1 cos
void orc_trig_array(const float *t, int n, int what, float *out) {
    for (int i = 0; i < n; ++i) out[i] = what ? cr_cosf(t[i]) : cr_sinf(t[i]);
}
float orc_kernel(float r, float sf2) { return cov_sparse_elem(r, sf2); }
void orc_kernel_array(const float *r, int n, float sf2, float *out) {
    for (int i = 0; i < n; ++i) out[i] = cov_sparse_elem(r[i], sf2);
}
// k(r) without the <0 clamp (for the support-radius test)
float orc_kernel_raw(float r, float sf2) {
    float t = (r * 2.0f) * 3.1415926f;
    float a = ((2.0f + cr_cosf(t)) * (1.0f - r)) / 3.0f;
    float b = cr_sinf(t) / (2.0f * 3.1415926f);
    return (a + b) * sf2;
}
// exhaustive scan of fp32 r in [r0, r1]: returns max raw kernel value (must be <= 0 for r >= 1)
float orc_kernel_max_over(float r0, float r1, float sf2) {
    float mx = -std::numeric_limits<float>::infinity();
    for (float r = r0; r <= r1; r = std::nextafter(r, std::numeric_limits<float>::infinity())) {
        float k = orc_kernel_raw(r, sf2);
        if (k > mx) mx = k;
    }
    return mx;
}
void orc_bgk_predict(float sf2, float ell, const float *xs, int M, const float *x, const float *y, int N, float *ybar,
                     float *kbar) {
    bgk_predict(sf2, ell, xs, M, x, y, N, ybar, kbar);
}
// node update on a bare (A,B,state) triple
void orc_node_update(void *h, float *A, float *B, uint8_t *state, float ybar, float kbar) {
    Node n{0, *A, *B, *state};
    node_update(((Map *)h)->p, n, ybar, kbar);
    *A = n.A; *B = n.B; *state = n.state;
}
float orc_node_var(float A, float B) { return node_var(Node{0, A, B, 0}); }
float orc_node_prob(float A, float B) { return node_prob(Node{0, A, B, 0}); }

int orc_voxel_grid(const float *xyz, int n, float leaf, float *out_xyz) {
    std::vector<V3> in(n), out;
    for (int i = 0; i < n; ++i) in[i] = V3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    voxel_grid(in, leaf, out);
    for (size_t i = 0; i < out.size(); ++i) {
        out_xyz[3 * i] = out[i].x; out_xyz[3 * i + 1] = out[i].y; out_xyz[3 * i + 2] = out[i].z;
    }
    return (int)out.size();
}
int orc_beam_sample(const float *hit, const float *origin, float free_res, float *out_xyz, int cap) {
    std::vector<V3> f;
    beam_sample(V3{hit[0], hit[1], hit[2]}, V3{origin[0], origin[1], origin[2]}, free_res, f);
    int n = (int)std::min<size_t>(f.size(), cap);
    for (int i = 0; i < n; ++i) { out_xyz[3 * i] = f[i].x; out_xyz[3 * i + 1] = f[i].y; out_xyz[3 * i + 2] = f[i].z; }
    return (int)f.size();
}

// returns number of training points; out may be null to query the size (call twice)
static std::vector<XY> g_xy;
int64_t orc_get_training_data(const float *xyz, int64_t n, const float *origin, float ds, float free_res,
                              float max_range, float *out_xyzy, int64_t cap) {
    std::vector<V3> cloud(n);
    for (int64_t i = 0; i < n; ++i) cloud[i] = V3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    get_training_data(cloud, V3{origin[0], origin[1], origin[2]}, ds, free_res, max_range, g_xy, nullptr, nullptr);
    if (out_xyzy) {
        int64_t m = std::min<int64_t>(cap, (int64_t)g_xy.size());
        for (int64_t i = 0; i < m; ++i) {
            out_xyzy[4 * i] = g_xy[i].p.x; out_xyzy[4 * i + 1] = g_xy[i].p.y; out_xyzy[4 * i + 2] = g_xy[i].p.z;
            out_xyzy[4 * i + 3] = g_xy[i].y;
        }
    }
    return (int64_t)g_xy.size();
}

// BGKOctoMap::insert_pointcloud, src/bgkoctomap/bgkoctomap.cpp:214-366
void orc_insert_pointcloud(void *h, const float *xyz, int64_t n, const float *origin, float ds_resolution,
                           float free_res, float max_range) {
    Map *m = (Map *)h;
    double t0 = now_s();
    std::vector<V3> cloud(n);
    for (int64_t i = 0; i < n; ++i) cloud[i] = V3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    std::vector<XY> xy;
    size_t nh = 0, nf = 0;
    get_training_data(cloud, V3{origin[0], origin[1], origin[2]}, ds_resolution, free_res, max_range, xy, &nh, &nf,
                      m->p.variant == 1 ? -1.0f : 0.0f);
    m->st.n_hits = (double)nh; m->st.n_frees = (double)nf;
    m->st.t_frontend = now_s() - t0;
    insert_xy(*m, xy);
    m->st.t_total = now_s() - t0;
}
// BGKLOctoMap::insert_pointcloud, src/bgkloctomap/bgkloctomap.cpp:83-296
void orc_l_insert_pointcloud(void *h, const float *xyz, int64_t n, const float *origin, float ds_resolution, float free_res,
                             float max_range) {
    Map *m = (Map *)h;
    double t0 = now_s();
    std::vector<V3> cloud(n);
    for (int64_t i = 0; i < n; ++i) cloud[i] = V3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    std::vector<XY> xy;
    LData ld;
    get_training_data_l(cloud, V3{origin[0], origin[1], origin[2]}, ds_resolution, free_res, max_range, xy, ld);
    m->st.n_hits = (double)ld.rays.size();
    m->st.n_frees = (double)(xy.size() - ld.rays.size());
    m->st.t_frontend = now_s() - t0;
    insert_xy(*m, xy, &ld);
    m->st.t_total = now_s() - t0;
}
// training set of BGKLOctoMap: samples (x, y, z, ray index or -1) and rays (6 floats); counts via null pointers
int64_t orc_l_training_data(const float *xyz, int64_t n, const float *origin, float ds, float free_res, float max_range,
                            float *out_xyzr, int64_t cap, float *out_rays, int64_t cap_rays, int64_t *n_rays) {
    std::vector<V3> cloud(n);
    for (int64_t i = 0; i < n; ++i) cloud[i] = V3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    std::vector<XY> xy;
    LData ld;
    get_training_data_l(cloud, V3{origin[0], origin[1], origin[2]}, ds, free_res, max_range, xy, ld);
    if (out_xyzr)
        for (int64_t i = 0; i < std::min<int64_t>(cap, (int64_t)xy.size()); ++i) {
            out_xyzr[4 * i] = xy[i].p.x; out_xyzr[4 * i + 1] = xy[i].p.y; out_xyzr[4 * i + 2] = xy[i].p.z;
            out_xyzr[4 * i + 3] = (float)ld.ray_idx[i];
        }
    if (out_rays)
        for (int64_t i = 0; i < std::min<int64_t>(cap_rays, (int64_t)ld.rays.size()); ++i) {
            const Seg &sg = ld.rays[i];
            const float v[6] = {sg.a.x, sg.a.y, sg.a.z, sg.b.x, sg.b.y, sg.b.z};
            std::memcpy(out_rays + 6 * i, v, sizeof(v));
        }
    if (n_rays) *n_rays = (int64_t)ld.rays.size();
    return (int64_t)xy.size();
}
float orc_l_seg_dist(const float *p, const float *p0, const float *p1) {
    return seg_dist_l(V3{p[0], p[1], p[2]}, V3{p0[0], p0[1], p0[2]}, V3{p1[0], p1[1], p1[2]});
}
// BGKLInference::predict on bare arrays: M points xs, N rows of 6 floats (segment start, end) with labels y; the sums in the
// mode orc_set_sum_mode selects
void orc_l_predict(float sf2, float ell, const float *xs, int M, const float *rows6, const float *y, int N, float *ybar,
                   float *kbar) {
    std::vector<Seg> rows((size_t)N);
    for (int j = 0; j < N; ++j)
        rows[j] = Seg{V3{rows6[6 * j], rows6[6 * j + 1], rows6[6 * j + 2]}, V3{rows6[6 * j + 3], rows6[6 * j + 4], rows6[6 * j + 5]}};
    bgkl_predict(sf2, ell, xs, M, rows.data(), y, N, ybar, kbar);
}
// stages B..G on a prepared training set (x,y,z,label per point)
void orc_insert_training_data(void *h, const float *xyzy, int64_t n) {
    Map *m = (Map *)h;
    std::vector<XY> xy(n);
    double nh = 0;
    for (int64_t i = 0; i < n; ++i) {
        xy[i] = XY{V3{xyzy[4 * i], xyzy[4 * i + 1], xyzy[4 * i + 2]}, xyzy[4 * i + 3]};
        nh += xyzy[4 * i + 3] > 0.5f;
    }
    m->st.n_hits = nh; m->st.n_frees = (double)n - nh; m->st.t_frontend = 0;
    insert_xy(*m, xy, nullptr, true);
}
void orc_insert_xy(void *h, const float *xyzy, int64_t n) {
    Map *m = (Map *)h;
    double t0 = now_s();
    std::vector<XY> xy(n);
    double nh = 0;
    for (int64_t i = 0; i < n; ++i) {
        xy[i] = XY{V3{xyzy[4 * i], xyzy[4 * i + 1], xyzy[4 * i + 2]}, xyzy[4 * i + 3]};
        nh += xyzy[4 * i + 3] > 0.5f;
    }
    m->st.n_hits = nh; m->st.n_frees = (double)n - nh; m->st.t_frontend = 0;
    insert_xy(*m, xy);
    m->st.t_total = now_s() - t0;
}
void orc_stats(void *h, double *out15) { std::memcpy(out15, &((Map *)h)->st, sizeof(Stats)); }
int orc_num_threads() {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

int64_t orc_block_count(void *h) { return (int64_t)((Map *)h)->blocks.size(); }
int64_t orc_leaf_count(void *h) {
    Map *m = (Map *)h;
    int64_t n = 0;
    std::vector<int> keys;
    for (auto &kv : m->blocks) { enumerate_leaves(m->p, *kv.second, keys); n += (int64_t)keys.size(); }
    return n;
}
// Dump all leaves, blocks in ascending hash key, leaves in LeafIterator order.
int64_t orc_dump_leaves(void *h, int64_t *block_key, int32_t *node_key, float *loc_xyz, float *size, float *A,
                        float *B, uint8_t *state, uint8_t *classified, int64_t cap) {
    Map *m = (Map *)h;
    std::vector<int64_t> bk;
    for (auto &kv : m->blocks) bk.push_back(kv.first);
    std::sort(bk.begin(), bk.end());
    int64_t n = 0;
    std::vector<int> keys;
    for (int64_t key : bk) {
        Block *b = m->blocks[key];
        enumerate_leaves(m->p, *b, keys);
        for (int k : keys) {
            if (n >= cap) return n;
            const Node &nd = b->layer[k >> 16][k & 0xFFFF];
            const V3 &o = m->lut[k >> 16][k & 0xFFFF];
            block_key[n] = key; node_key[n] = k;
            loc_xyz[3 * n] = o.x + b->center.x; loc_xyz[3 * n + 1] = o.y + b->center.y; loc_xyz[3 * n + 2] = o.z + b->center.z;
            size[n] = float(m->p.block_size / pow(2, k >> 16));  // bgkblock.h:69-73
            A[n] = nd.A; B[n] = nd.B; state[n] = nd.state; classified[n] = nd.classified;
            ++n;
        }
    }
    return n;
}

// ---- leaf export: src/bgkoctomap/bgkoctomap_static_node.cpp:101-136 (the publish loop), get_bbox
// src/bgkoctomap/bgkoctomap.cpp:368-381, MarkerArrayPub::insert_point3d + heightMapColor
// include/common/markerarray_pub.h:21-147, get_pruned_locs include/bgkoctomap/bgkoctomap.h:269-287.
// Blocks in ascending hash key (the reference walks an unordered_map; a cube list has no order), leaves in
// LeafIterator order, expanded cells in the loop order x, y, z.
static void height_map_color(double h, float *rgba) {  // markerarray_pub.h:21-76
    double s = 1.0, v = 1.0;
    h -= floor(h);
    h *= 6;
    int i;
    double m, n, f;
    i = (int)floor(h);
    f = h - i;
    if (!(i & 1)) f = 1 - f;  // if i is even
    m = v * (1 - s);
    n = v * (1 - s * f);
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
    rgba[0] = (float)r; rgba[1] = (float)g; rgba[2] = (float)b; rgba[3] = 1.0f;
}
void orc_height_map_color(double h, float *rgba) { height_map_color(h, rgba); }

void orc_get_bbox(void *h, float *lo3, float *hi3) {
    Map *m = (Map *)h;
    for (int a = 0; a < 3; ++a) lo3[a] = hi3[a] = 0.0f;
    bool first = true;
    for (auto &kv : m->blocks) {
        const V3 &c = kv.second->center;
        const float v[3] = {c.x, c.y, c.z};
        for (int a = 0; a < 3; ++a) {
            if (first || v[a] < lo3[a]) lo3[a] = v[a];
            if (first || v[a] > hi3[a]) hi3[a] = v[a];
        }
        first = false;
    }
    if (!first) {
        const float half = m->p.block_size * 0.5f;  // point3f(block_size, ...) * 0.5  (point3f::operator*(float))
        for (int a = 0; a < 3; ++a) { lo3[a] -= half; hi3[a] += half; }
    }
}

int64_t orc_export_cells(void *h, int state, int original_size, float min_z, float max_z, float *cells, float *rgba,
                         int32_t *level, int64_t cap) {
    Map *m = (Map *)h;
    if (min_z == max_z) {  // static node :103-108
        float lo[3], hi[3];
        orc_get_bbox(h, lo, hi);
        min_z = lo[2];
        max_z = hi[2];
    }
    std::vector<int64_t> bk;
    for (auto &kv : m->blocks) bk.push_back(kv.first);
    std::sort(bk.begin(), bk.end());
    int64_t n = 0;
    auto insert = [&](float x, float y, float z, float size, const Node &nd) {
        if (n < cap) {
            cells[4 * n] = x; cells[4 * n + 1] = y; cells[4 * n + 2] = z; cells[4 * n + 3] = size;
            int depth = 0;
            if (size > 0) depth = (int)log2(size / m->p.resolution);
            level[n] = depth;
            float *c = rgba + 4 * n;
            c[0] = 0.0f; c[1] = 0.0f; c[2] = 1.0f; c[3] = 1.0f;  // marker default (ctor, :96-101)
            if (state == ST_OCCUPIED) {
                if (min_z < max_z) {
                    double hh = (1.0 - std::min(std::max((z - min_z) / (max_z - min_z), 0.0f), 1.0f)) * 0.8;
                    height_map_color(hh, c);
                }
            } else {
                const float prob = m->p.variant == 1 ? gp_node_prob(m->p, nd) : node_prob(nd);
                if (prob < 0.5) { c[0] = 0.8f; c[1] = 0.8f; c[2] = 0.8f; c[3] = 1.0f; }
                else height_map_color(std::min(2.0 - 2.0 * prob, 0.6), c);
            }
        }
        ++n;
    };
    std::vector<int> keys;
    for (int64_t key : bk) {
        Block *b = m->blocks[key];
        enumerate_leaves(m->p, *b, keys);
        for (int k : keys) {
            const Node &nd = b->layer[k >> 16][k & 0xFFFF];
            if ((int)nd.state != state) continue;
            const V3 &o = m->lut[k >> 16][k & 0xFFFF];
            const float cx = o.x + b->center.x, cy = o.y + b->center.y, cz = o.z + b->center.z;
            const float size = float(m->p.block_size / pow(2, k >> 16));
            if (original_size) {
                insert(cx, cy, cz, size, nd);
            } else {
                const float res = m->p.resolution;
                float x0 = cx - size * 0.5 + res * 0.5, y0 = cy - size * 0.5 + res * 0.5, z0 = cz - size * 0.5 + res * 0.5;
                float x1 = cx + size * 0.5, y1 = cy + size * 0.5, z1 = cz + size * 0.5;
                for (float x = x0; x < x1; x += res)
                    for (float y = y0; y < y1; y += res)
                        for (float z = z0; z < z1; z += res) insert(x, y, z, res, nd);
            }
        }
    }
    return n;
}

// ---- single-block access (known-answer tests against oracle/_ref) ----
void *orc_block_new(void *h, float cx, float cy, float cz) { return block_new(((Map *)h)->p, V3{cx, cy, cz}); }
void orc_block_free(void *b) { delete (Block *)b; }
int orc_block_leaves(void *h, void *b, int32_t *keys, float *loc_xyz, int cap) {
    Map *m = (Map *)h; Block *blk = (Block *)b;
    std::vector<int> k;
    enumerate_leaves(m->p, *blk, k);
    int n = (int)std::min<size_t>(k.size(), cap);
    for (int i = 0; i < n; ++i) {
        keys[i] = k[i];
        const V3 &o = m->lut[k[i] >> 16][k[i] & 0xFFFF];
        loc_xyz[3 * i] = o.x + blk->center.x; loc_xyz[3 * i + 1] = o.y + blk->center.y; loc_xyz[3 * i + 2] = o.z + blk->center.z;
    }
    return (int)k.size();
}
void orc_block_update(void *h, void *b, int32_t key, float ybar, float kbar) {
    node_update(((Map *)h)->p, ((Block *)b)->layer[key >> 16][key & 0xFFFF], ybar, kbar);
}
int orc_block_prune(void *h, void *b) { return block_prune(((Map *)h)->p, *(Block *)b); }
// returns 0 if the layer was deleted
int orc_block_node(void *b, int32_t key, float *A, float *B, uint8_t *state, uint8_t *classified) {
    Block *blk = (Block *)b;
    if (!blk->alive[key >> 16]) return 0;
    const Node &n = blk->layer[key >> 16][key & 0xFFFF];
    *A = n.A; *B = n.B; *state = n.state; *classified = n.classified;
    return 1;
}
// closed-box query on an arbitrary point set (R-tree inclusion rule KAT)
int orc_box_query(void *h, const float *xyz, int n, int64_t key, int32_t *ids, int cap) {
    Map *m = (Map *)h;
    V3 c = hash_key_to_block(m->p, key);
    int f = 0;
    for (int i = 0; i < n; ++i)
        if (in_closed_box(m->p, c, V3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]})) {
            if (f < cap) ids[f] = i;
            ++f;
        }
    return f;
}

// ---------------------------------------------------------------------------
// RayCaster: include/bgkoctomap/bgkoctomap.h:91-214 (voxel walk start -> end), on top of
// Block::get_index / get_node / get_point (src/bgkoctomap/bgkblock.cpp:131-150) and
// init_index_map (:34-67: finest-layer keys stably sorted by x, then y, then z of their LUT offsets).
// One output row per next() call; returns the number of calls until end().
// Deviation (documented in DESIGN.md): the reference never updates the static Block::cell_num after its
// static initialisation from the default statics (0.8 / 0.1 = 8, bgkblock.cpp:103-105 vs bgkoctomap.cpp:31-56),
// so its get_index() is only meaningful at block_depth 4; cell_num here is size / resolution, which is the
// same number at that depth (pinned by tests/golden/ref_kat_grid.npz).
// ---------------------------------------------------------------------------
// Block(center).get_index(p) -> cell, get_node -> key, get_point -> centre (bgkblock.cpp:131-150)
void orc_block_grid(void *h, const float *c3, const float *p3, int32_t *idx3, int32_t *node_key, float *point3) {
    Map *m = (Map *)h;
    const Params &P = m->p;
    const int dl = P.block_depth - 1, lim = 1 << dl;
    const int cell_num = (int)round(P.block_size / P.resolution);
    auto clip = [&](int a) { return std::max(0, std::min(a, cell_num - 1)); };
    for (int a = 0; a < 3; ++a) idx3[a] = clip((int)((p3[a] - c3[a]) / P.resolution + cell_num / 2));
    const std::vector<V3> &loc = m->lut[dl];
    std::vector<int> order(loc.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return loc[a].x < loc[b].x; });
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return loc[a].y < loc[b].y; });
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return loc[a].z < loc[b].z; });
    const int i = order[(size_t)idx3[0] + (size_t)idx3[1] * lim + (size_t)idx3[2] * lim * lim];
    *node_key = (dl << 16) + i;
    point3[0] = loc[i].x + c3[0]; point3[1] = loc[i].y + c3[1]; point3[2] = loc[i].z + c3[2];
}

int64_t orc_raycast(void *h, const float *s3, const float *e3, float *p_xyz, int64_t *block_key, int32_t *node_key,
                    uint8_t *valid, float *A, float *B, uint8_t *state, int64_t cap) {
    Map *m = (Map *)h;
    const Params &P = m->p;
    const int dl = P.block_depth - 1;
    const int lim = 1 << dl;
    // index_map: position in the (z, y, x)-sorted order of the finest layer -> node index
    std::vector<int> order((size_t)1 << (3 * dl));
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    const std::vector<V3> &loc = m->lut[dl];
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return loc[a].x < loc[b].x; });
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return loc[a].y < loc[b].y; });
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return loc[a].z < loc[b].z; });
    auto find_block = [&](int64_t key) -> Block * {
        auto it = m->blocks.find(key);
        return it == m->blocks.end() ? nullptr : it->second;
    };
    int64_t key = block_to_hash_key(P, s3[0], s3[1], s3[2]);
    Block *blk = find_block(key);
    if (blk == nullptr) return 0;
    const int cell_num = (int)round(P.block_size / P.resolution);
    auto clip = [&](int a) { return std::max(0, std::min(a, cell_num - 1)); };
    int x = clip((int)((s3[0] - blk->center.x) / P.resolution + cell_num / 2));
    int y = clip((int)((s3[1] - blk->center.y) / P.resolution + cell_num / 2));
    int z = clip((int)((s3[2] - blk->center.z) / P.resolution + cell_num / 2));
    V3 block_lim = blk->center, cur{s3[0], s3[1], s3[2]};
    const int x0 = (int)(s3[0] / P.resolution), y0 = (int)(s3[1] / P.resolution), z0 = (int)(s3[2] / P.resolution);
    const int x1 = (int)(e3[0] / P.resolution), y1 = (int)(e3[1] / P.resolution), z1 = (int)(e3[2] / P.resolution);
    int dx = abs(x1 - x0), dy = abs(y1 - y0), dz = abs(z1 - z0);
    int n = 1 + dx + dy + dz;
    const int x_inc = x1 > x0 ? 1 : (x1 == x0 ? 0 : -1), y_inc = y1 > y0 ? 1 : (y1 == y0 ? 0 : -1),
              z_inc = z1 > z0 ? 1 : (z1 == z0 ? 0 : -1);
    int xy_error = dx - dy, xz_error = dx - dz, yz_error = dy - dz;
    dx *= 2; dy *= 2; dz *= 2;
    int64_t rows = 0;
    while (n > 0) {
        const int nk = (dl << 16) + order[(size_t)x + (size_t)y * lim + (size_t)z * lim * lim];
        Node nd{0, P.prior_A, P.prior_B, ST_UNKNOWN};
        if (blk != nullptr) {
            nd = blk->layer[dl][nk & 0xFFFF];
            const V3 &o = loc[nk & 0xFFFF];
            cur = V3{o.x + blk->center.x, o.y + blk->center.y, o.z + blk->center.z};
        }
        if (rows < cap) {
            p_xyz[3 * rows] = cur.x; p_xyz[3 * rows + 1] = cur.y; p_xyz[3 * rows + 2] = cur.z;
            block_key[rows] = key; node_key[rows] = nk; valid[rows] = blk != nullptr;
            A[rows] = nd.A; B[rows] = nd.B; state[rows] = nd.state;
        }
        ++rows;
        auto cross = [&](float &lim_axis, int inc, int &i) {
            if (i >= lim || i < 0) {
                lim_axis += inc * P.block_size;
                key = block_to_hash_key(P, block_lim.x, block_lim.y, block_lim.z);
                blk = find_block(key);
                i = inc > 0 ? 0 : lim - 1;
            }
        };
        if (xy_error > 0 && xz_error > 0) {
            x += x_inc; cur.x += x_inc * P.resolution; xy_error -= dy; xz_error -= dz;
            cross(block_lim.x, x_inc, x);
        } else if (xy_error < 0 && yz_error > 0) {
            y += y_inc; cur.y += y_inc * P.resolution; xy_error += dx; yz_error -= dz;
            cross(block_lim.y, y_inc, y);
        } else if (yz_error < 0 && xz_error < 0) {
            z += z_inc; cur.z += z_inc * P.resolution; xz_error += dx; yz_error += dy;
            cross(block_lim.z, z_inc, z);
        } else if (xy_error == 0) {
            x += x_inc; y += y_inc; n -= 2;
            cur.x += x_inc * P.resolution; cur.y += y_inc * P.resolution;
            cross(block_lim.x, x_inc, x);
            cross(block_lim.y, y_inc, y);
        }
        --n;
    }
    return rows;
}

}  // extern "C"
