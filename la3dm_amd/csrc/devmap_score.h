// devmap_score.h — likelihood-field scoring of one scan under many poses on the device-resident map
// (la3dm_devmap_score_poses_*, include/la3dm_hip.h; host twin and definition: BGKOctoMap::score_poses,
// host/bgkoctomap.cpp).  Stage 1 is distance_field's launch chain (devmap_distance.h) into working storage; the kernels
// below are stage 2.  The transform and the point-to-voxel arithmetic are host/region_contract.h's inlines, compiled here
// as they are for the host form; everything after them is integers, so any reduction order gives the same answer.
//
// dm_score_pairs   one pose per workgroup and chunk (grid = n_poses x chunks, flattened): the pose's 12 floats are read
//                  at a wave-uniform address, the chunk's points coalesced, 256 a trip — every workgroup of a chunk reads
//                  the same points, so the cloud comes from cache after its first reader.  Each lane resolves its voxel,
//                  gathers the cost from distance_field's 32-bit words (a 16-bit copy of them was measured and is no
//                  faster: DESIGN.md 3.18) and keeps five counts and a 64-bit sum in registers; a wave folds them by
//                  shuffles, the four waves through LDS, and one lane writes the seven words — to the outputs when the
//                  pose has one chunk, else to the chunk's partial record.  No atomic: about 29 ns each on one address
//                   would serialise the waves of a pose.
// dm_score_fold    chunks > 1 (few poses, the machine filled by chunks of the cloud instead): one wave per pose adds the
//                  pose's partial records and writes the outputs.
//
// sum_d2 is written as two 32-bit words: a device pointer need only be 4-byte aligned.  The cost of a voxel is read through
// ObstacleField (devmap_distance.h): on the empty map it has no array, every voxel costs its `fill`, and the pool is not
// read.  Every loop is bounded by an argument.
#ifndef LA3DM_DEVMAP_SCORE_H
#define LA3DM_DEVMAP_SCORE_H

#include "devmap_distance.h"
#include "host/region_contract.h"

namespace la3dm_dev {

constexpr uint32_t kScoreWords = 8;   // words of a partial record: the five counts, the sum's low and high word, one unused

struct ScoreArgs {
    const float *points;    // 3 per point
    const float *poses;     // 12 per pose
    uint32_t n_points, n_poses;
    uint32_t chunks;        // workgroups per pose
    uint32_t per_chunk;     // points per chunk, a multiple of 256
    float resolution, block_size;
    int lim;                // cells of a block per axis
    uint32_t g0[3], dims[3];
    ObstacleField cost;     // the cost of a voxel: its d2 word (devmap_distance.h)
    uint32_t *partial;      // [n_poses chunks kScoreWords], chunks > 1
    uint32_t *sum_d2;       // [2 n_poses]: low word, high word
    uint32_t *counts;       // [5 n_poses] or null
};

// every lane ends with the wave's totals
__device__ __forceinline__ void score_wave_sum(uint32_t *c, unsigned long long &sum) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 5; ++k) c[k] += __shfl_xor(c[k], off);
        const uint32_t olo = __shfl_xor((uint32_t)sum, off), ohi = __shfl_xor((uint32_t)(sum >> 32), off);
        sum += ((unsigned long long)ohi << 32) | olo;
    }
}

// the seven words of a pose: to the outputs
__device__ __forceinline__ void score_write(const ScoreArgs &a, uint32_t pose, const uint32_t *c, unsigned long long sum) {
    a.sum_d2[2 * (size_t)pose] = (uint32_t)sum;
    a.sum_d2[2 * (size_t)pose + 1] = (uint32_t)(sum >> 32);
    if (a.counts)
        for (int k = 0; k < 5; ++k) a.counts[5 * (size_t)pose + k] = c[k];
}

__global__ __launch_bounds__(256) void dm_score_pairs(ScoreArgs a) {
    __shared__ uint32_t fold[4][kScoreWords];
    const uint32_t pose = blockIdx.x / a.chunks, chunk = blockIdx.x - pose * a.chunks;
    const float *P = a.poses + 12 * (size_t)pose;   // wave-uniform
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = P[k];
    const uint32_t begin = chunk * a.per_chunk, end = min(begin + a.per_chunk, a.n_points);   // (n_points <= 2^20: no overflow)
    uint32_t c[5] = {0, 0, 0, 0, 0};
    unsigned long long sum = 0;
    for (uint32_t i = begin + threadIdx.x; i < end; i += 256u) {   // at most per_chunk / 256 trips
        const float *q = a.points + 3 * (size_t)i;
        uint32_t f = 0;
        uint32_t cls = la3dm_region::score_voxel(T, q[0], q[1], q[2], a.resolution, a.block_size, a.lim, a.g0, a.dims, f);
        if (cls == LA3DM_SCORE_HIT) {
            const uint32_t v = a.cost.at(f);
            cls = la3dm_region::score_class(v);
            sum += cls != LA3DM_SCORE_FAR ? v : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) c[k] += cls == k ? 1u : 0u;   // (no runtime-indexed array: registers)
    }
    score_wave_sum(c, sum);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < 5; ++k) fold[wave][k] = c[k];
        fold[wave][5] = (uint32_t)sum;
        fold[wave][6] = (uint32_t)(sum >> 32);
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    unsigned long long total = 0;
    for (int w = 0; w < 4; ++w) {
        if (w > 0)
            for (int k = 0; k < 5; ++k) c[k] += fold[w][k];
        total += ((unsigned long long)fold[w][6] << 32) | fold[w][5];
    }
    if (a.chunks == 1u) {
        score_write(a, pose, c, total);
        return;
    }
    uint32_t *rec = a.partial + kScoreWords * (size_t)blockIdx.x;
    for (int k = 0; k < 5; ++k) rec[k] = c[k];
    rec[5] = (uint32_t)total;
    rec[6] = (uint32_t)(total >> 32);
}

// one wave per pose: the sum of its `chunks` partial records
__global__ __launch_bounds__(64) void dm_score_fold(ScoreArgs a) {
    const uint32_t pose = blockIdx.x;
    uint32_t c[5] = {0, 0, 0, 0, 0};
    unsigned long long sum = 0;
    for (uint32_t ch = threadIdx.x; ch < a.chunks; ch += 64u) {   // at most chunks / 64 + 1 trips
        const uint32_t *rec = a.partial + kScoreWords * ((size_t)pose * a.chunks + ch);
#pragma unroll
        for (int k = 0; k < 5; ++k) c[k] += rec[k];
        sum += ((unsigned long long)rec[6] << 32) | rec[5];
    }
    score_wave_sum(c, sum);
    if (threadIdx.x == 0u) score_write(a, pose, c, sum);
}

}  // namespace la3dm_dev

#endif
