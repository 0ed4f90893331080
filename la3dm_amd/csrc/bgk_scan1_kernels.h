// bgk_scan1_kernels.h — the BGK predict + fuse scan of full blocks in ONE launch (block_depth 3, bgk_sum 1, tables).
//
// bgk_predict_fuse_t1 is a COPY of bgk_predict_fuse_t<kTrig, false> (bgk_kernels.h) with the work of the bgk_prepare
// launch folded in: it reads the caller's unscaled training points and divides them by ell as it stages them, and it
// forms the descriptor of the 7 neighbour ranges from nbr / train_off in its own prologue.  It stands beside the
// original, in a header of its own, for one reason only: bgk_kernels.h belongs to the source closure that the counter
// files under profiles/ are stamped with (tests/test_profiles_stamps_cpu.py), so no line of it can change without
// recording all three counter files again.  The pull request that records them again ("BGK scan: merge
// bgk_predict_fuse_t1 into bgk_kernels.h and re-stamp the counter files") folds this kernel back into
// bgk_predict_fuse_t and deletes this header.  Until then: a change to the table path of one kernel belongs in the other too.
// The exceptions, all of them bookkeeping round the same arithmetic (profiles/one_launch_trim/README.md), which the merge
// carries over: (1) the correctly rounded evaluation (kTrig 0) is a copy here, scan1_sincos_cr_eval / scan1_cov, that takes
// the four constant addends of its polynomials from vcc instead of four SGPR pairs; (2) alpha, beta, state and the stamp
// record are read again from the kernarg segment on the way out (scan1_arg_again) instead of being carried through the
// body; (3) the column groups of a table sub-round are eight trips with immediate offsets, not a loop that moves the
// three row addresses; (4) the cull's masks are the ballots of its three compares, joined on the scalar side; (5) the tile
// body has a second, "production" instance (bgk_scan1_tile<0, true>, profiles/one_launch_special/README.md) with what the host
// has verified for the launch compiled in — depth 3 and one tile per block (no leaf_off load, no full-block compare, the LUT
// index a literal minus the lane), remap 2, inv_ell != 0 (div_const without div_by_ell's branch), sf2 == 1 (no multiply:
// scan1_cov_unit, which also forms t = 2 pi r in one multiply), a gated scan, no ablation switch — and with the last column
// group of a sub-round, where it is not full, through a trip that pushes its candidates only (LA3DM_SCAN1_PAD_TRIP; the table
// is not padded).  The merge carries the instance over as a template parameter of bgk_predict_fuse_t.
//
// Everything else — device functions, the LA3DM_TP_* macros, WaveLdsT, the ablation flags — is bgk_kernels.h's, used
// from here (include this header after it).  One difference in the table path: this kernel notes a training point at no
// finite distance while it stages it and answers as the reference does (NaN sums); the two-launch kernels get the same
// answer from bgk_poison_nbr (la3dm_hip.hip), which edits the neighbour table ahead of them.  Same pairs, same fp32 terms in the same order: alpha, beta and state are
// bit-identical to the two-launch path (tests/test_bgk_one_launch_gpu.py).
#pragma once
#include "bgk_kernels.h"

namespace la3dm_dev {

// v_fma_f64 d = a * b + CONSTANT with the constant in no register of the kernel's: its two words are moved into vcc right
// ahead of the instruction (LO, HI: string literals).  fma64_sc (bgk_kernels.h) keeps each addend in an SGPR pair for the whole
// tile — eight scalar registers that this kernel, at 78 SGPRs, pays for with scalars parked in lanes of a VGPR (a
// v_writelane / v_readlane each, on the unit that bounds the kernel); two s_mov_b32 per use go to the scalar unit, which has
// room.  A scalar write of vcc followed by a vector read of it as a constant needs no wait state on gfx9 (the table of the
// ISA manual lists only VALU writers of an SGPR); the s_nop is there because the compiler pads nothing inside a statement.
#define LA3DM_FMA64_VCC(D, A, B, LO, HI)                                                             \
    asm("s_mov_b32 vcc_lo, " LO "\n"                                                                 \
        "s_mov_b32 vcc_hi, " HI "\n"                                                                 \
        "s_nop 0\n"                                                                                  \
        "v_fma_f64 %0, %1, %2, vcc\n" : "=v"(D) : "v"(A), "v"(B) : "vcc")

// sincos_cr_eval of bgk_kernels.h — the same operations on the same constants in the same order — with the four constant
// addends taken from vcc (tests/test_bgk_one_launch_trim_gpu.py compares the words with the original's)
__device__ __forceinline__ void scan1_sincos_cr_eval(float y32, double sa, double ca, float &s, float &c) {
    const double y = (double)y32;
    const double z = y * y;
    const double s3 = __builtin_bit_cast(double, 0xbf2a014a5f1de813ull), c3 = __builtin_bit_cast(double, 0x3efa015b846c26deull);
    double ps, pc;
    LA3DM_FMA64_VCC(ps, z, s3, "0x10c194d4", "0x3f811111");   // 0x3f81111110c194d4
    LA3DM_FMA64_VCC(pc, z, c3, "0x1681d56a", "0xbf56c16c");   // 0xbf56c16c1681d56a
    const double zy = z * y;
    LA3DM_FMA64_VCC(ps, z, ps, "0x5555552a", "0xbfc55555");   // 0xbfc555555555552a
    LA3DM_FMA64_VCC(pc, z, pc, "0x55555544", "0x3fa55555");   // 0x3fa5555555555544
    const double sy = __builtin_fma(zy, ps, y);      // sin y
    pc = __builtin_fma(z, pc, -0.5);
    const double cm1 = z * pc;                       // cos y - 1
    const double sd = __builtin_fma(ca, sy, __builtin_fma(sa, cm1, sa));
    const double cd = __builtin_fma(-sa, sy, __builtin_fma(ca, cm1, ca));
    s = (float)sd;
    c = (float)cd;
}
// cov_sparse_fast<kTrig, true, true> (bgk_kernels.h); the correctly rounded instance (kTrig 0) through the evaluation above
template <int kTrig>
__device__ __forceinline__ float scan1_cov(float r, float sf2) {
    if (kTrig != 0) return cov_sparse_fast<kTrig, true, true>(r, sf2);
    const float t = (r * 2.0f) * 3.1415926f;
    float y32, s, c;
    const la3dm_v2d e = sincos_cr_entry(sincos_cr_reduce(t, y32));
    scan1_sincos_cr_eval(y32, e.x, e.y, s, c);
    return cov_sparse_formula<true>(r, s, c, sf2);
}
// scan1_cov<0> of a map whose sf2 is 1.0f (the production instance below), two instructions shorter per pair, same bits:
//  * t = (r * 2.0f) * 3.1415926f is r * 6.2831852f.  r * 2 is exact for every r,
//    and 2 * RN(3.1415926) = 0x40c90fda is a float, the one the literal 6.2831852f rounds to (tests/test_bgk_one_launch_special_gpu.py
//    reads the literal here and sweeps both forms): both forms round the same real product r * 0x1.921fb4p+2 once.
//  * (a + b) * sf2 at sf2 == 1.0f is a + b, for every value including -0 and NaN; the compiler keeps the multiply (no fast-math).
__device__ __forceinline__ float scan1_cov_unit(float r) {
    const float t = r * 6.2831852f;
    float y32, s, c;
    const la3dm_v2d e = sincos_cr_entry(sincos_cr_reduce(t, y32));
    scan1_sincos_cr_eval(y32, e.x, e.y, s, c);
    const float a = div_const((2.0f + c) * (1.0f - r), 3.0f, 0.333333343f);   // cov_sparse_formula<true> (bgk_kernels.h) from here on
    const float b = div_const(s, 2.0f * 3.1415926f, 0.159154952f);
    return fmaxf(a + b, 0.0f);
}

// The last column group of a table sub-round when it holds fewer than four candidates (production instance): LA3DM_TP_TRIP
// with the pushes of the slots that hold no candidate left out — NP = 1, 2 or 3 pushes, a scalar — and no fourth compare.
// The ring gets the entries LA3DM_TP_TRIP gives it from a group padded with candidates out of every leaf's reach, in the same order.
#define LA3DM_SCAN1_PAD_TRIP(OFF)                                                                   \
    asm volatile("ds_read_b128 v[52:55], %[ax] offset:" OFF "\n"                                    \
                 "ds_read_b128 v[56:59], %[ay] offset:" OFF "\n"                                    \
                 "ds_read_b128 v[60:63], %[az] offset:" OFF "\n"                                    \
                 "s_waitcnt lgkmcnt(0)\n"                                                           \
                 "v_pk_add_f32 v[56:57], v[56:57], v[60:61]\n"                                      \
                 "v_pk_add_f32 v[58:59], v[58:59], v[62:63]\n"                                      \
                 "s_nop 0\n"                                                                        \
                 "v_pk_add_f32 v[52:53], v[52:53], v[56:57]\n"                                      \
                 "v_pk_add_f32 v[54:55], v[54:55], v[58:59]\n"                                      \
                 "s_nop 0\n"                                                                        \
                 "v_cmp_gt_f32_e64 %[m0], %[T], |v52|\n"                                            \
                 "v_cmp_gt_f32_e64 %[m1], %[T], |v53|\n"                                            \
                 "v_cmp_gt_f32_e64 %[m2], %[T], |v54|\n"                                            \
                 LA3DM_TP_PUSH("v52", "%[m0]")                                                      \
                 "s_cmp_lt_u32 %[np], 2\n"                                                          \
                 "s_cbranch_scc1 .Lscan1_pad_%=\n"                                                  \
                 LA3DM_TP_PUSH("v53", "%[m1]")                                                      \
                 "s_cmp_lt_u32 %[np], 3\n"                                                          \
                 "s_cbranch_scc1 .Lscan1_pad_%=\n"                                                  \
                 LA3DM_TP_PUSH("v54", "%[m2]")                                                      \
                 ".Lscan1_pad_%=:\n"                                                                \
                 "s_mov_b64 exec, -1\n"                                                             \
                 : [tail] "+s"(tailb), [tr] "=&v"(tr), [st] "=&s"(st), [m0] "=&s"(hm0), [m1] "=&s"(hm1), [m2] "=&s"(hm2) \
                 : [ax] "v"(aX), [ay] "v"(aY), [az] "v"(aZ), [T] "s"(hit_t), [w] "v"(w0), [np] "s"(np) \
                 : "scc", "memory", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63")

// A pointer argument read AGAIN from the kernarg segment, at the place that needs it (the statement is volatile: it stays
// there).  alpha, beta, state and the stamp record are needed on the way out of a tile only; carried through the body they
// were eight and more scalars parked in lanes of a VGPR, a v_writelane going in and a v_readlane coming out each.  BgkArgs is
// the kernel's first argument: its members sit at their offsets in the segment.
template <class T, int kOff>
__device__ __forceinline__ T *scan1_arg_again() {
    T *p;
    asm volatile("s_load_dwordx2 %0, %1, %2\n"
                 "s_waitcnt lgkmcnt(0)\n" : "=&s"(p) : "s"(__builtin_amdgcn_kernarg_segment_ptr()), "i"(kOff));
    return p;
}

// BgkArgs as bgk_predict_fuse_t takes them, except: pts = the caller's UNSCALED points (x, y, z, label); blk_desc,
// nbr_range and label_seq are not read.  Full blocks only (the host verifies it from the leaf count), tpb_shift 0 or more,
// one descriptor per block (desc_shift is not read: the host takes this path at block_depth 3 only).
//
// kProd: the instance for the scan this kernel runs in production — what la3dm_bgk_scan_device has verified for the launch or
// what la3dm_create fixed for the map is compiled in instead of carried in scalar registers and tested per tile, chunk,
// sub-round or batch.  The host picks it when, beside the conditions of the one launch (block_depth 3, hence tpb_shift 0: a
// tile is a block, task == blk, 64 leaves, leaf_off[blk] == 64 * blk; one workgroup per tile: gridDim.x == n_tasks), all of
// these hold: kTrig 0, inv_ell != 0, sf2 == 1.0f, remap 2, no ablation switch, no extra LDS, a gated scan.  Same pairs, same
// fp32 terms, same ring contents at every flush, hence the same order of a leaf's double additions: same bits.
template <int kTrig, bool kProd = false>
__device__ __forceinline__ void bgk_scan1_tile(BgkArgs a) {
    static_assert(!kProd || kTrig == 0, "the production instance is the correctly rounded evaluation");
    __shared__ __attribute__((aligned(16))) unsigned char s_lds[5120];
    uint32_t task;
    if (kProd) {  // bgk_task_of_workgroup at remap 2; every workgroup of the grid has a tile
        uint32_t wg = blockIdx.x;
        if (wg < (gridDim.x & ~63u)) wg = (wg & ~63u) | ((wg & 7u) << 3) | ((wg >> 3) & 7u);
        task = __builtin_amdgcn_readfirstlane(wg);
    } else {
        task = bgk_task_of_workgroup(a);
        if (task >= a.n_tasks) return;
    }
    const uint32_t blk = kProd ? task : task >> a.tpb_shift;
    // the block's scalar inputs — leaf range, the 7 neighbour indices, centre — in one round trip.  The row of a block is
    // 7 words at a 4-byte-aligned address and the last block's row ends the array: 4 + 2 + 1 words, never word 7.
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x4 n03;
    u32x2 n45, lbr;
    uint32_t n6;
    float cx, cy, cz;
    if (kProd)   // the block's leaves are [64 * blk, 64 * blk + 64): nothing to load, nothing to compare
        asm("s_load_dwordx4 %[n03], %[nr], 0x0\n"
            "s_load_dwordx2 %[n45], %[nr], 0x10\n"
            "s_load_dword %[n6], %[nr], 0x18\n"
            "s_load_dword %[cx], %[ctr], 0x0\n"
            "s_load_dword %[cy], %[ctr], 0x4\n"
            "s_load_dword %[cz], %[ctr], 0x8\n"
            "s_waitcnt lgkmcnt(0)\n"
            : [n03] "=&s"(n03), [n45] "=&s"(n45), [n6] "=&s"(n6), [cx] "=&s"(cx), [cy] "=&s"(cy), [cz] "=&s"(cz)
            : [nr] "s"(a.nbr + 7 * (size_t)blk), [ctr] "s"(a.blk_center + 3 * (size_t)blk));
    else
    asm("s_load_dwordx2 %[lb], %[lop], 0x0\n"
        "s_load_dwordx4 %[n03], %[nr], 0x0\n"
        "s_load_dwordx2 %[n45], %[nr], 0x10\n"
        "s_load_dword %[n6], %[nr], 0x18\n"
        "s_load_dword %[cx], %[ctr], 0x0\n"
        "s_load_dword %[cy], %[ctr], 0x4\n"
        "s_load_dword %[cz], %[ctr], 0x8\n"
        "s_waitcnt lgkmcnt(0)\n"
        : [lb] "=&s"(lbr), [n03] "=&s"(n03), [n45] "=&s"(n45), [n6] "=&s"(n6), [cx] "=&s"(cx), [cy] "=&s"(cy), [cz] "=&s"(cz)
        : [lop] "s"(a.leaf_off + blk), [nr] "s"(a.nbr + 7 * (size_t)blk), [ctr] "s"(a.blk_center + 3 * (size_t)blk));
    const uint32_t lb0 = kProd ? blk << 6 : lbr[0];
    if (!kProd && lbr[1] - lb0 != 1u << (3u * (a.depth - 1u))) return;  // (the host vouched for full blocks: a tile that is not is left untouched)
    // second round trip: train_off[tb], train_off[tb + 1] of every neighbour that exists (tb < 0: the block's leaf range is
    // read instead — two words that are always there, train_off may hold a single one — and dropped; the production instance
    // keeps this stand-in although it no longer reads the range: leaf_off has n_test_blk + 1 words whatever n_train_blk is), then bgk_prepare's
    // thirteen words at shift 0 in scalar registers: adj[b] = first point of neighbour b minus the flat index where b starts, pend[b] = flat index where b ends, M = pend[6]
    uint32_t adj[7], pend[7];
    {
        const int32_t tb[7] = {(int32_t)n03[0], (int32_t)n03[1], (int32_t)n03[2], (int32_t)n03[3], (int32_t)n45[0], (int32_t)n45[1], (int32_t)n6};
        u32x2 r[7];
        auto pair = [&](int b) { return tb[b] >= 0 ? a.train_off + tb[b] : a.leaf_off + blk; };
        asm("s_load_dwordx2 %0, %7, 0x0\n"
            "s_load_dwordx2 %1, %8, 0x0\n"
            "s_load_dwordx2 %2, %9, 0x0\n"
            "s_load_dwordx2 %3, %10, 0x0\n"
            "s_load_dwordx2 %4, %11, 0x0\n"
            "s_load_dwordx2 %5, %12, 0x0\n"
            "s_load_dwordx2 %6, %13, 0x0\n"
            "s_waitcnt lgkmcnt(0)\n"
            : "=&s"(r[0]), "=&s"(r[1]), "=&s"(r[2]), "=&s"(r[3]), "=&s"(r[4]), "=&s"(r[5]), "=&s"(r[6])
            : "s"(pair(0)), "s"(pair(1)), "s"(pair(2)), "s"(pair(3)), "s"(pair(4)), "s"(pair(5)), "s"(pair(6)));
        uint32_t pre = 0;
#pragma unroll
        for (int b = 0; b < 7; ++b) {
            const uint32_t first = tb[b] >= 0 ? r[b][0] : 0u, cnt = tb[b] >= 0 ? r[b][1] - r[b][0] : 0u;
            adj[b] = first - pre;
            pre += cnt;
            pend[b] = pre;
        }
    }
    const uint32_t M = pend[6];
    WaveLdsT &L = *reinterpret_cast<WaveLdsT *>(s_lds);
    const uint32_t lane = threadIdx.x;
    const uint32_t tile = kProd ? 0u : task & ((1u << a.tpb_shift) - 1u);
    const uint32_t li = lb0 + tile * kWave + lane;
    // LeafIterator order is descending: the leaf at list position j of a full block has the finest-level index
    // 8^(depth-1) - 1 - j, so the key needs no load
    const uint32_t n_fine = kProd ? 64u : 1u << (3u * (a.depth - 1u));
    const uint32_t lut_idx = (kProd ? lut_layer_base(2u) : lut_layer_base(a.depth - 1u)) + (n_fine - 1u - tile * kWave) - lane;
    // x / ell: the production instance runs only where inv_ell != 0, div_by_ell without its branch
    auto by_ell = [&](float x) { return kProd ? div_const(x, a.ell, a.inv_ell) : div_by_ell(x, a.ell, a.inv_ell); };

    // the UNSCALED points of flat indices cb + lane (chunk() divides them by ell); a lane past the end reads the range's
    // last point (the caller masks it).  The descriptor stays in scalar registers for the whole tile; its offsets are
    // copied to VGPRs per call (a v_cndmask reads one scalar operand, and its mask is one).
    auto gather = [&](uint32_t cb) {
        uint32_t adjv[7];
#pragma unroll
        for (int b = 0; b < 7; ++b) {
            adjv[b] = adj[b];
            asm volatile("" : "+v"(adjv[b]));
        }
        const uint32_t f = min(cb + lane, M - 1u);
        uint32_t ad;
        unsigned long long m1, m2, m3, m4, m5, m6;
        asm("v_cmp_le_u32 %[m1], %[e0], %[f]\n"
            "v_cmp_le_u32 %[m2], %[e1], %[f]\n"
            "v_cmp_le_u32 %[m3], %[e2], %[f]\n"
            "v_cmp_le_u32 %[m4], %[e3], %[f]\n"
            "v_cmp_le_u32 %[m5], %[e4], %[f]\n"
            "v_cmp_le_u32 %[m6], %[e5], %[f]\n"
            "v_cndmask_b32 %[ad], %[a0], %[a1], %[m1]\n"
            "v_cndmask_b32 %[ad], %[ad], %[a2], %[m2]\n"
            "v_cndmask_b32 %[ad], %[ad], %[a3], %[m3]\n"
            "v_cndmask_b32 %[ad], %[ad], %[a4], %[m4]\n"
            "v_cndmask_b32 %[ad], %[ad], %[a5], %[m5]\n"
            "v_cndmask_b32 %[ad], %[ad], %[a6], %[m6]\n"
            : [ad] "=&v"(ad), [m1] "=&s"(m1), [m2] "=&s"(m2), [m3] "=&s"(m3), [m4] "=&s"(m4), [m5] "=&s"(m5), [m6] "=&s"(m6)
            : [f] "v"(f), [e0] "s"(pend[0]), [e1] "s"(pend[1]), [e2] "s"(pend[2]), [e3] "s"(pend[3]), [e4] "s"(pend[4]),
              [e5] "s"(pend[5]), [a0] "v"(adjv[0]), [a1] "v"(adjv[1]), [a2] "v"(adjv[2]), [a3] "v"(adjv[3]), [a4] "v"(adjv[4]),
              [a5] "v"(adjv[5]), [a6] "v"(adjv[6]));
        return a.pts[f + ad];
    };
#if LA3DM_T_EARLY_AB
    const float A0 = a.alpha[li], B0 = a.beta[li];  // needed by the epilogue only: loaded here, a round trip off the tile's tail
#endif
    if (M == 0u) {  // no training point in the 7 blocks: nothing reaches the tile
        uint8_t *const state = scan1_arg_again<uint8_t, offsetof(BgkArgs, state)>();
        if (kProd || !(a.flags & 1u)) state[li] = 0;
        else {  // insert_training_data: update() runs with (0, 0)
#if LA3DM_T_EARLY_AB
            const float A = A0, B = B0;
#else
            const float A = a.alpha[li], B = a.beta[li];
#endif
            state[li] = (uint8_t)(classify(A, B, a) | 0x80u);
        }
        return;
    }
    float4 pc = gather(0), pn = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (M > (uint32_t)kWave) pn = gather(kWave);

    const float4 off4 = a.lut[lut_idx];
    const float xs0 = by_ell(off4.x + cx), ys0 = by_ell(off4.y + cy), zs0 = by_ell(off4.z + cz);
    L.acc0[lane] = 0.0;
    L.acc1[lane] = 0.0;

    // the four coordinates per axis.  Lane l holds leaf index c = 63 - l of the cube; c = (i1 j1 k1 i0 j0 k0) in binary:
    // child number i*4 + j*2 + k at the parent level (bits 5-3) and at the leaf level (bits 2-0).
    // Axis value r = 2 * (high bit) + (low bit); the lanes read below have the other two axes' bits clear.
    auto rl = [](float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
    const la3dm_v2f X01 = {rl(xs0, 63), rl(xs0, 59)}, X23 = {rl(xs0, 31), rl(xs0, 27)};
    const la3dm_v2f Y01 = {rl(ys0, 63), rl(ys0, 61)}, Y23 = {rl(ys0, 47), rl(ys0, 45)};
    const la3dm_v2f Z01 = {rl(zs0, 63), rl(zs0, 62)}, Z23 = {rl(zs0, 55), rl(zs0, 54)};
    const uint32_t c6 = lane ^ 63u;
    const uint32_t ix = ((c6 >> 4) & 2u) | ((c6 >> 2) & 1u), iy = ((c6 >> 3) & 2u) | ((c6 >> 1) & 1u), iz = ((c6 >> 2) & 2u) | (c6 & 1u);
    const uint32_t tab_base = (uint32_t)(uintptr_t)&L.tab[0][0][0];
    constexpr uint32_t kRowB = 4u * 16u, kHalfB = 12u * kRowB;
    static_assert(kTabSlots == 32, "the B loop below walks two halves of 16 slots");
    const uint32_t ax0 = tab_base + ix * kRowB, ay0 = tab_base + (4u + iy) * kRowB, az0 = tab_base + (8u + iz) * kRowB;
    const uint32_t ring_base = (uint32_t)(uintptr_t)&L.ring[0];
    const uint32_t w0 = (uint32_t)(uintptr_t)&L.acc0[0] + 8u * lane;
    if (w0 & 0x200u) __builtin_trap();   // (s_lds is the kernel's only static LDS object: it starts at LDS address 0)
    static_assert(offsetof(WaveLdsT, acc1) - offsetof(WaveLdsT, acc0) == 512, "c_eval adds 512 to the address of acc0[leaf] for a label-1 pair");
    const float hit_t = __uint_as_float(kHitTBits);
    const uint32_t tail_cap = ring_base + 8u * (uint32_t)(kRingT - 4 * kWave);
    uint32_t tailb = ring_base;  // LDS byte address of the ring's first free entry

    // C: lane evaluates ring entry i and adds k to the leaf's accumulator 0 or 1 (the sign of d2 is the label)
    auto c_eval = [&](uint32_t i) {
        const uint2 e = L.ring[i];
        const float r = sqrt_cr(__builtin_fabsf(__uint_as_float(e.x)));
        const float kv = kProd ? scan1_cov_unit(r) : scan1_cov<kTrig>(r, a.sf2);
        const double kd = (double)kv;
        const uint32_t ad = e.y | ((e.x >> 22) & 0x200u);  // label 1 (negative d2): acc1[leaf], 512 bytes up
        asm volatile("ds_add_f64 %0, %1\n" : : "v"(ad), "v"(kd) : "memory");
    };
    // C round: the full 64-entry batches, taken from the ring's END so that the remainder (< 64 entries) stays at the front
    auto c_flush = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t tail = (tailb - ring_base) >> 3;
        const uint32_t rem = tail & 63u;
        if (kProd || !(a.flags & 0x100u))  // 0x100: profiling ablation
            for (uint32_t p = rem; p < tail; p += kWave) c_eval(p + lane);
        tailb = ring_base + 8u * rem;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };

    unsigned long long nonfinite = 0ull;  // lanes whose point, in some chunk, lay at no finite distance (wave-uniform)
    // A + B for one chunk of 64 training points (lane = point)
    auto chunk = [&](const float4 &pu, const uint32_t cb) {
        // x / ell, y / ell, z / ell as bgk_prepare's IEEE divisions leave them (div_by_ell is the correctly rounded quotient;
        // a zero may come out with the other sign, which the squares below remove); the label is untouched
        const float px = by_ell(pu.x), py = by_ell(pu.y), pz = by_ell(pu.z);
        const la3dm_v2f bx = {px, px}, by = {py, py}, bz = {pz, pz};
        la3dm_v2f x01 = bx - X01, x23 = bx - X23, y01 = by - Y01, y23 = by - Y23, z01 = bz - Z01, z23 = bz - Z23;
        x01 *= x01, x23 *= x23, y01 *= y01, y23 *= y23, z01 *= z01, z23 *= z23;
        const float mx = fminf(fminf(x01.x, x01.y), fminf(x23.x, x23.y));
        const float my = fminf(fminf(y01.x, y01.y), fminf(y23.x, y23.y));
        const float mz = fminf(fminf(z01.x, z01.y), fminf(z23.x, z23.y));
        // min over the 64 leaves of d2 (+ and * are monotone): staged iff some leaf hits (lanes past the end hold a
        // copy of the last point: masked)
        const float md = mx + (my + mz);
        const bool keep = md < hit_t && cb + lane < M;
        // a point at no finite distance (a NaN coordinate, an overflowing square): the reference's kernel matrix holds NaN in
        // its column, the sums of every leaf are NaN and `kbar > 0` rejects the update (see bgk_poison_nbr in la3dm_hip.hip)
        // (the masks from the three compares' own ballots, joined on the scalar side: the ballot of a conjunction is rebuilt
        // from a 0 / 1 value per lane, a v_cndmask and a v_cmp each)
        const unsigned long long live = __ballot(cb + lane < M);
        nonfinite |= __ballot(!(md < __builtin_inff())) & live;
        const unsigned long long m = __ballot(md < hit_t) & live;
        if (m == 0ull) return;
        const float sg = 1.0f - (pu.w + pu.w);  // label 0 -> +1, label 1 -> -1 (exact)
        const la3dm_v2f s2 = {sg, sg};
        x01 *= s2, x23 *= s2, y01 *= s2, y23 *= s2, z01 *= s2, z23 *= s2;
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
        const uint32_t n = (uint32_t)__popcll(m);
        for (uint32_t base = 0; base < n; base += kTabSlots) {
            const uint32_t nr = min(n - base, (uint32_t)kTabSlots), ngroup = (nr + 3u) >> 2;
            // pad the last column group with entries no leaf can reach (an X row suffices: the sum stays huge or NaN); the
            // production instance pushes nothing from those slots (LA3DM_SCAN1_PAD_TRIP) and leaves them as they are
            if (!kProd && lane < 4u && nr + lane < 4u * ngroup) {
                float big;
                asm volatile("v_mov_b32 %0, 0x5e268890" : "=v"(big));
#pragma unroll
                for (int r = 0; r < 4; ++r) L.tab[(nr + lane) >> 4][r][(nr + lane) & 15u] = big;
            }
            const uint32_t slot = rank - base;
            if (keep && slot < (uint32_t)kTabSlots) {
                float(&T)[12][16] = L.tab[slot >> 4];
                const uint32_t c = slot & 15u;
                T[0][c] = x01.x, T[1][c] = x01.y, T[2][c] = x23.x, T[3][c] = x23.y;
                T[4][c] = y01.x, T[5][c] = y01.y, T[6][c] = y23.x, T[7][c] = y23.y;
                T[8][c] = z01.x, T[9][c] = z01.y, T[10][c] = z23.x, T[11][c] = z23.y;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (!kProd && (a.flags & 0x200u)) continue;  // 0x200: profiling ablation
            // one trip per column group, the group's place in the table as the immediate offset of its three reads (groups
            // 0-3 sit in the first half, 4-7 kHalfB = 768 bytes up in the second): the lane's three row addresses never move.
            // The ring is tested after every trip, as before: a trip pushes up to 4 x 64 entries, which is the head room
            // tail_cap leaves.  Eight trips are eight copies of the C round in the code (a loop over g with the trips behind
            // a switch or an if-chain, which would share one, does not compile: "illegal VGPR to SGPR copy" where the
            // trips' scalar outputs meet); a copy that is not entered costs the branch round it, as the loop's two did.
            const uint32_t aX = ax0, aY = ay0, aZ = az0;
            static_assert(kHalfB == 768u, "the immediates below");
            if (!kProd) {
#define LA3DM_SCAN1_GROUP(G, OFF)                   \
    if (G < ngroup) {                               \
        uint32_t st;                                \
        float tr;                                   \
        unsigned long long hm0, hm1, hm2, hm3;      \
        LA3DM_TP_TRIP(OFF);                         \
        if (tailb > tail_cap) c_flush();
            // (nested, so that the last group of a sub-round leaves through one branch)
            LA3DM_SCAN1_GROUP(0u, "0")
            LA3DM_SCAN1_GROUP(1u, "16")
            LA3DM_SCAN1_GROUP(2u, "32")
            LA3DM_SCAN1_GROUP(3u, "48")
            LA3DM_SCAN1_GROUP(4u, "768")
            LA3DM_SCAN1_GROUP(5u, "784")
            LA3DM_SCAN1_GROUP(6u, "800")
            LA3DM_SCAN1_GROUP(7u, "816")
            }}}}}}}}
#undef LA3DM_SCAN1_GROUP
            } else {
                // production: the same trips for the nr / 4 full groups; then, where nr is no multiple of four, the last group
                // through the trip that pushes its nr % 4 candidates only, and the ring test that follows every trip (after a
                // full group it has just been made: it fails again, or the ring was drained).  Nested as above; a group that
                // is not full is the last of its sub-round, so each level ends in it or in nothing.
                const uint32_t nfull = nr >> 2, np = nr & 3u;
#define LA3DM_SCAN1_GROUP(G, OFF)                   \
    if (G < nfull) {                                \
        uint32_t st;                                \
        float tr;                                   \
        unsigned long long hm0, hm1, hm2, hm3;      \
        LA3DM_TP_TRIP(OFF);                         \
        if (tailb > tail_cap) c_flush();
#define LA3DM_SCAN1_LAST(OFF)                       \
    } else if (np != 0u) {                          \
        uint32_t st;                                \
        float tr;                                   \
        unsigned long long hm0, hm1, hm2;           \
        LA3DM_SCAN1_PAD_TRIP(OFF);                  \
    }
                LA3DM_SCAN1_GROUP(0u, "0")
                LA3DM_SCAN1_GROUP(1u, "16")
                LA3DM_SCAN1_GROUP(2u, "32")
                LA3DM_SCAN1_GROUP(3u, "48")
                LA3DM_SCAN1_GROUP(4u, "768")
                LA3DM_SCAN1_GROUP(5u, "784")
                LA3DM_SCAN1_GROUP(6u, "800")
                LA3DM_SCAN1_GROUP(7u, "816")
                LA3DM_SCAN1_LAST("816")   // (G == nfull: the group after the full ones, at its own place in the table)
                LA3DM_SCAN1_LAST("800")
                LA3DM_SCAN1_LAST("784")
                LA3DM_SCAN1_LAST("768")
                LA3DM_SCAN1_LAST("48")
                LA3DM_SCAN1_LAST("32")
                LA3DM_SCAN1_LAST("16")
                LA3DM_SCAN1_LAST("0")
#undef LA3DM_SCAN1_GROUP
#undef LA3DM_SCAN1_LAST
                if (tailb > tail_cap) c_flush();
            }
            // (the next sub-round overwrites the table: LDS operations of a wave complete in order)
        }
    };

    for (uint32_t cb = 0;;) {
        chunk(pc, cb);
        cb += kWave;
        if (cb >= M) break;
        pc = pn;
        if (cb + kWave < M) pn = gather(cb + kWave);
    }

    // the tile's last, partly filled batch(es)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    {
        const uint32_t tail = (tailb - ring_base) >> 3;
        if (kProd || !(a.flags & 0x100u))
            for (uint32_t p = 0; p < tail; p += kWave)
                if (p + lane < tail) c_eval(p + lane);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    {
        const double s0 = L.acc0[lane], s1 = L.acc1[lane];
        double K = s0 + s1, Y = s1;
        if (nonfinite != 0ull) K = Y = __builtin_nan("");  // (gated: K > 0 is false, the leaf is left alone; ungated: alpha = beta = NaN)
        uint32_t lw = li;
        asm volatile("" : "+v"(lw));
        float *const alpha = scan1_arg_again<float, offsetof(BgkArgs, alpha)>(), *const beta = scan1_arg_again<float, offsetof(BgkArgs, beta)>();
        uint8_t *const state = scan1_arg_again<uint8_t, offsetof(BgkArgs, state)>();
        if (K > 0.0 || (!kProd && (a.flags & 1u) != 0u)) {  // flag 1: insert_training_data, update() runs unconditionally
#if LA3DM_T_EARLY_AB
            const float A = (float)((double)A0 + Y);
            const float B = (float)((double)B0 + (K - Y));
#else
            const float A = (float)((double)alpha[lw] + Y);
            const float B = (float)((double)beta[lw] + (K - Y));
#endif
            alpha[lw] = A;
            beta[lw] = B;
            state[lw] = (uint8_t)(classify_fast(A, B, a) | 0x80u);
        } else {
            state[lw] = 0;
        }
    }
}

// the untimed launch: the tile body and nothing else
template <int kTrig, bool kProd = false>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(8, 8))) void bgk_predict_fuse_t1(BgkArgs a) {
    bgk_scan1_tile<kTrig, kProd>(a);
}

// One record of stamps per launch, all zero before the launch (la3dm_ctx.h: the stamp pool): kStampSlots entry stamps of
// 8 bytes side by side, then kStampSlots exit stamps of 8 bytes, each on a 128-byte line of its own.
constexpr uint32_t kStampSlots = 64, kStampExitStride = 16;   // (stride in 8-byte words)
constexpr uint32_t kStampRecordBytes = 8u * (kStampSlots + kStampSlots * kStampExitStride);

// "time_kernel" 1: the same tile body between two reads of the device's constant-rate wall clock, so that the kernel's time
// needs no event and no packet beside the kernel's own.  Entry: each of the first kStampSlots workgroups stores its stamp in a
// slot of its own (the host takes the least of the slots that were written).  Exit, on EVERY path out of the body (the early
// returns of bgk_scan1_tile come back here): one atomicMax without a return value per wave, on exit slot blockIdx.x mod
// kStampSlots (the host takes the greatest).  The exit slots are shards that must not share a line: atomics on one 128-byte
// line queue up behind each other wherever in the line they land — with the 64 slots side by side (four lines) a grid of
// 40 000 waves was 40 us longer and the 20 000-ray scan took 101 us instead of 36; a line per slot costs nothing that can be
// measured (profiles/kernel_stamps/README.md).  The clock reads and the entry stores are free.  The stamps leave through
// `stamps` only; nothing the scan computes depends on them.
template <int kTrig, bool kProd = false>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(8, 8))) void bgk_predict_fuse_t1s(BgkArgs a, unsigned long long *stamps) {
    const unsigned long long t_in = wall_clock64();
    if (blockIdx.x < kStampSlots && threadIdx.x == 0) stamps[blockIdx.x] = t_in;
    bgk_scan1_tile<kTrig, kProd>(a);
    const unsigned long long t_out = wall_clock64();
    uint32_t lane = threadIdx.x;
    asm volatile("" : "+v"(lane));  // (compared again here: the entry's comparison is not kept in registers across the body)
    static_assert(sizeof(BgkArgs) % 8 == 0, "the stamp pointer follows BgkArgs in the kernarg segment");
    unsigned long long *const rec = scan1_arg_again<unsigned long long, sizeof(BgkArgs)>();   // (`stamps`, not carried through the body)
    if (lane == 0) atomicMax(rec + kStampSlots + kStampExitStride * (blockIdx.x & (kStampSlots - 1u)), t_out);
}

}  // namespace la3dm_dev
