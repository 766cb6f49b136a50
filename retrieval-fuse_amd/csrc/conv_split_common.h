// Shared by the split-operand kernels (conv3d_split.hip, conv3d_split_zc.hip, conv3d_up_split.hip): the halo-box image in LDS, the STAGING STEP of the
// prologue that fills it (rf_stage8 = rf_norm_split8 + rf_store_hl), the pre-split output (SplitPreOut and its makers) and the HAND-OVER EPILOGUE that
// writes it.  The operand format itself is split_operand.h; the triple from (sum, sum of squares) is rf_gn_triple (common.h); the host side of the
// conv3d_split entry points (ConvArgs builders, pointer refusals) is conv_split_args.h and the launch tail is rf_launch (common.h).
#pragma once
#include "common.h"
#include "split_operand.h"

namespace {
// halo box [10][10][10] in 16-byte slots, Y-MAJOR with a padded y stride: slot(z, y, x) = y * 104 + z * 10 + x.  An A operand is a ds_read_b128 of
// an m-block = 8 x by 2 y voxels, served in four fixed 16-lane groups (MI355X_MICROARCH.md, LDS): lanes {0-3, 12-15} of one tap and {4-11} of the
// next, i.e. x 0-3 of row y, x 4-7 of row y + 1 and the other halves one tap on.  With slot(z, y, x) = z * 100 + y * 10 + x (rounds 2-3) row y + 1
// sat 10 slots on: x = 6, 7 of it on the slots (mod 16) of x = 0, 1 of row y -- two LDS cycles per group for every A operand of every box kernel
// (SQ_LDS_BANK_CONFLICT: 0.36-0.46 of the active LDS cycles).  With the rows of a tile 104 = 8 (mod 16) slots apart the group covers 16 different
// slots except where two taps meet: 1.29 cycles per group over the 7 k-steps (model: tools/lds_bank_model.py).
constexpr int CS_SY = 104, CS_SZ = 10, CS_VOX = 1000, CS_SLOTS = 1040;
constexpr int CS_PLANE = CS_SLOTS * 16;                          // bytes of one (h or l) plane
constexpr int CS_BUF = 2 * CS_PLANE;
constexpr int CS_LDS_BYTES = 2 * CS_BUF;                         // 66,560
}   // namespace

// pre-split OUTPUT (whole 8^3 samples, 16 couts in one workgroup): the NEXT layer's GroupNorm -- its gamma / beta / groups / eps over this layer's couts --
// is applied in the epilogue from the sample's own statistics and the result written as that layer's pre-split input; null: off
struct SplitPreOut {
    h8* out = nullptr;
    const float* gamma = nullptr;
    const float* beta = nullptr;
    int groups = 0;
    float eps = 0.f;
    // ... or the final decoder's pointwise head (reference model/refinement.py:48-61: Conv3d(nf, 1, 1) + bias -> tanh -> network_pred_to_df) applied to the
    // ReLU'd output in the epilogue: pw_out [n][1][edge^3] = (tanh(sum_c w[c] y[c] + b) + post_add) * post_mul, the nf-channel tensor is never written
    float* pw_out = nullptr;
    const float* pw_w = nullptr;
    const float* pw_b = nullptr;
    float post_add = 0.f, post_mul = 0.f;

    static SplitPreOut presplit(void* out_presplit, const float* next_gamma, const float* next_beta, int next_groups, float eps) {
        SplitPreOut po;
        po.out = reinterpret_cast<h8*>(out_presplit); po.gamma = next_gamma; po.beta = next_beta; po.groups = next_groups; po.eps = eps;
        return po;
    }
    static SplitPreOut pointwise(float* out1, const float* pw_w, const float* pw_b, float post_add, float post_mul) {
        SplitPreOut po;
        po.pw_out = out1; po.pw_w = pw_w; po.pw_b = pw_b; po.post_add = post_add; po.post_mul = post_mul;
        return po;
    }
};

// ------------------------------------------------------------------------------------------------------- the staging step of the prologue
// Every kernel of the family stages its input the same way: 8 channels of one voxel, y = (x - center) * scale + shift by the channels' GroupNorm triples, zeros
// where the voxel is padding of the NORMALISED tensor, split, h into the voxel's 16-byte slot and l one plane further on.  What is scheduling stays with the
// kernel: sched_barriers, opaque copies of the thread index, the slot arithmetic, which waves stage, guards on the stores.

// the two stores alone (also: pre-split copies, which stage h / l they did not compute); `plane`: bytes from the h plane to the l plane
__device__ __forceinline__ void rf_store_hl(unsigned char* slot, int plane, const h8& h, const h8& l) {
    *reinterpret_cast<h8*>(slot) = h;
    *reinterpret_cast<h8*>(slot + plane) = l;
}
// channel j of the staged voxel: x is the 8 register-staged values, or a callable for a site that loads the value where it is used
__device__ __forceinline__ float rf_chan(const float (&x)[8], int j) { return x[j]; }
template <class X>
__device__ __forceinline__ auto rf_chan(X&& x, int j) -> decltype(x(j)) { return x(j); }
// normalise (triple(j) -> float4 of channel j; !live: the zero padding of the NORMALISED tensor) and split, for a kernel that guards its stores or forms the
// slot address after the conversion (the order of the source is the order hipcc schedules from)
template <class X, class Triple>
__device__ __forceinline__ void rf_norm_split8(X&& x, Triple&& triple, h8& h, h8& l, bool live = true) {
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float4 af = triple(j);
        y[j] = live ? fmaf(rf_chan(x, j) - af.x, af.y, af.z) : 0.f;
    }
    rf_split8(y, h, l);
}
// the whole step
template <class X, class Triple>
__device__ __forceinline__ void rf_stage8(unsigned char* slot, int plane, X&& x, Triple&& triple, bool live = true) {
    h8 h, l;
    rf_norm_split8(x, triple, h, l, live);
    rf_store_hl(slot, plane, h, l);
}

// ------------------------------------------------------------------------------------------------------- the hand-over epilogue
// ReLU'd tile [cout][8^3] in LDS -> per-channel float64 sums -> the next layer's GroupNorm triples -> normalise, split, [h | l] slots.  Three pieces that a
// kernel composes; its barriers (__syncthreads / lds_barrier) and its opaque copy of the thread index stay with the kernel.

// (sum, sum of squares) of one cout's 512 tile values: TPC threads per cout (`part` = 0 .. TPC - 1) read TPC-strided values, then a butterfly over the TPC
// lanes -- a fixed order, so every route gives the same bits.  Valid in every lane of the TPC; !live: zeros (the lanes still take part in the butterfly)
template <int STRIDE, int TPC>
__device__ __forceinline__ double2 rf_tile_channel_sums(const float* e, int co, int part, bool live) {
    constexpr int PER = 512 / TPC, UNROLL = PER <= 16 ? PER : 8;
    double sm = 0.0, sq = 0.0;
    if (live) {
#pragma unroll UNROLL
        for (int i = 0; i < PER; ++i) {
            const float v = e[co * STRIDE + part + TPC * i];
            sm += (double)v; sq += (double)v * v;
        }
    }
    rf_xor_sum2<1, TPC / 2>(sm, sq);
    return make_double2(sm, sq);
}

// the next layer's triple of channel c, as rf_gn_from_stats: the sums of its group (cpg channels of `voxels` values each) in channel order, float64
__device__ __forceinline__ float4 rf_group_triple(const double2* chst, int c, int cpg, double voxels, float eps, const float* gamma, const float* beta) {
    const int c0 = (c / cpg) * cpg;
    double sm = 0.0, sq = 0.0;
    for (int k = c0; k < c0 + cpg; ++k) { sm += chst[k].x; sq += chst[k].y; }
    return rf_gn_triple(sm, sq, (double)cpg * voxels, (double)eps, gamma[c], beta[c]);
}

// this thread's voxel of every 8-channel group: value(c) -- a tile read, or the zc kernel's L2 read-back -- normalised by trip[c], split, stored to the h and
// the l plane (VOX slots each) of group sg; `o` = the sample's pre-split image + this thread's voxel
template <int VOX, class Value>
__device__ __forceinline__ void rf_presplit_store(h8* __restrict__ o, int cgroups, const float4* trip, Value&& value) {
    for (int sg = 0; sg < cgroups; ++sg) {
        // rf_norm_split8 written out: through it k_conv3_split_zc<true> spills one more VGPR (12 against 11); keep the two in step
        float y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4 t4 = trip[sg * 8 + j];
            y[j] = fmaf(value(sg * 8 + j) - t4.x, t4.y, t4.z);
        }
        h8 h, l;
        rf_split8(y, h, l);
        rf_store_hl(reinterpret_cast<unsigned char*>(o + (size_t)sg * 2 * VOX), VOX * 16, h, l);
    }
}
