// The split-operand format of the F16 MFMA kernels: fp32 GEMMs evaluated on the F16 matrix cores by OPERAND SPLITTING.
//
//     every fp32 operand x is carried as two f16 numbers   h = f16(x),  l = f16((x - h) * 2^11)       (x - h is exact in fp32)
//     so that x = h + l / 2^11 up to 2^-22 |x|, and        a * b  ~  ah * bh  +  (ah * bl + al * bh) / 2^11  (al * bl: 2^-22 relative, dropped).
//     An f16 x f16 product is exact in fp32.  v_mfma_f32_16x16x32_f16 accumulates in fp32; the ah*bh sums and the cross sums go to
//     SEPARATE accumulators (hi, lo) and meet once, in the epilogue:  out = hi + lo / 2^11.
//
// Three f16 MFMAs (16 cycles each for 16x16x32) replace eight fp32 MFMAs (32 cycles each for 16x16x4): 5.3x the multiply-add rate of the
// fp32 matrix path at -- measured, tools/micro/split_probe.hip -- HALF its rounding error against float64 (K = 216 ... 5184: rms 1.2e-8
// vs 2.5e-8 of sum|a b|, max 9.7e-8 vs 3.1e-7): the fp32 MFMA is a sequential fmaf chain with one rounding per product, the f16 MFMA
// rounds once per 32 products, and the 2^-22 representation error of the operands is random per element and does not accumulate.
// Activations are scaled by 2^-4 and weights by 2^4 before the split (exact): f16 overflows at 65504, so a GroupNorm output would have to
// exceed 1e6 to saturate (it is clamped, never inf), while small values lose nothing (whatever h drops, l carries).  The host's range guard
// (rfuse/ops.py SPLIT_MAX_ABS_WEIGHT / SPLIT_MAX_ABS_ACT) and the ABI text of include/rfuse.h state the same scales.
//
// Every kernel that produces or consumes the format takes its pieces, scales, splits, MFMA triple and recombine from here.
#pragma once
#include "common.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

namespace {
constexpr float SPLIT_ACT_SCALE = 1.0f / 16, SPLIT_W_SCALE = 16.0f, SPLIT_LO = 2048.0f;
static_assert(SPLIT_ACT_SCALE * SPLIT_W_SCALE == 1.0f, "epilogues assume the operand scales cancel");
static_assert(SPLIT_LO == 2048.0f, "l carries (x - h) * 2^11");
}   // namespace

// one activation that already carries the 2^-4 -> its two f16 pieces (saturating, never inf; NaN stays NaN)
__device__ __forceinline__ void rf_split(float v, _Float16& h, _Float16& l) {
    v = rf_clamp_f16(v);
    h = (_Float16)v;
    l = (_Float16)fmaf(-SPLIT_LO, (float)h, v * SPLIT_LO);          // (v - h) * 2^11: exact either way, one v_fma_mix instead of cvt + sub + mul
}

// ... into element j of h8 / h4 pieces (vector elements do not bind to _Float16&).  The body is rf_split's, written out: through a call to it the
// kernels' code comes out reordered.
template <class V>
__device__ __forceinline__ void rf_split_at(float v, V& h, V& l, int j) {
    v = rf_clamp_f16(v);
    const _Float16 hh = (_Float16)v;
    h[j] = hh;
    l[j] = (_Float16)fmaf(-SPLIT_LO, (float)hh, v * SPLIT_LO);
}

// 8 normalised channel values of one voxel -> the two f16 pieces (scaled by 2^-4 here)
__device__ __forceinline__ void rf_split8(const float (&y)[8], h8& h, h8& l) {
#pragma unroll
    for (int j = 0; j < 8; ++j) rf_split_at(y[j] * SPLIT_ACT_SCALE, h, l, j);
}

// one weight, from its float64 value (or a float64 sum of weights) -> its pieces, for the packed weight images
__device__ __forceinline__ void rf_split_weight(double w, _Float16& h, _Float16& l) {
    double v = w * (double)SPLIT_W_SCALE;
    v = v > 65504.0 ? 65504.0 : (v < -65504.0 ? -65504.0 : v);
    h = (_Float16)(float)v;
    l = (_Float16)(float)((v - (double)(float)h) * (double)SPLIT_LO);
}

// the MFMA triple ah*bh -> hi, ah*bl -> lo, al*bh -> lo over NB n-blocks: three passes, so that consecutive MFMAs never share an accumulator
template <int NB>
__device__ __forceinline__ void rf_split_mfma(f32x4 (&hi)[NB], f32x4 (&lo)[NB], const h8& ah, const h8& al, const h8 (&bh)[NB], const h8 (&bl)[NB]) {
#pragma unroll
    for (int n = 0; n < NB; ++n) hi[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[n], hi[n], 0, 0, 0);
#pragma unroll
    for (int n = 0; n < NB; ++n) lo[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[n], lo[n], 0, 0, 0);
#pragma unroll
    for (int n = 0; n < NB; ++n) lo[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[n], lo[n], 0, 0, 0);
}

// the accumulators back to one fp32 value: hi + lo / 2^11
__device__ __forceinline__ float rf_split_join(float hi, float lo) { return fmaf(lo, 1.0f / SPLIT_LO, hi); }
