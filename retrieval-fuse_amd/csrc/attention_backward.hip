// Backward of the patch attention's row route for gfx950: rf_attn_fuse_backward (the gradient of rf_attn_fuse with respect to x, p and the RAW
// encoder outputs xf, pf) and rf_attn_scatter_retrieved (the inverse of rf_attn_gather_retrieved's index map).  Unfold3D / Fold3D need nothing new:
// rf_unfold3d and rf_fold3d are each other's backward.
//
// Reference arithmetic being differentiated: model/attention.py:92-110 (AttentionBlock.forward: F.normalize, scores, MaxPool1d(K) + relu switch,
// softmax | gumbel_softmax(hard=True), weighted sum, blend), :148-152 (PatchedAttentionBlock's regroup of the retrieved features).
//
// Per row, g = the row of dout, sw = switch, w = the forward weights, y = the soft weights that carry the gradient (softmax: y = w; Gumbel-hard: the
// y_soft of the straight-through form), a = sharpness | 25, k* = the FIRST index of the maximal score (max_pool1d / max(dim) send the whole gradient of
// the maximum there; amax would split it among ties):
//   dx    = g * (1 - sw)                       dp_k  = g * (w_k * sw)
//   dsw   = <g, sum_k w_k p_k - x>             dw_k  = sw * <g, p_k>
//   ds_k  = a * y_k * (dw_k - sum_j y_j dw_j)  +  (k == k* and max score > 0 ? dsw : 0)
//   dxn   = sum_k ds_k pn_k                    dpn_k = ds_k xn
//   dxf   = (dxn - xn <xn, dxn>) / |xf|        dpf_k = (dpn_k - pn_k <pn_k, dpn_k>) / |pf_k|        (|v| <= 1e-12: F.normalize is v / 1e-12, so dn / 1e-12)
//
// One wave per row, as k_attn_fuse.  The DECISIONS -- k*, "max score > 0", the slot Gumbel-hard chose -- are recomputed with the forward's own code
// (attn_row.h, every lane redundantly, fp32): they are the ones the forward took, bit for bit.  The VALUES the gradient is made of (scores, switch,
// soft weights and everything after them) are float64 and spread over the lanes: lane i owns features i and i + 64 of the normalisations and of the
// K score dot products, lane k owns slot k of the softmax and of its backward, the K + 1 dot products over d are per-lane partial sums + wave
// reductions.  With the fp32 values of the forward (sequential 32-term sums, then a sharpness of 1024) dx = g (1 - sw) and the softmax backward came
// out at 1.5 .. 5 x the error of an fp32 torch evaluation; in float64 the error left is the fp32 rounding of the outputs.
// No workspace, no atomics, fixed summation order: the same bits on every call.
// The kernel is HBM-bound: per row it reads (2 + K) d + (1 + K) f + K floats and writes (1 + K) (d + f).
#include "common.h"
#include "attn_row.h"
#include "../../include/rfuse_attn_train.h"

// This file is built with -ffp-contract=off like attention.hip (csrc/build.py): the float64 chain uses explicit fma() where a fused sum is meant.

// waves per SIMD the register allocation aims at (the row's chain is latency-bound: wave reductions and a float64 exp in sequence)
#ifndef RF_ATTN_BWD_WAVES
#define RF_ATTN_BWD_WAVES 3
#endif
__global__ __launch_bounds__(256, RF_ATTN_BWD_WAVES) void k_attn_fuse_backward(const float* __restrict__ x, const float* __restrict__ p, const float* __restrict__ xf,
                                                            const float* __restrict__ pf, const float* __restrict__ noise,
                                                            const float* __restrict__ dout, int rows, int K, int d, int f, int mode, float sharpness,
                                                            float* __restrict__ dx, float* __restrict__ dp, float* __restrict__ dxf,
                                                            float* __restrict__ dpf) {
    const int lane = threadIdx.x & 63;
    const bool feat = dxf != nullptr || dpf != nullptr;
    // the row is the wave's: readfirstlane tells the compiler so (row bases in scalar registers, 32-bit lane offsets)
    for (int row = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); row < rows; row += gridDim.x * 4) {
        const float* xfrow = xf + (size_t)row * f;
        const float* pfrow = pf + (size_t)row * K * f;
        const float* nrow = noise ? noise + (size_t)row * K : nullptr;
        // ---- the forward's decisions, bit for bit (uniform loads, every lane)
        int kstar, hard;
        bool alive;
        {
            float sc[RF_MAX_K], w[RF_MAX_K], y[RF_MAX_K], sw, smax;
            rf_attn_row_weights_ex(xfrow, pfrow, nrow, K, f, mode, sharpness, sc, w, y, sw, smax, kstar, hard);
            alive = smax > 0.f;
        }

        // ---- lane i owns features i and i + 64 (f <= 128): norms and the K scores in float64; lane k keeps slot k's
        const int i0 = lane, i1 = lane + 64;
        const double x0 = i0 < f ? (double)xfrow[i0] : 0.0, x1 = i1 < f ? (double)xfrow[i1] : 0.0;
        const double xnorm = sqrt(wave_sum(fma(x0, x0, x1 * x1)));
        const double xrden = 1.0 / (xnorm > 1e-12 ? xnorm : 1e-12);
        const double xn0 = x0 * xrden, xn1 = x1 * xrden;
        double my_s = 0.0, my_prden = 0.0, my_pnorm = 0.0;
#pragma unroll
        for (int k = 0; k < RF_MAX_K; ++k)
            if (k < K) {
                const double p0 = i0 < f ? (double)pfrow[k * f + i0] : 0.0, p1 = i1 < f ? (double)pfrow[k * f + i1] : 0.0;
                const double pnorm = sqrt(wave_sum(fma(p0, p0, p1 * p1)));
                const double prden = 1.0 / (pnorm > 1e-12 ? pnorm : 1e-12);
                const double s = wave_sum(fma(xn0, p0, xn1 * p1)) * prden;
                if (k == lane) { my_s = s; my_prden = prden; my_pnorm = pnorm; }
            }

        // ---- lane k owns slot k: switch, weights (softmax(a s) | the one-hot of the forward's choice) and soft weights y
        const double sw = alive ? fmax(__shfl(my_s, kstar, 64), 0.0) : 0.0;
        const double a = mode == RF_ATTN_SOFTMAX ? (double)sharpness : 25.0;
        double my_w = 0.0, my_y = 0.0;
        {
            // logits relative to the forward's choice of the largest (the largest up to fp32 rounding: the exponent stays near 0)
            const double logit = mode == RF_ATTN_SOFTMAX ? a * my_s : fma(a, my_s, lane < K ? (double)nrow[lane] : 0.0);
            const double top = __shfl(logit, mode == RF_ATTN_SOFTMAX ? kstar : hard, 64);
            const double ex = lane < K ? exp(logit - top) : 0.0;
            my_y = ex / wave_sum(ex);
            my_w = mode == RF_ATTN_SOFTMAX ? my_y : (lane == hard ? 1.0 : 0.0);
        }

        // ---- one pass over the d values of the row: dx, dp, and this lane's share of <g, x> and <g, p_k>
        // static indexing only (runtime-indexed register arrays go to scratch)
        const float* grow = dout + (size_t)row * d;
        const float* xrow = x + (size_t)row * d;
        const float* prow = p + (size_t)row * K * d;
        float* dxrow = dx ? dx + (size_t)row * d : nullptr;
        float* dprow = dp ? dp + (size_t)row * K * d : nullptr;
        const float oms = (float)(1.0 - sw);
        const float my_wsw = (float)(my_w * sw);
        float wsw[RF_MAX_K];
        double acc[RF_MAX_K], accx = 0.0;
#pragma unroll
        for (int k = 0; k < RF_MAX_K; ++k) {
            wsw[k] = __shfl(my_wsw, k, 64);
            acc[k] = 0.0;
        }
        for (int j = lane; j < d; j += 64) {
            const float g = grow[j];
            if (dx) dxrow[j] = g * oms;
            if (feat) accx = fma((double)g, (double)xrow[j], accx);
#pragma unroll
            for (int k = 0; k < RF_MAX_K; ++k)
                if (k < K) {
                    if (dp) dprow[k * d + j] = g * wsw[k];
                    if (feat) acc[k] = fma((double)g, (double)prow[k * d + j], acc[k]);
                }
        }
        if (!feat) continue;

        // ---- dw_k, then ds_k
        const double gx = wave_sum(accx);
        double my_gp = 0.0;
#pragma unroll
        for (int k = 0; k < RF_MAX_K; ++k)
            if (k < K) {
                const double t = wave_sum(acc[k]);
                if (k == lane) my_gp = t;
            }
        const double dwk = sw * my_gp;
        const double ybar = wave_sum(my_y * dwk);                  // lanes >= K add 0
        const double dsw = wave_sum(my_w * my_gp) - gx;
        double ds = 0.0;
        if (lane < K) {
            ds = a * my_y * (dwk - ybar);
            if (lane == kstar && alive) ds += dsw;
        }

        // ---- F.normalize backward of xf and of every pf_k; <pn_k, dpn_k> = ds_k <pn_k, xn> = ds_k s_k
        double dxn0 = 0.0, dxn1 = 0.0;
#pragma unroll
        for (int k = 0; k < RF_MAX_K; ++k)
            if (k < K) {
                const double prden = __shfl(my_prden, k, 64), pnorm = __shfl(my_pnorm, k, 64), sk = __shfl(my_s, k, 64), dsk = __shfl(ds, k, 64);
                const double pn0 = (i0 < f ? (double)pfrow[k * f + i0] : 0.0) * prden, pn1 = (i1 < f ? (double)pfrow[k * f + i1] : 0.0) * prden;
                dxn0 = fma(dsk, pn0, dxn0);
                dxn1 = fma(dsk, pn1, dxn1);
                if (dpf) {
                    const double proj = pnorm > 1e-12 ? dsk * sk : 0.0;
                    float* o = dpf + ((size_t)row * K + k) * f;
                    if (i0 < f) o[i0] = (float)(fma(dsk, xn0, -(pn0 * proj)) * prden);
                    if (i1 < f) o[i1] = (float)(fma(dsk, xn1, -(pn1 * proj)) * prden);
                }
            }
        if (dxf) {
            const double dot = wave_sum(fma(xn0, dxn0, xn1 * dxn1));
            const double proj = xnorm > 1e-12 ? dot : 0.0;
            float* o = dxf + (size_t)row * f;
            if (i0 < f) o[i0] = (float)((dxn0 - xn0 * proj) * xrden);
            if (i1 < f) o[i1] = (float)((dxn1 - xn1 * proj) * xrden);
        }
    }
}

extern "C" int rf_attn_fuse_backward(const float* x, const float* p, const float* xf, const float* pf, const float* noise, const float* dout,
                                     int rows, int k, int d, int f, int mode, float sharpness, float* dx, float* dp, float* dxf, float* dpf,
                                     void* stream) {
    RF_REQUIRE(x && p && xf && pf && dout && rows > 0 && d > 0, RF_E_INVALID, "rf_attn_fuse_backward: bad arguments");
    RF_REQUIRE(k >= 1 && k <= RF_MAX_K, RF_E_UNSUPPORTED, "rf_attn_fuse_backward: K=%d outside 1..%d", k, RF_MAX_K);
    RF_REQUIRE(f >= 1 && f <= 128, RF_E_UNSUPPORTED, "rf_attn_fuse_backward: feature width %d outside 1..128", f);
    RF_REQUIRE(mode == RF_ATTN_SOFTMAX || (mode == RF_ATTN_GUMBEL_HARD && noise), RF_E_INVALID,
               "rf_attn_fuse_backward: Gumbel-hard mode needs the noise tensor");
    if (!dx && !dp && !dxf && !dpf) return RF_OK;
    return rf_launch<k_attn_fuse_backward>("rf_attn_fuse_backward", dim3(rf_blocks(rows, 4, 4096)), dim3(256), (hipStream_t)stream, x, p, xf, pf, noise, dout,
                                           rows, k, d, f, mode, sharpness, dx, dp, dxf, dpf);
}

// dsrc[i] = dp_rows[the element rf_attn_gather_retrieved filled from src[i]]: i walks the DESTINATION (the retrieved features' own layout), so the
// writes are the coalesced side.  The gather is a bijection: every element of dsrc is written exactly once.
__global__ __launch_bounds__(256) void k_attn_scatter(const float* __restrict__ dp_rows, int layout, int b, int K, int c, int s, int e, int t,
                                                      float* __restrict__ dsrc) {
    const int r = s / e, q = s / t;
    const size_t e3 = (size_t)e * e * e, t3 = (size_t)t * t * t, s3 = (size_t)s * s * s;
    const size_t total = (size_t)b * K * c * s3;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        int d0, d1, d2, cc;
        size_t vol;
        if (layout == 0) {                       // [vol][c][s][s][s]
            d2 = (int)(i % s), d1 = (int)((i / s) % s), d0 = (int)((i / ((size_t)s * s)) % s);
            cc = (int)((i / s3) % c);
            vol = i / (s3 * c);
        } else {                                 // [((vol*q + q0)*q + q1)*q + q2][c][t][t][t]
            const int t2 = (int)(i % t), t1 = (int)((i / t) % t), t0 = (int)((i / ((size_t)t * t)) % t);
            cc = (int)((i / t3) % c);
            const size_t patch = i / (t3 * c);
            const int q2 = (int)(patch % q), q1 = (int)((patch / q) % q), q0 = (int)((patch / ((size_t)q * q)) % q);
            vol = patch / ((size_t)q * q * q);
            d0 = q0 * t + t0, d1 = q1 * t + t1, d2 = q2 * t + t2;
        }
        const size_t bb = vol / K;
        const int k = (int)(vol % K);
        const size_t row = ((bb * r + d0 / e) * r + d1 / e) * r + d2 / e;
        dsrc[i] = dp_rows[((row * K + k) * c + cc) * e3 + ((size_t)(d0 % e) * e + (d1 % e)) * e + (d2 % e)];
    }
}

extern "C" int rf_attn_scatter_retrieved(const float* dp_rows, int src_layout, int b, int k, int c, int s, int e, int t, float* dsrc, void* stream) {
    RF_REQUIRE(dp_rows && dsrc && b > 0 && k > 0 && c > 0 && s > 0 && e > 0 && s % e == 0, RF_E_INVALID, "rf_attn_scatter_retrieved: bad arguments");
    RF_REQUIRE(src_layout == 0 || (src_layout == 1 && t > 0 && s % t == 0 && t % e == 0), RF_E_INVALID,
               "rf_attn_scatter_retrieved: bad layout %d / patch edge %d", src_layout, t);
    if (src_layout == 0) t = s;
    return rf_launch<k_attn_scatter>("rf_attn_scatter_retrieved", dim3(rf_blocks((size_t)b * k * c * s * s * s, 256, 8192)), dim3(256), (hipStream_t)stream,
                                     dp_rows, src_layout, b, k, c, s, e, t, dsrc);
}
