/*
 * rfuse_attn_train.h -- the patch attention's training ABI of librfuse_hip.so: the backward of the row route of rfuse.h's attention
 * section (rf_attn_fuse, rf_attn_gather_retrieved; the reference trains through this stage in trainer/train_refinement.py:108-120,
 * phases 2 and 3).  rf_unfold3d and rf_fold3d (rfuse.h) are each other's backward and need nothing here.
 *
 * A sixth header beside rfuse.h, rfuse_eval.h, rfuse_train.h, rfuse_contrastive.h and rfuse_pairs.h, in the same vocabulary and with the
 * same conventions (extern "C", device pointers to contiguous float32 arrays, no allocation, stream-ordered on `stream`, 0 or an RF_E_*
 * code from every `int` function whose last parameter is `stream`, rf_last_error() for the message).  The other five stay as they are.
 * Modes (RF_ATTN_SOFTMAX 0, RF_ATTN_GUMBEL_HARD 1), layouts and limits (K 1..16, f 1..128) are those of rfuse.h.
 */
#ifndef RFUSE_ATTN_TRAIN_H
#define RFUSE_ATTN_TRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

/* Backward of rf_attn_fuse: x, dout, dx [rows][d]; p, dp [rows][k][d]; xf, dxf [rows][f]; pf, dpf [rows][k][f] (xf, pf the RAW encoder
 * outputs: F.normalize's backward is inside); noise [rows][k], required in Gumbel-hard mode.  Each of the four outputs may be NULL = not
 * computed, not written.  Per row, with g = the row of dout, sw = switch, w = the forward weights (Gumbel-hard: the one-hot), y = the soft
 * weights (Gumbel-hard: softmax(25 s + noise), torch's straight-through form), a = sharpness | 25, k* = the FIRST index of the maximal score
 * (where MaxPool1d(K), model/attention.py:99, sends the gradient of the maximum):
 *   dx   = g * (1 - sw)                        dp_k  = g * (w_k * sw)
 *   dsw  = <g, sum_k w_k p_k - x>              dw_k  = sw * <g, p_k>
 *   ds_k = a * y_k * (dw_k - sum_j y_j dw_j)  +  (k == k* and max score > 0 ? dsw : 0)
 *   dxn  = sum_k ds_k pn_k                     dpn_k = ds_k xn
 *   dxf  = (dxn - xn <xn, dxn>) / |xf|         dpf_k = (dpn_k - pn_k <pn_k, dpn_k>) / |pf_k|       (|v| <= 1e-12: dn / 1e-12, as F.normalize)
 * The discrete decisions (k*, max score > 0, the slot Gumbel-hard chose) are recomputed from xf, pf and noise with the forward's own code
 * and are the ones rf_attn_fuse took, bit for bit; the values are evaluated in float64 and rounded to float32 once.
 * One launch, no workspace, no atomics, the same bits on every call. */
int rf_attn_fuse_backward(const float* x, const float* p, const float* xf, const float* pf, const float* noise,
                          const float* dout, int rows, int k, int d, int f, int mode, float sharpness,
                          float* dx, float* dp, float* dxf, float* dpf, void* stream);

/* Backward of rf_attn_gather_retrieved: its exact inverse index map (the gather is a bijection), dp_rows [(b*r^3)][k][c][e^3] -> dsrc in the
 * layout of the gather's src (src_layout 0: [b*k][c][s^3]; 1: patch-major [(b*k*q^3)][c][t^3], q = s/t).  Every element of dsrc is written
 * exactly once: no zero-fill, no accumulation. */
int rf_attn_scatter_retrieved(const float* dp_rows, int src_layout, int b, int k, int c, int s, int e, int t,
                              float* dsrc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
