/*
 * rfuse_contrastive.h -- the contrastive-loss ABI of librfuse_hip.so: NT-Xent (model/loss.py NTXentLoss.forward) and its sliced form, the
 * attention contrastive loss of the reference's refinement trainer (trainer/train_refinement.py:208-221
 * compute_sliced_attn_nt_xent_loss), on the device.
 *
 * A fourth header beside rfuse.h, rfuse_eval.h and rfuse_train.h, in the same vocabulary and with the same conventions (extern "C",
 * device pointers to contiguous arrays, no allocation, stream-ordered on `stream`, 0 or an RF_E_* code from every `int` function
 * whose last parameter is `stream`, rf_last_error() for the message, no `double` scalar, argument checks before any device is
 * touched).  The other three headers stay as they are.
 *
 * One group of n pairs: rows stacked [zjs; zis], 2n in all;  w = z / max(|z|, 1e-8) (cosine) or z (dot);  s_ij = w_i . w_j;
 *   pos(i) = (i + n) mod 2n;  l_ij = s_ij / tau_ij,  tau_ij = tau for the positive and, for a negative, tau or with an IoU matrix
 *   tau + (1 - tau) * sigmoid(iou[i][j] * sig_scale + sig_shift);  loss = (1 / 2n) sum_i (lse_{j != i} l_ij - l_{i,pos(i)}).
 * The sliced form cuts the n_rows rows of zis / zjs into num_slices slices of split = n_rows / num_slices rows (rows past
 * num_slices * split are ignored), keeps the occupied rows of a slice as one group, and takes slices greedily in order: slice s
 * is taken iff count_s > 0 and taken + count_s <= max_rows (one that does not fit is skipped, a later one may still be taken).
 * The loss is the SUM over the taken groups of each group's mean; no taken group: 0, with a zero gradient.
 * occupancy == null: every row is occupied (num_slices = 1, max_rows = n_rows: one NTXentLoss call on all rows).
 *
 * Supported: 1 <= dim <= 256, 1 <= num_slices <= 4096, 1 <= min(split, max_rows) <= 4096 (the largest possible group);
 * otherwise RF_E_UNSUPPORTED.  Arithmetic is float64 from the float32 inputs on; sums run in a fixed order without atomics:
 * the same bits on every call.  The three launches of one evaluation share a workspace that the backward reads again.
 */
#ifndef RFUSE_CONTRASTIVE_H
#define RFUSE_CONTRASTIVE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t rf_ntx_ws_bytes(int n_rows, int num_slices, int max_rows, int dim);      /* 0 = outside the supported range */

/* The selection, on the device: per-slice occupied counts, the greedy rule, the compacted row list, the per-group tiles and a
 * selected flag per row, all into `ws`.  occupancy uint8 [n_rows] (non-zero = occupied) or null.
 * counts [3] int64 = occupied rows over all slices, selected rows, selected groups.  Nothing returns to the host. */
int rf_ntx_plan(const uint8_t* occupancy, int n_rows, int num_slices, int max_rows, int dim, void* ws, size_t ws_bytes,
                int64_t* counts, void* stream);

/* loss [1] float32 of the planned selection.  zis, zjs float32 [n_rows][dim]; iou float32 [2n][2n] or null, indexed by the
 * position in the stacked selected rows (needs num_slices == 1).  Saves in `ws` what rf_ntx_backward needs: the stacked w in
 * float64, the row norms and the per-row log-sum-exp.  Grids are sized by max_rows, not by the counts on the device. */
int rf_ntx_forward(const float* zis, const float* zjs, const float* iou, int n_rows, int num_slices, int max_rows, int dim,
                   int cosine, float tau, float sig_scale, float sig_shift, void* ws, size_t ws_bytes, float* loss, void* stream);

/* dzis, dzjs float32 [n_rows][dim] in one launch: with G_ij = (softmax_ij - [j = pos(i)]) / tau_ij / 2n row i gets
 * dw_i = sum_j (G_ij + G_ji) w_j (G_ji from lse_j and iou[j][i]), carried through the normalisation in cosine mode:
 * (dw - w (w . dw)) / |z|, or dw / 1e-8 where |z| < 1e-8; times grad_loss [1] float32 ON THE DEVICE; scattered to the rows'
 * own positions.  Rows that were not selected receive exact zeros.  `ws`: as rf_ntx_forward left it. */
int rf_ntx_backward(const float* iou, const float* grad_loss, int n_rows, int num_slices, int max_rows, int dim, int cosine,
                    float tau, float sig_scale, float sig_shift, const void* ws, size_t ws_bytes, float* dzis, float* dzjs,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
