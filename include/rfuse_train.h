/*
 * rfuse_train.h -- the training-loss ABI of librfuse_hip.so: the shape loss of the reference's trainer
 * (trainer/train_refinement.py:175-183 loss_shape, :231-253 augment_batch_data / adjust_weights;
 * dataset/patched_scene_dataset.py:139-146 compute_normals; model/loss.py get_cosine_similarity) on the device.
 *
 * A third header beside rfuse.h and rfuse_eval.h, in the same vocabulary and with the same conventions (extern "C", device
 * pointers to contiguous arrays, no allocation, stream-ordered on `stream`, 0 or an RF_E_* code from every `int`
 * function whose last parameter is `stream`, rf_last_error() for the message, no `double` scalar).  rfuse.h and
 * rfuse_eval.h stay as they are.
 *
 * Volumes are float32 [n][d][h][w] (the reference's [B,1,D,H,W]), normals float32 [n][3][d][h][w].  Any d, h, w >= 1 with
 * d * h * w <= 2^31 - 1 and at most 2^31 - 1 tiles of 8 x 8 x 32 voxels over the batch (more: RF_E_UNSUPPORTED).
 * Neighbourhoods are clipped to the volume: what lies outside is the constant `pad` (the reference pads with target_trunc).
 *
 * Sobel gradient g = (gx, gy, gz) of a volume v at voxel (z, y, x), S = [1,2,1] (x) [1,2,1] smoothing over the two other axes:
 *   gx = S v(z-1, ., .) - S v(z+1, ., .)      gy = S v(., y-1, .) - S v(., y+1, .)      gz = S v(., ., x+1) - S v(., ., x-1)
 * (the cross-correlation with sobel_3d_x / _y / _z).  The 27 taps are accumulated in float64 and rounded to float32 once, so g is
 * exactly 0 wherever the neighbourhood is flat.  Everything after g is float32, one rounding per operation, no FMA contraction.
 */
#ifndef RFUSE_TRAIN_H
#define RFUSE_TRAIN_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* normals = g / sqrt((gx^2 + gy^2 + gz^2) + 1e-5) of the volume u = v * scale + shift (compute_normals of a denormalised target;
 * scale = 1, shift = 0: of v itself).  When `weights` / `empty` are given (each may be null) the augment_batch_data outputs are
 * written in the same pass, from v itself: weights = 1 + float(v < thr) * w_occ_minus_1, empty = (v >= thr) as uint8 0 / 1. */
int rf_train_sobel_normals(const float* v, int n, int d, int h, int w, float scale, float shift, float pad, float thr,
                           float w_occ_minus_1, float* normals, float* weights, uint8_t* empty, void* stream);

/* loss_shape forward.  pred, target, weights [n][d][h][w], empty uint8, normals_t [n][3][d][h][w] (the augment outputs).
 *   df = (pred + 1) * trunc / 2;  t = 2 * ((target * std + mean) / trunc) - 1;  W' = 0 where empty and df >= trunc, else weights
 *   l1 = mean |pred - t| * W';  normal = 1 - mean over valid voxels of cos(np, nt), np = the normals of df (pad = trunc),
 *   valid = |np| != 0 and |nt| != 0;  total = lambda_rec * l1 + lambda_n * normal.  A term whose lambda is <= 0 is not
 *   evaluated and reported as 0.  No valid voxel: normal and total are NaN.
 * out [3] float32 = total, l1, normal; counts [2] int64 = valid voxels, voxels with empty and df >= trunc.
 * grad_l1 [n][d][h][w] and grad_g [n][3][d][h][w] (both or neither; null = forward only) receive what
 * rf_train_shape_loss_backward consumes: sign(pred - t) * W' and d cos / d g (0 at voxels that are not valid).
 * Sums are float64 per thread, per-workgroup partials in `ws` combined in a fixed order: the same bits on every call. */
int rf_train_shape_loss(const float* pred, const float* target, const float* weights, const uint8_t* empty, const float* normals_t,
                        int n, int d, int h, int w, float trunc, float mean, float std, float lambda_rec, float lambda_n, float* out,
                        int64_t* counts, float* grad_l1, float* grad_g, void* ws, size_t ws_bytes, void* stream);
size_t rf_train_shape_loss_ws_bytes(int n, int d, int h, int w);      /* 0 = a shape outside the supported range */

/* d pred [n][d][h][w] in one launch: coef[0] * grad_l1 / N + coef[1] * (trunc / 2) / valid * (the three Sobel stencils applied to the
 * three channels of grad_g, zero outside the volume), N = n d h w.  (normal = 1 - mean cos, and the transposed stencils are the
 * negated ones: the two signs cancel.)  coef [2] float32 ON THE DEVICE: a = g_total * lambda_rec + g_l1 and b = g_total * lambda_n +
 * g_normal, the upstream gradients of the three outputs.  counts: the forward's.  With no valid voxel the normal term contributes
 * nothing (the reference's gradient is then the L1 part alone).  Either of grad_l1 / grad_g may be null: its term is skipped. */
int rf_train_shape_loss_backward(const float* grad_l1, const float* grad_g, const float* coef, const int64_t* counts, int n, int d,
                                 int h, int w, float trunc, float* dpred, void* stream);

#ifdef __cplusplus
}
#endif
#endif
