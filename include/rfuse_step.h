/*
 * rfuse_step.h -- the refinement-step ABI of librfuse_hip.so: the two places where a training step of the reference's refinement trainer
 * (trainer/train_refinement.py:50-86, :101-120) still left HIP once convs, GroupNorm, attention, losses, data and Adam were on the device --
 * the backward of the decoder's head (model/refinement.py:54-55, Conv3d(nf, 1, 1) + Tanh) and the attention rows' occupancy
 * (trainer :245-247 occupancy_from_prediction, then model/attention.py:132-139 unfold + any).
 *
 * A tenth header, in the vocabulary and with the conventions of rfuse_train.h (extern "C", device pointers to contiguous arrays, no allocation,
 * stream-ordered on `stream`, 0 or an RF_E_* code from every `int` function whose last parameter is `stream`, rf_last_error() for the message,
 * no `double` scalar, argument checks before any device is touched).  rfuse.h and the other eight headers stay as they are.
 */
#ifndef RFUSE_STEP_H
#define RFUSE_STEP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Backward of out = tanh(sum_c w[c] * h[., c, .] + b), the forward being rf_conv1x1_tanh with post_add = 0, post_mul = 1.
 *   h [n][c][voxels] float32 (the head's input), out [n][voxels] (the saved tanh output), dout [n][voxels], w [c]
 *   g     = dout * fmaf(-out, out, 1.0f)       rounded to float32 once, used for all three outputs
 *   dh    = g * w[c]                            float32, [n][c][voxels]
 *   dw[c] = sum over n, voxels of (double)g * (double)h   (the products are exact in float64), rounded to float32 once
 *   db[0] = sum over n, voxels of (double)g, likewise
 * Sums: float64 per thread, per wave, per workgroup (wave order); the per-workgroup partials go to `ws` and a second small launch adds them in
 * workgroup order.  No atomics, no device-side ticket, the grid a function of the shape only: the same bits on every call.  Non-finite inputs are
 * not masked: a NaN or Inf of dout reaches dh at its voxel, and dw and db.
 * Supported: voxels % 4 == 0, 1 <= c <= 64, n * voxels / 4 < 2^31 (anything else RF_E_UNSUPPORTED); the tensor pointers 16-byte aligned.
 * dw and db may both be null (a frozen head): dh alone is computed, in one launch, with the same bits, and `ws` is not used.
 * One thread takes four consecutive voxels at a time; at most rf_pointwise_tanh_backward_grid_threads() threads are launched, each striding
 * over the quads that are left. */
int rf_pointwise_tanh_backward(const float* h, const float* out, const float* dout, const float* w, int n, int c, size_t voxels, float* dh,
                               float* dw, float* db, void* ws, size_t ws_bytes, void* stream);
size_t rf_pointwise_tanh_backward_ws_bytes(int n, int c, size_t voxels);      /* 0 = a shape outside the supported range */
int rf_pointwise_tanh_backward_grid_threads(void);

/* rows [n * (edge / (2e))^3] uint8 0 / 1 from pred [n][edge][edge][edge] (the decoder's tanh output), rows in Unfold3D's order (b, px, py, pz):
 *   df  = ((pred + 1.0f) * trunc) / 2.0f        three float32 operations, no contraction (network_pred_to_df as torch evaluates it)
 *   row = any over its (2e)^3 block of (df <= thr)      NaN compares false
 * which is max_pool3d((df <= thr).float(), 2, 2).bool(), Unfold3D(e, 1) and any(dim = 1), for every input.  `thr`: the float32 value torch gives the
 * threshold beside a float32 tensor.  One launch, no atomics.  Supported: e >= 1, edge % (2e) == 0, fewer than 2^31 rows. */
int rf_attn_occupancy_rows(const float* pred, int n, int edge, int e, float trunc, float thr, uint8_t* rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif
