/*
 * rfuse_pairs.h -- the pairwise-occupancy ABI of librfuse_hip.so: the IoU matrix of the reference's retrieval trainer
 * (util/misc.py:51-59 get_iou_matrix, called from trainer/train_retrieval.py:85 on
 * `denormalize_target(batch['target']) <= 0.75 * voxel_size_target`), on the device.
 *
 * A fifth header, in the vocabulary and with the conventions of the other four (extern "C", device pointers to contiguous
 * arrays, no allocation, stream-ordered on `stream`, 0 or an RF_E_* code from every `int` function whose last parameter is
 * `stream`, rf_last_error() for the message, no `double` scalar, argument checks before any device is touched).  The other
 * headers stay as they are.
 *
 * Two steps.  rf_iou_pack turns n occupancy windows of `voxels` voxels each into one bit per voxel, words = ceil(voxels / 64)
 * 64-bit words per sample (voxel v is bit v % 64 of word v / 64; the bits at and beyond `voxels` are zero), and counts the set
 * bits of every sample.  rf_iou_matrix takes two packed sets a and b (or one, against itself):
 *   inter[i][j] = sum_w popcount(a_i[w] & b_j[w]),  union = count_a[i] + count_b[j] - inter,
 *   iou = float(inter) / (float(union) + 1e-5f)
 * with the two conversions, the add and the divide each one correctly rounded float32 operation: for counts below 2^24 that is
 * the reference's `intersection / (union + 1e-5)` bit for bit.  Integer sums, no atomics: the same bits on every call.
 *
 * Supported: 1 <= n, n_a, n_b <= 8192, 1 <= voxels <= 2^24 (every count is exact in float32), repeat 1 or 2;
 * otherwise RF_E_UNSUPPORTED.
 */
#ifndef RFUSE_PAIRS_H
#define RFUSE_PAIRS_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* What a caller holds between the two steps: the bytes of the packed form of both sets, uint64 [n][words] and int [n] for
 * n = n_a and for n = n_b, each of the four arrays rounded up to a multiple of 256.  0 = outside the supported range. */
size_t rf_iou_ws_bytes(int n_a, int n_b, long long voxels);

/* x: n windows of `voxels` voxels.  kind 0: uint8 / bool, non-zero = occupied (scale, shift, thr are not read).
 * kind 1: float32, occupied iff x * scale + shift <= thr -- a float32 multiply, a float32 add and a compare, no FMA: the
 * trainer's `patch * target_std + target_mean <= t` with the Python scalars cast to float32.  NaN is unoccupied, -inf is
 * occupied when scale > 0.  bits uint64 [n][ceil(voxels / 64)], counts int [n] = the set bits of each sample. */
int rf_iou_pack(const void* x, int kind, float scale, float shift, float thr, int n, long long voxels, uint64_t* bits,
                int* counts, void* stream);

/* out float32 [repeat * n_a][repeat * n_b]:  out[i + p * n_a][j + q * n_b] = iou(a_i, b_j) for all p, q < repeat (repeat = 2
 * is the trainer's `.repeat(2, 2)`, written once).  bits_b == null: b = a (counts_b is not read, n_b must equal n_a). */
int rf_iou_matrix(const uint64_t* bits_a, const int* counts_a, int n_a, const uint64_t* bits_b, const int* counts_b, int n_b,
                  long long voxels, int repeat, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
