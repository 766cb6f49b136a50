/*
 * rfuse_level.h -- the level ABI of librfuse_hip.so: a whole encoder level of the U-Net in one launch.
 *
 * A further header beside rfuse.h, in its vocabulary and with its conventions (extern "C", device pointers to contiguous arrays in the
 * reference's layouts, no allocation, nothing kept between calls, stream-ordered on `stream`, 0 or an RF_E_* code from every `int` function
 * whose last parameter is `stream`, rf_last_error() for the message, argument checks before any device is touched).  The other headers stay
 * as they are.
 *
 * rf_conv3d_e2_level (csrc/conv3d_e2_level.hip; reference model/unet.py:230-253, an Encoder with pooling whose DoubleConv runs on 2^3 volumes):
 *   MaxPool3d(2) of x [n][c][4^3] -> GroupNorm(groups1) -> conv 3^3 (c -> cmid) -> ReLU -> GroupNorm(groups2) -> conv 3^3 (cmid -> cout) -> ReLU
 *   -> out [n][cout][2^3]
 * with stats [n][cout][1][2] float64 (sum, sum of squares) of out -- bit for bit what rf_maxpool3d_2_stats, rf_gn_from_stats,
 * rf_conv3d_e2_split_k3_gn_relu, rf_gn_from_stats, rf_conv3d_e2_split_k3_gn_relu of rfuse.h give; w1_packed / w2_packed are
 * rf_conv3_e2_split_pack_weight images for edge 2, unchanged.
 * c_skip > 0: also dec_affine [n][c_skip + cout][4], the triples that
 *   rf_gn_from_stats(skip_stats, c_skip, tiles_skip, stats, cout, 1, n, 4, gamma_dec, beta_dec, groups_dec, eps_dec, ...)
 * would write for the decoder stage that reads out upsampled beside a skip tensor [n][c_skip][4^3] whose statistics
 * skip_stats [n][c_skip][tiles_skip][2] exist when this launch runs (the LATER producer of a GroupNorm that straddles two tensors has both
 * halves).  c_skip = 0: no table; the seven arguments after c_skip are not read.
 *
 * rf_conv3d_e2_level_supported: 1 for c = 8 .. 64 (a multiple of 4), cmid = 64, cout 64 or 128, and GroupNorm plans for which
 * rf_gn_from_stats sums with one thread per (sample, group) -- n * groups >= 1024 and at most 128 statistics entries per group, for each
 * of the two (with a table: three) GroupNorms; its other form sums in another order.  Otherwise 0: run the launches above.
 */
#ifndef RFUSE_LEVEL_H
#define RFUSE_LEVEL_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

int rf_conv3d_e2_level_supported(int n, int c, int cmid, int cout, int groups1, int groups2, int c_skip, int tiles_skip, int groups_dec);
int rf_conv3d_e2_level(const float* x, int n, int c, const float* gamma1, const float* beta1, int groups1, float eps1, const void* w1_packed, int cmid,
                       const float* gamma2, const float* beta2, int groups2, float eps2, const void* w2_packed, int cout, float* out, double* stats,
                       const double* skip_stats, int c_skip, int tiles_skip, const float* gamma_dec, const float* beta_dec, int groups_dec,
                       float eps_dec, float* dec_affine, void* stream);

#ifdef __cplusplus
}
#endif
#endif
