// Host side of the split-operand conv entry points (conv3d_split.hip; conv3d_split_zc.hip's launchers take what these build): the ConvArgs of a layer,
// its output forms and the refusals about output pointers, each written once.  The SplitPreOut forms are SplitPreOut::presplit / ::pointwise.
#pragma once
#include <math.h>
#include "conv_box.h"
#include "conv_split_common.h"

// a split-operand layer: every field set, the output side off, ReLU.  src: fp32 NCDHW (or channel-interleaved), or a pre-split tensor (affine = null)
static inline ConvArgs split_conv_args(const void* src, int cin, int n, int edge, const float* gn_affine, const void* w_packed, int cout) {
    ConvArgs a;
    a.src0 = reinterpret_cast<const float*>(src); a.src1 = nullptr; a.affine = reinterpret_cast<const float4*>(gn_affine);
    a.wp = reinterpret_cast<const float*>(w_packed); a.out = nullptr;
    a.c0 = cin; a.c1 = 0; a.n = n; a.edge = edge; a.cout = cout; a.cin4 = cin; a.cout16 = rf_round_up(cout, 16);
    a.stats = nullptr; a.stats_tiles = 0; a.pool_out = nullptr; a.pool_stats = nullptr; a.pool_mode = 0; a.floor = 0.f; a.src_pm = 0;
    return a;
}
// full-resolution and / or pooled output, each with optional statistics in `tiles` tiles per (sample, cout)
static inline ConvArgs split_with_outputs(ConvArgs a, float* out, double* stats, float* pool_out, double* pool_stats, int tiles) {
    a.out = out; a.stats = reinterpret_cast<double2*>(stats); a.pool_out = pool_out; a.pool_stats = reinterpret_cast<double2*>(pool_stats);
    a.stats_tiles = (stats || pool_stats) ? tiles : 0;
    a.pool_mode = pool_out ? (out ? 1 : 2) : 0;
    return a;
}
// the output handed over pre-split (SplitPreOut::presplit): optional statistics [n][cout] of the ReLU'd tensor that is not written
static inline ConvArgs split_with_handover_stats(ConvArgs a, double* stats) { return split_with_outputs(a, nullptr, stats, nullptr, nullptr, 1); }
// the plain operator of the training slice's data gradient: full output alone, ReLU optional (floor = -inf: none)
static inline ConvArgs split_with_plain_output(ConvArgs a, float* out, int relu) {
    a.out = out; a.floor = relu ? 0.f : -INFINITY;
    return a;
}
// the pre-split source has its voxel slots in parity-major order (ConvArgs::src_pm)
static inline ConvArgs split_from_parity_major(ConvArgs a) { a.src_pm = 1; return a; }

// The pointer refusals of entry point `who`: `inputs` = all its required inputs are non-null; an output (full or pooled); statistics only of an output
// that is written.  Entry points with one output pass it as `out` and nulls for the pooled pair.
static inline int split_check_pointers(const char* who, bool inputs, const void* out, const void* stats, const void* pool_out, const void* pool_stats) {
    RF_REQUIRE(inputs && (out || pool_out), RF_E_INVALID, "%s: null pointer", who);
    RF_REQUIRE(out || !stats, RF_E_INVALID, "%s: statistics of an output that is not written", who);
    RF_REQUIRE(pool_out || !pool_stats, RF_E_INVALID, "%s: pooled statistics without a pooled output", who);
    return RF_OK;
}
