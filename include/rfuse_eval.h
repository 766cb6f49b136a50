/*
 * rfuse_eval.h -- the evaluation ABI of librfuse_hip.so: mesh metrics of the reference's util/mesh_metrics.py:13-120
 * (compute_iou, compute_metrics, distance_p2p, get_threshold_percentage) on the device.
 *
 * A second header beside rfuse.h, in the same vocabulary and with the same conventions (extern "C", device
 * pointers to contiguous arrays, no allocation, stream-ordered on `stream`, 0 or an RF_E_* code from every `int`
 * function whose last parameter is `stream`, rf_last_error() for the message).  rfuse.h is the inference and
 * training boundary and stays as it is; what is declared here is needed only to score a mesh.
 *
 * Types: vertices / points / normals float32 [n][3], triangles int32 [n][3] (0-based), distances float64.
 * The vocabulary has no `double` scalar: float64 values travel through device pointers, scalars as `float`.
 */
#ifndef RFUSE_EVAL_H
#define RFUSE_EVAL_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* areas[f] = 0.5 * |(v1 - v0) x (v2 - v0)| of face f, float64 arithmetic on the float32 vertices.  A face with an index
 * outside [0, n_vert) gets area 0 (and is therefore never drawn by rf_eval_sample_surface). */
int rf_eval_face_areas(const float* vertices, int n_vert, const int* triangles, int n_tri, double* areas, void* stream);

/* n surface samples, area-weighted (trimesh's mesh.sample + face_normals[idx]; util/mesh_metrics.py:29-35).
 * cdf [n_tri] float64: the inclusive prefix sum of rf_eval_face_areas.  Sample i draws Philox4x32-10 with key = seed and
 * counter = (i, 0): u (53 bits) picks the first face with cdf[f] > u * cdf[n_tri - 1], (r1, r2) (32 bits each, in (0, 1)) are
 * reflected when r1 + r2 > 1; point = v0 + r1 (v1 - v0) + r2 (v2 - v0) in float64, stored float32.  normals: the unit
 * face normal (float64 cross product, normalised, stored float32).  Faces of area 0 are never drawn.  A mesh of total
 * area 0 gives NaN points and normals and face -1.  The output depends on (mesh, n, seed) only. */
int rf_eval_sample_surface(const float* vertices, const int* triangles, const double* cdf, int n_tri, int n, int64_t seed,
                           float* points, int* face, float* normals, void* stream);

/* For every src point the exact nearest tgt point (cKDTree.query, util/mesh_metrics.py:92-93):
 *   d2[i] = min_j ((dx dx + dy dy) + dz dz), dx, dy, dz the float64 differences of the float32 coordinates, every
 *   operation rounded once (no fused multiply-add); idx[i] = the LOWEST j that attains it.
 * 1 <= n_src, n_tgt <= 2^24.  A src point with no finite distance (NaN coordinates) gets d2 = +inf, idx = 0.
 * ws: rf_eval_nearest3_ws_bytes(n_src, n_tgt) bytes (0 = sizes outside the supported range). */
int rf_eval_nearest3(const float* src, int n_src, const float* tgt, int n_tgt, double* d2, int* idx, void* ws,
                     size_t ws_bytes, void* stream);
size_t rf_eval_nearest3_ws_bytes(int n_src, int n_tgt);

/* Point-to-point statistics of one direction (util/mesh_metrics.py:84-120):
 *   dist[i] = sqrt(d2[i]) (correctly rounded); dots[i] = |n_tgt[idx[i]] . n_src[i]| with both normals renormalised in
 *   float64 (NaN when normals_src or normals_tgt is null, or idx[i] is outside [0, n_tgt));
 *   counts[t] = #{i : dist[i] <= thresholds[t]} for the n_thr ASCENDING float64 thresholds (int64);
 *   sums[0..2] = sum dist, sum dist^2 (= d2), sum dots, float64, in a fixed order (the same bits on every call).
 * d2 null: dist [n] is an INPUT (statistics of given distances; sum dist^2 then adds dist * dist); idx may be null when a normal array is.
 * ws: rf_eval_p2p_stats_ws_bytes(n). */
int rf_eval_p2p_stats(const double* d2, const int* idx, const float* normals_src, const float* normals_tgt, int n,
                      int n_tgt, const double* thresholds, int n_thr, double* dist, double* dots, int64_t* counts, double* sums,
                      void* ws, size_t ws_bytes, void* stream);
size_t rf_eval_p2p_stats_ws_bytes(int n);

/* Surface voxelisation (trimesh's mesh.voxelized(pitch).points as cells; util/mesh_metrics.py:13-21): voxel (i, j, k) is the
 * closed cube of edge `pitch` centred at pitch * (i, j, k); grid[(i - lo[0]) * dims[1] * dims[2] + (j - lo[1]) * dims[2] +
 * (k - lo[2])] is set to 1 when some triangle intersects it (13-axis separating-axis test in float64).  The grid is NOT
 * cleared: rasterise several meshes into one, or clear it first.  lo_* : the index of the grid's first cell, dim_* its edges
 * (1..2048); cells outside the grid are skipped.  Faces with an index outside [0, n_vert) or a non-finite vertex are skipped. */
int rf_eval_voxelize(const float* vertices, int n_vert, const int* triangles, int n_tri, float pitch, int lo_x, int lo_y,
                     int lo_z, int dim_x, int dim_y, int dim_z, uint8_t* grid, void* stream);

#ifdef __cplusplus
}
#endif
#endif
