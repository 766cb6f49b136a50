/*
 * rfuse_data.h -- the dataset ABI of librfuse_hip.so: what the reference's SceneHandler and PatchedSceneDataset (dataset/scene.py,
 * dataset/patched_scene_dataset.py) do per item on the host, for a whole batch on the device: the occupancy count of a target window
 * (scene.py:148-150), the normalised input / target / retrieval windows of __getitem__ (patched_scene_dataset.py:117-137), and the occupancy grid of
 * a sampled point cloud (scene.py:81-90, util/misc.py:73-78 point_cloud_to_grid).
 *
 * A sixth header, in the vocabulary and with the conventions of the other five (extern "C", device pointers to contiguous arrays, no allocation,
 * stream-ordered on `stream`, 0 or an RF_E_* code from every `int` function whose last parameter is `stream`, rf_last_error() for the message, no
 * `double` scalar, argument checks before any device is touched).  The other headers stay as they are.
 *
 * One addressing scheme for all three.  A store is one flat array per field; scene s occupies the elements from offsets[s] (int64, in elements of
 * the store's type), `channels` volumes of sizes[s] = (X, Y, Z) voxels each (int32 [n_scenes][3], z fastest), UNPADDED; scenes need not be one size.
 * An item is four int32 (scene, x0, y0, z0): the start of its window in PADDED coordinates, i.e. voxel (x, y, z) of the window is voxel
 * (x0 + x - pad, y0 + y - pad, z0 + z - pad) of the scene, and every voxel outside the scene has the value `fill` (the reference pads its scenes with
 * the truncation).  The kernels read nothing outside [offsets[s], offsets[s] + channels * X * Y * Z): an item whose scene is outside [0, n_scenes)
 * counts 0 / is written as `fill`, whatever its window.  Whether a window leaves the padded scene is the caller's check (the items are his).
 *
 * Supported: 1 <= m <= 2^20, 1 <= window <= 256, 0 <= pad <= 256, 1 <= channels <= 64, m * channels * window^3 < 2^31, 1 <= points <= 2^20;
 * otherwise RF_E_UNSUPPORTED.  Integer sums and plain stores, no atomics: the same bits on every call.
 */
#ifndef RFUSE_DATA_H
#define RFUSE_DATA_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* counts int32 [m]: the voxels of each item's window^3 whose value, as float32, is <= thr; a voxel outside the scene counts iff fill <= thr.
 * store_f32 0: float16 store, 1: float32 store.  NaN is unoccupied. */
int rf_data_occupancy(const void* store, int store_f32, const int64_t* offsets, const int* sizes, int n_scenes, const int* items, int m, int window,
                      int pad, float fill, float thr, int* counts, void* stream);

/* out float32 [m][channels][window^3].  normalise 1: (v - mean) / std, one float32 subtract and one correctly rounded float32 divide (no
 * reciprocal, no FMA), v the stored value as float32 or `fill`; normalise 0: v itself (mean and std are not read). */
int rf_data_gather(const void* store, int store_f32, const int64_t* offsets, const int* sizes, int n_scenes, int channels, const int* items, int m,
                   int window, int pad, float fill, int normalise, float mean, float std, float* out, void* stream);

/* Point clouds to occupancy windows.  clouds: one flat array of rows of 3 coordinates, float32 (cloud_f64 0) or float64 (1); scene s owns rows[s]
 * rows from row offsets[s] (int64).  A cloud with fewer than 20000 rows is read as stacked twice: row i >= rows[s] is row i - rows[s].  table:
 * [table_rows][points] row indices, uint16 (table_kind 0), int32 (1) or int64 (2); item i samples the cloud of its scene with table row
 * item_rows[i] (int32 [m]).  Per sampled point and axis: p * scale in the cloud's own type, clip to [0, grid_res - 1], truncate toward zero, + pad:
 * a voxel of the padded grid of (grid_res + 2 pad)^3.  out float32 [m][window^3]: the item's window of that grid, 1 where a point fell and 0
 * elsewhere (the padding included), then (g - mean) / std as above when normalise is 1.  A point with a NaN coordinate is skipped; +-inf clips.
 * A table row outside [0, table_rows) or an index at or beyond the (doubled) cloud is skipped: registering the table is where they are refused.
 * Two launches: a fill, then one store per point that falls into the window (all of one value, so the order does not matter). */
int rf_data_points(const void* clouds, int cloud_f64, const int64_t* offsets, const int* rows, int n_scenes, const void* table, int table_kind,
                   int table_rows, int points, const int* items, const int* item_rows, int m, int window, int grid_res, int pad, float scale,
                   int normalise, float mean, float std, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
