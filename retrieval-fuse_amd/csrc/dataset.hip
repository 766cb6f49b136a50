// The device side of the patch dataset (reference dataset/scene.py, dataset/patched_scene_dataset.py, util/misc.py:73-78): occupancy counts of target
// windows, the normalised windows of a batch, and the occupancy windows of sampled point clouds.  The entry points and the addressing scheme (flat stores,
// per-scene offsets and sizes, items = scene + window start in padded coordinates) are declared in include/rfuse_data.h.
//
//   k_data_occupancy   one workgroup of 4 waves per item: a wave tests 64 voxels of the window per step (__ballot + popcount, as k_iou_pack does), the
//                      waves' counts are added through LDS.  Voxels outside the scene take the verdict of the fill.
//   k_data_gather      one thread per V consecutive voxels of a z row of the output (V = 4 where the window is a multiple of 4: one 16-byte store; V = 1
//                      otherwise); the reads are scalar, a window starts anywhere in its scene.  (v - mean) / std as a subtract and an IEEE divide: the file
//                      is built with -ffp-contract=off, and hipcc's float `/` is correctly rounded.
//   k_data_fill        out[i] = the value of an empty voxel, (0 - mean) / std with the 0 a kernel argument (see there)
//   k_data_points      one thread per (item, sampled point): table row -> cloud row -> voxel of the padded grid -> a store of (1 - mean) / std when the voxel
//                      lies in the item's window.  Points that share a voxel store the same value: the result does not depend on their order.
//
// Every index is checked against what it addresses inside the kernels (scene, table row, cloud row, window), so a wrong item reads and writes nothing out
// of bounds; the callers' checks decide what is an error.
#include "common.h"
#include "../../include/rfuse_data.h"

namespace {
constexpr int kMaxItems = 1 << 20, kMaxWindow = 256, kMaxPad = 256, kMaxChannels = 64, kMaxPoints = 1 << 20;
constexpr long long kMaxOut = (1ll << 31) - 1;
constexpr int kOccThreads = 256, kOccWaves = kOccThreads / 64;
constexpr int kThreads = 256;
constexpr int kDoubledBelow = 20000;                 // scene.py:86-87: a cloud with fewer rows is stacked twice

const char* kRange = "%s: %d items of %d channels, window %d, pad %d (1 <= items <= 2^20, 1 <= window <= 256, 0 <= pad <= 256, 1 <= channels <= 64, "
                     "items * channels * window^3 < 2^31)";
bool in_range(int m, int channels, int window, int pad) {
    if (m < 1 || m > kMaxItems || window < 1 || window > kMaxWindow || pad < 0 || pad > kMaxPad || channels < 1 || channels > kMaxChannels) return false;
    return (long long)m * channels * window * window * window <= kMaxOut;
}

template <bool F32> __device__ __forceinline__ float load_value(const void* store, long long i) {
    if (F32) return reinterpret_cast<const float*>(store)[i];
    return (float)reinterpret_cast<const _Float16*>(store)[i];
}

struct Scene {
    long long off;
    int X, Y, Z, ox, oy, oz;      // sizes; the scene coordinate of the window's first voxel
    bool ok;
};
__device__ __forceinline__ Scene scene_of(const long long* offsets, const int* sizes, int n_scenes, const int* items, int item, int pad) {
    Scene s;
    const int sc = items[4 * item];
    s.ok = sc >= 0 && sc < n_scenes;
    const int q = s.ok ? sc : 0;
    s.off = offsets[q];
    s.X = sizes[3 * q], s.Y = sizes[3 * q + 1], s.Z = sizes[3 * q + 2];
    s.ox = items[4 * item + 1] - pad, s.oy = items[4 * item + 2] - pad, s.oz = items[4 * item + 3] - pad;
    return s;
}
}   // namespace

template <bool F32>
__global__ __launch_bounds__(kOccThreads) void k_data_occupancy(const void* __restrict__ store, const long long* __restrict__ offsets, const int* __restrict__ sizes,
                                                                int n_scenes, const int* __restrict__ items, int w, int pad, float fill, float thr,
                                                                int* __restrict__ counts) {
    __shared__ int part[kOccWaves][1];
    const int item = blockIdx.x;
    const Scene s = scene_of(offsets, sizes, n_scenes, items, item, pad);
    const unsigned w2 = (unsigned)w * w, w3 = w2 * w;
    const bool fill_on = fill <= thr;                 // NaN: unoccupied
    int cnt = 0;
    for (unsigned base = 0; base < w3; base += kOccThreads) {
        const unsigned v = base + threadIdx.x;
        bool on = false;
        if (v < w3 && s.ok) {
            const unsigned x = v / w2, r = v - x * w2, y = r / w, z = r - y * w;
            const int sx = s.ox + (int)x, sy = s.oy + (int)y, sz = s.oz + (int)z;
            if (sx >= 0 && sx < s.X && sy >= 0 && sy < s.Y && sz >= 0 && sz < s.Z)
                on = load_value<F32>(store, s.off + ((long long)sx * s.Y + sy) * s.Z + sz) <= thr;
            else
                on = fill_on;
        }
        cnt += __popcll(__ballot(on));
    }
    rf_waves_put(part, {cnt});
    if (threadIdx.x == 0) counts[item] = rf_waves_sum(part);
}

template <bool F32, int V>
__global__ __launch_bounds__(kThreads) void k_data_gather(const void* __restrict__ store, const long long* __restrict__ offsets, const int* __restrict__ sizes, int n_scenes,
                                                          int channels, const int* __restrict__ items, unsigned total, int w, int pad, float fill, int normalise,
                                                          float mean, float std, float* __restrict__ out) {
    const unsigned w2 = (unsigned)w * w, w3 = w2 * w;
    for (unsigned g = blockIdx.x * kThreads + threadIdx.x; g < total / V; g += gridDim.x * kThreads) {
        const unsigned e = g * V;
        const unsigned row = e / w3, v = e - row * w3;
        const unsigned item = row / channels, c = row - item * channels;
        const unsigned x = v / w2, r = v - x * w2, y = r / w, z = r - y * w;
        const Scene s = scene_of(offsets, sizes, n_scenes, items, (int)item, pad);
        const int sx = s.ox + (int)x, sy = s.oy + (int)y;
        const bool row_in = s.ok && sx >= 0 && sx < s.X && sy >= 0 && sy < s.Y;
        const long long at = s.off + (((long long)c * s.X + sx) * s.Y + sy) * s.Z;
        float val[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int sz = s.oz + (int)z + k;
            float t = fill;
            if (row_in && sz >= 0 && sz < s.Z) t = load_value<F32>(store, at + sz);
            val[k] = normalise ? (t - mean) / std : t;
        }
        if (V == 4) {
            f32x4 q;
            q[0] = val[0], q[1] = val[1 % V], q[2] = val[2 % V], q[3] = val[3 % V];
            *reinterpret_cast<f32x4*>(out + e) = q;
        } else {
            out[e] = val[0];
        }
    }
}

// `empty` (0) and `set` (1) are kernel arguments: with a literal 0 the compiler turns 0.f - mean into -mean, which is -0 for a mean of 0 where numpy has +0
__global__ __launch_bounds__(kThreads) void k_data_fill(float* __restrict__ out, unsigned total, float empty, int normalise, float mean, float std) {
    const float zero = normalise ? (empty - mean) / std : empty;
    for (unsigned e = blockIdx.x * kThreads + threadIdx.x; e < total; e += gridDim.x * kThreads) out[e] = zero;
}

template <class T> __device__ __forceinline__ bool voxel_of(T p, T scale, int grid_res, int* q) {
    T v = p * scale;                                  // in the cloud's own type
    if (v != v) return false;                         // NaN: no voxel
    v = v < (T)0 ? (T)0 : v;                          // np.clip(., 0, grid_res - 1); -0.0 stays a zero
    v = v > (T)(grid_res - 1) ? (T)(grid_res - 1) : v;
    *q = (int)v;                                      // astype(np.uint32) of a value in [0, grid_res - 1]: truncation
    return true;
}

template <bool F64>
__global__ __launch_bounds__(kThreads) void k_data_points(const void* __restrict__ clouds, const long long* __restrict__ offsets, const int* __restrict__ rows, int n_scenes,
                                                          const void* __restrict__ table, int table_kind, int table_rows, int points, const int* __restrict__ items,
                                                          const int* __restrict__ item_rows, unsigned total, int w, int grid_res, int pad, float scale,
                                                          float set, int normalise, float mean, float std, float* __restrict__ out) {
    const float one = normalise ? (set - mean) / std : set;
    const size_t w3 = (size_t)w * w * w;
    for (unsigned t = blockIdx.x * kThreads + threadIdx.x; t < total; t += gridDim.x * kThreads) {
        const unsigned item = t / points, j = t - item * points;
        const int sc = items[4 * item], trow = item_rows[item];
        if (sc < 0 || sc >= n_scenes || trow < 0 || trow >= table_rows) continue;
        const size_t ti = (size_t)trow * points + j;
        long long i = table_kind == 0 ? (long long)reinterpret_cast<const uint16_t*>(table)[ti]
                    : table_kind == 1 ? (long long)reinterpret_cast<const int*>(table)[ti] : reinterpret_cast<const long long*>(table)[ti];
        const int n = rows[sc];
        if (i >= n && n < kDoubledBelow) i -= n;      // np.vstack([pc, pc])
        if (i < 0 || i >= n) continue;
        const long long at = (offsets[sc] + i) * 3;
        int q[3];
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (F64) ok = voxel_of<double>(reinterpret_cast<const double*>(clouds)[at + a], (double)scale, grid_res, &q[a]) && ok;
            else ok = voxel_of<float>(reinterpret_cast<const float*>(clouds)[at + a], scale, grid_res, &q[a]) && ok;
        }
        if (!ok) continue;
        const int x = q[0] + pad - items[4 * item + 1], y = q[1] + pad - items[4 * item + 2], z = q[2] + pad - items[4 * item + 3];
        if (x < 0 || x >= w || y < 0 || y >= w || z < 0 || z >= w) continue;
        out[item * w3 + ((size_t)x * w + y) * w + z] = one;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int rf_data_occupancy(const void* store, int store_f32, const int64_t* offsets, const int* sizes, int n_scenes, const int* items, int m, int window,
                                 int pad, float fill, float thr, int* counts, void* stream) {
    RF_REQUIRE(store && offsets && sizes && items && counts && n_scenes >= 1 && m >= 1 && window >= 1 && pad >= 0 && (store_f32 == 0 || store_f32 == 1), RF_E_INVALID,
               "rf_data_occupancy: bad arguments");
    RF_REQUIRE(in_range(m, 1, window, pad), RF_E_UNSUPPORTED, kRange, "rf_data_occupancy", m, 1, window, pad);
    const long long* off = reinterpret_cast<const long long*>(offsets);
    if (store_f32)
        return rf_launch<k_data_occupancy<true>>("rf_data_occupancy", dim3((unsigned)m), dim3(kOccThreads), (hipStream_t)stream, store, off, sizes, n_scenes, items, window,
                                                 pad, fill, thr, counts);
    return rf_launch<k_data_occupancy<false>>("rf_data_occupancy", dim3((unsigned)m), dim3(kOccThreads), (hipStream_t)stream, store, off, sizes, n_scenes, items, window,
                                              pad, fill, thr, counts);
}

extern "C" int rf_data_gather(const void* store, int store_f32, const int64_t* offsets, const int* sizes, int n_scenes, int channels, const int* items, int m,
                              int window, int pad, float fill, int normalise, float mean, float std, float* out, void* stream) {
    RF_REQUIRE(store && offsets && sizes && items && out && n_scenes >= 1 && channels >= 1 && m >= 1 && window >= 1 && pad >= 0 && (store_f32 == 0 || store_f32 == 1) &&
                   (normalise == 0 || normalise == 1),
               RF_E_INVALID, "rf_data_gather: bad arguments");
    RF_REQUIRE(in_range(m, channels, window, pad), RF_E_UNSUPPORTED, kRange, "rf_data_gather", m, channels, window, pad);
    const long long* off = reinterpret_cast<const long long*>(offsets);
    const unsigned total = (unsigned)((long long)m * channels * window * window * window);
    const bool vec = window % 4 == 0;
    const dim3 grid(rf_blocks(total / (vec ? 4 : 1), kThreads, 1u << 20)), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
#define RF_DATA_GATHER(F32, V) \
    return rf_launch<k_data_gather<F32, V>>("rf_data_gather", grid, block, st, store, off, sizes, n_scenes, channels, items, total, window, pad, fill, normalise, mean, std, out)
    if (store_f32) {
        if (vec) RF_DATA_GATHER(true, 4);
        RF_DATA_GATHER(true, 1);
    }
    if (vec) RF_DATA_GATHER(false, 4);
    RF_DATA_GATHER(false, 1);
#undef RF_DATA_GATHER
}

extern "C" int rf_data_points(const void* clouds, int cloud_f64, const int64_t* offsets, const int* rows, int n_scenes, const void* table, int table_kind,
                              int table_rows, int points, const int* items, const int* item_rows, int m, int window, int grid_res, int pad, float scale,
                              int normalise, float mean, float std, float* out, void* stream) {
    RF_REQUIRE(clouds && offsets && rows && table && items && item_rows && out && n_scenes >= 1 && table_rows >= 1 && points >= 1 && m >= 1 && window >= 1 && grid_res >= 1 &&
                   pad >= 0 && (cloud_f64 == 0 || cloud_f64 == 1) && table_kind >= 0 && table_kind <= 2 && (normalise == 0 || normalise == 1),
               RF_E_INVALID, "rf_data_points: bad arguments");
    RF_REQUIRE(in_range(m, 1, window, pad) && points <= kMaxPoints && (long long)m * points <= kMaxOut && grid_res <= (1 << 20), RF_E_UNSUPPORTED,
               "rf_data_points: %d items of %d points, window %d, pad %d, grid %d (1 <= items <= 2^20, 1 <= window <= 256, 0 <= pad <= 256, 1 <= points <= 2^20, "
               "items * window^3 and items * points < 2^31, grid <= 2^20)",
               m, points, window, pad, grid_res);
    const long long* off = reinterpret_cast<const long long*>(offsets);
    hipStream_t st = (hipStream_t)stream;
    const unsigned total = (unsigned)((long long)m * window * window * window), pts = (unsigned)((long long)m * points);
    if (int rc = rf_launch<k_data_fill>("rf_data_points", dim3(rf_blocks(total, kThreads, 1u << 16)), dim3(kThreads), st, out, total, 0.f, normalise, mean, std)) return rc;
    const dim3 grid(rf_blocks(pts, kThreads, 1u << 16)), block(kThreads);
    if (cloud_f64)
        return rf_launch<k_data_points<true>>("rf_data_points", grid, block, st, clouds, off, rows, n_scenes, table, table_kind, table_rows, points, items, item_rows, pts,
                                              window, grid_res, pad, scale, 1.f, normalise, mean, std, out);
    return rf_launch<k_data_points<false>>("rf_data_points", grid, block, st, clouds, off, rows, n_scenes, table, table_kind, table_rows, points, items, item_rows, pts,
                                           window, grid_res, pad, scale, 1.f, normalise, mean, std, out);
}
