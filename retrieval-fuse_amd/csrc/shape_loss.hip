// The shape loss of the reference's refinement trainer (trainer/train_refinement.py:175-183 loss_shape, :231-253 augment_batch_data / adjust_weights;
// dataset/patched_scene_dataset.py:139-146 compute_normals; model/loss.py:78-85 get_cosine_similarity) on the device; the entry points are declared in
// include/rfuse_train.h.  Built with -ffp-contract=off: the float32 expressions below are the reference's, operation by operation.
//
//   k_sobel_normals      u = v * scale + shift staged in LDS with a one-voxel halo (`pad` outside the volume), n = g / sqrt(|g|^2 + 1e-5); the
//                        augment_batch_data weights / empty mask of v in the same pass
//   k_shape_loss         one pass over pred, target, weights, empty, normals_t: df(pred) staged in LDS with a one-voxel halo, the 27 Sobel taps read
//                        from there; per-thread float64 sums (|.| W', cos) and counts, one partial per workgroup; optionally what the backward needs
//   k_shape_loss_finish  one workgroup adds the partials in a fixed order and writes the three float32 scalars and the two int64 counts
//   k_shape_loss_bwd     d pred: d cos / d g staged in LDS (three channels, zero outside the volume), the transposed stencils (= the negated ones)
//
// A workgroup of 256 threads owns a tile of 8 x 8 x 32 voxels (thread = (y, x) of the tile, a loop over its 8 z); tiles are clipped to the volume.
// The Sobel taps are accumulated in float64 (exact for float32 inputs of comparable magnitude) and rounded once: a flat neighbourhood gives g = 0
// exactly, whatever its value, which the valid mask of the loss (g != 0) depends on.
#include "common.h"
#include "../../include/rfuse_train.h"

namespace {
constexpr int kTD = 8, kTH = 8, kTW = 32;                 // tile
constexpr int kLH = kTH + 2, kLW = kTW + 2;               // LDS tile with its halo: [kTD + 2][kLH][kLW]
constexpr int kLds = (kTD + 2) * kLH * kLW;
constexpr int kThreads = kTH * kTW;
constexpr int kPartials = 4;                              // per workgroup: sum |.| W', sum cos, valid voxels, empty-on-both-sides voxels

struct Geo {
    int d, h, w, tiles_d, tiles_h, tiles_w;
};
struct Tile {
    int z0, y0, x0;
    size_t base;      // of the sample
};
__device__ __forceinline__ Tile tile_of(const Geo& g, unsigned b) {
    Tile t;
    t.x0 = (int)(b % g.tiles_w) * kTW;
    b /= g.tiles_w;
    t.y0 = (int)(b % g.tiles_h) * kTH;
    b /= g.tiles_h;
    t.z0 = (int)(b % g.tiles_d) * kTD;
    t.base = (size_t)(b / g.tiles_d) * ((size_t)g.d * g.h * g.w);
    return t;
}
// s[(lz * kLH + ly) * kLW + lx] = f(voxel index within the sample) for the tile and its halo; `outside` beyond the volume
template <class F>
__device__ __forceinline__ void stage(float* s, const Geo& g, const Tile& t, float outside, F f) {
    for (int i = threadIdx.x; i < kLds; i += kThreads) {
        const int lx = i % kLW, ly = i / kLW % kLH, lz = i / (kLW * kLH);
        const int z = t.z0 + lz - 1, y = t.y0 + ly - 1, x = t.x0 + lx - 1;
        const bool in = z >= 0 && z < g.d && y >= 0 && y < g.h && x >= 0 && x < g.w;
        s[i] = in ? f(((size_t)z * g.h + y) * g.w + x) : outside;
    }
}
// the cross-correlation with sobel_3d_x (AX 0: derivative along z), _y (1: along y), _z (2: along x) at LDS position c, in float64
template <int AX>
__device__ __forceinline__ double sobel(const float* s, int c) {
    double acc = 0.0;
#pragma unroll
    for (int kd = 0; kd < 3; ++kd)
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int sm_d = kd == 1 ? 2 : 1, sm_h = kh == 1 ? 2 : 1, sm_w = kw == 1 ? 2 : 1;
                const int wt = AX == 0 ? (1 - kd) * sm_h * sm_w : AX == 1 ? sm_d * (1 - kh) * sm_w : sm_d * sm_h * (kw - 1);
                if (wt != 0) acc += (double)wt * (double)s[c + ((kd - 1) * kLH + (kh - 1)) * kLW + (kw - 1)];
            }
    return acc;
}
__device__ __forceinline__ float norm3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }
}   // namespace

__global__ __launch_bounds__(kThreads) void k_sobel_normals(const float* __restrict__ v, Geo g, float scale, float shift, float pad, float thr,
                                                            float w_occ_minus_1, float* __restrict__ normals, float* __restrict__ weights,
                                                            uint8_t* __restrict__ empty) {
    __shared__ float s[kLds];
    const Tile t = tile_of(g, blockIdx.x);
    const float* vb = v + t.base;
    stage(s, g, t, pad, [&](size_t i) { return vb[i] * scale + shift; });
    __syncthreads();
    const int ly = threadIdx.x / kTW, lx = threadIdx.x % kTW, y = t.y0 + ly, x = t.x0 + lx;
    if (y >= g.h || x >= g.w) return;
    const size_t vol = (size_t)g.d * g.h * g.w;
    for (int lz = 0; lz < kTD && t.z0 + lz < g.d; ++lz) {
        const size_t i = ((size_t)(t.z0 + lz) * g.h + y) * g.w + x;
        const int c = ((lz + 1) * kLH + ly + 1) * kLW + lx + 1;
        const float gx = (float)sobel<0>(s, c), gy = (float)sobel<1>(s, c), gz = (float)sobel<2>(s, c);
        const float nrm = sqrtf(((gx * gx + gy * gy) + gz * gz) + 1e-5f);
        float* o = normals + 3 * t.base + i;
        o[0] = gx / nrm;
        o[vol] = gy / nrm;
        o[2 * vol] = gz / nrm;
        const float tv = vb[i];
        if (weights) weights[t.base + i] = 1.f + (tv < thr ? 1.f : 0.f) * w_occ_minus_1;
        if (empty) empty[t.base + i] = tv >= thr ? 1 : 0;
    }
}

__global__ __launch_bounds__(kThreads) void k_shape_loss(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ weights,
                                                         const uint8_t* __restrict__ empty, const float* __restrict__ normals_t, Geo g, float trunc,
                                                         float mean, float std, int do_l1, int do_normal, float* __restrict__ grad_l1,
                                                         float* __restrict__ grad_g, double* __restrict__ partial) {
    __shared__ float s[kLds];
    __shared__ double red[kThreads / 64][kPartials];
    const Tile t = tile_of(g, blockIdx.x);
    const float* pb = pred + t.base;
    if (do_normal) {
        stage(s, g, t, trunc, [&](size_t i) { return (pb[i] + 1.f) * trunc / 2.f; });
        __syncthreads();
    }
    const int ly = threadIdx.x / kTW, lx = threadIdx.x % kTW, y = t.y0 + ly, x = t.x0 + lx;
    const size_t vol = (size_t)g.d * g.h * g.w;
    double sum_l1 = 0.0, sum_cos = 0.0, n_valid = 0.0, n_both = 0.0;
    if (y < g.h && x < g.w) {
        for (int lz = 0; lz < kTD && t.z0 + lz < g.d; ++lz) {
            const size_t i = ((size_t)(t.z0 + lz) * g.h + y) * g.w + x;
            const float p = pb[i];
            const float df = (p + 1.f) * trunc / 2.f;
            const bool both = empty[t.base + i] != 0 && df >= trunc;
            n_both += both ? 1.0 : 0.0;
            if (do_l1) {
                const float den = target[t.base + i] * std + mean;
                const float tn = 2.f * (den / trunc) - 1.f;
                const float wp = both ? 0.f : weights[t.base + i];
                const float diff = p - tn;
                sum_l1 += (double)(fabsf(diff) * wp);
                if (grad_l1) grad_l1[t.base + i] = (float)((0.f < diff) - (diff < 0.f)) * wp;
            }
            if (do_normal) {
                const int c = ((lz + 1) * kLH + ly + 1) * kLW + lx + 1;
                const float gx = (float)sobel<0>(s, c), gy = (float)sobel<1>(s, c), gz = (float)sobel<2>(s, c);
                const float nrm = sqrtf(((gx * gx + gy * gy) + gz * gz) + 1e-5f);
                const float nx = gx / nrm, ny = gy / nrm, nz = gz / nrm;
                const float* q = normals_t + 3 * t.base + i;
                const float tx = q[0], ty = q[vol], tz = q[2 * vol];
                const float pn = norm3(nx, ny, nz), tl = norm3(tx, ty, tz);
                const bool valid = pn != 0.f && tl != 0.f;          // a NaN norm counts as valid, as `!=` does in the reference
                float dgx = 0.f, dgy = 0.f, dgz = 0.f;
                if (valid) {
                    const float pd = fmaxf(pn, 1e-12f), td = fmaxf(tl, 1e-12f);
                    sum_cos += (double)(((nx / pd) * (tx / td) + (ny / pd) * (ty / td)) + (nz / pd) * (tz / td));
                    n_valid += 1.0;
                    if (grad_g) {      // d cos / d g = (t^ - g^ (g^ . t^)) / |g|, float64 from the float32 g and normals_t, stored float32
                        const double gl = sqrt(((double)gx * gx + (double)gy * gy) + (double)gz * gz);
                        const double tl64 = sqrt(((double)tx * tx + (double)ty * ty) + (double)tz * tz);
                        const double ux = gx / gl, uy = gy / gl, uz = gz / gl, bx = tx / tl64, by = ty / tl64, bz = tz / tl64;
                        const double dot = (ux * bx + uy * by) + uz * bz;
                        dgx = (float)((bx - ux * dot) / gl);
                        dgy = (float)((by - uy * dot) / gl);
                        dgz = (float)((bz - uz * dot) / gl);
                    }
                }
                if (grad_g) {
                    float* o = grad_g + 3 * t.base + i;
                    o[0] = dgx;
                    o[vol] = dgy;
                    o[2 * vol] = dgz;
                }
            }
        }
    }
    rf_waves_put(red, {wave_sum(sum_l1), wave_sum(sum_cos), wave_sum(n_valid), wave_sum(n_both)});
    if (threadIdx.x < kPartials) partial[(size_t)blockIdx.x * kPartials + threadIdx.x] = rf_waves_sum(red, threadIdx.x);
}

// one workgroup: thread k adds the partials of workgroups k, k + 256, ... in ascending order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void k_shape_loss_finish(const double* __restrict__ partial, int n_partial, double n_voxels, float lambda_rec,
                                                           float lambda_n, int do_l1, int do_normal, float* __restrict__ out, long long* __restrict__ counts) {
    __shared__ double red[256][kPartials];
    double acc[kPartials] = {0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < n_partial; b += 256)
#pragma unroll
        for (int k = 0; k < kPartials; ++k) acc[k] += partial[(size_t)b * kPartials + k];
    rf_tree_sum(red, acc);
    if (threadIdx.x == 0) {
        const float l1 = do_l1 ? (float)(red[0][0] / n_voxels) : 0.f;
        const float normal = do_normal ? 1.f - (float)(red[0][1] / red[0][2]) : 0.f;      // no valid voxel: 0 / 0 = NaN, as the reference's mean of nothing
        out[0] = lambda_rec * l1 + lambda_n * normal;
        out[1] = l1;
        out[2] = normal;
        counts[0] = (long long)red[0][2];
        counts[1] = (long long)red[0][3];
    }
}

__global__ __launch_bounds__(kThreads) void k_shape_loss_bwd(const float* __restrict__ grad_l1, const float* __restrict__ grad_g,
                                                             const float* __restrict__ coef, const long long* __restrict__ counts, Geo g, float trunc,
                                                             double n_voxels, float* __restrict__ dpred) {
    __shared__ float s[3][kLds];
    const Tile t = tile_of(g, blockIdx.x);
    const size_t vol = (size_t)g.d * g.h * g.w;
    const long long n_valid = counts[0];
    const bool with_normal = grad_g != nullptr && n_valid > 0;          // uniform over the launch
    if (with_normal) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* gb = grad_g + 3 * t.base + ch * vol;
            stage(s[ch], g, t, 0.f, [&](size_t i) { return gb[i]; });
        }
        __syncthreads();
    }
    const int ly = threadIdx.x / kTW, lx = threadIdx.x % kTW, y = t.y0 + ly, x = t.x0 + lx;
    if (y >= g.h || x >= g.w) return;
    const double ca = grad_l1 ? (double)coef[0] / n_voxels : 0.0;
    const double cb = with_normal ? (double)coef[1] * (double)(trunc / 2.f) / (double)n_valid : 0.0;
    for (int lz = 0; lz < kTD && t.z0 + lz < g.d; ++lz) {
        const size_t i = ((size_t)(t.z0 + lz) * g.h + y) * g.w + x;
        double acc = grad_l1 ? ca * (double)grad_l1[t.base + i] : 0.0;
        if (with_normal) {
            const int c = ((lz + 1) * kLH + ly + 1) * kLW + lx + 1;
            // normal = 1 - mean cos and the transposed stencils are the negated ones: the two signs cancel
            acc += cb * ((sobel<0>(s[0], c) + sobel<1>(s[1], c)) + sobel<2>(s[2], c));
        }
        dpred[t.base + i] = (float)acc;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
namespace {
// 0 = outside the supported range: d * h * w <= 2^31 - 1 and at most 2^31 - 1 tiles over the batch
long long tiles_of(int n, int d, int h, int w, Geo* g) {
    if (n < 1 || d < 1 || h < 1 || w < 1) return 0;
    if ((long long)d * h * w > 0x7fffffffll) return 0;
    const long long td = (d + kTD - 1) / kTD, th = (h + kTH - 1) / kTH, tw = (w + kTW - 1) / kTW;
    const long long tiles = td * th * tw * n;
    if (tiles > 0x7fffffffll) return 0;
    if (g) *g = Geo{d, h, w, (int)td, (int)th, (int)tw};
    return tiles;
}
}   // namespace

extern "C" int rf_train_sobel_normals(const float* v, int n, int d, int h, int w, float scale, float shift, float pad, float thr, float w_occ_minus_1,
                                      float* normals, float* weights, uint8_t* empty, void* stream) {
    RF_REQUIRE(v && normals && n >= 1 && d >= 1 && h >= 1 && w >= 1, RF_E_INVALID, "rf_train_sobel_normals: bad arguments");
    Geo g;
    const long long tiles = tiles_of(n, d, h, w, &g);
    RF_REQUIRE(tiles > 0, RF_E_UNSUPPORTED, "rf_train_sobel_normals: %d volumes of %d x %d x %d voxels (at most 2^31 - 1 voxels per volume and tiles per batch)", n,
               d, h, w);
    return rf_launch<k_sobel_normals>("rf_train_sobel_normals", dim3((unsigned)tiles), dim3(kThreads), (hipStream_t)stream, v, g, scale, shift, pad, thr,
                                      w_occ_minus_1, normals, weights, empty);
}

extern "C" size_t rf_train_shape_loss_ws_bytes(int n, int d, int h, int w) {
    const long long tiles = tiles_of(n, d, h, w, nullptr);
    return tiles > 0 ? (((size_t)tiles * kPartials * sizeof(double)) + 255) & ~(size_t)255 : 0;
}

extern "C" int rf_train_shape_loss(const float* pred, const float* target, const float* weights, const uint8_t* empty, const float* normals_t, int n, int d,
                                   int h, int w, float trunc, float mean, float std, float lambda_rec, float lambda_n, float* out, int64_t* counts,
                                   float* grad_l1, float* grad_g, void* ws, size_t ws_bytes, void* stream) {
    RF_REQUIRE(pred && target && weights && empty && normals_t && out && counts && ws && n >= 1 && d >= 1 && h >= 1 && w >= 1, RF_E_INVALID,
               "rf_train_shape_loss: bad arguments");
    RF_REQUIRE((grad_l1 == nullptr) == (grad_g == nullptr), RF_E_INVALID, "rf_train_shape_loss: grad_l1 and grad_g come together or not at all");
    Geo g;
    const long long tiles = tiles_of(n, d, h, w, &g);
    RF_REQUIRE(tiles > 0, RF_E_UNSUPPORTED, "rf_train_shape_loss: %d volumes of %d x %d x %d voxels (at most 2^31 - 1 voxels per volume and tiles per batch)", n, d,
               h, w);
    const size_t need = rf_train_shape_loss_ws_bytes(n, d, h, w);
    RF_REQUIRE(ws_bytes >= need, RF_E_WORKSPACE, "rf_train_shape_loss: workspace of %zu bytes, needs %zu", ws_bytes, need);
    const int do_l1 = lambda_rec > 0.f, do_normal = lambda_n > 0.f;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = rf_launch<k_shape_loss>("rf_train_shape_loss", dim3((unsigned)tiles), dim3(kThreads), s, pred, target, weights, empty, normals_t, g, trunc, mean, std,
                                         do_l1, do_normal, grad_l1, grad_g, reinterpret_cast<double*>(ws)))
        return rc;
    return rf_launch<k_shape_loss_finish>("rf_train_shape_loss (finish)", dim3(1), dim3(256), s, reinterpret_cast<const double*>(ws), (int)tiles,
                                          (double)n * d * h * w, lambda_rec, lambda_n, do_l1, do_normal, out, reinterpret_cast<long long*>(counts));
}

extern "C" int rf_train_shape_loss_backward(const float* grad_l1, const float* grad_g, const float* coef, const int64_t* counts, int n, int d, int h, int w,
                                            float trunc, float* dpred, void* stream) {
    RF_REQUIRE(coef && counts && dpred && n >= 1 && d >= 1 && h >= 1 && w >= 1, RF_E_INVALID, "rf_train_shape_loss_backward: bad arguments");
    Geo g;
    const long long tiles = tiles_of(n, d, h, w, &g);
    RF_REQUIRE(tiles > 0, RF_E_UNSUPPORTED,
               "rf_train_shape_loss_backward: %d volumes of %d x %d x %d voxels (at most 2^31 - 1 voxels per volume and tiles per batch)", n, d, h, w);
    return rf_launch<k_shape_loss_bwd>("rf_train_shape_loss_backward", dim3((unsigned)tiles), dim3(kThreads), (hipStream_t)stream, grad_l1, grad_g, coef,
                                       reinterpret_cast<const long long*>(counts), g, trunc, (double)n * d * h * w, dpred);
}
