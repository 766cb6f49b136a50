// The two kernels a refinement training step adds to the library (include/rfuse_step.h).
//
//   k_pwt_backward   backward of the decoder's head, tanh(sum_c w[c] h[c] + b): memory-bound -- h read once, dh written once, out and dout read once per
//                    chunk of kChunk channels (one chunk at the shipped widths 12 and 16).  A thread takes a quad of four consecutive voxels: the
//                    16-byte loads of all the chunk's channels are issued before the first use, w sits in scalar registers, g = dout * (1 - out^2) is
//                    rounded once and feeds dh = g * w[c] and the float64 sums of dw[c] and db.  Those sums: per thread over its quads, wave_sum,
//                    rf_waves_put / rf_waves_sum (wave order), one partial per workgroup and output in `ws`.
//   k_pwt_finish     thread k adds output k's partials in workgroup order and rounds to float32 once.
//   k_occupancy_rows one byte per attention row from the decoder's prediction: a lane ORs (df <= thr) down the (2e)^2 lines of one W position of a
//                    row's block, the wave's __ballot collects the 2e lanes of every row it holds.
//
// No atomics and no ticket: grids depend on the shapes only, every sum has one order.  Built with -ffp-contract=off: df is an add, a multiply and a
// divide as torch evaluates network_pred_to_df, the one fused operation is the explicit fmaf() of 1 - out^2.
#include "common.h"
#include "../../include/rfuse_step.h"

namespace {
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 16;                    // channels whose loads a thread holds at once (16 x 4 VGPRs)
constexpr int kMaxChannels = 64;
constexpr int kMaxBlocks = 512;               // two workgroups per CU of an MI355X; 2^17 threads: the 64^3 layer at B = 4 is two quads per thread
constexpr int kFinishTile = 6144;             // doubles of LDS (48 KB) the second launch stages the partials through: 361 workgroups' at 16 channels
constexpr size_t kMaxQuads = (1ull << 31) - 1;

inline unsigned pwt_blocks(size_t quads) { return rf_blocks(quads, kThreads, kMaxBlocks); }
}   // namespace

// FULL: c is a multiple of kChunk, every chunk has kChunk channels (no per-channel predicate around the loads).  SUMS: dw and db are wanted; without them
// (a frozen head) the kernel is dh alone: no float64 work, no reduction, no second launch.
template <bool FULL, bool SUMS>
__global__ __launch_bounds__(kThreads) void k_pwt_backward(const float* __restrict__ h, const float* __restrict__ out, const float* __restrict__ dout,
                                                           const float* __restrict__ w, int c, unsigned vox4, unsigned total, float* __restrict__ dh,
                                                           double* __restrict__ part) {
    __shared__ double red[kWaves][kChunk + 1];
    const f32x4* __restrict__ out4 = reinterpret_cast<const f32x4*>(out);
    const f32x4* __restrict__ dout4 = reinterpret_cast<const f32x4*>(dout);
    for (int c0 = 0; c0 < c; c0 += kChunk) {
        const int cc = FULL ? kChunk : (c - c0 < kChunk ? c - c0 : kChunk);      // workgroup-uniform
        float wv[kChunk];
#pragma unroll
        for (int k = 0; k < kChunk; ++k) wv[k] = k < cc ? w[c0 + k] : 0.f;
        double acc[kChunk + 1];                                                 // dw of the chunk's channels, then db
#pragma unroll
        for (int k = 0; k <= kChunk; ++k) acc[k] = 0.0;
        for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < total; i += gridDim.x * kThreads) {
            const unsigned nn = i / vox4, v4 = i - nn * vox4;
            const size_t at = ((size_t)nn * c + c0) * vox4 + v4;
            const f32x4* __restrict__ hp = reinterpret_cast<const f32x4*>(h) + at;
            f32x4* __restrict__ dhp = reinterpret_cast<f32x4*>(dh) + at;
            f32x4 hv[kChunk];
#pragma unroll
            for (int k = 0; k < kChunk; ++k)
                if (k < cc) hv[k] = hp[(size_t)k * vox4];
            const f32x4 o = out4[i], d = dout4[i];
            f32x4 g;
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = d[e] * fmaf(-o[e], o[e], 1.0f);
#pragma unroll
            for (int k = 0; k < kChunk; ++k)
                if (k < cc) {
                    f32x4 r;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        r[e] = g[e] * wv[k];
                        if (SUMS) acc[k] += (double)g[e] * (double)hv[k][e];
                    }
                    dhp[(size_t)k * vox4] = r;
                }
            if (SUMS && c0 == 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[kChunk] += (double)g[e];
            }
        }
        if (!SUMS) continue;
#pragma unroll
        for (int k = 0; k <= kChunk; ++k) acc[k] = wave_sum(acc[k]);
        rf_waves_put<kWaves, kChunk + 1>(red, acc);
        const int k = threadIdx.x;
        double* __restrict__ mine = part + (size_t)blockIdx.x * (c + 1);
        if (k < cc) mine[c0 + k] = rf_waves_sum<kWaves, kChunk + 1>(red, k);
        if (k == kChunk && c0 == 0) mine[c] = rf_waves_sum<kWaves, kChunk + 1>(red, kChunk);
        __syncthreads();                                                        // red is written again by the next chunk
    }
}

// dw[k] (k < c) and db[0] (k == c): the partials of output k in workgroup order, from workgroup 0's own value, rounded to float32 once.  A serial sum
// per output, so the latency that matters is the operands': the workgroup copies the partials into LDS a tile of workgroups at a time (contiguous,
// coalesced loads, all in flight together), then thread k walks its column of the tile.
__global__ __launch_bounds__(kThreads) void k_pwt_finish(const double* __restrict__ part, int blocks, int c, float* __restrict__ dw, float* __restrict__ db) {
    __shared__ double tile[kFinishTile];
    const int cols = c + 1, per_tile = kFinishTile / cols, k = threadIdx.x;
    double s = 0.0;
    for (int b0 = 0; b0 < blocks; b0 += per_tile) {
        const int nb = blocks - b0 < per_tile ? blocks - b0 : per_tile;
        for (int i = k; i < nb * cols; i += kThreads) tile[i] = part[(size_t)b0 * cols + i];
        __syncthreads();
        if (k < cols) {
            int j = 0;
            if (b0 == 0) s = tile[k], j = 1;                                    // no zero in front: a sum of -0.0 stays -0.0
            for (; j < nb; ++j) s += tile[j * cols + k];
        }
        __syncthreads();
    }
    if (k < c) dw[k] = (float)s;
    else if (k == c) db[0] = (float)s;
}

// A wave holds G = 64 / wl rows, wl = min(2e, 64) lanes each; lane (g, wo) takes the W positions wo, wo + wl, .. of row g's block and ORs the
// predicate down the block's (2e)^2 lines.  Consecutive rows are consecutive in pz, so where 2e divides 64 a wave's loads are 256 contiguous bytes.
__global__ __launch_bounds__(kThreads) void k_occupancy_rows(const float* __restrict__ pred, int edge, int e2, int r, unsigned rows_total, float trunc,
                                                             float thr, uint8_t* __restrict__ rows) {
    const int lane = threadIdx.x & 63;
    const int wl = e2 < 64 ? e2 : 64, per_wave = 64 / wl;
    const unsigned wave = blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int g = lane / wl, wo = lane - g * wl;
    const unsigned long long row = (unsigned long long)wave * per_wave + g;
    const bool valid = g < per_wave && row < rows_total;
    bool occ = false;
    if (valid) {
        unsigned t = (unsigned)row;
        const unsigned pz = t % r; t /= r;
        const unsigned py = t % r; t /= r;
        const unsigned px = t % r, b = t / r;
        const size_t line = edge, plane = (size_t)edge * edge;
        const float* __restrict__ base = pred + (size_t)b * plane * edge + (size_t)px * e2 * plane + (size_t)py * e2 * line + (size_t)pz * e2;
        for (int dd = 0; dd < e2; ++dd)
            for (int hh = 0; hh < e2; ++hh) {
                const float* __restrict__ p = base + dd * plane + hh * line;
                for (int x = wo; x < e2; x += wl) {
                    const float df = ((p[x] + 1.0f) * trunc) / 2.0f;
                    occ |= df <= thr;                                           // NaN: false
                }
            }
    }
    const unsigned long long mask = __ballot(valid && occ);
    if (valid && wo == 0) {
        const unsigned long long mine = wl == 64 ? mask : (mask >> (g * wl)) & ((1ull << wl) - 1ull);
        rows[row] = mine != 0ull ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int rf_pointwise_tanh_backward_grid_threads(void) { return kMaxBlocks * kThreads; }

extern "C" size_t rf_pointwise_tanh_backward_ws_bytes(int n, int c, size_t voxels) {
    if (n < 1 || c < 1 || c > kMaxChannels || voxels < 4 || (voxels & 3) != 0) return 0;
    if (voxels / 4 > kMaxQuads / (size_t)n) return 0;
    return (size_t)pwt_blocks((size_t)n * (voxels / 4)) * (c + 1) * sizeof(double);
}

extern "C" int rf_pointwise_tanh_backward(const float* h, const float* out, const float* dout, const float* w, int n, int c, size_t voxels, float* dh,
                                          float* dw, float* db, void* ws, size_t ws_bytes, void* stream) {
    const bool sums = dw != nullptr;
    RF_REQUIRE(h && out && dout && w && dh && (dw != nullptr) == (db != nullptr) && (ws || !sums) && n > 0 && c > 0 && voxels > 0, RF_E_INVALID,
               "rf_pointwise_tanh_backward: bad arguments");
    RF_REQUIRE(((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(dout) | reinterpret_cast<uintptr_t>(dh)) & 15u) == 0 &&
               (reinterpret_cast<uintptr_t>(ws) & 7u) == 0, RF_E_INVALID, "rf_pointwise_tanh_backward: h, out, dout and dh must be 16-byte aligned, ws 8-byte aligned");
    const size_t need = rf_pointwise_tanh_backward_ws_bytes(n, c, voxels);
    RF_REQUIRE(need != 0, RF_E_UNSUPPORTED, "rf_pointwise_tanh_backward: n = %d, c = %d, voxels = %zu is outside the supported range (voxels %% 4 == 0, 1 <= c <= %d, "
               "fewer than 2^31 quads)", n, c, voxels, kMaxChannels);
    RF_REQUIRE(!sums || ws_bytes >= need, RF_E_WORKSPACE, "rf_pointwise_tanh_backward: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const unsigned vox4 = (unsigned)(voxels / 4), total = (unsigned)((size_t)n * vox4), blocks = pwt_blocks(total);
    double* part = reinterpret_cast<double*>(ws);
    const hipStream_t st = (hipStream_t)stream;
    const bool full = c % kChunk == 0;
    if (!sums)
        return full ? rf_launch<k_pwt_backward<true, false>>("rf_pointwise_tanh_backward", dim3(blocks), dim3(kThreads), st, h, out, dout, w, c, vox4, total, dh, part)
                    : rf_launch<k_pwt_backward<false, false>>("rf_pointwise_tanh_backward", dim3(blocks), dim3(kThreads), st, h, out, dout, w, c, vox4, total, dh, part);
    if (int rc = full ? rf_launch<k_pwt_backward<true, true>>("rf_pointwise_tanh_backward", dim3(blocks), dim3(kThreads), st, h, out, dout, w, c, vox4, total, dh, part)
                      : rf_launch<k_pwt_backward<false, true>>("rf_pointwise_tanh_backward", dim3(blocks), dim3(kThreads), st, h, out, dout, w, c, vox4, total, dh, part))
        return rc;
    return rf_launch<k_pwt_finish>("rf_pointwise_tanh_backward", dim3(1), dim3(kThreads), st, (const double*)part, (int)blocks, c, dw, db);
}

extern "C" int rf_attn_occupancy_rows(const float* pred, int n, int edge, int e, float trunc, float thr, uint8_t* rows, void* stream) {
    RF_REQUIRE(pred && rows && n > 0 && edge > 0 && e > 0, RF_E_INVALID, "rf_attn_occupancy_rows: bad arguments");
    RF_REQUIRE(e <= (1 << 20) && edge % (2 * e) == 0, RF_E_UNSUPPORTED, "rf_attn_occupancy_rows: edge = %d is no multiple of 2 e = %d", edge, 2 * e);
    const int e2 = 2 * e, r = edge / e2;
    const unsigned long long total = r <= 1290 ? (unsigned long long)n * r * r * r : ~0ull;      // 1290^3 < 2^31: no overflow below
    RF_REQUIRE(total < (1ull << 31), RF_E_UNSUPPORTED, "rf_attn_occupancy_rows: n = %d volumes of (%d)^3 rows each (fewer than 2^31 rows)", n, r);
    const unsigned per_wave = 64 / (e2 < 64 ? e2 : 64);
    const unsigned waves = (unsigned)((total + per_wave - 1) / per_wave);
    return rf_launch<k_occupancy_rows>("rf_attn_occupancy_rows", dim3((waves + kWaves - 1) / kWaves), dim3(kThreads), (hipStream_t)stream, pred, edge, e2, r,
                                       (unsigned)total, trunc, thr, rows);
}
