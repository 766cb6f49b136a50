// Evaluation metrics of the reference (util/metrics.py:6-89: IoU, Chamfer3D, Precision, Recall; trainer/train_refinement.py:16,122-146,223-227 and
// util/retrieval.py:167-175) on occupancy grids: per volume the exact counts n_pred, n_target, n_inter and the two directed Chamfer sums
//   s_tp = sum_{t in T} min_{p in P} |t - p|^2,   s_pt = sum_{p in P} min_{t in T} |p - t|^2
// in squared voxel-index units, as int64.  The points are integer voxel coordinates, so the nearest-neighbour term is a squared Euclidean distance
// transform (EDT) of one grid sampled at the other grid's voxels; the EDT is separable (min over w, then over h, then over d of g + delta^2) and
// computed here with integer arithmetic only: exact, and the same bits in any order (integer sums, integer atomics).
//
//   k_occ_pack        one workgroup per (volume, d): every 64-wide w tile of a line -> one 64-bit word per grid (__ballot); popcounts -> the counts
//   k_minplus<true>   g2(d, h, w) = min_h' g1(d, h', w) + (h - h')^2 with g1 = (w - nearest set bit of the line (d, h'))^2 read from the words
//                     while staging (clz below, ctz above, on into the neighbour words of wide lines); both directions (EDT of P, EDT of T) in one
//                     launch, g2 to the workspace
//   k_minplus<false>  min_d' g2(d', h, w) + (d - d')^2 at the voxels of the OTHER grid only, summed into the volume's int64 slot
// A min-plus workgroup owns 64 consecutive positions of the inner extent and 64 outputs along the transform axis (16 per thread, in registers),
// walks the candidates in chunks of 64 staged in LDS as u = g + a'^2 and keeps min_a' (u - 2 a a') -- one v_mad_i32_i24 and one v_min_i32 per
// (output, candidate) -- adding a^2 once at the end.  Brute force over the candidates: exact and branch-free.  Edges 1..2048 on every axis.
#include "common.h"

namespace {
constexpr int kInf = 1 << 30;          // no voxel on this line / plane; kInf + 2047^2 stays far below 2^31 and is clamped back after each pass
constexpr int kMaxEdge = 2048;
constexpr int kTile = 64;              // positions of the inner extent per workgroup, candidates per LDS chunk, outputs per workgroup
constexpr int kRows = 4;               // waves per workgroup; thread (x, r) owns the outputs a0 + r + 4 j, j < 16
constexpr int kPer = kTile / kRows;
constexpr int kBatch = 4;              // k_occ_pack: words per wave and step

__device__ __forceinline__ bool occupied(const void* src, int kind, float thr, size_t i) {
    if (kind == RF_OCC_GRID) return reinterpret_cast<const uint8_t*>(src)[i] != 0;
    if (kind == RF_OCC_DF_F32) return reinterpret_cast<const float*>(src)[i] <= thr;          // NaN: unoccupied, -inf: occupied
    return (float)reinterpret_cast<const _Float16*>(src)[i] <= thr;                            // thr arrives rounded to f16 (exact in fp32)
}

// (w - nearest set bit of the line)^2, or kInf for an empty line.  Bits at w >= W are zero (k_occ_pack).
__device__ __forceinline__ int nearest_sq(const unsigned long long* __restrict__ line, int wn, int w) {
    const int k = w >> 6, i = w & 63;
    int best = kInf;
    unsigned long long m = line[k] & (~0ull >> (63 - i));            // bits 0..i
    int kk = k;
    while (!m && kk > 0) m = line[--kk];
    if (m) {
        const int d = w - (64 * kk + 63 - __builtin_clzll(m));
        best = d * d;
    }
    m = line[k] & (~0ull << i);                                        // bits i..63
    kk = k;
    // the next word's first bit is 64 (kk + 1) - w away: stop once that cannot beat the voxel below
    while (!m && kk + 1 < wn && (long long)(64 * (kk + 1) - w) * (64 * (kk + 1) - w) < best) m = line[++kk];
    if (m) {
        const int d = 64 * kk + __builtin_ctzll(m) - w;
        best = min(best, d * d);
    }
    return best;
}
}   // namespace

__global__ __launch_bounds__(256) void k_occ_pack(const void* __restrict__ pred, int pred_kind, float pred_thr, const void* __restrict__ target,
                                                  int target_kind, float target_thr, int D, int H, int W, unsigned long long* __restrict__ bits_p,
                                                  unsigned long long* __restrict__ bits_t, long long* __restrict__ out) {
    __shared__ unsigned long long part[kRows][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wn = (W + 63) >> 6;
    const size_t plane = blockIdx.x;                                   // b * D + d
    unsigned long long np = 0, nt = 0, ni = 0;
    const int words = H * wn;                                          // the plane's words; a wave takes kBatch of them per step (loads in flight)
    for (int base = wave; base < words; base += kBatch * kRows) {
        bool op[kBatch], ot[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int word = base + u * kRows, w = 64 * (word % wn) + lane;
            const size_t i = (plane * H + word / wn) * W + w;
            op[u] = word < words && w < W && occupied(pred, pred_kind, pred_thr, i);
            ot[u] = word < words && w < W && occupied(target, target_kind, target_thr, i);
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int word = base + u * kRows;
            const unsigned long long bp = __ballot(op[u]), bt = __ballot(ot[u]);
            if (lane == 0 && word < words) {
                bits_p[plane * words + word] = bp;
                bits_t[plane * words + word] = bt;
            }
            np += __popcll(bp);
            nt += __popcll(bt);
            ni += __popcll(bp & bt);
        }
    }
    rf_waves_put(part, {np, nt, ni});                                  // ballot counts: wave-uniform already
    if (threadIdx.x < 3) {
        const unsigned long long s = rf_waves_sum(part, threadIdx.x);
        if (s) atomicAdd(reinterpret_cast<unsigned long long*>(out + plane / D * 5 + threadIdx.x), s);
    }
}

// One min-plus pass along the axis A of a [Z][A][X] int32 grid.
//   FIRST:  Z = 2 B D (direction, volume, d), A = H, X = W; the grid is g1, made from the line words while staging; g2 is written.
//   !FIRST: Z = 2 B (direction, volume), A = D, X = H W; the grid is g2; the result is summed at the voxels of the query grid into
//           out[b][3 + direction].  Direction 0: EDT of P queried at T (s_tp); direction 1: EDT of T queried at P (s_pt).
template <bool FIRST>
__global__ __launch_bounds__(256) void k_minplus(int B, int D, int H, int W, const unsigned long long* __restrict__ bits_p,
                                                 const unsigned long long* __restrict__ bits_t, int* __restrict__ g2, long long* __restrict__ out) {
    __shared__ int u[kTile][kTile];
    __shared__ long long part[kRows][1];
    const int A = FIRST ? H : D;
    const long long X = FIRST ? (long long)W : (long long)H * W;
    const long long tiles_a = (A + kTile - 1) / kTile;
    const long long tiles_x = (X + kTile - 1) / kTile;
    const long long blk = blockIdx.x;
    const long long z = blk / (tiles_a * tiles_x);
    const int ta = (int)(blk / tiles_x % tiles_a);
    const long long x0 = blk % tiles_x * kTile;
    const int tx = threadIdx.x & 63, r = threadIdx.x >> 6;
    const long long x = x0 + tx;
    const bool xin = x < X;
    const int a0 = ta * kTile + r;
    const int wn = (W + 63) >> 6;
    const int dir = FIRST ? (int)(z / ((long long)B * D)) : (int)(z / B);
    const unsigned long long* src_bits = dir == 0 ? bits_p : bits_t;

    unsigned qmask = 0;                                               // !FIRST: bit j <=> output a0 + 4 j is a voxel of the query grid
    size_t b = 0;
    if (!FIRST) {
        b = (size_t)(z % B);
        const int h = xin ? (int)(x / W) : 0, w = xin ? (int)(x % W) : 0;
        const unsigned long long* q = (dir == 0 ? bits_t : bits_p) + (b * D * H + h) * wn + (w >> 6);
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int a = a0 + kRows * j;
            if (xin && a < A && ((q[(size_t)a * H * wn] >> (w & 63)) & 1ull)) qmask |= 1u << j;
        }
        if (!__syncthreads_or(qmask != 0)) return;                     // no query voxel in the tile: nothing to add (the same for every thread)
    }

    int best[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) best[j] = 0x7fffffff;
    for (int c0 = 0; c0 < A; c0 += kTile) {
        const int nc = min(kTile, A - c0);
        __syncthreads();
        for (int i = 0; i < kPer; ++i) {                               // u[a'][x] = g(c0 + a') + (c0 + a')^2
            const int ar = r + kRows * i, ac = c0 + ar;
            int g = kInf;
            if (xin && ar < nc) {
                if (FIRST)
                    g = nearest_sq(src_bits + ((size_t)(z % ((long long)B * D)) * H + ac) * wn, wn, (int)x);
                else
                    g = g2[((size_t)z * A + ac) * X + x];
            }
            u[ar][tx] = g + ac * ac;
        }
        __syncthreads();
        for (int ar = 0; ar < nc; ++ar) {
            const int v = u[ar][tx], ac = c0 + ar;
#pragma unroll
            for (int j = 0; j < kPer; ++j) best[j] = min(best[j], __mul24(-2 * (a0 + kRows * j), ac) + v);
        }
    }

    if (FIRST) {
        if (!xin) return;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int a = a0 + kRows * j;
            if (a < A) g2[((size_t)z * A + a) * X + x] = min(best[j] + a * a, kInf);
        }
        return;
    }
    long long s = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int a = a0 + kRows * j;
        const int v = min(best[j] + a * a, kInf);
        if (((qmask >> j) & 1u) && v < kInf) s += v;                   // an empty source grid leaves every value at kInf: its sum stays 0
    }
    rf_waves_put(part, {wave_sum(s)});
    if (threadIdx.x == 0) {
        const long long t = rf_waves_sum(part);
        if (t) atomicAdd(reinterpret_cast<unsigned long long*>(out + b * 5 + 3 + dir), (unsigned long long)t);
    }
}

namespace {
size_t words_per_grid(int b, int d, int h, int w) { return (size_t)b * d * h * ((w + 63) / 64); }
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
bool edges_ok(int d, int h, int w) { return d >= 1 && h >= 1 && w >= 1 && d <= kMaxEdge && h <= kMaxEdge && w <= kMaxEdge; }
}   // namespace

extern "C" size_t rf_occupancy_stats_ws_bytes(int b, int d, int h, int w, int chamfer) {
    if (b < 1 || !edges_ok(d, h, w)) return 0;
    const size_t bits = align256(2 * words_per_grid(b, d, h, w) * sizeof(unsigned long long));
    return chamfer ? bits + align256((size_t)2 * b * d * h * w * sizeof(int)) : bits;
}

extern "C" int rf_occupancy_stats(const void* pred, int pred_kind, float pred_thr, const void* target, int target_kind, float target_thr, int b, int d,
                                  int h, int w, int chamfer, int64_t* out, void* ws, size_t ws_bytes, void* stream) {
    RF_REQUIRE(pred && target && out && ws && b >= 1, RF_E_INVALID, "rf_occupancy_stats: bad arguments");
    RF_REQUIRE(pred_kind >= RF_OCC_GRID && pred_kind <= RF_OCC_DF_F16 && target_kind >= RF_OCC_GRID && target_kind <= RF_OCC_DF_F16, RF_E_INVALID,
               "rf_occupancy_stats: unknown input kinds %d / %d", pred_kind, target_kind);
    RF_REQUIRE(edges_ok(d, h, w), RF_E_UNSUPPORTED, "rf_occupancy_stats: edges %d x %d x %d (each must be 1..%d)", d, h, w, kMaxEdge);
    const long long tiles_x_h = (w + kTile - 1) / kTile, tiles_a_h = (h + kTile - 1) / kTile;
    const long long tiles_x_d = ((long long)h * w + kTile - 1) / kTile, tiles_a_d = (d + kTile - 1) / kTile;
    const long long grid_pack = (long long)b * d, grid_h = 2ll * b * d * tiles_a_h * tiles_x_h, grid_d = 2ll * b * tiles_a_d * tiles_x_d;
    // HIP takes fewer than 2^32 work-items per launch: 2^24 workgroups of 256
    RF_REQUIRE(grid_pack < (1ll << 24) && grid_h < (1ll << 24) && grid_d < (1ll << 24), RF_E_UNSUPPORTED,
               "rf_occupancy_stats: %d volumes of %d x %d x %d need more than 2^24 workgroups in one launch", b, d, h, w);
    const size_t need = rf_occupancy_stats_ws_bytes(b, d, h, w, chamfer);
    RF_REQUIRE(ws_bytes >= need, RF_E_WORKSPACE, "rf_occupancy_stats: workspace of %zu bytes, needs %zu", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* bits_p = reinterpret_cast<unsigned long long*>(ws);
    unsigned long long* bits_t = bits_p + words_per_grid(b, d, h, w);
    int* g2 = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + align256(2 * words_per_grid(b, d, h, w) * sizeof(unsigned long long)));
    long long* o = reinterpret_cast<long long*>(out);
    if (hipMemsetAsync(o, 0, (size_t)b * 5 * sizeof(long long), s) != hipSuccess) {
        rf_set_error("rf_occupancy_stats: cannot clear the output");
        return RF_E_LAUNCH;
    }
    if (int rc = rf_launch<k_occ_pack>("rf_occupancy_stats (pack)", dim3((unsigned)grid_pack), dim3(256), s, pred, pred_kind, pred_thr, target, target_kind, target_thr,
                                       d, h, w, bits_p, bits_t, o))
        return rc;
    if (!chamfer) return RF_OK;
    if (int rc = rf_launch<k_minplus<true>>("rf_occupancy_stats (min-plus along h)", dim3((unsigned)grid_h), dim3(256), s, b, d, h, w, bits_p, bits_t, g2, o)) return rc;
    return rf_launch<k_minplus<false>>("rf_occupancy_stats (min-plus along d)", dim3((unsigned)grid_d), dim3(256), s, b, d, h, w, bits_p, bits_t, g2, o);
}
