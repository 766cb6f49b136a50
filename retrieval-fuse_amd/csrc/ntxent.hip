// NT-Xent (model/loss.py NTXentLoss.forward) and the sliced attention contrastive loss of the reference's refinement trainer
// (trainer/train_refinement.py:208-221 compute_sliced_attn_nt_xent_loss) on the device; the entry points are declared in include/rfuse_contrastive.h.
//
//   k_ntx_plan    one workgroup: occupied rows per slice (ballot / popcount), the greedy rule by one thread, then the compacted row list in row order,
//                 the tile table (a tile = 16 consecutive rows of one group's stacked [zjs; zis]) and a selected flag per row
//   k_ntx_rows    one wave per selected stacked row: gathers it, |z| in float64, w = z / max(|z|, 1e-8) (or z) as float64 into the workspace
//   k_ntx_lse     one workgroup per tile: the tile's rows against the group's columns, 64 at a time through LDS; every lane keeps a running (max, sum)
//                 per row over its own columns, combined over the wave at the end: lse_i, and (lse_i - l_i,pos) / 2n per row
//   k_ntx_finish  one workgroup adds the per-row terms in a fixed order
//   k_ntx_bwd     the same tiles: s_ij again, c_ij = G_ij + G_ji into LDS, dw_i += c_ij w_j with the lanes over the features; then the normalisation's
//                 backward and the scatter; the workgroups behind the tiles write the zeros of the rows that were not selected
//
// Float64 VALU throughout (on gfx950 its FMA rate is the float32 one, and at tau = 0.05 an error of s_ij is multiplied by 20): the similarity matrix never
// exists, and what is left of the cost is launch and memory latency.  No atomics; every sum has one order.
#include "common.h"
#include "../../include/rfuse_contrastive.h"

namespace {
constexpr int kTI = 16;              // rows of a tile: 4 per wave
constexpr int kTJ = 64;              // columns per step: one per lane
constexpr int kKC = 64;              // features per LDS chunk
constexpr int kLd = kKC + 1;         // odd leading dimension: lanes over rows AND lanes over features read without bank conflicts
constexpr int kMaxChunks = 4;        // dim <= 256
constexpr int kThreads = 256;
constexpr int kPlanThreads = 1024;
constexpr int kMaxSlices = 4096, kMaxGroup = 4096, kMaxDim = 256;
constexpr double kEps = 1e-8;

struct Layout {                      // byte offsets into the workspace, each a multiple of 256
    size_t hdr, rows, tiles, sel, w, nrm, lse, term, total;
    int tiles_max;
};
// hdr: int [4] = groups, selected rows, tiles, -;  rows: int [max_rows] = the row of a compact slot;  tiles: int4 [tiles_max] = group start (compact), n, first
// stacked row, -;  sel: uint8 [n_rows];  w: double [2][max_rows][dim] ([0] = zjs, [1] = zis, by compact slot);  nrm, lse, term: double [2][max_rows]
bool layout_of(int n_rows, int num_slices, int max_rows, int dim, Layout* L) {
    if (n_rows < 1 || num_slices < 1 || max_rows < 1 || dim < 1) return false;
    if (dim > kMaxDim || num_slices > kMaxSlices) return false;
    const int split = n_rows / num_slices, group = split < max_rows ? split : max_rows;
    if (group < 1 || group > kMaxGroup) return false;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t mr = (size_t)max_rows;
    L->tiles_max = (int)((2 * mr + kTI - 1) / kTI) + (num_slices < max_rows ? num_slices : max_rows);
    size_t o = 0;
    L->hdr = o, o += 256;
    L->rows = o, o += up(mr * sizeof(int));
    L->tiles = o, o += up((size_t)L->tiles_max * 4 * sizeof(int));
    L->sel = o, o += up((size_t)n_rows);
    L->w = o, o += up(2 * mr * dim * sizeof(double));
    L->nrm = o, o += up(2 * mr * sizeof(double));
    L->lse = o, o += up(2 * mr * sizeof(double));
    L->term = o, o += up(2 * mr * sizeof(double));
    L->total = o;
    return true;
}

struct Ws {
    int* hdr;
    int* rows;
    int4* tiles;
    uint8_t* sel;
    double* w;
    double* nrm;
    double* lse;
    double* term;
};
Ws pointers(const Layout& L, void* ws) {
    char* b = reinterpret_cast<char*>(ws);
    return Ws{reinterpret_cast<int*>(b + L.hdr), reinterpret_cast<int*>(b + L.rows), reinterpret_cast<int4*>(b + L.tiles), reinterpret_cast<uint8_t*>(b + L.sel),
              reinterpret_cast<double*>(b + L.w), reinterpret_cast<double*>(b + L.nrm), reinterpret_cast<double*>(b + L.lse), reinterpret_cast<double*>(b + L.term)};
}

struct Temp {
    float tau, sig_scale, sig_shift;
};
// the temperature of logit (i, j) of a group of n pairs; iou [2n][2n] or null
__device__ __forceinline__ double tau_of(const float* iou, int i, int j, int n2, bool pos, const Temp& t) {
    if (pos || iou == nullptr) return (double)t.tau;
    const double x = (double)iou[(size_t)i * n2 + j] * (double)t.sig_scale + (double)t.sig_shift;
    return (double)t.tau + (1.0 - (double)t.tau) * (1.0 / (1.0 + exp(-x)));
}
// the workspace slot of stacked row x of the group that starts at compact slot o: [zjs; zis]
__device__ __forceinline__ int slot_of(int x, int o, int n, int max_rows) { return x < n ? o + x : max_rows + o + (x - n); }

// rows [first, first + count) of the group's stacked w, features [k0, k0 + kc), into s[row][feature]; zeros past the group's 2n rows
__device__ __forceinline__ void stage(double* s, const double* __restrict__ w, int first, int count, int o, int n, int max_rows, int dim, int k0, int kc) {
    for (int e = threadIdx.x; e < count * kc; e += kThreads) {
        const int r = e / kc, d = e - r * kc, x = first + r;
        s[r * kLd + d] = x < 2 * n ? w[(size_t)slot_of(x, o, n, max_rows) * dim + k0 + d] : 0.0;
    }
}

// s_ij of the tile's 4 rows of this wave (acc[r]: row i0 + 4 * wave + r) against column j0 + lane.  Leaves the LAST chunk of the columns in sB.
__device__ __forceinline__ void similarities(double* sA, double* sB, const double* __restrict__ w, int i0, int j0, int o, int n, int max_rows, int dim, int chunks,
                                             bool a_staged, double acc[4]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
    for (int ch = 0; ch < chunks; ++ch) {
        const int k0 = ch * kKC, kc = dim - k0 < kKC ? dim - k0 : kKC;
        __syncthreads();
        if (!a_staged) stage(sA, w, i0, kTI, o, n, max_rows, dim, k0, kc);
        stage(sB, w, j0, kTJ, o, n, max_rows, dim, k0, kc);
        __syncthreads();
        const double* a = sA + 4 * wv * kLd;
        const double* b = sB + lane * kLd;
#pragma unroll 8
        for (int d = 0; d < kc; ++d) {
            const double bv = b[d];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = fma(a[r * kLd + d], bv, acc[r]);
        }
    }
}
}   // namespace

__global__ __launch_bounds__(kPlanThreads) void k_ntx_plan(const uint8_t* __restrict__ occ, int n_rows, int num_slices, int max_rows, int tiles_max, int* __restrict__ hdr,
                                                           int* __restrict__ rows, int4* __restrict__ tiles, uint8_t* __restrict__ sel, long long* __restrict__ counts) {
    __shared__ int cnt[kMaxSlices], off[kMaxSlices];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, waves = kPlanThreads / 64;
    const int split = n_rows / num_slices;
    for (int s = wv; s < num_slices; s += waves) {
        int c = 0;
        if (occ == nullptr)
            c = split;
        else
            for (int k = 0; k < split; k += 64) {
                const bool on = k + lane < split && occ[(size_t)s * split + k + lane] != 0;
                c += __popcll(__ballot(on));
            }
        if (lane == 0) cnt[s] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int taken = 0, groups = 0, nt = 0;
        long long occupied = 0;
        for (int s = 0; s < num_slices; ++s) {
            const int c = cnt[s];
            occupied += c;
            if (c > 0 && taken + c <= max_rows) {
                off[s] = taken;
                for (int i0 = 0; i0 < 2 * c && nt < tiles_max; i0 += kTI) tiles[nt++] = make_int4(taken, c, i0, 0);
                taken += c;
                ++groups;
            } else {
                off[s] = -1;
            }
        }
        hdr[0] = groups, hdr[1] = taken, hdr[2] = nt, hdr[3] = 0;
        counts[0] = occupied, counts[1] = taken, counts[2] = groups;
    }
    __syncthreads();
    for (int s = wv; s < num_slices; s += waves) {
        const int o = off[s];
        int base = 0;
        for (int k = 0; k < split; k += 64) {
            const int row = s * split + k + lane;
            const bool in = k + lane < split;
            const bool on = in && (occ == nullptr || occ[row] != 0);
            const unsigned long long mask = __ballot(on);
            if (in) sel[row] = on && o >= 0 ? 1 : 0;
            if (on && o >= 0) rows[o + base + __popcll(mask & ((1ull << lane) - 1ull))] = row;
            base += __popcll(mask);
        }
    }
    for (int row = num_slices * split + (int)threadIdx.x; row < n_rows; row += kPlanThreads) sel[row] = 0;
}

__global__ __launch_bounds__(kThreads) void k_ntx_rows(const float* __restrict__ zis, const float* __restrict__ zjs, const int* __restrict__ hdr,
                                                       const int* __restrict__ rows, int max_rows, int dim, int cosine, double* __restrict__ w,
                                                       double* __restrict__ nrm) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (q >= 2 * max_rows) return;
    const int h = q >= max_rows, c = q - h * max_rows;
    if (c >= hdr[1]) return;
    const float* z = (h ? zis : zjs) + (size_t)rows[c] * dim;
    double ss = 0.0;
    for (int d = lane; d < dim; d += 64) ss = fma((double)z[d], (double)z[d], ss);
    ss = wave_sum(ss);
    const double len = sqrt(ss), den = cosine ? fmax(len, kEps) : 1.0;
    for (int d = lane; d < dim; d += 64) w[(size_t)q * dim + d] = (double)z[d] / den;
    if (lane == 0) nrm[q] = len;
}

__global__ __launch_bounds__(kThreads) void k_ntx_lse(const float* __restrict__ iou, const int* __restrict__ hdr, const int4* __restrict__ tiles,
                                                      const double* __restrict__ w, int max_rows, int dim, Temp tp, double* __restrict__ lse,
                                                      double* __restrict__ term) {
    __shared__ double sA[kTI * kLd], sB[kTJ * kLd];
    if ((int)blockIdx.x >= hdr[2]) return;
    const int4 t = tiles[blockIdx.x];
    const int o = t.x, n = t.y, i0 = t.z, n2 = 2 * n;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, chunks = (dim + kKC - 1) / kKC;
    double m[4], sum[4], lpos[4], acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = -INFINITY, sum[r] = 0.0, lpos[r] = 0.0;
    for (int j0 = 0; j0 < n2; j0 += kTJ) {
        similarities(sA, sB, w, i0, j0, o, n, max_rows, dim, chunks, chunks == 1 && j0 > 0, acc);
        const int j = j0 + lane;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * wv + r;
            if (i < n2 && j < n2 && j != i) {
                const bool pos = j == (i < n ? i + n : i - n);
                const double l = acc[r] / tau_of(iou, i, j, n2, pos, tp);
                if (pos) lpos[r] = l;
                // running (max, sum of exp(l - max)); a NaN logit fails `d > 0` and lands in the sum
                const double d = l - m[r], e = exp(-fabs(d));
                if (d > 0.0) {
                    sum[r] = fma(sum[r], e, 1.0);
                    m[r] = l;
                } else {
                    sum[r] += e;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * wv + r;
        const double top = wave_max(m[r]);                              // some lane holds the positive: finite unless the logits are not
        const double part = sum[r] == 0.0 ? 0.0 : sum[r] * exp(m[r] - top);      // a lane without a column: (max, sum) = (-inf, 0)
        const double all = wave_sum(part), lp = wave_sum(lpos[r]);
        if (lane == 0 && i < n2) {
            const int q = slot_of(i, o, n, max_rows);
            const double v = top + log(all);
            lse[q] = v;
            term[q] = (v - lp) / (double)n2;
        }
    }
}

// one workgroup: thread k adds the terms of compact slots k, k + 256, ... (zjs then zis of each), then a fixed tree over the 256 threads
__global__ __launch_bounds__(kThreads) void k_ntx_finish(const int* __restrict__ hdr, const double* __restrict__ term, int max_rows, float* __restrict__ loss) {
    __shared__ double red[kThreads][1];
    const int taken = hdr[1];
    double acc = 0.0;
    for (int c = threadIdx.x; c < taken; c += kThreads) acc += term[c] + term[max_rows + c];
    rf_tree_sum(red, {acc});
    if (threadIdx.x == 0) loss[0] = (float)red[0][0];
}

__global__ __launch_bounds__(kThreads) void k_ntx_bwd(const float* __restrict__ iou, const float* __restrict__ grad_loss, const int* __restrict__ hdr,
                                                      const int* __restrict__ rows, const int4* __restrict__ tiles, const uint8_t* __restrict__ sel,
                                                      const double* __restrict__ w, const double* __restrict__ nrm, const double* __restrict__ lse, int n_rows,
                                                      int max_rows, int dim, int cosine, Temp tp, int tiles_max, float* __restrict__ dzis,
                                                      float* __restrict__ dzjs) {
    __shared__ double sA[kTI * kLd], sB[kTJ * kLd], sC[kTI * kTJ];
    if ((int)blockIdx.x >= tiles_max) {      // the rows that were not selected: exact zeros
        const size_t total = (size_t)n_rows * dim, step = (size_t)(gridDim.x - tiles_max) * kThreads;
        for (size_t e = (size_t)(blockIdx.x - tiles_max) * kThreads + threadIdx.x; e < total; e += step)
            if (!sel[e / dim]) dzis[e] = 0.f, dzjs[e] = 0.f;
        return;
    }
    if ((int)blockIdx.x >= hdr[2]) return;
    const int4 t = tiles[blockIdx.x];
    const int o = t.x, n = t.y, i0 = t.z, n2 = 2 * n;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, chunks = (dim + kKC - 1) / kKC;
    double acc[4], dw[kMaxChunks][4], lse_i[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * wv + r;
        lse_i[r] = i < n2 ? lse[slot_of(i, o, n, max_rows)] : 0.0;
#pragma unroll
        for (int ch = 0; ch < kMaxChunks; ++ch) dw[ch][r] = 0.0;
    }
    for (int j0 = 0; j0 < n2; j0 += kTJ) {
        similarities(sA, sB, w, i0, j0, o, n, max_rows, dim, chunks, chunks == 1 && j0 > 0, acc);
        const int j = j0 + lane;
        const double lse_j = j < n2 ? lse[slot_of(j, o, n, max_rows)] : 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * wv + r;
            double c = 0.0;
            if (i < n2 && j < n2 && j != i) {
                const bool pos = j == (i < n ? i + n : i - n);
                const double t_ij = tau_of(iou, i, j, n2, pos, tp), t_ji = iou ? tau_of(iou, j, i, n2, pos, tp) : t_ij;
                const double one = pos ? 1.0 : 0.0;
                c = ((exp(acc[r] / t_ij - lse_i[r]) - one) / t_ij + (exp(acc[r] / t_ji - lse_j) - one) / t_ji) / (double)n2;
            }
            sC[(4 * wv + r) * kTJ + lane] = c;
        }
#pragma unroll
        for (int ch = 0; ch < kMaxChunks; ++ch) {
            if (ch < chunks) {
                const int k0 = ch * kKC, kc = dim - k0 < kKC ? dim - k0 : kKC;
                __syncthreads();
                if (chunks > 1) {      // one chunk: the columns are still staged
                    stage(sB, w, j0, kTJ, o, n, max_rows, dim, k0, kc);
                    __syncthreads();
                }
                if (lane < kc) {
                    const double* cr = sC + 4 * wv * kTJ;
#pragma unroll 8
                    for (int jj = 0; jj < kTJ; ++jj) {
                        const double bv = sB[jj * kLd + lane];
#pragma unroll
                        for (int r = 0; r < 4; ++r) dw[ch][r] = fma(cr[r * kTJ + jj], bv, dw[ch][r]);
                    }
                }
            }
        }
    }
    const double g = (double)grad_loss[0];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * wv + r;
        if (i >= n2) continue;                       // uniform over the wave
        const int q = slot_of(i, o, n, max_rows);
        double wi[kMaxChunks], dot = 0.0;
#pragma unroll
        for (int ch = 0; ch < kMaxChunks; ++ch) {
            const int d = ch * kKC + lane;
            wi[ch] = d < dim ? w[(size_t)q * dim + d] : 0.0;
            if (d < dim) dot = fma(wi[ch], dw[ch][r], dot);
        }
        dot = wave_sum(dot);
        const double len = nrm[q];
        float* dst = (i < n ? dzjs : dzis) + (size_t)rows[i < n ? o + i : o + i - n] * dim;
#pragma unroll
        for (int ch = 0; ch < kMaxChunks; ++ch) {
            const int d = ch * kKC + lane;
            if (d < dim) {
                double v = dw[ch][r];
                if (cosine) v = len >= kEps ? (v - wi[ch] * dot) / len : v / kEps;      // below the clamp w = z / 1e-8 is linear in z
                dst[d] = (float)(v * g);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ entry points
namespace {
const char* kRange = "%s: %d rows in %d slices, at most %d rows, %d features (1 <= features <= 256, slices <= 4096, 1 <= min(rows / slices, max_rows) <= 4096)";
}

extern "C" size_t rf_ntx_ws_bytes(int n_rows, int num_slices, int max_rows, int dim) {
    Layout L;
    return layout_of(n_rows, num_slices, max_rows, dim, &L) ? L.total : 0;
}

extern "C" int rf_ntx_plan(const uint8_t* occupancy, int n_rows, int num_slices, int max_rows, int dim, void* ws, size_t ws_bytes, int64_t* counts,
                           void* stream) {
    RF_REQUIRE(ws && counts && n_rows >= 1 && num_slices >= 1 && max_rows >= 1 && dim >= 1, RF_E_INVALID, "rf_ntx_plan: bad arguments");
    Layout L;
    RF_REQUIRE(layout_of(n_rows, num_slices, max_rows, dim, &L), RF_E_UNSUPPORTED, kRange, "rf_ntx_plan", n_rows, num_slices, max_rows, dim);
    RF_REQUIRE(ws_bytes >= L.total, RF_E_WORKSPACE, "rf_ntx_plan: workspace of %zu bytes, needs %zu", ws_bytes, L.total);
    const Ws p = pointers(L, ws);
    return rf_launch<k_ntx_plan>("rf_ntx_plan", dim3(1), dim3(kPlanThreads), (hipStream_t)stream, occupancy, n_rows, num_slices, max_rows, L.tiles_max, p.hdr, p.rows,
                                 p.tiles, p.sel, reinterpret_cast<long long*>(counts));
}

extern "C" int rf_ntx_forward(const float* zis, const float* zjs, const float* iou, int n_rows, int num_slices, int max_rows, int dim, int cosine, float tau,
                              float sig_scale, float sig_shift, void* ws, size_t ws_bytes, float* loss, void* stream) {
    RF_REQUIRE(zis && zjs && ws && loss && n_rows >= 1 && num_slices >= 1 && max_rows >= 1 && dim >= 1, RF_E_INVALID, "rf_ntx_forward: bad arguments");
    RF_REQUIRE(iou == nullptr || num_slices == 1, RF_E_INVALID, "rf_ntx_forward: an IoU matrix needs one slice, got %d", num_slices);
    Layout L;
    RF_REQUIRE(layout_of(n_rows, num_slices, max_rows, dim, &L), RF_E_UNSUPPORTED, kRange, "rf_ntx_forward", n_rows, num_slices, max_rows, dim);
    RF_REQUIRE(ws_bytes >= L.total, RF_E_WORKSPACE, "rf_ntx_forward: workspace of %zu bytes, needs %zu", ws_bytes, L.total);
    const Ws p = pointers(L, ws);
    const Temp tp{tau, sig_scale, sig_shift};
    hipStream_t s = (hipStream_t)stream;
    if (int rc = rf_launch<k_ntx_rows>("rf_ntx_forward (rows)", dim3((unsigned)((2 * (size_t)max_rows + 3) / 4)), dim3(kThreads), s, zis, zjs, p.hdr, p.rows, max_rows,
                                       dim, cosine, p.w, p.nrm))
        return rc;
    if (int rc = rf_launch<k_ntx_lse>("rf_ntx_forward", dim3((unsigned)L.tiles_max), dim3(kThreads), s, iou, p.hdr, p.tiles, p.w, max_rows, dim, tp, p.lse, p.term))
        return rc;
    return rf_launch<k_ntx_finish>("rf_ntx_forward (finish)", dim3(1), dim3(kThreads), s, p.hdr, p.term, max_rows, loss);
}

extern "C" int rf_ntx_backward(const float* iou, const float* grad_loss, int n_rows, int num_slices, int max_rows, int dim, int cosine, float tau, float sig_scale,
                               float sig_shift, const void* ws, size_t ws_bytes, float* dzis, float* dzjs, void* stream) {
    RF_REQUIRE(grad_loss && ws && dzis && dzjs && n_rows >= 1 && num_slices >= 1 && max_rows >= 1 && dim >= 1, RF_E_INVALID, "rf_ntx_backward: bad arguments");
    RF_REQUIRE(iou == nullptr || num_slices == 1, RF_E_INVALID, "rf_ntx_backward: an IoU matrix needs one slice, got %d", num_slices);
    Layout L;
    RF_REQUIRE(layout_of(n_rows, num_slices, max_rows, dim, &L), RF_E_UNSUPPORTED, kRange, "rf_ntx_backward", n_rows, num_slices, max_rows, dim);
    RF_REQUIRE(ws_bytes >= L.total, RF_E_WORKSPACE, "rf_ntx_backward: workspace of %zu bytes, needs %zu", ws_bytes, L.total);
    const Ws p = pointers(L, const_cast<void*>(ws));
    const Temp tp{tau, sig_scale, sig_shift};
    const unsigned zero_wgs = rf_blocks((size_t)n_rows * dim, 4 * kThreads, 1024);
    return rf_launch<k_ntx_bwd>("rf_ntx_backward", dim3((unsigned)L.tiles_max + zero_wgs), dim3(kThreads), (hipStream_t)stream, iou, grad_loss, p.hdr, p.rows, p.tiles,
                                p.sel, p.w, p.nrm, p.lse, n_rows, max_rows, dim, cosine, tp, L.tiles_max, dzis, dzjs);
}
