// Backward of the patch encoders' valid strided conv + bias + LeakyReLU (model/retrieval.py, reference model/retrieval.py:4-361; trained by the
// reference's trainer/train_retrieval.py):
//   dz        = y > 0 ? dy : slope * dy    (y = the saved output; torch's rule)           rf_conv3d_valid_leaky_backward (+ db = sum dz, float64)
//   dx[p]     = sum_{co, t : p = o * stride + t} dz[co][o] * W[co][ci][t]                rf_conv3d_valid_dgrad   -- fp32 MFMA, per parity phase
//   dW[t]     = sum_{n, o} dz[n][co][o] * x[n][ci][o * stride + t]                       rf_conv3d_valid_wgrad   -- fp32 MFMA, split K, float64 sum
// Every sum runs in a fixed order (no atomics): two calls give the same bits.
#include "common.h"

// ------------------------------------------------------------------------------------------- LeakyReLU backward + db
// Workgroup (g, co): the flat range [g * chunk, (g + 1) * chunk) of channel co's n * vol elements; its fp32 sum of dz (rf_tree_sum) goes
// to parts[g][co]; rf_slice_sum adds the G partials of a channel in float64.
static int lrb_groups(int n, size_t vol) {
    const size_t per = (size_t)n * vol;
    const size_t g = (per + 4095) / 4096;
    return (int)(g < 128 ? g : 128);
}

__global__ __launch_bounds__(256) void k_leaky_bwd(const float* __restrict__ dy, const float* __restrict__ y, int n, int cout, size_t vol, float slope,
                                                   float* __restrict__ dz, float* __restrict__ parts) {
    __shared__ float red[256][1];
    const int g = blockIdx.x, G = gridDim.x, co = blockIdx.y, tid = threadIdx.x;
    const size_t per = (size_t)n * vol, chunk = (per + G - 1) / G;
    const size_t j0 = (size_t)g * chunk, j1 = j0 + chunk < per ? j0 + chunk : per;
    float s = 0.f;
    for (size_t j = j0 + tid; j < j1; j += 256) {
        const size_t nn = j / vol, v = j - nn * vol;
        const size_t i = (nn * cout + co) * vol + v;
        const float d = dy[i];
        const float r = y[i] > 0.f ? d : d * slope;
        dz[i] = r;
        s += r;
    }
    rf_tree_sum(red, {s});
    if (tid == 0) parts[(size_t)g * cout + co] = red[0][0];
}

extern "C" size_t rf_conv3d_valid_leaky_backward_ws_bytes(int n, int cout, int so) {
    return (size_t)lrb_groups(n, (size_t)so * so * so) * cout * sizeof(float);
}

extern "C" int rf_conv3d_valid_leaky_backward(const float* dy, const float* y, int n, int cout, int so, float slope, float* dz, float* db, void* ws,
                                              size_t ws_bytes, void* stream) {
    RF_REQUIRE(dy && y && dz && db && ws && n > 0 && cout > 0 && so > 0 && so <= 128, RF_E_INVALID, "rf_conv3d_valid_leaky_backward: bad arguments");
    RF_REQUIRE(ws_bytes >= rf_conv3d_valid_leaky_backward_ws_bytes(n, cout, so), RF_E_WORKSPACE, "rf_conv3d_valid_leaky_backward: workspace too small");
    const size_t vol = (size_t)so * so * so;
    const int G = lrb_groups(n, vol);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = rf_launch<k_leaky_bwd>("rf_conv3d_valid_leaky_backward", dim3(G, cout), dim3(256), s, dy, y, n, cout, vol, slope, dz, (float*)ws)) return rc;
    return rf_slice_sum((const float*)ws, G, (size_t)cout, db, s, "rf_conv3d_valid_leaky_backward(db)");
}

// --------------------------------------------------------------------------------------------------- data gradient
// Parity phases: along an axis an input plane p = ph + stride * q (ph < stride) is read by the taps t = ph + stride * i (t < k) through the output
// o = q - i.  A phase is a dense implicit GEMM  D[ci][voxel] = sum_{tap of the phase, co} Wd[tap][co][ci] * dz[co][o(voxel, tap)]  -- no inserted
// zeros: stride 2, k = 3 has phases of 8/4/4/4/2/2/2/1 taps.  Planes no tap reaches (stride 2, (s - k) odd: the last one) belong to a phase whose
// outputs are all out of range and come out as exact 0.
// MFMA f32 16x16x4: A = Wd (16 channels x 4 couts), B = dz (4 couts x 16 voxels of the phase lattice), D = [16 ci][16 voxels]; a wave keeps four voxel
// tiles (64 voxels) and reuses the A operand across them.  Workgroup = 4 waves = 256 voxels of one phase of one sample, one 16-channel block.
// Wd: the host packs W OIDHW as [k^3][cout_pad4][cin_pad16] (zero padded) -- rfuse/ops.py:pack_convv_dgrad_weight.
struct DgradArgs {
    const float* dz;
    const float* wd;
    float* dx;
    int n, cin, cout, s, so, k, stride, cin_pad, cout_pad;
};

__global__ __launch_bounds__(256) void k_convv_dgrad(DgradArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int st = a.stride, nph = st * st * st;
    const int nn = blockIdx.z / nph, ph = blockIdx.z % nph;
    const int phz = ph / (st * st), phy = (ph / st) % st, phx = ph % st;
    // phase lattice: q along an axis with ph + st * q < s
    const int nqz = (a.s - phz + st - 1) / st, nqy = (a.s - phy + st - 1) / st, nqx = (a.s - phx + st - 1) / st;
    const int nvox = nqz * nqy * nqx;
    const int cib = blockIdx.y * 16;
    const size_t vol_o = (size_t)a.so * a.so * a.so, vol_i = (size_t)a.s * a.s * a.s;
    const float* dzn = a.dz + (size_t)nn * a.cout * vol_o;
    int qz[4], qy[4], qx[4];
    bool vin[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int v = (blockIdx.x * 4 + wave) * 64 + m * 16 + li;
        vin[m] = v < nvox;
        const int vv = vin[m] ? v : 0;
        qx[m] = vv % nqx;
        qy[m] = (vv / nqx) % nqy;
        qz[m] = vv / (nqx * nqy);
    }
    f32x4 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int iz = 0; phz + st * iz < a.k; ++iz)
        for (int iy = 0; phy + st * iy < a.k; ++iy)
            for (int ix = 0; phx + st * ix < a.k; ++ix) {
                const int tap = ((phz + st * iz) * a.k + (phy + st * iy)) * a.k + (phx + st * ix);
                const float* wt = a.wd + (size_t)tap * a.cout_pad * a.cin_pad + cib + li;
                long off[4];
                bool ok[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int oz = qz[m] - iz, oy = qy[m] - iy, ox = qx[m] - ix;
                    ok[m] = vin[m] && (unsigned)oz < (unsigned)a.so && (unsigned)oy < (unsigned)a.so && (unsigned)ox < (unsigned)a.so;
                    off[m] = ok[m] ? ((long)oz * a.so + oy) * a.so + ox : 0;
                }
                for (int c0 = 0; c0 < a.cout; c0 += 4) {
                    const int co = c0 + kq;
                    const float av = wt[(size_t)co * a.cin_pad];             // co < cout_pad: zero rows past cout
                    const bool cok = co < a.cout;
                    const float* dzc = dzn + (size_t)(cok ? co : 0) * vol_o;
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const float bv = (cok && ok[m]) ? dzc[off[m]] : 0.f;
                        acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[m], 0, 0, 0);
                    }
                }
            }
    // D[row = ci (4 kq + r)][col = voxel li]
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (!vin[m]) continue;
        const size_t p = ((size_t)(phz + st * qz[m]) * a.s + (phy + st * qy[m])) * a.s + (phx + st * qx[m]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ci = cib + kq * 4 + r;
            if (ci < a.cin) a.dx[((size_t)nn * a.cin + ci) * vol_i + p] = acc[m][r];
        }
    }
}

extern "C" size_t rf_convv_dgrad_packed_floats(int cout, int cin, int k) {
    return (size_t)k * k * k * rf_round_up(cout, 4) * rf_round_up(cin, 16);
}

extern "C" int rf_conv3d_valid_dgrad(const float* dz, int n, int cout, int so, const float* wd_packed, int cin, int k, int stride, int s, float* dx,
                                     void* stream) {
    RF_REQUIRE(dz && wd_packed && dx && n > 0 && cout > 0 && cin > 0 && so > 0, RF_E_INVALID, "rf_conv3d_valid_dgrad: bad arguments");
    RF_REQUIRE(k >= 1 && k <= 5 && (stride == 1 || stride == 2) && s >= k && s <= 128 && (s - k) / stride + 1 == so, RF_E_UNSUPPORTED,
               "rf_conv3d_valid_dgrad: k %d stride %d input %d output %d (k <= 5, stride 1 or 2, so = (s - k) / stride + 1)", k, stride, s, so);
    DgradArgs a;
    a.dz = dz; a.wd = wd_packed; a.dx = dx;
    a.n = n; a.cin = cin; a.cout = cout; a.s = s; a.so = so; a.k = k; a.stride = stride;
    a.cin_pad = rf_round_up(cin, 16); a.cout_pad = rf_round_up(cout, 4);
    const int nq = (s + stride - 1) / stride;                      // the largest phase lattice edge
    const int blocks = (nq * nq * nq + 255) / 256;
    return rf_launch<k_convv_dgrad>("rf_conv3d_valid_dgrad", dim3(blocks, a.cin_pad / 16, n * stride * stride * stride), dim3(256), (hipStream_t)stream, a);
}

// ------------------------------------------------------------------------------------------------- weight gradient
// GEMM  dW[co][col] = sum_k dz[co][k] * X[k][col],  col = ci * k^3 + tap (the OIDHW order), k = (n, oz, oy, ox).  K is cut into fixed slices of
// WG_ROWS output rows (n, oz, oy); a workgroup walks the rows of its slice, four ox per MFMA step (lane group kq takes ox = x0 + kq), and writes its
// fp32 partial tile to parts[slice][co][col]; rf_slice_sum (common.h) adds the slices in float64 in slice order.  MFMA f32 16x16x4: A = dz (16 couts x 4 k),
// B = x gathered at o * stride + tap (4 k x 16 columns); a wave keeps four column tiles (64 columns) and reuses the dz operand across them.
// Workgroup = 4 waves = 16 couts x 256 columns.
constexpr int WG_ROWS = 256;

struct WgradVArgs {
    const float* x;
    const float* dz;
    float* parts;             // [slices][cout][cin * k^3]
    int n, cin, cout, s, so, k, stride, cols, slices;
};

__global__ __launch_bounds__(256) void k_convv_wgrad(WgradVArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int slice = blockIdx.x, cob = blockIdx.z * 16;
    const int k3 = a.k * a.k * a.k;
    const size_t vol_o = (size_t)a.so * a.so * a.so, vol_i = (size_t)a.s * a.s * a.s;
    // this lane's B columns: four tiles of 16
    long xoff[4];
    bool colok[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int col = blockIdx.y * 256 + wave * 64 + m * 16 + li;
        colok[m] = col < a.cols;
        const int c = colok[m] ? col : 0, ci = c / k3, t = c % k3;
        const int tz = t / (a.k * a.k), ty = (t / a.k) % a.k, tx = t % a.k;
        xoff[m] = (long)ci * vol_i + ((long)tz * a.s + ty) * a.s + tx;
    }
    const int co = cob + li;
    const bool cook = co < a.cout;
    const long rows = (long)a.n * a.so * a.so;
    const long r0 = (long)slice * WG_ROWS, r1 = r0 + WG_ROWS < rows ? r0 + WG_ROWS : rows;
    f32x4 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (long r = r0; r < r1; ++r) {
        const int oy = (int)(r % a.so), oz = (int)((r / a.so) % a.so), nn = (int)(r / ((long)a.so * a.so));
        const float* dzr = a.dz + ((size_t)nn * a.cout + (cook ? co : 0)) * vol_o + ((size_t)oz * a.so + oy) * a.so;
        const float* xr = a.x + (size_t)nn * a.cin * vol_i + ((size_t)oz * a.stride * a.s + (size_t)oy * a.stride) * a.s;
        for (int x0 = 0; x0 < a.so; x0 += 4) {
            const int ox = x0 + kq;
            const bool xok = ox < a.so;
            const float av = (cook && xok) ? dzr[ox] : 0.f;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float bv = (colok[m] && xok) ? xr[xoff[m] + (long)ox * a.stride] : 0.f;
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[m], 0, 0, 0);
            }
        }
    }
    // D[row = co (4 kq + r)][col = li]
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (!colok[m]) continue;
        const int col = blockIdx.y * 256 + wave * 64 + m * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = cob + kq * 4 + r;
            if (c < a.cout) a.parts[((size_t)slice * a.cout + c) * a.cols + col] = acc[m][r];
        }
    }
}

static int wgradv_slices(int n, int so) {
    const long rows = (long)n * so * so;
    return (int)((rows + WG_ROWS - 1) / WG_ROWS);
}

extern "C" size_t rf_conv3d_valid_wgrad_ws_bytes(int n, int cin, int cout, int so, int k) {
    return (size_t)wgradv_slices(n, so) * cout * cin * k * k * k * sizeof(float);
}

extern "C" int rf_conv3d_valid_wgrad(const float* x, int n, int cin, int s, const float* dz, int cout, int k, int stride, float* dw, void* ws,
                                     size_t ws_bytes, void* stream) {
    RF_REQUIRE(x && dz && dw && ws && n > 0 && cin > 0 && cout > 0, RF_E_INVALID, "rf_conv3d_valid_wgrad: bad arguments");
    RF_REQUIRE(k >= 1 && k <= 5 && (stride == 1 || stride == 2) && s >= k && s <= 128, RF_E_UNSUPPORTED,
               "rf_conv3d_valid_wgrad: k %d stride %d input %d (k <= 5, stride 1 or 2)", k, stride, s);
    const int so = (s - k) / stride + 1;
    RF_REQUIRE(ws_bytes >= rf_conv3d_valid_wgrad_ws_bytes(n, cin, cout, so, k), RF_E_WORKSPACE, "rf_conv3d_valid_wgrad: workspace too small");
    WgradVArgs a;
    a.x = x; a.dz = dz; a.parts = (float*)ws;
    a.n = n; a.cin = cin; a.cout = cout; a.s = s; a.so = so; a.k = k; a.stride = stride;
    a.cols = cin * k * k * k; a.slices = wgradv_slices(n, so);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = rf_launch<k_convv_wgrad>("rf_conv3d_valid_wgrad", dim3(a.slices, (a.cols + 255) / 256, (cout + 15) / 16), dim3(256), st, a)) return rc;
    return rf_slice_sum((const float*)ws, a.slices, (size_t)cout * a.cols, dw, st, "rf_conv3d_valid_wgrad(sum)");
}
