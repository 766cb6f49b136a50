// rf_conv3d_e2_level: one encoder level of a U-Net whose DoubleConv runs on whole 2^3 volumes, in ONE launch:
//     MaxPool3d(2) of [n][c][4^3] -> GroupNorm -> conv 3^3 (c -> cmid) -> ReLU -> GroupNorm -> conv 3^3 (cmid -> cout) -> ReLU          (reference model/unet.py:230-253)
// and, optionally, the GroupNorm triples of the decoder stage that reads this output upsampled beside a skip tensor whose statistics already exist.
// The six launches it replaces (rf_maxpool3d_2_stats, rf_gn_from_stats, rf_conv3d_e2_split_k3_gn_relu, rf_gn_from_stats, rf_conv3d_e2_split_k3_gn_relu,
// rf_gn_from_stats) spend most of their time on a one-ahead weight staging chain and on gathering / converting the same A rows once per column chunk
// (conv3d_e2_split.hip).  Arithmetic: bit for bit that route's -- every sum below keeps the order of the kernel it restates, and says which.
//
// A workgroup (8 waves) owns 32 samples for the whole level.
//   phase 0   the tile's 4^3 input is one contiguous run; lane = (plane, pooled voxel) as k_maxpool2_small<8>, statistics by its butterfly (distance 4, 2, 1);
//             group sums as k_gn_from_stats<1>; the pooled values (registers) are normalised, split and written ONCE as the first GEMM's A image in
//             fragment order: [k-step][m-block][h | l][lane] h8 -- A operands are then one ds_read_b128 each.
//   GEMM 1    32 x (8 c) x (8 cmid = 512 columns): wave w owns columns 64 w .. 64 w + 63 (2 m-blocks x 4 n-blocks, hi and lo: 64 accumulator registers).  No two
//             waves share a B fragment, so the weights need no LDS: each wave streams its own fragments of the rf_conv3_e2_split_pack_weight image
//             global -> registers, TWO k-steps ahead of the one being multiplied (a ring of three register blocks; a fourth spills).
//   between   ReLU, statistics (the e2 kernel's butterfly: distance 1, 2, 4), group sums, triples; the mid tensor goes accumulators -> normalised, split ->
//             the second A image, in place of the first (dead after a barrier).  It never leaves the CU.
//   GEMM 2    8 cout columns as passes of 512 over that image; rows leave as 64-byte pieces, statistics as rf_conv3d_e2_split_k3_gn_relu writes them.
//   table     group sums of the decoder's GroupNorm as k_gn_from_stats<1> with two sources (skip entries, then this output's entries as 8.0 * a), triples.
#include "common.h"
#include "split_operand.h"
#include "../../include/rfuse_level.h"

namespace {
constexpr int LV_M = 32;                                     // samples per workgroup
constexpr int LV_THREADS = 512;
constexpr int LV_NC = 256;                                   // columns per chunk of the packed weight image (conv3d_e2_split.hip: E2_NC)
constexpr int LV_STEP_H8 = (LV_NC / 16) * 2 * 64;            // h8 elements of one k-step of one chunk (E2_STEP_H8)
constexpr int LV_CMAX = 64;                                  // most channels of an A image: 16 k-steps x 4 KB = 64 KB
constexpr int LV_COMAX = 128;
constexpr int LV_A_BYTES = (LV_CMAX / 4) * 2 * 2 * 64 * 16;  // 65,536
constexpr int LV_S_BYTES = LV_M * LV_COMAX * 16;             // statistics of the widest tensor as double2: 65,536 (first half: c / cmid statistics, second half: their triples)
constexpr int LV_LDS_BYTES = LV_A_BYTES + LV_S_BYTES;        // 131,072
constexpr int LV_RING = 3;                                   // register blocks of the weight stream: the one being multiplied + two in flight
static_assert(LV_M * LV_CMAX * 16 * 2 <= LV_S_BYTES, "statistics and triples of a 64-channel tensor share the S region");
}

struct LvArgs {
    const float* x;            // [n][c][4^3]
    float* out;                // [n][cout][8]
    double2* stats;            // [n][cout]
    const h8 *w1, *w2;         // rf_conv3_e2_split_pack_weight images, edge 2
    const float *g1, *b1, *g2, *b2;
    const double2* skip_stats; // [n][c_skip][t_skip] or null (no table)
    const float *gd, *bd;
    float4* dec;               // [n][c_skip + cout]
    double eps1, eps2, epsd;
    int n, c, cm, co, groups1, groups2, c_skip, t_skip, groups_d;
};

// the value lane ^ D holds (D = 1, 2, 4: inside a group of 8 lanes), what __shfl_xor(x, D, 64) returns -- as DPP moves on the VALU: the shuffle is a
// ds_bpermute, and the statistics butterflies of a workgroup are 12,288 of them on the CU's one LDS pipe.  D = 4: lanes 0-3 / 8-11 of a row read four lanes up
// (row_shl:4 under bank mask 0101), lanes 4-7 / 12-15 four lanes down (row_shr:4 under 1010).
template <int D>
__device__ __forceinline__ int lv_xor32(int v) {
    static_assert(D == 1 || D == 2 || D == 4, "inside 8 lanes");
    if constexpr (D == 1) return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);          // quad_perm:[1,0,3,2]
    else if constexpr (D == 2) return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);     // quad_perm:[2,3,0,1]
    else {
        const int t = __builtin_amdgcn_update_dpp(0, v, 0x104, 0xf, 0x5, false);                    // row_shl:4
        return __builtin_amdgcn_update_dpp(t, v, 0x114, 0xf, 0xA, false);                           // row_shr:4
    }
}
template <int D>
__device__ __forceinline__ double lv_xor(double x) {
    return __hiloint2double(lv_xor32<D>(__double2hiint(x)), lv_xor32<D>(__double2loint(x)));
}

// sm, sq += the entries p[0 .. len) in that order, as `for (i) { sm += p[i].x; sq += p[i].y; }` does -- with the loads of eight entries issued together
__device__ __forceinline__ void lv_seq_sum(const double2* p, int len, double& sm, double& sq) {
    for (int i0 = 0; i0 < len; i0 += 8) {
        double2 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[i0 + k < len ? i0 + k : len - 1];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (i0 + k < len) { sm += v[k].x; sq += v[k].y; }
    }
}

// the GEMM of one 512-column pass: A image in LDS (ks k-steps), this wave's four n-blocks of B from wb (lane's h8 of k-step 0, n-block 0, piece h) through
// the register ring.  k-steps ascend; per tile and k-step hi += ah bh, lo += ah bl, lo += al bh (k_conv3_e2_split's order).  ks >= LV_RING - 1.
__device__ __forceinline__ void lv_gemm(const h8* __restrict__ aimg, const h8* __restrict__ wb, int ks, int lane, f32x4 (&hi)[2][4], f32x4 (&lo)[2][4]) {
    h8 ring[LV_RING][8];
    auto load = [&](int slot, int s) {
#pragma unroll
        for (int q = 0; q < 8; ++q) ring[slot][q] = wb[(size_t)s * LV_STEP_H8 + q * 64];      // q = 2 j + piece: [n-block][h | l][lane]
    };
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { hi[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; lo[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int r = 0; r < LV_RING - 1; ++r) load(r, r);
    // unrolled over the most k-steps an A image holds, forward exits only: inside a rolled loop the compiler's wait counts drain the whole ring at the back edge
#pragma unroll
    for (int s = 0; s < LV_CMAX / 4; ++s) {
        {
            const int r = s % LV_RING;
            if (s >= ks) break;
            if (s + LV_RING - 1 < ks) load((r + LV_RING - 1) % LV_RING, s + LV_RING - 1);
            h8 ah[2], al[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ah[i] = aimg[((s * 2 + i) * 2 + 0) * 64 + lane];
                al[i] = aimg[((s * 2 + i) * 2 + 1) * 64 + lane];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) hi[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], ring[r][2 * j], hi[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) lo[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], ring[r][2 * j + 1], lo[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) lo[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], ring[r][2 * j], lo[i][j], 0, 0, 0);
        }
    }
}

// the triples of a [LV_M][C] tensor from its per-(sample, channel) sums in LDS: group sums as k_gn_from_stats<1> (sequential float64 adds in channel order from 0.0)
__device__ __forceinline__ void lv_triples(const double2* st, float4* trip, int C, int cpg, double count, double eps, const float* __restrict__ gamma,
                                           const float* __restrict__ beta, int tid) {
    for (int u = tid; u < LV_M * C; u += LV_THREADS) {
        const int sl = u / C, c = u - sl * C, ca = (c / cpg) * cpg;
        const double2* p = st + sl * C + ca;
        double sm = 0.0, sq = 0.0;
        lv_seq_sum(p, cpg, sm, sq);
        trip[u] = rf_gn_triple(sm, sq, count, eps, gamma[c], beta[c]);
    }
}

__global__ __launch_bounds__(LV_THREADS, 1) void k_conv3_e2_level(LvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    h8* aimg = reinterpret_cast<h8*>(lds_raw);
    _Float16* a16 = reinterpret_cast<_Float16*>(lds_raw);
    double2* st = reinterpret_cast<double2*>(lds_raw + LV_A_BYTES);
    float4* trip = reinterpret_cast<float4*>(lds_raw + LV_A_BYTES + LV_S_BYTES / 2);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kg = lane >> 4;
    const int n0 = blockIdx.x * LV_M;
    const int C = a.c, CM = a.cm, CO = a.co;

    // ---- phase 0: pool (k_maxpool2_small<8>: lane = (plane, pooled voxel o), rf_max over the same 8 inputs, butterfly 4, 2, 1)
    const int planes = LV_M * C;                                   // a multiple of 64: an iteration's 64 planes are all inside the tile or all past it
    const int o = tid & 7, ox = o & 1, oy = (o >> 1) & 1, oz = o >> 2;
    const int voff = ((2 * oz) * 4 + 2 * oy) * 4 + 2 * ox;
    float m[32];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        float2 v[8][4];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int pl = (b * 8 + q) * 64 + (tid >> 3);
            const int sl = pl / C;
            const bool live = pl < planes && n0 + sl < a.n;
            const float* src = a.x + ((size_t)n0 * C + (live ? pl : 0)) * 64 + voff;       // plane 0 of the tile exists
#pragma unroll
            for (int d = 0; d < 4; ++d) v[q][d] = *reinterpret_cast<const float2*>(src + ((d >> 1) * 4 + (d & 1)) * 4);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int pl = (b * 8 + q) * 64 + (tid >> 3);
            const int sl = pl / C;
            const bool live = pl < planes && n0 + sl < a.n;
            float mm = -INFINITY;
#pragma unroll
            for (int d = 0; d < 4; ++d) mm = rf_max(mm, rf_max(v[q][d].x, v[q][d].y));
            mm = live ? mm : 0.f;
            m[b * 8 + q] = mm;
            double sm = (double)mm, sq = (double)mm * mm;
            sm += lv_xor<4>(sm); sq += lv_xor<4>(sq);
            sm += lv_xor<2>(sm); sq += lv_xor<2>(sq);
            sm += lv_xor<1>(sm); sq += lv_xor<1>(sq);
            if (o == 0 && pl < planes) st[pl] = make_double2(sm, sq);
        }
    }
    __syncthreads();
    lv_triples(st, trip, C, C / a.groups1, (double)(C / a.groups1) * 8.0, a.eps1, a.g1, a.b1, tid);
    __syncthreads();
    // the first A image: K index 32 s + 8 kg + j <-> channel 4 s + kg, voxel j; row = sample
#pragma unroll
    for (int it = 0; it < 32; ++it) {
        const int pl = it * 64 + (tid >> 3);
        if (pl < planes) {
            const int sl = pl / C, c = pl - sl * C;
            const float4 t = trip[pl];
            _Float16 h, l;
            rf_split(fmaf(m[it] - t.x, t.y, t.z) * SPLIT_ACT_SCALE, h, l);
            const int e = ((((c >> 2) * 2 + (sl >> 4)) * 2) * 64 + (c & 3) * 16 + (sl & 15)) * 8 + o;
            a16[e] = h;
            a16[e + 64 * 8] = l;
        }
    }
    __syncthreads();

    // ---- GEMM 1: columns 64 wave .. 64 wave + 63 of 8 cmid = 512 (cmid = 64)
    f32x4 hi[2][4], lo[2][4];
    const int ks1 = C >> 2, ks2 = CM >> 2, t0 = (wave & 3) * 4;
    lv_gemm(aimg, a.w1 + ((size_t)(wave >> 2) * ks1) * LV_STEP_H8 + t0 * 128 + lane, ks1, lane, hi, lo);
    // D[row = sample 4 kg + r of the m-block][col = li]: column 64 wave + 16 j + li -> (cm, v).  Statistics: the e2 kernel's butterfly over the 8 voxel lanes
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float y = rf_relu(rf_split_join(hi[i][j][r], lo[i][j][r]));
                hi[i][j][r] = y;
                double sv = (double)y, sq = (double)y * (double)y;
                sv += lv_xor<1>(sv); sq += lv_xor<1>(sq);
                sv += lv_xor<2>(sv); sq += lv_xor<2>(sq);
                sv += lv_xor<4>(sv); sq += lv_xor<4>(sq);
                if ((li & 7) == 0) st[(i * 16 + kg * 4 + r) * CM + wave * 8 + j * 2 + (li >> 3)] = make_double2(sv, sq);
            }
    __syncthreads();                                                // ... and every wave has read the first A image for the last time
    lv_triples(st, trip, CM, CM / a.groups2, (double)(CM / a.groups2) * 8.0, a.eps2, a.g2, a.b2, tid);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cm = wave * 8 + j * 2 + (li >> 3);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = kg * 4 + r;
                const float4 t = trip[(i * 16 + row) * CM + cm];
                _Float16 h, l;
                rf_split(fmaf(hi[i][j][r] - t.x, t.y, t.z) * SPLIT_ACT_SCALE, h, l);
                const int e = ((((cm >> 2) * 2 + i) * 2) * 64 + (cm & 3) * 16 + row) * 8 + (li & 7);
                a16[e] = h;
                a16[e + 64 * 8] = l;
            }
        }
    __syncthreads();

    // ---- GEMM 2: 8 cout columns in passes of 512
    const int ncols = CO * 8;
    const bool table = a.dec != nullptr;
    for (int pass = 0; pass < ncols / 512; ++pass) {
        lv_gemm(aimg, a.w2 + ((size_t)(pass * 2 + (wave >> 2)) * ks2) * LV_STEP_H8 + t0 * 128 + lane, ks2, lane, hi, lo);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = pass * 512 + wave * 64 + j * 16 + li;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = i * 16 + kg * 4 + r, sm = n0 + row;
                    const float y = rf_relu(rf_split_join(hi[i][j][r], lo[i][j][r]));
                    const bool live = sm < a.n;
                    if (live) a.out[(size_t)sm * ncols + col] = y;
                    double sv = (double)y, sq = (double)y * (double)y;
                    sv += lv_xor<1>(sv); sq += lv_xor<1>(sq);
                    sv += lv_xor<2>(sv); sq += lv_xor<2>(sq);
                    sv += lv_xor<4>(sv); sq += lv_xor<4>(sq);
                    if ((li & 7) == 0) {
                        if (live) a.stats[(size_t)sm * CO + (col >> 3)] = make_double2(sv, sq);
                        if (table) st[row * CO + (col >> 3)] = make_double2(sv, sq);       // the S region: its last readers passed the barrier before GEMM 2
                    }
                }
            }
    }
    if (!table) return;                                             // uniform over the grid

    // ---- the decoder stage's GroupNorm over c_skip skip channels + cout upsampled channels (k_gn_from_stats<1>, two sources; count = channels per group x 4^3)
    __syncthreads();                                                // ... and the A image is dead
    double2* gs = reinterpret_cast<double2*>(lds_raw);
    const int c0 = a.c_skip, CD = c0 + CO, GD = a.groups_d, cpg = CD / GD, tl = a.t_skip;
    for (int u = tid; u < LV_M * GD; u += LV_THREADS) {
        const int sl = u / GD, g = u - sl * GD, nn = n0 + sl;
        if (nn >= a.n) continue;
        const int ca = g * cpg, cb = ca + cpg;
        double sm = 0.0, sq = 0.0;
        {
            const int hi_c = cb < c0 ? cb : c0;
            if (ca < hi_c) {
                const double2* p = a.skip_stats + ((size_t)nn * c0 + ca) * tl;
                const int len = (hi_c - ca) * tl;
                lv_seq_sum(p, len, sm, sq);
            }
        }
        {
            const int lo_c = ca > c0 ? ca : c0;
            if (lo_c < cb) {
                const double2* p = st + sl * CO + (lo_c - c0);
                const int len = cb - lo_c;
                double s1 = 0.0, s2 = 0.0;
                lv_seq_sum(p, len, s1, s2);
                sm += 8.0 * s1;
                sq += 8.0 * s2;
            }
        }
        gs[u] = make_double2(sm, sq);
    }
    __syncthreads();
    const double count = (double)cpg * 64.0;
    for (int e = tid; e < LV_M * CD; e += LV_THREADS) {
        const int sl = e / CD, c = e - sl * CD, nn = n0 + sl;
        if (nn >= a.n) continue;
        const double2 s = gs[sl * GD + c / cpg];
        a.dec[(size_t)nn * CD + c] = rf_gn_triple(s.x, s.y, count, a.epsd, a.gd[c], a.bd[c]);
    }
}

// The form stands in for the six-launch route only where that route runs the kernels whose sums it restates: rf_gn_from_stats takes its one-thread-per-unit
// form (k_gn_from_stats<1>) when n * groups >= 1024 and a group spans <= 128 statistics entries; below that its 64-lane form sums in another order.
static bool lv_gn_plan(int n, int channels, int groups, int tiles) {
    return groups > 0 && channels % groups == 0 && (long long)n * groups >= 1024 && (long long)(channels / groups) * tiles <= 128;
}

// c_skip = 0: no decoder table (tiles_skip and groups_dec are then not read)
extern "C" int rf_conv3d_e2_level_supported(int n, int c, int cmid, int cout, int groups1, int groups2, int c_skip, int tiles_skip, int groups_dec) {
    if (n < 1 || c < 8 || c > LV_CMAX || c % 4 != 0 || cmid != 64 || (cout != 64 && cout != LV_COMAX)) return 0;     // the tiling: whole k-steps, one A image, 512 mid columns
    if (!lv_gn_plan(n, c, groups1, 1) || !lv_gn_plan(n, cmid, groups2, 1)) return 0;
    if (c_skip < 0 || (c_skip > 0 && (tiles_skip < 1 || groups_dec > 128 || !lv_gn_plan(n, c_skip + cout, groups_dec, tiles_skip)))) return 0;     // (its group sums: one A image)
    return 1;
}

extern "C" int rf_conv3d_e2_level(const float* x, int n, int c, const float* gamma1, const float* beta1, int groups1, float eps1, const void* w1_packed, int cmid,
                                  const float* gamma2, const float* beta2, int groups2, float eps2, const void* w2_packed, int cout, float* out, double* stats,
                                  const double* skip_stats, int c_skip, int tiles_skip, const float* gamma_dec, const float* beta_dec, int groups_dec,
                                  float eps_dec, float* dec_affine, void* stream) {
    RF_REQUIRE(rf_conv3d_e2_level_supported(n, c, cmid, cout, groups1, groups2, c_skip, tiles_skip, groups_dec), RF_E_UNSUPPORTED,
               "rf_conv3d_e2_level: takes c = 8 .. 64 (a multiple of 4), cmid 64, cout 64 or 128, and GroupNorm plans of at least 1024 (sample, group) units with at most "
               "128 entries per group (got n=%d c=%d cmid=%d cout=%d groups=%d,%d skip=%d x %d tiles, %d groups)", n, c, cmid, cout, groups1, groups2, c_skip,
               tiles_skip, groups_dec);
    RF_REQUIRE(x && gamma1 && beta1 && w1_packed && gamma2 && beta2 && w2_packed && out && stats, RF_E_INVALID, "rf_conv3d_e2_level: null pointer");
    RF_REQUIRE(c_skip == 0 || (skip_stats && gamma_dec && beta_dec && dec_affine), RF_E_INVALID, "rf_conv3d_e2_level: null pointer (decoder table)");
    LvArgs a;
    a.x = x; a.out = out; a.stats = reinterpret_cast<double2*>(stats);
    a.w1 = reinterpret_cast<const h8*>(w1_packed); a.w2 = reinterpret_cast<const h8*>(w2_packed);
    a.g1 = gamma1; a.b1 = beta1; a.g2 = gamma2; a.b2 = beta2;
    a.skip_stats = c_skip ? reinterpret_cast<const double2*>(skip_stats) : nullptr;
    a.gd = gamma_dec; a.bd = beta_dec; a.dec = c_skip ? reinterpret_cast<float4*>(dec_affine) : nullptr;
    a.eps1 = (double)eps1; a.eps2 = (double)eps2; a.epsd = (double)eps_dec;
    a.n = n; a.c = c; a.cm = cmid; a.co = cout; a.groups1 = groups1; a.groups2 = groups2; a.c_skip = c_skip; a.t_skip = tiles_skip; a.groups_d = groups_dec;
    return rf_launch<k_conv3_e2_level>("rf_conv3d_e2_level", dim3((unsigned)((n + LV_M - 1) / LV_M)), dim3(LV_THREADS), LV_LDS_BYTES, LV_LDS_BYTES, (hipStream_t)stream, a);
}
