// The FIXED-ORDER reductions of the kernels' epilogues, each defined once: wave reductions, the workgroup reductions behind them (wave totals in wave order,
// the maximum over waves, the halving tree), the float64 (sum, sum of squares) butterflies of the GroupNorm
// statistics, the fused MaxPool3d(2) cell, the recursive-halving transpose sum and the cin = 1 tap loop.  The "bit-equal between routes" tests hold only while
// every route adds in the same order: a helper here owns the arithmetic and that order; the kernel keeps its barriers, sched_barriers, opaque thread-index
// copies, LDS addresses and store guards.  Device helpers only, no dependence on the rest of the library (tests/testkit probes them one by one).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------------- whole-wave reductions
// wave64 sum reduction (partner masks 32, 16, .. 1); result valid in every lane
template <class T>      // double, float; long long: the metrics' exact integer sums
__device__ __forceinline__ T wave_sum(T v) {
    static_assert(std::is_same<T, double>::value || std::is_same<T, float>::value || std::is_same<T, long long>::value, "wave_sum: double, float or long long");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// fmaxf / fmax (maxNum) on purpose: the top-k scan's seed bound (retrieval.hip), the backward pass's gradient maximum (which records a non-finite gradient
// separately) and the loss kernels' row maximum use these, no forward activation does
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// Max and ReLU of the forward kernels, NaN-propagating like the reference (torch.relu, F.max_pool3d, fp32 arithmetic).  fmaxf is IEEE maxNum (v_max_f32):
// given one NaN it returns the other operand, so a NaN accumulator came out of a ReLU as 0 and out of a max-pool as its neighbours' maximum.  For finite
// inputs these give the same bits as before.
__device__ __forceinline__ float rf_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }      // IEEE-754-2019 maximum: v_maximum3_f32
__device__ __forceinline__ float rf_relu(float v) { return __builtin_elementwise_maximum(v, 0.f); }

// ------------------------------------------------------------------------------------------------------- workgroup reductions
// The step after a wave of the loss, metric, statistics and backward kernels: wave totals -> a workgroup total.  The kernel owns the __shared__ array and
// the guard of its store; the helpers own the adds and their order.  "Two calls give the same bits", the float64 kernels that are compared bit for bit
// with numpy and the loss goldens rest on these orders (tests/test_lane_reduce_gpu.py pins them; profiles/block_reductions_ab.txt).
//
// Wave totals through LDS.  rf_waves_put: lane 0 of every wave stores the wave's K wave-uniform values (out of wave_sum / wave_max, or ballot counts) to
// red[wave][:], then the helper's ONE barrier.  After it ANY thread may take any of the K totals: thread k < K its own (one store each), thread 0 all of
// them, or every thread.  All NW waves of the workgroup call it.
template <int NW, int K, class T>
__device__ __forceinline__ void rf_waves_put(T (&red)[NW][K], const T (&v)[K]) {
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
}
// value k's total in WAVE ORDER, left to right from wave 0's own value: ((red[0][k] + red[1][k]) + red[2][k]) + ...  No zero in front: all-(-0.0) wave
// totals give -0.0, a site that used to start from a literal 0.0 writes `0.0 + rf_waves_sum(..)` to keep its +0.0.  (Also the last step of
// k_wgrad_split_reduce, whose red[slice][output] holds per-thread sums.)
template <int NW, int K, class T>
__device__ __forceinline__ T rf_waves_sum(const T (&red)[NW][K], int k = 0) {
    static_assert(std::is_same<T, double>::value || std::is_same<T, long long>::value || std::is_same<T, unsigned long long>::value || std::is_same<T, int>::value,
                  "rf_waves_sum: double, long long, unsigned long long or int");
    T s = red[0][k];
#pragma unroll
    for (int w = 1; w < NW; ++w) s += red[w][k];
    return s;
}
// value k's maximum over the waves, in no promised association.  Safe for the two gradient-maximum kernels it serves: their values are maxima of |x|
// (>= +0, never -0) and a non-finite gradient was folded into +inf beforehand, so fmaxf (maxNum) meets no NaN to drop and no -0 / +0 pair to order.
template <int NW, int K>
__device__ __forceinline__ float rf_waves_max(const float (&red)[NW][K], int k = 0) {
    float m = red[0][k];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = fmaxf(m, red[w][k]);
    return m;
}
// Halving tree over ALL NT threads of the workgroup, K values each: red[t][:] = v, then for o = NT / 2 .. 1 thread t < o does red[t][k] += red[t + o][k],
// a barrier after the store and after every level.  The totals are red[0][:], valid in thread 0 (whatever a thread added up before -- strided inputs in
// ascending order at every site -- stays in its kernel).
template <int NT, int K, class T>
__device__ __forceinline__ void rf_tree_sum(T (&red)[NT][K], const T (&v)[K]) {
    static_assert(std::is_same<T, double>::value || std::is_same<T, float>::value, "rf_tree_sum: double or float");
    static_assert(NT >= 2 && (NT & (NT - 1)) == 0, "the tree halves a power of two");
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) red[t][k] = v[k];
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int k = 0; k < K; ++k) red[t][k] += red[t + o][k];
        }
        __syncthreads();
    }
}
// Left as they are, on purpose: k_gnb_partial (run-time butterfly span, per-row wave ranges), k_gnb_finalize / k_gnb_sum_n / k_p2p_finish (one thread's
// serial sums), k_linear_wgrad (per-lane accumulators summed by wave 0), and every conv forward kernel (the sections below).

// ------------------------------------------------------------------------------------------------------- GroupNorm statistics: accumulators -> sums
// (sm, sq) += (sum, sum of squares) in float64 of the ReLU'd registers of one accumulator block, in register order ...
__device__ __forceinline__ void rf_relu_sums(const f32x4& acc, double& sm, double& sq) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double v = (double)rf_relu(acc[r]);
        sm += v; sq += v * v;
    }
}
// ... and of N blocks, block-major
template <int N>
__device__ __forceinline__ void rf_relu_sums(const f32x4 (&acc)[N], double& sm, double& sq) {
#pragma unroll
    for (int m = 0; m < N; ++m) rf_relu_sums(acc[m], sm, sq);
}

// Pair butterfly: both values summed over the lanes that differ in the mask bits FIRST .. LAST, one partner mask after the other -- doubling from FIRST when
// FIRST < LAST, halving otherwise; FIRST == 0 or LAST == 0 (a span of one lane): no step.  The mask order fixes the association of the float64 adds and with it the bits: a site keeps its own.
template <int FIRST, int LAST>
__device__ __forceinline__ void rf_xor_sum2(double& a, double& b) {
    static_assert(FIRST >= 0 && FIRST < 64 && LAST >= 0 && LAST < 64 && (FIRST & (FIRST - 1)) == 0 && (LAST & (LAST - 1)) == 0, "masks are powers of two inside a wave");
    constexpr bool UP = FIRST < LAST;
#pragma unroll
    for (int m = FIRST; m > 0 && LAST > 0 && (UP ? m <= LAST : m >= LAST); m = UP ? m << 1 : m >> 1) {
        a += __shfl_xor(a, m, 64); b += __shfl_xor(b, m, 64);
    }
}

// ------------------------------------------------------------------------------------------------------- the fused MaxPool3d(2) cell
// u, v: the accumulator blocks of the cell's two z planes (or y rows); x pairs sit in the registers (0, 1) and (2, 3), the third pair in lane ^ 32.
// (p0, p1) = the lane's two pooled, ReLU'd values, valid in both lanes of the exchange.  NaN propagates (rf_max).
__device__ __forceinline__ void rf_pool_cell(const f32x4& u, const f32x4& v, float& p0, float& p1) {
    p0 = rf_max(rf_max(u[0], u[1]), rf_max(v[0], v[1]));
    p1 = rf_max(rf_max(u[2], u[3]), rf_max(v[2], v[3]));
    p0 = rf_max(p0, __shfl_xor(p0, 32, 64));
    p1 = rf_max(p1, __shfl_xor(p1, 32, 64));
    p0 = rf_relu(p0);                                               // max and ReLU commute
    p1 = rf_relu(p1);
}
// the pooled tensor's statistics of that cell pair (the caller guards it: only one lane of each exchange counts)
__device__ __forceinline__ void rf_pool_sums(float p0, float p1, double& sm, double& sq) {
    sm += (double)p0 + (double)p1;
    sq += (double)p0 * (double)p0 + (double)p1 * (double)p1;
}

// ------------------------------------------------------------------------------------------------------- 16 values per lane -> one per lane
// Recursive-halving transpose sum over the wave: at step k = 0 .. 3 a lane keeps half of its values and hands the other half to lane ^ (1 << k) (the lane with
// bit k set keeps the upper half), then the survivor is summed over lanes ^ 16 and ^ 32 -- 17 value exchanges instead of 16 x 6.  Returns the wave's total
// of value rf_transpose_slot16(lane); v is used up.  (Sibling: pp_row16_transpose_sum8 in conv3d_up_split.hip, another partner order, on DPP.)
template <int K>      // step k as a template: its value offsets must be constants before the array can live in registers
__device__ __forceinline__ void rf_transpose_halve(double (&v)[16], int lane) {
    constexpr int C = 8 >> K;
    const bool up = (lane >> K) & 1;
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const double send = up ? v[i] : v[i + C], keep = up ? v[i + C] : v[i];
        v[i] = keep + __shfl_xor(send, 1 << K, 64);
    }
}
__device__ __forceinline__ double rf_transpose_sum16(double (&v)[16], int lane) {
    rf_transpose_halve<0>(v, lane);
    rf_transpose_halve<1>(v, lane);
    rf_transpose_halve<2>(v, lane);
    rf_transpose_halve<3>(v, lane);
    v[0] += __shfl_xor(v[0], 16, 64);
    v[0] += __shfl_xor(v[0], 32, 64);
    return v[0];
}
// which of the 16 values lane (& 15) ends up with
__device__ __forceinline__ int rf_transpose_slot16(int lane) { return (lane & 1) * 8 + ((lane >> 1) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 3) & 1); }

// ------------------------------------------------------------------------------------------------------- the cin = 1 tap loop
// One thread's (y, x) column of TZ output voxels, 2 CP couts in registers as cout PAIRS: v_pk_fma_f32 (two fp32 FMAs per lane and issue -- the 157 TFLOP/s
// vector peak is the packed rate); per output the 27 taps are accumulated one by one in (dy, dx, dz) order, each with a single rounding.  xs: the column's
// origin in the normalised halo tile (plane stride SZ, row stride SY floats); wl: [27 taps][8 couts], 16-byte aligned.
template <int TZ, int CP, int SZ, int SY>
__device__ __forceinline__ void rf_cin1_taps(const float* xs, const float* wl, f32x2 (&acc2)[TZ][CP]) {
    static_assert(CP >= 1 && CP <= 4, "a tap's weights are 8 couts = 4 pairs");
#pragma unroll
    for (int z = 0; z < TZ; ++z)
#pragma unroll
        for (int cp = 0; cp < CP; ++cp) acc2[z][cp] = (f32x2){0.f, 0.f};
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            float col[TZ + 2];
#pragma unroll
            for (int hz = 0; hz < TZ + 2; ++hz) col[hz] = xs[hz * SZ + dy * SY + dx];
#pragma unroll
            for (int dz = 0; dz < 3; ++dz) {
                const float4 w0 = *reinterpret_cast<const float4*>(wl + ((dz * 3 + dy) * 3 + dx) * 8);
                const float4 w1 = *reinterpret_cast<const float4*>(wl + ((dz * 3 + dy) * 3 + dx) * 8 + 4);
                const f32x2 wv[4] = {(f32x2){w0.x, w0.y}, (f32x2){w0.z, w0.w}, (f32x2){w1.x, w1.y}, (f32x2){w1.z, w1.w}};
#pragma unroll
                for (int z = 0; z < TZ; ++z) {
                    const f32x2 c2 = (f32x2){col[z + dz], col[z + dz]};
#pragma unroll
                    for (int cp = 0; cp < CP; ++cp) acc2[z][cp] = __builtin_elementwise_fma(c2, wv[cp], acc2[z][cp]);
                }
            }
        }
}
