// Shared device/host helpers for librfuse_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/rfuse.h"

#include "lane_reduce.h"      // f32x4, wave_sum / wave_max, rf_max / rf_relu and the fixed-order reductions of the epilogues

void rf_set_error(const char* fmt, ...);

#define RF_REQUIRE(cond, code, ...)            \
    do {                                       \
        if (!(cond)) {                         \
            rf_set_error(__VA_ARGS__);         \
            return (code);                     \
        }                                      \
    } while (0)

#define RF_CHECK_LAUNCH(name)                                                    \
    do {                                                                         \
        hipError_t e__ = hipGetLastError();                                      \
        if (e__ != hipSuccess) {                                                 \
            rf_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return RF_E_LAUNCH;                                                  \
        }                                                                        \
    } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel: a process that drives several GPUs has to
// opt in on each of them.  One instance per kernel instantiation (the function-local static of rf_launch below, its only user); bit d = "done on device d".
#include <atomic>
struct RfLdsOptIn {
    std::atomic<unsigned long long> done[4];
    RfLdsOptIn() { for (auto& d : done) d.store(0ull); }
    int ensure(const void* kernel, int bytes, const char* who) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 256) { rf_set_error("%s: cannot query the current device", who); return RF_E_LAUNCH; }
        const unsigned long long bit = 1ull << (dev & 63);
        if (done[dev >> 6].load(std::memory_order_acquire) & bit) return RF_OK;
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) { rf_set_error("%s: cannot raise the LDS limit to %d bytes: %s", who, bytes, hipGetErrorString(e)); return RF_E_LAUNCH; }
        done[dev >> 6].fetch_or(bit, std::memory_order_release);
        return RF_OK;
    }
};

// The tail of EVERY launcher (the only caller of hipLaunchKernelGGL and the only user of RfLdsOptIn): opt in where the kernel instantiation KERN ever
// asks for more than the 64 KB of dynamic LDS a kernel gets without asking, launch, check.  `lds` = this launch's bytes; `lds_limit` = the most the
// INSTANTIATION asks for, a compile-time or file-scope constant (T::LDS_BYTES, VL_LDS_MAX, ...) and never this call's `lds`: the opt-in is made once per
// device, so a limit taken from the first call would be too low for a later, larger one.  `who`: the entry point the caller serves, for the error texts.
// An entry point that launches more than once writes `if (int rc = rf_launch<...>(...)) return rc;` for all but its last launch.
template <auto KERN, class... Args>
static inline int rf_launch(const char* who, dim3 grid, dim3 block, size_t lds, size_t lds_limit, hipStream_t stream, Args... args) {
    if (lds_limit > 64 * 1024) {
        static RfLdsOptIn opt;
        if (int rc = opt.ensure(reinterpret_cast<const void*>(KERN), (int)lds_limit, who)) return rc;
    }
    hipLaunchKernelGGL(KERN, grid, block, lds, stream, args...);
    RF_CHECK_LAUNCH(who);
    return RF_OK;
}
// ... of a kernel without dynamic LDS
template <auto KERN, class... Args>
static inline int rf_launch(const char* who, dim3 grid, dim3 block, hipStream_t stream, Args... args) {
    hipLaunchKernelGGL(KERN, grid, block, 0, stream, args...);
    RF_CHECK_LAUNCH(who);
    return RF_OK;
}

// Blocks of a capped grid-stride launch: ceil(total / per_block), at most `cap`.
static inline unsigned rf_blocks(size_t total, size_t per_block, size_t cap) {
    const size_t want = (total + per_block - 1) / per_block;
    return (unsigned)(want < cap ? want : cap);
}

// out[i] = (float)(sum over g = 0..slices-1, in that order, of (double)parts[g * count + i]): the end of every split-K weight gradient whose slices
// are plain fp32 partials (rf_conv3d_k3_wgrad, rf_conv3d_valid_wgrad, rf_linear_wgrad) and of the valid conv's bias gradient
// (rf_conv3d_valid_leaky_backward).  Deterministic, no atomics.  Defined in conv3d_backward.hip.
int rf_slice_sum(const float* parts, int slices, size_t count, float* out, hipStream_t stream, const char* who);

static inline bool rf_is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
static inline int rf_ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
static inline int rf_round_up(int v, int m) { return (v + m - 1) / m * m; }

// Workgroups of a PERSISTENT launch (k_conv3_split_zc / _zcm, k_conv3_up_split_boxp: 512 threads, <= 80 KB of LDS, <= 128 VGPRs -> two resident per CU): two per
// CU of the current device (hipDeviceProp_t::multiProcessorCount, 256 on MI355X -> 512; ADVICE r4: this was a literal 512 in three launchers and in the
// scratch-slot count), times RF_PERSIST_ROUNDS.  One round = every workgroup resident for the whole launch, a static share of the items each -- and then
// the launch ends when its UNLUCKIEST workgroup does: inside the pipelined step the other streams' kernels (the chunk-level U-Net's ~40 small launches, the
// top-k scan) hold a CU for 10-100 us at a time, the workgroup that waits for that CU starts late and still has its full share in front of it (round 5:
// the U-Net backbone beside the back end cost the step 0.35 ms for ~0.1 ms of work, tools/overlap_parts.py).  With FOUR rounds the workgroups of a late CU's
// later rounds go to whichever CU is free: same-box A/B of the C2 step 1 / 2 / 4 / 8 rounds = 6.47 / 6.43 / 6.39 / 6.42 ms (tools/abn_bench.sh; 8 pays more
// prologues -- weights to LDS, first halo image -- than it balances).  The launchers and rf_conv3d_split_pre_pool_presplit_scratch_floats (a scratch
// slot per workgroup, slot = blockIdx.x) all take the count from here.
#ifndef RF_PERSIST_ROUNDS
#define RF_PERSIST_ROUNDS 4
#endif
static inline int rf_resident_wgs() {
    // per device of the process (a count cached at first call would be the first device's for every later one), cached: hipGetDeviceProperties is slow
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 512;
    if (dev < 64) {
        const int c = cached[dev].load(std::memory_order_relaxed);
        if (c > 0) return c;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount <= 0) return 512;
    if (dev < 64) cached[dev].store(2 * prop.multiProcessorCount, std::memory_order_relaxed);
    return 2 * prop.multiProcessorCount;
}
static inline int rf_persistent_wgs() { return rf_resident_wgs() * RF_PERSIST_ROUNDS; }

// Workgroups are handed to the 8 XCDs round-robin by linear id, each XCD with its own L2.  Tiles that split a sample
// (8-voxel = 32-byte row pieces of 64..512-byte rows) would then share every cache line across XCDs: partial-line writes
// that no L2 can merge and 128-byte fills for 32 bytes of use.  Remap so that XCD k walks a contiguous range of tiles.
__device__ __forceinline__ unsigned rf_xcd_contiguous(unsigned b, unsigned g) {
    const unsigned per = g >> 3, rem = g & 7u, k = b & 7u;
    return k * per + (k < rem ? k : rem) + (b >> 3);
}

// The split operands' f16-range clamp, NaN-propagating like rf_max / rf_relu (lane_reduce.h); v_med3_f32 alone returns a bound for a NaN input.
// clamp to [-65504, 65504]; NaN and +-inf come out as NaN.  0 * v is NaN for those and a zero of v's sign otherwise, and adding a zero of
// v's sign to med3(v, ...) changes no finite result (-0 included): two VALU ops (v_med3_f32 + v_fma_f32), the f16 split after it keeps the NaN.
// The fma is inline asm: as fmaf the compiler pairs it into v_pk_fma_f32 with op_sel on src1, which build.py:check_isa refuses
__device__ __forceinline__ float rf_clamp_f16(float v) {
    const float m = __builtin_amdgcn_fmed3f(v, -65504.f, 65504.f);
    float r;
    asm("v_fma_f32 %0, %1, 0, %2" : "=v"(r) : "v"(v), "v"(m));
    return r;
}

// GroupNorm as the conv kernels apply it: y = (x - center) * scale + shift with, per (sample, channel),
//   center = fl32(mean),  scale = fl32(gamma * rstd),  shift = fl32(beta - (mean - center) * gamma * rstd).
// Subtracting the (fp32-representable) centre first keeps the product at the magnitude of the RESULT: the plain two-term form
// x*scale' + shift' carries an absolute error of eps * |mean * rstd * gamma|, which for near-constant inputs (a truncation-
// saturated TSDF patch: rstd up to 316) is 100x the fp32 resolution of y and was the largest single error source of the path
// (tools/error_budget.py, first layer of the retrieval backbone).  What fl32(mean) loses is folded into `shift` in float64.
__device__ __forceinline__ float4 gn_affine(double mean, double rstd, float gamma, float beta) {
    const double sc = (double)gamma * rstd;
    const float center = (float)mean;
    return make_float4(center, (float)sc, (float)((double)beta - (mean - (double)center) * sc), 0.f);
}
// THE hand-over from (sum, sum of squares) of `count` values to that triple, float64 throughout: biased variance, clamped at 0 (cancellation
// can leave it just below), rstd = 1 / sqrt(var + eps).  Every route that derives a GroupNorm from statistics goes through here -- the "bit-equal
// between routes" tests hold only as long as there is one definition.  (Written out instead, each with its reason: k_conv3_up_split_pp, k_conv3_split's pre-split epilogue, conv3d_backward.hip.)
__device__ __forceinline__ float4 rf_gn_triple(double sm, double sq, double count, double eps, float gamma, float beta) {
    const double mean = sm / count;
    double var = sq / count - mean * mean;
    if (var < 0.0) var = 0.0;
    return gn_affine(mean, 1.0 / sqrt(var + eps), gamma, beta);
}
