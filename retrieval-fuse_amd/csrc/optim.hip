// The optimiser step (include/rfuse_optim.h): torch/optim/adam.py:_single_tensor_adam (amsgrad=False, maximize=False, capturable=False) over a list of
// tensors.  torch's default (foreach) Adam makes about a dozen multi-tensor passes over every parameter and state tensor; this is one pass: p, g, m, v
// read once, p, m, v written once (28 bytes per element).
//
//   k_adam   one workgroup of 4 waves per SEGMENT of kSegment consecutive elements of one tensor.  The records of up to kMaxTensors tensors and the
//            prefix table first[] (first[t] = segments of the tensors before t) travel BY VALUE in the kernel arguments: nothing to stage, nothing that
//            could be stale (gradient pointers change every step).  A workgroup finds its tensor by a binary search of first[] (wave-uniform scalar
//            loads from the argument segment) and its segment as blockIdx.x - first[t].  Where the four pointers of a record are 16-byte aligned the
//            segment's whole quads are 16-byte loads and stores (a segment starts at a multiple of kSegment elements, so it stays aligned) and the
//            up-to-3 elements of the tensor's tail are 4-byte ones; a record with any other alignment (a view at an odd element offset) is updated with
//            4-byte accesses throughout.  The grid is the sum of the segments: one workgroup for a bias of 16 elements, 489 for 10^6.
//
// The file is built with -ffp-contract=off: the compiler fuses nothing.  The update is torch's CPU kernels' sequence of float32 roundings, which has three
// fused multiply-adds (the weight decay's add with alpha, lerp, addcmul), written here as explicit fmaf(); hipcc's float `/` and sqrtf() are correctly
// rounded.  The result depends on nothing but the inputs.
#include "common.h"
#include "../../include/rfuse_optim.h"

namespace {
constexpr int kMaxTensors = 48;               // 48 * 64 + 49 * 4 = 3268 bytes of the 4 KB of kernel arguments
constexpr int kThreads = 256;
constexpr int kSegment = 2048;                // elements per workgroup: two 16-byte accesses per thread and array
constexpr int kQuadsPerThread = kSegment / 4 / kThreads;
constexpr long long kMaxElements = (1ll << 31) - 1;

struct HostRecord {                           // the table the caller fills (rfuse_optim.h)
    uint64_t p, g, m, v;
    int64_t n;
    float neg_step, bc2_sqrt, w1, beta2, w2, eps, wd;
    uint32_t unused;
};
static_assert(sizeof(HostRecord) == 72, "rfuse_optim.h states 72 bytes");

struct Scalars {
    float neg_step, bc2_sqrt, w1, beta2, w2, eps, wd;
};
struct Record {
    float* p;
    const float* g;
    float* m;
    float* v;
    Scalars s;
    unsigned n;
};
static_assert(sizeof(Record) == 64, "48 records and the prefix table fit the kernel arguments");

struct AdamArgs {
    Record rec[kMaxTensors];
    unsigned first[kMaxTensors + 1];          // first[t] = segments before tensor t; the entries past the last tensor hold the total
};
static_assert(sizeof(AdamArgs) <= 3584, "HIP passes 4 KB of kernel arguments; leave room for the hidden ones");

// one element, in torch's order (see the header).  `decay` and `low` are wave-uniform.  The three fmaf() are the three places where torch's own CPU
// kernels round once (add with alpha, lerp, addcmul: each checked against an exact emulation, tests/optim_ref.py); everything else rounds per operation.
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const Scalars& s, bool decay, bool low) {
    if (decay) g = fmaf(s.wd, p, g);
    const float d = g - m;
    m = low ? fmaf(s.w1, d, m) : fmaf(-d, 1.f - s.w1, g);
    v = fmaf(s.w2 * g, g, v * s.beta2);
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    p = p + (s.neg_step * m) / denom;
}
}   // namespace

__global__ __launch_bounds__(kThreads) void k_adam(const AdamArgs a) {
    const unsigned b = blockIdx.x;
    int lo = 0, hi = kMaxTensors;             // first[lo] <= b < first[hi]: first[0] = 0, first[kMaxTensors] = the grid
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.first[mid] <= b) lo = mid;
        else hi = mid;
    }
    const Scalars s = a.rec[lo].s;
    float* __restrict__ p = a.rec[lo].p;
    const float* __restrict__ g = a.rec[lo].g;
    float* __restrict__ m = a.rec[lo].m;
    float* __restrict__ v = a.rec[lo].v;
    const unsigned n = a.rec[lo].n;
    const unsigned s0 = (b - a.first[lo]) * (unsigned)kSegment;
    if (s0 >= n) return;                      // cannot happen for a table rf_adam_step built; a bound all the same
    const unsigned len = n - s0 < (unsigned)kSegment ? n - s0 : (unsigned)kSegment;
    const bool decay = s.wd != 0.f, low = fabsf(s.w1) < 0.5f;
    const bool aligned = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15u) == 0;
    p += s0, g += s0, m += s0, v += s0;
    unsigned done = 0;
    if (aligned) {
        const unsigned quads = len >> 2;
#pragma unroll
        for (int k = 0; k < kQuadsPerThread; ++k) {
            const unsigned q = k * kThreads + threadIdx.x;
            if (q < quads) {
                f32x4 pp = reinterpret_cast<const f32x4*>(p)[q], mm = reinterpret_cast<const f32x4*>(m)[q], vv = reinterpret_cast<const f32x4*>(v)[q];
                const f32x4 gg = reinterpret_cast<const f32x4*>(g)[q];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pe = pp[e], me = mm[e], ve = vv[e];
                    adam_one(pe, gg[e], me, ve, s, decay, low);
                    pp[e] = pe, mm[e] = me, vv[e] = ve;
                }
                reinterpret_cast<f32x4*>(p)[q] = pp;
                reinterpret_cast<f32x4*>(m)[q] = mm;
                reinterpret_cast<f32x4*>(v)[q] = vv;
            }
        }
        done = quads << 2;
    }
    for (unsigned i = done + threadIdx.x; i < len; i += kThreads) {
        float pe = p[i], me = m[i], ve = v[i];
        adam_one(pe, g[i], me, ve, s, decay, low);
        p[i] = pe, m[i] = me, v[i] = ve;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int rf_adam_step_max_tensors(void) { return kMaxTensors; }
extern "C" int rf_adam_step_record_bytes(void) { return (int)sizeof(HostRecord); }
extern "C" int rf_adam_step_segment(void) { return kSegment; }

extern "C" int rf_adam_step(const void* records, int count, void* stream) {
    RF_REQUIRE(records && count >= 1, RF_E_INVALID, "rf_adam_step: bad arguments");
    const HostRecord* h = reinterpret_cast<const HostRecord*>(records);
    for (int i = 0; i < count; ++i) {
        RF_REQUIRE(h[i].p && h[i].g && h[i].m && h[i].v && ((h[i].p | h[i].g | h[i].m | h[i].v) & 3u) == 0 && h[i].n >= 1, RF_E_INVALID,
                   "rf_adam_step: bad arguments (record %d: a null or misaligned pointer, or n < 1)", i);
        RF_REQUIRE(h[i].n <= kMaxElements, RF_E_UNSUPPORTED, "rf_adam_step: record %d has %lld elements (1 <= n < 2^31)", i, (long long)h[i].n);
    }
    for (int at = 0; at < count; at += kMaxTensors) {
        const int take = count - at < kMaxTensors ? count - at : kMaxTensors;
        AdamArgs a;
        unsigned segments = 0;
        for (int t = 0; t < kMaxTensors; ++t) {
            a.first[t] = segments;
            if (t < take) {
                const HostRecord& r = h[at + t];
                a.rec[t] = Record{reinterpret_cast<float*>(r.p), reinterpret_cast<const float*>(r.g), reinterpret_cast<float*>(r.m), reinterpret_cast<float*>(r.v),
                                  Scalars{r.neg_step, r.bc2_sqrt, r.w1, r.beta2, r.w2, r.eps, r.wd}, (unsigned)r.n};
                segments += (unsigned)((r.n + kSegment - 1) / kSegment);      // <= 2^20 each, 48 of them
            } else {
                a.rec[t] = Record{nullptr, nullptr, nullptr, nullptr, Scalars{0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 0.f}, 0u};
            }
        }
        a.first[kMaxTensors] = segments;
        if (int rc = rf_launch<k_adam>("rf_adam_step", dim3(segments), dim3(kThreads), (hipStream_t)stream, a)) return rc;
    }
    return RF_OK;
}
