// The pairwise occupancy IoU matrix of the reference's retrieval trainer (util/misc.py:51-59 get_iou_matrix, trainer/train_retrieval.py:85) on the
// device; the entry points are declared in include/rfuse_pairs.h.
//
//   k_iou_pack    one workgroup of 16 waves per sample: a wave turns 64 voxels into one 64-bit word (__ballot), kPackBatch words per wave in flight (a 32^3
//                 window is four such steps; the kernel is bound by their latency); the popcounts of the words -> counts[sample].  Bits at and beyond
//                 `voxels` are zero.
//   k_iou_pairs   one workgroup per tile of kT rows of a x kT rows of b.  The word loop runs over chunks of kKC words staged in LDS (the next chunk's
//                 global loads are issued before the current one is used).  Lane (ty, tx) of every wave owns the 4 x 4 pairs (4 ty + r, 4 tx + c), so a word
//                 read from LDS feeds four AND + popcount pairs; the eight waves split the words of a chunk and add their partial counts through LDS at the
//                 end.  Then iou = float(inter) / (float(union) + 1e-5f), written `repeat` x `repeat` times.
//
// LDS rows are kKC + 1 words long: the 4 (a) or 8 (b) distinct rows that the lanes of one 32-lane half read in one ds_read_b64 are 4 rows = 520 dwords
// apart, 8 banks modulo 64, and do not share a bank.  Integer sums throughout, no atomics: the same bits on every call, whatever the order.
// Workgroup sizes by A/B on one MI355X (256 -> 1024 threads to pack, 4 -> 8 waves per pair tile): the trainer's batches are bound by the chain of
// chunk loads of a single workgroup per CU, not by the popcounts, and gain a third; B = 2048, which is bound by the popcounts, loses 3 %.
#include "common.h"
#include "../../include/rfuse_pairs.h"

namespace {
typedef unsigned long long u64;
constexpr int kMaxN = 8192;
constexpr long long kMaxVoxels = 1ll << 24;
constexpr int kPackThreads = 1024, kPackWaves = kPackThreads / 64;
constexpr int kPackBatch = 8;                        // words per wave and step: the loads in flight
constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr int kT = 32;                               // rows of a and rows of b per tile: 8 x 8 lanes, 4 x 4 pairs each
constexpr int kKC = 64;                              // words per LDS chunk: one per lane when staging
constexpr int kLd = kKC + 1;                         // odd row length in words (see above)
constexpr int kPerWave = kKC / kWaves;               // words of a chunk per wave
constexpr int kStage = 2 * kT / kWaves;              // words a thread stages per chunk: rows wave, wave + kWaves, ... of a, then of b
static_assert(kWaves * 16 * 64 * sizeof(int) <= 2 * kT * kLd * sizeof(u64), "the partial counts reuse the staging area");

const char* kRange = "%s: %d x %d samples of %lld voxels, repeat %d (1 <= samples <= 8192, 1 <= voxels <= 2^24, repeat 1 or 2)";
bool in_range(int n_a, int n_b, long long voxels) { return n_a >= 1 && n_a <= kMaxN && n_b >= 1 && n_b <= kMaxN && voxels >= 1 && voxels <= kMaxVoxels; }
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
}   // namespace

__global__ __launch_bounds__(kPackThreads) void k_iou_pack(const void* __restrict__ x, int kind, float scale, float shift, float thr, long long voxels, int words,
                                                           u64* __restrict__ bits, int* __restrict__ counts) {
    __shared__ int part[kPackWaves][1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t sample = blockIdx.x;
    const uint8_t* g = reinterpret_cast<const uint8_t*>(x) + sample * (size_t)voxels;
    const float* f = reinterpret_cast<const float*>(x) + sample * (size_t)voxels;
    int cnt = 0;
    for (int base = wave; base < words; base += kPackBatch * kPackWaves) {
        bool on[kPackBatch];
#pragma unroll
        for (int u = 0; u < kPackBatch; ++u) {
            const int word = base + u * kPackWaves;
            const long long v = 64ll * word + lane;
            on[u] = false;
            if (word < words && v < voxels) on[u] = kind == 0 ? g[v] != 0 : f[v] * scale + shift <= thr;      // NaN: unoccupied
        }
#pragma unroll
        for (int u = 0; u < kPackBatch; ++u) {
            const int word = base + u * kPackWaves;
            const u64 m = __ballot(on[u]);
            if (lane == 0 && word < words) bits[sample * words + word] = m;
            cnt += __popcll(m);
        }
    }
    rf_waves_put(part, {cnt});
    if (threadIdx.x == 0) counts[sample] = rf_waves_sum(part);
}

__global__ __launch_bounds__(kThreads) void k_iou_pairs(const u64* __restrict__ bits_a, const int* __restrict__ counts_a, int n_a, const u64* __restrict__ bits_b,
                                                        const int* __restrict__ counts_b, int n_b, int words, int repeat, float* __restrict__ out) {
    __shared__ u64 s[2 * kT * kLd];
    u64* sA = s;
    u64* sB = s + kT * kLd;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, ty = lane >> 3, tx = lane & 7;
    const int i0 = blockIdx.y * kT, j0 = blockIdx.x * kT;
    u64 pre[kStage];
    int acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0;

    // thread (wave, lane) stages word k0 + lane of rows wave + kWaves q' of the a tile (the first half of pre) and of the b tile (the second half); zeros
    // past the rows and past the words
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < kStage; ++q) {
            const bool is_a = q < kStage / 2;
            const int row = (is_a ? i0 : j0) + wv + kWaves * (q % (kStage / 2));
            const u64* src = is_a ? bits_a : bits_b;
            pre[q] = row < (is_a ? n_a : n_b) && k0 + lane < words ? src[(size_t)row * words + k0 + lane] : 0ull;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < words; k0 += kKC) {
        __syncthreads();                               // the previous chunk has been used
#pragma unroll
        for (int q = 0; q < kStage; ++q) s[(q < kStage / 2 ? 0 : kT * kLd) + (wv + kWaves * (q % (kStage / 2))) * kLd + lane] = pre[q];
        __syncthreads();
        if (k0 + kKC < words) fetch(k0 + kKC);
        const int left = words - k0 - wv * kPerWave;      // this wave's words of the chunk: uniform over the wave
        const int mine = left < kPerWave ? left : kPerWave;
        const u64* a = sA + 4 * ty * kLd + wv * kPerWave;
        const u64* b = sB + 4 * tx * kLd + wv * kPerWave;
#pragma unroll 4
        for (int w = 0; w < mine; ++w) {
            u64 av[4], bv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) av[r] = a[r * kLd + w], bv[r] = b[r * kLd + w];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[4 * r + c] += __popcll(av[r] & bv[c]);
        }
    }
    __syncthreads();
    int* red = reinterpret_cast<int*>(s);              // [wave][pair of the lane][lane]
#pragma unroll
    for (int k = 0; k < 16; ++k) red[(wv * 16 + k) * 64 + lane] = acc[k];
    __syncthreads();
    const size_t ld_out = (size_t)repeat * n_b;
#pragma unroll
    for (int q = 0; q < kT * kT / kThreads; ++q) {
        const int e = threadIdx.x + kThreads * q, il = e / kT, jl = e % kT;       // consecutive threads: consecutive columns of one row
        const int owner = (il >> 2) * 8 + (jl >> 2), k = (il & 3) * 4 + (jl & 3);
        int inter = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) inter += red[(w * 16 + k) * 64 + owner];
        const int i = i0 + il, j = j0 + jl;
        if (i < n_a && j < n_b) {
            const int uni = counts_a[i] + counts_b[j] - inter;
            const float v = (float)inter / ((float)uni + 1e-5f);
            for (int p = 0; p < repeat; ++p)
                for (int r = 0; r < repeat; ++r) out[((size_t)i + (size_t)p * n_a) * ld_out + (size_t)j + (size_t)r * n_b] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" size_t rf_iou_ws_bytes(int n_a, int n_b, long long voxels) {
    if (!in_range(n_a, n_b, voxels)) return 0;
    const size_t words = (size_t)((voxels + 63) / 64);
    return up256((size_t)n_a * words * sizeof(u64)) + up256((size_t)n_a * sizeof(int)) + up256((size_t)n_b * words * sizeof(u64)) + up256((size_t)n_b * sizeof(int));
}

extern "C" int rf_iou_pack(const void* x, int kind, float scale, float shift, float thr, int n, long long voxels, uint64_t* bits, int* counts, void* stream) {
    RF_REQUIRE(x && bits && counts && n >= 1 && voxels >= 1 && (kind == 0 || kind == 1), RF_E_INVALID, "rf_iou_pack: bad arguments");
    RF_REQUIRE(in_range(n, n, voxels), RF_E_UNSUPPORTED, kRange, "rf_iou_pack", n, n, voxels, 1);
    const int words = (int)((voxels + 63) / 64);
    return rf_launch<k_iou_pack>("rf_iou_pack", dim3((unsigned)n), dim3(kPackThreads), (hipStream_t)stream, x, kind, scale, shift, thr, voxels, words,
                                 reinterpret_cast<u64*>(bits), counts);
}

extern "C" int rf_iou_matrix(const uint64_t* bits_a, const int* counts_a, int n_a, const uint64_t* bits_b, const int* counts_b, int n_b, long long voxels,
                             int repeat, float* out, void* stream) {
    RF_REQUIRE(bits_a && counts_a && out && n_a >= 1 && n_b >= 1 && voxels >= 1 && repeat >= 1, RF_E_INVALID, "rf_iou_matrix: bad arguments");
    RF_REQUIRE(bits_b ? counts_b != nullptr : n_b == n_a, RF_E_INVALID, "rf_iou_matrix: b needs its counts, and without b n_b = n_a (got %d, %d)", n_a, n_b);
    RF_REQUIRE(in_range(n_a, n_b, voxels) && repeat <= 2, RF_E_UNSUPPORTED, kRange, "rf_iou_matrix", n_a, n_b, voxels, repeat);
    const int words = (int)((voxels + 63) / 64);
    const u64* a = reinterpret_cast<const u64*>(bits_a);
    const u64* b = bits_b ? reinterpret_cast<const u64*>(bits_b) : a;
    return rf_launch<k_iou_pairs>("rf_iou_matrix", dim3((unsigned)((n_b + kT - 1) / kT), (unsigned)((n_a + kT - 1) / kT)), dim3(kThreads), (hipStream_t)stream, a,
                                  counts_a, n_a, b, bits_b ? counts_b : counts_a, n_b, words, repeat, out);
}
