// Mesh evaluation metrics of the reference (util/mesh_metrics.py:13-120: compute_iou, compute_metrics, distance_p2p, get_threshold_percentage) on
// the device; the entry points are declared in include/rfuse_eval.h.  Built with -ffp-contract=off: every float64 expression below is evaluated
// operation by operation, as numpy evaluates the reference's, so the exact-argmin contract of rf_eval_nearest3 is a statement about IEEE operations.
//
//   k_face_areas / k_sample_surface   area-weighted surface samples with face normals, one Philox4x32-10 draw per sample (keyed by the seed, counter
//                                     = the sample index: the output does not depend on the launch geometry)
//   k_nn_scan / k_nn_reduce           exact nearest neighbour in 3-D by brute force in float64: a workgroup keeps kNnPer source points per thread in
//                                     registers and walks its share of the targets through LDS tiles (every lane reads the SAME target: a broadcast
//                                     read per three float64 subtractions, five multiply/adds and one compare per source).  The targets are split
//                                     over blockIdx.y so that small source clouds still fill the machine; the partial (d2, idx) pairs are merged in
//                                     ascending split order with a strict `<`, which keeps the lowest index on ties exactly as the scan itself does.
//   k_p2p_stats / k_p2p_finish        sqrt, |normal dot products|, threshold histogram (binary search, LDS bins), per-workgroup partial sums; the
//                                     finish kernel adds the partials in a fixed order and turns the histogram into cumulative counts
//   k_voxelize                        one wave per triangle over the cells of its index bounding box, 13-axis separating-axis test in float64
#include "common.h"
#include "philox.h"
#include "../../include/rfuse_eval.h"

namespace {
constexpr int kMaxPoints = 1 << 24;
constexpr int kNnThreads = 256;
constexpr int kNnPer = 4;                       // source points per thread
constexpr int kNnSrcBlock = kNnThreads * kNnPer;
constexpr int kNnTile = 1024;                   // targets per LDS tile (3 x 8 KB)
constexpr int kNnWantedBlocks = 2048;           // the target split aims at this many workgroups (8 per CU of an MI355X)
constexpr int kHistLds = 4096;                  // thresholds up to this count are binned in LDS
constexpr int kStatBlocks = 512;                // k_p2p_stats: at most this many workgroups (and partial-sum slots)
constexpr int kMaxEdge = 2048;

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int nn_splits(int n_src, int n_tgt) {
    const int src_blocks = (n_src + kNnSrcBlock - 1) / kNnSrcBlock, tiles = (n_tgt + kNnTile - 1) / kNnTile;
    const int wanted = (kNnWantedBlocks + src_blocks - 1) / src_blocks;
    return wanted < tiles ? wanted : tiles;
}

struct D3 {
    double x, y, z;
};
__device__ __forceinline__ D3 load3(const float* __restrict__ p, size_t i) { return {(double)p[3 * i], (double)p[3 * i + 1], (double)p[3 * i + 2]}; }
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ bool finite3(D3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
__device__ __forceinline__ bool face_ok(const int* __restrict__ tri, int f, int n_vert, int (&v)[3]) {
    v[0] = tri[3 * (size_t)f], v[1] = tri[3 * (size_t)f + 1], v[2] = tri[3 * (size_t)f + 2];
    return v[0] >= 0 && v[1] >= 0 && v[2] >= 0 && v[0] < n_vert && v[1] < n_vert && v[2] < n_vert;
}
}   // namespace

// ------------------------------------------------------------------------------------------------ surface sampler
__global__ __launch_bounds__(256) void k_face_areas(const float* __restrict__ vert, int n_vert, const int* __restrict__ tri, int n_tri,
                                                    double* __restrict__ areas) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_tri) return;
    int v[3];
    double a = 0.0;
    if (face_ok(tri, f, n_vert, v)) {
        const D3 p0 = load3(vert, v[0]);
        const D3 c = cross(sub(load3(vert, v[1]), p0), sub(load3(vert, v[2]), p0));
        a = 0.5 * sqrt(dot(c, c));
        if (!isfinite(a)) a = 0.0;
    }
    areas[f] = a;
}

__global__ __launch_bounds__(256) void k_sample_surface(const float* __restrict__ vert, const int* __restrict__ tri, const double* __restrict__ cdf,
                                                        int n_tri, int n, unsigned long long seed, float* __restrict__ points, int* __restrict__ face,
                                                        float* __restrict__ normals) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double total = cdf[n_tri - 1];
    if (!(total > 0.0)) {
        const float q = __builtin_nanf("");
        for (int k = 0; k < 3; ++k) points[3 * (size_t)i + k] = q, normals[3 * (size_t)i + k] = q;
        face[i] = -1;
        return;
    }
    unsigned c[4] = {(unsigned)i, 0u, 0u, 0u};
    rf_philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    const double u = ((double)(c[0] >> 5) * 67108864.0 + (double)(c[1] >> 6)) * (1.0 / 9007199254740992.0);        // 53 bits, in [0, 1)
    double r1 = ((double)c[2] + 0.5) * (1.0 / 4294967296.0), r2 = ((double)c[3] + 0.5) * (1.0 / 4294967296.0);     // in (0, 1)
    const double x = u * total;
    // the first face whose inclusive sum exceeds x (a face of area 0 repeats its predecessor's sum and cannot be it); u * total may round up to
    // total itself: then the first face that reaches total, which has a positive area too
    const bool at_end = x >= total;
    int lo = 0, hi = n_tri - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const double cm = cdf[mid];
        if (at_end ? cm >= total : cm > x) hi = mid; else lo = mid + 1;
    }
    if (r1 + r2 > 1.0) r1 = 1.0 - r1, r2 = 1.0 - r2;
    const int v0 = tri[3 * (size_t)lo], v1 = tri[3 * (size_t)lo + 1], v2 = tri[3 * (size_t)lo + 2];        // in range: its area is positive (k_face_areas)
    const D3 p0 = load3(vert, v0), e1 = sub(load3(vert, v1), p0), e2 = sub(load3(vert, v2), p0);
    points[3 * (size_t)i] = (float)((p0.x + r1 * e1.x) + r2 * e2.x);
    points[3 * (size_t)i + 1] = (float)((p0.y + r1 * e1.y) + r2 * e2.y);
    points[3 * (size_t)i + 2] = (float)((p0.z + r1 * e1.z) + r2 * e2.z);
    const D3 nrm = cross(e1, e2);
    const double len = sqrt(dot(nrm, nrm));
    normals[3 * (size_t)i] = (float)(nrm.x / len);
    normals[3 * (size_t)i + 1] = (float)(nrm.y / len);
    normals[3 * (size_t)i + 2] = (float)(nrm.z / len);
    face[i] = lo;
}

// ------------------------------------------------------------------------------------------------ exact nearest neighbour
// grid (source blocks, splits).  Split s scans the targets [s * chunk, min(n_tgt, (s + 1) * chunk)), chunk a multiple of kNnTile, and writes its
// (d2, idx) for every source of the block to out_d2 / out_idx + s * n_src.
__global__ __launch_bounds__(kNnThreads) void k_nn_scan(const float* __restrict__ src, int n_src, const float* __restrict__ tgt, int n_tgt, int chunk,
                                                        double* __restrict__ out_d2, int* __restrict__ out_idx) {
    __shared__ double tx[kNnTile], ty[kNnTile], tz[kNnTile];
    const double qnan = __builtin_nan("");
    double sx[kNnPer], sy[kNnPer], sz[kNnPer], best[kNnPer];
    int bi[kNnPer];
#pragma unroll
    for (int r = 0; r < kNnPer; ++r) {
        const int s = blockIdx.x * kNnSrcBlock + r * kNnThreads + threadIdx.x;
        const bool in = s < n_src;
        sx[r] = in ? (double)src[3 * (size_t)s] : qnan;           // a NaN source never updates
        sy[r] = in ? (double)src[3 * (size_t)s + 1] : qnan;
        sz[r] = in ? (double)src[3 * (size_t)s + 2] : qnan;
        best[r] = __builtin_inf();
        bi[r] = 0;
    }
    const int begin = blockIdx.y * chunk, end = min(n_tgt, begin + chunk);
    for (int j0 = begin; j0 < end; j0 += kNnTile) {
        const int cnt = min(kNnTile, end - j0);
        __syncthreads();
        for (int k = threadIdx.x; k < cnt; k += kNnThreads) {
            const size_t j = (size_t)(j0 + k);
            tx[k] = (double)tgt[3 * j];
            ty[k] = (double)tgt[3 * j + 1];
            tz[k] = (double)tgt[3 * j + 2];
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < cnt; ++k) {
            const double x = tx[k], y = ty[k], z = tz[k];
#pragma unroll
            for (int r = 0; r < kNnPer; ++r) {
                const double dx = sx[r] - x, dy = sy[r] - y, dz = sz[r] - z;
                const double d = (dx * dx + dy * dy) + dz * dz;
                if (d < best[r]) {                                 // ascending j and a strict `<`: the lowest index of a tie stays
                    best[r] = d;
                    bi[r] = j0 + k;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kNnPer; ++r) {
        const int s = blockIdx.x * kNnSrcBlock + r * kNnThreads + threadIdx.x;
        if (s < n_src) {
            out_d2[(size_t)blockIdx.y * n_src + s] = best[r];
            out_idx[(size_t)blockIdx.y * n_src + s] = bi[r];
        }
    }
}

__global__ __launch_bounds__(256) void k_nn_reduce(const double* __restrict__ part_d2, const int* __restrict__ part_idx, int n_src, int splits,
                                                   double* __restrict__ d2, int* __restrict__ idx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_src) return;
    double best = __builtin_inf();
    int bi = 0;
    for (int s = 0; s < splits; ++s) {
        const double d = part_d2[(size_t)s * n_src + i];
        if (d < best) {
            best = d;
            bi = part_idx[(size_t)s * n_src + i];
        }
    }
    d2[i] = best;
    idx[i] = bi;
}

// ------------------------------------------------------------------------------------------------ point-to-point statistics
__global__ __launch_bounds__(256) void k_p2p_stats(const double* __restrict__ d2, const int* __restrict__ idx, const float* __restrict__ nsrc,
                                                   const float* __restrict__ ntgt, int n, int n_tgt, const double* __restrict__ thr, int n_thr,
                                                   double* __restrict__ dist, double* __restrict__ dots, unsigned long long* __restrict__ counts,
                                                   double* __restrict__ partial) {
    __shared__ unsigned hist[kHistLds];
    __shared__ double red[4][3];
    const bool lds_hist = n_thr <= kHistLds;
    if (lds_hist)
        for (int t = threadIdx.x; t < n_thr; t += blockDim.x) hist[t] = 0u;
    __syncthreads();
    double s_dist = 0.0, s_d2 = 0.0, s_dot = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double q, d;
        if (d2) {
            q = d2[i];
            d = sqrt(q);
            dist[i] = d;
        } else {                                                     // distances given: statistics only
            d = dist[i];
            q = d * d;
        }
        double nd = __builtin_nan("");
        const int j = idx ? idx[i] : -1;
        if (nsrc && ntgt && j >= 0 && j < n_tgt) {
            D3 a = load3(ntgt, (size_t)j), b = load3(nsrc, (size_t)i);
            const double la = sqrt(dot(a, a)), lb = sqrt(dot(b, b));
            a = {a.x / la, a.y / la, a.z / la};
            b = {b.x / lb, b.y / lb, b.z / lb};
            nd = fabs(dot(a, b));
        }
        dots[i] = nd;
        s_dist += d;
        s_d2 += q;
        s_dot += nd;
        int lo = 0, hi = n_thr;                                      // the first threshold >= dist; none (or a NaN distance): counted nowhere
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (thr[mid] >= d) hi = mid; else lo = mid + 1;
        }
        if (lo < n_thr) {
            if (lds_hist) atomicAdd(&hist[lo], 1u);
            else atomicAdd(&counts[lo], 1ull);
        }
    }
    rf_waves_put(red, {wave_sum(s_dist), wave_sum(s_d2), wave_sum(s_dot)});
    if (threadIdx.x < 3) partial[3 * blockIdx.x + threadIdx.x] = rf_waves_sum(red, threadIdx.x);
    if (lds_hist)
        for (int t = threadIdx.x; t < n_thr; t += blockDim.x)
            if (hist[t]) atomicAdd(&counts[t], (unsigned long long)hist[t]);
}

// one workgroup: sums[k] = the partial sums added in slot order (one thread's serial sum, numpy's order: no rf_tree_sum); counts: histogram -> inclusive prefix sums
__global__ __launch_bounds__(256) void k_p2p_finish(const double* __restrict__ partial, int n_partial, unsigned long long* __restrict__ counts, int n_thr,
                                                    double* __restrict__ sums) {
    __shared__ unsigned long long chunk_sum[256];
    if (threadIdx.x < 3) {
        double s = 0.0;
        for (int b = 0; b < n_partial; ++b) s += partial[3 * b + threadIdx.x];
        sums[threadIdx.x] = s;
    }
    const int per = (n_thr + 255) / 256, t0 = threadIdx.x * per, t1 = min(n_thr, t0 + per);
    unsigned long long s = 0;
    for (int t = t0; t < t1; ++t) s += counts[t];
    chunk_sum[threadIdx.x] = s;
    __syncthreads();
    unsigned long long run = 0;
    for (int k = 0; k < (int)threadIdx.x; ++k) run += chunk_sum[k];
    for (int t = t0; t < t1; ++t) {
        run += counts[t];
        counts[t] = run;
    }
}

// ------------------------------------------------------------------------------------------------ surface voxelisation
namespace {
// separated along axis a?  The triangle's projections against the cube's radius h (|ax| + |ay| + |az|); the cube is closed: touching is not separated
__device__ __forceinline__ bool separated(D3 a, D3 v0, D3 v1, D3 v2, double h) {
    const double p0 = dot(a, v0), p1 = dot(a, v1), p2 = dot(a, v2);
    const double r = h * ((fabs(a.x) + fabs(a.y)) + fabs(a.z));
    return fmin(fmin(p0, p1), p2) > r || fmax(fmax(p0, p1), p2) < -r;
}
}   // namespace

__global__ __launch_bounds__(256) void k_voxelize(const float* __restrict__ vert, int n_vert, const int* __restrict__ tri, int n_tri, float pitch_f,
                                                  int lo_x, int lo_y, int lo_z, int dim_x, int dim_y, int dim_z, uint8_t* __restrict__ grid) {
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (f >= n_tri) return;
    int v[3];
    if (!face_ok(tri, f, n_vert, v)) return;
    const D3 a = load3(vert, v[0]), b = load3(vert, v[1]), c = load3(vert, v[2]);
    if (!finite3(a) || !finite3(b) || !finite3(c)) return;
    const double pitch = (double)pitch_f, h = 0.5 * pitch;
    // a superset of the cells the triangle can touch (one spare cell on either side; the test below decides), clamped to the grid while still float64
    const double lo_d[3] = {floor(fmin(fmin(a.x, b.x), c.x) / pitch - 0.5) - 1.0, floor(fmin(fmin(a.y, b.y), c.y) / pitch - 0.5) - 1.0,
                            floor(fmin(fmin(a.z, b.z), c.z) / pitch - 0.5) - 1.0};
    const double hi_d[3] = {ceil(fmax(fmax(a.x, b.x), c.x) / pitch + 0.5) + 1.0, ceil(fmax(fmax(a.y, b.y), c.y) / pitch + 0.5) + 1.0,
                            ceil(fmax(fmax(a.z, b.z), c.z) / pitch + 0.5) + 1.0};
    const int glo[3] = {lo_x, lo_y, lo_z}, gdim[3] = {dim_x, dim_y, dim_z};
    int i0[3], cnt[3];
    for (int k = 0; k < 3; ++k) {
        const double l = fmax(lo_d[k], (double)glo[k]), u = fmin(hi_d[k], (double)glo[k] + (double)(gdim[k] - 1));
        if (!(l <= u)) return;
        i0[k] = (int)l;
        cnt[k] = (int)u - (int)l + 1;
    }
    const D3 e0 = sub(b, a), e1 = sub(c, b), e2 = sub(a, c);
    const D3 nrm = cross(e0, e1);
    const D3 edges[3] = {e0, e1, e2};
    const long long cells = (long long)cnt[0] * cnt[1] * cnt[2];
    for (long long q = lane; q < cells; q += 64) {
        const int k = i0[2] + (int)(q % cnt[2]), j = i0[1] + (int)(q / cnt[2] % cnt[1]), i = i0[0] + (int)(q / cnt[2] / cnt[1]);
        const D3 ctr = {pitch * (double)i, pitch * (double)j, pitch * (double)k};
        const D3 v0 = sub(a, ctr), v1 = sub(b, ctr), v2 = sub(c, ctr);
        bool out = separated({1.0, 0.0, 0.0}, v0, v1, v2, h) || separated({0.0, 1.0, 0.0}, v0, v1, v2, h) || separated({0.0, 0.0, 1.0}, v0, v1, v2, h) ||
                   separated(nrm, v0, v1, v2, h);
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const D3 d = edges[e];
            out = out || separated({0.0, -d.z, d.y}, v0, v1, v2, h) || separated({d.z, 0.0, -d.x}, v0, v1, v2, h) ||
                  separated({-d.y, d.x, 0.0}, v0, v1, v2, h);
        }
        if (!out) grid[((size_t)(i - lo_x) * dim_y + (size_t)(j - lo_y)) * dim_z + (size_t)(k - lo_z)] = 1;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int rf_eval_face_areas(const float* vertices, int n_vert, const int* triangles, int n_tri, double* areas, void* stream) {
    RF_REQUIRE(vertices && triangles && areas && n_vert >= 1 && n_tri >= 1, RF_E_INVALID, "rf_eval_face_areas: bad arguments");
    RF_REQUIRE(n_vert <= (1 << 28) && n_tri <= (1 << 28), RF_E_UNSUPPORTED, "rf_eval_face_areas: %d vertices, %d triangles (at most 2^28 each)", n_vert, n_tri);
    return rf_launch<k_face_areas>("rf_eval_face_areas", dim3((n_tri + 255) / 256), dim3(256), (hipStream_t)stream, vertices, n_vert, triangles, n_tri, areas);
}

extern "C" int rf_eval_sample_surface(const float* vertices, const int* triangles, const double* cdf, int n_tri, int n, int64_t seed, float* points,
                                      int* face, float* normals, void* stream) {
    RF_REQUIRE(vertices && triangles && cdf && points && face && normals && n_tri >= 1 && n >= 1, RF_E_INVALID, "rf_eval_sample_surface: bad arguments");
    RF_REQUIRE(n_tri <= (1 << 28) && n <= (1 << 28), RF_E_UNSUPPORTED, "rf_eval_sample_surface: %d triangles, %d samples (at most 2^28 each)", n_tri, n);
    return rf_launch<k_sample_surface>("rf_eval_sample_surface", dim3((n + 255) / 256), dim3(256), (hipStream_t)stream, vertices, triangles, cdf, n_tri, n,
                                       (unsigned long long)seed, points, face, normals);
}

extern "C" size_t rf_eval_nearest3_ws_bytes(int n_src, int n_tgt) {
    if (n_src < 1 || n_tgt < 1 || n_src > kMaxPoints || n_tgt > kMaxPoints) return 0;
    const size_t slots = (size_t)nn_splits(n_src, n_tgt) * (size_t)n_src;
    return align256(slots * sizeof(double)) + align256(slots * sizeof(int));
}

extern "C" int rf_eval_nearest3(const float* src, int n_src, const float* tgt, int n_tgt, double* d2, int* idx, void* ws, size_t ws_bytes, void* stream) {
    RF_REQUIRE(src && tgt && d2 && idx && ws && n_src >= 1 && n_tgt >= 1, RF_E_INVALID, "rf_eval_nearest3: bad arguments");
    RF_REQUIRE(n_src <= kMaxPoints && n_tgt <= kMaxPoints, RF_E_UNSUPPORTED, "rf_eval_nearest3: %d source and %d target points (at most 2^24 each)", n_src,
               n_tgt);
    const size_t need = rf_eval_nearest3_ws_bytes(n_src, n_tgt);
    RF_REQUIRE(ws_bytes >= need, RF_E_WORKSPACE, "rf_eval_nearest3: workspace of %zu bytes, needs %zu", ws_bytes, need);
    const int splits = nn_splits(n_src, n_tgt), tiles = (n_tgt + kNnTile - 1) / kNnTile;
    const int chunk = (tiles + splits - 1) / splits * kNnTile;
    const int used = (n_tgt + chunk - 1) / chunk;            // <= splits; every used split holds at least one target
    const int src_blocks = (n_src + kNnSrcBlock - 1) / kNnSrcBlock;
    double* part_d2 = reinterpret_cast<double*>(ws);
    int* part_idx = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + align256((size_t)splits * n_src * sizeof(double)));
    hipStream_t s = (hipStream_t)stream;
    if (used == 1) return rf_launch<k_nn_scan>("rf_eval_nearest3 (scan)", dim3(src_blocks, 1), dim3(kNnThreads), s, src, n_src, tgt, n_tgt, chunk, d2, idx);
    if (int rc = rf_launch<k_nn_scan>("rf_eval_nearest3 (scan)", dim3(src_blocks, used), dim3(kNnThreads), s, src, n_src, tgt, n_tgt, chunk, part_d2, part_idx)) return rc;
    return rf_launch<k_nn_reduce>("rf_eval_nearest3 (reduce)", dim3((n_src + 255) / 256), dim3(256), s, part_d2, part_idx, n_src, used, d2, idx);
}

extern "C" size_t rf_eval_p2p_stats_ws_bytes(int n) { return n < 1 ? 0 : align256((size_t)kStatBlocks * 3 * sizeof(double)); }

extern "C" int rf_eval_p2p_stats(const double* d2, const int* idx, const float* normals_src, const float* normals_tgt, int n, int n_tgt,
                                 const double* thresholds, int n_thr, double* dist, double* dots, int64_t* counts, double* sums, void* ws, size_t ws_bytes, void* stream) {
    RF_REQUIRE(dist && dots && sums && ws && n >= 1 && n_thr >= 0 && (n_thr == 0 || (thresholds && counts)), RF_E_INVALID,
               "rf_eval_p2p_stats: bad arguments");
    RF_REQUIRE(idx || !(normals_src && normals_tgt), RF_E_INVALID, "rf_eval_p2p_stats: normals without neighbour indices");
    RF_REQUIRE(n_thr <= (1 << 24), RF_E_UNSUPPORTED, "rf_eval_p2p_stats: %d thresholds (at most 2^24)", n_thr);
    const size_t need = rf_eval_p2p_stats_ws_bytes(n);
    RF_REQUIRE(ws_bytes >= need, RF_E_WORKSPACE, "rf_eval_p2p_stats: workspace of %zu bytes, needs %zu", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    if (n_thr && hipMemsetAsync(counts, 0, (size_t)n_thr * sizeof(int64_t), s) != hipSuccess) {
        rf_set_error("rf_eval_p2p_stats: cannot clear the counts");
        return RF_E_LAUNCH;
    }
    const int blocks = (int)rf_blocks(n, 256, kStatBlocks);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    if (int rc = rf_launch<k_p2p_stats>("rf_eval_p2p_stats", dim3(blocks), dim3(256), s, d2, idx, normals_src, normals_tgt, n, n_tgt, thresholds, n_thr, dist, dots, cnt,
                                        reinterpret_cast<double*>(ws)))
        return rc;
    return rf_launch<k_p2p_finish>("rf_eval_p2p_stats (finish)", dim3(1), dim3(256), s, reinterpret_cast<const double*>(ws), blocks, cnt, n_thr, sums);
}

extern "C" int rf_eval_voxelize(const float* vertices, int n_vert, const int* triangles, int n_tri, float pitch, int lo_x, int lo_y, int lo_z, int dim_x,
                                int dim_y, int dim_z, uint8_t* grid, void* stream) {
    RF_REQUIRE(vertices && triangles && grid && n_vert >= 1 && n_tri >= 1, RF_E_INVALID, "rf_eval_voxelize: bad arguments");
    RF_REQUIRE(pitch > 0.f && pitch <= 3.0e38f, RF_E_INVALID, "rf_eval_voxelize: pitch %g (must be positive and finite)", (double)pitch);
    RF_REQUIRE(dim_x >= 1 && dim_y >= 1 && dim_z >= 1 && dim_x <= kMaxEdge && dim_y <= kMaxEdge && dim_z <= kMaxEdge, RF_E_UNSUPPORTED,
               "rf_eval_voxelize: grid of %d x %d x %d voxels (each edge must be 1..%d)", dim_x, dim_y, dim_z, kMaxEdge);
    const long long far = 1ll << 30;
    RF_REQUIRE(lo_x > -far && lo_y > -far && lo_z > -far && lo_x < far && lo_y < far && lo_z < far, RF_E_UNSUPPORTED,
               "rf_eval_voxelize: grid origin (%d, %d, %d) outside +-2^30", lo_x, lo_y, lo_z);
    RF_REQUIRE(n_tri <= (1 << 28) && n_vert <= (1 << 28), RF_E_UNSUPPORTED, "rf_eval_voxelize: %d vertices, %d triangles (at most 2^28 each)", n_vert, n_tri);
    return rf_launch<k_voxelize>("rf_eval_voxelize", dim3((n_tri + 3) / 4), dim3(256), (hipStream_t)stream, vertices, n_vert, triangles, n_tri, pitch, lo_x, lo_y, lo_z,
                                 dim_x, dim_y, dim_z, grid);
}
