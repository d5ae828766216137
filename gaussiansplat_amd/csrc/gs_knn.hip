// gs_knn.hip -- point-cloud initialisation on the device: the exact mean squared distance to the three nearest neighbours
// (gs_knn_mean_dist2, 3DGS's distCUDA2) and the model a training run starts from (gs_init_from_points).  Semantics: include/gsplat.h;
// the statements: gs_knn.h; DESIGN.md 5.8e.  Built with -ffp-contract=off.
//
// The search: the finite points are put in Morton order inside their bounding box (gs_radix_sort_u64 on key << 32 | index), cut into
// boxes of GS_KNN_BOX consecutive points with their min/max, and those into super-boxes of GS_KNN_SUPER boxes.  One wave per box, one
// query per lane: the triple is seeded from the own box, then the wave walks ALL super-boxes and, inside those that some lane cannot
// rule out, all boxes; a box is opened only when some lane's lower bound is below its b2.  Box bounds and candidates are read with
// wave-uniform addresses (the scalar path: loads only), so an opened box costs one 16-byte scalar load and 13 vector operations per
// candidate for the whole wave.  No workgroup waits for another; every loop is bounded by the box count.
#include "gs_knn.h"
#include "gs_sh.h"

#include <algorithm>

namespace {

constexpr int KNN_THREADS = 256;

// floats as words whose unsigned order is the floats' order (NaNs never get here)
__device__ __forceinline__ uint32_t ordered(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float unordered(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

__device__ __forceinline__ float wave_min(float v) { for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ float wave_max(float v) { for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o)); return v; }

__global__ void knn_init_kernel(uint32_t *__restrict__ stats) {
    const int t = threadIdx.x;
    if (t < GS_KNN_STAT_WORDS) stats[t] = t < 3 ? 0xFFFFFFFFu : 0u;       // minima, maxima, the count, the spare word
}

// bounding box and count of the finite points.  One set of atomics per WORKGROUP, and a minimum / maximum only where it still improves on
// the word (a relaxed load first: the words move one way only, so a stale value can cost an atomic, never lose one) -- with one set per
// wave on the same seven words the kernel took 0.65 ms at 1 M points, all of it waiting for atomics.
constexpr int KNN_BBOX_BLOCKS = 1024;
__global__ __launch_bounds__(KNN_THREADS) void knn_bbox_kernel(const float *__restrict__ points, int64_t n, uint32_t *__restrict__ stats) {
    __shared__ float part[KNN_THREADS / GS_WAVE][6];
    __shared__ uint32_t part_cnt[KNN_THREADS / GS_WAVE];
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    uint32_t cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * KNN_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KNN_THREADS) {
        const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
        if (gs_knn_finite(x, y, z)) {
            lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
            hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
            ++cnt;
        }
    }
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
    for (int o = 32; o; o >>= 1) cnt += __shfl_xor(cnt, o);
    const int w = threadIdx.x / GS_WAVE;
    if ((threadIdx.x & (GS_WAVE - 1)) == 0) {
        for (int a = 0; a < 3; ++a) { part[w][a] = lo[a]; part[w][3 + a] = hi[a]; }
        part_cnt[w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < KNN_THREADS / GS_WAVE; ++k) {
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], part[k][a]); hi[a] = fmaxf(hi[a], part[k][3 + a]); }
        cnt += part_cnt[k];
    }
    if (!cnt) return;
    for (int a = 0; a < 3; ++a) {
        const uint32_t l = ordered(lo[a]), h = ordered(hi[a]);
        if (l < __atomic_load_n(&stats[a], __ATOMIC_RELAXED)) atomicMin(&stats[a], l);
        if (h > __atomic_load_n(&stats[3 + a], __ATOMIC_RELAXED)) atomicMax(&stats[3 + a], h);
    }
    atomicAdd(&stats[6], cnt);
}

__global__ __launch_bounds__(KNN_THREADS) void knn_keys_kernel(const float *__restrict__ points, int64_t n, const uint32_t *__restrict__ stats,
                                                               uint64_t *__restrict__ pairs) {
    const int64_t i = (int64_t)blockIdx.x * KNN_THREADS + threadIdx.x;
    if (i >= n) return;
    const float lo[3] = {unordered(stats[0]), unordered(stats[1]), unordered(stats[2])};
    const float hi[3] = {unordered(stats[3]), unordered(stats[4]), unordered(stats[5])};
    const uint32_t key = gs_knn_key(points[3 * i], points[3 * i + 1], points[3 * i + 2], lo, hi);
    pairs[i] = ((uint64_t)key << 32) | (uint64_t)(uint32_t)i;
}

// one wave per box: the sorted points as (x, y, z, index) -- +Inf coordinates for a point that is not finite and for the padding behind
// n, which no bound and no distance can then bring into a triple -- and the min/max of the box's finite points
static_assert(GS_KNN_BOX % GS_WAVE == 0, "a box is whole waves of queries");
__global__ __launch_bounds__(GS_WAVE) void knn_gather_kernel(const float *__restrict__ points, int64_t n, const uint64_t *__restrict__ pairs,
                                                             float4 *__restrict__ sorted, float4 *__restrict__ boxes) {
    const float inf = __builtin_inff();
    float lx = inf, ly = inf, lz = inf, hx = -inf, hy = -inf, hz = -inf;
    for (int r = 0; r < GS_KNN_BOX / GS_WAVE; ++r) {
        const int64_t pos = (int64_t)blockIdx.x * GS_KNN_BOX + r * GS_WAVE + threadIdx.x;
        float4 e = make_float4(inf, inf, inf, __uint_as_float(0xFFFFFFFFu));
        if (pos < n) {
            const uint64_t p = pairs[pos];
            const uint32_t idx = (uint32_t)p;
            e.w = __uint_as_float(idx);
            if ((uint32_t)(p >> 32) != GS_KNN_KEY_NONFINITE) {
                e.x = points[3 * (int64_t)idx]; e.y = points[3 * (int64_t)idx + 1]; e.z = points[3 * (int64_t)idx + 2];
                lx = fminf(lx, e.x); ly = fminf(ly, e.y); lz = fminf(lz, e.z);
                hx = fmaxf(hx, e.x); hy = fmaxf(hy, e.y); hz = fmaxf(hz, e.z);
            }
        }
        sorted[pos] = e;                                                   // the array holds whole boxes
    }
    lx = wave_min(lx); ly = wave_min(ly); lz = wave_min(lz);
    hx = wave_max(hx); hy = wave_max(hy); hz = wave_max(hz);
    if (threadIdx.x == 0) {
        boxes[2 * (int64_t)blockIdx.x] = make_float4(lx, ly, lz, 0.0f);
        boxes[2 * (int64_t)blockIdx.x + 1] = make_float4(hx, hy, hz, 0.0f);
    }
}

__global__ __launch_bounds__(KNN_THREADS) void knn_super_kernel(const float4 *__restrict__ boxes, int nb, int ns, float4 *__restrict__ supers) {
    const int s = blockIdx.x * KNN_THREADS + threadIdx.x;
    if (s >= ns) return;
    const float inf = __builtin_inff();
    float4 lo = make_float4(inf, inf, inf, 0.0f), hi = make_float4(-inf, -inf, -inf, 0.0f);
    const int k1 = min(nb, (s + 1) * GS_KNN_SUPER);
    for (int k = s * GS_KNN_SUPER; k < k1; ++k) {
        const float4 l = boxes[2 * (int64_t)k], h = boxes[2 * (int64_t)k + 1];
        lo.x = fminf(lo.x, l.x); lo.y = fminf(lo.y, l.y); lo.z = fminf(lo.z, l.z);
        hi.x = fmaxf(hi.x, h.x); hi.y = fmaxf(hi.y, h.y); hi.z = fmaxf(hi.z, h.z);
    }
    supers[2 * (int64_t)s] = lo; supers[2 * (int64_t)s + 1] = hi;
}

// the candidates of one box into every lane's triple; `skip`: the sorted position inside the box that is the lane's own (-1: none)
__device__ __forceinline__ void knn_open_box(const float4 *__restrict__ cand, const float4 &q, int skip, float &b0, float &b1, float &b2) {
#pragma unroll 8
    for (int j = 0; j < GS_KNN_BOX; ++j) {
        const float4 c = cand[j];                                          // wave-uniform address
        float d = gs_knn_d2(q.x, q.y, q.z, c.x, c.y, c.z);
        d = j == skip ? __builtin_inff() : d;                              // self is excluded by sorted position, never by distance
        gs_knn_insert(d, b0, b1, b2);
    }
}

__global__ __launch_bounds__(GS_KNN_BOX) void knn_search_kernel(const float4 *__restrict__ sorted, const float4 *__restrict__ boxes,
                                                                const float4 *__restrict__ supers, const uint32_t *__restrict__ stats,
                                                                int64_t n, int nb, int ns, float *__restrict__ dist2) {
    const int box = blockIdx.x, lane = threadIdx.x;
    const int64_t pos = (int64_t)box * GS_KNN_BOX + lane;
    const float4 q = sorted[pos];
    const float inf = __builtin_inff();
    float b0 = inf, b1 = inf, b2 = inf;
    knn_open_box(sorted + (int64_t)box * GS_KNN_BOX, q, lane, b0, b1, b2);                // the seed: the own box
    for (int s = 0; s < ns; ++s) {
        const float4 slo = supers[2 * (int64_t)s], shi = supers[2 * (int64_t)s + 1];
        if (!__any(gs_knn_box_bound(q.x, q.y, q.z, slo.x, slo.y, slo.z, shi.x, shi.y, shi.z) < b2)) continue;
        const int k1 = min(nb, (s + 1) * GS_KNN_SUPER);
        for (int k = s * GS_KNN_SUPER; k < k1; ++k) {
            if (k == box) continue;
            const float4 lo = boxes[2 * (int64_t)k], hi = boxes[2 * (int64_t)k + 1];
            if (!__any(gs_knn_box_bound(q.x, q.y, q.z, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z) < b2)) continue;
            knn_open_box(sorted + (int64_t)k * GS_KNN_BOX, q, -1, b0, b1, b2);
        }
    }
    if (pos < n) {
        const bool ok = stats[6] >= (uint32_t)GS_KNN_MIN_POINTS && __builtin_isfinite(q.x);
        dist2[__float_as_uint(q.w)] = ok ? gs_knn_mean3(b0, b1, b2) : __builtin_nanf("");
    }
}

__global__ __launch_bounds__(KNN_THREADS) void init_from_points_kernel(GsInitPointsArgs a) {
    const int64_t i = (int64_t)blockIdx.x * KNN_THREADS + threadIdx.x;
    if (i >= a.n) return;
    for (int c = 0; c < 3; ++c) a.dst[0][3 * i + c] = a.points[3 * i + c];
    const float d = a.dist2[i];
    const float v = d > 1e-7f ? d : 1e-7f;                                 // a NaN compares false
    const float s = (float)(0.5 * log((double)v));
    for (int c = 0; c < 3; ++c) a.dst[1][3 * i + c] = s;
    a.dst[2][4 * i] = 1.0f; a.dst[2][4 * i + 1] = 0.0f; a.dst[2][4 * i + 2] = 0.0f; a.dst[2][4 * i + 3] = 0.0f;
    a.dst[3][i] = a.opacity_logit;
    float *sh = a.dst[4] + (int64_t)a.k3 * i;
    for (int c = 0; c < 3; ++c) sh[c] = a.colors ? (a.colors[3 * i + c] - 0.5f) / SH_C0 : 0.0f;
    for (int c = 3; c < a.k3; ++c) sh[c] = 0.0f;
}

}  // namespace

hipError_t gs_launch_knn_mean_dist2(const GsKnnArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const int nb = (int)gs_knn_boxes(a.n), ns = (int)gs_knn_supers(a.n);
    const int64_t chunks = (a.n + KNN_THREADS - 1) / KNN_THREADS;
    hipLaunchKernelGGL(knn_init_kernel, dim3(1), dim3(64), 0, s, a.stats);
    hipLaunchKernelGGL(knn_bbox_kernel, dim3((unsigned)std::min<int64_t>(chunks, KNN_BBOX_BLOCKS)), dim3(KNN_THREADS), 0, s, a.points, a.n, a.stats);
    hipLaunchKernelGGL(knn_keys_kernel, dim3((unsigned)chunks), dim3(KNN_THREADS), 0, s, a.points, a.n, a.stats, a.pairs_a);
    int in_b = 0;
    const hipError_t e = gs_radix_sort_u64(a.pairs_a, a.pairs_b, a.n, 32, 32 + GS_KNN_KEY_BITS + 1, a.table, a.digit_total, &in_b, s, a.ballot_ranks);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(knn_gather_kernel, dim3(nb), dim3(GS_WAVE), 0, s, a.points, a.n, in_b ? a.pairs_b : a.pairs_a, a.sorted, a.boxes);
    hipLaunchKernelGGL(knn_super_kernel, dim3((ns + KNN_THREADS - 1) / KNN_THREADS), dim3(KNN_THREADS), 0, s, a.boxes, nb, ns, a.supers);
    hipLaunchKernelGGL(knn_search_kernel, dim3(nb), dim3(GS_KNN_BOX), 0, s, a.sorted, a.boxes, a.supers, a.stats, a.n, nb, ns, a.dist2);
    return hipGetLastError();
}

hipError_t gs_launch_init_from_points(const GsInitPointsArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(init_from_points_kernel, dim3((unsigned)((a.n + KNN_THREADS - 1) / KNN_THREADS)), dim3(KNN_THREADS), 0, s, a);
    return hipGetLastError();
}
