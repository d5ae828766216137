// gs_knn.h -- point-cloud initialisation (gs_knn_mean_dist2, gs_init_from_points; semantics: include/gsplat.h).
// The statements of the exact 3-nearest-neighbour search, written ONCE: the squared distance, the Morton key of a point inside the
// cloud's bounding box, the lower bound of the squared distance from a query to a box, and the insertion into a sorted triple.
// Every function turns contraction off inside its body, so it rounds alike in every translation unit whatever that unit's flags,
// and all of them are __host__ __device__: tests/knn_host.cpp runs the whole pipeline serially on the CPU with these statements,
// against a NumPy brute force, bit for bit.
//
// Why the search is exact: d2 is a fixed sequence of individually rounded fp32 operations, rounding is monotone, and gs_knn_box_bound
// combines per-axis gaps that are <= |x_a - p_a| for every point p inside the box in the same order as d2 -- so the bound never
// exceeds the fp32 d2 of any point inside.  A box is skipped only when bound >= b2: none of its values could be < b2, and a value
// equal to b2 leaves the multiset {b0, b1, b2} as it is.
#pragma once
#include "gs_common.h"

#define GS_KNN __host__ __device__ __forceinline__
#ifndef GS_KNN_BOX
#define GS_KNN_BOX 64                      // B: consecutive sorted points per box = queries per workgroup of the search (one wave); a multiple of 64
#endif
#ifndef GS_KNN_SUPER
#define GS_KNN_SUPER 32                    // boxes per super-box (the second level of the walk)
#endif
#define GS_KNN_KEY_BITS 30                 // 10 bits per axis
#define GS_KNN_KEY_NONFINITE (1u << GS_KNN_KEY_BITS)   // above every finite point's key: non-finite points sort behind all others
#define GS_KNN_MIN_POINTS 4                // finite points a cloud needs: three neighbours besides the query

GS_KNN bool gs_knn_finite(float x, float y, float z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }

// d2(i, j) = ((dx dx + dy dy) + dz dz), d = p_i - p_j: eight fp32 operations, each rounded on its own; an overflowed square is +Inf
GS_KNN float gs_knn_d2(float xi, float yi, float zi, float xj, float yj, float zj) {
#pragma clang fp contract(off)
    const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return (dx * dx + dy * dy) + dz * dz;
}

// the cell 0..1023 of v on one axis of the bounding box [lo, hi] (finite floats, lo <= v <= hi).  In double: hi - lo cannot overflow
// there; a zero extent gives cell 0.  The key only orders the points -- no result depends on how it rounds.
GS_KNN uint32_t gs_knn_cell(float v, float lo, float hi) {
    const double ext = (double)hi - (double)lo;
    if (!(ext > 0.0)) return 0u;
    const double t = ((double)v - (double)lo) / ext * 1024.0;
    return t >= 1023.0 ? 1023u : t > 0.0 ? (uint32_t)t : 0u;
}
GS_KNN uint32_t gs_knn_spread3(uint32_t v) {          // 10 bits -> every third bit of 30
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// 30-bit Morton key of a point inside the bounding box lo[3], hi[3] of the finite points; GS_KNN_KEY_NONFINITE for a point that is not finite
GS_KNN uint32_t gs_knn_key(float x, float y, float z, const float (&lo)[3], const float (&hi)[3]) {
    if (!gs_knn_finite(x, y, z)) return GS_KNN_KEY_NONFINITE;
    return gs_knn_spread3(gs_knn_cell(x, lo[0], hi[0])) | (gs_knn_spread3(gs_knn_cell(y, lo[1], hi[1])) << 1) | (gs_knn_spread3(gs_knn_cell(z, lo[2], hi[2])) << 2);
}

// lower bound of d2(query, p) over every p with lo <= p <= hi: g_a = max(0, lo_a - x_a, x_a - hi_a), combined as d2 combines its d.
// An empty box (lo = +Inf, hi = -Inf) gives +Inf; a query at +Inf (the padding of the sorted array) gives +Inf for every box.
GS_KNN float gs_knn_box_bound(float x, float y, float z, float lox, float loy, float loz, float hix, float hiy, float hiz) {
#pragma clang fp contract(off)
    const float gx = fmaxf(0.0f, fmaxf(lox - x, x - hix));
    const float gy = fmaxf(0.0f, fmaxf(loy - y, y - hiy));
    const float gz = fmaxf(0.0f, fmaxf(loz - z, z - hiz));
    return (gx * gx + gy * gy) + gz * gz;
}

// d into the sorted triple b0 <= b1 <= b2 (the three smallest values seen; +Inf three times to start).  d is never NaN for finite
// points (Inf - Inf does not occur: the differences of finite floats are finite or one-signed infinities).
GS_KNN void gs_knn_insert(float d, float &b0, float &b1, float &b2) {
    b2 = fminf(b2, fmaxf(b1, d));
    b1 = fminf(b1, fmaxf(b0, d));
    b0 = fminf(b0, d);
}

// dist2 = ((b0 + b1) + b2) / 3.0f
GS_KNN float gs_knn_mean3(float b0, float b1, float b2) {
#pragma clang fp contract(off)
    return ((b0 + b1) + b2) / 3.0f;
}

// ---- the launchers of gs_knn.hip, as gs_api_knn.hip sees them
inline int64_t gs_knn_boxes(int64_t n) { return (n + GS_KNN_BOX - 1) / GS_KNN_BOX; }
inline int64_t gs_knn_supers(int64_t n) { return (gs_knn_boxes(n) + GS_KNN_SUPER - 1) / GS_KNN_SUPER; }
#define GS_KNN_STAT_WORDS 8                // lo[3], hi[3] as ordered words, the count of finite points, one spare

struct GsKnnArgs {
    int64_t n;
    const float *points;                   // 3 x n
    float *dist2;                          // n
    uint32_t *stats;                       // GS_KNN_STAT_WORDS
    uint64_t *pairs_a, *pairs_b;           // n (key << 32 | index) each
    float4 *sorted;                        // boxes x GS_KNN_BOX: (x, y, z, index) in key order, padded with +Inf points
    float4 *boxes;                         // 2 x boxes: {lo, hi} of the finite points of a box
    float4 *supers;                        // 2 x supers: {lo, hi} of GS_KNN_SUPER consecutive boxes
    uint32_t *table, *digit_total;         // the radix sort's scratch
    bool ballot_ranks;
};
hipError_t gs_launch_knn_mean_dist2(const GsKnnArgs &a, hipStream_t s);

struct GsInitPointsArgs {
    int64_t n;
    int k3;                                // floats of an SH row
    const float *points, *colors, *dist2;  // colors may be null
    float opacity_logit;
    float *dst[5];                         // means, scales, quats, opacities, shs
};
hipError_t gs_launch_init_from_points(const GsInitPointsArgs &a, hipStream_t s);
