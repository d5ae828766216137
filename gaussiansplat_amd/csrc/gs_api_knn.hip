// gs_api_knn.hip -- point-cloud initialisation below the C ABI: gs_knn_mean_dist2 and gs_init_from_points (the kernels are in gs_knn.hip,
// the semantics in include/gsplat.h and DESIGN.md 5.8e).  Neither call needs a model, a camera or a frame, and neither touches one: the
// scratch is the ctx's own knn_* buffers, the frame's stage and plans are not read or written.  Every refusal happens before anything is
// enqueued; nothing synchronises.
#include "gs_ctx.h"
#include "gs_knn.h"

static ByteRange range_of(const void *p, size_t floats) { return {p, sizeof(float) * floats}; }

extern "C" {

int gs_knn_mean_dist2(gs_ctx *c, const float *points, int64_t n, float *dist2) {
    if (!c) return GS_ERR_INVALID;
    if (n < 0) return fail(c, GS_ERR_INVALID, "gs_knn_mean_dist2: n < 0");
    if (n == 0) return GS_OK;
    if (!points || !dist2) return fail(c, GS_ERR_INVALID, "gs_knn_mean_dist2: NULL array");
    if (n > (int64_t)INT32_MAX) return fail(c, GS_ERR_UNSUPPORTED, "gs_knn_mean_dist2: more than 2^31 - 1 points");
    if (overlaps(range_of(points, 3 * (size_t)n), range_of(dist2, (size_t)n))) return fail(c, GS_ERR_INVALID, "gs_knn_mean_dist2: dist2 overlaps points");
    if (bind_device(c)) return GS_ERR_HIP;
    const size_t nb = (size_t)gs_knn_boxes(n), ns = (size_t)gs_knn_supers(n);
    HIPCHK(c, c->knn_pairs_a.ensure(sizeof(uint64_t) * (size_t)n));
    HIPCHK(c, c->knn_pairs_b.ensure(sizeof(uint64_t) * (size_t)n));
    HIPCHK(c, c->knn_table.ensure(sizeof(uint32_t) * gs_sort_table_entries(n)));
    HIPCHK(c, c->knn_digit_total.ensure(sizeof(uint32_t) * 4 * 256));
    HIPCHK(c, c->knn_sorted.ensure(sizeof(float4) * nb * GS_KNN_BOX));
    HIPCHK(c, c->knn_boxes.ensure(sizeof(float4) * 2 * nb));
    HIPCHK(c, c->knn_supers.ensure(sizeof(float4) * 2 * ns));
    HIPCHK(c, c->knn_stats.ensure(sizeof(uint32_t) * GS_KNN_STAT_WORDS));
    GsKnnArgs a{};
    a.n = n; a.points = points; a.dist2 = dist2;
    a.stats = c->knn_stats.as<uint32_t>();
    a.pairs_a = c->knn_pairs_a.as<uint64_t>(); a.pairs_b = c->knn_pairs_b.as<uint64_t>();
    a.sorted = c->knn_sorted.as<float4>(); a.boxes = c->knn_boxes.as<float4>(); a.supers = c->knn_supers.as<float4>();
    a.table = c->knn_table.as<uint32_t>(); a.digit_total = c->knn_digit_total.as<uint32_t>();
    a.ballot_ranks = c->cfg.rank_mode != 0;
    HIPCHK(c, gs_launch_knn_mean_dist2(a, c->stream));
    return GS_OK;
}

int gs_init_from_points(gs_ctx *c, const float *points, const float *colors, const float *dist2, int64_t n, int sh_degree, float opacity_logit,
                        const gs_grads *dst_model) {
    if (!c) return GS_ERR_INVALID;
    if (n < 0) return fail(c, GS_ERR_INVALID, "gs_init_from_points: n < 0");
    if (sh_degree < 0 || sh_degree > 3) return fail(c, GS_ERR_INVALID, "gs_init_from_points: sh_degree must be 0..3");
    if (!points || !dist2 || !dst_model) return fail(c, GS_ERR_INVALID, "gs_init_from_points: NULL argument");
    const Five<float> dst = five(*dst_model);
    const size_t k3 = 3 * (size_t)(sh_degree + 1) * (size_t)(sh_degree + 1), un = (size_t)n;
    const size_t width[5] = {3, 3, 4, 1, k3};
    ByteRange rd[5];
    const ByteRange rs[3] = {range_of(points, 3 * un), range_of(colors, colors ? 3 * un : 0), range_of(dist2, un)};
    for (int i = 0; i < 5; ++i) {
        if (!dst[i]) return fail(c, GS_ERR_INVALID, "gs_init_from_points: NULL array in dst_model");
        rd[i] = range_of(dst[i], width[i] * un);
    }
    for (int i = 0; i < 5; ++i) {
        for (const ByteRange &s : rs)
            if (overlaps(rd[i], s)) return fail(c, GS_ERR_INVALID, "gs_init_from_points: a destination overlaps a source");
        for (int j = i + 1; j < 5; ++j)
            if (overlaps(rd[i], rd[j])) return fail(c, GS_ERR_INVALID, "gs_init_from_points: destinations overlap");
    }
    if (n == 0) return GS_OK;
    if (bind_device(c)) return GS_ERR_HIP;
    GsInitPointsArgs a{};
    a.n = n; a.k3 = (int)k3; a.points = points; a.colors = colors; a.dist2 = dist2; a.opacity_logit = opacity_logit;
    for (int i = 0; i < 5; ++i) a.dst[i] = dst[i];
    HIPCHK(c, gs_launch_init_from_points(a, c->stream));
    return GS_OK;
}

}  // extern "C"
