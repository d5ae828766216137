// gs_api_touched.hip -- the touched-rows colour exchange below the C ABI: gs_color_rows_pack (one view -> bitmap, compacted rows,
// count) and gs_sh_grads_from_touched (all gathered views -> d_shs).  The kernels are in gs_touched.hip; the per-chunk counts and
// offsets they pass to each other live in grow-only ctx scratch (touched_cnt, touched_off).  Neither call synchronises.
#include "gs_chunk.h"
#include "gs_ctx.h"

static int touched_scratch(gs_ctx *c, int64_t views, int64_t n) {
    const size_t chunks = (size_t)views * (size_t)gs_chunks(n);
    HIPCHK(c, c->touched_cnt.ensure(sizeof(uint32_t) * chunks));
    HIPCHK(c, c->touched_off.ensure(sizeof(int64_t) * chunks));
    return GS_OK;
}

extern "C" {

int gs_color_rows_pack(gs_ctx *c, const float *drgb, int64_t n, int32_t *bits, float *rows, int64_t *count) {
    if (!c || !bits || !rows || !count || n < 0) return GS_ERR_INVALID;
    int rc = need_3d(c, "gs_color_rows_pack");
    if (rc || (!drgb && (rc = need_stage(c, gs_ctx::Stage::COMPOSITE_ADJOINT, "gs_color_rows_pack: gs_backward first (or pass drgb)")))) return rc;
    if (!drgb && n != c->n) return fail(c, GS_ERR_INVALID, "gs_color_rows_pack: n must be gs_num_gaussians when the ctx's own sums are packed");
    if (bind_device(c)) return GS_ERR_HIP;
    if (n == 0) {
        HIPCHK(c, hipMemsetAsync(count, 0, sizeof(int64_t), c->stream));
        return GS_OK;
    }
    if ((rc = touched_scratch(c, 1, n))) return rc;
    const gs_ctx::Rows own = drgb ? gs_ctx::Rows{nullptr, nullptr} : c->rows(c->g2d);    // the ctx's own sums, unless the caller brings dense ones
    HIPCHK(c, gs_launch_touched_pack(drgb, own.g2d, own.g2d_fixed, n, bits, rows, count, c->touched_cnt.as<uint32_t>(), c->touched_off.as<int64_t>(), c->stream));
    return GS_OK;
}

int gs_sh_grads_from_touched(gs_ctx *c, int32_t nviews, const float *cams, const int32_t *bits, const float *rows, int64_t rows_cap,
                             float *d_shs, int flags) {
    if (!c || !cams || !bits || !rows || !d_shs || nviews <= 0 || rows_cap < 1) return GS_ERR_INVALID;
    if (const int rc = need_3d(c, "gs_sh_grads_from_touched")) return rc;
    if (bind_device(c)) return GS_ERR_HIP;
    if (c->n <= 0) return GS_OK;
    const size_t bytes = sizeof(float) * GS_VIEW_RECORD_FLOATS * (size_t)nviews;
    HIPCHK(c, c->view_cams.ensure(bytes));
    if (const int rc = touched_scratch(c, nviews, c->n)) return rc;
    if (!c->touched_zero.p) {                                            // the row an untouched (view, gaussian) is loaded from: zeroed once, before any kernel reads it
        HIPCHK(c, c->touched_zero.ensure(4 * sizeof(float)));
        HIPCHK(c, hipMemset(c->touched_zero.p, 0, c->touched_zero.cap));
    }
    HIPCHK(c, hipMemcpyAsync(c->view_cams.p, cams, bytes, hipMemcpyHostToDevice, c->stream));   // pageable source: staged before return
    HIPCHK(c, gs_launch_sh_from_touched(c->n, c->active_sh_degree(), c->sh_row_floats(), c->means, nviews, c->view_cams.as<float>(), bits, rows, rows_cap,
                                        c->touched_cnt.as<uint32_t>(), c->touched_off.as<int64_t>(), c->touched_zero.as<float>(), d_shs,
                                        (flags & GS_BWD_OVERWRITE) ? 1 : 0, c->stream));
    return GS_OK;
}

}  // extern "C"
