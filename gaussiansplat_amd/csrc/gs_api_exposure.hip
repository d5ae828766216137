// gs_api_exposure.hip -- gs_exposure_apply / gs_exposure_backward / gs_exposure_adam: the per-view exposure stage between gs_forward and the
// loss (gs_exposure.hip, the statements in gs_exposure.h).  The three calls need no model, camera or frame and work under both renderers, as the
// loss and the metrics do.  Every pointer is a device pointer; the work is enqueued on the ctx stream, no synchronise.  They read their arguments
// and write their outputs and one buffer of their own (gs_ctx::exposure_partials: one row of 12 doubles per workgroup of a backward that wants
// d_exposure): the frame's image, transmittance, gradient sums, stage, view-slot history and stage timers stay what they were.  Every refusal
// is made before anything is enqueued or allocated.
#include "gs_ctx.h"
#include "gs_exposure.h"

namespace {

// the pixel count of a legal image, or 0 with the refusal left for gs_last_error
int64_t exposure_pixels(gs_ctx *c, const char *who, int32_t W, int32_t H) {
    if (W <= 0 || H <= 0) { fail(c, GS_ERR_INVALID, std::string(who) + ": bad image size"); return 0; }
    if (3 * (int64_t)W * H >= ((int64_t)1 << 31)) { fail(c, GS_ERR_INVALID, std::string(who) + ": 3 * H * W must be below 2^31"); return 0; }
    return (int64_t)W * H;
}

}  // namespace

extern "C" {

int gs_exposure_apply(gs_ctx *c, const float *img, const float *exposure, const float *weight, int32_t W, int32_t H, float *out) {
    if (!c) return GS_ERR_INVALID;
    if (!img || !exposure || !out) return fail(c, GS_ERR_INVALID, "gs_exposure_apply: NULL argument");
    const int64_t px = exposure_pixels(c, "gs_exposure_apply", W, H);
    if (!px) return GS_ERR_INVALID;
    const size_t plane = sizeof(float) * (size_t)px;
    const ByteRange o{out, 3 * plane};
    if (overlaps(o, {img, 3 * plane}) || overlaps(o, {weight, plane}) || overlaps(o, {exposure, sizeof(float) * GS_EXPOSURE_FLOATS}))
        return fail(c, GS_ERR_INVALID, "gs_exposure_apply: out overlaps an input");
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, gs_launch_exposure_apply(img, exposure, weight, W, H, out, c->stream));
    return GS_OK;
}

int gs_exposure_backward(gs_ctx *c, const float *img, const float *d_out, const float *exposure, const float *weight, int32_t W, int32_t H,
                         float *d_img, float *d_exposure) {
    if (!c) return GS_ERR_INVALID;
    if (!img || !d_out || !exposure || !d_img) return fail(c, GS_ERR_INVALID, "gs_exposure_backward: NULL argument");
    const int64_t px = exposure_pixels(c, "gs_exposure_backward", W, H);
    if (!px) return GS_ERR_INVALID;
    const size_t plane = sizeof(float) * (size_t)px, row = sizeof(float) * GS_EXPOSURE_FLOATS;
    const ByteRange o{d_img, 3 * plane};
    if (overlaps(o, {img, 3 * plane}) || overlaps(o, {weight, plane}) || overlaps(o, {exposure, row}) || overlaps(o, {d_exposure, row}))
        return fail(c, GS_ERR_INVALID, "gs_exposure_backward: d_img overlaps an input or d_exposure");
    if (d_img != d_out && overlaps(o, {d_out, 3 * plane}))
        return fail(c, GS_ERR_INVALID, "gs_exposure_backward: d_img may be d_out itself, not a part of it");
    if (bind_device(c)) return GS_ERR_HIP;
    double *partials = nullptr;
    if (d_exposure) {
        HIPCHK(c, c->exposure_partials.ensure(sizeof(double) * GS_EXPOSURE_FLOATS * (size_t)gs_exposure_rows(W, H)));
        partials = c->exposure_partials.as<double>();
    }
    HIPCHK(c, gs_launch_exposure_backward(img, d_out, exposure, weight, W, H, d_img, partials, d_exposure, c->stream));
    return GS_OK;
}

int gs_exposure_adam(gs_ctx *c, float *exposure, const float *d_exposure, float *exp_avg, float *exp_avg_sq, float lr, float beta1, float beta2,
                     float eps, int64_t step) {
    if (!c) return GS_ERR_INVALID;
    if (!exposure || !d_exposure || !exp_avg || !exp_avg_sq) return fail(c, GS_ERR_INVALID, "gs_exposure_adam: NULL argument");
    GsAdamHyper h{};
    if (const int rc = gs_adam_scalars(c, "gs_exposure_adam", &lr, 1, beta1, beta2, eps, step, &h)) return rc;
    const size_t row = sizeof(float) * GS_EXPOSURE_FLOATS;
    const ByteRange r[4] = {{exposure, row}, {d_exposure, row}, {exp_avg, row}, {exp_avg_sq, row}};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (overlaps(r[i], r[j])) return fail(c, GS_ERR_INVALID, "gs_exposure_adam: parameter, gradient and moment rows overlap");
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, gs_launch_exposure_adam(exposure, d_exposure, exp_avg, exp_avg_sq, h, c->stream));
    return GS_OK;
}

}  // extern "C"
