// gs_api_bilagrid.hip -- gs_bilagrid_apply / gs_bilagrid_backward / gs_bilagrid_tv / gs_bilagrid_adam: the per-view bilateral grid between
// gs_forward and the loss (gs_bilagrid.hip, the statements in gs_bilagrid.h).  The four calls need no model, camera or frame and work under
// both renderers, as the exposure stage does.  Every pointer is a device pointer; the work is enqueued on the ctx stream, no synchronise.  They
// read their arguments and write their outputs and nothing else -- the ctx holds no buffer of theirs: the frame's image, transmittance,
// gradient sums, stage, view-slot history and stage timers stay what they were.  Every refusal is made before anything is enqueued.
#include "gs_ctx.h"
#include "gs_bilagrid.h"

#include <cmath>

namespace {

// the pixel count of a legal image and the float count of a legal grid, or 0 with the refusal left for gs_last_error
int64_t bilagrid_pixels(gs_ctx *c, const char *who, int32_t W, int32_t H) {
    if (W <= 0 || H <= 0) { fail(c, GS_ERR_INVALID, std::string(who) + ": bad image size"); return 0; }
    if (3 * (int64_t)W * H >= ((int64_t)1 << 31)) { fail(c, GS_ERR_INVALID, std::string(who) + ": 3 * H * W must be below 2^31"); return 0; }
    return (int64_t)W * H;
}
int64_t bilagrid_floats(gs_ctx *c, const char *who, int32_t Gx, int32_t Gy, int32_t Gz) {
    for (const int32_t n : {Gx, Gy, Gz})
        if (n < 1 || n > GS_BILAGRID_MAX_DIM) { fail(c, GS_ERR_INVALID, std::string(who) + ": every grid dimension must be in 1..64"); return 0; }
    return (int64_t)Gx * Gy * Gz * GS_BILAGRID_FLOATS;
}

}  // namespace

extern "C" {

int gs_bilagrid_apply(gs_ctx *c, const float *img, const float *grid, int32_t Gx, int32_t Gy, int32_t Gz, const float *weight, int32_t W, int32_t H,
                      float *out) {
    if (!c) return GS_ERR_INVALID;
    if (!img || !grid || !out) return fail(c, GS_ERR_INVALID, "gs_bilagrid_apply: NULL argument");
    const int64_t px = bilagrid_pixels(c, "gs_bilagrid_apply", W, H), nf = px ? bilagrid_floats(c, "gs_bilagrid_apply", Gx, Gy, Gz) : 0;
    if (!nf) return GS_ERR_INVALID;
    const size_t plane = sizeof(float) * (size_t)px;
    const ByteRange o{out, 3 * plane};
    if (overlaps(o, {img, 3 * plane}) || overlaps(o, {weight, plane}) || overlaps(o, {grid, sizeof(float) * (size_t)nf}))
        return fail(c, GS_ERR_INVALID, "gs_bilagrid_apply: out overlaps an input");
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, gs_launch_bilagrid_apply(img, grid, Gx, Gy, Gz, weight, W, H, out, c->stream));
    return GS_OK;
}

int gs_bilagrid_backward(gs_ctx *c, const float *img, const float *d_out, const float *grid, int32_t Gx, int32_t Gy, int32_t Gz, const float *weight,
                         int32_t W, int32_t H, float *d_img, float *d_grid) {
    if (!c) return GS_ERR_INVALID;
    if (!img || !d_out || !grid || !d_img) return fail(c, GS_ERR_INVALID, "gs_bilagrid_backward: NULL argument");
    const int64_t px = bilagrid_pixels(c, "gs_bilagrid_backward", W, H), nf = px ? bilagrid_floats(c, "gs_bilagrid_backward", Gx, Gy, Gz) : 0;
    if (!nf) return GS_ERR_INVALID;
    const size_t plane = sizeof(float) * (size_t)px, gbytes = sizeof(float) * (size_t)nf;
    const ByteRange o{d_img, 3 * plane}, dg{d_grid, gbytes};
    if (overlaps(o, {img, 3 * plane}) || overlaps(o, {weight, plane}) || overlaps(o, {grid, gbytes}) || overlaps(o, dg))
        return fail(c, GS_ERR_INVALID, "gs_bilagrid_backward: d_img overlaps an input or d_grid");
    if (d_img != d_out && overlaps(o, {d_out, 3 * plane}))
        return fail(c, GS_ERR_INVALID, "gs_bilagrid_backward: d_img may be d_out itself, not a part of it");
    if (overlaps(dg, {img, 3 * plane}) || overlaps(dg, {d_out, 3 * plane}) || overlaps(dg, {weight, plane}) || overlaps(dg, {grid, gbytes}))
        return fail(c, GS_ERR_INVALID, "gs_bilagrid_backward: d_grid overlaps an input");
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, gs_launch_bilagrid_backward(img, d_out, grid, Gx, Gy, Gz, weight, W, H, d_img, d_grid, c->stream));
    return GS_OK;
}

int gs_bilagrid_tv(gs_ctx *c, const float *grid, int32_t Gx, int32_t Gy, int32_t Gz, float coef, float *d_grid, double *tv_out) {
    if (!c) return GS_ERR_INVALID;
    if (!grid) return fail(c, GS_ERR_INVALID, "gs_bilagrid_tv: NULL argument");
    const int64_t nf = bilagrid_floats(c, "gs_bilagrid_tv", Gx, Gy, Gz);
    if (!nf) return GS_ERR_INVALID;
    if (!(coef >= 0.0f) || !std::isfinite(coef)) return fail(c, GS_ERR_INVALID, "gs_bilagrid_tv: coef must be finite and >= 0");
    const size_t gbytes = sizeof(float) * (size_t)nf;
    const ByteRange g{grid, gbytes}, dg{d_grid, gbytes}, tv{tv_out, sizeof(double)};
    if (overlaps(g, dg) || overlaps(g, tv) || overlaps(dg, tv)) return fail(c, GS_ERR_INVALID, "gs_bilagrid_tv: grid, d_grid and tv_out overlap");
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, gs_launch_bilagrid_tv(grid, Gx, Gy, Gz, coef, d_grid, tv_out, c->stream));
    return GS_OK;
}

int gs_bilagrid_adam(gs_ctx *c, float *grid, const float *d_grid, float *exp_avg, float *exp_avg_sq, int64_t n_floats, float lr, float beta1, float beta2,
                     float eps, int64_t step) {
    if (!c) return GS_ERR_INVALID;
    if (!grid || !d_grid || !exp_avg || !exp_avg_sq) return fail(c, GS_ERR_INVALID, "gs_bilagrid_adam: NULL argument");
    const int64_t most = (int64_t)GS_BILAGRID_MAX_DIM * GS_BILAGRID_MAX_DIM * GS_BILAGRID_MAX_DIM * GS_BILAGRID_FLOATS;
    if (n_floats < 1 || n_floats > most) return fail(c, GS_ERR_INVALID, "gs_bilagrid_adam: n_floats must be in 1..64^3 * 12");
    GsAdamHyper h{};
    if (const int rc = gs_adam_scalars(c, "gs_bilagrid_adam", &lr, 1, beta1, beta2, eps, step, &h)) return rc;
    const size_t bytes = sizeof(float) * (size_t)n_floats;
    const ByteRange r[4] = {{grid, bytes}, {d_grid, bytes}, {exp_avg, bytes}, {exp_avg_sq, bytes}};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (overlaps(r[i], r[j])) return fail(c, GS_ERR_INVALID, "gs_bilagrid_adam: parameter, gradient and moment arrays overlap");
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, gs_launch_bilagrid_adam(grid, d_grid, exp_avg, exp_avg_sq, (long long)n_floats, h, c->stream));
    return GS_OK;
}

}  // extern "C"
