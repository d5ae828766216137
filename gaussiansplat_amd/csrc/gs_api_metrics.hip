// gs_api_metrics.hip -- gs_image_metrics / gs_metrics_finish: the evaluation metrics of two images (PSNR, MAE, standard SSIM; gs_metrics.hip,
// the statements in gs_metrics.h).  gs_image_metrics needs no model, camera or frame and works under both renderers, as the loss does.  It reads its
// arguments and writes `sums`, `ssim_map` and buffers of its own (gs_ctx::metrics_partials: 256 bytes for the staged sums of a GS_MEM_HOST call,
// then one row of four doubles per tile; metrics_in / metrics_map: the staged images, weight and map of a GS_MEM_HOST call): the frame's image,
// transmittance, gradient sums, stage, view-slot history and stage timers stay what they were.  Every refusal is made before anything is enqueued
// or allocated.  gs_metrics_finish is pure host arithmetic.
#include "gs_ctx.h"
#include "gs_metrics.h"

static_assert(GS_METRIC_SUMS == GS_METRIC_NSUMS, "the ABI's four sums are the statement's");
#define GS_METRIC_HEAD_BYTES 256          // the staged sums in front of the partial rows

extern "C" {

int gs_image_metrics(gs_ctx *c, const float *img, const float *gt, const float *weight, int32_t W, int32_t H, int32_t C, float *ssim_map,
                     double *sums, int mem) {
    if (!c) return GS_ERR_INVALID;
    if (!img || !gt || !sums) return fail(c, GS_ERR_INVALID, "gs_image_metrics: NULL argument");
    if (W <= 0 || H <= 0 || C <= 0) return fail(c, GS_ERR_INVALID, "gs_image_metrics: bad image size");
    if ((int64_t)W * H * C >= ((int64_t)1 << 31)) return fail(c, GS_ERR_INVALID, "gs_image_metrics: C * H * W must be below 2^31");
    if (const int rc = need_mem(c, "gs_image_metrics", mem)) return rc;
    if (bind_device(c)) return GS_ERR_HIP;
    const size_t px = (size_t)W * H, n = px * (size_t)C;
    const int tiles = gs_metric_tiles(W, H, C);
    HIPCHK(c, c->metrics_partials.ensure(GS_METRIC_HEAD_BYTES + sizeof(double) * GS_METRIC_NSUMS * (size_t)tiles));
    double *d_sums = sums, *partials = reinterpret_cast<double *>(c->metrics_partials.as<char>() + GS_METRIC_HEAD_BYTES);
    const float *d_img = img, *d_gt = gt, *d_w = weight;
    float *d_map = ssim_map;
    if (mem == GS_MEM_HOST) {
        const float *src[3] = {img, gt, weight};
        const size_t bytes[3] = {sizeof(float) * n, sizeof(float) * n, sizeof(float) * px};
        const float **dst[3] = {&d_img, &d_gt, &d_w};
        for (int i = 0; i < 3; ++i) {
            if (!src[i]) continue;
            HIPCHK(c, c->metrics_in[i].ensure(bytes[i]));
            HIPCHK(c, hipMemcpyAsync(c->metrics_in[i].p, src[i], bytes[i], hipMemcpyHostToDevice, c->stream));
            *dst[i] = c->metrics_in[i].as<float>();
        }
        if (ssim_map) { HIPCHK(c, c->metrics_map.ensure(sizeof(float) * n)); d_map = c->metrics_map.as<float>(); }
        d_sums = c->metrics_partials.as<double>();
    }
    HIPCHK(c, gs_launch_metrics(d_img, d_gt, d_w, W, H, C, d_map, partials, d_sums, c->stream));
    if (mem == GS_MEM_HOST) {
        if (ssim_map) HIPCHK(c, hipMemcpyAsync(ssim_map, d_map, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(sums, d_sums, sizeof(double) * GS_METRIC_NSUMS, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return GS_OK;
}

int gs_metrics_finish(const double sums[GS_METRIC_SUMS], double out[GS_METRIC_COUNT]) {
    if (!sums || !out) return GS_ERR_INVALID;
    gs_metric_finish(sums, out);
    return GS_OK;
}

}  // extern "C"
