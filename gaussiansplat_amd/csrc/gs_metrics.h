// gs_metrics.h -- the statements of the evaluation metrics (gs_image_metrics: PSNR, MAE, standard SSIM) that the kernels of gs_metrics.hip
// execute, written ONCE and usable from host and device: the 11-tap Gaussian window, an 11-tap window sum, the products of a sample pair,
// the SSIM of a pixel from its five window sums, and what gs_metrics_finish makes of the four sums.  tests/metrics_host.cpp is a host build
// of the same text, compared with a float64 torch restatement per pixel (tests/test_metrics_host.py).
//
// Everything is double: the float32 samples are widened, a product of two float32 values is exact in double, and the five window sums, the
// map formula and (x - y) are evaluated in double (a float32 SSIM is off by more than 1e-3 per pixel on nearly flat images,
// where s_xx - mu^2 cancels against C2 = 9e-4).  The window is separable: a pixel's sum is an 11-tap sum over columns of 11-tap sums over rows.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_MT __host__ __device__ inline
#else
#define GS_MT inline
#endif

#define GS_METRIC_WIN 11                  // window taps per axis
#define GS_METRIC_PAD 5                   // zero padding: samples outside the image contribute 0 to all five sums
#define GS_METRIC_PLANES 5                // window sums per pixel: x, y, x^2, y^2, x y
#define GS_METRIC_C1 (0.01 * 0.01)
#define GS_METRIC_C2 (0.03 * 0.03)
#define GS_METRIC_NSUMS 4                 // = GS_METRIC_SUMS of include/gsplat.h: sum w (x - y)^2, sum w |x - y|, sum w S, sum w

// g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), normalised to sum 1 in double (host: the kernels take the eleven values as arguments)
inline void gs_metric_window(double g[GS_METRIC_WIN]) {
    double sum = 0.0;
    for (int i = 0; i < GS_METRIC_WIN; ++i) {
        const double d = (double)(i - GS_METRIC_PAD);
        g[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += g[i];
    }
    for (int i = 0; i < GS_METRIC_WIN; ++i) g[i] /= sum;
}

// the five planes of a sample pair, widened first: the three products are exact
GS_MT void gs_metric_planes(float x, float y, double (&p)[GS_METRIC_PLANES]) {
    const double xd = (double)x, yd = (double)y;
    p[0] = xd; p[1] = yd; p[2] = xd * xd; p[3] = yd * yd; p[4] = xd * yd;
}

// sum_i g[i] v[i * stride], taps in ascending order, one fma per tap
GS_MT double gs_metric_taps(const double *g, const double *v, int stride) {
    double a = 0.0;
    for (int i = 0; i < GS_METRIC_WIN; ++i) a = fma(g[i], v[i * stride], a);
    return a;
}

// S = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_x^2 + s_y^2 + C2)) from the window sums {x, y, x^2, y^2, x y}
GS_MT double gs_ssim_pixel(const double (&m)[GS_METRIC_PLANES]) {
    const double mux = m[0], muy = m[1];
    const double s2x = m[2] - mux * mux, s2y = m[3] - muy * muy, cxy = m[4] - mux * muy;
    const double A1 = 2.0 * mux * muy + GS_METRIC_C1, A2 = 2.0 * cxy + GS_METRIC_C2;
    const double B1 = mux * mux + muy * muy + GS_METRIC_C1, B2 = s2x + s2y + GS_METRIC_C2;
    return (A1 * A2) / (B1 * B2);
}

// the four sums -> {mse, mae, ssim, psnr}: data range 1, psnr = +inf at mse == 0, four NaNs unless sum w > 0
inline void gs_metric_finish(const double sums[GS_METRIC_NSUMS], double out[4]) {
    if (!(sums[3] > 0.0)) { out[0] = out[1] = out[2] = out[3] = (double)NAN; return; }
    out[0] = sums[0] / sums[3]; out[1] = sums[1] / sums[3]; out[2] = sums[2] / sums[3];
    out[3] = out[0] == 0.0 ? (double)INFINITY : -10.0 * log10(out[0]);
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// gs_metrics.hip.  partials: gs_metric_tiles(W, H, C) rows of GS_METRIC_NSUMS doubles, one per workgroup, all of them written by the call;
// sums: GS_METRIC_NSUMS device doubles; weight and ssim_map may be null.  Two launches on s, no atomics, no memset.
int gs_metric_tiles(int W, int H, int C);
hipError_t gs_launch_metrics(const float *img, const float *gt, const float *weight, int W, int H, int C, float *ssim_map, double *partials,
                             double *sums, hipStream_t s);
#endif
