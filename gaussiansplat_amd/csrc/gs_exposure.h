// gs_exposure.h -- the statements of the per-view exposure stage (gs_exposure_apply / gs_exposure_backward: a learned 3 x 4 colour affine
// and an optional per-pixel weight between the frame and the loss), written ONCE and usable from host and device: the kernels of
// gs_exposure.hip execute them per pixel, tests/exposure_host.cpp is a host build of the same text that tests/test_exposure_host.py compares
// bit for bit with the NumPy restatement of tests/exposure_ref.py.
//
// Layout: images are planar [3][H][W] float32; E is 12 floats, row-major 3 x 4: E[4 r + 0..2] the matrix row r, E[4 r + 3] its offset; the
// weight is one float per pixel, or absent.  Contraction is off in every body: one fp32 rounding per operation, in the order written.
//   forward   a_r = ((E[r][0] x0 + E[r][1] x1) + E[r][2] x2) + E[r][3];   out_r = w a_r   (no weight: out_r = a_r)
//   into x    g_r = w d_r   (no weight: g_r = d_r);   dx_k = (E[0][k] g0 + E[1][k] g1) + E[2][k] g2
//   into E    t[r][k] = (double)g_r * (double)x_k, x_3 = 1: a product of two floats is exact in double; dE[r][k] is the sum of t[r][k] over the
//             pixels in double, rounded to float once (the sum's order is the kernels': gs_exposure.hip)
// Identity E without a weight returns x for every finite x (x + 0 + 0 + 0: the bits are equal but for -0, which becomes +0); identity E
// with a weight returns w * x exactly (w * (x + 0 + 0 + 0)), so a masked target needs no kernel of its own.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_EXP __host__ __device__ inline
#else
#define GS_EXP inline
#endif

#define GS_EXPOSURE_FLOATS 12             // a row of the table: 3 x 4, row-major
#define GS_EXPOSURE_QUAD 4                // consecutive pixels a lane takes (one 16-byte access per plane)
#define GS_EXPOSURE_BLOCK 256             // lanes of a workgroup: GS_EXPOSURE_BLOCK * GS_EXPOSURE_QUAD pixels, one row of partial sums

// the affine of one pixel, before the weight
GS_EXP void gs_exposure_affine(const float *E, const float (&x)[3], float (&a)[3]) {
#pragma clang fp contract(off)
    for (int r = 0; r < 3; ++r) a[r] = ((E[4 * r] * x[0] + E[4 * r + 1] * x[1]) + E[4 * r + 2] * x[2]) + E[4 * r + 3];
}
GS_EXP void gs_exposure_forward(const float *E, const float (&x)[3], float (&out)[3]) { gs_exposure_affine(E, x, out); }
GS_EXP void gs_exposure_forward(const float *E, const float (&x)[3], float w, float (&out)[3]) {
#pragma clang fp contract(off)
    float a[3];
    gs_exposure_affine(E, x, a);
    for (int r = 0; r < 3; ++r) out[r] = w * a[r];
}

// g = w d: what both adjoints start from
GS_EXP void gs_exposure_weigh(const float (&d)[3], float w, float (&g)[3]) {
#pragma clang fp contract(off)
    for (int r = 0; r < 3; ++r) g[r] = w * d[r];
}
// the adjoint into the image from g (the transposed 3 x 3 product)
GS_EXP void gs_exposure_dx(const float *E, const float (&g)[3], float (&dx)[3]) {
#pragma clang fp contract(off)
    for (int k = 0; k < 3; ++k) dx[k] = (E[k] * g[0] + E[4 + k] * g[1]) + E[8 + k] * g[2];
}
// the twelve terms of one pixel of the adjoint into E, added to acc (row-major like E): exact products, one double addition each
GS_EXP void gs_exposure_dE_add(const float (&g)[3], const float (&x)[3], double (&acc)[GS_EXPOSURE_FLOATS]) {
#pragma clang fp contract(off)
    for (int r = 0; r < 3; ++r) {
        const double gr = (double)g[r];
        for (int k = 0; k < 3; ++k) acc[4 * r + k] = acc[4 * r + k] + gr * (double)x[k];
        acc[4 * r + 3] = acc[4 * r + 3] + gr;
    }
}

// rows of partial sums of a backward that wants dE = workgroups of every launch: a function of (W, H) alone
GS_EXP int gs_exposure_rows(int W, int H) {
    const long long px = (long long)W * H, per = (long long)GS_EXPOSURE_BLOCK * GS_EXPOSURE_QUAD;
    return (int)((px + per - 1) / per);
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "gs_adam.h"
// gs_exposure.hip.  Every pointer is a device pointer; weight may be null.  No atomics, no memset.
// apply: one launch.  backward: d_exposure null -- one launch, no double arithmetic; else two: every one of the gs_exposure_rows(W, H) rows
// of 12 doubles in `partials` is written by the first and summed in a fixed order by the second.  d_img == d_out exactly is legal.
hipError_t gs_launch_exposure_apply(const float *img, const float *E, const float *weight, int W, int H, float *out, hipStream_t s);
hipError_t gs_launch_exposure_backward(const float *img, const float *d_out, const float *E, const float *weight, int W, int H, float *d_img,
                                       double *partials, float *d_exposure, hipStream_t s);
// one Adam step of the 12 floats of a row (gs_adam_update with h.step_size[0]); one wave, one launch
hipError_t gs_launch_exposure_adam(float *E, const float *dE, float *m, float *v, const GsAdamHyper &h, hipStream_t s);
#endif
