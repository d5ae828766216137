// gs_camera_grad.h -- what ONE gaussian adds to the gradient of a frame's loss with respect to the arguments of gs_set_camera, written
// ONCE: gs_camera_grad_kernel (gs_camera.hip) evaluates it per thread, tests/camera_grad_host.cpp runs it on the CPU against fp64 autograd.
//
// In this forward the gaussian's own R stands in J R (the reference's quirk), so the 2-D covariance does not see the camera rotation: the
// camera is reached through t = T [m; 1] (hence J, p = P t, mu), through fx, fy in J, and through lookAt - eye in the SH direction
// dir = normalize(p[0:3] - (lookAt - eye)).  With dt the complete adjoint of t (the J terms plus P^T dp) and dp the complete adjoint of p
// (the mu terms plus the colour path dpc), the 40 values are, in the order of the view record (GS_VIEW_RECORD_FLOATS) and two more:
//   [0..15]  d_T, column major like T:  d_T[i + 4 j] = dt[i] * mh[j],  mh = (m1, m2, m3, 1)
//   [16..31] d_P:                       d_P[i + 4 j] = dp[i] * t[j]
//   [32..34] d_eye = + dpc              [35..37] d_lookAt = - dpc
//   [38]     d_fx = dJ[0][0] itz - dJ[0][2] tx itz^2          [39] d_fy = dJ[1][1] itz - dJ[1][2] ty itz^2
// the partial derivatives with respect to T, P, eye, lookAt, fx, fy taken as INDEPENDENT inputs (the fourth row of T is zero in the
// reference's cameras; its gradient row is still the formal one).
//
// The whole chain is fp64 from the fp32 inputs, and it is the backward's own text: gs_geom_chain_cov.inc (J .. dJ) and gs_geom_chain_tail.inc
// (J(t), mu(p), p = P t), which gs_geom_bwd_body.inc includes as well.  The colour -> direction path is fp64 here (gs_sh_bwd_kernel has it in
// fp32): the derivative polynomials of the basis are one text too, gs_sh_ddir.inc, included here with double and with the coefficient lists of
// gs_sh.h widened.  The basis VALUES (gs_sh_basis.inc) enter d_shs only and are not needed.  Contraction is off in the body, so the host
// build and the kernel round alike.
//
// The `live` rule of gs_geom_bwd_body.inc: a gaussian whose ten row words are all zero (no pixel touched it, or the forward skipped it) has
// a colour path of zero too; it contributes exactly + 0 in all 40 places and NONE of its model rows is read -- its recomputed chain may be
// Inf or NaN (tz == 0, exp overflow, singular covariance) and must not reach a sum.
#pragma once
#include "gs_pergaussian.h"
#include "gs_sh.h"             // SH_C1, GS_SH_C2_VALUES / GS_SH_C3_VALUES

#define GS_CAMERA_GRAD_VALUES 40          // == GS_CAMERA_GRAD_FLOATS of include/gsplat.h

// The 40 values are outer products of 21 factors.  The statement is written in two halves so that the kernel can reduce the values one after
// another without ever holding 40 of them: gs_camera_grad_factors (the chain) and gs_camera_grad_value (value c from the factors: one
// multiply, a subtraction from zero, or a copy).  gs_camera_grad, what the host program calls, is the two together.
struct GsCameraGradFactors { double dt[4], mh[4], dp[4], t[4], dpc[3], dfx, dfy; };

GS_PG double gs_camera_grad_value(const GsCameraGradFactors &f, int c) {
#pragma clang fp contract(off)
    if (c < 16) return f.dt[c & 3] * f.mh[c >> 2];
    if (c < 32) return f.dp[c & 3] * f.t[(c - 16) >> 2];
    if (c < 35) return f.dpc[c - 32];
    if (c < 38) return 0.0 - f.dpc[c - 35];                              // (0 - x: + 0 where the colour path is + 0, e.g. at degree 0)
    return c == 38 ? f.dfx : f.dfy;
}

// g2f: the ten used words of the row, raw moments, as gs_g2d_row_load returns them; mean, scale, quat, opac, sh: the gaussian's own rows (sh:
// its first 3 (DEG + 1)^2 floats, DEG the ACTIVE degree) -- read only if the row is live
template <int DEG>
GS_PG void gs_camera_grad_factors(const float (&g2f)[10], const float *mean, const float *scale, const float *quat, const float *opac, const float *sh,
                                  const GsCamera &cam, GsCameraGradFactors &f) {
#pragma clang fp contract(off)
    constexpr int K = (DEG + 1) * (DEG + 1);
    bool live = false;
#pragma unroll
    for (int i = 0; i < 10; ++i) live = live || g2f[i] != 0.0f;
    if (!live) {                                                          // every factor + 0: every value + 0 * + 0, + 0 or 0 - 0
        f = GsCameraGradFactors{};
        return;
    }
    const float *T = cam.T, *P = cam.P;
    // ---- forward recompute in fp64: t and p are text in every caller (gs_pergaussian.h says why)
    const double m1 = mean[0], m2 = mean[1], m3 = mean[2];
    double t[4], p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = T[i] * m1 + T[i + 4] * m2 + T[i + 8] * m3 + T[i + 12];
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = P[i] * t[0] + P[i + 4] * t[1] + P[i + 8] * t[2] + P[i + 12] * t[3];
    double g2[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) g2[i] = (double)g2f[i];

    // ---- the colour path: d L / d p[0:3] through dir = normalize(p[0:3] - (lookAt - eye)); cs[k] = d rgb . sh[:, k]
    double dpc[3] = {0.0, 0.0, 0.0};
    if constexpr (DEG >= 1) {
        const double v0 = p[0] - ((double)cam.lookAt[0] - (double)cam.eye[0]);
        const double v1 = p[1] - ((double)cam.lookAt[1] - (double)cam.eye[1]);
        const double v2 = p[2] - ((double)cam.lookAt[2] - (double)cam.eye[2]);
        const double inrm = 1.0 / sqrt(v0 * v0 + v1 * v1 + v2 * v2);
        const double X = v0 * inrm, Y = v1 * inrm, Z = v2 * inrm;
        double cs[K];
#pragma unroll
        for (int k = 0; k < K; ++k) cs[k] = g2[0] * (double)sh[3 * k] + g2[1] * (double)sh[3 * k + 1] + g2[2] * (double)sh[3 * k + 2];
        // the derivative polynomials of gs_sh_bwd_kernel in double: bC2, bC3 are device arrays in gs_sh.h, not usable in a constant expression or
        // on the host -- here the two names are the same literals, widened
        constexpr double bC2[5] = {GS_SH_C2_VALUES}, bC3[7] = {GS_SH_C3_VALUES};
        double ddir[3] = {0.0, 0.0, 0.0};
#define GS_SH_DDIR_T double
#include "gs_sh_ddir.inc"
#undef GS_SH_DDIR_T
        const double dd = X * ddir[0] + Y * ddir[1] + Z * ddir[2];
        dpc[0] = (ddir[0] - X * dd) * inrm; dpc[1] = (ddir[1] - Y * dd) * inrm; dpc[2] = (ddir[2] - Z * dd) * inrm;
    }

    // ---- J, R, Sigma, cov, M, dcov, dA, dJ; then J(t), mu(p), p = P t: the backward's own text
    double dt[4] = {0.0, 0.0, 0.0, 0.0}, dp[4] = {dpc[0], dpc[1], dpc[2], 0.0};
#include "gs_geom_chain_cov.inc"
#include "gs_geom_chain_tail.inc"

    // ---- the factors of the 40 values
#pragma unroll
    for (int i = 0; i < 4; ++i) { f.dt[i] = dt[i]; f.dp[i] = dp[i]; f.t[i] = t[i]; }
    f.mh[0] = m1; f.mh[1] = m2; f.mh[2] = m3; f.mh[3] = 1.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) f.dpc[i] = dpc[i];
    f.dfx = dJ[0][0] * itz - dJ[0][2] * tx * itz2;
    f.dfy = dJ[1][1] * itz - dJ[1][2] * ty * itz2;
}

template <int DEG>
GS_PG void gs_camera_grad(const float (&g2f)[10], const float *mean, const float *scale, const float *quat, const float *opac, const float *sh,
                          const GsCamera &cam, double (&out)[GS_CAMERA_GRAD_VALUES]) {
    GsCameraGradFactors f;
    gs_camera_grad_factors<DEG>(g2f, mean, scale, quat, opac, sh, cam, f);
#pragma unroll
    for (int c = 0; c < GS_CAMERA_GRAD_VALUES; ++c) out[c] = gs_camera_grad_value(f, c);
}

// ---- the two kernels (gs_camera.hip)
struct GsCameraGradArgs {
    int64_t n;
    int sh_degree, sh_stride;             // the ACTIVE degree; floats per stored row of shs
    const float *means, *scales, *quats, *opac, *shs;
    const float *g2d;                     // the frame's rows of 2-D gradient sums (gs_g2d_row_load) ...
    const long long *g2d_fixed;           // ... non-null: the fixed-point ones
    double *partials;                     // gs_camera_grad_rows(n) rows of GS_CAMERA_GRAD_VALUES doubles, one per workgroup
};
inline int64_t gs_camera_grad_rows(int64_t n) { return n > 0 ? (n + 255) / 256 : 0; }
// two launches on s: the partial rows, then out[0 .. 40) = their sums rounded to float once (n == 0: 40 x + 0; out: device memory)
hipError_t gs_launch_camera_grad(const GsCameraGradArgs &a, const GsCamera &cam, float *out, hipStream_t s);
