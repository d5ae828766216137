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
// The whole chain is fp64 from the fp32 inputs, as gs_geom_bwd_body.inc has it: the same forward recompute, gs_quat_to_rot,
// gs_sigmoid_logit<double>, gs_g2d_to_grads<double>.  The colour -> direction path is fp64 here as well (gs_sh_bwd_kernel has it in fp32):
// the derivative polynomials of the basis as they stand there, on the constants of gs_sh.h widened to double.  The basis VALUES
// (gs_sh_basis.inc) enter d_shs only and are not needed.  Contraction is off in the body, so the host build and the kernel round alike.
//
// The `live` rule of gs_geom_bwd_body.inc: a gaussian whose ten row words are all zero (no pixel touched it, or the forward skipped it) has
// a colour path of zero too; it contributes exactly + 0 in all 40 places and NONE of its model rows is read -- its recomputed chain may be
// Inf or NaN (tz == 0, exp overflow, singular covariance) and must not reach a sum.
#pragma once
#include "gs_pergaussian.h"
#include "gs_sh.h"             // SH_C1; the values of bC2 / bC3

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
    // ---- forward recompute in fp64 (gs_geom_bwd_body.inc)
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
        // the constants of gs_sh.h (bC2, bC3 are device arrays there, not usable in a constant expression: the same float literals, widened;
        // tests/test_camera_grad_host.py compares the two texts)
        constexpr double C1 = (double)SH_C1;
        constexpr double c2[5] = {(double)1.0925484305920792f, (double)-1.0925484305920792f, (double)0.31539156525252005f,
                                  (double)-1.0925484305920792f, (double)0.5462742152960396f};
        constexpr double c3[7] = {(double)-0.5900435899266435f, (double)2.890611442640554f, (double)-0.4570457994644658f, (double)0.3731763325901154f,
                                  (double)-0.4570457994644658f, (double)1.445305721320277f, (double)-0.5900435899266435f};
        double ddir[3] = {0.0, 0.0, 0.0};
        ddir[0] += -C1 * cs[3]; ddir[1] += -C1 * cs[1]; ddir[2] += C1 * cs[2];
        if constexpr (DEG >= 2) {
            ddir[0] += c2[0] * Y * cs[4] - 2 * c2[2] * X * cs[6] + c2[3] * Z * cs[7] + 2 * c2[4] * X * cs[8];
            ddir[1] += c2[0] * X * cs[4] + c2[1] * Z * cs[5] - 2 * c2[2] * Y * cs[6] - 2 * c2[4] * Y * cs[8];
            ddir[2] += c2[1] * Y * cs[5] + 4 * c2[2] * Z * cs[6] + c2[3] * X * cs[7];
        }
        if constexpr (DEG >= 3) {
            const double xx = X * X, yy = Y * Y, zz = Z * Z, xy = X * Y, yz = Y * Z, xz = X * Z;
            ddir[0] += 6 * c3[0] * xy * cs[9] + c3[1] * yz * cs[10] - 2 * c3[2] * xy * cs[11] - 6 * c3[3] * xz * cs[12]
                       + c3[4] * (4 * zz - 3 * xx - yy) * cs[13] + 2 * c3[5] * xz * cs[14] + c3[6] * (3 * xx - 3 * yy) * cs[15];
            ddir[1] += c3[0] * (3 * xx - 3 * yy) * cs[9] + c3[1] * xz * cs[10] + c3[2] * (4 * zz - xx - 3 * yy) * cs[11]
                       - 6 * c3[3] * yz * cs[12] - 2 * c3[4] * xy * cs[13] - 2 * c3[5] * yz * cs[14] - 6 * c3[6] * xy * cs[15];
            ddir[2] += c3[1] * xy * cs[10] + 8 * c3[2] * yz * cs[11] + c3[3] * (6 * zz - 3 * xx - 3 * yy) * cs[12]
                       + 8 * c3[4] * xz * cs[13] + c3[5] * (xx - yy) * cs[14];
        }
        const double dd = X * ddir[0] + Y * ddir[1] + Z * ddir[2];
        dpc[0] = (ddir[0] - X * dd) * inrm; dpc[1] = (ddir[1] - Y * dd) * inrm; dpc[2] = (ddir[2] - Z * dd) * inrm;
    }

    // ---- J, R, Sigma, cov, M (gs_geom_bwd_body.inc, statement for statement)
    double dp[4] = {dpc[0], dpc[1], dpc[2], 0.0};
    const double tx = t[0], ty = t[1], tz = t[2], fx = cam.fx, fy = cam.fy;
    const double itz = 1.0 / tz, itz2 = itz * itz;
    const double J[2][3] = {{fx * itz, 0.0, -fx * tx * itz2}, {0.0, fy * itz, -fy * ty * itz2}};
    double R[3][3];
    gs_quat_to_rot((double)quat[0], (double)quat[1], (double)quat[2], (double)quat[3], R);
    const double e[3] = {exp((double)scale[0]), exp((double)scale[1]), exp((double)scale[2])};
    double Wm[3][3], Sg[3][3], A[2][3], ASg[2][3], cov[2][2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Wm[i][j] = R[i][j] * e[j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Sg[i][j] = Wm[i][0] * Wm[j][0] + Wm[i][1] * Wm[j][1] + Wm[i][2] * Wm[j][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A[i][j] = J[i][0] * R[0][j] + J[i][1] * R[1][j] + J[i][2] * R[2][j];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) ASg[i][j] = A[i][0] * Sg[0][j] + A[i][1] * Sg[1][j] + A[i][2] * Sg[2][j];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) cov[i][j] = ASg[i][0] * A[j][0] + ASg[i][1] * A[j][1] + ASg[i][2] * A[j][2] + 0.3;
    const double idet = 1.0 / (cov[0][0] * cov[1][1] - cov[0][1] * cov[1][0]);
    const double M[2][2] = {{cov[1][1] * idet, -cov[0][1] * idet}, {-cov[1][0] * idet, cov[0][0] * idet}};
    const double sg = gs_sigmoid_logit<double>(opac[0]);
    gs_g2d_to_grads(g2, sg, M[0][0], 0.5 * (M[0][1] + M[1][0]), M[1][1]);
    const double gmx = g2[4], gmy = g2[5];
    const double G[2][2] = {{g2[6], g2[7]}, {g2[8], g2[9]}};           // G[r][c] = dL/dM[r][c]
    // ---- M = cov^-1  =>  dcov = -M^T G M^T ;  cov = A Sg A^T (+0.3): dA = (dcov + dcov^T) A Sg ;  A = J R: dJ = dA R^T
    double t1[2][2], dcov[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) t1[i][j] = M[0][i] * G[0][j] + M[1][i] * G[1][j];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) dcov[i][j] = -(t1[i][0] * M[j][0] + t1[i][1] * M[j][1]);
    const double off = dcov[0][1] + dcov[1][0];
    const double ds2[2][2] = {{2 * dcov[0][0], off}, {off, 2 * dcov[1][1]}};
    double dA[2][3], dJ[2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) dA[i][j] = ds2[i][0] * ASg[0][j] + ds2[i][1] * ASg[1][j];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) dJ[i][j] = dA[i][0] * R[j][0] + dA[i][1] * R[j][1] + dA[i][2] * R[j][2];
    // ---- J(t)
    double dt[4] = {0.0, 0.0, 0.0, 0.0};
    const double itz3 = itz2 * itz;
    dt[0] += dJ[0][2] * (-fx * itz2);
    dt[1] += dJ[1][2] * (-fy * itz2);
    dt[2] += dJ[0][0] * (-fx * itz2) + dJ[1][1] * (-fy * itz2) + dJ[0][2] * (2 * fx * tx * itz3) + dJ[1][2] * (2 * fy * ty * itz3);
    // ---- mu(p): mu = (W p0/p3 + 1)/2 + W/2
    const double ip3 = 1.0 / p[3];
    const double Wd = (double)cam.W, Hd = (double)cam.H;
    dp[0] += gmx * 0.5 * Wd * ip3;
    dp[1] += gmy * 0.5 * Hd * ip3;
    dp[3] += -(gmx * 0.5 * Wd * p[0] + gmy * 0.5 * Hd * p[1]) * ip3 * ip3;
    // ---- p = P t
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) dt[j] += P[i + 4 * j] * dp[i];

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
