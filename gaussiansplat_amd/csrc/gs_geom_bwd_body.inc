// gs_geom_bwd_body.inc -- the geometry chain of gaussian g, as TEXT included into a kernel body inside do { ... } while (0):
// gs_geom_bwd_kernel (d L / d tps through the colour read back from a.dpc) and the fused form of gs_sh_bwd_kernel (handed over in
// registers).  Expects: a (GsPreprocessBwdArgs), cam (GsCamera), g, g2f (float[10], the gaussian's row of 2-D gradients), OVERWRITE,
// and the macro GS_GEOM_DPC (a float4 expression); with GS_GEOM_ADAM defined (gs_sh_bwd_kernel) also ADAM, ad (GsAdamFused), sh (the
// thread's row of SH gradients in the LDS tile), K and srow_live -- ADAM != 0 steps p, m, v with the gradients instead of storing them.
// What the camera gradient computes as well -- J .. dJ, and J(t), mu(p), p = P t -- is not here but in gs_geom_chain_cov.inc and
// gs_geom_chain_tail.inc, which gs_camera_grad.h includes too; this file keeps the touched / live tests, dSg, dR, de, the quaternion and the tails.
// Text, not a function: as a __forceinline__ function the same statements took 186 VGPRs instead of 148 (two waves per SIMD instead of three).  Contraction is off: which products the compiler fuses into fma depends on
// the code around them, and both kernels must produce the same bits (a backward in two steps == a backward in one, tests/test_gpu_multiview.py).
// The eleven gradients stay written twice, for the fused Adam and for the store: formed once into one array with one sink behind it, the
// fused accumulating kernels took 156 .. 160 VGPRs instead of 144 (profiles/HISTORY.md); the two share grad_put, the one store line.
#pragma clang fp contract(off)
    const float *T = cam.T, *P = cam.P;
    if (!OVERWRITE) {   // untouched by the view (see gs_sh_bwd_kernel): a gradient of exactly zero is added to nothing -- the model is not read
        const float4 dpc0 = GS_GEOM_DPC;
        bool touched = dpc0.x != 0.0f || dpc0.y != 0.0f || dpc0.z != 0.0f;
#pragma unroll
        for (int i = 0; i < 10; ++i) touched = touched || g2f[i] != 0.0f;
        if (!touched) break;
    }

    // ---- forward recompute in fp64: R and the sigmoid are the forward's own functions (gs_pergaussian.h); t and p are text (that header says why)
    const double m1 = a.means[3 * g], m2 = a.means[3 * g + 1], m3 = a.means[3 * g + 2];
    double t[4], p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = T[i] * m1 + T[i + 4] * m2 + T[i + 8] * m3 + T[i + 12];
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = P[i] * t[0] + P[i + 4] * t[1] + P[i + 8] * t[2] + P[i + 12] * t[3];
    const float4 dpc = GS_GEOM_DPC;
    // all-zero moments and colour path: the forward skipped this gaussian (payload not finite) or no pixel touched it.
    // Its gradient is exactly zero; the recomputed J, cov, M below may hold Inf/NaN (tz == 0, exp overflow, singular
    // covariance), and 0 * NaN must not reach the parameter gradients.
    bool live = dpc.x != 0.0 || dpc.y != 0.0 || dpc.z != 0.0;
#pragma unroll
    for (int i = 0; i < 10; ++i) live = live || g2f[i] != 0.0;
    double g2[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) g2[i] = (double)g2f[i];
    double dt[4] = {0, 0, 0, 0}, dp[4] = {dpc.x, dpc.y, dpc.z, 0.0};
    const float *quat = a.quats + 4 * g, *scale = a.scales + 3 * g, *opac = a.opac + g;
#include "gs_geom_chain_cov.inc"
    const double gsig = g2[3];
    // ---- dSg = A^T dcov A ;  A = J R: dR = J^T dA
    double dSg[3][3], dR[3][3], dWm[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            dSg[i][j] = A[0][i] * (dcov[0][0] * A[0][j] + dcov[0][1] * A[1][j]) + A[1][i] * (dcov[1][0] * A[0][j] + dcov[1][1] * A[1][j]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) dR[i][j] = J[0][i] * dA[0][j] + J[1][i] * dA[1][j];
    // ---- Sg = Wm Wm^T, Wm = R diag(e)
    double de[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s += (dSg[i][k] + dSg[k][i]) * Wm[k][j];
            dWm[i][j] = s;
            dR[i][j] += s * e[j];
            de[j] += R[i][j] * s;
        }
    // ---- R(q), with the reference's R22
    double dw = 0, dx = 0, dy = 0, dz = 0;
    dy += -4 * y * dR[0][0]; dz += -4 * z * dR[0][0];
    dx += 2 * y * dR[1][0]; dy += 2 * x * dR[1][0]; dw += 2 * z * dR[1][0]; dz += 2 * w * dR[1][0];
    dx += 2 * z * dR[2][0]; dz += 2 * x * dR[2][0]; dw += -2 * y * dR[2][0]; dy += -2 * w * dR[2][0];
    dx += 2 * y * dR[0][1]; dy += 2 * x * dR[0][1]; dw += -2 * z * dR[0][1]; dz += -2 * w * dR[0][1];
    dx += -4 * x * dR[1][1]; dz += 4 * z * dR[1][1];
    dy += 2 * z * dR[2][1]; dz += 2 * y * dR[2][1]; dw += 2 * x * dR[2][1]; dx += 2 * w * dR[2][1];
    dx += 2 * z * dR[0][2]; dz += 2 * x * dR[0][2]; dw += 2 * y * dR[0][2]; dy += 2 * w * dR[0][2];
    dy += 2 * z * dR[1][2]; dz += 2 * y * dR[1][2]; dw += -2 * x * dR[1][2]; dx += -2 * w * dR[1][2];
    dx += -4 * x * dR[2][2]; dy += -4 * y * dR[2][2];
    // ---- J(t), mu(p), p = P t;  t = T [m; 1] follows where the mean's gradient is formed
#include "gs_geom_chain_tail.inc"
#ifdef GS_GEOM_ADAM
    if constexpr (ADAM != 0) {
        // the eleven gradients exactly as the OVERWRITE instantiation below stores them (its quaternion row is 0 + v, added to zeros)
        float gq[11];
#pragma unroll
        for (int j = 0; j < 3; ++j) gq[j] = live ? (float)(T[4 * j] * dt[0] + T[1 + 4 * j] * dt[1] + T[2 + 4 * j] * dt[2] + T[3 + 4 * j] * dt[3]) : 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) gq[3 + j] = live ? (float)(de[j] * e[j]) : 0.0f;
        gq[6] = live ? add_exact(0.0f, (float)dw) : 0.0f; gq[7] = live ? add_exact(0.0f, (float)dx) : 0.0f;
        gq[8] = live ? add_exact(0.0f, (float)dy) : 0.0f; gq[9] = live ? add_exact(0.0f, (float)dz) : 0.0f;
        gq[10] = live ? (float)(gsig * sg * (1.0 - sg)) : 0.0f;
        bool stepped = true;
        if (ADAM == 2) {   // selective: live if any of the 11 + 3K gradient floats != 0 (the SH ones are this thread's row of the LDS tile)
            bool any = false;
#pragma unroll
            for (int i = 0; i < 11; ++i) any = any || gq[i] != 0.0f;
#pragma unroll
            for (int i = 0; i < 3 * K; ++i) any = any || sh[i] != 0.0f;
            srow_live[threadIdx.x] = any ? 1 : 0;
            stepped = any;
        }
        if (stepped) {
            float *pp[4] = {const_cast<float *>(a.means) + 3 * g, const_cast<float *>(a.scales) + 3 * g, const_cast<float *>(a.quats) + 4 * g,
                            const_cast<float *>(a.opac) + g};
            float *mp[4] = {ad.m[0] + 3 * g, ad.m[1] + 3 * g, ad.m[2] + 4 * g, ad.m[3] + g};
            float *vp[4] = {ad.v[0] + 3 * g, ad.v[1] + 3 * g, ad.v[2] + 4 * g, ad.v[3] + g};
            constexpr int first[5] = {0, 3, 6, 10, 11};
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < first[q + 1] - first[q]; ++j) {
                    float pv = pp[q][j], mv = mp[q][j], vv = vp[q][j];
                    gs_adam_update(pv, mv, vv, gq[first[q] + j], ad.h, ad.h.step_size[q]);
                    pp[q][j] = pv; mp[q][j] = mv; vp[q][j] = vv;
                }
        }
    } else
#endif
    {
    if (a.d_means) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float v = live ? (float)(T[4 * j] * dt[0] + T[1 + 4 * j] * dt[1] + T[2 + 4 * j] * dt[2] + T[3 + 4 * j] * dt[3]) : 0.0f;
            grad_put<OVERWRITE>(&a.d_means[3 * g + j], v, a.sgd_scale);
        }
    }
    if (a.d_scales) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float v = live ? (float)(de[j] * e[j]) : 0.0f;
            grad_put<OVERWRITE>(&a.d_scales[3 * g + j], v, a.sgd_scale);
        }
    }
    if (a.d_quats) {
        float4 *q = reinterpret_cast<float4 *>(a.d_quats) + g;
        float4 o = OVERWRITE ? make_float4(0.f, 0.f, 0.f, 0.f) : *q;
        if (live) { o.x = acc_or_step(o.x, (float)dw, a.sgd_scale); o.y = acc_or_step(o.y, (float)dx, a.sgd_scale); o.z = acc_or_step(o.z, (float)dy, a.sgd_scale); o.w = acc_or_step(o.w, (float)dz, a.sgd_scale); }
        *q = o;
    }
    if (a.d_opac) {
        const float v = live ? (float)(gsig * sg * (1.0 - sg)) : 0.0f;
        grad_put<OVERWRITE>(&a.d_opac[g], v, a.sgd_scale);
    }
    }
