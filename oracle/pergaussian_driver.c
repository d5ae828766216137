/*
 * pergaussian_driver.c -- stand-alone driver of the per-gaussian reference functions (gso_forward64, gso_composite_rows,
 * gso_composite_rows_f32, gso_chain, gso_sh_path, gso_sh_path_f32) on a tiny built-in scene, for the host sanitizers: `make -C oracle sanitize-pergaussian`
 * compiles it together with gs_oracle.c under AddressSanitizer + UndefinedBehaviorSanitizer and runs it.  It also checks what
 * must hold whatever the scene: every output finite, untouched gaussians all zero, the fp32 twin inside the mass.
 */
#include "gs_oracle.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

static uint32_t lcg_state = 12345u;
static float urand(float lo, float hi) {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return lo + (hi - lo) * (float)(lcg_state >> 8) * (1.0f / 16777216.0f);
}

int main(void) {
    enum { N = 96, W = 40, H = 27, DEG = 2, K = 9, TILE = 16 };          /* ragged: 3 x 2 tiles, the last row 11 pixels high */
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    float means[3 * N], scales[3 * N], quats[4 * N], opac[N], shs[3 * K * N], dC[3 * W * H];
    for (int g = 0; g < N; ++g) {
        means[3 * g] = urand(-0.3f, 0.3f); means[3 * g + 1] = urand(-0.2f, 0.2f); means[3 * g + 2] = urand(-1.0f, 1.0f);
        for (int i = 0; i < 3; ++i) scales[3 * g + i] = urand(-4.0f, -2.5f);
        float q[4], nq = 0.0f;
        for (int i = 0; i < 4; ++i) { q[i] = urand(-1.0f, 1.0f); nq += q[i] * q[i]; }
        for (int i = 0; i < 4; ++i) quats[4 * g + i] = q[i] / sqrtf(nq > 0.0f ? nq : 1.0f);
        opac[g] = urand(-2.0f, 4.0f);
        for (int i = 0; i < 3 * K; ++i) shs[3 * K * g + i] = urand(-0.2f, 0.2f);
    }
    means[0] = 1.0e4f;                                                   /* off screen: no pixel takes gaussian 0 */
    for (int i = 0; i < 3 * W * H; ++i) dC[i] = urand(-1.0f, 1.0f);
    const float eye[3] = { 0.0f, 0.0f, -8.0f }, look[3] = { 0.0f, 0.0f, 0.0f }, up[3] = { 0.0f, 1.0f, 0.0f };
    gso_camera cam;
    gso_camera_matrices(eye, look, up, 400.0f, 400.0f, 0.1f, 100.0f, W, H, &cam);

    float tps[4 * N], mu[2 * N], invcov[4 * N], bbs[4 * N], rgb[3 * N], sig[N];
    gso_preprocess(N, DEG, means, scales, quats, opac, shs, &cam, NULL, tps, mu, NULL, NULL, invcov, bbs, rgb, sig);
    uint32_t perm[N], ranges[2 * 6];
    gso_depth_order(N, tps, GSO_ORDER_DEPTH_DESC, perm);
    const int64_t total = gso_bin(N, bbs, tps, perm, GSO_ORDER_DEPTH_DESC, TILE, gx, gy, ranges, NULL, NULL, 0);
    uint32_t *ids = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(total > 0 ? total : 1));
    gso_bin(N, bbs, tps, perm, GSO_ORDER_DEPTH_DESC, TILE, gx, gy, ranges, ids, NULL, total);

    int bad = 0;
    for (int pass = 0; pass < 3; ++pass) {                               /* t_min 0 (literal), 1e-5, 0.2 (pixels freeze) */
        const float t_min = pass == 0 ? 0.0f : (pass == 1 ? 1.0e-5f : 0.2f);
        double mu64[2 * N], M64[4 * N], sig64[N], rgb64[3 * N];
        for (int i = 0; i < 2 * N; ++i) mu64[i] = mu[i];
        for (int i = 0; i < 4 * N; ++i) M64[i] = invcov[i];
        for (int i = 0; i < N; ++i) sig64[i] = sig[i];
        for (int i = 0; i < 3 * N; ++i) rgb64[i] = rgb[i];
        double rows[10 * N] = { 0 }, mass[10 * N] = { 0 }, dropped[10 * N] = { 0 }, floor_[10 * N] = { 0 };
        int32_t ntiles[N] = { 0 };
        float rows32[10 * N] = { 0 };
        gso_composite_rows(&cam, TILE, gx, gy, ranges, ids, N, mu64, M64, bbs, sig64, rgb64, tps, t_min, dC, rows, mass, dropped, floor_, ntiles);
        gso_composite_rows_f32(&cam, TILE, gx, gy, ranges, ids, N, mu, invcov, bbs, sig, rgb, tps, t_min, dC, rows32);
        double kappa = 0.0;
        int touched = 0;
        for (int g = 0; g < N; ++g) {
            touched += ntiles[g] > 0;
            for (int c = 0; c < 10; ++c) {
                const double r = rows[10 * g + c], m = mass[10 * g + c], e = fabs((double)rows32[10 * g + c] - r) - floor_[10 * g + c];
                if (!isfinite(r) || !isfinite(m) || !isfinite((double)rows32[10 * g + c])) { printf("not finite: gaussian %d word %d\n", g, c); ++bad; }
                if (ntiles[g] == 0 && (r != 0.0 || m != 0.0 || rows32[10 * g + c] != 0.0f)) { printf("untouched gaussian %d word %d not zero\n", g, c); ++bad; }
                if (m > 0.0 && e / (m * 5.9604644775390625e-08) > kappa) kappa = e / (m * 5.9604644775390625e-08);
                if (m == 0.0 && e > 0.0) { printf("gaussian %d word %d: error without mass\n", g, c); ++bad; }
            }
        }
        if (ntiles[0] != 0) { printf("the off-screen gaussian was touched\n"); ++bad; }
        if (kappa > 4.0) { printf("twin outside 4 x 2^-24 x mass: kappa %.3f\n", kappa); ++bad; }
        /* the fp64 payload and the chain */
        gso_forward64(N, DEG, means, scales, quats, opac, shs, &cam, mu64, M64, sig64, rgb64);
        double dmeans[3 * N] = { 0 }, dscales[3 * N] = { 0 }, dquats[4 * N] = { 0 }, dopac[N] = { 0 }, dshs[3 * K * N] = { 0 };
        gso_chain(N, DEG, means, scales, quats, opac, shs, &cam, rows, 1, dmeans, dscales, dquats, dopac, dshs);
        for (int i = 0; i < 3 * N; ++i) if (!isfinite(dmeans[i]) || !isfinite(dscales[i])) { printf("chain: not finite at %d\n", i); ++bad; }
        for (int i = 0; i < 3; ++i) if (dmeans[i] != 0.0 || dscales[i] != 0.0) { printf("chain: untouched gaussian moved\n"); ++bad; }
        /* the SH colour path and its twin at the rows' colour gradient */
        double drgb[3 * N], sh64[3 * K * N], msh[3 * K * N], dpc[3 * N], mdpc[3 * N];
        float drgb32[3 * N], sh32[3 * K * N], dpc32[3 * N];
        for (int g = 0; g < N; ++g) for (int c = 0; c < 3; ++c) { drgb32[3 * g + c] = (float)rows[10 * g + c]; drgb[3 * g + c] = drgb32[3 * g + c]; }
        gso_sh_path(N, DEG, means, shs, &cam, drgb, sh64, msh, dpc, mdpc);
        gso_sh_path_f32(N, DEG, means, shs, &cam, drgb32, sh32, dpc32);
        for (int i = 0; i < 3 * K * N; ++i) {
            const double e = fabs((double)sh32[i] - sh64[i]) - gso_floor_unit();
            if (!isfinite(sh64[i]) || !isfinite(msh[i]) || e > 4.0 * 5.9604644775390625e-08 * msh[i]) { printf("SH path: d_shs[%d] outside its mass\n", i); ++bad; }
        }
        for (int i = 0; i < 3 * N; ++i) {
            const double e = fabs((double)dpc32[i] - dpc[i]) - gso_floor_unit();
            if (!isfinite(dpc[i]) || !isfinite(mdpc[i]) || e > 4.0 * 5.9604644775390625e-08 * mdpc[i]) { printf("SH path: dpc[%d] outside its mass\n", i); ++bad; }
        }
        printf("t_min %g: %lld list entries, %d of %d gaussians touched, twin kappa %.3f\n", (double)t_min, (long long)total, touched, N, kappa);
    }
    free(ids);
    printf(bad ? "FAILED (%d)\n" : "ok\n", bad);
    return bad ? 1 : 0;
}
