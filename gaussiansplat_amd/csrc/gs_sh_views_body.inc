// gs_sh_views_body.inc -- the body of the kernels that rebuild the SH gradients from the colour gradients of several views
// (d sh[k][c] = sum_v basis_k(dir_v) * d rgb_v[c]), included by gs_sh_from_views_kernel (gs_preprocess_bwd.hip: d rgb from dense
// [views][3n] slots) and by gs_sh_from_touched_kernel (gs_touched.hip: from bitmaps plus compacted rows).  ONE text, so that both
// compute the direction, the basis and the sums alike; they differ in two macros only: GS_SH_VIEWS_BEGIN (first thing in the loop over the views:
// whatever the source needs before the arithmetic; may be empty) and GS_SH_VIEWS_DRGB, which declares the three floats g0, g1, g2
// of (view v, gaussian g) as plain loads.  Expects n, means, nviews, cams, d_shs, sh_stride and the template parameters DEG, OVERWRITE,
// STRIDED in scope, and gs_sh.h included (the basis is gs_sh_basis.inc).  DEG is the ACTIVE degree; STRIDED: the rows of d_shs are sh_stride > 3 K floats apart (an active degree below the
// stored one): their first 3 K floats are rebuilt, the rest become + 0 when overwriting and are left alone when accumulating.
    constexpr int K = (DEG + 1) * (DEG + 1);
    constexpr int ROW = 3 * K + 1;
    extern __shared__ __attribute__((aligned(16))) float tile[];       // [256][ROW] accumulators
    const int64_t gb = (int64_t)blockIdx.x * blockDim.x;
    const int nb = (int)min((int64_t)blockDim.x, n - gb);
    const int64_t g = gb + threadIdx.x;
    float *acc = tile + threadIdx.x * ROW;
#pragma unroll
    for (int i = 0; i < 3 * K; ++i) acc[i] = 0.0f;
    if (g < n) {
        const float m1 = means[3 * g], m2 = means[3 * g + 1], m3 = means[3 * g + 2];
        for (int v = 0; v < nviews; ++v) {
            GS_SH_VIEWS_BEGIN
            const float *T = cams + 38 * v, *P = T + 16, *eye = T + 32, *lookAt = T + 35;
            float t[4], p[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) t[i] = T[i] * m1 + T[i + 4] * m2 + T[i + 8] * m3 + T[i + 12];
#pragma unroll
            for (int i = 0; i < 4; ++i) p[i] = P[i] * t[0] + P[i + 4] * t[1] + P[i + 8] * t[2] + P[i + 12] * t[3];
            const float v0 = p[0] - (lookAt[0] - eye[0]);
            const float v1 = p[1] - (lookAt[1] - eye[1]);
            const float v2 = p[2] - (lookAt[2] - eye[2]);
            const float inrm = rsqrtf(v0 * v0 + v1 * v1 + v2 * v2);
            const float X = v0 * inrm, Y = v1 * inrm, Z = v2 * inrm;
#include "gs_sh_basis.inc"
            GS_SH_VIEWS_DRGB
#pragma unroll
            for (int k = 0; k < K; ++k) { acc[3 * k] += bs[k] * g0; acc[3 * k + 1] += bs[k] * g1; acc[3 * k + 2] += bs[k] * g2; }
        }
    }
    __syncthreads();
    const int RS = STRIDED ? sh_stride : 3 * K;
    for (int idx = threadIdx.x; idx < nb * 3 * K; idx += blockDim.x) {     // coalesced rows
        const float v = tile[(idx / (3 * K)) * ROW + idx % (3 * K)];
        const int64_t gi = gs_sh_row_index<3 * K, STRIDED>(gb, RS, idx);
        if (OVERWRITE) d_shs[gi] = v; else d_shs[gi] += v;
    }
    if constexpr (STRIDED && OVERWRITE) gs_sh_zero_inactive<3 * K>(d_shs, gb, nb, RS);
