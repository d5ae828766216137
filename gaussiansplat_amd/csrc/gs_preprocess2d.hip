// gs_preprocess2d.hip -- the 2-D image-fitting renderer (RendererType GAUSSIAN_2D) for gfx950.
//
// Forward: preprocess(::GaussianRenderer2D) (reference src/forward.jl:9-33) = computeCov2d_kernel
// (src/cov2d.jl:3-28: Sigma = R(theta) diag(exp s)^2 R' with +0.3 on the diagonal), computeInvCov2d
// (src/cov2d.jl:30-45) and computeBB (src/boundingbox.jl:4-36), three launches with a device sync each in the
// reference, one kernel here.  It emits the SAME 64-byte payload as the 3-D preprocess, so binning and both
// composite kernels are shared.  SplatData2D (src/splat.jl:20-26): means 2xN in [0,1]^2 (pixel position
// (w*mx, h*my), splat.jl:337-339), scales 2xN (log), rotations 1xN, opacities 1xN (used raw, splat.jl:341),
// colors 3xN.  The reference hands the [0,1] means to computeBB (forward.jl:25-31), which would pin every box
// to the image origin; the pixel position is used instead.
//
// Backward: the chain from the composite's per-gaussian sums d{rgb3, sig, mu2, inv4} to SplatGrads2D
// (src/splat.jl:28-34).  The reference's splatGrads (splat.jl:271-396) mixes several forwards
// and is not reproduced; this is the derived adjoint, checked against fp64 autograd of the restated forward.
//
// Compiled with -ffp-contract=off: tile rectangles must be bit-identical to the CPU oracle.
// HBM-bound: 36 B read + 60 B written per gaussian forward, 76 B read + 36 B written backward.
#include "gs_pergaussian.h"

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void gs_preprocess2d_kernel(GsPreprocess2DArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;
    // ---- computeCov2d_kernel, cov2d.jl:5-26
    float sn, cs;
    gs_sincosf(a.rots[g], sn, cs);
    const float R[2][2] = {{cs, -sn}, {sn, cs}};
    const float S[2][2] = {{gs_expf(a.scales[2 * g]), 0.0f}, {0.0f, gs_expf(a.scales[2 * g + 1])}};
    float Wm[2][2], Jm[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float s = R[i][0] * S[0][j];
            s = s + R[i][1] * S[1][j];
            Wm[i][j] = s;                                              // :18 W = R*S
        }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float s = Wm[i][0] * Wm[j][0];
            s = s + Wm[i][1] * Wm[j][1];
            Jm[i][j] = s;                                              // :19 J = W*W'
        }
    GsSplatView sv;
    sv.cov[0] = (float)((double)Jm[0][0] + 0.3);                       // :25 (Float64 literal, diagonal only)
    sv.cov[1] = Jm[1][0]; sv.cov[2] = Jm[0][1];
    sv.cov[3] = (float)((double)Jm[1][1] + 0.3);                       // :26
    // ---- pixel position, splat.jl:337-339
    sv.mux = (float)a.W * a.means[2 * g]; sv.muy = (float)a.H * a.means[2 * g + 1];
    gs_conic_box(sv.cov, sv.mux, sv.muy, a.W, a.H, sv.inv, sv.bb);     // computeInvCov2d, computeBB
    gs_tile_rect(sv.bb, a.gx, a.gy, sv.rc);                            // binning.jl:6-27
    // raw opacity (splat.jl:341) clamped to [0, 1): alpha must stay below 1 for the adjoint's 1/(1-alpha); NaN -> 0
    sv.sig = fminf(fmaxf(a.opac[g], 0.0f), 0.99999994f);
    sv.rgb[0] = a.colors[3 * g]; sv.rgb[1] = a.colors[3 * g + 1]; sv.rgb[2] = a.colors[3 * g + 2];
    gs_store_splat(sv, g, true, a.payload, a.invcov, a.rect, a.dbg, a.dbg.mu != nullptr);
    a.depth_key[g] = 0u;                                               // no depth: lists are in gaussian-index order
}

// accumulate (+=) or overwrite
template <bool OVERWRITE>
__device__ __forceinline__ void put(float *p, float v) { if (OVERWRITE) *p = v; else *p += v; }

// d{rgb3, sig, mu2, inv4} -> d{means2, scales2, rotation, opacity, colors3}; accumulate (+=) or overwrite.
template <bool OVERWRITE>
__global__ __launch_bounds__(256) void gs_preprocess2d_bwd_kernel(GsPreprocess2DBwdArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;
    float g2[10];
    gs_g2d_row_load(a, g, g2);
    // forward pieces again (cheaper than storing them): Sigma = Wm Wm' + 0.3 I, M = Sigma^-1
    float sn, cs;
    gs_sincosf(a.rots[g], sn, cs);
    const float e0 = gs_expf(a.scales[2 * g]), e1 = gs_expf(a.scales[2 * g + 1]);
    const float Wm[2][2] = {{cs * e0, -sn * e1}, {sn * e0, cs * e1}};
    const float c00 = Wm[0][0] * Wm[0][0] + Wm[0][1] * Wm[0][1] + 0.3f;
    const float c01 = Wm[0][0] * Wm[1][0] + Wm[0][1] * Wm[1][1];
    const float c11 = Wm[1][0] * Wm[1][0] + Wm[1][1] * Wm[1][1] + 0.3f;
    const float idet = 1.0f / (c00 * c11 - c01 * c01);
    const float M[2][2] = {{c11 * idet, -c01 * idet}, {-c01 * idet, c00 * idet}};
    const float op = a.opac[g];
    gs_g2d_to_grads(g2, fminf(fmaxf(op, 0.0f), 0.99999994f), M[0][0], M[0][1], M[1][1]);      // raw moments -> d{sig, mu, conic}
    const float G[2][2] = {{g2[6], g2[8]}, {g2[7], g2[9]}};            // column-major inv4: [r + 2c]
    // dSigma = -M' G M'
    float t1[2][2], dcov[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) t1[i][j] = M[0][i] * G[0][j] + M[1][i] * G[1][j];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) dcov[i][j] = -(t1[i][0] * M[j][0] + t1[i][1] * M[j][1]);
    // Sigma = Wm Wm': dWm = (dSigma + dSigma') Wm ; Wm = R(theta) diag(e)
    float dWm[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            dWm[i][j] = (dcov[i][0] + dcov[0][i]) * Wm[0][j] + (dcov[i][1] + dcov[1][i]) * Wm[1][j];
    const float R[2][2] = {{cs, -sn}, {sn, cs}}, dR[2][2] = {{-sn, -cs}, {cs, -sn}};
    const float e[2] = {e0, e1};
    float ds[2], dth = 0.0f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float de = R[0][j] * dWm[0][j] + R[1][j] * dWm[1][j];
        dth = dth + (dR[0][j] * dWm[0][j] + dR[1][j] * dWm[1][j]) * e[j];
        ds[j] = de * e[j];
    }
    const float dm0 = (float)a.W * g2[4], dm1 = (float)a.H * g2[5];
    if (a.d_means) { put<OVERWRITE>(a.d_means + 2 * g, dm0); put<OVERWRITE>(a.d_means + 2 * g + 1, dm1); }
    if (a.d_scales) { put<OVERWRITE>(a.d_scales + 2 * g, ds[0]); put<OVERWRITE>(a.d_scales + 2 * g + 1, ds[1]); }
    if (a.d_rots) put<OVERWRITE>(a.d_rots + g, dth);
    const float dop = (op > 0.0f && op < 0.99999994f) ? g2[3] : 0.0f;       // the clamp of the forward has zero slope outside
    if (a.d_opac) put<OVERWRITE>(a.d_opac + g, dop);
    if (a.d_colors) {
#pragma unroll
        for (int k = 0; k < 3; ++k) put<OVERWRITE>(a.d_colors + 3 * g + k, g2[k]);
    }
}

hipError_t gs_launch_preprocess2d(const GsPreprocess2DArgs &a, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_preprocess2d_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t gs_launch_preprocess2d_bwd(const GsPreprocess2DBwdArgs &a, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.n + 255) / 256)), block(256);
    if (a.overwrite) hipLaunchKernelGGL(gs_preprocess2d_bwd_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(gs_preprocess2d_bwd_kernel<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}
