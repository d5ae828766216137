// gs_preprocess.hip -- fused per-gaussian preprocess for gfx950.
//
// Replaces five reference launches (each with a device sync) by one kernel, one thread per
// gaussian: frustumCulling (src/projection.jl:39-100), tValues (:103-155), computeInvCov2d
// (src/cov2d.jl:30-45), computeBB (src/boundingbox.jl:4-36), plus sh2color / cusigmoid
// hoisted out of the per-pixel loop (src/splat.jl:175-193; they depend on gaussian and view
// only), the depth radix key for forward.jl:103 and the tile rectangle of hitBinning
// (src/binning.jl:3-35).
//
// This translation unit is compiled with -ffp-contract=off: every fp32 operation below is
// individually rounded in the reference's written order, so tile rectangles and depth keys
// are bit-identical to the CPU oracle.  HBM-bound: 4*(11+3K) B read +
// 60 B written per gaussian; no LDS, no MFMA.
#include "gs_pergaussian.h"
#include "gs_sh.h"

#pragma clang fp contract(off)

// DEG is the ACTIVE degree: the bands evaluated.  STRIDED: the model stores more bands than that (gs_set_active_sh_degree below the model's
// degree) -- a row is sh_stride floats apart and its first 3 K are read, in the same order: the colour is what the model truncated to DEG gives.
template <int DEG, bool STRIDED = false>
__global__ __launch_bounds__(256) void gs_preprocess_kernel(GsPreprocessArgs a, GsCamera cam, int sh_stride) {
    constexpr int K = (DEG + 1) * (DEG + 1);
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;

    // ---- frustumCulling, projection.jl:46-93
    const float *T = cam.T, *P = cam.P;
    const float m1 = a.means[3 * g], m2 = a.means[3 * g + 1], m3 = a.means[3 * g + 2];
    float ts[4], tps[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float s = T[i] * m1;
        s = s + T[i + 4] * m2;
        s = s + T[i + 8] * m3;
        s = s + T[i + 12] * 1.0f;
        ts[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float s = P[i] * ts[0];
        s = s + P[i + 4] * ts[1];
        s = s + P[i + 8] * ts[2];
        s = s + P[i + 12] * ts[3];
        tps[i] = s;
    }
    const double cx = cam.W / 2.0, cy = cam.H / 2.0;                  // forward.jl:58-59 (Float64)
    const float wf = (float)cam.W, hf = (float)cam.H;
    const float mux = (float)((double)((wf * tps[0] / tps[3] + 1.0f) / 2.0f) + cx);   // projection.jl:88
    const float muy = (float)((double)((hf * tps[1] / tps[3] + 1.0f) / 2.0f) + cy);   // :89

    // ---- tValues, projection.jl:107-152
    const float tx = ts[0], ty = ts[1], tz = ts[2];
    float J[2][3];
    J[0][0] = cam.fx / tz; J[1][0] = 0.0f;
    J[0][1] = 0.0f;        J[1][1] = cam.fy / tz;
    J[0][2] = -cam.fx * tx / (tz * tz);
    J[1][2] = -cam.fy * ty / (tz * tz);
    float R[3][3];                                                    // quatToRot, projection.jl:1-14
    gs_quat_to_rot(a.quats[4 * g], a.quats[4 * g + 1], a.quats[4 * g + 2], a.quats[4 * g + 3], R);
    float S[3][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    S[0][0] = gs_expf(a.scales[3 * g]);
    S[1][1] = gs_expf(a.scales[3 * g + 1]);
    S[2][2] = gs_expf(a.scales[3 * g + 2]);
    float Wm[3][3], C3[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float s = R[i][0] * S[0][j];
            s = s + R[i][1] * S[1][j];
            s = s + R[i][2] * S[2][j];
            Wm[i][j] = s;
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float s = Wm[i][0] * Wm[j][0];
            s = s + Wm[i][1] * Wm[j][1];
            s = s + Wm[i][2] * Wm[j][2];
            C3[i][j] = s;
        }
    float JR[2][3], JCR[2][3], c2[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float s = J[i][0] * R[0][j];
            s = s + J[i][1] * R[1][j];
            s = s + J[i][2] * R[2][j];
            JR[i][j] = s;
        }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float s = JR[i][0] * C3[0][j];
            s = s + JR[i][1] * C3[1][j];
            s = s + JR[i][2] * C3[2][j];
            JCR[i][j] = s;
        }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float s = JCR[i][0] * JR[j][0];
            s = s + JCR[i][1] * JR[j][1];
            s = s + JCR[i][2] * JR[j][2];
            c2[i][j] = (float)((double)s + 0.3);                      // :150 (+0.3 on all four, Float64)
        }
    GsSplatView sv;
    sv.mux = mux; sv.muy = muy;
    sv.cov[0] = c2[0][0]; sv.cov[1] = c2[1][0]; sv.cov[2] = c2[0][1]; sv.cov[3] = c2[1][1];
    gs_conic_box(sv.cov, mux, muy, cam.W, cam.H, sv.inv, sv.bb);      // computeInvCov2d, computeBB

    // ---- sh2color, splat.jl:180-193 (degrees 2,3: build extension, same accumulation order)
    const float d0 = tps[0] - (cam.lookAt[0] - cam.eye[0]);
    const float d1 = tps[1] - (cam.lookAt[1] - cam.eye[1]);
    const float d2 = tps[2] - (cam.lookAt[2] - cam.eye[2]);
    const float nrm = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
    const float ninv = 1.0f / nrm;
    const float x = ninv * d0, y = ninv * d1, z = ninv * d2;
    const float X = x, Y = y, Z = z;
#include "gs_sh_basis.inc"
    const float *sh = a.shs + (STRIDED ? (int64_t)sh_stride : (int64_t)3 * K) * g;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float s = sh[c] * bs[0];
#pragma unroll
        for (int k = 1; k < K; ++k) s = s + sh[c + 3 * k] * bs[k];
        sv.rgb[c] = (float)((double)s + 0.5);                            // :192
    }
    sv.sig = gs_sigmoid_logit<float>(a.opac[g]);                      // cusigmoid, splat.jl:175-178

    // ---- payload, conic, tile rectangle; the near/far skip of splat.jl:227 becomes an empty pixel box
    // (the rectangle is formed here, not where the box is: there the degree-3 kernel takes 101 VGPRs instead of 118 -- a fifth wave per SIMD --
    // and the stage 0.073 instead of 0.070 ms at C3, profiles/pergaussian_once_ab.log)
    gs_tile_rect(sv.bb, a.gx, a.gy, sv.rc);                           // binning.jl:6-27
    const uint32_t key = gs_depth_key(tps[2], a.order);
    const bool depth_ok = !(tps[2] < cam.near_ || tps[2] > cam.far_);
    gs_store_splat(sv, g, depth_ok, a.payload, a.invcov, a.rect, a.dbg, a.dbg.ts != nullptr);
    a.depth_key[g] = key;
    if (a.key_range) {                                                  // the frame's key range, for the two-step depth sort (gs_sort.hip)
        uint32_t *lo = a.key_range + (size_t)(blockIdx.x % GS_KEY_RANGE_SLOTS) * GS_KEY_RANGE_STRIDE;
        uint32_t *hi = lo + (size_t)GS_KEY_RANGE_SLOTS * GS_KEY_RANGE_STRIDE;
        // keys of non-finite depths (NaN, +-Inf) stay out of the range: ds_bucket clamps them into the end buckets, and a single
        // one would otherwise stretch the range until every finite key shares a bucket
        const bool finite = key > 0x007FFFFFu && key < 0xFF800000u;
        if (__ballot(1) == ~0ull) {                                     // a full wave (every wave but the grid's last) folds first
            uint32_t mn = finite ? key : 0xFFFFFFFFu, mx = finite ? key : 0u;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) { mn = min(mn, (uint32_t)__shfl_xor((int)mn, d)); mx = max(mx, (uint32_t)__shfl_xor((int)mx, d)); }
            if ((threadIdx.x & 63) == 0) { atomicMin(lo, mn); atomicMax(hi, mx); }
        } else if (finite) { atomicMin(lo, key); atomicMax(hi, key); }
    }
    if (a.dbg.ts) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { a.dbg.ts[4 * g + i] = ts[i]; a.dbg.tps[4 * g + i] = tps[i]; }
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) a.dbg.cov3d[9 * g + i + 3 * j] = C3[i][j];
    }
}

hipError_t gs_launch_preprocess(const GsPreprocessArgs &a, const GsCamera &cam, int sh_stride, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    const dim3 block(256), grid((unsigned)((a.n + 255) / 256));
    return gs_sh_dispatch(a.sh_degree, sh_stride, [&](auto D, auto S) {
        hipLaunchKernelGGL((gs_preprocess_kernel<decltype(D)::value, decltype(S)::value>), grid, block, 0, stream, a, cam, sh_stride);
        return hipGetLastError();
    });
}
