// gs_preprocess_bwd.hip -- per-gaussian chain rule from the 2-D splat gradients back to the
// model parameters (means, scales, quaternions, opacities, SH coefficients).
//
// The reference has no 3-D backward: backward.jl:3-38 launches splatGrads (splat.jl:271-396),
// the adjoint of an older 2-D fitting forward, and grads.jl:1-3 (updateColorGrads) is an empty
// stub.  What is contractual is kept: gradients ACCUMULATE into arrays shaped like the
// parameters (splat.jl:137-156) until resetGrads (splat.jl:158-173).  The mathematics is the
// derived adjoint of the reference FORWARD (projection.jl:39-155, cov2d.jl:30-45,
// splat.jl:175-193), including its quirks: R22 = 1 - 2(x^2 - z^2), the gaussian's own R in
// J*R, +0.3 on all four covariance entries, clip-space view direction for SH.
//
// Two kernels, one thread per gaussian, no atomics (each thread owns its rows); HBM-bound:
//   gs_sh_bwd_kernel    d rgb -> d shs, plus d rgb / d(clip position) handed to the second kernel
//                       (16 B/gaussian).  The SH gradients (3K floats = 192 B at degree 3, thread-strided in
//                       HBM) go through an LDS tile [256][3K+1]: conflict-free per-thread rows (odd stride),
//                       stored/added to d_shs with coalesced accesses.  The SH coefficients are read only for
//                       gaussians a pixel touched, by their own thread (the colour's dependence on the view direction).
//   gs_geom_bwd_kernel  d{mu', invCov2d, sig} -> d{means, scales, quaternions, opacities}.  The chain (3x3 / 2x3 / 2x2
//                       products, the 2x2 inverse and the quaternion terms) is evaluated in fp64 from the fp32 inputs:
//                       in fp32 its cancellations put the quaternion gradient at 2e-4 .. 2e-3 relative L2 of the fp64
//                       adjoint (C3, C5 tile samples) while every other array sits at 2e-5 .. 1e-4; ~400 flops per
//                       gaussian, so the kernel stays HBM-bound.
// Splitting keeps both under 128 VGPRs (the fused version needed 168 + spills).
// `overwrite` stores instead of accumulating: used for the first backward after resetGrads, so
// the reset needs no 4(11+3K)-byte/gaussian zero fill and this pass no read of the old gradients.
#include "gs_pergaussian.h"  // quatToRot and the sigmoid as the forward has them, the row of 2-D gradient sums (gs_g2d_row_load)
#include "gs_sh.h"            // SH_C0 / SH_C1 / bC2 / bC3, gs_sh_dispatch, the strided rows
#include "gs_wave.h"
#include <stdlib.h>

#ifndef GS_NT_STORES
#define GS_NT_STORES 2               // overwrite-mode gradient stores bypass the caches: 1 the SH gradients, 2 the geometry chain's too (0: A/B builds)
#endif
// old + v as one rounded add that the compiler may not fuse with the products v came from: the accumulating and the
// overwriting instantiation must produce the SAME v (accumulating eight views == the sum of eight single-view gradients)
__device__ __forceinline__ float add_exact(float old, float v) {
#pragma clang fp contract(off)
    return old + v;
}
// accumulate, or (sgd_scale != 0) apply the step: the same fma gs_sgd_step would do on the stored float gradient
__device__ __forceinline__ float acc_or_step(float old, float v, float sgd_scale) {
    return sgd_scale != 0.0f ? fmaf(sgd_scale, v, old) : add_exact(old, v);
}
// one geometry gradient to its place: stored past the caches (overwriting), or accumulated / stepped
template <bool OVERWRITE>
__device__ __forceinline__ void grad_put(float *dst, float v, float sgd_scale) {
    if (OVERWRITE) { if (GS_NT_STORES > 1) __builtin_nontemporal_store(v, dst); else *dst = v; }
    else *dst = acc_or_step(*dst, v, sgd_scale);
}

// FUSED: the geometry chain of the gaussian follows in the same thread (gs_backward's usual case: both phases) -- its row of 2-D gradients
// and its mean are read once, d L / d tps stays in registers, one launch less.  The two-kernel form remains for callers that run the
// phases apart (a multi-GPU host starts the exchange of the SH gradients between them).
// ADAM (with OVERWRITE and FUSED; gs_backward_adam): 1 dense, 2 selective -- where the OVERWRITE instantiation stores a gradient, the
// same float steps p, m and v instead (gs_adam_update): the geometry rows in the thread, the SH rows in the coalesced loop behind the
// LDS tile.  Every row is visited (dense Adam moves untouched rows too: the moments decay); selective mode decides liveness per
// gaussian on all 11 + 3K gradient floats, as gs_adam_step does.
// DEG is the ACTIVE degree: basis, bs / cs, the ladders, the tile's width.  STRIDED (an active degree below the stored one, gs_set_active_sh_degree):
// the rows of shs, d_shs and the SH moments are RS = a.sh_stride floats apart and their first 3 K are this kernel's -- the same floats the model
// truncated to DEG gets.  The floats behind them: overwriting, + 0 (unless the fill workgroups wrote it, a.shs_zeroed); Adam, stepped with a
// gradient of + 0 in every row that is stepped (what gs_adam_step does with the stored + 0); accumulating or SGD, neither read nor written.
template <int DEG, bool OVERWRITE, bool FUSED, int ADAM = 0, bool STRIDED = false>
__global__ __launch_bounds__(256) void gs_sh_bwd_kernel(GsPreprocessBwdArgs a, GsCamera cam, GsAdamFused ad) {
#pragma clang fp contract(off)   // the fused and the two-kernel form must produce the same bits: no context-dependent fma formation
    constexpr int K = (DEG + 1) * (DEG + 1);
    constexpr int ROW = 3 * K + 1;
    const int RS = STRIDED ? a.sh_stride : 3 * K;                       // floats between two rows in global memory
    extern __shared__ __attribute__((aligned(16))) float tile[];       // [256][ROW]
    // Untouched gaussians.  With the transmittance early-out most gaussians of a dense view are never composited (C3: 63 %, C5: 90 %,
    // tools/touched_rows.py): their colour gradient d rgb is exactly zero, hence d shs = basis * 0 and the colour -> direction term are
    // exactly zero.  When ACCUMULATING (views after the first of a batch) their d_shs rows are neither read nor written: C4 on one GPU
    // 8.85 -> 8.71 ms per 8 views, same box (profiles/r04j_ab_untouched_rows.log).  When OVERWRITING the zeros have to be written -- by
    // this kernel, or (a.shs_zeroed) by the fill workgroups at the end of the composite backward's launch, which zeroed ALL of d_shs: then
    // only the live rows are stored here.  Either way an untouched row ends as + 0.0 in every float (the store loop writes 0.0f for it,
    // not the tile's basis * 0, whose sign depends on the basis).
    constexpr bool SKIP = !OVERWRITE;
    __shared__ uint8_t srow_live[256];
    const int64_t gb = (int64_t)blockIdx.x * blockDim.x;
    const int nb = (int)min((int64_t)blockDim.x, a.n - gb);
    float g2[10];
    if (SKIP) {
        const int64_t g0 = gb + threadIdx.x;
        bool lv = false;
        if (g0 < a.n) { gs_g2d_row_load(a, g0, g2); lv = g2[0] != 0.0f || g2[1] != 0.0f || g2[2] != 0.0f; }
        srow_live[threadIdx.x] = lv ? 1 : 0;
        __syncthreads();
    }
    // 3K is a multiple of 4 only for K = 4, 16 ... : use 16-byte global accesses when it is
    // (strided: the rows must start on 16 bytes too -- active 1 in stored 3 only; everything else one float per lane)
    constexpr bool VEC = (3 * K) % 4 == 0;
    const bool vec_rows = VEC && (!STRIDED || RS % 4 == 0);
    const bool vec_out = vec_rows && (reinterpret_cast<uintptr_t>(a.d_shs) & 15) == 0;   // e.g. a flat buffer slice at 44 n bytes
    const int64_t g = gb + threadIdx.x;
    if (g < a.n) {
        if (!SKIP) gs_g2d_row_load(a, g, g2);
        // a gaussian no pixel touched (off screen, or skipped by the composite because its per-view payload is not finite:
        // tz == 0, exp(scale) overflow, singular covariance) has an all-zero row: its gradient is exactly zero, and the
        // recomputed direction may be NaN, so zeros are substituted for the basis instead of forming 0 * NaN
        const bool live = g2[0] != 0.0f || g2[1] != 0.0f || g2[2] != 0.0f;
        const float grgb[3] = {g2[0], g2[1], g2[2]};
        const float *T = cam.T, *P = cam.P;
        const float m1 = a.means[3 * g], m2 = a.means[3 * g + 1], m3 = a.means[3 * g + 2];
        float t[4], p[4];                                               // (text, not a function: gs_pergaussian.h says why)
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = T[i] * m1 + T[i + 4] * m2 + T[i + 8] * m3 + T[i + 12];
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = P[i] * t[0] + P[i + 4] * t[1] + P[i + 8] * t[2] + P[i + 12] * t[3];
        // ---- rgb(sh, dir(p)), splat.jl:180-193
        const float v0 = p[0] - (cam.lookAt[0] - cam.eye[0]);
        const float v1 = p[1] - (cam.lookAt[1] - cam.eye[1]);
        const float v2 = p[2] - (cam.lookAt[2] - cam.eye[2]);
        const float inrm = live ? rsqrtf(v0 * v0 + v1 * v1 + v2 * v2) : 0.0f;
        const float X = live ? v0 * inrm : 0.0f, Y = live ? v1 * inrm : 0.0f, Z = live ? v2 * inrm : 0.0f;
#include "gs_sh_basis.inc"
        float *sh = tile + threadIdx.x * ROW;
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sh[c + 3 * k] = bs[k] * grgb[c];   // the tile carries d L / d sh (stored coalesced below)
        }
        if (OVERWRITE && ADAM == 0) srow_live[threadIdx.x] = live ? 1 : 0;     // (the barrier below stands between this and its readers)
        float ddir[3] = {0.0f, 0.0f, 0.0f};
        if (live) {
            // d L / d dir through the colour needs the coefficients: those of THIS gaussian, read by its own thread as twelve 16-byte
            // loads, and only if a pixel touched it (37 % of the gaussians at C3, 10 % at C5) -- cs[k] = d rgb . sh[:, k], then the
            // derivative polynomials of the basis.  (Until round 4 every row came in through the LDS tile, touched or not: 192 of the
            // kernel's 476 bytes per gaussian.  A 3 x 3 Jacobian d rgb / d dir written by the preprocess instead was measured too: the
            // backward 10 us faster than this, the preprocess 30 us slower -- 131 VGPRs, three waves per SIMD; profiles/r04s_ab_lazy_sh.log.)
            const float4 *row = reinterpret_cast<const float4 *>(a.shs + (int64_t)RS * g);
            float shv[3 * K];
            if (vec_rows) {                                             // (a constant unless STRIDED: then the first 3 K floats of a row that starts on 16 bytes)
#pragma unroll
                for (int q = 0; q < 3 * K / 4; ++q) { const float4 t4 = row[q]; shv[4 * q] = t4.x; shv[4 * q + 1] = t4.y; shv[4 * q + 2] = t4.z; shv[4 * q + 3] = t4.w; }
            } else {
#pragma unroll
                for (int q = 0; q < 3 * K; ++q) shv[q] = a.shs[(int64_t)RS * g + q];
            }
            float cs[K];
#pragma unroll
            for (int k = 0; k < K; ++k) cs[k] = grgb[0] * shv[3 * k] + grgb[1] * shv[3 * k + 1] + grgb[2] * shv[3 * k + 2];
#define GS_SH_DDIR_T float
#include "gs_sh_ddir.inc"
#undef GS_SH_DDIR_T
        }
        const float dd = X * ddir[0] + Y * ddir[1] + Z * ddir[2];
        // d L / d tps[1:3] through the colour (dir = normalize(tps[1:3] - (lookAt - eye)))
        const float4 dpc_sh = make_float4((ddir[0] - X * dd) * inrm, (ddir[1] - Y * dd) * inrm, (ddir[2] - Z * dd) * inrm, 0.0f);
        if (FUSED) {
            const float (&g2f)[10] = g2;
#define GS_GEOM_DPC dpc_sh
#define GS_GEOM_ADAM
            do {
#include "gs_geom_bwd_body.inc"
            } while (0);
#undef GS_GEOM_ADAM
#undef GS_GEOM_DPC
        } else reinterpret_cast<float4 *>(a.dpc)[g] = dpc_sh;
    }
    __syncthreads();
    if constexpr (ADAM != 0) {
        // p, m, v of the SH rows: group 4 for the first three floats of a row, 5 for the rest
        const int64_t o = gb * RS;
        float *ps = const_cast<float *>(a.shs) + o, *ms = ad.m[4] + o, *vs = ad.v[4] + o;
        const bool vec = vec_rows && ((reinterpret_cast<uintptr_t>(a.shs) | reinterpret_cast<uintptr_t>(ad.m[4]) | reinterpret_cast<uintptr_t>(ad.v[4])) & 15) == 0;
        const float ss4 = ad.h.step_size[4], ss5 = ad.h.step_size[5];
        // selective: the live rows compacted (a ballot per wave), so that every lane of the loops below steps a live float -- the
        // correctly rounded update is ~55 VALU operations per float, which the masked lanes of a mixed wave would pay as well
        int nrow = nb;
        __shared__ int srow_order[ADAM == 2 ? 256 : 1], swave_live[16];
        if constexpr (ADAM == 2) {
            const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
            const bool l = threadIdx.x < nb && srow_live[threadIdx.x];
            const GsWaveRank r = gs_wave_rank(l, lane);
            if (lane == 0) swave_live[wv] = r.count;
            __syncthreads();
            int off = 0;
            nrow = 0;
            for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { off += w < wv ? swave_live[w] : 0; nrow += swave_live[w]; }
            if (l) srow_order[off + r.below] = threadIdx.x;
            __syncthreads();
        }
        if (vec) {
            for (int c4 = threadIdx.x; c4 < nrow * (3 * K / 4); c4 += blockDim.x) {
                const int ri = (c4 * 4) / (3 * K), j = (c4 * 4) % (3 * K);
                const int row = ADAM == 2 ? srow_order[ri] : ri;
                const int i4 = (row * RS + j) / 4;
                const float *t = tile + row * ROW + j;
                float4 p = reinterpret_cast<float4 *>(ps)[i4], m = reinterpret_cast<float4 *>(ms)[i4], v = reinterpret_cast<float4 *>(vs)[i4];
                gs_adam_update(p.x, m.x, v.x, t[0], ad.h, j < 3 ? ss4 : ss5);
                gs_adam_update(p.y, m.y, v.y, t[1], ad.h, j + 1 < 3 ? ss4 : ss5);
                gs_adam_update(p.z, m.z, v.z, t[2], ad.h, j + 2 < 3 ? ss4 : ss5);
                gs_adam_update(p.w, m.w, v.w, t[3], ad.h, j + 3 < 3 ? ss4 : ss5);
                reinterpret_cast<float4 *>(ps)[i4] = p; reinterpret_cast<float4 *>(ms)[i4] = m; reinterpret_cast<float4 *>(vs)[i4] = v;
            }
        } else {
            for (int c = threadIdx.x; c < nrow * 3 * K; c += blockDim.x) {
                const int ri = c / (3 * K), j = c % (3 * K);
                const int row = ADAM == 2 ? srow_order[ri] : ri;
                const int idx = row * RS + j;
                float p = ps[idx], m = ms[idx], v = vs[idx];
                gs_adam_update(p, m, v, tile[row * ROW + j], ad.h, j < 3 ? ss4 : ss5);
                ps[idx] = p; ms[idx] = m; vs[idx] = v;
            }
        }
        if constexpr (STRIDED) {
            // the inactive floats of the rows stepped above: a gradient of + 0 -- the moments decay, p moves where old moments are non-zero
            const int hi = RS - 3 * K;
            for (int c = threadIdx.x; c < nrow * hi; c += blockDim.x) {
                const int ri = c / hi, j = 3 * K + c % hi;
                const int row = ADAM == 2 ? srow_order[ri] : ri;
                const int idx = row * RS + j;
                float p = ps[idx], m = ms[idx], v = vs[idx];
                gs_adam_update(p, m, v, 0.0f, ad.h, ss5);
                ps[idx] = p; ms[idx] = m; vs[idx] = v;
            }
        }
    } else if (a.d_shs) {
        if (vec_out) {
            float4 *dst = reinterpret_cast<float4 *>(a.d_shs + gb * RS);
            for (int t4 = threadIdx.x; t4 < nb * (3 * K / 4); t4 += blockDim.x) {
                const int row = (t4 * 4) / (3 * K);
                const int i4 = STRIDED ? (row * RS + (t4 * 4) % (3 * K)) / 4 : t4;   // where the four floats sit in global memory
                const bool lv = srow_live[row] != 0;
                if ((!OVERWRITE || a.shs_zeroed) && !lv) continue;       // + 0 (or a step of 0): the row stays as it is; overwriting: it holds its zeros already
                const float *t = tile + row * ROW + (t4 * 4) % (3 * K);
                float4 v = make_float4(t[0], t[1], t[2], t[3]);
                if (OVERWRITE && !lv) v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (!OVERWRITE) {
                    const float4 o = dst[i4];
                    if (a.sgd_scale != 0.0f) { v.x = fmaf(a.sgd_scale, v.x, o.x); v.y = fmaf(a.sgd_scale, v.y, o.y); v.z = fmaf(a.sgd_scale, v.z, o.z); v.w = fmaf(a.sgd_scale, v.w, o.w); }
                    else { v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
                }
                if (OVERWRITE && GS_NT_STORES) {
                    // streamed past the caches: 192 B per gaussian that nothing on the GPU reads again this frame.  Stored normally they
                    // pushed the model's SH rows out of the 256 MB infinity cache, and the next frame's preprocess fetched them from
                    // HBM again (C3: preprocess 86 -> 73 us, same box, profiles/r04t_ab_nontemporal.log).  (Accumulating views read the
                    // rows back: cached stores.)
                    typedef float v4f __attribute__((ext_vector_type(4)));
                    const v4f vv = {v.x, v.y, v.z, v.w};
                    __builtin_nontemporal_store(vv, reinterpret_cast<v4f *>(dst) + i4);
                } else dst[i4] = v;
            }
        } else {
            for (int idx = threadIdx.x; idx < nb * 3 * K; idx += blockDim.x) {
                const bool lv = srow_live[idx / (3 * K)] != 0;
                if ((!OVERWRITE || a.shs_zeroed) && !lv) continue;
                const float v = (OVERWRITE && !lv) ? 0.0f : tile[(idx / (3 * K)) * ROW + idx % (3 * K)];
                const int64_t gi = gs_sh_row_index<3 * K, STRIDED>(gb, RS, idx);
                if (OVERWRITE) a.d_shs[gi] = v;
                else if (a.sgd_scale != 0.0f) a.d_shs[gi] = fmaf(a.sgd_scale, v, a.d_shs[gi]);
                else a.d_shs[gi] += v;
            }
        }
        if constexpr (STRIDED && OVERWRITE) {
            // the inactive floats of EVERY row, touched or not, end as + 0 (a.shs_zeroed: the fill workgroups wrote all of d_shs already)
            if (!a.shs_zeroed) gs_sh_zero_inactive<3 * K>(a.d_shs, gb, nb, RS);
        }
    }
}

template <bool OVERWRITE>
__global__ __launch_bounds__(256) void gs_geom_bwd_kernel(GsPreprocessBwdArgs a, GsCamera cam) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;
    float g2f[10];
    gs_g2d_row_load(a, g, g2f);         // colour gradient + raw moments (gs_common.h: gs_g2d_to_grads)
#define GS_GEOM_DPC (reinterpret_cast<const float4 *>(a.dpc)[g])
    do {
#include "gs_geom_bwd_body.inc"
    } while (0);
#undef GS_GEOM_DPC
}

// ---------------------------------------------------------------- colour-factored gradient exchange (multi-GPU)
// d L / d sh[k][c] of one view is basis_k(dir_view) * d rgb[c]: rank one in (k, c).  A multi-view step therefore need
// not all-reduce the 3K floats per gaussian (48 at degree 3 = 81 % of the gradient buffer): ranks exchange the THREE
// floats d rgb per (view, gaussian) -- an all-gather of 12 B instead of an all-reduce of 192 B per gaussian -- and
// every rank rebuilds sum_v basis(dir_v) (x) d rgb_v locally from the cameras it already knows.
__global__ __launch_bounds__(256) void gs_pack_drgb_kernel(const float *__restrict__ g2d, const long long *__restrict__ g2d_fixed,
                                                            float *__restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // over 3n
    if (i >= 3 * n) return;
    const int64_t g = i / 3; const int c = (int)(i - 3 * g);
    __builtin_assume(c < 3);                                               // (one fixed-point scale for the three: no select)
    out[i] = gs_g2d_load(GsG2dRows{g2d, g2d_fixed}, g, c);
}

// cams: nviews records of 38 floats {T[16], P[16], eye[3], lookAt[3]}; drgb: [nviews][3n]; the direction and the
// basis are those of gs_sh_bwd_kernel (one basis text, gs_sh_basis.inc; this kernel lets the compiler fuse it, that one does not).  The body
// (gs_sh_views_body.inc) is shared with the kernel that reads the views' colour gradients from bitmaps and compacted rows (gs_touched.hip).
template <int DEG, bool OVERWRITE, bool STRIDED = false>
__global__ __launch_bounds__(256) void gs_sh_from_views_kernel(int64_t n, const float *__restrict__ means, int nviews,
                                                                const float *__restrict__ cams, const float *__restrict__ drgb,
                                                                float *__restrict__ d_shs, int sh_stride) {
#define GS_SH_VIEWS_BEGIN
#define GS_SH_VIEWS_DRGB const float *gr = drgb + (size_t)v * 3 * (size_t)n + 3 * g; const float g0 = gr[0], g1 = gr[1], g2 = gr[2];
#include "gs_sh_views_body.inc"
#undef GS_SH_VIEWS_DRGB
#undef GS_SH_VIEWS_BEGIN
}

hipError_t gs_launch_pack_drgb(const float *g2d, const long long *g2d_fixed, float *out, int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_pack_drgb_kernel, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, s, g2d, g2d_fixed, out, n);
    return hipGetLastError();
}

// sh_degree: the ACTIVE degree; sh_stride: floats per stored row of d_shs (3 K, or more: the strided instantiations, degrees 0..2)
hipError_t gs_launch_sh_from_views(int64_t n, int sh_degree, int sh_stride, const float *means, int nviews, const float *cams, const float *drgb,
                                   float *d_shs, int overwrite, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const dim3 block(256), grid((unsigned)((n + 255) / 256));
    return gs_sh_dispatch(sh_degree, sh_stride, [&](auto D, auto S) {
        constexpr int DEG = decltype(D)::value, K = (DEG + 1) * (DEG + 1);
        constexpr bool STRIDED = decltype(S)::value;
        const size_t lds = sizeof(float) * 256 * (3 * K + 1);
        if (overwrite) hipLaunchKernelGGL((gs_sh_from_views_kernel<DEG, true, STRIDED>), grid, block, lds, s, n, means, nviews, cams, drgb, d_shs, sh_stride);
        else hipLaunchKernelGGL((gs_sh_from_views_kernel<DEG, false, STRIDED>), grid, block, lds, s, n, means, nviews, cams, drgb, d_shs, sh_stride);
        return hipGetLastError();
    });
}

// gaussians per workgroup of the SH kernel: its LDS tile is (3K + 1) floats per gaussian (49 at SH degree 3), so 256 gaussians
// allow three workgroups per CU, 128 six (64 / 128 / 256 measured equal: profiles/HISTORY.md)
#ifndef GS_SHBWD_THREADS
#define GS_SHBWD_THREADS 256
#endif
static int sh_bwd_threads() { return GS_SHBWD_THREADS; }
hipError_t gs_launch_preprocess_bwd(const GsPreprocessBwdArgs &a, const GsCamera &cam, hipStream_t s, const GsPreprocessBwdMode &mode) {
    if (a.n <= 0) return hipSuccess;
    const int phases = mode.phases, adam_mode = mode.adam_mode;
    const GsAdamFused *adam = mode.adam;
    const GsAdamFused ad = adam ? *adam : GsAdamFused{};
    if (adam_mode && (!adam || !a.overwrite || (phases & 3) != 3 || (adam_mode != 1 && adam_mode != 2))) return hipErrorInvalidValue;
    const bool fused = (phases & 3) == 3;
    // a.sh_degree: the ACTIVE degree (the tile holds the bands evaluated); a.sh_stride above 3 K: an active degree below the stored one
    const hipError_t e = gs_sh_dispatch(a.sh_degree, a.sh_stride, [&](auto D, auto S) {
        constexpr int DEG = decltype(D)::value, K = (DEG + 1) * (DEG + 1);
        constexpr bool STRIDED = decltype(S)::value;
        const int T = sh_bwd_threads();
        const dim3 block(T), grid((unsigned)((a.n + T - 1) / T));
        const size_t lds = sizeof(float) * T * (3 * K + 1);
        auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, lds, s, a, cam, ad); };
        if (adam_mode == 2) launch(gs_sh_bwd_kernel<DEG, true, true, 2, STRIDED>);      // fused backward + Adam: one launch, both phases
        else if (adam_mode) launch(gs_sh_bwd_kernel<DEG, true, true, 1, STRIDED>);
        else if (phases & 1) {                                          // (not: the geometry chain alone; degree and stride are checked all the same)
            if (a.overwrite && fused) launch(gs_sh_bwd_kernel<DEG, true, true, 0, STRIDED>);
            else if (a.overwrite) launch(gs_sh_bwd_kernel<DEG, true, false, 0, STRIDED>);
            else if (fused) launch(gs_sh_bwd_kernel<DEG, false, true, 0, STRIDED>);
            else launch(gs_sh_bwd_kernel<DEG, false, false, 0, STRIDED>);
        }
        return hipSuccess;
    });
    if (e != hipSuccess) return e;
    if ((phases & 2) && !fused) {
        const dim3 block(256), grid((unsigned)((a.n + 255) / 256));
        if (a.overwrite) hipLaunchKernelGGL(gs_geom_bwd_kernel<true>, grid, block, 0, s, a, cam);
        else hipLaunchKernelGGL(gs_geom_bwd_kernel<false>, grid, block, 0, s, a, cam);
    }
    return hipGetLastError();
}
