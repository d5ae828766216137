// gs_exposure.hip -- the per-view exposure stage between the frame and the loss (include/gsplat.h: gs_exposure_apply, gs_exposure_backward,
// gs_exposure_adam): out = w (M rgb + b) per pixel, its adjoint into the image, its adjoint into the 12 floats of E, and the Adam step of
// those 12 floats.  The statements are gs_exposure.h's.  Four kernels, no atomics, no counters, no hand-off between workgroups inside a
// launch; grids and the number of partial rows are functions of (W, H) alone -- every result is bitwise reproducible and independent of
// what the ctx did before.
//   exposure_apply_kernel    streaming: 12 bytes in (+ 4 with a weight), 12 out per pixel.  Lane q of the grid takes the pixels 4 q .. 4 q + 3 of
//                            every plane: one 16-byte access per plane (VEC: W H % 4 == 0, so that the planes, W H floats apart, keep the
//                            alignment of their bases, and every base 16-byte aligned -- there is no tail then), else four 4-byte ones,
//                            which also cover the tail.  E is a device pointer (the row lives in a table that Adam has just stepped): its
//                            address is uniform, so the 12 floats come through the scalar unit once per wave and stay in registers.
//   exposure_bwd_kernel      the same mapping: x, d and the weight in, dx out.  A lane reads its own pixels of d before it writes them, so
//                            d_img == d_out is legal (neither is __restrict__).  WANT_DE: 12 double accumulators per lane over its four
//                            pixels in ascending order, then through gs_block_tree_row (gs_wave.h) into one row of 12 doubles per workgroup.
//                            Lanes past the image add + 0.  Without WANT_DE the instantiation has no double in it.
//   exposure_finish_kernel   one workgroup: gs_tree_finish_rows (gs_wave.h), one rounding to float each.
//   exposure_adam_kernel     one wave, 12 lanes live: gs_adam_update (gs_adam.h) on a row with the scalars of one step.
// The pixel -> lane mapping does not depend on VEC: an unaligned base changes the accesses, not a bit of dE.
// Built with -ffp-contract=off (gaussiansplat_amd/build.py); the statements turn contraction off themselves.
#include "gs_exposure.h"
#include "gs_wave.h"

#include <cstdint>
#include <initializer_list>
#include <type_traits>

#pragma clang fp contract(off)

namespace {

struct Px4 { float v[GS_EXPOSURE_QUAD]; };

// the lane's pixels p0 .. p0 + n - 1 of one plane (n == 4 under VEC); the rest + 0
template <bool VEC>
__device__ __forceinline__ Px4 load4(const float *plane, int p0, int n) {
    Px4 r;
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4 *>(plane + p0);
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < GS_EXPOSURE_QUAD; ++j) r.v[j] = j < n ? plane[p0 + j] : 0.0f;
    }
    return r;
}
template <bool VEC>
__device__ __forceinline__ void store4(float *plane, int p0, int n, const Px4 &r) {
    if (VEC) {
        *reinterpret_cast<float4 *>(plane + p0) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < GS_EXPOSURE_QUAD; ++j)
            if (j < n) plane[p0 + j] = r.v[j];
    }
}
__device__ __forceinline__ void load_row(const float *__restrict__ E, float (&e)[GS_EXPOSURE_FLOATS]) {
#pragma unroll
    for (int i = 0; i < GS_EXPOSURE_FLOATS; ++i) e[i] = E[i];
}

template <bool VEC, bool HAS_W>
__global__ __launch_bounds__(GS_EXPOSURE_BLOCK) void exposure_apply_kernel(const float *__restrict__ img, const float *__restrict__ E,
                                                                           const float *__restrict__ weight, int px, float *__restrict__ out) {
    const int p0 = (blockIdx.x * GS_EXPOSURE_BLOCK + threadIdx.x) * GS_EXPOSURE_QUAD;   // < px + 1024 <= 2^31 / 3 + 1024
    if (p0 >= px) return;
    const int n = min(GS_EXPOSURE_QUAD, px - p0);
    float e[GS_EXPOSURE_FLOATS];
    load_row(E, e);
    const Px4 x0 = load4<VEC>(img, p0, n), x1 = load4<VEC>(img + px, p0, n), x2 = load4<VEC>(img + 2 * (size_t)px, p0, n);
    Px4 w{};
    if (HAS_W) w = load4<VEC>(weight, p0, n);
    Px4 o[3];
#pragma unroll
    for (int j = 0; j < GS_EXPOSURE_QUAD; ++j) {
        const float x[3] = {x0.v[j], x1.v[j], x2.v[j]};
        float a[3];
        if (HAS_W) gs_exposure_forward(e, x, w.v[j], a); else gs_exposure_forward(e, x, a);
        o[0].v[j] = a[0]; o[1].v[j] = a[1]; o[2].v[j] = a[2];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) store4<VEC>(out + r * (size_t)px, p0, n, o[r]);
}

template <bool VEC, bool HAS_W, bool WANT_DE>
__global__ __launch_bounds__(GS_EXPOSURE_BLOCK) void exposure_bwd_kernel(const float *__restrict__ img, const float *d_out, const float *__restrict__ E,
                                                                         const float *__restrict__ weight, int px, float *d_img,
                                                                         double *__restrict__ partials) {
    const int p0 = (blockIdx.x * GS_EXPOSURE_BLOCK + threadIdx.x) * GS_EXPOSURE_QUAD;
    const int n = p0 < px ? min(GS_EXPOSURE_QUAD, px - p0) : 0;
    double acc[GS_EXPOSURE_FLOATS];                          // (dead without WANT_DE)
    if constexpr (WANT_DE) {
#pragma unroll
        for (int i = 0; i < GS_EXPOSURE_FLOATS; ++i) acc[i] = 0.0;
    }
    if (n > 0) {
        float e[GS_EXPOSURE_FLOATS];
        load_row(E, e);
        const Px4 d0 = load4<VEC>(d_out, p0, n), d1 = load4<VEC>(d_out + px, p0, n), d2 = load4<VEC>(d_out + 2 * (size_t)px, p0, n);
        Px4 x0{}, x1{}, x2{}, w{};
        if constexpr (WANT_DE) { x0 = load4<VEC>(img, p0, n); x1 = load4<VEC>(img + px, p0, n); x2 = load4<VEC>(img + 2 * (size_t)px, p0, n); }
        if (HAS_W) w = load4<VEC>(weight, p0, n);
        Px4 o[3];
#pragma unroll
        for (int j = 0; j < GS_EXPOSURE_QUAD; ++j) {
            const float d[3] = {d0.v[j], d1.v[j], d2.v[j]};
            float g[3] = {d[0], d[1], d[2]}, dx[3];
            if (HAS_W) gs_exposure_weigh(d, w.v[j], g);
            gs_exposure_dx(e, g, dx);
            o[0].v[j] = dx[0]; o[1].v[j] = dx[1]; o[2].v[j] = dx[2];
            if constexpr (WANT_DE) if (j < n) {
                const float x[3] = {x0.v[j], x1.v[j], x2.v[j]};
                gs_exposure_dE_add(g, x, acc);
            }
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) store4<VEC>(d_img + r * (size_t)px, p0, n, o[r]);
    }
    if constexpr (WANT_DE) {
        gs_block_tree_row<GS_EXPOSURE_FLOATS, GS_EXPOSURE_BLOCK / 64>([&](int c) { return acc[c]; },
                                                                      [&](int c, double s) { partials[(size_t)blockIdx.x * GS_EXPOSURE_FLOATS + c] = s; });
    }
}

__global__ __launch_bounds__(GS_EXPOSURE_BLOCK) void exposure_finish_kernel(const double *__restrict__ partials, int rows, float *__restrict__ d_exposure) {
    gs_tree_finish_rows<GS_EXPOSURE_FLOATS, GS_EXPOSURE_BLOCK>(partials, rows, [&](int c, double s) { d_exposure[c] = (float)s; });   // 96 r bytes: 16-byte aligned rows
}

__global__ __launch_bounds__(64) void exposure_adam_kernel(float *__restrict__ E, const float *__restrict__ dE, float *__restrict__ m_, float *__restrict__ v_,
                                                           GsAdamHyper h) {
    const int i = threadIdx.x;
    if (i >= GS_EXPOSURE_FLOATS) return;
    float p = E[i], m = m_[i], v = v_[i];
    gs_adam_update(p, m, v, dE[i], h, h.step_size[0]);
    E[i] = p; m_[i] = m; v_[i] = v;
}

bool aligned16(std::initializer_list<const void *> ps) {
    uintptr_t bits = 0;
    for (const void *p : ps) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & 15) == 0;
}

}  // namespace

hipError_t gs_launch_exposure_apply(const float *img, const float *E, const float *weight, int W, int H, float *out, hipStream_t s) {
    const int px = W * H, rows = gs_exposure_rows(W, H);
    const bool vec = px % GS_EXPOSURE_QUAD == 0 && aligned16({img, weight, out});
    auto launch = [&](auto V, auto HW) {
        hipLaunchKernelGGL((exposure_apply_kernel<decltype(V)::value, decltype(HW)::value>), dim3((unsigned)rows), dim3(GS_EXPOSURE_BLOCK), 0, s, img, E, weight, px, out);
    };
    using T = std::true_type; using F = std::false_type;
    if (vec) { if (weight) launch(T{}, T{}); else launch(T{}, F{}); }
    else     { if (weight) launch(F{}, T{}); else launch(F{}, F{}); }
    return hipGetLastError();
}

hipError_t gs_launch_exposure_backward(const float *img, const float *d_out, const float *E, const float *weight, int W, int H, float *d_img,
                                       double *partials, float *d_exposure, hipStream_t s) {
    const int px = W * H, rows = gs_exposure_rows(W, H);
    const bool vec = px % GS_EXPOSURE_QUAD == 0 && aligned16({img, d_out, weight, d_img});
    auto launch = [&](auto V, auto HW, auto DE) {
        hipLaunchKernelGGL((exposure_bwd_kernel<decltype(V)::value, decltype(HW)::value, decltype(DE)::value>), dim3((unsigned)rows), dim3(GS_EXPOSURE_BLOCK), 0, s,
                           img, d_out, E, weight, px, d_img, partials);
    };
    using T = std::true_type; using F = std::false_type;
    auto pick_de = [&](auto V, auto HW) { if (d_exposure) launch(V, HW, T{}); else launch(V, HW, F{}); };
    if (vec) { if (weight) pick_de(T{}, T{}); else pick_de(T{}, F{}); }
    else     { if (weight) pick_de(F{}, T{}); else pick_de(F{}, F{}); }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !d_exposure) return e;
    hipLaunchKernelGGL(exposure_finish_kernel, dim3(1), dim3(GS_EXPOSURE_BLOCK), 0, s, partials, rows, d_exposure);
    return hipGetLastError();
}

hipError_t gs_launch_exposure_adam(float *E, const float *dE, float *m, float *v, const GsAdamHyper &h, hipStream_t s) {
    hipLaunchKernelGGL(exposure_adam_kernel, dim3(1), dim3(64), 0, s, E, dE, m, v, h);
    return hipGetLastError();
}
