// gs_background.hip -- the background colour: what the forward adds behind the last splat, and the target image composited over the same colour.
//
// The composite kernels leave C = sum c_i alpha_i T_i in the image and T = prod (1 - alpha_i) beside it (reference src/splat.jl:224-261 has no
// background: every frame stands on black).  Over a background the frame is C + T bg, and because the composite backward seeds its suffix
// sums from the image it finds (gs_composite.hip: S = image . dC), an image that already carries T bg gives every dL/dalpha_i its background
// term -T_final (bg . dC) / (1 - alpha_i) with no change to that kernel: the blend is an epilogue of the forward and nothing else.
//
// Two elementwise kernels over pixel planes, no LDS, no atomics.  A thread takes four consecutive pixels, one 16-byte access per plane, when
// the plane length is a multiple of four and every base pointer is 16-byte aligned (then every plane start is too); one pixel otherwise.
// Rounding contract (include/gsplat.h): every operation below is ONE fp32 operation, rounded on its own, in the order written -- this
// translation unit is built with -ffp-contract=off and says so itself, so NumPy in float32 reproduces both kernels bit for bit.
#include "gs_common.h"
#pragma clang fp contract(off)

namespace {

constexpr int BG_THREADS = 256;

struct Bg3 { float c[3]; };

__device__ inline float blend1(float c, float t, float bg) {
    const float tb = t * bg;
    return c + tb;
}
__device__ inline float4 blend4(float4 c, float4 t, float bg) {
    return make_float4(blend1(c.x, t.x, bg), blend1(c.y, t.y, bg), blend1(c.z, t.z, bg), blend1(c.w, t.w, bg));
}
__device__ inline float over1(float c, float a, float bg) {
    const float ca = c * a;
    const float na = 1.0f - a;
    const float bn = bg * na;
    return ca + bn;
}
__device__ inline float4 over4(float4 c, float4 a, float bg) {
    return make_float4(over1(c.x, a.x, bg), over1(c.y, a.y, bg), over1(c.z, a.z, bg), over1(c.w, a.w, bg));
}

// image[c][p] += trans[p] * bg[c], three planes of `px` pixels; VEC: units of four pixels (px % 4 == 0, 16-byte aligned bases)
template <bool VEC>
__global__ __launch_bounds__(BG_THREADS) void gs_blend_background_kernel(float *__restrict__ image, const float *__restrict__ trans, size_t px, Bg3 bg) {
    const size_t i = (size_t)blockIdx.x * BG_THREADS + threadIdx.x;
    if (VEC) {
        if (i >= px / 4) return;
        const float4 t = reinterpret_cast<const float4 *>(trans)[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float4 *plane = reinterpret_cast<float4 *>(image + (size_t)c * px);
            plane[i] = blend4(plane[i], t, bg.c[c]);
        }
    } else {
        if (i >= px) return;
        const float t = trans[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) image[(size_t)c * px + i] = blend1(image[(size_t)c * px + i], t, bg.c[c]);
    }
}

// out[c][p] = rgba[c][p] * a + bg[c] * (1 - a), a = rgba[3][p]: straight alpha, planar in and out
template <bool VEC>
__global__ __launch_bounds__(BG_THREADS) void gs_compose_target_kernel(const float *__restrict__ rgba, float *__restrict__ out, size_t px, Bg3 bg) {
    const size_t i = (size_t)blockIdx.x * BG_THREADS + threadIdx.x;
    if (VEC) {
        if (i >= px / 4) return;
        const float4 a = reinterpret_cast<const float4 *>(rgba + 3 * px)[i];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            reinterpret_cast<float4 *>(out + (size_t)c * px)[i] = over4(reinterpret_cast<const float4 *>(rgba + (size_t)c * px)[i], a, bg.c[c]);
    } else {
        if (i >= px) return;
        const float a = rgba[3 * px + i];
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(size_t)c * px + i] = over1(rgba[(size_t)c * px + i], a, bg.c[c]);
    }
}

inline bool quads_ok(size_t px, const void *p0, const void *p1) {
    return px % 4 == 0 && (((uintptr_t)p0 | (uintptr_t)p1) & 15u) == 0;
}
inline unsigned blocks_for(size_t units) { return (unsigned)((units + BG_THREADS - 1) / BG_THREADS); }   // (images end at 32767^2 pixels: 4.2 M blocks at most)

}  // namespace

hipError_t gs_launch_blend_background(float *image, const float *trans, size_t px, const float bg[3], hipStream_t s) {
    if (px == 0) return hipSuccess;
    const Bg3 b{{bg[0], bg[1], bg[2]}};
    if (quads_ok(px, image, trans)) hipLaunchKernelGGL(gs_blend_background_kernel<true>, dim3(blocks_for(px / 4)), dim3(BG_THREADS), 0, s, image, trans, px, b);
    else hipLaunchKernelGGL(gs_blend_background_kernel<false>, dim3(blocks_for(px)), dim3(BG_THREADS), 0, s, image, trans, px, b);
    return hipGetLastError();
}

hipError_t gs_launch_compose_target(const float *rgba, float *out, size_t px, const float bg[3], hipStream_t s) {
    if (px == 0) return hipSuccess;
    const Bg3 b{{bg[0], bg[1], bg[2]}};
    if (quads_ok(px, rgba, out)) hipLaunchKernelGGL(gs_compose_target_kernel<true>, dim3(blocks_for(px / 4)), dim3(BG_THREADS), 0, s, rgba, out, px, b);
    else hipLaunchKernelGGL(gs_compose_target_kernel<false>, dim3(blocks_for(px)), dim3(BG_THREADS), 0, s, rgba, out, px, b);
    return hipGetLastError();
}
