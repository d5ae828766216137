// gs_camera.hip -- the camera gradient of a frame (include/gsplat.h: gs_backward_camera): the 40 sums over the gaussians of the statement
// in gs_camera_grad.h.  Two kernels, no atomics, no counters, no hand-off between workgroups inside a launch -- the 40 floats are a pure
// function of the rows, the model and the camera, bit-reproducible whatever the dispatch order:
//   gs_camera_grad_kernel         one thread per gaussian, 256 per workgroup: the statement's 21 factors, then the 40 values ONE AFTER
//                                 ANOTHER through a fixed tree -- a butterfly over the wave (gs_wave_sum: DPP inside a row of 16 lanes, shuffles
//                                 of the two 32-bit halves across rows), lane 0 of each of the four waves into LDS, and behind one
//                                 barrier (w0 + w1) + (w2 + w3) -- into one row of 40 doubles per workgroup.  Never 40 live fp64 values:
//                                 a value is formed from its two factors when its turn comes.  Threads past n contribute + 0.
//   gs_camera_grad_finish_kernel  one workgroup: thread i sums the rows i, i + 256, ... in that order, then the same tree; each sum is rounded
//                                 to float once and stored.
// Built with -ffp-contract=off (gaussiansplat_amd/build.py); the statement turns contraction off itself.
#include "gs_camera_grad.h"
#include "gs_sh.h"             // gs_sh_dispatch: the instantiation from (active degree, row stride)
#include "gs_wave_sum.h"       // gs_wave_sum: the fixed tree over the wave

#pragma clang fp contract(off)

template <int DEG>
__global__ __launch_bounds__(256) void gs_camera_grad_kernel(GsCameraGradArgs a, GsCamera cam) {
    __shared__ double swave[GS_CAMERA_GRAD_VALUES][4];
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    GsCameraGradFactors f{};
    if (g < a.n) {
        float g2f[10];
        gs_g2d_row_load(a, g, g2f);
        gs_camera_grad_factors<DEG>(g2f, a.means + 3 * g, a.scales + 3 * g, a.quats + 4 * g, a.opac + g, a.shs + (int64_t)a.sh_stride * g, cam, f);
    }
#pragma unroll
    for (int c = 0; c < GS_CAMERA_GRAD_VALUES; ++c) {
        const double s = gs_wave_sum(gs_camera_grad_value(f, c));
        if (lane == 0) swave[c][wv] = s;
    }
    __syncthreads();
    if (threadIdx.x < GS_CAMERA_GRAD_VALUES) {
        const double *w = swave[threadIdx.x];
        a.partials[(size_t)blockIdx.x * GS_CAMERA_GRAD_VALUES + threadIdx.x] = (w[0] + w[1]) + (w[2] + w[3]);
    }
}

__global__ __launch_bounds__(256) void gs_camera_grad_finish_kernel(const double *__restrict__ partials, int64_t rows, float *__restrict__ out) {
    __shared__ double swave[GS_CAMERA_GRAD_VALUES][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    static_assert(GS_CAMERA_GRAD_VALUES % 2 == 0, "two columns per 16-byte load");
    // One pass over the rows with 40 accumulators: the twenty 16-byte loads of a row are independent, so a thread waits for memory once
    // per row it owns and not once per row and group of columns (at 1 M gaussians 3 907 rows: 16 round trips per thread instead of 80).
    // One workgroup on the whole chip: its registers cost nobody anything.
    double acc[GS_CAMERA_GRAD_VALUES];
#pragma unroll
    for (int c = 0; c < GS_CAMERA_GRAD_VALUES; ++c) acc[c] = 0.0;
    for (int64_t r = threadIdx.x; r < rows; r += 256) {
        const double2 *row = reinterpret_cast<const double2 *>(partials + (size_t)r * GS_CAMERA_GRAD_VALUES);   // 320 r bytes: 16-byte aligned
#pragma unroll
        for (int q = 0; q < GS_CAMERA_GRAD_VALUES / 2; ++q) { const double2 v = row[q]; acc[2 * q] = acc[2 * q] + v.x; acc[2 * q + 1] = acc[2 * q + 1] + v.y; }
    }
#pragma unroll
    for (int c = 0; c < GS_CAMERA_GRAD_VALUES; ++c) {
        const double s = gs_wave_sum(acc[c]);
        if (lane == 0) swave[c][wv] = s;
    }
    __syncthreads();
    if (threadIdx.x < GS_CAMERA_GRAD_VALUES) {
        const double *w = swave[threadIdx.x];
        out[threadIdx.x] = (float)((w[0] + w[1]) + (w[2] + w[3]));
    }
}

hipError_t gs_launch_camera_grad(const GsCameraGradArgs &a, const GsCamera &cam, float *out, hipStream_t s) {
    const int64_t rows = gs_camera_grad_rows(a.n);
    if (rows > 0x7FFFFFFFll) return hipErrorInvalidValue;                  // (beyond a one-dimensional grid: 5.5e11 gaussians)
    if (rows > 0) {
        const hipError_t e = gs_sh_dispatch(a.sh_degree, a.sh_stride, [&](auto D, auto) {
            hipLaunchKernelGGL(gs_camera_grad_kernel<decltype(D)::value>, dim3((unsigned)rows), dim3(256), 0, s, a, cam);
            return hipGetLastError();
        });
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(gs_camera_grad_finish_kernel, dim3(1), dim3(256), 0, s, a.partials, rows, out);   // rows == 0: 40 x + 0
    return hipGetLastError();
}
