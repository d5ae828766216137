// gs_camera.hip -- the camera gradient of a frame (include/gsplat.h: gs_backward_camera): the 40 sums over the gaussians of the statement
// in gs_camera_grad.h.  Two kernels, no atomics, no counters, no hand-off between workgroups inside a launch -- the 40 floats are a pure
// function of the rows, the model and the camera, bit-reproducible whatever the dispatch order:
//   gs_camera_grad_kernel         one thread per gaussian, 256 per workgroup: the statement's 21 factors, then the 40 values through
//                                 gs_block_tree_row (gs_wave.h) into one row of 40 doubles per workgroup.  Never 40 live fp64 values: a value
//                                 is formed from its two factors when its turn comes.  Threads past n contribute + 0.
//   gs_camera_grad_finish_kernel  one workgroup: gs_tree_finish_rows (gs_wave.h); each sum is rounded to float once and stored.
// Built with -ffp-contract=off (gaussiansplat_amd/build.py); the statement turns contraction off itself.
#include "gs_camera_grad.h"
#include "gs_sh.h"             // gs_sh_dispatch: the instantiation from (active degree, row stride)
#include "gs_wave.h"           // gs_block_tree_row, gs_tree_finish_rows: the fixed tree

#pragma clang fp contract(off)

template <int DEG>
__global__ __launch_bounds__(256) void gs_camera_grad_kernel(GsCameraGradArgs a, GsCamera cam) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    GsCameraGradFactors f{};
    if (g < a.n) {
        float g2f[10];
        gs_g2d_row_load(a, g, g2f);
        gs_camera_grad_factors<DEG>(g2f, a.means + 3 * g, a.scales + 3 * g, a.quats + 4 * g, a.opac + g, a.shs + (int64_t)a.sh_stride * g, cam, f);
    }
    gs_block_tree_row<GS_CAMERA_GRAD_VALUES, 4>([&](int c) { return gs_camera_grad_value(f, c); },
                                                [&](int c, double s) { a.partials[(size_t)blockIdx.x * GS_CAMERA_GRAD_VALUES + c] = s; });
}

__global__ __launch_bounds__(256) void gs_camera_grad_finish_kernel(const double *__restrict__ partials, int64_t rows, float *__restrict__ out) {
    gs_tree_finish_rows<GS_CAMERA_GRAD_VALUES, 256>(partials, rows, [&](int c, double s) { out[c] = (float)s; });   // 320 r bytes: 16-byte aligned rows
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
