// gs_features.hip -- the per-gaussian kernels of the feature maps (include/gsplat.h: gs_view_depth, gs_render_features,
// gs_backward_features, gs_view_depth_backward).  Three streaming kernels, HBM-bound, no LDS, no atomics:
//   gs_view_depth_kernel        z[g] = ts[2] of the preprocess (gs_features.h: the statement, once), one gaussian per lane: 12 B in, 4 B out
//   gs_view_depth_bwd_kernel    d_means[3 g + j] += T[2 + 4 j] * dz[g], one gaussian per lane; rows whose dz compares == 0 are not read
//   gs_feature_payload_kernel   the frame's 64-byte payload rows copied with r, g, b replaced: FOUR lanes per row, one 16-byte quad each, so
//                               that lane i of a wave reads and writes base + 16 i -- 1 KiB per instruction, the widest coalesced access.  One
//                               lane per row would have made every instruction touch 64 rows' worth of 64-byte segments at a 64-byte stride.
//                               Quads 0, 1 and 3 pass through as bits; quad 2 = {r, g, b, ylo} takes the three features and keeps ylo.
// Built with -ffp-contract=off (gaussiansplat_amd/build.py): the depth equals GS_ARR_TS row 2 bit for bit.
#include "gs_features.h"

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void gs_view_depth_kernel(const float *__restrict__ means, int64_t n, GsCamera cam, float *__restrict__ z) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    z[g] = gs_view_depth_of(cam.T, means[3 * g], means[3 * g + 1], means[3 * g + 2]);
}

__global__ __launch_bounds__(256) void gs_view_depth_bwd_kernel(const float *__restrict__ dz, int64_t n, GsCamera cam, float *__restrict__ d_means) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const float d = dz[g];
    if (d == 0.0f) return;                                                 // untouched: a gradient of exactly zero is added to nothing
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float v = cam.T[2 + 4 * j] * d;
        d_means[3 * g + j] = d_means[3 * g + j] + v;
    }
}

static_assert(offsetof(GsPayload, r) == 32 && offsetof(GsPayload, g) == 36 && offsetof(GsPayload, b) == 40 && offsetof(GsPayload, ylo) == 44,
              "the colour floats are the first three words of quad 2");
__global__ __launch_bounds__(256) void gs_feature_payload_kernel(const uint4 *__restrict__ src, const float *__restrict__ feat, int64_t n,
                                                                 uint4 *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // over the 4 n quads
    if (i >= 4 * n) return;
    uint4 q = src[i];
    if ((i & 3) == 2) {
        const int64_t g = i >> 2;
        q.x = __float_as_uint(feat[3 * g]); q.y = __float_as_uint(feat[3 * g + 1]); q.z = __float_as_uint(feat[3 * g + 2]);
    }
    dst[i] = q;
}

static dim3 blocks_for(int64_t items) { return dim3((unsigned)((items + 255) / 256)); }

hipError_t gs_launch_view_depth(const float *means, int64_t n, const GsCamera &cam, float *z, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_view_depth_kernel, blocks_for(n), dim3(256), 0, s, means, n, cam, z);
    return hipGetLastError();
}

hipError_t gs_launch_view_depth_bwd(const float *dz, int64_t n, const GsCamera &cam, float *d_means, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_view_depth_bwd_kernel, blocks_for(n), dim3(256), 0, s, dz, n, cam, d_means);
    return hipGetLastError();
}

hipError_t gs_launch_feature_payload(const GsPayload *src, const float *feat, int64_t n, GsPayload *dst, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (4 * n > 0xFFFFFFFFll * 256) return hipErrorInvalidValue;           // (beyond a one-dimensional grid: 2.7e11 gaussians)
    hipLaunchKernelGGL(gs_feature_payload_kernel, blocks_for(4 * n), dim3(256), 0, s, reinterpret_cast<const uint4 *>(src), feat, n,
                       reinterpret_cast<uint4 *>(dst));
    return hipGetLastError();
}
