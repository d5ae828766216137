// gs_features.h -- feature maps (include/gsplat.h: gs_view_depth, gs_render_features, gs_backward_features, gs_view_depth_backward):
// the one statement of a gaussian's view-space depth, and the launchers of the per-gaussian kernels around the feature payload
// (gs_features.hip).  The depth is __host__ __device__ with contraction off inside its body, as the statements of gs_pergaussian.h are:
// tests/features_host.cpp runs it on the CPU, against the oracle's ts[2], bit for bit.
#pragma once
#include "gs_common.h"

// ts[2] of the preprocess (gs_preprocess.hip; frustumCulling, projection.jl:46-93): row 2 of t = T [m; 1], T column major, every step a
// single fp32 operation in the written order.  Non-finite means pass through as IEEE gives them.
__host__ __device__ __forceinline__ float gs_view_depth_of(const float *T, float m1, float m2, float m3) {
#pragma clang fp contract(off)
    float s = T[2] * m1;
    s = s + T[6] * m2;
    s = s + T[10] * m3;
    s = s + T[14] * 1.0f;
    return s;
}

// launchers (each enqueues on `stream`, returns hipGetLastError()); n == 0: nothing is launched
// z[g] = gs_view_depth_of(cam.T, means[3 g ..])
hipError_t gs_launch_view_depth(const float *means, int64_t n, const GsCamera &cam, float *z, hipStream_t s);
// d_means[3 g + j] = d_means[3 g + j] + (T[2 + 4 j] * dz[g]), one multiply and one add; a dz[g] that compares == 0 leaves the row unread
hipError_t gs_launch_view_depth_bwd(const float *dz, int64_t n, const GsCamera &cam, float *d_means, hipStream_t s);
// dst[g] = src[g] with (r, g, b) = feat[3 g ..]; the other 52 bytes of the row bit for bit.  src and dst: 16-byte aligned rows, not overlapping
hipError_t gs_launch_feature_payload(const GsPayload *src, const float *feat, int64_t n, GsPayload *dst, hipStream_t s);
