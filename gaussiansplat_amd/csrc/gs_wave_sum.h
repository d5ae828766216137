// gs_wave_sum.h -- the sum of a double over the wave's 64 lanes in a fixed tree, written ONCE for the reductions that must be bitwise
// reproducible: the camera gradient (gs_camera.hip) and the exposure gradient (gs_exposure.hip).  Device only.
#pragma once
#include <hip/hip_runtime.h>

// a double moved across lanes by a DPP control, as its two 32-bit halves
template <int CTRL>
__device__ __forceinline__ double gs_dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
// The sum over the wave's 64 lanes in a fixed tree; every lane returns it.  Inside a row of 16 lanes the partner comes by DPP (two moves on
// the vector unit): lane ^ 1, lane ^ 2 (quad_perm), then the mirror image inside 8 and inside 16 lanes -- after the first two steps the
// four lanes of a quad hold the same sum, so the mirror pairs quad with quad, and then half with half.  Across rows: __shfl_xor by 16
// and 32 (ds_bpermute_b32 of the two halves).  Both partners of a pair form a + b and b + a: the same bits.
__device__ __forceinline__ double gs_wave_sum(double v) {
#pragma clang fp contract(off)
    v = v + gs_dpp_f64<0xB1>(v);           // quad_perm [1, 0, 3, 2]
    v = v + gs_dpp_f64<0x4E>(v);           // quad_perm [2, 3, 0, 1]
    v = v + gs_dpp_f64<0x141>(v);          // row_half_mirror
    v = v + gs_dpp_f64<0x140>(v);          // row_mirror
    v = v + __shfl_xor(v, 16, 64);
    v = v + __shfl_xor(v, 32, 64);
    return v;
}
