// gs_sh.h -- what the kernels that evaluate spherical harmonics share: the constants, the choice of an instantiation from (active degree,
// row stride), and the addressing of strided rows.  The basis itself is gs_sh_basis.inc, its derivative gs_sh_ddir.inc (text: see there).
//
// The coefficient arrays are `inline __constant__`: ONE definition for every translation unit of the library (no host symbol, nothing
// registered twice) that the kernels LOAD.  Not `static __constant__`: the compiler then folds the values into the instruction stream and
// every kernel of degree >= 2 changes its code and its register counts (profiles/HISTORY.md).  The forward (bit-identical to the CPU
// oracle), the backward and the two kernels that rebuild SH gradients from views must see the same values and the same basis text: each
// rounds it as its own scope says, and the two rebuild kernels (same flags in build.py) round alike.
#pragma once
#include "gs_common.h"
#include <type_traits>

#define SH_C0 0.28209479177387814f
#define SH_C1 0.48860251190291990f
// each list of literals stands ONCE: the device arrays below, and the constexpr doubles of gs_camera_grad.h (the same floats, widened)
#define GS_SH_C2_VALUES 1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f
#define GS_SH_C3_VALUES -0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f, \
                        -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f
inline __constant__ float bC2[5] = {GS_SH_C2_VALUES};
inline __constant__ float bC3[7] = {GS_SH_C3_VALUES};

// The instantiation of an SH kernel.  active_degree: the bands evaluated, 0..3; row_stride: floats per stored row, 3 K = 3 (active_degree + 1)^2
// or more -- more is an active degree below the stored one, hence 0..2 only (the STRIDED instantiations).  Anything else: hipErrorInvalidValue
// and nothing is launched.  Else returns f(std::integral_constant<int, DEG>, std::bool_constant<STRIDED>).
template <class F>
inline hipError_t gs_sh_dispatch(int active_degree, int row_stride, F &&f) {
    if (active_degree < 0 || active_degree > 3) return hipErrorInvalidValue;
    const int K3 = 3 * (active_degree + 1) * (active_degree + 1);
    if (row_stride < K3 || (row_stride > K3 && active_degree == 3)) return hipErrorInvalidValue;
    const bool strided = row_stride > K3;
    using std::integral_constant;
    switch (active_degree) {
        case 0: return strided ? f(integral_constant<int, 0>{}, std::true_type{}) : f(integral_constant<int, 0>{}, std::false_type{});
        case 1: return strided ? f(integral_constant<int, 1>{}, std::true_type{}) : f(integral_constant<int, 1>{}, std::false_type{});
        case 2: return strided ? f(integral_constant<int, 2>{}, std::true_type{}) : f(integral_constant<int, 2>{}, std::false_type{});
        default: return f(integral_constant<int, 3>{}, std::false_type{});
    }
}

// A workgroup's rows start at row gb; K3 = 3 K floats of a row are active, the rows RS floats apart (STRIDED) or K3.
// Where float idx of the active floats, counted through the workgroup's rows, sits in global memory:
template <int K3, bool STRIDED>
__device__ __forceinline__ int64_t gs_sh_row_index(int64_t gb, int RS, int idx) {
    return STRIDED ? gb * RS + (int64_t)(idx / K3) * RS + idx % K3 : gb * K3 + idx;
}
// + 0 into the inactive floats (K3 .. RS) of the workgroup's nb rows
template <int K3>
__device__ __forceinline__ void gs_sh_zero_inactive(float *d_shs, int64_t gb, int nb, int RS) {
    const int hi = RS - K3;
    for (int c = threadIdx.x; c < nb * hi; c += blockDim.x) d_shs[gb * RS + (int64_t)(c / hi) * RS + K3 + c % hi] = 0.0f;
}
