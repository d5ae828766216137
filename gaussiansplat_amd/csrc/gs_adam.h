// gs_adam.h -- the per-float Adam update shared by the standalone step (gs_adam.hip) and the fused backward + Adam
// (gs_sh_bwd_kernel, gs_geom_bwd_body.inc).  One function for both paths is what makes gs_backward_adam bit-identical to
// gs_backward_ex(GS_BWD_OVERWRITE) followed by gs_adam_step.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define GS_ADAM_NGROUPS 6

// the scalars of one step, each computed by the host in double and rounded to float once (gs_adam_hyper, gs_adam.hip)
struct GsAdamHyper {
    float beta1, beta2;
    float omb1, omb2;                        // 1 - beta1, 1 - beta2
    float eps;
    float sqrt_bc2;                          // sqrt(1 - beta2^t)
    float step_size[GS_ADAM_NGROUPS];        // lr[grp] / (1 - beta1^t)
};

// the fused path's extra kernel argument: first and second moments of the five parameter arrays
struct GsAdamFused {
    float *m[5], *v[5];
    GsAdamHyper h;
};

// group of float j (0 .. w - 1) of a row of the fifth array: SH band 0 (the first three floats) -> 4, higher bands -> 5.
// The 2-D renderer's colours (w = 3) all fall in group 4.
__host__ __device__ inline int gs_adam_sh_group(int j) { return j < 3 ? 4 : 5; }

// torch's order of operations, in float32 with no fma contraction; sqrtf and '/' are the correctly rounded forms (hipcc's
// default -fhip-fp32-correctly-rounded-divide-sqrt: v_div_scale / v_div_fmas / v_div_fixup and the scaled v_sqrt with its fma
// correction, not a bare v_rcp_f32 / v_sqrt_f32).  (__fsqrt_rn is NOT used: without OCML_BASIC_ROUNDED_OPERATIONS the HIP headers
// map it to the approximate native sqrt.)
__device__ __forceinline__ void gs_adam_update(float &p, float &m, float &v, float g, const GsAdamHyper &h, float step_size) {
#pragma clang fp contract(off)
    m = h.beta1 * m + h.omb1 * g;
    v = h.beta2 * v + (h.omb2 * g) * g;
    const float den = sqrtf(v) / h.sqrt_bc2 + h.eps;
    p = p - step_size * (m / den);
}

// host (gs_adam.hip): the checks shared by gs_adam_step and gs_backward_adam, and the step's scalars.  g == NULL: the fused form
// (every group stepped, no gradient arrays).  On failure nothing has been enqueued.
struct gs_ctx;
// ... and the part of it that every Adam step shares, gs_exposure_adam included: the refusals of step, betas, eps and the nlr rates, then
// the scalars, each in double and rounded to float once (step_size[i] from lr[i], i < nlr; the rest 0)
int gs_adam_scalars(struct gs_ctx *c, const char *who, const float *lr, int nlr, float beta1, float beta2, float eps, int64_t step, GsAdamHyper *h);
int gs_adam_prepare(struct gs_ctx *c, const char *who, const float *const p[5], const float *const g[5], float *const m[5], float *const v[5],
                    const float *lr, float beta1, float beta2, float eps, int64_t step, int flags, GsAdamHyper *h);
