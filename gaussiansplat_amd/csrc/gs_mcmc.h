// gs_mcmc.h -- the statements of the MCMC densification strategy ("3D Gaussian Splatting as Markov Chain Monte Carlo", Kheradmand et al. 2024)
// written ONCE and usable from host and device: the kernels of gs_mcmc.hip execute them per gaussian or per draw, tests/mcmc_host.cpp is a host
// build of the same text that tests/test_mcmc_host.py compares with the NumPy restatement of tests/mcmc_ref.py.  Contraction is off in every
// body: one rounding per operation, in the order written.  Semantics: include/gsplat.h, DESIGN.md 5.8l.
//   weight     sig = sigmoid(opacity) (the preprocess's);  alive = opacity > min_opacity_logit (a NaN is not);
//              w = alive && sig finite ? (uint32_t)floorf(sig * 2^24) : 0 -- INTEGERS, so that their prefix sum is exact in any order
//   draw       uc = u clamped into [0, 1 - 2^-24], NaN -> 0;  t = min((uint64_t)((double)uc * (double)total), total - 1);
//              src = the smallest i with cdf[i] > t  (np.searchsorted(cdf, t, side = "right"))
//   relocate   in DOUBLE, for a source drawn c >= 1 times, n = min(c + 1, 51):  o = sig clamped to [0, 1 - 2^-24];  p = -expm1(log1p(-o) / n);
//              s = sum_{i = 1..n} sum_{k = 0..i-1} (B[i-1][k] ((-1)^k / sqrt(k + 1))) p^(k+1);  pc = min(max(p, min_opacity), 1 - 2^-23);
//              opacity' = (float)(log(pc) - log1p(-pc));  scale_j' = (float)((double)scale_j + log(o / s))      (the paper's Eq. 9)
//   noise      all float:  gate = 1 / (1 + exp(gate_k (sig - gate_t)));  e_j = exp(scale_j);  R of the RAW quaternion;
//              a_j = (R[0][j] z0 + R[1][j] z1) + R[2][j] z2;  b_j = (e_j e_j) a_j;  d_i = (R[i][0] b_0 + R[i][1] b_1) + R[i][2] b_2;
//              mean_i' = mean_i + (lr gate) d_i -- all three, or none when one of them would not be finite
//   regulariser  d_opacity += c_o (sig (1 - sig));  d_scale_j += c_s exp(scale_j)
#pragma once
#include "gs_pergaussian.h"
#include <math.h>

#define GS_MCMC_NMAX 51                   // rows of the binomial table: a source counts as drawn at most 50 times
#define GS_MCMC_BINOM (GS_MCMC_NMAX * GS_MCMC_NMAX)
#define GS_MCMC_W_ONE 16777216.0f         // 2^24: the weight of sig = 1

// Pascal's triangle in double, row-major [GS_MCMC_NMAX][GS_MCMC_NMAX]: B[i][k] = C(i, k), 0 above the diagonal.  Exact: C(50, 25) < 2^53.
inline void gs_mcmc_binom_fill(double *B) {
    for (int i = 0; i < GS_MCMC_NMAX; ++i)
        for (int k = 0; k < GS_MCMC_NMAX; ++k)
            B[i * GS_MCMC_NMAX + k] = k > i ? 0.0 : (k == 0 || k == i) ? 1.0 : B[(i - 1) * GS_MCMC_NMAX + k - 1] + B[(i - 1) * GS_MCMC_NMAX + k];
}

GS_PG bool gs_mcmc_alive(float opacity, float min_opacity_logit) { return opacity > min_opacity_logit; }

GS_PG uint32_t gs_mcmc_weight(float opacity, float min_opacity_logit) {
#pragma clang fp contract(off)
    const float sig = gs_sigmoid_logit<float>(opacity);
    return (gs_mcmc_alive(opacity, min_opacity_logit) && __builtin_isfinite(sig)) ? (uint32_t)floorf(sig * GS_MCMC_W_ONE) : 0u;
}

// the place on the CDF a uniform number points at; total > 0
GS_PG uint64_t gs_mcmc_target(float u, uint64_t total) {
#pragma clang fp contract(off)
    float uc = u;
    if (!(uc >= 0.0f)) uc = 0.0f;                                          // negative, or NaN
    if (uc > 0.99999994f) uc = 0.99999994f;                                // 1 - 2^-24
    const uint64_t t = (uint64_t)((double)uc * (double)total);
    return t < total - 1 ? t : total - 1;
}
// the smallest i in [0, n) with cdf[i] > t; t < cdf[n - 1]
GS_PG int64_t gs_mcmc_search(const uint64_t *cdf, int64_t n, uint64_t t) {
    int64_t lo = 0, hi = n - 1;                                            // the answer lies in [lo, hi]
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > t) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// opacity and scales of a source drawn c >= 1 times, and of every gaussian relocated onto it.  B: gs_mcmc_binom_fill's table.
GS_PG void gs_mcmc_relocated(float opacity, const float (&scale)[3], int c, float min_opacity, const double *B, float &opacity_out, float (&scale_out)[3]) {
#pragma clang fp contract(off)
    const int n = c + 1 < GS_MCMC_NMAX ? c + 1 : GS_MCMC_NMAX;
    double o = (double)gs_sigmoid_logit<float>(opacity);
    if (!(o >= 0.0)) o = 0.0;
    if (o > 0.999999940395355224609375) o = 0.999999940395355224609375;    // 1 - 2^-24
    const double p = -expm1(log1p(-o) / (double)n);
    double s = 0.0;
    for (int i = 1; i <= n; ++i) {
        double pk = p;                                                     // p^(k+1), by repeated multiplication
        for (int k = 0; k < i; ++k) {
            const double rs = 1.0 / sqrt((double)k + 1.0);
            s = s + (B[(i - 1) * GS_MCMC_NMAX + k] * ((k & 1) ? -rs : rs)) * pk;
            pk = pk * p;
        }
    }
    double pc = p > (double)min_opacity ? p : (double)min_opacity;         // max(p, min_opacity); a NaN p takes min_opacity
    if (pc > 0.99999988079071044921875) pc = 0.99999988079071044921875;    // 1 - 2^-23
    opacity_out = (float)(log(pc) - log1p(-pc));
    const double shift = log(o / s);
    for (int j = 0; j < 3; ++j) scale_out[j] = (float)((double)scale[j] + shift);
}

// the noise statement; false (and mean untouched) when one of the three results would not be finite
GS_PG bool gs_mcmc_noise(float (&mean)[3], const float (&scale)[3], const float (&quat)[4], float opacity, const float (&z)[3], float lr, float gate_k, float gate_t) {
#pragma clang fp contract(off)
    const float sig = gs_sigmoid_logit<float>(opacity);
    const float gate = 1.0f / (1.0f + gs_expf(gate_k * (sig - gate_t)));
    float R[3][3];
    gs_quat_to_rot(quat[0], quat[1], quat[2], quat[3], R);
    float b[3];
    for (int j = 0; j < 3; ++j) {
        const float e = gs_expf(scale[j]);
        const float a = (R[0][j] * z[0] + R[1][j] * z[1]) + R[2][j] * z[2];
        b[j] = (e * e) * a;
    }
    const float step = lr * gate;
    float m[3];
    for (int i = 0; i < 3; ++i) {
        const float d = (R[i][0] * b[0] + R[i][1] * b[1]) + R[i][2] * b[2];
        m[i] = mean[i] + step * d;
    }
    if (!(__builtin_isfinite(m[0]) && __builtin_isfinite(m[1]) && __builtin_isfinite(m[2]))) return false;
    mean[0] = m[0]; mean[1] = m[1]; mean[2] = m[2];
    return true;
}

// the regularisers' gradients with respect to the stored logit / log parameters, added to d
GS_PG float gs_mcmc_reg_opacity(float d, float c_o, float opacity) {
#pragma clang fp contract(off)
    const float sig = gs_sigmoid_logit<float>(opacity);
    return d + c_o * (sig * (1.0f - sig));
}
GS_PG float gs_mcmc_reg_scale(float d, float c_s, float scale) {
#pragma clang fp contract(off)
    return d + c_s * gs_expf(scale);
}

#if defined(__HIPCC__)
#include "gs_density.h"
// gs_mcmc.hip.  Every pointer is a device pointer.
// plan: chunk_sum / chunk_off are [2][gs_chunks(n)] words (row 0: the chunks' weight sums, row 1: their dead counts; then the exclusive offsets of both),
// totals two words {sum of the weights, dead}.  Three launches, none waits for another workgroup.
hipError_t gs_launch_mcmc_plan(const float *opac, int64_t n, float min_opacity_logit, unsigned long long *chunk_sum, unsigned long long *chunk_off,
                               unsigned long long *totals, unsigned long long *cdf, int32_t *dead, hipStream_t s);
hipError_t gs_launch_mcmc_sample(const unsigned long long *cdf, int64_t n, const float *u, int64_t m, int32_t *src, hipStream_t s);
struct GsMcmcRelocateArgs {
    int64_t n, m;
    int k3;                               // floats of an SH row
    const int32_t *src, *dst;             // m words each (dst: the caller's, or the plan's dead list)
    int32_t *hist;                        // n words of ctx scratch: how often a gaussian is a source (the launcher zeroes it)
    const double *binom;
    float min_opacity;
    float *model[5];
    int nsets;
    float *set[GS_DENSITY_MAX_SETS][5];   // a null array: skipped
};
hipError_t gs_launch_mcmc_relocate(const GsMcmcRelocateArgs &a, hipStream_t s);
hipError_t gs_launch_mcmc_noise(float *means, const float *scales, const float *quats, const float *opac, const float *z, int64_t n, float lr,
                                float gate_k, float gate_t, hipStream_t s);
hipError_t gs_launch_mcmc_regularize(const float *scales, const float *opac, float *d_scales, float *d_opac, int64_t n, float c_opacity, float c_scale,
                                     hipStream_t s);
#endif
