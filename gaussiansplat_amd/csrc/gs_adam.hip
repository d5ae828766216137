// gs_adam.hip -- Adam on the device (gs_adam_step): the ctx's resident model updated in place from the gradients of a gs_grads and
// two caller-owned moment buffers of the same layout.  The fused form (gs_backward_adam) lives in gs_preprocess_bwd.hip; both apply
// gs_adam_update (gs_adam.h) to every float, so that the fused step is bit-identical to a backward followed by this one.
//
// One launch for all five arrays (SGD launches five).  HBM-bound: 4 reads + 3 writes per float (p, g, m, v in; p, m, v out).
//   dense      a capped grid strides over each array in turn, 16-byte accesses where p, g, m and v are all 16-byte aligned (the
//              slices of a flat buffer at 12n / 40n / 44n bytes are not when n % 4 != 0: those arrays go one float per lane, still
//              coalesced), a scalar tail otherwise.
//   selective  a workgroup takes GS_ADAM_ROWS gaussians at a time: their gradient rows come into LDS once (coalesced) and mark the live
//              rows on the way; one wave compacts the live rows, and the workgroup steps only their p, m and v (every lane on a live
//              float: the correctly rounded '/' and sqrt make the update ~55 VALU operations per float, which dead lanes of a mixed
//              wave would pay too).  A dead row costs its gradient read only.
#include "gs_ctx.h"
#include "gs_adam.h"
#include "gs_wave.h"

#define GS_ADAM_ROWS 64              // gaussians per workgroup pass of the selective kernel (= the wave size: one ballot compacts them)
#define GS_ADAM_MAX_BLOCKS 2048      // 256 CUs x 8 workgroups: memory-bound, capped grid + grid-stride loops

namespace {

struct AdamSeg {
    float *p;
    const float *g;
    float *m, *v;
    int64_t len;       // floats of the array (w x n)
    int64_t units;     // float4 units (vec) or floats
    int w;             // floats per row
    int sh;            // 1: the fifth array, group by the float's place in its row (gs_adam_sh_group)
    int vec;           // p, g, m, v all 16-byte aligned
    int lds_off;       // selective kernel: first float of the array's rows in the LDS tile
    float ss;          // step size of the group (sh == 0)
};
struct AdamArgs {
    AdamSeg seg[5];
    int nseg;
    int64_t n;
    GsAdamHyper h;
};

__device__ __forceinline__ int row_mod(int64_t i, int w) {          // i % w, 32-bit when i fits
    return (i >> 32) == 0 ? (int)((uint32_t)i % (uint32_t)w) : (int)(i % w);
}
__device__ __forceinline__ float seg_ss(const AdamSeg &s, const GsAdamHyper &h, int j) {
    return s.sh ? (j < 3 ? h.step_size[4] : h.step_size[5]) : s.ss;
}
__device__ __forceinline__ void step_one(const AdamSeg &s, const GsAdamHyper &h, int64_t i, float g, float ss) {
    float p = s.p[i], m = s.m[i], v = s.v[i];
    gs_adam_update(p, m, v, g, h, ss);
    s.p[i] = p; s.m[i] = m; s.v[i] = v;
}
// four floats i .. i + 3 of one array, 16-byte accesses; j = i % w (sh arrays)
__device__ __forceinline__ void step_four(const AdamSeg &s, const GsAdamHyper &h, int64_t i, float4 g, int j) {
    float4 p = *reinterpret_cast<const float4 *>(s.p + i), m = *reinterpret_cast<const float4 *>(s.m + i),
           v = *reinterpret_cast<const float4 *>(s.v + i);
    const int j1 = j + 1 >= s.w ? j + 1 - s.w : j + 1, j2 = j1 + 1 >= s.w ? j1 + 1 - s.w : j1 + 1, j3 = j2 + 1 >= s.w ? j2 + 1 - s.w : j2 + 1;
    gs_adam_update(p.x, m.x, v.x, g.x, h, seg_ss(s, h, j));
    gs_adam_update(p.y, m.y, v.y, g.y, h, seg_ss(s, h, j1));
    gs_adam_update(p.z, m.z, v.z, g.z, h, seg_ss(s, h, j2));
    gs_adam_update(p.w, m.w, v.w, g.w, h, seg_ss(s, h, j3));
    *reinterpret_cast<float4 *>(s.p + i) = p; *reinterpret_cast<float4 *>(s.m + i) = m; *reinterpret_cast<float4 *>(s.v + i) = v;
}

__global__ __launch_bounds__(256) void gs_adam_dense_kernel(AdamArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        if (k >= a.nseg) break;
        const AdamSeg &s = a.seg[k];
        if (s.vec) {
            for (int64_t u = t0; u < s.units; u += stride) {
                const int64_t i = 4 * u;
                if (i + 4 <= s.len) {
                    step_four(s, a.h, i, *reinterpret_cast<const float4 *>(s.g + i), s.sh ? row_mod(i, s.w) : 0);
                } else {
                    for (int64_t e = i; e < s.len; ++e) step_one(s, a.h, e, s.g[e], seg_ss(s, a.h, s.sh ? row_mod(e, s.w) : 0));
                }
            }
        } else {
            for (int64_t e = t0; e < s.len; e += stride) step_one(s, a.h, e, s.g[e], seg_ss(s, a.h, s.sh ? row_mod(e, s.w) : 0));
        }
    }
}

__global__ __launch_bounds__(256) void gs_adam_selective_kernel(AdamArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gt[];        // [GS_ADAM_ROWS x sum of the widths] gradient rows of the pass
    __shared__ int live[GS_ADAM_ROWS], order[GS_ADAM_ROWS], nlive;
    const int64_t npass = (a.n + GS_ADAM_ROWS - 1) / GS_ADAM_ROWS;
    for (int64_t pass = blockIdx.x; pass < npass; pass += gridDim.x) {
        const int64_t r0 = pass * GS_ADAM_ROWS;
        const int rows = (int)min((int64_t)GS_ADAM_ROWS, a.n - r0);
        if (threadIdx.x < GS_ADAM_ROWS) live[threadIdx.x] = 0;
        __syncthreads();
        // the gradient rows into LDS; a row is live if any of its floats compares != 0 (-0 is dead, NaN live)
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            if (k >= a.nseg) break;
            const AdamSeg &s = a.seg[k];
            const int len = rows * s.w;
            const float *src = s.g + r0 * s.w;
            float *dst = gt + s.lds_off;
            int e0 = 0;
            if (s.vec) {                                                   // r0 * w is a multiple of 64 floats: aligned with the array
                e0 = len & ~3;
                for (int q = threadIdx.x; q < (len >> 2); q += blockDim.x) {
                    const float4 g4 = reinterpret_cast<const float4 *>(src)[q];
                    reinterpret_cast<float4 *>(dst)[q] = g4;
                    if (g4.x != 0.0f) live[(4 * q) / s.w] = 1;
                    if (g4.y != 0.0f) live[(4 * q + 1) / s.w] = 1;
                    if (g4.z != 0.0f) live[(4 * q + 2) / s.w] = 1;
                    if (g4.w != 0.0f) live[(4 * q + 3) / s.w] = 1;
                }
            }
            for (int e = e0 + threadIdx.x; e < len; e += blockDim.x) {
                const float gv = src[e];
                dst[e] = gv;
                if (gv != 0.0f) live[e / s.w] = 1;
            }
        }
        __syncthreads();
        // the live rows, compacted by one wave, so that the lanes of the update loop all do useful work
        if (threadIdx.x < GS_ADAM_ROWS) {
            const bool l = threadIdx.x < rows && live[threadIdx.x];
            const GsWaveRank r = gs_wave_rank(l, threadIdx.x);
            if (l) order[r.below] = threadIdx.x;
            if (threadIdx.x == 0) nlive = r.count;
        }
        __syncthreads();
        const int nl = nlive;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            if (k >= a.nseg) break;
            const AdamSeg &s = a.seg[k];
            const float *lg = gt + s.lds_off;
            if (s.vec && (s.w & 3) == 0) {                                 // float4s stay inside a row
                for (int q = threadIdx.x; q < nl * (s.w >> 2); q += blockDim.x) {
                    const int e = 4 * q, row = order[e / s.w], j = e % s.w;
                    step_four(s, a.h, (r0 + row) * s.w + j, *reinterpret_cast<const float4 *>(lg + row * s.w + j), j);
                }
            } else {
                for (int e = threadIdx.x; e < nl * s.w; e += blockDim.x) {
                    const int row = order[e / s.w], j = e % s.w;
                    step_one(s, a.h, (r0 + row) * s.w + j, lg[row * s.w + j], seg_ss(s, a.h, s.sh ? j : 0));
                }
            }
        }
        __syncthreads();                                                   // the next pass reuses gt and live
    }
}

}  // namespace

int gs_adam_scalars(gs_ctx *c, const char *who, const float *lr, int nlr, float beta1, float beta2, float eps, int64_t step, GsAdamHyper *h) {
    const std::string w(who);
    if (step < 1) return fail(c, GS_ERR_INVALID, w + ": step counts from 1");
    if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f)) return fail(c, GS_ERR_INVALID, w + ": betas must lie in [0, 1)");
    if (!std::isfinite(eps) || !(eps > 0.0f)) return fail(c, GS_ERR_INVALID, w + ": eps must be finite and > 0");
    if (!lr) return fail(c, GS_ERR_INVALID, w + ": NULL lr");
    for (int i = 0; i < nlr; ++i)
        if (!std::isfinite(lr[i]) || lr[i] < 0.0f) return fail(c, GS_ERR_INVALID, w + ": every lr must be finite and >= 0");
    // the scalars: each in double, rounded to float once
    const double t = (double)step;
    h->beta1 = beta1; h->beta2 = beta2; h->eps = eps;
    h->omb1 = (float)(1.0 - (double)beta1);
    h->omb2 = (float)(1.0 - (double)beta2);
    const double bc1 = 1.0 - std::pow((double)beta1, t);
    for (int i = 0; i < GS_ADAM_NGROUPS; ++i) h->step_size[i] = i < nlr ? (float)((double)lr[i] / bc1) : 0.0f;
    h->sqrt_bc2 = (float)std::sqrt(1.0 - std::pow((double)beta2, t));
    return GS_OK;
}

int gs_adam_prepare(gs_ctx *c, const char *who, const float *const p[5], const float *const g[5], float *const m[5], float *const v[5],
                    const float *lr, float beta1, float beta2, float eps, int64_t step, int flags, GsAdamHyper *h) {
    const std::string w(who);
    if (const int rc = gs_adam_scalars(c, who, lr, GS_ADAM_GROUPS, beta1, beta2, eps, step, h)) return rc;
    if (flags & ~GS_ADAM_SELECTIVE) return fail(c, GS_ERR_INVALID, w + ": unknown flag bits");
    // the arrays the step touches must not overlap: p, g, m, v of every group that is stepped
    ByteRange r[20];
    int nr = 0;
    for (int i = 0; i < 5; ++i) {
        if (g && !g[i]) continue;                                          // frozen group: nothing of it is touched
        if (!m[i] || !v[i]) return fail(c, GS_ERR_INVALID, w + ": a stepped group needs both moment arrays");
        const size_t bytes = sizeof(float) * c->width[i] * (size_t)c->n;
        if (bytes && !p[i]) return fail(c, GS_ERR_INVALID, w + ": no model (gs_set_model first)");
        const void *arr[4] = {p[i], g ? g[i] : nullptr, m[i], v[i]};
        for (const void *q : arr)
            if (q) r[nr++] = {q, bytes};
    }
    for (int i = 0; i < nr; ++i)
        for (int j = i + 1; j < nr; ++j)
            if (overlaps(r[i], r[j])) return fail(c, GS_ERR_INVALID, w + ": parameter, gradient and moment arrays overlap");
    return GS_OK;
}

extern "C" int gs_adam_step(gs_ctx *c, const gs_grads *grads, const gs_grads *exp_avg, const gs_grads *exp_avg_sq, const float lr[GS_ADAM_GROUPS],
                            float beta1, float beta2, float eps, int64_t step, int flags) {
    if (!c) return GS_ERR_INVALID;
    if (!grads || !exp_avg || !exp_avg_sq) return fail(c, GS_ERR_INVALID, "gs_adam_step: NULL argument");
    const Five<float> p = c->model5_mut(), g = five(*grads), m = five(*exp_avg), v = five(*exp_avg_sq);
    AdamArgs a{};
    if (const int rc = gs_adam_prepare(c, "gs_adam_step", p.p, g.p, m.p, v.p, lr, beta1, beta2, eps, step, flags, &a.h)) return rc;
    if (bind_device(c)) return GS_ERR_HIP;
    const int64_t n = c->n;
    int64_t most = 0;
    int lds = 0;
    for (int i = 0; i < 5; ++i) {
        if (!g[i] || n <= 0) continue;
        AdamSeg &s = a.seg[a.nseg++];
        s.p = p[i]; s.g = g[i]; s.m = m[i]; s.v = v[i];
        s.w = (int)c->width[i]; s.len = (int64_t)s.w * n;
        s.sh = i == 4; s.ss = a.h.step_size[i < 4 ? i : 4];
        s.vec = ((reinterpret_cast<uintptr_t>(s.p) | reinterpret_cast<uintptr_t>(s.g) | reinterpret_cast<uintptr_t>(s.m) |
                  reinterpret_cast<uintptr_t>(s.v)) & 15) == 0;
        s.units = s.vec ? (s.len + 3) / 4 : s.len;
        s.lds_off = lds; lds += GS_ADAM_ROWS * s.w;
        most = std::max(most, s.units);
    }
    a.n = n;
    if (a.nseg) {
        if (flags & GS_ADAM_SELECTIVE) {
            const int64_t npass = (n + GS_ADAM_ROWS - 1) / GS_ADAM_ROWS;
            const unsigned grid = (unsigned)std::min<int64_t>(npass, GS_ADAM_MAX_BLOCKS);
            hipLaunchKernelGGL(gs_adam_selective_kernel, dim3(grid), dim3(256), sizeof(float) * lds, c->stream, a);
        } else {
            const unsigned grid = (unsigned)std::min<int64_t>((most + 255) / 256, GS_ADAM_MAX_BLOCKS);
            hipLaunchKernelGGL(gs_adam_dense_kernel, dim3(grid), dim3(256), 0, c->stream, a);
        }
        HIPCHK(c, hipGetLastError());
    }
    c->inputs_changed();
    return GS_OK;
}
