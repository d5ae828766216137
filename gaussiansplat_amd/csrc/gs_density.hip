// gs_density.hip -- density control on the device: what a 3DGS trainer does every hundred iterations besides stepping Adam.
//
//   gs_density_accumulate_kernel   one thread per gaussian, after a backward of the frame: the gaussian's row of 2-D gradient sums becomes
//                                  d L / d mu' exactly as gs_get_array(GS_ARR_GRAD2D) forms it on the host (gs_g2d_to_grads with the view's
//                                  sig and conic), its length in NDC units is added to grad_sum; the view's packed pixel box gives
//                                  `visible` and the extent.  Reads 16 B of the payload row (its last quad: sig and the box), 16 B conic,
//                                  the 64-byte row, 12 B of statistics; writes 12 B.
//   gs_density_decide_kernel       element-wise: 0 keep, 1 clone, 2 split, 3 prune -- comparisons of stored floats and integers only.
//   PLAN: the ordered compaction of gs_chunk.h over three output classes: gs_density_class_kernel (per chunk of 256 gaussians: ballots ->
//   three counts), then gs_launch_chunk_scan (one workgroup per class: exclusive offsets and the class total).
//   gs_density_restructure_kernel  per chunk: every thread re-derives its rank inside the chunk from the same ballots and copies its row to
//                                  the survivors' block, the clones' block and / or writes its two children into the splits' block; the
//                                  gradient-shaped companion sets (Adam's moments) ride along: survivors copied, new rows +0.
//                                  A row is moved by its own thread (gs_row_put), SH rows as 16-byte accesses where 3K % 4 == 0 and the arrays are
//                                  16-byte aligned (twelve loads and stores at degree 3).  That is the form that was measured (C3: a quarter
//                                  of the copy rate); a cooperative copy through the chunk's ranks in LDS was not built: the
//                                  kernel runs once per hundred iterations.
//   gs_opacity_reset_kernel        element-wise clamp of the logit opacities from above, +0 into their two moment words.
//
// Built with -ffp-contract=off: every product and sum below is rounded on its own (tests/density_ref.py is the NumPy twin, bit for bit);
// sqrtf is the correctly rounded form (hipcc's default, see gs_adam.h).  Random numbers are an input: the kernels are pure functions.
#include "gs_density.h"
#include "gs_pergaussian.h"
#include "gs_wave.h"
#include <stddef.h>

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void gs_density_accumulate_kernel(GsDensityAccArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;
    float row[10];
    gs_g2d_row_load(a, g, row);
    const float4 ic = reinterpret_cast<const float4 *>(a.invcov)[g];
    const uint4 q = reinterpret_cast<const uint4 *>(a.payload + g)[GS_PAYLOAD_QUADS - 1];   // {yhi, sig, bbx, bby}
    static_assert(offsetof(GsPayload, sig) == 52 && offsetof(GsPayload, bbx) == 56 && offsetof(GsPayload, bby) == 60, "the payload row's last quad");
    gs_g2d_to_grads(row, __uint_as_float(q.y), ic.x, 0.5f * (ic.y + ic.z), ic.w);
    const float da = a.half_w * row[4], db = a.half_h * row[5];
    const float s = da * da + db * db;
    a.grad_sum[g] = a.grad_sum[g] + sqrtf(s);
    const int xmin = (int)(short)(q.z & 0xFFFFu), xmax = (int)(short)(q.z >> 16);
    const int ymin = (int)(short)(q.w & 0xFFFFu), ymax = (int)(short)(q.w >> 16);
    const bool visible = xmax >= xmin && ymax >= ymin;                     // gs_payload_box_edges' `empty`, negated
    const int ext = visible ? max(xmax - xmin, ymax - ymin) + 1 : 0;
    a.count[g] = a.count[g] + (visible ? 1 : 0);
    a.max_extent[g] = max(a.max_extent[g], ext);
}

__global__ __launch_bounds__(256) void gs_density_decide_kernel(GsDensityDecideArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;
    const float s0 = a.scales[3 * g], s1 = a.scales[3 * g + 1], s2 = a.scales[3 * g + 2];
    float smax = fmaxf(fmaxf(s0, s1), s2);
    if (s0 != s0 || s1 != s1 || s2 != s2) smax = __builtin_nanf("");       // a NaN scale makes every comparison below false
    const int cnt = a.count[g];
    const bool dens = cnt > 0 && a.grad_sum[g] >= a.grad_threshold * (float)cnt;
    const bool split = dens && smax > a.log_split_scale;
    const float remain = split ? smax - a.log_shrink : smax;
    const bool prune = a.opac[g] < a.min_opacity_logit || (a.max_extent_px > 0 && a.max_extent[g] > a.max_extent_px) ||
                       remain > a.log_max_world_scale;
    a.action[g] = prune ? 3 : split ? 2 : dens ? 1 : 0;
}

// the three classes a source row feeds, from its action: survivors (0, 1), clones (1), split sources (2)
__device__ __forceinline__ void density_classes(int act, bool in, bool (&cls)[GS_DENSITY_CLASSES]) {
    cls[0] = in && (act == 0 || act == 1); cls[1] = in && act == 1; cls[2] = in && act == 2;
}

__global__ __launch_bounds__(GS_CHUNK) void gs_density_class_kernel(const int32_t *__restrict__ action, int64_t n, uint32_t *__restrict__ chunk_cnt,
                                                                             int64_t nchunks, int64_t *__restrict__ totals) {
    __shared__ int wave_cnt[GS_DENSITY_CLASSES][GS_CHUNK_WAVES];
    const int64_t g = (int64_t)blockIdx.x * GS_CHUNK + threadIdx.x;
    const bool in = g < n;
    const int act = in ? action[g] : 0;
    bool cls[GS_DENSITY_CLASSES];
    density_classes(act, in, cls);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < GS_DENSITY_CLASSES; ++k) {
        const GsWaveRank r = gs_wave_rank(cls[k], lane);
        if (lane == 0) wave_cnt[k][wv] = r.count;
    }
    const unsigned long long bad = gs_wave_rank(in && (act < 0 || act > 3), lane).ballot;
    if (lane == 0 && bad) atomicOr(reinterpret_cast<unsigned long long *>(totals + 3), 1ull);
    __syncthreads();
    if (threadIdx.x < GS_DENSITY_CLASSES)
        chunk_cnt[(int64_t)threadIdx.x * nchunks + blockIdx.x] = (uint32_t)gs_chunk_count(wave_cnt[threadIdx.x]);
}

__global__ __launch_bounds__(GS_CHUNK) void gs_density_restructure_kernel(GsDensityRestructureArgs a, int64_t nchunks) {
    __shared__ int wave_cnt[GS_DENSITY_CLASSES][GS_CHUNK_WAVES];
    const int64_t g = (int64_t)blockIdx.x * GS_CHUNK + threadIdx.x;
    const bool in = g < a.n;
    const int act = in ? a.action[g] : 0;
    bool cls[GS_DENSITY_CLASSES];
    density_classes(act, in, cls);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int rank[GS_DENSITY_CLASSES];
#pragma unroll
    for (int k = 0; k < GS_DENSITY_CLASSES; ++k) {
        const GsWaveRank r = gs_wave_rank(cls[k], lane);
        rank[k] = r.below;
        if (lane == 0) wave_cnt[k][wv] = r.count;
    }
    __syncthreads();
    int64_t idx[GS_DENSITY_CLASSES];                                       // the row's place inside its class
#pragma unroll
    for (int k = 0; k < GS_DENSITY_CLASSES; ++k) idx[k] = a.chunk_off[(int64_t)k * nchunks + blockIdx.x] + gs_chunk_before(wave_cnt[k], wv) + rank[k];
    // survivors, then clones: copies of the source row; the companions of a survivor are copied, those of a clone are +0.  Every place is
    // checked against the plan's totals: an action array edited since the plan cannot send a row outside the destination
    if (cls[0] && idx[0] < a.survivors) {
#pragma unroll
        for (int i = 0; i < 5; ++i) gs_row_put(a.dst[i], idx[0], a.src[i], g, gs_row_width(i, a.k3));
        gs_rows_copy_sets(a.set_dst, a.set_src, a.nsets, idx[0], g, a.k3);
    }
    if (cls[1] && idx[1] < a.clones) {
        const int64_t r = a.survivors + idx[1];
#pragma unroll
        for (int i = 0; i < 5; ++i) gs_row_put(a.dst[i], r, a.src[i], g, gs_row_width(i, a.k3));
        gs_rows_zero_sets(a.set_dst, a.nsets, r, a.k3);
    }
    if (cls[2] && idx[2] < a.splits) {
        const float m[3] = {a.src[0][3 * g], a.src[0][3 * g + 1], a.src[0][3 * g + 2]};
        const float sc[3] = {a.src[1][3 * g], a.src[1][3 * g + 1], a.src[1][3 * g + 2]};
        float R[3][3];                                                     // quatToRot as the forward writes it: raw quaternion, the reference's signs
        gs_quat_to_rot(a.src[2][4 * g], a.src[2][4 * g + 1], a.src[2][4 * g + 2], a.src[2][4 * g + 3], R);
        const float ex[3] = {gs_expf(sc[0]), gs_expf(sc[1]), gs_expf(sc[2])};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int64_t r = a.survivors + a.clones + 2 * idx[2] + c;
            const float *z = a.noise + (2 * g + c) * 3;
            const float e0 = ex[0] * z[0], e1 = ex[1] * z[1], e2 = ex[2] * z[2];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float w = (R[i][0] * e0 + R[i][1] * e1) + R[i][2] * e2;
                a.dst[0][3 * r + i] = m[i] + w;
                a.dst[1][3 * r + i] = sc[i] - a.log_shrink;
            }
#pragma unroll
            for (int i = 2; i < 5; ++i) gs_row_put(a.dst[i], r, a.src[i], g, gs_row_width(i, a.k3));
            gs_rows_zero_sets(a.set_dst, a.nsets, r, a.k3);
        }
    }
}

__global__ __launch_bounds__(256) void gs_opacity_reset_kernel(float *__restrict__ opac, float max_logit, float *__restrict__ m_opac,
                                                                float *__restrict__ v_opac, int64_t n) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const float o = opac[g];
    opac[g] = o > max_logit ? max_logit : o;                               // a NaN stays
    if (m_opac) m_opac[g] = 0.0f;
    if (v_opac) v_opac[g] = 0.0f;
}

hipError_t gs_launch_density_accumulate(const GsDensityAccArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    unsigned blocks;
    if (!gs_grid_256(a.n, &blocks) || (!a.g2d == !a.g2d_fixed)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gs_density_accumulate_kernel, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t gs_launch_density_decide(const GsDensityDecideArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    unsigned blocks;
    if (!gs_grid_256(a.n, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gs_density_decide_kernel, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t gs_launch_density_plan(const int32_t *action, int64_t n, uint32_t *chunk_cnt, int64_t *chunk_off, int64_t *totals, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(totals, 0, 4 * sizeof(int64_t), s);
    if (e != hipSuccess || n <= 0) return e;
    unsigned blocks;
    if (!gs_grid_256(n, &blocks)) return hipErrorInvalidValue;
    const int64_t nchunks = gs_chunks(n);
    hipLaunchKernelGGL(gs_density_class_kernel, dim3(blocks), dim3(GS_CHUNK), 0, s, action, n, chunk_cnt, nchunks, totals);
    return gs_launch_chunk_scan(chunk_cnt, chunk_off, nchunks, GS_DENSITY_CLASSES, totals, s);
}

hipError_t gs_launch_density_restructure(const GsDensityRestructureArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    unsigned blocks;
    if (!gs_grid_256(a.n, &blocks) || a.nsets < 0 || a.nsets > GS_DENSITY_MAX_SETS || a.k3 <= 0 || (a.splits > 0 && !a.noise)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gs_density_restructure_kernel, dim3(blocks), dim3(GS_CHUNK), 0, s, a, gs_chunks(a.n));
    return hipGetLastError();
}

hipError_t gs_launch_opacity_reset(float *opac, float max_logit, float *m_opac, float *v_opac, int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    unsigned blocks;
    if (!gs_grid_256(n, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gs_opacity_reset_kernel, dim3(blocks), dim3(256), 0, s, opac, max_logit, m_opac, v_opac, n);
    return hipGetLastError();
}
