// gs_mcmc.hip -- the MCMC densification strategy on the device: the statements of gs_mcmc.h, per gaussian or per draw.
//
//   PLAN: the integer weights, their device-wide inclusive prefix sum (the CDF) and the ordered list of the gaussians that are not alive, WITHOUT any
//   workgroup waiting for another -- the compaction of gs_chunk.h: gs_mcmc_weigh_kernel (per chunk of 256 gaussians: the sum of the weights by
//   gs_block_sum, the dead count by ballots), gs_launch_chunk_scan on 64-bit words (one workgroup per row of chunk words: exclusive offsets and the
//   total; every thread sums a contiguous span, so any number of chunks), gs_mcmc_emit_kernel (per chunk: every thread re-derives its weight, a wave scan
//   and the four wave sums give its inclusive sum inside the chunk, the same ballots its rank among the dead).  Integers: exact in any order.
//   gs_mcmc_sample_kernel     one thread per draw: the target on the CDF, one binary search (about log2 n dependent 8-byte loads).
//   RELOCATE, three launches behind the zero fill of the histogram: gs_mcmc_count_kernel (how often every gaussian is a source: int32 atomics),
//   gs_mcmc_move_kernel (one thread per draw j: row dst[j] = means, quaternion and SH row of src[j] bit for bit, opacity and scales the relocation
//   statement's; +0 into the companion rows of dst[j]) and only THEN gs_mcmc_source_kernel (one thread per gaussian with a count: the same statement
//   on the same inputs into its own opacity and scales, +0 into its companion rows) -- no source is written before every read of it is over, and
//   the destinations are no sources by contract.  A draw recomputes its source's statement (1326 double multiply-adds at the largest n)
//   instead of reading it from a staging array: the call runs once per hundred iterations.
//   gs_mcmc_noise_kernel      one thread per gaussian: 14 floats read, 3 written; the 12-byte rows coalesce across a wave as they are.
//   gs_mcmc_regularize_kernel one thread per gaussian: 4 floats read, 4 read and written.
//
// Built with -ffp-contract=off (tests/mcmc_ref.py is the NumPy twin); random numbers are an input: the kernels are pure functions.
#include "gs_mcmc.h"
#include "gs_wave.h"

#pragma clang fp contract(off)

typedef unsigned long long u64;

__global__ __launch_bounds__(GS_CHUNK) void gs_mcmc_weigh_kernel(const float *__restrict__ opac, int64_t n, float min_logit, u64 *__restrict__ chunk_sum,
                                                                       int64_t nchunks) {
    __shared__ u64 sm[GS_CHUNK_WAVES];
    __shared__ int dead_cnt[GS_CHUNK_WAVES];
    const int64_t g = (int64_t)blockIdx.x * GS_CHUNK + threadIdx.x;
    const bool in = g < n;
    const float o = in ? opac[g] : 0.0f;
    const u64 w = in ? (u64)gs_mcmc_weight(o, min_logit) : 0ull;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const GsWaveRank r = gs_wave_rank(in && !gs_mcmc_alive(o, min_logit), lane);
    if (lane == 0) dead_cnt[wv] = r.count;
    const u64 total = gs_block_sum(w, sm, GS_CHUNK_WAVES);                  // (its barrier covers dead_cnt too)
    if (threadIdx.x == 0) {
        chunk_sum[blockIdx.x] = total;
        chunk_sum[nchunks + blockIdx.x] = (u64)gs_chunk_count(dead_cnt);
    }
}

__global__ __launch_bounds__(GS_CHUNK) void gs_mcmc_emit_kernel(const float *__restrict__ opac, int64_t n, float min_logit, const u64 *__restrict__ chunk_off,
                                                                      int64_t nchunks, u64 *__restrict__ cdf, int32_t *__restrict__ dead) {
    __shared__ u64 wave_sum[GS_CHUNK_WAVES];
    __shared__ int dead_cnt[GS_CHUNK_WAVES];
    const int64_t g = (int64_t)blockIdx.x * GS_CHUNK + threadIdx.x;
    const bool in = g < n;
    const float o = in ? opac[g] : 0.0f;
    u64 v = in ? (u64)gs_mcmc_weight(o, min_logit) : 0ull;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {                                     // inclusive scan inside the wave
        const u64 up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    const bool is_dead = in && !gs_mcmc_alive(o, min_logit);
    const GsWaveRank r = gs_wave_rank(is_dead, lane);
    if (lane == 63) wave_sum[wv] = v;
    if (lane == 0) dead_cnt[wv] = r.count;
    __syncthreads();
    if (in) cdf[g] = chunk_off[blockIdx.x] + gs_chunk_before(wave_sum, wv) + v;
    // a rank below the dead total <= n: inside the caller's n words, even if the opacities were edited between the launches
    const int64_t place = (int64_t)chunk_off[nchunks + blockIdx.x] + gs_chunk_before(dead_cnt, wv) + r.below;
    if (is_dead && place < n) dead[place] = (int32_t)g;
}

__global__ __launch_bounds__(256) void gs_mcmc_sample_kernel(const u64 *__restrict__ cdf, int64_t n, const float *__restrict__ u, int64_t m, int32_t *__restrict__ src) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const u64 total = cdf[n - 1];
    if (total == 0) return;                                                // nobody is alive: nothing is written
    src[j] = (int32_t)gs_mcmc_search(reinterpret_cast<const uint64_t *>(cdf), n, gs_mcmc_target(u[j], total));
}

// the pair (source, destination) of draw j, or false: an entry outside [0, n) makes the draw a no-op
__device__ __forceinline__ bool mcmc_pair(const GsMcmcRelocateArgs &a, int64_t j, int64_t &s, int64_t &d) {
    s = a.src[j]; d = a.dst[j];
    return s >= 0 && s < a.n && d >= 0 && d < a.n;
}

__global__ __launch_bounds__(256) void gs_mcmc_count_kernel(GsMcmcRelocateArgs a) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.m) return;
    int64_t s, d;
    if (mcmc_pair(a, j, s, d)) atomicAdd(a.hist + s, 1);
}

__global__ __launch_bounds__(256) void gs_mcmc_move_kernel(GsMcmcRelocateArgs a) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.m) return;
    int64_t s, d;
    if (!mcmc_pair(a, j, s, d)) return;
    const float sc[3] = {a.model[1][3 * s], a.model[1][3 * s + 1], a.model[1][3 * s + 2]};
    float op, so[3];
    gs_mcmc_relocated(a.model[3][s], sc, a.hist[s], a.min_opacity, a.binom, op, so);
#pragma unroll
    for (int i = 0; i < 5; i += 2) gs_row_put(a.model[i], d, a.model[i], s, gs_row_width(i, a.k3));   // means, quaternion, SH row: inside one array
    a.model[1][3 * d] = so[0]; a.model[1][3 * d + 1] = so[1]; a.model[1][3 * d + 2] = so[2];
    a.model[3][d] = op;
    gs_rows_zero_sets(a.set, a.nsets, d, a.k3);
}

__global__ __launch_bounds__(256) void gs_mcmc_source_kernel(GsMcmcRelocateArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;
    const int c = a.hist[g];
    if (c <= 0) return;
    const float sc[3] = {a.model[1][3 * g], a.model[1][3 * g + 1], a.model[1][3 * g + 2]};
    float op, so[3];
    gs_mcmc_relocated(a.model[3][g], sc, c, a.min_opacity, a.binom, op, so);
    a.model[1][3 * g] = so[0]; a.model[1][3 * g + 1] = so[1]; a.model[1][3 * g + 2] = so[2];
    a.model[3][g] = op;
    gs_rows_zero_sets(a.set, a.nsets, g, a.k3);
}

__global__ __launch_bounds__(256) void gs_mcmc_noise_kernel(float *__restrict__ means, const float *__restrict__ scales, const float *__restrict__ quats,
                                                             const float *__restrict__ opac, const float *__restrict__ z, int64_t n, float lr, float gate_k,
                                                             float gate_t) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    float m[3] = {means[3 * g], means[3 * g + 1], means[3 * g + 2]};
    const float sc[3] = {scales[3 * g], scales[3 * g + 1], scales[3 * g + 2]};
    const float zz[3] = {z[3 * g], z[3 * g + 1], z[3 * g + 2]};
    const float q[4] = {quats[4 * g], quats[4 * g + 1], quats[4 * g + 2], quats[4 * g + 3]};
    if (gs_mcmc_noise(m, sc, q, opac[g], zz, lr, gate_k, gate_t)) { means[3 * g] = m[0]; means[3 * g + 1] = m[1]; means[3 * g + 2] = m[2]; }
}

__global__ __launch_bounds__(256) void gs_mcmc_regularize_kernel(const float *__restrict__ scales, const float *__restrict__ opac, float *__restrict__ d_scales,
                                                                  float *__restrict__ d_opac, int64_t n, float c_o, float c_s) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    if (d_opac) d_opac[g] = gs_mcmc_reg_opacity(d_opac[g], c_o, opac[g]);
    if (d_scales) {
#pragma unroll
        for (int j = 0; j < 3; ++j) d_scales[3 * g + j] = gs_mcmc_reg_scale(d_scales[3 * g + j], c_s, scales[3 * g + j]);
    }
}

hipError_t gs_launch_mcmc_plan(const float *opac, int64_t n, float min_opacity_logit, u64 *chunk_sum, u64 *chunk_off, u64 *totals, u64 *cdf, int32_t *dead,
                               hipStream_t s) {
    const hipError_t e = hipMemsetAsync(totals, 0, 2 * sizeof(u64), s);
    if (e != hipSuccess || n <= 0) return e;
    unsigned blocks;
    if (!gs_grid_256(n, &blocks)) return hipErrorInvalidValue;
    const int64_t nchunks = gs_chunks(n);
    hipLaunchKernelGGL(gs_mcmc_weigh_kernel, dim3(blocks), dim3(GS_CHUNK), 0, s, opac, n, min_opacity_logit, chunk_sum, nchunks);
    const hipError_t es = gs_launch_chunk_scan(chunk_sum, chunk_off, nchunks, 2, totals, s);   // (also reports the weigh launch)
    if (es != hipSuccess) return es;
    hipLaunchKernelGGL(gs_mcmc_emit_kernel, dim3(blocks), dim3(GS_CHUNK), 0, s, opac, n, min_opacity_logit, chunk_off, nchunks, cdf, dead);
    return hipGetLastError();
}

hipError_t gs_launch_mcmc_sample(const u64 *cdf, int64_t n, const float *u, int64_t m, int32_t *src, hipStream_t s) {
    if (n <= 0 || m <= 0) return hipSuccess;
    unsigned blocks;
    if (!gs_grid_256(m, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gs_mcmc_sample_kernel, dim3(blocks), dim3(256), 0, s, cdf, n, u, m, src);
    return hipGetLastError();
}

hipError_t gs_launch_mcmc_relocate(const GsMcmcRelocateArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.m <= 0) return hipSuccess;
    unsigned bm, bn;
    if (!gs_grid_256(a.m, &bm) || !gs_grid_256(a.n, &bn) || a.nsets < 0 || a.nsets > GS_DENSITY_MAX_SETS || a.k3 <= 0 || !a.src || !a.dst || !a.hist || !a.binom)
        return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(a.hist, 0, sizeof(int32_t) * (size_t)a.n, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gs_mcmc_count_kernel, dim3(bm), dim3(256), 0, s, a);
    hipLaunchKernelGGL(gs_mcmc_move_kernel, dim3(bm), dim3(256), 0, s, a);
    hipLaunchKernelGGL(gs_mcmc_source_kernel, dim3(bn), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t gs_launch_mcmc_noise(float *means, const float *scales, const float *quats, const float *opac, const float *z, int64_t n, float lr, float gate_k,
                                float gate_t, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    unsigned blocks;
    if (!gs_grid_256(n, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gs_mcmc_noise_kernel, dim3(blocks), dim3(256), 0, s, means, scales, quats, opac, z, n, lr, gate_k, gate_t);
    return hipGetLastError();
}

hipError_t gs_launch_mcmc_regularize(const float *scales, const float *opac, float *d_scales, float *d_opac, int64_t n, float c_opacity, float c_scale,
                                     hipStream_t s) {
    if (n <= 0 || (!d_scales && !d_opac)) return hipSuccess;
    unsigned blocks;
    if (!gs_grid_256(n, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gs_mcmc_regularize_kernel, dim3(blocks), dim3(256), 0, s, scales, opac, d_scales, d_opac, n, c_opacity, c_scale);
    return hipGetLastError();
}
