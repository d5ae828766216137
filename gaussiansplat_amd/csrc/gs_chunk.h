// gs_chunk.h -- ordered compaction over chunks of 256 gaussians WITHOUT any workgroup waiting for another, written ONCE.
// Three launches: a kernel of one workgroup per chunk leaves one word per chunk (a count, or a sum), gs_launch_chunk_scan turns every row of
// such words into exclusive offsets and the row's total, and a second kernel per chunk re-derives every thread's place inside the chunk
// and adds the chunk's offset.  Users: the touched-rows pack and rebuild (gs_touched.hip), the density plan and restructure
// (gs_density.hip), the MCMC plan (gs_mcmc.hip).  The per-gaussian backward's selective compaction and Adam's one-wave compaction are not
// users: the first forms "the waves before mine" and the total in one loop, the second has one wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GS_CHUNK 256                  // gaussians per workgroup: four wave64 ballots, eight bitmap words
#define GS_CHUNK_WAVES (GS_CHUNK / 64)
static_assert(GS_CHUNK == 256, "one workgroup of 256 threads = four wave64 ballots (eight bitmap words) per chunk");
inline int64_t gs_chunks(int64_t n) { return (n + GS_CHUNK - 1) / GS_CHUNK; }

// gs_chunk.hip: exclusive prefix sums of `rows` rows of nchunks per-chunk words, one workgroup per row (the views of a touched-rows
// rebuild, the classes of a density plan, {weights, dead} of an MCMC plan); totals (may be null): the rows' sums.  32-bit counts give
// 64-bit offsets, 64-bit sums give 64-bit offsets.  Any number of chunks: every thread sums a contiguous span.
hipError_t gs_launch_chunk_scan(const uint32_t *chunk_cnt, int64_t *chunk_off, int64_t nchunks, int rows, int64_t *totals, hipStream_t s);
hipError_t gs_launch_chunk_scan(const unsigned long long *chunk_sum, unsigned long long *chunk_off, int64_t nchunks, int rows, unsigned long long *totals,
                                hipStream_t s);

// ---------------------------------------------------------------- inside a chunk's workgroup: wave[w] is what wave w left in LDS (T: int or 64-bit)
// the chunk's word: the sum over its waves
template <class T>
__device__ __forceinline__ T gs_chunk_count(const T *wave) {
    T s = 0;
#pragma unroll
    for (int w = 0; w < GS_CHUNK_WAVES; ++w) s += wave[w];
    return s;
}
// what the waves before wave `wv` hold: a thread's place in the chunk is this plus its rank (or its inclusive sum) inside its wave.  A select,
// not a loop bound: every thread reads the four words
template <class T>
__device__ __forceinline__ T gs_chunk_before(const T *wave, int wv) {
    T s = 0;
#pragma unroll
    for (int w = 0; w < GS_CHUNK_WAVES; ++w) s += w < wv ? wave[w] : T(0);
    return s;
}

// ---------------------------------------------------------------- rows of the five model arrays, moved by their own thread
// floats per row of array i of (means, scales, quaternions, opacities, SH rows); k3: floats of an SH row
__device__ __forceinline__ int gs_row_width(int i, int k3) { return i < 2 ? 3 : i == 2 ? 4 : i == 3 ? 1 : k3; }

// w floats of row `srow` of src to row `drow` of dst, bit for bit (src null: +0).  16-byte accesses when the rows are 16-byte aligned.  dst and
// src may be one array (an MCMC relocation moves rows inside the model): no __restrict__.
__device__ __forceinline__ void gs_row_put(float *dst, int64_t drow, const float *src, int64_t srow, int w) {
    float *d = dst + drow * w;
    const float *s = src ? src + srow * w : nullptr;
    const bool vec = (w & 3) == 0 && ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0;
    if (vec) {
        for (int j = 0; j < w; j += 4)
            *reinterpret_cast<float4 *>(d + j) = s ? *reinterpret_cast<const float4 *>(s + j) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else {
        for (int j = 0; j < w; ++j) d[j] = s ? s[j] : 0.0f;
    }
}
// The gradient-shaped companion sets (Adam's moments) of a row: +0 into row `row` of every array that is there ...
template <int SETS>
__device__ __forceinline__ void gs_rows_zero_sets(float *const (&set)[SETS][5], int nsets, int64_t row, int k3) {
    for (int t = 0; t < nsets; ++t)
#pragma unroll
        for (int i = 0; i < 5; ++i)
            if (set[t][i]) gs_row_put(set[t][i], row, nullptr, 0, gs_row_width(i, k3));
}
// ... or row `srow` of src to row `drow` of dst, where both arrays are there
template <int SETS>
__device__ __forceinline__ void gs_rows_copy_sets(float *const (&dst)[SETS][5], const float *const (&src)[SETS][5], int nsets, int64_t drow, int64_t srow, int k3) {
    for (int t = 0; t < nsets; ++t)
#pragma unroll
        for (int i = 0; i < 5; ++i)
            if (dst[t][i] && src[t][i]) gs_row_put(dst[t][i], drow, src[t][i], srow, gs_row_width(i, k3));
}
