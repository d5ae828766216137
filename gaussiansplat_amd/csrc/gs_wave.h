// gs_wave.h -- the wave (64 lanes) and workgroup primitives of the kernels, written ONCE.  Device only.  Two conventions, stated here and
// nowhere else:
//   the _down sums (gs_wave_sum_down, gs_block_sum)  a __shfl_down ladder: the wave's sum is valid in LANE 0 ONLY.  gs_block_sum then adds the
//                                                     waves' sums in ascending order and returns that in every thread.
//   the tree sums (gs_wave_sum, gs_block_tree_row,    a butterfly: valid in EVERY lane, and bit-reproducible -- both partners of a pair form
//                  gs_tree_finish_rows)               a + b and b + a, the waves are added as (w0 + w1) + (w2 + w3), nothing depends on dispatch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---------------------------------------------------------------- sums by __shfl_down
// The sum of v over the wave's 64 lanes (uint32_t, int, unsigned long long, float, double): lane 0 holds it, the other lanes hold partial sums.
template <class T>
__device__ __forceinline__ T gs_wave_sum_down(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;
}
// The sum of v over a workgroup of nwaves waves, in every thread: wave sums, lane 0 of wave w into sm[w], a barrier, then sm[0] + sm[1] + ... in
// ascending order (floating point: ((s0 + s1) + s2) + s3).  LEAD: a barrier before the LDS write too, for a caller whose sm may still be read.
template <bool LEAD = false, class T>
__device__ __forceinline__ T gs_block_sum(T v, T *sm, int nwaves) {
    v = gs_wave_sum_down(v);
    if (LEAD) __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = T(-0.0);                                         // the identity of + in floating point too: -0.0 + x is x bit for bit (0 for the integers)
    for (int i = 0; i < nwaves; ++i) t += sm[i];
    return t;
}

// ---------------------------------------------------------------- the reproducible sums
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
// NV values summed over a workgroup of WAVES = 4 waves: value(0), value(1), ... ONE AFTER ANOTHER through gs_wave_sum (a caller that forms
// value(c) from its factors when its turn comes never holds NV live doubles), lane 0 of each wave into LDS, one barrier, and thread c < NV
// hands (w0 + w1) + (w2 + w3) of value c to emit(c, sum), which stores it: as a double into a row of partials, or rounded once to float.
// The LDS is the function's own and nothing guards it for a second call: once per kernel.
template <int NV, int WAVES, class F, class E>
__device__ __forceinline__ void gs_block_tree_row(F value, E emit) {
#pragma clang fp contract(off)
    static_assert(WAVES == 4, "the tree over the waves is written for four");
    __shared__ double swave[NV][WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        const double s = gs_wave_sum(value(c));
        if (lane == 0) swave[c][wv] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const double *w = swave[threadIdx.x];
        emit((int)threadIdx.x, (w[0] + w[1]) + (w[2] + w[3]));
    }
}
// The body of a finishing workgroup of BLOCK threads over `rows` rows of NV doubles (16-byte aligned): thread t sums the rows t, t + BLOCK, ...
// in that order -- one pass with NV accumulators, so that the NV / 2 16-byte loads of a row are independent and a thread waits for memory once
// per row it owns (one workgroup on the whole chip: its registers cost nobody anything) -- then gs_block_tree_row with the same emit.
template <int NV, int BLOCK, class Index, class E>
__device__ __forceinline__ void gs_tree_finish_rows(const double *__restrict__ partials, Index rows, E emit) {
#pragma clang fp contract(off)
    static_assert(NV % 2 == 0, "two columns per 16-byte load");
    double acc[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) acc[c] = 0.0;
    for (Index r = threadIdx.x; r < rows; r += BLOCK) {
        const double2 *row = reinterpret_cast<const double2 *>(partials + (size_t)r * NV);
#pragma unroll
        for (int q = 0; q < NV / 2; ++q) { const double2 v = row[q]; acc[2 * q] = acc[2 * q] + v.x; acc[2 * q + 1] = acc[2 * q + 1] + v.y; }
    }
    gs_block_tree_row<NV, BLOCK / 64>([&](int c) { return acc[c]; }, emit);
}

// ---------------------------------------------------------------- ranks inside a wave
// The wave's vote on pred: the ballot word (lane i is bit i), the number of set lanes below `lane`, and the wave's count.
struct GsWaveRank { unsigned long long ballot; int below, count; };
__device__ __forceinline__ GsWaveRank gs_wave_rank(bool pred, int lane) {
    const unsigned long long b = __ballot(pred);
    return {b, (int)__popcll(b & ((1ull << lane) - 1ull)), (int)__popcll(b)};
}

// ---------------------------------------------------------------- the XCD tile order
// The tile `id` of workgroup `block` out of T tiles in row-major order; false: the workgroup has none (the grid is 8 ceil(T / 8)).  The dispatcher
// deals workgroups to the 8 XCDs round-robin (block b runs on XCD b % 8), each XCD with its own L2; in plain grid order the eight tiles around a
// tile sit on eight different XCDs and every one fetches the shared halo from memory itself.  Here XCD x works through the x-th eighth of the
// tiles in row-major order, so the tiles in flight on an XCD are neighbours (the loss kernels: stats 109 -> 105 us, grad 72 -> 68 us at
// 1920x1080x3).  (Persistent workgroups that fetch the next tile's halo before the stencil of the current one were measured too, into registers
// and by LDS-DMA into a second pair of buffers: 111 / 114 us for the stats kernel against 105 -- the kernel is bound by its 2700 VALU
// instructions per wave, not by the fetch; profiles/r04m_loss_persistent.log, r04n_loss_lds_dma.log.)
__device__ __forceinline__ bool gs_xcd_tile(unsigned block, int T, int &id) {
    const int chunk = (T + 7) / 8;
    const int k = (int)(block >> 3);
    id = (int)(block & 7u) * chunk + k;
    return k < chunk && id < T;
}
