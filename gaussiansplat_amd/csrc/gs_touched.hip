// gs_touched.hip -- the touched-rows colour exchange on the device (multi-GPU, distributed.multi_view_step(sync = "touched")).
//
// A view's composite adjoint leaves d rgb = 0 for every gaussian no pixel evaluated (63 % of them at C3), so a view travels as a
// bitmap of n bits plus the three floats of every TOUCHED gaussian, in gaussian order.  Gaussian g is touched when any of its three
// floats has (bit pattern & 0x7fffffff) != 0: +-0 is untouched; denormals, NaN and Inf are touched (the bit pattern is tested, not
// the float: the denormal mode cannot change the answer).  Bit g % 32 of int32 word g / 32; the bits of the last word beyond n are 0.
//
// PACK (one view): the ordered compaction of gs_chunk.h -- three launches over chunks of GS_CHUNK = 256 gaussians (one workgroup,
// four wave64 ballots = eight bitmap words):
//   gs_touched_mark_kernel     per chunk: ballots -> bitmap words, popcounts -> the chunk's count
//   gs_launch_chunk_scan       ONE workgroup: exclusive scan of the chunk counts (5 M gaussians = 19.5 k counts, 20 per thread),
//                              and the total -> *count
//   gs_touched_scatter_kernel  per chunk: every lane re-derives its rank from the chunk's eight bitmap words and copies its row
// The source is a caller's dense [n][3] array or the ctx's own 2-D gradient sums (float, or fixed point in deterministic mode,
// converted exactly as gs_pack_drgb_kernel does: the touched test is made on the converted float).
//
// REBUILD (all gathered views): gs_sh_from_touched_kernel is gs_sh_from_views_kernel (one body: gs_sh_views_body.inc) whose three
// floats of (view v, gaussian g) are loaded from rows[v][offset of g's chunk + rank within the chunk] when bit g of view v is set and
// from three +0 floats otherwise -- the arithmetic of an untouched view is NOT skipped (a non-finite basis times zero must give what the
// dense path gives), so the result equals gs_sh_from_views_kernel on the unpacked array bit for bit.  Its workgroup covers one
// chunk, so per view it needs ONE offset and its own eight words, all wave-uniform loads.  A pre-pass of two launches
// (gs_touched_count_kernel: popcounts per (view, chunk); gs_launch_chunk_scan, one workgroup per view) makes the offsets.
// Nothing is read outside a view's rows_cap rows whatever the bitmap says: bits at positions >= n belong to no thread, and a
// rank >= rows_cap (a corrupt or truncated gather) reads as a zero row.
#include "gs_pergaussian.h"   // gs_g2d_rgb_load; gs_sh_views_body.inc keeps its own t and p (this unit contracts, and both kernels share that body)
#include "gs_chunk.h"
#include "gs_sh.h"
#include "gs_wave.h"

#define GS_TOUCHED_WORDS (GS_CHUNK / 32)

struct GsColorRowSrc {
    const float *dense;                 // SRC 0: [n][3]
    const float *g2d;                   // SRC 1: the composite backward's float sums, GS_G2D_STRIDE per gaussian, d rgb first
    const long long *g2d_fixed;         // SRC 2: ... its fixed-point sums (deterministic mode)
};
template <int SRC>
__device__ __forceinline__ void load_row(const GsColorRowSrc &s, int64_t g, float &a, float &b, float &c) {
    if constexpr (SRC == 0) { const float *p = s.dense + 3 * g; a = p[0]; b = p[1]; c = p[2]; }
    else {
        __builtin_assume(SRC != 2 || s.g2d_fixed != nullptr);              // (SRC is the launcher's reading of these pointers)
        gs_g2d_rgb_load(GsG2dRows{s.g2d, SRC == 2 ? s.g2d_fixed : nullptr}, g, a, b, c);
    }
}
__device__ __forceinline__ bool touched3(float a, float b, float c) {
    return ((__float_as_uint(a) | __float_as_uint(b) | __float_as_uint(c)) & 0x7fffffffu) != 0u;
}

// Gaussian `local` of chunk `chunk` in one view's bitmap (`words` words): is its bit set, and how many set bits of the chunk
// precede it.  The eight loads are the same for every lane of the workgroup (words past the end of the bitmap read as 0).  Kept free of
// branches: the rebuild's per-view loop body then stays ONE basic block, as in the dense kernel, and is vectorised and fused alike.
__device__ __forceinline__ bool touched_rank(const int32_t *__restrict__ bits, int64_t words, int64_t chunk, int local, uint32_t &rank) {
    const int mw = local >> 5, bit = local & 31;
    uint32_t before = 0, mine = 0;
#pragma unroll
    for (int j = 0; j < GS_TOUCHED_WORDS; ++j) {
        const int64_t wi = chunk * GS_TOUCHED_WORDS + j;
        const uint32_t raw = (uint32_t)bits[min(wi, words - 1)];            // an unconditional clamped load, then a select: no branch
        const uint32_t w = wi < words ? raw : 0u;
        before += j < mw ? (uint32_t)__popc(w) : 0u;
        mine = j == mw ? w : mine;
    }
    rank = before + (uint32_t)__popc(mine & ((1u << bit) - 1u));
    return ((mine >> bit) & 1u) != 0u;
}

template <int SRC>
__global__ __launch_bounds__(GS_CHUNK) void gs_touched_mark_kernel(GsColorRowSrc src, int64_t n, int32_t *__restrict__ bits, int64_t words,
                                                                            uint32_t *__restrict__ chunk_cnt) {
    __shared__ int wave_cnt[GS_CHUNK_WAVES];
    const int64_t g = (int64_t)blockIdx.x * GS_CHUNK + threadIdx.x;
    bool t = false;
    if (g < n) {                                                           // lanes past n vote 0: the padding bits of the last word
        float a, b, c;
        load_row<SRC>(src, g, a, b, c);
        t = touched3(a, b, c);
    }
    const GsWaveRank r = gs_wave_rank(t, threadIdx.x & 63);               // (the vote in front of lane and wv, as it stood: the kernel's schedule follows the order)
    const unsigned long long bal = r.ballot;                               // wave64: two words, low lanes first
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t wi = (int64_t)blockIdx.x * GS_TOUCHED_WORDS + 2 * wv;
    if (lane == 0 && wi < words) bits[wi] = (int32_t)(uint32_t)bal;
    if (lane == 32 && wi + 1 < words) bits[wi + 1] = (int32_t)(uint32_t)(bal >> 32);
    if (lane == 0) wave_cnt[wv] = r.count;
    __syncthreads();
    if (threadIdx.x == 0) chunk_cnt[blockIdx.x] = (uint32_t)gs_chunk_count(wave_cnt);
}

// popcounts per (view = blockIdx.y, chunk) of gathered bitmaps [views][words]; bits at positions >= n are ignored
__global__ __launch_bounds__(256) void gs_touched_count_kernel(const int32_t *__restrict__ bits, int64_t words, int64_t n,
                                                                uint32_t *__restrict__ chunk_cnt, int64_t nchunks) {
    const int64_t wi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t w = wi < words ? (uint32_t)bits[(int64_t)blockIdx.y * words + wi] : 0u;
    if (wi == words - 1 && (n & 31)) w &= (1u << (int)(n & 31)) - 1u;
    int p = __popc(w);
    p += __shfl_xor(p, 1); p += __shfl_xor(p, 2); p += __shfl_xor(p, 4);  // the eight words of a chunk sit in eight neighbouring lanes
    const int64_t chunk = wi / GS_TOUCHED_WORDS;
    if ((threadIdx.x & (GS_TOUCHED_WORDS - 1)) == 0 && chunk < nchunks) chunk_cnt[(int64_t)blockIdx.y * nchunks + chunk] = (uint32_t)p;
}

template <int SRC>
__global__ __launch_bounds__(GS_CHUNK) void gs_touched_scatter_kernel(GsColorRowSrc src, int64_t n, const int32_t *__restrict__ bits, int64_t words,
                                                                               const int64_t *__restrict__ chunk_off, float *__restrict__ rows) {
    const int64_t g = (int64_t)blockIdx.x * GS_CHUNK + threadIdx.x;
    if (g >= n) return;
    uint32_t rank;
    if (!touched_rank(bits, words, blockIdx.x, threadIdx.x, rank)) return;
    float a, b, c;
    load_row<SRC>(src, g, a, b, c);                                        // plain loads and stores: the 32 bits travel as they are
    float *r = rows + 3 * (chunk_off[blockIdx.x] + (int64_t)rank);          // rank < the total <= n: inside the caller's 3 n floats
    r[0] = a; r[1] = b; r[2] = c;
}

// Where the three floats d rgb of (view v, gaussian of this thread) are: in the gathered rows [views][rows_cap][3] when the bit
// of the gathered bitmaps [views][words] is set, else in `zero` (three +0 floats in device memory).  An ADDRESS is chosen, not a
// value: the body then loads the floats as the dense kernel does, and the compiler sees the same arithmetic in both (with a value
// chosen between a load and a literal 0 it pulled the products into the branch and no longer fused them with the sums).
// The workgroup is chunk blockIdx.x.
struct GsTouchedColorSrc {
    const int32_t *bits;
    const float *rows;
    const int64_t *chunk_off;              // [views][nchunks]
    const float *zero;
    int64_t words, nchunks, rows_cap;
    __device__ __forceinline__ const float *row(int v) const {
        uint32_t rank;
        const bool t = touched_rank(bits + (int64_t)v * words, words, blockIdx.x, threadIdx.x, rank);
        const int64_t r = chunk_off[(int64_t)v * nchunks + blockIdx.x] + (int64_t)rank;
        return (t && r < rows_cap) ? rows + ((int64_t)v * rows_cap + r) * 3 : zero;
    }
};

template <int DEG, bool OVERWRITE, bool STRIDED = false>
__global__ __launch_bounds__(GS_CHUNK) void gs_sh_from_touched_kernel(int64_t n, const float *__restrict__ means, int nviews,
                                                                               const float *__restrict__ cams, GsTouchedColorSrc src,
                                                                               float *__restrict__ d_shs, int sh_stride) {
#define GS_SH_VIEWS_BEGIN const float *gr = src.row(v);      // the integer work first: the arithmetic behind it is then laid out as in the dense kernel
#define GS_SH_VIEWS_DRGB const float g0 = gr[0], g1 = gr[1], g2 = gr[2];
#include "gs_sh_views_body.inc"
#undef GS_SH_VIEWS_DRGB
#undef GS_SH_VIEWS_BEGIN
}

hipError_t gs_launch_touched_pack(const float *dense, const float *g2d, const long long *g2d_fixed, int64_t n, int32_t *bits, float *rows,
                                  int64_t *count, uint32_t *chunk_cnt, int64_t *chunk_off, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t nchunks = gs_chunks(n), words = (n + 31) / 32;
    if (nchunks > 0x7fffffffLL) return hipErrorInvalidValue;
    const GsColorRowSrc src{dense, g2d, g2d_fixed};
    const dim3 grid((unsigned)nchunks), block(GS_CHUNK);
#define GS_TP(K, ...) do { if (dense) hipLaunchKernelGGL(K<0>, grid, block, 0, s, __VA_ARGS__); \
                           else if (g2d_fixed) hipLaunchKernelGGL(K<2>, grid, block, 0, s, __VA_ARGS__); \
                           else hipLaunchKernelGGL(K<1>, grid, block, 0, s, __VA_ARGS__); } while (0)
    GS_TP(gs_touched_mark_kernel, src, n, bits, words, chunk_cnt);
    const hipError_t e = gs_launch_chunk_scan(chunk_cnt, chunk_off, nchunks, 1, count, s);   // (also reports the mark launch)
    if (e != hipSuccess) return e;
    GS_TP(gs_touched_scatter_kernel, src, n, (const int32_t *)bits, words, (const int64_t *)chunk_off, rows);
#undef GS_TP
    return hipGetLastError();
}

hipError_t gs_launch_sh_from_touched(int64_t n, int sh_degree, int sh_stride, const float *means, int nviews, const float *cams, const int32_t *bits,
                                     const float *rows, int64_t rows_cap, uint32_t *chunk_cnt, int64_t *chunk_off, const float *zero3,
                                     float *d_shs, int overwrite, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t nchunks = gs_chunks(n), words = (n + 31) / 32;
    if (nchunks > 0x7fffffffLL || nviews <= 0 || nviews > 65535) return hipErrorInvalidValue;
    // sh_degree: the ACTIVE degree; sh_stride: floats per stored row of d_shs
    return gs_sh_dispatch(sh_degree, sh_stride, [&](auto D, auto S) {
        hipLaunchKernelGGL(gs_touched_count_kernel, dim3((unsigned)((words + 255) / 256), (unsigned)nviews), dim3(256), 0, s, bits, words, n, chunk_cnt, nchunks);
        const hipError_t e = gs_launch_chunk_scan(chunk_cnt, chunk_off, nchunks, nviews, nullptr, s);   // (also reports the count launch)
        if (e != hipSuccess) return e;
        constexpr int DEG = decltype(D)::value, K = (DEG + 1) * (DEG + 1);
        constexpr bool STRIDED = decltype(S)::value;
        const GsTouchedColorSrc src{bits, rows, chunk_off, zero3, words, nchunks, rows_cap};
        const dim3 grid((unsigned)nchunks), block(GS_CHUNK);
        const size_t lds = sizeof(float) * GS_CHUNK * (3 * K + 1);
        if (overwrite) hipLaunchKernelGGL((gs_sh_from_touched_kernel<DEG, true, STRIDED>), grid, block, lds, s, n, means, nviews, cams, src, d_shs, sh_stride);
        else hipLaunchKernelGGL((gs_sh_from_touched_kernel<DEG, false, STRIDED>), grid, block, lds, s, n, means, nviews, cams, src, d_shs, sh_stride);
        return hipGetLastError();
    });
}
