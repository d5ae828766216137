// gs_chunk.hip -- the one scan of the chunk words (gs_chunk.h).  Integers only: exact in any order, no flags of its own in build.py.
#include "gs_chunk.h"

// One workgroup per row of `nchunks` words (blockIdx.x: the touched-rows pack has one row, its rebuild one per view, a density plan one per
// class, an MCMC plan two): exclusive prefix sums, and the row's total when `total` is not null.  Every thread sums a contiguous span, the
// 1024 span sums are scanned in LDS.  C: a chunk's word, O: an offset (5 M gaussians = 19.5 k words, 20 per thread).
template <class C, class O>
__global__ __launch_bounds__(1024) void gs_chunk_scan_kernel(const C *__restrict__ chunk_cnt, O *__restrict__ chunk_off, int64_t nchunks, O *__restrict__ total) {
    __shared__ O s[2][1024];
    const C *c = chunk_cnt + (int64_t)blockIdx.x * nchunks;
    O *o = chunk_off + (int64_t)blockIdx.x * nchunks;
    const int t = threadIdx.x;
    const int64_t per = (nchunks + 1023) / 1024;
    const int64_t lo = min((int64_t)t * per, nchunks), hi = min(lo + per, nchunks);
    O sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += c[i];
    s[0][t] = sum;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < 1024; d <<= 1) {                                   // reads s[cur], writes s[cur ^ 1]: one barrier per step
        O v = s[cur][t];
        if (t >= d) v += s[cur][t - d];
        s[cur ^ 1][t] = v;
        __syncthreads();
        cur ^= 1;
    }
    O run = s[cur][t] - sum;
    for (int64_t i = lo; i < hi; ++i) { o[i] = run; run += c[i]; }
    if (t == 1023 && total) total[blockIdx.x] = s[cur][1023];
}

template <class C, class O>
static hipError_t chunk_scan(const C *chunk_cnt, O *chunk_off, int64_t nchunks, int rows, O *totals, hipStream_t s) {
    hipLaunchKernelGGL((gs_chunk_scan_kernel<C, O>), dim3((unsigned)rows), dim3(1024), 0, s, chunk_cnt, chunk_off, nchunks, totals);
    return hipGetLastError();
}
hipError_t gs_launch_chunk_scan(const uint32_t *chunk_cnt, int64_t *chunk_off, int64_t nchunks, int rows, int64_t *totals, hipStream_t s) {
    return chunk_scan(chunk_cnt, chunk_off, nchunks, rows, totals, s);
}
hipError_t gs_launch_chunk_scan(const unsigned long long *chunk_sum, unsigned long long *chunk_off, int64_t nchunks, int rows, unsigned long long *totals,
                                hipStream_t s) {
    return chunk_scan(chunk_sum, chunk_off, nchunks, rows, totals, s);
}
