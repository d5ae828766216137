// gs_order.hip -- the longest-first launch orders of the composite kernels (gs_config.schedule 3 / 4) and the small kernels beside them:
// tile_lpt_order_kernel and its layout (gs_lpt_order_len), the two summing kernels (per-tile work counters, written entries of capped
// lists) and the clock probe.  Nothing here composites: gs_composite.hip reads an order's entries (tile_of_block; the entry format and
// GS_LPT_NONE stand in gs_common.h), the host side keeps the orders per view slot (gs_ctx::ViewSlot, build_frame_order).
// Built like gs_composite.hip (build.py: same flags, contraction off), so that the kernels are what they were inside that unit.
#include "gs_common.h"
#include "gs_wave.h"
#pragma clang fp contract(off)
// Longest-first order for a PLAIN launch (gs_config.schedule 3 / 4).  The dispatcher hands workgroups out in blockIdx order,
// round-robin over the XCDs: block b runs on XCD b % 8.  order[8 j + x] is therefore the j-th tile of XCD x, and the kernel
// decides two things.
// (1) WHICH tiles an XCD gets.  Round 2 / early round 3 kept what the plain tile order has (XCD = tile % 8): neighbours in x on
//     eight different XCDs, so a gaussian's payload row was fetched by nearly every XCD whose L2 it then filled.  Now the tiles are
//     dealt in GROUPS of 8 x 8 (lpt_group_side): the groups are ranked by their work and dealt to the XCDs in snake order (rank k ->
//     XCD k % 8, every second round reversed), which balances the XCDs' work to better than 1 % on the synthetic scenes
//     (tools/xcd_order.py) and gives every XCD spatially compact sets of tiles.  Measured at C3 (rocprofv3 FETCH_SIZE, per launch):
//     forward 338 -> 202 MB, backward 378 -> 225 MB requested from the fabric -- backward traffic 1.02 x its algorithmic bytes.
// (2) IN WHICH ORDER an XCD starts its tiles: heavier first, so the workgroups that start last are the lightest ones and the
//     kernel ends without a tail (C3 backward round 2: 0.84 -> 0.74 ms).  A STABLE counting sort on NB work classes (work / max in
//     NB steps); inside a class the tiles stay in (group, row, column) order, so neighbours still start together.  Only the START
//     order of the light tail matters for the balance -- with 5 waves per SIMD the first 5120 of C3's 8160 tiles start at once
//     whatever their order -- so a few classes lose nothing.
// Ranks come from an LDS bitmap [XCD][class][slot]: slot = 64 * (ordinal of the tile's group on its XCD) + position in the group;
// atomic OR (order free), word prefix, popcount below the own bit -- the construction of the level-1 binning (gs_bin3.hip).
// An XCD's list may be shorter than the longest one: the holes of `order` hold GS_LPT_NONE and their workgroups exit at once;
// order has gs_lpt_order_len(gx, gy) entries and that is the launch's grid.  One workgroup; work = src[t], or the list length
// (ranges_mode).
#ifndef GS_LPT_BUCKETS
#define GS_LPT_BUCKETS 32
#endif
// group side: 8 tiles (a gaussian of the C3 scene covers 5-6 tiles across), smaller on small grids so that every XCD still gets
// sixteen or more groups to balance with (config C2, 50 x 50 tiles: 4; a 16 x 16 grid: single tiles, i.e. longest-first over the XCDs)
static inline int lpt_groups(int gx, int gy, int gs) { return ((gx + gs - 1) / gs) * ((gy + gs - 1) / gs); }
static inline int lpt_group_side(int gx, int gy) {
    for (int gs = 8; gs > 1; gs >>= 1) if (lpt_groups(gx, gy, gs) >= 128) return gs;
    return 1;
}
int gs_lpt_order_len(int gx, int gy) { const int gs = lpt_group_side(gx, gy); return 8 * gs * gs * ((lpt_groups(gx, gy, gs) + 7) / 8); }

// (3) SPLIT TILES (round 5; front > 0).  A trained scene's work is heavy-tailed: a tile whose list is ten times the median is one wave64
//     running alone long after the rest of the chip has drained (measured on the clustered scene of tools/clustered_probe.py: 55 % of the
//     SIMD time idle).  A tile whose work is at least (sum of all work) / split_div -- about what a wave slot gets when the work is spread
//     evenly -- is composited by two waves, from twice that by four, each owning two or one of the tile's four 16 x 4 pixel strips (the
//     machinery of gs_config.tile_parts).  Its first part keeps the tile's place in the order (entry = tile | log2(parts) << 30); the other
//     parts go to the FRONT region order[0 .. front) -- they are among the heaviest units of the launch and must start first.  Only the
//     front / 24 heaviest tiles of every XCD's list are eligible (the heaviest must never be the one left whole): the tile at position
//     pos of XCD x owns the entries order[8 (3 pos + j) + x], j = 0 .. 2.  The ordinary entries follow from order[front] on; unused
//     entries of the front region hold GS_LPT_NONE (an empty workgroup).  front = 0: no tile is split.
__global__ __launch_bounds__(1024) void tile_lpt_order_kernel(const uint32_t *__restrict__ src, int ranges_mode, int ntiles, int gx, int ng, int gs, int nb,
                                                               uint32_t *__restrict__ order, unsigned long long *__restrict__ zero14, int front, int split_div,
                                                               const uint32_t *__restrict__ walked, uint32_t *__restrict__ zero_words,
                                                               uint32_t *__restrict__ host_nsplit) {
    extern __shared__ uint32_t lds[];
    __shared__ uint32_t wmax, wtot, nsplit;
    __shared__ uint32_t rowtot[8 * 32], rowstart[8 * 32], xcount[8];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int GT = gs * gs;                                              // tiles of a full group (gs = 8, 4, 2 or 1: a power of two)
    const int ordmax = (ng + 7) >> 3;                                    // groups per XCD (upper bound)
    const int per = ordmax * GT;                                         // slots per XCD
    const int W = (per + 31) >> 5;                                       // bitmap words per row
    const int rows = 8 * nb;                                             // row = XCD * nb + class
    const int ngx = (gx + gs - 1) / gs;
    uint32_t *bm = lds;                                                  // [rows][W]
    uint32_t *gsum = bm + rows * W;                                      // [ng] work of the group
    uint16_t *pre = reinterpret_cast<uint16_t *>(gsum + ng);             // [rows][W] set bits of the row below word w
    uint16_t *ginfo = pre + rows * W;                                    // [ng] XCD | ordinal << 3
    uint8_t *cls = reinterpret_cast<uint8_t *>(ginfo + ng + (ng & 1) + ((rows * W) & 1));   // [ntiles]
    for (int i = tid; i < rows * W + ng; i += 1024) bm[i] = 0;          // bitmap and group sums
    for (int i = tid; i < front; i += 1024) order[i] = GS_LPT_NONE;     // the front region: filled by the split tiles at the very end
    uint32_t *seg_len = order + front + 8 * per;                        // [front / 3] list entries per backward segment of the split tiles (0: none)
    if (front > 0) for (int i = tid; i < front / 3; i += 1024) { seg_len[i] = 0; if (zero_words) zero_words[i] = 0; }
    if (tid == 0) { wmax = 1; nsplit = 0; }
    if (zero14 && tid < 14) zero14[tid] = 0ull;
    __syncthreads();
    // the tiles' work is read twice (maximum + group sums, then classes), eight independent loads in flight per thread each time:
    // the second read comes from L2, and a copy in LDS would not fit beside the bitmap for 4K-class grids
    auto load8 = [&](int t0, uint32_t (&v)[8]) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int t = t0 + k * 1024 + tid;
            v[k] = 0;
            if (t < ntiles) v[k] = ranges_mode ? src[2 * t + 1] - src[2 * t] : src[t];
        }
    };
    auto group_of = [&](int t, int &local) {
        const int ty = t / gx, tx = t - ty * gx;
        local = (ty & (gs - 1)) * gs + (tx & (gs - 1));
        return (ty / gs) * ngx + tx / gs;
    };
    uint32_t m = 0;
    for (int t0 = 0; t0 < ntiles; t0 += 8 * 1024) {
        uint32_t v[8];
        load8(t0, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int t = t0 + k * 1024 + tid;
            m = max(m, v[k]);
            if (t < ntiles && v[k]) { int local; atomicAdd(&gsum[group_of(t, local)], v[k]); }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d));
    if (lane == 0) atomicMax(&wmax, m);
    __syncthreads();
    if (wv == 0) {                                                       // the frame's total work (the group sums are complete)
        uint32_t sw = 0;
        for (int g = lane; g < ng; g += 64) sw += gsum[g];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) sw += (uint32_t)__shfl_xor((int)sw, d);
        if (lane == 0) wtot = sw;
    }
    // rank of every group by work (ties by index), dealt in snake order: round r = rank / 8 gives each XCD one group
    for (int g = tid; g < ng; g += 1024) {
        const uint32_t mine = gsum[g];
        int rank = 0;
        for (int h = 0; h < ng; ++h) { const uint32_t o = gsum[h]; rank += (o > mine || (o == mine && h < g)) ? 1 : 0; }
        const int r = rank >> 3, x = (r & 1) ? 7 - (rank & 7) : (rank & 7);
        ginfo[g] = (uint16_t)(x | (r << 3));
    }
    __syncthreads();
    const float scale = (float)nb / (float)wmax;
    for (int t0 = 0; t0 < ntiles; t0 += 8 * 1024) {
        uint32_t v[8];
        load8(t0, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int t = t0 + k * 1024 + tid;
            if (t < ntiles) {
                const int c = min(nb - 1, max(0, nb - 1 - (int)((float)v[k] * scale)));        // class 0 = heaviest
                cls[t] = (uint8_t)c;
                int local;
                const uint32_t gi = ginfo[group_of(t, local)];
                const int i = (int)(gi >> 3) * GT + local;
                atomicOr(&bm[((int)(gi & 7u) * nb + c) * W + (i >> 5)], 1u << (i & 31));
            }
        }
    }
    __syncthreads();
    for (int r = wv; r < rows; r += 16) {                                // one wave per row: exclusive scan of the word popcounts
        uint32_t carry = 0;
        for (int w0 = 0; w0 < W; w0 += 64) {
            const int w = w0 + lane;
            const uint32_t c = w < W ? (uint32_t)__popc(bm[r * W + w]) : 0u;
            uint32_t incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(incl, d); if (lane >= d) incl += u; }
            if (w < W) pre[r * W + w] = (uint16_t)(carry + incl - c);
            carry += (uint32_t)__shfl((int)incl, 63);
        }
        if (lane == 0) rowtot[r] = carry;
    }
    __syncthreads();
    if (tid < 8) {                                                       // class starts inside each XCD's list, and its length
        uint32_t run = 0;
        for (int c = 0; c < nb; ++c) { rowstart[tid * nb + c] = run; run += rowtot[tid * nb + c]; }
        xcount[tid] = run;
    }
    __syncthreads();
    uint32_t *main_order = order + front;
    for (int i = tid; i < 8 * per; i += 1024)                            // holes behind the shorter lists
        if ((uint32_t)(i >> 3) >= xcount[i & 7]) main_order[i] = GS_LPT_NONE;
    const uint32_t thr = front > 0 ? max(wtot / (uint32_t)max(split_div, 1), 256u) : 0xFFFFFFFFu, eligible = (uint32_t)front / 24u;
    for (int t = tid; t < ntiles; t += 1024) {
        int local;
        const uint32_t gi = ginfo[group_of(t, local)];
        const int x = (int)(gi & 7u), r = x * nb + cls[t], i = (int)(gi >> 3) * GT + local;
        const uint32_t pos = rowstart[r] + pre[r * W + (i >> 5)] + (uint32_t)__popc(bm[r * W + (i >> 5)] & ((1u << (i & 31)) - 1u));
        uint32_t entry = (uint32_t)t;
        if (pos < eligible) {                                            // among the heaviest of its XCD (front = 0: nobody)
            const uint32_t w = ranges_mode ? src[2 * t + 1] - src[2 * t] : src[t];
            if (w >= thr) {
                const uint32_t pc = w >= 2u * thr ? 2u : 1u, extra = (1u << pc) - 1u;
                for (uint32_t j = 0; j < extra; ++j) order[8u * (3u * pos + j) + (uint32_t)x] = (uint32_t)t | ((j + 1u) << 28) | (pc << 30);
                entry |= pc << 30;
                atomicAdd(&nsplit, 1u);
                if (walked) {                                            // the backward's list segments: GS_SEG_MAX at most, none shorter than GS_SEG_MIN_LEN
                    const uint32_t wk = walked[t], per_seg = (wk + GS_SEG_MAX - 1) / GS_SEG_MAX;
                    const uint32_t sl = max((per_seg + 63u) & ~63u, (uint32_t)GS_SEG_MIN_LEN);
                    seg_len[8u * pos + (uint32_t)x] = wk > sl ? sl : 0u;   // (a walk of one segment: nothing to split)
                }
            }
        }
        main_order[8u * pos + (uint32_t)x] = entry;
    }
    if (host_nsplit) {                                                   // coherent pinned host word: how many tiles of this order are split (the host picks
        __syncthreads();                                                 // the composite kernels' instantiations by it; it holds 0xFFFFFFFF until this store lands)
        if (tid == 0) *host_nsplit = nsplit;
    }
}

hipError_t gs_launch_tile_lpt_order(const uint32_t *work_or_ranges, int ranges_mode, int gx, int gy, uint32_t *order, hipStream_t s,
                                    unsigned long long *zero14, int buckets, int front, int split_div, const uint32_t *walked, uint32_t *zero_words, uint32_t *host_nsplit) {
    const int ntiles = gx * gy;
    if (ntiles <= 0) return hipSuccess;
    if (ntiles > GS_LPT_MAX_TILES) return hipErrorInvalidValue;          // beyond 8K-class images: the callers keep launch order
    int nb = buckets > 0 && buckets <= 32 ? buckets : GS_LPT_BUCKETS;
    const int gs = lpt_group_side(gx, gy), ng = lpt_groups(gx, gy, gs), W = (gs_lpt_order_len(gx, gy) / 8 + 31) / 32;
    auto lds_of = [&](int b) { return (size_t)8 * b * W * 4 + (size_t)ng * 4 + ((size_t)8 * b * W + ng + 2) * 2 + (size_t)ntiles + 16; };
    while (nb > 2 && lds_of(nb) > 150 * 1024) nb >>= 1;                  // very large grids: fewer work classes
    const size_t lds = lds_of(nb);
    if (lds > 150 * 1024) return hipErrorInvalidValue;
    if (lds > 40 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(tile_lpt_order_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    if (front < 0 || (front % 24) || ntiles > (int)GS_ORDER_TILE_MASK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tile_lpt_order_kernel, dim3(1), dim3(1024), lds, s, work_or_ranges, ranges_mode, ntiles, gx, ng, gs, nb, order, zero14, front, split_div, walked, zero_words, host_nsplit);
    return hipGetLastError();
}

// ---------------------------------------------------------------- small helpers
// the per-tile work counters of a composite launch, summed when somebody asks (gs_get_work_counters, the radix binning paths)
__global__ __launch_bounds__(1024) void sum_tiles_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, int n,
                                                          unsigned long long *__restrict__ out) {
    __shared__ unsigned long long sm[2][16];
    unsigned long long sa = 0, sb = 0;
    for (int i = threadIdx.x; i < n; i += 1024) { if (a) sa += a[i]; if (b) sb += b[i]; }
    sa = gs_block_sum(sa, sm[0], 16); sb = gs_block_sum(sb, sm[1], 16);
    if (threadIdx.x == 0) { out[0] = sa; out[1] = sb; }
}
__global__ __launch_bounds__(1024) void sum_listed_kernel(const uint2 *__restrict__ ext, int n, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long sm[16];
    unsigned long long sa = 0;
    for (int i = threadIdx.x; i < n; i += 1024) sa += ext[i].x;
    sa = gs_block_sum(sa, sm, 16);
    if (threadIdx.x == 0) out[0] = sa;
}
hipError_t gs_launch_sum_listed(const uint2 *ext, int n, unsigned long long *out, hipStream_t s) {
    hipLaunchKernelGGL(sum_listed_kernel, dim3(1), dim3(1024), 0, s, ext, n, out);
    return hipGetLastError();
}
hipError_t gs_launch_sum_tiles(const uint32_t *a, const uint32_t *b, int n, unsigned long long *out, hipStream_t s) {
    hipLaunchKernelGGL(sum_tiles_kernel, dim3(1), dim3(1024), 0, s, a, b, n, out);
    return hipGetLastError();
}

__global__ void clock_probe_kernel(unsigned long long *__restrict__ out) {
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_amdgcn_s_memtime();
    unsigned long long r1 = r0;
    for (int i = 0; i < (1 << 20) && r1 - r0 < 2000ull; ++i) r1 = __builtin_amdgcn_s_memrealtime();      // 20 us, bounded
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = r1 - r0; }
}
hipError_t gs_launch_clock_probe(unsigned long long *out, hipStream_t s) {
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, s, out);
    return hipGetLastError();
}
