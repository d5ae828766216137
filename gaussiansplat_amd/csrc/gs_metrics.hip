// gs_metrics.hip -- the evaluation metrics of gs_image_metrics: per call the four double sums
//     sum w (x - y)^2,  sum w |x - y|,  sum w S,  sum w          (over the C H W pixel-channels; S the standard SSIM map, w = 1 without a weight)
// and, on request, the map itself as float32.  The statements are gs_metrics.h's, all in double.
//
// One workgroup of 256 threads owns a tile of 64 x 16 outputs of one channel:
//   1. the halo of both images (26 rows x 74 columns, zero outside the image) goes to LDS as float32, every load in flight before the first
//      LDS store (halo_fetch / halo_store of gs_halo_tile.h, the loss kernels' own);
//   2. COLUMN pass: a thread takes one halo column and four output rows, widens its 14 sample pairs, forms the three products (exact in double)
//      and keeps the five 11-tap sums of each row in registers; once every thread has read its samples they go to LDS as double [5][16][74],
//      over the samples (47 KB per workgroup: three per CU).  Columns first because the tile is wide: the pass runs over 74 / 64 of the tile's
//      outputs, rows first would run over 26 / 16 of them;
//   3. ROW pass: a thread takes four consecutive outputs of a row, reads 14 doubles per plane and finishes the five sums (22 taps per plane and
//      output in all, not 121), evaluates S, and adds its terms of the four sums.
// The sums use no atomics: a workgroup leaves its four partials in the row of its TILE in a scratch buffer (every row is written by every
// call: nothing to clear, nothing left from an earlier call), and a one-workgroup kernel adds the rows in a fixed order.  The result is bitwise
// reproducible call to call and independent of what the context did before.
#include "gs_metrics.h"
#include "gs_halo_tile.h"         // the 64 x 16 tile with its halo, the tile of a workgroup, the grid; gs_wave.h (gs_block_sum)

#include <stdint.h>

#define MP GS_METRIC_PAD
#define MW GS_METRIC_WIN
#define MNP GS_METRIC_PLANES
#define MNT 256                   // threads
#define MRG 4                     // output rows per thread of the column pass
static_assert(GS_HALO_PAD == GS_METRIC_PAD, "the tile's halo is the window's reach");

struct GsMetricArgs {
    int W, H, C;
    const float *img, *gt, *weight;      // weight: [H, W] or null
    float *map;                          // [C, H, W] or null
    double *partials;                    // [tiles][GS_METRIC_NSUMS]
    double g[MW];
};

// the five 11-tap column sums of NR consecutive output rows r0 .. of halo column hx: output row r0 + o takes the halo rows r0 + o .. + 10, taps in
// ascending order; the NR + 10 sample pairs are widened and multiplied once
template <int NR>
__device__ __forceinline__ void metric_column_sums(double (&acc)[NR][MNP], const float (*sx)[GS_HALO_PITCH], const float (*sy)[GS_HALO_PITCH], const double (&g)[MW], int r0, int hx) {
#pragma unroll
    for (int o = 0; o < NR; ++o)
#pragma unroll
        for (int q = 0; q < MNP; ++q) acc[o][q] = 0.0;
#pragma unroll
    for (int j = 0; j < NR + MW - 1; ++j) {
        double p[MNP];
        gs_metric_planes(sx[r0 + j][hx], sy[r0 + j][hx], p);
#pragma unroll
        for (int o = 0; o < NR; ++o) {
            const int t = j - o;
            if (t >= 0 && t < MW) {
#pragma unroll
                for (int q = 0; q < MNP; ++q) acc[o][q] = fma(g[t], p[q], acc[o][q]);
            }
        }
    }
}
template <int NR>
__device__ __forceinline__ void metric_column_store(double (*sv)[GS_HALO_TY][GS_HALO_HX], const double (&acc)[NR][MNP], int r0, int hx) {
#pragma unroll
    for (int o = 0; o < NR; ++o)
#pragma unroll
        for (int q = 0; q < MNP; ++q) sv[q][r0 + o][hx] = acc[o][q];
}

// The column pass over the 74 halo columns of 16 output rows, dealt so that no wave carries twice another's work: every thread takes MRG = 4
// rows of one of the first 64 columns (wave w: rows 4 w ..), then the threads below MEDGE take ONE row of one of the last 10 columns
#define MEDGE ((GS_HALO_HX - GS_HALO_TX) * GS_HALO_TY)        // 160
static_assert(GS_HALO_TX * (GS_HALO_TY / MRG) == MNT && MEDGE <= MNT, "the column pass is written for one wide unit per thread and at most one edge unit");
static_assert(2 * GS_HALO_HY * GS_HALO_PITCH * sizeof(float) <= MNP * GS_HALO_TY * GS_HALO_HX * sizeof(double), "the samples fit where the column sums go");

__global__ __launch_bounds__(MNT, 3) void metrics_tile_kernel(GsMetricArgs a) {
    // the column sums (double [5][16][74], 47 KB) take the place of the samples (float 2 x [26][76]) once every thread has read its samples:
    // three workgroups per CU instead of two
    __shared__ __attribute__((aligned(16))) char smem[MNP * GS_HALO_TY * GS_HALO_HX * sizeof(double)];
    __shared__ double red[GS_METRIC_NSUMS][4];
    float (*sx)[GS_HALO_PITCH] = reinterpret_cast<float (*)[GS_HALO_PITCH]>(smem), (*sy)[GS_HALO_PITCH] = sx + GS_HALO_HY;
    double (*sv)[GS_HALO_TY][GS_HALO_HX] = reinterpret_cast<double (*)[GS_HALO_TY][GS_HALO_HX]>(smem);
    GsHaloTile tile;
    if (!gs_halo_tile(a, tile)) return;                           // (the whole workgroup)
    const int x0 = tile.x0, y0 = tile.y0, c = tile.c, id = tile.id;           // id: the tile's row of the partials
    const size_t cb = (size_t)c * ((size_t)a.W * a.H);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int py = y0 + ty;
    float wq[4];                                                              // the outputs' weights: fetched with the halos, used last
#pragma unroll
    for (int o = 0; o < 4; ++o)
        wq[o] = a.weight ? a.weight[(uint32_t)(min(py, a.H - 1) * a.W + min(x0 + 4 * tx + o, a.W - 1))] : 1.0f;
    {
        float hx_[HaloIt<MNT>::n], hy_[HaloIt<MNT>::n];
        halo_fetch<MNT>(hx_, a.img + cb, a.W, a.H, x0, y0);
        halo_fetch<MNT>(hy_, a.gt + cb, a.W, a.H, x0, y0);
        halo_store<MNT>(sx, hx_); halo_store<MNT>(sy, hy_);
    }
    double g[MW];
#pragma unroll
    for (int i = 0; i < MW; ++i) g[i] = a.g[i <= MP ? i : MW - 1 - i];         // g[i] == g[10 - i] bit for bit: six values in registers, not eleven
    __syncthreads();
    // ---- column pass, results in registers; the outputs' own samples are read before the column sums overwrite them
    const int cr0 = MRG * ((int)threadIdx.x >> 6), chx = (int)threadIdx.x & 63;
    const bool edge = (int)threadIdx.x < MEDGE;
    const int er0 = (int)threadIdx.x / (GS_HALO_HX - GS_HALO_TX), ehx = GS_HALO_TX + (int)threadIdx.x - er0 * (GS_HALO_HX - GS_HALO_TX);
    double acc0[MRG][MNP], acc1[1][MNP];
    metric_column_sums<MRG>(acc0, sx, sy, g, cr0, chx);
    if (edge) metric_column_sums<1>(acc1, sx, sy, g, er0, ehx);
    double dq[4];                                                             // x - y, exact in double
#pragma unroll
    for (int o = 0; o < 4; ++o) dq[o] = (double)sx[ty + MP][4 * tx + o + MP] - (double)sy[ty + MP][4 * tx + o + MP];
    __syncthreads();
    metric_column_store<MRG>(sv, acc0, cr0, chx);
    if (edge) metric_column_store<1>(sv, acc1, er0, ehx);
    __syncthreads();
    // ---- row pass: four consecutive outputs of row ty
    double m[4][MNP];
#pragma unroll
    for (int q = 0; q < MNP; ++q) {
        double v[4 + MW - 1];
#pragma unroll
        for (int i = 0; i < 4 + MW - 1; ++i) v[i] = sv[q][ty][4 * tx + i];
#pragma unroll
        for (int o = 0; o < 4; ++o) m[o][q] = gs_metric_taps(g, v + o, 1);
    }
    double s_se = 0.0, s_ae = 0.0, s_ss = 0.0, s_w = 0.0;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int px = x0 + 4 * tx + o;
        if (px < a.W && py < a.H) {
            const double d = dq[o];
            const double S = gs_ssim_pixel(m[o]);
            const double w = (double)wq[o];
            s_se += w * (d * d); s_ae += w * fabs(d); s_ss += w * S; s_w += w;
            if (a.map) a.map[cb + (size_t)py * a.W + px] = (float)S;        // one rounding from the double value
        }
    }
    const double t0 = gs_block_sum(s_se, red[0], 4);
    const double t1 = gs_block_sum(s_ae, red[1], 4);
    const double t2 = gs_block_sum(s_ss, red[2], 4);
    const double t3 = gs_block_sum(s_w, red[3], 4);
    if (threadIdx.x == 0) {
        double *row = a.partials + (size_t)id * GS_METRIC_NSUMS;
        row[0] = t0; row[1] = t1; row[2] = t2; row[3] = t3;
    }
}

// one workgroup: thread t adds the rows t, t + 256, ... in ascending order (four rows' loads in flight at a time; a row past the end counts as
// four +0), then gs_block_sum (gs_wave.h)
__global__ __launch_bounds__(MNT) void metrics_finish_kernel(const double *__restrict__ partials, int tiles, double *__restrict__ sums) {
    __shared__ double red[GS_METRIC_NSUMS][4];
    static_assert(GS_METRIC_NSUMS == 4, "a row is two double2");
    const double2 *rows = reinterpret_cast<const double2 *>(partials);
    double s[GS_METRIC_NSUMS] = {0.0, 0.0, 0.0, 0.0};
    for (int i = (int)threadIdx.x; i < tiles; i += 4 * MNT) {
        double2 r[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = i + u * MNT, jc = min(j, tiles - 1);
            r[u][0] = rows[2 * (size_t)jc]; r[u][1] = rows[2 * (size_t)jc + 1];
            if (j >= tiles) r[u][0] = r[u][1] = make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { s[0] += r[u][0].x; s[1] += r[u][0].y; s[2] += r[u][1].x; s[3] += r[u][1].y; }
    }
#pragma unroll
    for (int k = 0; k < GS_METRIC_NSUMS; ++k) {
        const double t = gs_block_sum(s[k], red[k], 4);
        if (threadIdx.x == 0) sums[k] = t;
    }
}

int gs_metric_tiles(int W, int H, int C) { return gs_halo_grid(W, H, C).tiles; }

hipError_t gs_launch_metrics(const float *img, const float *gt, const float *weight, int W, int H, int C, float *ssim_map, double *partials,
                             double *sums, hipStream_t s) {
    GsMetricArgs a{};
    a.W = W; a.H = H; a.C = C; a.img = img; a.gt = gt; a.weight = weight; a.map = ssim_map; a.partials = partials;
    gs_metric_window(a.g);
    const GsHaloGrid grid = gs_halo_grid(W, H, C);
    hipLaunchKernelGGL(metrics_tile_kernel, dim3(grid.blocks), dim3(MNT), 0, s, a);
    hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(MNT), 0, s, partials, grid.tiles, sums);
    return hipGetLastError();
}
