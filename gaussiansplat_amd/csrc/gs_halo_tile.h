// gs_halo_tile.h -- the image tile of the stencil kernels (the loss, gs_loss.hip; the metrics, gs_metrics.hip), written ONCE: 64 x 16 outputs of
// one channel per workgroup with the 5 pixels around them that an 11 x 11 window reaches, staged into LDS; which tile a workgroup owns; and
// how many workgroups a launch needs.  Device code only (it stands on gs_wave.h).  Functions, not text: they cost nothing.
#pragma once
#include "gs_wave.h"              // gs_xcd_tile

constexpr int GS_HALO_TX = 64, GS_HALO_TY = 16;       // outputs of a tile
constexpr int GS_HALO_PAD = 5;                        // (window - 1) / 2
constexpr int GS_HALO_HX = GS_HALO_TX + 2 * GS_HALO_PAD, GS_HALO_HY = GS_HALO_TY + 2 * GS_HALO_PAD;   // 74 halo columns, 26 halo rows
constexpr int GS_HALO_PITCH = 76;                     // floats per LDS row (16-byte aligned rows for ds_read_b128)

// halo tile of one plane: rows y0-5 .. y0+20, columns x0-5 .. x0+68, zero outside the image (loss.jl:29 pads with zeros).
// Two steps, so that a kernel can put the fetches of ALL its planes in flight before the first LDS store waits for one of them:
// as one loop (load, wait, store per element) the 8 elements per thread and plane were 16 .. 24 global-load latencies in a row
// (round 4: ssim_stats 172 -> 145 us, ssim_grad 92 -> 68 us at 1920x1080x3).  The address is clamped instead of predicated
// (every load is unconditional, the select happens on the value).  NT: the threads of the workgroup.
template <int NT> struct HaloIt { static constexpr int n = (GS_HALO_HY * GS_HALO_PITCH + NT - 1) / NT; };     // halo elements per thread and plane
template <int NT>
__device__ __forceinline__ void halo_fetch(float (&v)[HaloIt<NT>::n], const float *__restrict__ plane, int W, int H, int x0, int y0) {
    int hy = (int)threadIdx.x / GS_HALO_PITCH, hx = (int)threadIdx.x - hy * GS_HALO_PITCH;   // element i = thread + NT k: one division, then steps
#pragma unroll
    for (int k = 0; k < HaloIt<NT>::n; ++k) {
        const int gx = x0 + hx - GS_HALO_PAD, gy = y0 + hy - GS_HALO_PAD;
        const bool in = hx < GS_HALO_HX && gx >= 0 && gx < W && gy >= 0 && gy < H;   // (hy >= GS_HALO_HY: gy may still be inside; never stored)
        const float t = plane[(uint32_t)(min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1))];   // uniform base + 32-bit lane offset
        v[k] = in ? t : 0.0f;
        hx += NT % GS_HALO_PITCH; hy += NT / GS_HALO_PITCH;
        if (hx >= GS_HALO_PITCH) { hx -= GS_HALO_PITCH; hy += 1; }
    }
}
template <int NT>
__device__ __forceinline__ void halo_store(float (*dst)[GS_HALO_PITCH], const float (&v)[HaloIt<NT>::n]) {
    float *d = &dst[0][0];
#pragma unroll
    for (int k = 0; k < HaloIt<NT>::n; ++k) {
        const int i = (int)threadIdx.x + NT * k;
        if (i < GS_HALO_HY * GS_HALO_PITCH) d[i] = v[k];
    }
}

// The tile of a workgroup: gs_xcd_tile's order (gs_wave.h), so that the tiles in flight on an XCD are neighbours that share their halos in its
// L2.  id = (channel, tile row, tile column) in row-major order; x0, y0: the tile's first output.  false: the whole workgroup has no tile.
// a: the kernel's argument struct, for its members W, H, C -- by reference, as gs_g2d_load takes its: handed the three ints, metrics_tile_kernel
// reordered around its argument loads (1712 -> 1711 instructions).
struct GsHaloTile { int x0, y0, c, id; };
template <class A>
__device__ __forceinline__ bool gs_halo_tile(const A &a, GsHaloTile &t) {
    const int gx = (a.W + GS_HALO_TX - 1) / GS_HALO_TX, gy = (a.H + GS_HALO_TY - 1) / GS_HALO_TY, T = gx * gy * a.C;
    if (!gs_xcd_tile(blockIdx.x, T, t.id)) return false;
    t.c = t.id / (gx * gy);
    const int r = t.id - t.c * (gx * gy);
    t.y0 = (r / gx) * GS_HALO_TY; t.x0 = (r % gx) * GS_HALO_TX;
    return true;
}
// host: the tiles of a C x H x W image and the workgroups of a launch over them (gs_xcd_tile: an eighth of the tiles per XCD, rounded up)
struct GsHaloGrid { int tiles, blocks; };
inline GsHaloGrid gs_halo_grid(int W, int H, int C) {
    const int tiles = ((W + GS_HALO_TX - 1) / GS_HALO_TX) * ((H + GS_HALO_TY - 1) / GS_HALO_TY) * C;
    return {tiles, 8 * ((tiles + 7) / 8)};
}
