// gs_bilagrid.hip -- the per-view bilateral grid between the frame and the loss (include/gsplat.h: gs_bilagrid_apply, gs_bilagrid_backward,
// gs_bilagrid_tv, gs_bilagrid_adam).  The statements are gs_bilagrid.h's.  Six kernels, no atomics, no counters, no scratch buffer, no hand-off
// between workgroups inside a launch; every grid is a function of (W, H, Gx, Gy, Gz) alone -- every result is bitwise reproducible and
// independent of what the ctx did before.
//   bilagrid_pixel_kernel    BWD false, apply: streaming.  A workgroup covers a run of GS_BILAGRID_BLOCK * 4 pixels of ONE image row; lane q of the run takes the
//                            pixels 4 q .. 4 q + 3: one 16-byte access per plane (VEC: W % 4 == 0 and every base 16-byte aligned, so that every
//                            row of every plane keeps the alignment), else four 4-byte ones, which also cover the row's tail.  The pixel ->
//                            lane mapping does not depend on VEC.  A row has ONE y cell: the workgroup touches two y planes of the grid,
//                            2 Gz Gx 48 bytes (12 KiB at 16 x 16 x 8).  STAGE: the workgroup copies those two planes into LDS first (4-byte
//                            loads: the grid's base may sit anywhere) and gathers the eight rows of a pixel from LDS as 16-byte reads; taken
//                            where the two planes fit in GS_BILAGRID_STAGE_BYTES.  Larger grids (a 64 x 64 pair of planes is 384 KiB) gather
//                            from global memory.  The slice runs four floats of the row at a time, so that 32 gathered floats are live.
//   ... BWD true             the same mapping and staging: x, d and the weight in, d_img out.  A lane reads its own pixels of d before it writes
//                            them, so d_img == d_out is legal (neither is __restrict__).
//   bilagrid_dgrid_kernel    the adjoint into the grid, a GATHER: one workgroup per vertex.  The pixels whose x cell and y cell have the vertex
//                            as a corner form a rectangle of columns and rows -- found with the cell statement itself by two bisections per
//                            axis (the cell index is monotone in the column), so the rectangle is exact whatever float32 does to c * sx.  The
//                            workgroup's lanes walk the rectangle in row-major order, lane t the pixels t, t + 256, ...; a pixel whose z cell
//                            does not have the vertex is dropped after its three colour loads.  A lane keeps 12 double accumulators and adds
//                            the terms of its pixels in ascending order, corner by corner; gs_block_tree_row (gs_wave.h) adds the lanes and
//                            thread m < 12 rounds to float once and stores float m of the vertex.  Every vertex is written by every call (no
//                            pixel: + 0).  The kernel reads img, d_out and the weight with 4-byte loads only: alignment changes nothing.
//   bilagrid_tv_kernel       one workgroup over the Gz Gy Gx 12 floats: three double sums of squared forward differences per lane, the same tree.
//   bilagrid_tv_grad_kernel  one thread per float: gs_bilagrid_tv_grad into d_grid.
//   bilagrid_adam_kernel     one thread per float: gs_adam_update (gs_adam.h) with the scalars of one step.
// Built with -ffp-contract=off (gaussiansplat_amd/build.py); the statements turn contraction off themselves.
#include "gs_bilagrid.h"
#include "gs_wave.h"

#include <cstdint>
#include <initializer_list>
#include <type_traits>

#pragma clang fp contract(off)

namespace {

extern __shared__ __align__(16) float bila_lds[];          // STAGE: [2][Gz][Gx][12], the y planes y0 and y1 of the workgroup's image row

struct BilaArgs {
    const float *img, *d_out, *grid, *weight;
    float *out;                                            // apply: out; backward: d_img
    int W, H, Gx, Gy, Gz, bpr;                             // bpr: workgroups per image row
    float sx, sy;
};

struct Px4 { float v[GS_BILAGRID_QUAD]; };

// the lane's pixels p0 .. p0 + n - 1 of one plane (n == 4 under VEC); the rest + 0
template <bool VEC>
__device__ __forceinline__ Px4 load4(const float *plane, int p0, int n) {
    Px4 r;
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4 *>(plane + p0);
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < GS_BILAGRID_QUAD; ++j) r.v[j] = j < n ? plane[p0 + j] : 0.0f;
    }
    return r;
}
template <bool VEC>
__device__ __forceinline__ void store4(float *plane, int p0, int n, const Px4 &r) {
    if (VEC) {
        *reinterpret_cast<float4 *>(plane + p0) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < GS_BILAGRID_QUAD; ++j)
            if (j < n) plane[p0 + j] = r.v[j];
    }
}

// the two y planes of image row `row` into LDS; every thread of the workgroup calls it
__device__ __forceinline__ void stage_planes(const BilaArgs &a, int row) {
    const GsBilaAxis ya = gs_bilagrid_cell((float)row * a.sy, a.Gy);
    const int rowf = a.Gx * GS_BILAGRID_FLOATS, plane = a.Gz * rowf;
    for (int i = threadIdx.x; i < 2 * plane; i += GS_BILAGRID_BLOCK) {
        const int yy = i >= plane, rem = i - yy * plane, z = rem / rowf, j = rem - z * rowf;
        bila_lds[i] = a.grid[(z * a.Gy + (yy ? ya.i1 : ya.i0)) * rowf + j];
    }
    __syncthreads();
}

// the slice of a pixel, four floats of the row at a time
template <bool STAGE>
__device__ __forceinline__ void slice_pixel(const BilaArgs &a, const GsBilaCell &c, float (&A)[GS_BILAGRID_FLOATS], float (&S)[GS_BILAGRID_FLOATS]) {
    int off[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (STAGE) off[k] = ((((k >> 1) & 1) * a.Gz + (k & 4 ? c.z.i1 : c.z.i0)) * a.Gx + (k & 1 ? c.x.i1 : c.x.i0)) * GS_BILAGRID_FLOATS;
        else off[k] = gs_bilagrid_vertex(c, k, a.Gx, a.Gy) * GS_BILAGRID_FLOATS;
    }
#pragma unroll
    for (int q = 0; q < GS_BILAGRID_FLOATS / 4; ++q) {
        float g[4][8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (STAGE) {
                const float4 r = *reinterpret_cast<const float4 *>(bila_lds + off[k] + 4 * q);
                g[0][k] = r.x; g[1][k] = r.y; g[2][k] = r.z; g[3][k] = r.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j][k] = a.grid[off[k] + 4 * q + j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) gs_bilagrid_slice1(c, g[j], A[4 * q + j], S[4 * q + j]);
    }
}

template <bool VEC, bool HAS_W, bool STAGE, bool BWD>
__global__ __launch_bounds__(GS_BILAGRID_BLOCK) void bilagrid_pixel_kernel(BilaArgs a) {
    const int row = blockIdx.x / a.bpr;
    const int col = ((blockIdx.x - row * a.bpr) * GS_BILAGRID_BLOCK + threadIdx.x) * GS_BILAGRID_QUAD;
    if (STAGE) stage_planes(a, row);
    if (col >= a.W) return;
    const int n = min(GS_BILAGRID_QUAD, a.W - col), px = a.W * a.H, p0 = row * a.W + col;      // < 2^31 / 3
    const Px4 x0 = load4<VEC>(a.img, p0, n), x1 = load4<VEC>(a.img + px, p0, n), x2 = load4<VEC>(a.img + 2 * (size_t)px, p0, n);
    Px4 d0{}, d1{}, d2{}, w{};
    if (BWD) { d0 = load4<VEC>(a.d_out, p0, n); d1 = load4<VEC>(a.d_out + px, p0, n); d2 = load4<VEC>(a.d_out + 2 * (size_t)px, p0, n); }
    if (HAS_W) w = load4<VEC>(a.weight, p0, n);
    Px4 o[3] = {};
#pragma unroll
    for (int j = 0; j < GS_BILAGRID_QUAD; ++j) {
        if (j < n) {
            const float x[3] = {x0.v[j], x1.v[j], x2.v[j]};
            const float l = gs_bilagrid_luminance(x);
            const GsBilaCell c = gs_bilagrid_pixel_cell(col + j, row, l, a.sx, a.sy, a.Gx, a.Gy, a.Gz);
            float A[GS_BILAGRID_FLOATS], S[GS_BILAGRID_FLOATS], r[3];
            slice_pixel<STAGE>(a, c, A, S);
            if (BWD) {
                const float d[3] = {d0.v[j], d1.v[j], d2.v[j]};
                float g[3] = {d[0], d[1], d[2]};
                if (HAS_W) gs_bilagrid_weigh(d, w.v[j], g);
                gs_bilagrid_dx(A, S, g, x, l, a.Gz, r);
            } else {
                gs_bilagrid_affine(A, x, r);
                if (HAS_W) { r[0] = w.v[j] * r[0]; r[1] = w.v[j] * r[1]; r[2] = w.v[j] * r[2]; }
            }
            o[0].v[j] = r[0]; o[1].v[j] = r[1]; o[2].v[j] = r[2];
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) store4<VEC>(a.out + r * (size_t)px, p0, n, o[r]);
}

// the first coordinate in 0 .. extent whose cell index is at least `target` (extent: none)
__device__ __forceinline__ int first_at_least(int target, int extent, float s, int n) {
    int lo = 0, hi = extent;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (gs_bilagrid_cell((float)mid * s, n).i0 >= target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

template <bool HAS_W>
__global__ __launch_bounds__(GS_BILAGRID_BLOCK) void bilagrid_dgrid_kernel(BilaArgs a, float *__restrict__ d_grid) {
    const int v = blockIdx.x, vx = v % a.Gx, vy = (v / a.Gx) % a.Gy, vz = v / (a.Gx * a.Gy);
    // the columns whose x cell starts at vx - 1 or vx, the rows likewise (an axis of one vertex: all of them)
    const int c_lo = first_at_least(vx - 1, a.W, a.sx, a.Gx), c_hi = first_at_least(vx + 1, a.W, a.sx, a.Gx);
    const int r_lo = first_at_least(vy - 1, a.H, a.sy, a.Gy), r_hi = first_at_least(vy + 1, a.H, a.sy, a.Gy);
    const int nc = c_hi - c_lo, nfoot = nc * (r_hi - r_lo), px = a.W * a.H;
    double acc[GS_BILAGRID_FLOATS];
#pragma unroll
    for (int i = 0; i < GS_BILAGRID_FLOATS; ++i) acc[i] = 0.0;
    for (int t = threadIdx.x; t < nfoot; t += GS_BILAGRID_BLOCK) {
        const int rr = t / nc, col = c_lo + (t - rr * nc), row = r_lo + rr, p = row * a.W + col;
        const float x[3] = {a.img[p], a.img[px + p], a.img[2 * (size_t)px + p]};
        const GsBilaCell c = gs_bilagrid_pixel_cell(col, row, gs_bilagrid_luminance(x), a.sx, a.sy, a.Gx, a.Gy, a.Gz);
        if (c.z.i0 != vz && c.z.i1 != vz) continue;
        const float d[3] = {a.d_out[p], a.d_out[px + p], a.d_out[2 * (size_t)px + p]};
        float g[3] = {d[0], d[1], d[2]};
        if (HAS_W) gs_bilagrid_weigh(d, a.weight[p], g);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (gs_bilagrid_vertex(c, k, a.Gx, a.Gy) == v) gs_bilagrid_dG_add(gs_bilagrid_weight(c, k), g, x, acc);
    }
    gs_block_tree_row<GS_BILAGRID_FLOATS, GS_BILAGRID_BLOCK / 64>([&](int m) { return acc[m]; },
                                                                  [&](int m, double s) { d_grid[(size_t)v * GS_BILAGRID_FLOATS + m] = (float)s; });
}

__global__ __launch_bounds__(GS_BILAGRID_BLOCK) void bilagrid_tv_kernel(const float *__restrict__ G, int Gx, int Gy, int Gz, double *__restrict__ tv_out) {
    __shared__ double sums[3];
    const int rowf = Gx * GS_BILAGRID_FLOATS, plane = Gy * rowf, total = Gz * plane;
    double s[3] = {0.0, 0.0, 0.0};
    for (int e = threadIdx.x; e < total; e += GS_BILAGRID_BLOCK) {
        const int z = e / plane, rem = e - z * plane, y = rem / rowf, x = (rem - y * rowf) / GS_BILAGRID_FLOATS;
        gs_bilagrid_tv_add([&](int dz, int dy, int dx) { return G[e + dz * plane + dy * rowf + dx * GS_BILAGRID_FLOATS]; }, x, y, z, Gx, Gy, Gz, s);
    }
    gs_block_tree_row<3, GS_BILAGRID_BLOCK / 64>([&](int c) { return s[c]; }, [&](int c, double t) { sums[c] = t; });
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t[3] = {sums[0], sums[1], sums[2]};
        *tv_out = gs_bilagrid_tv_value(t, Gx, Gy, Gz);
    }
}

__global__ __launch_bounds__(GS_BILAGRID_BLOCK) void bilagrid_tv_grad_kernel(const float *__restrict__ G, int Gx, int Gy, int Gz, float s_x, float s_y, float s_z,
                                                                             float *__restrict__ d_grid) {
    const int rowf = Gx * GS_BILAGRID_FLOATS, plane = Gy * rowf, total = Gz * plane;
    const int e = blockIdx.x * GS_BILAGRID_BLOCK + threadIdx.x;
    if (e >= total) return;
    const int z = e / plane, rem = e - z * plane, y = rem / rowf, x = (rem - y * rowf) / GS_BILAGRID_FLOATS;
    d_grid[e] = gs_bilagrid_tv_grad(d_grid[e], [&](int dz, int dy, int dx) { return G[e + dz * plane + dy * rowf + dx * GS_BILAGRID_FLOATS]; },
                                    x, y, z, Gx, Gy, Gz, s_x, s_y, s_z);
}

__global__ __launch_bounds__(GS_BILAGRID_BLOCK) void bilagrid_adam_kernel(float *__restrict__ G, const float *__restrict__ dG, float *__restrict__ m_,
                                                                          float *__restrict__ v_, long long n, GsAdamHyper h) {
    const long long i = (long long)blockIdx.x * GS_BILAGRID_BLOCK + threadIdx.x;
    if (i >= n) return;
    float p = G[i], m = m_[i], v = v_[i];
    gs_adam_update(p, m, v, dG[i], h, h.step_size[0]);
    G[i] = p; m_[i] = m; v_[i] = v;
}

bool aligned16(std::initializer_list<const void *> ps) {
    uintptr_t bits = 0;
    for (const void *p : ps) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & 15) == 0;
}

BilaArgs make_args(const float *img, const float *d_out, const float *grid, int Gx, int Gy, int Gz, const float *weight, int W, int H, float *out) {
    const int quads = (W + GS_BILAGRID_QUAD - 1) / GS_BILAGRID_QUAD;
    return BilaArgs{img, d_out, grid, weight, out, W, H, Gx, Gy, Gz, (quads + GS_BILAGRID_BLOCK - 1) / GS_BILAGRID_BLOCK,
                    gs_bilagrid_scale(Gx, W), gs_bilagrid_scale(Gy, H)};
}

// the streaming pass of apply (BWD false) or of the backward into the image
template <bool BWD>
hipError_t launch_pixels(const BilaArgs &a, hipStream_t s) {
    const bool vec = a.W % GS_BILAGRID_QUAD == 0 && aligned16({a.img, a.d_out, a.weight, a.out});
    const size_t lds = 2 * sizeof(float) * GS_BILAGRID_FLOATS * (size_t)a.Gx * a.Gz;
    const bool stage = lds <= GS_BILAGRID_STAGE_BYTES;
    const dim3 grid((unsigned)((long long)a.bpr * a.H));                              // <= W H / 4 + H < 2^31
    auto launch = [&](auto V, auto HW, auto ST) {
        constexpr bool st = decltype(ST)::value;
        hipLaunchKernelGGL((bilagrid_pixel_kernel<decltype(V)::value, decltype(HW)::value, st, BWD>), grid, dim3(GS_BILAGRID_BLOCK), st ? lds : 0, s, a);
    };
    using T = std::true_type; using F = std::false_type;
    auto pick_stage = [&](auto V, auto HW) { if (stage) launch(V, HW, T{}); else launch(V, HW, F{}); };
    if (vec) { if (a.weight) pick_stage(T{}, T{}); else pick_stage(T{}, F{}); }
    else     { if (a.weight) pick_stage(F{}, T{}); else pick_stage(F{}, F{}); }
    return hipGetLastError();
}

}  // namespace

hipError_t gs_launch_bilagrid_apply(const float *img, const float *grid, int Gx, int Gy, int Gz, const float *weight, int W, int H, float *out, hipStream_t s) {
    return launch_pixels<false>(make_args(img, nullptr, grid, Gx, Gy, Gz, weight, W, H, out), s);
}

hipError_t gs_launch_bilagrid_backward(const float *img, const float *d_out, const float *grid, int Gx, int Gy, int Gz, const float *weight, int W, int H,
                                       float *d_img, float *d_grid, hipStream_t s) {
    const BilaArgs a = make_args(img, d_out, grid, Gx, Gy, Gz, weight, W, H, d_img);
    if (d_grid) {                                          // first: it reads d_out, which the image pass may overwrite
        const dim3 grid_v((unsigned)(Gx * Gy * Gz));
        if (weight) hipLaunchKernelGGL(bilagrid_dgrid_kernel<true>, grid_v, dim3(GS_BILAGRID_BLOCK), 0, s, a, d_grid);
        else        hipLaunchKernelGGL(bilagrid_dgrid_kernel<false>, grid_v, dim3(GS_BILAGRID_BLOCK), 0, s, a, d_grid);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_pixels<true>(a, s);
}

hipError_t gs_launch_bilagrid_tv(const float *grid, int Gx, int Gy, int Gz, float coef, float *d_grid, double *tv_out, hipStream_t s) {
    if (d_grid) {
        const int total = Gx * Gy * Gz * GS_BILAGRID_FLOATS;
        const float s_x = gs_bilagrid_tv_scale(coef, gs_bilagrid_tv_count(Gx, Gy * Gz)), s_y = gs_bilagrid_tv_scale(coef, gs_bilagrid_tv_count(Gy, Gx * Gz)),
                    s_z = gs_bilagrid_tv_scale(coef, gs_bilagrid_tv_count(Gz, Gx * Gy));
        hipLaunchKernelGGL(bilagrid_tv_grad_kernel, dim3((unsigned)((total + GS_BILAGRID_BLOCK - 1) / GS_BILAGRID_BLOCK)), dim3(GS_BILAGRID_BLOCK), 0, s,
                           grid, Gx, Gy, Gz, s_x, s_y, s_z, d_grid);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (tv_out) hipLaunchKernelGGL(bilagrid_tv_kernel, dim3(1), dim3(GS_BILAGRID_BLOCK), 0, s, grid, Gx, Gy, Gz, tv_out);
    return hipGetLastError();
}

hipError_t gs_launch_bilagrid_adam(float *grid, const float *d_grid, float *m, float *v, long long n, const GsAdamHyper &h, hipStream_t s) {
    hipLaunchKernelGGL(bilagrid_adam_kernel, dim3((unsigned)((n + GS_BILAGRID_BLOCK - 1) / GS_BILAGRID_BLOCK)), dim3(GS_BILAGRID_BLOCK), 0, s, grid, d_grid, m, v, n, h);
    return hipGetLastError();
}
