// gs_bilagrid.h -- the statements of the per-view bilateral grid (gs_bilagrid_apply / gs_bilagrid_backward / gs_bilagrid_tv: a lattice of
// 3 x 4 colour affines indexed by pixel position and pixel luminance, sliced per pixel and applied to the colour, between the frame and the
// loss), written ONCE and usable from host and device: the kernels of gs_bilagrid.hip execute them per pixel, tests/bilagrid_host.cpp is a
// host build of the same text that tests/test_bilagrid_host.py compares bit for bit with the NumPy restatement of tests/bilagrid_ref.py.
//
// Layout: images are planar [3][H][W] float32; the weight is [H][W] or absent; the grid G is [Gz][Gy][Gx][12] float32, vertex-major, the 12
// floats of a vertex A[r][k] row-major 3 x 4 as a row of the exposure table is; 1 <= Gx, Gy, Gz <= GS_BILAGRID_MAX_DIM.  Contraction is off in
// every body: one fp32 rounding per operation, in the order written.
//   cell      of a coordinate g on an axis of n vertices: g = g < n - 1 ? g : n - 1;  i0 = min((int)g, max(n - 2, 0));  i1 = min(i0 + 1, n - 1);
//             f = g - (float)i0
//   pixel     (column c, row r):  gx = (float)c * sx,  sx = (float)((double)(Gx - 1) / (double)(W - 1)), 0 when W == 1;  gy likewise;
//             l = (0.299f x0 + 0.587f x1) + 0.114f x2;   lc = l > 0 ? l : 0;  lc = lc < 1 ? lc : 1  (a NaN l and -0 give +0);
//             gz = lc * (float)(Gz - 1)
//   slice     per float m of the row, three nested interpolations, x innermost:
//                 e[z][y] = G[z][y][x0] + fx * (G[z][y][x1] - G[z][y][x0]);   h[z] = e[z][y0] + fy * (e[z][y1] - e[z][y0]);
//                 S = h[z1] - h[z0];   A = h[z0] + fz * S
//             Equal corners give that value itself (the differences are + 0): the identity grid slices to [I | 0] EXACTLY at every pixel.  (The
//             sum of the eight weighted corners does not: in float32 the eight weights add up to something else than 1, between 1 - 2^-22
//             and 1 + 2^-22, at about a quarter of all pixels, and an identity grid would not return the image.)
//   forward   a_r = ((A[r][0] x0 + A[r][1] x1) + A[r][2] x2) + A[r][3];   out_r = w a_r   (no weight: out_r = a_r)
//   into x    g_r = w d_r  (no weight: g_r = d_r);   dA[r][k] = g_r x_k  (x_3 = 1: dA[r][3] = g_r);
//             dl = (float)(Gz - 1) * ((..(dA[0] S[0] + dA[1] S[1]) + ..) + dA[11] S[11])  when 0 < l and l < 1, else + 0  (S is the slice's own: the
//             derivative of A along z);   d_img_k = ((A[0][k] g0 + A[1][k] g1) + A[2][k] g2) + lam_k dl,   lam = (0.299f, 0.587f, 0.114f)
//   into G    corner weights u = (wz wy) wx with w?0 = 1 - f?, w?1 = f?, corners in the order z0y0x0, z0y0x1, z0y1x0, z0y1x1, z1y0x0, ...;
//             the term of corner c into float [r][k] of its vertex is t = (double)u_c * ((double)g_r * (double)x_k): the inner product of
//             two floats is exact in double, the outer one rounds once.  d_grid[v][m] is the sum of the terms of every (pixel, corner)
//             whose vertex is v, in double, rounded to float once (the sum's order is the kernel's: gs_bilagrid.hip); a vertex no pixel
//             touches gets + 0.  On an axis of one vertex both corners are that vertex (weights 1 and 0).
//   TV        per axis a with n_a >= 2: S_a = sum over the vertex pairs along a and the 12 floats of (double)d * (double)d, d = G[+1] - G in
//             float32 (the square of a float is exact in double); count_a = the number of those differences; tv = (S_x / count_x + S_y /
//             count_y) + S_z / count_z in double, absent axes skipped.  Its gradient into float m of vertex v, accumulated into d_grid in
//             float32: acc = d_grid[v][m]; for a in x, y, z with n_a >= 2: (i_a > 0) acc = acc + s_a * (G[v] - G[v - e_a]); (i_a < n_a - 1)
//             acc = acc - s_a * (G[v + e_a] - G[v]);  s_a = (float)(2 coef / count_a), the quotient formed in double.
#pragma once

#include "../../include/gsplat.h"        // GS_BILAGRID_FLOATS, GS_BILAGRID_MAX_DIM

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_BG __host__ __device__ inline
#else
#define GS_BG inline
#endif

#define GS_BILAGRID_QUAD 4                // consecutive pixels of a row a lane takes (one 16-byte access per plane)
#define GS_BILAGRID_BLOCK 256             // lanes of a workgroup
#define GS_BILAGRID_STAGE_BYTES 65536     // two y planes of the grid are staged in LDS where they fit in this (gs_bilagrid.hip)

struct GsBilaAxis { int i0, i1; float f; };
// the cell of coordinate g on an axis of n vertices
GS_BG GsBilaAxis gs_bilagrid_cell(float g, int n) {
#pragma clang fp contract(off)
    const float top = (float)(n - 1);
    g = g < top ? g : top;
    const int lim = n - 2 > 0 ? n - 2 : 0;
    GsBilaAxis a;
    a.i0 = (int)g < lim ? (int)g : lim;
    a.i1 = a.i0 + 1 < n - 1 ? a.i0 + 1 : n - 1;
    a.f = g - (float)a.i0;
    return a;
}
// grid units per pixel step along an axis of n vertices over `extent` pixels
GS_BG float gs_bilagrid_scale(int n, int extent) { return extent > 1 ? (float)((double)(n - 1) / (double)(extent - 1)) : 0.0f; }

GS_BG float gs_bilagrid_luminance(const float (&x)[3]) {
#pragma clang fp contract(off)
    return (0.299f * x[0] + 0.587f * x[1]) + 0.114f * x[2];
}
// the z coordinate of a luminance
GS_BG float gs_bilagrid_gz(float l, int Gz) {
#pragma clang fp contract(off)
    float lc = l > 0.0f ? l : 0.0f;
    lc = lc < 1.0f ? lc : 1.0f;
    return lc * (float)(Gz - 1);
}

// the three cells of a pixel
struct GsBilaCell { GsBilaAxis x, y, z; };
GS_BG GsBilaCell gs_bilagrid_pixel_cell(int col, int row, float l, float sx, float sy, int Gx, int Gy, int Gz) {
#pragma clang fp contract(off)
    GsBilaCell c;
    c.x = gs_bilagrid_cell((float)col * sx, Gx);
    c.y = gs_bilagrid_cell((float)row * sy, Gy);
    c.z = gs_bilagrid_cell(gs_bilagrid_gz(l, Gz), Gz);
    return c;
}
// vertex index (rows of 12 floats) of corner c = 4 z + 2 y + x of a cell
GS_BG int gs_bilagrid_vertex(const GsBilaCell &c, int corner, int Gx, int Gy) {
    const int z = corner & 4 ? c.z.i1 : c.z.i0, y = corner & 2 ? c.y.i1 : c.y.i0, x = corner & 1 ? c.x.i1 : c.x.i0;
    return (z * Gy + y) * Gx + x;
}
// the weight of corner c = 4 z + 2 y + x, and all eight in corner order
GS_BG float gs_bilagrid_weight(const GsBilaCell &c, int corner) {
#pragma clang fp contract(off)
    const float wz = corner & 4 ? c.z.f : 1.0f - c.z.f, wy = corner & 2 ? c.y.f : 1.0f - c.y.f, wx = corner & 1 ? c.x.f : 1.0f - c.x.f;
    return (wz * wy) * wx;
}
GS_BG void gs_bilagrid_weights(const GsBilaCell &c, float (&u)[8]) {
    for (int k = 0; k < 8; ++k) u[k] = gs_bilagrid_weight(c, k);
}

// the slice of one float of the row from its values g at the eight corners: A, and S its derivative along z
GS_BG void gs_bilagrid_slice1(const GsBilaCell &c, const float (&g)[8], float &A, float &S) {
#pragma clang fp contract(off)
    float h[2];
    for (int z = 0; z < 2; ++z) {
        const float e0 = g[4 * z] + c.x.f * (g[4 * z + 1] - g[4 * z]);
        const float e1 = g[4 * z + 2] + c.x.f * (g[4 * z + 3] - g[4 * z + 2]);
        h[z] = e0 + c.y.f * (e1 - e0);
    }
    S = h[1] - h[0];
    A = h[0] + c.z.f * S;
}
// the slice of the whole row: G(corner, m) is float m of the vertex of that corner
template <class Fetch>
GS_BG void gs_bilagrid_slice(const GsBilaCell &c, Fetch G, float (&A)[GS_BILAGRID_FLOATS], float (&S)[GS_BILAGRID_FLOATS]) {
    for (int m = 0; m < GS_BILAGRID_FLOATS; ++m) {
        float g[8];
        for (int k = 0; k < 8; ++k) g[k] = G(k, m);
        gs_bilagrid_slice1(c, g, A[m], S[m]);
    }
}

// the affine of one pixel, before the weight
GS_BG void gs_bilagrid_affine(const float (&A)[GS_BILAGRID_FLOATS], const float (&x)[3], float (&a)[3]) {
#pragma clang fp contract(off)
    for (int r = 0; r < 3; ++r) a[r] = ((A[4 * r] * x[0] + A[4 * r + 1] * x[1]) + A[4 * r + 2] * x[2]) + A[4 * r + 3];
}
// g = w d: what both adjoints start from
GS_BG void gs_bilagrid_weigh(const float (&d)[3], float w, float (&g)[3]) {
#pragma clang fp contract(off)
    for (int r = 0; r < 3; ++r) g[r] = w * d[r];
}
// the adjoint into the image from g = w d (or d), the pixel's x and luminance l, and the slice's A and S
GS_BG void gs_bilagrid_dx(const float (&A)[GS_BILAGRID_FLOATS], const float (&S)[GS_BILAGRID_FLOATS], const float (&g)[3], const float (&x)[3], float l,
                          int Gz, float (&dx)[3]) {
#pragma clang fp contract(off)
    float dl = 0.0f;
    if (0.0f < l && l < 1.0f) {
        float acc = 0.0f;
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 4; ++k) {
                const float dA = k < 3 ? g[r] * x[k] : g[r];
                const float t = dA * S[4 * r + k];
                acc = (r == 0 && k == 0) ? t : acc + t;
            }
        dl = (float)(Gz - 1) * acc;
    }
    const float lam[3] = {0.299f, 0.587f, 0.114f};
    for (int k = 0; k < 3; ++k) dx[k] = ((A[k] * g[0] + A[4 + k] * g[1]) + A[8 + k] * g[2]) + lam[k] * dl;
}
// the twelve terms of one (pixel, corner) into its vertex, added to acc: u (g_r x_k) in double, one double addition each
GS_BG void gs_bilagrid_dG_add(float u, const float (&g)[3], const float (&x)[3], double (&acc)[GS_BILAGRID_FLOATS]) {
#pragma clang fp contract(off)
    const double ud = (double)u;
    for (int r = 0; r < 3; ++r) {
        const double gr = (double)g[r];
        for (int k = 0; k < 3; ++k) acc[4 * r + k] = acc[4 * r + k] + ud * (gr * (double)x[k]);
        acc[4 * r + 3] = acc[4 * r + 3] + ud * gr;
    }
}

// ---- total variation
// the number of differences along the axis of n vertices with `others` vertices across (0: the axis has none)
GS_BG long long gs_bilagrid_tv_count(int n, int others) { return n >= 2 ? (long long)(n - 1) * others * GS_BILAGRID_FLOATS : 0; }
// float32 factor of the gradient along an axis: 2 coef / count, formed in double (0 for an absent axis)
GS_BG float gs_bilagrid_tv_scale(float coef, long long count) { return count > 0 ? (float)(2.0 * (double)coef / (double)count) : 0.0f; }
// the squared forward differences of one float of the grid (of vertex x, y, z), added to the sums of their axes: G(dz, dy, dx) as below
template <class Fetch>
GS_BG void gs_bilagrid_tv_add(Fetch G, int x, int y, int z, int Gx, int Gy, int Gz, double (&s)[3]) {
#pragma clang fp contract(off)
    const float g = G(0, 0, 0);
    if (x < Gx - 1) { const float d = G(0, 0, 1) - g; s[0] = s[0] + (double)d * (double)d; }
    if (y < Gy - 1) { const float d = G(0, 1, 0) - g; s[1] = s[1] + (double)d * (double)d; }
    if (z < Gz - 1) { const float d = G(1, 0, 0) - g; s[2] = s[2] + (double)d * (double)d; }
}
// tv from the three sums: (S_x / count_x + S_y / count_y) + S_z / count_z, absent axes skipped (none: + 0)
GS_BG double gs_bilagrid_tv_value(const double (&s)[3], int Gx, int Gy, int Gz) {
#pragma clang fp contract(off)
    const long long cnt[3] = {gs_bilagrid_tv_count(Gx, Gy * Gz), gs_bilagrid_tv_count(Gy, Gx * Gz), gs_bilagrid_tv_count(Gz, Gx * Gy)};
    double tv = 0.0;
    bool first = true;
    for (int a = 0; a < 3; ++a)
        if (cnt[a] > 0) { const double q = s[a] / (double)cnt[a]; tv = first ? q : tv + q; first = false; }
    return tv;
}
// the gradient of coef tv into one float: G(dz, dy, dx) is the same float of the neighbour vertex (only asked for inside the grid)
template <class Fetch>
GS_BG float gs_bilagrid_tv_grad(float acc, Fetch G, int x, int y, int z, int Gx, int Gy, int Gz, float s_x, float s_y, float s_z) {
#pragma clang fp contract(off)
    const float g = G(0, 0, 0);
    if (Gx >= 2) {
        if (x > 0) acc = acc + s_x * (g - G(0, 0, -1));
        if (x < Gx - 1) acc = acc - s_x * (G(0, 0, 1) - g);
    }
    if (Gy >= 2) {
        if (y > 0) acc = acc + s_y * (g - G(0, -1, 0));
        if (y < Gy - 1) acc = acc - s_y * (G(0, 1, 0) - g);
    }
    if (Gz >= 2) {
        if (z > 0) acc = acc + s_z * (g - G(-1, 0, 0));
        if (z < Gz - 1) acc = acc - s_z * (G(1, 0, 0) - g);
    }
    return acc;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "gs_adam.h"
// gs_bilagrid.hip.  Every pointer is a device pointer; weight may be null.  No atomics, no memset, no scratch buffer.
// apply: one launch.  backward: d_grid null -- one launch; else two: the gather of d_grid (one workgroup per vertex, which reads d_out) and
// then the image pass, so that d_img == d_out is legal.  tv: one launch per non-null output.  adam: one launch over n floats.
hipError_t gs_launch_bilagrid_apply(const float *img, const float *grid, int Gx, int Gy, int Gz, const float *weight, int W, int H, float *out, hipStream_t s);
hipError_t gs_launch_bilagrid_backward(const float *img, const float *d_out, const float *grid, int Gx, int Gy, int Gz, const float *weight, int W, int H,
                                       float *d_img, float *d_grid, hipStream_t s);
hipError_t gs_launch_bilagrid_tv(const float *grid, int Gx, int Gy, int Gz, float coef, float *d_grid, double *tv_out, hipStream_t s);
hipError_t gs_launch_bilagrid_adam(float *grid, const float *d_grid, float *m, float *v, long long n, const GsAdamHyper &h, hipStream_t s);
#endif
