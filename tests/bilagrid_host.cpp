// The bilateral grid's statements (csrc/gs_bilagrid.h) run on the CPU: bilagrid_host IN OUT, or bilagrid_host alone.
// Host code only: built and run by tests/test_bilagrid_host.py (which compares OUT bit for bit with tests/bilagrid_ref.py), no device.
// IN: int32 {W, H, Gx, Gy, Gz, has_weight}, float32 coef, then G [Gz][Gy][Gx][12], d_grid0 [Gz][Gy][Gx][12], x [3][H][W], d [3][H][W] and
// (has_weight) weight [H][W] as float32.
// OUT: out [3][H][W] and dx [3][H][W] as float32; the vertex of every corner of every pixel, [8][H W] int32; the terms of the adjoint into the
// grid, [8][H W][12] float64 (each the difference of gs_bilagrid_dG_add's accumulators around one corner, from + 0: the term itself); tv, one
// float64 (the squares added float by float in the grid's order); d_grid0 + the gradient of coef tv, [Gz][Gy][Gx][12] float32.
// Without arguments: a built-in scene (odd sizes, an image smaller than the grid, axes of one vertex, weights of 0 and 1, a -0 and a NaN sample,
// the two identity consequences) checked in place; what _build/bilagrid_host_asan runs under ASan + UBSan.
#include "gs_bilagrid.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct Result {
    std::vector<float> out, dx;
    std::vector<int32_t> vertex;
    std::vector<double> terms;
    double tv;
    std::vector<float> d_grid;
};

static Result run(int W, int H, int Gx, int Gy, int Gz, float coef, const std::vector<float> &G, const std::vector<float> &d_grid0,
                  const std::vector<float> &x, const std::vector<float> &d, const float *w) {
    const size_t px = (size_t)W * H, nf = (size_t)Gx * Gy * Gz * GS_BILAGRID_FLOATS;
    Result r{std::vector<float>(3 * px), std::vector<float>(3 * px), std::vector<int32_t>(8 * px), std::vector<double>(8 * px * GS_BILAGRID_FLOATS), 0.0,
             std::vector<float>(nf)};
    const float sx = gs_bilagrid_scale(Gx, W), sy = gs_bilagrid_scale(Gy, H);
    for (int row = 0; row < H; ++row)
        for (int col = 0; col < W; ++col) {
            const size_t p = (size_t)row * W + col;
            const float xi[3] = {x[p], x[px + p], x[2 * px + p]}, di[3] = {d[p], d[px + p], d[2 * px + p]};
            const float l = gs_bilagrid_luminance(xi);
            const GsBilaCell c = gs_bilagrid_pixel_cell(col, row, l, sx, sy, Gx, Gy, Gz);
            float A[GS_BILAGRID_FLOATS], S[GS_BILAGRID_FLOATS], o[3], g[3] = {di[0], di[1], di[2]}, dx[3], u[8];
            gs_bilagrid_slice(c, [&](int k, int m) { return G[(size_t)gs_bilagrid_vertex(c, k, Gx, Gy) * GS_BILAGRID_FLOATS + m]; }, A, S);
            gs_bilagrid_affine(A, xi, o);
            if (w) {
                for (int q = 0; q < 3; ++q) o[q] = w[p] * o[q];
                gs_bilagrid_weigh(di, w[p], g);
            }
            gs_bilagrid_dx(A, S, g, xi, l, Gz, dx);
            gs_bilagrid_weights(c, u);
            for (int q = 0; q < 3; ++q) { r.out[q * px + p] = o[q]; r.dx[q * px + p] = dx[q]; }
            for (int k = 0; k < 8; ++k) {
                double acc[GS_BILAGRID_FLOATS] = {};
                gs_bilagrid_dG_add(u[k], g, xi, acc);
                r.vertex[k * px + p] = gs_bilagrid_vertex(c, k, Gx, Gy);
                for (int m = 0; m < GS_BILAGRID_FLOATS; ++m) r.terms[(k * px + p) * GS_BILAGRID_FLOATS + m] = acc[m];
            }
        }
    const int rowf = Gx * GS_BILAGRID_FLOATS, plane = Gy * rowf;
    const float s_x = gs_bilagrid_tv_scale(coef, gs_bilagrid_tv_count(Gx, Gy * Gz)), s_y = gs_bilagrid_tv_scale(coef, gs_bilagrid_tv_count(Gy, Gx * Gz)),
                s_z = gs_bilagrid_tv_scale(coef, gs_bilagrid_tv_count(Gz, Gx * Gy));
    double s[3] = {0.0, 0.0, 0.0};
    for (int z = 0; z < Gz; ++z)
        for (int y = 0; y < Gy; ++y)
            for (int xv = 0; xv < Gx; ++xv)
                for (int m = 0; m < GS_BILAGRID_FLOATS; ++m) {
                    const int e = z * plane + y * rowf + xv * GS_BILAGRID_FLOATS + m;
                    auto at = [&](int dz, int dy, int dxv) { return G[e + dz * plane + dy * rowf + dxv * GS_BILAGRID_FLOATS]; };
                    gs_bilagrid_tv_add(at, xv, y, z, Gx, Gy, Gz, s);
                    r.d_grid[e] = gs_bilagrid_tv_grad(d_grid0[e], at, xv, y, z, Gx, Gy, Gz, s_x, s_y, s_z);
                }
    r.tv = gs_bilagrid_tv_value(s, Gx, Gy, Gz);
    return r;
}

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static int self_check() {
    uint32_t s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(int32_t)s * (1.0f / 2147483648.0f); };      // [-1, 1)
    int bad = 0;
    static const int shapes[5][5] = {{37, 23, 4, 3, 2}, {5, 3, 16, 16, 8}, {64, 1, 3, 1, 4}, {1, 9, 2, 5, 1}, {67, 9, 64, 1, 64}};
    for (const auto &sh : shapes) {
        const int W = sh[0], H = sh[1], Gx = sh[2], Gy = sh[3], Gz = sh[4];
        const size_t px = (size_t)W * H, nv = (size_t)Gx * Gy * Gz, nf = nv * GS_BILAGRID_FLOATS;
        std::vector<float> x(3 * px), d(3 * px), w(px), I(nf), G(nf), zero(nf, 0.0f);
        for (float &v : x) v = 0.5f + 0.6f * rnd();                              // [-0.1, 1.1)
        for (float &v : d) v = rnd();
        for (size_t p = 0; p < px; ++p) w[p] = p % 4 == 0 ? 0.0f : p % 4 == 1 ? 1.0f : 0.5f * (rnd() + 1.0f);
        for (size_t i = 0; i < nf; ++i) { I[i] = (i % 12) % 5 == 0 ? 1.0f : 0.0f; G[i] = I[i] + 0.2f * rnd(); }
        x[0] = x[px] = x[2 * px] = -0.0f;
        const Result plain = run(W, H, Gx, Gy, Gz, 0.0f, I, zero, x, d, nullptr), masked = run(W, H, Gx, Gy, Gz, 0.0f, I, zero, x, d, w.data());
        for (size_t i = 0; i < 3 * px; ++i) {
            // identity, no weight: x itself (the bits but for -0 -> +0); identity with a weight: w * x exactly
            if (!(plain.out[i] == x[i]) || (x[i] != 0.0f && bits(plain.out[i]) != bits(x[i]))) ++bad;
            if (bits(masked.out[i]) != bits(w[i % px] * (x[i] + 0.0f))) ++bad;
        }
        if (bits(plain.out[0]) != 0u) ++bad;                                      // -0 became +0
        if (plain.tv != 0.0) ++bad;
        for (size_t i = 0; i < nf; ++i) if (bits(plain.d_grid[i]) != 0u) ++bad;    // a flat grid has no TV gradient
        x[px + px / 2] = NAN;
        const Result full = run(W, H, Gx, Gy, Gz, 10.0f, G, zero, x, d, w.data());
        for (size_t p = 0; p < px; ++p) {
            const bool nan_px = p == px / 2;                                      // a NaN sample: every channel of out is NaN (0 * NaN too)
            for (int q = 0; q < 3; ++q)
                if (std::isfinite(full.out[q * px + p]) == nan_px || (!nan_px && !std::isfinite(full.dx[q * px + p]))) ++bad;
            for (int k = 0; k < 8; ++k) {
                const int v = full.vertex[k * px + p];
                if (v < 0 || (size_t)v >= nv) ++bad;
            }
        }
        if (!(full.tv > 0.0) || !std::isfinite(full.tv)) ++bad;
    }
    printf("bilagrid_host self-check: %d mismatches\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc == 1) return self_check();
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[6];
    float coef;
    if (fread(h, 4, 6, f) != 6 || fread(&coef, 4, 1, f) != 1) return 2;
    for (int i = 0; i < 2; ++i) if (h[i] <= 0) return 2;
    for (int i = 2; i < 5; ++i) if (h[i] < 1 || h[i] > GS_BILAGRID_MAX_DIM) return 2;
    const int W = h[0], H = h[1], Gx = h[2], Gy = h[3], Gz = h[4];
    const size_t px = (size_t)W * H, nf = (size_t)Gx * Gy * Gz * GS_BILAGRID_FLOATS;
    std::vector<float> G(nf), d0(nf), x(3 * px), d(3 * px), w(h[5] ? px : 0);
    if (fread(G.data(), 4, nf, f) != nf || fread(d0.data(), 4, nf, f) != nf || fread(x.data(), 4, 3 * px, f) != 3 * px || fread(d.data(), 4, 3 * px, f) != 3 * px)
        return 2;
    if (h[5] && fread(w.data(), 4, px, f) != px) return 2;
    fclose(f);
    const Result r = run(W, H, Gx, Gy, Gz, coef, G, d0, x, d, h[5] ? w.data() : nullptr);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(r.out.data(), 4, 3 * px, f); fwrite(r.dx.data(), 4, 3 * px, f); fwrite(r.vertex.data(), 4, 8 * px, f);
    fwrite(r.terms.data(), 8, 8 * px * GS_BILAGRID_FLOATS, f); fwrite(&r.tv, 8, 1, f); fwrite(r.d_grid.data(), 4, nf, f);
    fclose(f);
    return 0;
}
