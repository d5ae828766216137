// The exposure stage's statements (csrc/gs_exposure.h) run on the CPU: exposure_host IN OUT, or exposure_host alone.
// Host code only: built and run by tests/test_exposure_host.py (which compares OUT bit for bit with tests/exposure_ref.py), no device.
// IN: int32 {W, H, has_weight}, then E [3][4], x [3][H][W], d [3][H][W] and (has_weight) weight [H][W] as float32.
// OUT: out [3][H][W] and dx [3][H][W] as float32, then the per-pixel terms of the adjoint into E, [12][H W] as float64 (each term the
// difference of gs_exposure_dE_add's accumulators around one pixel, from + 0: the term itself).
// Without arguments: a built-in scene (odd sizes, weights of 0 and 1 among them, the two identity consequences) checked in place; what
// `make -C tests sanitize-exposure` runs under ASan + UBSan.
#include "gs_exposure.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct Result { std::vector<float> out, dx; std::vector<double> terms; };

static Result run(int W, int H, const float *E, const std::vector<float> &x, const std::vector<float> &d, const float *w) {
    const size_t px = (size_t)W * H;
    Result r{std::vector<float>(3 * px), std::vector<float>(3 * px), std::vector<double>(GS_EXPOSURE_FLOATS * px)};
    for (size_t p = 0; p < px; ++p) {
        const float xi[3] = {x[p], x[px + p], x[2 * px + p]}, di[3] = {d[p], d[px + p], d[2 * px + p]};
        float o[3], g[3] = {di[0], di[1], di[2]}, dx[3];
        if (w) { gs_exposure_forward(E, xi, w[p], o); gs_exposure_weigh(di, w[p], g); } else gs_exposure_forward(E, xi, o);
        gs_exposure_dx(E, g, dx);
        double acc[GS_EXPOSURE_FLOATS] = {};
        gs_exposure_dE_add(g, xi, acc);
        for (int c = 0; c < 3; ++c) { r.out[c * px + p] = o[c]; r.dx[c * px + p] = dx[c]; }
        for (int c = 0; c < GS_EXPOSURE_FLOATS; ++c) r.terms[c * px + p] = acc[c];
    }
    return r;
}

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static int self_check() {
    const float I[GS_EXPOSURE_FLOATS] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    uint32_t s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(int32_t)s * (1.0f / 2147483648.0f); };      // [-1, 1)
    int bad = 0;
    static const int sizes[4][2] = {{1, 1}, {5, 7}, {67, 3}, {129, 33}};
    for (const auto &wh : sizes) {
        const int W = wh[0], H = wh[1];
        const size_t px = (size_t)W * H;
        std::vector<float> x(3 * px), d(3 * px), w(px);
        for (float &v : x) v = 4.0f * rnd();
        for (float &v : d) v = rnd();
        for (size_t p = 0; p < px; ++p) w[p] = p % 4 == 0 ? 0.0f : p % 4 == 1 ? 1.0f : 0.5f * (rnd() + 1.0f);
        x[0] = -0.0f;
        float E[GS_EXPOSURE_FLOATS];
        for (int i = 0; i < GS_EXPOSURE_FLOATS; ++i) E[i] = I[i] + 0.2f * rnd();
        const Result plain = run(W, H, I, x, d, nullptr), masked = run(W, H, I, x, d, w.data()), full = run(W, H, E, x, d, w.data());
        for (size_t i = 0; i < 3 * px; ++i) {
            // identity, no weight: x itself (the bits but for -0 -> +0); identity with a weight: w * x exactly
            if (!(plain.out[i] == x[i]) || (x[i] != 0.0f && bits(plain.out[i]) != bits(x[i]))) ++bad;
            if (bits(masked.out[i]) != bits(w[i % px] * (x[i] + 0.0f))) ++bad;
            if (!std::isfinite(full.out[i]) || !std::isfinite(full.dx[i])) ++bad;
        }
        if (bits(plain.out[0]) != 0u) ++bad;                                      // -0 became +0
        for (size_t p = 0; p < px; ++p)
            for (int r = 0; r < 3; ++r) {
                const float g = w[p] * d[r * px + p];
                for (int k = 0; k < 4; ++k)
                    if (full.terms[(4 * r + k) * px + p] != (double)g * (k < 3 ? (double)x[k * px + p] : 1.0)) ++bad;
            }
    }
    if (gs_exposure_rows(1, 1) != 1 || gs_exposure_rows(1024, 1) != 1 || gs_exposure_rows(1025, 1) != 2 || gs_exposure_rows(1920, 1080) != 2025) ++bad;
    printf("exposure_host self-check: %d mismatches\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc == 1) return self_check();
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[3];
    if (fread(h, 4, 3, f) != 3 || h[0] <= 0 || h[1] <= 0) return 2;
    const int W = h[0], H = h[1];
    const size_t px = (size_t)W * H;
    float E[GS_EXPOSURE_FLOATS];
    std::vector<float> x(3 * px), d(3 * px), w(h[2] ? px : 0);
    if (fread(E, 4, GS_EXPOSURE_FLOATS, f) != GS_EXPOSURE_FLOATS || fread(x.data(), 4, 3 * px, f) != 3 * px || fread(d.data(), 4, 3 * px, f) != 3 * px) return 2;
    if (h[2] && fread(w.data(), 4, px, f) != px) return 2;
    fclose(f);
    const Result r = run(W, H, E, x, d, h[2] ? w.data() : nullptr);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(r.out.data(), 4, 3 * px, f); fwrite(r.dx.data(), 4, 3 * px, f); fwrite(r.terms.data(), 8, GS_EXPOSURE_FLOATS * px, f);
    fclose(f);
    return 0;
}
