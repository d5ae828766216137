// The evaluation metrics' statements (csrc/gs_metrics.h) run on the CPU: metrics_host IN OUT.
// Host code only: built and run by tests/test_metrics_host.py (which compares OUT with a float64 torch restatement), no device.
// IN: int32 {C, H, W, has_weight}, then img [C][H][W], gt [C][H][W] and (has_weight) weight [H][W] as float32.
// OUT, float64: the four sums, {mse, mae, ssim, psnr} of gs_metric_finish, then the map [C][H][W].
// The passes are the kernel's: zero padding of 5, the five planes of a widened sample pair, columns first, then rows, taps in ascending order.
#include "gs_metrics.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[4];
    if (fread(h, 4, 4, f) != 4) return 2;
    const int C = h[0], H = h[1], W = h[2];
    const size_t px = (size_t)H * W, n = px * C;
    std::vector<float> img(n), gt(n), wt(h[3] ? px : 0);
    if (fread(img.data(), 4, n, f) != n || fread(gt.data(), 4, n, f) != n) return 2;
    if (h[3] && fread(wt.data(), 4, px, f) != px) return 2;
    fclose(f);
    double g[GS_METRIC_WIN];
    gs_metric_window(g);
    const int PW = W + 2 * GS_METRIC_PAD, PH = H + 2 * GS_METRIC_PAD;
    std::vector<double> pad((size_t)GS_METRIC_PLANES * PH * PW), col((size_t)GS_METRIC_PLANES * H * PW), map(n);
    double sums[GS_METRIC_NSUMS] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < C; ++c) {
        std::fill(pad.begin(), pad.end(), 0.0);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                double p[GS_METRIC_PLANES];
                gs_metric_planes(img[c * px + (size_t)y * W + x], gt[c * px + (size_t)y * W + x], p);
                for (int q = 0; q < GS_METRIC_PLANES; ++q) pad[((size_t)q * PH + y + GS_METRIC_PAD) * PW + x + GS_METRIC_PAD] = p[q];
            }
        for (int q = 0; q < GS_METRIC_PLANES; ++q)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < PW; ++x) col[((size_t)q * H + y) * PW + x] = gs_metric_taps(g, &pad[((size_t)q * PH + y) * PW + x], PW);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                double m[GS_METRIC_PLANES];
                for (int q = 0; q < GS_METRIC_PLANES; ++q) m[q] = gs_metric_taps(g, &col[((size_t)q * H + y) * PW + x], 1);
                const size_t i = c * px + (size_t)y * W + x;
                const double S = gs_ssim_pixel(m), d = (double)img[i] - (double)gt[i], w = h[3] ? (double)wt[(size_t)y * W + x] : 1.0;
                map[i] = S;
                sums[0] += w * (d * d); sums[1] += w * fabs(d); sums[2] += w * S; sums[3] += w;
            }
    }
    double fin[4];
    gs_metric_finish(sums, fin);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(sums, 8, GS_METRIC_NSUMS, f); fwrite(fin, 8, 4, f); fwrite(map.data(), 8, n, f);
    fclose(f);
    return 0;
}
