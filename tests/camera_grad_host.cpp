// The per-gaussian statement of the camera gradient (csrc/gs_camera_grad.h: gs_camera_grad) run on the CPU: camera_grad_host IN OUT.
// Host code only: built and run by tests/test_camera_grad_host.py, which compares OUT with fp64 autograd; no device.
// IN, 32-bit words: {n, active degree, floats per stored SH row}, the GsCamera (44 words: T[16], P[16], fx, fy, near, far, eye[3],
//   lookAt[3], W, H), means [n][3], scales [n][3], quats [n][4], opacities [n], shs [n][stride], raw rows [n][10].
// OUT, doubles: the contributions [n][40], then their sums [40] in index order.
#include "gs_camera_grad.h"
#include <cstdio>
#include <cstring>
#include <vector>

static_assert(sizeof(GsCamera) == 44 * 4, "the camera record of the input file");

template <int DEG>
static void run(size_t n, size_t stride, const GsCamera &cam, const float *means, const float *scales, const float *quats, const float *opac,
                const float *shs, const float *rows, double *out) {
    double *sum = out + GS_CAMERA_GRAD_VALUES * n;
    for (int c = 0; c < GS_CAMERA_GRAD_VALUES; ++c) sum[c] = 0.0;
    for (size_t g = 0; g < n; ++g) {
        float g2f[10];
        std::memcpy(g2f, rows + 10 * g, sizeof(g2f));
        double v[GS_CAMERA_GRAD_VALUES];
        gs_camera_grad<DEG>(g2f, means + 3 * g, scales + 3 * g, quats + 4 * g, opac + g, shs + stride * g, cam, v);
        for (int c = 0; c < GS_CAMERA_GRAD_VALUES; ++c) { out[GS_CAMERA_GRAD_VALUES * g + c] = v[c]; sum[c] += v[c]; }
    }
}

// words -> doubles; 0, or the exit code of a malformed input
static int process(const std::vector<uint32_t> &in, std::vector<double> &out) {
    if (in.size() < 47) return 3;
    const size_t n = in[0], deg = in[1], stride = in[2];
    if (deg > 3 || stride < 3 * (deg + 1) * (deg + 1) || in.size() != 47 + n * (3 + 3 + 4 + 1 + stride + 10)) return 3;
    GsCamera cam;
    std::memcpy(&cam, &in[3], sizeof(cam));
    std::vector<float> data(in.size() - 47 + 1);
    std::memcpy(data.data(), in.data() + 47, sizeof(float) * (in.size() - 47));
    const float *means = data.data(), *scales = means + 3 * n, *quats = scales + 3 * n, *opac = quats + 4 * n, *shs = opac + n, *rows = shs + stride * n;
    out.assign(GS_CAMERA_GRAD_VALUES * (n + 1), 0.0);
    switch (deg) {
        case 0: run<0>(n, stride, cam, means, scales, quats, opac, shs, rows, out.data()); break;
        case 1: run<1>(n, stride, cam, means, scales, quats, opac, shs, rows, out.data()); break;
        case 2: run<2>(n, stride, cam, means, scales, quats, opac, shs, rows, out.data()); break;
        default: run<3>(n, stride, cam, means, scales, quats, opac, shs, rows, out.data()); break;
    }
    return 0;
}

// Without arguments: a small built-in scene at every degree (and degree 1 on rows of degree 3) through the same path, for the host
// sanitizers (make -C tests sanitize-camera-grad): every output finite, a zero row exactly + 0 whatever its model row holds.
static int self_test() {
    uint32_t lcg = 12345u;
    auto uni = [&]() { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) * (1.0f / 16777216.0f); };
    const size_t n = 97;
    for (int pass = 0; pass < 5; ++pass) {
        const size_t deg = pass < 4 ? pass : 1, stride = pass < 4 ? 3 * (deg + 1) * (deg + 1) : 48;
        GsCamera cam{};
        cam.T[0] = 1.0f; cam.T[5] = 1.0f; cam.T[10] = 1.0f; cam.T[14] = 30.0f;
        cam.P[0] = 3.0f; cam.P[5] = 4.0f; cam.P[10] = 1.002f; cam.P[14] = -0.2f; cam.P[11] = 1.0f;
        cam.fx = 100.0f; cam.fy = 100.0f; cam.near_ = 0.1f; cam.far_ = 100.0f; cam.eye[2] = -30.0f; cam.W = 64; cam.H = 48;
        std::vector<uint32_t> in(47 + n * (11 + stride + 10));
        in[0] = (uint32_t)n; in[1] = (uint32_t)deg; in[2] = (uint32_t)stride;
        std::memcpy(&in[3], &cam, sizeof(cam));
        std::vector<float> d(in.size() - 47);
        for (float &v : d) v = uni() - 0.5f;
        float *rows = d.data() + n * (11 + stride);
        for (size_t g = 0; g < n; g += 3) {
            for (int i = 0; i < 10; ++i) rows[10 * g + i] = 0.0f;
            d[3 * g] = g % 2 ? __builtin_nanf("") : 0.0f; d[3 * g + 1] = 0.0f; d[3 * g + 2] = -30.0f;   // NaN mean, or tz == 0
            d[3 * n + 3 * g] = 200.0f;                                                                 // exp overflow
        }
        std::memcpy(&in[47], d.data(), sizeof(float) * d.size());
        std::vector<double> out;
        if (process(in, out)) return 4;
        for (size_t g = 0; g < n; ++g)
            for (int c = 0; c < GS_CAMERA_GRAD_VALUES; ++c) {
                const double v = out[GS_CAMERA_GRAD_VALUES * g + c];
                uint64_t bits;
                std::memcpy(&bits, &v, 8);
                if (!__builtin_isfinite(v) || (g % 3 == 0 && bits != 0)) { std::printf("self-test: pass %d gaussian %zu value %d = %g\n", pass, g, c, v); return 5; }
            }
        for (int c = 0; c < GS_CAMERA_GRAD_VALUES; ++c) if (!__builtin_isfinite(out[GS_CAMERA_GRAD_VALUES * n + c])) return 6;
    }
    std::printf("camera_grad_host self-test: ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 1) return self_test();
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    std::vector<uint32_t> in((size_t)ftell(f) / 4);
    fseek(f, 0, SEEK_SET);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    fclose(f);
    std::vector<double> out;
    if (const int rc = process(in, out)) return rc;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
}
