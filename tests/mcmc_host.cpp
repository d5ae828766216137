// mcmc_host.cpp -- the statements of gaussiansplat_amd/csrc/gs_mcmc.h in a HOST build: a stand-alone program with its own main.
//     mcmc_host <mode> <in.bin> <out.bin>     tests/test_mcmc_host.py feeds it cases and compares with tests/mcmc_ref.py
//     mcmc_host                               a built-in scene that checks itself (what `make -C tests sanitize-mcmc` runs)
// Every file starts with int64 n.  Modes and layouts (little endian, packed):
//   weight    in: float threshold, float opac[n]                                      out: uint32 w[n]
//   draw      in: int64 m, uint64 cdf[n], float u[m]                                  out: int32 src[m]
//   relocate  in: float min_opacity, float opac[n], float scales[n][3], int32 c[n]    out: float opac'[n], float scales'[n][3]
//   noise     in: float lr, gate_k, gate_t, float means[n][3], scales[n][3], quats[n][4], opac[n], z[n][3]    out: float means'[n][3]
//   reg       in: float c_o, c_s, float opac[n], scales[n][3], d_opac[n], d_scales[n][3]                       out: float d_opac'[n], d_scales'[n][3]
#include "gs_mcmc.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

struct Reader {
    std::vector<unsigned char> buf;
    size_t at = 0;
    bool ok = true;
    explicit Reader(const char *path) {
        FILE *f = std::fopen(path, "rb");
        if (!f) { ok = false; return; }
        unsigned char tmp[65536];
        size_t k;
        while ((k = std::fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + k);
        std::fclose(f);
    }
    template <typename T> T one() {
        T v{};
        if (at + sizeof(T) > buf.size()) { ok = false; return v; }
        std::memcpy(&v, buf.data() + at, sizeof(T));
        at += sizeof(T);
        return v;
    }
    template <typename T> std::vector<T> many(size_t n) {
        std::vector<T> v(n);
        if (n > (buf.size() - at) / sizeof(T)) { ok = false; return v; }
        if (n) std::memcpy(v.data(), buf.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return v;
    }
};

template <typename T> bool put(FILE *f, const std::vector<T> &v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

std::vector<double> binom() {
    std::vector<double> B(GS_MCMC_BINOM);
    gs_mcmc_binom_fill(B.data());
    return B;
}

void run_weight(float thr, const std::vector<float> &opac, std::vector<uint32_t> &w) {
    w.resize(opac.size());
    for (size_t i = 0; i < opac.size(); ++i) w[i] = gs_mcmc_weight(opac[i], thr);
}
void run_draw(const std::vector<uint64_t> &cdf, const std::vector<float> &u, std::vector<int32_t> &src) {
    src.assign(u.size(), -1);
    if (cdf.empty() || cdf.back() == 0) return;
    for (size_t j = 0; j < u.size(); ++j) src[j] = (int32_t)gs_mcmc_search(cdf.data(), (int64_t)cdf.size(), gs_mcmc_target(u[j], cdf.back()));
}
void run_relocate(float min_opacity, const std::vector<float> &opac, const std::vector<float> &sc, const std::vector<int32_t> &c, std::vector<float> &op_out,
                  std::vector<float> &sc_out) {
    const std::vector<double> B = binom();
    op_out.resize(opac.size()); sc_out.resize(sc.size());
    for (size_t i = 0; i < opac.size(); ++i) {
        const float s[3] = {sc[3 * i], sc[3 * i + 1], sc[3 * i + 2]};
        float so[3];
        gs_mcmc_relocated(opac[i], s, c[i], min_opacity, B.data(), op_out[i], so);
        for (int j = 0; j < 3; ++j) sc_out[3 * i + j] = so[j];
    }
}
void run_noise(float lr, float gk, float gt, std::vector<float> &means, const std::vector<float> &sc, const std::vector<float> &q, const std::vector<float> &opac,
               const std::vector<float> &z) {
    for (size_t i = 0; i < opac.size(); ++i) {
        float m[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
        const float s[3] = {sc[3 * i], sc[3 * i + 1], sc[3 * i + 2]};
        const float qq[4] = {q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]};
        const float zz[3] = {z[3 * i], z[3 * i + 1], z[3 * i + 2]};
        if (gs_mcmc_noise(m, s, qq, opac[i], zz, lr, gk, gt))
            for (int j = 0; j < 3; ++j) means[3 * i + j] = m[j];
    }
}
void run_reg(float co, float cs, const std::vector<float> &opac, const std::vector<float> &sc, std::vector<float> &d_op, std::vector<float> &d_sc) {
    for (size_t i = 0; i < opac.size(); ++i) {
        d_op[i] = gs_mcmc_reg_opacity(d_op[i], co, opac[i]);
        for (int j = 0; j < 3; ++j) d_sc[3 * i + j] = gs_mcmc_reg_scale(d_sc[3 * i + j], cs, sc[3 * i + j]);
    }
}

// the built-in scene: properties that need no second implementation
int self_check() {
    int bad = 0;
    const int n = 301;
    std::vector<float> opac(n), sc(3 * n), q(4 * n), means(3 * n), z(3 * n);
    uint32_t r = 12345u;
    auto rnd = [&]() { r = r * 1664525u + 1013904223u; return (float)(r >> 8) * (1.0f / 16777216.0f); };
    for (int i = 0; i < n; ++i) {
        opac[i] = -8.0f + 16.0f * rnd();
        for (int j = 0; j < 3; ++j) { sc[3 * i + j] = -6.0f + 5.0f * rnd(); means[3 * i + j] = 4.0f * rnd() - 2.0f; z[3 * i + j] = 2.0f * rnd() - 1.0f; }
        for (int j = 0; j < 4; ++j) q[4 * i + j] = 2.0f * rnd() - 1.0f;
    }
    opac[3] = __builtin_nanf(""); opac[4] = __builtin_huge_valf(); opac[5] = -__builtin_huge_valf(); opac[6] = 40.0f;
    const float thr = -5.2933049f;                                         // logit(0.005)
    std::vector<uint32_t> w;
    run_weight(thr, opac, w);
    std::vector<uint64_t> cdf(n);
    uint64_t run = 0;
    for (int i = 0; i < n; ++i) {
        if (w[i] > 16777216u || (!(opac[i] > thr) && w[i])) ++bad;
        run += w[i]; cdf[i] = run;
    }
    if (w[3] || w[4] || w[5] || w[6] != 16777216u) ++bad;                  // NaN, +Inf (sig NaN), -Inf (not alive): 0; sig rounding to 1: 2^24
    std::vector<float> u = {0.0f, 0.99999994f, 1.0f, -1.0f, __builtin_nanf(""), 0.5f, 0.25f, 0.75f};
    for (int i = 0; i < 100; ++i) u.push_back(rnd());
    std::vector<int32_t> src;
    run_draw(cdf, u, src);
    for (size_t j = 0; j < u.size(); ++j) {                                // against a linear search, and never a weightless gaussian
        const uint64_t t = gs_mcmc_target(u[j], run);
        int64_t lin = 0;
        while (lin < n && !(cdf[lin] > t)) ++lin;
        if (src[j] != lin || src[j] < 0 || src[j] >= n || w[src[j]] == 0) ++bad;
    }
    std::vector<int32_t> c(n);
    for (int i = 0; i < n; ++i) { c[i] = 1 + i % 60; if (!(opac[i] > thr) || !(opac[i] < 15.0f)) opac[i] = 0.5f; }
    std::vector<float> op2, sc2;
    run_relocate(0.005f, opac, sc, c, op2, sc2);
    for (int i = 0; i < n; ++i) {                                          // (1 - p)^n = 1 - o while the clamp is idle; the copies shrink
        const int nn = c[i] + 1 < GS_MCMC_NMAX ? c[i] + 1 : GS_MCMC_NMAX;
        const double o = (double)gs_sigmoid_logit<float>(opac[i]), p = 1.0 / (1.0 + exp(-(double)op2[i]));
        if (p > 0.0051 && fabs(pow(1.0 - p, nn) - (1.0 - o)) > 1e-5) ++bad;    // (p went through a float: 51 * 2^-24 at the most)
        for (int j = 0; j < 3; ++j) if (!(sc2[3 * i + j] <= sc[3 * i + j]) || !__builtin_isfinite(sc2[3 * i + j])) ++bad;
    }
    std::vector<float> m0 = means, zero(3 * n, 0.0f);
    run_noise(80.0f, 100.0f, 0.005f, m0, sc, q, opac, zero);               // z = 0: +0 is added
    for (int i = 0; i < 3 * n; ++i) if (m0[i] != means[i]) ++bad;
    m0 = means;
    run_noise(80.0f, 100.0f, 0.005f, m0, sc, q, opac, z);
    for (int i = 0; i < 3 * n; ++i) if (!__builtin_isfinite(m0[i])) ++bad;
    std::vector<float> d_op(n, 0.25f), d_sc(3 * n, -0.5f);
    run_reg(0.0f, 0.0f, opac, sc, d_op, d_sc);
    for (int i = 0; i < n; ++i) if (d_op[i] != 0.25f || d_sc[3 * i] != -0.5f) ++bad;
    run_reg(1e-3f, 1e-3f, opac, sc, d_op, d_sc);
    for (int i = 0; i < n; ++i) if (!(d_op[i] > 0.25f) || !(d_sc[3 * i + 2] > -0.5f)) ++bad;
    std::printf("mcmc_host: %d mismatches\n", bad);
    return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 1) return self_check();
    if (argc != 4) { std::fprintf(stderr, "usage: mcmc_host [weight|draw|relocate|noise|reg in.bin out.bin]\n"); return 2; }
    const std::string mode = argv[1];
    Reader in(argv[2]);
    const int64_t n64 = in.one<int64_t>();
    if (!in.ok || n64 < 0 || n64 > (int64_t)1 << 28) { std::fprintf(stderr, "mcmc_host: bad input\n"); return 2; }
    const size_t n = (size_t)n64;
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) { std::fprintf(stderr, "mcmc_host: cannot write %s\n", argv[3]); return 2; }
    bool ok = true;
    if (mode == "weight") {
        const float thr = in.one<float>();
        const std::vector<float> opac = in.many<float>(n);
        std::vector<uint32_t> w;
        if (in.ok) { run_weight(thr, opac, w); ok = put(out, w); }
    } else if (mode == "draw") {
        const int64_t m = in.one<int64_t>();
        if (m < 0 || m > (int64_t)1 << 28) in.ok = false;
        const std::vector<uint64_t> cdf = in.many<uint64_t>(in.ok ? n : 0);
        const std::vector<float> u = in.many<float>(in.ok ? (size_t)m : 0);
        std::vector<int32_t> src;
        if (in.ok) { run_draw(cdf, u, src); ok = put(out, src); }
    } else if (mode == "relocate") {
        const float mo = in.one<float>();
        const std::vector<float> opac = in.many<float>(n), sc = in.many<float>(3 * n);
        const std::vector<int32_t> c = in.many<int32_t>(n);
        std::vector<float> op2, sc2;
        if (in.ok) { run_relocate(mo, opac, sc, c, op2, sc2); ok = put(out, op2) && put(out, sc2); }
    } else if (mode == "noise") {
        const float lr = in.one<float>(), gk = in.one<float>(), gt = in.one<float>();
        std::vector<float> means = in.many<float>(3 * n);
        const std::vector<float> sc = in.many<float>(3 * n), q = in.many<float>(4 * n), opac = in.many<float>(n), z = in.many<float>(3 * n);
        if (in.ok) { run_noise(lr, gk, gt, means, sc, q, opac, z); ok = put(out, means); }
    } else if (mode == "reg") {
        const float co = in.one<float>(), cs = in.one<float>();
        const std::vector<float> opac = in.many<float>(n), sc = in.many<float>(3 * n);
        std::vector<float> d_op = in.many<float>(n), d_sc = in.many<float>(3 * n);
        if (in.ok) { run_reg(co, cs, opac, sc, d_op, d_sc); ok = put(out, d_op) && put(out, d_sc); }
    } else {
        in.ok = false;
    }
    ok = (std::fclose(out) == 0) && ok;
    if (!in.ok || !ok) { std::fprintf(stderr, "mcmc_host: bad input or short write\n"); return 2; }
    return 0;
}
