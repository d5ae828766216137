// The spec's per-gaussian statements (csrc/gs_pergaussian.h, csrc/gs_detmath.h) run on the CPU: pergaussian_host IN OUT.
// Host code only: built and run by tests/test_pergaussian_host.py (which compares OUT with the oracle bit for bit), no device.
// IN, 32-bit words: header {n3, W3, H3, n2, W2, H2, nz, nx, na, nq, nf}, then per set cov2d [n][4] and mu [n][2], the clip depths [nz],
// the exp arguments [nx], the angles [na], the quaternions [nq][4], the fixed-point words as {lo, hi, comp} [nf].
// OUT: per set invcov [n][4], bbs [n][4], rect int32 [n][4]; depth keys for orders 0, 1, 2 [3][nz]; exp [nx]; sin [na], cos [na];
// R [nq][9] as R[i][j] at 3 i + j; the fixed-point words as floats [nf].
#include "gs_pergaussian.h"
#include <cstdio>
#include <cstring>
#include <vector>

static std::vector<uint32_t> in, out;
static size_t pos = 0;
static float getf() { return gs_u2f(in[pos++]); }
static void putf(float f) { out.push_back(gs_f2u(f)); }

static void conic_box_rect(int n, int W, int H) {
    const int gx = (W + GS_TILE - 1) / GS_TILE, gy = (H + GS_TILE - 1) / GS_TILE;
    std::vector<float> cov(4 * n), mu(2 * n);
    for (float &v : cov) v = getf();
    for (float &v : mu) v = getf();
    std::vector<GsSplatView> sv(n);
    for (int g = 0; g < n; ++g) {
        for (int i = 0; i < 4; ++i) sv[g].cov[i] = cov[4 * g + i];
        gs_conic_box(sv[g].cov, mu[2 * g], mu[2 * g + 1], W, H, sv[g].inv, sv[g].bb);
        gs_tile_rect(sv[g].bb, gx, gy, sv[g].rc);
    }
    for (int g = 0; g < n; ++g) for (int i = 0; i < 4; ++i) putf(sv[g].inv[i]);
    for (int g = 0; g < n; ++g) for (int i = 0; i < 4; ++i) putf(sv[g].bb[i]);
    for (int g = 0; g < n; ++g) for (int i = 0; i < 4; ++i) out.push_back((uint32_t)sv[g].rc[i]);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    in.resize((size_t)ftell(f) / 4);
    fseek(f, 0, SEEK_SET);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    fclose(f);
    int h[11];
    for (int &v : h) v = (int)in[pos++];
    conic_box_rect(h[0], h[1], h[2]);
    conic_box_rect(h[3], h[4], h[5]);
    const int nz = h[6], nx = h[7], na = h[8], nq = h[9], nf = h[10];
    for (int order = 0; order < 3; ++order)
        for (int i = 0; i < nz; ++i) out.push_back(gs_depth_key(gs_u2f(in[pos + i]), order));
    pos += nz;
    for (int i = 0; i < nx; ++i) putf(gs_expf(getf()));
    std::vector<float> sn(na), cs(na);
    for (int i = 0; i < na; ++i) gs_sincosf(getf(), sn[i], cs[i]);
    for (float v : sn) putf(v);
    for (float v : cs) putf(v);
    for (int q = 0; q < nq; ++q) {
        float R[3][3];
        const float w = getf(), x = getf(), y = getf(), z = getf();
        gs_quat_to_rot(w, x, y, z, R);
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) putf(R[i][j]);
    }
    for (int i = 0; i < nf; ++i, pos += 3)
        putf(gs_fixed_to_float((long long)(((uint64_t)in[pos + 1] << 32) | in[pos]), (int)in[pos + 2]));
    if (pos != in.size()) return 3;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
}
