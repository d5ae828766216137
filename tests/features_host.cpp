// The view-space depth of the feature maps (csrc/gs_features.h: gs_view_depth_of) run on the CPU: features_host IN OUT.
// Host code only: built and run by tests/test_features_host.py, which compares OUT with ts[2] of the oracle bit for bit; no device.
// IN, 32-bit words: {n}, T [16] column major, means [n][3].  OUT: z [n].
#include "gs_features.h"
#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    std::vector<uint32_t> in((size_t)ftell(f) / 4);
    fseek(f, 0, SEEK_SET);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    fclose(f);
    if (in.size() < 17) return 3;
    const size_t n = in[0];
    if (in.size() != 17 + 3 * n) return 3;
    float T[16];
    std::memcpy(T, &in[1], sizeof(T));
    std::vector<float> m(3 * n), z(n);
    if (n) std::memcpy(m.data(), &in[17], sizeof(float) * 3 * n);
    for (size_t g = 0; g < n; ++g) z[g] = gs_view_depth_of(T, m[3 * g], m[3 * g + 1], m[3 * g + 2]);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(z.data(), 4, z.size(), f) != z.size()) return 2;
    fclose(f);
    return 0;
}
