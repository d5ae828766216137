// knn_host.cpp -- the whole 3-NN pipeline of csrc/gs_knn.hip, serially on the CPU, with the statements of csrc/gs_knn.h: bounding box and
// count of the finite points, Morton keys, a stable sort, boxes and super-boxes, the bound-pruned search.  A stand-alone program
// (tests/test_pointcloud_host.py builds it host-side and runs it as a child process; also built with sanitizers):
//   knn_host in.bin out.bin
// in.bin : u32 clouds, then per cloud u32 n and 3 n floats.     out.bin: per cloud n floats (dist2).
// stdout : per cloud one line "cloud <k> n <n> pruned <P> opened <O>": the (query, box) pairs its search ruled out by a bound / opened.
// It prunes per QUERY (the device prunes per wave: a box is opened when some lane needs it), so every bound is put to the test on its own.
#include "gs_knn.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

namespace {

struct P4 { float x, y, z; uint32_t idx; };
struct Box { float lo[3], hi[3]; };

Box empty_box() {
    const float inf = std::numeric_limits<float>::infinity();
    return Box{{inf, inf, inf}, {-inf, -inf, -inf}};
}
void grow(Box &b, const float *lo, const float *hi) {
    for (int a = 0; a < 3; ++a) { b.lo[a] = fminf(b.lo[a], lo[a]); b.hi[a] = fmaxf(b.hi[a], hi[a]); }
}
float bound(const P4 &q, const Box &b) { return gs_knn_box_bound(q.x, q.y, q.z, b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]); }

void knn(const std::vector<float> &pts, size_t n, std::vector<float> &out, unsigned long long &pruned, unsigned long long &opened) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    pruned = opened = 0;
    out.assign(n, nan);
    if (n == 0) return;
    Box all = empty_box();
    size_t m = 0;
    for (size_t i = 0; i < n; ++i)
        if (gs_knn_finite(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2])) { grow(all, &pts[3 * i], &pts[3 * i]); ++m; }
    std::vector<uint64_t> pairs(n);
    for (size_t i = 0; i < n; ++i)
        pairs[i] = ((uint64_t)gs_knn_key(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], all.lo, all.hi) << 32) | (uint64_t)i;
    std::stable_sort(pairs.begin(), pairs.end(), [](uint64_t a, uint64_t b) { return (a >> 32) < (b >> 32); });
    const size_t nb = (n + GS_KNN_BOX - 1) / GS_KNN_BOX, ns = (nb + GS_KNN_SUPER - 1) / GS_KNN_SUPER;
    std::vector<P4> sorted(nb * GS_KNN_BOX, P4{inf, inf, inf, 0xFFFFFFFFu});
    std::vector<Box> boxes(nb, empty_box()), supers(ns, empty_box());
    for (size_t pos = 0; pos < n; ++pos) {
        const uint32_t idx = (uint32_t)pairs[pos];
        sorted[pos].idx = idx;
        if ((uint32_t)(pairs[pos] >> 32) == GS_KNN_KEY_NONFINITE) continue;
        sorted[pos].x = pts[3 * (size_t)idx]; sorted[pos].y = pts[3 * (size_t)idx + 1]; sorted[pos].z = pts[3 * (size_t)idx + 2];
        grow(boxes[pos / GS_KNN_BOX], &pts[3 * (size_t)idx], &pts[3 * (size_t)idx]);
    }
    for (size_t k = 0; k < nb; ++k) grow(supers[k / GS_KNN_SUPER], boxes[k].lo, boxes[k].hi);
    for (size_t pos = 0; pos < n; ++pos) {
        const P4 q = sorted[pos];
        if (m < GS_KNN_MIN_POINTS || !std::isfinite(q.x)) continue;        // NaN stays
        const size_t own = pos / GS_KNN_BOX;
        float b0 = inf, b1 = inf, b2 = inf;
        auto open = [&](size_t k) {
            for (size_t j = k * GS_KNN_BOX; j < (k + 1) * GS_KNN_BOX; ++j) {
                const P4 &c = sorted[j];
                gs_knn_insert(j == pos ? inf : gs_knn_d2(q.x, q.y, q.z, c.x, c.y, c.z), b0, b1, b2);      // self: by sorted position
            }
        };
        open(own);
        for (size_t s = 0; s < ns; ++s) {
            const size_t k0 = s * GS_KNN_SUPER, k1 = std::min(nb, k0 + GS_KNN_SUPER);
            if (!(bound(q, supers[s]) < b2)) { pruned += (k1 - k0) - (own >= k0 && own < k1 ? 1 : 0); continue; }
            for (size_t k = k0; k < k1; ++k) {
                if (k == own) continue;
                if (!(bound(q, boxes[k]) < b2)) { ++pruned; continue; }
                ++opened;
                open(k);
            }
        }
        out[q.idx] = gs_knn_mean3(b0, b1, b2);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: knn_host in.bin out.bin\n"); return 2; }
    FILE *fi = std::fopen(argv[1], "rb");
    if (!fi) { std::perror(argv[1]); return 1; }
    FILE *fo = std::fopen(argv[2], "wb");
    if (!fo) { std::perror(argv[2]); std::fclose(fi); return 1; }
    uint32_t clouds = 0;
    int rc = std::fread(&clouds, sizeof(clouds), 1, fi) == 1 ? 0 : 1;
    for (uint32_t k = 0; !rc && k < clouds; ++k) {
        uint32_t n = 0;
        if (std::fread(&n, sizeof(n), 1, fi) != 1) { rc = 1; break; }
        std::vector<float> pts(3 * (size_t)n), out;
        if (n && std::fread(pts.data(), sizeof(float), pts.size(), fi) != pts.size()) { rc = 1; break; }
        unsigned long long pruned = 0, opened = 0;
        knn(pts, n, out, pruned, opened);
        if (n && std::fwrite(out.data(), sizeof(float), out.size(), fo) != out.size()) { rc = 1; break; }
        std::printf("cloud %u n %u pruned %llu opened %llu\n", k, n, pruned, opened);
    }
    std::fclose(fi);
    if (std::fclose(fo) != 0) rc = 1;
    if (rc) std::fprintf(stderr, "knn_host: short read or write\n");
    return rc;
}
