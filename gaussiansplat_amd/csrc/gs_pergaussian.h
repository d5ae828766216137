// gs_pergaussian.h -- the statements of the numeric spec that more than one per-gaussian kernel executes,
// written ONCE: quatToRot, the sigmoid of the logit opacity, computeInvCov2d + computeBB, the tile rectangle,
// the depth key, the payload row with its stores, and a gaussian's row of 2-D gradient sums.  Every function turns contraction off
// inside its body (as gs_g2d_to_grads does), so it rounds alike in every translation unit whatever that unit's flags, and everything
// but the stores is __host__ __device__: tests/pergaussian_host.cpp runs the statements that decide tile ids and depth keys on the
// CPU, against the oracle, bit for bit.
//
// Who takes what: DESIGN.md section 5.2.  Not here: t = T [m; 1], p = P t.  As a function it moved the kernels' camera loads and cost
// registers in each of its three callers (geometry chain 148 -> 154 VGPRs, forward at degree 1 68 -> 76 SGPRs; profiles/HISTORY.md), so the
// forward, gs_sh_bwd_kernel and gs_geom_bwd_body.inc keep those two loops as text; gs_sh_views_body.inc has its own as well (its
// translation units contract on purpose, and both of its kernels already share that one body).  The fp64 chain behind t and p is text for
// the same reason, but one text: gs_geom_chain_cov.inc and gs_geom_chain_tail.inc, for the backward and the camera gradient alike.
#pragma once
#include "gs_common.h"
#include "gs_detmath.h"

#define GS_PG __host__ __device__ __forceinline__

// quatToRot, projection.jl:1-14: the raw quaternion (w, x, y, z), the reference's R22 = 1 - 2 (x^2 - z^2) (minus, as written)
template <typename T>
GS_PG void gs_quat_to_rot(T w, T x, T y, T z, T (&R)[3][3]) {
#pragma clang fp contract(off)
    R[0][0] = T(1) - T(2) * (y * y + z * z);
    R[1][0] = T(2) * (x * y + w * z);
    R[2][0] = T(2) * (x * z - w * y);
    R[0][1] = T(2) * (x * y - w * z);
    R[1][1] = T(1) - T(2) * (x * x - z * z);                          // :8
    R[2][1] = T(2) * (y * z + w * x);
    R[0][2] = T(2) * (x * z + w * y);
    R[1][2] = T(2) * (y * z - w * x);
    R[2][2] = T(1) - T(2) * (x * x + y * y);
}

// cusigmoid, splat.jl:175-178: e^x / (1 + e^x); float: the spec's exp, double (the geometry chain): the library's
template <typename T>
GS_PG T gs_sigmoid_logit(float x) {
#pragma clang fp contract(off)
    T ez;
    if constexpr (sizeof(T) == sizeof(float)) ez = gs_expf(x); else ez = exp((double)x);
    return ez / (T(1) + ez);
}

// computeInvCov2d (cov2d.jl:30-45) and computeBB (boundingbox.jl:19-27) of the 2 x 2 covariance a (column major) at the pixel position
// (mux, muy): inv column major, bb = {xmin, ymin, xmax, ymax} (renderer.bbs)
GS_PG void gs_conic_box(const float (&a)[4], float mux, float muy, int W, int H, float (&inv)[4], float (&bb)[4]) {
#pragma clang fp contract(off)
    const float det = a[0] * a[3] - a[2] * a[1];
    const float idet = 1.0f / det;
    inv[0] = a[3] * idet; inv[1] = -(a[1] * idet); inv[2] = -(a[2] * idet); inv[3] = a[0] * idet;
    const float halfad = (a[0] + a[3]) / 2.0f;
    const double disc = (double)(halfad * halfad - det);
    const double sq = sqrt(gs_jlmax(0.1, disc));
    const double e1 = (double)halfad - sq;
    const double e2 = (double)halfad + sq;
    const double r = ceil(3.0 * sqrt(gs_jlmax(e1, e2)));
    bb[0] = (float)gs_jlmax(1.0, floor(-r + (double)mux));
    bb[2] = (float)gs_jlmin((double)W, ceil(r + (double)mux));
    bb[1] = (float)gs_jlmax(1.0, floor(-r + (double)muy));
    bb[3] = (float)gs_jlmin((double)H, ceil(r + (double)muy));
}

GS_PG int gs_tile_div(float v) {
    // Julia div(v, 16f0) + saturation (see oracle gso_tile_rect): v is integer valued.
    v = fminf(fmaxf(v, -1073741824.0f), 1073741824.0f);
    return (int)v / GS_TILE;                       // C integer division truncates like div()
}

GS_PG uint32_t gs_pack_i16(float lo, float hi) {
    const int a = (int)fminf(fmaxf(lo, -32768.0f), 32767.0f);
    const int b = (int)fminf(fmaxf(hi, -32768.0f), 32767.0f);
    return ((uint32_t)a & 0xFFFFu) | ((uint32_t)b << 16);
}

GS_PG bool gs_box_finite(const float (&bb)[4]) {
    return __builtin_isfinite(bb[0]) && __builtin_isfinite(bb[2]) && __builtin_isfinite(bb[1]) && __builtin_isfinite(bb[3]);
}

// tile rectangle, binning.jl:6-27: rc = {x0, x1, y0, y1}, 1-based inclusive; all zero (and false) for a box that is not finite
// (dropped), inverted, or outside the grid
GS_PG bool gs_tile_rect(const float (&bb)[4], int gx, int gy, uint16_t (&rc)[4]) {
    rc[0] = rc[1] = rc[2] = rc[3] = 0;
    if (!gs_box_finite(bb)) return false;
    int bminx = gs_tile_div(floorf(bb[0])) + 1, bmaxx = gs_tile_div(ceilf(bb[2])) + 1;
    int bminy = gs_tile_div(floorf(bb[1])) + 1, bmaxy = gs_tile_div(ceilf(bb[3])) + 1;
    if (bminx > bmaxx || bminy > bmaxy) return false;
    bminx = bminx > 1 ? bminx : 1; bminy = bminy > 1 ? bminy : 1;
    bmaxx = bmaxx < gx ? bmaxx : gx; bmaxy = bmaxy < gy ? bmaxy : gy;
    if (bminx > bmaxx || bminy > bmaxy) return false;
    rc[0] = (uint16_t)bminx; rc[1] = (uint16_t)bmaxx; rc[2] = (uint16_t)bminy; rc[3] = (uint16_t)bmaxy;
    return true;
}

// depth key for sortperm(-tps[3,:], lt=isless), forward.jl:103: order 0 index (no key), 1 descending clip depth, 2 ascending
GS_PG uint32_t gs_depth_key(float clipz, int order) {
    if (order == 0) return 0u;
    const float v = (order == 1) ? -clipz : clipz;
    const uint32_t u = gs_f2u(v);
    return (v != v) ? 0xFFFFFFFFu : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}

// ---- what a preprocess kernel knows of (gaussian, view) when it writes its rows
struct GsSplatView {
    float mux, muy, sig, rgb[3];
    float cov[4], inv[4], bb[4];                   // 2 x 2 column major; bb as gs_conic_box leaves it
    uint16_t rc[4];                                // gs_tile_rect of bb
};
// The payload row, the raw conic, the tile rectangle and (dbg_on) the debug arrays both renderers have.  The near/far skip of
// splat.jl:227 (depth_ok false) becomes an empty pixel box.  A splat whose per-view payload is not finite (degenerate covariance,
// NaN/Inf colour or opacity) is skipped the same way: the reference would write NaN into its pixel box, and its example scrubs those
// NaNs afterwards (examples/main.jl:35); the composite kernels mask arithmetically and could not keep a NaN inside the box.
__device__ __forceinline__ void gs_store_splat(const GsSplatView &s, int64_t g, bool depth_ok, GsPayload *payload, float *invcov,
                                               uint16_t *rect, const GsDebugArrays &dbg, bool dbg_on) {
#pragma clang fp contract(off)
    const bool pay_ok = __builtin_isfinite(s.rgb[0]) && __builtin_isfinite(s.rgb[1]) && __builtin_isfinite(s.rgb[2]) && __builtin_isfinite(s.sig) &&
                        __builtin_isfinite(s.mux) && __builtin_isfinite(s.muy) &&
                        __builtin_isfinite(s.inv[0]) && __builtin_isfinite(s.inv[1]) && __builtin_isfinite(s.inv[2]) && __builtin_isfinite(s.inv[3]);
    GsPayload p;
    p.mx = s.mux; p.my = s.muy; p.sig = s.sig;
    // what the composite kernels' inner loops consume, formed once per (gaussian, view) instead of once per (tile, splat):
    // alpha = exp2(ka dX^2 + kb dX dY + kc dY^2 + l2s); log2 of sig == 0 is -inf: alpha = exp2(-inf) = 0
    p.l2s = fminf(__builtin_amdgcn_logf(s.sig), GS_L2S_CAP);
    p.ka = GS_NEG_HALF_LOG2E * s.inv[0]; p.kb = GS_NEG_HALF_LOG2E * (s.inv[1] + s.inv[2]); p.kc = GS_NEG_HALF_LOG2E * s.inv[3];
    p.r = s.rgb[0]; p.g = s.rgb[1]; p.b = s.rgb[2];
    if (gs_box_finite(s.bb) && depth_ok && pay_ok) { p.bbx = gs_pack_i16(s.bb[0], s.bb[2]); p.bby = gs_pack_i16(s.bb[1], s.bb[3]); }
    else { p.bbx = 1u; p.bby = 1u; }                                   // min 1, max 0: empty
    gs_payload_box_edges(p);
    payload[g] = p;
    reinterpret_cast<float4 *>(invcov)[g] = make_float4(s.inv[0], s.inv[1], s.inv[2], s.inv[3]);
    reinterpret_cast<uint2 *>(rect)[g] = make_uint2((uint32_t)s.rc[0] | ((uint32_t)s.rc[1] << 16), (uint32_t)s.rc[2] | ((uint32_t)s.rc[3] << 16));
    if (dbg_on) {
        dbg.mu[2 * g] = s.mux; dbg.mu[2 * g + 1] = s.muy;
#pragma unroll
        for (int i = 0; i < 4; ++i) { dbg.cov2d[4 * g + i] = s.cov[i]; dbg.invcov[4 * g + i] = s.inv[i]; dbg.bbs[4 * g + i] = s.bb[i]; }
    }
}

// ---- a gaussian's row of 2-D gradient sums (GsCompositeArgs.g2d).  `a`: any argument struct with the members g2d (the float atomics
// buffer) and g2d_fixed (non-null: the deterministic fixed-point buffer, word `comp` scaled by gs_fixed_inv(comp)); GsG2dRows is the bare one.
// (By reference, as the kernels' own copies took it: handing the two pointers over moved the kernels' argument loads and cost the
// degree-0 Adam kernels an SGPR.)
struct GsG2dRows { const float *g2d; const long long *g2d_fixed; };
GS_PG float gs_fixed_to_float(long long word, int comp) { return (float)((double)word * gs_fixed_inv(comp)); }
template <typename A>
GS_PG float gs_g2d_load(const A &a, int64_t g, int comp) {
    return a.g2d_fixed ? gs_fixed_to_float(a.g2d_fixed[GS_G2D_STRIDE * g + comp], comp) : a.g2d[GS_G2D_STRIDE * g + comp];
}
// the three floats d rgb
template <typename A>
GS_PG void gs_g2d_rgb_load(const A &a, int64_t g, float &r, float &gr, float &b) {
    r = gs_g2d_load(a, g, 0); gr = gs_g2d_load(a, g, 1); b = gs_g2d_load(a, g, 2);
}
// the ten used words; the float row is ONE 64-byte sector: three 16-byte loads
template <typename A>
GS_PG void gs_g2d_row_load(const A &a, int64_t g, float (&o)[10]) {
    if (a.g2d_fixed) {
#pragma unroll
        for (int i = 0; i < 10; ++i) o[i] = gs_fixed_to_float(a.g2d_fixed[GS_G2D_STRIDE * g + i], i);
    } else {
        const float4 *r = reinterpret_cast<const float4 *>(a.g2d + GS_G2D_STRIDE * g);
        const float4 v0 = r[0], v1 = r[1], v2 = r[2];
        o[0] = v0.x; o[1] = v0.y; o[2] = v0.z; o[3] = v0.w; o[4] = v1.x; o[5] = v1.y; o[6] = v1.z; o[7] = v1.w; o[8] = v2.x; o[9] = v2.y;
    }
}
