// gs_sh_basis.inc -- the SH basis of a unit direction, bs[0 .. K) (splat.jl:180-193; degrees 2 and 3 the build's extension), written ONCE.
// Expects in scope: the floats X, Y, Z (the direction), the constants K and DEG (the ACTIVE degree, K = (DEG + 1)^2) and gs_sh.h.
// Declares float bs[K].  Included by gs_preprocess_kernel, gs_sh_bwd_kernel and gs_sh_views_body.inc.
// It is TEXT and not a function because floating-point contraction belongs to the including scope, and the users differ in it on purpose:
// gs_preprocess.hip is built with -ffp-contract=off (bit-identical to the oracle), gs_sh_bwd_kernel turns it off in its body (the fused and
// the two-kernel form must agree) and the two rebuild kernels keep the compiler's default and do fuse.  A __forceinline__ function keeps
// the setting of its own definition wherever it is inlined, so no one function rounds like all three (compare gs_geom_bwd_body.inc).
    float bs[K];
    bs[0] = SH_C0;
    if constexpr (DEG >= 1) { bs[1] = -Y * SH_C1; bs[2] = Z * SH_C1; bs[3] = -X * SH_C1; }
    if constexpr (DEG >= 2) {
        const float xx = X * X, yy = Y * Y, zz = Z * Z, xy = X * Y, yz = Y * Z, xz = X * Z;
        bs[4] = bC2[0] * xy; bs[5] = bC2[1] * yz; bs[6] = bC2[2] * (2 * zz - xx - yy); bs[7] = bC2[3] * xz; bs[8] = bC2[4] * (xx - yy);
        if constexpr (DEG >= 3) {
            bs[9] = bC3[0] * Y * (3 * xx - yy); bs[10] = bC3[1] * xy * Z; bs[11] = bC3[2] * Y * (4 * zz - xx - yy);
            bs[12] = bC3[3] * Z * (2 * zz - 3 * xx - 3 * yy); bs[13] = bC3[4] * X * (4 * zz - xx - yy);
            bs[14] = bC3[5] * Z * (xx - yy); bs[15] = bC3[6] * X * (xx - 3 * yy);
        }
    }
