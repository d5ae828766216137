// gs_sh_ddir.inc -- the derivative of the SH basis (gs_sh_basis.inc) with respect to the unit direction, contracted with the colour:
// ddir[a] += sum_k cs[k] d bs[k] / d dir[a], degrees 1 .. 3, written ONCE.
// Expects in scope: the macro GS_SH_DDIR_T (the scalar type), X, Y, Z (the direction) and cs[K] (cs[k] = d rgb . sh[:, k]) of that type,
// ddir[3] to add to, the constant DEG (the ACTIVE degree), SH_C1 and the coefficients bC2[5], bC3[7] -- whatever those two names mean in the
// including scope.  Included by gs_sh_bwd_kernel with float (bC2 / bC3: the __constant__ arrays of gs_sh.h, loaded) and by
// gs_camera_grad_factors (gs_camera_grad.h) with double (local constexpr arrays of the same literals, GS_SH_C2_VALUES / GS_SH_C3_VALUES,
// widened; SH_C1 stays the float macro: a float literal times a double is the widened value).
// Text for the reason gs_sh_basis.inc gives: the type and the contraction are the including scope's; both includers turn contraction off.
    if constexpr (DEG >= 1) { ddir[0] += -SH_C1 * cs[3]; ddir[1] += -SH_C1 * cs[1]; ddir[2] += SH_C1 * cs[2]; }
    if constexpr (DEG >= 2) {
        ddir[0] += bC2[0] * Y * cs[4] - 2 * bC2[2] * X * cs[6] + bC2[3] * Z * cs[7] + 2 * bC2[4] * X * cs[8];
        ddir[1] += bC2[0] * X * cs[4] + bC2[1] * Z * cs[5] - 2 * bC2[2] * Y * cs[6] - 2 * bC2[4] * Y * cs[8];
        ddir[2] += bC2[1] * Y * cs[5] + 4 * bC2[2] * Z * cs[6] + bC2[3] * X * cs[7];
    }
    if constexpr (DEG >= 3) {
        const GS_SH_DDIR_T xx = X * X, yy = Y * Y, zz = Z * Z, xy = X * Y, yz = Y * Z, xz = X * Z;
        ddir[0] += 6 * bC3[0] * xy * cs[9] + bC3[1] * yz * cs[10] - 2 * bC3[2] * xy * cs[11] - 6 * bC3[3] * xz * cs[12]
                   + bC3[4] * (4 * zz - 3 * xx - yy) * cs[13] + 2 * bC3[5] * xz * cs[14] + bC3[6] * (3 * xx - 3 * yy) * cs[15];
        ddir[1] += bC3[0] * (3 * xx - 3 * yy) * cs[9] + bC3[1] * xz * cs[10] + bC3[2] * (4 * zz - xx - 3 * yy) * cs[11]
                   - 6 * bC3[3] * yz * cs[12] - 2 * bC3[4] * xy * cs[13] - 2 * bC3[5] * yz * cs[14] - 6 * bC3[6] * xy * cs[15];
        ddir[2] += bC3[1] * xy * cs[10] + 8 * bC3[2] * yz * cs[11] + bC3[3] * (6 * zz - 3 * xx - 3 * yy) * cs[12]
                   + 8 * bC3[4] * xz * cs[13] + bC3[5] * (xx - yy) * cs[14];
    }
