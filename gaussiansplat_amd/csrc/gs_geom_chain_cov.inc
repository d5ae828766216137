// gs_geom_chain_cov.inc -- the fp64 geometry chain of one gaussian from t down to the 2 x 2 conic and back up to dJ, written ONCE:
// J, R, Sigma, cov = A Sg A^T + 0.3, M = cov^-1, the raw row of 2-D gradient sums turned into gradients, then dcov, dA, dJ.
// Expects in scope: cam (GsCamera); quat, scale, opac (const float *: the gaussian's own rows); double t[4] (t = T [m; 1]) and double g2[10]
// (the row, raw moments, widened) -- g2 is converted in place (gs_g2d_to_grads).
// Declares: tx, ty, tz, fx, fy, itz, itz2, J, w, x, y, z, R, e, Wm, Sg, A, ASg, cov, idet, M, sg, gmx, gmy, G, t1, dcov, off, ds2, dA, dJ.
// Included by gs_geom_bwd_body.inc (which goes on to dSg, dR, de and the quaternion) and by gs_camera_grad_factors (gs_camera_grad.h, which
// needs dJ alone); gs_geom_chain_tail.inc follows in both.
// It is TEXT and not a function for the register counts recorded in gs_geom_bwd_body.inc and gs_pergaussian.h: the chain as a __forceinline__
// function took 186 VGPRs instead of 148 in the backward.  Contraction is the including scope's, and both includers turn it off.
    const double tx = t[0], ty = t[1], tz = t[2], fx = cam.fx, fy = cam.fy;
    const double itz = 1.0 / tz, itz2 = itz * itz;
    const double J[2][3] = {{fx * itz, 0.0, -fx * tx * itz2}, {0.0, fy * itz, -fy * ty * itz2}};
    const double w = quat[0], x = quat[1], y = quat[2], z = quat[3];
    double R[3][3];
    gs_quat_to_rot(w, x, y, z, R);                                    // with the reference's R22 (gs_pergaussian.h)
    const double e[3] = {exp((double)scale[0]), exp((double)scale[1]), exp((double)scale[2])};
    double Wm[3][3], Sg[3][3], A[2][3], ASg[2][3], cov[2][2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Wm[i][j] = R[i][j] * e[j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Sg[i][j] = Wm[i][0] * Wm[j][0] + Wm[i][1] * Wm[j][1] + Wm[i][2] * Wm[j][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A[i][j] = J[i][0] * R[0][j] + J[i][1] * R[1][j] + J[i][2] * R[2][j];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) ASg[i][j] = A[i][0] * Sg[0][j] + A[i][1] * Sg[1][j] + A[i][2] * Sg[2][j];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) cov[i][j] = ASg[i][0] * A[j][0] + ASg[i][1] * A[j][1] + ASg[i][2] * A[j][2] + 0.3;
    const double idet = 1.0 / (cov[0][0] * cov[1][1] - cov[0][1] * cov[1][0]);
    const double M[2][2] = {{cov[1][1] * idet, -cov[0][1] * idet}, {-cov[1][0] * idet, cov[0][0] * idet}};
    const double sg = gs_sigmoid_logit<double>(opac[0]);
    gs_g2d_to_grads(g2, sg, M[0][0], 0.5 * (M[0][1] + M[1][0]), M[1][1]);
    const double gmx = g2[4], gmy = g2[5];
    const double G[2][2] = {{g2[6], g2[7]}, {g2[8], g2[9]}};           // G[r][c] = dL/dM[r][c]

    // ---- M = cov^-1  =>  dcov = -M^T G M^T
    double t1[2][2], dcov[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) t1[i][j] = M[0][i] * G[0][j] + M[1][i] * G[1][j];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) dcov[i][j] = -(t1[i][0] * M[j][0] + t1[i][1] * M[j][1]);
    // ---- cov = A Sg A^T (+0.3): dA = (dcov + dcov^T) A Sg ;  A = J R: dJ = dA R^T
    const double off = dcov[0][1] + dcov[1][0];
    const double ds2[2][2] = {{2 * dcov[0][0], off}, {off, 2 * dcov[1][1]}};
    double dA[2][3], dJ[2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) dA[i][j] = ds2[i][0] * ASg[0][j] + ds2[i][1] * ASg[1][j];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) dJ[i][j] = dA[i][0] * R[j][0] + dA[i][1] * R[j][1] + dA[i][2] * R[j][2];
