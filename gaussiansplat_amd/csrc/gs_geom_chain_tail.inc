// gs_geom_chain_tail.inc -- the end of the fp64 geometry chain, written ONCE: dJ into dt (J(t)), the pixel position's gradient into dp (mu(p)),
// and dp into dt (p = P t).  Afterwards dt and dp are the COMPLETE adjoints of t and p.
// Expects in scope: everything gs_geom_chain_cov.inc declares (it stands before this in both includers), cam (GsCamera), P (= cam.P),
// double p[4] (p = P t), double dt[4] (zeros) and double dp[4] (the colour path's d L / d p, fourth entry zero).  Declares itz3, ip3, Wd, Hd.
// Included by gs_geom_bwd_body.inc and gs_camera_grad_factors (gs_camera_grad.h).  Text for the reason given in gs_geom_chain_cov.inc;
// contraction is the including scope's, and both includers turn it off.
    // ---- J(t)
    const double itz3 = itz2 * itz;
    dt[0] += dJ[0][2] * (-fx * itz2);
    dt[1] += dJ[1][2] * (-fy * itz2);
    dt[2] += dJ[0][0] * (-fx * itz2) + dJ[1][1] * (-fy * itz2) + dJ[0][2] * (2 * fx * tx * itz3) + dJ[1][2] * (2 * fy * ty * itz3);
    // ---- mu(p): mu = (W p0/p3 + 1)/2 + W/2
    const double ip3 = 1.0 / p[3];
    const double Wd = (double)cam.W, Hd = (double)cam.H;
    dp[0] += gmx * 0.5 * Wd * ip3;
    dp[1] += gmy * 0.5 * Hd * ip3;
    dp[3] += -(gmx * 0.5 * Wd * p[0] + gmy * 0.5 * Hd * p[1]) * ip3 * ip3;
    // ---- p = P t
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) dt[j] += P[i + 4 * j] * dp[i];
