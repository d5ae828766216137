"""NumPy restatement of the MCMC densification semantics of include/gsplat.h (gs_mcmc_plan / _sample / _relocate / _noise / _regularize; the
statements are csrc/gs_mcmc.h): float32 operation by operation where the statement is float32, uint64 cumsum / searchsorted for the CDF and the
draws, float64 for the relocation.  exp is the numeric spec's (density_ref.expf_spec, the preprocess's gs_expf)."""
import math

import numpy as np

from density_ref import expf_spec, quat_to_rot

f32, f64 = np.float32, np.float64
NMAX = 51
W_ONE = f32(16777216.0)
U_MAX = f32(1.0) - f32(2.0 ** -24)            # 1 - 2^-24: the largest float below 1
O_MAX = 1.0 - 2.0 ** -24
P_MAX = 1.0 - 2.0 ** -23
BINOM = np.array([[float(math.comb(i, k)) if k <= i else 0.0 for k in range(NMAX)] for i in range(NMAX)], f64)   # exact: C(50, 25) < 2^53
RS = 1.0 / np.sqrt(np.arange(NMAX, dtype=f64) + 1.0)


def sigmoid(opac):
    """e / (1 + e) with the spec's exp, float32 (gs_sigmoid_logit<float>)."""
    with np.errstate(all="ignore"):
        e = expf_spec(np.asarray(opac, f32))
        return (e / (f32(1.0) + e)).astype(f32)


def alive(opac, min_logit):
    with np.errstate(invalid="ignore"):
        return np.asarray(opac, f32) > f32(min_logit)


def weights(opac, min_logit):
    """uint32 [n]: floor(sig * 2^24) of the alive gaussians with a finite sig, else 0."""
    sig = sigmoid(opac)
    ok = alive(opac, min_logit) & np.isfinite(sig)
    with np.errstate(all="ignore"):
        w = np.floor(np.where(ok, sig, f32(0.0)) * W_ONE)
    return w.astype(np.uint32)


def plan(opac, min_logit):
    """(cdf uint64 [n], dead int32 ascending, (alive, dead, total)) of gs_mcmc_plan."""
    opac = np.asarray(opac, f32).reshape(-1)
    cdf = np.cumsum(weights(opac, min_logit).astype(np.uint64), dtype=np.uint64)
    dead = np.flatnonzero(~alive(opac, min_logit)).astype(np.int32)
    total = int(cdf[-1]) if len(cdf) else 0
    return cdf, dead, (len(opac) - len(dead), len(dead), total)


def targets(u, total):
    u = np.asarray(u, f32)
    with np.errstate(invalid="ignore"):
        uc = np.where(u >= f32(0.0), u, f32(0.0)).astype(f32)            # negative, or NaN
        uc = np.where(uc > U_MAX, U_MAX, uc).astype(f32)
    t = (uc.astype(f64) * f64(total)).astype(np.uint64)
    return np.minimum(t, np.uint64(total - 1))


def sample(cdf, u):
    """int32 [m]: the smallest i with cdf[i] > t; total > 0."""
    cdf = np.asarray(cdf, np.uint64)
    return np.searchsorted(cdf, targets(u, int(cdf[-1])), side="right").astype(np.int32)


def relocate_p(o, n):
    """p = -expm1(log1p(-o) / n) in float64: 1 - (1 - p)^n = o."""
    return -np.expm1(np.log1p(-np.asarray(o, f64)) / np.asarray(n, f64))


def relocate_values(opac, scales, c, min_opacity):
    """(opacity' float32 [n], scales' float32 [n, 3]) of gaussians drawn c >= 1 times (c int [n]); all arithmetic float64."""
    opac = np.asarray(opac, f32).reshape(-1)
    scales = np.asarray(scales, f32).reshape(-1, 3)
    c = np.asarray(c, np.int64).reshape(-1)
    assert (c >= 1).all()
    nn = np.minimum(c + 1, NMAX)
    with np.errstate(all="ignore"):
        o = sigmoid(opac).astype(f64)
        o = np.where(o >= 0.0, o, 0.0)
        o = np.where(o > O_MAX, O_MAX, o)
        p = relocate_p(o, nn)
        s = np.zeros(len(o), f64)
        for n in np.unique(nn):
            sel = nn == n
            ps, acc = p[sel], np.zeros(int(sel.sum()), f64)
            for i in range(1, int(n) + 1):
                pk = ps.copy()
                for k in range(i):
                    acc = acc + (BINOM[i - 1, k] * (-RS[k] if k & 1 else RS[k])) * pk
                    pk = pk * ps
            s[sel] = acc
        mo = f64(f32(min_opacity))
        pc = np.where(p > mo, p, mo)
        pc = np.where(pc > P_MAX, P_MAX, pc)
        new_op = (np.log(pc) - np.log1p(-pc)).astype(f32)
        new_sc = (scales.astype(f64) + np.log(o / s)[:, None]).astype(f32)
    return new_op, new_sc


def relocate(model, src, dst, min_opacity, sets=()):
    """gs_mcmc_relocate on (means [n,3], scales [n,3], quats [n,4], opacities [n,1], shs [n,3K]) and gradient-shaped companion sets (lists of five
    [n, w] arrays or None).  Returns (new model, new sets, counts int [n]).  Entries of src / dst outside [0, n) make their draw a no-op."""
    means, scales, quats, opac, shs = [np.array(x, f32, copy=True) for x in model]
    n = len(means)
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    src, dst = src[ok], dst[ok]
    cnt = np.bincount(src, minlength=n)
    srcs = np.flatnonzero(cnt > 0)
    new_op, new_sc = relocate_values(opac[srcs, 0], scales[srcs], cnt[srcs], min_opacity)
    op_of, sc_of = np.zeros(n, f32), np.zeros((n, 3), f32)
    op_of[srcs], sc_of[srcs] = new_op, new_sc
    old = [x.copy() for x in (means, quats, shs)]
    means[dst], quats[dst], shs[dst] = old[0][src], old[1][src], old[2][src]
    opac[dst, 0], scales[dst] = op_of[src], sc_of[src]
    opac[srcs, 0], scales[srcs] = new_op, new_sc
    new_sets = []
    for s in sets:
        out = []
        for x in s:
            if x is None:
                out.append(None); continue
            y = np.array(x, f32, copy=True)
            y[srcs] = 0.0; y[dst] = 0.0
            out.append(y)
        new_sets.append(out)
    return [means, scales, quats, opac, shs], new_sets, cnt


def noise(means, scales, quats, opac, z, lr, gate_k=100.0, gate_t=0.005):
    """gs_mcmc_noise: the new means, float32 [n, 3]."""
    means, scales, z = (np.asarray(x, f32).reshape(-1, 3) for x in (means, scales, z))
    lr, gate_k, gate_t = f32(lr), f32(gate_k), f32(gate_t)
    with np.errstate(all="ignore"):
        sig = sigmoid(np.asarray(opac, f32).reshape(-1))
        gate = f32(1.0) / (f32(1.0) + expf_spec((gate_k * (sig - gate_t)).astype(f32)))
        R = quat_to_rot(np.asarray(quats, f32).reshape(-1, 4))
        e = expf_spec(scales)
        b = np.empty_like(means)
        for j in range(3):
            a = (R[:, 0, j] * z[:, 0] + R[:, 1, j] * z[:, 1]) + R[:, 2, j] * z[:, 2]
            b[:, j] = (e[:, j] * e[:, j]) * a
        step = (lr * gate).astype(f32)
        new = np.empty_like(means)
        for i in range(3):
            d = (R[:, i, 0] * b[:, 0] + R[:, i, 1] * b[:, 1]) + R[:, i, 2] * b[:, 2]
            new[:, i] = means[:, i] + step * d
    ok = np.isfinite(new).all(axis=1)
    return np.where(ok[:, None], new, means).astype(f32)


def reg_coefficients(opacity_reg, scale_reg, n):
    """c_o = (float)(lambda_o / N), c_s = (float)(lambda_s / (3 N)): formed in double, rounded once."""
    return f32(float(opacity_reg) / n), f32(float(scale_reg) / (3 * n))


def regularize(d_opac, d_scales, opac, scales, c_o, c_s):
    """gs_mcmc_regularize: (d_opacities', d_scales'); None stays None."""
    with np.errstate(all="ignore"):
        sig = sigmoid(np.asarray(opac, f32).reshape(-1))
        out_o = None if d_opac is None else (np.asarray(d_opac, f32).reshape(-1) + f32(c_o) * (sig * (f32(1.0) - sig))).astype(f32)
        out_s = None if d_scales is None else (np.asarray(d_scales, f32).reshape(-1, 3) + f32(c_s) * expf_spec(np.asarray(scales, f32).reshape(-1, 3))).astype(f32)
    return out_o, out_s
