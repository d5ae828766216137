"""NumPy float32 restatement of the Adam step documented in include/gsplat.h (gs_adam_step / gs_backward_adam).

The host scalars are computed in double and rounded to float once; every float is then stepped in float32 with one rounding
per operation (NumPy has no fma contraction, and its sqrt and '/' are correctly rounded), in torch's order:
    m = b1*m + omb1*g;   v = b2*v + (omb2*g)*g;   p = p - step_size[grp] * (m / (sqrt(v)/sqrt_bc2 + eps))
"""
import math

import numpy as np

GROUPS = 6
ARRAYS = ("means", "scales", "quats", "opacities", "shs")      # the five arrays of a gs_grads, in order


def hyper(lr, beta1, beta2, eps, step):
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))     # the C ABI takes the betas as float
    bc1 = 1.0 - math.pow(b1, float(step))
    return dict(b1=np.float32(b1), b2=np.float32(b2), omb1=np.float32(1.0 - b1), omb2=np.float32(1.0 - b2), eps=np.float32(eps),
                step_size=[np.float32(float(np.float32(x)) / bc1) for x in lr],
                sqrt_bc2=np.float32(math.sqrt(1.0 - math.pow(b2, float(step)))))


def update(p, m, v, g, h, step_size):
    """One step of float32 arrays; step_size: a float32 scalar or an array broadcast against p.  Returns (p, m, v)."""
    p, m, v, g = (np.asarray(a, np.float32) for a in (p, m, v, g))
    with np.errstate(all="ignore"):
        m = h["b1"] * m + h["omb1"] * g
        v = h["b2"] * v + (h["omb2"] * g) * g
        den = np.sqrt(v) / h["sqrt_bc2"] + h["eps"]
        p = p - np.asarray(step_size, np.float32) * (m / den)
    return p.astype(np.float32), m.astype(np.float32), v.astype(np.float32)


def group_steps(h, k, width):
    """Step sizes of array k (0..4) of rows `width` floats wide: arrays 0..3 one group each, the fifth by column (SH band 0 = the
    first three floats -> group 4, the rest -> group 5; the 2-D renderer's colours are three floats wide: all group 4)."""
    if k < 4:
        return h["step_size"][k]
    col = np.arange(width)
    return np.where(col < 3, h["step_size"][4], h["step_size"][5]).astype(np.float32)[None, :]


def step(params, grads, m, v, lr, beta1, beta2, eps, t, selective=False):
    """params / m / v: lists of five float32 arrays [n, w] (updated copies are returned); grads: five arrays or None (frozen).
    selective: rows whose gradient floats all compare == 0 (over every non-None gradient array) are left alone."""
    h = hyper(lr, beta1, beta2, eps, t)
    P, M, V = [np.array(a, np.float32, copy=True) for a in params], [np.array(a, np.float32, copy=True) for a in m], \
              [np.array(a, np.float32, copy=True) for a in v]
    n = P[0].shape[0]
    live = np.zeros(n, bool)
    for g in grads:
        if g is not None:
            live |= np.any(np.asarray(g, np.float32).reshape(n, -1) != 0.0, axis=1)
    for k in range(5):
        if grads[k] is None:
            continue
        shape = P[k].shape
        p2, m2, v2, g2 = (np.asarray(a, np.float32).reshape(n, -1) for a in (P[k], M[k], V[k], grads[k]))
        ss = group_steps(h, k, p2.shape[1])
        pn, mn, vn = update(p2, m2, v2, g2, h, ss)
        if selective:
            pn[~live], mn[~live], vn[~live] = p2[~live], m2[~live], v2[~live]
        P[k], M[k], V[k] = pn.reshape(shape), mn.reshape(shape), vn.reshape(shape)
    return P, M, V


def split_flat(flat, n, widths):
    """The five arrays [n, w] of a flat buffer in the initGrads layout."""
    out, o = [], 0
    for w in widths:
        out.append(np.asarray(flat[o:o + w * n]).reshape(n, w))
        o += w * n
    return out


def torch_adam(p0, grads, lr, betas, eps):
    """torch.optim.Adam (CPU, foreach=False) over a sequence of gradients, with the float-rounded scalars the C ABI sees.
    Returns (p, exp_avg, exp_avg_sq) as float32 arrays."""
    import torch
    p = torch.tensor(np.asarray(p0, np.float32))
    b = tuple(float(np.float32(x)) for x in betas)
    opt = torch.optim.Adam([p], lr=float(np.float32(lr)), betas=b, eps=float(np.float32(eps)), foreach=False)
    for g in grads:
        p.grad = torch.tensor(np.asarray(g, np.float32))
        opt.step()
    st = opt.state[p]
    return p.numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
