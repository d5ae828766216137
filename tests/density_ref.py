"""NumPy float32 restatement of the density-control semantics of include/gsplat.h (gs_density_accumulate / _decide / _plan /
_restructure, gs_opacity_reset): every operation rounded on its own, in the order the header writes it, so the device results can be
compared bit for bit.  exp is the numeric spec's (oracle.gs_oracle_np.expf_spec, the preprocess's gs_expf)."""
import numpy as np

from oracle.gs_oracle_np import expf_spec

f32 = np.float32
LOG_SHRINK_3DGS = f32(np.log(1.6))


def visibility(bbs, tps, rgb, sig, mu, invcov, near, far):
    """(visible [n] bool, extent [n] int32) of one view from the export_debug arrays: the pixel box the preprocess packs into the
    payload row is non-empty exactly for a finite box (GS_ARR_BBS: xmin ymin xmax ymax), a clip-space depth inside [near, far]
    (GS_ARR_TPS[:, 2]; a NaN depth passes, as in the kernel) and a finite payload (colour, sigmoid, mu', conic); the box is
    clamped to int16 on its way into the row."""
    bbs = np.asarray(bbs, f32)
    finite_bb = np.isfinite(bbs).all(axis=1)
    z = np.asarray(tps, f32)[:, 2]
    with np.errstate(invalid="ignore"):
        depth_ok = ~((z < f32(near)) | (z > f32(far)))
    pay_ok = (np.isfinite(np.asarray(rgb, f32)).all(axis=1) & np.isfinite(np.asarray(sig, f32)) & np.isfinite(np.asarray(mu, f32)).all(axis=1) &
              np.isfinite(np.asarray(invcov, f32)).all(axis=1))
    ok = finite_bb & depth_ok & pay_ok
    box = np.where(ok[:, None], np.clip(np.nan_to_num(bbs, nan=0.0, posinf=0.0, neginf=0.0), -32768.0, 32767.0), 0.0).astype(np.int32)
    xmin, ymin, xmax, ymax = box[:, 0], box[:, 1], box[:, 2], box[:, 3]
    visible = ok & (xmax >= xmin) & (ymax >= ymin)
    extent = np.where(visible, np.maximum(xmax - xmin, ymax - ymin) + 1, 0).astype(np.int32)
    return visible, extent


def accumulate(grad_sum, count, max_extent, grad2d, W, H, visible, extent):
    """One gs_density_accumulate: grad2d is the view's GS_ARR_GRAD2D read-back [n, 10] (d L / d mu' in pixels at columns 4, 5)."""
    g = np.asarray(grad2d, f32)
    with np.errstate(all="ignore"):
        a = (f32(0.5) * f32(W)) * g[:, 4]
        b = (f32(0.5) * f32(H)) * g[:, 5]
        s = a * a + b * b
        r = np.sqrt(s)
        out = np.asarray(grad_sum, f32) + r
    return (out.astype(f32), (np.asarray(count, np.int32) + visible.astype(np.int32)).astype(np.int32),
            np.maximum(np.asarray(max_extent, np.int32), extent).astype(np.int32))


def decide(scales, opac, grad_sum, count, max_extent, grad_threshold, log_split_scale, log_shrink, min_opacity_logit, log_max_world_scale,
           max_extent_px):
    """action [n] int32: 0 keep, 1 clone, 2 split, 3 prune.  A NaN compares false everywhere (np.max propagates a NaN scale)."""
    scales = np.asarray(scales, f32).reshape(-1, 3)
    n = len(scales)
    opac = np.asarray(opac, f32).reshape(-1)
    cnt = np.asarray(count, np.int32)
    with np.errstate(invalid="ignore"):
        smax = np.max(scales, axis=1) if n else np.zeros(0, f32)
        dens = (cnt > 0) & (np.asarray(grad_sum, f32) >= f32(grad_threshold) * cnt.astype(f32))
        split = dens & (smax > f32(log_split_scale))
        remain = np.where(split, smax - f32(log_shrink), smax).astype(f32)
        prune = (opac < f32(min_opacity_logit)) | ((int(max_extent_px) > 0) & (np.asarray(max_extent, np.int32) > int(max_extent_px))) | \
                (remain > f32(log_max_world_scale))
    return np.where(prune, 3, np.where(split, 2, np.where(dens, 1, 0))).astype(np.int32)


def counts(action):
    """{survivors, clones, splits, pruned} of gs_density_plan."""
    a = np.asarray(action)
    return int(((a == 0) | (a == 1)).sum()), int((a == 1).sum()), int((a == 2).sum()), int((a == 3).sum())


def n_out(c):
    return c[0] + c[1] + 2 * c[2]


def quat_to_rot(q):
    """The nine expressions of the preprocess (the reference's quatToRot with its sign, raw quaternion) -> R[n, 3, 3]."""
    q = np.asarray(q, f32)
    qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = f32(1.0), f32(2.0)
    R = np.empty((len(q), 3, 3), f32)
    R[:, 0, 0] = one - two * (qy * qy + qz * qz)
    R[:, 1, 0] = two * (qx * qy + qw * qz)
    R[:, 2, 0] = two * (qx * qz - qw * qy)
    R[:, 0, 1] = two * (qx * qy - qw * qz)
    R[:, 1, 1] = one - two * (qx * qx - qz * qz)
    R[:, 2, 1] = two * (qy * qz + qw * qx)
    R[:, 0, 2] = two * (qx * qz + qw * qy)
    R[:, 1, 2] = two * (qy * qz - qw * qx)
    R[:, 2, 2] = one - two * (qx * qx + qy * qy)
    return R


def restructure(model, action, noise, log_shrink=LOG_SHRINK_3DGS, sets=()):
    """model: (means [n,3], scales [n,3], quats [n,4], opacities [n,1], shs [n,3K]); noise [n,2,3] (read for split sources only);
    sets: gradient-shaped companions, each a list of five [n, w] arrays or None.  Returns (new model, new sets): survivors in ascending
    source order, then the clones, then child 0 and child 1 of every split source."""
    a = np.asarray(action)
    means, scales, quats, opac, shs = [np.asarray(x, f32) for x in model]
    assert all(x.ndim == 2 and x.shape[0] == len(a) for x in (means, scales, quats, opac, shs)), "five [n, w] arrays"
    surv, cl, sp = np.flatnonzero((a == 0) | (a == 1)), np.flatnonzero(a == 1), np.flatnonzero(a == 2)
    with np.errstate(all="ignore"):
        e = expf_spec(scales[sp])[:, None, :] * np.asarray(noise, f32).reshape(len(a), 2, 3)[sp] if len(sp) else np.zeros((0, 2, 3), f32)
        R = quat_to_rot(quats[sp])
        w = np.empty((len(sp), 2, 3), f32)
        for i in range(3):
            w[:, :, i] = (R[:, None, i, 0] * e[:, :, 0] + R[:, None, i, 1] * e[:, :, 1]) + R[:, None, i, 2] * e[:, :, 2]
        c_means = (means[sp][:, None, :] + w).reshape(-1, 3).astype(f32)
        c_scales = np.repeat((scales[sp] - f32(log_shrink)).astype(f32), 2, axis=0)
    twice = lambda x: np.repeat(x[sp], 2, axis=0)
    new = [np.concatenate([means[surv], means[cl], c_means]), np.concatenate([scales[surv], scales[cl], c_scales]),
           np.concatenate([quats[surv], quats[cl], twice(quats)]), np.concatenate([opac[surv], opac[cl], twice(opac)]),
           np.concatenate([shs[surv], shs[cl], twice(shs)])]
    fresh = len(cl) + 2 * len(sp)
    new_sets = []
    for s in sets:
        new_sets.append([None if x is None else np.concatenate([np.asarray(x, f32)[surv], np.zeros((fresh, m.shape[1]), f32)])
                         for x, m in zip(s, new)])
    return new, new_sets


def opacity_reset(opac, max_logit, m=None, v=None):
    """o > max_logit ? max_logit : o (a NaN stays); +0 into the moment arrays that are given."""
    o = np.asarray(opac, f32)
    with np.errstate(invalid="ignore"):
        out = np.where(o > f32(max_logit), f32(max_logit), o).astype(f32)
    return out, (None if m is None else np.zeros_like(np.asarray(m, f32))), (None if v is None else np.zeros_like(np.asarray(v, f32)))
