"""fp64 torch restatements used ONLY to check the camera gradient (gs_backward_camera, camera.camera_param_grads) by autograd.

per_gaussian restates torch_ref.per_gaussian with the camera differentiable: T, P, fx, fy, eye, lookAt are float64 tensors, either one
copy shared by all gaussians (the end-to-end adjoint through torch_ref.composite) or one copy PER gaussian ([n, 4, 4], [n], [n, 3]), so
that autograd returns each gaussian's own contribution to the camera gradient.  The SH constants are the kernels': the float32 values of
csrc/gs_sh.h widened to float64 (torch_ref carries the float64 literals; the two differ by 3e-8 relative, which a 1e-9 bar would see).
transform / projection restate camera.compute_transform / compute_projection in float64 without the fp32 roundings.
"""
import numpy as np
import torch

import torch_ref
from common import scene_and_cameras
from gaussiansplat_amd import camera as gcam
from gaussiansplat_amd import synthetic

F64 = torch.float64
_f = lambda x: float(np.float32(x))
C1 = _f(torch_ref.C1)
C2 = [_f(c) for c in torch_ref.C2]
C3 = [_f(c) for c in torch_ref.C3]


def sh_basis(deg, x, y, z):
    b = [torch.full_like(x, _f(torch_ref.C0))]
    if deg >= 1:
        b += [-y * C1, z * C1, -x * C1]
    if deg >= 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b += [C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
    if deg >= 3:
        b += [C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
              C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)]
    return torch.stack(b, 1)


def camera_tensors(T, P, fx, fy, eye, lookAt, n=None):
    """The six camera inputs as float64 leaves that require grad: shared (n None) or n copies each."""
    T = torch.tensor(np.asarray(T, np.float64).reshape(4, 4, order="F"))
    P = torch.tensor(np.asarray(P, np.float64).reshape(4, 4, order="F"))
    out = [T, P, torch.tensor(float(fx), dtype=F64), torch.tensor(float(fy), dtype=F64),
           torch.tensor(np.asarray(eye, np.float64)), torch.tensor(np.asarray(lookAt, np.float64))]
    if n is not None:
        out = [t.expand(n, *t.shape).clone() for t in out]
    return [t.requires_grad_(True) for t in out]


def per_gaussian(means, scales, quats, opac, shs, deg, cam, W, H):
    """torch_ref.per_gaussian with cam = [T, P, fx, fy, eye, lookAt] tensors (camera_tensors), shared or per gaussian."""
    T, P, fx, fy, eye, lookAt = cam
    n = means.shape[0]
    if T.dim() == 2:
        T, P, fx, fy, eye, lookAt = (t.expand(n, *t.shape) for t in (T, P, fx, fy, eye, lookAt))
    mh = torch.cat([means, torch.ones(n, 1, dtype=F64)], 1)
    t = torch.einsum("nij,nj->ni", T, mh)
    p = torch.einsum("nij,nj->ni", P, t)
    mux = (W * p[:, 0] / p[:, 3] + 1) / 2 + W / 2
    muy = (H * p[:, 1] / p[:, 3] + 1) / 2 + H / 2
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    z0 = torch.zeros_like(tx)
    J = torch.stack([torch.stack([fx / tz, z0, -fx * tx / tz ** 2], 1), torch.stack([z0, fy / tz, -fy * ty / tz ** 2], 1)], 1)
    w, x, y, z = quats[:, 0], quats[:, 1], quats[:, 2], quats[:, 3]
    R = torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x - z * z), 2 * (y * z - w * x)], 1),      # projection.jl:8 quirk
        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    Wm = R * torch.exp(scales)[:, None, :]
    Sg = Wm @ Wm.transpose(1, 2)
    A = J @ R
    cov = A @ Sg @ A.transpose(1, 2) + 0.3
    M = torch.linalg.inv(cov)
    sig = torch.sigmoid(opac.reshape(-1))
    v = p[:, :3] - (lookAt - eye)
    d = v / v.norm(dim=1, keepdim=True)
    B = sh_basis(deg, d[:, 0], d[:, 1], d[:, 2])
    rgb = torch.einsum("nk,nkc->nc", B, shs.reshape(n, -1, 3)) + 0.5
    return mux, muy, M, sig, rgb


def _grad(L, leaves):
    """autograd of L in the leaves; a leaf L does not depend on (eye and lookAt at degree 0) gets zeros"""
    g = torch.autograd.grad(L, leaves, allow_unused=True)
    return [torch.zeros_like(t) if x is None else x for x, t in zip(g, leaves)]


def flat40(grads):
    """[d_T, d_P, d_fx, d_fy, d_eye, d_lookAt] (autograd's, per gaussian [n, ...] or shared) -> [n, 40] or [40] in the ABI's order."""
    gT, gP, gfx, gfy, geye, glook = (g.detach().numpy() for g in grads)
    if gT.ndim == 2:
        return np.concatenate([gT.reshape(-1, order="F"), gP.reshape(-1, order="F"), geye, glook, [gfx], [gfy]])
    n = gT.shape[0]
    return np.concatenate([gT.transpose(0, 2, 1).reshape(n, 16), gP.transpose(0, 2, 1).reshape(n, 16), geye, glook, gfx[:, None], gfy[:, None]], 1)


def params64(sc, n_sh=None):
    """The model as float64 tensors (no grad); n_sh: keep the first n_sh SH coefficients (an active degree below the stored one)."""
    shs = np.asarray(sc["shs"], np.float64)
    if n_sh is not None:
        shs = shs[:, :n_sh]
    return [torch.tensor(np.asarray(sc[k], np.float64)) for k in ("means", "scales", "quats", "opacities")] + [torch.tensor(shs)]


def rows_scalar_grads(sc, deg, T, P, fx, fy, eye, lookAt, W, H, rows):
    """Per-gaussian camera gradients [n, 40] of  sum_g (row_g converted by gs_g2d_to_grads in float64) . (rgb, sig, mux, muy, M)_g,
    rows [n, 10] the RAW rows (d rgb | S0 Sx Sy Sxx Sxy - Syy).  deg: the active degree (the first (deg + 1)^2 coefficients are used)."""
    n = rows.shape[0]
    par = params64(sc, (deg + 1) ** 2)
    cam = camera_tensors(T, P, fx, fy, eye, lookAt, n)
    mux, muy, M, sig, rgb = per_gaussian(*par, deg, cam, W, H)
    r = torch.tensor(np.asarray(rows, np.float64))
    Md, sd = M.detach(), sig.detach()
    i0, mc, i3 = Md[:, 0, 0], 0.5 * (Md[:, 0, 1] + Md[:, 1, 0]), Md[:, 1, 1]
    S0, Sx, Sy, Sxx, Sxy, Syy = r[:, 3], r[:, 4], r[:, 5], r[:, 6], r[:, 7], r[:, 9]
    dsig = torch.where(sd > 0, -S0 / sd, torch.zeros_like(S0))
    dmx, dmy = -(i0 * Sx + mc * Sy), -(mc * Sx + i3 * Sy)
    L = (r[:, :3] * rgb).sum() + (dsig * sig).sum() + (dmx * mux).sum() + (dmy * muy).sum() + \
        (0.5 * Sxx * M[:, 0, 0] + 0.5 * Sxy * M[:, 0, 1] + 0.5 * Sxy * M[:, 1, 0] + 0.5 * Syy * M[:, 1, 1]).sum()
    return flat40(_grad(L, cam))


# ---------------------------------------------------------------- the chain to Camera fields

def _unit(v):
    return v / torch.sqrt((v * v).sum())


def transform(eye, lookAt, up):
    """camera.compute_transform in float64 torch: [4, 4], rows u, v, w, fourth column -axis . eye, fourth row zero."""
    w = _unit(lookAt - eye)
    u = _unit(torch.linalg.cross(up, w))
    v = torch.linalg.cross(w, u)
    rows = [torch.cat([a, -(a * eye).sum().reshape(1)]) for a in (u, v, w)]
    return torch.stack(rows + [torch.zeros(4, dtype=F64)])


def projection(fx, fy, near, far, W, H):
    """camera.compute_projection in float64 torch."""
    P = torch.zeros(4, 4, dtype=F64)
    P[0, 0] = 2.0 * fx / W
    P[1, 1] = 2.0 * fy / H
    P[2, 2] = (far + near) / (far - near)
    P[2, 3] = -2.0 * (far * near) / (far - near)
    P[3, 2] = 1.0
    return P


def param_grads_autograd(cam, W, H, raw40):
    """d / d (eye, lookAt, up, fx, fy) of  raw . (T(eye, lookAt, up), P(fx, fy), eye, lookAt, fx, fy)  by autograd, float64."""
    g = np.asarray(raw40, np.float64)
    eye, look, up = (torch.tensor(np.asarray(a, np.float32).astype(np.float64), requires_grad=True) for a in (cam.eye, cam.lookAt, cam.up))
    fx = torch.tensor(float(cam.fx), dtype=F64, requires_grad=True)
    fy = torch.tensor(float(cam.fy), dtype=F64, requires_grad=True)
    T = transform(eye, look, up)
    P = projection(fx, fy, float(np.float32(cam.near)), float(np.float32(cam.far)), W, H)
    L = (T * torch.tensor(g[0:16].reshape(4, 4, order="F"))).sum() + (P * torch.tensor(g[16:32].reshape(4, 4, order="F"))).sum() + \
        (eye * torch.tensor(g[32:35])).sum() + (look * torch.tensor(g[35:38])).sum() + fx * g[38] + fy * g[39]
    ge, gl, gu, gfx, gfy = torch.autograd.grad(L, [eye, look, up, fx, fy])
    return dict(eye=ge.numpy(), lookAt=gl.numpy(), up=gu.numpy(), fx=float(gfx), fy=float(gfy))


# ---------------------------------------------------------------- the end-to-end case (tests/test_gpu_camera_grad.py test 2 and its teeth check)

E2E = dict(n=400, W=64, H=48, deg=2, seed=91, shift=0.02)


def shifted_camera(cam, frac):
    """cam with the eye moved by frac x its distance to lookAt, along a fixed direction off the view axis."""
    import dataclasses
    e, l = np.asarray(cam.eye, np.float64), np.asarray(cam.lookAt, np.float64)
    d = np.array([0.6, -0.64, 0.48])                    # unit length
    return dataclasses.replace(cam, eye=(e + frac * np.linalg.norm(l - e) * d).astype(np.float32))


def e2e_setup(oracle, shift=None):
    """Scene, camera, the oracle's discrete decisions (lists, boxes, clip depths) and the oracle's renders at the true and the shifted eye."""
    c = E2E
    sc, cam, T, P, ocam = scene_and_cameras(c["n"], c["W"], c["H"], c["deg"], c["seed"])
    args = (sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], c["deg"])
    ref = oracle.render(*args, ocam, order=1, t_min=0.0)
    cam2 = shifted_camera(cam, c["shift"] if shift is None else shift)
    T2, P2 = gcam.compute_transform(cam2), gcam.compute_projection(cam2, c["W"], c["H"])
    ocam2 = oracle.camera_from_arrays(T2, P2, np.float32(cam2.fx), np.float32(cam2.fy), np.float32(cam2.near), np.float32(cam2.far),
                                      cam2.eye, cam2.lookAt, c["W"], c["H"])
    ref2 = oracle.render(*args, ocam2, order=1, t_min=0.0)
    return dict(sc=sc, cam=cam, T=T, P=P, ocam=ocam, ref=ref, cam2=cam2, T2=T2, P2=P2, target_oracle=ref2["image"], **c)


def e2e_contributions(s, dC):
    """[n, 40] per-gaussian contributions to the camera gradient of  sum image . dC  through the fp64 restatement (one camera copy per
    gaussian, torch_ref.composite on the oracle's lists); their sum over n is the adjoint."""
    cam, ref, n = s["cam"], s["ref"], s["n"]
    par = params64(s["sc"])
    ct = camera_tensors(s["T"], s["P"], _f(cam.fx), _f(cam.fy), cam.eye, cam.lookAt, n)
    mux, muy, M, sig, rgb = per_gaussian(*par, s["deg"], ct, s["W"], s["H"])
    img, _ = torch_ref.composite(mux, muy, M, sig, rgb, _f(cam.near), _f(cam.far), s["W"], s["H"], ref["ranges"], ref["ids"],
                                 ref["pre"]["bbs"], ref["pre"]["tps"][:, 2], t_min=0.0)
    L = (img * torch.tensor(np.asarray(dC, np.float64))).sum()
    return flat40(_grad(L, ct))


def mse_dC(image, target):
    image, target = np.asarray(image, np.float64), np.asarray(target, np.float64)
    return (2.0 * (image - target) / image.size).astype(np.float32)
