"""The loss kernels' yardstick: src/loss.jl restated with torch autograd in float64 (the reference) and in float32 (what a plain
single-precision evaluation of the same formula can do), the image families the kernels are pinned at, and the bars derived from
the two.  CPU only; imports no GPU code.

A kernel is compared with the float64 restatement and is allowed FACTOR x the float32 restatement's own error on the same input
(gradient max, gradient L2, loss, and the L2 of every border strip): the kernel is another float32 evaluation of the same formula
with a different summation order (36 folded weights, fma, one reciprocal for two divisions), so its error is of the same order, on
either side.  The factor is not fitted to the kernel (RAISED lists the parts where it had to be raised, and why);
tests/test_loss.py caps the bars themselves, so that a lost window tap cannot hide under them.
"""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

from oracle import loss_oracle_np as LO

SHARP = ("uniform", "black", "range", "checker", "impulse")          # float32 is within ~1e-5 of float64
CANCELLING = ("smooth_near", "flat_noise", "two_consts", "step")     # s_xx - mu^2 cancels against C2 = 9e-4; 1e-4 .. 2e-3
FAMILIES = SHARP + CANCELLING
LAMS = (0.1, 0.2, 1.0)
# (C, H, W): below the 11 x 11 window, one pixel wide or high, W % 4 == 3, one pixel either side of the 64 x 16 tile,
# exactly 8 tiles (one full round of the XCDs), several tiles with a ragged end
SHAPES = ((3, 1, 1), (3, 2, 3), (1, 10, 10), (3, 11, 11), (2, 40, 5), (2, 5, 40), (3, 15, 63), (1, 16, 64), (3, 17, 65),
          (5, 16, 67), (1, 64, 128), (2, 33, 129), (3, 49, 193))
FACTOR = 4.0
CAP_SHARP, CAP_CANCELLING = 5e-5, 2e-2                               # on FACTOR * e_max and FACTOR * e_l2 (tests/test_loss.py)
# Where a kernel that was read and found correct needs more than FACTOR, the factor is raised for that family, and only for the part
# named here, with the reason beside it -- never past 16, never replaced by a tolerance taken from the kernel's output.
#   "tiny": the gradient of images of at most 6 pixels per plane (3x1x1, 3x2x3).  Three to eighteen numbers, each a handful of
#           roundings through the same cancellation (c0 + 2x c1 + y c2), so the ratio is one rounding draw over another, not an
#           error level: in ulps of the largest element, restatement against kernel, range 0.12 : 1.4 (ratio 12.1), step
#           0.4 : 2.7 (11.0), smooth_near 1.2 : 4.8 (4.3), two_consts 5 : 21 (4.2), flat_noise 770 : 2900 (4.1, deep in the
#           cancellation).  Every larger shape of these families stays below 2.
#   "loss": impulse only.  The map is exactly 1 away from the four impulses, so the restatement's mean is a sum of ones, exact in
#           float32, with a few fractions added (e_loss 5e-10 on a loss of 0.03); the kernel adds a thread's four pixels, then the
#           wave, then the workgroup in float32 before the double atomics, and the fractions round against partial sums of
#           hundreds: 5e-9, a ratio of 10.1 (5x16x67, lam = 1).  A finding about the kernel's summation order.
RAISED = {("range", "tiny"): 16.0, ("step", "tiny"): 16.0, ("smooth_near", "tiny"): 16.0, ("flat_noise", "tiny"): 16.0,
          ("two_consts", "tiny"): 16.0, ("impulse", "loss"): 16.0}


def factor(name, shape, key):
    """the factor of one of ratios()'s keys for a family at a shape"""
    part = "loss" if key == "loss" else ("tiny" if shape[1] * shape[2] <= 6 else None)
    return RAISED.get((name, part), FACTOR)


def restate(img, gt, lam, dtype):
    """(loss, grad, ssim_map) of loss.jl:41-72 in `dtype`: grouped conv2d with zero padding 5, the gradient by autograd."""
    x = torch.tensor(np.asarray(img), dtype=dtype, requires_grad=True)
    y = torch.tensor(np.asarray(gt), dtype=dtype)
    Cn = x.shape[0]
    k4 = torch.as_tensor(LO.kernel_window()).to(dtype)[None, None].repeat(Cn, 1, 1, 1)
    conv = lambda t: torch.nn.functional.conv2d(t[None], k4, padding=5, groups=Cn)[0]
    mux, muy = conv(x), conv(y)
    s2x, s2y, sxy = conv(x * x) - mux * mux, conv(y * y) - muy * muy, conv(x * y) - mux * muy
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    S = (2 * mux * muy + c1) / (mux ** 2 + muy ** 2 + c1) * (2 * sxy + c2) / (s2x + s2y + c2)
    loss = (1 - lam) * (x - y).abs().sum() / (2.0 * x.numel()) + lam * (1 - S.mean()) / 2.0
    loss.backward()
    return float(loss.detach()), x.grad.numpy().copy(), S.detach().numpy().copy()


def _tie_blocks(img, gt):
    """exact ties, img == gt: one block in the first tile, one in the ragged corner (sign(0) = 0)"""
    img[0, :3, :5] = gt[0, :3, :5]
    img[-1, -7:, -9:] = gt[-1, -7:, -9:]


def family(name, C, H, W, rng):
    """contiguous float32 [C, H, W] pair (img, gt) of one family"""
    f32 = np.float32
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    shape = (C, H, W)
    if name == "uniform":
        img, gt = rng.random(shape, dtype=f32), rng.random(shape, dtype=f32)
    elif name == "black":
        img, gt = f32(1e-4) * rng.random(shape, dtype=f32), np.zeros(shape, f32)
    elif name == "range":                                            # a frame over a background or an unclamped render leaves [0, 1]
        img, gt = (f32(-0.5) + f32(4.5) * rng.random(shape, dtype=f32) for _ in range(2))
    elif name == "checker":                                          # period 1 against its dimmed inverse
        b = ((xx + yy) % 2).astype(f32)
        img, gt = np.broadcast_to(b, shape).copy(), np.broadcast_to(f32(0.6) * (1 - b), shape).copy()
    elif name == "impulse":                                          # every tap of the window shows up separately in dC
        img, gt = np.zeros(shape, f32), np.zeros(shape, f32)
        for py, px in ((0, 0), (H - 1, W - 1), (15, 63), (16, 64)):  # the corners, and either side of the first tile's corner
            img[:, min(py, H - 1), min(px, W - 1)] = 1.0
    elif name == "smooth_near":                                      # late training: a render 0.2 % from a smooth target
        ph = rng.random((C, 1, 1)) * 2 * np.pi
        gt = (0.5 + 0.4 * np.sin(2 * np.pi * xx / 37.0 + ph) * np.cos(2 * np.pi * yy / 23.0)).astype(f32)
        img = np.clip(gt + f32(0.002) * rng.standard_normal(shape).astype(f32), 0.0, 1.0).astype(f32)
    elif name == "flat_noise":
        gt = np.full(shape, 0.9, f32)
        img = (gt + f32(1e-3) * rng.standard_normal(shape).astype(f32)).astype(f32)
    elif name == "two_consts":
        img, gt = np.full(shape, 0.7, f32), np.full(shape, 0.6, f32)
    elif name == "step":                                             # on the tile boundary and one column past it (clamped into the image)
        xi = min(64, W - 1)
        img = np.broadcast_to(np.where(xx >= xi, 0.8, 0.2).astype(f32), shape).copy()
        gt = np.broadcast_to(np.where(xx >= xi + 1, 0.8, 0.2).astype(f32), shape).copy()
    else:
        raise ValueError(name)
    if name not in ("two_consts", "impulse"):
        _tie_blocks(img, gt)
    return np.ascontiguousarray(img, f32), np.ascontiguousarray(gt, f32)


def strips(H, W):
    """the borders see a truncated window, the columns round x = 64 two tiles: the outer 6 rows and columns, and the 6 columns
    either side of x = 64 where the image has them"""
    s = [np.s_[:, :6, :], np.s_[:, -6:, :], np.s_[:, :, :6], np.s_[:, :, -6:]]
    if W > 58:
        s.append(np.s_[:, :, 58:64])
    if W > 64:
        s.append(np.s_[:, :, 64:70])
    return s


Bars = namedtuple("Bars", "e_max e_l2 e_loss loss grad abs_max abs_l2 abs_strips")


def bars(img, gt, lam):
    """Both restatements of one input.  e_max = max|g32 - g64| / max|g64|, e_l2 = |g32 - g64| / |g64|,
    e_loss = max(|loss32 - loss64|, lam/2 mean|S32 - S64| + (1 - lam)/2 2^-23 mean|img - gt|): the mean absolute error of the map
    bounds what the mean of such pixels can be off by, so a lucky cancellation in loss32 cannot make the bar vanish.
    Also the float64 loss and gradient, and the float32 gradient's absolute errors (whole image and per strip of strips())."""
    l64, g64, s64 = restate(img, gt, lam, torch.float64)
    l32, g32, s32 = restate(img, gt, lam, torch.float32)
    d = g32.astype(np.float64) - g64
    amax, al2 = float(np.abs(d).max()), float(np.linalg.norm(d))
    diff = np.abs(np.asarray(img, np.float64) - np.asarray(gt, np.float64)).mean()
    e_loss = max(abs(l32 - l64), lam / 2 * float(np.abs(s32.astype(np.float64) - s64).mean()) + (1 - lam) / 2 * 2.0 ** -23 * float(diff))
    H, W = g64.shape[1:]
    # a strip is allowed its own float32 error, and no less than the image's float32 error per element over the strip's elements:
    # where the gradient vanishes (the flat sides of `step`, img == gt) the restatement's terms cancel to exactly 0 and a strip's own
    # error says nothing about what float32 can do there
    return Bars(amax / float(np.abs(g64).max()), al2 / float(np.linalg.norm(g64)), e_loss, l64, g64, amax, al2,
                tuple(max(float(np.linalg.norm(d[sl])), al2 * float(np.sqrt(d[sl].size / d.size))) for sl in strips(H, W)))


def ratios(dC, loss, b):
    """A kernel's errors against the float64 restatement over the float32 restatement's own (Bars b): <= factor() passes.
    0 / 0 counts as 0, x / 0 as inf."""
    over = lambda err, e: 0.0 if err == 0.0 else (float("inf") if e == 0.0 else err / e)
    d = np.asarray(dC, np.float64) - b.grad
    H, W = b.grad.shape[1:]
    return dict(max=over(float(np.abs(d).max()), b.abs_max), l2=over(float(np.linalg.norm(d)), b.abs_l2),
                loss=over(abs(loss - b.loss), b.e_loss),
                strips=max(over(float(np.linalg.norm(d[sl])), e) for sl, e in zip(strips(H, W), b.abs_strips)))


@functools.lru_cache(maxsize=None)
def case(name, shape, lam):
    """(img, gt, Bars) of one cell of the matrix: computed once per process, shared by the tests that need it, never written to"""
    rng = np.random.default_rng(zlib.crc32(repr((name, shape)).encode()))
    img, gt = family(name, *shape, rng)
    b = bars(img, gt, lam)
    for a in (img, gt, b.grad):
        a.setflags(write=False)
    return img, gt, b
