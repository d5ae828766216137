"""The evaluation metrics' yardstick (gs_image_metrics: PSNR, MAE, standard SSIM): two independent restatements and the cases the
kernels are pinned at.  CPU only; imports no GPU code.

restate()   torch: grouped conv2d with the 11 x 11 outer-product window and zero padding 5, in the dtype asked for
separable() NumPy float64: zero-padded planes, an 11-tap pass over rows then one over columns (another summation order)
finish()    the four sums -> (mse, mae, ssim, psnr)

Families and shapes are tests/loss_ref.py's, read only: the kernel's tile is the loss kernels' 64 x 16, so the shapes that can break
a tiled 11-tap stencil are the same (below the window, one pixel wide or high, W % 4 == 3, either side of a tile edge, exactly one
round of the XCDs, ragged ends).  Inputs are clipped to [0, 1] before either side sees them: the metrics assume a data range of 1
(`range` reaches 4.0 unclipped).
"""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

import loss_ref as LR

FAMILIES, SHAPES = LR.FAMILIES, LR.SHAPES
WIN, PAD = 11, 5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window(drop=None) -> np.ndarray:
    """g_i = exp(-(i - 5)^2 / (2 1.5^2)), normalised to sum 1 in float64; drop: a tap set to 0 first (a window that lost it)"""
    i = np.arange(WIN, dtype=np.float64)
    g = np.exp(-((i - PAD) ** 2) / (2.0 * 1.5 ** 2))
    if drop is not None:
        g[drop] = 0.0
    return g / g.sum()


def _ssim(mux, muy, sxx, syy, sxy):
    s2x, s2y, cxy = sxx - mux * mux, syy - muy * muy, sxy - mux * muy
    return (2 * mux * muy + C1) * (2 * cxy + C2) / ((mux * mux + muy * muy + C1) * (s2x + s2y + C2))


def ssim_map(img, gt, dtype=torch.float64, g=None) -> np.ndarray:
    """the map by grouped conv2d in `dtype` (the samples are converted first, so float32 is a plain single-precision evaluation)"""
    g = window() if g is None else g
    x, y = torch.tensor(np.asarray(img), dtype=dtype), torch.tensor(np.asarray(gt), dtype=dtype)
    Cn = x.shape[0]
    k4 = torch.as_tensor(np.outer(g, g)).to(dtype)[None, None].repeat(Cn, 1, 1, 1)
    conv = lambda t: torch.nn.functional.conv2d(t[None], k4, padding=PAD, groups=Cn)[0]
    return _ssim(conv(x), conv(y), conv(x * x), conv(y * y), conv(x * y)).numpy().copy()


def ssim_map_separable(img, gt, g=None) -> np.ndarray:
    """the map in NumPy float64: rows first, then columns, tap by tap"""
    g = window() if g is None else g
    x, y = np.asarray(img, np.float64), np.asarray(gt, np.float64)
    Cn, H, W = x.shape

    def blur(p):
        q = np.zeros((Cn, H + 2 * PAD, W + 2 * PAD))
        q[:, PAD:PAD + H, PAD:PAD + W] = p
        rows = np.zeros((Cn, H + 2 * PAD, W))
        for i in range(WIN):
            rows += g[i] * q[:, :, i:i + W]
        out = np.zeros((Cn, H, W))
        for j in range(WIN):
            out += g[j] * rows[:, j:j + H, :]
        return out
    return _ssim(blur(x), blur(y), blur(x * x), blur(y * y), blur(x * y))


def sums_of(img, gt, S, weight=None) -> np.ndarray:
    """the four float64 sums of gs_image_metrics from a map S: sum w d^2, sum w |d|, sum w S, sum w (w = 1 without a weight)"""
    x, y = np.asarray(img, np.float64), np.asarray(gt, np.float64)
    d = x - y
    w = np.ones(x.shape[1:]) if weight is None else np.asarray(weight, np.float64)
    wb = np.broadcast_to(w, x.shape)
    return np.array([(wb * d * d).sum(), (wb * np.abs(d)).sum(), (wb * np.asarray(S, np.float64)).sum(), wb.sum()], np.float64)


def restate(img, gt, weight=None, dtype=torch.float64):
    """(sums, map): the map in `dtype`, the sums from it in float64"""
    S = ssim_map(img, gt, dtype)
    return sums_of(img, gt, S, weight), S


Finished = namedtuple("Finished", "mse mae ssim psnr")


def finish(sums) -> Finished:
    s = np.asarray(sums, np.float64)
    if not s[3] > 0:
        return Finished(*(float("nan"),) * 4)
    mse = s[0] / s[3]
    return Finished(float(mse), float(s[1] / s[3]), float(s[2] / s[3]), float("inf") if mse == 0 else float(-10.0 * np.log10(mse)))


def images(name, shape):
    """the clipped float32 pair of one family at one shape (seeded as loss_ref.case seeds it)"""
    rng = np.random.default_rng(zlib.crc32(repr((name, shape)).encode()))
    img, gt = LR.family(name, *shape, rng)
    return (np.ascontiguousarray(np.clip(a, 0.0, 1.0), np.float32) for a in (img, gt))


Case = namedtuple("Case", "img gt S sums fin")


@functools.lru_cache(maxsize=None)
def case(name, shape) -> Case:
    """one cell of the matrix with its float64 reference: computed once per process, shared by the tests, never written to"""
    img, gt = images(name, shape)
    sums, S = restate(img, gt)
    for a in (img, gt, S, sums):
        a.setflags(write=False)
    return Case(img, gt, S, sums, finish(sums))
