"""Evaluation metrics on the device: PSNR, MAE and the standard SSIM of rendered views against their targets.

    m = image_metrics(renderer, img, gt)                       # Metrics(mse, mae, ssim, psnr, ssim_map)
    res = evaluate(renderer, cameras, targets)                 # EvalResult(per_view=[Metrics, ...], mean=Metrics)

The numbers come from gs_image_metrics (csrc/gs_metrics.hip): the float32 images are widened to double and the window sums, the SSIM
formula and the differences are evaluated in double, the sums added in a fixed order without atomics -- bitwise reproducible, and
not the training loss's `exp(-r)` window but the Gaussian window (11 taps, sigma 1.5, zero padding) of 3DGS's `ssim()`.  The data
range is 1: PSNR = -10 log10(mse).  There is no CPU path.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import backend as B
from . import renderer as R

Metrics = namedtuple("Metrics", "mse mae ssim psnr ssim_map")
EvalResult = namedtuple("EvalResult", "per_view mean")


def _finish(sums, ssim_map=None) -> Metrics:
    o = B.metrics_finish(sums)
    return Metrics(float(o[B.METRIC_MSE]), float(o[B.METRIC_MAE]), float(o[B.METRIC_SSIM]), float(o[B.METRIC_PSNR]), ssim_map)


def _metrics_into(renderer, img, gt, weight, sums_row, smap=None):
    """gs_image_metrics with device pointers on the renderer's stream: the four sums into `sums_row` (a float64 device tensor).  No sync."""
    Cn, H, W = img.shape
    renderer._begin().image_metrics_device(img.data_ptr(), gt.data_ptr(), weight.data_ptr() if weight is not None else 0, W, H, Cn,
                                           smap.data_ptr() if smap is not None else 0, sums_row.data_ptr())


def image_metrics(renderer_or_ctx, img, gt, weight=None, want_map: bool = False) -> Metrics:
    """Metrics of img against gt, [C, H, W] float32 each (torch or numpy); weight: [H, W], shared by the channels, or None.
    With a renderer the inputs are moved to its device (as train.LossFunction does) and the call runs on its stream; with a bare
    backend.Context the inputs are host arrays staged through the context.  ssim_map (want_map): the map, float32, of the whole
    unweighted images -- a tensor on the renderer's device, or a numpy array.  All four values are NaN when the weights sum to 0."""
    if isinstance(renderer_or_ctx, B.Context):
        as_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else a
        sums, smap = renderer_or_ctx.image_metrics_host(as_np(img), as_np(gt), None if weight is None else as_np(weight), want_map)
        return _finish(sums, smap)
    import torch
    r = renderer_or_ctx
    dev = r.imageData.device
    img = R.as_device_tensor(img, dev, None, "img")
    if img.ndim != 3:
        raise ValueError("image_metrics: img must be a [C, H, W] image")
    gt = R.as_device_tensor(gt, dev, img.shape, "gt")
    w = None if weight is None else R.as_device_tensor(weight, dev, img.shape[1:], "weight")
    sums = torch.empty(B.GS_METRIC_SUMS, dtype=torch.float64, device=dev)
    smap = torch.empty_like(img) if want_map else None
    _metrics_into(r, img, gt, w, sums, smap)
    return _finish(sums.cpu().numpy(), smap)                                # (the read-back waits for the stream)


def evaluate(renderer, cameras, targets, weights=None, background=None) -> EvalResult:
    """Render every view (preprocess -> compactIdxs -> forward) and compare it with its target: per-view Metrics and their arithmetic
    mean (as 3DGS's metrics.py reports PSNR: the mean of the per-view values).  cameras: one Camera per target, or None for the 2-D
    renderer (or a list of None: the renderer's current view).  targets: [3, H, W], or [4, H, W] with straight alpha, which is
    composited over the evaluation background (gs_compose_target).  weights: None, or one [H, W] array or None per view.
    background: the colour to evaluate over; None: the renderer's current one.  The sums of all views land in one [V, 4] float64
    device tensor that is read back once.  renderer.camera, the background and the active SH degree are left as found; the frame is
    the last evaluated view's (render again before a backward)."""
    import torch
    targets = list(targets)
    V = len(targets)
    cameras = [None] * V if cameras is None else list(cameras)
    weights = [None] * V if weights is None else list(weights)
    if len(cameras) != V or len(weights) != V:
        raise ValueError(f"evaluate: {V} targets, {len(cameras)} cameras, {len(weights)} weights: one of each per view")
    dev = renderer.imageData.device
    H, W = renderer.transmittance.shape
    saved_camera, saved_bg = renderer.camera, renderer.background
    sums = torch.empty((max(V, 1), B.GS_METRIC_SUMS), dtype=torch.float64, device=dev)
    keep = []                                                               # what the enqueued calls read, until the read-back
    try:
        if background is not None:
            renderer.background = background
        for v in range(V):
            R.renderFrame(renderer, cameras[v])
            gt = R.as_device_tensor(targets[v], dev, None, "target")
            if gt.ndim != 3 or gt.shape[0] not in (3, 4) or tuple(gt.shape[1:]) != (H, W):
                raise ValueError(f"evaluate: target {v} must be [3, {H}, {W}] or [4, {H}, {W}], not {tuple(gt.shape)}")
            if gt.shape[0] == 4:
                rgb = torch.empty((3, H, W), dtype=torch.float32, device=dev)
                renderer._begin().compose_target(gt.data_ptr(), W, H, rgb.data_ptr())
                keep.append(gt)
                gt = rgb
            w = None if weights[v] is None else R.as_device_tensor(weights[v], dev, (H, W), "weight")
            _metrics_into(renderer, renderer.imageData, gt, w, sums[v])
            keep += [gt, w]
        host = sums.cpu().numpy()                                           # the one read-back
    finally:
        if background is not None and tuple(renderer.background) != tuple(saved_bg):
            renderer.background = saved_bg
        if saved_camera is not None and renderer.camera is not saved_camera:
            renderer._set_view(saved_camera)                                # the ctx's camera and view slot as well
        renderer.camera = saved_camera
    per_view = [_finish(host[v]) for v in range(V)]
    mean = Metrics(*(float(np.mean([getattr(m, k) for m in per_view])) if V else float("nan") for k in ("mse", "mae", "ssim", "psnr")), None)
    return EvalResult(per_view, mean)
