#!/usr/bin/env python3
"""What gs_image_metrics costs beside the training loss it sits next to (GPU box).

    python3 tools/metrics_time.py [--size 1920x1080x3] [--reps 30] [--batch 20] [--out profiles/metrics_time.json]

One process, device-resident inputs (a smooth target and a render 2 % from it, clipped to [0, 1]).  After a warm-up of every variant,
in each of `reps` repetitions the variants run in turn, each as `batch` back-to-back calls between two device events on the ctx's
stream; a call's time is the batch's over `batch`.  Variants:
  loss           gs_loss_l1_dssim(GS_MEM_DEVICE), dC written, the loss not read back: the yardstick (two kernels and a memset)
  metrics        gs_image_metrics(GS_MEM_DEVICE), no weight, no map (two kernels)
  metrics_map    ... with the float32 SSIM map written
  metrics_weight ... with a per-pixel weight and the map
Median, min and max per call; ratio = metrics median over loss median.  The sums of the first and the last metrics call are compared
bit for bit, and with the float64 NumPy restatement kept here (separable, another summation order) where --check is given."""
import argparse
import statistics

from _timing import emit, event_ms, interleaved, stat


def inputs(Cn, H, W, seed=7):
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ph = rng.random((Cn, 1, 1)) * 2 * np.pi
    gt = (0.5 + 0.4 * np.sin(2 * np.pi * xx / 37.0 + ph) * np.cos(2 * np.pi * yy / 23.0)).astype(np.float32)
    img = np.clip(gt + np.float32(0.02) * rng.standard_normal((Cn, H, W)).astype(np.float32), 0.0, 1.0).astype(np.float32)
    return img, gt, rng.random((H, W), dtype=np.float32)


def restate_mean_ssim(img, gt):
    """float64 NumPy, rows then columns: the mean of the standard SSIM map"""
    import numpy as np
    i = np.arange(11, dtype=np.float64)
    g = np.exp(-((i - 5) ** 2) / (2.0 * 1.5 ** 2)); g /= g.sum()
    x, y = img.astype(np.float64), gt.astype(np.float64)
    Cn, H, W = x.shape

    def blur(p):
        q = np.zeros((Cn, H + 10, W + 10)); q[:, 5:5 + H, 5:5 + W] = p
        rows = sum(g[k] * q[:, :, k:k + W] for k in range(11))
        return sum(g[k] * rows[:, k:k + H, :] for k in range(11))
    mx, my = blur(x), blur(y)
    sx, sy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    c1, c2 = 1e-4, 9e-4
    return float(((2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sx + sy + c2))).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080x3")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from gaussiansplat_amd import backend as B
    assert torch.cuda.is_available(), "needs a HIP device"
    W, H, Cn = (int(v) for v in a.size.split("x"))
    img, gt, wt = inputs(Cn, H, W)
    x, y, w = (torch.as_tensor(v).cuda() for v in (img, gt, wt))
    dC, smap = torch.empty_like(x), torch.empty_like(x)
    sums = torch.zeros(4, dtype=torch.float64, device="cuda")
    ctx = B.Context()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream or 1)
    variants = {
        "loss": lambda: ctx.loss_device(x.data_ptr(), y.data_ptr(), dC.data_ptr(), W, H, Cn, 0.2, False),
        "metrics": lambda: ctx.image_metrics_device(x.data_ptr(), y.data_ptr(), 0, W, H, Cn, 0, sums.data_ptr()),
        "metrics_map": lambda: ctx.image_metrics_device(x.data_ptr(), y.data_ptr(), 0, W, H, Cn, smap.data_ptr(), sums.data_ptr()),
        "metrics_weight": lambda: ctx.image_metrics_device(x.data_ptr(), y.data_ptr(), w.data_ptr(), W, H, Cn, smap.data_ptr(), sums.data_ptr()),
    }
    for f in variants.values():                                               # warm-up: code objects, scratch buffers
        for _ in range(3):
            f()
    variants["metrics"]()
    torch.cuda.synchronize()
    first = sums.cpu().numpy().copy()
    ms = interleaved({k: (lambda f=f: event_ms(f, a.batch)) for k, f in variants.items()}, a.reps, warmup=0)
    variants["metrics"]()
    torch.cuda.synchronize()
    last = sums.cpu().numpy().copy()
    fin = B.metrics_finish(last)
    res = {"device": torch.cuda.get_device_name(0), "width": W, "height": H, "channels": Cn, "reps": a.reps, "batch": a.batch,
           "ms_per_call": {k: stat(v) for k, v in ms.items()},
           "ratio_metrics_over_loss": statistics.median(ms["metrics"]) / statistics.median(ms["loss"]),
           "ratio_metrics_map_over_loss": statistics.median(ms["metrics_map"]) / statistics.median(ms["loss"]),
           "bitwise_reproducible": first.tobytes() == last.tobytes(),
           "mse": float(fin[B.METRIC_MSE]), "mae": float(fin[B.METRIC_MAE]), "ssim": float(fin[B.METRIC_SSIM]), "psnr": float(fin[B.METRIC_PSNR])}
    if a.check:
        res["ssim_minus_float64_restatement"] = float(fin[B.METRIC_SSIM]) - restate_mean_ssim(img, gt)
    ctx.close()
    emit(res, a.out)
    assert res["bitwise_reproducible"] and np.isfinite(last).all()
    assert not a.check or abs(res["ssim_minus_float64_restatement"]) <= 1e-10


if __name__ == "__main__":
    main()
