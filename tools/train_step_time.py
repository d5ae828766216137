#!/usr/bin/env python3
"""Time of one training iteration of src/train.jl as intended (preprocess, lists, forward, L1 + DSSIM loss with its image
gradient, backward, SGD step) at C3 -- the loss / optimiser rows of SURVEY 8(f).2 next to the fwd+bwd headline.
    python3 tools/train_step_time.py [C3]     (GPU box)"""
import sys

from _timing import host_clock_ms
import torch
from gaussiansplat_amd import renderer as R, synthetic, train as TR

cfg = sys.argv[1] if len(sys.argv) > 1 else "C3"
n, W, H, deg = synthetic.CONFIGS[cfg]
gx, gy = (W + 15) // 16, (H + 15) // 16
scene = synthetic.make_scene(n, W, H, deg, seed=1236)
r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), (gx, gy), scene, device=0, t_min=1e-5)
cam = synthetic.scene_camera(W, view=0)
gt = torch.rand((3, H, W), device="cuda")
lossFunc = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
for want, fused in ((False, False), (True, False), (False, True)):
    ms = host_clock_ms(lambda: TR.trainStep(r, gt, 1e-4, lossFunc, cam, want_loss=want, fused_sgd=fused), k=50, warmup=5)
    print({"config": cfg, "want_loss_value_on_host": want, "fused_backward_sgd": fused, "ms_per_iteration": round(ms, 3)})
# the pieces
print({"loss_and_grad_ms": round(host_clock_ms(lambda: lossFunc.value_and_grad(r.imageData, gt, False), k=50, warmup=3), 3)})
r._begin(); g = r._grads
print({"sgd_step_ms": round(host_clock_ms(lambda: r.ctx.sgd_step(1e-4, g), k=50, warmup=3), 3)})
