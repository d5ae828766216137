"""Adam timings at a BASELINE config (default C3: 1 M gaussians, 1920 x 1080, SH degree 3), variants interleaved in one process.

    python tools/adam_time.py [--config C3] [--reps 20] [--out profiles/NAME.json]

hipEvent times (torch.cuda.Event on the ctx's stream), median over `reps` rounds of every variant in turn:
  step_dense / step_selective   gs_adam_step alone on a stored gradient (the frame's own, OVERWRITE backward)
  bwd_sgd_unfused ...           the backward part of a training step (after loss): gs_backward_ex(OVERWRITE) + gs_sgd_step,
                                gs_backward_sgd, gs_backward_ex(OVERWRITE) + gs_adam_step (dense / selective), gs_backward_adam
                                (dense / selective)
  iter_*                        a whole train.trainStep (preprocess .. update) with SGD, fused SGD, Adam, fused Adam (dense / selective)
Every rate is 0 (a valid Adam step: m and v move, p does not), so the frame, and with it the work, is the same in every round.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a call of its own (--reps 5 is plenty there).
"""
from __future__ import annotations

import argparse
import statistics

from _timing import emit, event_ms, interleaved


def main():
    import torch
    from gaussiansplat_amd import renderer as R, synthetic, train as TR
    from gaussiansplat_amd.optim import Adam
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, W, H, deg = synthetic.CONFIGS[a.config]
    scene = synthetic.make_scene(n, W, H, deg, seed=1234 + list(synthetic.CONFIGS).index(a.config))
    cam = synthetic.scene_camera(W)
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, scene)
    lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
    gt = torch.rand((3, H, W), device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    zero = dict(means=0.0, scales=0.0, quaternions=0.0, opacities=0.0, sh_dc=0.0, sh_rest=0.0)
    opt = {k: Adam(r, lr=zero, selective=sel, fused=fu) for k, sel, fu in
           (("dense", False, False), ("selective", True, False), ("fused_dense", False, True), ("fused_selective", True, True))}

    def frame():
        tps = R.preprocess(r, cam); R.compactIdxs(r); R.forward(r, tps)
        return lf.value_and_grad(r.imageData, gt, want_loss=False)[1]

    def bwd(kind):
        dC = frame()
        def run():
            if kind == "sgd_unfused":
                R.resetGrads(r); R.backward(r, dC); r.ctx.sgd_step(0.0, r._grads)
            elif kind == "sgd_fused":
                r.ctx.backward_sgd(dC.data_ptr(), 1e-30)
            elif kind in ("adam_dense_unfused", "adam_selective_unfused"):
                R.resetGrads(r); R.backward(r, dC); opt[kind.split("_")[1]].step()
            else:
                opt["fused_" + kind.split("_")[1]].backward_step(dC)
        return event_ms(run)

    def step_only(kind):
        dC = frame()
        R.resetGrads(r); R.backward(r, dC); torch.cuda.synchronize()
        return event_ms(lambda: opt[kind].step())

    def iteration(kind):
        o = {"sgd": None, "sgd_fused": None, "adam": opt["dense"], "adam_selective": opt["selective"], "adam_fused": opt["fused_dense"],
             "adam_fused_selective": opt["fused_selective"]}[kind]
        return event_ms(lambda: TR.trainStep(r, gt, 0.0 if kind == "sgd" else 1e-30, lf, cam, want_loss=False, fused_sgd=kind == "sgd_fused",
                                             optimizer=o))

    variants = [("step_dense", lambda: step_only("dense")), ("step_selective", lambda: step_only("selective"))]
    variants += [("bwd_" + k, (lambda k=k: bwd(k))) for k in ("sgd_unfused", "sgd_fused", "adam_dense_unfused", "adam_selective_unfused",
                                                             "adam_dense_fused", "adam_selective_fused")]
    variants += [("iter_" + k, (lambda k=k: iteration(k))) for k in ("sgd", "sgd_fused", "adam", "adam_selective", "adam_fused",
                                                                    "adam_fused_selective")]
    times = interleaved(variants, a.reps, warmup=2)             # warm-up: view-slot history, allocations
    med = {k: statistics.median(v) for k, v in times.items()}
    n_floats = n * (11 + 3 * (deg + 1) ** 2)
    dC = frame()
    R.resetGrads(r); R.backward(r, dC)
    g = r.splatGrads.flat
    rows = torch.cat([g[:3 * n].view(n, 3), g[3 * n:6 * n].view(n, 3), g[6 * n:10 * n].view(n, 4), g[10 * n:11 * n].view(n, 1),
                      g[11 * n:].view(n, -1)], dim=1)
    touched = float((rows != 0).any(dim=1).float().mean())
    res = dict(config=a.config, n=n, W=W, H=H, sh_degree=deg, reps=a.reps, median_ms=med,
               live_fraction=touched, step_dense_bytes=7 * 4 * n_floats,
               step_dense_tbps=7 * 4 * n_floats / (med["step_dense"] * 1e-3) / 1e12,
               fused_selective_over_dense=med["bwd_adam_selective_fused"] / med["bwd_adam_dense_fused"],
               device=torch.cuda.get_device_name(0))
    emit(res, a.out, indent=1)


if __name__ == "__main__":
    main()
