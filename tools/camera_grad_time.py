#!/usr/bin/env python3
"""What gs_backward_camera costs beside the frame's own per-gaussian backward (GPU box).

    python3 tools/camera_grad_time.py [--configs C3,C2] [--reps 20] [--out profiles/camera_grad_time.json]

Per config (BASELINE scene, view 0, random dC): frames are rendered forward and backward (overwriting); alternating in every
repetition, after two warm-up frames:
  backward        one frame's preprocess .. gs_backward; the per-gaussian backward is read from the ctx's own stage timer
                  (GS_STAGE_PREPROCESS_BWD: device events around gs_sh_bwd_kernel with the geometry chain fused in)
  camera          gs_backward_camera(GS_MEM_DEVICE) on that frame, device events around the call (two launches)
Median, min and max of `reps`; the share of gaussians with a live row (the others cost the camera kernel one 64-byte row read)."""
import argparse
import statistics

from _timing import emit, event_ms, stat


def run(config, reps):
    import numpy as np
    import torch
    from gaussiansplat_amd import backend as B, renderer as R, synthetic
    n, W, H, deg = synthetic.CONFIGS[config]
    scene = synthetic.make_scene(n, W, H, deg, seed=1234)
    cam = synthetic.scene_camera(W, view=0)
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, scene, profile_stages=True)
    dC = torch.as_tensor(synthetic.make_dC(W, H, 1)).cuda()
    out = torch.zeros(B.GS_CAMERA_GRAD_FLOATS, dtype=torch.float32, device="cuda")

    def frame():
        tps = R.preprocess(r, cam)
        R.compactIdxs(r)
        R.forward(r, tps)
        R.resetGrads(r)
        R.backward(r, dC)

    for _ in range(2):
        frame()
        r.ctx.backward_camera(out.data_ptr())
    torch.cuda.synchronize()
    first = out.cpu().numpy().copy()
    cam_ms, bwd_ms = [], []
    for _ in range(reps):
        frame()
        torch.cuda.synchronize()
        bwd_ms.append(r.ctx.stage_times()["preprocess_bwd"])
        cam_ms.append(event_ms(lambda: r.ctx.backward_camera(out.data_ptr())))
    g2d = r.ctx.get_array(B.ARR_GRAD2D)
    return {"config": config, "gaussians": n, "width": W, "height": H, "sh_degree": deg, "reps": reps,
            "live_row_share": float(np.count_nonzero(g2d.reshape(n, -1).any(axis=1))) / n,
            "finite": bool(np.isfinite(first).all()), "nonzero": bool(first.any()),
            "backward_camera_ms": stat(cam_ms), "preprocess_bwd_ms": stat(bwd_ms),
            "ratio_of_medians": statistics.median(cam_ms) / max(statistics.median(bwd_ms), 1e-9)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,C2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    res = {"device": torch.cuda.get_device_name(0), "results": [run(c, a.reps) for c in a.configs.split(",")]}
    emit(res, a.out)
    assert all(x["finite"] and x["nonzero"] for x in res["results"])


if __name__ == "__main__":
    main()
