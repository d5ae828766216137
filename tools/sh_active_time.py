"""What an active SH degree below the stored one costs or saves, per stage, at a BASELINE config (default C3: 1 M gaussians,
1920 x 1080, SH degree 3): the preprocess and the per-gaussian backward under gs_set_active_sh_degree 3, 2, 1, 0 on the same model.

    python tools/sh_active_time.py [--config C3] [--reps 15] [--out profiles/NAME.json]

Times are gs_get_stage_times (hipEvents around the stage on the ctx's stream), median / min / max over `reps` rounds; the degrees are
interleaved inside every round, so clock ramps and neighbours hit all of them alike.  Two forms of the backward: the overwriting
gs_backward (its SH zeros ride the composite launch) and the fused gs_backward_adam (every rate 0: the model, and with it the frame,
stays the same).  The stored rows stay 3 (D + 1)^2 floats apart whatever the active degree: this measures strided access, not a
narrower model.
"""
from __future__ import annotations

import argparse

from _timing import emit, interleaved, stat


def main():
    import torch
    from gaussiansplat_amd import renderer as R, synthetic, train as TR
    from gaussiansplat_amd.optim import Adam
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, W, H, deg = synthetic.CONFIGS[a.config]
    scene = synthetic.make_scene(n, W, H, deg, seed=1234 + list(synthetic.CONFIGS).index(a.config))
    cam = synthetic.scene_camera(W)
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, scene, profile_stages=True)
    lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
    gt = torch.rand((3, H, W), device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    zero = dict(means=0.0, scales=0.0, quaternions=0.0, opacities=0.0, sh_dc=0.0, sh_rest=0.0)
    opt = Adam(r, lr=zero, fused=True)

    def frame(form):
        tps = R.preprocess(r, cam); R.compactIdxs(r); R.forward(r, tps)
        dC = lf.value_and_grad(r.imageData, gt, want_loss=False)[1]
        if form == "overwrite":
            R.resetGrads(r); R.backward(r, dC)
        else:
            opt.backward_step(dC)
        torch.cuda.synchronize()
        t = r.ctx.stage_times()
        return t["preprocess"], t["preprocess_bwd"]

    degrees = list(range(deg, -1, -1))
    forms = ("overwrite", "adam_fused")

    def at_degree(d, f):
        r.active_sh_degree = d
        frame(f)                                                # the degree changed: one frame to settle, the next one counts
        return frame(f)

    # two untimed calls of each: view-slot history, allocations, code objects
    pairs = interleaved({(d, f): (lambda d=d, f=f: at_degree(d, f)) for d in degrees for f in forms}, a.reps, warmup=2)
    times = {k: list(zip(*v)) for k, v in pairs.items()}        # (preprocess samples, per-gaussian backward samples)
    r.active_sh_degree = -1
    res = dict(config=a.config, n=n, W=W, H=H, stored_degree=deg, reps=a.reps, unit="ms", device=torch.cuda.get_device_name(0),
               stages={f"active{d}": {f: dict(preprocess=stat(times[d, f][0]), preprocess_bwd=stat(times[d, f][1])) for f in forms}
                       for d in degrees})
    emit(res, a.out, indent=1)
    print("active  form        preprocess (median ms)  per-gaussian backward (median ms)")
    for d in degrees:
        for f in forms:
            s = res["stages"][f"active{d}"][f]
            print(f"{d:6d}  {f:<10s}  {s['preprocess']['median']:22.4f}  {s['preprocess_bwd']['median']:33.4f}")


if __name__ == "__main__":
    main()
