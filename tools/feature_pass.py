"""What a feature map costs beside the frame it is rendered over, at a BASELINE config (default C3: 1 M gaussians, 1920 x 1080, SH
degree 3): gs_render_features and gs_backward_features against the same frame's composite stages.

    python tools/feature_pass.py [--config C3] [--reps 50] [--tile-parts 0] [--out profiles/NAME.json]

The feature calls are timed with hipEvents on the ctx's stream (torch's current stream) around ONE call, `reps` times after five
untimed ones, on one finished frame (the calls keep no state and leave the frame alone, so every repetition does the same work); the
frame's own composite forward / backward and per-gaussian backward are gs_get_stage_times of `reps` frames rendered before.  Yardstick
for the payload copy (64 B read + 64 B written per gaussian): a device-to-device copy of 64 n bytes, timed the same way.
Expected beforehand: forward = the frame's composite forward + one 128-byte-per-gaussian streaming kernel; backward (whole tiles) no more than
the frame's composite backward under tile_parts = 1, plus the geometry chain.  --tile-parts 1 renders the frame that way.
"""
from __future__ import annotations

import argparse

from _timing import emit, event_ms, interleaved, stat


def main():
    import torch
    from gaussiansplat_amd import backend as B, renderer as R, synthetic
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--tile-parts", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, W, H, deg = synthetic.CONFIGS[a.config]
    scene = synthetic.make_scene(n, W, H, deg, seed=1234 + list(synthetic.CONFIGS).index(a.config))
    cam = synthetic.scene_camera(W)
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, scene, profile_stages=True, slab_mode=0, tile_parts=a.tile_parts)
    dC = torch.as_tensor(synthetic.make_dC(W, H, 7)).cuda()

    def frame():
        tps = R.preprocess(r, cam); R.compactIdxs(r); R.forward(r, tps)
        R.resetGrads(r); R.backward(r, dC)
        torch.cuda.synchronize()
        return r.ctx.stage_times()

    frames = interleaved({"frame": frame}, a.reps, warmup=3)["frame"]     # three untimed frames: view-slot history, allocations, code objects
    stages = {k: [st[k] for st in frames] for k in ("composite_fwd", "composite_bwd", "preprocess_bwd")}
    tps = R.preprocess(r, cam); R.compactIdxs(r); R.forward(r, tps)  # the frame the feature calls run over (between its forward and backward)
    z = R.viewDepth(r)
    feat = torch.stack((z, z * z, torch.ones_like(z)), 1).contiguous()
    F = torch.empty((3, H, W), device="cuda"); T = torch.empty((H, W), device="cuda")
    dF = torch.randn((3, H, W), device="cuda") * 1e-3
    d_feat = torch.empty((n, 3), device="cuda")
    g = r._grads
    grads = B.GsGrads(g.d_means, g.d_scales, g.d_quats, g.d_opacities, None)
    src, dst = torch.rand(16 * n, device="cuda"), torch.empty(16 * n, device="cuda")
    calls = dict(
        view_depth=lambda: r.ctx.view_depth(z.data_ptr()),
        render_features=lambda: r.ctx.render_features(feat.data_ptr(), F.data_ptr(), T.data_ptr()),
        backward_features=lambda: r.ctx.backward_features(feat.data_ptr(), F.data_ptr(), dF.data_ptr(), d_feat.data_ptr(), grads),
        backward_features_no_chain=lambda: r.ctx.backward_features(feat.data_ptr(), F.data_ptr(), dF.data_ptr(), d_feat.data_ptr(), None),
        copy_64n_bytes=lambda: dst.copy_(src))
    times = interleaved({k: (lambda fn=fn: event_ms(fn)) for k, fn in calls.items()}, a.reps, warmup=5)
    R.backward(r, dC)                                             # the frame goes on
    torch.cuda.synchronize()
    res = dict(config=a.config, n=n, W=W, H=H, sh_degree=deg, reps=a.reps, unit="ms", device=torch.cuda.get_device_name(0),
               tile_parts_asked=a.tile_parts, tile_parts_of_frame=r.ctx.tile_parts_of_frame(), payload_bytes=128 * n,
               frame={k: stat(v) for k, v in stages.items()}, calls={k: stat(v) for k, v in times.items()})
    m = lambda d: d["median"]
    res["render_minus_composite_fwd"] = m(res["calls"]["render_features"]) - m(res["frame"]["composite_fwd"])
    res["backward_no_chain_minus_composite_bwd"] = m(res["calls"]["backward_features_no_chain"]) - m(res["frame"]["composite_bwd"])
    res["chain"] = m(res["calls"]["backward_features"]) - m(res["calls"]["backward_features_no_chain"])
    emit(res, a.out, indent=1)


if __name__ == "__main__":
    main()
