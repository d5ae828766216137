"""What a background colour costs the forward, at a BASELINE config (default C3: 1 M gaussians, 1920 x 1080, SH degree 3): the
composite-forward stage with the background off (black: nothing is launched) and on (one elementwise launch behind the last composite
round, inside the stage's pair of events), and a plain device-to-device copy of the bytes that launch moves.

    python tools/background_time.py [--config C3] [--reps 15] [--out profiles/NAME.json]

Times are gs_get_stage_times (hipEvents around the stage on the ctx's stream), median / min / max over `reps` rounds; off and on are
interleaved inside every round, so clock ramps and neighbours hit both alike.  The blend reads image and transmittance and writes the image:
28 B per pixel, 58 MB at 1920 x 1080.  The copy (torch's Tensor.copy_, 14 B per pixel read and 14 B written, timed by events on torch's
stream in the same process and the same rounds) is the yardstick for a pass of that size: it has no kernel boundary in front of it that
it must wait at, the blend does.
"""
from __future__ import annotations

import argparse

from _timing import emit, event_ms, interleaved, stat

BG = (1.0, 0.25, 0.6)


def main():
    import torch
    from gaussiansplat_amd import renderer as R, synthetic
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, W, H, deg = synthetic.CONFIGS[a.config]
    scene = synthetic.make_scene(n, W, H, deg, seed=1234 + list(synthetic.CONFIGS).index(a.config))
    cam = synthetic.scene_camera(W)
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, scene, profile_stages=True)
    px = W * H
    src, dst = torch.rand(7 * px // 2, device="cuda"), torch.empty(7 * px // 2, device="cuda")   # 14 B per pixel each way

    def frame():
        tps = R.preprocess(r, cam); R.compactIdxs(r); R.forward(r, tps)
        torch.cuda.synchronize()
        return r.ctx.stage_times()["composite_fwd"]

    def with_background(bg):
        r.background = bg
        frame()                                                 # the colour changed: one frame to settle, the next one counts
        return frame()

    # two untimed calls of each: view-slot history, allocations, code objects
    times = interleaved(dict(off=lambda: with_background((0.0, 0.0, 0.0)), on=lambda: with_background(BG),
                             copy=lambda: event_ms(lambda: dst.copy_(src))), a.reps, warmup=2)
    r.background = (0.0, 0.0, 0.0)
    res = dict(config=a.config, n=n, W=W, H=H, sh_degree=deg, reps=a.reps, unit="ms", device=torch.cuda.get_device_name(0), background=BG,
               blend_bytes=28 * px, copy_bytes=2 * src.numel() * 4,
               composite_fwd=dict(off=stat(times["off"]), on=stat(times["on"])), copy=stat(times["copy"]))
    res["added_median"] = res["composite_fwd"]["on"]["median"] - res["composite_fwd"]["off"]["median"]
    res["added_over_copy"] = res["added_median"] / res["copy"]["median"]
    emit(res, a.out, indent=1)
    print("composite forward, background off  %.4f ms (min %.4f max %.4f)" % tuple(res["composite_fwd"]["off"][k] for k in ("median", "min", "max")))
    print("composite forward, background on   %.4f ms (min %.4f max %.4f)" % tuple(res["composite_fwd"]["on"][k] for k in ("median", "min", "max")))
    print("device-to-device copy, %d bytes     %.4f ms (min %.4f max %.4f)" % ((res["copy_bytes"],) + tuple(res["copy"][k] for k in ("median", "min", "max"))))
    print("added by the background: %.4f ms = %.2f x the copy" % (res["added_median"], res["added_over_copy"]))


if __name__ == "__main__":
    main()
