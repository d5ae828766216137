"""Density-control timings at a BASELINE config (default C3: 1 M gaussians, 1920 x 1080, SH degree 3), variants interleaved in one process.

    python tools/density_time.py [--config C3] [--reps 20] [--out profiles/NAME.json]

hipEvent times (torch.cuda.Event on the ctx's stream), median over `reps` rounds of every variant in turn:
  iter_adam / iter_adam_accumulate   an unfused train.trainStep with optim.Adam, without and with gs_density_accumulate between the
                                     backward and the step (a DensityController whose schedule never restructures)
  accumulate                         gs_density_accumulate alone on the frame's sums
  decide / plan / restructure        the three calls of one densify_and_prune on actions dealt at random: about 10 % clones, 5 % splits,
                                     5 % pruned (plan includes its synchronise and the read-back of the four counts)
  densify_and_prune                  the whole density.densify_and_prune (allocations, normals, gs_set_model included) with thresholds
                                     taken from the run's own statistics so that the same shares clone, split and are pruned
Every rate is 0 (a valid Adam step: m and v move, p does not), so the frame, and with it the work, is the same in every round.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a call of its own (--reps 5 is plenty there).
"""
from __future__ import annotations

import argparse
import statistics

import numpy as np

from _timing import emit, event_ms as timed, interleaved


def main():
    import torch
    from gaussiansplat_amd import backend as B, renderer as R, synthetic, train as TR
    from gaussiansplat_amd.density import DensityController, DensityStats, densify_and_prune, density_params
    from gaussiansplat_amd.optim import Adam
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, W, H, deg = synthetic.CONFIGS[a.config]
    k3 = 3 * (deg + 1) ** 2
    scene = synthetic.make_scene(n, W, H, deg, seed=1234 + list(synthetic.CONFIGS).index(a.config))
    cam = synthetic.scene_camera(W)
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, scene)
    lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
    gt = torch.rand((3, H, W), device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    zero = dict(means=0.0, scales=0.0, quaternions=0.0, opacities=0.0, sh_dc=0.0, sh_rest=0.0)
    opt = Adam(r, lr=zero)
    never = DensityController(scene_extent=1.0, from_iter=10 ** 9, until_iter=10 ** 9, interval=1, opacity_reset_interval=0)
    stats = DensityStats(r)

    def frame():
        tps = R.preprocess(r, cam); R.compactIdxs(r); R.forward(r, tps)
        dC = lf.value_and_grad(r.imageData, gt, want_loss=False)[1]
        R.resetGrads(r); R.backward(r, dC)

    def iteration(with_stats):
        return timed(lambda: TR.trainStep(r, gt, 0.0, lf, cam, want_loss=False, optimizer=opt, density=never if with_stats else None))

    def accumulate():
        frame(); torch.cuda.synchronize()
        return timed(stats.accumulate)

    # one restructure's worth of inputs: actions dealt at random, destinations of the planned size, Adam's moments as companions
    rng = np.random.default_rng(0)
    act = torch.from_numpy(rng.choice(4, n, p=[0.80, 0.10, 0.05, 0.05]).astype(np.int32)).cuda()
    noise = torch.randn((n, 2, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    params = density_params(scene_extent=1.0)
    scratch_action = torch.empty(n, dtype=torch.int32, device="cuda")
    r._begin()
    counts = r.ctx.density_plan(act.data_ptr())
    n_out = counts[0] + counts[1] + 2 * counts[2]
    widths = [3, 3, 4, 1, k3]
    dst = [torch.empty((n_out, w), device="cuda") for w in widths]
    dst_m = [[torch.empty((n_out, w), device="cuda") for w in widths] for _ in range(2)]
    g = lambda ts: B.GsGrads(*[t.data_ptr() for t in ts])

    def restructure():
        r.ctx.density_plan(act.data_ptr())
        return timed(lambda: r.ctx.density_restructure(act.data_ptr(), noise.data_ptr(), g(dst), opt.moment_structs(),
                                                       [g(dst_m[0]), g(dst_m[1])], n_out))

    variants = [("iter_adam", lambda: iteration(False)), ("iter_adam_accumulate", lambda: iteration(True)), ("accumulate", accumulate),
                ("decide", lambda: timed(lambda: r.ctx.density_decide(stats.struct(), params, scratch_action.data_ptr()))),
                ("plan", lambda: timed(lambda: r.ctx.density_plan(act.data_ptr()))), ("restructure", restructure)]
    times = interleaved(variants, a.reps, warmup=2)             # warm-up: view-slot history, allocations
    med = {k: statistics.median(v) for k, v in times.items()}
    # the whole densify_and_prune, once per fresh renderer (it changes the model): thresholds from the statistics of four frames
    whole = []
    shares = None
    for _ in range(max(1, min(a.reps, 5))):
        r2 = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, scene)
        lf2 = TR.getLossFunction((W, H, 3), 11, 3, renderer=r2)
        opt2 = Adam(r2, lr=zero)
        ctl = DensityController(scene_extent=1.0, from_iter=10 ** 9, until_iter=10 ** 9, interval=1, opacity_reset_interval=0)
        for _ in range(4):
            TR.trainStep(r2, gt, 0.0, lf2, cam, want_loss=False, optimizer=opt2, density=ctl)
        st = ctl.stats
        mean = (st.grad_sum / st.count.clamp(min=1).float())[st.count > 0]
        thr = float(torch.quantile(mean[torch.randperm(mean.numel(), device="cuda")[:1_000_000]], 0.85))      # 15 % densify ...
        smax = r2.splatData.scales.max(dim=1).values
        kw = dict(scene_extent=1.0, grad_threshold=thr, percent_dense=float(torch.quantile(smax[:1_000_000], 2.0 / 3.0).exp()),   # ... a third of them split
                  min_opacity=float(torch.sigmoid(torch.quantile(r2.splatData.opacities[:1_000_000, 0], 0.05))), max_world_fraction=None)
        torch.cuda.synchronize()
        out = {}
        whole.append(timed(lambda: out.update(densify_and_prune(r2, st, opt2, generator=torch.Generator("cuda").manual_seed(2), **kw))))
        shares = {k: out[k] / n for k in ("clones", "splits", "pruned")}
        del r2, lf2, opt2, ctl, st
    med["densify_and_prune"] = statistics.median(whole)
    row = 4 * (11 + k3)
    # bytes of the restructure: the action word per source row, every output row read once and written once, the two companion sets alike
    # (rows of survivors: read and written; new rows: written), 24 B of normals per split source
    fresh = counts[1] + 2 * counts[2]
    restructure_bytes = 4 * n + 2 * row * n_out + 2 * (2 * row * counts[0] + row * fresh) + 24 * counts[2]
    res = dict(config=a.config, n=n, W=W, H=H, sh_degree=deg, reps=a.reps, median_ms=med,
               accumulate_bytes=168 * n, accumulate_tbps=168 * n / (med["accumulate"] * 1e-3) / 1e12,
               accumulate_cost_per_iteration_ms=med["iter_adam_accumulate"] - med["iter_adam"],
               restructure_counts=dict(survivors=counts[0], clones=counts[1], splits=counts[2], pruned=counts[3], n_out=n_out),
               restructure_bytes=restructure_bytes, restructure_tbps=restructure_bytes / (med["restructure"] * 1e-3) / 1e12,
               densify_and_prune_shares=shares, device=torch.cuda.get_device_name(0))
    emit(res, a.out, indent=1)


if __name__ == "__main__":
    main()
