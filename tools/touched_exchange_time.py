#!/usr/bin/env python3
"""What the touched-rows exchange costs a rank outside the collectives (GPU box).

    python3 tools/touched_exchange_time.py [--config C3] [--views 8] [--reps 20] [--out profiles/touched_exchange_device.json]

One view of the config is rendered forward and backward once; its colour gradients stand for all `views` gathered views (the
same bitmap and rows replicated).  Timed, alternating, with device events around each variant and a host clock around the same
window ending in a synchronise (median of `reps` after a warm-up of each):
  device    gs_color_rows_pack of the view from the ctx + gs_sh_grads_from_touched over the gathered views
  torch     what "touched" did before the device kernels: gs_color_grads_pack into a dense slot, distributed.pack_touched_rows, the
            padding loop of exchange_touched_rows, unpack_touched_rows into a dense [views, N, 3] array, gs_sh_grads_from_views
  factored  the plain colour-factored path: gs_color_grads_pack + gs_sh_grads_from_views over dense slots
All three must leave the same d_shs, bit for bit; the script fails otherwise."""
import argparse

from _timing import emit, event_ms, host_clock_ms, interleaved, stat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from gaussiansplat_amd import distributed as D, renderer as R, synthetic
    assert torch.cuda.is_available(), "needs a HIP device"
    n, W, H, deg = synthetic.CONFIGS[a.config]
    V = a.views
    scene = synthetic.make_scene(n, W, H, deg, seed=1234)
    cams = [synthetic.scene_camera(W, view=0)] * V
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, scene)
    hv = D.HipViewRenderer(r)
    dC = torch.as_tensor(synthetic.make_dC(W, H, 1)).cuda()
    hv.reset()
    slot = hv.color_slots(1)
    hv.render_view_factored(cams[0], dC, slot[0])                          # the backward whose sums every variant packs
    ctx, recs = r.ctx, D.view_records(cams, W, H)
    d_shs = r.splatGrads.Δshs
    bits, rows, counts = hv.touched_buffers(1)
    words = bits.shape[1]
    dense_all = torch.empty((V, n, 3), dtype=torch.float32, device="cuda")

    def device():
        ctx.color_rows_pack(None, n, bits.data_ptr(), rows.data_ptr(), counts.data_ptr())
        cap = max(int(counts.max()), 1)                                    # the step's one host read
        all_bits = bits.expand(V, words).contiguous()                      # stands for the gathers
        all_rows = rows[:, :cap].expand(V, cap, 3).contiguous()
        ctx.sh_grads_from_touched(recs, all_bits.data_ptr(), all_rows.data_ptr(), cap, d_shs.data_ptr(), overwrite=True)

    def torch_path():
        ctx.color_grads_pack(slot.data_ptr())
        b, c, rw = D.pack_touched_rows(slot)
        cap = max(int(c.max()), 1)
        mine = torch.zeros((1, cap, 3), dtype=slot.dtype, device=slot.device)
        mine[0, :rw[0].shape[0]] = rw[0]
        all_bits, all_counts = b.expand(V, words).contiguous(), c.expand(V).contiguous()
        all_rows = mine.expand(V, cap, 3).contiguous()
        dense = D.unpack_touched_rows(all_bits, all_counts, all_rows, n, slot.dtype)
        ctx.sh_grads_from_views(recs, dense.data_ptr(), d_shs.data_ptr(), overwrite=True)

    def factored():
        ctx.color_grads_pack(slot.data_ptr())
        dense_all.copy_(slot.expand(V, n, 3))                              # stands for the gather
        ctx.sh_grads_from_views(recs, dense_all.data_ptr(), d_shs.data_ptr(), overwrite=True)

    variants = {"device": device, "torch": torch_path, "factored": factored}
    results = {}
    for name, f in variants.items():                                       # warm-up, and the results must agree
        r._begin()
        f(); f()
        torch.cuda.synchronize()
        results[name] = d_shs.cpu().numpy().view(np.uint32).copy()
    same = all(np.array_equal(results["factored"], v) for v in results.values())

    def both_clocks(f):                                                    # the host clock runs around the events' window
        ev = []
        host = host_clock_ms(lambda: ev.append(event_ms(f)), k=1)
        return ev[0], host

    both = interleaved({k: (lambda f=f: both_clocks(f)) for k, f in variants.items()}, a.reps, warmup=0)
    out = {"config": a.config, "gaussians": n, "views": V, "reps": a.reps, "touched_share": float(counts.cpu()[0]) / n,
           "same_bits": bool(same),
           "device_events_ms": {k: stat([e for e, _ in v]) for k, v in both.items()},
           "host_clock_ms": {k: stat([h for _, h in v]) for k, v in both.items()}}
    emit(out, a.out)
    assert same, "the three paths left different d_shs"


if __name__ == "__main__":
    main()
