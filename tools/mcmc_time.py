"""MCMC densification timings at 1 M and 100 k gaussians (SH degree 3), every device call beside the same step written in torch, interleaved in
one process.

    python tools/mcmc_time.py [--sizes 1000000,100000] [--reps 20] [--out profiles/NAME.json]

hipEvent times (torch.cuda.Event on the ctx's stream) after two warm-up rounds, median over `reps` rounds of every variant in turn:
  noise / torch_noise            gs_mcmc_noise against sigmoid, exp, the rotation and two einsums over [n, 3, 3] in torch (normals drawn outside)
  noise_burst / regularize_burst twenty calls between ONE pair of events, per call: a single call at these sizes is shorter than what an event pair and
                                 a launch cost, so the bandwidth figures are taken from these
  regularize / torch_regularize  mcmc.regularize (gs_mcmc_regularize and its Python) against (l_o sigmoid(o).mean() + l_s exp(s).mean()).backward() added to the gradients
  relocate / torch_relocate      gs_mcmc_plan + _sample + _relocate with 5 % of the gaussians dead and Adam's moments as companions (the plan's
                                 synchronise and the uniform draws included) against torch.multinomial + bincount + the row copies and the zeroing
                                 of the moment rows -- WITHOUT the corrected opacity and scales, which torch would need 1 326 more passes for
  grow / torch_grow              mcmc.grow by 5 % (allocations, gs_set_model, moments) against multinomial + torch.cat of the five arrays and moments
Bandwidth of the two per-iteration kernels: 68 B per gaussian for the noise (14 floats read, 3 written), 48 B for the regularisers (4 read, 4 read
and written), against what a copy reaches on the card.  Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a call of
its own (--reps 5 is plenty there).
"""
from __future__ import annotations

import argparse
import statistics

from _timing import emit, event_ms as timed, interleaved

MIN_OPACITY = 0.005


def one_size(n, reps):
    import torch
    from gaussiansplat_amd import backend as B, mcmc, renderer as R, synthetic
    from gaussiansplat_amd.density import logit
    from gaussiansplat_amd.optim import Adam
    deg, W = 3, 64
    scene = synthetic.make_scene(n, W, W, deg, seed=1234)
    r = R.getRenderer("GAUSSIAN_3D", (W, W, 3), (16, 16), None, scene)
    opt = Adam(r, lr=0.0)
    d = r.splatData
    gen = torch.Generator("cuda").manual_seed(0)
    z = torch.randn((n, 3), device="cuda", generator=gen)
    opac0 = d.opacities.clone()
    means0 = d.means.clone()
    dead_rows = torch.randperm(n, device="cuda", generator=gen)[:n // 20]
    r._begin()

    def restore():
        d.opacities.copy_(opac0); d.means.copy_(means0)
        d.opacities[dead_rows] = -8.0
        torch.cuda.synchronize()

    def torch_noise():
        sig = torch.sigmoid(d.opacities[:, 0])
        gate = 1.0 / (1.0 + torch.exp(100.0 * (sig - 0.005)))
        w, x, y, zz = d.quaternions.unbind(1)
        Rm = torch.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y - w * zz), 2 * (x * zz + w * y), 2 * (x * y + w * zz), 1 - 2 * (x * x - zz * zz),
                          2 * (y * zz - w * x), 2 * (x * zz - w * y), 2 * (y * zz + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)
        cov = torch.einsum("nij,nj,nkj->nik", Rm, torch.exp(2.0 * d.scales), Rm)
        d.means.add_(torch.einsum("nij,nj->ni", cov, z) * (80.0 * gate)[:, None])

    grads = r.splatGrads

    def torch_regularize():
        o, s = d.opacities.detach().requires_grad_(), d.scales.detach().requires_grad_()
        (0.01 * torch.sigmoid(o).mean() + 0.01 * torch.exp(s).mean()).backward()
        grads.Δopacities.add_(o.grad.reshape(grads.Δopacities.shape)); grads.Δscales.add_(s.grad.reshape(grads.Δscales.shape))

    def relocate():
        restore()
        return timed(lambda: mcmc.relocate(r, opt, min_opacity=MIN_OPACITY, generator=gen))

    moments = [opt.exp_avg, opt.exp_avg_sq]

    def torch_relocate():
        restore()

        def go():
            sig = torch.sigmoid(d.opacities[:, 0])
            alive = d.opacities[:, 0] > logit(MIN_OPACITY)
            dead = (~alive).nonzero()[:, 0]
            src = torch.multinomial(sig * alive, dead.numel(), replacement=True, generator=gen)
            cnt = torch.bincount(src, minlength=n)
            for t in (d.means, d.scales, d.quaternions, d.opacities, d.shs):
                t[dead] = t[src]
            rows = torch.cat([dead, (cnt > 0).nonzero()[:, 0]])
            for m in moments:
                for off, t in zip(R.layout_of(r._splatGrads)[0], (d.means, d.scales, d.quaternions, d.opacities, d.shs)):
                    m[off:off + t.numel()].view(t.shape)[rows] = 0.0
        return timed(go)

    g_struct = r._grads
    c_o, c_s = 0.01 / n, 0.01 / (3 * n)

    burst = lambda fn: timed(fn, batch=20)                       # twenty calls behind one another between one pair of events: the pair's own cost and
                                                                 # the first launch's latency are shared, what remains is the kernel (or the launch rate)

    variants = [("noise", lambda: timed(lambda: r.ctx.mcmc_noise(z.data_ptr(), 80.0, 100.0, 0.005))), ("torch_noise", lambda: timed(torch_noise)),
                ("noise_burst", lambda: burst(lambda: r.ctx.mcmc_noise(z.data_ptr(), 80.0, 100.0, 0.005))),
                ("regularize_burst", lambda: burst(lambda: r.ctx.mcmc_regularize(g_struct, c_o, c_s))),
                ("regularize", lambda: timed(lambda: mcmc.regularize(r))), ("torch_regularize", lambda: timed(torch_regularize)),
                ("relocate", relocate), ("torch_relocate", torch_relocate)]
    times = interleaved(variants, reps, warmup=2)
    med = {k: statistics.median(v) for k, v in times.items()}
    # growth changes n: a fresh renderer per round
    grow_t, torch_grow_t = [], []
    for _ in range(max(2, min(reps, 5))):
        r2 = R.getRenderer("GAUSSIAN_3D", (W, W, 3), (16, 16), None, scene)
        opt2 = Adam(r2, lr=0.0)
        torch.cuda.synchronize()
        grow_t.append(timed(lambda: mcmc.grow(r2, opt2, cap_max=2 * n, generator=gen)))
        d2 = r2.splatData

        def tg():
            add = int(1.05 * n) - n
            src = torch.multinomial(torch.sigmoid(d2.opacities[:n, 0]), add, replacement=True, generator=gen)
            new = [torch.cat([t[:n], t[src]]) for t in (d2.means, d2.scales, d2.quaternions, d2.opacities, d2.shs)]
            mom = [torch.cat([m, torch.zeros(add * 59, device="cuda")]) for m in (opt2.exp_avg, opt2.exp_avg_sq)]   # 59 floats per gaussian at degree 3
            return new, mom
        torch_grow_t.append(timed(tg))
        del r2, opt2, d2
    med["grow"], med["torch_grow"] = statistics.median(grow_t[1:]), statistics.median(torch_grow_t[1:])
    return dict(n=n, sh_degree=deg, reps=reps, median_ms=med, noise_bytes=68 * n, noise_tbps=68 * n / (med["noise_burst"] * 1e-3) / 1e12,
                regularize_bytes=48 * n, regularize_tbps=48 * n / (med["regularize_burst"] * 1e-3) / 1e12, dead_share=0.05)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,100000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), sizes=[one_size(int(s), a.reps) for s in a.sizes.split(",")])
    emit(res, a.out, indent=1)


if __name__ == "__main__":
    main()
