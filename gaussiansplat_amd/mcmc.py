"""MCMC densification on the device: the strategy of "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al. 2024).

    train.trainStep(..., optimizer=opt, density=MCMCController(cap_max=1_000_000))

or, by hand, per iteration between backward and the optimiser step `regularize(renderer)`, after the step `inject_noise(renderer, lr)`,
and every hundred iterations `relocate(renderer, opt)` then `grow(renderer, opt, cap_max=...)`.

A fixed budget of gaussians (cap_max) instead of a gradient threshold; dead gaussians (opacity <= min_opacity) are relocated onto live
ones drawn with probability proportional to opacity, and the opacity and scales of both are corrected so that the rendered result is
unchanged; the model grows by 5 % per interval up to the cap by the same draw; noise shaped by every gaussian's covariance is added to the
means after every step; two L1 regularisers on opacity and scale make unused gaussians die.  No opacity reset, and memory is predictable.

Everything runs in the HIP library (csrc/gs_mcmc.hip; semantics in include/gsplat.h and DESIGN.md 5.8l).  torch allocates the arrays and
draws the random numbers (so the caller's generator decides them); the kernels are pure functions of their inputs.

Not covered: the fused backwards (Adam(fused=True), fused_sgd: trainStep refuses them with `density=`), multi-GPU relocation (it is
deterministic given equal draws, so replicated ranks may each run it with generators seeded alike), and the 2-D renderer (the library
answers GS_ERR_UNSUPPORTED).
"""
from __future__ import annotations

import math

from . import renderer as R
from ._checks import integer, logit, positive, probability


def _plan(renderer, min_opacity: float):
    """gs_mcmc_plan on the renderer's model: (cdf, dead, (alive, dead count, total))."""
    import torch
    n = renderer.nGaussians
    dev = renderer.splatData.means.device
    cdf = torch.empty(max(n, 1), dtype=torch.int64, device=dev)          # uint64 words: torch has no unsigned 64-bit arithmetic, nor is any done here
    dead = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    counts = renderer._begin().mcmc_plan(logit(min_opacity), cdf.data_ptr(), dead.data_ptr())
    return cdf, dead, counts


def _draw(renderer, cdf, m: int, generator):
    """m sources from the plan's CDF by m uniform numbers of `generator`: an int32 device tensor."""
    import torch
    u = R.draw(torch.rand, m, generator, cdf.device)
    src = torch.empty(m, dtype=torch.int32, device=cdf.device)
    renderer._begin().mcmc_sample(cdf.data_ptr(), renderer.nGaussians, u.data_ptr(), m, src.data_ptr())
    return src


def _moment_sets(renderer, optimizer, who: str):
    if optimizer is None:
        return []
    if optimizer.renderer is not renderer:
        raise ValueError(f"{who}: the optimiser belongs to another renderer")
    return optimizer.moment_structs()


def relocate(renderer, optimizer=None, *, min_opacity=0.005, generator=None) -> dict:
    """Every dead gaussian (opacity <= min_opacity, or NaN) becomes a copy of a live one drawn with probability proportional to opacity;
    source and copies get the opacity and scales that leave the rendered result unchanged, their rows of `optimizer`'s moments become
    zero.  Returns dict(alive, dead, relocated, src): relocated is 0 when nothing is dead or nothing is alive; src is the int32 device
    tensor of the draws (None when nothing was relocated)."""
    R.require_3d(renderer, "relocate")
    mo = probability("density: min_opacity", min_opacity)
    sets = _moment_sets(renderer, optimizer, "relocate")
    cdf, dead_list, (alive, dead, total) = _plan(renderer, mo)   # dead_list: what the ctx's plan points at; it lives until the relocation is enqueued
    if dead == 0 or total == 0:
        return dict(alive=alive, dead=dead, relocated=0, src=None)
    src = _draw(renderer, cdf, dead, generator)
    renderer._begin().mcmc_relocate(src.data_ptr(), None, dead, mo, sets)
    return dict(alive=alive, dead=dead, relocated=dead, src=src)


def grow(renderer, optimizer=None, *, cap_max, growth=1.05, min_opacity=0.005, generator=None) -> dict:
    """The model grows to min(cap_max, int(growth * n)) gaussians: the new ones are copies of live ones drawn with probability proportional
    to opacity, corrected like a relocation.  The renderer gets new splatData, a fresh zero gradient buffer and the new model; `optimizer`
    (optim.Adam) gets moment buffers of the new size -- old rows carried over, rows of sources and new gaussians zero, step_count kept.
    Returns dict(n, added, src)."""
    import torch
    R.require_3d(renderer, "grow")
    renderer.check_resize(optimizer, "grow")
    integer("mcmc", "cap_max", cap_max, 1, strict=True)
    g = positive("density: growth", growth)
    mo = probability("density: min_opacity", min_opacity)
    n = renderer.nGaussians
    added = max(0, min(cap_max, int(g * n)) - n)
    if added == 0:
        return dict(n=n, added=0, src=None)
    cdf, _, (_, _, total) = _plan(renderer, mo)
    if total == 0:                                               # nobody is alive: nothing to draw from
        return dict(n=n, added=0, src=None)
    src = _draw(renderer, cdf, added, generator)
    n_out = n + added
    new = renderer.alloc_model(n_out, zero=True)                 # the first n rows copied on the device, the new ones +0 until the relocation fills them
    for t_new, t_old in zip(R.model_arrays(new), R.model_arrays(renderer.splatData)):
        t_new[:n].copy_(t_old)
    moments, sets = (), []
    if optimizer is not None:
        *moments, sets = optimizer.resized_moments(n_out, zero=True, keep_rows=n)
    renderer.adopt_model(new, "grow")
    dst = torch.arange(n, n_out, dtype=torch.int32, device=new.means.device)
    renderer._begin().mcmc_relocate(src.data_ptr(), dst.data_ptr(), added, mo, sets)
    if optimizer is not None:
        optimizer._rebind(*moments)
    return dict(n=n_out, added=added, src=src)


def inject_noise(renderer, lr, *, gate_k=100.0, gate_t=0.005, generator=None):
    """means += lr * gate * Sigma z with z standard normals of `generator`, Sigma the covariance the renderer draws and
    gate = 1 / (1 + exp(gate_k * (sigmoid(opacity) - gate_t))): opaque gaussians stay, transparent ones explore.  lr == 0: nothing."""
    import torch
    R.require_3d(renderer, "inject_noise")
    rate = positive("density: lr", lr, allow_zero=True)
    for name, v in (("gate_k", gate_k), ("gate_t", gate_t)):
        if not math.isfinite(float(v)):
            raise ValueError(f"mcmc: {name} must be finite, got {v!r}")
    if rate == 0.0 or renderer.nGaussians == 0:
        return
    z = R.draw(torch.randn, (renderer.nGaussians, 3), generator, renderer.splatData.means.device)
    renderer._begin().mcmc_noise(z.data_ptr(), rate, float(gate_k), float(gate_t))


def regularize(renderer, *, opacity_reg=0.01, scale_reg=0.01):
    """Adds the gradients of opacity_reg * mean(sigmoid(opacity)) + scale_reg * mean(exp(scale)) to renderer.splatGrads: between the
    backward and the optimiser step.  The frame stands."""
    R.require_3d(renderer, "regularize")
    lo, ls = positive("density: opacity_reg", opacity_reg, allow_zero=True), positive("density: scale_reg", scale_reg, allow_zero=True)
    n = renderer.nGaussians
    if n == 0 or (lo == 0.0 and ls == 0.0):
        return
    renderer.splatGrads                                          # a pending resetGrads zero-fills here: the sums start from zeros, not stale values
    renderer._begin().mcmc_regularize(renderer._grads, lo / n, ls / (3 * n))   # double here, rounded once to float at the call


class MCMCController:
    """The MCMC schedule for train.trainStep(..., density=controller): the same two hooks as density.DensityController.  Iterations count
    from 1:
      the regulariser gradients are added in every iteration, between the backward and the update;
      relocate, then grow, run after the step of iteration it when from_iter <= it <= until_iter and it % interval == 0;
      noise is injected after the step of EVERY iteration, with lr = noise_lr * the optimiser's current rate of the means (means_lr
      when there is no optimiser: the SGD rate).
    The defaults are the paper's: from 500, until 25 000, every 100, noise_lr 5e5, both regularisers 0.01, growth 1.05.  All arguments
    are validated here, on the host."""

    def __init__(self, *, cap_max, means_lr=None, noise_lr=5e5, from_iter: int = 500, until_iter: int = 25000, interval: int = 100,
                 min_opacity=0.005, opacity_reg=0.01, scale_reg=0.01, growth=1.05, generator=None):
        for name, v, lo in (("cap_max", cap_max, 1), ("from_iter", from_iter, 0), ("until_iter", until_iter, 0), ("interval", interval, 1)):
            integer("MCMCController", name, v, lo, strict=True)
        if until_iter < from_iter:
            raise ValueError(f"MCMCController: until_iter ({until_iter}) lies before from_iter ({from_iter})")
        self.cap_max = cap_max
        self.means_lr = None if means_lr is None else positive("density: means_lr", means_lr, allow_zero=True)
        self.noise_lr = positive("density: noise_lr", noise_lr, allow_zero=True)
        self.min_opacity = probability("density: min_opacity", min_opacity)
        self.opacity_reg = positive("density: opacity_reg", opacity_reg, allow_zero=True)
        self.scale_reg = positive("density: scale_reg", scale_reg, allow_zero=True)
        self.growth = positive("density: growth", growth)
        if self.growth < 1.0:
            raise ValueError(f"MCMCController: growth must be >= 1, got {self.growth}")
        self.from_iter, self.until_iter, self.interval, self.generator = from_iter, until_iter, interval, generator
        self.iteration = 0                                      # completed iterations
        self.history = []                                       # (iteration, dict(alive, dead, relocated, n, added, relocate_src, grow_src)) of every interval

    def refine_due(self, it: int) -> bool:
        return self.from_iter <= it <= self.until_iter and it >= 1 and it % self.interval == 0

    def _noise_rate(self, optimizer) -> float:
        if optimizer is not None:
            return self.noise_lr * float(optimizer.lr["means"])
        if self.means_lr is not None:
            return self.noise_lr * self.means_lr
        raise ValueError("MCMCController: the noise needs the rate of the means: pass optimizer= to trainStep, or means_lr= here for SGD")

    # -- the two hooks of train.trainStep
    def accumulate(self, renderer):
        """Between backward and the optimiser step: the regularisers' gradients join the loss's."""
        regularize(renderer, opacity_reg=self.opacity_reg, scale_reg=self.scale_reg)

    def after_step(self, renderer, optimizer=None):
        """After the optimiser step: counts the iteration, relocates and grows when due, injects the noise.  Returns the counts or None."""
        rate = self._noise_rate(optimizer)
        self.iteration += 1
        it, out = self.iteration, None
        if self.refine_due(it):
            rel = relocate(renderer, optimizer, min_opacity=self.min_opacity, generator=self.generator)
            gr = grow(renderer, optimizer, cap_max=self.cap_max, growth=self.growth, min_opacity=self.min_opacity, generator=self.generator)
            out = dict(alive=rel["alive"], dead=rel["dead"], relocated=rel["relocated"], n=gr["n"], added=gr["added"],
                       relocate_src=rel["src"], grow_src=gr["src"])
            self.history.append((it, out))
        inject_noise(renderer, rate, generator=self.generator)
        return out
