"""Density control on the device: the half of the 3DGS recipe (Kerbl et al. 2023) that changes the number of gaussians.

    stats = DensityStats(renderer)
    ... per iteration, between backward(renderer, dC) and optimizer.step():   stats.accumulate()
    ... every hundred iterations:   densify_and_prune(renderer, stats, optimizer, scene_extent=extent)
    ... every three thousand:       reset_opacity(renderer, optimizer)

or `train.trainStep(..., density=DensityController(scene_extent=extent))`, which carries that schedule.

Everything runs in the HIP library (csrc/gs_density.hip; semantics in include/gsplat.h and DESIGN.md 5.8b): the screen-space positional
gradient never leaves it, the decision is a comparison of stored numbers against thresholds this module converts to log / logit space
once, and the model, the gradient buffer and Adam's moments are rebuilt in one ordered pass -- survivors, then clones, then the two
children of every split.  torch allocates the new arrays and draws the normals of the split (so the caller's generator decides them);
the kernels are pure functions of their inputs.

Not covered: accumulation inside the fused backwards (Adam(fused=True), fused_sgd: they leave no frame to accumulate from), multi-GPU
restructuring (it is deterministic given equal noise, so replicated ranks may each run it with generators seeded alike), and the 2-D
renderer (the library answers GS_ERR_UNSUPPORTED).
"""
from __future__ import annotations

import math

from . import backend as B
from . import renderer as R
from ._checks import integer, logit, positive, probability  # noqa: F401  (logit: imported from here by callers)

LOG_SHRINK_3DGS = math.log(1.6)         # the children of a split are 1.6 times smaller


def density_params(*, scene_extent, grad_threshold=2e-4, percent_dense=0.01, min_opacity=0.005, max_world_fraction=0.1,
                   max_extent_px=0, log_shrink=LOG_SHRINK_3DGS) -> B.GsDensityParams:
    """The thresholds of gs_density_decide from the 3DGS hyper-parameters: a densified gaussian is split when its largest scale exceeds
    percent_dense * scene_extent (else cloned); a gaussian is pruned below min_opacity, above max_extent_px pixels (0: off) or when
    the scale it would keep exceeds max_world_fraction * scene_extent (None: off).  grad_threshold = inf turns densification off."""
    extent = positive("density: scene_extent", scene_extent)
    gt = float(grad_threshold)
    if math.isnan(gt) or gt < 0.0:
        raise ValueError(f"density: grad_threshold must be >= 0 (inf: no densification), got {gt}")
    pd = positive("density: percent_dense", percent_dense)
    mo = probability("density: min_opacity", min_opacity)
    if max_world_fraction is not None:
        mw = positive("density: max_world_fraction", max_world_fraction)
    px = int(max_extent_px)
    if px < 0:
        raise ValueError(f"density: max_extent_px must be >= 0 (0: off), got {px}")
    ls = float(log_shrink)
    if not math.isfinite(ls):
        raise ValueError(f"density: log_shrink must be finite, got {ls}")
    return B.GsDensityParams(struct_size=B.C.sizeof(B.GsDensityParams), grad_threshold=gt, log_split_scale=math.log(pd * extent), log_shrink=ls,
                             min_opacity_logit=logit(mo), log_max_world_scale=math.inf if max_world_fraction is None else math.log(mw * extent),
                             max_extent_px=px)


class DensityStats:
    """Three device tensors of one element per gaussian -- grad_sum (float32: sum over the accumulated views of |d L / d mu'| in NDC
    units), count (int32: views in which the gaussian was visible), max_extent (int32: its largest pixel extent) -- and the two calls
    that maintain them.  accumulate() belongs between backward and the optimiser step: the step drops the frame."""

    def __init__(self, renderer):
        R.require_3d(renderer, "DensityStats")
        self.renderer = renderer
        self.resize(renderer.nGaussians)

    def resize(self, n: int):
        import torch
        dev = self.renderer.imageData.device
        self.grad_sum = torch.zeros(int(n), dtype=torch.float32, device=dev)
        self.count = torch.zeros(int(n), dtype=torch.int32, device=dev)
        self.max_extent = torch.zeros(int(n), dtype=torch.int32, device=dev)

    def reset(self):
        self.grad_sum.zero_(); self.count.zero_(); self.max_extent.zero_()

    def struct(self) -> B.GsDensityStats:
        return B.GsDensityStats(self.grad_sum.data_ptr(), self.count.data_ptr(), self.max_extent.data_ptr())

    def accumulate(self):
        r = self.renderer
        if self.grad_sum.numel() != r.nGaussians:
            raise ValueError("DensityStats.accumulate: the renderer's number of gaussians changed; resize() first")
        r._begin().density_accumulate(self.struct())


def densify_and_prune(renderer, stats: DensityStats, optimizer=None, *, scene_extent, grad_threshold=2e-4, percent_dense=0.01,
                      min_opacity=0.005, max_world_fraction=0.1, max_extent_px=0, generator=None, max_gaussians=None) -> dict:
    """Clone, split and prune by the statistics of the window, on the device; returns dict(survivors, clones, splits, pruned, n).

    The renderer gets new splatData, a fresh zero gradient buffer and the new model; `optimizer` (optim.Adam) gets its moments
    restructured alongside -- rows of survivors carried over, rows of clones and children zero, step_count kept; `stats` is resized and
    zeroed.  If the new size would exceed max_gaussians the decision is made again without densification (pruning only).
    generator: the torch.Generator the normals of the split are drawn from (n x 2 x 3 of them, whatever is split)."""
    import torch
    R.require_3d(renderer, "densify_and_prune")
    renderer.check_resize(optimizer, "densify_and_prune")
    if max_gaussians is not None and int(max_gaussians) < 1:
        raise ValueError(f"density: max_gaussians must be >= 1 or None, got {max_gaussians}")
    kw = dict(scene_extent=scene_extent, percent_dense=percent_dense, min_opacity=min_opacity, max_world_fraction=max_world_fraction,
              max_extent_px=max_extent_px)
    params = density_params(grad_threshold=grad_threshold, **kw)
    n = renderer.nGaussians
    if stats.grad_sum.numel() != n:
        raise ValueError("densify_and_prune: stats do not match the renderer's number of gaussians")
    dev = renderer.splatData.means.device
    ctx = renderer._begin()
    action = torch.empty(n, dtype=torch.int32, device=dev)
    st = stats.struct()
    ctx.density_decide(st, params, action.data_ptr())
    survivors, clones, splits, pruned = ctx.density_plan(action.data_ptr())
    n_out = survivors + clones + 2 * splits
    if max_gaussians is not None and n_out > int(max_gaussians):
        ctx.density_decide(st, density_params(grad_threshold=math.inf, **kw), action.data_ptr())
        survivors, clones, splits, pruned = ctx.density_plan(action.data_ptr())
        n_out = survivors + clones + 2 * splits
    noise = R.draw(torch.randn, (n, 2, 3), generator, dev)
    new = renderer.alloc_model(n_out, zero=False)                # every row is written by the restructure
    src_sets, dst_sets, moments = [], [], ()
    if optimizer is not None:                                   # the flat layout depends on n: the moments move into new flat buffers
        *moments, dst_sets = optimizer.resized_moments(n_out, zero=False)
        src_sets = optimizer.moment_structs()
    ctx.density_restructure(action.data_ptr(), noise.data_ptr(), B.GsGrads(*(t.data_ptr() for t in R.model_arrays(new))), src_sets, dst_sets, n_out)
    renderer.adopt_model(new, "densify_and_prune")
    if optimizer is not None:
        optimizer._rebind(*moments)
    stats.resize(n_out)
    return dict(survivors=survivors, clones=clones, splits=splits, pruned=pruned, n=n_out)


def reset_opacity(renderer, optimizer=None, opacity: float = 0.01):
    """opacity = min(opacity, logit(`opacity`)) on the resident model; the opacities' Adam moments of `optimizer` become zero."""
    R.require_3d(renderer, "reset_opacity")
    p = probability("density: opacity", opacity)
    m = v = 0
    if optimizer is not None:
        if optimizer.renderer is not renderer:
            raise ValueError("reset_opacity: the optimiser belongs to another renderer")
        m, v = optimizer.moment_ptrs("opacities")
    renderer._begin().opacity_reset(logit(p), m, v)


class DensityController:
    """The 3DGS schedule for train.trainStep(..., density=controller).  Iterations count from 1:
      statistics are accumulated in every iteration up to until_iter;
      densify_and_prune runs after the step of iteration it when from_iter <= it <= until_iter and it % interval == 0;
      reset_opacity runs after the step of iteration it when it <= until_iter and it % opacity_reset_interval == 0 (0: never).
    The defaults are the paper's: from 500, until 15 000, every 100, reset every 3 000.  The other arguments are densify_and_prune's
    and reset_opacity's; all are validated here, on the host."""

    def __init__(self, *, scene_extent, from_iter: int = 500, until_iter: int = 15000, interval: int = 100, opacity_reset_interval: int = 3000,
                 reset_opacity_to: float = 0.01, grad_threshold=2e-4, percent_dense=0.01, min_opacity=0.005, max_world_fraction=0.1,
                 max_extent_px: int = 0, max_gaussians=None, generator=None):
        for name, v, lo in (("from_iter", from_iter, 0), ("until_iter", until_iter, 0), ("interval", interval, 1),
                            ("opacity_reset_interval", opacity_reset_interval, 0)):
            integer("DensityController", name, v, lo, strict=True)
        if until_iter < from_iter:
            raise ValueError(f"DensityController: until_iter ({until_iter}) lies before from_iter ({from_iter})")
        if max_gaussians is not None and (isinstance(max_gaussians, bool) or not isinstance(max_gaussians, int) or max_gaussians < 1):
            raise ValueError(f"DensityController: max_gaussians must be an integer >= 1 or None, got {max_gaussians!r}")
        self.kw = dict(scene_extent=scene_extent, grad_threshold=grad_threshold, percent_dense=percent_dense, min_opacity=min_opacity,
                       max_world_fraction=max_world_fraction, max_extent_px=max_extent_px)
        density_params(**self.kw)                               # validates the thresholds
        self.reset_opacity_to = probability("density: reset_opacity_to", reset_opacity_to)
        self.from_iter, self.until_iter, self.interval, self.opacity_reset_interval = from_iter, until_iter, interval, opacity_reset_interval
        self.max_gaussians, self.generator = max_gaussians, generator
        self.iteration = 0                                      # completed iterations
        self.stats = None
        self.history = []                                       # (iteration, counts) of every densify_and_prune

    # -- the schedule (pure functions of the iteration number, counted from 1)
    def wants_stats(self, it: int) -> bool:
        return 1 <= it <= self.until_iter

    def densify_due(self, it: int) -> bool:
        return self.from_iter <= it <= self.until_iter and it >= 1 and it % self.interval == 0

    def reset_due(self, it: int) -> bool:
        return self.opacity_reset_interval > 0 and 1 <= it <= self.until_iter and it % self.opacity_reset_interval == 0

    # -- the two hooks of train.trainStep
    def accumulate(self, renderer):
        """Between backward and the optimiser step of iteration self.iteration + 1."""
        if not self.wants_stats(self.iteration + 1):
            return
        if self.stats is None or self.stats.renderer is not renderer:
            self.stats = DensityStats(renderer)
        self.stats.accumulate()

    def after_step(self, renderer, optimizer=None):
        """After the optimiser step: counts the iteration and restructures / resets when due.  Returns the counts or None."""
        self.iteration += 1
        it, out = self.iteration, None
        if self.densify_due(it) and self.stats is not None:
            out = densify_and_prune(renderer, self.stats, optimizer, generator=self.generator, max_gaussians=self.max_gaussians, **self.kw)
            self.history.append((it, out))
        if self.reset_due(it):
            reset_opacity(renderer, optimizer, self.reset_opacity_to)
        return out
