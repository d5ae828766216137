"""Host-side mirror of the reference's loss and training step (src/loss.jl, src/train.jl).

`kernelWindow`, `getLossFunction` and `train` keep the reference's names and argument meaning.
The reference's loop is stale (it needs an AD package that is not in its Manifest and its
backward/SGD lines are commented out, train.jl:39-46); what it intends is implemented:

    preprocess -> compactIdxs -> forward -> loss + dL/dimage -> backward -> param .-= lr*grad -> resetGrads

with the loss, its image gradient and the SGD update running on the GPU (csrc/gs_loss.hip) so the
step has no host round trip.  `optimizer=optim.Adam(...)` replaces the SGD update by Adam with per-group rates
(csrc/gs_adam.hip; fused with the backward when the optimiser was made with fused=True).  `density=density.DensityController(...)`
adds the other half of the 3DGS recipe: statistics after every backward, clone / split / prune and the opacity reset on schedule.
`sh_schedule=SHDegreeSchedule(...)` is the recipe's SH degree schedule: band 0 first, one more band every `every` iterations.
`background=(r, g, b)` or `background=RandomBackground(...)` renders and trains over that colour; an RGBA target is composited over it.
`evaluator=Evaluator(cameras, targets, every)` (train) measures held-out views every `every` iterations: PSNR, MAE and the standard SSIM
(metrics.evaluate, csrc/gs_metrics.hip), without changing what the iterations compute.
`exposure=appearance.Exposure(...)` with `view=v` puts the per-view exposure stage between the frame and the loss: a learned 3 x 4 colour
affine per training view and per-view pixel weights (csrc/gs_exposure.hip); the optimisers see its d_img where they saw the loss's.
`bilagrid=appearance.BilateralGrid(...)` with `view=v` puts a per-view bilateral grid there instead: a lattice of such affines indexed by
pixel position and luminance, for what changes across a photograph (csrc/gs_bilagrid.hip).
"""
from __future__ import annotations

import numpy as np

from . import renderer as R
from ._checks import integer


def kernelWindow(windowSize: int = 11, σ: float = 1.5) -> np.ndarray:
    """loss.jl:5-12 (host copy for inspection; the kernels rebuild the same window)."""
    c = np.ceil(windowSize / 2.0)
    idx = np.arange(1, windowSize + 1, dtype=np.float64)
    k = np.exp(-np.sqrt((c - idx[:, None]) ** 2 + (c - idx[None, :]) ** 2)) / np.sqrt(2.0 * σ ** 2)
    return (k / k.sum()).astype(np.float32)


class LossFunction:
    """What getLossFunction returns: callable (img, gt) -> loss like the reference's closure
    (loss.jl:60-72), plus .value_and_grad for the training step."""

    def __init__(self, renderer, imSize, windowSize: int, nChannels: int, λ: float = 0.1):
        if windowSize != 11:
            raise NotImplementedError("only the reference's windowSize = 11 (loss.jl:14) is built")
        self.r, self.λ = renderer, float(λ)
        self.W, self.H, self.C = int(imSize[0]), int(imSize[1]), int(nChannels)
        self._dC = None
        self._target = None                 # scratch of compose_target: an RGBA target over the renderer's background

    def compose_target(self, rgba):
        """A straight-alpha target [4, H, W] over the renderer's current background (gs_compose_target, on the GPU): the [3, H, W]
        target the loss compares the frame against.  The result is a scratch tensor kept here and overwritten by the next call."""
        import torch
        dev = self.r.imageData.device
        rgba = R.as_device_tensor(rgba, dev, (4, self.H, self.W), "compose_target: the target")
        if self._target is None:
            self._target = torch.empty((3, self.H, self.W), dtype=torch.float32, device=dev)
        self.r._begin().compose_target(rgba.data_ptr(), self.W, self.H, self._target.data_ptr())
        self._keep_rgba = rgba
        return self._target

    def _ptrs(self, img, gt):
        dev, shape = self.r.imageData.device, (self.C, self.H, self.W)
        return R.as_device_tensor(img, dev, shape, "the loss's image"), R.as_device_tensor(gt, dev, shape, "the loss's target")

    def value_and_grad(self, img, gt, want_loss: bool = True):
        import torch
        img, gt = self._ptrs(img, gt)
        if self._dC is None:
            self._dC = torch.empty_like(img)
        val = self.r._begin().loss_device(img.data_ptr(), gt.data_ptr(), self._dC.data_ptr(), self.W, self.H, self.C, self.λ, want_loss)
        self._keep = (img, gt)
        return val, self._dC

    def __call__(self, img, gt) -> float:
        return self.value_and_grad(img, gt)[0]


def getLossFunction(imSize, windowSize: int, nChannels: int, renderer=None, λ: float = 0.1) -> LossFunction:
    """loss.jl:60-72.  `renderer` supplies the GPU context (the reference's closure captures a CuArray kernel)."""
    if renderer is None:
        raise ValueError("getLossFunction needs the renderer whose GPU context runs the loss kernels")
    return LossFunction(renderer, imSize, windowSize, nChannels, λ)


class SHDegreeSchedule:
    """The SH degree schedule of 3DGS training: iteration `it` (counted from 0) runs at the active degree
    min(max_degree, start + it // every) -- band 0 only at first, one more band every `every` iterations.  The model keeps all its
    bands; the kernels evaluate the active ones and the others get zero gradients (renderer.active_sh_degree).
    max_degree None: the model's own degree.  The object counts the iterations it was applied to (`iteration`), as
    density.DensityController does, so one schedule serves one training run."""

    def __init__(self, every: int = 1000, start: int = 0, max_degree: "int | None" = None):
        integer("SHDegreeSchedule", "every", every, 1)
        if int(start) != start or not 0 <= start <= 3:
            raise ValueError(f"SHDegreeSchedule: start must be in 0..3, not {start!r}")
        if max_degree is not None and (int(max_degree) != max_degree or not 0 <= max_degree <= 3):
            raise ValueError(f"SHDegreeSchedule: max_degree must be None or in 0..3, not {max_degree!r}")
        self.every, self.start = int(every), int(start)
        self.max_degree = None if max_degree is None else int(max_degree)
        self.iteration = 0                                      # iterations the schedule was applied to

    def degree_at(self, iteration: int) -> int:
        """The active degree of iteration `iteration` (from 0); without max_degree capped at 3, and by the model when applied."""
        if iteration < 0:
            raise ValueError("SHDegreeSchedule.degree_at: iteration must be >= 0")
        return min(3 if self.max_degree is None else self.max_degree, self.start + int(iteration) // self.every)

    def apply(self, renderer) -> int:
        """Set the renderer's active degree for the iteration about to run and count it.  Returns the effective degree."""
        if not isinstance(renderer, R.GaussianRenderer3D):
            raise ValueError("SHDegreeSchedule: the SH degree schedule needs a GaussianRenderer3D (the 2-D renderer has colours, not SH)")
        renderer.active_sh_degree = self.degree_at(self.iteration)
        self.iteration += 1
        return renderer.active_sh_degree


class RandomBackground:
    """A fresh random background every iteration, the usual remedy against floaters: numpy.random.default_rng(seed) draws three uniform
    float32 values in [0, 1) per iteration, and the RGBA target is composited over the same colour (trainStep).  The object counts the
    iterations it was applied to (`iteration`), as SHDegreeSchedule does, so one object serves one training run."""

    def __init__(self, seed: int = 0):
        self.seed = seed
        self.rng = np.random.default_rng(seed)
        self.iteration = 0                                      # iterations a colour was drawn for

    def draw(self) -> tuple:
        """The colour of the iteration about to run (three floats that are exact float32 values); counts it."""
        rgb = self.rng.random(3, dtype=np.float32)
        self.iteration += 1
        return (float(rgb[0]), float(rgb[1]), float(rgb[2]))

    def apply(self, renderer) -> tuple:
        """Set the renderer's background for the iteration about to run and count it.  Returns the colour."""
        if not isinstance(renderer, R._Renderer):
            raise ValueError("RandomBackground: apply needs a GaussianRenderer3D or GaussianRenderer2D")
        rgb = self.draw()
        renderer.background = rgb
        return rgb


def _channels(gtimg) -> int:
    shape = getattr(gtimg, "shape", None)
    if shape is None or len(shape) != 3 or int(shape[0]) not in (3, 4):
        raise ValueError("trainStep: with `background` the target must be a [3, H, W] or [4, H, W] image")
    return int(shape[0])


def _pose_step(renderer, pose):
    """backwardCamera on the frame at hand -> the camera's fields -> one step of the pose optimiser."""
    from .camera import camera_param_grads
    H, W = renderer.transmittance.shape
    pose.step(camera_param_grads(pose.camera, W, H, R.backwardCamera(renderer)))


def trainStep(renderer, gtimg, lr: float, lossFunc: LossFunction, camera=None, want_loss: bool = True, fused_sgd: bool = False,
              optimizer=None, density=None, sh_schedule=None, background=None, pose=None, freeze_model: bool = False, exposure=None,
              view=None, bilagrid=None):
    """One iteration of train.jl:33-56 as intended (see module docstring).
    fused_sgd (3-D renderer): backward and the parameter update in one pass (gs_backward_sgd) -- the same parameters bit for
    bit (deterministic mode), but renderer.splatGrads is not filled.
    optimizer (optim.Adam): it does the parameter update instead of SGD and `lr` is ignored -- optimizer.backward_step when it
    was made with fused=True (renderer.splatGrads then is not filled), else backward, optimizer.step() and resetGrads.
    density (density.DensityController): its statistics are accumulated between the backward and the update (the update drops the
    frame, so this is the only place), and after the update it clones / splits / prunes and resets opacities when its schedule says so.
    The fused forms leave no frame to accumulate from: a fused optimiser or fused_sgd with `density` is a ValueError.
    density may also be an mcmc.MCMCController, the other strategy, through the same two hooks: between the backward and the update it adds
    the gradients of its opacity and scale regularisers, after the update it relocates dead gaussians and grows the model when its schedule
    says so and injects its noise into the means, every iteration (rate: noise_lr times the optimiser's rate of the means; SGD: its means_lr).
    sh_schedule (SHDegreeSchedule, 3-D renderer): sets the active SH degree of this iteration before preprocess; every optimiser form,
    the fused ones included, and density control run under it unchanged (the request survives a restructured model).
    background: None leaves the renderer's background as it is; (r, g, b) sets it; a RandomBackground draws this iteration's colour and
    sets it, before preprocess.  A [4, H, W] target (straight alpha) is composited over the renderer's current background before the
    loss (lossFunc.compose_target), a [3, H, W] one is used as it is -- so a RandomBackground with a 3-channel target is a ValueError:
    the target could not follow the colour.  Every optimiser form, density control and the SH schedule run unchanged under it.
    pose (optim.CameraAdam, 3-D renderer): the iteration renders under pose.camera; after the unfused backward and before the parameter
    update (the camera gradient is recomputed from the resident model, so this is the only place) it takes renderer.backwardCamera,
    chains it to the camera's fields (camera.camera_param_grads) and steps the pose.  The fused forms leave no frame: a ValueError, as
    with density control; so is an explicit `camera` beside it.  None: the same calls in the same order as without the argument.
    freeze_model: no parameter update (the gradients are still reset) -- with `pose`, registering a view against a trained model.
    exposure (appearance.Exposure) with view (its row): after the forward the frame goes through exposure.apply(view, imageData); the
    target, composed as above, through exposure.mask_target; the loss compares the two; exposure.backward(view, dC) turns the loss's image
    gradient into the frame's, in place, and keeps the row's gradient; exposure.step(view) steps the row; the rest of the iteration is
    the one above on that gradient, so every optimiser form, the fused ones included, density control, the SH schedule, the backgrounds,
    pose and freeze_model run unchanged.  One without the other, or a view out of range, is a ValueError.  None: the same calls in the
    same order as without the arguments.
    bilagrid (appearance.BilateralGrid) with view (its grid): the same stage with a per-view bilateral grid in the place of the affine --
    apply, mask_target, backward (which also adds the grid's total-variation gradient) and step, exactly where exposure's sit.  The two are
    alternatives: both at once is a ValueError, and so is one of bilagrid and view without the other."""
    fused = fused_sgd or (optimizer is not None and optimizer.fused)        # a fused form is in use: no frame is left behind the backward
    if exposure is not None and bilagrid is not None:
        raise ValueError("trainStep: exposure and bilagrid are alternatives (one appearance stage between the frame and the loss)")
    appearance = exposure if exposure is not None else bilagrid              # the stage of this iteration, or None
    if (appearance is None) != (view is None):
        if bilagrid is None:
            raise ValueError("trainStep: exposure and view go together (the view names the row of the exposure table)")
        raise ValueError("trainStep: bilagrid and view go together (the view names the grid of the table)")
    if appearance is not None:
        view = appearance._view(view)
    if pose is not None and camera is not None:
        raise ValueError("trainStep: camera and pose exclude each other (the iteration renders under pose.camera)")
    if pose is not None and fused:
        raise ValueError("trainStep: pose refinement needs the unfused backward (no fused_sgd, no Adam(fused=True)): "
                         "the fused forms leave no frame to take the camera gradient from")
    if freeze_model and fused:
        raise ValueError("trainStep: freeze_model needs the unfused backward (no fused_sgd, no Adam(fused=True)): "
                         "the fused forms step the model inside the backward")
    if pose is not None:
        camera = pose.camera
    if isinstance(background, RandomBackground) and _channels(gtimg) != 4:
        raise ValueError("trainStep: a RandomBackground needs a [4, H, W] target (RGBA, straight alpha): a 3-channel target "
                         "could not follow the colour")
    if optimizer is not None and fused_sgd:
        raise ValueError("trainStep: fused_sgd and optimizer exclude each other (make the optimiser with fused=True instead)")
    if density is not None and fused:
        raise ValueError("trainStep: density control needs the unfused backward (no fused_sgd, no Adam(fused=True)): "
                         "the fused forms leave no frame to accumulate statistics from")
    if sh_schedule is not None:
        sh_schedule.apply(renderer)
    if isinstance(background, RandomBackground):
        background.apply(renderer)
    elif background is not None:
        renderer.background = background
    R.renderFrame(renderer, camera)
    if getattr(gtimg, "ndim", 0) == 3 and gtimg.shape[0] == 4:
        gtimg = lossFunc.compose_target(gtimg)
    if appearance is None:
        loss, ΔC = lossFunc.value_and_grad(renderer.imageData, gtimg, want_loss)
    else:
        adjusted = appearance.apply(view, renderer.imageData)
        loss, ΔC = lossFunc.value_and_grad(adjusted, appearance.mask_target(view, gtimg), want_loss)
        ΔC = appearance.backward(view, ΔC)
        appearance.step(view)
    if fused:                                                    # backward and update in one pass: renderer.splatGrads is not filled
        if optimizer is not None:
            optimizer.backward_step(ΔC)
        else:
            renderer._dC_keepalive = ΔC
            renderer._begin().backward_sgd(ΔC.data_ptr(), float(lr))
        return loss
    R.backward(renderer, ΔC)
    if pose is not None:
        _pose_step(renderer, pose)
    if density is not None:
        density.accumulate(renderer)
    if not freeze_model and optimizer is not None:
        optimizer.step()
    elif not freeze_model:
        renderer._begin().sgd_step(float(lr), renderer._grads)   # param .-= lr * Δparam (train.jl:42-46)
    R.resetGrads(renderer)                                       # train.jl:55
    if density is not None:
        density.after_step(renderer, optimizer)
    return loss


class Evaluator:
    """Held-out views evaluated during a training run: every `every` iterations train() renders `cameras` and compares them with
    `targets` (metrics.evaluate: PSNR, MAE and the standard SSIM in double on the GPU) and appends (iteration, mean Metrics) to
    `history`.  cameras: one Camera per target (None for the 2-D renderer); targets: [3, H, W] or RGBA [4, H, W] images; weights:
    None or one [H, W] array or None per view; background: the colour to evaluate over (None: the renderer's current one).  Give the
    evaluation cameras ids of their own: the id names the view slot, and the training views keep their launch-order history."""

    def __init__(self, cameras, targets, every: int, weights=None, background=None):
        integer("Evaluator", "every", every, 1)
        self.targets = list(targets)
        V = len(self.targets)
        self.cameras = [None] * V if cameras is None else list(cameras)
        self.weights = None if weights is None else list(weights)
        if len(self.cameras) != V:
            raise ValueError(f"Evaluator: {len(self.cameras)} cameras for {V} targets")
        if self.weights is not None and len(self.weights) != V:
            raise ValueError(f"Evaluator: {len(self.weights)} weights for {V} targets")
        self.every, self.background = int(every), background
        self.history = []                                       # (iteration, metrics.Metrics: the mean over the views)

    def due(self, iteration: int) -> bool:
        """After iteration `iteration` (from 0): every `every`-th one."""
        return (int(iteration) + 1) % self.every == 0

    def run(self, renderer, iteration: int):
        """Evaluate now and record the mean under `iteration`.  Returns the metrics.EvalResult."""
        from .metrics import evaluate
        res = evaluate(renderer, self.cameras, self.targets, self.weights, self.background)
        self.history.append((int(iteration), res.mean))
        return res


def train(renderer, gtimg, lr: float, lossFunc: LossFunction, iterations: int = 100, camera=None, log_every: int = 0, optimizer=None,
          density=None, sh_schedule=None, background=None, pose=None, freeze_model: bool = False, evaluator=None, exposure=None, view=None,
          bilagrid=None):
    """train.jl:16-59 without the GUI; the reference loops `while score < 0.99` on a score it never updates.
    optimizer: an optim.Adam that replaces the SGD update (lr is then ignored); density: a density.DensityController,
    sh_schedule: an SHDegreeSchedule, background: a colour or a RandomBackground, pose: an optim.CameraAdam that refines the view,
    freeze_model: no parameter update -- with `pose`, pose refinement against a trained model (trainStep).
    evaluator: an Evaluator; after iteration `it` with (it + 1) % evaluator.every == 0 its views are rendered and measured
    (evaluator.history).  The evaluation leaves the renderer's camera, background and active SH degree as they were; None: the same
    calls in the same order as without the argument.
    exposure, view: an appearance.Exposure and the row of this target's view (trainStep); the evaluator's views are measured without it.
    bilagrid: an appearance.BilateralGrid in the place of exposure (trainStep); the evaluator's views get no grid either."""
    losses = []
    for it in range(iterations):
        l = trainStep(renderer, gtimg, lr, lossFunc, camera, want_loss=True, optimizer=optimizer, density=density, sh_schedule=sh_schedule,
                      background=background, pose=pose, freeze_model=freeze_model, exposure=exposure, view=view, bilagrid=bilagrid)
        losses.append(l)
        if log_every and it % log_every == 0:
            print(f"loss : {l}")                             # loss.jl:69
        if evaluator is not None and evaluator.due(it):
            evaluator.run(renderer, it)
    return losses
