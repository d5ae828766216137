"""Adam on the device (gs_adam_step / gs_backward_adam), with per-group learning rates.

The reference steps with plain SGD, one rate for everything (train.jl:42-46: `param .-= lr*Δparam`).  3-D splats live on very
different scales (world-unit means, log scales, raw quaternions, logit opacities, SH band 0 vs the higher bands), so every 3DGS
trainer uses Adam with rates that span about three orders of magnitude.  torch.optim.Adam cannot stand in: the SH band-0 and
higher-band coefficients are interleaved inside one [n, 3K] row, so they cannot be two torch parameter groups.

    opt = Adam.for_3dgs(renderer, scene_extent)          # or Adam(renderer, lr=1e-3 | {group: rate}, ...)
    train.trainStep(renderer, gt, 0.0, loss, camera, optimizer=opt)

The optimiser owns two flat moment buffers in the initGrads layout ([means | scales | quats | opacities | shs], the buffer
distributed.multi_view_step returns) and the step count; the model is updated in place on the device.
"""
from __future__ import annotations

import math

from . import backend as B
from . import renderer as R
from ._checks import betas_eps, integer, positive

GROUPS_3D = ("means", "scales", "quaternions", "opacities", "sh_dc", "sh_rest")
GROUPS_2D = ("means", "scales", "rotations", "opacities", "colors")     # colors -> lr[4]; lr[5] unused


def _is_2d(renderer) -> bool:
    return isinstance(renderer, R.GaussianRenderer2D)


def _check_rate(name: str, value) -> float:
    return positive(f"Adam: lr[{name!r}]", value, allow_zero=True)


class ExponentialLR:
    """ExponentialLR(lr_init, lr_final, max_steps, delay_steps=0, delay_mult=1.0): the 3DGS recipe's log-linear decay, callable as lr(step).

        t = clip(step / max_steps, 0, 1);   lr = exp((1 - t) log lr_init + t log lr_final)
        times  delay_mult + (1 - delay_mult) sin(pi / 2 clip(step / delay_steps, 0, 1))  when delay_steps > 0

    0 for a negative step, or when both rates are 0.  Pure host arithmetic in double: for Adam.set_lr(means=lr(it)) -- the decay of the
    position rate -- and appearance.Exposure.set_lr(lr(it)) alike."""

    def __init__(self, lr_init: float, lr_final: float, max_steps: int, delay_steps: int = 0, delay_mult: float = 1.0):
        self.lr_init, self.lr_final = _check_rate("lr_init", lr_init), _check_rate("lr_final", lr_final)
        if (self.lr_init == 0.0) != (self.lr_final == 0.0):
            raise ValueError("ExponentialLR: lr_init and lr_final must both be > 0, or both 0 (a log-linear decay cannot reach or leave 0)")
        self.max_steps, self.delay_steps = integer("ExponentialLR", "max_steps", max_steps, 1), integer("ExponentialLR", "delay_steps", delay_steps, 0)
        self.delay_mult = float(delay_mult)
        if not math.isfinite(self.delay_mult) or self.delay_mult < 0.0:
            raise ValueError(f"ExponentialLR: delay_mult must be finite and >= 0, got {delay_mult!r}")

    def __call__(self, step) -> float:
        if step < 0 or (self.lr_init == 0.0 and self.lr_final == 0.0):
            return 0.0
        t = min(max(step / self.max_steps, 0.0), 1.0)
        lr = math.exp((1.0 - t) * math.log(self.lr_init) + t * math.log(self.lr_final))
        if self.delay_steps > 0:
            lr *= self.delay_mult + (1.0 - self.delay_mult) * math.sin(0.5 * math.pi * min(max(step / self.delay_steps, 0.0), 1.0))
        return lr


class Adam:
    """Adam(renderer, lr, betas=(0.9, 0.999), eps=1e-8, selective=False, fused=False).

    lr: one rate for every group, or a dict with one rate per group -- 3-D: means, scales, quaternions, opacities, sh_dc (SH band 0,
    the first three floats of a shs row), sh_rest (the higher bands); 2-D renderer: means, scales, rotations, opacities, colors.
    selective: step only the gaussians with a non-zero gradient float (gs_adam_step's GS_ADAM_SELECTIVE).
    fused (3-D): train.trainStep runs backward_step, the backward and the step in one pass (gs_backward_adam).
    The rates may be changed between steps (set_lr), e.g. the exponential decay of the position rate."""

    def __init__(self, renderer, lr=1e-3, betas=(0.9, 0.999), eps: float = 1e-8, selective: bool = False, fused: bool = False):
        self.renderer = renderer
        self.is_2d = _is_2d(renderer)
        self.groups = GROUPS_2D if self.is_2d else GROUPS_3D
        self.lr = self._rates(lr)
        self.betas, self.eps = betas_eps("Adam", betas, eps)
        if fused and self.is_2d:
            raise ValueError("Adam: fused=True needs the 3-D renderer (gs_backward_adam)")
        self.selective, self.fused = bool(selective), bool(fused)
        self.step_count = 0
        import torch
        flat = renderer._splatGrads.flat
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        # floats from the start of the flat buffer to each of the five arrays, and its length (the initGrads layout)
        self._offsets, self._numel = R.layout_of(renderer._splatGrads)

    @classmethod
    def for_3dgs(cls, renderer, scene_extent: float, selective: bool = False, fused: bool = False) -> "Adam":
        """The 3DGS defaults (Kerbl et al. 2023): position rate scaled by the scene extent, eps 1e-15."""
        lr = dict(means=1.6e-4 * float(scene_extent), scales=5e-3, quaternions=1e-3, opacities=5e-2, sh_dc=2.5e-3, sh_rest=1.25e-4)
        return cls(renderer, lr, betas=(0.9, 0.999), eps=1e-15, selective=selective, fused=fused)

    # -- rates
    def _rates(self, lr) -> dict:
        if isinstance(lr, dict):
            unknown = sorted(set(lr) - set(self.groups))
            if unknown:
                raise ValueError(f"Adam: unknown parameter groups {unknown}; the groups are {list(self.groups)}")
            missing = [k for k in self.groups if k not in lr]
            if missing:
                raise ValueError(f"Adam: no rate for the groups {missing}")
            return {k: _check_rate(k, lr[k]) for k in self.groups}
        v = _check_rate("*", lr)
        return {k: v for k in self.groups}

    def set_lr(self, lr=None, **rates):
        """Replace every rate (lr: a number or a full dict) and/or some of them by name: set_lr(means=1e-5)."""
        new = self._rates(lr) if lr is not None else dict(self.lr)
        for k, v in rates.items():
            if k not in self.groups:
                raise ValueError(f"Adam: unknown parameter group {k!r}; the groups are {list(self.groups)}")
            new[k] = _check_rate(k, v)
        self.lr = new

    def lr_vector(self) -> list:
        """The GS_ADAM_GROUPS rates of the C ABI (2-D: lr[5] unused, 0)."""
        v = [self.lr[k] for k in self.groups]
        return v + [0.0] * (B.GS_ADAM_GROUPS - len(v))

    # -- the buffers of the C ABI
    def _struct(self, flat) -> B.GsGrads:
        return R.grads_struct(flat, self._offsets)

    def moment_structs(self) -> list:
        """[exp_avg, exp_avg_sq] as the gradient-shaped companion sets of a call that moves rows (density, mcmc)."""
        return [self._struct(self.exp_avg), self._struct(self.exp_avg_sq)]

    def moment_ptrs(self, group: str) -> tuple:
        """(exp_avg, exp_avg_sq) device pointers of one parameter group's array (sh_dc and sh_rest share the SH rows)."""
        o = 4 * self._offsets[min(self.groups.index(group), 4)]
        return self.exp_avg.data_ptr() + o, self.exp_avg_sq.data_ptr() + o

    def _grads_struct(self, grads) -> B.GsGrads:
        import torch
        if grads is None:
            self.renderer.splatGrads                       # a pending resetGrads zero-fills here: the step sees zeros, not stale values
            return self.renderer._grads
        if isinstance(grads, B.GsGrads):
            return grads
        if isinstance(grads, torch.Tensor):                # a flat buffer in the initGrads layout (distributed.multi_view_step)
            if grads.numel() != self._numel or grads.dtype != torch.float32 or not grads.is_contiguous() or grads.device != self.exp_avg.device:
                raise ValueError("Adam.step: grads must be a contiguous float32 flat gradient buffer of the renderer's layout on its device")
            self._keep = grads
            return self._struct(grads)
        flat = getattr(grads, "flat", None)                # SplatGrads3D / SplatGrads2D
        if flat is not None:
            return self._grads_struct(flat)
        raise TypeError("Adam.step: grads must be None, a flat tensor, a SplatGrads3D / 2D or a backend.GsGrads")

    # -- steps
    def _step_args(self) -> tuple:
        """What gs_adam_step and gs_backward_adam take behind the gradients: moments, rates, betas, eps and the number of the step about to run."""
        return (self._struct(self.exp_avg), self._struct(self.exp_avg_sq), self.lr_vector(), self.betas[0], self.betas[1], self.eps,
                self.step_count + 1)

    def step(self, grads=None):
        """One Adam step from `grads` (default renderer.splatGrads); the model is updated in place on the device."""
        g = self._grads_struct(grads)
        self.renderer._begin().adam_step(g, *self._step_args(), selective=self.selective)
        self.step_count += 1

    def backward_step(self, dC):
        """Backward of the current frame and the Adam step in one pass (gs_backward_adam, 3-D renderer).  renderer.splatGrads is
        not filled."""
        r = self.renderer
        if self.is_2d:
            raise ValueError("Adam.backward_step needs the 3-D renderer (gs_backward_adam)")
        d = R.as_device_tensor(dC, r.imageData.device, r.imageData.shape, "Adam.backward_step: dC")
        r._dC_keepalive = d
        r._begin().backward_adam(d.data_ptr(), *self._step_args(), selective=self.selective)
        self.step_count += 1

    # -- the number of gaussians changes (renderer.adopt_model): moment buffers of the new size first, _rebind once the renderer has adopted
    def resized_moments(self, n_out: int, zero: bool, keep_rows: int = 0) -> tuple:
        """(exp_avg, exp_avg_sq, structs) for a model of n_out gaussians: two flat buffers in the layout the renderer's gradient buffer
        will have -- zeros, or uninitialised for a call that writes every row -- and their gs_grads.  keep_rows: that many leading rows
        of every array are copied from the present moments, on the device."""
        import torch
        widths = [v.shape[1] for v in R.grads_views(self.renderer._splatGrads)]
        offsets, total = R.grads_layout(widths, n_out)
        make = torch.zeros if zero else torch.empty
        new = [make(total, dtype=self.exp_avg.dtype, device=self.exp_avg.device) for _ in range(2)]
        for old, m in zip((self.exp_avg, self.exp_avg_sq), new) if keep_rows else ():
            for o_old, o_new, w in zip(self._offsets, offsets, widths):
                m[o_new:o_new + keep_rows * w].copy_(old[o_old:o_old + keep_rows * w])
        return new[0], new[1], [R.grads_struct(m, offsets) for m in new]

    def _rebind(self, exp_avg, exp_avg_sq):
        """The renderer adopted a model of another size: take the moment buffers made for it and its gradient buffer's layout.
        step_count stays: the bias corrections are a property of the run."""
        flat = self.renderer._splatGrads.flat
        for t in (exp_avg, exp_avg_sq):
            if t.numel() != flat.numel() or t.dtype != flat.dtype or t.device != flat.device or not t.is_contiguous():
                raise ValueError("Adam._rebind: the moment buffers must match the renderer's flat gradient buffer")
        self._offsets, self._numel = R.layout_of(self.renderer._splatGrads)
        self.exp_avg, self.exp_avg_sq = exp_avg, exp_avg_sq

    # -- checkpoints
    def state_dict(self) -> dict:
        return dict(step=self.step_count, lr=dict(self.lr), betas=tuple(self.betas), eps=self.eps, selective=self.selective,
                    fused=self.fused, exp_avg=self.exp_avg.detach().clone(), exp_avg_sq=self.exp_avg_sq.detach().clone())

    def load_state_dict(self, state: dict):
        import torch
        for k in ("exp_avg", "exp_avg_sq"):
            t = state[k]
            if not isinstance(t, torch.Tensor) or t.numel() != self._numel:
                raise ValueError(f"Adam.load_state_dict: {k} does not match this renderer's gradient layout ({self._numel} floats)")
        step = int(state["step"])
        if step < 0:
            raise ValueError("Adam.load_state_dict: negative step")
        lr = self._rates(state["lr"])
        betas, eps = betas_eps("Adam.load_state_dict", state["betas"], state["eps"], got=False)
        self.exp_avg.copy_(state["exp_avg"].reshape(-1))
        self.exp_avg_sq.copy_(state["exp_avg_sq"].reshape(-1))
        self.step_count, self.lr, self.betas, self.eps = step, lr, betas, eps
        self.selective = bool(state.get("selective", self.selective))


class CameraAdam:
    """CameraAdam(camera, lr_eye, lr_lookat, lr_focal=0.0, betas=(0.9, 0.999), eps=1e-8): Adam on a view's eye, lookAt and (lr_focal != 0)
    fx, fy -- pose refinement against a trained model, or beside its training (train.trainStep(..., pose=...)).  Nine numbers do not need a
    kernel: the state is float64 on the host.  `.camera` is the current Camera (float32 fields; up, near, far, id as given: they are not
    optimised); `.step(param_grads)` takes what camera.camera_param_grads returns."""

    def __init__(self, camera, lr_eye: float, lr_lookat: float, lr_focal: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8):
        import numpy as np
        self.lr = dict(eye=_check_rate("eye", lr_eye), lookAt=_check_rate("lookAt", lr_lookat), focal=_check_rate("focal", lr_focal))
        self.betas, self.eps = betas_eps("CameraAdam", betas, eps)
        self._template = camera
        # the parameter vector: eye[3], lookAt[3], fx, fy
        self.x = np.concatenate([np.asarray(camera.eye, np.float64).reshape(3), np.asarray(camera.lookAt, np.float64).reshape(3),
                                 np.array([camera.fx, camera.fy], np.float64)])
        if not np.isfinite(self.x).all():
            raise ValueError("CameraAdam: the camera's eye, lookAt, fx and fy must be finite")
        self.m = np.zeros(8, np.float64)
        self.v = np.zeros(8, np.float64)
        self.step_count = 0
        self._camera = None

    def _rates(self):
        import numpy as np
        return np.array([self.lr["eye"]] * 3 + [self.lr["lookAt"]] * 3 + [self.lr["focal"]] * 2, np.float64)

    @property
    def camera(self):
        """The current Camera: float32 eye and lookAt, fx and fy rounded to float32; one object until the next step."""
        if self._camera is None:
            import dataclasses
            import numpy as np
            self._camera = dataclasses.replace(self._template, eye=self.x[0:3].astype(np.float32), lookAt=self.x[3:6].astype(np.float32),
                                               fx=float(np.float32(self.x[6])), fy=float(np.float32(self.x[7])))
        return self._camera

    def step(self, param_grads: dict):
        """One Adam step from dict(eye, lookAt, fx, fy) (camera.camera_param_grads; `up` is ignored)."""
        import numpy as np
        g = np.concatenate([np.asarray(param_grads["eye"], np.float64).reshape(3), np.asarray(param_grads["lookAt"], np.float64).reshape(3),
                            np.array([param_grads["fx"], param_grads["fy"]], np.float64).reshape(2)])
        if not np.isfinite(g).all():
            raise ValueError("CameraAdam.step: a gradient is not finite")
        b1, b2 = self.betas
        t = self.step_count + 1
        self.m = b1 * self.m + (1.0 - b1) * g
        self.v = b2 * self.v + (1.0 - b2) * (g * g)
        mhat = self.m / (1.0 - b1 ** t)
        vhat = self.v / (1.0 - b2 ** t)
        self.x = self.x - self._rates() * (mhat / (np.sqrt(vhat) + self.eps))
        self.step_count = t
        self._camera = None
