"""Per-view appearance: a learned 3 x 4 colour affine per training view ("exposure compensation") and per-view pixel weights (masks).

A real capture has auto-exposure and white balance that change from photograph to photograph, and regions that are not to be explained
(sky, people, the rig).  The 3DGS recipe answers with one 3 x 4 affine per training image, learned by Adam beside the model, and with a
mask multiplied into both images before the loss.  Both are one image-space stage between the frame and the loss,

    out = w * (M rgb + b),        E = [M | b], 12 floats per view, starting at [I | 0]

run on the device (csrc/gs_exposure.hip: gs_exposure_apply / gs_exposure_backward / gs_exposure_adam), bitwise reproducible.

    exp = Exposure(renderer, n_views, weights=masks)         # masks: None, or one [H, W] array or None per view
    train.trainStep(renderer, gt, lr, loss, camera, exposure=exp, view=v)
    exp.set_lr(optim.ExponentialLR(0.01, 0.001, 30000)(it))  # the recipe's decay

A view is an independent Adam problem: it has its own step count and is stepped when it is rendered, so a row never drifts on momentum
while other views train.  Held-out views are measured without exposure (train.Evaluator), as the recipe does.

What changes ACROSS a photograph -- vignetting, local tone mapping, a window that blows out one corner -- one affine per view cannot
absorb.  BilateralGrid is the other half: a small 3-D lattice of 3 x 4 affines per view, indexed by pixel position and pixel luminance,
sliced trilinearly per pixel and applied to the rendered colour, with a total-variation term that keeps it smooth
(csrc/gs_bilagrid.hip: gs_bilagrid_apply / gs_bilagrid_backward / gs_bilagrid_tv / gs_bilagrid_adam), bitwise reproducible too.

    grid = BilateralGrid(renderer, n_views, grid=(16, 16, 8))
    train.trainStep(renderer, gt, lr, loss, camera, bilagrid=grid, view=v)      # in the place of exposure=: the two are alternatives
"""
from __future__ import annotations

import numpy as np

from ._checks import betas_eps, integer, positive
from .renderer import as_device_tensor


def _check_lr(lr, who: str = "Exposure") -> float:
    return positive(f"{who}: lr", lr, allow_zero=True)


def _host_weights(who: str, weights, n_views: int, H: int, W: int) -> list:
    """weights as a list of n_views entries, each None or a contiguous [H, W] float32 host array"""
    host_w = [None] * n_views
    if weights is not None:
        weights = list(weights)
        if len(weights) != n_views:
            raise ValueError(f"{who}: {len(weights)} weights for {n_views} views")
        for v, w in enumerate(weights):
            if w is None:
                continue
            a = np.ascontiguousarray(w.detach().cpu().numpy() if hasattr(w, "detach") else w, np.float32)
            if a.shape != (H, W):
                raise ValueError(f"{who}: the weight of view {v} must be [{H}, {W}], not {a.shape}")
            host_w[v] = a
    return host_w


class Exposure:
    """Exposure(renderer, n_views, weights=None, lr=0.01, betas=(0.9, 0.999), eps=1e-15).

    Holds three device [V, 3, 4] float32 tensors -- the table (row v = view v's E, [I | 0] at the start), exp_avg and exp_avg_sq -- and
    one Adam step count per view on the host.  weights: None, or a sequence of n_views entries, each None or an [H, W] array (uploaded
    once).  Argument errors are ValueErrors raised before any GPU call."""

    def __init__(self, renderer, n_views: int, weights=None, lr: float = 0.01, betas=(0.9, 0.999), eps: float = 1e-15):
        self.n_views = integer("Exposure", "n_views", n_views, 1)
        self.lr = _check_lr(lr)
        self.betas, self.eps = betas_eps("Exposure", betas, eps)
        shape = tuple(int(s) for s in renderer.imageData.shape)
        if len(shape) != 3 or shape[0] != 3:
            raise ValueError(f"Exposure: the renderer's image must be [3, H, W], not {shape}")
        self.H, self.W = shape[1], shape[2]
        host_w = _host_weights("Exposure", weights, self.n_views, self.H, self.W)
        # -- everything above needs no device
        import torch
        self.renderer = renderer
        dev = renderer.imageData.device
        ident = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]], dtype=torch.float32, device=dev)
        self.table = ident.repeat(self.n_views, 1, 1).contiguous()
        self.exp_avg = torch.zeros_like(self.table)
        self.exp_avg_sq = torch.zeros_like(self.table)
        self.step_counts = [0] * self.n_views
        self.weights = [None if a is None else torch.tensor(a, dtype=torch.float32, device=dev) for a in host_w]
        self._identity = ident                                  # the resident row of mask_target
        self._grad = torch.zeros(12, dtype=torch.float32, device=dev)
        self._out = None                                        # scratch of apply
        self._masked = None                                     # scratch of mask_target
        self._keep_gt = None                                    # the target of the last mask_target, kept alive behind the asynchronous call
        self._x = None                                          # the image of the last apply: what backward's d_exposure is taken at
        self._x_view = -1
        self._have_grad = -1                                    # the view whose gradient _grad holds (-1: none)

    # -- arguments
    def _view(self, view) -> int:
        if isinstance(view, bool) or view is None or int(view) != view or not 0 <= int(view) < self.n_views:
            raise ValueError(f"Exposure: view must be in 0..{self.n_views - 1}, not {view!r}")
        return int(view)

    def _image(self, img, what: str):
        return as_device_tensor(img, self.table.device, (3, self.H, self.W), f"Exposure.{what}: the image")

    def _wptr(self, v: int) -> int:
        w = self.weights[v]
        return 0 if w is None else w.data_ptr()

    def set_lr(self, lr):
        """The rate of every later step, e.g. optim.ExponentialLR(0.01, 0.001, max_steps)(iteration)."""
        self.lr = _check_lr(lr)

    # -- the stage
    def apply(self, view, img):
        """w * (M img + b) under view `view`'s row and weight: a scratch tensor kept here and overwritten by the next call.  `img` (the
        renderer's imageData in a training step) is what the next backward takes d_exposure at."""
        import torch
        v = self._view(view)
        x = self._image(img, "apply")
        if self._out is None:
            self._out = torch.empty((3, self.H, self.W), dtype=torch.float32, device=self.table.device)
        self.renderer._begin().exposure_apply(x.data_ptr(), self.table[v].data_ptr(), self._wptr(v), self.W, self.H, self._out.data_ptr())
        self._x, self._x_view = x, v
        return self._out

    def backward(self, view, d_out, want_grad: bool = True):
        """The adjoint of the last apply(view, img): returns d_img, written in place into d_out, and (want_grad) keeps the 12-float
        gradient of the row for step()."""
        v = self._view(view)
        if self._x is None or self._x_view != v:
            raise ValueError(f"Exposure.backward: apply(view={v}, img) first")
        d = self._image(d_out, "backward")
        self.renderer._begin().exposure_backward(self._x.data_ptr(), d.data_ptr(), self.table[v].data_ptr(), self._wptr(v), self.W, self.H,
                                                 d.data_ptr(), self._grad.data_ptr() if want_grad else 0)
        if want_grad:
            self._have_grad = v
        return d

    def step(self, view):
        """One Adam step of view `view`'s row from the gradient the last backward kept; the view's own step count advances."""
        v = self._view(view)
        if self._have_grad != v:
            raise ValueError(f"Exposure.step: backward(view={v}, ...) with want_grad first")
        t = self.step_counts[v] + 1
        self.renderer._begin().exposure_adam(self.table[v].data_ptr(), self._grad.data_ptr(), self.exp_avg[v].data_ptr(),
                                             self.exp_avg_sq[v].data_ptr(), self.lr, self.betas[0], self.betas[1], self.eps, t)
        self.step_counts[v] = t
        self._have_grad = -1

    def mask_target(self, view, gt):
        """w * gt for view `view` (gs_exposure_apply with a resident identity row: exact), a scratch tensor overwritten by the next call;
        `gt` itself when the view has no weight."""
        import torch
        v = self._view(view)
        if self.weights[v] is None:
            return gt
        g = self._image(gt, "mask_target")
        if self._masked is None:
            self._masked = torch.empty((3, self.H, self.W), dtype=torch.float32, device=self.table.device)
        self.renderer._begin().exposure_apply(g.data_ptr(), self._identity.data_ptr(), self._wptr(v), self.W, self.H, self._masked.data_ptr())
        self._keep_gt = g
        return self._masked

    def exposure(self, view) -> np.ndarray:
        """View `view`'s row as a 3 x 4 float32 array (one read-back)."""
        return self.table[self._view(view)].detach().cpu().numpy()

    # -- checkpoints
    def state_dict(self) -> dict:
        return dict(table=self.table.detach().clone(), exp_avg=self.exp_avg.detach().clone(), exp_avg_sq=self.exp_avg_sq.detach().clone(),
                    steps=list(self.step_counts), lr=self.lr)

    def load_state_dict(self, state: dict):
        import torch
        shape = (self.n_views, 3, 4)
        for k in ("table", "exp_avg", "exp_avg_sq"):
            t = state[k]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                raise ValueError(f"Exposure.load_state_dict: {k} must be a tensor of shape {shape}")
        steps = [int(s) for s in state["steps"]]
        if len(steps) != self.n_views or min(steps) < 0:
            raise ValueError(f"Exposure.load_state_dict: {self.n_views} step counts >= 0 expected")
        lr = _check_lr(state["lr"])
        for k in ("table", "exp_avg", "exp_avg_sq"):
            getattr(self, k).copy_(state[k])
        self.step_counts, self.lr = steps, lr
        self._have_grad = -1


class BilateralGrid:
    """BilateralGrid(renderer, n_views, grid=(16, 16, 8), weights=None, lr=2e-3, betas=(0.9, 0.999), eps=1e-15, tv_coef=10.0).

    Holds three device [V, Gz, Gy, Gx, 12] float32 tensors -- the table (view v's grid, [I | 0] at every vertex at the start), exp_avg and
    exp_avg_sq -- and one Adam step count per view on the host.  grid = (Gx, Gy, Gz): vertices across the image, down the image and along
    the luminance, each in 1..64.  weights as Exposure's.  tv_coef: backward adds the gradient of tv_coef * tv(grid) to the grid's gradient
    (0: none).  Argument errors are ValueErrors raised before any GPU call."""

    def __init__(self, renderer, n_views: int, grid=(16, 16, 8), weights=None, lr: float = 2e-3, betas=(0.9, 0.999), eps: float = 1e-15,
                 tv_coef: float = 10.0):
        from .backend import GS_BILAGRID_FLOATS, GS_BILAGRID_MAX_DIM
        self.n_views = integer("BilateralGrid", "n_views", n_views, 1)
        if isinstance(grid, (str, bytes)) or len(tuple(grid)) != 3:
            raise ValueError(f"BilateralGrid: grid must be (Gx, Gy, Gz), not {grid!r}")
        self.dims = tuple(integer("BilateralGrid", "grid", g, 1) for g in grid)
        if max(self.dims) > GS_BILAGRID_MAX_DIM:
            raise ValueError(f"BilateralGrid: every grid dimension must be in 1..{GS_BILAGRID_MAX_DIM}, not {self.dims}")
        self.lr = _check_lr(lr, "BilateralGrid")
        self.tv_coef = positive("BilateralGrid: tv_coef", tv_coef, allow_zero=True)
        self.betas, self.eps = betas_eps("BilateralGrid", betas, eps)
        shape = tuple(int(s) for s in renderer.imageData.shape)
        if len(shape) != 3 or shape[0] != 3:
            raise ValueError(f"BilateralGrid: the renderer's image must be [3, H, W], not {shape}")
        self.H, self.W = shape[1], shape[2]
        host_w = _host_weights("BilateralGrid", weights, self.n_views, self.H, self.W)
        # -- everything above needs no device
        import torch
        self.renderer = renderer
        dev = renderer.imageData.device
        gx, gy, gz = self.dims
        self.n_floats = gx * gy * gz * GS_BILAGRID_FLOATS
        ident = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float32, device=dev)
        self._identity = ident.repeat(gz, gy, gx, 1).contiguous()               # the resident grid of mask_target
        self.table = self._identity.repeat(self.n_views, 1, 1, 1, 1).contiguous()
        self.exp_avg = torch.zeros_like(self.table)
        self.exp_avg_sq = torch.zeros_like(self.table)
        self.step_counts = [0] * self.n_views
        self.weights = [None if a is None else torch.tensor(a, dtype=torch.float32, device=dev) for a in host_w]
        self._grad = torch.zeros(self.n_floats, dtype=torch.float32, device=dev)
        self._tv = torch.zeros(1, dtype=torch.float64, device=dev)
        self._out = None                                        # scratch of apply
        self._masked = None                                     # scratch of mask_target
        self._keep_gt = None                                    # the target of the last mask_target, kept alive behind the asynchronous call
        self._x = None                                          # the image of the last apply: what backward's d_grid is taken at
        self._x_view = -1
        self._have_grad = -1                                    # the view whose gradient _grad holds (-1: none)

    # -- arguments
    def _view(self, view) -> int:
        if isinstance(view, bool) or view is None or int(view) != view or not 0 <= int(view) < self.n_views:
            raise ValueError(f"BilateralGrid: view must be in 0..{self.n_views - 1}, not {view!r}")
        return int(view)

    def _image(self, img, what: str):
        return as_device_tensor(img, self.table.device, (3, self.H, self.W), f"BilateralGrid.{what}: the image")

    def _wptr(self, v: int) -> int:
        w = self.weights[v]
        return 0 if w is None else w.data_ptr()

    def set_lr(self, lr):
        """The rate of every later step, e.g. optim.ExponentialLR(2e-3, 2e-5, max_steps)(iteration)."""
        self.lr = _check_lr(lr, "BilateralGrid")

    # -- the stage
    def apply(self, view, img):
        """w * (A img + b) with [A | b] sliced per pixel from view `view`'s grid: a scratch tensor kept here and overwritten by the next
        call.  `img` (the renderer's imageData in a training step) is what the next backward takes the grid's gradient at."""
        import torch
        v = self._view(view)
        x = self._image(img, "apply")
        if self._out is None:
            self._out = torch.empty((3, self.H, self.W), dtype=torch.float32, device=self.table.device)
        self.renderer._begin().bilagrid_apply(x.data_ptr(), self.table[v].data_ptr(), self.dims, self._wptr(v), self.W, self.H, self._out.data_ptr())
        self._x, self._x_view = x, v
        return self._out

    def backward(self, view, d_out, want_grad: bool = True):
        """The adjoint of the last apply(view, img): returns d_img, written in place into d_out, and (want_grad) keeps the gradient of the
        view's grid for step(), the gradient of tv_coef * tv added to it when tv_coef > 0."""
        v = self._view(view)
        if self._x is None or self._x_view != v:
            raise ValueError(f"BilateralGrid.backward: apply(view={v}, img) first")
        d = self._image(d_out, "backward")
        ctx = self.renderer._begin()
        ctx.bilagrid_backward(self._x.data_ptr(), d.data_ptr(), self.table[v].data_ptr(), self.dims, self._wptr(v), self.W, self.H,
                              d.data_ptr(), self._grad.data_ptr() if want_grad else 0)
        if want_grad:
            if self.tv_coef > 0:
                ctx.bilagrid_tv(self.table[v].data_ptr(), self.dims, self.tv_coef, self._grad.data_ptr(), 0)
            self._have_grad = v
        return d

    def step(self, view):
        """One Adam step of view `view`'s grid from the gradient the last backward kept; the view's own step count advances."""
        v = self._view(view)
        if self._have_grad != v:
            raise ValueError(f"BilateralGrid.step: backward(view={v}, ...) with want_grad first")
        t = self.step_counts[v] + 1
        self.renderer._begin().bilagrid_adam(self.table[v].data_ptr(), self._grad.data_ptr(), self.exp_avg[v].data_ptr(),
                                             self.exp_avg_sq[v].data_ptr(), self.n_floats, self.lr, self.betas[0], self.betas[1], self.eps, t)
        self.step_counts[v] = t
        self._have_grad = -1

    def mask_target(self, view, gt):
        """w * gt for view `view` (gs_bilagrid_apply with a resident identity grid: exact), a scratch tensor overwritten by the next call;
        `gt` itself when the view has no weight."""
        import torch
        v = self._view(view)
        if self.weights[v] is None:
            return gt
        g = self._image(gt, "mask_target")
        if self._masked is None:
            self._masked = torch.empty((3, self.H, self.W), dtype=torch.float32, device=self.table.device)
        self.renderer._begin().bilagrid_apply(g.data_ptr(), self._identity.data_ptr(), self.dims, self._wptr(v), self.W, self.H,
                                              self._masked.data_ptr())
        self._keep_gt = g
        return self._masked

    def grid(self, view) -> np.ndarray:
        """View `view`'s grid as a [Gz, Gy, Gx, 12] float32 array (one read-back)."""
        return self.table[self._view(view)].detach().cpu().numpy()

    def tv(self, view) -> float:
        """The total variation of view `view`'s grid (gs_bilagrid_tv; one read-back): what tv_coef multiplies in the objective."""
        v = self._view(view)
        self.renderer._begin().bilagrid_tv(self.table[v].data_ptr(), self.dims, 0.0, 0, self._tv.data_ptr())
        return float(self._tv.cpu()[0])

    # -- checkpoints
    def state_dict(self) -> dict:
        return dict(table=self.table.detach().clone(), exp_avg=self.exp_avg.detach().clone(), exp_avg_sq=self.exp_avg_sq.detach().clone(),
                    steps=list(self.step_counts), lr=self.lr)

    def load_state_dict(self, state: dict):
        import torch
        shape = tuple(self.table.shape)
        for k in ("table", "exp_avg", "exp_avg_sq"):
            t = state[k]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                raise ValueError(f"BilateralGrid.load_state_dict: {k} must be a tensor of shape {shape}")
        steps = [int(s) for s in state["steps"]]
        if len(steps) != self.n_views or min(steps) < 0:
            raise ValueError(f"BilateralGrid.load_state_dict: {self.n_views} step counts >= 0 expected")
        lr = _check_lr(state["lr"], "BilateralGrid")
        for k in ("table", "exp_avg", "exp_avg_sq"):
            getattr(self, k).copy_(state[k])
        self.step_counts, self.lr = steps, lr
        self._have_grad = -1
