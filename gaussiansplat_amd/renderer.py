"""Host-side mirror of the reference renderer API (src/renderer.jl, src/forward.jl,
src/backward.jl, src/splat.jl) over the C ABI of libgsplat_hip.so.

The reference's call sequence (src/examples/main.jl:14-34) works unchanged in spirit:

    renderer = getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), (gx, gy), path_or_scene)
    tps = preprocess(renderer)
    compactIdxs(renderer, (16, 16), (gx, gy))
    forward(renderer, tps, (16, 16), (gx, gy))
    backward(renderer, dC); ...optimiser...; resetGrads(renderer.splatGrads)

Names, argument meaning and in-place semantics follow the reference: outputs land in
`renderer.imageData` / `renderer.transmittance`, gradients ACCUMULATE in
`renderer.splatGrads.*` until `resetGrads`.  Arrays are torch tensors on the renderer's GPU
with the reference's memory layout ([n, comp] row-major == Julia [comp, n] column-major;
imageData [3, H, W] == Julia [W, H, 3]).  torch is plumbing only (device memory, streams);
all compute is in the HIP library and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import enum
from dataclasses import dataclass

import numpy as np

from . import backend as B
from .camera import Camera, compute_projection, compute_transform, default_camera


class RendererType(enum.Enum):          # renderer.jl:20-24
    GAUSSIAN_2D = 0
    GAUSSIAN_3D = 1
    OPTIMAL_PROJECTION_3D = 2


@dataclass
class SplatData3D:                      # splat.jl:36-43
    means: "torch.Tensor"               # [n, 3]
    scales: "torch.Tensor"              # [n, 3]  log-space
    shs: "torch.Tensor"                 # [n, 3K] element [3k + c]
    quaternions: "torch.Tensor"         # [n, 4]  (w, x, y, z), not normalised by the kernels
    opacities: "torch.Tensor"           # [n, 1]  logit
    features: object = None


@dataclass
class SplatGrads3D:                     # splat.jl:45-52 -- views into ONE flat buffer (single all-reduce)
    flat: "torch.Tensor"
    Δmeans: "torch.Tensor"
    Δscales: "torch.Tensor"
    Δquaternions: "torch.Tensor"
    Δopacities: "torch.Tensor"
    Δshs: "torch.Tensor"
    Δfeatures: object = None


@dataclass
class SplatData2D:                      # splat.jl:20-26
    means: "torch.Tensor"               # [n, 2]  fractions of the image, pixel position (W*mx, H*my)
    scales: "torch.Tensor"              # [n, 2]  log-space
    rotations: "torch.Tensor"           # [n, 1]  theta
    opacities: "torch.Tensor"           # [n, 1]  used raw (splat.jl:341)
    colors: "torch.Tensor"              # [n, 3]


@dataclass
class SplatGrads2D:                     # splat.jl:28-34 -- views into ONE flat buffer
    flat: "torch.Tensor"
    Δmeans: "torch.Tensor"
    Δscales: "torch.Tensor"
    Δrotations: "torch.Tensor"
    Δopacities: "torch.Tensor"
    Δcolors: "torch.Tensor"


def grads_layout(widths, n: int):
    """The layout of a flat gradient buffer, in floats: array i holds widths[i] floats per gaussian and starts at offsets[i], the arrays
    stand behind one another.  Returns (offsets, total).  Pure: everything that needs an offset asks here (initGrads, optim.Adam)."""
    offsets, o = [], 0
    for w in widths:
        offsets.append(o); o += int(w) * int(n)
    return tuple(offsets), o


def grads_views(grads) -> tuple:
    """The five views of a SplatGrads3D / SplatGrads2D in the order of the C ABI's gs_grads."""
    if isinstance(grads, SplatGrads2D):
        return grads.Δmeans, grads.Δscales, grads.Δrotations, grads.Δopacities, grads.Δcolors
    return grads.Δmeans, grads.Δscales, grads.Δquaternions, grads.Δopacities, grads.Δshs


def layout_of(grads):
    """grads_layout of the buffer a SplatGrads3D / SplatGrads2D views."""
    views = grads_views(grads)
    return grads_layout([v.shape[1] for v in views], views[0].shape[0])


def grads_struct(flat, offsets) -> B.GsGrads:
    """Five pointers into a flat buffer of the layout `offsets` (the gradient buffer itself, or Adam's moments)."""
    base = flat.data_ptr()
    return B.GsGrads(*(base + 4 * o for o in offsets))


def _zero_flat(widths, n, device):
    import torch
    offsets, total = grads_layout(widths, n)
    flat = torch.zeros(total, dtype=torch.float32, device=device)
    return flat, [flat[o:o + w * n].view(n, w) for o, w in zip(offsets, widths)]


def initGrads2D(splatData: SplatData2D) -> SplatGrads2D:
    """initGrads(::SplatData2D), splat.jl:121-135, as one flat buffer [Δmeans 2N | Δscales 2N | Δrot N | Δopac N | Δcolors 3N]."""
    flat, views = _zero_flat((2, 2, 1, 1, 3), splatData.means.shape[0], splatData.means.device)
    return SplatGrads2D(flat, *views)


def initGrads(splatData: SplatData3D) -> SplatGrads3D:
    """splat.jl:137-156; laid out as one flat fp32 buffer
    [Δmeans 3N | Δscales 3N | Δquats 4N | Δopac N | Δshs 3K·N] so that a multi-view step needs a
    single RCCL all-reduce."""
    flat, views = _zero_flat((3, 3, 4, 1, splatData.shs.shape[1]), splatData.means.shape[0], splatData.means.device)
    return SplatGrads3D(flat, *views)


def model_arrays(splatData: SplatData3D) -> tuple:
    """The five arrays of a model in the order of the C ABI (gs_set_model, gs_grads)."""
    return splatData.means, splatData.scales, splatData.quaternions, splatData.opacities, splatData.shs


def as_device_tensor(value, device, shape, name: str):
    """value (a tensor, an array, nested numbers) as a contiguous float32 tensor on `device`; shape None: any, else a ValueError that
    names `name`.  A tensor that already is all that comes back as the same object: no copy.  A caller that queues a library call on the
    result keeps it referenced until the call has run (_dC_keepalive, _keep*)."""
    import torch
    t = value if isinstance(value, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(value, np.float32))
    t = t.to(device, torch.float32).contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def draw(fn, shape, generator, device):
    """fn (torch.rand, torch.randn) float32 numbers of `shape` on `device`, drawn on the generator's own device so that the caller's
    generator decides them."""
    import torch
    gdev = generator.device if generator is not None else device
    return fn(shape, generator=generator, device=gdev, dtype=torch.float32).to(device).contiguous()


class _Renderer:
    """What the two renderers share: the output tensors, the context and its stream bind, the lazily zeroed gradients, the background."""

    def __init__(self, imgSize, tensor_device, **ctx_kw):
        import torch
        W, H = int(imgSize[0]), int(imgSize[1])
        self.imageData = torch.zeros((3, H, W), dtype=torch.float32, device=tensor_device)     # CUDA.zeros(imgSize...)
        self.transmittance = torch.ones((H, W), dtype=torch.float32, device=tensor_device)     # CUDA.ones(imgSize[1:2])
        self.camera: Camera | None = None
        self.ctx = B.Context(**ctx_kw)
        # the library enqueues on the caller's CURRENT torch stream (re-read at every API call), like any torch
        # op: no cross-stream fences, so consecutive calls run back to back on the GPU
        self._stream_handle = None

    def _begin(self) -> B.Context:
        """The way into the library: bind the ctx to torch's current stream (handle 0 = the legacy default stream = GS_STREAM_LEGACY;
        an unchanged handle costs no call) and return it."""
        h = _current_stream_handle(self.imageData.device) or 1
        if h != self._stream_handle:
            self.ctx.set_stream(h)
            self._stream_handle = h
        return self.ctx

    @property
    def background(self) -> tuple:
        """The colour behind the last splat, three floats (default black): forward() leaves C + T * background in imageData, and
        backward() differentiates that image -- transparent pixels of a white-background dataset then carry a gradient.  Setting it
        keeps the tile lists and drops the image: render again before the next backward.  It survives a restructured model."""
        return self.ctx.background

    @background.setter
    def background(self, rgb):
        self.ctx.set_background(rgb)

    @property
    def splatGrads(self):
        """renderer.splatGrads (renderer.jl:207).  resetGrads is lazy: the zero fill is skipped when the
        next backward overwrites anyway, and materialised here if somebody looks first."""
        if self._grads_lazy_zero:
            self._splatGrads.flat.zero_()
            self._grads_lazy_zero = False
        return self._splatGrads

    def _set_grads(self, splatGrads):
        self._splatGrads = splatGrads
        self._grads_lazy_zero = False       # True: resetGrads() pending, the next backward overwrites
        self._grads = grads_struct(splatGrads.flat, layout_of(splatGrads)[0])

    # scratch arrays of the reference struct, fetched on demand (export_debug for the fp32 ones)
    @property
    def positions(self): return self.ctx.get_array(B.ARR_MU)
    @property
    def cov2ds(self): return self.ctx.get_array(B.ARR_COV2D)
    @property
    def invCov2ds(self): return self.ctx.get_array(B.ARR_INVCOV)
    @property
    def bbs(self): return self.ctx.get_array(B.ARR_BBS)


class GaussianRenderer3D(_Renderer):    # renderer.jl:205-219
    def __init__(self, splatData: SplatData3D, imgSize, sh_degree: int, device: int = 0, order: int = B.ORDER_DEPTH_DESC,
                 t_min: float = 1e-5, export_debug: bool = False, profile_stages: bool = False, deterministic: bool = False,
                 alpha_cull: bool = True, rank_mode: int = 1, slab_mode: int = 1, schedule: int = 0, share_grads_with=None,
                 background=None, **ctx_kw):
        """background: (r, g, b) behind the last splat (the `background` property); None: black, the reference's frame.
        share_grads_with: another GaussianRenderer3D over the same splatData whose gradient buffer this one accumulates into
        (a second view in flight, distributed.HipViewRenderer): no buffer of its own is allocated."""
        self._shares_grads = share_grads_with is not None   # (a resize replaces the buffer: only its owner may, check_resize)
        super().__init__(imgSize, splatData.means.device, device=device, order=order, t_min=t_min, export_debug=export_debug,
                         profile_stages=profile_stages, deterministic=deterministic, alpha_cull=alpha_cull, rank_mode=rank_mode,
                         slab_mode=slab_mode, schedule=schedule, **ctx_kw)
        self.sh_degree = sh_degree
        self._set_model(splatData, share_grads_with._splatGrads if share_grads_with is not None else None)
        if background is not None:
            self.background = background

    # -- the model and its size.  These three methods are the only code that assigns splatData and nGaussians, and the only callers of
    # _set_grads: a strategy that changes the number of gaussians allocates with alloc_model, fills the arrays through the
    # library and hands them to adopt_model; optim.Adam follows with resized_moments / _rebind
    def _set_model(self, splatData: SplatData3D, shared_grads=None):
        self.splatData = splatData
        self.nGaussians = splatData.means.shape[0]
        self._set_grads(shared_grads if shared_grads is not None else initGrads(splatData))
        self._begin().set_model_device(self.nGaussians, self.sh_degree, [t.data_ptr() for t in model_arrays(splatData)])

    def check_resize(self, optimizer, who: str):
        """A call that changes the number of gaussians needs the renderer that owns its gradient buffer, and that renderer's optimiser."""
        if self._shares_grads:
            raise ValueError(f"{who}: this renderer accumulates into another renderer's gradient buffer (share_grads_with); "
                             "restructure the renderer that owns it and rebuild this one")
        if optimizer is not None and optimizer.renderer is not self:
            raise ValueError(f"{who}: the optimiser belongs to another renderer")

    def alloc_model(self, n_out: int, zero: bool) -> SplatData3D:
        """Five arrays of n_out rows like the model's own (dtype, device, SH row; `features` carried over): zeros, or uninitialised for a
        call that writes every row."""
        import torch
        make = torch.zeros if zero else torch.empty
        d = self.splatData
        new = lambda t: make((int(n_out),) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        return SplatData3D(means=new(d.means), scales=new(d.scales), shs=new(d.shs), quaternions=new(d.quaternions), opacities=new(d.opacities),
                           features=d.features)

    def adopt_model(self, new_data: SplatData3D, who: str):
        """new_data becomes the model: a fresh zero gradient buffer of its size, and gs_set_model on the bound stream.  The arrays replaced
        stay referenced until here; torch frees them in stream order behind the kernels that read them."""
        self.check_resize(None, who)
        self._set_model(new_data)

    @property
    def active_sh_degree(self) -> int:
        """The SH degree the kernels evaluate: the model's own unless a lower one was set (the degree schedule of a training run,
        train.SHDegreeSchedule; a viewer drawing a degree-3 model at degree 0).  Setting it (-1: the model's own again) changes
        neither splatData.shs nor the gradients' layout: the inactive bands get zero gradients."""
        return self.ctx.active_sh_degree

    @active_sh_degree.setter
    def active_sh_degree(self, degree: int):
        self.ctx.set_active_sh_degree(int(degree))

    def _set_view(self, camera):
        cam = camera or self.camera or default_camera()
        self.camera = cam
        H, W = self.transmittance.shape
        # A small frame is bound by its caller (C1: ten thousand gaussians take the GPU 70 us, tools/host_rate.py): the view's matrices
        # (computeTransform / computeProjection, camera.jl:53-111: 60 us of numpy) are kept with the camera object and rebuilt when
        # one of its fields, or the image size, has changed
        snap = (np.asarray(cam.eye, np.float32).tobytes(), np.asarray(cam.lookAt, np.float32).tobytes(), np.asarray(cam.up, np.float32).tobytes(),
                cam.fx, cam.fy, cam.near, cam.far, W, H)
        ent = getattr(cam, "_gs_view", None)
        if ent is None or ent[0] != snap:
            ent = (snap, self.ctx.camera_record(compute_transform(cam), compute_projection(cam, W, H), float(np.float32(cam.fx)), float(np.float32(cam.fy)),
                                                float(np.float32(cam.near)), float(np.float32(cam.far)), cam.eye, cam.lookAt, W, H))
            try:
                cam._gs_view = ent
            except AttributeError:                  # (a camera type without room for it: rebuilt every time)
                pass
        self.ctx.set_camera_record(ent[1])
        # the camera's id (camera.jl:10-22; `id` of cameras.json) names the view slot: a training loop cycles over a fixed
        # camera set and the library launches the forward's tiles heaviest-first by what the same view measured last time
        slot = getattr(cam, "id", None)
        slot = int(slot) if isinstance(slot, (int, np.integer)) and 0 <= int(slot) < B.GS_MAX_VIEW_SLOTS else -1
        if slot != getattr(self, "_view_slot", None):
            self.ctx.set_view_slot(slot)
            self._view_slot = slot

    @property
    def sortIdxs(self): return self.ctx.get_array(B.ARR_SORT_IDXS)
    @property
    def cov3ds(self): return self.ctx.get_array(B.ARR_COV3D)


class GaussianRenderer2D(_Renderer):     # renderer.jl:7-18
    """The 2-D image-fitting renderer: same binning and composite kernels as the 3-D one behind a different
    preprocess (cov2d.jl:3-28).  The reference's own 2-D constructors reference undefined names (renderer.jl:38-82)
    and its backward (splat.jl:271-396) is not the adjoint of any one forward; this is the consistent version
    (DESIGN.md, 2-D renderer)."""

    def __init__(self, splatData: SplatData2D, imgSize, device: int = 0, t_min: float = 1e-5, export_debug: bool = False,
                 profile_stages: bool = False, deterministic: bool = False, alpha_cull: bool = True, background=None):
        super().__init__(imgSize, splatData.means.device, device=device, order=B.ORDER_INDEX, t_min=t_min, export_debug=export_debug,
                         profile_stages=profile_stages, deterministic=deterministic, alpha_cull=alpha_cull)
        self.splatData = splatData
        self.nGaussians = splatData.means.shape[0]
        self._set_grads(initGrads2D(splatData))
        self._begin().set_model_2d_device(self.nGaussians, [t.data_ptr() for t in (splatData.means, splatData.scales, splatData.rotations,
                                                                                   splatData.opacities, splatData.colors)])
        if background is not None:
            self.background = background

    def _set_view(self, camera=None):
        H, W = self.transmittance.shape
        self.ctx.set_image_size(W, H)


def initData2D(nGaussians: int, seed: int = 0) -> dict:
    """initData(Val(SPLAT2D), n), splat.jl:74-87: everything uniform [0,1), rotations pi/2*(U-0.5)."""
    rng = np.random.default_rng(seed)
    r = lambda *sh: rng.random(sh, dtype=np.float32)
    return dict(means=r(nGaussians, 2), scales=r(nGaussians, 2), rots=np.float32(np.pi / 2) * (r(nGaussians) - np.float32(0.5)),
                opacities=r(nGaussians), colors=r(nGaussians, 3))


def _to_device_data_2d(scene: dict, device) -> SplatData2D:
    import torch
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(device).contiguous()
    n = np.asarray(scene["means"]).shape[0]
    return SplatData2D(means=t(scene["means"]), scales=t(scene["scales"]), rotations=t(np.reshape(scene["rots"], (n, 1))),
                       opacities=t(np.reshape(scene["opacities"], (n, 1))), colors=t(scene["colors"]))


def _to_device_data(scene: dict, device) -> SplatData3D:
    import torch
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(device).contiguous()
    n = scene["means"].shape[0]
    return SplatData3D(means=t(scene["means"]), scales=t(scene["scales"]), shs=t(np.reshape(scene["shs"], (n, -1))),
                       quaternions=t(scene["quats"]), opacities=t(np.reshape(scene["opacities"], (n, 1))))


def initData(nGaussians: int, seed: int = 0) -> dict:
    """splat.jl:90-104: uniform [0,1) parameters (the reference draws a 9xN `shs`, inconsistent
    with the 12 floats splatDraw reads; 12 are drawn here = SH degree 1)."""
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.random(s, dtype=np.float32)
    return dict(means=r(nGaussians, 3), quats=r(nGaussians, 4), scales=r(nGaussians, 3), shs=r(nGaussians, 4, 3),
                opacities=r(nGaussians))


def getRenderer(rendererType, imgSize, threads, blocks, source=None, *, device: int = 0, **kw):
    """renderer.jl:164-186.  `source`: a PLY path (splat.jl:106-119), an int nGaussians
    (splat.jl:90-104), a dict of arrays (means, scales, quats, opacities, shs[n,K,3]) or a pointcloud.PointCloud (an SfM point
    cloud: the model a training run starts from, pointcloud.from_points)."""
    import torch
    if isinstance(rendererType, str):
        rendererType = RendererType[rendererType.lstrip(":")]
    if rendererType == RendererType.OPTIMAL_PROJECTION_3D:
        raise NotImplementedError("OPTIMAL_PROJECTION_3D: the reference has an enum value and a forwarding method "
                                  "(renderer.jl:23,189-195) but no implementation to follow")
    if tuple(threads) != (16, 16):
        raise ValueError("threads must be (16, 16) (tile size of the reference's example, main.jl:9)")
    W, H = int(imgSize[0]), int(imgSize[1])
    if blocks is not None and tuple(blocks) != ((W + 15) // 16, (H + 15) // 16):
        raise ValueError("blocks must be ceil(imgSize/threads)")
    if not torch.cuda.is_available():
        raise RuntimeError("gaussiansplat_amd needs a HIP device (no CPU fallback)")
    if rendererType == RendererType.GAUSSIAN_2D:         # renderer.jl:38-82: nGaussians or arrays (no PLY form)
        if isinstance(source, int):
            scene = initData2D(source)
        elif isinstance(source, dict):
            scene = source
        else:
            raise TypeError("GAUSSIAN_2D: source must be an int (nGaussians) or a dict of arrays (means, scales, rots, opacities, colors)")
        kw.pop("order", None)
        return GaussianRenderer2D(_to_device_data_2d(scene, torch.device("cuda", device)), (W, H), device=device, **kw)
    from .pointcloud import PointCloud, from_points
    if isinstance(source, PointCloud):                   # the start of a training run: 3-NN scales and the model built on the device
        return GaussianRenderer3D(from_points(source, device=device), (W, H), source.sh_degree, device=device, **kw)
    if isinstance(source, str):
        from .ply import load_ply
        scene = load_ply(source)
    elif isinstance(source, int):
        scene = initData(source)
    elif isinstance(source, dict):
        scene = source
    else:
        raise TypeError("source must be a PLY path, an int, a dict of arrays or a pointcloud.PointCloud")
    shs = np.asarray(scene["shs"])
    K = shs.reshape(shs.shape[0], -1).shape[1] // 3
    deg = {1: 0, 4: 1, 9: 2, 16: 3}[K]
    data = _to_device_data(scene, torch.device("cuda", device))
    return GaussianRenderer3D(data, (W, H), deg, device=device, **kw)


def preprocess(renderer, camera: Camera | None = None):
    """forward.jl:35-111 (3-D; the reference hard-codes defaultCamera(), forward.jl:53 -- a camera may be passed
    instead) and forward.jl:9-33 (2-D: no camera).  Returns `tps` lazily (the reference returns the clip-space
    positions only to hand them to forward()); None for the 2-D renderer."""
    renderer._set_view(camera)
    renderer._begin().preprocess()
    return _LazyTps(renderer) if isinstance(renderer, GaussianRenderer3D) else None


def _current_stream_handle(device) -> int:
    """torch's current stream on `device` as a raw handle (0: the legacy default stream).  The private fast path costs 0.3 us, the
    public one (a Stream object per call) 2.5 us -- four times per frame."""
    import torch
    try:
        return int(torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch.cuda.current_device()))
    except Exception:
        return int(torch.cuda.current_stream(device).cuda_stream)


class _LazyTps:
    def __init__(self, r): self._r = r
    def numpy(self): return self._r.ctx.get_array(B.ARR_TPS)


def compactIdxs(renderer, threads=(16, 16), blocks=None):
    """forward.jl:118-161: builds the per-tile splat lists (tile|depth keys, radix sort, ranges)."""
    gx, gy = blocks if blocks is not None else (0, 0)
    renderer._begin().bin(int(gx), int(gy))


def _bind_outputs(renderer):
    """The way into the library for a call that reads or writes the frame's image: _begin(), and
    renderer.imageData / renderer.transmittance ARE the library's output buffers (gs_bind_outputs: no copy).  The raw
    pointers are re-read at every forward / backward: if the caller replaced a tensor since, the new one is bound (and a
    backward then refuses to run on a forward that wrote somewhere else).  Returns the ctx; the pointers bound are renderer._bound_out."""
    ctx = renderer._begin()
    img, tr = renderer.imageData, renderer.transmittance
    H, W = tr.shape
    if tuple(img.shape) != (3, H, W) or not img.is_contiguous() or not tr.is_contiguous():
        raise ValueError("renderer.imageData must be a contiguous [3, H, W] tensor matching renderer.transmittance [H, W]")
    key = (img.data_ptr(), tr.data_ptr())
    if getattr(renderer, "_bound_out", None) != key:
        ctx.bind_outputs(*key)                                  # (the ctx falls back to the binned frame: a new forward is due)
        renderer._bound_out = key
    return ctx


def forward(renderer, tps=None, threads=(16, 16), blocks=None):
    """forward.jl:163-198: writes renderer.imageData and renderer.transmittance in place.
    Contract: the two tensors stay the library's buffers until the frame's last backward -- the backward reads the rendered
    colours from renderer.imageData, so editing it in place between forward and backward changes the gradients, and
    replacing it makes backward() raise (render again first)."""
    _bind_outputs(renderer).forward_device(*renderer._bound_out)


def renderFrame(renderer, camera: Camera | None = None):
    """preprocess -> compactIdxs -> forward under `camera`: the frame of a training step, of an evaluated view, of every view of a
    multi-view step."""
    tps = preprocess(renderer, camera)
    compactIdxs(renderer)
    forward(renderer, tps)


def backward(renderer, ΔC, skip_shs: bool = False, phase: str = "all"):
    """backward.jl:3-38: ΔC has the shape of imageData; accumulates into renderer.splatGrads.
    skip_shs (3-D renderer, colour-factored multi-GPU exchange): leave Δshs alone -- the caller rebuilds it from the
    per-view colour gradients (distributed.multi_view_step(sync="factored")).
    phase: "all" (default); "composite" then "params" (split backward); or "composite", "params_sh", "params_geom": the
    per-gaussian chain in two steps, so that the all-reduce of Δshs can start while the geometry chain still runs."""
    dC = as_device_tensor(ΔC, renderer.imageData.device, renderer.imageData.shape, "ΔC")
    renderer._dC_keepalive = dC
    ctx = _bind_outputs(renderer)                               # a replaced imageData is caught here: the ctx then reports "gs_forward first"
    grads = renderer._grads
    if skip_shs:
        grads = _without_shs(grads)
    ctx.backward(dC.data_ptr(), grads, overwrite=renderer._grads_lazy_zero, phase=phase)
    if phase not in ("composite", "params_sh"):                 # "params_sh" is followed by "params_geom" with the same overwrite flag
        renderer._grads_lazy_zero = False


def _without_shs(g: B.GsGrads) -> B.GsGrads:
    """The gradient arrays without Δshs: a call that leaves the SH gradients alone."""
    return B.GsGrads(g.d_means, g.d_scales, g.d_quats, g.d_opacities, None)


# ---------------------------------------------------------------- feature maps (3-D renderer): depth, opacity, per-gaussian features

def renderFeatures(renderer, feat):
    """Composite three per-gaussian floats over the frame forward() rendered: feat [n, 3] -> (F [3, H, W], T [H, W]) with
    F[c] = sum feat[:, c] * alpha * T over the same entries, in the same order, under the same early-out as the colour image; no
    background is added, T is the frame's transmittance.  New tensors; renderer.imageData / transmittance and the frame stay as they are
    (a frame binned in depth slabs is refused: pass slab_mode=0 to getRenderer).  Wider features are rendered in triples."""
    import torch
    H, W = renderer.transmittance.shape
    f = as_device_tensor(feat, renderer.imageData.device, (renderer.nGaussians, 3), "feat")
    F = torch.empty((3, H, W), dtype=torch.float32, device=f.device)
    T = torch.empty((H, W), dtype=torch.float32, device=f.device)
    _bind_outputs(renderer).render_features(f.data_ptr(), F.data_ptr(), T.data_ptr())
    return F, T


def backwardFeatures(renderer, feat, F, dF):
    """The adjoint of renderFeatures for the loss sum F * dF: returns d_feat [n, 3] and ACCUMULATES the alpha-path gradients into
    renderer.splatGrads (means, scales, quaternions, opacities; the SH gradients are not touched: the features do not depend on the model
    here).  F is what renderFeatures returned for this feat on this frame.  Legal before, between or after backward()."""
    import torch
    H, W = renderer.transmittance.shape
    n, dev = renderer.nGaussians, renderer.imageData.device
    f = as_device_tensor(feat, dev, (n, 3), "feat")
    F = as_device_tensor(F, dev, (3, H, W), "F")
    dF = as_device_tensor(dF, dev, (3, H, W), "dF")
    d_feat = torch.empty((n, 3), dtype=torch.float32, device=f.device)
    renderer.splatGrads                                         # a pending lazy reset becomes zeros now: this call accumulates
    _bind_outputs(renderer).backward_features(f.data_ptr(), F.data_ptr(), dF.data_ptr(), d_feat.data_ptr(), _without_shs(renderer._grads))
    return d_feat


def viewDepth(renderer):
    """z [n]: the view-space depth of every gaussian under the renderer's current camera (preprocess() sets it), as the preprocess
    computes it (ts[3, :] of the reference's tValues)."""
    import torch
    z = torch.empty((renderer.nGaussians,), dtype=torch.float32, device=renderer.imageData.device)
    renderer._begin().view_depth(z.data_ptr())
    return z


def renderDepth(renderer, mode: str = "accumulated"):
    """Depth of the frame forward() rendered, from the features (z, z^2, 1): planes [3, H, W] = (sum z w, sum z^2 w, sum w) with
    w = alpha * T -- accumulated depth, its second moment (a variance: planes[1] / planes[2] - expected^2) and the opacity 1 - T.
    mode "accumulated": returns planes.  mode "expected": returns (planes, depth [H, W]) with depth = planes[0] / planes[2] where
    planes[2] > 1e-8, else 0.  backwardDepth differentiates the three planes."""
    import torch
    if mode not in ("accumulated", "expected"):
        raise ValueError('renderDepth: mode must be "accumulated" or "expected"')
    z = viewDepth(renderer)
    feat = torch.stack((z, z * z, torch.ones_like(z)), 1).contiguous()
    planes, _ = renderFeatures(renderer, feat)
    renderer._depth_state = (feat, planes, z)
    if mode == "accumulated":
        return planes
    return planes, torch.where(planes[2] > 1e-8, planes[0] / planes[2], torch.zeros_like(planes[0]))


def backwardDepth(renderer, dD):
    """The adjoint of renderDepth's three planes for the loss sum planes * dD (dD [3, H, W]; for the expected depth the caller chains
    d depth -> d planes first: d planes[0] = g / planes[2], d planes[2] = -g * depth / planes[2]).  Accumulates into
    renderer.splatGrads: the alpha path through backwardFeatures, and the value path z(means) -- dz = d_feat[:, 0] + 2 z d_feat[:, 1] --
    into the means."""
    st = getattr(renderer, "_depth_state", None)
    if st is None:
        raise RuntimeError("backwardDepth: renderDepth first")
    feat, planes, z = st
    d_feat = backwardFeatures(renderer, feat, planes, dD)
    dz = (d_feat[:, 0] + 2.0 * z * d_feat[:, 1]).contiguous()
    renderer._begin().view_depth_backward(dz.data_ptr(), renderer._grads.d_means)
    return d_feat


# ---------------------------------------------------------------- camera gradient (3-D renderer): pose refinement

@dataclass
class CameraGrads:
    """What backwardCamera returns: the frame's gradient into the arguments of gs_set_camera, taken as independent inputs, float32.
    T and P are flat column-major like compute_transform / compute_projection; camera.camera_param_grads chains them to Camera fields."""
    T: np.ndarray
    P: np.ndarray
    eye: np.ndarray
    lookAt: np.ndarray
    fx: np.ndarray
    fy: np.ndarray

    @classmethod
    def from_flat(cls, v) -> "CameraGrads":
        v = np.ascontiguousarray(v, np.float32).reshape(-1)
        if v.shape != (B.GS_CAMERA_GRAD_FLOATS,):
            raise ValueError(f"CameraGrads: {B.GS_CAMERA_GRAD_FLOATS} floats expected, got {v.shape}")
        return cls(v[0:16].copy(), v[16:32].copy(), v[32:35].copy(), v[35:38].copy(), v[38:39].copy().reshape(()), v[39:40].copy().reshape(()))

    def flat(self) -> np.ndarray:
        return np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in (self.T, self.P, self.eye, self.lookAt, self.fx, self.fy)])


def backwardCamera(renderer) -> CameraGrads:
    """The gradient of the frame's loss with respect to the view (gs_backward_camera): call it after backward() on the frame and BEFORE
    anything steps the model -- the chain is recomputed from the resident parameters.  The frame and renderer.splatGrads stay as they
    are.  The 2-D renderer has no camera: the library's error (GS_ERR_UNSUPPORTED) is raised."""
    return CameraGrads.from_flat(renderer._begin().backward_camera())


def require_3d(renderer, who: str):
    if not isinstance(renderer, GaussianRenderer3D):
        raise ValueError(f"{who}: needs the 3-D renderer")


def resetGrads(renderer_or_grads):
    """splat.jl:158-173."""
    if isinstance(renderer_or_grads, _Renderer):
        renderer_or_grads._grads_lazy_zero = True      # zero fill deferred: see GaussianRenderer3D.splatGrads
    else:
        renderer_or_grads.flat.zero_()
