"""ctypes binding of libgsplat_hip.so (include/gsplat.h) -- the Python twin of julia/backend.jl.

This is the only way the package reaches the GPU: there is NO CPU fallback here.  If the
shared library is missing or the HIP device is absent every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSPLAT_HIP_LIB") or os.path.join(_HERE, "lib", "libgsplat_hip.so")   # override: diagnostic builds

# Every integer below states a value of include/gsplat.h (or, where the comment says so, of a csrc/ header); tests/test_abi.py reads the
# headers and compares each one, and fails on an integer constant of this module that it cannot place.
GS_MEM_HOST, GS_MEM_DEVICE = 0, 1
ORDER_INDEX, ORDER_DEPTH_DESC, ORDER_DEPTH_ASC = 0, 1, 2          # GS_ORDER_*

(ARR_TS, ARR_TPS, ARR_MU, ARR_COV3D, ARR_COV2D, ARR_INVCOV, ARR_BBS, ARR_RGB, ARR_SIG, ARR_DEPTH_KEY,
 ARR_TILE_RECT, ARR_SORT_IDXS, ARR_TILE_RANGES, ARR_SORTED_IDS, ARR_SORTED_KEYS, ARR_GRAD2D) = range(16)   # GS_ARR_*

STAGES = ("preprocess", "depth_sort", "count_scan", "emit", "tile_sort", "ranges", "composite_fwd",
          "composite_bwd", "preprocess_bwd")                     # gs_stage, lower case

GS_CAMERA_GRAD_FLOATS = 40  # gs_backward_camera
GS_METRIC_SUMS = 4          # gs_image_metrics
GS_EXPOSURE_FLOATS = 12     # csrc/gs_exposure.h: a row of the exposure table, 3 x 4 row-major
GS_BILAGRID_FLOATS = 12     # gs_bilagrid_*: a vertex of a bilateral grid, 3 x 4 row-major
GS_BILAGRID_MAX_DIM = 64    # ... and the most vertices along an axis
(METRIC_MSE, METRIC_MAE, METRIC_SSIM, METRIC_PSNR, GS_METRIC_COUNT) = range(5)   # GS_METRIC_*
GS_ABI_VERSION = 3          # load() refuses a library that reports another version
GS_DEBUG_WIDE_CURSORS = 1
GS_DEBUG_ALWAYS_ORDER = 2     # launch orders + side stream also on small frames (tests)
GS_DEBUG_SUPER16 = 8          # two-level binning: super-tiles of 16 x 16 tiles whatever the grid (tests)
GS_DEBUG_SUPER8 = 16          # ... of 8 x 8 tiles whatever the grid
GS_DEBUG_NO_TAIL_FILL = 32    # the frame's zero fills in line instead of at the end of the composite launches' grids (A/B runs, tests)
GS_DEBUG_TINY_CAPS = 4        # capped lists with the minimum cap on every tile (tests: every busy tile extends its list in the composite kernel)
GS_MAX_VIEW_SLOTS = 4096
GS_BWD_OVERWRITE, GS_BWD_COMPOSITE_ONLY, GS_BWD_PARAMS_ONLY, GS_BWD_PARAMS_SH, GS_BWD_PARAMS_GEOM = 1, 2, 4, 8, 16   # gs_backward_ex
GS_ADAM_GROUPS = 6            # lr[0] means, [1] scales, [2] quaternions, [3] opacities, [4] SH band 0, [5] SH bands >= 1
GS_ADAM_SELECTIVE = 1         # step only the gaussians with a non-zero gradient float ("selective Adam")
GS_ERR_INVALID, GS_ERR_UNSUPPORTED = -1, -5
KNN_BOX = 64                  # points per box of the 3-NN search (GS_KNN_BOX in csrc/gs_knn.h; tests pick their sizes around it)
TOUCHED_CHUNK = 256           # gaussians per workgroup of the touched-rows pack (GS_CHUNK in csrc/gs_chunk.h; tests pick their sizes around it)


class GsConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("abi_version", C.c_int32), ("tile_size", C.c_int32), ("order", C.c_int32), ("t_min", C.c_float),
                ("deterministic", C.c_int32), ("export_debug", C.c_int32), ("profile_stages", C.c_int32),
                ("bin_path", C.c_int32), ("rank_mode", C.c_int32), ("alpha_cull", C.c_int32), ("schedule", C.c_int32),
                ("slab_mode", C.c_int32), ("slab_max_ratio", C.c_float), ("slab_fractions", C.c_float * 3), ("debug_flags", C.c_int32),
                ("depth_sort", C.c_int32), ("list_cap", C.c_int32), ("tile_parts", C.c_int32), ("reserved", C.c_int32 * 3)]


class GsGrads(C.Structure):
    _fields_ = [("d_means", C.c_void_p), ("d_scales", C.c_void_p), ("d_quats", C.c_void_p),
                ("d_opacities", C.c_void_p), ("d_shs", C.c_void_p)]


class GsDensityStats(C.Structure):
    """gs_density_stats: three caller-owned device arrays of n elements (float32, int32, int32)."""
    _fields_ = [("grad_sum", C.c_void_p), ("count", C.c_void_p), ("max_extent", C.c_void_p)]


class GsDensityParams(C.Structure):
    """gs_density_params: the thresholds of gs_density_decide, already in log / logit space."""
    _fields_ = [("struct_size", C.c_int32), ("grad_threshold", C.c_float), ("log_split_scale", C.c_float), ("log_shrink", C.c_float),
                ("min_opacity_logit", C.c_float), ("log_max_world_scale", C.c_float), ("max_extent_px", C.c_int32)]


class GsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libgsplat_hip error {code}: {msg}")
        self.code = code


# one prototype of include/gsplat.h as ctypes states it; optional: load() tolerates a library without the symbol
Sig = namedtuple("Sig", "restype argtypes optional", defaults=(False,))
_i, _i32, _i64, _f, _vp = C.c_int, C.c_int32, C.c_int64, C.c_float, C.c_void_p
_fp, _dp, _i32p, _i64p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
_G, _cfg = C.POINTER(GsGrads), C.POINTER(GsConfig)

# The C ABI, stated once for Python, in the header's order: load() applies it, SYMBOLS is its keys, and tests/test_abi.py checks every entry
# against the header's prototype (arity, scalar widths, pointees) and that neither side has a function the other lacks.
ABI = {
    "gs_default_config": Sig(None, [_cfg]),
    "gs_abi_version": Sig(_i, []),
    "gs_create": Sig(_i, [C.POINTER(_vp), _i, _cfg]),
    "gs_destroy": Sig(_i, [_vp]),
    "gs_last_error": Sig(C.c_char_p, [_vp]),
    "gs_set_stream": Sig(_i, [_vp, _vp]),
    "gs_synchronize": Sig(_i, [_vp]),
    "gs_set_model": Sig(_i, [_vp, _i64, _i, _vp, _vp, _vp, _vp, _vp, _i]),
    "gs_set_model_2d": Sig(_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i]),
    "gs_set_active_sh_degree": Sig(_i, [_vp, _i]),
    "gs_get_active_sh_degree": Sig(_i, [_vp]),
    "gs_set_background": Sig(_i, [_vp, _fp]),
    "gs_get_background": Sig(_i, [_vp, _fp]),
    "gs_compose_target": Sig(_i, [_vp, _vp, _i32, _i32, _vp]),
    "gs_set_image_size": Sig(_i, [_vp, _i32, _i32]),
    "gs_set_camera": Sig(_i, [_vp, _fp, _fp, _f, _f, _f, _f, _fp, _fp, _i32, _i32]),
    "gs_set_view_slot": Sig(_i, [_vp, _i32]),
    "gs_preprocess": Sig(_i, [_vp]),
    "gs_bin": Sig(_i, [_vp, _i32, _i32]),
    "gs_bind_outputs": Sig(_i, [_vp, _vp, _vp]),
    "gs_forward": Sig(_i, [_vp, _vp, _vp, _i]),
    "gs_backward": Sig(_i, [_vp, _vp, _i, _G]),
    "gs_backward_ex": Sig(_i, [_vp, _vp, _i, _G, _i]),
    "gs_backward_sgd": Sig(_i, [_vp, _vp, _i, _f]),
    "gs_reset_grads": Sig(_i, [_vp, _G]),
    "gs_grads_alloc": Sig(_i, [_vp, _G]),
    "gs_grads_read": Sig(_i, [_vp, _G, _vp, _vp, _vp, _vp, _vp]),
    "gs_color_grads_pack": Sig(_i, [_vp, _vp]),
    "gs_sh_grads_from_views": Sig(_i, [_vp, _i32, _vp, _vp, _vp, _i]),
    "gs_color_rows_pack": Sig(_i, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "gs_sh_grads_from_touched": Sig(_i, [_vp, _i32, _vp, _vp, _vp, _i64, _vp, _i]),
    "gs_comm_unique_id": Sig(_i, [_vp]),
    "gs_comm_init": Sig(_i, [_vp, _i, _i, _vp]),
    "gs_allreduce_grads": Sig(_i, [_vp, _G]),
    "gs_comm_destroy": Sig(_i, [_vp]),
    "gs_loss_l1_dssim": Sig(_i, [_vp, _vp, _vp, _i32, _i32, _i32, _f, _vp, _dp, _i]),
    "gs_sgd_step": Sig(_i, [_vp, _f, _G]),
    "gs_adam_step": Sig(_i, [_vp, _G, _G, _G, _fp, _f, _f, _f, _i64, _i]),
    "gs_backward_adam": Sig(_i, [_vp, _vp, _i, _G, _G, _fp, _f, _f, _f, _i64, _i]),
    "gs_density_accumulate": Sig(_i, [_vp, C.POINTER(GsDensityStats)]),
    "gs_density_decide": Sig(_i, [_vp, C.POINTER(GsDensityStats), C.POINTER(GsDensityParams), _vp]),
    "gs_density_plan": Sig(_i, [_vp, _vp, _i64p]),
    "gs_density_restructure": Sig(_i, [_vp, _vp, _vp, _G, _i32, _G, _G, _i64]),
    "gs_opacity_reset": Sig(_i, [_vp, _f, _vp, _vp]),
    "gs_mcmc_plan": Sig(_i, [_vp, _f, _vp, _vp, _i64p]),
    "gs_mcmc_sample": Sig(_i, [_vp, _vp, _i64, _vp, _i64, _vp]),
    "gs_mcmc_relocate": Sig(_i, [_vp, _vp, _vp, _i64, _f, _i32, _G]),
    "gs_mcmc_noise": Sig(_i, [_vp, _vp, _f, _f, _f]),
    "gs_mcmc_regularize": Sig(_i, [_vp, _G, _f, _f]),
    "gs_knn_mean_dist2": Sig(_i, [_vp, _vp, _i64, _vp]),
    "gs_init_from_points": Sig(_i, [_vp, _vp, _vp, _vp, _i64, _i, _f, _G]),
    "gs_view_depth": Sig(_i, [_vp, _vp]),
    "gs_view_depth_backward": Sig(_i, [_vp, _vp, _vp]),
    "gs_render_features": Sig(_i, [_vp, _vp, _vp, _vp]),
    "gs_backward_features": Sig(_i, [_vp, _vp, _vp, _vp, _vp, _G]),
    "gs_backward_camera": Sig(_i, [_vp, _vp, _i]),
    "gs_image_metrics": Sig(_i, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _i]),
    "gs_metrics_finish": Sig(_i, [_dp, _dp]),
    "gs_exposure_apply": Sig(_i, [_vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "gs_exposure_backward": Sig(_i, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "gs_exposure_adam": Sig(_i, [_vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _i64]),
    "gs_bilagrid_apply": Sig(_i, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _vp]),
    "gs_bilagrid_backward": Sig(_i, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
    "gs_bilagrid_tv": Sig(_i, [_vp, _vp, _i32, _i32, _i32, _f, _vp, _vp]),
    "gs_bilagrid_adam": Sig(_i, [_vp, _vp, _vp, _vp, _vp, _i64, _f, _f, _f, _f, _i64]),
    "gs_num_gaussians": Sig(_i64, [_vp]),
    "gs_num_instances": Sig(_i64, [_vp]),
    "gs_num_coarse_instances": Sig(_i64, [_vp]),
    "gs_num_rounds": Sig(_i, [_vp]),
    "gs_get_array": Sig(_i, [_vp, _i, _vp, _i64]),
    "gs_get_stage_times": Sig(_i, [_vp, _fp]),
    "gs_get_stage_stats": Sig(_i, [_vp, _dp, _i64p, _i]),
    "gs_get_work_counters": Sig(_i, [_vp, _i64p, _i64p]),
    "gs_get_list_stats": Sig(_i, [_vp, _i64p]),
    "gs_get_tile_parts": Sig(_i, [_vp]),
    "gs_get_bin_path": Sig(_i, [_vp]),
    "gs_get_work_counters_ex": Sig(_i, [_vp, _i64p]),
    "gs_debug_time_composite": Sig(_i, [_vp, _i, _i, _i, _fp]),
    "gs_debug_tile_clock": Sig(_i, [_vp, _i, _i, _vp]),
    "gs_debug_tile_clock_rows": Sig(_i, [_vp]),
    "gs_debug_tail_fill": Sig(_i, [_vp, _i32p], optional=True),   # an older library built for an A/B run loads without it; only tail_fill_blocks fails
    "gs_debug_clock_mhz": Sig(_i, [_vp, _fp]),
    "gs_debug_set_window": Sig(_i, [_vp, _i32, _i32]),
    "gs_rank_probe_result": Sig(_i, [_vp]),
}
SYMBOLS = tuple(ABI)

_lib = None


def load():
    """dlopen the library; raises if it has not been built (python -m gaussiansplat_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # ONE HIP runtime per process: torch bundles its own libamdhip64.so.7 / libhsa-runtime64;
        # loading it first makes our library's NEEDED libamdhip64.so.7 resolve to the same copy
        # (loading /opt/rocm's copy first leaves torch with "No HIP GPUs are available").
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} not found: build it with `python -m gaussiansplat_amd.build` "
                                "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    for name, sig in ABI.items():
        try:
            f = getattr(L, name)
        except AttributeError:
            if sig.optional:
                continue
            raise
        f.restype, f.argtypes = sig.restype, sig.argtypes
    if L.gs_abi_version() != GS_ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} has ABI version {L.gs_abi_version()}, this binding is written for {GS_ABI_VERSION}: "
                           "rebuild with `python -m gaussiansplat_amd.build --force`")
    _lib = L
    return L


def default_config() -> GsConfig:
    cfg = GsConfig()
    load().gs_default_config(C.byref(cfg))
    return cfg


def metrics_finish(sums) -> np.ndarray:
    """gs_metrics_finish: the four sums of gs_image_metrics -> float64 [mse, mae, ssim, psnr] (METRIC_*).  Pure host arithmetic: data range 1,
    psnr = +inf at mse == 0, four NaNs when sum w is not > 0.  Needs the library, not a GPU."""
    s = np.ascontiguousarray(sums, np.float64).reshape(-1)
    if s.shape != (GS_METRIC_SUMS,):
        raise ValueError(f"metrics_finish: {GS_METRIC_SUMS} sums expected, got {s.shape}")
    out = np.empty(GS_METRIC_COUNT, np.float64)
    rc = load().gs_metrics_finish(s.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
    if rc != 0:
        raise GsError(rc, "gs_metrics_finish")
    return out


_BWD_PHASE = {"all": 0, "composite": GS_BWD_COMPOSITE_ONLY, "params": GS_BWD_PARAMS_ONLY, "params_sh": GS_BWD_PARAMS_ONLY | GS_BWD_PARAMS_SH,
              "params_geom": GS_BWD_PARAMS_ONLY | GS_BWD_PARAMS_GEOM}      # Context.backward(phase=...)


class Context:
    """Owns one gs_ctx (one GPU, one stream)."""

    def __init__(self, device: int = 0, order: int = ORDER_DEPTH_DESC, t_min: float = 1e-5, export_debug: bool = False,
                 profile_stages: bool = False, deterministic: bool = False, bin_path: int = 0, rank_mode: int = 1,
                 alpha_cull: bool = True, schedule: int = 0, slab_mode: int = 1, slab_fractions=(), slab_max_ratio: float = 0.0,
                 debug_flags: int = 0, depth_sort: int = 0, list_cap: int = 0, tile_parts: "int | None" = None,
                 cfg: "GsConfig | None" = None):
        """schedule 0 = the library default (3); slab_fractions / slab_max_ratio / debug_flags: gs_config fields for tests;
        depth_sort 0 automatic, 1 the four-pass radix sort, 2 always key-range buckets + LDS (same permutation);
        list_cap 0 automatic (tile lists written as far as the view slot's previous frame walked them), 1 never, 2 also on small grids.
        cfg: a complete gs_config to copy instead (every field: a second ctx that must take the same code paths as the first)."""
        self.L = load()
        if cfg is not None:
            cfg = GsConfig.from_buffer_copy(cfg)
        else:
            cfg = default_config()
            assert cfg.struct_size == C.sizeof(GsConfig) and cfg.abi_version == GS_ABI_VERSION
            cfg.schedule = int(schedule)
            cfg.slab_mode = int(slab_mode)
            cfg.slab_max_ratio = float(slab_max_ratio)
            for i, f in enumerate(tuple(slab_fractions)[:3]):
                cfg.slab_fractions[i] = float(f)
            cfg.debug_flags = int(debug_flags)
            cfg.depth_sort = int(depth_sort)
            cfg.list_cap = int(list_cap)
            # waves per tile on small grids: 0 = automatic; None = GSPLAT_TILE_PARTS (the test suite pins 1 there: its cross-mode tests
            # assert bit-identical results, which holds under one partition of the pixels only) or automatic
            cfg.tile_parts = int(os.environ.get("GSPLAT_TILE_PARTS", "0")) if tile_parts is None else int(tile_parts)
            cfg.order, cfg.t_min = int(order), float(t_min)
            cfg.export_debug, cfg.profile_stages, cfg.deterministic = int(export_debug), int(profile_stages), int(deterministic)
            cfg.bin_path, cfg.rank_mode, cfg.alpha_cull = int(bin_path), int(rank_mode), int(alpha_cull)
        self.cfg = cfg
        self.h = C.c_void_p()
        rc = self.L.gs_create(C.byref(self.h), device, C.byref(cfg))
        if rc != 0:
            raise GsError(rc, (self.L.gs_last_error(None) or b"").decode())
        self._keep = []

    def _chk(self, rc: int):
        if rc != 0:
            raise GsError(rc, (self.L.gs_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.gs_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing
    def set_stream(self, hip_stream: int | None):
        self._chk(self.L.gs_set_stream(self.h, hip_stream or 0))

    def synchronize(self):
        self._chk(self.L.gs_synchronize(self.h))

    # -- model / camera
    def set_model_host(self, means, scales, quats, opacities, shs, sh_degree: int):
        arrs = [np.ascontiguousarray(a, np.float32) for a in (means, scales, quats, opacities, shs)]
        n = arrs[0].shape[0]
        self._chk(self.L.gs_set_model(self.h, n, sh_degree, *(a.ctypes.data for a in arrs), GS_MEM_HOST))

    def set_model_device(self, n: int, sh_degree: int, ptrs):
        """ptrs: five device pointers (means, scales, quats, opacities, shs); borrowed, not copied."""
        self._chk(self.L.gs_set_model(self.h, n, sh_degree, *(int(p) for p in ptrs), GS_MEM_DEVICE))

    def set_model_2d_host(self, means, scales, rots, opacities, colors):
        """SplatData2D (splat.jl:20-26): means [n,2], scales [n,2], rotations [n], opacities [n], colors [n,3]."""
        arrs = [np.ascontiguousarray(a, np.float32) for a in (means, scales, rots, opacities, colors)]
        n = arrs[0].shape[0]
        self._chk(self.L.gs_set_model_2d(self.h, n, *(a.ctypes.data for a in arrs), GS_MEM_HOST))

    def set_model_2d_device(self, n: int, ptrs):
        self._chk(self.L.gs_set_model_2d(self.h, n, *(int(p) for p in ptrs), GS_MEM_DEVICE))

    def set_active_sh_degree(self, degree: int = -1):
        """gs_set_active_sh_degree: evaluate the SH bands 0 .. degree only, on rows that keep the model's stride (-1: the model's own
        degree).  The request is the ctx's: it survives set_model_*; a change of the effective degree drops the frame."""
        self._chk(self.L.gs_set_active_sh_degree(self.h, int(degree)))

    @property
    def active_sh_degree(self) -> int:
        """gs_get_active_sh_degree: the effective degree, min(requested, the model's)."""
        rc = self.L.gs_get_active_sh_degree(self.h)
        if rc < 0:
            self._chk(rc)
        return int(rc)

    def set_background(self, rgb=(0.0, 0.0, 0.0)):
        """gs_set_background: the colour behind the last splat, image = C + T * bg (three finite floats; the default is black).  The request
        is the ctx's: it survives set_model_*; a changed value drops the image (backward wants a new forward), the lists stand."""
        vals = [float(x) for x in rgb]
        if len(vals) != 3:
            raise ValueError("set_background: three components (r, g, b)")
        self._chk(self.L.gs_set_background(self.h, (C.c_float * 3)(*vals)))

    @property
    def background(self) -> tuple:
        """gs_get_background: the current background as three floats."""
        o = (C.c_float * 3)()
        self._chk(self.L.gs_get_background(self.h, o))
        return (float(o[0]), float(o[1]), float(o[2]))

    def compose_target(self, rgba_ptr: int, W: int, H: int, out_ptr: int):
        """gs_compose_target: a straight-alpha target [4, H, W] over the ctx's background into [3, H, W], device buffers, on the ctx
        stream: out = rgba[c] * a + bg[c] * (1 - a), four fp32 operations.  No sync."""
        self._chk(self.L.gs_compose_target(self.h, int(rgba_ptr), int(W), int(H), int(out_ptr)))

    def set_image_size(self, W: int, H: int):
        self._chk(self.L.gs_set_image_size(self.h, int(W), int(H)))
        self.W, self.H = int(W), int(H)

    def set_camera(self, T, P, fx, fy, near, far, eye, lookAt, W, H):
        a = [np.ascontiguousarray(v, np.float32).reshape(-1) for v in (T, P, eye, lookAt)]
        self._chk(self.L.gs_set_camera(self.h, a[0].ctypes.data_as(_fp), a[1].ctypes.data_as(_fp), fx, fy, near, far,
                                       a[2].ctypes.data_as(_fp), a[3].ctypes.data_as(_fp), int(W), int(H)))
        self.W, self.H = int(W), int(H)

    def camera_record(self, T, P, fx, fy, near, far, eye, lookAt, W, H):
        """The arguments of gs_set_camera converted once (ctypes arrays): set_camera_record(rec) then costs one foreign call."""
        f16, f3 = C.c_float * 16, C.c_float * 3
        a = [np.ascontiguousarray(v, np.float32).reshape(-1) for v in (T, P, eye, lookAt)]
        return (f16(*a[0]), f16(*a[1]), float(fx), float(fy), float(near), float(far), f3(*a[2]), f3(*a[3]), int(W), int(H))

    def set_camera_record(self, rec):
        self._chk(self.L.gs_set_camera(self.h, *rec))
        self.W, self.H = rec[8], rec[9]

    def set_view_slot(self, slot: int):
        """gs_set_view_slot: name the view about to be rendered (e.g. the camera's id); -1 = none."""
        self._chk(self.L.gs_set_view_slot(self.h, int(slot)))

    # -- pipeline
    def preprocess(self):
        self._chk(self.L.gs_preprocess(self.h))

    def bin(self, gx: int = 0, gy: int = 0):
        self._chk(self.L.gs_bin(self.h, gx, gy))

    def forward_host(self):
        img = np.empty((3, self.H, self.W), np.float32)
        tr = np.empty((self.H, self.W), np.float32)
        self._chk(self.L.gs_forward(self.h, img.ctypes.data, tr.ctypes.data, GS_MEM_HOST))
        return img, tr

    def bind_outputs(self, image_ptr: int = 0, trans_ptr: int = 0):
        """gs_bind_outputs: the forward writes straight into these device buffers (0, 0 unbinds); they must stay valid and
        unmodified until the frame's last backward."""
        self._chk(self.L.gs_bind_outputs(self.h, image_ptr, trans_ptr))

    def forward_device(self, image_ptr: int = 0, trans_ptr: int = 0):
        self._chk(self.L.gs_forward(self.h, image_ptr, trans_ptr, GS_MEM_DEVICE))

    def backward(self, dC_ptr_or_array, grads: GsGrads, overwrite: bool = False, phase: str = "all"):
        """phase: "all", "composite" (GS_BWD_COMPOSITE_ONLY), "params" (GS_BWD_PARAMS_ONLY), or the chain in two steps:
        "params_sh" (GS_BWD_PARAMS_ONLY | GS_BWD_PARAMS_SH) then "params_geom" (GS_BWD_PARAMS_ONLY | GS_BWD_PARAMS_GEOM)."""
        flags = (GS_BWD_OVERWRITE if overwrite else 0) | _BWD_PHASE[phase]
        if isinstance(dC_ptr_or_array, np.ndarray):
            a = np.ascontiguousarray(dC_ptr_or_array, np.float32)
            self._chk(self.L.gs_backward_ex(self.h, a.ctypes.data, GS_MEM_HOST, C.byref(grads), flags))
        else:
            self._chk(self.L.gs_backward_ex(self.h, int(dC_ptr_or_array), GS_MEM_DEVICE, C.byref(grads), flags))

    def color_grads_pack(self, drgb_ptr: int):
        """d rgb of the last backward, packed [n, 3] into a device buffer (colour-factored exchange)."""
        self._chk(self.L.gs_color_grads_pack(self.h, int(drgb_ptr)))

    @staticmethod
    def _camera_records(cam_records) -> np.ndarray:
        """[nviews, 38] host float32 {T16, P16, eye3, lookAt3} (distributed.view_records), contiguous."""
        cr = np.ascontiguousarray(cam_records, np.float32)
        assert cr.ndim == 2 and cr.shape[1] == 38
        return cr

    def sh_grads_from_views(self, cam_records: np.ndarray, drgb_ptr: int, d_shs_ptr: int, overwrite: bool = True):
        """cam_records [nviews, 38] host float32 {T16, P16, eye3, lookAt3}; drgb [nviews, n, 3] device."""
        cr = self._camera_records(cam_records)
        self._chk(self.L.gs_sh_grads_from_views(self.h, cr.shape[0], cr.ctypes.data, int(drgb_ptr), int(d_shs_ptr), 1 if overwrite else 0))

    def color_rows_pack(self, drgb_ptr: "int | None", n: int, bits_ptr: int, rows_ptr: int, count_ptr: int):
        """gs_color_rows_pack: one view as a bitmap of touched gaussians (int32 words), their d rgb rows in gaussian order and an
        int64 count, all device buffers; drgb_ptr None / 0 = the ctx's own sums of the last backward (n = num_gaussians).  No sync."""
        self._chk(self.L.gs_color_rows_pack(self.h, int(drgb_ptr or 0), int(n), int(bits_ptr), int(rows_ptr), int(count_ptr)))

    def sh_grads_from_touched(self, cam_records: np.ndarray, bits_ptr: int, rows_ptr: int, rows_cap: int, d_shs_ptr: int,
                              overwrite: bool = True):
        """cam_records as sh_grads_from_views; bits [nviews, ceil(n / 32)] int32 and rows [nviews, rows_cap, 3] float32, device."""
        cr = self._camera_records(cam_records)
        self._chk(self.L.gs_sh_grads_from_touched(self.h, cr.shape[0], cr.ctypes.data, int(bits_ptr), int(rows_ptr), int(rows_cap), int(d_shs_ptr),
                                                  1 if overwrite else 0))

    def backward_sgd(self, dC_ptr: int, lr: float):
        """gs_backward_sgd: backward and `param .-= lr * grad` (train.jl:42-46) in one pass on the resident model; dC on the device."""
        self._chk(self.L.gs_backward_sgd(self.h, dC_ptr, GS_MEM_DEVICE, lr))

    def grads_alloc(self) -> GsGrads:
        """Library-owned flat gradient buffer (for hosts without a device allocator, e.g. plain Julia)."""
        g = GsGrads()
        self._chk(self.L.gs_grads_alloc(self.h, C.byref(g)))
        return g

    def _grads_read(self, grads: GsGrads, **rows) -> dict:
        """gs_grads_read into five host arrays, named and shaped [n, *rows[name]] in the order of the gs_grads slots."""
        n = self.num_gaussians
        out = {k: np.empty((n,) + row, np.float32) for k, row in rows.items()}
        self._chk(self.L.gs_grads_read(self.h, C.byref(grads), *(a.ctypes.data for a in out.values())))
        return out

    def grads_read(self, grads: GsGrads, sh_degree: int) -> dict:
        return self._grads_read(grads, means=(3,), scales=(3,), quats=(4,), opacities=(), shs=(3 * (sh_degree + 1) ** 2,))

    def grads_read_2d(self, grads: GsGrads) -> dict:
        """SplatGrads2D (splat.jl:28-34) from a gs_grads whose slots are read as (means, scales, rotations, opacities, colors)."""
        return self._grads_read(grads, means=(2,), scales=(2,), rots=(), opacities=(), colors=(3,))

    def loss_host(self, img: np.ndarray, gt: np.ndarray, lam: float = 0.1):
        """(loss, dC) for host images [C, H, W] (src/loss.jl:62-72 and its gradient)."""
        img = np.ascontiguousarray(img, np.float32); gt = np.ascontiguousarray(gt, np.float32)
        dC = np.empty_like(img)
        out = C.c_double()
        Cn, H, W = img.shape
        self._chk(self.L.gs_loss_l1_dssim(self.h, img.ctypes.data, gt.ctypes.data, W, H, Cn, lam, dC.ctypes.data, C.byref(out), GS_MEM_HOST))
        return float(out.value), dC

    def loss_device(self, img_ptr: int, gt_ptr: int, dC_ptr: int, W: int, H: int, Cn: int, lam: float = 0.1, want_loss: bool = True):
        out = C.c_double()
        self._chk(self.L.gs_loss_l1_dssim(self.h, img_ptr, gt_ptr, W, H, Cn, lam, dC_ptr,
                                          C.byref(out) if want_loss else None, GS_MEM_DEVICE))
        return float(out.value) if want_loss else None

    # -- RCCL directly through the C ABI (what the Julia glue uses; the Python mirror defaults to torch.distributed)
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = load().gs_comm_unique_id(buf)
        if rc != 0:
            raise GsError(rc, (load().gs_last_error(None) or b"").decode())
        return buf.raw

    def comm_init(self, rank: int, nranks: int, unique_id: bytes):
        self._chk(self.L.gs_comm_init(self.h, rank, nranks, unique_id))

    def allreduce_grads(self, grads: GsGrads):
        self._chk(self.L.gs_allreduce_grads(self.h, C.byref(grads)))

    def sgd_step(self, lr: float, grads: GsGrads):
        self._chk(self.L.gs_sgd_step(self.h, lr, C.byref(grads)))

    @staticmethod
    def _adam_args(exp_avg: GsGrads, exp_avg_sq: GsGrads, lr, beta1, beta2, eps, step, selective, flags) -> tuple:
        """The arguments gs_adam_step and gs_backward_adam share, from the moments on."""
        return (C.byref(exp_avg), C.byref(exp_avg_sq), (C.c_float * GS_ADAM_GROUPS)(*[float(x) for x in lr]), beta1, beta2, eps, int(step),
                (GS_ADAM_SELECTIVE if selective else 0) if flags is None else int(flags))

    def adam_step(self, grads: GsGrads, exp_avg: GsGrads, exp_avg_sq: GsGrads, lr, beta1: float, beta2: float, eps: float, step: int,
                  selective: bool = False, flags: "int | None" = None):
        """gs_adam_step: Adam on the resident model from the gradients of `grads` (a NULL array freezes its group); exp_avg /
        exp_avg_sq: caller-owned moment arrays of the same layout; lr: GS_ADAM_GROUPS rates; step counts from 1."""
        self._chk(self.L.gs_adam_step(self.h, C.byref(grads), *self._adam_args(exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, selective, flags)))

    def backward_adam(self, dC_ptr: int, exp_avg: GsGrads, exp_avg_sq: GsGrads, lr, beta1: float, beta2: float, eps: float, step: int,
                      selective: bool = False, flags: "int | None" = None):
        """gs_backward_adam: backward and gs_adam_step in one pass on the resident model (3-D renderer); dC on the device."""
        self._chk(self.L.gs_backward_adam(self.h, int(dC_ptr), GS_MEM_DEVICE,
                                          *self._adam_args(exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, selective, flags)))

    # -- density control (3-D renderer): statistics, clone / split / prune, opacity reset
    def density_accumulate(self, stats: GsDensityStats):
        """gs_density_accumulate: after a non-fused backward of the frame, stats += this view (|d L / d mu'| in NDC units, visibility,
        pixel extent).  No sync."""
        self._chk(self.L.gs_density_accumulate(self.h, C.byref(stats)))

    def density_decide(self, stats: GsDensityStats, params: GsDensityParams, action_ptr: int):
        """gs_density_decide: action[g] = 0 keep, 1 clone, 2 split, 3 prune (int32 device array of n words).  No sync."""
        self._chk(self.L.gs_density_decide(self.h, C.byref(stats), C.byref(params), int(action_ptr or 0)))

    def density_plan(self, action_ptr: int):
        """gs_density_plan: (survivors, clones, splits, pruned); n_out = survivors + clones + 2 * splits.  The one call that synchronises."""
        o = (C.c_int64 * 4)()
        self._chk(self.L.gs_density_plan(self.h, int(action_ptr or 0), o))
        return int(o[0]), int(o[1]), int(o[2]), int(o[3])

    def density_restructure(self, action_ptr: int, noise_ptr: "int | None", dst_model: GsGrads, src_sets, dst_sets, n_out: int):
        """gs_density_restructure: the planned model into dst_model (five device arrays of n_out rows) and the gradient-shaped
        src_sets into dst_sets (sequences of GsGrads, up to four).  The ctx's model is not switched.  No sync."""
        src_sets, dst_sets = list(src_sets), list(dst_sets)
        if len(src_sets) != len(dst_sets):
            raise ValueError("density_restructure: one destination per source set")
        k = len(src_sets)
        sa, da = (GsGrads * max(k, 1))(*src_sets), (GsGrads * max(k, 1))(*dst_sets)
        self._chk(self.L.gs_density_restructure(self.h, int(action_ptr or 0), int(noise_ptr or 0), C.byref(dst_model), k,
                                                sa, da, int(n_out)))

    def opacity_reset(self, max_logit: float, m_opac_ptr: int = 0, v_opac_ptr: int = 0):
        """gs_opacity_reset: opacity = min(opacity, max_logit) on the resident model (NaN stays), +0 into the two moment arrays."""
        self._chk(self.L.gs_opacity_reset(self.h, max_logit, int(m_opac_ptr or 0), int(v_opac_ptr or 0)))

    # -- MCMC densification (3-D renderer): plan, draws, relocation, noise, regularisers
    def mcmc_plan(self, min_opacity_logit: float, cdf_ptr: int, dead_ptr: int):
        """gs_mcmc_plan: the integer weights' inclusive prefix sum into cdf (uint64 device array of n words), the indices of the gaussians
        that are not alive, ascending, into dead (int32, n words); (alive, dead, total).  The one call of the five that synchronises."""
        o = (C.c_int64 * 3)()
        self._chk(self.L.gs_mcmc_plan(self.h, min_opacity_logit, int(cdf_ptr or 0), int(dead_ptr or 0), o))
        return int(o[0]), int(o[1]), int(o[2])

    def mcmc_sample(self, cdf_ptr: int, n: int, u_ptr: int, m: int, src_ptr: int):
        """gs_mcmc_sample: src[j] = the gaussian the uniform number u[j] points at on the CDF (int32, m words).  No sync."""
        self._chk(self.L.gs_mcmc_sample(self.h, int(cdf_ptr or 0), int(n), int(u_ptr or 0), int(m), int(src_ptr or 0)))

    def mcmc_relocate(self, src_ptr: int, dst_ptr: "int | None", m: int, min_opacity: float, sets=()):
        """gs_mcmc_relocate: in place on the resident model, gaussian dst[j] becomes a copy of src[j] and both get the corrected opacity and
        scales; dst_ptr None / 0: the first m entries of the current plan's dead list.  sets: up to four GsGrads whose rows of sources and
        destinations become +0 (Adam's moments).  No sync."""
        sets = list(sets)
        k = len(sets)
        sa = (GsGrads * max(k, 1))(*sets)
        self._chk(self.L.gs_mcmc_relocate(self.h, int(src_ptr or 0), int(dst_ptr or 0), int(m), min_opacity, k, sa))

    def mcmc_noise(self, z_ptr: int, lr: float, gate_k: float = 100.0, gate_t: float = 0.005):
        """gs_mcmc_noise: means += lr * gate(opacity) * Sigma z on the resident model, z: [n, 3] standard normals on the device.  No sync."""
        self._chk(self.L.gs_mcmc_noise(self.h, int(z_ptr or 0), lr, gate_k, gate_t))

    def mcmc_regularize(self, grads: GsGrads, c_opacity: float, c_scale: float):
        """gs_mcmc_regularize: d_opacities += c_opacity * sig (1 - sig), d_scales += c_scale * exp(scale) into `grads`.  The frame stands.  No sync."""
        self._chk(self.L.gs_mcmc_regularize(self.h, C.byref(grads), c_opacity, c_scale))

    # -- point-cloud initialisation: needs no model, camera or frame, and leaves the ctx's frame as it is
    def knn_mean_dist2(self, points_ptr: int, n: int, dist2_ptr: int):
        """gs_knn_mean_dist2: dist2[i] = the mean of the three smallest squared distances from point i to the other finite points (exact:
        bit for bit a brute force).  points: 3 x n device floats, dist2: n device floats.  No sync."""
        self._chk(self.L.gs_knn_mean_dist2(self.h, int(points_ptr or 0), int(n), int(dist2_ptr or 0)))

    def init_from_points(self, points_ptr: int, colors_ptr: "int | None", dist2_ptr: int, n: int, sh_degree: int, opacity_logit: float,
                         dst_model: GsGrads):
        """gs_init_from_points: the model a training run starts from, into dst_model (five device arrays of n rows).  colors_ptr None / 0:
        grey.  The ctx's model is not switched.  No sync."""
        self._chk(self.L.gs_init_from_points(self.h, int(points_ptr or 0), int(colors_ptr or 0), int(dist2_ptr or 0), int(n), int(sh_degree),
                                             opacity_logit, C.byref(dst_model)))

    # -- feature maps (3-D renderer): depth, opacity and per-gaussian features through the frame's own composite launches
    def view_depth(self, z_ptr: int):
        """gs_view_depth: z[g] = the view-space depth ts[2] of gaussian g (n device floats; GS_ARR_TS row 2 bit for bit).  Needs a model and
        a camera, no frame.  No sync."""
        self._chk(self.L.gs_view_depth(self.h, int(z_ptr or 0)))

    def view_depth_backward(self, dz_ptr: int, d_means_ptr: int):
        """gs_view_depth_backward: d_means[g][j] += T[2 + 4 j] * dz[g]; rows whose dz compares == 0 are left unread.  No sync."""
        self._chk(self.L.gs_view_depth_backward(self.h, int(dz_ptr or 0), int(d_means_ptr or 0)))

    def render_features(self, feat_ptr: int, out_ptr: int, trans_ptr: int = 0):
        """gs_render_features: out [3, H, W] = sum feat[g] * alpha * T over the finished frame's own walk (feat [n, 3] device floats); no
        background; trans_ptr 0: the transmittance is not wanted.  The frame stays as forward left it.  No sync."""
        self._chk(self.L.gs_render_features(self.h, int(feat_ptr or 0), int(out_ptr or 0), int(trans_ptr or 0)))

    def backward_features(self, feat_ptr: int, image_f_ptr: int, dF_ptr: int, d_feat_ptr: int, grads: "GsGrads | None"):
        """gs_backward_features: the gradients of sum out . dF -- d_feat [n, 3] overwritten, the alpha path accumulated into the means,
        scales, quaternions and opacities of `grads` (None: d_feat only; d_shs is not touched).  No sync."""
        self._chk(self.L.gs_backward_features(self.h, int(feat_ptr or 0), int(image_f_ptr or 0), int(dF_ptr or 0), int(d_feat_ptr or 0),
                                              C.byref(grads) if grads is not None else None))

    def backward_camera(self, out_ptr: "int | None" = None):
        """gs_backward_camera: the frame's gradient into the arguments of set_camera, GS_CAMERA_GRAD_FLOATS floats {d_T[16], d_P[16], d_eye[3],
        d_lookAt[3], d_fx, d_fy} (overwritten).  Needs the frame's colour backward and must precede anything that steps the model.
        out_ptr None: returned as a float32 array (synchronises); else a device pointer that is filled on the stream (no sync)."""
        if out_ptr is None:
            out = np.empty(GS_CAMERA_GRAD_FLOATS, np.float32)
            self._chk(self.L.gs_backward_camera(self.h, out.ctypes.data, GS_MEM_HOST))
            return out
        self._chk(self.L.gs_backward_camera(self.h, int(out_ptr), GS_MEM_DEVICE))
        return None

    # -- evaluation metrics: needs no model, camera or frame, and leaves the ctx's frame as it is
    def image_metrics_host(self, img: np.ndarray, gt: np.ndarray, weight: "np.ndarray | None" = None, want_map: bool = False):
        """gs_image_metrics on host images [C, H, W] (weight [H, W] or None): (sums, ssim_map) with sums the four float64 values
        {sum w (x - y)^2, sum w |x - y|, sum w S, sum w} and ssim_map float32 [C, H, W] or None.  Synchronises."""
        img = np.ascontiguousarray(img, np.float32); gt = np.ascontiguousarray(gt, np.float32)
        if img.ndim != 3 or img.shape != gt.shape:
            raise ValueError("image_metrics: img and gt must be [C, H, W] arrays of one shape")
        Cn, H, W = img.shape
        if weight is not None:
            weight = np.ascontiguousarray(weight, np.float32)
            if weight.shape != (H, W):
                raise ValueError(f"image_metrics: the weight must be [{H}, {W}], not {weight.shape}")
        sums = np.empty(GS_METRIC_SUMS, np.float64)
        smap = np.empty_like(img) if want_map else None
        self._chk(self.L.gs_image_metrics(self.h, img.ctypes.data, gt.ctypes.data, weight.ctypes.data if weight is not None else None, W, H, Cn,
                                          smap.ctypes.data if smap is not None else None, sums.ctypes.data, GS_MEM_HOST))
        return sums, smap

    def image_metrics_device(self, img_ptr: int, gt_ptr: int, weight_ptr: int, W: int, H: int, Cn: int, map_ptr: int, sums_ptr: int):
        """gs_image_metrics with device pointers (weight_ptr / map_ptr 0: none); sums_ptr: four device float64.  On the ctx stream, no sync."""
        self._chk(self.L.gs_image_metrics(self.h, int(img_ptr or 0), int(gt_ptr or 0), int(weight_ptr or 0),
                                          int(W), int(H), int(Cn), int(map_ptr or 0), int(sums_ptr or 0), GS_MEM_DEVICE))

    # -- per-view exposure: needs no model, camera or frame, and leaves the ctx's frame as it is.  Device pointers, no sync
    def exposure_apply(self, img_ptr: int, exposure_ptr: int, weight_ptr: int, W: int, H: int, out_ptr: int):
        """gs_exposure_apply: out [3, H, W] = w * (M img + b) per pixel, E = [M | b] 12 device floats (row-major 3 x 4), weight_ptr 0: none."""
        self._chk(self.L.gs_exposure_apply(self.h, int(img_ptr or 0), int(exposure_ptr or 0), int(weight_ptr or 0), int(W), int(H),
                                           int(out_ptr or 0)))

    def exposure_backward(self, img_ptr: int, d_out_ptr: int, exposure_ptr: int, weight_ptr: int, W: int, H: int, d_img_ptr: int,
                          d_exposure_ptr: int = 0):
        """gs_exposure_backward: d_img (may be d_out itself) and, unless d_exposure_ptr is 0, the 12 floats of d_exposure (overwritten)."""
        self._chk(self.L.gs_exposure_backward(self.h, int(img_ptr or 0), int(d_out_ptr or 0), int(exposure_ptr or 0), int(weight_ptr or 0),
                                              int(W), int(H), int(d_img_ptr or 0), int(d_exposure_ptr or 0)))

    def exposure_adam(self, exposure_ptr: int, d_exposure_ptr: int, exp_avg_ptr: int, exp_avg_sq_ptr: int, lr: float, beta1: float, beta2: float,
                      eps: float, step: int):
        """gs_exposure_adam: one Adam step of a row of 12 floats (gs_adam_step's update); step counts from 1 and is the row's own."""
        self._chk(self.L.gs_exposure_adam(self.h, int(exposure_ptr or 0), int(d_exposure_ptr or 0), int(exp_avg_ptr or 0),
                                          int(exp_avg_sq_ptr or 0), float(lr), float(beta1), float(beta2), float(eps), int(step)))

    # -- per-view bilateral grid: needs no model, camera or frame, and leaves the ctx's frame as it is.  Device pointers, no sync
    def bilagrid_apply(self, img_ptr: int, grid_ptr: int, dims, weight_ptr: int, W: int, H: int, out_ptr: int):
        """gs_bilagrid_apply: out [3, H, W] = w * (A img + b) per pixel, [A | b] sliced from the grid [Gz, Gy, Gx, 12]; dims = (Gx, Gy, Gz)."""
        gx, gy, gz = dims
        self._chk(self.L.gs_bilagrid_apply(self.h, int(img_ptr or 0), int(grid_ptr or 0), int(gx), int(gy), int(gz), int(weight_ptr or 0),
                                           int(W), int(H), int(out_ptr or 0)))

    def bilagrid_backward(self, img_ptr: int, d_out_ptr: int, grid_ptr: int, dims, weight_ptr: int, W: int, H: int, d_img_ptr: int,
                          d_grid_ptr: int = 0):
        """gs_bilagrid_backward: d_img (may be d_out itself) and, unless d_grid_ptr is 0, every float of d_grid (overwritten)."""
        gx, gy, gz = dims
        self._chk(self.L.gs_bilagrid_backward(self.h, int(img_ptr or 0), int(d_out_ptr or 0), int(grid_ptr or 0), int(gx), int(gy), int(gz),
                                              int(weight_ptr or 0), int(W), int(H), int(d_img_ptr or 0), int(d_grid_ptr or 0)))

    def bilagrid_tv(self, grid_ptr: int, dims, coef: float, d_grid_ptr: int = 0, tv_ptr: int = 0):
        """gs_bilagrid_tv: the total variation into one device float64 (tv_ptr) and the gradient of coef * tv added to d_grid; 0: not wanted."""
        gx, gy, gz = dims
        self._chk(self.L.gs_bilagrid_tv(self.h, int(grid_ptr or 0), int(gx), int(gy), int(gz), float(coef), int(d_grid_ptr or 0), int(tv_ptr or 0)))

    def bilagrid_adam(self, grid_ptr: int, d_grid_ptr: int, exp_avg_ptr: int, exp_avg_sq_ptr: int, n_floats: int, lr: float, beta1: float,
                      beta2: float, eps: float, step: int):
        """gs_bilagrid_adam: one Adam step of a view's grid (gs_adam_step's update); step counts from 1 and is the view's own."""
        self._chk(self.L.gs_bilagrid_adam(self.h, int(grid_ptr or 0), int(d_grid_ptr or 0), int(exp_avg_ptr or 0), int(exp_avg_sq_ptr or 0),
                                          int(n_floats), float(lr), float(beta1), float(beta2), float(eps), int(step)))

    def reset_grads(self, grads: GsGrads):
        self._chk(self.L.gs_reset_grads(self.h, C.byref(grads)))

    # -- introspection
    @property
    def num_gaussians(self) -> int:
        return int(self.L.gs_num_gaussians(self.h))

    @property
    def num_instances(self) -> int:
        return int(self.L.gs_num_instances(self.h))

    @property
    def num_coarse_instances(self) -> int:
        """two-level binning: (super-tile, gaussian) instances of the last bin()"""
        return int(self.L.gs_num_coarse_instances(self.h))

    @property
    def num_rounds(self) -> int:
        """binning rounds of the last bin(): 1 = classic full lists, 2..4 = depth slabs"""
        return int(self.L.gs_num_rounds(self.h))

    def get_array(self, which: int, gx: int | None = None, gy: int | None = None) -> np.ndarray:
        n, ni = self.num_gaussians, self.num_instances
        spec = {ARR_TS: ((n, 4), np.float32), ARR_TPS: ((n, 4), np.float32), ARR_MU: ((n, 2), np.float32),
                ARR_COV3D: ((n, 9), np.float32), ARR_COV2D: ((n, 4), np.float32), ARR_INVCOV: ((n, 4), np.float32),
                ARR_BBS: ((n, 4), np.float32), ARR_RGB: ((n, 3), np.float32), ARR_SIG: ((n,), np.float32),
                ARR_DEPTH_KEY: ((n,), np.uint32), ARR_TILE_RECT: ((n, 4), np.uint16), ARR_SORT_IDXS: ((n,), np.uint32),
                ARR_SORTED_IDS: ((ni,), np.uint32), ARR_SORTED_KEYS: ((ni,), np.uint64), ARR_GRAD2D: ((n, 10), np.float32)}
        if which == ARR_TILE_RANGES:
            ntiles = ((self.W + 15) // 16) * ((self.H + 15) // 16)
            shape, dt = (ntiles, 2), np.uint32
        else:
            shape, dt = spec[which]
        out = np.empty(shape, dt)
        self._chk(self.L.gs_get_array(self.h, which, out.ctypes.data, out.nbytes))
        return out

    def stage_stats(self, reset: bool = False) -> dict:
        """{stage: (sum_ms, launches)} accumulated by hipEvents on the ctx stream since the last reset."""
        sm = (C.c_double * len(STAGES))()
        ct = (C.c_int64 * len(STAGES))()
        self._chk(self.L.gs_get_stage_stats(self.h, sm, ct, int(reset)))
        return {k: (float(sm[i]), int(ct[i])) for i, k in enumerate(STAGES)}

    def work_counters(self):
        a, b = C.c_int64(), C.c_int64()
        self._chk(self.L.gs_get_work_counters(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def work_counters_ex(self) -> dict:
        """walked = list entries staged; evaluated = those that survived the alpha_cull no-op test."""
        o = (C.c_int64 * 4)()
        self._chk(self.L.gs_get_work_counters_ex(self.h, o))
        return dict(walked_fwd=int(o[0]), walked_bwd=int(o[1]), evaluated_fwd=int(o[2]), evaluated_bwd=int(o[3]))

    def list_stats(self) -> dict:
        """entries written into the tile lists of the last frame, list segments appended by composite waves, capped or not"""
        o = (C.c_int64 * 3)()
        self._chk(self.L.gs_get_list_stats(self.h, o))
        return dict(listed=int(o[0]), extended_segments=int(o[1]), capped=bool(o[2]))

    def tile_parts_of_frame(self) -> int:
        """waves per tile (1, 2, 4) of the last frame's composite launches (gs_config.tile_parts)"""
        rc = self.L.gs_get_tile_parts(self.h)
        if rc < 0:
            self._chk(rc)
        return int(rc)

    def bin_path_of_frame(self) -> int:
        """the path that built the last frame's lists: 0 two-level, 1 / 2 radix, 3 small-frame path (gs_config.bin_path)"""
        rc = self.L.gs_get_bin_path(self.h)
        if rc < 0:
            self._chk(rc)
        return int(rc)

    def time_composite(self, which: int, variant: int, reps: int = 10) -> float:
        ms = C.c_float()
        self._chk(self.L.gs_debug_time_composite(self.h, which, variant, reps, C.byref(ms)))
        return float(ms.value)

    def tile_clock(self, which: int, variant: int = 0) -> np.ndarray:
        """[ntiles, 15] uint64 per tile {start, end (100 MHz ticks), HW_ID | XCC_ID << 32, walked << 32 | evaluated, shader cycles
        inside the per-entry loops, shader cycles outside them, strip slots executed << 32 | slots with live pixels packed,
        strips with a live pixel << 32 | live pixels} of one composite launch (which: 0 forward, 1 backward)."""
        ntiles = ((self.W + 15) // 16) * ((self.H + 15) // 16)
        rows = ntiles
        if variant < 0:                                     # one record per workgroup of the launch (split tiles as production runs them)
            rows = int(self.L.gs_debug_tile_clock_rows(self.h))
            if rows <= 0:
                raise GsError(-1, "tile_clock: records by workgroup need a frame with a launch order")
        out = np.zeros((rows, 15), np.uint64)
        self._chk(self.L.gs_debug_tile_clock(self.h, which, variant, out.ctypes.data))
        return out

    def tail_fill_blocks(self):
        """(forward, backward): fill workgroups the last frame's composite launches carried at the end of their grids (0: the in-line form)"""
        o = (C.c_int32 * 2)()
        self._chk(self.L.gs_debug_tail_fill(self.h, o))
        return int(o[0]), int(o[1])

    def tile_clock_rows(self) -> int:
        """workgroups of the frame's composite launches as gs_debug_tile_clock records them (0: one wave per tile, no launch order)"""
        return int(self.L.gs_debug_tile_clock_rows(self.h))

    def set_debug_window(self, start: int = 0, length: int = 0):
        """debug launches cover only order[start : start + length] of the frame's launch order (0, 0: all of it)"""
        self._chk(self.L.gs_debug_set_window(self.h, start, length))

    def clock_mhz(self) -> float:
        """the shader clock the chip runs at right now (one wave counting cycles over 20 us; waits for the stream)"""
        mhz = C.c_float()
        self._chk(self.L.gs_debug_clock_mhz(self.h, C.byref(mhz)))
        return float(mhz.value)

    @property
    def rank_probe_result(self) -> int:
        return int(self.L.gs_rank_probe_result(self.h))

    def stage_times(self) -> dict:
        ms = (C.c_float * len(STAGES))()
        self._chk(self.L.gs_get_stage_times(self.h, ms))
        return {k: float(ms[i]) for i, k in enumerate(STAGES)}
