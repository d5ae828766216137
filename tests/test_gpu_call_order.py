"""The order in which the C ABI accepts its calls, pinned call by call: what a fresh ctx refuses (code and message), what every
call leaves of a complete frame, the two phases of the backward, the flag errors of the backward family, that a refused call
changes nothing, and that a closed ctx gives its device memory back."""
import ctypes as C

import numpy as np
import pytest

from common import hip_context, refused, scene_and_cameras
from gaussiansplat_amd import synthetic

pytestmark = pytest.mark.gpu

N, DEG, W, H = 64, 1, 48, 32
WIDTHS = [3, 3, 4, 1, 3 * (DEG + 1) ** 2]
N2D = 32
LR6, B1, B2, EPS = [1e-3] * 6, 0.9, 0.999, 1e-8
COMPOSITE_ONLY, PARAMS_ONLY, PARAMS_SH = 2, 4, 8            # GS_BWD_* (include/gsplat.h)
KEYS = ("means", "scales", "quats", "opacities", "shs")


def _scene(seed=3):
    return scene_and_cameras(N, W, H, DEG, seed)


def _ctx3d(seed=3, **kw):
    sc, cam, T, P, _ = _scene(seed)
    return hip_context(sc, cam, T, P, W, H, DEG, **kw)


def _ctx2d(**kw):
    from gaussiansplat_amd import backend as B
    sc = synthetic.make_scene_2d(N2D, W, H, 5)
    ctx = B.Context(order=B.ORDER_INDEX, **kw)
    ctx.set_model_2d_host(sc["means"], sc["scales"], sc["rots"], sc["opacities"], sc["colors"])
    ctx.set_image_size(W, H)
    return ctx


class _Moments:
    """two zeroed moment sets on the device, as gs_grads"""

    def __init__(self):
        import torch
        from gaussiansplat_amd import backend as B
        self.t = [[torch.zeros(N * w, dtype=torch.float32, device="cuda") for w in WIDTHS] for _ in range(2)]
        self.m, self.v = (B.GsGrads(*(x.data_ptr() for x in ts)) for ts in self.t)


def _dC_dev(seed=3):
    import torch
    return torch.as_tensor(synthetic.make_dC(W, H, seed)).cuda()


def _backward_ex(ctx, dC_ptr, grads, flags):
    ctx._chk(ctx.L.gs_backward_ex(ctx.h, C.c_void_p(dC_ptr), 1, C.byref(grads) if grads is not None else None, flags))


def _frame(ctx, dC, g):
    ctx.preprocess(); ctx.bin(); ctx.forward_device()
    ctx.backward(dC.data_ptr(), g, overwrite=True)


def test_fresh_ctx_refuses_every_call_out_of_order():
    import torch
    from gaussiansplat_amd import backend as B
    sc, cam, T, P, _ = _scene()
    ctx = B.Context()
    ctx.set_model_host(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"].reshape(N, WIDTHS[4]), DEG)
    ctx.W, ctx.H = W, H
    dC, mo = _dC_dev(), _Moments()
    g = ctx.grads_alloc()
    scratch = torch.zeros(4 * N + 64, dtype=torch.float32, device="cuda")
    p = scratch.data_ptr()
    refused(ctx.preprocess, "gs_preprocess: gs_set_camera first")
    refused(ctx.bin, "gs_bin: gs_preprocess first")
    refused(ctx.forward_device, "gs_forward: gs_bin first")
    for call in (lambda: ctx._chk(ctx.L.gs_backward(ctx.h, C.c_void_p(dC.data_ptr()), 1, C.byref(g))),
                 lambda: ctx.backward(dC.data_ptr(), g, overwrite=True),
                 lambda: ctx.backward(dC.data_ptr(), g, phase="composite"),
                 lambda: ctx.backward(dC.data_ptr(), g, phase="params"),
                 lambda: ctx.backward_sgd(dC.data_ptr(), 1e-3),
                 lambda: ctx.backward_adam(dC.data_ptr(), mo.m, mo.v, LR6, B1, B2, EPS, 1),
                 lambda: ctx.backward_adam(dC.data_ptr(), mo.m, mo.v, LR6, B1, B2, EPS, 1, selective=True)):
        refused(call, "gs_backward: gs_forward first")
    refused(lambda: ctx.get_array(B.ARR_DEPTH_KEY), "gs_get_array: gs_preprocess first")
    refused(lambda: ctx.get_array(B.ARR_TILE_RECT), "gs_get_array: gs_preprocess first")
    refused(lambda: ctx.get_array(B.ARR_SORT_IDXS), "gs_get_array: gs_bin first")
    refused(lambda: ctx.get_array(B.ARR_TILE_RANGES), "gs_get_array: gs_bin first")
    refused(lambda: ctx.get_array(B.ARR_GRAD2D), "gs_get_array: gs_backward first")
    refused(lambda: ctx.color_grads_pack(p), "gs_color_grads_pack: gs_backward first")
    refused(lambda: ctx.color_rows_pack(None, N, p, p + 64, p + 4 * 64 + 12 * N), "gs_color_rows_pack: gs_backward first")
    refused(ctx.tile_parts_of_frame, "gs_get_tile_parts: gs_forward first")
    refused(ctx.work_counters, "gs_get_work_counters: gs_forward first")
    refused(ctx.work_counters_ex, "gs_get_work_counters_ex: gs_forward first")
    refused(ctx.list_stats, "gs_get_list_stats: gs_forward first")
    refused(ctx.tail_fill_blocks, "gs_debug_tail_fill: gs_forward first")
    refused(ctx.bin_path_of_frame, "gs_get_bin_path: gs_bin first")
    refused(lambda: ctx.time_composite(0, 0, 1), "gs_debug_time_composite: gs_forward first")
    # the frame step by step: each call opens the next one and nothing beyond it
    ctx.set_camera(T, P, float(np.float32(cam.fx)), float(np.float32(cam.fy)), float(np.float32(cam.near)), float(np.float32(cam.far)),
                   cam.eye, cam.lookAt, W, H)
    ctx.preprocess()
    assert ctx.get_array(B.ARR_DEPTH_KEY).shape == (N,)
    refused(lambda: ctx.get_array(B.ARR_SORT_IDXS), "gs_get_array: gs_bin first")
    refused(ctx.forward_device, "gs_forward: gs_bin first")
    ctx.bin()
    assert ctx.get_array(B.ARR_SORT_IDXS).shape == (N,) and ctx.bin_path_of_frame() in (0, 1, 2, 3)
    refused(lambda: ctx.backward(dC.data_ptr(), g), "gs_backward: gs_forward first")
    refused(ctx.tile_parts_of_frame, "gs_get_tile_parts: gs_forward first")
    ctx.forward_device()
    assert ctx.tile_parts_of_frame() in (1, 2, 4) and ctx.time_composite(0, 0, 1) >= 0.0
    refused(lambda: ctx.time_composite(1, 0, 1), "gs_debug_time_composite: gs_backward first")
    refused(lambda: ctx.get_array(B.ARR_GRAD2D), "gs_get_array: gs_backward first")
    refused(lambda: ctx.color_grads_pack(p), "gs_color_grads_pack: gs_backward first")
    ctx.backward(dC.data_ptr(), g, overwrite=True)
    assert ctx.time_composite(1, 0, 1) >= 0.0 and ctx.get_array(B.ARR_GRAD2D).shape == (N, 10)
    ctx.close()


def test_what_each_call_leaves_of_a_complete_frame():
    from gaussiansplat_amd import backend as B
    sc, cam, T, P, _ = _scene()
    ctx = hip_context(sc, cam, T, P, W, H, DEG)
    dC, mo = _dC_dev(), _Moments()
    g = ctx.grads_alloc()
    camera = (T, P, float(np.float32(cam.fx)), float(np.float32(cam.fy)), float(np.float32(cam.near)), float(np.float32(cam.far)),
              cam.eye, cam.lookAt, W, H)
    # the model or the view changed: the frame is gone, down to the preprocess
    for call in (lambda: ctx.set_model_host(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"].reshape(N, WIDTHS[4]), DEG),
                 lambda: ctx.set_camera(*camera),
                 lambda: ctx.set_image_size(W, H),
                 lambda: ctx.sgd_step(1e-3, g),
                 lambda: ctx.adam_step(g, mo.m, mo.v, LR6, B1, B2, EPS, 1),
                 lambda: ctx.backward_sgd(dC.data_ptr(), 1e-3),
                 lambda: ctx.backward_adam(dC.data_ptr(), mo.m, mo.v, LR6, B1, B2, EPS, 2)):
        _frame(ctx, dC, g)
        call()
        refused(ctx.bin, "gs_bin: gs_preprocess first")
        refused(ctx.forward_device, "gs_forward: gs_bin first")
        refused(lambda: ctx.backward(dC.data_ptr(), g), "gs_backward: gs_forward first")
        refused(lambda: ctx.get_array(B.ARR_DEPTH_KEY), "gs_get_array: gs_preprocess first")
    # other output buffers: the lists stand, the picture does not
    _frame(ctx, dC, g)
    ctx.bind_outputs()
    refused(lambda: ctx.backward(dC.data_ptr(), g), "gs_backward: gs_forward first")
    refused(lambda: ctx.get_array(B.ARR_GRAD2D), "gs_get_array: gs_backward first")
    ctx.forward_device()                                                    # accepted without a new gs_bin
    ctx.backward(dC.data_ptr(), g, overwrite=True)
    # a new preprocess
    ctx.preprocess()
    refused(ctx.forward_device, "gs_forward: gs_bin first")
    refused(lambda: ctx.backward(dC.data_ptr(), g), "gs_backward: gs_forward first")
    # a new bin
    _frame(ctx, dC, g)
    ctx.bin()
    refused(lambda: ctx.backward(dC.data_ptr(), g), "gs_backward: gs_forward first")
    refused(lambda: ctx.get_array(B.ARR_GRAD2D), "gs_get_array: gs_backward first")
    # a second forward: the first one's composite adjoint is gone
    _frame(ctx, dC, g)
    ctx.forward_device()
    refused(lambda: ctx.backward(dC.data_ptr(), g, phase="params"), "gs_backward: GS_BWD_PARAMS_ONLY needs a GS_BWD_COMPOSITE_ONLY call on this frame")
    refused(lambda: ctx.get_array(B.ARR_GRAD2D), "gs_get_array: gs_backward first")
    refused(lambda: ctx.time_composite(1, 0, 1), "gs_debug_time_composite: gs_backward first")
    ctx.backward(dC.data_ptr(), g, overwrite=True)                          # ... and the frame is still good for a whole backward
    ctx.synchronize()
    ctx.close()


def test_phases_of_the_backward():
    import torch
    from gaussiansplat_amd import backend as B
    ctx = _ctx3d(deterministic=True)
    dC = _dC_dev()
    g = ctx.grads_alloc()
    drgb = torch.zeros(3 * N, dtype=torch.float32, device="cuda")
    ctx.preprocess(); ctx.bin(); ctx.forward_device()
    ctx.backward(dC.data_ptr(), g, phase="composite")
    g2d = ctx.get_array(B.ARR_GRAD2D)
    ctx.color_grads_pack(drgb.data_ptr())
    ctx.synchronize()
    assert np.array_equal(drgb.cpu().numpy().reshape(N, 3), g2d[:, :3])
    ctx.backward(dC.data_ptr(), g, overwrite=True, phase="params")
    first = {k: v.copy() for k, v in ctx.grads_read(g, DEG).items()}
    ctx.backward(dC.data_ptr(), g, overwrite=True, phase="params")         # the sums still stand: the same bits again
    second = ctx.grads_read(g, DEG)
    assert any(np.any(first[k] != 0) for k in KEYS)
    for k in KEYS:
        assert first[k].tobytes() == second[k].tobytes(), k
    # ... and they are those of one whole backward
    ctx.backward(dC.data_ptr(), g, overwrite=True)
    whole = ctx.grads_read(g, DEG)
    for k in KEYS:
        assert first[k].tobytes() == whole[k].tobytes(), k
    ctx.close()


def test_flag_errors_one_fault_per_call():
    from gaussiansplat_amd import backend as B
    ctx = _ctx3d()
    dC, mo = _dC_dev(), _Moments()
    g = ctx.grads_alloc()
    ctx.preprocess(); ctx.bin(); ctx.forward_device()
    refused(lambda: _backward_ex(ctx, dC.data_ptr(), g, COMPOSITE_ONLY | PARAMS_ONLY), "gs_backward: COMPOSITE_ONLY and PARAMS_ONLY exclude each other")
    refused(lambda: _backward_ex(ctx, dC.data_ptr(), g, PARAMS_SH), "gs_backward: GS_BWD_PARAMS_SH / _GEOM need GS_BWD_PARAMS_ONLY")
    refused(lambda: ctx.backward_sgd(dC.data_ptr(), 0.0), "gs_backward_sgd: lr must be non-zero")
    refused(lambda: _backward_ex(ctx, 0, g, 1), "gs_backward: NULL argument")
    refused(lambda: _backward_ex(ctx, dC.data_ptr(), None, 1), "gs_backward: NULL argument")
    refused(lambda: ctx.backward_sgd(0, 1e-3), "gs_backward: NULL argument")
    refused(lambda: ctx.backward_adam(0, mo.m, mo.v, LR6, B1, B2, EPS, 1), "gs_backward_adam: NULL argument")
    refused(lambda: ctx._chk(ctx.L.gs_backward_ex(ctx.h, C.c_void_p(dC.data_ptr()), 7, C.byref(g), 1)), "gs_backward: bad mem")
    ctx.backward(dC.data_ptr(), g, overwrite=True)                          # none of them touched the frame
    ctx.synchronize()
    ctx.close()
    c2 = _ctx2d()
    g2 = c2.grads_alloc()
    c2.preprocess(); c2.bin(); c2.forward_device()
    refused(lambda: _backward_ex(c2, dC.data_ptr(), g2, PARAMS_ONLY | PARAMS_SH), "gs_backward: GS_BWD_PARAMS_SH / _GEOM: 3-D renderer only", B.GS_ERR_UNSUPPORTED)
    refused(lambda: c2.backward_sgd(dC.data_ptr(), 1e-3), "gs_backward_sgd: 3-D renderer only", B.GS_ERR_UNSUPPORTED)
    refused(lambda: c2.backward_adam(dC.data_ptr(), mo.m, mo.v, LR6, B1, B2, EPS, 1), "gs_backward_adam: 3-D renderer only", B.GS_ERR_UNSUPPORTED)
    c2.backward(dC.data_ptr(), g2, overwrite=True)
    got = c2.grads_read_2d(g2)
    assert all(np.all(np.isfinite(v)) for v in got.values()) and np.any(got["colors"] != 0)
    c2.close()


def test_a_refused_call_changes_nothing():
    dC, mo = _dC_dev(), _Moments()
    out = []
    for refuse in (True, False):
        ctx = _ctx3d(deterministic=True)
        g = ctx.grads_alloc()
        ctx.preprocess(); ctx.bin(); ctx.forward_device()
        if refuse:
            refused(lambda: ctx.backward_adam(dC.data_ptr(), mo.m, mo.v, LR6, 1.0, B2, EPS, 1), "gs_backward_adam: betas must lie in [0, 1)")
            refused(lambda: ctx.backward_adam(dC.data_ptr(), mo.m, mo.v, LR6, B1, -0.5, EPS, 1, selective=True), "gs_backward_adam: betas must lie in [0, 1)")
            refused(lambda: ctx.backward_sgd(dC.data_ptr(), 0.0), "gs_backward_sgd: lr must be non-zero")
            refused(lambda: _backward_ex(ctx, dC.data_ptr(), g, 1 | COMPOSITE_ONLY | PARAMS_ONLY), "exclude each other")
            refused(lambda: _backward_ex(ctx, dC.data_ptr(), g, 1 | PARAMS_ONLY), "needs a GS_BWD_COMPOSITE_ONLY call on this frame")
        ctx.backward(dC.data_ptr(), g, overwrite=True)
        out.append({k: v.copy() for k, v in ctx.grads_read(g, DEG).items()})
        ctx.close()
    assert all(float(t.abs().max()) == 0.0 for ts in mo.t for t in ts)    # the moments of the refused calls: untouched
    assert any(np.any(out[0][k] != 0) for k in KEYS)
    for k in KEYS:
        assert out[0][k].tobytes() == out[1][k].tobytes(), k


def test_a_closed_ctx_gives_its_memory_back():
    """Eight times create, one whole frame with backward, close.  F = the device memory a live ctx holds; after cycle 8 no more
    than F / 2 less is free than after cycle 2 (a coarse guard: a sixth of a ctx leaked per cycle would show)."""
    import torch
    n, deg, w, h = 20_000, 3, 256, 256
    sc, cam, T, P, _ = scene_and_cameras(n, w, h, deg, 17)
    dC = synthetic.make_dC(w, h, 17)
    torch.cuda.synchronize()
    free_after, held = [], []
    for cycle in range(8):
        before = torch.cuda.mem_get_info()[0]
        ctx = hip_context(sc, cam, T, P, w, h, deg)
        g = ctx.grads_alloc()
        ctx.preprocess(); ctx.bin(); ctx.forward_host()
        ctx.backward(dC, g, overwrite=True)
        ctx.synchronize()
        held.append(before - torch.cuda.mem_get_info()[0])
        ctx.close()
        free_after.append(torch.cuda.mem_get_info()[0])
    F = held[0]
    print("held per ctx", held, "free after each cycle", free_after)
    assert F > 0
    assert free_after[7] >= free_after[1] - F // 2, (free_after, F)
