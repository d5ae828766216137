"""Shared helpers of the tests, each written once: scene/camera set-up identical for the oracle and the HIP path, the bit comparisons (the
bar in the name or in an explicit argument), the ctx-level frame, the renderer-level scenes, the refusal check, and the host programs of
tests/*_host.cpp (built through tests/Makefile, one compile per session) with their in.bin / out.bin round trip."""
import os
import subprocess

import numpy as np
import pytest

from gaussiansplat_amd import camera as gcam
from gaussiansplat_amd import synthetic

TESTS = os.path.dirname(os.path.abspath(__file__))
GRADS = ("means", "scales", "quats", "opacities", "shs")


def scene_and_cameras(n, W, H, deg, seed, view=0):
    from oracle import oracle as O
    sc = synthetic.make_scene(n, W, H, deg, seed=seed)
    cam = synthetic.scene_camera(W, view=view)
    T = gcam.compute_transform(cam)
    P = gcam.compute_projection(cam, W, H)
    ocam = O.camera_from_arrays(T, P, np.float32(cam.fx), np.float32(cam.fy), np.float32(cam.near), np.float32(cam.far),
                                cam.eye, cam.lookAt, W, H)
    return sc, cam, T, P, ocam


def hip_context(sc, cam, T, P, W, H, deg, **kw):
    from gaussiansplat_amd import backend as B
    ctx = B.Context(**kw)
    n = sc["means"].shape[0]
    ctx.set_model_host(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"].reshape(n, 3 * (deg + 1) ** 2), deg)
    ctx.set_camera(T, P, float(np.float32(cam.fx)), float(np.float32(cam.fy)), float(np.float32(cam.near)),
                   float(np.float32(cam.far)), cam.eye, cam.lookAt, W, H)
    return ctx


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    d = np.linalg.norm(a - b)
    return d / max(np.linalg.norm(b), 1e-30)


# ---------------------------------------------------------------- bit comparison
def _on_host(a):
    """a torch tensor is brought to the host; everything else goes through np.asarray.  No cast, no reshape."""
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def same_bits(a, b, nan_equal=False):
    """Equal shape, equal dtype, equal bytes.  Nothing is cast: float32 against float64 is False, (2, 3) against (6,) is False, -0.0 differs
    from +0.0, and a NaN equals a NaN only where sign and payload agree.  A caller that means less says so where it calls: np.float32(x),
    .astype, .reshape.  nan_equal=True is the one relaxation: any NaN equals any NaN (which NaN an invalid operation produces -- sign,
    payload -- is the one thing IEEE 754 leaves open, and x86 and gfx950 differ in it); every other element still bit for bit."""
    a, b = _on_host(a), _on_host(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.tobytes() == b.tobytes():
        return True
    if not (nan_equal and a.dtype.kind == "f"):
        return False
    word = "u%d" % a.dtype.itemsize
    same = np.ascontiguousarray(a).view(word) == np.ascontiguousarray(b).view(word)
    return bool(np.all(same | (np.isnan(a) & np.isnan(b))))


def bits(a):
    """the uint32 view of float32 data, shape kept: for arithmetic on the bit patterns.  Anything but float32 is refused, not cast."""
    a = _on_host(a)
    assert a.dtype == np.float32, a.dtype
    return np.ascontiguousarray(a).view(np.uint32).reshape(a.shape)


def halves(col):
    """(high, low) 32-bit halves of uint64 words, as int64"""
    return (col >> np.uint64(32)).astype(np.int64), (col & np.uint64(0xFFFFFFFF)).astype(np.int64)


# ---------------------------------------------------------------- the device side
def dev(a, dtype=np.float32):
    """a copy of `a` as `dtype` (None: its own) on the device; a copy, so that shared read-only arrays are accepted"""
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def host(ts):
    """the tensors after a synchronize, each as a [rows, everything else] host array of its own"""
    import torch
    torch.cuda.synchronize()
    return [t.detach().cpu().numpy().reshape(t.shape[0], int(np.prod(t.shape[1:]))).copy() for t in ts]


def on_torch_stream(ctx):
    """ctx works on torch's current stream; 0, the legacy default stream, is 1 here"""
    import torch
    ctx.set_stream(torch.cuda.current_stream().cuda_stream or 1)
    return ctx


def refused(call, text=None, code=None):
    """call() raises GsError with `code` (default GS_ERR_INVALID) and, where given, `text` in its message"""
    from gaussiansplat_amd import backend as B
    with pytest.raises(B.GsError) as e:
        call()
    assert e.value.code == (B.GS_ERR_INVALID if code is None else code), (e.value.code, code, str(e.value))
    assert text is None or text in str(e.value), str(e.value)


def one_wave_per_tile(monkeypatch):
    """The body of the autouse fixture of tests/test_gpu_caps.py and tests/test_gpu_slabs.py.  Frames with capped lists, and frames binned
    in depth slabs, are composited by one wave per tile (gs_config.tile_parts); the plain frames they are compared with BIT FOR BIT there
    must be too: on these small grids the default would give a tile two or four waves, each testing its entries against its own pixels
    (differences below 2^-27 per entry, tests/test_gpu_parts.py)."""
    monkeypatch.setenv("GSPLAT_TILE_PARTS", "1")


def run_frame(ctx, dC, deg, *, slot=None, overwrite=False, phases=("all",), kind="3d", g2d=False):
    """One frame at the ctx level: preprocess, bin, forward, backward (one call per phase), everything read back.  The state-changing calls
    in the one order every test uses; the getters in between only read.  g: the gradient handle, for calls that follow the frame."""
    from gaussiansplat_amd import backend as B
    if slot is not None:
        ctx.set_view_slot(slot)
    ctx.preprocess(); ctx.bin()
    rounds = ctx.num_rounds
    img, tr = ctx.forward_host()
    st = ctx.list_stats()
    g = ctx.grads_alloc()
    for phase in phases:
        ctx.backward(dC, g, overwrite=overwrite, phase=phase)
    grads = ctx.grads_read_2d(g) if kind == "2d" else ctx.grads_read(g, deg)
    out = dict(img=img, tr=tr, grads=grads, g=g, wc=ctx.work_counters_ex(), st=st, inst=ctx.num_instances, rounds=rounds,
               parts=ctx.tile_parts_of_frame())
    if g2d:
        out["g2d"] = ctx.get_array(B.ARR_GRAD2D)
    return out


# ---------------------------------------------------------------- the renderer level
def synthetic_renderer(n, deg, seed, W=128, H=96, scene=None, **kw):
    import torch
    from gaussiansplat_amd import renderer as R
    if n == 0:                                  # (getRenderer reshapes its arrays by their row count: an empty model is built by hand)
        z = lambda w: torch.empty((0, w), device="cuda")
        return R.GaussianRenderer3D(R.SplatData3D(means=z(3), scales=z(3), shs=z(3 * (deg + 1) ** 2), quaternions=z(4), opacities=z(1)), (W, H), deg, **kw)
    scene = scene if scene is not None else synthetic.make_scene(n, W, H, deg, seed=seed)
    return R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, scene, **kw)


def render(r, cam):
    from gaussiansplat_amd import renderer as R
    tps = R.preprocess(r, cam); R.compactIdxs(r); R.forward(r, tps)


def small_scene_renderer(n, seed):
    """(renderer, camera of view 0, W, H) of a 64 x 48 scene of degree 1: deterministic, one wave per tile, so that frames compare bit for bit"""
    W, H, deg = 64, 48, 1
    r = synthetic_renderer(n, deg, seed, W, H, deterministic=True, tile_parts=1)
    return r, synthetic.scene_camera(W), W, H


def perturbed_start(n, Wi, Hi, deg):
    """(start model, camera, target image) of the training tests (tests/test_gpu_loss.py::test_sgd_step_and_training_reduces_loss,
    tests/test_gpu_adam.py, tests/test_gpu_density.py): the target is the rendered scene, the start its SH and opacities perturbed."""
    from gaussiansplat_amd import renderer as R
    target = synthetic.make_scene(n, Wi, Hi, deg, seed=1)
    cam = synthetic.scene_camera(Wi)
    rt = R.getRenderer("GAUSSIAN_3D", (Wi, Hi, 3), (16, 16), None, target)
    render(rt, cam)
    gt = rt.imageData.clone()
    start = {k: v.copy() for k, v in target.items()}
    start["shs"] = (start["shs"] + 0.2 * np.random.default_rng(2).standard_normal(start["shs"].shape)).astype(np.float32)
    start["opacities"] = (start["opacities"] - 0.5).astype(np.float32)
    return start, cam, gt


# ---------------------------------------------------------------- host programs (tests/NAME_host.cpp)
_HOST_PROGRAMS = {}


def host_program(name, tmp_dir):
    """tests/NAME_host.cpp as a host program, built through tests/Makefile (the one statement of its flags) into tmp_dir; one compile per
    session, whoever asks.  Returns the executable; its folder is free for the caller's files."""
    if name not in _HOST_PROGRAMS:
        from gaussiansplat_amd import build as gbuild
        subprocess.run(["make", "-C", TESTS, f"{tmp_dir}/{name}_host", f"OUT={tmp_dir}", f"HIPCC={gbuild._hipcc()}"],
                       check=True, capture_output=True, text=True)
        _HOST_PROGRAMS[name] = os.path.join(str(tmp_dir), name + "_host")
    return _HOST_PROGRAMS[name]


def run_host(exe, args, header_bytes, arrays, outs, stdout=False):
    """The round trip of a host program: in.bin = header_bytes, then the arrays as they are; `exe args in.bin out.bin`; out.bin read as
    outs = [(dtype, count)], every byte of it consumed.  Returns the output arrays (and what the program printed, where stdout is asked)."""
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as fh:
        fh.write(header_bytes)
        for a in arrays:
            fh.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, *args, fin, fout], check=True, timeout=120, capture_output=stdout, text=True)
    with open(fout, "rb") as fh:
        raw = fh.read()
    res, at = [], 0
    for dt, cnt in outs:
        res.append(np.frombuffer(raw, dt, cnt, at).copy())
        at += cnt * np.dtype(dt).itemsize
    assert at == len(raw), (at, len(raw))
    return (res, r.stdout) if stdout else res
