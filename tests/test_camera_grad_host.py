"""The camera gradient without a GPU: the per-gaussian statement (csrc/gs_camera_grad.h) on the CPU against fp64 autograd, the chain from the
40 raw partials to Camera fields (camera.camera_param_grads), the pose optimiser (optim.CameraAdam), the argument refusals of
train.trainStep, and the teeth check of the end-to-end bar of tests/test_gpu_camera_grad.py.

The statement is a __host__ __device__ function with contraction off: tests/camera_grad_host.cpp is a host build of it, run as a child
process.  tests/camera_ref.py restates the forward with the camera differentiable, one copy of T, P, fx, fy, eye, lookAt per gaussian, so
autograd returns per-gaussian camera gradients of  sum_g (row_g converted by gs_g2d_to_grads in float64) . (rgb, sig, mux, muy, M)_g.

The bar, per component c: |host - autograd| <= 1e-9 x max_g |autograd[g, c]|.  Both sides are fp64 from the same fp32 inputs; the chain's
cancellation was measured as 1e3 .. 1e4 x epsilon (gs_preprocess_bwd.hip's header: 2e-4 .. 2e-3 in fp32), i.e. 1e-13 .. 1e-12 here --
the bar stands three orders above it.  `make -C tests sanitize-camera-grad` runs the same program under ASan + UBSan."""
import os

import numpy as np
import pytest

import camera_ref
from common import host_program, run_host, scene_and_cameras
from gaussiansplat_amd import build as gbuild
from gaussiansplat_amd import camera as gcam
from gaussiansplat_amd import optim, synthetic, train

N, W, H = 300, 64, 48
# (active degree, stored degree)
CASES = [(0, 0), (1, 1), (2, 2), (3, 3), (1, 3)]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return host_program("camera_grad", tmp_path_factory.mktemp("camera_grad_host"))


def camera_words(cam, T, P, W, H):
    f = np.concatenate([np.asarray(T, np.float32).reshape(-1), np.asarray(P, np.float32).reshape(-1),
                        np.array([cam.fx, cam.fy, cam.near, cam.far], np.float32), np.asarray(cam.eye, np.float32), np.asarray(cam.lookAt, np.float32)])
    return np.concatenate([f.view(np.uint32), np.array([W, H], np.int32).view(np.uint32)])


def _run_host(host_exe, sc, deg, cam, T, P, rows):
    n = sc["means"].shape[0]
    shs = np.asarray(sc["shs"], np.float32).reshape(n, -1)
    arrays = [camera_words(cam, T, P, W, H)] + [np.asarray(a, np.float32) for a in (sc["means"], sc["scales"], sc["quats"], sc["opacities"], shs, rows)]
    per, total = run_host(host_exe, [], np.array([n, deg, shs.shape[1]], np.uint32).tobytes(), arrays, [(np.float64, 40 * n), (np.float64, 40)])
    return per.reshape(n, 40), total


def make_rows(n, seed):
    """Raw rows [n, 10]: d rgb, S0, Sx, Sy, Sxx, Sxy, (unused), Syy; a third of them all zero."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, 10)).astype(np.float32)
    rows[:, 6:] *= 4.0
    rows[:, 8] = 0.0
    rows[rng.permutation(n)[: n // 3]] = 0.0
    return rows


@pytest.fixture(scope="module", params=CASES, ids=[f"active{a}_stored{s}" for a, s in CASES])
def case(request, host_exe):
    deg, stored = request.param
    sc, cam, T, P, _ = scene_and_cameras(N, W, H, stored, 300 + 10 * stored + deg)
    rows = make_rows(N, 17 + deg)
    # three planted gaussians behind the scene, each with a ZERO row: the mean at the eye (t = 0), a NaN mean, scale 200 (exp overflows)
    scp = {k: np.concatenate([v, v[:3]]) for k, v in sc.items()}
    scp["means"][N] = cam.eye; scp["means"][N + 1] = (np.nan, 0.0, 0.0); scp["scales"][N + 2] = 200.0
    rows_p = np.concatenate([rows, np.zeros((3, 10), np.float32)])
    per, total = _run_host(host_exe, scp, deg, cam, T, P, rows_p)
    want = camera_ref.rows_scalar_grads(sc, deg, T, P, float(np.float32(cam.fx)), float(np.float32(cam.fy)), cam.eye, cam.lookAt, W, H, rows)
    return dict(deg=deg, per=per, total=total, want=want, rows=rows)


def test_statement_equals_fp64_autograd(case):
    per, want = case["per"][:N], case["want"]
    scale = np.abs(want).max(axis=0)
    assert np.isfinite(want).all() and np.count_nonzero(scale[:32]) >= 21           # the reference is real work: d_T rows 0..2, d_P rows 0, 1, 3 by t[0:3] (t[3] == 0)
    if case["deg"] >= 1:
        assert (scale[32:38] > 0).all()                                             # the colour path reaches eye and lookAt
    err = np.abs(per - want).max(axis=0)
    print("max |host - autograd| / max |autograd| per component:", np.array2string(err / np.maximum(scale, 1e-300), precision=2))
    assert (err <= 1e-9 * scale).all(), (err / np.maximum(scale, 1e-300)).max()
    assert scale[38] > 0 and scale[39] > 0


def test_zero_rows_contribute_exact_plus_zero(case):
    zero = ~case["rows"].any(axis=1)
    assert zero.sum() == N // 3
    z = np.concatenate([case["per"][:N][zero], case["per"][N:]])                    # ... and the three planted ones
    assert z.shape == (N // 3 + 3, 40)
    assert not z.view(np.uint64).any()                                              # + 0: not - 0, not NaN
    assert (np.abs(case["per"][:N][~zero]).sum(axis=1) > 0).all()


def test_sum_is_finite_and_in_index_order(case):
    s = np.zeros(40)
    for row in case["per"]:
        s = s + row
    assert np.isfinite(case["total"]).all() and np.array_equal(s, case["total"])


# ---------------------------------------------------------------- the chain to Camera fields

def _cameras():
    return [("default", gcam.default_camera(), 1920, 1080), ("view0", synthetic.scene_camera(64, 0), 64, 48), ("view1", synthetic.scene_camera(128, 1), 128, 96)]


@pytest.mark.parametrize("name,cam,w,h", _cameras(), ids=[c[0] for c in _cameras()])
def test_camera_param_grads_equals_autograd(name, cam, w, h):
    raw = np.random.default_rng(5).standard_normal(40)
    got = gcam.camera_param_grads(cam, w, h, raw)
    want = camera_ref.param_grads_autograd(cam, w, h, raw)
    assert set(got) == {"eye", "lookAt", "up", "fx", "fy"}
    for k in got:
        g, r = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert g.dtype == np.float64 and np.abs(g - r).max() <= 1e-10 * np.abs(r).max(), (k, g, r)
    # the record form gives the same numbers
    from gaussiansplat_amd.renderer import CameraGrads
    rec = gcam.camera_param_grads(cam, w, h, CameraGrads.from_flat(raw.astype(np.float32)))
    again = gcam.camera_param_grads(cam, w, h, raw.astype(np.float32))
    assert all(np.array_equal(rec[k], again[k]) for k in rec)


@pytest.mark.parametrize("name,cam,w,h", _cameras(), ids=[c[0] for c in _cameras()])
def test_the_restatements_are_the_camera_functions(name, cam, w, h):
    """camera_ref.transform / projection, whose autograd the chain is checked against, equal camera.compute_transform / compute_projection
    up to the fp32 roundings those carry: a convention shared by the restatement and the analytic adjoint alone would show here."""
    import torch
    eye, look, up = (torch.tensor(np.asarray(a, np.float32).astype(np.float64)) for a in (cam.eye, cam.lookAt, cam.up))
    T = camera_ref.transform(eye, look, up).numpy()
    P = camera_ref.projection(torch.tensor(float(cam.fx)), torch.tensor(float(cam.fy)), float(np.float32(cam.near)), float(np.float32(cam.far)), w, h).numpy()
    T32 = gcam.compute_transform(cam).astype(np.float64).reshape(4, 4, order="F")
    P32 = gcam.compute_projection(cam, w, h).astype(np.float64).reshape(4, 4, order="F")
    assert np.abs(T - T32).max() <= 1e-6 * max(1.0, np.abs(T32).max()) and np.abs(T32[:3, :3]).max() > 0.9 and not T32[3].any()
    assert np.abs(P - P32).max() <= 1e-6 * np.abs(P32).max() and P32[0, 0] > 0 and P32[3, 2] == 1.0


def test_shared_device_text_is_written_once():
    """The geometry chain, the SH direction derivative, the SH coefficient literals and the halo staging each stand in ONE file under csrc/,
    and every user includes that file: a second copy, typed out or pasted back, fails here."""
    import re
    text = {f: open(os.path.join(gbuild.CSRC, f)).read() for f in sorted(os.listdir(gbuild.CSRC)) if f.endswith((".h", ".inc", ".hip"))}

    # the coefficient lists: 5 and 7 float literals, once, in gs_sh.h; the device arrays and the camera statement's doubles are made of the two macros
    sh = text["gs_sh.h"]
    for name, n in (("GS_SH_C2_VALUES", 5), ("GS_SH_C3_VALUES", 7)):
        m = re.search(r"#define %s ((?:.*\\\n)*.*)\n" % name, sh)
        assert m, name
        lits = re.findall(r"-?\d+\.\d+f", m.group(1))
        assert len(lits) == n, (name, lits)
        for digits in {x.lstrip("-").rstrip("f") for x in lits}:
            where = {f: t.count(digits) for f, t in text.items() if digits in t}
            assert where == {"gs_sh.h": sum(x.lstrip("-").rstrip("f") == digits for x in lits)}, (name, digits, where)
    assert re.search(r"bC2\[5\] = \{GS_SH_C2_VALUES\}", sh) and re.search(r"bC3\[7\] = \{GS_SH_C3_VALUES\}", sh)
    assert re.search(r"constexpr double bC2\[5\] = \{GS_SH_C2_VALUES\}, bC3\[7\] = \{GS_SH_C3_VALUES\}", text["gs_camera_grad.h"])

    # one marker statement of each shared text: in exactly one file, once (whitespace and the coefficient's name aside)
    markers = {
        "gs_geom_chain_cov.inc": r"idet\s*=\s*1\.0\s*/\s*\(\s*cov\[0\]\[0\]\s*\*\s*cov\[1\]\[1\]",   # the 2 x 2 inverse
        "gs_sh_ddir.inc": r"\(\s*4\s*\*\s*zz\s*-\s*3\s*\*\s*xx\s*-\s*yy\s*\)\s*\*\s*cs\[13\]",   # a degree-3 ddir term
        "gs_halo_tile.h": r"min\(max\(gy, 0\), H - 1\)\s*\*\s*W\s*\+\s*min\(max\(gx, 0\), W - 1\)",   # the clamped halo load
    }
    for home, pat in markers.items():
        where = {f: len(re.findall(pat, t)) for f, t in text.items() if re.search(pat, t)}
        assert where == {home: 1}, (home, where)

    # every user names the file it takes the text from
    includers = {
        "gs_geom_chain_cov.inc": ("gs_geom_bwd_body.inc", "gs_camera_grad.h"),
        "gs_geom_chain_tail.inc": ("gs_geom_bwd_body.inc", "gs_camera_grad.h"),
        "gs_sh_ddir.inc": ("gs_preprocess_bwd.hip", "gs_camera_grad.h"),
        "gs_halo_tile.h": ("gs_loss.hip", "gs_metrics.hip"),
        "gs_geom_bwd_body.inc": ("gs_preprocess_bwd.hip",),
    }
    for frag, users in includers.items():
        have = sorted(f for f, t in text.items() if '#include "%s"' % frag in t)
        assert have == sorted(users), (frag, have)
    assert text["gs_preprocess_bwd.hip"].count('#include "gs_geom_bwd_body.inc"') == 2      # fused in gs_sh_bwd_kernel, alone in gs_geom_bwd_kernel


def test_camera_param_grads_sign_and_scale_by_finite_difference():
    cam, w, h = synthetic.scene_camera(64, 1), 64, 48
    raw = np.random.default_rng(6).standard_normal(40)

    def value(e0):
        import torch
        eye = torch.tensor(np.asarray(cam.eye, np.float32).astype(np.float64)); eye[0] = e0
        look, up = (torch.tensor(np.asarray(a, np.float32).astype(np.float64)) for a in (cam.lookAt, cam.up))
        T = camera_ref.transform(eye, look, up).numpy()
        return float((T * raw[0:16].reshape(4, 4, order="F")).sum() + eye.numpy() @ raw[32:35])
    e0, hstep = float(np.float32(cam.eye[0])), 1e-5
    fd = (value(e0 + hstep) - value(e0 - hstep)) / (2 * hstep)
    an = gcam.camera_param_grads(cam, w, h, raw)["eye"][0]
    assert abs(fd - an) <= 1e-5 * abs(fd), (fd, an)


# ---------------------------------------------------------------- CameraAdam, trainStep's refusals

def test_camera_adam_equals_numpy_adam():
    cam = synthetic.scene_camera(64, 1)
    lr_e, lr_l, lr_f, b1, b2, eps = 3e-2, 1e-2, 0.5, 0.8, 0.95, 1e-9
    opt = optim.CameraAdam(cam, lr_e, lr_l, lr_f, betas=(b1, b2), eps=eps)
    x = np.concatenate([np.asarray(cam.eye, np.float64), np.asarray(cam.lookAt, np.float64), [cam.fx, cam.fy]])
    lr = np.array([lr_e] * 3 + [lr_l] * 3 + [lr_f] * 2)
    m, v = np.zeros(8), np.zeros(8)
    rng = np.random.default_rng(3)
    for t in range(1, 8):
        g = rng.standard_normal(8)
        opt.step(dict(eye=g[0:3], lookAt=g[3:6], up=np.ones(3), fx=g[6], fy=g[7]))
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * (g * g)
        x = x - lr * ((m / (1.0 - b1 ** t)) / (np.sqrt(v / (1.0 - b2 ** t)) + eps))
        assert np.array_equal(opt.x, x) and opt.step_count == t
        c = opt.camera
        assert c is opt.camera and c.eye.dtype == np.float32 and c.lookAt.dtype == np.float32
        assert np.array_equal(c.eye, x[0:3].astype(np.float32)) and np.array_equal(c.lookAt, x[3:6].astype(np.float32))
        assert c.fx == float(np.float32(x[6])) and c.fy == float(np.float32(x[7]))
        assert np.array_equal(c.up, cam.up) and c.near == cam.near and c.far == cam.far and c.id == cam.id
    fixed = optim.CameraAdam(cam, 1e-2, 1e-2)                                       # lr_focal = 0: fx, fy stay
    fixed.step(dict(eye=np.ones(3), lookAt=np.ones(3), fx=5.0, fy=-5.0))
    assert fixed.camera.fx == cam.fx and fixed.camera.fy == cam.fy and not np.array_equal(fixed.camera.eye, cam.eye)
    with pytest.raises(ValueError):
        optim.CameraAdam(cam, -1.0, 1e-2)
    with pytest.raises(ValueError):
        optim.CameraAdam(cam, 1e-2, 1e-2, betas=(1.0, 0.9))
    with pytest.raises(ValueError):
        fixed.step(dict(eye=np.array([np.nan, 0, 0]), lookAt=np.ones(3), fx=0.0, fy=0.0))


class _Untouchable:
    """A renderer that never reaches the device: any use is an error."""
    def __getattr__(self, name):
        raise AssertionError(f"trainStep touched the renderer ({name}) before refusing")


def test_train_step_refuses_before_touching_the_renderer():
    cam = synthetic.scene_camera(64, 0)
    pose = optim.CameraAdam(cam, 1e-2, 1e-2)
    fused = type("FusedAdam", (), {"fused": True})()
    r, gt = _Untouchable(), np.zeros((3, 4, 4), np.float32)
    with pytest.raises(ValueError, match="pose refinement needs the unfused backward"):
        train.trainStep(r, gt, 0.1, None, pose=pose, fused_sgd=True)
    with pytest.raises(ValueError, match="pose refinement needs the unfused backward"):
        train.trainStep(r, gt, 0.1, None, pose=pose, optimizer=fused)
    with pytest.raises(ValueError, match="camera and pose exclude each other"):
        train.trainStep(r, gt, 0.1, None, camera=cam, pose=pose)
    with pytest.raises(ValueError, match="freeze_model needs the unfused backward"):
        train.trainStep(r, gt, 0.1, None, freeze_model=True, fused_sgd=True)
    assert pose.step_count == 0


# ---------------------------------------------------------------- the teeth of the end-to-end bar (test_gpu_camera_grad.py, test 2)

def test_end_to_end_bar_has_teeth(oracle):
    """That bar is 1e-3 x || sum_g |c_g| ||: it only binds if the sum does not cancel to nothing against its absolute mass.  On the
    reference alone (the oracle's renders stand in for the device's): || sum_g c_g || / || sum_g |c_g| || >= 0.05 for d_T."""
    s = camera_ref.e2e_setup(oracle)
    dC = camera_ref.mse_dC(s["ref"]["image"], s["target_oracle"])
    c = camera_ref.e2e_contributions(s, dC)[:, :16]
    ratio = np.linalg.norm(c.sum(axis=0)) / np.linalg.norm(np.abs(c).sum(axis=0))
    print("|| sum c_g || / || sum |c_g| || for d_T:", ratio)
    assert ratio >= 0.05, ratio
