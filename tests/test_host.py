"""Host-side mirror of the reference interface: camera, synthetic scenes, loaders (CPU only)."""
import json

import numpy as np

from gaussiansplat_amd import camera as gcam
from gaussiansplat_amd import synthetic


def test_default_camera_matches_reference_literals():
    c = gcam.default_camera()                          # camera.jl:24-47
    assert list(c.eye) == [1.0, 3.0, 30.0] and list(c.lookAt) == [0, 0, 0] and list(c.up) == [0, 1, 0]
    assert (c.fx, c.fy, c.near, c.far) == (3200.0, 3200.0, 0.1, 100.0)


def test_get_camera_from_cameras_json(tmp_path):
    rot = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    entry = dict(id=3, img_name="im0", width=640, height=480, position=[1.0, 2.0, 3.0], rotation=rot, fx=500.0, fy=510.0)
    p = tmp_path / "cameras.json"
    p.write_text(json.dumps([entry]))
    c = gcam.get_camera(str(p), 1)                     # 1-based like the reference (camera.jl:119)
    assert np.allclose(c.eye, [-1, -2, -3]) and np.allclose(c.lookAt, [0, 0, -1])   # camera.jl:130-131
    assert (c.fx, c.fy, c.near, c.far, c.id, c.data) == (500.0, 510.0, 0.010, 100.0, 3, "im0")


def test_synthetic_scene_is_deterministic_and_shaped():
    a = synthetic.make_scene(1000, 256, 256, 3, seed=1234)
    b = synthetic.make_scene(1000, 256, 256, 3, seed=1234)
    for k in a:
        assert np.array_equal(a[k], b[k]) and a[k].dtype == np.float32
    assert a["shs"].shape == (1000, 16, 3) and a["quats"].shape == (1000, 4)
    assert np.allclose(np.linalg.norm(a["quats"], axis=1), 1, atol=1e-6)
    assert (a["scales"] >= -4.5).all() and (a["scales"] <= -2.5).all()
    assert (a["opacities"] >= -2).all() and (a["opacities"] <= 4).all()
    c0 = synthetic.scene_camera(1920, 0); c2 = synthetic.scene_camera(1920, 2)
    assert c0.fx == 3200.0 and np.allclose(c0.eye, [1, 3, 30])
    assert np.isclose(np.linalg.norm(c2.eye), np.linalg.norm(c0.eye), rtol=1e-6) and np.isclose(c2.eye[1], 3.0)


def test_ply_round_trip_reference_field_mapping(tmp_path):
    from gaussiansplat_amd import ply
    sc = synthetic.make_scene(257, 128, 128, 3, seed=5)
    p = str(tmp_path / "scene.ply")
    ply.save_ply(p, sc)
    d1 = ply.load_ply(p)                                  # reference mapping: f_dc + f_rest[0:9] -> 12 floats
    assert d1["shs"].shape == (257, 4, 3)
    assert np.array_equal(d1["shs"].reshape(257, -1), sc["shs"].reshape(257, -1)[:, :12])
    d3 = ply.load_ply(p, sh_degree=3)
    for k in ("means", "scales", "quats", "opacities", "shs"):
        assert np.array_equal(d3[k], sc[k]), k


def test_export_image_like_reference_viewer(tmp_path):
    from gaussiansplat_amd import export
    img = np.zeros((3, 2, 4), np.float32)            # C=3, H=2, W=4
    img[0, 0, 3] = 2.0                               # clamps to 1
    img[1, 1, 0] = np.nan                            # scrubbed to 0
    img[2, 1, 2] = 0.5
    out = export.to_rgb8(img, rotate=False)
    assert out.shape == (4, 2, 3) and out.dtype == np.uint8        # Julia: W rows, H columns
    assert out[3, 0, 0] == 255 and out[0, 1, 1] == 0 and out[2, 1, 2] == 128
    rot = export.to_rgb8(img)
    assert rot.shape == (2, 4, 3) and np.array_equal(rot, np.rot90(out, 1, (0, 1)))
    p = tmp_path / "a.ppm"
    export.save_ppm(str(p), rot)
    assert p.read_bytes().startswith(b"P6\n4 2\n255\n") and len(p.read_bytes()) == 11 + 24


def test_bench_self_launch_command():
    """`python bench.py --gpus N` from a bare shell starts N ranks as CHILD processes of torch.distributed.run, before
    anything imports torch or touches HIP (GS_BENCH_DRY_LAUNCH shows the command instead of running it)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["GS_BENCH_DRY_LAUNCH"] = "1"
    code = ("import sys, runpy; sys.argv = ['bench.py', '--gpus', '4', '--steps', '7', '--backend', 'gloo'];"
            "runpy.run_path(%r, run_name='__main__'); assert 'torch' not in sys.modules, 'torch imported before the launch'"
            % os.path.join(root, "bench.py"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    cmd = json.loads(r.stdout.strip().splitlines()[-1])["launch"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-6:] == ["--gpus", "4", "--steps", "7", "--backend", "gloo"] and cmd[-7].endswith("bench.py")


def test_bench_dump_outputs_writes_a_fixed_sample_in_float32(tmp_path):
    """bench.py --dump-outputs: above DUMP_GAUSSIANS gaussians / DUMP_PIXELS pixels a seeded sample of rows / pixels, the same
    for the same seed, float32, and under 64 MB in all at the largest stated size (5 M gaussians at 3840x2160, SH3)."""
    import os
    import sys
    from types import SimpleNamespace
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    n, H, W, K = bench.DUMP_GAUSSIANS + 1000, 1500, 1500, 48
    flat = torch.randn(n * (11 + K), generator=torch.Generator().manual_seed(5))
    views, o = {}, 0
    for name, k in (("Δmeans", 3), ("Δscales", 3), ("Δquaternions", 4), ("Δopacities", 1), ("Δshs", K)):
        views[name] = flat[o:o + k * n].view(n, k)
        o += k * n
    ctx = object()
    r = SimpleNamespace(splatGrads=SimpleNamespace(flat=flat, **views), imageData=torch.rand(3, H, W), transmittance=torch.rand(H, W),
                        ctx=ctx, _bench_hv=SimpleNamespace(last_ctx=ctx))
    bench.dump_outputs(str(tmp_path / "a"), r, 7)
    bench.dump_outputs(str(tmp_path / "b"), r, 7)
    names = ["d_means", "d_scales", "d_quaternions", "d_opacities", "d_shs", "image", "transmittance"]
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f + ".npy" for f in names)
    rng = np.random.default_rng(7)
    rows = np.sort(rng.choice(n, bench.DUMP_GAUSSIANS, replace=False))
    pix = np.sort(rng.choice(H * W, bench.DUMP_PIXELS, replace=False))
    for f in names:
        a, b = np.load(tmp_path / "a" / (f + ".npy")), np.load(tmp_path / "b" / (f + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, b), f
    assert np.array_equal(np.load(tmp_path / "a" / "d_shs.npy"), views["Δshs"].numpy()[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "image.npy"), r.imageData.reshape(3, -1).numpy()[:, pix])
    assert np.array_equal(np.load(tmp_path / "a" / "transmittance.npy"), r.transmittance.reshape(-1).numpy()[pix])
    assert (59 * 4 * bench.DUMP_GAUSSIANS + 16 * bench.DUMP_PIXELS) < 64 * 2 ** 20

def test_view_record_is_kept_with_the_camera_and_follows_its_fields():
    """renderer._set_view (the host side of preprocess(renderer, camera), forward.jl:35-53): a small frame is bound by its caller, so the
    view's matrices (computeTransform / computeProjection, camera.jl:53-111) are built once per camera and again whenever one of its
    fields -- or the image size -- changes, in place or by assignment."""
    from gaussiansplat_amd import renderer as R

    class Ctx:                                          # what _set_view needs of backend.Context
        def __init__(self): self.built, self.set, self.slots = [], [], []
        def camera_record(self, T, P, fx, fy, near, far, eye, lookAt, W, H):
            rec = (np.array(T, np.float32), np.array(P, np.float32), fx, fy, near, far, np.array(eye, np.float32), np.array(lookAt, np.float32), W, H)
            self.built.append(rec); return rec
        def set_camera_record(self, rec): self.set.append(rec)
        def set_view_slot(self, s): self.slots.append(s)

    class Fake:                                         # the two fields of GaussianRenderer3D it touches
        def __init__(self, W, H): self.ctx, self.camera, self.transmittance = Ctx(), None, np.ones((H, W), np.float32)
    f = Fake(64, 48)
    a, b = synthetic.scene_camera(64, view=0), synthetic.scene_camera(64, view=4)
    a.id, b.id = 0, 4
    for cam in (a, b, a, b, a):
        R.GaussianRenderer3D._set_view(f, cam)
    assert len(f.ctx.built) == 2 and len(f.ctx.set) == 5 and f.ctx.slots == [0, 4, 0, 4, 0]
    assert f.ctx.set[0] is f.ctx.set[2] and f.ctx.set[1] is f.ctx.set[3]
    assert np.array_equal(f.ctx.built[0][0], gcam.compute_transform(a)) and np.array_equal(f.ctx.built[1][1], gcam.compute_projection(b, 64, 48))
    a.eye[0] += np.float32(0.5)                          # in place
    R.GaussianRenderer3D._set_view(f, a)
    assert len(f.ctx.built) == 3 and np.array_equal(f.ctx.built[2][0], gcam.compute_transform(a))
    b.fx = b.fx * 1.25                                  # by assignment
    R.GaussianRenderer3D._set_view(f, b)
    assert len(f.ctx.built) == 4 and np.array_equal(f.ctx.built[3][1], gcam.compute_projection(b, 64, 48))
    g = Fake(80, 48)                                    # another image size: the same camera object is rebuilt for it
    R.GaussianRenderer3D._set_view(g, a)
    assert len(g.ctx.built) == 1 and g.ctx.built[0][8:] == (80, 48)
    R.GaussianRenderer3D._set_view(f, a)
    assert len(f.ctx.built) == 5                        # (one record per camera: the other size pushed it out)


# ---------------------------------------------------------------- the mirror's one coercion function

def test_as_device_tensor_coerces_checks_and_passes_through():
    """renderer.as_device_tensor: float64 NumPy comes out float32 and contiguous, a strided tensor comes out contiguous, a tensor that
    already matches is returned as the same object (no copy), and a wrong shape is a ValueError that carries the given name."""
    import pytest
    import torch
    from gaussiansplat_amd import renderer as R
    cpu = torch.device("cpu")
    a = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    t = R.as_device_tensor(a[:, ::-1], cpu, (2, 3, 4), "a")
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous() and np.array_equal(t.numpy(), a[:, ::-1].astype(np.float32))
    s = torch.arange(12, dtype=torch.float32).reshape(3, 4).t()
    assert not s.is_contiguous()
    c = R.as_device_tensor(s, cpu, (4, 3), "s")
    assert c.is_contiguous() and torch.equal(c, s)
    m = torch.zeros((3, 4, 5), dtype=torch.float32)
    assert R.as_device_tensor(m, cpu, (3, 4, 5), "m") is m and R.as_device_tensor(m, cpu, None, "m") is m
    with pytest.raises(ValueError, match="the_name"):
        R.as_device_tensor(m, cpu, (3, 5, 4), "the_name")
    with pytest.raises(ValueError, match="the_name"):
        R.as_device_tensor(a, cpu, (4, 3, 2), "the_name")


# ---------------------------------------------------------------- the order of a training step's library calls, pinned literally

def _recording_renderer():
    """A GaussianRenderer3D built by hand (no getRenderer, no library): 4 x 4 CPU images, five gaussians, a context that records the name
    of every method called on it; the stream bind and the view are logged as <bind> and <view>."""
    import torch
    from gaussiansplat_amd import renderer as R
    log = []

    class Ctx:
        def __getattr__(self, name):
            def call(*a, **k):
                log.append(name)
                return np.zeros(R.B.GS_CAMERA_GRAD_FLOATS, np.float32) if name == "backward_camera" else None
            return call

    class Rec(R.GaussianRenderer3D):
        def __init__(self):
            z = lambda *s: torch.zeros(s, dtype=torch.float32)
            self.splatData = R.SplatData3D(means=z(5, 3), scales=z(5, 3), shs=z(5, 12), quaternions=z(5, 4), opacities=z(5, 1))
            self.nGaussians, self.sh_degree, self.camera, self.ctx = 5, 1, None, Ctx()
            self.imageData, self.transmittance = z(3, 4, 4), torch.ones((4, 4), dtype=torch.float32)
            self._splatGrads = R.initGrads(self.splatData)
            self._grads_lazy_zero = False
            self._grads = R.grads_struct(self._splatGrads.flat, R.layout_of(self._splatGrads)[0])

        def _begin(self):
            log.append("<bind>")
            return self.ctx

        def _set_view(self, camera):
            log.append("<view>")
            self.camera = camera

    return Rec(), log


def test_train_step_library_call_order():
    """trainStep in six forms against a recording context: every list is literal; a <bind> stands before every library call."""
    from gaussiansplat_amd import optim, train as TR
    gt = np.zeros((3, 4, 4), np.float32)
    frame = ["<view>", "<bind>", "preprocess", "<bind>", "bin", "<bind>", "bind_outputs", "forward_device", "<bind>", "loss_device"]
    frame2 = [x for x in frame if x != "bind_outputs"]              # the second step of a renderer: its outputs are bound already

    def run(**kw):
        r, log = _recording_renderer()
        loss = TR.getLossFunction((4, 4), 11, 3, renderer=r)
        stubs = {}
        if "optimizer" in kw:
            fused = kw["optimizer"]
            stubs["optimizer"] = type("Opt", (), dict(fused=fused, renderer=r, step=lambda self: log.append("opt.step"),
                                                      backward_step=lambda self, dC: log.append("opt.backward_step")))()
        if kw.get("density"):
            stubs["density"] = type("Den", (), dict(accumulate=lambda self, rr: log.append("density.accumulate"),
                                                    after_step=lambda self, rr, opt: log.append("density.after_step")))()
        if kw.get("pose"):
            stubs["pose"] = type("Pose", (), dict(camera=synthetic.scene_camera(64, 0), step=lambda self, g: log.append("pose.step")))()
        rest = {k: v for k, v in kw.items() if k not in ("optimizer", "density", "pose")}
        TR.trainStep(r, gt, 0.1, loss, want_loss=False, **stubs, **rest)
        first = list(log)
        del log[:]
        TR.trainStep(r, gt, 0.1, loss, want_loss=False, **stubs, **rest)
        assert log == [x for x in first if x != "bind_outputs"]
        return first

    assert run() == frame + ["<bind>", "backward", "<bind>", "sgd_step"]
    assert run(fused_sgd=True) == frame + ["<bind>", "backward_sgd"]
    assert run(optimizer=False) == frame + ["<bind>", "backward", "opt.step"]
    assert run(optimizer=False, density=True) == frame + ["<bind>", "backward", "density.accumulate", "opt.step", "density.after_step"]
    assert run(density=True) == frame + ["<bind>", "backward", "density.accumulate", "<bind>", "sgd_step", "density.after_step"]
    assert run(optimizer=True) == frame + ["opt.backward_step"]
    assert run(freeze_model=True) == frame + ["<bind>", "backward"]
    assert run(optimizer=False, freeze_model=True) == frame + ["<bind>", "backward"]
    assert run(pose=True) == frame + ["<bind>", "backward", "<bind>", "backward_camera", "pose.step", "<bind>", "sgd_step"]
    assert run(optimizer=False, pose=True, density=True) == frame + ["<bind>", "backward", "<bind>", "backward_camera", "pose.step",
                                                                      "density.accumulate", "opt.step", "density.after_step"]
    assert frame2 == ["<view>", "<bind>", "preprocess", "<bind>", "bin", "<bind>", "forward_device", "<bind>", "loss_device"]
