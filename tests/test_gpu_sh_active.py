"""The active SH degree (gs_set_active_sh_degree): a degree-D model at active degree d against its TRUNCATED TWIN -- the same scene
with shs[:, :Ka, :] and sh_degree = d in a second ctx, the path every other test of the suite pins.  All comparisons are bit for bit
(deterministic mode, one wave per tile); the one tolerance is the oracle's pixel bar of tests/test_gpu_parity.py.

Shapes: N = 1281 gaussians (n % 4 == 1, not a multiple of 256: a flat gradient buffer's d_shs slice at 44 n bytes is not 16-byte
aligned), 128 x 96 pixels (48 tiles); one case at N = 300, 64 x 48 with separate, 16-byte-aligned arrays."""
import numpy as np
import pytest

from common import bits, same_bits

pytestmark = pytest.mark.gpu

W, H, N = 128, 96, 1281
PAIRS = [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]                 # (stored, active), active < stored
BWD_PAIRS = [(3, 0), (3, 1), (3, 2), (2, 1), (1, 0)]
PIX_ATOL, PIX_RTOL = 1e-4, 1e-4                                            # tests/test_gpu_parity.py
LR6 = (1e-3, 4e-3, 2e-3, 5e-2, 2.5e-3, 1.25e-4)
B1, B2, EPS = 0.9, 0.999, 1e-8
NO_TAIL_FILL = 32


def _k3(deg):
    return 3 * (deg + 1) ** 2


def _scene(n, w, h, deg, seed):
    from gaussiansplat_amd import synthetic
    return synthetic.make_scene(n, w, h, deg, seed=seed)


def _twin_scene(sc, active):
    tw = dict(sc)
    tw["shs"] = np.ascontiguousarray(sc["shs"][:, :(active + 1) ** 2, :])
    return tw


class _Rig:
    """One ctx over a device copy of a scene, on torch's stream; frames of the synthetic cameras."""

    def __init__(self, sc, deg, active=None, w=W, h=H, **kw):
        import torch
        from gaussiansplat_amd import backend as B
        self.n, self.deg, self.w, self.h = sc["means"].shape[0], deg, w, h
        kw.setdefault("deterministic", True)
        kw.setdefault("tile_parts", 1)
        self.ctx = B.Context(**kw)
        self.ctx.set_stream(1)                                             # the legacy default stream: in order with torch's copies
        self.p = [torch.as_tensor(np.ascontiguousarray(sc[k], np.float32).reshape(self.n, -1)).cuda().contiguous()
                  for k in ("means", "scales", "quats", "opacities", "shs")]
        assert self.p[4].shape[1] == _k3(deg)
        self.ctx.set_model_device(self.n, deg, [t.data_ptr() for t in self.p])
        if active is not None:
            self.ctx.set_active_sh_degree(active)

    def view(self, v=0):
        from gaussiansplat_amd import camera as gcam, synthetic
        cam = synthetic.scene_camera(self.w, view=v)
        f = lambda x: float(np.float32(x))
        self.ctx.set_camera(gcam.compute_transform(cam), gcam.compute_projection(cam, self.w, self.h), f(cam.fx), f(cam.fy), f(cam.near),
                            f(cam.far), cam.eye, cam.lookAt, self.w, self.h)

    def frame(self, v=0):
        self.view(v)
        self.ctx.preprocess(); self.ctx.bin()
        self.ctx.forward_device(0, 0)

    def close(self):
        self.ctx.close()


def _dC(v, w=W, h=H):
    import torch
    from gaussiansplat_amd import synthetic
    return torch.as_tensor(synthetic.make_dC(w, h, 900 + v)).cuda()


class _Grads:
    """Five device arrays of the model's widths: views into ONE flat buffer of the initGrads layout, or five separate tensors."""

    def __init__(self, n, deg, layout, fill):
        import torch
        widths = [3, 3, 4, 1, _k3(deg)]
        if layout == "flat":
            self.flat = torch.empty(sum(widths) * n, device="cuda")
            self.t, o = [], 0
            for w in widths:
                self.t.append(self.flat[o:o + w * n].view(n, w)); o += w * n
        else:
            self.t = [torch.empty((n, w), device="cuda") for w in widths]
        for t in self.t:
            if isinstance(fill, float):
                t.fill_(fill)
            else:
                t.copy_(torch.as_tensor(fill(tuple(t.shape))))

    def struct(self):
        from gaussiansplat_amd import backend as B
        return B.GsGrads(*[t.data_ptr() for t in self.t])

    def host(self):
        import torch
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in self.t]


def _backward(rig, g, dC, overwrite, phases="all"):
    if phases == "all":
        rig.ctx.backward(dC.data_ptr(), g.struct(), overwrite=overwrite)
    else:
        for ph in ("composite", "params_sh", "params_geom"):
            rig.ctx.backward(dC.data_ptr(), g.struct(), overwrite=overwrite, phase=ph)


# ---------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("stored,active", PAIRS)
def test_forward_equals_the_truncated_twin_and_meets_the_oracle_bar(oracle, stored, active):
    from common import scene_and_cameras
    from gaussiansplat_amd import backend as B
    sc, cam, T, P, ocam = scene_and_cameras(N, W, H, stored, 100 + 10 * stored + active)
    tw = _twin_scene(sc, active)
    out = []
    for scene, deg, act in ((sc, stored, active), (tw, active, None)):
        rig = _Rig(scene, deg, act, order=1, t_min=0.0)
        assert rig.ctx.active_sh_degree == active
        rig.view(0); rig.ctx.preprocess(); rig.ctx.bin()
        img, tr = rig.ctx.forward_host()
        out.append((img, tr, rig.ctx.get_array(B.ARR_RGB), rig.ctx.get_array(B.ARR_TILE_RANGES), rig.ctx.get_array(B.ARR_SORTED_IDS)))
        rig.close()
    for name, a, b in zip(("image", "transmittance", "rgb", "tile ranges", "sorted ids"), *out):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    ref = oracle.render(tw["means"], tw["scales"], tw["quats"], tw["opacities"], tw["shs"], active, ocam, order=1, t_min=0.0)
    img, tr = out[0][0], out[0][1]
    assert np.all(np.abs(img - ref["image"]) <= PIX_ATOL + PIX_RTOL * np.abs(ref["image"])), np.abs(img - ref["image"]).max()
    assert np.all(np.abs(tr - ref["trans"]) <= PIX_ATOL + PIX_RTOL * np.abs(ref["trans"]))
    # and the active degree is not the stored one's picture (the test would pass on a setter that does nothing otherwise)
    full = _Rig(sc, stored, order=1, t_min=0.0)
    full.view(0); full.ctx.preprocess(); full.ctx.bin()
    assert not np.array_equal(full.ctx.forward_host()[0], img)
    full.close()


# ---------------------------------------------------------------- 2. default and identity
def test_default_minus_one_and_own_degree_are_the_same_renderer():
    stored = 2
    sc = _scene(N, W, H, stored, 120)
    dC = _dC(0)
    res = []
    for request in (None, -1, stored, 3):                                  # 3 on a degree-2 model: effectively 2
        rig = _Rig(sc, stored, request)
        assert rig.ctx.active_sh_degree == stored
        rig.view(0); rig.ctx.preprocess(); rig.ctx.bin()
        img, tr = rig.ctx.forward_host()
        g = _Grads(N, stored, "flat", float("nan"))
        _backward(rig, g, dC, overwrite=True)
        res.append([img, tr] + g.host())
        rig.close()
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert same_bits(a, b)
    assert np.isfinite(res[0][6]).all() and np.any(res[0][6][:, 12:] != 0)   # the band-2 gradients are there


# ---------------------------------------------------------------- 3. backward, overwrite
def _overwrite_case(stored, active, n, w, h, fill_flag, layouts):
    from gaussiansplat_amd import backend as B
    sc = _scene(n, w, h, stored, 130 + 10 * stored + active)
    dC = _dC(1, w, h)
    tw = _Rig(_twin_scene(sc, active), active, w=w, h=h)
    tw.frame(0)
    gt = _Grads(n, active, "separate", float("nan"))
    _backward(tw, gt, dC, overwrite=True)
    want = gt.host()
    tw.close()
    assert np.isfinite(want[4]).all() and np.any(want[4] != 0) and np.any(want[0] != 0)
    ka3 = _k3(active)
    rig = _Rig(sc, stored, active, w=w, h=h, debug_flags=fill_flag)
    for layout in layouts:
        for phases in ("all", "split"):
            rig.frame(0)
            g = _Grads(n, stored, layout, float("nan"))
            if layout == "flat":
                assert (g.t[4].data_ptr() % 16 != 0) == (n % 4 != 0)
            _backward(rig, g, dC, overwrite=True, phases=phases)
            got = g.host()
            tag = (layout, phases)
            if phases == "all":                                            # the composite launch carried the zero fill of d_shs, or did not
                assert (rig.ctx.tail_fill_blocks()[1] > 0) == (fill_flag == 0), tag
            for k in range(4):
                assert same_bits(got[k], want[k]), (tag, k)
            assert same_bits(got[4][:, :ka3], want[4]), tag
            assert not bits(got[4][:, ka3:]).any(), (tag, "an inactive float is not +0")
    rig.close()


@pytest.mark.parametrize("fill_flag", [0, NO_TAIL_FILL], ids=["tail_fill", "no_tail_fill"])
@pytest.mark.parametrize("stored,active", BWD_PAIRS)
def test_backward_overwrite(stored, active, fill_flag):
    _overwrite_case(stored, active, N, W, H, fill_flag, ("flat", "separate"))


@pytest.mark.parametrize("fill_flag", [0, NO_TAIL_FILL], ids=["tail_fill", "no_tail_fill"])
def test_backward_overwrite_small_aligned(fill_flag):
    _overwrite_case(3, 1, 300, 64, 48, fill_flag, ("separate",))


# ---------------------------------------------------------------- 4. backward, accumulate
@pytest.mark.parametrize("layout", ["flat", "separate"])
@pytest.mark.parametrize("stored,active", BWD_PAIRS)
def test_backward_accumulate_two_views(stored, active, layout):
    sc = _scene(N, W, H, stored, 140 + 10 * stored + active)
    ka3 = _k3(active)
    rng = np.random.default_rng(stored * 7 + active)
    start = [rng.standard_normal((N, w)).astype(np.float32) for w in (3, 3, 4, 1, _k3(stored))]
    full, tw = _Rig(sc, stored, active), _Rig(_twin_scene(sc, active), active)
    it = iter(start)
    g = _Grads(N, stored, layout, lambda shape: next(it))
    it2 = iter(start[:4] + [start[4][:, :ka3]])
    gt = _Grads(N, active, layout, lambda shape: np.ascontiguousarray(next(it2)))
    for v in (0, 1):
        for rig, gg in ((full, g), (tw, gt)):
            rig.frame(v)
            _backward(rig, gg, _dC(v), overwrite=False)
    got, want = g.host(), gt.host()
    for k in range(4):
        assert same_bits(got[k], want[k]), k
    assert same_bits(got[4][:, :ka3], want[4])
    assert same_bits(got[4][:, ka3:], start[4][:, ka3:])                        # neither read nor written
    assert not same_bits(got[4][:, :ka3], start[4][:, :ka3])
    full.close(); tw.close()


# ---------------------------------------------------------------- 5. fused forms
@pytest.mark.parametrize("selective", [False, True], ids=["dense", "selective"])
@pytest.mark.parametrize("stored,active", BWD_PAIRS)
def test_backward_adam_equals_backward_then_adam_step(stored, active, selective):
    import torch
    sc = _scene(N, W, H, stored, 150 + 10 * stored + active)
    dC = _dC(2)
    rng = np.random.default_rng(31 * stored + active)
    widths = (3, 3, 4, 1, _k3(stored))
    m0 = [(0.01 * rng.standard_normal((N, w))).astype(np.float32) for w in widths]      # non-zero moments, the inactive bands included
    v0 = [(0.01 * rng.random((N, w)) + 1e-6).astype(np.float32) for w in widths]
    res = []
    for fused in (True, False):
        rig = _Rig(sc, stored, active)
        im, iv = iter(m0), iter(v0)
        m, v = _Grads(N, stored, "flat", lambda s: next(im)), _Grads(N, stored, "flat", lambda s: next(iv))
        rig.frame(0)
        if fused:
            rig.ctx.backward_adam(dC.data_ptr(), m.struct(), v.struct(), LR6, B1, B2, EPS, 3, selective=selective)
        else:
            g = _Grads(N, stored, "flat", float("nan"))
            _backward(rig, g, dC, overwrite=True)
            rig.ctx.adam_step(g.struct(), m.struct(), v.struct(), LR6, B1, B2, EPS, 3, selective=selective)
        torch.cuda.synchronize()
        res.append([t.cpu().numpy().copy() for t in rig.p] + m.host() + v.host())
        rig.close()
    for k, (a, b) in enumerate(zip(*res)):
        assert same_bits(a, b), k
    ka3 = _k3(active)
    shs0 = sc["shs"].reshape(N, -1)
    moved = (bits(res[0][4]) != bits(shs0)).any(axis=1)
    assert (bits(res[0][4][:, ka3:]) != bits(shs0[:, ka3:])).any()        # old moments move the inactive floats of the rows that are stepped
    if selective:
        assert 0 < moved.sum() < N                                          # ... and dead rows stay as they were
    else:
        assert moved.all()


@pytest.mark.parametrize("stored,active", BWD_PAIRS)
def test_backward_sgd_equals_backward_then_sgd_step(stored, active):
    import torch
    sc = _scene(N, W, H, stored, 160 + 10 * stored + active)
    dC = _dC(3)
    res = []
    for fused in (True, False):
        rig = _Rig(sc, stored, active)
        rig.frame(0)
        if fused:
            rig.ctx.backward_sgd(dC.data_ptr(), 0.05)
        else:
            g = _Grads(N, stored, "flat", float("nan"))
            _backward(rig, g, dC, overwrite=True)
            rig.ctx.sgd_step(0.05, g.struct())
        torch.cuda.synchronize()
        res.append([t.cpu().numpy().copy() for t in rig.p])
        rig.close()
    for k, (a, b) in enumerate(zip(*res)):
        assert same_bits(a, b), k
    ka3 = _k3(active)
    shs0 = sc["shs"].reshape(N, -1)
    assert same_bits(res[0][4][:, ka3:], shs0[:, ka3:])
    assert not same_bits(res[0][4][:, :ka3], shs0[:, :ka3])


# ---------------------------------------------------------------- 6. exchange kernels
@pytest.mark.parametrize("overwrite", [True, False], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("stored,active", BWD_PAIRS)
def test_exchange_kernels_rebuild_the_active_bands(stored, active, overwrite):
    import torch
    from gaussiansplat_amd import distributed as D, synthetic
    sc = _scene(N, W, H, stored, 170 + 10 * stored + active)
    cams = D.view_records([synthetic.scene_camera(W, view=v) for v in range(3)], W, H)
    rng = np.random.default_rng(stored * 11 + active)
    dense = rng.standard_normal((3, N, 3)).astype(np.float32)
    dense[rng.random((3, N)) < 0.6] = 0.0                                 # untouched gaussians
    dense[1] = 0.0                                                          # a view that touches nothing
    mask, counts, rows = D.pack_touched_rows(torch.from_numpy(dense))
    cap = int(counts.max()) + 5
    padded = torch.full((3, cap, 3), float("nan"), dtype=torch.float32)
    for v, r in enumerate(rows):
        padded[v, :r.shape[0]] = r
    d_dense, d_bits, d_rows = torch.from_numpy(dense).cuda(), mask.cuda().contiguous(), padded.cuda().contiguous()
    ka3, ks3 = _k3(active), _k3(stored)
    start = rng.standard_normal((N, ks3)).astype(np.float32) if not overwrite else np.full((N, ks3), np.nan, np.float32)
    full, tw = _Rig(sc, stored, active), _Rig(_twin_scene(sc, active), active)
    res = {}
    for name, rig, init in (("full", full, start), ("twin", tw, np.ascontiguousarray(start[:, :ka3]))):
        for kind in ("views", "touched"):
            out = torch.as_tensor(init).cuda().contiguous()
            if kind == "views":
                rig.ctx.sh_grads_from_views(cams, d_dense.data_ptr(), out.data_ptr(), overwrite=overwrite)
            else:
                rig.ctx.sh_grads_from_touched(cams, d_bits.data_ptr(), d_rows.data_ptr(), cap, out.data_ptr(), overwrite=overwrite)
            torch.cuda.synchronize()
            res[name, kind] = out.cpu().numpy()
    for kind in ("views", "touched"):
        got, want = res["full", kind], res["twin", kind]
        assert np.isfinite(want).all() and np.any(want != start[:, :ka3])
        assert same_bits(got[:, :ka3], want), kind
        if overwrite:
            assert not bits(got[:, ka3:]).any(), kind
        else:
            assert same_bits(got[:, ka3:], start[:, ka3:]), kind
    full.close(); tw.close()


# ---------------------------------------------------------------- 7. contract
def test_contract_range_clamp_and_2d():
    from gaussiansplat_amd import backend as B, synthetic
    rig = _Rig(_scene(N, W, H, 1, 180), 1)
    L, h = rig.ctx.L, rig.ctx.h
    for bad in (-2, 4):
        assert L.gs_set_active_sh_degree(h, bad) == B.GS_ERR_INVALID
        assert rig.ctx.active_sh_degree == 1                               # a refused call changes nothing
    rig.ctx.set_active_sh_degree(3)
    assert rig.ctx.active_sh_degree == 1                                   # a request above the model's degree
    rig.ctx.set_active_sh_degree(0)
    assert rig.ctx.active_sh_degree == 0
    rig.ctx.set_active_sh_degree(-1)
    assert rig.ctx.active_sh_degree == 1
    rig.close()
    ctx2 = B.Context()
    s2 = synthetic.make_scene_2d(50, 64, 48, seed=3)
    ctx2.set_model_2d_host(s2["means"], s2["scales"], s2["rots"], s2["opacities"], s2["colors"])
    assert ctx2.L.gs_set_active_sh_degree(ctx2.h, 0) == B.GS_ERR_UNSUPPORTED
    assert ctx2.L.gs_get_active_sh_degree(ctx2.h) == B.GS_ERR_UNSUPPORTED
    ctx2.close()


def test_contract_a_change_drops_the_frame_and_a_noop_keeps_it():
    from gaussiansplat_amd import backend as B
    rig = _Rig(_scene(N, W, H, 2, 181), 2)
    rig.view(0)
    rig.ctx.preprocess()
    rig.ctx.set_active_sh_degree(2)                                        # the value in force, three ways
    rig.ctx.set_active_sh_degree(-1)
    rig.ctx.set_active_sh_degree(3)
    rig.ctx.bin()                                                          # the frame stands
    rig.ctx.preprocess()
    rig.ctx.set_active_sh_degree(1)
    with pytest.raises(B.GsError) as e:
        rig.ctx.bin()
    assert e.value.code == B.GS_ERR_INVALID
    rig.ctx.preprocess(); rig.ctx.bin()
    rig.ctx.set_active_sh_degree(1)                                        # in force already: the binned frame renders
    rig.ctx.forward_device(0, 0)
    rig.close()


def test_contract_the_request_survives_set_model():
    import torch
    from gaussiansplat_amd import backend as B
    rig = _Rig(_scene(N, W, H, 3, 182), 3, active=1)
    other = _scene(300, W, H, 2, 183)                                      # another size and another degree
    p2 = [torch.as_tensor(np.ascontiguousarray(other[k], np.float32).reshape(300, -1)).cuda() for k in ("means", "scales", "quats", "opacities", "shs")]
    rig.ctx.set_model_device(300, 2, [t.data_ptr() for t in p2])
    assert rig.ctx.active_sh_degree == 1
    rig.n, rig.deg, rig.p = 300, 2, p2
    rig.frame(0)
    img = rig.ctx.forward_host()[0]
    tw = _Rig(_twin_scene(other, 1), 1)
    tw.frame(0)
    assert same_bits(img, tw.ctx.forward_host()[0])
    p0 = [torch.as_tensor(np.ascontiguousarray(other[k], np.float32).reshape(300, -1)[:, :w]).cuda().contiguous()
          for k, w in zip(("means", "scales", "quats", "opacities", "shs"), (3, 3, 4, 1, 3))]
    rig.ctx.set_model_device(300, 0, [t.data_ptr() for t in p0])           # a model below the request: its own degree, the request kept
    assert rig.ctx.active_sh_degree == 0
    rig.ctx.set_model_device(300, 2, [t.data_ptr() for t in p2])
    assert rig.ctx.active_sh_degree == 1
    rig.close(); tw.close()


def test_contract_the_request_survives_a_density_restructure():
    import torch
    from gaussiansplat_amd import renderer as R, synthetic, train as TR
    from gaussiansplat_amd.density import DensityController
    from gaussiansplat_amd.optim import Adam
    sc = _scene(N, W, H, 2, 184)
    cam = synthetic.scene_camera(W)
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, sc, deterministic=True, tile_parts=1)
    r.active_sh_degree = 0
    assert r.active_sh_degree == 0
    lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
    gt = torch.rand((3, H, W), device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    extent = float(np.linalg.norm(sc["means"].max(0) - sc["means"].min(0)) / 2)
    ctl = DensityController(scene_extent=extent, from_iter=1, until_iter=10, interval=2, opacity_reset_interval=0, grad_threshold=2e-6,
                            generator=torch.Generator("cuda").manual_seed(6))
    opt = Adam(r, lr=1e-3)
    for _ in range(2):
        TR.trainStep(r, gt, 0.0, lf, cam, want_loss=False, optimizer=opt, density=ctl)
    assert len(ctl.history) == 1 and r.nGaussians != N                     # one restructure: gs_set_model onto a model of another size
    assert r.active_sh_degree == 0
    before = r.splatData.shs.clone()
    TR.trainStep(r, gt, 0.0, lf, cam, want_loss=False, optimizer=opt)
    torch.cuda.synchronize()
    # clones and children start with zero moments, survivors carry theirs: whatever moves, no inactive gradient arrived -- the moments of
    # the inactive bands were zero before the restructure (degree 0 from the start), so these floats stand still
    assert torch.equal(before[:, 3:].view(torch.int32), r.splatData.shs[:, 3:].view(torch.int32))
    assert not torch.equal(before[:, :3], r.splatData.shs[:, :3])


# ---------------------------------------------------------------- 8. schedule
@pytest.mark.parametrize("fused", [False, True], ids=["adam", "fused_adam"])
def test_schedule_equals_a_hand_written_loop(fused):
    import torch
    from gaussiansplat_amd import renderer as R, synthetic, train as TR
    from gaussiansplat_amd.optim import Adam
    sc = _scene(N, W, H, 2, 190)
    cam = synthetic.scene_camera(W)
    gt = torch.rand((3, H, W), device="cuda", generator=torch.Generator("cuda").manual_seed(9))
    rates = dict(means=1e-3, scales=4e-3, quaternions=2e-3, opacities=5e-2, sh_dc=2.5e-3, sh_rest=1.25e-4)
    start = torch.as_tensor(sc["shs"].reshape(N, -1)).cuda()
    snaps = {}
    for how in ("schedule", "by_hand"):
        r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, sc, deterministic=True, tile_parts=1)
        R.resetGrads(r)
        lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
        opt = Adam(r, lr=rates, fused=fused)
        sched = TR.SHDegreeSchedule(every=2)
        for it in range(4):
            if how == "schedule":
                TR.trainStep(r, gt, 0.0, lf, cam, want_loss=False, optimizer=opt, sh_schedule=sched)
            else:
                r.active_sh_degree = min(2, it // 2)
                TR.trainStep(r, gt, 0.0, lf, cam, want_loss=False, optimizer=opt)
            assert r.active_sh_degree == it // 2
            torch.cuda.synchronize()
            sd = r.splatData
            snaps[how, it] = [t.clone() for t in (sd.means, sd.scales, sd.quaternions, sd.opacities, sd.shs, opt.exp_avg, opt.exp_avg_sq)]
        assert how != "schedule" or sched.iteration == 4
    for it in range(4):
        for k, (a, b) in enumerate(zip(snaps["schedule", it], snaps["by_hand", it])):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (it, k)
    i32 = lambda t: t.view(torch.int32)
    s1, s3 = snaps["schedule", 1][4], snaps["schedule", 3][4]
    assert torch.equal(i32(s1[:, 3:]), i32(start[:, 3:])) and not torch.equal(s1[:, :3], start[:, :3])     # after step 1: bands 1, 2 untouched
    assert not torch.equal(s3[:, 3:12], start[:, 3:12])                                                     # after step 3: band 1 has moved ...
    assert torch.equal(i32(s3[:, 12:]), i32(start[:, 12:]))                                                 # ... band 2 has not


# ---------------------------------------------------------------- 9. views in flight follow the renderer
def test_pipelined_view_batch_follows_the_renderers_active_degree():
    """distributed.multi_view_step renders a rank's views on twin renderers with ctxs of their own: they take the active degree of
    the rank's renderer, also when it changes between two batches; the batch equals the views rendered one after the other."""
    import torch
    from gaussiansplat_amd import distributed as D, renderer as R, synthetic
    sc = _scene(N, W, H, 3, 200)
    cams = [synthetic.scene_camera(W, view=v) for v in range(3)]
    dCs = [_dC(10 + v) for v in range(3)]
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, sc, deterministic=True, tile_parts=1)
    r2 = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, sc, deterministic=True, tile_parts=1)
    hv = D.HipViewRenderer(r)
    for active in (1, 0, 3):
        r.active_sh_degree = r2.active_sh_degree = active
        R.resetGrads(r)
        flat = D.multi_view_step(hv, cams, dCs, exchange=False).clone()
        R.resetGrads(r2)
        for cam, dC in zip(cams, dCs):
            R.forward(r2, (R.preprocess(r2, cam), R.compactIdxs(r2))[0])
            R.backward(r2, dC)
        torch.cuda.synchronize()
        want = r2.splatGrads.flat
        assert torch.equal(flat.view(torch.int32), want.view(torch.int32)), active
        shs = flat[11 * N:].view(N, 48)
        ka3 = _k3(active)
        assert torch.any(shs[:, :ka3] != 0) and not torch.any(shs[:, ka3:].view(torch.int32) != 0)
