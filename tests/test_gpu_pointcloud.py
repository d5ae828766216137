"""Point-cloud initialisation on the device (gs_knn_mean_dist2, gs_init_from_points, gaussiansplat_amd.pointcloud): the exact 3-NN search
bit for bit against the NumPy brute force of tests/knn_ref.py on every planted cloud and against a torch brute force on larger ones, a
frame that a search in its middle leaves untouched, the model arrays against NumPy float32 (the scales within one float ulp of the double
log's rounding, as include/gsplat.h derives), the refusals, and a renderer built from a PointCloud."""
import math

import numpy as np
import pytest

import knn_ref as K
from common import bits, dev, on_torch_stream, refused, same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = f32(-777.25)
PAD = 64                                    # floats / rows of SENTINEL behind every output: nothing may be written there
SH_C0 = f32(0.28209479177387814)


@pytest.fixture(scope="module")
def ctx():
    from gaussiansplat_amd import backend as B
    c = B.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def clouds():
    return K.clouds()


@pytest.fixture(scope="module")
def refs(clouds):
    return {name: K.knn_mean_dist2(p) for name, p in clouds.items()}


def _knn(ctx, pts):
    """dist2 of the host array pts through the raw call, with the checks every case shares: the pad behind dist2 and the points are untouched"""
    import torch
    n = len(pts)
    tp = dev(pts)
    out = torch.full((n + PAD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    on_torch_stream(ctx)
    ctx.knn_mean_dist2(tp.data_ptr(), n, out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[n:] == SENTINEL)
    assert same_bits(tp.cpu().numpy(), pts, nan_equal=True)
    return got[:n]


def _mismatch(got, want):
    return np.flatnonzero(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


# ---------------------------------------------------------------- 1. bit for bit against the NumPy brute force
def test_case_list_is_complete(clouds):
    from gaussiansplat_amd import backend as B
    assert B.KNN_BOX == K.BOX
    want = {f"uniform{n}" for n in (4, 5, 63, 64, 65, K.BOX - 1, K.BOX, K.BOX + 1, 4097)}
    want |= {"clustered", "duplicates", "all_identical", "line", "plane", "lattice", "nonfinite", "too_few", "overflow", "overflow_mixed"}
    assert want <= set(clouds)
    assert 4097 % 4096 == 1 and 4097 % K.BOX == 1                        # one past a radix chunk and past a multiple of the box


@pytest.mark.parametrize("name", list(K.clouds()))
def test_knn_matches_brute_force_bit_for_bit(ctx, clouds, refs, name):
    pts, ref = clouds[name], refs[name]
    K.check_planted(name, pts, ref)                                      # the reference alone shows the case's kind of result
    got = _knn(ctx, pts)
    bad = _mismatch(got, ref)
    assert bad.size == 0, (name, bad[:8], got[bad[:8]], ref[bad[:8]])


def test_python_knn_mean_dist2_on_a_tensor(ctx, clouds, refs):
    from gaussiansplat_amd import pointcloud
    pts = clouds["nonfinite"]
    for c in (None, ctx):                                                # a short-lived ctx of its own, or the caller's
        got = pointcloud.knn_mean_dist2(dev(pts), c).cpu().numpy()
        assert _mismatch(got, refs["nonfinite"]).size == 0
    with pytest.raises(TypeError):
        pointcloud.knn_mean_dist2(pts)                                   # host memory: there is no CPU path


# ---------------------------------------------------------------- 2. a larger cloud against a torch brute force on the device
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_larger_cloud_matches_torch_brute_force(ctx, kind):
    import torch
    from gaussiansplat_amd import synthetic
    n = 30001
    pts = K.uniform(n, 21) if kind == "uniform" else synthetic.make_scene(n, 1920, 1080, 0, seed=22, clustered=True)["means"]
    want = K.torch_brute(dev(pts))
    assert np.isfinite(want).all() and np.count_nonzero(want > 0) > n // 2
    got = _knn(ctx, pts)
    bad = _mismatch(got, want)
    assert bad.size == 0, (kind, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


# ---------------------------------------------------------------- 3. the frame is left alone
def test_a_search_between_forward_and_backward_leaves_the_frame_untouched():
    import torch
    from gaussiansplat_amd import renderer as R, synthetic
    n, W, H, deg = 3000, 200, 136, 1
    scene = synthetic.make_scene(n, W, H, deg, seed=31)
    cam = synthetic.scene_camera(W)
    dC = torch.as_tensor(synthetic.make_dC(W, H, 32)).cuda()
    pts = dev(K.uniform(5000, 33))
    want = K.knn_mean_dist2(pts.cpu().numpy())
    res = []
    for with_knn in (False, True):
        r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, scene, deterministic=True, tile_parts=1)
        R.forward(r, (R.preprocess(r, cam), R.compactIdxs(r))[0])
        d2 = None
        if with_knn:
            d2 = torch.empty(pts.shape[0], dtype=torch.float32, device="cuda")
            r.ctx.knn_mean_dist2(pts.data_ptr(), pts.shape[0], d2.data_ptr())      # the renderer's own ctx, in the middle of its frame
        R.resetGrads(r)
        R.backward(r, dC)
        torch.cuda.synchronize()
        res.append((r.imageData.cpu().numpy().copy(), r.transmittance.cpu().numpy().copy(), r.splatGrads.flat.cpu().numpy().copy()))
        if with_knn:
            assert _mismatch(d2.cpu().numpy(), want).size == 0
    (img0, tr0, g0), (img1, tr1, g1) = res
    assert float(tr0.min()) < 1.0 and np.count_nonzero(g0) > g0.size // 10      # a real frame with real gradients
    assert same_bits(img0, img1, nan_equal=True) and same_bits(tr0, tr1, nan_equal=True) and same_bits(g0, g1, nan_equal=True)


# ---------------------------------------------------------------- 4. gs_init_from_points
def _ordered(a):
    """float32 -> integers whose difference counts float steps (across zero as well)"""
    i = np.ascontiguousarray(a, f32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _init_inputs(n=1000, seed=41):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((n, 3)).astype(f32)
    col = rng.random((n, 3), dtype=f32)
    col[0], col[1], col[2] = 0.0, 1.0, 0.5
    d2 = (10.0 ** rng.uniform(-9.0, 6.0, n)).astype(f32)
    d2[:6] = [0.0, 1e-8, np.nan, np.inf, 1e-7, np.nextafter(f32(1e-7), f32(1.0))]
    d2[6] = 1.0
    return pts, col, d2


def _dst(n, k3):
    import torch
    return [torch.full((n + PAD, w), float(SENTINEL), dtype=torch.float32, device="cuda") for w in (3, 3, 4, 1, k3)]


def _grads(ts):
    from gaussiansplat_amd import backend as B
    return B.GsGrads(*(t.data_ptr() for t in ts))


@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("with_colors", [True, False])
def test_init_from_points_matches_numpy(ctx, deg, with_colors):
    import torch
    n, k3 = 1000, 3 * (deg + 1) ** 2
    pts, col, d2 = _init_inputs(n)
    tp, tc, td = dev(pts), dev(col), dev(d2)
    dst = _dst(n, k3)
    logit = f32(math.log(0.1 / 0.9))
    on_torch_stream(ctx)
    ctx.init_from_points(tp.data_ptr(), tc.data_ptr() if with_colors else None, td.data_ptr(), n, deg, float(logit), _grads(dst))
    torch.cuda.synchronize()
    means, scales, quats, opac, shs = (t.cpu().numpy() for t in dst)
    for a in (means, scales, quats, opac, shs):
        assert np.all(a[n:] == SENTINEL)
    assert same_bits(means[:n], pts, nan_equal=True)
    assert same_bits(quats[:n], np.tile(np.array([1.0, 0.0, 0.0, 0.0], f32), (n, 1)), nan_equal=True)
    assert same_bits(opac[:n], np.full((n, 1), logit, f32), nan_equal=True)
    want_sh = np.zeros((n, k3), f32)                                     # +0.0
    if with_colors:
        want_sh[:, :3] = (col - f32(0.5)) / SH_C0
    assert same_bits(shs[:n], want_sh, nan_equal=True)
    with np.errstate(invalid="ignore"):
        v = np.where(d2 > f32(1e-7), d2, f32(1e-7))                      # a NaN compares false
    assert v[0] == v[1] == v[2] == v[4] == f32(1e-7) and v[3] == np.inf and v[5] > f32(1e-7)
    with np.errstate(divide="ignore"):
        want_s = (0.5 * np.log(v.astype(np.float64))).astype(f32)
    assert want_s[3] == np.inf and want_s[6] == 0.0
    s = scales[:n]
    assert same_bits(s[:, 0], s[:, 1], nan_equal=True) and same_bits(s[:, 0], s[:, 2], nan_equal=True)
    fin = np.isfinite(want_s)
    assert same_bits(s[~fin, 0], want_s[~fin], nan_equal=True)
    steps = np.abs(_ordered(s[fin, 0]) - _ordered(want_s[fin]))
    print("init_from_points deg %d: scales differ from float32(0.5 * log(float64(v))) by at most %d float steps (%d of %d rows differ)"
          % (deg, int(steps.max()), int(np.count_nonzero(steps)), int(fin.sum())))
    assert steps.max() <= 1


def test_refusals_return_their_code_and_write_nothing(ctx):
    import torch
    from gaussiansplat_amd import backend as B
    n, deg, k3 = 200, 1, 12
    pts, col, d2 = _init_inputs(n)
    tp, tc, td = dev(pts), dev(col), dev(d2)
    dst = _dst(n, k3)
    on_torch_stream(ctx)
    P, Cc, D = tp.data_ptr(), tc.data_ptr(), td.data_ptr()

    for bad_deg in (-1, 4):
        refused(lambda: ctx.init_from_points(P, Cc, D, n, bad_deg, -2.0, _grads(dst)), code=B.GS_ERR_INVALID)
    refused(lambda: ctx.init_from_points(None, Cc, D, n, deg, -2.0, _grads(dst)), code=B.GS_ERR_INVALID)
    refused(lambda: ctx.init_from_points(P, Cc, None, n, deg, -2.0, _grads(dst)), code=B.GS_ERR_INVALID)
    refused(lambda: ctx.init_from_points(P, Cc, D, -1, deg, -2.0, _grads(dst)), code=B.GS_ERR_INVALID)
    for i in range(5):                                                   # a NULL destination
        g = _grads(dst)
        setattr(g, B.GsGrads._fields_[i][0], None)
        refused(lambda: ctx.init_from_points(P, Cc, D, n, deg, -2.0, g), code=B.GS_ERR_INVALID)
    g = _grads(dst)
    g.d_scales = g.d_means + 4                                           # two destinations overlap
    refused(lambda: ctx.init_from_points(P, Cc, D, n, deg, -2.0, g), code=B.GS_ERR_INVALID)
    for src in (P, Cc, D):                                               # a destination overlaps a source
        g = _grads(dst)
        g.d_opacities = src
        refused(lambda: ctx.init_from_points(P, Cc, D, n, deg, -2.0, g), code=B.GS_ERR_INVALID)
    # the search
    out = torch.full((n + PAD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    refused(lambda: ctx.knn_mean_dist2(None, n, out.data_ptr()), code=B.GS_ERR_INVALID)
    refused(lambda: ctx.knn_mean_dist2(P, n, None), code=B.GS_ERR_INVALID)
    refused(lambda: ctx.knn_mean_dist2(P, -1, out.data_ptr()), code=B.GS_ERR_INVALID)
    refused(lambda: ctx.knn_mean_dist2(P, n, P + 4 * (3 * n - 1)), code=B.GS_ERR_INVALID)   # dist2 starts on the last float of points
    refused(lambda: ctx.knn_mean_dist2(P + 4, n - 1, P), code=B.GS_ERR_INVALID)             # ... or ends inside them
    refused(lambda: ctx.knn_mean_dist2(P, 2 ** 31, out.data_ptr()), code=B.GS_ERR_UNSUPPORTED)
    ctx.knn_mean_dist2(P, 0, out.data_ptr())                             # n == 0: fine, nothing enqueued
    ctx.knn_mean_dist2(None, 0, None)
    torch.cuda.synchronize()
    for t in dst + [out]:
        assert bool((t == float(SENTINEL)).all())
    assert same_bits(tp.cpu().numpy(), pts, nan_equal=True) and same_bits(tc.cpu().numpy(), col, nan_equal=True) and same_bits(td.cpu().numpy(), d2, nan_equal=True)


# ---------------------------------------------------------------- 5. end to end
def test_renderer_from_a_point_cloud():
    import torch
    from gaussiansplat_amd import renderer as R, synthetic
    from gaussiansplat_amd.camera import scene_extent
    from gaussiansplat_amd.density import density_params
    from gaussiansplat_amd.pointcloud import PointCloud, from_points
    n, W, H, deg = 2000, 128, 96, 2
    means = synthetic.make_scene(n, W, H, deg, seed=51)["means"]
    colours = np.random.default_rng(52).random((n, 3), dtype=f32)
    pc = PointCloud(means, colours, sh_degree=deg)
    cams = [synthetic.scene_camera(W, view=v) for v in range(4)]
    r1 = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, pc, deterministic=True, tile_parts=1)
    assert r1.nGaussians == n and r1.sh_degree == deg
    d = from_points(pc)
    scene = dict(means=d.means.cpu().numpy(), scales=d.scales.cpu().numpy(), quats=d.quaternions.cpu().numpy(),
                 opacities=d.opacities.cpu().numpy().reshape(n), shs=d.shs.cpu().numpy().reshape(n, (deg + 1) ** 2, 3))
    # what from_points built is what the contract says, from the reference search
    v = np.maximum(K.knn_mean_dist2(means), f32(1e-7))
    steps = np.abs(_ordered(scene["scales"][:, 0]) - _ordered((0.5 * np.log(v.astype(np.float64))).astype(f32)))
    assert steps.max() <= 1 and same_bits(scene["means"], means, nan_equal=True)
    assert same_bits(scene["opacities"], np.full(n, f32(math.log(0.1 / 0.9)), f32), nan_equal=True)
    assert same_bits(scene["shs"][:, 0, :], (colours - f32(0.5)) / SH_C0, nan_equal=True) and not scene["shs"][:, 1:, :].any()
    r2 = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, scene, deterministic=True, tile_parts=1)
    imgs = []
    for r in (r1, r2):
        R.forward(r, (R.preprocess(r, cams[0]), R.compactIdxs(r))[0])
        torch.cuda.synchronize()
        imgs.append((r.imageData.cpu().numpy().copy(), r.transmittance.cpu().numpy().copy()))
    assert same_bits(imgs[0][0], imgs[1][0], nan_equal=True) and same_bits(imgs[0][1], imgs[1][1], nan_equal=True)
    assert float(imgs[0][1].min()) < 1.0 and float(imgs[0][0].max()) > 0.0
    R.resetGrads(r1)
    R.backward(r1, torch.as_tensor(synthetic.make_dC(W, H, 53)).cuda())
    torch.cuda.synchronize()
    g = r1.splatGrads.flat.cpu().numpy()
    assert np.isfinite(g).all() and np.count_nonzero(g) > 0
    density_params(scene_extent=scene_extent(cams))
    with pytest.raises(TypeError, match="PointCloud"):
        R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, 3.5)
