"""Feature maps (gs_view_depth, gs_render_features, gs_backward_features, gs_view_depth_backward; renderer.renderFeatures / renderDepth
and their backwards): the finished frame's composite launches over a second payload whose three colour floats are the caller's.

1. depth values: gs_view_depth == GS_ARR_TS row 2 bit for bit, legal without a frame and in the middle of one
2. the walk is the frame's walk: feat = GS_ARR_RGB gives the frame's image and transmittance bit for bit (one wave per tile; both early-out
   settings, both cull settings, capped and extended lists), within the pixel bar with tiles shared between waves
3. forward parity of the depth planes against the fp32 oracle composited with rgb := (z, z^2, 1), also on a grid with a launch order
4. gradient parity against fp64 autograd (tests/torch_ref.py), features constant and features = depth; deterministic runs repeat bit for bit
5. the frame is untouched: a twin ctx without the feature calls gives the same bits everywhere
6. refusals, after which the frame still renders and backpropagates identically

Bars.  Pixels: the project's 1e-4 + 1e-4 |x| for colours of magnitude ~1; C is linear in the triple and the alpha errors are the same, so
plane c gets s_c 1e-4 + 1e-4 |x| with s_c = max(1, max |feat_c|) over the listed gaussians.  Gradients: 1e-3 rel-L2, the standing bar."""
import numpy as np
import pytest
import torch

import torch_ref
from common import GRADS, dev, hip_context, on_torch_stream, refused, rel_l2, scene_and_cameras

pytestmark = pytest.mark.gpu


def _ctx(sc, cam, T, P, W, H, deg, **kw):
    return on_torch_stream(hip_context(sc, cam, T, P, W, H, deg, **kw))


def _scene(n, W, H, deg, seed, grow=3.0, dop=4.0):
    """Dense by default: larger and more opaque splats, so that pixels saturate and the early-out stops tiles inside their lists (at the
    sizes used here a quarter of the pixels and more end below t_min; with grow = 1, dop = 0 none does)."""
    sc, cam, T, P, ocam = scene_and_cameras(n, W, H, deg, seed)
    sc["scales"] = (sc["scales"] + np.float32(grow)).astype(np.float32)
    sc["opacities"] = (sc["opacities"] + np.float32(dop)).astype(np.float32)
    return sc, cam, T, P, ocam


def _bound_forward(ctx, W, H):
    """forward into two torch tensors the ctx is bound to: what the frame's image IS can be read at any later time"""
    img = torch.zeros((3, H, W), dtype=torch.float32, device="cuda"); tr = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    ctx.bind_outputs(img.data_ptr(), tr.data_ptr())
    ctx.preprocess(); ctx.bin()
    ctx.forward_device(img.data_ptr(), tr.data_ptr())
    return img, tr


def _render_features(ctx, feat, W, H, want_trans=True):
    f = feat if isinstance(feat, torch.Tensor) else dev(feat)
    out = torch.full((3, H, W), -7.0, dtype=torch.float32, device="cuda")
    tr = torch.full((H, W), -7.0, dtype=torch.float32, device="cuda") if want_trans else None
    ctx.render_features(f.data_ptr(), out.data_ptr(), tr.data_ptr() if want_trans else 0)
    torch.cuda.synchronize()
    return out, tr


def _grad_tensors(n, deg):
    k3 = 3 * (deg + 1) ** 2
    return [torch.zeros(s, dtype=torch.float32, device="cuda") for s in ((n, 3), (n, 3), (n, 4), (n,), (n, k3))]


def _gs_grads(ts):
    from gaussiansplat_amd import backend as B
    return B.GsGrads(*(t.data_ptr() for t in ts))


# ---------------------------------------------------------------- 1. depth values

def test_view_depth_equals_ts_row_2_bit_for_bit():
    from gaussiansplat_amd import backend as B, synthetic
    n, W, H, deg = 1000, 80, 56, 1
    sc, cam, T, P, ocam = _scene(n, W, H, deg, 81)
    ctx = _ctx(sc, cam, T, P, W, H, deg, export_debug=True, deterministic=True)
    z = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    ctx.view_depth(z.data_ptr())                                          # no frame yet
    torch.cuda.synchronize()
    z0 = z.cpu().numpy()
    ctx.preprocess(); ctx.bin()
    img, tr = ctx.forward_host()
    ts = ctx.get_array(B.ARR_TS)
    assert np.isfinite(ts[:, 2]).all() and len(np.unique(ts[:, 2])) > n // 2
    assert np.array_equal(z0.view(np.uint32), ts[:, 2].view(np.uint32))
    z.fill_(-1.0)
    ctx.view_depth(z.data_ptr())                                          # between forward and backward
    torch.cuda.synchronize()
    assert np.array_equal(z.cpu().numpy().view(np.uint32), ts[:, 2].view(np.uint32))
    dC = synthetic.make_dC(W, H, 81)
    g = ctx.grads_alloc()
    ctx.backward(dC, g)                                                   # the frame went on as if nothing had happened
    got = ctx.grads_read(g, deg)
    twin = _ctx(sc, cam, T, P, W, H, deg, export_debug=True, deterministic=True)
    twin.preprocess(); twin.bin()
    img2, tr2 = twin.forward_host()
    g2 = twin.grads_alloc()
    twin.backward(dC, g2)
    want = twin.grads_read(g2, deg)
    assert np.array_equal(img, img2) and np.array_equal(tr, tr2)
    for k in GRADS:
        assert np.array_equal(got[k], want[k]), k
    # the adjoint: d_means[g][j] += T[2 + 4 j] * dz[g], one multiply and one add; dz == 0 rows are left alone (a NaN there stays a NaN)
    rng = np.random.default_rng(81)
    dz = rng.standard_normal(n).astype(np.float32)
    dz[::7] = 0.0
    dz[7] = -0.0
    base = rng.standard_normal((n, 3)).astype(np.float32)
    base[14] = np.nan
    dm = dev(base)
    ctx.view_depth_backward(dev(dz).data_ptr(), dm.data_ptr())
    torch.cuda.synchronize()
    Tf = np.ascontiguousarray(T, np.float32).reshape(-1)
    want_dm = base.copy()
    live = dz != 0.0
    for j in range(3):
        want_dm[live, j] = base[live, j] + Tf[2 + 4 * j] * dz[live]
    got_dm = dm.cpu().numpy()
    assert np.array_equal(got_dm.view(np.uint32), want_dm.view(np.uint32))


# ---------------------------------------------------------------- 2. the walk is the frame's walk

def _rgb_round_trip(ctx, W, H, bitwise):
    from gaussiansplat_amd import backend as B
    img, tr = _bound_forward(ctx, W, H)
    rgb = ctx.get_array(B.ARR_RGB)
    out, tro = _render_features(ctx, rgb, W, H)
    a, b = out.cpu().numpy(), img.cpu().numpy()
    assert np.abs(b).max() > 0.1 and tr.min().item() < 0.5                 # the frame shows something
    if bitwise:
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(tro.cpu().numpy().view(np.uint32), tr.cpu().numpy().view(np.uint32))
    else:
        assert np.all(np.abs(a - b) <= 1e-4 + 1e-4 * np.abs(b))
        assert np.all(np.abs(tro.cpu().numpy() - tr.cpu().numpy()) <= 1e-4 + 1e-4 * np.abs(tr.cpu().numpy()))
    out2, none = _render_features(ctx, rgb, W, H, want_trans=False)        # without trans_out: the same image
    assert none is None and torch.equal(out2, out)
    return img, tr


@pytest.mark.parametrize("t_min", [1e-5, 0.0])
@pytest.mark.parametrize("alpha_cull", [False, True])
def test_features_equal_to_the_colours_give_the_frames_image_bit_for_bit(t_min, alpha_cull):
    n, W, H, deg = 2000, 80, 56, 1                                         # 5 x 4 tiles, ragged on both edges
    sc, cam, T, P, ocam = _scene(n, W, H, deg, 82)
    ctx = _ctx(sc, cam, T, P, W, H, deg, t_min=t_min, alpha_cull=alpha_cull, tile_parts=1, slab_mode=0)
    _rgb_round_trip(ctx, W, H, bitwise=True)
    assert ctx.tile_parts_of_frame() == 1
    wc = ctx.work_counters_ex()
    if t_min > 0:
        assert wc["walked_fwd"] < ctx.num_instances                        # the early-out did stop tiles
    ctx.close()


@pytest.mark.parametrize("n,grow,dop", [(2000, 3.0, 4.0), (8000, 2.0, 0.0)])
def test_features_over_capped_and_extended_lists_bit_for_bit(n, grow, dop):
    """2000: the size the other walk tests use -- the one super-tile's list fits one segment of the two-level binning, so the minimum cap
    already covers every list.  8000, sparser: the cap ends inside the lists and most tiles walk past it, so the frame's forward appends
    segments and the feature walk runs over what it left."""
    from gaussiansplat_amd import backend as B
    W, H, deg = 80, 56, 1
    sc, cam, T, P, ocam = _scene(n, W, H, deg, 82, grow=grow, dop=dop)
    ctx = _ctx(sc, cam, T, P, W, H, deg, tile_parts=1, slab_mode=0, list_cap=2, debug_flags=B.GS_DEBUG_TINY_CAPS)
    ctx.set_view_slot(3)
    _bound_forward(ctx, W, H)                                              # the slot's first frame
    _rgb_round_trip(ctx, W, H, bitwise=True)                               # its second: capped lists, extended by the frame's forward
    st = ctx.list_stats()
    print("list stats", n, st, ctx.num_instances)
    assert st["capped"], st
    if n > 2000:
        assert st["extended_segments"] > 0, st
    ctx.close()


def test_features_with_tiles_shared_between_waves_within_the_pixel_bar():
    n, W, H, deg = 2000, 80, 56, 1
    sc, cam, T, P, ocam = _scene(n, W, H, deg, 82)
    ctx = _ctx(sc, cam, T, P, W, H, deg, tile_parts=0, slab_mode=0)
    _rgb_round_trip(ctx, W, H, bitwise=False)
    assert ctx.tile_parts_of_frame() == 4                                  # twenty tiles: four waves each
    ctx.close()


# ---------------------------------------------------------------- 3. forward parity for depth

def _depth_parity(oracle, n, W, H, deg, seed, frames, grow):
    from gaussiansplat_amd import backend as B, renderer as R
    O = oracle
    sc, cam, T, P, ocam = _scene(n, W, H, deg, seed, grow=grow, dop=4.0 if grow > 1 else 0.0)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), (gx, gy), sc, device=0, order=B.ORDER_DEPTH_DESC, slab_mode=0)
    for _ in range(frames):                                                # (the camera's id names the view slot: the same one every time)
        tps = R.preprocess(r, cam)
        R.compactIdxs(r, (16, 16), (gx, gy))
        R.forward(r, tps, (16, 16), (gx, gy))
    planes, depth = R.renderDepth(r, mode="expected")
    assert torch.equal(R.renderDepth(r), planes)                           # "accumulated": the planes alone
    torch.cuda.synchronize()
    pre = O.preprocess(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], deg, ocam, omp=True)
    ranges, ids, keys = O.bin_lists(pre["bbs"], pre["tps"], O.ORDER_DEPTH_DESC, 16, gx, gy)
    z = pre["ts"][:, 2]
    feat = np.stack([z, z * z, np.ones_like(z)], 1).astype(np.float32)
    pre_f = dict(pre); pre_f["rgb"] = np.ascontiguousarray(feat)
    want, want_tr = O.composite_forward(pre_f, ranges, ids, ocam, 16, gx, gy, t_min=1e-5, omp=True)
    got = planes.cpu().numpy()
    listed = np.unique(ids)
    assert len(listed) > n // 4 and want[2].max() > 0.5
    for c in range(3):
        s = max(1.0, float(np.abs(feat[listed, c]).max()))
        err = np.abs(got[c] - want[c])
        assert np.all(err <= s * 1e-4 + 1e-4 * np.abs(want[c])), (c, s, float(err.max()))
    tr = r.transmittance.cpu().numpy()
    assert np.all(np.abs(got[2] - (1.0 - tr)) <= 1e-4 + 1e-4 * np.abs(1.0 - tr))
    assert np.all(np.abs(got[2] - (1.0 - want_tr)) <= 1e-4 + 1e-4 * np.abs(1.0 - want_tr))
    d = depth.cpu().numpy()
    hit = got[2] > 1e-8
    assert np.array_equal(d[~hit], np.zeros_like(d[~hit])) and np.array_equal(d[hit], (got[0][hit] / got[2][hit]).astype(np.float32))
    assert d[hit].min() >= z[listed].min() * (1 - 1e-3) and d[hit].max() <= z[listed].max() * (1 + 1e-3)   # a weighted mean of the listed depths
    return r


def test_depth_planes_against_the_oracle(oracle):
    _depth_parity(oracle, 2000, 80, 56, 1, 82, frames=1, grow=3.0)


def test_depth_planes_against_the_oracle_on_a_grid_with_a_launch_order(oracle):
    r = _depth_parity(oracle, 20_000, 1296, 1040, 1, 83, frames=2, grow=0.5)   # 81 x 65 = 5265 tiles: above the wave slots
    assert r.ctx.tile_clock_rows() > 0                                     # the frame has a launch order


# ---------------------------------------------------------------- 4. gradient parity

def _reference_grads(oracle, sc, cam, T, P, ocam, W, H, deg, t_min, dF, feat=None):
    """fp64 autograd of sum F . dF, F the composite of a feature triple: `feat` [n, 3] constant, or None = (z, z^2, 1) with z from the means."""
    O = oracle
    ref = O.render(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], deg, ocam, order=1, t_min=t_min)
    params = [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in ("means", "scales", "quats", "opacities", "shs")]
    mux, muy, M, sig, rgb = torch_ref.per_gaussian(*params, deg, T, P, float(cam.fx), float(cam.fy), cam.eye, cam.lookAt, W, H)
    if feat is None:
        Tm = torch.as_tensor(np.asarray(T, np.float64).reshape(4, 4, order="F"))
        z = torch.cat([params[0], torch.ones(params[0].shape[0], 1, dtype=torch.float64)], 1) @ Tm.T[:, 2]
        f = torch.stack([z, z * z, torch.ones_like(z)], 1)
    else:
        f = torch.tensor(np.asarray(feat, np.float64), requires_grad=True)
    F, _ = torch_ref.composite(mux, muy, M, sig, f, float(np.float32(cam.near)), float(np.float32(cam.far)), W, H, ref["ranges"], ref["ids"],
                               ref["pre"]["bbs"], ref["pre"]["tps"][:, 2], t_min=t_min)
    (F * torch.tensor(dF, dtype=torch.float64)).sum().backward()
    g = {k: (p.grad.numpy() if p.grad is not None else np.zeros(p.shape)) for k, p in zip(GRADS, params)}
    if feat is not None:
        g["feat"] = f.grad.numpy()
    return g, F.detach().numpy()


@pytest.mark.parametrize("t_min", [1e-5, 0.0])
@pytest.mark.parametrize("det", [False, True])
def test_feature_gradients_against_fp64_autograd(oracle, det, t_min):
    n, W, H, deg = 300, 48, 40, 1
    sc, cam, T, P, ocam = _scene(n, W, H, deg, 84)
    rng = np.random.default_rng(84)
    feat = rng.uniform(-1.0, 2.0, (n, 3)).astype(np.float32)
    dF = rng.standard_normal((3, H, W)).astype(np.float32)
    want, F64 = _reference_grads(oracle, sc, cam, T, P, ocam, W, H, deg, t_min, dF, feat)
    ctx = _ctx(sc, cam, T, P, W, H, deg, t_min=t_min, deterministic=det, slab_mode=0)
    img, tr = _bound_forward(ctx, W, H)                                    # (kept: the frame's image lives in these two)
    f_d, dF_d = dev(feat), dev(dF)
    F, _ = _render_features(ctx, f_d, W, H)
    assert np.all(np.abs(F.cpu().numpy() - F64) <= 2e-4 + 1e-4 * np.abs(F64))       # |feat| <= 2
    runs = []
    for rep in range(2):
        gt = _grad_tensors(n, deg)
        gt[4].fill_(3.0)                                                   # d_shs is neither read nor written
        d_feat = torch.full((n, 3), 9.0, dtype=torch.float32, device="cuda")         # overwritten
        ctx.backward_features(f_d.data_ptr(), F.data_ptr(), dF_d.data_ptr(), d_feat.data_ptr(), _gs_grads(gt))
        torch.cuda.synchronize()
        runs.append([d_feat.cpu().numpy()] + [t.cpu().numpy() for t in gt])
    got = runs[0]
    assert np.all(got[5] == 3.0)
    print("rel-L2 d_feat", rel_l2(got[0].reshape(-1), want["feat"].reshape(-1)))
    assert rel_l2(got[0].reshape(-1), want["feat"].reshape(-1)) <= 1e-3
    for i, k in enumerate(GRADS[:4]):
        e = rel_l2(got[1 + i].reshape(-1), want[k].reshape(-1))
        print("rel-L2", k, e)
        assert np.linalg.norm(want[k]) > 0 and e <= 1e-3, (k, e)
    if det:
        for a, b in zip(runs[0], runs[1]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # with a NULL gradient set, or NULL arrays, d_feat is the same and nothing else is written
    d2 = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    ctx.backward_features(f_d.data_ptr(), F.data_ptr(), dF_d.data_ptr(), d2.data_ptr(), None)
    torch.cuda.synchronize()
    assert rel_l2(d2.cpu().numpy().reshape(-1), got[0].reshape(-1)) <= (0.0 if det else 1e-5)
    ctx.close()


@pytest.mark.parametrize("t_min", [1e-5, 0.0])
@pytest.mark.parametrize("det", [False, True])
def test_depth_gradients_against_fp64_autograd(oracle, det, t_min):
    from gaussiansplat_amd import backend as B, renderer as R
    n, W, H, deg = 300, 48, 40, 1
    sc, cam, T, P, ocam = _scene(n, W, H, deg, 84)
    rng = np.random.default_rng(85)
    dD = rng.standard_normal((3, H, W)).astype(np.float32)
    dD[1] *= np.float32(1.0 / 30.0)                                        # z ~ 30: the three planes weigh alike
    want, _ = _reference_grads(oracle, sc, cam, T, P, ocam, W, H, deg, t_min, dD, None)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), (gx, gy), sc, device=0, order=B.ORDER_DEPTH_DESC, t_min=t_min, deterministic=det,
                      slab_mode=0)
    runs = []
    for rep in range(2):
        tps = R.preprocess(r, cam)
        R.compactIdxs(r, (16, 16), (gx, gy))
        R.forward(r, tps, (16, 16), (gx, gy))
        R.resetGrads(r)
        R.renderDepth(r)
        R.backwardDepth(r, dD)
        torch.cuda.synchronize()
        g = r.splatGrads
        runs.append([t.cpu().numpy().copy() for t in (g.Δmeans, g.Δscales, g.Δquaternions, g.Δopacities, g.Δshs)])
    got = runs[0]
    assert not got[4].any()                                                # no SH gradient: the depth does not depend on the colours
    for i, k in enumerate(GRADS[:4]):
        e = rel_l2(got[i].reshape(-1), want[k].reshape(-1))
        print("rel-L2 depth", k, e)
        assert np.linalg.norm(want[k]) > 0 and e <= 1e-3, (k, e)
    if det:
        for a, b in zip(runs[0], runs[1]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------- 5. the frame is untouched

def _three_frames(sc, cam, T, P, W, H, deg, dC, mode, feat, dF):
    """Three frames of one view slot on a deterministic ctx; in the second, between forward and backward: mode "plain" nothing,
    "scratch" the feature calls with a gradient set of their own, "shared" the feature backward into the colour backward's set (after it)."""
    n = sc["means"].shape[0]
    ctx = _ctx(sc, cam, T, P, W, H, deg, deterministic=True, slab_mode=0)
    ctx.set_view_slot(2)
    dC_d, f_d, dF_d = dev(dC), dev(feat), dev(dF)
    out = {}
    for frame in range(3):
        img, tr = _bound_forward(ctx, W, H)
        gt = _grad_tensors(n, deg)
        if frame == 1 and mode != "plain":
            F, Ft = _render_features(ctx, f_d, W, H)
            sg = _grad_tensors(n, deg) if mode == "scratch" else None
            d_feat = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            if mode == "scratch":
                ctx.backward_features(f_d.data_ptr(), F.data_ptr(), dF_d.data_ptr(), d_feat.data_ptr(), _gs_grads(sg))
                out["feat_grads"] = sg
        if frame < 2:
            ctx.backward(dC_d.data_ptr(), _gs_grads(gt))
        if frame == 1 and mode == "shared":
            ctx.backward_features(f_d.data_ptr(), F.data_ptr(), dF_d.data_ptr(), d_feat.data_ptr(), _gs_grads(gt))
        torch.cuda.synchronize()
        out[frame] = dict(img=img.cpu().numpy(), tr=tr.cpu().numpy(), wc=ctx.work_counters_ex(), fill=ctx.tail_fill_blocks(),
                          parts=ctx.tile_parts_of_frame(), grads=[t.cpu().numpy() for t in gt])
    if "feat_grads" in out:
        out["feat_grads"] = [t.cpu().numpy() for t in out["feat_grads"]]
    ctx.close()
    return out


def test_the_frame_is_untouched_by_the_feature_calls():
    from gaussiansplat_amd import synthetic
    n, W, H, deg = 2000, 80, 56, 1
    sc, cam, T, P, ocam = _scene(n, W, H, deg, 86)
    rng = np.random.default_rng(86)
    dC = synthetic.make_dC(W, H, 86)
    feat = rng.uniform(0.0, 3.0, (n, 3)).astype(np.float32)
    dF = rng.standard_normal((3, H, W)).astype(np.float32)
    A = _three_frames(sc, cam, T, P, W, H, deg, dC, "scratch", feat, dF)
    Bp = _three_frames(sc, cam, T, P, W, H, deg, dC, "plain", feat, dF)
    for frame in (1, 2):                                                   # the frame with the feature calls, and the slot's next one
        a, b = A[frame], Bp[frame]
        assert np.array_equal(a["img"].view(np.uint32), b["img"].view(np.uint32)) and np.array_equal(a["tr"].view(np.uint32), b["tr"].view(np.uint32))
        assert a["wc"] == b["wc"] and a["fill"] == b["fill"] and a["parts"] == b["parts"], (a["wc"], b["wc"], a["fill"], b["fill"])
        for k, x, y in zip(GRADS, a["grads"], b["grads"]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (frame, k)
    assert Bp[1]["wc"]["walked_bwd"] > 0 and any(g.any() for g in Bp[1]["grads"])
    assert any(g.any() for g in A["feat_grads"][:4]) and not A["feat_grads"][4].any()
    # into the colour backward's own set: its gradients plus the feature's, up to the order of one float addition
    S = _three_frames(sc, cam, T, P, W, H, deg, dC, "shared", feat, dF)
    for i, k in enumerate(GRADS):
        want = Bp[1]["grads"][i].astype(np.float64) + A["feat_grads"][i].astype(np.float64)
        assert rel_l2(S[1]["grads"][i].reshape(-1), want.reshape(-1)) <= 1e-6, k
    assert np.array_equal(S[2]["img"].view(np.uint32), Bp[2]["img"].view(np.uint32))


# ---------------------------------------------------------------- 6. refusals

def test_refusals_leave_the_frame_as_it_was():
    from gaussiansplat_amd import backend as B, synthetic
    n, W, H, deg = 2000, 80, 56, 1                                         # (depth slabs need 1024 gaussians or more)
    sc, cam, T, P, ocam = _scene(n, W, H, deg, 87)
    dC = dev(synthetic.make_dC(W, H, 87))
    feat = dev(np.random.default_rng(87).uniform(0.0, 1.0, (n, 3)).astype(np.float32))
    out = torch.zeros((3, H, W), dtype=torch.float32, device="cuda"); tro = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    d_feat = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    fp, op, tp, dp = feat.data_ptr(), out.data_ptr(), tro.data_ptr(), d_feat.data_ptr()

    def frame(ctx, poke):
        img = torch.zeros((3, H, W), dtype=torch.float32, device="cuda"); tr = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        ctx.bind_outputs(img.data_ptr(), tr.data_ptr())
        ctx.preprocess(); ctx.bin()
        if poke:                                                           # a call before gs_forward
            refused(lambda: ctx.render_features(fp, op, tp), code=B.GS_ERR_INVALID)
            refused(lambda: ctx.backward_features(fp, op, dC.data_ptr(), dp, None), code=B.GS_ERR_INVALID)
        ctx.forward_device(img.data_ptr(), tr.data_ptr())
        if poke:
            ip, trp = img.data_ptr(), tr.data_ptr()
            for o, t in ((ip, tp), (op, trp), (ip + 4, tp), (trp, tp), (op, ip + 8 * W * H), (op, op + 4 * W * H), (op, op)):   # overlapping outputs
                refused(lambda: ctx.render_features(fp, o, t), code=B.GS_ERR_INVALID)
            refused(lambda: ctx.render_features(0, op, tp), code=B.GS_ERR_INVALID)                 # NULL pointers
            refused(lambda: ctx.render_features(fp, 0, tp), code=B.GS_ERR_INVALID)
            for args in ((0, op, dC.data_ptr(), dp), (fp, 0, dC.data_ptr(), dp), (fp, op, 0, dp), (fp, op, dC.data_ptr(), 0)):
                refused(lambda: ctx.backward_features(*args, None), code=B.GS_ERR_INVALID)
            refused(lambda: ctx.view_depth(0), code=B.GS_ERR_INVALID)
            refused(lambda: ctx.view_depth_backward(0, dp), code=B.GS_ERR_INVALID)
            refused(lambda: ctx.view_depth_backward(dp, 0), code=B.GS_ERR_INVALID)
        gt = _grad_tensors(n, deg)
        ctx.backward(dC.data_ptr(), _gs_grads(gt))
        torch.cuda.synchronize()
        return [img.cpu().numpy(), tr.cpu().numpy()] + [t.cpu().numpy() for t in gt]

    # (one wave per tile: what a slab frame runs as, so that the three frames below agree bit for bit)
    a = frame(_ctx(sc, cam, T, P, W, H, deg, deterministic=True, slab_mode=0, tile_parts=1), True)
    b = frame(_ctx(sc, cam, T, P, W, H, deg, deterministic=True, slab_mode=0, tile_parts=1), False)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert not out.any().item() and not tro.any().item() and not d_feat.any().item()               # nothing was enqueued

    # a frame binned in depth slabs
    slab = _ctx(sc, cam, T, P, W, H, deg, deterministic=True, slab_mode=1, slab_fractions=(0.3, 0.6), tile_parts=1)
    img, tr = _bound_forward(slab, W, H)
    assert slab.num_rounds > 1
    refused(lambda: slab.render_features(fp, op, tp), code=B.GS_ERR_UNSUPPORTED)
    refused(lambda: slab.backward_features(fp, op, dC.data_ptr(), dp, None), code=B.GS_ERR_UNSUPPORTED)
    gt = _grad_tensors(n, deg)
    slab.backward(dC.data_ptr(), _gs_grads(gt))
    torch.cuda.synchronize()
    for x, y in zip([img.cpu().numpy(), tr.cpu().numpy()] + [t.cpu().numpy() for t in gt], b):    # slab frames: bit-identical to classic ones
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert not out.any().item() and not d_feat.any().item()

    # the 2-D renderer
    s2 = synthetic.make_scene_2d(500, W, H, 88)
    c2 = on_torch_stream(B.Context(order=B.ORDER_INDEX, deterministic=True))
    c2.set_model_2d_host(s2["means"], s2["scales"], s2["rots"], s2["opacities"], s2["colors"])
    c2.set_image_size(W, H)

    def frame2d(poke):
        c2.preprocess(); c2.bin()
        i2, t2 = c2.forward_host()
        if poke:
            refused(lambda: c2.render_features(fp, op, tp), code=B.GS_ERR_UNSUPPORTED)
            refused(lambda: c2.backward_features(fp, op, dC.data_ptr(), dp, None), code=B.GS_ERR_UNSUPPORTED)
            refused(lambda: c2.view_depth(dp), code=B.GS_ERR_UNSUPPORTED)
            refused(lambda: c2.view_depth_backward(dp, dp), code=B.GS_ERR_UNSUPPORTED)
        g = c2.grads_alloc()
        c2.backward(dC.data_ptr(), g, overwrite=True)
        return [i2, t2] + list(c2.grads_read_2d(g).values())

    for x, y in zip(frame2d(True), frame2d(False)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert not out.any().item() and not d_feat.any().item()
