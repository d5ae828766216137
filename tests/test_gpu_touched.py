"""The touched-rows colour exchange on the device: gs_color_rows_pack (a view -> bitmap, compacted rows, count) and
gs_sh_grads_from_touched (gathered bitmaps + rows -> d_shs), and distributed.multi_view_step(sync="touched") on top of them.

Every expected value comes from the torch functions distributed.pack_touched_rows / unpack_touched_rows run on CPU copies of the
inputs and from the existing gs_sh_grads_from_views -- never from the new kernels.  All comparisons are bit for bit."""
import ctypes as C
import os
import re
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x7FC0DEAD                    # a NaN with a payload: no kernel produces it
W, H = 160, 112


def _chunk():
    from gaussiansplat_amd import backend as B
    src = open(os.path.join(ROOT, "gaussiansplat_amd", "csrc", "gs_chunk.h")).read()
    assert int(re.search(r"#define GS_CHUNK (\d+)", src).group(1)) == B.TOUCHED_CHUNK
    return B.TOUCHED_CHUNK


def _six_rows():
    """(-0,-0,-0) | (0,0,1e-45) | (nan,0,0) | (0,-1e-40,0) | (0,0,0) | (0,0,inf): rows 1, 2, 3, 5 are touched"""
    return np.array([[-0.0, -0.0, -0.0], [0, 0, 1e-45], [np.nan, 0, 0], [0, -1e-40, 0], [0, 0, 0], [0, 0, np.inf]], np.float32)


def _patterns(n, seed):
    rng = np.random.default_rng(seed)
    out = {}
    a = rng.standard_normal((n, 3)).astype(np.float32)
    a[rng.random(n) < 0.6] = 0
    u = a.view(np.uint32)
    for k, bits in enumerate((0xFFC12345, 0x7FA00001, 0x80000000, 0x00000001, 0xFF800000)):     # NaN payloads and signs, -0, a denormal, -inf
        u[(7 * k + 3) % n, k % 3] = bits
    out["random"] = a
    out["zero"] = np.zeros((n, 3), np.float32)
    out["all"] = (rng.standard_normal((n, 3)).astype(np.float32) + np.float32(4.0))
    for c in range(3):
        b = np.zeros((n, 3), np.float32)
        rows = rng.random(n) < 0.5
        rows[0] = True
        b[rows, c] = (rng.random(int(rows.sum())) + 0.5).astype(np.float32)
        out[f"one_component_{c}"] = b
    out["six"] = np.tile(_six_rows(), ((n + 5) // 6, 1))[:n].copy()
    return out


def _reference_pack(arr):
    """distributed.pack_touched_rows on the CPU: (bits [words] int32, count, rows [count, 3] as uint32)"""
    import torch
    from gaussiansplat_amd import distributed as D
    bits, counts, rows = D.pack_touched_rows(torch.from_numpy(arr)[None])
    return bits[0].numpy(), int(counts[0]), rows[0].numpy().view(np.uint32)


def test_reference_rule_on_the_six_rows():
    bits, count, _ = _reference_pack(_six_rows())
    assert bits.tolist() == [46] and count == 4


class _PackBuffers:
    def __init__(self, n):
        import torch
        self.n, self.words = n, (n + 31) // 32
        self.bits = torch.empty(max(self.words, 1), dtype=torch.int32, device="cuda")
        self.rows = torch.empty(3 * max(n, 1), dtype=torch.int32, device="cuda")
        self.count = torch.empty(1, dtype=torch.int64, device="cuda")

    def fill(self):
        import torch
        self.bits.fill_(-1); self.rows.fill_(SENTINEL); self.count.fill_(-7)
        torch.cuda.synchronize()

    def check(self, arr, what):
        import torch
        torch.cuda.synchronize()
        n = self.n
        want_bits, want_count, want_rows = _reference_pack(arr)
        got_bits = self.bits.cpu().numpy()[:self.words]
        got_rows = self.rows.cpu().numpy().view(np.uint32).reshape(-1, 3)
        assert int(self.count.cpu()[0]) == want_count, what
        assert np.array_equal(got_bits, want_bits), what
        assert np.array_equal(got_rows[:want_count], want_rows), what
        assert np.all(got_rows[want_count:] == SENTINEL), f"{what}: rows at and beyond count were written"
        if n % 32:
            assert int(got_bits.view(np.uint32)[-1]) >> (n % 32) == 0, f"{what}: padding bits of the last word"


def _pack_sizes():
    c = 256                               # backend.TOUCHED_CHUNK (checked in the test: collection must not need the package)
    return [1, 31, 32, 33, 63, 64, 65, c - 1, c, c + 1, 2 * c + 1, 70_001]


@pytest.mark.parametrize("n", _pack_sizes())
def test_pack_explicit_source_bit_for_bit(n):
    """every pattern into the SAME buffers, one after the other: each result is its own pattern's (no state left in the scratch)"""
    import torch
    from gaussiansplat_amd import backend as B
    assert _chunk() == 256
    ctx = B.Context()
    buf = _PackBuffers(n)
    for name, arr in _patterns(n, 1000 + n).items():
        src = torch.from_numpy(arr).cuda()
        assert np.array_equal(src.cpu().numpy().view(np.uint32), arr.view(np.uint32))        # the upload kept the bits
        buf.fill()
        ctx.color_rows_pack(src.data_ptr(), n, buf.bits.data_ptr(), buf.rows.data_ptr(), buf.count.data_ptr())
        ctx.synchronize()
        buf.check(arr, f"n={n} {name}")
    ctx.close()


@pytest.mark.parametrize("deterministic", [False, True])
def test_pack_from_the_ctx_equals_pack_of_the_dense_slot(deterministic):
    """gs_color_rows_pack(drgb = NULL) against gs_color_grads_pack into a slot + the torch pack of that slot: the new kernel's two
    sources (the ctx's float sums / its fixed-point sums) agree with the dense one"""
    import torch
    from common import hip_context, scene_and_cameras
    from gaussiansplat_amd import backend as B, synthetic
    n, deg = 3000, 3
    sc, cam, T, P, _ = scene_and_cameras(n, W, H, deg, 61)
    ctx = hip_context(sc, cam, T, P, W, H, deg, t_min=0.0, deterministic=deterministic)
    buf = _PackBuffers(n)
    buf.fill()
    ctx.preprocess(); ctx.bin(); ctx.forward_host()
    rc = ctx.L.gs_color_rows_pack(ctx.h, None, n, C.c_void_p(buf.bits.data_ptr()), C.c_void_p(buf.rows.data_ptr()), C.c_void_p(buf.count.data_ptr()))
    assert rc == B.GS_ERR_INVALID                                       # no backward yet
    g = ctx.grads_alloc()
    ctx.backward(synthetic.make_dC(W, H, 200), g)
    slot = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.color_grads_pack(slot.data_ptr())
    ctx.color_rows_pack(None, n, buf.bits.data_ptr(), buf.rows.data_ptr(), buf.count.data_ptr())
    ctx.synchronize()
    dense = slot.cpu().numpy()
    count = int(buf.count.cpu()[0])
    print(f"deterministic={deterministic}: {count} of {n} gaussians touched")
    assert 0 < count < n
    buf.check(dense, f"deterministic={deterministic}")
    with pytest.raises(B.GsError) as e:                                 # the ctx's own sums are n = gs_num_gaussians rows
        ctx.color_rows_pack(None, n - 1, buf.bits.data_ptr(), buf.rows.data_ptr(), buf.count.data_ptr())
    assert e.value.code == B.GS_ERR_INVALID
    ctx.close()


def _views(n, seed):
    """V = 3 dense views [3, n, 3]: random (60 % zero rows, special values), all zero, all touched"""
    p = _patterns(n, seed)
    dense = np.stack([p["random"], p["zero"], p["all"]])
    dense[0, 5 % n] = 0                   # the gaussian with the non-finite basis (below) keeps finite colour gradients everywhere
    return dense


def _padded(dense, cap_extra=7, cap=None):
    """torch pack on the CPU -> (bits [V, words] int32, rows [V, cap, 3] float32 padded with NaN, cap)"""
    import torch
    from gaussiansplat_amd import distributed as D
    bits, counts, rows = D.pack_touched_rows(torch.from_numpy(dense))
    cap = int(counts.max()) + cap_extra if cap is None else cap
    padded = torch.full((dense.shape[0], cap, 3), float("nan"), dtype=torch.float32)
    for v, r in enumerate(rows):
        k = min(r.shape[0], cap)
        padded[v, :k] = r[:k]
    # the round trip through unpack_touched_rows gives the dense views back: the reference pair is consistent
    if cap >= int(counts.max()):
        back = D.unpack_touched_rows(bits, counts, padded, dense.shape[1], torch.float32).numpy().view(np.uint32)
        touched = (dense.view(np.uint32) & 0x7FFFFFFF).any(axis=2)
        assert np.array_equal(back[touched], dense.view(np.uint32)[touched]) and not back[~touched].any()
    return bits, padded, cap


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [33, 3000])
def test_rebuild_bit_for_bit(n, deg):
    import torch
    from common import hip_context, scene_and_cameras
    from gaussiansplat_amd import distributed as D, synthetic
    sc, cam, T, P, _ = scene_and_cameras(n, W, H, deg, 77)
    sc["means"][5 % n, 0] = np.float32("nan")                           # no view direction: a non-finite basis times zero
    ctx = hip_context(sc, cam, T, P, W, H, deg)
    cams = D.view_records([synthetic.scene_camera(W, view=v) for v in range(3)], W, H)
    dense = _views(n, 31 * n + deg)
    bits, padded, cap = _padded(dense)
    k3 = 3 * (deg + 1) ** 2
    d_dense, d_bits, d_rows = torch.from_numpy(dense).cuda(), bits.cuda().contiguous(), padded.cuda().contiguous()
    stray = bits.clone()                                                # bits at positions >= n in the last word must change nothing
    assert 0 < n % 32 < 31
    stray[0, -1] |= -(1 << (n % 32))                                    # every bit from position n up
    stray[1, -1] |= -(1 << 31)                                          # the top bit, in the view that touches nothing
    assert not torch.equal(stray[0], bits[0]) and not torch.equal(stray[1], bits[1])
    d_stray = stray.cuda().contiguous()
    torch.cuda.synchronize()
    for overwrite in (True, False):
        want = torch.ones((n, k3), dtype=torch.float32, device="cuda")
        got = torch.ones((n, k3), dtype=torch.float32, device="cuda")
        got2 = torch.ones((n, k3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.sh_grads_from_views(cams, d_dense.data_ptr(), want.data_ptr(), overwrite=overwrite)
        ctx.sh_grads_from_touched(cams, d_bits.data_ptr(), d_rows.data_ptr(), cap, got.data_ptr(), overwrite=overwrite)
        ctx.sh_grads_from_touched(cams, d_stray.data_ptr(), d_rows.data_ptr(), cap, got2.data_ptr(), overwrite=overwrite)
        ctx.synchronize()
        w = want.cpu().numpy().view(np.uint32)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), w), f"overwrite={overwrite}"
        assert np.array_equal(got2.cpu().numpy().view(np.uint32), w), f"overwrite={overwrite}, stray bits beyond n"
        assert np.isfinite(want.cpu().numpy()).any() and (want.cpu().numpy() != 1.0).any()
        if deg >= 1:
            assert not np.isfinite(want.cpu().numpy()[5 % n, 3:]).any()   # the non-finite basis reached the dense result (and ours equals it)
    ctx.close()


def test_rebuild_reads_a_truncated_gather_as_zero_rows():
    """rows_cap below a view's count: the rows that did not travel read as zero rows, nothing is read outside the view's rows"""
    import torch
    from common import hip_context, scene_and_cameras
    from gaussiansplat_amd import distributed as D, synthetic
    n, deg = 3000, 2
    sc, cam, T, P, _ = scene_and_cameras(n, W, H, deg, 78)
    ctx = hip_context(sc, cam, T, P, W, H, deg)
    cams = D.view_records([synthetic.scene_camera(W, view=v) for v in range(3)], W, H)
    dense = _views(n, 5)
    cap = 700                                                           # view 0 has ~1200 touched rows, view 2 all 3000
    bits, padded, _ = _padded(dense, cap=cap)
    cut = dense.copy()
    for v in range(3):
        idx = np.nonzero((dense[v].view(np.uint32) & 0x7FFFFFFF).any(axis=1))[0]
        assert v == 1 or idx.size > cap
        cut[v, idx[cap:]] = 0
    want = torch.empty((n, 3 * (deg + 1) ** 2), dtype=torch.float32, device="cuda")
    got = torch.empty_like(want)
    d_cut, d_bits, d_rows = torch.from_numpy(cut).cuda(), bits.cuda().contiguous(), padded.cuda().contiguous()
    torch.cuda.synchronize()
    ctx.sh_grads_from_views(cams, d_cut.data_ptr(), want.data_ptr(), overwrite=True)
    ctx.sh_grads_from_touched(cams, d_bits.data_ptr(), d_rows.data_ptr(), cap, got.data_ptr(), overwrite=True)
    ctx.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    ctx.close()


def _scene_views(nviews):
    import torch
    from gaussiansplat_amd import synthetic
    n, deg = 3000, 3
    scene = synthetic.make_scene(n, W, H, deg, seed=61)
    cams = [synthetic.scene_camera(W, view=v) for v in range(nviews)]
    dCs = [synthetic.make_dC(W, H, 200 + v) for v in range(nviews)]
    dCs[1] = np.zeros_like(dCs[1])                                      # a view that touches nothing: count 0
    return n, scene, cams, [torch.as_tensor(d).cuda() for d in dCs]


def test_touched_step_equals_factored_on_one_gpu():
    import torch
    from gaussiansplat_amd import distributed as D, renderer as R
    n, scene, cams, dCs = _scene_views(3)
    flats, hvs = {}, {}
    for sync in ("factored", "touched"):
        r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, scene, t_min=0.0, deterministic=True)
        hvs[sync] = D.HipViewRenderer(r)
        flats[sync] = D.multi_view_step(hvs[sync], cams, dCs, sync=sync).clone()
        torch.cuda.synchronize()
    a, b = flats["factored"].cpu().numpy(), flats["touched"].cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.abs(a[11 * n:]).max() > 0 and np.abs(a[:11 * n]).max() > 0
    hv = hvs["touched"]
    assert hv.device_touched_packs == 3 and hv.device_touched_rebuilds == 1          # the device path, not the torch functions
    assert not hasattr(hvs["factored"], "device_touched_packs")
    assert hv.touched_buffers(3)[2].cpu().tolist()[1] == 0                           # the view with dC = 0
    assert all(0 < c < n for c in hv.touched_buffers(3)[2].cpu().tolist()[::2])


class _HostStagedGather:
    """torch.distributed.all_gather_into_tensor for a gloo build that refuses device tensors: the collective runs on host copies"""
    def __init__(self, native):
        self.native = native

    def __call__(self, out, inp, group=None, async_op=False):
        import torch
        if not inp.is_cuda:
            return self.native(out, inp, group=group, async_op=async_op)
        torch.cuda.synchronize()
        h_out = torch.empty(out.shape, dtype=out.dtype)
        self.native(h_out, inp.cpu(), group=group)
        out.copy_(h_out)

        class _Done:
            def wait(self): pass
        return _Done()


def _worker(rank, world, port, nviews, out):
    import torch
    import torch.distributed as dist
    from gaussiansplat_amd import distributed as D, renderer as R
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    native = dist.all_gather_into_tensor
    try:
        try:                                                            # does this build's gloo gather device tensors?  (both ranks find the same answer)
            probe = torch.zeros(world, dtype=torch.int64, device="cuda")
            native(probe, torch.full((1,), rank + 1, dtype=torch.int64, device="cuda"))
            torch.cuda.synchronize()
            assert probe.cpu().tolist() == [1, 2]
        except (RuntimeError, NotImplementedError):
            dist.all_gather_into_tensor = _HostStagedGather(native)     # this worker process only
        n, scene, cams, dCs = _scene_views(nviews)
        flats, hvs = {}, {}
        for sync in ("factored", "touched"):
            r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, scene, t_min=0.0, deterministic=True, tile_parts=1)
            hvs[sync] = D.HipViewRenderer(r)
            for _ in range(2):                                          # two steps: the second runs on view-slot history and reused buffers
                flat = D.multi_view_step(hvs[sync], cams, dCs, sync=sync)
            torch.cuda.synchronize()
            flats[sync] = flat.cpu().clone()
        assert torch.equal(flats["factored"].view(torch.int32), flats["touched"].view(torch.int32))
        assert hvs["touched"].device_touched_packs == 2 * (nviews // world) and hvs["touched"].device_touched_rebuilds == 2
        both = [torch.zeros_like(flats["touched"]) for _ in range(world)]
        dist.all_gather(both, flats["touched"])
        assert all(torch.equal(both[0].view(torch.int32), b.view(torch.int32)) for b in both)      # identical on every rank
        if rank == 0:
            np.save(out, flats["touched"].numpy())
    finally:
        dist.all_gather_into_tensor = native
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_touched_equals_factored_bitwise(tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "flat_touched.npy")
    mp.spawn(_worker, args=(2, port, 4, out), nprocs=2, join=True)
    got = np.load(out)
    assert got.shape == (59 * 3000,) and np.abs(got[11 * 3000:]).max() > 0 and np.abs(got[:11 * 3000]).max() > 0


def test_argument_errors_leave_the_outputs_alone():
    import torch
    from common import hip_context, scene_and_cameras
    from gaussiansplat_amd import backend as B, distributed as D, synthetic
    n, deg = 33, 1
    sc, cam, T, P, _ = scene_and_cameras(n, W, H, deg, 9)
    ctx = hip_context(sc, cam, T, P, W, H, deg)
    L, vp = ctx.L, C.c_void_p
    buf = _PackBuffers(n)
    buf.fill()
    src = torch.ones((n, 3), dtype=torch.float32, device="cuda")
    d_shs = torch.full((n, 12), SENTINEL, dtype=torch.int32, device="cuda")
    bits = torch.full((2, 2), -1, dtype=torch.int32, device="cuda")
    rows = torch.ones((2, 40, 3), dtype=torch.float32, device="cuda")
    cams = np.ascontiguousarray(D.view_records([synthetic.scene_camera(W, view=v) for v in range(2)], W, H), np.float32)
    torch.cuda.synchronize()
    s, b, r, c = (vp(t.data_ptr()) for t in (src, buf.bits, buf.rows, buf.count))
    pack_cases = {"ctx": (None, s, n, b, r, c), "bits": (ctx.h, s, n, None, r, c), "rows": (ctx.h, s, n, b, None, c),
                  "count": (ctx.h, s, n, b, r, None), "n < 0": (ctx.h, s, -1, b, r, c)}
    for what, args in pack_cases.items():
        assert L.gs_color_rows_pack(*args) == B.GS_ERR_INVALID, what
    cm, bi, ro, ds = vp(cams.ctypes.data), vp(bits.data_ptr()), vp(rows.data_ptr()), vp(d_shs.data_ptr())
    rebuild_cases = {"ctx": (None, 2, cm, bi, ro, 40, ds, 1), "cams": (ctx.h, 2, None, bi, ro, 40, ds, 1), "bits": (ctx.h, 2, cm, None, ro, 40, ds, 1),
                     "rows": (ctx.h, 2, cm, bi, None, 40, ds, 1), "d_shs": (ctx.h, 2, cm, bi, ro, 40, None, 1),
                     "nviews 0": (ctx.h, 0, cm, bi, ro, 40, ds, 1), "nviews < 0": (ctx.h, -1, cm, bi, ro, 40, ds, 1),
                     "rows_cap 0": (ctx.h, 2, cm, bi, ro, 0, ds, 1), "rows_cap < 0": (ctx.h, 2, cm, bi, ro, -3, ds, 1)}
    for what, args in rebuild_cases.items():
        assert L.gs_sh_grads_from_touched(*args) == B.GS_ERR_INVALID, what
    # a 2-D ctx: both are 3-D-renderer only
    sc2 = synthetic.make_scene_2d(50, 64, 64, 3, scale_hi=2.0)
    ctx2 = B.Context(order=B.ORDER_INDEX)
    ctx2.set_model_2d_host(sc2["means"], sc2["scales"], sc2["rots"], sc2["opacities"], sc2["colors"])
    ctx2.set_image_size(64, 64)
    assert L.gs_color_rows_pack(ctx2.h, s, n, b, r, c) == B.GS_ERR_UNSUPPORTED
    assert L.gs_sh_grads_from_touched(ctx2.h, 2, cm, bi, ro, 40, ds, 1) == B.GS_ERR_UNSUPPORTED
    ctx.synchronize(); ctx2.synchronize(); torch.cuda.synchronize()
    assert np.all(buf.bits.cpu().numpy() == -1) and np.all(buf.rows.cpu().numpy() == SENTINEL) and int(buf.count.cpu()[0]) == -7
    assert np.all(d_shs.cpu().numpy() == SENTINEL)
    # n == 0: GS_OK, count 0, nothing else written
    assert L.gs_color_rows_pack(ctx.h, s, 0, b, r, c) == 0
    ctx.synchronize()
    assert int(buf.count.cpu()[0]) == 0 and np.all(buf.bits.cpu().numpy() == -1) and np.all(buf.rows.cpu().numpy() == SENTINEL)
    ctx.close(); ctx2.close()
