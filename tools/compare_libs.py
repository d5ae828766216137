#!/usr/bin/env python3
"""Bit-for-bit comparison of two builds of libgsplat_hip.so (a refactor against its parent, tools/build_old_lib.sh).  GPU box.

  tools/compare_libs.py run LIB_A LIB_B [LOG]   one fresh process per library (each under its own timeout), then the table; appends to LOG
  tools/compare_libs.py record OUT.npz          every case below with the library GSPLAT_HIP_LIB names -> OUT.npz
  tools/compare_libs.py compare A.npz B.npz     the table alone; exit status 1 if an array differs
  tools/compare_libs.py frames                  three frames each of C1, C3 and a forced-slab bin_path 2 frame (to run under rocprofv3 --kernel-trace)
  tools/compare_libs.py kernels DIR             digest of the ordered kernel names of the kernel trace (csv) below DIR

Fixed seeds; every ctx whose gradients are recorded is deterministic (fixed-point gradient sums), and the two cases with float atomics
record no gradients (C1_small_float_atomics; tile_clock: counts only), so every array must be EQUAL.  Arrays above 4096 elements are kept as a
blake2b digest of their bytes.  A call the library refuses is recorded with its message: the refusal must be alike on both sides.
History (case_history): what frames inherit under a view slot, across slots, grids, an abandoned frame and without slots, small and at C3 scale.
Per frame: image, T, the five gradient arrays, tile ranges, sorted ids, sortIdxs, num_instances / _coarse_instances / _rounds,
bin_path_of_frame, list_stats, work_counters_ex; and the counting words of the composite kernels' debug record on one small frame.
The per-gaussian kernels beyond a frame: a density cycle (statistics, actions, plan, the restructured model and one moment set), the five
MCMC calls (plan at n = 1000 and at 1025 chunks, draws, a relocation from the plan and one onto an explicit dst at degree 3, noise, regularisers), the
touched-rows pack of two views and the SH gradients rebuilt from them, one fused backward + Adam step dense and selective (parameters
and moments), a frame at active SH degree 1 of a stored degree 3, and the backward's forms at n = 300 (two workgroups, the second's last wave partly past n):
stored = active degree 0 .. 3 and active 0 of stored 3, each over two views on one set of gradient buffers (overwriting, then accumulating),
both phases in one call and the phases apart.
The stages around a frame whose reductions run through csrc/gs_wave.h, each at the smallest shape that reaches every path: the loss and
the metrics on a 67 x 35 x 3 pair (two tile columns, three tile rows, ragged both ways: more tiles than XCDs, some XCD chunks short), the
camera gradient of a 64 x 48 frame at degree 1 at n = 300 and n = 257 (two partial rows; the second workgroup's last wave partly past n /
one thread) and at degrees 0, 2, 3 at n = 300, the exposure backward at 129 x 33 (five partial rows, scalar tail, 4-byte accesses) and 64 x 16 (one row, 16-byte accesses),
with and without a weight.  The loss VALUE alone is no bit-for-bit quantity (double atomics over 64 slots: its last bits depend on the
dispatch order): its key ends in REL_KEY and is compared to a relative 2^-40."""
import csv, glob, hashlib, os, subprocess, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


REL_KEY, REL = "~rel_2^-40", 2.0 ** -40


def same(k, x, y):
    if k.endswith(REL_KEY):
        return x.shape == y.shape and bool(np.all(np.abs(x - y) <= REL * np.maximum(np.abs(x), np.abs(y))))
    return np.array_equal(x, y)


def keep(a):
    a = np.ascontiguousarray(a)
    if a.size <= 4096:
        return a
    return np.frombuffer(hashlib.blake2b(a.tobytes() + str((a.shape, a.dtype)).encode(), digest_size=16).digest(), np.uint8)


class Recorder:
    def __init__(self):
        self.out = {}

    def put(self, key, value):
        assert key not in self.out, key
        self.out[key] = keep(np.asarray(value))

    def call(self, key, fn):
        """fn() -> array-like or dict of them; a refusal is recorded as its message"""
        try:
            v = fn()
        except Exception as e:                                   # GsError: must be alike on both sides
            self.put(key + "!refused", np.frombuffer(("%s: %s" % (type(e).__name__, e)).encode(), np.uint8))
            return None
        if isinstance(v, dict):
            for k, x in v.items():
                self.put(key + "." + k, x)
        else:
            self.put(key, v)
        return v


def set_cam(ctx, W, H, view):
    from gaussiansplat_amd import camera as gcam, synthetic
    cam = synthetic.scene_camera(W, view=view)
    ctx.set_camera(gcam.compute_transform(cam), gcam.compute_projection(cam, W, H), float(cam.fx), float(cam.fy), float(cam.near), float(cam.far),
                   cam.eye, cam.lookAt, W, H)


def frame(R, tag, ctx, dC, g, read_grads, sort_before=False, ids_between=False):
    """preprocess .. backward as a caller runs them (nothing asked in between unless the case says so), then everything the frame left"""
    from gaussiansplat_amd import backend as B
    ctx.preprocess(); ctx.bin()
    if sort_before:
        R.call(tag + "/sortIdxs_before_forward", lambda: ctx.get_array(B.ARR_SORT_IDXS))
    img, tr = ctx.forward_host()
    R.put(tag + "/image", img); R.put(tag + "/T", tr)
    if ids_between:
        R.call(tag + "/sorted_ids_between", lambda: ctx.get_array(B.ARR_SORTED_IDS))
    ctx.backward(dC, g, overwrite=True)
    R.call(tag + "/grads", lambda: read_grads(g))
    R.put(tag + "/num_instances", ctx.num_instances); R.put(tag + "/num_coarse_instances", ctx.num_coarse_instances)
    R.put(tag + "/num_rounds", ctx.num_rounds); R.put(tag + "/bin_path", ctx.bin_path_of_frame())
    R.call(tag + "/list_stats", lambda: {k: int(v) for k, v in ctx.list_stats().items()})
    R.call(tag + "/work_counters_ex", ctx.work_counters_ex)
    R.call(tag + "/tile_ranges", lambda: ctx.get_array(B.ARR_TILE_RANGES))
    R.call(tag + "/sorted_ids", lambda: ctx.get_array(B.ARR_SORTED_IDS))
    R.call(tag + "/sortIdxs", lambda: ctx.get_array(B.ARR_SORT_IDXS))


_scenes = {}


def scene(cfg, n=None):
    from gaussiansplat_amd import synthetic
    n0, W, H, deg = synthetic.CONFIGS[cfg]
    n = n0 if n is None else n
    if (cfg, n) not in _scenes:
        _scenes[(cfg, n)] = synthetic.make_scene(n, W, H, deg, seed=1234 + ["C1", "C2", "C3"].index(cfg))
    return _scenes[(cfg, n)], n, W, H, deg


def synthetic_config(cfg):
    from gaussiansplat_amd import synthetic
    return synthetic.CONFIGS[cfg]


def set_model(ctx, sc, n, deg):
    ctx.set_model_host(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"].reshape(n, -1), deg)


def case_3d(R, name, cfg, frames=4, n=None, sort_before=False, ids_between=False, deterministic=True, **kw):
    """First frame of a ctx (nothing to launch against: no speculation), then frames - 1 more on the same view slot (speculative on the two-level path)"""
    from gaussiansplat_amd import backend as B, synthetic
    sc, n, W, H, deg = scene(cfg, n)
    ctx = B.Context(deterministic=deterministic, **kw)
    set_model(ctx, sc, n, deg)
    dC = synthetic.make_dC(W, H, 1)
    g = ctx.grads_alloc()
    read = (lambda gg: ctx.grads_read(gg, deg)) if deterministic else (lambda gg: {})
    for k in range(frames):
        ctx.set_view_slot(0)
        set_cam(ctx, W, H, 0)
        frame(R, "%s/f%d" % (name, k), ctx, dC, g, read, sort_before=sort_before and k % 2 == 0, ids_between=ids_between)
    ctx.close()


def case_grow(R):
    """The model grows between frames: the second frame's speculative lists outgrow the first frame's buffers and settle_totals lists again"""
    from gaussiansplat_amd import backend as B, synthetic
    big, n2, W, H, deg = scene("C2")
    n1 = 20000
    small = {k: v[:n1] for k, v in big.items()}
    ctx = B.Context(deterministic=True)
    dC = synthetic.make_dC(W, H, 1)
    inst = []
    for k, (sc, n) in enumerate(((small, n1), (big, n2), (big, n2))):
        set_model(ctx, sc, n, deg)
        g = ctx.grads_alloc()
        ctx.set_view_slot(0)
        set_cam(ctx, W, H, 0)
        frame(R, "grow/f%d" % k, ctx, dC, g, lambda gg: ctx.grads_read(gg, deg))
        inst.append(ctx.num_instances)
    # The capacity, in entries, the first frame left for the second frame's speculative launch.  The ABI does not report a buffer's capacity, so
    # this RECOMPUTES it from DevBuf::ensure's growth rule (bytes + bytes / 8 + 256), and for the ids buffer alone (cids / clr may overflow as
    # well; one is enough).  If that rule changes, change this line with it: otherwise the assert no longer proves that the lists were written twice.
    cap = inst[0] + inst[0] // 8 + 64
    assert inst[1] > cap, ("the second frame did not outgrow the first frame's ids buffer", inst, cap)
    R.put("grow/first_frame_capacity", cap)
    ctx.close()


def case_history(R, name, n, W, H, deg, seed, grow=0.0, **kw):
    """What frames inherit (gs_ctx.h, HISTORY): the sequences of tests/test_gpu_history.py, three frames per step, one after another on ONE ctx --
    same slot; slot A, slot B, slot A; the grid transposed and back; gs_set_view_slot between gs_bin and gs_forward; a frame abandoned after gs_bin
    -- then three slot-less frames under schedule 3 and under schedule 4, each on a ctx of its own.  Deterministic; under the default tile_parts the
    gradient bits depend on the history a frame ran on, so equal arrays say that both libraries read the same history."""
    from gaussiansplat_amd import backend as B, synthetic
    sc = synthetic.make_scene(n, W, H, deg, seed=seed)
    sc["scales"] = (sc["scales"] + np.float32(grow)).astype(np.float32)
    dC = {(W, H): synthetic.make_dC(W, H, 1), (H, W): synthetic.make_dC(H, W, 1)}

    def step(ctx, g, tag, slot, view=0, w=W, h=H, frames=3, between=None):
        for k in range(frames):
            ctx.set_view_slot(slot)
            set_cam(ctx, w, h, view)
            ctx.preprocess(); ctx.bin()
            if between is not None:
                ctx.set_view_slot(between)
            img, tr = ctx.forward_host()
            ctx.backward(dC[(w, h)], g, overwrite=True)
            t = "%s/%s_f%d" % (name, tag, k)
            R.put(t + "/image", img); R.put(t + "/T", tr)
            R.call(t + "/grads", lambda: ctx.grads_read(g, deg))
            R.call(t + "/stats", lambda: dict({k: int(v) for k, v in ctx.list_stats().items()}, num_instances=ctx.num_instances, num_rounds=ctx.num_rounds,
                                              tile_parts=ctx.tile_parts_of_frame(), tile_clock_rows=ctx.tile_clock_rows(), **ctx.work_counters_ex()))

    ctx = B.Context(deterministic=True, **kw)
    set_model(ctx, sc, n, deg)
    g = ctx.grads_alloc()
    step(ctx, g, "same_slot", 0)
    step(ctx, g, "slot_b", 1, view=4); step(ctx, g, "slot_a_again", 0)
    step(ctx, g, "transposed", 0, w=H, h=W); step(ctx, g, "grid_back", 0)
    step(ctx, g, "slot_changed_after_bin", 0, frames=1, between=2); step(ctx, g, "second_slot", 2)
    ctx.set_view_slot(0); set_cam(ctx, W, H, 0); ctx.preprocess(); ctx.bin()          # abandoned: binned, never rendered
    step(ctx, g, "after_abandoned", 0)
    ctx.close()
    for schedule in (3, 4):
        ctx = B.Context(deterministic=True, **dict(kw, schedule=schedule))
        set_model(ctx, sc, n, deg)
        step(ctx, ctx.grads_alloc(), "slotless_schedule_%d" % schedule, -1)
        ctx.close()


def case_2d(R):
    from gaussiansplat_amd import backend as B, synthetic
    n, W, H = 3000, 256, 256
    sc = synthetic.make_scene_2d(n, W, H, 5, scale_hi=2.5)
    dC = synthetic.make_dC(W, H, 5)
    for bp in (0, 3, 2):
        ctx = B.Context(order=B.ORDER_INDEX, deterministic=True, bin_path=bp)
        ctx.set_model_2d_host(sc["means"], sc["scales"], sc["rots"], sc["opacities"], sc["colors"])
        ctx.set_image_size(W, H)
        g = ctx.grads_alloc()
        for k in range(2):
            frame(R, "2d_bin_path_%d/f%d" % (bp, k), ctx, dC, g, ctx.grads_read_2d)
        ctx.close()


def case_empty(R):
    """n = 0: accepted or refused, alike on both sides"""
    from gaussiansplat_amd import backend as B, synthetic
    W = H = 256

    def run():
        ctx = B.Context(deterministic=True)
        z = lambda *s: np.zeros(s, np.float32)
        ctx.set_model_host(z(0, 3), z(0, 3), z(0, 4), z(0), z(0, 3), 0)
        set_cam(ctx, W, H, 0)
        out = {}
        for k in range(2):
            ctx.preprocess(); ctx.bin()
            img, tr = ctx.forward_host()
            out.update({"f%d.image" % k: img, "f%d.T" % k: tr, "f%d.num_instances" % k: ctx.num_instances, "f%d.bin_path" % k: ctx.bin_path_of_frame(),
                        "f%d.tile_ranges" % k: ctx.get_array(B.ARR_TILE_RANGES)})
        ctx.close()
        return out
    R.call("empty", run)


def case_tile_clock(R):
    """The run-to-run stable words of the debug record (GsCompositeArgs.tile_clock): counts, not clocks.  One small frame, one wave per tile,
    float atomics (the backward's clock kernels have no fixed-point form); records by tile in tile order (10) and in the frame's launch order (30)"""
    from gaussiansplat_amd import backend as B, synthetic
    sc, n, W, H, deg = scene("C1")
    ctx = B.Context(deterministic=False, tile_parts=1, slab_mode=0)
    set_model(ctx, sc, n, deg)
    set_cam(ctx, W, H, 0)
    ctx.preprocess(); ctx.bin()
    ctx.forward_host()
    ctx.backward(synthetic.make_dC(W, H, 1), ctx.grads_alloc(), overwrite=True)
    for v in (10, 30):                                                  # (put, not call: a refusal here ends the record, it is not a result)
        fwd, bwd = ctx.tile_clock(0, v), ctx.tile_clock(1, v)
        assert (fwd[:, 3] & np.uint64(0xFFFFFFFF)).sum() > 0 and np.array_equal(fwd[:, 3], bwd[:, 3]), "tile_clock: an empty record"
        R.put("tile_clock/fwd_variant_%d_words_3_6to14" % v, fwd[:, [3] + list(range(6, 15))])
        R.put("tile_clock/bwd_variant_%d_words_3_6_7" % v, bwd[:, [3, 6, 7]])
    ctx.close()


def small_scene(n, deg, seed):
    """n gaussians of SH degree `deg` on a C1-sized image, the model in caller-owned device arrays (so that a step or a restructure can be read back)"""
    import torch
    from gaussiansplat_amd import synthetic
    W = H = 256
    sc = synthetic.make_scene(n, W, H, deg, seed=seed)
    model = [torch.as_tensor(np.ascontiguousarray(sc[k], np.float32).reshape(n, -1)).cuda() for k in ("means", "scales", "quats", "opacities", "shs")]
    return model, W, H


def device_ctx(model, n, deg, W, H, view=0, **kw):
    from gaussiansplat_amd import backend as B
    ctx = B.Context(deterministic=True, **kw)
    ctx.set_model_device(n, deg, [t.data_ptr() for t in model])
    set_cam(ctx, W, H, view)
    return ctx


def host(ts):
    import torch
    torch.cuda.synchronize()
    return {("means", "scales", "quats", "opacities", "shs")[i]: t.cpu().numpy() for i, t in enumerate(ts)}


def case_density(R):
    """One density cycle at n = 1000: accumulate, decide, plan, restructure with clones and splits, one moment set"""
    import torch
    from gaussiansplat_amd import backend as B, synthetic
    from gaussiansplat_amd.density import density_params
    n, deg = 1000, 1
    model, W, H = small_scene(n, deg, 501)
    ctx = device_ctx(model, n, deg, W, H)
    ctx.preprocess(); ctx.bin(); ctx.forward_host()
    ctx.backward(synthetic.make_dC(W, H, 502), ctx.grads_alloc(), overwrite=True)
    gs, cnt, ext = torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    st = B.GsDensityStats(gs.data_ptr(), cnt.data_ptr(), ext.data_ptr())
    ctx.density_accumulate(st)
    action = torch.zeros(n, dtype=torch.int32, device="cuda")
    gsum = np.sort(gs.cpu().numpy())
    # thresholds from the recorded statistics themselves: the upper half densifies, and the median scale parts clones from splits
    smax = float(np.median(model[1].cpu().numpy().max(axis=1)))
    par = density_params(scene_extent=float(np.exp(smax)) / 0.01, grad_threshold=float(gsum[n // 2]), percent_dense=0.01, min_opacity=0.2,
                         max_world_fraction=None)
    ctx.density_decide(st, par, action.data_ptr())
    plan = ctx.density_plan(action.data_ptr())
    assert plan[1] > 0 and plan[2] > 0 and plan[3] > 0, ("density: the cycle needs clones, splits and pruned rows", plan)
    no = plan[0] + plan[1] + 2 * plan[2]
    g = torch.Generator("cuda").manual_seed(503)
    noise = torch.randn((n, 2, 3), device="cuda", generator=g)
    moments = [torch.randn(t.shape, device="cuda", generator=g) for t in model]
    dst = [torch.full((no, t.shape[1]), 7.0, device="cuda") for t in model]
    dst_m = [torch.full((no, t.shape[1]), 7.0, device="cuda") for t in model]
    G = lambda ts: B.GsGrads(*[t.data_ptr() for t in ts])
    ctx.density_restructure(action.data_ptr(), noise.data_ptr(), G(dst), [G(moments)], [G(dst_m)], no)
    ctx.synchronize()
    R.put("density/grad_sum", gs.cpu().numpy()); R.put("density/count", cnt.cpu().numpy()); R.put("density/max_extent", ext.cpu().numpy())
    R.put("density/action", action.cpu().numpy()); R.put("density/plan", plan)
    for k, v in host(dst).items():
        R.put("density/model." + k, v)
    for k, v in host(dst_m).items():
        R.put("density/moments." + k, v)
    ctx.close()


def case_mcmc(R):
    """The five MCMC calls.  Plan at n = 1000 (four chunks) and n = 262145 (1025 chunks: two words per scan thread, half of the threads with an empty
    span), a tenth of the opacities dead; 500 draws; a relocation from the plan with one moment set; one onto an explicit dst at SH degree 3 (16-byte
    rows); noise and the regularisers at n = 300"""
    import torch
    from gaussiansplat_amd import backend as B
    from gaussiansplat_amd.density import logit
    G = lambda ts: B.GsGrads(*[t.data_ptr() for t in ts])
    min_opacity = 0.005

    def planned(n, deg, seed):
        model, W, H = small_scene(n, deg, seed)
        g = torch.Generator("cuda").manual_seed(seed + 1)
        model[3][torch.randperm(n, device="cuda", generator=g)[:max(n // 10, 1)]] = -8.0
        ctx = device_ctx(model, n, deg, W, H)
        cdf, dead = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda")
        counts = ctx.mcmc_plan(logit(min_opacity), cdf.data_ptr(), dead.data_ptr())
        assert counts[1] == max(n // 10, 1) and counts[0] + counts[1] == n and counts[2] > 0, ("mcmc: the plan needs dead and live gaussians", counts)
        return model, ctx, g, cdf, dead, counts

    def draw(ctx, g, cdf, n, m):
        u = torch.rand(m, device="cuda", generator=g)
        src = torch.full((m,), -1, dtype=torch.int32, device="cuda")
        ctx.mcmc_sample(cdf.data_ptr(), n, u.data_ptr(), m, src.data_ptr())
        return src

    def put_model(tag, ctx, model, moments):
        ctx.synchronize()
        for k, v in host(model).items():
            R.put(tag + "/model." + k, v)
        for k, v in host(moments).items():
            R.put(tag + "/moments." + k, v)

    for n in (1000, 262145):
        model, ctx, g, cdf, dead, counts = planned(n, 1, 581)
        ctx.synchronize()
        tag = "mcmc_n%d" % n
        R.put(tag + "/counts", counts); R.put(tag + "/cdf", cdf.cpu().numpy()); R.put(tag + "/dead", dead.cpu().numpy()[:counts[1]])
        if n == 1000:
            src = draw(ctx, g, cdf, n, 500)
            ctx.synchronize()
            R.put(tag + "/sample_500", src.cpu().numpy())
            src = draw(ctx, g, cdf, n, counts[1])
            moments = [torch.randn(t.shape, device="cuda", generator=g) for t in model]
            ctx.mcmc_relocate(src.data_ptr(), None, counts[1], min_opacity, [G(moments)])
            R.put(tag + "/relocate_src", src.cpu().numpy())
            put_model(tag + "/relocate", ctx, model, moments)
        ctx.close()
    # an explicit dst at degree 3: the last 50 rows take copies of sources drawn from the plan (dead rows among them: a draw never names one)
    n = 1000
    model, ctx, g, cdf, dead, counts = planned(n, 3, 583)
    src = draw(ctx, g, cdf, n, 50)
    dst = torch.arange(n - 50, n, dtype=torch.int32, device="cuda")
    keep_rows = ~torch.isin(src.long(), dst.long())              # destinations are no sources by contract: such a draw becomes a no-op (-1)
    src = torch.where(keep_rows, src, torch.full_like(src, -1))
    moments = [torch.randn(t.shape, device="cuda", generator=g) for t in model]
    ctx.mcmc_relocate(src.data_ptr(), dst.data_ptr(), 50, min_opacity, [G(moments)])
    R.put("mcmc_dst_degree_3/src", src.cpu().numpy())
    put_model("mcmc_dst_degree_3", ctx, model, moments)
    ctx.close()
    n = 300
    model, W, H = small_scene(n, 1, 585)
    ctx = device_ctx(model, n, 1, W, H)
    g = torch.Generator("cuda").manual_seed(586)
    z = torch.randn((n, 3), device="cuda", generator=g)
    model[3][:60] = -8.0                                         # the gate opens for transparent gaussians only
    before = model[0].clone()
    ctx.mcmc_noise(z.data_ptr(), 80.0, 100.0, 0.005)
    grads = [torch.randn(t.shape, device="cuda", generator=g) for t in model]
    ctx.mcmc_regularize(G(grads), 0.01 / n, 0.01 / (3 * n))
    ctx.synchronize()
    assert not torch.equal(before, model[0]), "mcmc: the noise moved nothing"
    R.put("mcmc_noise_n300/means", model[0].cpu().numpy())
    R.put("mcmc_regularize_n300/d_scales", grads[1].cpu().numpy()); R.put("mcmc_regularize_n300/d_opacities", grads[3].cpu().numpy())
    ctx.close()


def case_touched(R):
    """color_rows_pack of two views' own gradient sums, then sh_grads_from_touched on the gathered pair, n = 1000"""
    import torch
    from gaussiansplat_amd import camera as gcam, synthetic
    n, deg, V = 1000, 3, 2
    model, W, H = small_scene(n, deg, 511)
    words = (n + 31) // 32
    bits = torch.zeros((V, words), dtype=torch.int32, device="cuda")
    rows = torch.zeros((V, n, 3), device="cuda")
    count = torch.zeros(V, dtype=torch.int64, device="cuda")
    recs = []
    for v in range(V):
        ctx = device_ctx(model, n, deg, W, H, view=v)
        ctx.preprocess(); ctx.bin(); ctx.forward_host()
        ctx.backward(synthetic.make_dC(W, H, 512 + v), ctx.grads_alloc(), overwrite=True)
        ctx.color_rows_pack(None, n, bits[v].data_ptr(), rows[v].data_ptr(), count[v:].data_ptr())
        ctx.synchronize()
        cam = synthetic.scene_camera(W, view=v)
        recs.append(np.concatenate([gcam.compute_transform(cam), gcam.compute_projection(cam, W, H), cam.eye, cam.lookAt]).astype(np.float32))
        if v + 1 < V:
            ctx.close()
    assert 0 < int(count.min()) and int(count.max()) < n, ("touched: both views must touch some rows and not all", count)
    d_shs = torch.full((n, 3 * (deg + 1) ** 2), 7.0, device="cuda")
    ctx.sh_grads_from_touched(np.stack(recs), bits.data_ptr(), rows.data_ptr(), n, d_shs.data_ptr(), overwrite=True)
    ctx.synchronize()
    R.put("touched/bits", bits.cpu().numpy()); R.put("touched/count", count.cpu().numpy())
    R.put("touched/rows", rows.cpu().numpy()); R.put("touched/d_shs", d_shs.cpu().numpy())
    ctx.close()


def case_adam(R):
    """One backward_adam step, dense and selective, n = 1000 at SH degree 3: parameters and both moments afterwards"""
    import torch
    from gaussiansplat_amd import backend as B, synthetic
    n, deg = 1000, 3
    for selective in (False, True):
        model, W, H = small_scene(n, deg, 521)
        before = host(model)
        g = torch.Generator("cuda").manual_seed(522)
        m = [0.01 * torch.randn(t.shape, device="cuda", generator=g) for t in model]
        v = [1e-4 * torch.rand(t.shape, device="cuda", generator=g) for t in model]
        dC = torch.as_tensor(synthetic.make_dC(W, H, 523)).cuda()
        ctx = device_ctx(model, n, deg, W, H)
        ctx.preprocess(); ctx.bin(); ctx.forward_host()
        G = lambda ts: B.GsGrads(*[t.data_ptr() for t in ts])
        ctx.backward_adam(dC.data_ptr(), G(m), G(v), [1.6e-4, 5e-3, 1e-3, 5e-2, 2.5e-3, 1.25e-4], 0.9, 0.999, 1e-15, 3, selective=selective)
        ctx.synchronize()
        tag = "adam_selective" if selective else "adam_dense"
        after = host(model)
        assert any(not np.array_equal(after[k], before[k]) for k in after), "adam: the step moved nothing"
        for name, ts in (("p", model), ("m", m), ("v", v)):
            for k, a in host(ts).items():
                R.put("%s/%s.%s" % (tag, name, k), a)
        ctx.close()


def case_active_degree(R):
    """One frame at active degree 1 of a stored degree 3 (the strided instantiations): image, T, gradients"""
    from gaussiansplat_amd import backend as B, synthetic
    sc, n, W, H, deg = scene("C2", 20000)
    ctx = B.Context(deterministic=True)
    set_model(ctx, sc, n, deg)
    ctx.set_active_sh_degree(1)
    set_cam(ctx, W, H, 0)
    g = ctx.grads_alloc()
    frame(R, "active_degree_1_of_3/f0", ctx, synthetic.make_dC(W, H, 1), g, lambda gg: ctx.grads_read(gg, deg))
    ctx.close()


def case_backward_forms(R):
    """The per-gaussian backward's instantiations at n = 300 on a C1-sized image (two workgroups, the second's last wave partly past n): stored =
    active degree 0 .. 3 and active 0 of stored 3 (strided); per degree two views on ONE set of gradient buffers, the first overwriting, the
    second accumulating -- both phases in one call (the fused kernels), and the phases apart (gs_sh_bwd_kernel alone, then gs_geom_bwd_kernel)"""
    from gaussiansplat_amd import backend as B, synthetic
    n, W, H = 300, 256, 256
    for stored, active in ((0, 0), (1, 1), (2, 2), (3, 3), (3, 0)):
        sc = synthetic.make_scene(n, W, H, stored, seed=561 + stored)
        for form, phases in (("one_call", ("all",)), ("phases_apart", ("composite", "params_sh", "params_geom"))):
            ctx = B.Context(deterministic=True)
            set_model(ctx, sc, n, stored)
            ctx.set_active_sh_degree(active)
            g = ctx.grads_alloc()
            got = []
            for view in (0, 1):
                ctx.set_view_slot(view)
                set_cam(ctx, W, H, view)
                ctx.preprocess(); ctx.bin(); ctx.forward_host()
                dC = synthetic.make_dC(W, H, 571 + view)
                for ph in phases:
                    ctx.backward(dC, g, overwrite=view == 0, phase=ph)
                got.append(ctx.grads_read(g, stored))
                for k, v in got[-1].items():
                    R.put("backward_forms/active_%d_of_%d_%s_view%d.%s" % (active, stored, form, view, k), v)
            assert all(np.isfinite(v).all() for v in got[1].values()) and all(got[0][k].any() and not np.array_equal(got[0][k], got[1][k]) for k in got[0]), \
                "backward forms: a view added nothing"
            ctx.close()


def image_pair(W, H, Cn, seed):
    """a smooth image and a noisy copy of it in [0, 1], and a weight in [0, 1] with zeros in it"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    gt = np.stack([0.5 + 0.4 * np.sin(0.11 * (c + 1) * x + 0.07 * y) for c in range(Cn)]).astype(np.float32)
    img = np.clip(gt + 0.1 * rng.standard_normal(gt.shape).astype(np.float32), 0.0, 1.0)
    w = rng.random((H, W), dtype=np.float32)
    w[w < 0.2] = 0.0
    return img, gt, w


def case_loss_metrics(R):
    from gaussiansplat_amd import backend as B
    W, H, Cn = 67, 35, 3
    img, gt, w = image_pair(W, H, Cn, 531)
    ctx = B.Context(deterministic=True)
    loss, dC = ctx.loss_host(img, gt)
    assert np.isfinite(loss) and loss > 0 and dC.any(), "loss: nothing computed"
    R.put("loss/value" + REL_KEY, np.float64(loss)); R.put("loss/dC", dC)
    for tag, weight in (("metrics", None), ("metrics_weight", w)):
        sums, smap = ctx.image_metrics_host(img, gt, weight, want_map=True)
        assert np.isfinite(sums).all() and sums[3] > 0, "metrics: nothing computed"
        R.put(tag + "/sums", sums); R.put(tag + "/ssim_map", smap)
    ctx.close()


def case_camera_grad(R):
    """degree 1 at n = 300 and n = 257 (the reduction's ragged ends), the other degrees' instantiations at n = 300"""
    from gaussiansplat_amd import backend as B, synthetic
    W, H = 64, 48
    for deg, n in ((1, 300), (1, 257), (0, 300), (2, 300), (3, 300)):
        sc = synthetic.make_scene(n, W, H, deg, seed=541)
        ctx = B.Context(deterministic=True)
        set_model(ctx, sc, n, deg)
        set_cam(ctx, W, H, 0)
        ctx.preprocess(); ctx.bin(); ctx.forward_host()
        ctx.backward(synthetic.make_dC(W, H, 542), ctx.grads_alloc(), overwrite=True)
        got = ctx.backward_camera()
        assert np.isfinite(got).all() and got.any(), "camera gradient: nothing computed"
        R.put(("camera_grad_n%d/d_camera" % n) if deg == 1 else ("camera_grad_degree_%d_n%d/d_camera" % (deg, n)), got)
        ctx.close()


def case_exposure(R):
    import torch
    from gaussiansplat_amd import backend as B
    ctx = B.Context(deterministic=True)
    E = torch.tensor([1.1, 0.05, -0.02, 0.01, 0.03, 0.9, 0.04, -0.02, -0.01, 0.02, 1.05, 0.03], device="cuda")
    for W, H in ((129, 33), (64, 16)):
        img, d_out, w = image_pair(W, H, 3, 551 + W)
        img_t, d_t, w_t = (torch.as_tensor(a).cuda() for a in (img, d_out - 0.5, w))
        for tag, wp in (("", 0), ("_weight", w_t.data_ptr())):
            d_img, dE = torch.full_like(img_t, 7.0), torch.full((12,), 7.0, device="cuda")
            torch.cuda.synchronize()
            ctx.exposure_backward(img_t.data_ptr(), d_t.data_ptr(), E.data_ptr(), wp, W, H, d_img.data_ptr(), dE.data_ptr())
            ctx.synchronize()
            assert bool(torch.isfinite(dE).all()) and bool((dE != 7.0).all()), "exposure: d_exposure not written"
            R.put("exposure_%dx%d%s/d_img" % (W, H, tag), d_img.cpu().numpy()); R.put("exposure_%dx%d%s/d_exposure" % (W, H, tag), dE.cpu().numpy())
    ctx.close()


def record(path):
    from gaussiansplat_amd import backend as B
    R = Recorder()
    case_3d(R, "C1_small", "C1", sort_before=True)                      # small path; sortIdxs before the forward (frames 0, 2) and after it (every frame)
    case_3d(R, "C1_small_float_atomics", "C1", frames=2, deterministic=False)
    case_3d(R, "C1_bin_path_3", "C1", bin_path=3)
    case_3d(R, "C2", "C2")
    case_3d(R, "C3", "C3")
    case_grow(R)
    case_3d(R, "C3_list_cap_2", "C3", frames=3, list_cap=2)
    case_3d(R, "C3_list_cap_2_get_ids", "C3", frames=3, list_cap=2, ids_between=True)
    case_3d(R, "C2_tiny_caps", "C2", frames=3, debug_flags=B.GS_DEBUG_TINY_CAPS)
    case_3d(R, "C2_slabs_bin_path_0", "C2", frames=3, bin_path=0, slab_fractions=(0.3,))
    case_3d(R, "C2_slabs_bin_path_2", "C2", frames=3, bin_path=2, slab_fractions=(0.3,))
    case_3d(R, "C2_bin_path_1", "C2", frames=2, bin_path=1)
    case_3d(R, "C2_bin_path_2", "C2", frames=2, bin_path=2)
    case_3d(R, "C2_depth_sort_1", "C2", frames=2, depth_sort=1)
    case_3d(R, "C2_depth_sort_2", "C2", frames=2, depth_sort=2)
    case_3d(R, "C1_depth_sort_2", "C1", frames=2, depth_sort=2)
    case_3d(R, "C2_order_index", "C2", frames=2, order=B.ORDER_INDEX)
    case_3d(R, "C1_order_index", "C1", frames=2, order=B.ORDER_INDEX)
    case_3d(R, "C2_super16", "C2", frames=2, debug_flags=B.GS_DEBUG_SUPER16)
    case_3d(R, "C2_wide_cursors", "C2", frames=2, debug_flags=B.GS_DEBUG_WIDE_CURSORS)
    # small frames with the paths forced on (capped lists + orders + side stream; list segments; slab rounds), then C3 scale (8160 tiles, above the wave
    # slots) under the defaults: n = 1 000 000 with the order kernel on the side stream, n = 200 000 without
    small = dict(n=3000, W=160, H=96, deg=1, seed=41, grow=2.0)
    case_history(R, "history_small_caps", bin_path=3, list_cap=2, slab_mode=0, debug_flags=B.GS_DEBUG_ALWAYS_ORDER, **small)
    case_history(R, "history_small_segments", slab_mode=0, tile_parts=0, **small)
    case_history(R, "history_small_slabs", bin_path=3, slab_max_ratio=0.15, list_cap=1, **small)
    for n in (1_000_000, 200_000):
        case_history(R, "history_C3_n%d" % n, n, *synthetic_config("C3")[1:], seed=1236)
    case_2d(R)
    case_empty(R)
    case_tile_clock(R)
    case_density(R)
    case_mcmc(R)
    case_touched(R)
    case_adam(R)
    case_active_degree(R)
    case_backward_forms(R)
    case_loss_metrics(R)
    case_camera_grad(R)
    case_exposure(R)
    np.savez(path, **R.out)
    print("recorded %d arrays -> %s" % (len(R.out), path))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    cases, lines, differ = {}, [], 0
    for k in sorted(set(a.files) | set(b.files)):
        c = cases.setdefault(k.split("/")[0].split(".")[0].split("!")[0], dict(n=0, bad=[], refused=set()))
        c["n"] += 1
        if k not in a.files or k not in b.files or not same(k, a[k], b[k]):
            c["bad"].append(k)
        elif "!refused" in k:
            c["refused"].add(bytes(a[k]).decode()[:60])
    for name, c in sorted(cases.items()):
        differ += len(c["bad"])
        lines.append("%-28s %4d arrays  %s%s" % (name, c["n"], "equal" if not c["bad"] else "DIFFER: " + ", ".join(c["bad"][:6]),
                                                 "   [refused alike: %s]" % "; ".join(sorted(c["refused"])) if c["refused"] else ""))
    lines.append("total: %d arrays, %d differ" % (sum(c["n"] for c in cases.values()), differ))
    return lines, differ


def frames():
    R = Recorder()
    case_3d(R, "C1", "C1", frames=3)
    case_3d(R, "C3", "C3", frames=3)
    case_3d(R, "C2_slabs_bin_path_2", "C2", frames=3, bin_path=2, slab_fractions=(0.3,))


def kernels(d):
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), r.get("Queue_Id", "0"), r["Kernel_Name"]))
    rows.sort()
    h = lambda names: hashlib.blake2b("\n".join(names).encode(), digest_size=8).hexdigest()
    queues = {}
    for _, q, name in rows:
        queues.setdefault(q, []).append(name)
    per_queue = sorted((len(v), h(v)) for v in queues.values())
    print("%d kernels  in start order: %s  per queue, each in its own order: %s" % (len(rows), h([r[2] for r in rows]),
                                                                                   " ".join("%d:%s" % p for p in per_queue)))


def run(lib_a, lib_b, log=None):
    out = os.environ.get("OUT", "out")
    os.makedirs(out, exist_ok=True)
    files = []
    for tag, lib in (("a", lib_a), ("b", lib_b)):
        f = os.path.join(out, "compare_libs_%s.npz" % tag)
        rc = subprocess.run(["timeout", "-k", "10", "560", sys.executable, os.path.abspath(__file__), "record", f],
                            env=dict(os.environ, GSPLAT_HIP_LIB=os.path.abspath(lib))).returncode
        if rc != 0:
            sys.exit("record with %s ended with status %d: nothing more is run" % (lib, rc))
        files.append(f)
    lines, differ = compare(*files)
    text = "\n".join(["# %s against %s" % (lib_a, lib_b)] + lines)
    print(text)
    if log:
        open(log, "a").write(text + "\n")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "record":
        record(sys.argv[2])
    elif cmd == "compare":
        lines, differ = compare(sys.argv[2], sys.argv[3])
        print("\n".join(lines))
        sys.exit(1 if differ else 0)
    elif cmd == "run":
        run(*sys.argv[2:5])
    elif cmd == "frames":
        frames()
    elif cmd == "kernels":
        kernels(sys.argv[2])
    else:
        sys.exit(__doc__)
