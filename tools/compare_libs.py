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
Per frame: image, T, the five gradient arrays, tile ranges, sorted ids, sortIdxs, num_instances / _coarse_instances / _rounds,
bin_path_of_frame, list_stats, work_counters_ex; and the counting words of the composite kernels' debug record on one small frame."""
import csv, glob, hashlib, os, subprocess, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    case_2d(R)
    case_empty(R)
    case_tile_clock(R)
    np.savez(path, **R.out)
    print("recorded %d arrays -> %s" % (len(R.out), path))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    cases, lines, differ = {}, [], 0
    for k in sorted(set(a.files) | set(b.files)):
        c = cases.setdefault(k.split("/")[0].split(".")[0].split("!")[0], dict(n=0, bad=[], refused=set()))
        c["n"] += 1
        if k not in a.files or k not in b.files or not np.array_equal(a[k], b[k]):
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
        rc = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "record", f],
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
