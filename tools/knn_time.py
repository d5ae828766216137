"""Time of gs_knn_mean_dist2 (the exact 3-NN search of the point-cloud initialisation) against a torch brute force.

    python tools/knn_time.py [--reps 11] [--out profiles/knn_time.json]

hipEvent times (torch.cuda.Event on the ctx's stream), two warm-up runs, the median of `reps` (>= 10) runs of:
  uniform_100k / uniform_1m     points uniform in the unit cube
  clustered_1m                  the means of synthetic.make_scene(1_000_000, ..., clustered=True): 60 % of the points in three blobs
  torch_brute_100k              tests/knn_ref.torch_brute on the 100 k cloud: chunked sub / mul / add / topk, the independent yardstick
The one condition: at 100 k the library call must be faster than the brute force of the same run (exit status 1 otherwise -- the pruning
would not be working).  The 100 k results of the two are also compared bit for bit.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from _timing import ROOT, emit, event_ms, interleaved, stat

sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import knn_ref as K
    from gaussiansplat_amd import backend as B, synthetic
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default="")
    ap.add_argument("--box", type=int, default=B.KNN_BOX, help="GS_KNN_BOX of the library loaded (a variant build under GSPLAT_HIP_LIB): recorded only")
    ap.add_argument("--skip-brute", action="store_true", help="time the library only (A/B runs of variant builds)")
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    clouds = dict(uniform_100k=K.uniform(100_000, 1), uniform_1m=K.uniform(1_000_000, 2),
                  clustered_1m=synthetic.make_scene(1_000_000, 1920, 1080, 0, seed=3, clustered=True)["means"])
    ctx = B.Context()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream or 1)          # torch's current stream; 0, the legacy default stream, is 1 here

    def measure(name, fn):                                                # two warm-up runs, then `reps`
        s = stat(interleaved({name: lambda: event_ms(fn)}, a.reps, warmup=2)[name])
        med[name], spread[name] = s["median"], (s["min"], s["max"])

    med, spread, results = {}, {}, {}
    for name, pts in clouds.items():
        tp = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda()
        out = torch.empty(tp.shape[0], dtype=torch.float32, device="cuda")
        call = lambda: ctx.knn_mean_dist2(tp.data_ptr(), tp.shape[0], out.data_ptr())
        measure(name, call)
        results[name] = out.cpu().numpy()
        print(f"{name}: median {med[name]:.3f} ms (min {spread[name][0]:.3f}, max {spread[name][1]:.3f})", flush=True)
    same, ratio = None, None
    if not a.skip_brute:
        tp = torch.from_numpy(clouds["uniform_100k"]).cuda()
        brute = {}
        run = lambda: brute.update(r=K.torch_brute(tp))
        measure("torch_brute_100k", run)
        same = K.same_bits(results["uniform_100k"], brute["r"])
        ratio = med["torch_brute_100k"] / med["uniform_100k"]
    res = dict(box=a.box, lib=os.path.relpath(B.LIB_PATH, ROOT), reps=a.reps, median_ms=med, min_max_ms=spread, brute_over_hip_100k=ratio, bit_identical_100k=same,
               device=torch.cuda.get_device_name(0))
    emit(res, a.out, indent=1)
    ctx.close()
    if not a.skip_brute and (not same or not ratio > 1.0):
        print("FAILED: the search must equal the brute force and be faster than it at 100 k", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
