#!/usr/bin/env python3
"""What the per-view exposure stage costs, against the torch formulation a user would write without it (GPU box; no CPU fallback).

    python3 tools/exposure_time.py [--size 1920x1080] [--pairs 5] [--batch 20] [--out profiles/exposure_time.json]

One process, device-resident inputs (x, d ~ N(0, 1), E = [I | 0] + N(0, 0.2^2), a weight uniform in [0, 1] with a quarter of the pixels
0), with and without the weight.  After a warm-up of every variant, in each of `pairs` pairs the HIP path and the torch formulation run
in turn, each as `batch` back-to-back calls between two device events on the ctx's stream; a call's time is the batch's over `batch`.
  apply      gs_exposure_apply                      | w * (einsum('rk,khw->rhw', M, x) + b)
  backward   gs_exposure_backward with d_exposure   | g = w * d; einsum('rk,rhw->khw', M, g); (g * x_k).sum() for k < 3 and g.sum(): four sums
             (its two launches: the pixel kernel and the finishing workgroup)
Bytes per pixel: apply 24, backward 36, + 4 each with a weight; the achieved rate is set against the 6.29 TB/s DESIGN
records for a device copy.  Checks: the HIP d_img against a torch restatement in the statement's own order of operations, bit for bit;
against the einsum form (bits, and the largest difference: the library behind einsum chooses its own order); the HIP dE against the
float64 sum within P 2^-53 A + 2^-24 |exact| + 2^-149, and bit-equal between the first and the last call."""
import argparse
import statistics

from _timing import emit, event_ms, interleaved

COPY_TBS = 6.29                     # DESIGN: a device copy on MI355X
BYTES = {"apply": 24, "backward": 36}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from gaussiansplat_amd import backend as B
    assert torch.cuda.is_available(), "needs a HIP device"
    W, H = (int(v) for v in a.size.split("x"))
    P = W * H
    g = torch.Generator().manual_seed(3)
    x, d = (torch.randn((3, H, W), generator=g).cuda() for _ in range(2))
    E = (torch.eye(3, 4) + 0.2 * torch.randn((3, 4), generator=g)).cuda().contiguous()
    wt = torch.rand((H, W), generator=g)
    wt[torch.rand((H, W), generator=g) < 0.25] = 0.0
    wt = wt.cuda()
    M, b = E[:, :3].contiguous(), E[:, 3].contiguous()
    out, d_img, dE = torch.empty_like(x), torch.empty_like(x), torch.empty(12, device="cuda")
    ctx = B.Context()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream or 1)
    keep = {}

    def hip_apply(w):
        ctx.exposure_apply(x.data_ptr(), E.data_ptr(), w.data_ptr() if w is not None else 0, W, H, out.data_ptr())

    def hip_backward(w):
        ctx.exposure_backward(x.data_ptr(), d.data_ptr(), E.data_ptr(), w.data_ptr() if w is not None else 0, W, H, d_img.data_ptr(), dE.data_ptr())

    def torch_apply(w):
        o = torch.einsum("rk,khw->rhw", M, x) + b[:, None, None]
        keep["out"] = o if w is None else w * o

    def torch_backward(w):
        gg = d if w is None else w * d
        keep["d_img"] = torch.einsum("rk,rhw->khw", M, gg)
        keep["dE"] = [(gg * x[k]).sum((1, 2)) for k in range(3)] + [gg.sum((1, 2))]

    def in_order(w):                                    # the statement's own order of operations, elementwise: bit for bit the kernels'
        gg = d if w is None else w * d
        return torch.stack([(E[0, k] * gg[0] + E[1, k] * gg[1]) + E[2, k] * gg[2] for k in range(3)])

    def timed(f, w):
        return event_ms(lambda: f(w), a.batch) * 1e3    # us per call

    res = {"device": torch.cuda.get_device_name(0), "width": W, "height": H, "pairs": a.pairs, "batch": a.batch, "copy_TBs": COPY_TBS, "cases": {}}
    ok = True
    for name, w in (("no_weight", None), ("weight", wt)):
        for f in (hip_apply, torch_apply, hip_backward, torch_backward):       # warm-up: code objects, scratch buffers, the caching allocator
            for _ in range(3):
                f(w)
        torch.cuda.synchronize()
        first = dE.cpu().numpy().copy()
        case = {}
        for stage, hip, ref in (("apply", hip_apply, torch_apply), ("backward", hip_backward, torch_backward)):
            t = interleaved({"hip": lambda: timed(hip, w), "torch": lambda: timed(ref, w)}, a.pairs, warmup=0)
            pairs = list(zip(t["hip"], t["torch"]))
            nbytes = (BYTES[stage] + (4 if w is not None else 0)) * P
            med = statistics.median(p[0] for p in pairs)
            case[stage] = {"hip_us": [p[0] for p in pairs], "torch_us": [p[1] for p in pairs], "hip_median_us": med,
                           "torch_median_us": statistics.median(p[1] for p in pairs), "bytes": nbytes, "hip_TBs": nbytes / med * 1e-6,
                           "share_of_copy": nbytes / med * 1e-6 / COPY_TBS, "hip_not_slower_in_any_pair": all(p[0] <= p[1] for p in pairs),
                           "worst_pair_hip_over_torch": max(p[0] / p[1] for p in pairs)}
        torch.cuda.synchronize()
        hip_dimg, hip_dE = d_img.cpu().numpy(), dE.cpu().numpy().astype(np.float64).reshape(3, 4)
        gg = (d if w is None else w * d).double().reshape(3, -1)
        xa = torch.cat([x.double().reshape(3, -1), torch.ones((1, P), dtype=torch.float64, device="cuda")])
        exact, A = (gg @ xa.T).cpu().numpy(), (gg.abs() @ xa.abs().T).cpu().numpy()      # float64 sums of the exact terms (within P 2^-53 A themselves)
        bound = 2 * P * 2.0 ** -53 * A + 2.0 ** -24 * np.abs(exact) + 2.0 ** -149        # (twice: the yardstick here is a float64 sum, not fsum)
        case["d_img_bits_equal_statement_order"] = hip_dimg.tobytes() == in_order(w).cpu().numpy().tobytes()
        case["d_img_bits_equal_einsum"] = hip_dimg.tobytes() == keep["d_img"].cpu().numpy().tobytes()
        case["d_img_max_abs_diff_einsum"] = float(np.abs(hip_dimg - keep["d_img"].cpu().numpy()).max())
        case["out_bits_equal_einsum"] = out.cpu().numpy().tobytes() == keep["out"].cpu().numpy().tobytes()
        case["dE_error_over_bound"] = float((np.abs(hip_dE - exact) / bound).max())
        case["dE_bitwise_reproducible"] = first.tobytes() == dE.cpu().numpy().tobytes()
        torch_dE = torch.stack(keep["dE"], 1).cpu().numpy().astype(np.float64)
        case["torch_dE_error_over_bound"] = float((np.abs(torch_dE - exact) / bound).max())
        ok = ok and case["d_img_bits_equal_statement_order"] and case["dE_error_over_bound"] <= 1.0 and case["dE_bitwise_reproducible"]
        res["cases"][name] = case
    res["hip_not_slower_in_any_pair"] = all(c[s]["hip_not_slower_in_any_pair"] for c in res["cases"].values() for s in ("apply", "backward"))
    ctx.close()
    emit(res, a.out)
    assert ok, "the HIP path missed a check (see the JSON)"


if __name__ == "__main__":
    main()
