#!/usr/bin/env python3
"""What the per-view bilateral grid costs, against the torch formulation a user would write without it (GPU box; no CPU fallback).

    python3 tools/bilagrid_time.py [--size 1920x1080] [--grid 16x16x8] [--pairs 5] [--batch 10] [--out profiles/bilagrid_time.json]

One process, device-resident inputs (x ~ U(-0.1, 1.1), d ~ N(0, 1), G = identity + N(0, 0.2^2), no weight).  After a warm-up of every
variant, in each of `pairs` pairs the HIP path and the torch formulation run in turn, each as `batch` back-to-back calls between two
device events on the ctx's stream; a call's time is the batch's over `batch`.
  apply             gs_bilagrid_apply                      | grid_sample(G as [1, 12, Gz, Gy, Gx], (c / (W - 1), r / (H - 1), clamp(l)), bilinear,
                                                           | border, align_corners=True) and the affine, float32
  backward          gs_bilagrid_backward with d_grid       | torch.autograd.grad of that graph into (x, G), the graph built outside the clock
                    (its two launches: gather, image pass)
  backward_no_grid  gs_bilagrid_backward, d_grid NULL      | torch.autograd.grad into x alone
and a plain device copy of the three planes (dst.copy_(src): 24 bytes per pixel) gives the rate the streaming passes are set against:
apply moves 24 bytes per pixel, the image pass of the backward 36.  Checks: the HIP results against the float32 torch ones (largest
difference, relative to the largest entry for d_grid) and d_grid bit-equal between the first and the last call."""
import argparse
import statistics

from _timing import emit, event_ms, interleaved

BYTES = {"apply": 24, "backward": 36, "backward_no_grid": 36}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--grid", default="16x16x8")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as Fn
    from gaussiansplat_amd import backend as B
    assert torch.cuda.is_available(), "needs a HIP device"
    W, H = (int(v) for v in a.size.split("x"))
    dims = tuple(int(v) for v in a.grid.split("x"))
    Gx, Gy, Gz = dims
    P = W * H
    g = torch.Generator().manual_seed(3)
    x = (torch.rand((3, H, W), generator=g) * 1.2 - 0.1).cuda()
    d = torch.randn((3, H, W), generator=g).cuda()
    ident = torch.tensor([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    G = (ident.repeat(Gz, Gy, Gx, 1) + 0.2 * torch.randn((Gz, Gy, Gx, 12), generator=g)).cuda().contiguous()
    out, d_img, dG, copy_dst = torch.empty_like(x), torch.empty_like(x), torch.empty(G.numel(), device="cuda"), torch.empty_like(x)
    ctx = B.Context()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream or 1)
    cx = (torch.arange(W, device="cuda") / max(W - 1, 1))[None, :].expand(H, W)
    cy = (torch.arange(H, device="cuda") / max(H - 1, 1))[:, None].expand(H, W)
    keep = {}

    def torch_forward(xt, Gt):
        l = 0.299 * xt[0] + 0.587 * xt[1] + 0.114 * xt[2]
        coords = torch.stack([cx, cy, l.clamp(0, 1)], dim=-1) * 2 - 1
        A = Fn.grid_sample(Gt.permute(3, 0, 1, 2)[None], coords[None, None], mode="bilinear", padding_mode="border", align_corners=True)
        A = A[0, :, 0].reshape(3, 4, H, W)
        return (A[:, :3] * xt[None]).sum(1) + A[:, 3]

    xt, Gt = x.clone().requires_grad_(True), G.clone().requires_grad_(True)
    graph = torch_forward(xt, Gt)

    def hip_apply():
        ctx.bilagrid_apply(x.data_ptr(), G.data_ptr(), dims, 0, W, H, out.data_ptr())

    def hip_backward():
        ctx.bilagrid_backward(x.data_ptr(), d.data_ptr(), G.data_ptr(), dims, 0, W, H, d_img.data_ptr(), dG.data_ptr())

    def hip_backward_no_grid():
        ctx.bilagrid_backward(x.data_ptr(), d.data_ptr(), G.data_ptr(), dims, 0, W, H, d_img.data_ptr(), 0)

    def torch_apply():
        with torch.no_grad():
            keep["out"] = torch_forward(x, G)

    def torch_backward():
        keep["d_img"], keep["dG"] = torch.autograd.grad(graph, (xt, Gt), grad_outputs=d, retain_graph=True)

    def torch_backward_no_grid():
        keep["d_img_alone"], = torch.autograd.grad(graph, (xt,), grad_outputs=d, retain_graph=True)

    def copy():
        copy_dst.copy_(x)

    stages = (("apply", hip_apply, torch_apply), ("backward", hip_backward, torch_backward),
              ("backward_no_grid", hip_backward_no_grid, torch_backward_no_grid))
    for _, hip, ref in stages:                          # warm-up: code objects, the caching allocator
        for _ in range(3):
            hip(); ref()
    for _ in range(3):
        copy()
    torch.cuda.synchronize()
    first = dG.cpu().numpy().copy()
    us = lambda f: event_ms(f, a.batch) * 1e3           # us per call
    copy_us = statistics.median(us(copy) for _ in range(a.pairs))
    res = {"device": torch.cuda.get_device_name(0), "width": W, "height": H, "grid": list(dims), "pairs": a.pairs, "batch": a.batch,
           "copy_us": copy_us, "copy_TBs": 24 * P / copy_us * 1e-6, "stages": {}}
    for stage, hip, ref in stages:
        t = interleaved({"hip": lambda: us(hip), "torch": lambda: us(ref)}, a.pairs, warmup=0)
        pairs = list(zip(t["hip"], t["torch"]))
        med = statistics.median(p[0] for p in pairs)
        res["stages"][stage] = {"hip_us": [p[0] for p in pairs], "torch_us": [p[1] for p in pairs], "hip_median_us": med,
                                "torch_median_us": statistics.median(p[1] for p in pairs), "streamed_bytes": BYTES[stage] * P,
                                "streamed_TBs": BYTES[stage] * P / med * 1e-6, "hip_over_copy_time": med / copy_us,
                                "hip_not_slower_in_any_pair": all(p[0] <= p[1] for p in pairs),
                                "worst_pair_hip_over_torch": max(p[0] / p[1] for p in pairs)}
    hip_backward()
    torch.cuda.synchronize()
    res["out_max_abs_diff_torch"] = float((out - keep["out"]).abs().max())
    res["d_img_max_abs_diff_torch"] = float((d_img - keep["d_img"]).abs().max())
    res["d_grid_max_diff_over_largest_torch"] = float((dG.reshape(G.shape) - keep["dG"]).abs().max() / keep["dG"].abs().max())
    res["d_grid_bitwise_reproducible"] = first.tobytes() == dG.cpu().numpy().tobytes()
    ctx.close()
    emit(res, a.out)
    assert res["d_grid_bitwise_reproducible"], "d_grid changed between two calls"


if __name__ == "__main__":
    main()
