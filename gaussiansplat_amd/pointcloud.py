"""The first step of the 3DGS recipe (Kerbl et al. 2023): a model from an SfM point cloud.

    pc = PointCloud(points, colors)                    # or ply.load_points("points3D.ply")
    renderer = getRenderer("GAUSSIAN_3D", (W, H), (16, 16), None, source=pc)

Means are the points, SH band 0 the point colours, opacity 0.1, quaternions the identity, and the scale of every gaussian the mean
distance to its three nearest neighbours (`distCUDA2` in the original): `knn_mean_dist2` is an exact search on the device
(gs_knn_mean_dist2: bit for bit a brute force, include/gsplat.h), `from_points` writes the five arrays there (gs_init_from_points).
There is no CPU path: without a HIP device both raise.
"""
from __future__ import annotations

import math

import numpy as np

from . import backend as B

KNN_BOX = B.KNN_BOX                        # points per box of the search (GS_KNN_BOX)
MIN_POINTS = 4                             # a point needs three neighbours


class PointCloud:
    """points [n, 3] float32, colors [n, 3] in [0, 1] or None (grey), the SH degree of the model to build and its initial opacity.
    Checked on the host: ValueError for a non-finite point, fewer than 4 points, a colour outside [0, 1], a bad degree or opacity."""

    def __init__(self, points, colors=None, sh_degree: int = 3, opacity: float = 0.1):
        pts = np.ascontiguousarray(points, np.float32)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError(f"PointCloud: points must be [n, 3], got {pts.shape}")
        if pts.shape[0] < MIN_POINTS:
            raise ValueError(f"PointCloud: {pts.shape[0]} points; the 3-nearest-neighbour scale needs at least {MIN_POINTS}")
        if not np.isfinite(pts).all():
            raise ValueError("PointCloud: a point is not finite")
        if colors is not None:
            colors = np.ascontiguousarray(colors, np.float32)
            if colors.shape != pts.shape:
                raise ValueError(f"PointCloud: colors must be [n, 3] like points, got {colors.shape}")
            if not (np.all(colors >= 0.0) and np.all(colors <= 1.0)):      # a NaN fails both
                raise ValueError("PointCloud: colours must lie in [0, 1]")
        if isinstance(sh_degree, bool) or int(sh_degree) != sh_degree or not 0 <= int(sh_degree) <= 3:
            raise ValueError(f"PointCloud: sh_degree must be 0..3, got {sh_degree!r}")
        opacity = float(opacity)
        if not 0.0 < opacity < 1.0:                                         # a NaN fails
            raise ValueError(f"PointCloud: opacity must lie strictly between 0 and 1, got {opacity!r}")
        self.points, self.colors, self.sh_degree, self.opacity = pts, colors, int(sh_degree), opacity

    def __len__(self):
        return self.points.shape[0]


def _points_tensor(points):
    import torch
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise TypeError("a float32 tensor [n, 3] on a HIP device is needed (there is no CPU path)")
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
        raise ValueError("points must be a contiguous float32 tensor [n, 3]")
    return points


def knn_mean_dist2(points, ctx: "B.Context | None" = None):
    """dist2 [n] of a device tensor points [n, 3]: the mean of the three smallest squared distances to the other finite points (NaN for a
    point that is not finite, or when fewer than four are).  ctx: a backend.Context to run on (its frame is left alone); None: a
    short-lived one on the tensor's device."""
    import torch
    from .renderer import _current_stream_handle
    points = _points_tensor(points)
    dist2 = torch.empty(points.shape[0], dtype=torch.float32, device=points.device)
    own = ctx is None
    if own:
        ctx = B.Context(device=points.device.index or 0)
    try:
        ctx.set_stream(_current_stream_handle(points.device) or 1)      # torch's current stream (0 = the legacy default stream = 1 here)
        ctx.knn_mean_dist2(points.data_ptr(), points.shape[0], dist2.data_ptr())
        if own:
            ctx.synchronize()
    finally:
        if own:
            ctx.close()
    return dist2


def from_points(pc: PointCloud, device: int = 0):
    """The SplatData3D a training run starts from, built on the device by a short-lived backend.Context."""
    import torch
    from .renderer import SplatData3D, _current_stream_handle
    if not torch.cuda.is_available():
        raise RuntimeError("gaussiansplat_amd needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda", device)
    n, k3 = len(pc), 3 * (pc.sh_degree + 1) ** 2
    with torch.cuda.device(dev):
        points = torch.as_tensor(pc.points).to(dev).contiguous()
        colors = torch.as_tensor(pc.colors).to(dev).contiguous() if pc.colors is not None else None
        new = lambda w: torch.empty((n, w), dtype=torch.float32, device=dev)
        data = SplatData3D(means=new(3), scales=new(3), shs=new(k3), quaternions=new(4), opacities=new(1))
        dist2 = torch.empty(n, dtype=torch.float32, device=dev)
        dst = B.GsGrads(data.means.data_ptr(), data.scales.data_ptr(), data.quaternions.data_ptr(), data.opacities.data_ptr(), data.shs.data_ptr())
        ctx = B.Context(device=device)
        try:
            ctx.set_stream(_current_stream_handle(dev) or 1)
            ctx.knn_mean_dist2(points.data_ptr(), n, dist2.data_ptr())
            ctx.init_from_points(points.data_ptr(), colors.data_ptr() if colors is not None else None, dist2.data_ptr(), n, pc.sh_degree,
                                 math.log(pc.opacity / (1.0 - pc.opacity)), dst)
            ctx.synchronize()
        finally:
            ctx.close()
    return data
