"""Polyp localisation: labelled pixels + depth maps + trajectory -> where each polyp lies and how large it is.

The upstream README names "immediate polyp localization" beside the reconstruction, and its reconstruction figure prints a
localisation error "e:" next to each polyp.  Deciding WHICH pixels are polyp is a detector's job and stays the caller's; this
module is the other half, which needs exactly what the project produces: per frame and polyp the mean position of the labelled
surface in the camera frame and in the world frame, its covariance, pixel centre and bounding box, and per polyp the
sample-weighted position over all frames that show it, an extent, and the distance to ground truth after trajectory alignment.

Contract (csrc/localize.hip, one pass over the frames; include/colvo.h colvo_localize_* spells out every association)
  walked pixels  those of stitch_point_cloud / fuse_point_cloud: (u, v) = (i * stride, j * stride).
  labelled pixel of (n, l): a walked pixel of frame n carrying label l (1..num_labels; 0 is background; a value above num_labels
                 is treated as background and counted in n_ignored).
  sample         a labelled pixel with 0 < d < max_depth (NaN falls out) -- and, with clip_sigma, inside the clip bound.
  point          float32, one rounding per operation: px = ((u - cx) / fx) * d, py = ((v - cy) / fy) * d, pz = d, quantised to
                 q_a = rint(p_a * 4096).  Per (n, l) only integer sums are kept (counts, sum u, sum v, sum q_a, sum q_a q_b, the
                 bounding box), so the result is bit-identical between calls and streams; means and covariances are evaluated from
                 them in float64.
  clip           clip_sigma = k: after a first pass, every (n, l) with at least two samples gets mean_z and var_z of its quantised
                 depths; a second pass keeps a sample iff (q_z / 4096 - mean_z)^2 <= float32(k)^2 * var_z.  One round.  For masks
                 that spill onto the wall behind a polyp.  n_pixels and bbox do not depend on it.
  per polyp      over the frames with n_samples >= min_samples, in ascending frame order: the sample-weighted mean of center_world
                 and the covariance of all their samples in the world frame (law of total covariance).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._args import MAX_DEPTH, depth_views, f32
from .trajectory import align_trajectory


class PolypLocalization(NamedTuple):
    # per observation (frame n, polyp l = label - 1)
    n_pixels: torch.Tensor          # [N,L]   int32: labelled pixels
    n_samples: torch.Tensor         # [N,L]   int32: ... with a kept depth (and inside the clip bound)
    bbox: torch.Tensor              # [N,L,4] int32: (u0, v0, u1, v1) of the labelled pixels, inclusive; -1 where n_pixels = 0
    pixel: torch.Tensor             # [N,L,2] float64: mean (u, v) of the samples
    center_cam: torch.Tensor        # [N,L,3] float64: mean of the samples in the camera frame
    cov_cam: torch.Tensor           # [N,L,6] float64: their covariance, xx xy xz yy yz zz
    center_world: torch.Tensor      # [N,L,3] float64: cam2world applied to center_cam
    # per polyp
    n_frames: torch.Tensor          # [L]   int32: frames with n_samples >= min_samples
    n_samples_total: torch.Tensor   # [L]   int64: samples in those frames
    first_frame: torch.Tensor       # [L]   int32, -1 if never seen
    last_frame: torch.Tensor        # [L]   int32, -1 if never seen
    position: torch.Tensor          # [L,3] float64: sample-weighted mean of center_world
    cov_world: torch.Tensor         # [L,6] float64: covariance of the samples in the world frame
    radius: torch.Tensor            # [L]   float64: sqrt(max(trace(cov_world), 0)), the RMS distance of the samples from position
    # statistics (read back)
    n_labelled: int                 # labelled pixels in all frames
    n_ignored: int                  # walked pixels whose label is above num_labels


def quantum_bound(K: torch.Tensor, H: int, W: int, max_depth: float) -> float:
    """max_depth * ray_max * 4096 in float64: the largest |q_a| any sample of these cameras can have.  ray_max is the largest
    |(u - cx) / fx|, |(v - cy) / fy| or 1 over the image corners of any frame."""
    Kd = K.detach().to("cpu", torch.float64).reshape(-1, 3, 3)
    ray = 1.0
    for u in (0.0, float(W - 1)):
        ray = max(ray, float(((u - Kd[:, 0, 2]) / Kd[:, 0, 0]).abs().max()))
    for v in (0.0, float(H - 1)):
        ray = max(ray, float(((v - Kd[:, 1, 2]) / Kd[:, 1, 1]).abs().max()))
    return float(max_depth) * ray * 4096.0


def check_sum_bounds(K: torch.Tensor, H: int, W: int, stride: int, max_depth: float) -> None:
    """The two guards of the integer sums, on the host in float64; ValueError if either fails.  b = quantum_bound(...) must be
    below 2^31 (a quantum fits int32) and b^2 * ceil(H / stride) * ceil(W / stride) below 2^62 (a frame's sum of products fits
    int64).  At MAX_DEPTH and 256x320 with the synthetic intrinsics the second is about 2^47."""
    walked = -(-H // stride) * -(-W // stride)
    bound = quantum_bound(K, H, W, max_depth)
    if not bound < 2.0 ** 31:
        raise ValueError(f"localize_polyps: max_depth * ray_max * 4096 = {bound:.4g} is not below 2^31: a quantum could overflow int32")
    if not bound * bound * walked < 2.0 ** 62:
        raise ValueError(f"localize_polyps: (max_depth * ray_max * 4096)^2 * {walked} walked pixels = {bound * bound * walked:.4g} is "
                         "not below 2^62: a sum of products could overflow int64")


def localize_polyps(depths: torch.Tensor, labels: torch.Tensor, K: torch.Tensor, cam2world: torch.Tensor, *, num_labels: int,
                    stride: int = 1, max_depth: float = MAX_DEPTH, clip_sigma: Optional[float] = None,
                    min_samples: int = 1) -> PolypLocalization:
    """depths [N,1,H,W] float32, labels [N,1,H,W] uint8, K [N,3,3], cam2world [N,4,4], all on the GPU -> PolypLocalization
    (module docstring).  A label means the same polyp in every frame: associating detections across frames is the detector's
    or tracker's job, not this function's.  Refuses (ValueError, before any launch) cameras whose quanta could overflow the
    integer sums: max_depth * ray_max * 4096 must stay below 2^31 and its square times the walked pixels of a frame below 2^62.
    Reads K back for that check and two counts at the end."""
    lib = _lib.load()
    if not isinstance(num_labels, int) or not 1 <= num_labels <= 255:
        raise ValueError(f"localize_polyps: num_labels must be an integer in 1..255, got {num_labels!r}")
    if stride < 1 or min_samples < 1:
        raise ValueError("localize_polyps: stride and min_samples must be >= 1")
    if not (max_depth > 0.0 and math.isfinite(max_depth)):
        raise ValueError("localize_polyps: max_depth must be finite and positive")
    if clip_sigma is not None and not (clip_sigma >= 0.0 and math.isfinite(clip_sigma)):
        raise ValueError("localize_polyps: clip_sigma must be finite and not negative")
    depths, K, cam2world, N, H, W = depth_views("localize_polyps", depths, K, cam2world)
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda or labels.dtype != torch.uint8 or \
            tuple(labels.shape) != (N, 1, H, W) or labels.device != depths.device:
        raise ValueError(f"labels: expected a uint8 CUDA tensor of shape {(N, 1, H, W)} on {depths.device}, got "
                         f"{getattr(labels, 'dtype', None)} {tuple(getattr(labels, 'shape', ()))} on {getattr(labels, 'device', None)}")
    labels = labels.contiguous()
    L = num_labels
    check_sum_bounds(K, H, W, int(stride), f32(max_depth))
    nbytes = int(lib.colvo_localize_workspace_bytes(N, L))
    if nbytes == 0:
        raise ValueError(f"localize_polyps: unsupported N={N} (N <= 65535)")
    dev = depths.device
    records = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    stream = _lib.stream_ptr()
    geom = (N, H, W, int(stride), float(max_depth), L)

    def accumulate(bounds):
        _lib.call("colvo_localize_accumulate", depths, labels, K, *geom, bounds, records, stream)

    accumulate(None)
    if clip_sigma is not None:
        bounds = torch.empty(N, L, 2, device=dev, dtype=torch.float64)
        _lib.call("colvo_localize_bounds", records, N, L, float(clip_sigma), bounds, stream)
        accumulate(bounds)
    i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
    f64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float64)
    obs = (i32(N, L), i32(N, L), i32(N, L, 4), f64(N, L, 2), f64(N, L, 3), f64(N, L, 6), f64(N, L, 3))
    per = (i32(L), torch.empty(L, device=dev, dtype=torch.int64), i32(L), i32(L), f64(L, 3), f64(L, 6))
    stats = torch.empty(2, device=dev, dtype=torch.int64)
    _lib.call("colvo_localize_finish", records, cam2world, N, L, int(min_samples), *obs, *per, stats, stream)
    n_labelled, n_ignored = (int(v) for v in stats.tolist())
    # the square root is taken on the host, one correctly rounded math.sqrt per polyp: no device or vectorised sqrt enters a result
    trace = [(c[0] + c[3]) + c[5] for c in per[5].tolist()]
    radius = torch.tensor([math.sqrt(t) if t > 0.0 else (0.0 if t <= 0.0 else math.nan) for t in trace], dtype=torch.float64).to(dev)
    return PolypLocalization(*obs, *per, radius, n_labelled, n_ignored)


def localization_error(pred_positions, gt_positions, pred_cam2world=None, gt_cam2world=None, mode: str = "sim3") -> torch.Tensor:
    """Distance of every predicted polyp position [L,3] from its ground truth [L,3] -- the "e:" of the upstream reconstruction
    figure -- on the host in float64.  With both trajectories [M,4,4] the prediction is first mapped by
    (R, t, s) = evaluate.align_trajectory(pred_cam2world, gt_cam2world, mode): e_l = |g_l - (s R p_l + t)|.  Without trajectories
    the positions are compared as they are and mode must be "none".  A NaN position (a polyp never seen) gives a NaN error."""
    P = torch.as_tensor(pred_positions).detach().to("cpu", torch.float64)
    G = torch.as_tensor(gt_positions).detach().to("cpu", torch.float64)
    if P.dim() != 2 or P.shape[1] != 3 or P.shape != G.shape:
        raise ValueError(f"localization_error: expected two [L,3] position arrays, got {tuple(P.shape)} and {tuple(G.shape)}")
    if (pred_cam2world is None) != (gt_cam2world is None):
        raise ValueError("localization_error: give both trajectories, or neither")
    if pred_cam2world is None:
        if mode != "none":
            raise ValueError(f'localization_error: without trajectories there is nothing to align: mode must be "none", got {mode!r}')
        aligned = P
    else:
        R, t, s = align_trajectory(pred_cam2world, gt_cam2world, mode)
        aligned = s * (P @ R.t()) + t
    d = G - aligned
    return torch.sqrt((d * d).sum(dim=1))
