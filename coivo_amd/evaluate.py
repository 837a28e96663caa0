"""Evaluation: depth error measures with per-image median scaling, and trajectory error.

The measures behind the upstream README's claims (README.md: "superiority in depth and pose estimation", a trajectory "close
to the ground truth ... less drift or jitter"), in the Eigen et al. / Monodepth2 `compute_errors` convention.

Depth (csrc/evaluate.hip, one native call; these definitions are the contract)
  inputs   pred, gt: float32 [N,1,H,W] of the same shape (resizing a prediction to the ground truth's resolution is the
           caller's job: F.interpolate); optional mask: bool or uint8 [N,1,H,W].
  valid    a pixel is valid iff gt > min_depth, gt < max_depth and mask != 0 (when a mask is given); NaN and +-inf in gt
           therefore fall out.  pred must be finite and positive (DepthNet's output always is).
  median   over the valid pixels of one image, the LOWER median: the element of rank (n-1)//2 in ascending order
           (torch.median / torch.nanmedian semantics), exact to the bit.
  scaling  float32: s = med(gt) / med(pred) (IEEE-correctly-rounded division), p = min(max(s * pred, min_depth), max_depth).
           median_scaling=False: s = 1, the clamp still applies.
  metrics  means over the valid pixels, each per-pixel term in float32, the sums of an image accumulated in float64:
             abs_rel   mean |g - p| / g             sq_rel    mean (g - p)^2 / g
             rmse      sqrt(mean (g - p)^2)         rmse_log  sqrt(mean (ln g - ln p)^2)
             a1/a2/a3  fraction with max(g/p, p/g) < 1.25, 1.5625, 1.953125 (float32 quotients: exact counts)
  empty    an image with n = 0 valid pixels gets NaN metrics, s = NaN and n_valid = 0.
  summary  the mean of the per-image metrics over the images with n_valid > 0 (Monodepth's convention); skipped images are
           counted.
  determinism  two calls on the same inputs return the same bits (integer atomics only; fixed-order float reductions).

Trajectories      coivo_amd/trajectory.py    (host, float64: align_trajectory, ate, rpe)
Point clouds      coivo_amd/cloud_eval.py    (csrc/cloud.hip: nearest_neighbors, transform_cloud, cloud_metrics, reconstruction_metrics)
Registration      coivo_amd/registration.py  (csrc/register.hip: register_clouds, register_accumulate)
Surfaces          coivo_amd/surface_eval.py  (csrc/surface.hip: point_to_surface, surface_metrics, surface_reconstruction_metrics)
Every public name of the four is re-exported here."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from . import inference
from ._args import MAX_DEPTH, device_f32, frames_shape
from .cloud_eval import (CLOUD_STATS, MAX_THRESHOLDS, CloudMetrics, CloudNN, cloud_metrics, metrics_from_stats, nearest_neighbors,
                         reconstruction_metrics, transform_cloud)
from .fusion import Mesh, Meshing
from .registration import (REGISTER_HISTORY, REGISTER_METRICS, REGISTER_MODES, REGISTER_NOT_PD, REGISTER_OK, REGISTER_REVERTED,
                           REGISTER_TOO_FEW, Registration, RegistrationResult, register_accumulate, register_clouds)
from .surface_eval import (MAX_SURFACE_PAIRS, SURFACE_STATS, SurfaceMetrics, SurfaceNN, point_to_surface, surface_metrics,
                           surface_reconstruction_metrics)
from .topology import clean_mesh, mesh_topology
from .trajectory import ALIGN_MODES, align_trajectory, ate, poses, rpe

MIN_DEPTH = 0.1      # spec: MIN_DEPTH
METRICS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")


class DepthMetrics(NamedTuple):
    per_image: torch.Tensor     # [N,7] float64, columns in METRICS order
    scale: torch.Tensor         # [N]   float32, the median scale s
    n_valid: torch.Tensor       # [N]   int32


def depth_metrics(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None, *, min_depth: float = MIN_DEPTH,
                  max_depth: float = MAX_DEPTH, median_scaling: bool = True) -> DepthMetrics:
    """Per-image depth error measures (module docstring).  pred, gt [N,1,H,W] float32 on the GPU, mask bool / uint8 or None.
    Enqueues on the current stream and returns device tensors; no host synchronisation."""
    who = "depth_metrics"
    lib = _lib.load()
    N, H, W = frames_shape(who, "pred", pred)
    pred = device_f32(who, "pred", pred, (N, 1, H, W))
    gt = device_f32(who, "gt", gt, (N, 1, H, W))
    if gt.device != pred.device:
        raise ValueError(f"gt is on {gt.device}, pred on {pred.device}")
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dtype not in (torch.bool, torch.uint8) or \
                tuple(mask.shape) != tuple(pred.shape) or mask.device != pred.device:
            raise ValueError(f"mask: expected a bool or uint8 tensor of shape {tuple(pred.shape)} on {pred.device}, got "
                             f"{getattr(mask, 'dtype', None)} {tuple(getattr(mask, 'shape', ()))} on {getattr(mask, 'device', None)}")
        mask = mask.contiguous()
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
    if not min_depth < max_depth:
        raise ValueError(f"depth_metrics: min_depth {min_depth} must be below max_depth {max_depth}")
    nbytes = int(lib.colvo_depth_metrics_workspace_bytes(N, H, W))
    if nbytes == 0:
        raise ValueError(f"depth_metrics: unsupported shape {tuple(pred.shape)} (N <= 65535, H*W < 2^30)")
    ws = torch.empty(nbytes, device=pred.device, dtype=torch.uint8)
    per_image = torch.empty(N, 7, device=pred.device, dtype=torch.float64)
    scale = torch.empty(N, device=pred.device, dtype=torch.float32)
    n_valid = torch.empty(N, device=pred.device, dtype=torch.int32)
    _lib.call("colvo_depth_metrics", pred, gt, mask, N, H, W, float(min_depth), float(max_depth), int(bool(median_scaling)), ws,
              per_image, scale, n_valid, _lib.stream_ptr())
    return DepthMetrics(per_image, scale, n_valid)


def summarize(*results: DepthMetrics) -> dict:
    """Dataset summary of one or more depth_metrics results (a validation loop's batches): the mean of every measure over the
    images with n_valid > 0, "images" (how many were averaged) and "skipped" (how many had no valid pixel).  Reads back."""
    if not results:
        raise ValueError("summarize: no results")
    per_image = torch.cat([r.per_image for r in results]).cpu()
    n_valid = torch.cat([r.n_valid for r in results]).cpu()
    keep = n_valid > 0
    used = int(keep.sum())
    means = per_image[keep].mean(dim=0) if used else torch.full((7,), math.nan, dtype=torch.float64)
    out = {name: float(means[i]) for i, name in enumerate(METRICS)}
    out["images"] = used
    out["skipped"] = int(n_valid.numel()) - used
    return out


# ---- one sequence ------------------------------------------------------------------------------------------------------ #
class SequenceEvaluation(NamedTuple):
    depths: torch.Tensor                    # [N+1,1,H,W]
    rel_poses: torch.Tensor                 # [N,6]     frame k -> frame k+1
    cam2world: torch.Tensor                 # [N+1,4,4] float64, CPU (inference.integrate_trajectory)
    depth: Optional[DepthMetrics]           # with gt_depths
    summary: Optional[dict]                 # summarize(depth), with gt_depths
    ate: Optional[float]                    # with gt_cam2world
    rpe: Optional[Tuple[float, float]]      # with gt_cam2world: (translation, rotation in degrees), delta = 1


@torch.no_grad()
def evaluate_sequence(depth_net, pose_net, frames: torch.Tensor, *, gt_depths: Optional[torch.Tensor] = None,
                      gt_cam2world=None, chunk: int = 16, align: str = "sim3", **depth_kw) -> SequenceEvaluation:
    """frames [N+1,3,H,W] of one sequence -> the networks' depths and relative poses (run as inference.reconstruct_sequence
    runs them), the integrated trajectory, and whichever measures the given ground truth allows: depth_metrics(depths,
    gt_depths, **depth_kw) and its summary with gt_depths [N+1,1,H,W] (the depths' resolution); ate and rpe under `align` with
    gt_cam2world [N+1,4,4]."""
    n = frames.shape[0]
    if n < 2:
        raise ValueError("evaluate_sequence: need at least two frames")
    depths, rel = inference.run_networks(depth_net, pose_net, frames, chunk=chunk)
    traj = inference.integrate_trajectory(rel)
    dm = summary = a = r = None
    if gt_depths is not None:
        dm = depth_metrics(depths, gt_depths, **depth_kw)
        summary = summarize(dm)
    if gt_cam2world is not None:
        G = poses(gt_cam2world, "gt_cam2world")
        if G.shape[0] != n:
            raise ValueError(f"evaluate_sequence: gt_cam2world has {G.shape[0]} poses for {n} frames")
        a = ate(traj, G, mode=align)
        r = rpe(traj, G, delta=1, mode=align)
    return SequenceEvaluation(depths, rel, traj, dm, summary, a, r)

