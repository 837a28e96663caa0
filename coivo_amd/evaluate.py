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

Trajectories (host, float64; camera-to-world [M,4,4], the convention of inference.integrate_trajectory)
  align_trajectory  Umeyama on the camera positions, mode "sim3" (default: monocular scale is unobservable), "se3" or "none",
                    with the reflection fix; returns (R, t, s) such that gt_position ~ s R pred_position + t.
  ate               RMSE of the position error after alignment.
  rpe               on E_i = (G_i^-1 G_{i+d})^-1 (P_i^-1 P_{i+d}), P's translations multiplied by the alignment scale:
                    (RMSE of |t(E_i)|, RMSE of the rotation angle arccos(clamp((tr R(E_i) - 1) / 2, -1, 1)) in degrees).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from . import inference

MIN_DEPTH = 0.1      # spec: MIN_DEPTH
MAX_DEPTH = 10.0     # spec: MAX_DEPTH
METRICS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
ALIGN_MODES = ("sim3", "se3", "none")


class DepthMetrics(NamedTuple):
    per_image: torch.Tensor     # [N,7] float64, columns in METRICS order
    scale: torch.Tensor         # [N]   float32, the median scale s
    n_valid: torch.Tensor       # [N]   int32


def _chk_depth(t, name: str, shape=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 1 or \
            (shape is not None and tuple(t.shape) != tuple(shape)):
        want = "[N,1,H,W]" if shape is None else str(tuple(shape))
        raise ValueError(f"{name}: expected a float32 CUDA tensor of shape {want}, got {getattr(t, 'dtype', None)} "
                         f"{tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
    return t.contiguous()


def depth_metrics(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None, *, min_depth: float = MIN_DEPTH,
                  max_depth: float = MAX_DEPTH, median_scaling: bool = True) -> DepthMetrics:
    """Per-image depth error measures (module docstring).  pred, gt [N,1,H,W] float32 on the GPU, mask bool / uint8 or None.
    Enqueues on the current stream and returns device tensors; no host synchronisation."""
    lib = _lib.load()
    pred = _chk_depth(pred, "pred")
    gt = _chk_depth(gt, "gt", pred.shape)
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
    N, _, H, W = pred.shape
    nbytes = int(lib.colvo_depth_metrics_workspace_bytes(N, H, W))
    if nbytes == 0:
        raise ValueError(f"depth_metrics: unsupported shape {tuple(pred.shape)} (N <= 65535, H*W < 2^30)")
    ws = torch.empty(nbytes, device=pred.device, dtype=torch.uint8)
    per_image = torch.empty(N, 7, device=pred.device, dtype=torch.float64)
    scale = torch.empty(N, device=pred.device, dtype=torch.float32)
    n_valid = torch.empty(N, device=pred.device, dtype=torch.int32)
    _lib.check(lib.colvo_depth_metrics(_lib.ptr(pred), _lib.ptr(gt), _lib.ptr(mask), N, H, W, float(min_depth), float(max_depth),
                                       int(bool(median_scaling)), _lib.ptr(ws), _lib.ptr(per_image), _lib.ptr(scale),
                                       _lib.ptr(n_valid), _lib.stream_ptr()), "colvo_depth_metrics")
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


# ---- trajectories (host, float64) ------------------------------------------------------------------------------------- #
def _poses(T, name: str) -> torch.Tensor:
    T = torch.as_tensor(T).detach().to("cpu", torch.float64)
    if T.dim() != 3 or tuple(T.shape[1:]) != (4, 4):
        raise ValueError(f"{name}: expected [M,4,4] camera-to-world transforms, got {tuple(T.shape)}")
    return T


def _pair(pred, gt) -> Tuple[torch.Tensor, torch.Tensor]:
    P, G = _poses(pred, "pred"), _poses(gt, "gt")
    if P.shape != G.shape:
        raise ValueError(f"pred {tuple(P.shape)} and gt {tuple(G.shape)} differ in length")
    return P, G


def align_trajectory(pred, gt, mode: str = "sim3") -> Tuple[torch.Tensor, torch.Tensor, float]:
    """Umeyama alignment of pred's camera positions to gt's: (R [3,3], t [3], s) minimising sum |g - (s R p + t)|^2, float64.
    mode "sim3" estimates the scale, "se3" fixes s = 1, "none" returns the identity."""
    if mode not in ALIGN_MODES:
        raise ValueError(f"align_trajectory: mode must be one of {ALIGN_MODES}, got {mode!r}")
    P, G = _pair(pred, gt)
    if mode == "none":
        return torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), 1.0
    x, y = P[:, :3, 3], G[:, :3, 3]
    mx, my = x.mean(dim=0), y.mean(dim=0)
    xc, yc = x - mx, y - my
    cov = yc.t() @ xc / x.shape[0]
    U, D, Vt = torch.linalg.svd(cov)
    S = torch.ones(3, dtype=torch.float64)
    if torch.det(U) * torch.det(Vt) < 0:                 # reflection fix: a proper rotation
        S[2] = -1.0
    R = U @ torch.diag(S) @ Vt
    s = 1.0
    if mode == "sim3":
        var = float((xc * xc).sum(dim=1).mean())
        s = float((D * S).sum()) / var if var > 0 else 1.0
    t = my - s * (R @ mx)
    return R, t, s


def ate(pred, gt, mode: str = "sim3") -> float:
    """Absolute trajectory error: RMSE of the camera-position error after align_trajectory(pred, gt, mode)."""
    P, G = _pair(pred, gt)
    R, t, s = align_trajectory(P, G, mode)
    err = G[:, :3, 3] - (s * (P[:, :3, 3] @ R.t()) + t)
    return math.sqrt(float((err * err).sum(dim=1).mean()))


def _rel(T: torch.Tensor, delta: int) -> torch.Tensor:
    return torch.linalg.inv(T[:-delta]) @ T[delta:]


def rpe(pred, gt, delta: int = 1, mode: str = "sim3") -> Tuple[float, float]:
    """Relative pose error over `delta` frames: (RMSE of the translation error, RMSE of the rotation error in degrees) of
    E_i = (G_i^-1 G_{i+delta})^-1 (P_i^-1 P_{i+delta}), pred's translations scaled by align_trajectory's s."""
    P, G = _pair(pred, gt)
    if delta < 1 or delta >= P.shape[0]:
        raise ValueError(f"rpe: delta must be in [1, {P.shape[0] - 1}], got {delta}")
    _, _, s = align_trajectory(P, G, mode)
    P = P.clone()
    P[:, :3, 3] *= s
    E = torch.linalg.inv(_rel(G, delta)) @ _rel(P, delta)
    te = (E[:, :3, 3] ** 2).sum(dim=1)
    cos = ((E[:, 0, 0] + E[:, 1, 1] + E[:, 2, 2] - 1.0) / 2.0).clamp(-1.0, 1.0)
    ang = torch.rad2deg(torch.arccos(cos))
    return math.sqrt(float(te.mean())), math.sqrt(float((ang * ang).mean()))


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
        G = _poses(gt_cam2world, "gt_cam2world")
        if G.shape[0] != n:
            raise ValueError(f"evaluate_sequence: gt_cam2world has {G.shape[0]} poses for {n} frames")
        a = ate(traj, G, mode=align)
        r = rpe(traj, G, delta=1, mode=align)
    return SequenceEvaluation(depths, rel, traj, dm, summary, a, r)
