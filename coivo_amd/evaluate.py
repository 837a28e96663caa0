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

Point clouds (csrc/cloud.hip; these definitions are the contract, include/colvo.h says the same)
  inputs    a query cloud Q [N,3] and a reference cloud P [M,3], float32 on the GPU, and max_dist > 0.  The arithmetic is
            pinned: float32, every operation individually rounded (no FMA contraction).
  valid     a point is valid iff its three coordinates are finite.  Invalid points take no part on either side and are counted.
  d2(q,p)   ((dx*dx + dy*dy) + dz*dz) with dx = qx - px, dy = qy - py, dz = qz - pz, in that association.
  md2       float32(max_dist) * float32(max_dist), rounded once.
  reach     p is within reach of q iff d2(q,p) < md2; the comparison is strict.
  dist2[q]  the minimum of d2 over the valid p within reach; nearest[q] the smallest original index p attaining it.  No point
            within reach, or q invalid: dist2[q] = md2 and nearest[q] = -1.  dist[q] = sqrtf(dist2[q]), correctly rounded.
  stats     exact integers over the query cloud (CLOUD_STATS order): n_valid; n_reached, the valid queries with something within
            reach; for each of up to 8 non-descending thresholds tau_k <= max_dist the valid queries with
            dist2 < float32(tau_k) * float32(tau_k); the sum over the valid queries of quantum(dist) = uint32(rint(dist * s)) with
            s = float32(2^20) / float32(max_dist) (one IEEE division, the product rounded to float32, ties to even); and, a cost
            figure, the reference points examined.  The mean truncated distance is double(sum) / (double(s) * n_valid).
  determinism  every output bit follows from the inputs alone -- the minimum does not depend on the order it is taken in and the
            sums are integers -- not from the schedule, the stream or the order in which atomics land.
  transform out = ((s * ((r0*x + r1*y) + r2*z)) + t) per axis, R, t, s rounded to float32, pinned as above.
  measures  cloud_metrics(pred, gt): accuracy = mean truncated distance pred -> gt, completeness = the same gt -> pred, chamfer
            their mean; per threshold precision = the fraction of the valid pred points with dist2 < tau^2, recall = that of the
            valid gt points, fscore = 2 p r / (p + r), 0 when both are 0.  A side without a valid point gives NaN for the
            measures that divide by its count.  The clouds are compared as given (surfaces: point_to_surface, below), after the
            optional Sim(3) of align_trajectory and, with a Registration policy, its refinement by register_clouds (below).
  limits    N, M < 2^30; max_dist finite and positive with a finite positive float32 square; at most 8 thresholds.

Surfaces (csrc/surface.hip; the contract is include/colvo.h colvo_surface_*, replica tests/surface_ref.py)
  point_to_surface(points, mesh)  for every point the distance to the nearest point OF THE TRIANGLES of a mesh within max_dist, the
            face, the nearest point and the side; float64 on widened float32 coordinates in a written association; dead faces as
            mesh_topology's, faces with a coordinate that is not finite skipped; the least (d2, face) wins.  The first twelve
            statistics are CLOUD_STATS, so metrics_from_stats serves both.
  surface_metrics(pred, gt)  cloud_metrics' measures with each side's used vertices scored against the other side's triangles, and the
            shares of pred vertices in front of and behind the ground-truth surface.  surface_reconstruction_metrics meshes the
            ground-truth depths with the pred side's policy.  Not here: registration against faces, sampling a surface by area, a
            signed-distance volume, any use in training.

Registration (csrc/register.hip; the contract is include/colvo.h colvo_register_*)
  register_clouds(source, target)  a few Gauss-Newton steps of point-to-plane ICP (metric "plane", the default; "point" is point to
            point, which crawls on a tube: the points slide along the wall) that refine a Sim(3) ("sim3") or SE(3) ("se3") moving
            source onto target, x' = s R x + t.  Every iteration is one nearest-neighbour pass of the transformed source over the
            target's index -- nearest_neighbors' own walk, rule for rule -- and 37 float64 sums in a fixed order; the 6x6 / 7x7 step is
            solved on the device.  No read-back and no host synchronisation; identical bits on every call and stream.
  status    REGISTER_OK; REGISTER_TOO_FEW (fewer than min_pairs pairs used), REGISTER_NOT_PD (a surface with a free motion: an exact
            cylinder) and REGISTER_REVERTED (the final truncated cost per valid point is above the initial one) return the initial
            state to the bit.  There is no convergence test and no early exit.
"""
from __future__ import annotations

import math
import ctypes
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from . import inference
from ._args import f32 as _f32, int_range
from .fusion import Mesh, Meshing
from .topology import _mesh_arrays, clean_mesh, mesh_topology

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


# ---- point clouds (csrc/cloud.hip) ---------------------------------------------------------------------------------------- #
CLOUD_STATS = ("n_valid", "n_reached") + tuple(f"under_{k}" for k in range(8)) + ("sum_quanta", "examined")
MAX_THRESHOLDS = 8


class CloudNN(NamedTuple):
    dist: torch.Tensor          # [N] float32: sqrtf(dist2)
    dist2: torch.Tensor         # [N] float32: squared distance to the nearest reference point within reach, else md2
    nearest: torch.Tensor       # [N] int32: its index in the reference cloud, else -1
    stats: torch.Tensor         # [12] int64 on the device, CLOUD_STATS order
    max_dist: float             # as float32
    thresholds: Tuple[float, ...]   # as float32


class _CloudMetricsFields(NamedTuple):
    accuracy: float             # mean truncated distance pred -> gt
    completeness: float         # mean truncated distance gt -> pred
    chamfer: float              # (accuracy + completeness) / 2
    precision: Tuple[float, ...]    # per threshold
    recall: Tuple[float, ...]
    fscore: Tuple[float, ...]
    n_pred: int                 # valid pred points
    n_gt: int                   # valid gt points
    n_pred_reached: int         # ... with a gt point within max_dist
    n_gt_reached: int           # ... with a pred point within max_dist
    pred_to_gt: CloudNN
    gt_to_pred: CloudNN


class CloudMetrics(_CloudMetricsFields):
    """The twelve fields above -- it still unpacks into twelve -- and, behind them, `registration`: with a Registration policy the
    RegistrationResult whose transform the clouds were compared under, else None."""
    registration = None         # Optional[RegistrationResult]

    def __new__(cls, *args, registration=None, **kw):
        self = super().__new__(cls, *args, **kw)
        self.registration = registration
        return self

    def _replace(self, **kw):
        registration = kw.pop("registration", self.registration)
        return type(self)(*super()._replace(**kw), registration=registration)


def _chk_cloud(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name}: expected a float32 CUDA tensor of shape [N,3], got {getattr(t, 'dtype', None)} "
                         f"{tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
    return t.contiguous()


def _chk_reach(who: str, max_dist, thresholds) -> Tuple[float, Tuple[float, ...]]:
    """max_dist and the thresholds as float32 values, refused as the library refuses them."""
    try:
        md = _f32(max_dist)
    except (OverflowError, TypeError, ValueError):
        md = math.nan
    md2 = _f32(md * md) if math.isfinite(md) else math.nan
    if not (md > 0.0 and math.isfinite(md) and md2 >= 2.0 ** -126 and math.isfinite(md2)):
        raise ValueError(f"{who}: max_dist must be finite and positive with a finite positive float32 square, got {max_dist!r}")
    try:
        th = tuple(_f32(t) for t in thresholds)
    except (OverflowError, TypeError, ValueError):
        raise ValueError(f"{who}: thresholds must be numbers, got {thresholds!r}") from None
    if len(th) > MAX_THRESHOLDS:
        raise ValueError(f"{who}: at most {MAX_THRESHOLDS} thresholds, got {len(th)}")
    for k, t in enumerate(th):
        if not (t > 0.0 and t <= md and (k == 0 or t >= th[k - 1])):
            raise ValueError(f"{who}: thresholds must be positive, non-descending and at most max_dist {md}, got {th}")
    return md, th


def nearest_neighbors(query: torch.Tensor, ref: torch.Tensor, *, max_dist: float, thresholds: Sequence[float] = ()) -> CloudNN:
    """For every point of query [N,3] the nearest point of ref [M,3] closer than max_dist, and the exact statistics of the
    module docstring (float32 clouds on the GPU).  Enqueues on the current stream and returns device tensors; no host
    synchronisation."""
    lib = _lib.load()
    query = _chk_cloud(query, "query")
    ref = _chk_cloud(ref, "ref")
    if ref.device != query.device:
        raise ValueError(f"ref is on {ref.device}, query on {query.device}")
    md, th = _chk_reach("nearest_neighbors", max_dist, thresholds)
    N, M = query.shape[0], ref.shape[0]
    nbytes = int(lib.colvo_cloud_workspace_bytes(N, M))
    if nbytes == 0:
        raise ValueError(f"nearest_neighbors: {N} query and {M} reference points: each cloud must hold fewer than 2^30")
    dev = query.device
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    dist = torch.empty(N, device=dev, dtype=torch.float32)
    dist2 = torch.empty(N, device=dev, dtype=torch.float32)
    nearest = torch.empty(N, device=dev, dtype=torch.int32)
    stats = torch.empty(len(CLOUD_STATS), device=dev, dtype=torch.int64)
    tau = (ctypes.c_float * MAX_THRESHOLDS)(*th)
    stream = _lib.stream_ptr()
    _lib.check(lib.colvo_cloud_index_build(_lib.ptr(ref), M, md, _lib.ptr(ws), stream), "colvo_cloud_index_build")
    _lib.check(lib.colvo_cloud_query(_lib.ptr(query), N, M, md, ctypes.addressof(tau), len(th), _lib.ptr(ws), _lib.ptr(dist),
                                     _lib.ptr(dist2), _lib.ptr(nearest), _lib.ptr(stats), stream), "colvo_cloud_query")
    return CloudNN(dist, dist2, nearest, stats, md, th)


def transform_cloud(points: torch.Tensor, R, t, s) -> torch.Tensor:
    """out = ((s * ((r0*x + r1*y) + r2*z)) + t) per axis in pinned float32 (module docstring): the Sim(3) of align_trajectory,
    rounded to float32, applied to points [N,3] on the GPU."""
    lib = _lib.load()
    points = _chk_cloud(points, "points")
    R = torch.as_tensor(R).detach().to("cpu", torch.float64)
    t = torch.as_tensor(t).detach().to("cpu", torch.float64)
    if tuple(R.shape) != (3, 3) or tuple(t.shape) != (3,):
        raise ValueError(f"transform_cloud: expected R [3,3] and t [3], got {tuple(R.shape)} and {tuple(t.shape)}")
    rts = (ctypes.c_float * 13)(*([float(v) for v in R.reshape(-1)] + [float(v) for v in t] + [float(s)]))
    out = torch.empty_like(points)
    _lib.check(lib.colvo_cloud_transform(_lib.ptr(points), points.shape[0], ctypes.addressof(rts), _lib.ptr(out),
                                         _lib.stream_ptr()), "colvo_cloud_transform")
    return out


def _mean_distance(stats: Sequence[int], max_dist: float) -> float:
    """double(sum of quanta) / (double(s) * n_valid), s = float32(2^20) / float32(max_dist)."""
    n = int(stats[0])
    if n == 0:
        return math.nan
    # s: the float64 quotient of two float32 values, rounded to float32, is the correctly rounded float32 quotient (53 >= 2 * 24 + 2)
    return float(int(stats[10])) / (_f32(1048576.0 / _f32(max_dist)) * n)


def metrics_from_stats(pred_stats: Sequence[int], gt_stats: Sequence[int], max_dist: float, n_thresholds: int) -> dict:
    """The measures of cloud_metrics from the two directions' integer statistics (CLOUD_STATS order; pred_stats: pred -> gt,
    gt_stats: gt -> pred) and max_dist as float32.  Host arithmetic only."""
    acc, comp = _mean_distance(pred_stats, max_dist), _mean_distance(gt_stats, max_dist)
    n_pred, n_gt = int(pred_stats[0]), int(gt_stats[0])
    precision, recall, fscore = [], [], []
    for k in range(n_thresholds):
        p = int(pred_stats[2 + k]) / n_pred if n_pred else math.nan
        r = int(gt_stats[2 + k]) / n_gt if n_gt else math.nan
        precision.append(p)
        recall.append(r)
        fscore.append(0.0 if p == 0.0 and r == 0.0 else 2.0 * p * r / (p + r))
    return dict(accuracy=acc, completeness=comp, chamfer=0.5 * (acc + comp), precision=tuple(precision), recall=tuple(recall),
                fscore=tuple(fscore), n_pred=n_pred, n_gt=n_gt, n_pred_reached=int(pred_stats[1]), n_gt_reached=int(gt_stats[1]))


def cloud_metrics(pred: torch.Tensor, gt: torch.Tensor, *, max_dist: float, thresholds: Sequence[float],
                  transform=None, register: Optional["Registration"] = None, gt_normals: Optional[torch.Tensor] = None) -> CloudMetrics:
    """Accuracy, completeness, Chamfer distance and per-threshold precision / recall / F-score of pred [N,3] against gt [M,3]
    (module docstring), from one search each way.  transform = (R, t, s), as align_trajectory returns it, is applied to pred
    first.  The per-point results of both searches are returned (pred_to_gt.dist colours pred by its error).  Reads the 24
    statistics back once, at the end.
    With a Registration policy `register`, transform (the identity without one) is the start of register_clouds(pred, gt,
    target_normals=gt_normals), whose refined transform -- one more read-back of 13 values -- is what the clouds are compared under; the
    RegistrationResult is `.registration`.  The policy's max_dist None means this call's max_dist.  A registration that froze or
    was reverted returns its start, so the measures are then those of the plain call.  register=None: every bit as without it."""
    if register is not None:
        _chk_registration("cloud_metrics", register)
    pred = _chk_cloud(pred, "pred")
    gt = _chk_cloud(gt, "gt")
    md, th = _chk_reach("cloud_metrics", max_dist, thresholds)
    registration = None
    if register is not None:
        kw = register._asdict()
        if kw["max_dist"] is None:
            kw["max_dist"] = md
        registration = register_clouds(pred, gt, target_normals=gt_normals, init=transform, **kw)
        transform = registration.transform()
    if transform is not None:
        R, t, s = transform
        pred = transform_cloud(pred, R, t, s)
    a = nearest_neighbors(pred, gt, max_dist=md, thresholds=th)
    b = nearest_neighbors(gt, pred, max_dist=md, thresholds=th)
    both = torch.stack([a.stats, b.stats]).tolist()
    return CloudMetrics(**metrics_from_stats(both[0], both[1], md, len(th)), pred_to_gt=a, gt_to_pred=b, registration=registration)


def reconstruction_metrics(pred_cloud, pred_cam2world, gt_depths: torch.Tensor, K: torch.Tensor, gt_cam2world, *,
                           voxel_size: float, max_dist: Optional[float] = None, thresholds: Optional[Sequence[float]] = None,
                           align: str = "sim3", stride: int = 1, max_depth: float = MAX_DEPTH, min_obs: int = 1,
                           register: Optional["Registration"] = None) -> CloudMetrics:
    """A reconstruction against ground truth: pred_cloud (an inference.FusedCloud or [M,3] points) in the frame of the
    trajectory pred_cam2world [N,4,4], against the cloud fused from gt_depths [N,1,H,W] along gt_cam2world [N,4,4] by
    inference.fuse_point_cloud at the same voxel_size (stride, max_depth, min_obs as there).  pred is moved by
    align_trajectory(pred_cam2world, gt_cam2world, align) and the two are compared by cloud_metrics.
    max_dist defaults to 4 * voxel_size and thresholds to (voxel_size, 2 * voxel_size): choices, not tuned.  The comparison is point to
    point: it scores samples, and two samplings of one surface lie a fraction of a voxel apart; surface_reconstruction_metrics
    compares the meshed surfaces instead (point to surface).  The alignment is the trajectories' -- a fit to N camera centres, which carries the predicted
    trajectory's drift into the score -- unless a Registration policy `register` is given: the trajectories' alignment is then the
    start of register_clouds(pred, ground truth) (point to plane by default, against the normals inference.cloud_normals gives the
    ground-truth cloud from the very depths, stride and trajectory it was fused with), the refined transform is what the clouds are
    compared under, and the RegistrationResult is the result's `.registration`."""
    if register is not None:
        _chk_registration("reconstruction_metrics", register)
    points = pred_cloud.points if isinstance(pred_cloud, inference.FusedCloud) else pred_cloud
    points = _chk_cloud(points, "pred_cloud")
    G = _poses(gt_cam2world, "gt_cam2world")
    G32 = G.to(gt_depths.device, torch.float32)
    gt = inference.fuse_point_cloud(gt_depths, K, G32, voxel_size=voxel_size, stride=stride, max_depth=max_depth, min_obs=min_obs)
    R, t, s = align_trajectory(pred_cam2world, G, align)
    vs = _f32(voxel_size)
    gt_normals = None
    if register is not None and register.metric == "plane":
        gt_normals = inference.cloud_normals(gt, gt_depths, K, G32, stride=stride, max_depth=max_depth).normals
    return cloud_metrics(points, gt.points, max_dist=4.0 * vs if max_dist is None else max_dist,
                         thresholds=(vs, 2.0 * vs) if thresholds is None else thresholds,
                         transform=None if align == "none" else (R, t, s), register=register, gt_normals=gt_normals)


# ---- registration (csrc/register.hip) ------------------------------------------------------------------------------------- #
REGISTER_MODES = ("se3", "sim3")          # the C ABI's 0 and 1
REGISTER_METRICS = ("plane", "point")
REGISTER_OK, REGISTER_TOO_FEW, REGISTER_NOT_PD, REGISTER_REVERTED = 0, 1, 2, 3
REGISTER_HISTORY = ("n_valid", "n_reached", "n_used", "cost", "sum_r2")


class Registration(NamedTuple):
    """The policy of register_clouds.  Choices, not tuned values: sim3 because monocular scale is unobservable, plane because point
    to point crawls on a tube, 20 iterations where the test scenes converge in 3, a damping that only keeps a well-posed system
    away from a zero pivot, and 64 pairs as the least a 7-parameter fit should rest on."""
    mode: str = "sim3"              # "sim3" or "se3" (s is then left as given)
    metric: str = "plane"           # "plane" (needs the target's normals) or "point"
    iterations: int = 20            # 1 .. 64 Gauss-Newton steps; there is no early exit
    max_dist: Optional[float] = None    # reach of the nearest-neighbour search; None: the metrics' own max_dist
    damping: float = 1e-9           # H_kk <- H_kk + damping * H_kk
    min_pairs: int = 64             # fewer used pairs freeze the state (REGISTER_TOO_FEW)


class RegistrationResult(NamedTuple):
    R: torch.Tensor                 # [3,3] float64 on the device
    t: torch.Tensor                 # [3]   float64
    s: torch.Tensor                 # []    float64: x' = s R x + t
    history: torch.Tensor           # [iterations+1,5] float64: REGISTER_HISTORY of every evaluation
    status: torch.Tensor            # []    int32: REGISTER_*
    normal_matrix: torch.Tensor     # [7,7] float64: sum J^T J of the final evaluation (v, omega, sigma), undamped

    def transform(self) -> Tuple[torch.Tensor, torch.Tensor, float]:
        """(R [3,3], t [3], s) on the host, float64, as align_trajectory returns it and cloud_metrics(transform=...) and
        transform_cloud take it.  The one read-back."""
        v = torch.cat([self.R.reshape(9), self.t.reshape(3), self.s.reshape(1)]).to("cpu")
        return v[:9].reshape(3, 3).clone(), v[9:12].clone(), float(v[12])


def _chk_registration(who: str, policy) -> "Registration":
    if not isinstance(policy, Registration):
        raise ValueError(f"{who}: register must be a Registration or None, got {type(policy).__name__}")
    if policy.mode not in REGISTER_MODES:
        raise ValueError(f"{who}: mode must be one of {REGISTER_MODES}, got {policy.mode!r}")
    if policy.metric not in REGISTER_METRICS:
        raise ValueError(f"{who}: metric must be one of {REGISTER_METRICS}, got {policy.metric!r}")
    it = policy.iterations
    if isinstance(it, bool) or not isinstance(it, int) or not 1 <= it <= 64:
        raise ValueError(f"{who}: iterations must be an int in 1 .. 64, got {it!r}")
    mp = policy.min_pairs
    if isinstance(mp, bool) or not isinstance(mp, int) or not 1 <= mp < 2 ** 31:
        raise ValueError(f"{who}: min_pairs must be an int >= 1, got {mp!r}")
    try:
        d = float(policy.damping)
    except (TypeError, ValueError):
        d = math.nan
    if not (d >= 0.0 and math.isfinite(d)):
        raise ValueError(f"{who}: damping must be finite and >= 0, got {policy.damping!r}")
    if policy.max_dist is not None:
        _chk_reach(who, policy.max_dist, ())
    return policy


def _register_inputs(who: str, source, target, target_normals, init, pivot, max_dist, metric):
    """Checked inputs of the registration calls: (source, target, normals or None, state [13] float64 on the device, pivot [3] float32
    on the device, max_dist as float32, index workspace with the target's index enqueued)."""
    source = _chk_cloud(source, "source")
    target = _chk_cloud(target, "target")
    dev = source.device
    if target.device != dev:
        raise ValueError(f"{who}: target is on {target.device}, source on {dev}")
    if metric not in REGISTER_METRICS:
        raise ValueError(f"{who}: metric must be one of {REGISTER_METRICS}, got {metric!r}")
    if target_normals is None:
        if metric == "plane":
            raise ValueError(f"{who}: metric 'plane' needs target_normals [M,3] (inference.cloud_normals(...).normals)")
    else:
        target_normals = _chk_cloud(target_normals, "target_normals")
        if target_normals.shape != target.shape or target_normals.device != dev:
            raise ValueError(f"{who}: target_normals {tuple(target_normals.shape)} on {target_normals.device} do not match target "
                             f"{tuple(target.shape)} on {dev}")
    md, _ = _chk_reach(who, max_dist, ())
    if init is None:
        state = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], dtype=torch.float64)
    else:
        try:
            R, t, s = init
            R = torch.as_tensor(R).detach().to("cpu", torch.float64)
            t = torch.as_tensor(t).detach().to("cpu", torch.float64)
            s = torch.as_tensor(s).detach().to("cpu", torch.float64)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"{who}: init must be (R [3,3], t [3], s), as align_trajectory returns it") from None
        if tuple(R.shape) != (3, 3) or tuple(t.shape) != (3,) or s.numel() != 1:
            raise ValueError(f"{who}: init must be (R [3,3], t [3], s), got shapes {tuple(R.shape)}, {tuple(t.shape)}, {tuple(s.shape)}")
        state = torch.cat([R.reshape(9), t, s.reshape(1)])
        if not bool(torch.isfinite(state).all()):
            raise ValueError(f"{who}: init must be finite")
    M = target.shape[0]
    if pivot is None:
        # the centre of the box of the target's finite points: amin / amax are exact and order-free; no read-back
        if M == 0:
            pv = torch.zeros(3, device=dev, dtype=torch.float32)
        else:
            fin = torch.isfinite(target).all(dim=1, keepdim=True)
            lo = torch.where(fin, target, torch.full_like(target, math.inf)).amin(dim=0)
            hi = torch.where(fin, target, torch.full_like(target, -math.inf)).amax(dim=0)
            pv = 0.5 * lo + 0.5 * hi
            pv = torch.where(torch.isfinite(pv), pv, torch.zeros_like(pv))
    else:
        try:
            pv = torch.as_tensor(pivot).detach().to(torch.float32).reshape(-1)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"{who}: pivot must be three numbers") from None
        if pv.numel() != 3:
            raise ValueError(f"{who}: pivot must be three numbers, got {pv.numel()}")
        pv = pv.to(dev).contiguous()
    lib = _lib.load()
    nbytes = int(lib.colvo_cloud_workspace_bytes(0, M))
    if nbytes == 0 or int(lib.colvo_register_scratch_bytes(source.shape[0])) == 0:
        raise ValueError(f"{who}: {source.shape[0]} source and {M} target points: each cloud must hold fewer than 2^30")
    index = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    _lib.check(lib.colvo_cloud_index_build(_lib.ptr(target), M, md, _lib.ptr(index), _lib.stream_ptr()), "colvo_cloud_index_build")
    return source, target, target_normals, state.to(dev), pv, md, index


def register_accumulate(source: torch.Tensor, target: torch.Tensor, *, target_normals: Optional[torch.Tensor] = None, init=None,
                        pivot=None, max_dist: float, metric: str = "plane") -> Tuple[torch.Tensor, torch.Tensor]:
    """One evaluation of the registration's sums at the state `init` (contract: include/colvo.h colvo_register_accumulate):
    (sums [40] float64: the 28 upper-triangle entries of sum J^T J, the 7 of sum J^T r, the truncated cost C, sum r^2, three zeros;
    counts [4] int64: n_valid, n_reached, n_used, 0), on the device.  The test hook of register_clouds."""
    who = "register_accumulate"
    source, target, normals, state, pv, md, index = _register_inputs(who, source, target, target_normals, init, pivot, max_dist, metric)
    lib = _lib.load()
    dev = source.device
    N, M = source.shape[0], target.shape[0]
    ws = torch.empty(int(lib.colvo_register_scratch_bytes(N)), device=dev, dtype=torch.uint8)
    sums = torch.empty(40, device=dev, dtype=torch.float64)
    counts = torch.empty(4, device=dev, dtype=torch.int64)
    _lib.check(lib.colvo_register_accumulate(_lib.ptr(source), N, _lib.ptr(target), _lib.ptr(normals), M, md, _lib.ptr(index),
                                             _lib.ptr(state), _lib.ptr(pv), REGISTER_METRICS.index(metric), _lib.ptr(ws),
                                             _lib.ptr(sums), _lib.ptr(counts), _lib.stream_ptr()), "colvo_register_accumulate")
    return sums, counts


def register_clouds(source: torch.Tensor, target: torch.Tensor, *, target_normals: Optional[torch.Tensor] = None, init=None,
                    pivot=None, max_dist: float, mode: str = "sim3", metric: str = "plane", iterations: int = 20,
                    damping: float = 1e-9, min_pairs: int = 64) -> RegistrationResult:
    """Register source [N,3] onto target [M,3] (float32 clouds on the GPU): `iterations` Gauss-Newton steps of point-to-plane ICP
    against target_normals [M,3] (a zero normal: the point takes no part), or of point-to-point ICP, on the (R, t, s) of
    x' = s R x + t (module docstring; contract: include/colvo.h colvo_register_clouds).
    init = (R, t, s) as align_trajectory returns it (None: the identity); the source itself is never pre-transformed, so a sample is
    rounded to float32 once.  pivot: the point the update turns and scales about -- it conditions the problem and does not change
    what is minimised --, by default the centre of the box of the target's finite points.  max_dist is the reach of the search; pairs
    further apart do not exist.  The defaults are Registration's: choices, not tuned.
    Builds the target's index, enqueues everything on the current stream and returns device tensors: no read-back and no host
    synchronisation (RegistrationResult.transform() is the read-back).  Check `status`: anything but REGISTER_OK returned init."""
    who = "register_clouds"
    policy = _chk_registration(who, Registration(mode, metric, iterations, None, damping, min_pairs))
    source, target, normals, state, pv, md, index = _register_inputs(who, source, target, target_normals, init, pivot, max_dist, metric)
    lib = _lib.load()
    dev = source.device
    N, M = source.shape[0], target.shape[0]
    ws = torch.empty(int(lib.colvo_register_scratch_bytes(N)), device=dev, dtype=torch.uint8)
    out = torch.empty(13, device=dev, dtype=torch.float64)
    history = torch.empty(policy.iterations + 1, 5, device=dev, dtype=torch.float64)
    status = torch.empty(1, device=dev, dtype=torch.int32)
    normal = torch.empty(7, 7, device=dev, dtype=torch.float64)
    _lib.check(lib.colvo_register_clouds(_lib.ptr(source), N, _lib.ptr(target), _lib.ptr(normals), M, md, _lib.ptr(index),
                                         _lib.ptr(state), _lib.ptr(pv), REGISTER_MODES.index(policy.mode),
                                         REGISTER_METRICS.index(policy.metric), policy.iterations, float(policy.damping),
                                         int(policy.min_pairs), _lib.ptr(ws), _lib.ptr(out), _lib.ptr(history), _lib.ptr(status),
                                         _lib.ptr(normal), _lib.stream_ptr()), "colvo_register_clouds")
    return RegistrationResult(out[:9].view(3, 3), out[9:12], out[12], history, status[0], normal)


# ---- surfaces (csrc/surface.hip) ------------------------------------------------------------------------------------------ #
SURFACE_STATS = CLOUD_STATS + ("in_front", "behind", "plane_winners", "dead_faces", "skipped_faces", "pairs", "oversize")
MAX_SURFACE_PAIRS = (1 << 30) - 1


class SurfaceNN(NamedTuple):
    dist: torch.Tensor          # [N] float32: sqrt(dist2) in float64, rounded once
    dist2: torch.Tensor         # [N] float64: squared distance to the nearest point of the triangles within reach, else md2
    face: torch.Tensor          # [N] int32: the face that point lies on, else -1
    closest: torch.Tensor       # [N,3] float32: that point; the query itself where nothing is within reach
    side: torch.Tensor          # [N] int8: +1 in front of the face (the side its normal points to: free space), -1 behind, 0 on it
    stats: torch.Tensor         # [19] int64 on the device, SURFACE_STATS order
    max_dist: float             # as float32
    thresholds: Tuple[float, ...]   # as float32


class SurfaceMetrics(NamedTuple):
    accuracy: float             # mean truncated distance pred vertices -> gt surface
    completeness: float         # mean truncated distance gt vertices -> pred surface
    chamfer: float
    precision: Tuple[float, ...]
    recall: Tuple[float, ...]
    fscore: Tuple[float, ...]
    n_pred: int                 # valid pred vertices (those a live face uses)
    n_gt: int
    n_pred_reached: int
    n_gt_reached: int
    pred_to_gt: SurfaceNN
    gt_to_pred: SurfaceNN
    in_front: float             # share of the valid pred vertices in front of the ground-truth surface (its free-space side)
    behind: float               # ... behind it
    pred: Mesh                  # the two meshes as compared: cleaned, pred transformed
    gt: Mesh


def point_to_surface(points: torch.Tensor, mesh_or_vertices, faces: Optional[torch.Tensor] = None, *, max_dist: float,
                     thresholds: Sequence[float] = ()) -> SurfaceNN:
    """For every point of points [N,3] the nearest point of the TRIANGLES of a mesh closer than max_dist -- `point_to_surface(points,
    mesh, ...)` with a Mesh, or vertices [V,3] float32 and faces [F,3] int32 on the device -- its face, and the side of that face the
    point lies on, with the exact statistics of the module docstring (contract: include/colvo.h colvo_surface_*).  Every output bit
    follows from the inputs alone and equals the gridless NumPy replica tests/surface_ref.py.  Enqueues on the current stream and
    returns device tensors; the one read-back is the index's counts block, which sizes its records."""
    who = "point_to_surface"
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32 or points.dim() != 2 \
            or points.shape[1] != 3:
        raise ValueError(f"{who}: points: expected a float32 CUDA tensor of shape [N,3], got {getattr(points, 'dtype', None)} "
                         f"{tuple(getattr(points, 'shape', ()))} on {getattr(points, 'device', None)}")
    points = points.contiguous()
    vertices, faces, V, F = _mesh_arrays(who, mesh_or_vertices, faces)
    dev = points.device
    if vertices.device != dev:
        raise ValueError(f"{who}: the mesh is on {vertices.device}, points on {dev}")
    md, th = _chk_reach(who, max_dist, thresholds)
    N = points.shape[0]
    if N >= 1 << 30:
        raise ValueError(f"{who}: {N} points: fewer than 2^30")
    lib = _lib.load()
    scratch = torch.empty(int(lib.colvo_surface_scratch_bytes(V, F)), device=dev, dtype=torch.uint8)
    counts = torch.empty(8, device=dev, dtype=torch.int64)
    stream = _lib.stream_ptr()
    _lib.check(lib.colvo_surface_index_plan(_lib.ptr(vertices), _lib.ptr(faces), V, F, md, _lib.ptr(scratch), _lib.ptr(counts),
                                            stream), "colvo_surface_index_plan")
    pairs, _, _, _, record_bytes = (int(c) for c in counts[:5].tolist())
    if pairs > MAX_SURFACE_PAIRS:
        raise ValueError(f"{who}: {pairs} (cell, face) pairs in the index of {F} faces: fewer than 2^30 (use a larger max_dist)")
    records = torch.empty(max(pairs, 1) * record_bytes, device=dev, dtype=torch.uint8)
    _lib.check(lib.colvo_surface_index_fill(_lib.ptr(vertices), _lib.ptr(faces), V, F, _lib.ptr(scratch), pairs, record_bytes,
                                            _lib.ptr(records), stream), "colvo_surface_index_fill")
    dist2 = torch.empty(N, device=dev, dtype=torch.float64)
    dist = torch.empty(N, device=dev, dtype=torch.float32)
    face = torch.empty(N, device=dev, dtype=torch.int32)
    closest = torch.empty(N, 3, device=dev, dtype=torch.float32)
    side = torch.empty(N, device=dev, dtype=torch.int8)
    stats = torch.empty(len(SURFACE_STATS), device=dev, dtype=torch.int64)
    tau = (ctypes.c_float * MAX_THRESHOLDS)(*th)
    _lib.check(lib.colvo_surface_query(_lib.ptr(points), N, _lib.ptr(vertices), _lib.ptr(faces), V, F, md, ctypes.addressof(tau),
                                       len(th), _lib.ptr(scratch), _lib.ptr(records), pairs, record_bytes, _lib.ptr(dist2), _lib.ptr(dist),
                                       _lib.ptr(face), _lib.ptr(closest), _lib.ptr(side), _lib.ptr(stats), stream),
               "colvo_surface_query")
    return SurfaceNN(dist, dist2, face, closest, side, stats, md, th)


def _as_mesh(who: str, name: str, m) -> Mesh:
    """A Mesh, or a (vertices, faces) pair dressed as one (no colours, zero normals and cells)."""
    if isinstance(m, Mesh):
        return m
    try:
        vertices, faces = m
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must be a Mesh or a (vertices, faces) pair") from None
    vertices, faces, V, _ = _mesh_arrays(who, vertices, faces)
    return Mesh(vertices, faces, None, torch.zeros_like(vertices), torch.zeros(V, 3, device=vertices.device, dtype=torch.int32), 0)


def _cleaned(m: Mesh) -> Mesh:
    """clean_mesh's defaults: without the vertices no live face uses and without the dead faces (the unit only scales areas nobody
    reads here)."""
    return clean_mesh(m, mesh_topology(m, unit=1.0)).mesh


def surface_metrics(pred, gt, *, max_dist: float, thresholds: Sequence[float], transform=None) -> SurfaceMetrics:
    """cloud_metrics' twelve measures between two SURFACES: pred and gt are Meshes or (vertices, faces) pairs; both are first cleaned
    with clean_mesh's defaults, so that the queries of each direction are the vertices a live face uses; transform = (R, t, s), as
    align_trajectory returns it, moves pred's vertices through transform_cloud; then pred's vertices are scored against gt's triangles
    (accuracy, precision) and gt's against pred's (completeness, recall) by point_to_surface.  in_front / behind are the shares of the
    valid pred vertices on the free-space side of the ground-truth surface and behind it.  Reads the statistics back once, at the
    end, on top of the read-backs of clean_mesh and of the two indices."""
    who = "surface_metrics"
    md, th = _chk_reach(who, max_dist, thresholds)
    p, g = _cleaned(_as_mesh(who, "pred", pred)), _cleaned(_as_mesh(who, "gt", gt))
    if transform is not None:
        R, t, s = transform
        p = p._replace(vertices=transform_cloud(p.vertices, R, t, s))
    a = point_to_surface(p.vertices, g, max_dist=md, thresholds=th)
    b = point_to_surface(g.vertices, p, max_dist=md, thresholds=th)
    both = torch.stack([a.stats, b.stats]).tolist()
    m = metrics_from_stats(both[0], both[1], md, len(th))
    n = m["n_pred"]
    return SurfaceMetrics(**m, pred_to_gt=a, gt_to_pred=b, in_front=both[0][12] / n if n else math.nan,
                          behind=both[0][13] / n if n else math.nan, pred=p, gt=g)


def surface_reconstruction_metrics(pred_mesh: Mesh, pred_cam2world, gt_depths: torch.Tensor, K: torch.Tensor, gt_cam2world, *,
                                   voxel_size: float, meshing: Meshing = Meshing(), max_dist: Optional[float] = None,
                                   thresholds: Optional[Sequence[float]] = None, align: str = "sim3", stride: int = 1,
                                   max_depth: float = MAX_DEPTH, gt_colors: Optional[torch.Tensor] = None) -> SurfaceMetrics:
    """A reconstructed surface against ground truth, point to surface: pred_mesh (reconstruct_sequence's `mesh`) in the frame of the
    trajectory pred_cam2world [N,4,4], against the mesh that fuse_tsdf + extract_mesh give from gt_depths [N,1,H,W] along gt_cam2world
    [N,4,4] at the same voxel_size under the pred side's policy `meshing` (trunc, min_obs; with min_faces > 0 the ground-truth mesh is
    cleaned the same way, with fill_edges >= 3 its small holes are filled the same way).  pred is moved by align_trajectory(pred_cam2world, gt_cam2world, align) and the two are compared by
    surface_metrics.  max_dist defaults to 4 * voxel_size and thresholds to (voxel_size, 2 * voxel_size), as in
    reconstruction_metrics: choices, not tuned."""
    who = "surface_reconstruction_metrics"
    if not isinstance(pred_mesh, Mesh):
        raise ValueError(f"{who}: pred_mesh must be a Mesh")
    if not isinstance(meshing, Meshing):
        raise ValueError(f"{who}: meshing must be a Meshing")
    if not (type(meshing.fill_edges) is int and meshing.fill_edges == 0):      # (before the fusion runs)
        int_range(who, "meshing.fill_edges (or 0: no filling)", meshing.fill_edges, 3)
    G = _poses(gt_cam2world, "gt_cam2world")
    G32 = G.to(gt_depths.device, torch.float32)
    volume = inference.fuse_tsdf(gt_depths, K, G32, voxel_size=voxel_size, trunc=meshing.trunc, colors=gt_colors, stride=stride,
                                 max_depth=max_depth)
    gt = inference.extract_mesh(volume, min_obs=meshing.min_obs)
    if meshing.min_faces > 0:
        gt = clean_mesh(gt, mesh_topology(gt, unit=voxel_size), min_faces=meshing.min_faces).mesh
    if meshing.fill_edges != 0:
        gt = inference.fill_holes(gt, mesh_topology(gt, unit=voxel_size), max_edges=meshing.fill_edges).mesh
    R, t, s = align_trajectory(pred_cam2world, G, align)
    vs = _f32(voxel_size)
    return surface_metrics(pred_mesh, gt, max_dist=4.0 * vs if max_dist is None else max_dist,
                           thresholds=(vs, 2.0 * vs) if thresholds is None else thresholds,
                           transform=None if align == "none" else (R, t, s))
