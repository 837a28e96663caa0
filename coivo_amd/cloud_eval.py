"""Point clouds (csrc/cloud.hip; these definitions are the contract, include/colvo.h says the same)
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
coivo_amd.evaluate re-exports every name here."""
import ctypes
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._args import MAX_DEPTH, MAX_THRESHOLDS, cloud, f32, reach, sim3
from .fusion import FusedCloud, cloud_normals, fuse_point_cloud
from .registration import Registration, check_registration, register_clouds
from .trajectory import align_trajectory, poses

CLOUD_STATS = ("n_valid", "n_reached") + tuple(f"under_{k}" for k in range(8)) + ("sum_quanta", "examined")


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


def nearest_neighbors(query: torch.Tensor, ref: torch.Tensor, *, max_dist: float, thresholds: Sequence[float] = ()) -> CloudNN:
    """For every point of query [N,3] the nearest point of ref [M,3] closer than max_dist, and the exact statistics of the
    module docstring (float32 clouds on the GPU).  Enqueues on the current stream and returns device tensors; no host
    synchronisation."""
    who = "nearest_neighbors"
    lib = _lib.load()
    query = cloud(who, "query", query)
    ref = cloud(who, "ref", ref)
    if ref.device != query.device:
        raise ValueError(f"ref is on {ref.device}, query on {query.device}")
    md, th = reach(who, max_dist, thresholds)
    N, M = query.shape[0], ref.shape[0]
    nbytes = int(lib.colvo_cloud_workspace_bytes(N, M))
    if nbytes == 0:
        raise ValueError(f"{who}: {N} query and {M} reference points: each cloud must hold fewer than 2^30")
    dev = query.device
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    dist = torch.empty(N, device=dev, dtype=torch.float32)
    dist2 = torch.empty(N, device=dev, dtype=torch.float32)
    nearest = torch.empty(N, device=dev, dtype=torch.int32)
    stats = torch.empty(len(CLOUD_STATS), device=dev, dtype=torch.int64)
    tau = (ctypes.c_float * MAX_THRESHOLDS)(*th)
    stream = _lib.stream_ptr()
    _lib.call("colvo_cloud_index_build", ref, M, md, ws, stream)
    _lib.call("colvo_cloud_query", query, N, M, md, ctypes.addressof(tau), len(th), ws, dist, dist2, nearest, stats, stream)
    return CloudNN(dist, dist2, nearest, stats, md, th)


def transform_cloud(points: torch.Tensor, R, t, s) -> torch.Tensor:
    """out = ((s * ((r0*x + r1*y) + r2*z)) + t) per axis in pinned float32 (module docstring): the Sim(3) of align_trajectory,
    rounded to float32, applied to points [N,3] on the GPU."""
    who = "transform_cloud"
    points = cloud(who, "points", points)
    R, t, s = sim3(who, "(R, t, s)", (R, t, s))
    rts = (ctypes.c_float * 13)(*(R.reshape(-1).tolist() + t.tolist() + [s]))
    out = torch.empty_like(points)
    _lib.call("colvo_cloud_transform", points, points.shape[0], ctypes.addressof(rts), out, _lib.stream_ptr())
    return out


def mean_truncated_distance(stats: Sequence[int], max_dist: float) -> float:
    """double(sum of quanta) / (double(s) * n_valid), s = float32(2^20) / float32(max_dist)."""
    n = int(stats[0])
    if n == 0:
        return math.nan
    # s: the float64 quotient of two float32 values, rounded to float32, is the correctly rounded float32 quotient (53 >= 2 * 24 + 2)
    return float(int(stats[10])) / (f32(1048576.0 / f32(max_dist)) * n)


def metrics_from_stats(pred_stats: Sequence[int], gt_stats: Sequence[int], max_dist: float, n_thresholds: int) -> dict:
    """The measures of cloud_metrics from the two directions' integer statistics (CLOUD_STATS order; pred_stats: pred -> gt,
    gt_stats: gt -> pred) and max_dist as float32.  Host arithmetic only."""
    acc, comp = mean_truncated_distance(pred_stats, max_dist), mean_truncated_distance(gt_stats, max_dist)
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
                  transform=None, register: Optional[Registration] = None, gt_normals: Optional[torch.Tensor] = None) -> CloudMetrics:
    """Accuracy, completeness, Chamfer distance and per-threshold precision / recall / F-score of pred [N,3] against gt [M,3]
    (module docstring), from one search each way.  transform = (R, t, s), as align_trajectory returns it, is applied to pred
    first.  The per-point results of both searches are returned (pred_to_gt.dist colours pred by its error).  Reads the 24
    statistics back once, at the end.
    With a Registration policy `register`, transform (the identity without one) is the start of register_clouds(pred, gt,
    target_normals=gt_normals), whose refined transform -- one more read-back of 13 values -- is what the clouds are compared under; the
    RegistrationResult is `.registration`.  The policy's max_dist None means this call's max_dist.  A registration that froze or
    was reverted returns its start, so the measures are then those of the plain call.  register=None: every bit as without it."""
    who = "cloud_metrics"
    if register is not None:
        check_registration(who, register)
    pred = cloud(who, "pred", pred)
    gt = cloud(who, "gt", gt)
    md, th = reach(who, max_dist, thresholds)
    registration = None
    if register is not None:
        kw = register._asdict()
        if kw["max_dist"] is None:
            kw["max_dist"] = md
        registration = register_clouds(pred, gt, target_normals=gt_normals, init=transform, **kw)
        transform = registration.transform()
    if transform is not None:
        pred = transform_cloud(pred, *sim3(who, "transform", transform))
    a = nearest_neighbors(pred, gt, max_dist=md, thresholds=th)
    b = nearest_neighbors(gt, pred, max_dist=md, thresholds=th)
    both = torch.stack([a.stats, b.stats]).tolist()
    return CloudMetrics(**metrics_from_stats(both[0], both[1], md, len(th)), pred_to_gt=a, gt_to_pred=b, registration=registration)


def reconstruction_metrics(pred_cloud, pred_cam2world, gt_depths: torch.Tensor, K: torch.Tensor, gt_cam2world, *,
                           voxel_size: float, max_dist: Optional[float] = None, thresholds: Optional[Sequence[float]] = None,
                           align: str = "sim3", stride: int = 1, max_depth: float = MAX_DEPTH, min_obs: int = 1,
                           register: Optional[Registration] = None) -> CloudMetrics:
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
    who = "reconstruction_metrics"
    if register is not None:
        check_registration(who, register)
    points = cloud(who, "pred_cloud", pred_cloud.points if isinstance(pred_cloud, FusedCloud) else pred_cloud)
    G = poses(gt_cam2world, "gt_cam2world")
    G32 = G.to(gt_depths.device, torch.float32)
    gt = fuse_point_cloud(gt_depths, K, G32, voxel_size=voxel_size, stride=stride, max_depth=max_depth, min_obs=min_obs)
    R, t, s = align_trajectory(pred_cam2world, G, align)
    vs = f32(voxel_size)
    gt_normals = None
    if register is not None and register.metric == "plane":
        gt_normals = cloud_normals(gt, gt_depths, K, G32, stride=stride, max_depth=max_depth).normals
    return cloud_metrics(points, gt.points, max_dist=4.0 * vs if max_dist is None else max_dist,
                         thresholds=(vs, 2.0 * vs) if thresholds is None else thresholds,
                         transform=None if align == "none" else (R, t, s), register=register, gt_normals=gt_normals)
