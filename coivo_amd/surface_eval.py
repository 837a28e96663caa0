"""Surfaces (csrc/surface.hip; the contract is include/colvo.h colvo_surface_*, replica tests/surface_ref.py)
  point_to_surface(points, mesh)  for every point the distance to the nearest point OF THE TRIANGLES of a mesh within max_dist, the
            face, the nearest point and the side; float64 on widened float32 coordinates in a written association; dead faces as
            mesh_topology's, faces with a coordinate that is not finite skipped; the least (d2, face) wins.  The first twelve
            statistics are CLOUD_STATS, so metrics_from_stats serves both.
  surface_metrics(pred, gt)  cloud_metrics' measures with each side's used vertices scored against the other side's triangles, and the
            shares of pred vertices in front of and behind the ground-truth surface.  surface_reconstruction_metrics meshes the
            ground-truth depths with the pred side's policy.  Not here: registration against faces, sampling a surface by area, a
            signed-distance volume, any use in training.
coivo_amd.evaluate re-exports every name here."""
import ctypes
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._args import MAX_DEPTH, MAX_THRESHOLDS, cloud, f32, int_range, mesh_arrays, reach, sim3
from .cloud_eval import CLOUD_STATS, metrics_from_stats, transform_cloud
from .fusion import Mesh, Meshing, extract_mesh, fuse_tsdf
from .holes import fill_holes
from .topology import clean_mesh, mesh_topology
from .trajectory import align_trajectory, poses

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
    points = cloud(who, "points", points)
    vertices, faces, V, F = mesh_arrays(who, mesh_or_vertices, faces)
    dev = points.device
    if vertices.device != dev:
        raise ValueError(f"{who}: the mesh is on {vertices.device}, points on {dev}")
    md, th = reach(who, max_dist, thresholds)
    N = points.shape[0]
    if N >= 1 << 30:
        raise ValueError(f"{who}: {N} points: fewer than 2^30")
    scratch = torch.empty(int(_lib.load().colvo_surface_scratch_bytes(V, F)), device=dev, dtype=torch.uint8)
    counts = torch.empty(8, device=dev, dtype=torch.int64)
    stream = _lib.stream_ptr()
    _lib.call("colvo_surface_index_plan", vertices, faces, V, F, md, scratch, counts, stream)
    pairs, _, _, _, record_bytes = (int(c) for c in counts[:5].tolist())
    if pairs > MAX_SURFACE_PAIRS:
        raise ValueError(f"{who}: {pairs} (cell, face) pairs in the index of {F} faces: fewer than 2^30 (use a larger max_dist)")
    records = torch.empty(max(pairs, 1) * record_bytes, device=dev, dtype=torch.uint8)
    _lib.call("colvo_surface_index_fill", vertices, faces, V, F, scratch, pairs, record_bytes, records, stream)
    dist2 = torch.empty(N, device=dev, dtype=torch.float64)
    dist = torch.empty(N, device=dev, dtype=torch.float32)
    face = torch.empty(N, device=dev, dtype=torch.int32)
    closest = torch.empty(N, 3, device=dev, dtype=torch.float32)
    side = torch.empty(N, device=dev, dtype=torch.int8)
    stats = torch.empty(len(SURFACE_STATS), device=dev, dtype=torch.int64)
    tau = (ctypes.c_float * MAX_THRESHOLDS)(*th)
    _lib.call("colvo_surface_query", points, N, vertices, faces, V, F, md, ctypes.addressof(tau), len(th), scratch, records, pairs,
              record_bytes, dist2, dist, face, closest, side, stats, stream)
    return SurfaceNN(dist, dist2, face, closest, side, stats, md, th)


def _as_mesh(who: str, name: str, m) -> Mesh:
    """A Mesh, or a (vertices, faces) pair dressed as one (no colours, zero normals and cells)."""
    if isinstance(m, Mesh):
        return m
    try:
        vertices, faces = m
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must be a Mesh or a (vertices, faces) pair") from None
    vertices, faces, V, _ = mesh_arrays(who, vertices, faces)
    return Mesh(vertices, faces, None, torch.zeros_like(vertices), torch.zeros(V, 3, device=vertices.device, dtype=torch.int32), 0)


def cleaned(m: Mesh) -> Mesh:
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
    md, th = reach(who, max_dist, thresholds)
    if transform is not None:
        transform = sim3(who, "transform", transform)
    p, g = cleaned(_as_mesh(who, "pred", pred)), cleaned(_as_mesh(who, "gt", gt))
    if transform is not None:
        p = p._replace(vertices=transform_cloud(p.vertices, *transform))
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
    G = poses(gt_cam2world, "gt_cam2world")
    G32 = G.to(gt_depths.device, torch.float32)
    volume = fuse_tsdf(gt_depths, K, G32, voxel_size=voxel_size, trunc=meshing.trunc, colors=gt_colors, stride=stride, max_depth=max_depth)
    gt = extract_mesh(volume, min_obs=meshing.min_obs)
    if meshing.min_faces > 0:
        gt = clean_mesh(gt, mesh_topology(gt, unit=voxel_size), min_faces=meshing.min_faces).mesh
    if meshing.fill_edges != 0:
        gt = fill_holes(gt, mesh_topology(gt, unit=voxel_size), max_edges=meshing.fill_edges).mesh
    R, t, s = align_trajectory(pred_cam2world, G, align)
    vs = f32(voxel_size)
    return surface_metrics(pred_mesh, gt, max_dist=4.0 * vs if max_dist is None else max_dist,
                           thresholds=(vs, 2.0 * vs) if thresholds is None else thresholds,
                           transform=None if align == "none" else (R, t, s))
