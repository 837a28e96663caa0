"""Inference side of the path: depth maps + relative poses -> trajectory -> stitched point cloud, and
the coloured, voxel-averaged cloud fused from it; refine_edges / refine_trajectory correct the trajectory
against the depth maps and frames it connects (csrc/refine.hip).

Reference: README.md:9 ("complete 3D reconstruction of the intestine"), README.md:29 ("stitching together the dense depth
maps of each frame using the colonoscopic trajectory").  filter_depths is the cross-view check in front of both (DESIGN.md
§3.6f, csrc/consistency.hip).  Spec: oracle/colvo_spec.py integrate_trajectory / backproject /
stitch_point_cloud (oracle/SPEC.md §6c).  The per-pixel work runs in csrc/reconstruct.hip; the trajectory integration is N
products of 4x4 matrices and is done on the host in float64 (it is control flow, not a kernel).  The fusion runs in
csrc/fuse.hip.  render_cloud / render_fused draw a cloud back into camera views (csrc/render.hip).
  mesh_topology / clean_mesh say what the extracted surface is -- components, boundary loops, areas -- and remove its debris (DESIGN.md
§3.6o, csrc/topology.hip); fill_holes closes its small holes and measures every hole (csrc/fill.hip).  The entry points of
fusion, consistency, refine, render, topology, holes and ply are re-exported here.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from . import _lib, localize
from ._args import MAX_DEPTH, depth_views, int_range, per_view_K
from .consistency import Consistency, ConsistencyResult, check_consistency, filter_depths
from .holes import HoleFill, fill_holes
from .fusion import (CloudNormals, FusedCloud, Mesh, Meshing, TsdfVolume, cloud_normals, extract_mesh, fuse_point_cloud, fuse_tsdf,
                     fusion_grid, tsdf_voxels)
from .ply import write_ply
from .refine import (REFINE_BAD_EDGE, REFINE_NOT_PD, REFINE_OK, REFINE_REVERTED, REFINE_TOO_FEW, Refinement, RefinementResult,
                     _refine_inputs, check_refinement, refine_accumulate, refine_edges, refine_trajectory, rigid_inverse)
from .render import (MeshViews, Render, RenderedViews, SurfelViews, check_render, render_cloud, render_fused, render_mesh,
                     render_surfels)
from .topology import CleanedMesh, MeshTopology, clean_mesh, mesh_topology


def pose_to_matrix4(pose: torch.Tensor) -> torch.Tensor:
    """[N,6] (tx,ty,tz,rx,ry,rz; R = Rz Ry Rx, spec §4) -> [N,4,4] float64 on the CPU."""
    p = pose.detach().to("cpu", torch.float64)
    if p.dim() != 2 or p.shape[1] != 6:
        raise ValueError("pose_to_matrix4: expected [N,6]")
    out = torch.zeros(p.shape[0], 4, 4, dtype=torch.float64)
    for n in range(p.shape[0]):
        tx, ty, tz, rx, ry, rz = (float(v) for v in p[n])
        cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
        out[n] = torch.tensor([
            [cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx, tx],
            [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx, ty],
            [-sy, cy * sx, cy * cx, tz],
            [0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)
    return out


def integrate_trajectory(rel_poses: torch.Tensor) -> torch.Tensor:
    """Camera-to-world transforms of frames 0..N from the N relative poses of consecutive pairs (spec:
    integrate_trajectory): rel_poses[k] maps frame-k points into frame k+1; world = camera 0;
    M_0 = I, M_{k+1} = M_k @ inverse(T_k).  -> [N+1,4,4] float64 on the CPU."""
    T = pose_to_matrix4(rel_poses)
    M = [torch.eye(4, dtype=torch.float64)]
    for k in range(T.shape[0]):
        M.append(M[-1] @ rigid_inverse(T[k]))
    return torch.stack(M)


def backproject(depth: torch.Tensor, K: torch.Tensor, cam2world: torch.Tensor) -> torch.Tensor:
    """depth [B,1,H,W], K [B,3,3], cam2world [B,4,4] -> world points [B,H*W,3] (spec: backproject)."""
    depth, K, cam2world, B, H, W = depth_views("backproject", depth, K, cam2world, name="depth")
    points = torch.empty(B, H * W, 3, device=depth.device, dtype=torch.float32)
    _lib.call("colvo_backproject", depth, K, cam2world, B, H, W, points, _lib.stream_ptr())
    return points


def stitch_point_cloud(depths: torch.Tensor, K: torch.Tensor, cam2world: torch.Tensor, *, stride: int = 1,
                       max_depth: float = MAX_DEPTH) -> torch.Tensor:
    """Every `stride`-th pixel of every frame with depth < max_depth, in the world frame, frame-major / row-major order
    (spec: stitch_point_cloud).  depths [N,1,H,W], K [N,3,3], cam2world [N,4,4] -> [M,3].  Reads the point count back
    (one 4-byte copy) to size the result."""
    lib = _lib.load()
    int_range("stitch_point_cloud", "stride", stride, 1)
    depths, K, cam2world, N, H, W = depth_views("stitch_point_cloud", depths, K, cam2world)
    cap = N * -(-H // stride) * -(-W // stride)
    ws = torch.empty(int(lib.colvo_stitch_workspace_ints(N, H, W, stride)), device=depths.device, dtype=torch.int32)
    count = torch.empty(1, device=depths.device, dtype=torch.int32)
    points = torch.empty(cap, 3, device=depths.device, dtype=torch.float32)
    _lib.call("colvo_stitch_point_cloud", depths, K, cam2world, N, H, W, stride, float(max_depth), ws, points, count, _lib.stream_ptr())
    return points[: int(count.item())]


class _ReconstructionFields(NamedTuple):
    depths: torch.Tensor        # [N+1,1,H,W]
    rel_poses: torch.Tensor     # [N,6]    frame k -> frame k+1
    cam2world: torch.Tensor     # [N+1,4,4] float64, CPU
    points: torch.Tensor        # [M,3]    world frame (camera 0)
    fused: Optional[FusedCloud] = None   # with voxel_size: the coloured, voxel-averaged cloud


class Reconstruction(_ReconstructionFields):
    """The five fields above -- it still unpacks into five -- and, behind them, `polyps`: with labels the PolypLocalization
    of the same depths and trajectory (coivo_amd.localize), else None; and `consistency`: with a Consistency policy the
    ConsistencyResult whose depths points, fused and polyps were computed from (`depths` stays the raw network output), else
    None; and `refinement`: with a Refinement policy the RefinementResult of the consecutive pairs -- `cam2world` is then the
    refined trajectory, `rel_poses` stays the raw network output -- else None; and `rendered`: with a Render policy the
    RenderedViews of `fused` in every frame's own camera along `cam2world`, else None; and `normals`: with Render(surfels=True) the
    CloudNormals of `fused` (`rendered` is then the SurfelViews drawn with them), else None; and `mesh`: with a Meshing policy the
    Mesh extracted from the TSDF volume of the same depths and trajectory, else None (with Render(mesh=True) `rendered` is the
    MeshViews of that mesh); and `topology`: with a Meshing policy the MeshTopology of `mesh` (unit = the voxel size), else None; and `holes`: with Meshing(fill_edges >= 3) the
    HoleFill whose mesh `mesh` is, else None."""
    polyps = None               # Optional[PolypLocalization]
    consistency = None          # Optional[ConsistencyResult]
    refinement = None           # Optional[RefinementResult]
    rendered = None             # Optional[RenderedViews], SurfelViews with Render(surfels=True), MeshViews with Render(mesh=True)
    normals = None              # Optional[CloudNormals]
    mesh = None                 # Optional[Mesh]
    topology = None             # Optional[MeshTopology]
    holes = None                # Optional[HoleFill]

    def __new__(cls, depths, rel_poses, cam2world, points, fused=None, polyps=None, consistency=None, refinement=None,
                rendered=None, normals=None, mesh=None, topology=None, holes=None):
        self = super().__new__(cls, depths, rel_poses, cam2world, points, fused)
        self.polyps = polyps
        self.consistency = consistency
        self.refinement = refinement
        self.rendered = rendered
        self.normals = normals
        self.mesh = mesh
        self.topology = topology
        self.holes = holes
        return self

    def _replace(self, **kw):
        polyps = kw.pop("polyps", self.polyps)
        consistency = kw.pop("consistency", self.consistency)
        refinement = kw.pop("refinement", self.refinement)
        rendered = kw.pop("rendered", self.rendered)
        normals = kw.pop("normals", self.normals)
        mesh = kw.pop("mesh", self.mesh)
        topology = kw.pop("topology", self.topology)
        holes = kw.pop("holes", self.holes)
        return type(self)(*super()._replace(**kw), polyps=polyps, consistency=consistency, refinement=refinement, rendered=rendered,
                          normals=normals, mesh=mesh, topology=topology, holes=holes)


@torch.no_grad()
def run_networks(depth_net, pose_net, frames: torch.Tensor, *, chunk: int = 16):
    """frames [N+1,3,H,W] of one sequence -> (depths [N+1,1,H,W], rel_poses [N,6]): DepthNet on every frame and PoseNet on every
    consecutive pair (DCDP: PoseNet sees both depth maps), `chunk` frames or pairs per call."""
    n = frames.shape[0]
    depths = torch.cat([depth_net(frames[i:i + chunk].contiguous()) for i in range(0, n, chunk)])
    poses = []
    for i in range(0, n - 1, chunk):
        j = min(i + chunk, n - 1)
        pose, _, _ = pose_net(frames[i:j].contiguous(), frames[i + 1:j + 1].contiguous(),
                              depths[i:j].contiguous(), depths[i + 1:j + 1].contiguous())
        poses.append(pose)
    return depths, torch.cat(poses)


@torch.no_grad()
def reconstruct_sequence(depth_net, pose_net, frames: torch.Tensor, K: torch.Tensor, *, stride: int = 4,
                         max_depth: float = MAX_DEPTH, chunk: int = 16, voxel_size: Optional[float] = None,
                         min_obs: int = 1, labels: Optional[torch.Tensor] = None,
                         num_labels: Optional[int] = None, consistency: Optional[Consistency] = None,
                         refine: Optional[Refinement] = None, render: Optional[Render] = None,
                         mesh: Optional[Meshing] = None) -> Reconstruction:
    """frames [N+1,3,H,W] of one sequence, K [3,3] or [N+1,3,3] -> depth of every frame, the pose of every consecutive
    pair (DCDP: PoseNet sees both depth maps), the integrated trajectory and the stitched cloud.  With a voxel_size also
    the fused cloud of the same samples, coloured by the frames (fuse_point_cloud; `fused`, else None).  With labels
    [N+1,1,H,W] uint8 and num_labels also the polyps they mark, localised from the same depths, K, trajectory and max_depth at
    stride 1 (localize.localize_polyps; `polyps`, else None).  With a Consistency policy the depth maps first pass
    filter_depths along the integrated trajectory (same K and max_depth): points, fused and polyps are computed from the
    filtered depths, `depths` stays the raw network output and the ConsistencyResult is `consistency` (else None).  With a
    Refinement policy the integrated trajectory first passes refine_trajectory (raw depths, the frames, same K and max_depth): the
    refined trajectory is `cam2world` and is what the filter, the stitching, the fusion and the localisation use; `rel_poses` stays
    the raw network output and the RefinementResult is `refinement` (else None).  With a Render policy (needs voxel_size) the fused
    cloud is drawn back into every frame's own camera along the trajectory the call used (render_fused: same K, max_depth and
    image size; radius None is the voxel size) and the RenderedViews is `rendered` (else None).  With Render(surfels=True) the cloud's
    normals are first computed from the depths, stride, max_depth and trajectory it was fused with (cloud_normals; `normals`, else
    None) and the cloud is drawn as oriented discs: `rendered` is then a SurfelViews.  With a Meshing policy (needs voxel_size) the
    depths the fusion used (filtered if a Consistency is given), coloured by the frames, are integrated at full resolution into a
    TSDF volume along the trajectory the call used (fuse_tsdf: same K, voxel_size, stride and max_depth; policy.trunc) and the surface
    is extracted from it (extract_mesh: policy.min_obs): the Mesh is `mesh` (else None).  With Render(mesh=True) (needs a Meshing policy;
    not together with surfels=True) it is that mesh, not the cloud, that is drawn into every frame's own camera (render_mesh: same K,
    max_depth and image size, culling off): `rendered` is then a MeshViews and `normals` stays None.  With a Meshing policy the
    topology of the mesh is computed as well (mesh_topology, unit = voxel_size; `topology`, else None); with policy.min_faces > 0 the
    components with fewer faces -- and every vertex no face uses -- are first removed (clean_mesh) and the topology is that of the
    cleaned mesh, which is then `mesh` and what Render(mesh=True) draws; with min_faces = 0 `mesh` is extract_mesh's, bit for bit.  With
    policy.fill_edges >= 3 the simple boundary rings of at most that many edges are then closed (fill_holes, after the cleaning): the
    HoleFill is `holes` (else None), its mesh is `mesh` and what Render(mesh=True) draws, and `topology` is recomputed on it; with
    fill_edges = 0 (a choice, not a tuned value) every output is as without the field.  1 and 2 are refused."""
    who = "reconstruct_sequence"
    n = frames.shape[0]
    if n < 2:
        raise ValueError(f"{who}: need at least two frames")
    if labels is not None and num_labels is None:
        raise ValueError(f"{who}: labels need num_labels")
    if consistency is not None:
        consistency = Consistency(*consistency)
        check_consistency(who, *consistency, max_depth)
    if refine is not None:
        refine = Refinement(*refine)
        check_refinement(who, refine, max_depth)
    if render is not None:
        render = Render(*render, surfels=getattr(render, "surfels", False), mesh=getattr(render, "mesh", False))
        if voxel_size is None:
            raise ValueError(f"{who}: render needs voxel_size (it draws the fused cloud)")
        check_render(who, voxel_size if render.radius is None else render.radius, render.max_splat, max_depth)
        for name in ("surfels", "mesh"):
            if not isinstance(getattr(render, name), bool):
                raise ValueError(f"{who}: render.{name} must be a bool, got {getattr(render, name)!r}")
        if render.mesh and render.surfels:
            raise ValueError(f"{who}: Render(mesh=True) draws the surface mesh, surfels=True the cloud: give one of them")
        if render.mesh and mesh is None:
            raise ValueError(f"{who}: Render(mesh=True) needs a Meshing policy (mesh=Meshing()): it draws the extracted mesh")
    if mesh is not None:
        mesh = Meshing(*mesh, min_faces=mesh.min_faces, fill_edges=mesh.fill_edges) if isinstance(mesh, Meshing) else Meshing(*mesh)      # (a plain tuple may hold two to four)
        if voxel_size is None:
            raise ValueError(f"{who}: mesh needs voxel_size (the TSDF volume's voxels)")
        tsdf_voxels(who, voxel_size, mesh.trunc)
        int_range(who, "mesh.min_obs", mesh.min_obs, 1)
        int_range(who, "mesh.min_faces", mesh.min_faces, 0)
        if not (type(mesh.fill_edges) is int and mesh.fill_edges == 0):
            int_range(who, "mesh.fill_edges (or 0: no filling)", mesh.fill_edges, 3)
    K = per_view_K(K, n).to(frames.device, torch.float32).contiguous()
    depths, rel = run_networks(depth_net, pose_net, frames, chunk=chunk)
    traj = integrate_trajectory(rel)
    refined = None
    if refine is not None:
        traj, refined = refine_trajectory(depths, frames.to(torch.float32).contiguous(), K, traj, max_depth=max_depth,
                                          **refine._asdict())
    traj32 = traj.to(frames.device, torch.float32)
    raw, checked = depths, None
    if consistency is not None:
        checked = filter_depths(depths, K, traj32, **consistency._asdict(), max_depth=max_depth)
        depths = checked.depths
    cloud = stitch_point_cloud(depths, K, traj32, stride=stride, max_depth=max_depth)
    fused = None
    if voxel_size is not None:
        fused = fuse_point_cloud(depths, K, traj32, voxel_size=voxel_size, colors=frames.to(torch.float32).contiguous(),
                                 stride=stride, max_depth=max_depth, min_obs=min_obs)
    polyps = None
    if labels is not None:
        polyps = localize.localize_polyps(depths, labels, K, traj32, num_labels=num_labels, stride=1, max_depth=max_depth)
    rendered = normals = None
    if render is not None and not render.mesh:
        if render.surfels:
            normals = cloud_normals(fused, depths, K, traj32, stride=stride, max_depth=max_depth)
        rendered = render_fused(fused, K, traj32, int(frames.shape[2]), int(frames.shape[3]), radius=render.radius,
                                max_splat=render.max_splat, max_depth=max_depth, normals=normals)
    surface = topology = holes = None
    if mesh is not None:
        volume = fuse_tsdf(depths, K, traj32, voxel_size=voxel_size, trunc=mesh.trunc, colors=frames.to(torch.float32).contiguous(),
                           stride=stride, max_depth=max_depth)
        surface = extract_mesh(volume, min_obs=mesh.min_obs)
        topology = mesh_topology(surface, unit=voxel_size)
        if mesh.min_faces > 0:
            surface = clean_mesh(surface, topology, min_faces=mesh.min_faces).mesh
            topology = mesh_topology(surface, unit=voxel_size)
        if mesh.fill_edges != 0:
            holes = fill_holes(surface, topology, max_edges=mesh.fill_edges)
            surface = holes.mesh
            topology = mesh_topology(surface, unit=voxel_size)
        if render is not None and render.mesh:
            rendered = render_mesh(surface, K, traj32, int(frames.shape[2]), int(frames.shape[3]), max_depth=max_depth)
    return Reconstruction(raw, rel, traj, cloud, fused, polyps, checked, refined, rendered, normals, surface, topology, holes)
