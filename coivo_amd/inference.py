"""Inference side of the path: depth maps + relative poses -> trajectory -> stitched point cloud, and
the coloured, voxel-averaged cloud fused from it.

Reference: README.md:9 ("complete 3D reconstruction of the intestine"), README.md:29 ("stitching together the dense depth
maps of each frame using the colonoscopic trajectory").  filter_depths is the cross-view check in front of both (DESIGN.md
§3.6f, csrc/consistency.hip).  Spec: oracle/colvo_spec.py integrate_trajectory / backproject /
stitch_point_cloud (oracle/SPEC.md §6c).  The per-pixel work runs in csrc/reconstruct.hip; the trajectory integration is N
products of 4x4 matrices and is done on the host in float64 (it is control flow, not a kernel).  The fusion runs in
csrc/fuse.hip.
"""
from __future__ import annotations

import math
import struct
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib

MAX_DEPTH = 10.0     # spec: MAX_DEPTH


def _chk(t: torch.Tensor, name: str, shape) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected a float32 CUDA tensor of shape {tuple(shape)}, got "
                         f"{getattr(t, 'dtype', None)} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
    return t.contiguous()


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
        R, t = T[k, :3, :3], T[k, :3, 3]
        Tinv = torch.eye(4, dtype=torch.float64)
        Tinv[:3, :3] = R.t()
        Tinv[:3, 3] = -(R.t() @ t)
        M.append(M[-1] @ Tinv)
    return torch.stack(M)


def backproject(depth: torch.Tensor, K: torch.Tensor, cam2world: torch.Tensor) -> torch.Tensor:
    """depth [B,1,H,W], K [B,3,3], cam2world [B,4,4] -> world points [B,H*W,3] (spec: backproject)."""
    lib = _lib.load()
    if depth.dim() != 4:
        raise ValueError("backproject: depth must be [B,1,H,W]")
    B, _, H, W = depth.shape
    depth = _chk(depth, "depth", (B, 1, H, W))
    K = _chk(K, "K", (B, 3, 3))
    cam2world = _chk(cam2world, "cam2world", (B, 4, 4))
    points = torch.empty(B, H * W, 3, device=depth.device, dtype=torch.float32)
    _lib.check(lib.colvo_backproject(_lib.ptr(depth), _lib.ptr(K), _lib.ptr(cam2world), B, H, W, _lib.ptr(points),
                                     _lib.stream_ptr()), "colvo_backproject")
    return points


def stitch_point_cloud(depths: torch.Tensor, K: torch.Tensor, cam2world: torch.Tensor, *, stride: int = 1,
                       max_depth: float = MAX_DEPTH) -> torch.Tensor:
    """Every `stride`-th pixel of every frame with depth < max_depth, in the world frame, frame-major / row-major order
    (spec: stitch_point_cloud).  depths [N,1,H,W], K [N,3,3], cam2world [N,4,4] -> [M,3].  Reads the point count back
    (one 4-byte copy) to size the result."""
    lib = _lib.load()
    if depths.dim() != 4:
        raise ValueError("stitch_point_cloud: depths must be [N,1,H,W]")
    N, _, H, W = depths.shape
    if stride < 1:
        raise ValueError("stitch_point_cloud: stride must be >= 1")
    depths = _chk(depths, "depths", (N, 1, H, W))
    K = _chk(K, "K", (N, 3, 3))
    cam2world = _chk(cam2world, "cam2world", (N, 4, 4))
    cap = N * -(-H // stride) * -(-W // stride)
    ws = torch.empty(int(lib.colvo_stitch_workspace_ints(N, H, W, stride)), device=depths.device, dtype=torch.int32)
    count = torch.empty(1, device=depths.device, dtype=torch.int32)
    points = torch.empty(cap, 3, device=depths.device, dtype=torch.float32)
    _lib.check(lib.colvo_stitch_point_cloud(_lib.ptr(depths), _lib.ptr(K), _lib.ptr(cam2world), N, H, W, stride,
                                            float(max_depth), _lib.ptr(ws), _lib.ptr(points), _lib.ptr(count),
                                            _lib.stream_ptr()), "colvo_stitch_point_cloud")
    return points[: int(count.item())]


class FusedCloud(NamedTuple):
    points: torch.Tensor            # [M,3] float32: mean position of the samples of each voxel
    colors: Optional[torch.Tensor]  # [M,3] float32 in [0,1]: their mean colour (None without colours)
    counts: torch.Tensor            # [M]   int32: how many samples
    voxels: torch.Tensor            # [M,3] int32: (ix, iy, iz) in the grid
    origin: Tuple[float, float, float]   # lower corner of the grid (float32 values)
    dims: Tuple[int, int, int]      # voxels per axis
    voxel_size: float               # as float32
    n_input: int                    # samples with 0 < depth < max_depth
    n_outside: int                  # ... of which outside the grid
    n_bricks: int                   # 8x8x8 bricks holding a sample
    n_voxels: int                   # occupied voxels (M of them have at least min_obs samples)


def _f32(x) -> float:
    """x rounded to float32, as a Python float (what the C ABI's `float` arguments receive)."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def fusion_grid(K: torch.Tensor, cam2world: torch.Tensor, H: int, W: int, voxel_size: float, max_depth: float = MAX_DEPTH):
    """A grid that holds every sample of depth < max_depth seen from the given cameras: (origin, dims).  Host, float64.
    A sample at z-depth d lies d * |ray| from its camera, |ray| = sqrt(1 + ((u-cx)/fx)^2 + ((v-cy)/fy)^2), largest at an
    image corner; the box is the camera centres -/+ max_depth * (largest corner ray of any frame) -/+ one voxel, snapped
    outward to whole bricks (multiples of 8 voxels).  Loose is cheap -- 4 bytes per brick."""
    Kd = K.detach().to("cpu", torch.float64).reshape(-1, 3, 3)
    Md = cam2world.detach().to("cpu", torch.float64).reshape(-1, 4, 4)
    vs = _f32(voxel_size)
    if not (vs > 0.0 and math.isfinite(vs)) or not (max_depth > 0.0 and math.isfinite(max_depth)):
        raise ValueError("fusion_grid: voxel_size and max_depth must be finite and positive")
    ray = 0.0
    for u in (0.0, float(W - 1)):
        for v in (0.0, float(H - 1)):
            x = (u - Kd[:, 0, 2]) / Kd[:, 0, 0]
            y = (v - Kd[:, 1, 2]) / Kd[:, 1, 1]
            ray = max(ray, float(torch.sqrt(1.0 + x * x + y * y).max()))
    reach = float(max_depth) * ray + vs
    centres = Md[:, :3, 3]
    brick = 8.0 * vs
    lo = [math.floor((float(centres[:, a].min()) - reach) / brick) for a in range(3)]
    hi = [math.ceil((float(centres[:, a].max()) + reach) / brick) for a in range(3)]
    origin = tuple(_f32(l * brick) for l in lo)
    dims = tuple(8 * max(1, h - l) for l, h in zip(lo, hi))
    return origin, dims


def fuse_point_cloud(depths: torch.Tensor, K: torch.Tensor, cam2world: torch.Tensor, *, voxel_size: float,
                     colors: Optional[torch.Tensor] = None, stride: int = 1, max_depth: float = MAX_DEPTH, min_obs: int = 1,
                     origin=None, dims=None) -> FusedCloud:
    """Every `stride`-th pixel of every frame with 0 < depth < max_depth, gathered into the voxels of a regular grid: one
    point per voxel seen at least `min_obs` times, carrying the mean position, the mean colour (colors [N,3,H,W] in
    [0,1]) and the count of its samples, in ascending (8x8x8 brick, voxel in brick) order.  Integer sums: the result is
    bit-identical between calls, streams and frame orders (contract: include/colvo.h).  origin / dims
    default to fusion_grid's; samples outside the grid are counted in n_outside.  Reads two counts back (4 bytes each,
    after the plan and after the count) to size the voxel pool and the result."""
    lib = _lib.load()
    if not isinstance(depths, torch.Tensor) or depths.dim() != 4:
        raise ValueError("fuse_point_cloud: depths must be [N,1,H,W]")
    N, _, H, W = depths.shape
    if stride < 1 or min_obs < 1:
        raise ValueError("fuse_point_cloud: stride and min_obs must be >= 1")
    depths = _chk(depths, "depths", (N, 1, H, W))
    K = _chk(K, "K", (N, 3, 3))
    cam2world = _chk(cam2world, "cam2world", (N, 4, 4))
    if colors is not None:
        colors = _chk(colors, "colors", (N, 3, H, W))
    vs = _f32(voxel_size)
    if not (vs > 0.0 and math.isfinite(vs)):
        raise ValueError("fuse_point_cloud: voxel_size must be finite and positive")
    if (origin is None) != (dims is None):
        raise ValueError("fuse_point_cloud: give origin and dims together, or neither")
    if origin is None:
        origin, dims = fusion_grid(K, cam2world, H, W, vs, max_depth)
    origin = tuple(_f32(o) for o in origin)
    dims = tuple(int(d) for d in dims)
    if len(origin) != 3 or len(dims) != 3 or any(d <= 0 or d % 8 for d in dims):
        raise ValueError(f"fuse_point_cloud: dims must be three positive multiples of 8, got {dims}")
    dev = depths.device
    geom = (N, H, W, int(stride), float(max_depth), *origin, vs, *dims)
    ws_bytes = int(lib.colvo_fuse_plan_workspace_bytes(N, H, W, int(stride), *dims))
    if ws_bytes == 0:
        raise ValueError(f"fuse_point_cloud: shape N={N} H={H} W={W} stride={stride} or grid {dims} beyond the kernels' limits")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    stats = torch.empty(3, device=dev, dtype=torch.int32)
    stream = _lib.stream_ptr()
    _lib.check(lib.colvo_fuse_plan(_lib.ptr(depths), _lib.ptr(K), _lib.ptr(cam2world), *geom, _lib.ptr(ws), _lib.ptr(stats),
                                   stream), "colvo_fuse_plan")
    n_input, n_outside, n_bricks = (int(v) for v in stats.tolist())
    n_voxels = m = 0
    if n_bricks > 0:
        pool_bytes = int(lib.colvo_fuse_pool_bytes(n_bricks))
        if pool_bytes == 0:
            raise RuntimeError(f"fuse_point_cloud: {n_bricks} occupied bricks, the limit is 2^22 - 1: use a larger voxel_size")
        pool = torch.empty(pool_bytes, device=dev, dtype=torch.uint8)
        _lib.check(lib.colvo_fuse_accumulate(_lib.ptr(depths), _lib.ptr(colors), _lib.ptr(K), _lib.ptr(cam2world), *geom,
                                             _lib.ptr(ws), n_bricks, _lib.ptr(pool), stream), "colvo_fuse_accumulate")
        ews = torch.empty(int(lib.colvo_fuse_extract_workspace_bytes(n_bricks)), device=dev, dtype=torch.uint8)
        stats2 = torch.empty(3, device=dev, dtype=torch.int32)
        _lib.check(lib.colvo_fuse_count(_lib.ptr(pool), n_bricks, int(min_obs), _lib.ptr(ews), _lib.ptr(stats2), stream),
                   "colvo_fuse_count")
        n_voxels, m, overflow = (int(v) for v in stats2.tolist())
        if overflow:
            raise RuntimeError("fuse_point_cloud: overflow: a voxel received 2^24 or more samples (its 32-bit sums may have "
                               "wrapped); use a smaller voxel_size, a larger stride or fewer frames per call")
    points = torch.empty(m, 3, device=dev, dtype=torch.float32)
    out_colors = torch.empty(m, 3, device=dev, dtype=torch.float32) if colors is not None else None
    counts = torch.empty(m, device=dev, dtype=torch.int32)
    voxels = torch.empty(m, 3, device=dev, dtype=torch.int32)
    if m > 0:
        _lib.check(lib.colvo_fuse_write(_lib.ptr(ws), _lib.ptr(pool), n_bricks, int(min_obs), *origin, vs, *dims, _lib.ptr(ews),
                                        m, _lib.ptr(points), _lib.ptr(out_colors), _lib.ptr(counts), _lib.ptr(voxels), stream),
                   "colvo_fuse_write")
    return FusedCloud(points, out_colors, counts, voxels, origin, dims, vs, n_input, n_outside, n_bricks, n_voxels)


class Consistency(NamedTuple):
    """The policy of filter_depths; also what reconstruct_sequence takes.  The defaults are choices, not tuned values."""
    window: int = 2          # neighbours i +/- k*step, k = 1..window, that exist in [0, N)
    step: int = 1            # frame distance between neighbours (a wider baseline discriminates better)
    rel_tol: float = 0.01    # agree iff |P_z - s| / (P_z + s) < rel_tol
    min_agree: int = 1       # keep iff agree >= min_agree ...
    max_violated: int = 0    # ... and violated <= max_violated


class ConsistencyResult(NamedTuple):
    depths: torch.Tensor     # [N,1,H,W] float32: the input depth where kept, +inf elsewhere
    votes: torch.Tensor      # [N,3,H,W] uint8: planes agree / occluded / violated
    stats: torch.Tensor      # [N,5] int32: candidates, kept, no_view, few_agree, violated_out


def _check_consistency(who: str, window, step, rel_tol, min_agree, max_violated, max_depth) -> None:
    for name, val in (("window", window), ("step", step), ("min_agree", min_agree), ("max_violated", max_violated)):
        if isinstance(val, bool) or not isinstance(val, int):
            raise ValueError(f"{who}: {name} must be an int, got {val!r}")
    if not 1 <= window <= 16:
        raise ValueError(f"{who}: window must be in 1..16, got {window}")
    if step < 1:
        raise ValueError(f"{who}: step must be >= 1, got {step}")
    if min_agree < 0 or max_violated < 0:
        raise ValueError(f"{who}: min_agree and max_violated must be >= 0, got {min_agree}, {max_violated}")
    if min_agree > 2 * window:
        raise ValueError(f"{who}: min_agree {min_agree} can never be reached with 2 * window = {2 * window} neighbours")
    for name, val in (("rel_tol", rel_tol), ("max_depth", max_depth)):
        try:
            ok = math.isfinite(_f32(val)) and _f32(val) > 0.0
        except (TypeError, ValueError, OverflowError, struct.error):
            ok = False
        if not ok:
            raise ValueError(f"{who}: {name} must be finite and positive (as float32), got {val!r}")


def filter_depths(depths: torch.Tensor, K: torch.Tensor, cam2world: torch.Tensor, *, window: int = 2, step: int = 1,
                  rel_tol: float = 0.01, min_agree: int = 1, max_violated: int = 0,
                  max_depth: float = MAX_DEPTH) -> ConsistencyResult:
    """Multi-view consistency check of a sequence's depth maps (contract: include/colvo.h colvo_consistency_filter, DESIGN.md
    §3.6f; csrc/consistency.hip).  depths [N,1,H,W], K [N,3,3] (per frame), cam2world [N,4,4], float32 on the device.  Every
    pixel with 0 < d < max_depth is carried through the trajectory into the frames i +/- k*step, k = 1..window, that exist;
    a neighbour that sees the point (in front, inside the image, four valid taps) AGREES if |P_z - s| / (P_z + s) < rel_tol
    for its own interpolated depth s, is OCCLUDED if s < P_z (legitimate: it does not count against the pixel) and is
    VIOLATED otherwise (the neighbour sees through the point).  A pixel is kept iff agree >= min_agree and violated <=
    max_violated.  N = 1, or a window * step that reaches past the sequence, is legal: those neighbours do not exist.

    A rejected pixel, and one that never was a candidate, is written as +inf, not 0: stitch_point_cloud keeps d < max_depth,
    so 0 would pass and put a point at the camera centre; fuse_point_cloud and localize_polyps keep 0 < d < max_depth.  +inf
    is dropped by all three, so the result feeds them unchanged.  No read-back and no host synchronisation."""
    _check_consistency("filter_depths", window, step, rel_tol, min_agree, max_violated, max_depth)
    if not isinstance(depths, torch.Tensor) or depths.dim() != 4:
        raise ValueError("filter_depths: depths must be [N,1,H,W]")
    N, _, H, W = depths.shape
    depths = _chk(depths, "depths", (N, 1, H, W))
    K = _chk(K, "K", (N, 3, 3))
    cam2world = _chk(cam2world, "cam2world", (N, 4, 4))
    lib = _lib.load()
    ws_bytes = int(lib.colvo_consistency_workspace_bytes(N, window))
    if ws_bytes == 0 or H <= 0 or W <= 0 or H * W >= 1 << 30:
        raise ValueError(f"filter_depths: shape N={N} H={H} W={W} beyond the kernels' limits (N <= 65535, H*W < 2^30)")
    dev = depths.device
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    out = torch.empty(N, 1, H, W, device=dev, dtype=torch.float32)
    votes = torch.empty(N, 3, H, W, device=dev, dtype=torch.uint8)
    stats = torch.empty(N, 5, device=dev, dtype=torch.int32)
    _lib.check(lib.colvo_consistency_filter(_lib.ptr(depths), _lib.ptr(K), _lib.ptr(cam2world), N, H, W, window, min(step, 1 << 30),
                                            float(rel_tol), min_agree, max_violated, float(max_depth), _lib.ptr(ws), _lib.ptr(out),
                                            _lib.ptr(votes), _lib.ptr(stats), _lib.stream_ptr()), "colvo_consistency_filter")
    return ConsistencyResult(out, votes, stats)


def write_ply(path, points: torch.Tensor, colors: Optional[torch.Tensor] = None) -> None:
    """Binary little-endian PLY: `float x y z` per vertex and, with colours [M,3] in [0,1], `uchar red green blue`
    (rint(c * 255), clamped).  Host code; one device -> host copy."""
    import numpy as np
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("write_ply: points must be [M,3]")
    if colors is not None and tuple(colors.shape) != tuple(points.shape):
        raise ValueError("write_ply: colors must have the shape of points")
    both = points.detach().to(torch.float32) if colors is None else torch.cat(
        [points.detach().to(torch.float32), colors.detach().to(points.device, torch.float32)], dim=1)
    host = both.cpu().numpy()
    m = host.shape[0]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {m}", "property float x", "property float y",
              "property float z"]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header.append("end_header")
    rows = np.empty(m, dtype=np.dtype(fields))
    for a, name in enumerate("xyz"):
        rows[name] = host[:, a]
    if colors is not None:
        q = np.clip(np.rint(np.nan_to_num(host[:, 3:6], nan=0.0) * 255.0), 0, 255).astype(np.uint8)
        for k, name in enumerate(("red", "green", "blue")):
            rows[name] = q[:, k]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(rows.tobytes())


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
    None."""
    polyps = None               # Optional[PolypLocalization]
    consistency = None          # Optional[ConsistencyResult]

    def __new__(cls, depths, rel_poses, cam2world, points, fused=None, polyps=None, consistency=None):
        self = super().__new__(cls, depths, rel_poses, cam2world, points, fused)
        self.polyps = polyps
        self.consistency = consistency
        return self

    def _replace(self, **kw):
        polyps = kw.pop("polyps", self.polyps)
        consistency = kw.pop("consistency", self.consistency)
        return type(self)(*super()._replace(**kw), polyps=polyps, consistency=consistency)


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
                         num_labels: Optional[int] = None, consistency: Optional[Consistency] = None) -> Reconstruction:
    """frames [N+1,3,H,W] of one sequence, K [3,3] or [N+1,3,3] -> depth of every frame, the pose of every consecutive
    pair (DCDP: PoseNet sees both depth maps), the integrated trajectory and the stitched cloud.  With a voxel_size also
    the fused cloud of the same samples, coloured by the frames (fuse_point_cloud; `fused`, else None).  With labels
    [N+1,1,H,W] uint8 and num_labels also the polyps they mark, localised from the same depths, K, trajectory and max_depth at
    stride 1 (localize.localize_polyps; `polyps`, else None).  With a Consistency policy the depth maps first pass
    filter_depths along the integrated trajectory (same K and max_depth): points, fused and polyps are computed from the
    filtered depths, `depths` stays the raw network output and the ConsistencyResult is `consistency` (else None)."""
    n = frames.shape[0]
    if n < 2:
        raise ValueError("reconstruct_sequence: need at least two frames")
    if labels is not None and num_labels is None:
        raise ValueError("reconstruct_sequence: labels need num_labels")
    if consistency is not None:
        consistency = Consistency(*consistency)
        _check_consistency("reconstruct_sequence", *consistency, max_depth)
    if K.dim() == 2:
        K = K.unsqueeze(0).expand(n, 3, 3)
    K = K.to(frames.device, torch.float32).contiguous()
    depths, rel = run_networks(depth_net, pose_net, frames, chunk=chunk)
    traj = integrate_trajectory(rel)
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
        from . import localize                       # (localize imports this module)
        polyps = localize.localize_polyps(depths, labels, K, traj32, num_labels=num_labels, stride=1, max_depth=max_depth)
    return Reconstruction(raw, rel, traj, cloud, fused, polyps, checked)
