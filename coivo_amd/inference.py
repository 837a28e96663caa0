"""Inference side of the path: depth maps + relative poses -> trajectory -> stitched point cloud, and
the coloured, voxel-averaged cloud fused from it; refine_edges / refine_trajectory correct the trajectory
against the depth maps and frames it connects (csrc/refine.hip).

Reference: README.md:9 ("complete 3D reconstruction of the intestine"), README.md:29 ("stitching together the dense depth
maps of each frame using the colonoscopic trajectory").  filter_depths is the cross-view check in front of both (DESIGN.md
§3.6f, csrc/consistency.hip).  Spec: oracle/colvo_spec.py integrate_trajectory / backproject /
stitch_point_cloud (oracle/SPEC.md §6c).  The per-pixel work runs in csrc/reconstruct.hip; the trajectory integration is N
products of 4x4 matrices and is done on the host in float64 (it is control flow, not a kernel).  The fusion runs in
csrc/fuse.hip.  render_cloud / render_fused draw a cloud back into camera views (csrc/render.hip).
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


class TsdfVolume(NamedTuple):
    pool: torch.Tensor              # [n_bricks*512, 2] int32: (sum q, n) per voxel, row slot * 512 + (lz * 8 + ly) * 8 + lx
    color_sums: Optional[torch.Tensor]   # [n_bricks*512, 4] int32: sums of the colour quanta (r, g, b, 0); None without colours
    brick_list: torch.Tensor        # [n_bricks] int32: the allocated bricks, ascending (bz * nby + by) * nbx + bx
    table: torch.Tensor             # [bricks of the grid] int32: slot of each brick, -1 where not allocated
    origin: Tuple[float, float, float]   # lower corner of the grid (float32 values)
    dims: Tuple[int, int, int]      # voxels per axis
    voxel_size: float               # as float32
    trunc: float                    # truncation distance, a whole number of voxels (as float32)
    has_colors: bool
    n_input: int                    # walked samples with 0 < depth < max_depth
    n_outside: int                  # ... of which outside the grid
    n_bricks: int                   # allocated 8x8x8 bricks


class Mesh(NamedTuple):
    vertices: torch.Tensor          # [V,3] float32: one per active cell, in (brick, voxel in brick) order of the cell's minimum corner
    faces: torch.Tensor             # [F,3] int32: triangles, wound so that the normal points to free space (the camera side)
    colors: Optional[torch.Tensor]  # [V,3] float32 in [0,1] (None without colours)
    normals: torch.Tensor           # [V,3] float32: unit gradient of the distance field, towards free space; 0 for a zero gradient
    cells: torch.Tensor             # [V,3] int32: the cell (ix, iy, iz) of each vertex
    n_open: int                     # cells with a sign change among their observed corners and one or more corners not observed


class Meshing(NamedTuple):
    """reconstruct_sequence's meshing policy: fuse_tsdf's trunc and extract_mesh's min_obs.  The defaults are choices, not tuned
    values."""
    trunc: Optional[float] = None   # None: four voxels
    min_obs: int = 2


def _tsdf_voxels(who: str, voxel_size, trunc):
    """(voxel_size as float32, T): trunc must be a whole number T of voxels, 1 <= T <= 7; None is four voxels."""
    vs = _f32(voxel_size)
    if not (vs > 0.0 and math.isfinite(vs)):
        raise ValueError(f"{who}: voxel_size must be finite and positive")
    if trunc is None:
        return vs, 4
    if isinstance(trunc, bool) or not isinstance(trunc, (int, float)) or not math.isfinite(trunc) or not trunc > 0.0:
        raise ValueError(f"{who}: trunc must be a whole number of voxels, 1 to 7 of them (or None: four), got {trunc!r}")
    T = int(round(float(trunc) / vs))
    if not 1 <= T <= 7 or abs(float(trunc) - T * vs) > 1e-5 * float(trunc):
        raise ValueError(f"{who}: trunc must be a whole number of voxels, 1 to 7 of them (a band of T + 1 voxels never skips an "
                         f"8-voxel brick), got {trunc!r} = {float(trunc) / vs:.6g} voxels of {vs}")
    return vs, T


def fuse_tsdf(depths: torch.Tensor, K: torch.Tensor, cam2world: torch.Tensor, *, voxel_size: float, trunc: Optional[float] = None,
              colors: Optional[torch.Tensor] = None, stride: int = 1, max_depth: float = MAX_DEPTH, origin=None,
              dims=None) -> TsdfVolume:
    """Depth maps along a trajectory -> a truncated signed distance volume over fuse_point_cloud's grid (contract: include/colvo.h
    colvo_tsdf_*; csrc/tsdf.hip).  Every `stride`-th pixel with 0 < depth < max_depth allocates the 8x8x8 bricks
    within trunc + one voxel of its surface point along its ray; every voxel of an allocated brick then looks itself up in every
    frame's full-resolution depth map and adds the quantised, truncated distance d - z (in units of trunc / 4096) and a count, and
    with colors [N,3,H,W] the pixel's colour.  A voxel in front of the surface by more than trunc votes +1: frames that look through
    a floater outvote it.  A voxel behind the surface by more than trunc is not observed by that frame.  `trunc` must be a whole
    number of voxels, 1 to 7; None is four -- a choice, not a tuned value.  Integer sums: the volume is bit-identical between calls,
    streams and frame orders and equals the NumPy replica tests/tsdf_ref.py.  origin / dims default to fusion_grid's.  Reads one
    12-byte statistics block back after the plan to size the pool.  Not incremental: a call builds a volume from all its frames."""
    who = "fuse_tsdf"
    lib = _lib.load()
    if not isinstance(depths, torch.Tensor) or depths.dim() != 4:
        raise ValueError(f"{who}: depths must be [N,1,H,W]")
    N, _, H, W = depths.shape
    if isinstance(stride, bool) or not isinstance(stride, int) or stride < 1:
        raise ValueError(f"{who}: stride must be an int >= 1, got {stride!r}")
    if not _finite_pos32(max_depth):
        raise ValueError(f"{who}: max_depth must be finite and positive (as float32), got {max_depth!r}")
    vs, T = _tsdf_voxels(who, voxel_size, trunc)
    depths = _chk(depths, "depths", (N, 1, H, W))
    K = _chk(K, "K", (N, 3, 3))
    cam2world = _chk(cam2world, "cam2world", (N, 4, 4))
    if colors is not None:
        colors = _chk(colors, "colors", (N, 3, H, W))
    if (origin is None) != (dims is None):
        raise ValueError(f"{who}: give origin and dims together, or neither")
    if origin is None:
        origin, dims = fusion_grid(K, cam2world, H, W, vs, max_depth)
    origin = tuple(_f32(o) for o in origin)
    dims = tuple(int(d) for d in dims)
    if len(origin) != 3 or len(dims) != 3 or any(d <= 0 or d % 8 for d in dims):
        raise ValueError(f"{who}: dims must be three positive multiples of 8, got {dims}")
    scratch_bytes = int(lib.colvo_tsdf_plan_scratch_bytes(N, H, W, stride, *dims))
    if scratch_bytes == 0:
        raise ValueError(f"{who}: shape N={N} H={H} W={W} stride={stride} or grid {dims} beyond the kernels' limits")
    dev = depths.device
    total = (dims[0] // 8) * (dims[1] // 8) * (dims[2] // 8)
    scratch = torch.empty(scratch_bytes, device=dev, dtype=torch.uint8)
    table = torch.empty(total, device=dev, dtype=torch.int32)
    brick_list = torch.empty(min(total, 1 << 22), device=dev, dtype=torch.int32)
    stats = torch.empty(3, device=dev, dtype=torch.int32)
    stream = _lib.stream_ptr()
    _lib.check(lib.colvo_tsdf_plan(_lib.ptr(depths), _lib.ptr(K), _lib.ptr(cam2world), N, H, W, stride, float(max_depth), *origin, vs,
                                   *dims, T, _lib.ptr(scratch), _lib.ptr(table), _lib.ptr(brick_list), _lib.ptr(stats), stream),
               "colvo_tsdf_plan")
    n_input, n_outside, n_bricks = (int(v) for v in stats.tolist())
    if n_bricks >= 1 << 22:
        raise RuntimeError(f"{who}: {n_bricks} allocated bricks, the limit is 2^22 - 1: use a larger voxel_size")
    pool = torch.empty(n_bricks * 512, 2, device=dev, dtype=torch.int32)
    sums = torch.empty(n_bricks * 512, 4, device=dev, dtype=torch.int32) if colors is not None else None
    if n_bricks > 0:
        _lib.check(lib.colvo_tsdf_integrate(_lib.ptr(depths), _lib.ptr(colors), _lib.ptr(K), _lib.ptr(cam2world), N, H, W,
                                            float(max_depth), *origin, vs, *dims, T, _lib.ptr(brick_list), n_bricks, _lib.ptr(pool),
                                            _lib.ptr(sums), 0, stream), "colvo_tsdf_integrate")
    return TsdfVolume(pool, sums, brick_list[:n_bricks], table, origin, dims, vs, _f32(_f32(T) * vs), colors is not None, n_input,
                      n_outside, n_bricks)


def extract_mesh(volume: TsdfVolume, *, min_obs: int = 1) -> Mesh:
    """The zero surface of a TsdfVolume as an indexed triangle mesh by surface nets (contract: include/colvo.h colvo_tsdf_mesh_*,
    DESIGN.md §3.6m).  A voxel counts as observed with at least `min_obs` observations and as inside iff its integer sum is negative,
    so the topology never depends on a rounding.  A cell of 2x2x2 voxels that are all observed and of mixed sign gets one vertex --
    the mean of the sign changes along its edges --, a colour and a normal (the field's gradient, towards free space); a grid edge
    with a sign change and four such cells around it gets one quad, written as two triangles wound towards free space.  Vertices are
    shared by construction.  `n_open` counts the cells that would have had a vertex but for a corner that is not observed: what the
    band's edge and min_obs cost.  Every output bit is a function of the volume alone and equals tests/tsdf_ref.py.  A mesh's
    vertices are a cloud: evaluate.cloud_metrics(mesh.vertices, gt_points, ...) scores it.  Reads two small counts back (vertices,
    then triangles) to size the outputs.  No hole filling, no simplification."""
    who = "extract_mesh"
    if not isinstance(volume, TsdfVolume):
        raise ValueError(f"{who}: volume must be a TsdfVolume")
    if isinstance(min_obs, bool) or not isinstance(min_obs, int) or min_obs < 1:
        raise ValueError(f"{who}: min_obs must be an int >= 1, got {min_obs!r}")
    lib = _lib.load()
    dev = volume.table.device
    n_bricks = int(volume.n_bricks)
    origin = tuple(_f32(o) for o in volume.origin)
    dims = tuple(int(d) for d in volume.dims)
    vs = _f32(volume.voxel_size)
    V = F = n_open = 0
    stream = _lib.stream_ptr()
    if n_bricks > 0:
        if tuple(volume.pool.shape) != (n_bricks * 512, 2) or volume.pool.dtype != torch.int32 or not volume.pool.is_contiguous():
            raise ValueError(f"{who}: volume.pool must be a contiguous [n_bricks*512, 2] int32 tensor")
        scratch_bytes = int(lib.colvo_tsdf_mesh_scratch_bytes(n_bricks))
        if scratch_bytes == 0:
            raise ValueError(f"{who}: n_bricks {n_bricks} beyond the kernels' limits")
        scratch = torch.empty(scratch_bytes, device=dev, dtype=torch.uint8)
        stats2 = torch.empty(3, device=dev, dtype=torch.int32)
        bricks = (_lib.ptr(volume.table), _lib.ptr(volume.brick_list), n_bricks)
        _lib.check(lib.colvo_tsdf_mesh_count(_lib.ptr(volume.pool), *bricks, min_obs, *dims, _lib.ptr(scratch), _lib.ptr(stats2),
                                             stream), "colvo_tsdf_mesh_count")
        V, n_open = (int(v) for v in stats2[:2].tolist())
    vertices = torch.empty(V, 3, device=dev, dtype=torch.float32)
    normals = torch.empty(V, 3, device=dev, dtype=torch.float32)
    colors = torch.empty(V, 3, device=dev, dtype=torch.float32) if volume.color_sums is not None else None
    cells = torch.empty(V, 3, device=dev, dtype=torch.int32)
    if V > 0:
        vid = torch.empty(n_bricks * 512, device=dev, dtype=torch.int32)
        _lib.check(lib.colvo_tsdf_mesh_vertices(_lib.ptr(volume.pool), _lib.ptr(volume.color_sums), *bricks, min_obs, *origin, vs,
                                                *dims, _lib.ptr(scratch), V, _lib.ptr(vertices), _lib.ptr(colors), _lib.ptr(normals),
                                                _lib.ptr(cells), _lib.ptr(vid), stats2[2:].data_ptr(), stream),
                   "colvo_tsdf_mesh_vertices")
        F = int(stats2[2].item())
    faces = torch.empty(F, 3, device=dev, dtype=torch.int32)
    if F > 0:
        _lib.check(lib.colvo_tsdf_mesh_faces(_lib.ptr(volume.pool), *bricks, *dims, _lib.ptr(scratch), _lib.ptr(vid), F,
                                             _lib.ptr(faces), stream), "colvo_tsdf_mesh_faces")
    return Mesh(vertices, faces, colors, normals, cells, n_open)


class CloudNormals(NamedTuple):
    normals: torch.Tensor           # [M,3] float32: unit normal of each row of the cloud in the world frame, facing the cameras; 0 without one
    counts: torch.Tensor            # [M]   int32: samples that gave the row a normal
    coherence: torch.Tensor         # [M]   float32: |sum of the samples' unit normals| / count: 1 where they agree, towards 0 as they do not
    stats: torch.Tensor             # [4]   int32: samples kept, with a normal, ... in a row of the cloud, ... in no row


def cloud_normals(fused: FusedCloud, depths: torch.Tensor, K: torch.Tensor, cam2world: torch.Tensor, *, stride: int = 1,
                  max_depth: float = MAX_DEPTH, rel_edge: float = 0.05) -> CloudNormals:
    """Surface normals of a fused cloud (contract: include/colvo.h colvo_cloud_normals; csrc/normals.hip).  Every
    sample the fusion walked gets a finite-difference normal from its own depth map -- neighbours one pixel away, one-sided at the
    image border and wherever the relative depth difference |d_b - d_c| / (d_b + d_c) reaches `rel_edge`, so that no normal is taken
    across an occlusion edge --, faced to its camera, turned into the world frame and quantised to 2^-14.  The normals of the samples
    of a voxel are summed as integers in the voxel's row; the row's normal is the sum's direction and its coherence the sum's length
    per sample: 1 where all observations agree on the orientation, falling towards 0 at floaters, fold edges and bad poses.

    `depths`, `K`, `cam2world`, `stride` and `max_depth` MUST be those given to fuse_point_cloud (the grid comes from `fused`):
    a sample is matched to its row by the fusion's own voxel arithmetic, and samples of other depths, strides or poses end in the
    unmatched count stats[3] -- as do the samples of voxels below the cloud's min_obs and those outside the grid.  `rel_edge = 0.05`
    is a choice, not a tuned value.  Integer sums: identical bits on every call, stream and frame order, equal to the NumPy replica
    tests/normals_ref.py.  No read-back and no host synchronisation."""
    who = "cloud_normals"
    if not isinstance(fused, FusedCloud):
        raise ValueError(f"{who}: fused must be a FusedCloud")
    if not isinstance(depths, torch.Tensor) or depths.dim() != 4:
        raise ValueError(f"{who}: depths must be [N,1,H,W]")
    if isinstance(stride, bool) or not isinstance(stride, int) or stride < 1:
        raise ValueError(f"{who}: stride must be an int >= 1, got {stride!r}")
    if not _finite_pos32(max_depth):
        raise ValueError(f"{who}: max_depth must be finite and positive (as float32), got {max_depth!r}")
    if not _finite_pos32(rel_edge):
        raise ValueError(f"{who}: rel_edge must be finite and positive (as float32), got {rel_edge!r}")
    N, _, H, W = depths.shape
    origin = tuple(_f32(o) for o in fused.origin)
    dims = tuple(int(d) for d in fused.dims)
    vs = _f32(fused.voxel_size)
    if len(origin) != 3 or len(dims) != 3 or any(d <= 0 or d % 8 for d in dims) or not (vs > 0.0 and math.isfinite(vs)):
        raise ValueError(f"{who}: fused carries no valid grid (origin {origin}, dims {dims}, voxel_size {vs})")
    lib = _lib.load()
    if int(lib.colvo_fuse_plan_workspace_bytes(N, H, W, stride, *dims)) == 0:
        raise ValueError(f"{who}: shape N={N} H={H} W={W} stride={stride} or grid {dims} beyond the kernels' limits")
    depths = _chk(depths, "depths", (N, 1, H, W))
    K = _chk(K, "K", (N, 3, 3))
    cam2world = _chk(cam2world, "cam2world", (N, 4, 4))
    m = int(fused.voxels.shape[0])
    voxels = fused.voxels
    if voxels.dtype != torch.int32 or tuple(voxels.shape) != (m, 3) or voxels.device != depths.device:
        raise ValueError(f"{who}: fused.voxels must be [M,3] int32 on the device of depths")
    voxels = voxels.contiguous()
    dev = depths.device
    scratch = torch.empty(int(lib.colvo_cloud_normals_scratch_bytes(m)), device=dev, dtype=torch.uint8)
    normals = torch.empty(m, 3, device=dev, dtype=torch.float32)
    counts = torch.empty(m, device=dev, dtype=torch.int32)
    coherence = torch.empty(m, device=dev, dtype=torch.float32)
    stats = torch.empty(4, device=dev, dtype=torch.int32)
    _lib.check(lib.colvo_cloud_normals(_lib.ptr(depths), _lib.ptr(K), _lib.ptr(cam2world), N, H, W, stride, float(max_depth), *origin,
                                       vs, *dims, _lib.ptr(voxels), m, float(rel_edge), _lib.ptr(scratch), _lib.ptr(normals),
                                       _lib.ptr(counts), _lib.ptr(coherence), _lib.ptr(stats), _lib.stream_ptr()),
               "colvo_cloud_normals")
    return CloudNormals(normals, counts, coherence, stats)


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


class Refinement(NamedTuple):
    """The policy of refine_edges / refine_trajectory; also what reconstruct_sequence takes.  The defaults are choices, not values
    tuned on colonoscopy data (none is here): what the tests establish is on a synthetic textured tube."""
    iterations: int = 6          # Gauss-Newton steps
    sigma_geo: float = 0.01      # whitening of the geometric residual (P_z - s) / (P_z + s)
    sigma_photo: float = 0.02    # ... of the photometric residual (a c + b) - I_i, intensities in [0, 1]
    gate_geo: float = 0.05       # a geometric sample is used iff |residual| < gate_geo
    gate_photo: float = 0.1      # a photometric sample is used iff |residual| < gate_photo
    damping: float = 1e-6        # H + damping * diag(H)
    min_samples: int = 256       # an edge with fewer visible samples keeps its input
    geometric: bool = True       # alone, the geometric term is ill-conditioned in a tube: both terms are on by default
    photometric: bool = True
    brightness: bool = True      # solve a gain and an offset per edge alongside the pose (needs the photometric term)


class RefinementResult(NamedTuple):
    T: torch.Tensor          # [E,4,4] float64: frame-i camera coordinates -> frame j
    gain: torch.Tensor       # [E] float64
    offset: torch.Tensor     # [E] float64
    history: torch.Tensor    # [E, iterations + 1, 5] float64: n_visible, n_geo, C_g, n_photo, C_p of every evaluation
    status: torch.Tensor     # [E] int32: REFINE_OK, _TOO_FEW, _NOT_PD, _REVERTED, _BAD_EDGE


REFINE_OK, REFINE_TOO_FEW, REFINE_NOT_PD, REFINE_REVERTED, REFINE_BAD_EDGE = range(5)


def _finite_pos32(val) -> bool:
    try:
        return math.isfinite(_f32(val)) and _f32(val) > 0.0
    except (TypeError, ValueError, OverflowError, struct.error):
        return False


def _check_refinement(who: str, policy: Refinement, max_depth) -> int:
    """ValueError for what colvo_refine_edges would refuse; -> the `terms` bits."""
    for name in ("iterations", "min_samples"):
        val = getattr(policy, name)
        if isinstance(val, bool) or not isinstance(val, int):
            raise ValueError(f"{who}: {name} must be an int, got {val!r}")
    if not 1 <= policy.iterations <= 64:
        raise ValueError(f"{who}: iterations must be in 1..64, got {policy.iterations}")
    if policy.min_samples < 1:
        raise ValueError(f"{who}: min_samples must be >= 1, got {policy.min_samples}")
    for name, val in (("sigma_geo", policy.sigma_geo), ("sigma_photo", policy.sigma_photo), ("gate_geo", policy.gate_geo),
                      ("gate_photo", policy.gate_photo), ("max_depth", max_depth)):
        if not _finite_pos32(val):
            raise ValueError(f"{who}: {name} must be finite and positive (as float32), got {val!r}")
    try:
        ok = math.isfinite(float(policy.damping)) and float(policy.damping) >= 0.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{who}: damping must be finite and >= 0, got {policy.damping!r}")
    for name in ("geometric", "photometric", "brightness"):
        if not isinstance(getattr(policy, name), (bool, int)):
            raise ValueError(f"{who}: {name} must be a bool, got {getattr(policy, name)!r}")
    if not (policy.geometric or policy.photometric):
        raise ValueError(f"{who}: at least one of the geometric and the photometric term must be enabled")
    return (1 if policy.geometric else 0) | (2 if policy.photometric else 0) | (4 if policy.brightness else 0)


def _refine_inputs(who: str, depths, frames, K, edges_ij, T):
    """Checked inputs of the refinement calls: (depths, frames, K, edges [E,2] int32 on the device, T [E,4,4] float64 on the device,
    N, H, W, E).  edges_ij is host data -- a sequence of (i, j) or an integer CPU tensor [E,2] -- so that a bad edge is a ValueError
    here and not a status on the device."""
    if not isinstance(depths, torch.Tensor) or depths.dim() != 4:
        raise ValueError(f"{who}: depths must be [N,1,H,W]")
    N, _, H, W = depths.shape
    depths = _chk(depths, "depths", (N, 1, H, W))
    frames = _chk(frames, "frames", (N, 3, H, W))
    K = _chk(K, "K", (N, 3, 3))
    if isinstance(edges_ij, torch.Tensor):
        if edges_ij.is_cuda or edges_ij.is_floating_point():
            raise ValueError(f"{who}: edges_ij must be host data: a sequence of (i, j) or an integer CPU tensor [E,2]")
        edges_ij = edges_ij.tolist()
    try:
        pairs = [(int(i), int(j)) for i, j in edges_ij]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: edges_ij must be a sequence of (i, j)") from None
    E = len(pairs)
    if not 1 <= E <= 65535 or N > 65535 or H <= 0 or W <= 0 or H * W >= 1 << 30:
        raise ValueError(f"{who}: E={E} N={N} H={H} W={W} beyond the kernels' limits (1 <= E <= 65535, N <= 65535, H*W < 2^30)")
    for i, j in pairs:
        if not (0 <= i < N and 0 <= j < N) or i == j:
            raise ValueError(f"{who}: bad edge ({i}, {j}): i != j, both in [0, {N})")
    if not isinstance(T, torch.Tensor) or T.dtype != torch.float64 or tuple(T.shape) != (E, 4, 4):
        raise ValueError(f"{who}: T must be a float64 tensor of shape ({E}, 4, 4), got {getattr(T, 'dtype', None)} "
                         f"{tuple(getattr(T, 'shape', ()))}")
    edges = torch.tensor(pairs, dtype=torch.int32).to(depths.device)
    return depths, frames, K, edges, T.to(depths.device).contiguous(), N, H, W, E


def refine_accumulate(depths: torch.Tensor, frames: torch.Tensor, K: torch.Tensor, edges_ij, T: torch.Tensor, *,
                      gain: Optional[torch.Tensor] = None, offset: Optional[torch.Tensor] = None, sigma_geo: float = 0.01,
                      sigma_photo: float = 0.02, gate_geo: float = 0.05, gate_photo: float = 0.1, geometric: bool = True,
                      photometric: bool = True, max_depth: float = MAX_DEPTH):
    """One evaluation of the refinement's sums at the edge states given (contract: include/colvo.h colvo_refine_accumulate):
    -> (sums [E,48] float64: the 36 upper-triangle entries of sum J^T J, the 8 of sum J^T e, C_g, C_p, two zeros;
    counts [E,4] int32: n_visible, n_geo, n_photo, 0), on the device.  gain / offset [E] float64 default to 1 / 0."""
    who = "refine_accumulate"
    terms = _check_refinement(who, Refinement(sigma_geo=sigma_geo, sigma_photo=sigma_photo, gate_geo=gate_geo, gate_photo=gate_photo,
                                              geometric=geometric, photometric=photometric), max_depth) & 3
    depths, frames, K, edges, T, N, H, W, E = _refine_inputs(who, depths, frames, K, edges_ij, T)
    dev = depths.device
    for name, t in (("gain", gain), ("offset", offset)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != (E,)):
            raise ValueError(f"{who}: {name} must be a float64 tensor of shape ({E},)")
    gain = None if gain is None else gain.to(dev).contiguous()
    offset = None if offset is None else offset.to(dev).contiguous()
    lib = _lib.load()
    ws = torch.empty(int(lib.colvo_refine_workspace_bytes(E, N, H, W, 1)), device=dev, dtype=torch.uint8)
    sums = torch.empty(E, 48, device=dev, dtype=torch.float64)
    counts = torch.empty(E, 4, device=dev, dtype=torch.int32)
    _lib.check(lib.colvo_refine_accumulate(_lib.ptr(depths), _lib.ptr(frames), _lib.ptr(K), N, H, W, _lib.ptr(edges), E, _lib.ptr(T),
                                           _lib.ptr(gain), _lib.ptr(offset), float(sigma_geo), float(sigma_photo), float(gate_geo),
                                           float(gate_photo), terms, float(max_depth), _lib.ptr(ws), _lib.ptr(sums), _lib.ptr(counts),
                                           _lib.stream_ptr()), "colvo_refine_accumulate")
    return sums, counts


def refine_edges(depths: torch.Tensor, frames: torch.Tensor, K: torch.Tensor, edges_ij, T_init: torch.Tensor, *,
                 iterations: int = 6, sigma_geo: float = 0.01, sigma_photo: float = 0.02, gate_geo: float = 0.05,
                 gate_photo: float = 0.1, damping: float = 1e-6, min_samples: int = 256, geometric: bool = True,
                 photometric: bool = True, brightness: bool = True, max_depth: float = MAX_DEPTH) -> RefinementResult:
    """Dense direct alignment of every edge (i, j, T) (contract: include/colvo.h colvo_refine_edges, DESIGN.md §3.6g;
    csrc/refine.hip).  depths [N,1,H,W], frames [N,3,H,W] in [0,1], K [N,3,3] (per frame), float32 on the device; edges_ij host data (a
    sequence of (i, j) or an integer CPU tensor [E,2], i != j, both in [0, N)); T_init [E,4,4] float64, T maps frame-i camera
    coordinates into frame j.  `iterations` Gauss-Newton steps on the geometric residual (P_z - s) / (P_z + s) and the photometric
    residual (a c + b) - I_i of every pixel of frame i that frame j sees, with a gain a and an offset b per edge; hard gates; float32
    per sample, float64 sums in a fixed order, float64 solve on the device.  An edge with fewer than min_samples visible samples or a
    normal matrix that is not positive definite keeps its input (status REFINE_TOO_FEW / REFINE_NOT_PD); one whose truncated cost per
    visible sample ends above where it started is reverted to it (REFINE_REVERTED).  Everything stays on the device: no read-back and
    no host synchronisation (the edge list is uploaded)."""
    who = "refine_edges"
    policy = Refinement(iterations, sigma_geo, sigma_photo, gate_geo, gate_photo, damping, min_samples, geometric, photometric,
                        brightness)
    terms = _check_refinement(who, policy, max_depth)
    depths, frames, K, edges, T_init, N, H, W, E = _refine_inputs(who, depths, frames, K, edges_ij, T_init)
    dev = depths.device
    lib = _lib.load()
    ws = torch.empty(int(lib.colvo_refine_workspace_bytes(E, N, H, W, iterations)), device=dev, dtype=torch.uint8)
    T = torch.empty(E, 4, 4, device=dev, dtype=torch.float64)
    gain = torch.empty(E, device=dev, dtype=torch.float64)
    offset = torch.empty(E, device=dev, dtype=torch.float64)
    history = torch.empty(E, iterations + 1, 5, device=dev, dtype=torch.float64)
    status = torch.empty(E, device=dev, dtype=torch.int32)
    _lib.check(lib.colvo_refine_edges(_lib.ptr(depths), _lib.ptr(frames), _lib.ptr(K), N, H, W, _lib.ptr(edges), E, _lib.ptr(T_init),
                                      iterations, float(sigma_geo), float(sigma_photo), float(gate_geo), float(gate_photo),
                                      float(damping), min_samples, terms, float(max_depth), _lib.ptr(ws), _lib.ptr(T), _lib.ptr(gain),
                                      _lib.ptr(offset), _lib.ptr(history), _lib.ptr(status), _lib.stream_ptr()), "colvo_refine_edges")
    return RefinementResult(T, gain, offset, history, status)


def _rigid_inverse(T: torch.Tensor) -> torch.Tensor:
    R, t = T[:3, :3], T[:3, 3]
    out = torch.eye(4, dtype=torch.float64)
    out[:3, :3] = R.t()
    out[:3, 3] = -(R.t() @ t)
    return out


def refine_trajectory(depths: torch.Tensor, frames: torch.Tensor, K: torch.Tensor, cam2world: torch.Tensor, *,
                      max_depth: float = MAX_DEPTH, **policy):
    """Refines the N - 1 consecutive edges k -> k+1 of a trajectory (cam2world [N,4,4], any device; taken in float64):
    T_k = inverse(M_{k+1}) M_k, refine_edges with the Refinement policy given as keywords, one read-back of T, and the trajectory
    re-integrated from frame 0's pose exactly as integrate_trajectory does it, M_{k+1} = M_k inverse(T_k).
    -> (cam2world [N,4,4] float64 on the CPU, RefinementResult)."""
    policy = Refinement(**policy)
    if not isinstance(cam2world, torch.Tensor) or cam2world.dim() != 3 or tuple(cam2world.shape[1:]) != (4, 4):
        raise ValueError("refine_trajectory: cam2world must be [N,4,4]")
    M = cam2world.detach().to("cpu", torch.float64)
    n = M.shape[0]
    if n < 2:
        raise ValueError("refine_trajectory: need at least two frames")
    T0 = torch.stack([_rigid_inverse(M[k + 1]) @ M[k] for k in range(n - 1)])
    res = refine_edges(depths, frames, K, [(k, k + 1) for k in range(n - 1)], T0, **policy._asdict(), max_depth=max_depth)
    T = res.T.cpu()
    out = [M[0].clone()]
    for k in range(n - 1):
        out.append(out[-1] @ _rigid_inverse(T[k]))
    return torch.stack(out), res


class _RenderFields(NamedTuple):
    radius: Optional[float] = None   # world half-width of a splat; None: the fused cloud's voxel_size
    max_splat: int = 8               # largest half-width of a footprint in pixels


class Render(_RenderFields):
    """What reconstruct_sequence renders when asked: the fused cloud into every frame's own camera (render_fused).  The defaults
    are choices, not tuned values.  Behind the two fields -- it still unpacks into two -- `surfels`: True has the cloud's normals
    computed (cloud_normals) and the cloud drawn as oriented discs (render_surfels) instead of squares; and `mesh`: True has the
    extracted surface mesh drawn instead of the cloud (render_mesh; needs a Meshing policy, excludes surfels; radius and max_splat
    are not used)."""
    surfels = False
    mesh = False

    def __new__(cls, radius=None, max_splat=8, surfels=False, mesh=False):
        self = super().__new__(cls, radius, max_splat)
        self.surfels = surfels
        self.mesh = mesh
        return self

    def _replace(self, **kw):
        surfels = kw.pop("surfels", self.surfels)
        mesh = kw.pop("mesh", self.mesh)
        return type(self)(*super()._replace(**kw), surfels=surfels, mesh=mesh)

    def __repr__(self):
        return f"Render(radius={self.radius!r}, max_splat={self.max_splat!r}, surfels={self.surfels!r}, mesh={self.mesh!r})"


class RenderedViews(NamedTuple):
    depth: torch.Tensor              # [N,1,H,W] float32: camera-z of the nearest point, +inf where no point landed
    index: torch.Tensor              # [N,1,H,W] int32: its row in the cloud, -1 where empty
    colors: Optional[torch.Tensor]   # [N,3,H,W] float32: its colour, 0 where empty (None without colours)
    stats: torch.Tensor              # [N,4] int32: points in front, points drawn, points in front and clipped, covered pixels


def _check_render(who: str, radius, max_splat, max_depth) -> None:
    """ValueError for what colvo_render_cloud would refuse of the policy."""
    if isinstance(max_splat, bool) or not isinstance(max_splat, int):
        raise ValueError(f"{who}: max_splat must be an int, got {max_splat!r}")
    if not 0 <= max_splat <= 32:
        raise ValueError(f"{who}: max_splat must be in 0..32, got {max_splat}")
    try:
        ok = math.isfinite(_f32(radius)) and _f32(radius) >= 0.0
    except (TypeError, ValueError, OverflowError, struct.error):
        ok = False
    if not ok:
        raise ValueError(f"{who}: radius must be finite and >= 0 (as float32), got {radius!r}")
    if not _finite_pos32(max_depth):
        raise ValueError(f"{who}: max_depth must be finite and positive (as float32), got {max_depth!r}")


def render_cloud(points: torch.Tensor, K: torch.Tensor, cam2world: torch.Tensor, H: int, W: int, *, radius: float,
                 colors: Optional[torch.Tensor] = None, max_splat: int = 8, max_depth: float = MAX_DEPTH) -> RenderedViews:
    """A point cloud drawn into N camera views of H x W pixels (contract: include/colvo.h colvo_render_cloud, DESIGN.md §3.6j;
    csrc/render.hip).  points [M,3] in the world frame, colors [M,3] or None, K [3,3] or [N,3,3], cam2world [N,4,4], float32 on the
    device.  Every point in front of a camera (1e-3 < P_z < max_depth) is drawn as a screen-aligned square of world half-width
    `radius`, at most max_splat pixels to each side and at least its nearest pixel; a pixel keeps the nearest point, equal depths
    the smallest row.  The cameras need not be frames of the sequence.  Pinned float32 arithmetic, an integer minimum and integer
    sums: identical bits on every call and stream, equal to the NumPy replica tests/render_ref.py.

    A pixel no point landed on gets depth +inf and index -1: stitch_point_cloud, fuse_point_cloud, localize_polyps and
    filter_depths drop +inf, and `index >= 0` is the mask depth_metrics takes.  A square carries ONE depth: on a wall seen at a
    grazing angle the square of a nearer neighbour wins the pixel, so the rendered depth is biased towards the camera by about
    radius x slope (DESIGN.md §3.6j has the figures).  No read-back and no host synchronisation."""
    who = "render_cloud"
    _check_render(who, radius, max_splat, max_depth)
    for name, val in (("H", H), ("W", W)):
        if isinstance(val, bool) or not isinstance(val, int) or val < 1:
            raise ValueError(f"{who}: {name} must be a positive int, got {val!r}")
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{who}: points must be [M,3]")
    if not isinstance(cam2world, torch.Tensor) or cam2world.dim() != 3:
        raise ValueError(f"{who}: cam2world must be [N,4,4]")
    M, N = points.shape[0], cam2world.shape[0]
    if not 1 <= N <= 65535 or H * W >= 1 << 30 or N * H * W >= 1 << 31 or M >= 1 << 31:
        raise ValueError(f"{who}: M={M} N={N} H={H} W={W} beyond the kernels' limits (M < 2^31, 1 <= N <= 65535, H*W < 2^30, "
                         "N*H*W < 2^31)")
    points = _chk(points, "points", (M, 3))
    cam2world = _chk(cam2world, "cam2world", (N, 4, 4))
    if isinstance(K, torch.Tensor) and K.dim() == 2:
        K = K.unsqueeze(0).expand(N, 3, 3)
    K = _chk(K, "K", (N, 3, 3))
    if colors is not None:
        colors = _chk(colors, "colors", (M, 3))
    lib = _lib.load()
    dev = points.device
    scratch = torch.empty(int(lib.colvo_render_scratch_bytes(N, H, W)), device=dev, dtype=torch.uint8)
    depth = torch.empty(N, 1, H, W, device=dev, dtype=torch.float32)
    index = torch.empty(N, 1, H, W, device=dev, dtype=torch.int32)
    out_colors = torch.empty(N, 3, H, W, device=dev, dtype=torch.float32) if colors is not None else None
    stats = torch.empty(N, 4, device=dev, dtype=torch.int32)
    _lib.check(lib.colvo_render_cloud(_lib.ptr(points), _lib.ptr(colors), M, _lib.ptr(K), _lib.ptr(cam2world), N, H, W, float(radius),
                                      max_splat, float(max_depth), _lib.ptr(scratch), _lib.ptr(depth), _lib.ptr(index),
                                      _lib.ptr(out_colors), _lib.ptr(stats), _lib.stream_ptr()), "colvo_render_cloud")
    return RenderedViews(depth, index, out_colors, stats)


class SurfelViews(NamedTuple):
    depth: torch.Tensor              # [N,1,H,W] float32: camera-z where the pixel's ray meets the nearest disc, +inf where nothing landed
    index: torch.Tensor              # [N,1,H,W] int32: that point's row in the cloud, -1 where empty
    colors: Optional[torch.Tensor]   # [N,3,H,W] float32: its colour, 0 where empty (None without colours)
    normal: Optional[torch.Tensor]   # [N,3,H,W] float32: its normal in the camera frame, 0 where empty or without one (None unless asked)
    stats: torch.Tensor              # [N,6] int32: points in front, drawn, in front and clipped, covered pixels, culled, flat


def render_surfels(points: torch.Tensor, normals: torch.Tensor, K: torch.Tensor, cam2world: torch.Tensor, H: int, W: int, *,
                   radius: float, colors: Optional[torch.Tensor] = None, max_splat: int = 8, max_depth: float = MAX_DEPTH,
                   want_normals: bool = False) -> SurfelViews:
    """render_cloud with normals [M,3] in the world frame (contract: include/colvo.h colvo_render_surfels, DESIGN.md §3.6k;
    csrc/surfels.hip): a point is a disc of world radius `radius` perpendicular to its normal.  Each pixel of the point's footprint --
    the same rectangle as render_cloud's -- whose ray meets the disc's plane within `radius` of the point offers the depth of that
    meeting; the nearest pixel, when not hit, offers the point's own depth, so a point in front still lands somewhere.  The rendered
    depth of a wall seen at a grazing angle then lies on the wall instead of being biased towards the camera by radius x slope.  A
    point whose normal faces away from the camera is culled; a point whose normal is zero (or NaN) is drawn as render_cloud draws it
    and counted as flat.  want_normals: also the winner's camera-frame normal per pixel, to shade a preview with.  Pinned float32
    arithmetic, an integer minimum and integer sums: identical bits on every call and stream, equal to tests/surfel_ref.py.  A
    pixel only the nearest-pixel fallback reaches keeps the square's bias.  No read-back and no host synchronisation."""
    who = "render_surfels"
    _check_render(who, radius, max_splat, max_depth)
    for name, val in (("H", H), ("W", W)):
        if isinstance(val, bool) or not isinstance(val, int) or val < 1:
            raise ValueError(f"{who}: {name} must be a positive int, got {val!r}")
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{who}: points must be [M,3]")
    if not isinstance(normals, torch.Tensor) or tuple(normals.shape) != tuple(points.shape):
        raise ValueError(f"{who}: normals must have the shape of points")
    if not isinstance(cam2world, torch.Tensor) or cam2world.dim() != 3:
        raise ValueError(f"{who}: cam2world must be [N,4,4]")
    M, N = points.shape[0], cam2world.shape[0]
    if not 1 <= N <= 65535 or H * W >= 1 << 30 or N * H * W >= 1 << 31 or M >= 1 << 31:
        raise ValueError(f"{who}: M={M} N={N} H={H} W={W} beyond the kernels' limits (M < 2^31, 1 <= N <= 65535, H*W < 2^30, "
                         "N*H*W < 2^31)")
    points = _chk(points, "points", (M, 3))
    normals = _chk(normals, "normals", (M, 3))
    cam2world = _chk(cam2world, "cam2world", (N, 4, 4))
    if isinstance(K, torch.Tensor) and K.dim() == 2:
        K = K.unsqueeze(0).expand(N, 3, 3)
    K = _chk(K, "K", (N, 3, 3))
    if colors is not None:
        colors = _chk(colors, "colors", (M, 3))
    lib = _lib.load()
    dev = points.device
    scratch = torch.empty(int(lib.colvo_render_scratch_bytes(N, H, W)), device=dev, dtype=torch.uint8)
    depth = torch.empty(N, 1, H, W, device=dev, dtype=torch.float32)
    index = torch.empty(N, 1, H, W, device=dev, dtype=torch.int32)
    out_colors = torch.empty(N, 3, H, W, device=dev, dtype=torch.float32) if colors is not None else None
    out_normal = torch.empty(N, 3, H, W, device=dev, dtype=torch.float32) if want_normals else None
    stats = torch.empty(N, 6, device=dev, dtype=torch.int32)
    _lib.check(lib.colvo_render_surfels(_lib.ptr(points), _lib.ptr(normals), _lib.ptr(colors), M, _lib.ptr(K), _lib.ptr(cam2world), N,
                                        H, W, float(radius), max_splat, float(max_depth), _lib.ptr(scratch), _lib.ptr(depth),
                                        _lib.ptr(index), _lib.ptr(out_colors), _lib.ptr(out_normal), _lib.ptr(stats),
                                        _lib.stream_ptr()), "colvo_render_surfels")
    return SurfelViews(depth, index, out_colors, out_normal, stats)


def render_fused(fused: FusedCloud, K: torch.Tensor, cam2world: torch.Tensor, H: int, W: int, *, radius: Optional[float] = None,
                 max_splat: int = 8, max_depth: float = MAX_DEPTH, normals=None, want_normals: bool = False):
    """render_cloud of a FusedCloud's points and colours.  radius defaults to fused.voxel_size: the mean positions of neighbouring
    voxels are at most two voxels apart per axis, so squares of half-width one voxel close a fronto-parallel wall.  That default
    is a choice, not a tuned value.  With `normals` -- the CloudNormals of cloud_normals(fused, ...) or an [M,3] tensor -- it is
    render_surfels of the same and returns SurfelViews (want_normals as there); with None it returns RenderedViews."""
    if not isinstance(fused, FusedCloud):
        raise ValueError("render_fused: fused must be a FusedCloud")
    radius = fused.voxel_size if radius is None else radius
    if normals is None:
        if want_normals:
            raise ValueError("render_fused: want_normals needs normals")
        return render_cloud(fused.points, K, cam2world, H, W, radius=radius, colors=fused.colors, max_splat=max_splat,
                            max_depth=max_depth)
    if isinstance(normals, CloudNormals):
        normals = normals.normals
    return render_surfels(fused.points, normals, K, cam2world, H, W, radius=radius, colors=fused.colors, max_splat=max_splat,
                          max_depth=max_depth, want_normals=want_normals)


class MeshViews(NamedTuple):
    depth: torch.Tensor              # [N,1,H,W] float32: camera-z where the pixel centre's ray meets the nearest face, +inf where empty
    index: torch.Tensor              # [N,1,H,W] int32: that face's row, -1 where empty
    colors: Optional[torch.Tensor]   # [N,3,H,W] float32: its vertex colours interpolated perspective-correctly, 0 where empty (None without)
    normal: Optional[torch.Tensor]   # [N,3,H,W] float32: its unit face normal in the camera frame, towards the camera (None unless asked)
    stats: torch.Tensor              # [N,8] int32: faces front, drawn, straddling, outside the guard band, back-facing, degenerate; fragments; covered pixels
    face_pixels: Optional[torch.Tensor]   # [F] int32: the pixels of all views each face won (None unless asked)


def render_mesh(mesh_or_vertices, faces: Optional[torch.Tensor] = None, K: Optional[torch.Tensor] = None,
                cam2world: Optional[torch.Tensor] = None, H: Optional[int] = None, W: Optional[int] = None, *,
                colors: Optional[torch.Tensor] = None, cull_back: bool = False, max_depth: float = MAX_DEPTH,
                want_normals: bool = False, want_face_pixels: bool = False) -> MeshViews:
    """A triangle mesh drawn into N camera views of H x W pixels (contract: include/colvo.h colvo_render_mesh, DESIGN.md §3.6n;
    csrc/raster.hip).  Either a Mesh -- `render_mesh(mesh, K, cam2world, H, W)` or with keywords; its vertices, faces and colours are
    taken, `colors=` overrides the latter -- or vertices [V,3] float32 and faces [F,3] int32 in the world frame with colors [V,3] or
    None; K [3,3] or [N,3,3], cam2world [N,4,4], float32 on the device.  Every face whose three vertices are in front of a camera
    (1e-3 < P_z < max_depth) is snapped to a 1/256-pixel grid and covers the pixel centres inside it -- top-left rule: a pixel centre
    on an edge or a vertex shared by consistently wound faces belongs to exactly one of them --; a covered pixel gets the
    perspective-correct depth of its ray on the face, the nearest face wins, equal depths go to the smallest row.  No radius, no
    holes inside the surface.  cull_back drops the faces seen from behind (extract_mesh winds towards free space); off by default
    because the wall is opaque from both sides -- a choice.  want_normals: also the winner's camera-frame face normal per pixel;
    want_face_pixels: also how many pixels of all views each face won -- which part of the surface was seen, and how well.  The
    cameras need not be frames of the sequence.  Integer edge functions, float64 depth in a written association, an integer
    minimum and integer sums: identical bits on every call and stream, equal to the NumPy replica tests/raster_ref.py.

    A pixel no face covers gets depth +inf and index -1, as render_cloud's.  There is no near-plane clipping: a face with a vertex
    behind the camera or beyond max_depth is dropped whole and counted as straddling, a face with a vertex that projects more than
    16384 pixels from the origin is dropped whole and counted as outside.  No anti-aliasing, blending or smooth shading.  No read-back and no host synchronisation."""
    who = "render_mesh"
    if isinstance(mesh_or_vertices, Mesh):
        rest = [a for a in (faces, K, cam2world, H, W) if a is not None]
        if len(rest) != 4:
            raise ValueError(f"{who}: with a Mesh give K, cam2world, H and W (and no faces)")
        K, cam2world, H, W = rest
        vertices, faces = mesh_or_vertices.vertices, mesh_or_vertices.faces
        colors = mesh_or_vertices.colors if colors is None else colors
    else:
        vertices = mesh_or_vertices
    if not _finite_pos32(max_depth):
        raise ValueError(f"{who}: max_depth must be finite and positive (as float32), got {max_depth!r}")
    for name, val in (("cull_back", cull_back), ("want_normals", want_normals), ("want_face_pixels", want_face_pixels)):
        if not isinstance(val, bool):
            raise ValueError(f"{who}: {name} must be a bool, got {val!r}")
    for name, val in (("H", H), ("W", W)):
        if isinstance(val, bool) or not isinstance(val, int) or not 1 <= val <= 16384:
            raise ValueError(f"{who}: {name} must be an int in 1..16384, got {val!r}")
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{who}: vertices must be [V,3]")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{who}: faces must be [F,3] int32")
    if not isinstance(cam2world, torch.Tensor) or cam2world.dim() != 3:
        raise ValueError(f"{who}: cam2world must be [N,4,4]")
    V, F, N = vertices.shape[0], faces.shape[0], cam2world.shape[0]
    if not 1 <= N <= 65535 or N * H * W >= 1 << 31 or V >= 1 << 31 or F >= 1 << 31:
        raise ValueError(f"{who}: V={V} F={F} N={N} H={H} W={W} beyond the kernels' limits (V, F < 2^31, 1 <= N <= 65535, "
                         "H, W <= 16384, N*H*W < 2^31)")
    vertices = _chk(vertices, "vertices", (V, 3))
    if faces.device != vertices.device or not faces.is_contiguous():
        raise ValueError(f"{who}: faces must be contiguous and on the device of vertices")
    cam2world = _chk(cam2world, "cam2world", (N, 4, 4))
    if isinstance(K, torch.Tensor) and K.dim() == 2:
        K = K.unsqueeze(0).expand(N, 3, 3)
    K = _chk(K, "K", (N, 3, 3))
    if colors is not None:
        colors = _chk(colors, "colors", (V, 3))
    lib = _lib.load()
    dev = vertices.device
    scratch = torch.empty(int(lib.colvo_render_scratch_bytes(N, H, W)), device=dev, dtype=torch.uint8)
    depth = torch.empty(N, 1, H, W, device=dev, dtype=torch.float32)
    index = torch.empty(N, 1, H, W, device=dev, dtype=torch.int32)
    out_colors = torch.empty(N, 3, H, W, device=dev, dtype=torch.float32) if colors is not None else None
    out_normal = torch.empty(N, 3, H, W, device=dev, dtype=torch.float32) if want_normals else None
    face_pixels = torch.empty(F, device=dev, dtype=torch.int32) if want_face_pixels else None
    stats = torch.empty(N, 8, device=dev, dtype=torch.int32)
    _lib.check(lib.colvo_render_mesh(_lib.ptr(vertices), _lib.ptr(faces), _lib.ptr(colors), V, F, _lib.ptr(K), _lib.ptr(cam2world), N, H,
                                     W, float(max_depth), int(cull_back), _lib.ptr(scratch), _lib.ptr(depth), _lib.ptr(index),
                                     _lib.ptr(out_colors), _lib.ptr(out_normal), _lib.ptr(face_pixels), _lib.ptr(stats),
                                     _lib.stream_ptr()), "colvo_render_mesh")
    return MeshViews(depth, index, out_colors, out_normal, stats, face_pixels)


def write_ply(path, points: torch.Tensor, colors: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None,
              faces: Optional[torch.Tensor] = None) -> None:
    """Binary little-endian PLY: `float x y z` per vertex, with normals [M,3] `float nx ny nz` behind them (viewers shade by them)
    and, with colours [M,3] in [0,1], `uchar red green blue` (rint(c * 255), clamped).  With faces [F,3] (integer vertex indices, a
    Mesh's `faces`) an `element face F` with `property list uchar int vertex_indices` follows the vertices.  Without normals and
    without faces the bytes are what they were before either existed.  Host code; one device -> host copy (two with faces)."""
    import numpy as np
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("write_ply: points must be [M,3]")
    if faces is not None:
        if (not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.is_floating_point()
                or faces.dtype == torch.bool):
            raise ValueError("write_ply: faces must be an integer tensor [F,3]")
        if faces.numel() and (int(faces.min()) < 0 or int(faces.max()) >= points.shape[0]):
            raise ValueError("write_ply: faces index vertices that do not exist")
    if colors is not None and tuple(colors.shape) != tuple(points.shape):
        raise ValueError("write_ply: colors must have the shape of points")
    if normals is not None and (not isinstance(normals, torch.Tensor) or tuple(normals.shape) != tuple(points.shape)):
        raise ValueError("write_ply: normals must be a tensor of the shape of points")
    parts = [points.detach().to(torch.float32)]
    if normals is not None:
        parts.append(normals.detach().to(points.device, torch.float32))
    if colors is not None:
        parts.append(colors.detach().to(points.device, torch.float32))
    host = (parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)).cpu().numpy()
    m = host.shape[0]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {m}", "property float x", "property float y",
              "property float z"]
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    if faces is not None:
        header += [f"element face {faces.shape[0]}", "property list uchar int vertex_indices"]
    header.append("end_header")
    rows = np.empty(m, dtype=np.dtype(fields))
    n_float = 3 if normals is None else 6
    for a, name in enumerate(("x", "y", "z", "nx", "ny", "nz")[:n_float]):
        rows[name] = host[:, a]
    if colors is not None:
        q = np.clip(np.rint(np.nan_to_num(host[:, n_float:n_float + 3], nan=0.0) * 255.0), 0, 255).astype(np.uint8)
        for k, name in enumerate(("red", "green", "blue")):
            rows[name] = q[:, k]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(rows.tobytes())
        if faces is not None:
            tri = np.empty(faces.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
            tri["n"] = 3
            tri["v"] = faces.detach().cpu().numpy()
            f.write(tri.tobytes())


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
    MeshViews of that mesh)."""
    polyps = None               # Optional[PolypLocalization]
    consistency = None          # Optional[ConsistencyResult]
    refinement = None           # Optional[RefinementResult]
    rendered = None             # Optional[RenderedViews], SurfelViews with Render(surfels=True), MeshViews with Render(mesh=True)
    normals = None              # Optional[CloudNormals]
    mesh = None                 # Optional[Mesh]

    def __new__(cls, depths, rel_poses, cam2world, points, fused=None, polyps=None, consistency=None, refinement=None,
                rendered=None, normals=None, mesh=None):
        self = super().__new__(cls, depths, rel_poses, cam2world, points, fused)
        self.polyps = polyps
        self.consistency = consistency
        self.refinement = refinement
        self.rendered = rendered
        self.normals = normals
        self.mesh = mesh
        return self

    def _replace(self, **kw):
        polyps = kw.pop("polyps", self.polyps)
        consistency = kw.pop("consistency", self.consistency)
        refinement = kw.pop("refinement", self.refinement)
        rendered = kw.pop("rendered", self.rendered)
        normals = kw.pop("normals", self.normals)
        mesh = kw.pop("mesh", self.mesh)
        return type(self)(*super()._replace(**kw), polyps=polyps, consistency=consistency, refinement=refinement, rendered=rendered,
                          normals=normals, mesh=mesh)


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
    max_depth and image size, culling off): `rendered` is then a MeshViews and `normals` stays None."""
    n = frames.shape[0]
    if n < 2:
        raise ValueError("reconstruct_sequence: need at least two frames")
    if labels is not None and num_labels is None:
        raise ValueError("reconstruct_sequence: labels need num_labels")
    if consistency is not None:
        consistency = Consistency(*consistency)
        _check_consistency("reconstruct_sequence", *consistency, max_depth)
    if refine is not None:
        refine = Refinement(*refine)
        _check_refinement("reconstruct_sequence", refine, max_depth)
    if render is not None:
        render = Render(*render, surfels=getattr(render, "surfels", False), mesh=getattr(render, "mesh", False))
        if voxel_size is None:
            raise ValueError("reconstruct_sequence: render needs voxel_size (it draws the fused cloud)")
        _check_render("reconstruct_sequence", voxel_size if render.radius is None else render.radius, render.max_splat, max_depth)
        if not isinstance(render.surfels, bool):
            raise ValueError(f"reconstruct_sequence: render.surfels must be a bool, got {render.surfels!r}")
        if not isinstance(render.mesh, bool):
            raise ValueError(f"reconstruct_sequence: render.mesh must be a bool, got {render.mesh!r}")
        if render.mesh and render.surfels:
            raise ValueError("reconstruct_sequence: Render(mesh=True) draws the surface mesh, surfels=True the cloud: give one of them")
        if render.mesh and mesh is None:
            raise ValueError("reconstruct_sequence: Render(mesh=True) needs a Meshing policy (mesh=Meshing()): it draws the extracted mesh")
    if mesh is not None:
        mesh = Meshing(*mesh)
        if voxel_size is None:
            raise ValueError("reconstruct_sequence: mesh needs voxel_size (the TSDF volume's voxels)")
        _tsdf_voxels("reconstruct_sequence", voxel_size, mesh.trunc)
        if isinstance(mesh.min_obs, bool) or not isinstance(mesh.min_obs, int) or mesh.min_obs < 1:
            raise ValueError(f"reconstruct_sequence: mesh.min_obs must be an int >= 1, got {mesh.min_obs!r}")
    if K.dim() == 2:
        K = K.unsqueeze(0).expand(n, 3, 3)
    K = K.to(frames.device, torch.float32).contiguous()
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
        from . import localize                       # (localize imports this module)
        polyps = localize.localize_polyps(depths, labels, K, traj32, num_labels=num_labels, stride=1, max_depth=max_depth)
    rendered = normals = None
    if render is not None and not render.mesh:
        if render.surfels:
            normals = cloud_normals(fused, depths, K, traj32, stride=stride, max_depth=max_depth)
        rendered = render_fused(fused, K, traj32, int(frames.shape[2]), int(frames.shape[3]), radius=render.radius,
                                max_splat=render.max_splat, max_depth=max_depth, normals=normals)
    surface = None
    if mesh is not None:
        volume = fuse_tsdf(depths, K, traj32, voxel_size=voxel_size, trunc=mesh.trunc, colors=frames.to(torch.float32).contiguous(),
                           stride=stride, max_depth=max_depth)
        surface = extract_mesh(volume, min_obs=mesh.min_obs)
        if render is not None and render.mesh:
            rendered = render_mesh(surface, K, traj32, int(frames.shape[2]), int(frames.shape[3]), max_depth=max_depth)
    return Reconstruction(raw, rel, traj, cloud, fused, polyps, checked, refined, rendered, normals, surface)
