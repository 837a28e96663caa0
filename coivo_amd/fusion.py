"""Fusion of a sequence's depth maps along its trajectory: the coloured, voxel-averaged cloud (csrc/fuse.hip), its
surface normals (csrc/normals.hip), and the truncated signed distance volume with its surface-net mesh (DESIGN.md
§3.6m, csrc/tsdf.hip), all on one regular grid of 8x8x8 bricks (fusion_grid).  coivo_amd.inference re-exports every name here."""
import math
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._args import MAX_DEPTH, Mesh, depth_views, device_f32, f32, finite_pos32, frames_shape, int_range, voxel_grid


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


def fusion_grid(K: torch.Tensor, cam2world: torch.Tensor, H: int, W: int, voxel_size: float, max_depth: float = MAX_DEPTH):
    """A grid that holds every sample of depth < max_depth seen from the given cameras: (origin, dims).  Host, float64.
    A sample at z-depth d lies d * |ray| from its camera, |ray| = sqrt(1 + ((u-cx)/fx)^2 + ((v-cy)/fy)^2), largest at an
    image corner; the box is the camera centres -/+ max_depth * (largest corner ray of any frame) -/+ one voxel, snapped
    outward to whole bricks (multiples of 8 voxels).  Loose is cheap -- 4 bytes per brick."""
    Kd = K.detach().to("cpu", torch.float64).reshape(-1, 3, 3)
    Md = cam2world.detach().to("cpu", torch.float64).reshape(-1, 4, 4)
    vs = finite_pos32("fusion_grid", "voxel_size", voxel_size)
    finite_pos32("fusion_grid", "max_depth", max_depth)
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
    origin = tuple(f32(l * brick) for l in lo)
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
    who = "fuse_point_cloud"
    lib = _lib.load()
    int_range(who, "stride", stride, 1)
    int_range(who, "min_obs", min_obs, 1)
    depths, K, cam2world, N, H, W = depth_views(who, depths, K, cam2world)
    if colors is not None:
        colors = device_f32(who, "colors", colors, (N, 3, H, W))
    origin, dims, vs = voxel_grid(who, origin, dims, voxel_size)
    if origin is None:
        origin, dims = fusion_grid(K, cam2world, H, W, vs, max_depth)
    dev = depths.device
    geom = (N, H, W, stride, float(max_depth), *origin, vs, *dims)
    ws_bytes = int(lib.colvo_fuse_plan_workspace_bytes(N, H, W, stride, *dims))
    if ws_bytes == 0:
        raise ValueError(f"{who}: shape N={N} H={H} W={W} stride={stride} or grid {dims} beyond the kernels' limits")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    stats = torch.empty(3, device=dev, dtype=torch.int32)
    stream = _lib.stream_ptr()
    _lib.call("colvo_fuse_plan", depths, K, cam2world, *geom, ws, stats, stream)
    n_input, n_outside, n_bricks = (int(v) for v in stats.tolist())
    n_voxels = m = 0
    if n_bricks > 0:
        pool_bytes = int(lib.colvo_fuse_pool_bytes(n_bricks))
        if pool_bytes == 0:
            raise RuntimeError(f"{who}: {n_bricks} occupied bricks, the limit is 2^22 - 1: use a larger voxel_size")
        pool = torch.empty(pool_bytes, device=dev, dtype=torch.uint8)
        _lib.call("colvo_fuse_accumulate", depths, colors, K, cam2world, *geom, ws, n_bricks, pool, stream)
        ews = torch.empty(int(lib.colvo_fuse_extract_workspace_bytes(n_bricks)), device=dev, dtype=torch.uint8)
        stats2 = torch.empty(3, device=dev, dtype=torch.int32)
        _lib.call("colvo_fuse_count", pool, n_bricks, min_obs, ews, stats2, stream)
        n_voxels, m, overflow = (int(v) for v in stats2.tolist())
        if overflow:
            raise RuntimeError(f"{who}: overflow: a voxel received 2^24 or more samples (its 32-bit sums may have "
                               "wrapped); use a smaller voxel_size, a larger stride or fewer frames per call")
    points = torch.empty(m, 3, device=dev, dtype=torch.float32)
    out_colors = torch.empty(m, 3, device=dev, dtype=torch.float32) if colors is not None else None
    counts = torch.empty(m, device=dev, dtype=torch.int32)
    voxels = torch.empty(m, 3, device=dev, dtype=torch.int32)
    if m > 0:
        _lib.call("colvo_fuse_write", ws, pool, n_bricks, min_obs, *origin, vs, *dims, ews, m, points, out_colors, counts, voxels, stream)
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


class _MeshingFields(NamedTuple):
    trunc: Optional[float] = None   # None: four voxels
    min_obs: int = 2


class Meshing(_MeshingFields):
    """reconstruct_sequence's meshing policy: fuse_tsdf's trunc and extract_mesh's min_obs.  The defaults are choices, not tuned
    values.  Behind the two fields -- it still unpacks into two and equals the pair -- a third, `min_faces` (positional or by
    keyword; 0, a choice: the mesh is left as extracted): with min_faces > 0 the components with fewer faces, and every vertex no
    face uses, are removed (coivo_amd.topology.clean_mesh); and a fourth, `fill_edges` (likewise; 0, a choice: the holes stay open):
    with fill_edges >= 3 the simple boundary rings of at most that many edges are then closed (coivo_amd.holes.fill_holes)."""
    min_faces = 0
    fill_edges = 0

    def __new__(cls, trunc=None, min_obs=2, min_faces=0, fill_edges=0):
        self = super().__new__(cls, trunc, min_obs)
        self.min_faces = min_faces
        self.fill_edges = fill_edges
        return self

    def _replace(self, **kw):
        min_faces = kw.pop("min_faces", self.min_faces)
        fill_edges = kw.pop("fill_edges", self.fill_edges)
        return type(self)(*super()._replace(**kw), min_faces=min_faces, fill_edges=fill_edges)

    def __repr__(self):
        return (f"Meshing(trunc={self.trunc!r}, min_obs={self.min_obs!r}, min_faces={self.min_faces!r}, "
                f"fill_edges={self.fill_edges!r})")


def tsdf_voxels(who: str, voxel_size, trunc):
    """(voxel_size as float32, T): trunc must be a whole number T of voxels, 1 <= T <= 7; None is four voxels."""
    vs = finite_pos32(who, "voxel_size", voxel_size)
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
    int_range(who, "stride", stride, 1)
    finite_pos32(who, "max_depth", max_depth)
    vs, T = tsdf_voxels(who, voxel_size, trunc)
    depths, K, cam2world, N, H, W = depth_views(who, depths, K, cam2world)
    if colors is not None:
        colors = device_f32(who, "colors", colors, (N, 3, H, W))
    origin, dims, vs = voxel_grid(who, origin, dims, vs)
    if origin is None:
        origin, dims = fusion_grid(K, cam2world, H, W, vs, max_depth)
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
    _lib.call("colvo_tsdf_plan", depths, K, cam2world, N, H, W, stride, float(max_depth), *origin, vs, *dims, T, scratch, table,
              brick_list, stats, stream)
    n_input, n_outside, n_bricks = (int(v) for v in stats.tolist())
    if n_bricks >= 1 << 22:
        raise RuntimeError(f"{who}: {n_bricks} allocated bricks, the limit is 2^22 - 1: use a larger voxel_size")
    pool = torch.empty(n_bricks * 512, 2, device=dev, dtype=torch.int32)
    sums = torch.empty(n_bricks * 512, 4, device=dev, dtype=torch.int32) if colors is not None else None
    if n_bricks > 0:
        _lib.call("colvo_tsdf_integrate", depths, colors, K, cam2world, N, H, W, float(max_depth), *origin, vs, *dims, T, brick_list,
                  n_bricks, pool, sums, 0, stream)
    return TsdfVolume(pool, sums, brick_list[:n_bricks], table, origin, dims, vs, f32(f32(T) * vs), colors is not None, n_input,
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
    int_range(who, "min_obs", min_obs, 1)
    lib = _lib.load()
    dev = volume.table.device
    n_bricks = int(volume.n_bricks)
    origin = tuple(f32(o) for o in volume.origin)
    dims = tuple(int(d) for d in volume.dims)
    vs = f32(volume.voxel_size)
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
        bricks = (volume.table, volume.brick_list, n_bricks)
        _lib.call("colvo_tsdf_mesh_count", volume.pool, *bricks, min_obs, *dims, scratch, stats2, stream)
        V, n_open = (int(v) for v in stats2[:2].tolist())
    vertices = torch.empty(V, 3, device=dev, dtype=torch.float32)
    normals = torch.empty(V, 3, device=dev, dtype=torch.float32)
    colors = torch.empty(V, 3, device=dev, dtype=torch.float32) if volume.color_sums is not None else None
    cells = torch.empty(V, 3, device=dev, dtype=torch.int32)
    if V > 0:
        vid = torch.empty(n_bricks * 512, device=dev, dtype=torch.int32)
        _lib.call("colvo_tsdf_mesh_vertices", volume.pool, volume.color_sums, *bricks, min_obs, *origin, vs, *dims, scratch, V, vertices,
                  colors, normals, cells, vid, stats2[2:], stream)
        F = int(stats2[2].item())
    faces = torch.empty(F, 3, device=dev, dtype=torch.int32)
    if F > 0:
        _lib.call("colvo_tsdf_mesh_faces", volume.pool, *bricks, *dims, scratch, vid, F, faces, stream)
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
    N, H, W = frames_shape(who, "depths", depths)
    int_range(who, "stride", stride, 1)
    finite_pos32(who, "max_depth", max_depth)
    finite_pos32(who, "rel_edge", rel_edge)
    origin, dims, vs = voxel_grid(who, fused.origin, fused.dims, fused.voxel_size)
    lib = _lib.load()
    if int(lib.colvo_fuse_plan_workspace_bytes(N, H, W, stride, *dims)) == 0:
        raise ValueError(f"{who}: shape N={N} H={H} W={W} stride={stride} or grid {dims} beyond the kernels' limits")
    depths, K, cam2world, N, H, W = depth_views(who, depths, K, cam2world)
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
    _lib.call("colvo_cloud_normals", depths, K, cam2world, N, H, W, stride, float(max_depth), *origin, vs, *dims, voxels, m,
              float(rel_edge), scratch, normals, counts, coherence, stats, _lib.stream_ptr())
    return CloudNormals(normals, counts, coherence, stats)
