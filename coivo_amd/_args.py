"""How the post-training entry points (inference, fusion, consistency, refine, render, localize, topology, holes, evaluate, cloud_eval,
registration, surface_eval) check an argument: the one place that knows.  Every helper takes `who` -- the entry point's name -- and
the argument's name, so a ValueError names both.  Mesh is defined here, below everything that checks one; fusion re-exports it."""
import math
import struct
from typing import NamedTuple, Optional, Tuple

import torch

MAX_DEPTH = 10.0     # spec: MAX_DEPTH
MAX_THRESHOLDS = 8
MAX_FACES = (1 << 29) - 1


class Mesh(NamedTuple):
    vertices: torch.Tensor          # [V,3] float32: one per active cell, in (brick, voxel in brick) order of the cell's minimum corner
    faces: torch.Tensor             # [F,3] int32: triangles, wound so that the normal points to free space (the camera side)
    colors: Optional[torch.Tensor]  # [V,3] float32 in [0,1] (None without colours)
    normals: torch.Tensor           # [V,3] float32: unit gradient of the distance field, towards free space; 0 for a zero gradient
    cells: torch.Tensor             # [V,3] int32: the cell (ix, iy, iz) of each vertex
    n_open: int                     # cells with a sign change among their observed corners and one or more corners not observed


def f32(x) -> float:
    """x rounded to float32, as a Python float (what the C ABI's `float` arguments receive)."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def _finite32(who: str, name: str, val, least: str) -> float:
    try:
        v = f32(val)
    except (TypeError, ValueError, OverflowError, struct.error):      # None, a string, 1e39
        v = math.nan
    if not (math.isfinite(v) and (v > 0.0 or (v == 0.0 and least == ">= 0"))):
        raise ValueError(f"{who}: {name} must be finite and {least} (as float32), got {val!r}")
    return v


def finite_pos32(who: str, name: str, val) -> float:
    """-> val as float32; ValueError unless that is finite and positive."""
    return _finite32(who, name, val, "positive")


def finite_nonneg32(who: str, name: str, val) -> float:
    """-> val as float32; ValueError unless that is finite and >= 0."""
    return _finite32(who, name, val, ">= 0")


def finite_nonneg64(who: str, name: str, val) -> float:
    """-> val as a Python float (a `double` of the C ABI: not rounded); ValueError unless that is finite and >= 0."""
    try:
        v = float(val)
    except (TypeError, ValueError):
        v = math.nan
    if not (v >= 0.0 and math.isfinite(v)):
        raise ValueError(f"{who}: {name} must be finite and >= 0, got {val!r}")
    return v


def int_range(who: str, name: str, val, lo: int, hi: Optional[int] = None) -> int:
    """-> val; ValueError unless it is an int (a bool is not) with lo <= val, and val <= hi where a hi is given."""
    if isinstance(val, bool) or not isinstance(val, int) or val < lo or (hi is not None and val > hi):
        raise ValueError(f"{who}: {name} must be an int " + (f">= {lo}" if hi is None else f"in {lo}..{hi}") + f", got {val!r}")
    return val


def device_f32(who: str, name: str, t, shape) -> torch.Tensor:
    """-> t contiguous; ValueError unless it is a float32 tensor of that shape on the GPU."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name}: expected a float32 CUDA tensor of shape {tuple(shape)}, got "
                         f"{getattr(t, 'dtype', None)} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
    return t.contiguous()


def cloud(who: str, name: str, t) -> torch.Tensor:
    """-> t contiguous; ValueError unless it is a float32 tensor [N,3] on the GPU."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{who}: {name}: expected a float32 CUDA tensor of shape [N,3], got {getattr(t, 'dtype', None)} "
                         f"{tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
    return t.contiguous()


def frames_shape(who: str, name: str, depths) -> Tuple[int, int, int]:
    """(N, H, W) of a stack of depth maps [N,1,H,W]; ValueError for anything that is not a 4-D tensor."""
    if not isinstance(depths, torch.Tensor) or depths.dim() != 4:
        raise ValueError(f"{who}: {name} must be [N,1,H,W]")
    return int(depths.shape[0]), int(depths.shape[2]), int(depths.shape[3])


def depth_views(who: str, depths, K, cam2world=None, name: str = "depths"):
    """The trio depths [N,1,H,W] / K [N,3,3] / cam2world [N,4,4] (the latter may be left out: None comes back), float32 on the device:
    -> (depths, K, cam2world, N, H, W), the tensors contiguous."""
    N, H, W = frames_shape(who, name, depths)
    depths = device_f32(who, name, depths, (N, 1, H, W))
    K = device_f32(who, "K", K, (N, 3, 3))
    cam2world = None if cam2world is None else device_f32(who, "cam2world", cam2world, (N, 4, 4))
    return depths, K, cam2world, N, H, W


def per_view_K(K, N: int):
    """K [3,3] -> a view [N,3,3] of it; anything else as it came (device_f32 judges it)."""
    return K.unsqueeze(0).expand(N, 3, 3) if isinstance(K, torch.Tensor) and K.dim() == 2 else K


def voxel_grid(who: str, origin, dims, voxel_size):
    """(origin, dims, voxel_size) as the kernels take them: origin three float32 values, dims three positive multiples of 8 (whole
    8x8x8 bricks), voxel_size a finite positive float32.  origin and dims come together; with neither, both come back None and the
    grid is the caller's to choose (fusion.fusion_grid)."""
    vs = finite_pos32(who, "voxel_size", voxel_size)
    if (origin is None) != (dims is None):
        raise ValueError(f"{who}: give origin and dims together, or neither")
    if origin is None:
        return None, None, vs
    origin = tuple(f32(o) for o in origin)
    dims = tuple(int(d) for d in dims)
    if len(origin) != 3 or len(dims) != 3 or any(d <= 0 or d % 8 for d in dims):
        raise ValueError(f"{who}: the grid's dims must be three positive multiples of 8, got {dims} (origin {origin})")
    return origin, dims, vs


def reach(who: str, max_dist, thresholds) -> Tuple[float, Tuple[float, ...]]:
    """max_dist and the thresholds as float32 values, refused as the library refuses them."""
    try:
        md = f32(max_dist)
    except (OverflowError, TypeError, ValueError):
        md = math.nan
    md2 = f32(md * md) if math.isfinite(md) else math.nan
    if not (md > 0.0 and math.isfinite(md) and md2 >= 2.0 ** -126 and math.isfinite(md2)):
        raise ValueError(f"{who}: max_dist must be finite and positive with a finite positive float32 square, got {max_dist!r}")
    try:
        th = tuple(f32(t) for t in thresholds)
    except (OverflowError, TypeError, ValueError):
        raise ValueError(f"{who}: thresholds must be numbers, got {thresholds!r}") from None
    if len(th) > MAX_THRESHOLDS:
        raise ValueError(f"{who}: at most {MAX_THRESHOLDS} thresholds, got {len(th)}")
    for k, t in enumerate(th):
        if not (t > 0.0 and t <= md and (k == 0 or t >= th[k - 1])):
            raise ValueError(f"{who}: thresholds must be positive, non-descending and at most max_dist {md}, got {th}")
    return md, th


def sim3(who: str, name: str, value) -> Tuple[torch.Tensor, torch.Tensor, float]:
    """A Sim(3) given as (R, t, s), as align_trajectory returns it -> (R [3,3], t [3], s) in float64 on the host; ValueError unless
    it is such a triple and finite."""
    try:
        R, t, s = value
        R = torch.as_tensor(R).detach().to("cpu", torch.float64)
        t = torch.as_tensor(t).detach().to("cpu", torch.float64)
        s = torch.as_tensor(s).detach().to("cpu", torch.float64)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{who}: {name} must be (R [3,3], t [3], s), as align_trajectory returns it") from None
    if tuple(R.shape) != (3, 3) or tuple(t.shape) != (3,) or s.numel() != 1:
        raise ValueError(f"{who}: {name} must be (R [3,3], t [3], s), got shapes {tuple(R.shape)}, {tuple(t.shape)}, {tuple(s.shape)}")
    if not bool(torch.isfinite(torch.cat([R.reshape(9), t, s.reshape(1)])).all()):
        raise ValueError(f"{who}: {name} must be finite")
    return R, t, float(s)


def mesh_arrays(who: str, mesh_or_vertices, faces):
    """A Mesh, or vertices [V,3] float32 and faces [F,3] int32 on the device -> (vertices, faces, V, F), contiguous."""
    if isinstance(mesh_or_vertices, Mesh):
        if faces is not None:
            raise ValueError(f"{who}: with a Mesh give no faces")
        vertices, faces = mesh_or_vertices.vertices, mesh_or_vertices.faces
    else:
        vertices = mesh_or_vertices
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{who}: vertices must be [V,3]")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{who}: faces must be [F,3] int32")
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    if V >= 1 << 31 or F > MAX_FACES:
        raise ValueError(f"{who}: V = {V}, F = {F} beyond the kernels' limits (V < 2^31, F < 2^29)")
    vertices = device_f32(who, "vertices", vertices, (V, 3))
    if faces.device != vertices.device or not faces.is_contiguous():
        raise ValueError(f"{who}: faces must be contiguous and on the device of vertices")
    return vertices, faces, V, F


def mesh_attributes(who: str, mesh: Mesh, V: int, dev):
    """What a Mesh carries per vertex besides the position -> (colors or None, normals, cells), contiguous on dev."""
    colors = None if mesh.colors is None else device_f32(who, "mesh.colors", mesh.colors, (V, 3))
    normals = device_f32(who, "mesh.normals", mesh.normals, (V, 3))
    cells = mesh.cells
    if not isinstance(cells, torch.Tensor) or cells.dtype != torch.int32 or tuple(cells.shape) != (V, 3) or cells.device != dev:
        raise ValueError(f"{who}: mesh.cells must be [V,3] int32 on the device of the vertices")
    return colors, normals, cells.contiguous()


def own_topology(who: str, topology, V: int, F: int, dev, tables: Tuple[str, ...]) -> None:
    """ValueError unless the tables of a MeshTopology that the caller is about to read -- `tables`, of "components" (with
    vertex_component) and "loops" (with vertex_loop) -- are those of a mesh of V vertices and F faces on dev."""
    ok = tuple(topology.face_component.shape) == (F,)
    if "components" in tables:
        comp = topology.components
        ok = ok and tuple(topology.vertex_component.shape) == (V,) and comp.device == dev and (int(comp.shape[0]) == 0) == (V == 0)
    if "loops" in tables:
        loops, vertex_loop = topology.loops, topology.vertex_loop
        ok = ok and tuple(vertex_loop.shape) == (V,) and vertex_loop.dtype == torch.int32 and vertex_loop.device == dev \
            and loops.device == dev and loops.dim() == 2 and loops.shape[1] == 4 and loops.dtype == torch.int64 \
            and not (loops.shape[0] > 0 and (V == 0 or F == 0))
    if not ok:
        raise ValueError(f"{who}: topology is not this mesh's (V = {V}, F = {F} on {dev})")
