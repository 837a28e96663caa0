"""Drawing a reconstruction back into camera views: render_cloud (squares, DESIGN.md §3.6j, csrc/render.hip), render_surfels (oriented
discs, DESIGN.md §3.6k, csrc/surfels.hip) and render_mesh (triangles, DESIGN.md §3.6n, csrc/raster.hip).  The three share the views
they draw into and the outputs they fill; only what is drawn differs.  coivo_amd.inference re-exports every name here."""
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._args import MAX_DEPTH, device_f32, finite_nonneg32, finite_pos32, int_range, per_view_K
from .fusion import CloudNormals, FusedCloud, Mesh


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


def check_render(who: str, radius, max_splat, max_depth) -> None:
    """ValueError for what colvo_render_cloud would refuse of the policy."""
    int_range(who, "max_splat", max_splat, 0, 32)
    finite_nonneg32(who, "radius", radius)
    finite_pos32(who, "max_depth", max_depth)


def _check_views(who: str, K, cam2world, H, W, rows: dict, limits: str, hw_max: Optional[int] = None):
    """The N views of H x W pixels a renderer draws into, K [3,3] or [N,3,3]: -> (K [N,3,3], cam2world [N,4,4], N), contiguous on the
    device.  `rows`: the element counts of what is drawn, by the names the `limits` text has; hw_max: a renderer's own bound on H, W."""
    for name, val in (("H", H), ("W", W)):
        int_range(who, name, val, 1, hw_max)
    if not isinstance(cam2world, torch.Tensor) or cam2world.dim() != 3:
        raise ValueError(f"{who}: cam2world must be [N,4,4]")
    N = cam2world.shape[0]
    if not 1 <= N <= 65535 or H * W >= 1 << 30 or N * H * W >= 1 << 31 or any(r >= 1 << 31 for r in rows.values()):
        raise ValueError(f"{who}: " + " ".join(f"{k}={v}" for k, v in rows.items()) + f" N={N} H={H} W={W} beyond the kernels' "
                         f"limits ({limits})")
    cam2world = device_f32(who, "cam2world", cam2world, (N, 4, 4))
    return device_f32(who, "K", per_view_K(K, N), (N, 3, 3)), cam2world, N


def _outputs(dev, N: int, H: int, W: int, n_stats: int, colors: bool, normal: bool):
    """What every renderer fills: (scratch, depth, index, colours or None, normal or None, stats [N,n_stats])."""
    planes = lambda c, dtype=torch.float32: torch.empty(N, c, H, W, device=dev, dtype=dtype)
    scratch = torch.empty(int(_lib.load().colvo_render_scratch_bytes(N, H, W)), device=dev, dtype=torch.uint8)
    return (scratch, planes(1), planes(1, torch.int32), planes(3) if colors else None, planes(3) if normal else None,
            torch.empty(N, n_stats, device=dev, dtype=torch.int32))


def _check_cloud(who: str, points, colors, K, cam2world, H, W, radius, max_splat, max_depth):
    """What render_cloud and render_surfels take alike, policy first: -> (points, colors, K, cam2world, M, N)."""
    check_render(who, radius, max_splat, max_depth)
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{who}: points must be [M,3]")
    M = points.shape[0]
    K, cam2world, N = _check_views(who, K, cam2world, H, W, {"M": M}, "M < 2^31, 1 <= N <= 65535, H*W < 2^30, N*H*W < 2^31")
    colors = None if colors is None else device_f32(who, "colors", colors, (M, 3))
    return device_f32(who, "points", points, (M, 3)), colors, K, cam2world, M, N


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
    points, colors, K, cam2world, M, N = _check_cloud(who, points, colors, K, cam2world, H, W, radius, max_splat, max_depth)
    scratch, depth, index, out_colors, _, stats = _outputs(points.device, N, H, W, 4, colors is not None, False)
    _lib.call("colvo_render_cloud", points, colors, M, K, cam2world, N, H, W, float(radius), max_splat, float(max_depth), scratch, depth,
              index, out_colors, stats, _lib.stream_ptr())
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
    if not isinstance(normals, torch.Tensor) or tuple(normals.shape) != tuple(getattr(points, "shape", ())):
        raise ValueError(f"{who}: normals must have the shape of points")
    points, colors, K, cam2world, M, N = _check_cloud(who, points, colors, K, cam2world, H, W, radius, max_splat, max_depth)
    normals = device_f32(who, "normals", normals, (M, 3))
    scratch, depth, index, out_colors, out_normal, stats = _outputs(points.device, N, H, W, 6, colors is not None, want_normals)
    _lib.call("colvo_render_surfels", points, normals, colors, M, K, cam2world, N, H, W, float(radius), max_splat, float(max_depth),
              scratch, depth, index, out_colors, out_normal, stats, _lib.stream_ptr())
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
    finite_pos32(who, "max_depth", max_depth)
    for name, val in (("cull_back", cull_back), ("want_normals", want_normals), ("want_face_pixels", want_face_pixels)):
        if not isinstance(val, bool):
            raise ValueError(f"{who}: {name} must be a bool, got {val!r}")
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{who}: vertices must be [V,3]")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{who}: faces must be [F,3] int32")
    V, F = vertices.shape[0], faces.shape[0]
    K, cam2world, N = _check_views(who, K, cam2world, H, W, {"V": V, "F": F}, "V, F < 2^31, 1 <= N <= 65535, H, W <= 16384, N*H*W < 2^31",
                                   hw_max=16384)
    vertices = device_f32(who, "vertices", vertices, (V, 3))
    if faces.device != vertices.device or not faces.is_contiguous():
        raise ValueError(f"{who}: faces must be contiguous and on the device of vertices")
    if colors is not None:
        colors = device_f32(who, "colors", colors, (V, 3))
    dev = vertices.device
    scratch, depth, index, out_colors, out_normal, stats = _outputs(dev, N, H, W, 8, colors is not None, want_normals)
    face_pixels = torch.empty(F, device=dev, dtype=torch.int32) if want_face_pixels else None
    _lib.call("colvo_render_mesh", vertices, faces, colors, V, F, K, cam2world, N, H, W, float(max_depth), int(cull_back), scratch,
              depth, index, out_colors, out_normal, face_pixels, stats, _lib.stream_ptr())
    return MeshViews(depth, index, out_colors, out_normal, stats, face_pixels)
