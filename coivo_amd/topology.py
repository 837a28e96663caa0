"""What a triangle mesh is: its connected components, its edges, its boundary loops, their areas and lengths (mesh_topology), and the
mesh without the components a caller drops (clean_mesh) -- DESIGN.md §3.6o, csrc/topology.hip, contract include/colvo.h
colvo_mesh_topology_* / colvo_mesh_clean_*.  coivo_amd.inference re-exports every name here."""
import math
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._args import MAX_FACES, Mesh, finite_pos32, int_range, mesh_arrays, mesh_attributes, own_topology


class MeshTopology(NamedTuple):
    vertex_component: torch.Tensor  # [V] int32: the component of each vertex
    face_component: torch.Tensor    # [F] int32: the component of each face, -1 for a dead face
    vertex_loop: torch.Tensor       # [V] int32: the boundary loop of each vertex, -1 off the boundary
    components: torch.Tensor        # [C,8] int64: smallest vertex, vertices, faces, edges, boundary edges, non-manifold edges, loops, area in quanta
    loops: torch.Tensor             # [L,4] int64: smallest vertex, component, edges, length in quanta
    n_dead_faces: int               # faces with an index outside [0, V) or a repeated index
    n_unmeasured: int               # live faces and boundary edges whose measure is not finite (they add 0 quanta)
    unit: float                     # as float32: a length quantum is unit * 2^-16, an area quantum unit^2 * 2^-16

    @property
    def length_quantum(self) -> float:
        return float(self.unit) * 2.0 ** -16

    @property
    def area_quantum(self) -> float:
        return float(self.unit) * float(self.unit) * 2.0 ** -16

    @property
    def area(self) -> torch.Tensor:
        """[C] float64: the area of each component"""
        return self.components[:, 7].to(torch.float64) * self.area_quantum

    @property
    def length(self) -> torch.Tensor:
        """[L] float64: the length of each loop"""
        return self.loops[:, 3].to(torch.float64) * self.length_quantum

    @property
    def euler(self) -> torch.Tensor:
        """[C] int64: vertices - edges + faces of each component"""
        return self.components[:, 1] - self.components[:, 3] + self.components[:, 2]

    @property
    def closed(self) -> torch.Tensor:
        """[C] bool: a component with faces, no boundary edge and no non-manifold edge"""
        c = self.components
        return (c[:, 2] > 0) & (c[:, 4] == 0) & (c[:, 5] == 0)


class CleanedMesh(NamedTuple):
    mesh: Mesh                      # the kept vertices and faces, in their old order
    vertex_index: torch.Tensor      # [V'] int32: the old row of each new vertex
    face_index: torch.Tensor        # [F'] int32: the old row of each new face
    kept: torch.Tensor              # [C] bool: which components stayed


def mesh_topology(mesh_or_vertices, faces: Optional[torch.Tensor] = None, *, unit: float) -> MeshTopology:
    """The topology of a triangle mesh -- `mesh_topology(mesh, unit=...)` with a Mesh, or vertices [V,3] float32 and faces [F,3] int32
    on the device (contract: include/colvo.h colvo_mesh_topology_*; csrc/topology.hip).  A face with an index outside
    [0, V) or a repeated index is dead (render_mesh's notion): it joins nothing.  A component is a class of vertices joined by live
    faces -- a vertex no live face uses is a component of its own --, numbered by ascending smallest vertex; an edge with one live-face
    side is boundary, with more than two non-manifold; a loop is a connected piece of the boundary edges (two rings touching in a vertex
    are one loop), numbered likewise.  Areas and lengths are float64 in a written association, rounded to quanta of unit^2 * 2^-16 and
    unit * 2^-16 and summed as integers: every output bit is a function of the inputs alone -- identical between calls and streams,
    independent of the order of the faces up to face_component's own permutation -- and equals the NumPy replica
    tests/topology_ref.py.  `unit` is a positive float32 length; reconstruct_sequence gives the voxel size.  Reads three small blocks
    back (C, then L, then the counts) to size the tables.  The edge pass is quadratic in the number of edges at one smaller endpoint:
    meant for meshes of bounded degree, as extract_mesh's are (12 at most).  No hole filling, no simplification."""
    who = "mesh_topology"
    unit = finite_pos32(who, "unit", unit)
    vertices, faces, V, F = mesh_arrays(who, mesh_or_vertices, faces)
    dev = vertices.device
    i32 = dict(device=dev, dtype=torch.int32)
    components = torch.empty(0, 8, device=dev, dtype=torch.int64)
    loops = torch.empty(0, 4, device=dev, dtype=torch.int64)
    if V == 0:                              # every face is dead; nothing to launch
        return MeshTopology(torch.empty(0, **i32), torch.full((F,), -1, **i32), torch.empty(0, **i32), components, loops, F, 0, unit)
    lib = _lib.load()
    scratch = torch.empty(int(lib.colvo_mesh_topology_scratch_bytes(V, F)), device=dev, dtype=torch.uint8)
    vertex_component = torch.empty(V, **i32)
    face_component = torch.empty(F, **i32)
    vertex_loop = torch.empty(V, **i32)
    stats = torch.empty(8, **i32)
    stream = _lib.stream_ptr()
    _lib.call("colvo_mesh_topology_components", faces, V, F, scratch, vertex_component, face_component, stats, stream)
    C = int(stats[0].item())
    if not 1 <= C <= V:
        raise RuntimeError(f"{who}: {C} components of {V} vertices: the component pass failed")
    components = torch.empty(C, 8, device=dev, dtype=torch.int64)
    _lib.call("colvo_mesh_topology_edges", vertices, faces, V, F, unit, C, scratch, vertex_component, face_component, components,
              vertex_loop, stats, stream)
    L = int(stats[2].item())
    if L > 0:
        loops = torch.empty(L, 4, device=dev, dtype=torch.int64)
        _lib.call("colvo_mesh_topology_loops", vertices, V, F, unit, C, L, scratch, vertex_component, vertex_loop, components, loops,
                  stats, stream)
    st = stats.tolist()
    if st[5] != 0:
        raise RuntimeError(f"{who}: a thread exhausted the bound of a union-find loop (gave_up = {st[5]}): the result is not valid")
    return MeshTopology(vertex_component, face_component, vertex_loop, components, loops, int(st[1]), int(st[3]) + int(st[4]), unit)


def clean_mesh(mesh: Mesh, topology: MeshTopology, *, min_faces: int = 1, min_area: float = 0.0,
               largest: Optional[int] = None) -> CleanedMesh:
    """The mesh without its debris.  A component of `topology` (mesh_topology of this mesh) is kept iff it has at
    least `min_faces` faces and an area of at least `min_area`; with largest=k only the k kept components with the most faces stay,
    ties going to the smaller number.  The kept vertices -- with their colours, normals and cells -- and the live faces of the kept
    components are gathered in their old order and the faces re-indexed; n_open is carried over.  vertex_index / face_index are the old
    rows of the new ones, `kept` the [C] mask.  The default min_faces = 1 removes exactly the face-less vertices and the dead faces.
    The decision over the [C] table is plain torch on the device; marks, scans and gathers are kernels.  Reads the two new counts
    back."""
    who = "clean_mesh"
    if not isinstance(mesh, Mesh):
        raise ValueError(f"{who}: mesh must be a Mesh")
    if not isinstance(topology, MeshTopology):
        raise ValueError(f"{who}: topology must be a MeshTopology (mesh_topology of this mesh)")
    int_range(who, "min_faces", min_faces, 0)
    if isinstance(min_area, bool) or not isinstance(min_area, (int, float)) or not math.isfinite(min_area) or min_area < 0.0:
        raise ValueError(f"{who}: min_area must be finite and >= 0, got {min_area!r}")
    if largest is not None:
        int_range(who, "largest", largest, 1)
    vertices, faces, V, F = mesh_arrays(who, mesh, None)
    dev = vertices.device
    comp = topology.components
    C = int(comp.shape[0])
    own_topology(who, topology, V, F, dev, ("components",))
    kept = (comp[:, 2] >= min_faces) & (topology.area >= float(min_area))
    if largest is not None and C > 0:
        key = torch.where(kept, comp[:, 2], torch.full_like(comp[:, 2], -1))
        order = torch.argsort(key, descending=True, stable=True)[:largest]      # stable: ties to the smaller number
        top = torch.zeros_like(kept)
        top[order] = True
        kept = kept & top
    i32 = dict(device=dev, dtype=torch.int32)
    V2 = F2 = 0
    vertex_index = torch.empty(0, **i32)
    face_index = torch.empty(0, **i32)
    lib = _lib.load() if V > 0 else None
    stream = _lib.stream_ptr() if V > 0 else 0
    if V > 0:
        kept8 = kept.to(torch.uint8).contiguous()
        scratch = torch.empty(int(lib.colvo_mesh_clean_scratch_bytes(V, F)), device=dev, dtype=torch.uint8)
        vertex_map = torch.empty(V, **i32)
        vertex_index = torch.empty(V, **i32)
        face_index = torch.empty(F, **i32)
        counts = torch.empty(2, **i32)
        vc, fc = topology.vertex_component.contiguous(), topology.face_component.contiguous()
        _lib.call("colvo_mesh_clean_plan", vc, fc, kept8, V, F, C, scratch, vertex_map, vertex_index, face_index, counts, stream)
        V2, F2 = (int(v) for v in counts.tolist())
        vertex_index, face_index = vertex_index[:V2], face_index[:F2]
    out_vertices = torch.empty(V2, 3, device=dev, dtype=torch.float32)
    out_colors = None if mesh.colors is None else torch.empty(V2, 3, device=dev, dtype=torch.float32)
    out_normals = torch.empty(V2, 3, device=dev, dtype=torch.float32)
    out_cells = torch.empty(V2, 3, **i32)
    out_faces = torch.empty(F2, 3, **i32)
    if V2 + F2 > 0:
        colors, normals, cells = mesh_attributes(who, mesh, V, dev)
        _lib.call("colvo_mesh_clean_write", vertices, colors, normals, cells, faces, V, F, vertex_map, vertex_index, face_index, V2, F2,
                  out_vertices, out_colors, out_normals, out_cells, out_faces, stream)
    return CleanedMesh(Mesh(out_vertices, out_faces, out_colors, out_normals, out_cells, mesh.n_open), vertex_index, face_index, kept)
