"""The holes of a triangle mesh: which boundary loops are simple rings, the ring of each in order, the area each hole spans, and the mesh
with the short rings closed by a fan to the ring's mean (fill_holes) -- DESIGN.md §3.6q, csrc/fill.hip, contract include/colvo.h
colvo_mesh_fill_*.  coivo_amd.inference re-exports every name here."""
from typing import NamedTuple

import torch

from . import _lib
from ._args import Mesh, int_range, mesh_arrays, mesh_attributes, own_topology
from .topology import MeshTopology

FILLED, TOO_LONG, NOT_SIMPLE, UNMEASURED = 0, 1, 2, 3
MAX_VERTICES = (1 << 30) - 1


class HoleFill(NamedTuple):
    mesh: Mesh                      # the input's rows, then one vertex per filled ring of more than three edges and the fans' faces
    status: torch.Tensor            # [L] int32 per loop: 0 FILLED, 1 TOO_LONG, 2 NOT_SIMPLE, 3 UNMEASURED
    hole: torch.Tensor              # [L,2] int64: fan faces written, hole area in quanta (0 for a loop that is not simple or unmeasured)
    ring_offsets: torch.Tensor      # [L+1] int32: the ring of loop l is ring_vertices[ring_offsets[l]:ring_offsets[l+1]]
    ring_vertices: torch.Tensor     # [R] int32: the rings of the simple loops, each from its smallest vertex along the half-edges
    face_loop: torch.Tensor         # [F'] int32: the loop a face fills, -1 for the input's faces
    new_vertex_loop: torch.Tensor   # [V'-V] int32: the loop of each new vertex
    unit: float                     # the topology's: an area quantum is unit^2 * 2^-16

    @property
    def hole_area(self) -> torch.Tensor:
        """[L] float64: the area of the fan over each simple measured loop, filled or not"""
        return self.hole[:, 1].to(torch.float64) * (float(self.unit) * float(self.unit) * 2.0 ** -16)

    @property
    def filled(self) -> torch.Tensor:
        """[L] bool"""
        return self.status == FILLED

    @property
    def simple(self) -> torch.Tensor:
        """[L] bool: the loop is one directed ring (it has a range in ring_vertices)"""
        return self.status != NOT_SIMPLE


def fill_holes(mesh: Mesh, topology: MeshTopology, *, max_edges: int) -> HoleFill:
    """Close the small holes of a mesh and measure every hole (contract: include/colvo.h colvo_mesh_fill_*, DESIGN.md §3.6q;
    csrc/fill.hip).  `topology` is mesh_topology of this mesh; its unit is the unit here.  A boundary loop is simple iff every one of its
    vertices has exactly one boundary half-edge leaving and one entering: its ring is then the loop's vertices in order, from the smallest
    along the half-edges.  Rings that touch in a vertex, borders through non-manifold vertices and inconsistently wound neighbours are not
    simple and are skipped whole.  Every simple loop gets a centre (the mean of its ring in length quanta, float32) and a hole area (the
    fan from the ring to that centre, in mesh_topology's area quanta) -- filled or not: the long loops are the large unseen regions.  A
    simple, measured loop of at most `max_edges` edges is filled: one new vertex (centre, mean colour, the fan's unit normal, cell
    (-1, -1, -1)) and one face per ring edge, wound like its neighbour across the border; a 3-ring gets its one face and no vertex.  New
    vertices come in loop order, new faces in (loop, ring position) order, behind the input's rows, which keep their bits (dead faces
    included); n_open is carried over.  Integer sums throughout: every output bit is a function of the inputs alone, identical between
    calls and streams and under a permutation of the faces (up to that of the first F face rows), and equals the NumPy replica
    tests/fill_ref.py.  A fan to the mean suits small, near-planar holes and can fold on a large or strongly curved one: max_edges is the
    guard.  Reads one small block back: the plan's counts."""
    who = "fill_holes"
    if not isinstance(mesh, Mesh):
        raise ValueError(f"{who}: mesh must be a Mesh")
    if not isinstance(topology, MeshTopology):
        raise ValueError(f"{who}: topology must be a MeshTopology (mesh_topology of this mesh)")
    int_range(who, "max_edges", max_edges, 3, (1 << 31) - 1)
    vertices, faces, V, F = mesh_arrays(who, mesh, None)
    dev = vertices.device
    own_topology(who, topology, V, F, dev, ("loops",))
    loops, vertex_loop = topology.loops, topology.vertex_loop
    L = int(loops.shape[0])
    if V > MAX_VERTICES:
        raise ValueError(f"{who}: V = {V} beyond the kernels' limit (V < 2^30)")
    unit = float(topology.unit)
    i32 = dict(device=dev, dtype=torch.int32)
    status = torch.empty(L, **i32)
    hole = torch.empty(L, 2, device=dev, dtype=torch.int64)
    if V == 0 or L == 0:                    # nothing to launch: the mesh comes back as it is
        return HoleFill(mesh, status, hole, torch.zeros(L + 1, **i32), torch.empty(0, **i32), torch.full((F,), -1, **i32),
                        torch.empty(0, **i32), unit)
    colors, normals, cells = mesh_attributes(who, mesh, V, dev)
    loops, vertex_loop = loops.contiguous(), vertex_loop.contiguous()
    lib = _lib.load()
    stream = _lib.stream_ptr()
    scratch = torch.empty(int(lib.colvo_mesh_fill_scratch_bytes(V, F, L)), device=dev, dtype=torch.uint8)
    ring_offsets = torch.empty(L + 1, **i32)
    ring_vertices = torch.empty(V, **i32)
    counts = torch.empty(8, **i32)
    _lib.call("colvo_mesh_fill_plan", vertices, faces, colors, V, F, L, unit, max_edges, vertex_loop, loops, scratch, status, hole,
              ring_offsets, ring_vertices, counts, stream)
    R, n_v, n_f, _, gave_up, _, _, mismatch = (int(c) for c in counts.tolist())
    if mismatch != 0:
        raise RuntimeError(f"{who}: topology is not this mesh's: its loops do not match the mesh's boundary half-edges")
    if gave_up != 0:
        raise RuntimeError(f"{who}: a ring's ranking did not end at its last vertex (status = {gave_up}): the result is not valid")
    if not (0 <= R <= V and 0 <= n_v <= L and 0 <= n_f <= R):
        raise RuntimeError(f"{who}: the plan's counts are not valid (R = {R}, new vertices = {n_v}, new faces = {n_f})")
    out_vertices = torch.empty(V + n_v, 3, device=dev, dtype=torch.float32)
    out_colors = None if colors is None else torch.empty(V + n_v, 3, device=dev, dtype=torch.float32)
    out_normals = torch.empty(V + n_v, 3, device=dev, dtype=torch.float32)
    out_cells = torch.empty(V + n_v, 3, **i32)
    out_faces = torch.empty(F + n_f, 3, **i32)
    face_loop = torch.empty(F + n_f, **i32)
    new_vertex_loop = torch.empty(n_v, **i32)
    _lib.call("colvo_mesh_fill_write", vertices, colors, normals, cells, faces, V, F, L, R, n_v, n_f, scratch, vertex_loop, status,
              ring_offsets, ring_vertices, out_vertices, out_colors, out_normals, out_cells, out_faces, face_loop,
              new_vertex_loop if n_v > 0 else 0, stream)
    return HoleFill(Mesh(out_vertices, out_faces, out_colors, out_normals, out_cells, mesh.n_open), status, hole, ring_offsets,
                    ring_vertices[:R].clone(), face_loop, new_vertex_loop, unit)      # (a clone: a view would keep all V entries alive)
