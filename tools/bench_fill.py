"""Time inference.fill_holes (csrc/fill.hip) per call on one GPU, with hip events after a warm-up, on the mesh of tools/bench_tsdf.py's
scene, and report what the holes of that mesh are.

    python tools/bench_fill.py [--frames N] [--voxel V] [--min-obs M] [--max-edges E] [--iters K] [--warmup W] [--out PATH]

tools/bench_topology.py's mesh: N frames of 256x320 from coivo_amd.synth along a random trajectory, stride 1, with colours, max_depth
4.5, four voxels of truncation; fuse_tsdf -> extract_mesh -> mesh_topology.  Event windows, each a C call on buffers sized once:
colvo_mesh_fill_plan (half-edges, classify, rank, measure, number) and colvo_mesh_fill_write at --max-edges; then the whole wrapper with
its read-back, and mesh_topology's wrapper on the same mesh for scale.  For max_edges 8, 32 and 1024: how many loops are simple,
unmeasured and filled, the summed hole area, and the loops and non-manifold edges of the filled mesh.  The kernels inside one call are
not separated here: a kernel trace of this tool does that.  Prints one JSON line and, with --out, writes it to that file.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from coivo_amd import _args, _lib, build, holes, inference as I  # noqa: E402
from bench_fuse import H, MAX_DEPTH, W, make, time_us  # noqa: E402


class Phases:
    """The C calls of fill_holes on buffers sized once (what the wrapper does between its read-backs)."""

    def __init__(self, mesh, topo, max_edges):
        self.lib = lib = _lib.load()
        self.mesh, self.topo, self.max_edges = mesh, topo, max_edges
        self.V, self.F, self.L = V, F, L = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0]), int(topo.loops.shape[0])
        dev = mesh.vertices.device
        i32 = dict(device=dev, dtype=torch.int32)
        self.scratch = torch.empty(int(lib.colvo_mesh_fill_scratch_bytes(V, F, L)), device=dev, dtype=torch.uint8)
        self.status, self.hole = torch.empty(L, **i32), torch.empty(L, 2, device=dev, dtype=torch.int64)
        self.ring_offsets, self.ring_vertices, self.counts = torch.empty(L + 1, **i32), torch.empty(V, **i32), torch.empty(8, **i32)
        self.plan()
        self.R, self.nv, self.nf = (int(x) for x in self.counts[:3].tolist())
        self.out = [torch.empty(V + self.nv, 3, device=dev, dtype=torch.float32) for _ in range(3)]
        self.out_cells, self.out_faces = torch.empty(V + self.nv, 3, **i32), torch.empty(F + self.nf, 3, **i32)
        self.face_loop, self.new_vertex_loop = torch.empty(F + self.nf, **i32), torch.empty(max(self.nv, 1), **i32)

    def plan(self):
        m, t = self.mesh, self.topo
        _lib.check(self.lib.colvo_mesh_fill_plan(_lib.ptr(m.vertices), _lib.ptr(m.faces), _lib.ptr(m.colors), self.V, self.F, self.L,
                                                 t.unit, self.max_edges, _lib.ptr(t.vertex_loop), _lib.ptr(t.loops),
                                                 _lib.ptr(self.scratch), _lib.ptr(self.status), _lib.ptr(self.hole),
                                                 _lib.ptr(self.ring_offsets), _lib.ptr(self.ring_vertices), _lib.ptr(self.counts),
                                                 _lib.stream_ptr()), "colvo_mesh_fill_plan")

    def write(self):
        m, t = self.mesh, self.topo
        _lib.check(self.lib.colvo_mesh_fill_write(_lib.ptr(m.vertices), _lib.ptr(m.colors), _lib.ptr(m.normals), _lib.ptr(m.cells),
                                                  _lib.ptr(m.faces), self.V, self.F, self.L, self.R, self.nv, self.nf,
                                                  _lib.ptr(self.scratch), _lib.ptr(t.vertex_loop), _lib.ptr(self.status),
                                                  _lib.ptr(self.ring_offsets), _lib.ptr(self.ring_vertices), _lib.ptr(self.out[0]),
                                                  _lib.ptr(self.out[1] if m.colors is not None else None), _lib.ptr(self.out[2]),
                                                  _lib.ptr(self.out_cells), _lib.ptr(self.out_faces), _lib.ptr(self.face_loop),
                                                  _lib.ptr(self.new_vertex_loop), _lib.stream_ptr()), "colvo_mesh_fill_write")


def holes_of(mesh, topo, max_edges):
    """what fill_holes finds and leaves at one max_edges"""
    r = I.fill_holes(mesh, topo, max_edges=max_edges)
    after = I.mesh_topology(r.mesh, unit=topo.unit)
    st, n = r.status, topo.loops[:, 2]
    simple = st != holes.NOT_SIMPLE
    return dict(max_edges=max_edges, simple=int(simple.sum()), not_simple=int((~simple).sum()), unmeasured=int((st == holes.UNMEASURED).sum()),
                filled=int(r.filled.sum()), too_long=int((st == holes.TOO_LONG).sum()),
                boundary_edges_on_simple_loops=int(n[simple].sum()), boundary_edges_on_filled_loops=int(n[r.filled].sum()),
                hole_area=float(r.hole_area.sum()), hole_area_filled=float(r.hole_area[r.filled].sum()),
                new_vertices=int(r.new_vertex_loop.shape[0]), new_faces=int(r.hole[:, 0].sum()),
                loops_after=int(after.loops.shape[0]), boundary_edges_after=int(after.components[:, 4].sum()),
                nonmanifold_edges_after=int(after.components[:, 5].sum()), closed_components_after=int(after.closed.sum()),
                area_after=float(after.area.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--min-obs", type=int, default=2)
    ap.add_argument("--max-edges", type=int, default=32, help="the policy the timed calls run with")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    build.ensure()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fill.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    depths, colors, K, M = make(a.frames, dev)
    origin, dims = I.fusion_grid(K, M, H, W, a.voxel, MAX_DEPTH)
    unit = _args.f32(a.voxel)
    volume = I.fuse_tsdf(depths, K, M, voxel_size=a.voxel, colors=colors, max_depth=MAX_DEPTH, origin=origin, dims=dims)
    mesh = I.extract_mesh(volume, min_obs=a.min_obs)
    topo = I.mesh_topology(mesh, unit=unit)
    ph = Phases(mesh, topo, a.max_edges)
    c = topo.components
    out = dict(bench="fill_holes", N=a.frames, H=H, W=W, voxel=a.voxel, min_obs=a.min_obs, V=ph.V, F=ph.F, L=ph.L,
               boundary_edges=int(c[:, 4].sum()), nonmanifold_edges=int(c[:, 5].sum()), area=float(topo.area.sum()),
               longest_loop_edges=int(topo.loops[:, 2].max().item()), longest_simple_loop_edges=int(ph.counts[3].item()),
               doubling_rounds=max(int(ph.counts[3].item()) - 1, 0).bit_length(),
               round_launches=max(min(ph.V, 3 * ph.F) - 1, 0).bit_length(), ring_vertices=ph.R, scratch_mb=round(ph.scratch.numel() / 2 ** 20, 1),
               timed_max_edges=a.max_edges, iters=a.iters, warmup=a.warmup)
    print(json.dumps(out), flush=True)
    out["plan_us"] = round(time_us(ph.plan, a.iters, a.warmup), 1)
    out["write_us"] = round(time_us(ph.write, a.iters, a.warmup), 1)
    out["fill_holes_us"] = round(time_us(lambda: I.fill_holes(mesh, topo, max_edges=a.max_edges), a.iters, a.warmup), 1)
    out["mesh_topology_us"] = round(time_us(lambda: I.mesh_topology(mesh, unit=unit), a.iters, a.warmup), 1)
    out["policies"] = [holes_of(mesh, topo, e) for e in (8, 32, 1024)]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
