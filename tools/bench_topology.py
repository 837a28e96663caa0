"""Time inference.mesh_topology / clean_mesh (csrc/topology.hip) per call on one GPU, with hip events after a warm-up, on the mesh
of tools/bench_tsdf.py's scene, and report what that mesh is.

    python tools/bench_topology.py [--frames N] [--voxel V] [--min-obs M] [--iters K] [--warmup W] [--no-cpu] [--out PATH]

tools/bench_fuse.py's scene: N frames of 256x320 from coivo_amd.synth along a random trajectory, stride 1, with colours, max_depth
4.5, four voxels of truncation; fuse_tsdf -> extract_mesh gives the mesh.  Event windows, each a C call on buffers sized once:
colvo_mesh_topology_components (union-find over the faces, flatten, numbering of the roots), _edges (component records, areas, side
buckets, the bucket scan, the loops' union-find and numbering), _loops (loop records and lengths), colvo_mesh_clean_plan and _write for
min_faces = 1; then the whole wrappers with their read-backs; for scale, extract_mesh's own calls on the same volume and a CPU
connected-components pass over the same faces (scipy.sparse.csgraph if it is installed, else the replica's sequential union-find).
The kernels inside one call are not separated here: a kernel trace of this tool does that.  Prints one JSON line and, with --out,
writes it to that file.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from coivo_amd import _args, _lib, build, inference as I  # noqa: E402
from bench_fuse import H, MAX_DEPTH, W, make, time_us  # noqa: E402


class Phases:
    """The C calls of mesh_topology and clean_mesh on buffers sized once (what the wrappers do between their read-backs)."""

    def __init__(self, mesh, unit):
        self.lib = lib = _lib.load()
        self.mesh, self.unit = mesh, unit
        self.V, self.F = V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
        dev = mesh.vertices.device
        i32 = dict(device=dev, dtype=torch.int32)
        self.scratch = torch.empty(int(lib.colvo_mesh_topology_scratch_bytes(V, F)), device=dev, dtype=torch.uint8)
        self.vc, self.fc, self.vl = torch.empty(V, **i32), torch.empty(F, **i32), torch.empty(V, **i32)
        self.stats = torch.empty(8, **i32)
        self.components()
        self.C = int(self.stats[0].item())
        self.comp = torch.empty(self.C, 8, device=dev, dtype=torch.int64)
        self.edges()
        self.L = int(self.stats[2].item())
        self.loop = torch.empty(max(self.L, 1), 4, device=dev, dtype=torch.int64)
        self.kept = (self.comp[:, 2] >= 1).to(torch.uint8)
        self.cscratch = torch.empty(int(lib.colvo_mesh_clean_scratch_bytes(V, F)), device=dev, dtype=torch.uint8)
        self.vmap, self.vindex, self.findex = torch.empty(V, **i32), torch.empty(V, **i32), torch.empty(F, **i32)
        self.counts = torch.empty(2, **i32)
        self.clean_plan()
        self.V2, self.F2 = (int(x) for x in self.counts.tolist())
        self.out = [torch.empty(self.V2, 3, device=dev, dtype=torch.float32) for _ in range(3)]
        self.out_cells, self.out_faces = torch.empty(self.V2, 3, **i32), torch.empty(self.F2, 3, **i32)

    def components(self):
        _lib.check(self.lib.colvo_mesh_topology_components(_lib.ptr(self.mesh.faces), self.V, self.F, _lib.ptr(self.scratch), _lib.ptr(self.vc),
                                                           _lib.ptr(self.fc), _lib.ptr(self.stats), _lib.stream_ptr()),
                   "colvo_mesh_topology_components")

    def edges(self):
        _lib.check(self.lib.colvo_mesh_topology_edges(_lib.ptr(self.mesh.vertices), _lib.ptr(self.mesh.faces), self.V, self.F, self.unit,
                                                      self.C, _lib.ptr(self.scratch), _lib.ptr(self.vc), _lib.ptr(self.fc),
                                                      _lib.ptr(self.comp), _lib.ptr(self.vl), _lib.ptr(self.stats), _lib.stream_ptr()),
                   "colvo_mesh_topology_edges")

    def loops(self):
        _lib.check(self.lib.colvo_mesh_topology_loops(_lib.ptr(self.mesh.vertices), self.V, self.F, self.unit, self.C, self.L,
                                                      _lib.ptr(self.scratch), _lib.ptr(self.vc), _lib.ptr(self.vl), _lib.ptr(self.comp),
                                                      _lib.ptr(self.loop), _lib.ptr(self.stats), _lib.stream_ptr()),
                   "colvo_mesh_topology_loops")

    def clean_plan(self):
        _lib.check(self.lib.colvo_mesh_clean_plan(_lib.ptr(self.vc), _lib.ptr(self.fc), _lib.ptr(self.kept), self.V, self.F, self.C,
                                                  _lib.ptr(self.cscratch), _lib.ptr(self.vmap), _lib.ptr(self.vindex), _lib.ptr(self.findex),
                                                  _lib.ptr(self.counts), _lib.stream_ptr()), "colvo_mesh_clean_plan")

    def clean_write(self):
        m = self.mesh
        _lib.check(self.lib.colvo_mesh_clean_write(_lib.ptr(m.vertices), _lib.ptr(m.colors), _lib.ptr(m.normals), _lib.ptr(m.cells),
                                                   _lib.ptr(m.faces), self.V, self.F, _lib.ptr(self.vmap), _lib.ptr(self.vindex),
                                                   _lib.ptr(self.findex), self.V2, self.F2, _lib.ptr(self.out[0]),
                                                   _lib.ptr(self.out[1] if m.colors is not None else None), _lib.ptr(self.out[2]),
                                                   _lib.ptr(self.out_cells), _lib.ptr(self.out_faces), _lib.stream_ptr()),
                   "colvo_mesh_clean_write")


def cpu_components(faces, V):
    """(what ran, seconds, components) of a CPU connected-components pass over the faces' (a, b) and (b, c) pairs"""
    f = faces.cpu().numpy().astype("int64")
    try:
        import numpy as np
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        t0 = time.perf_counter()
        rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
        n, _ = connected_components(coo_matrix((np.ones(len(rows), "int8"), (rows, cols)), shape=(V, V)), directed=False)
        return "scipy.sparse.csgraph.connected_components", time.perf_counter() - t0, int(n)
    except ImportError:
        from tests import topology_ref as T
        t0 = time.perf_counter()
        root = T._union_find(V, [p for a, b, c in f.tolist() for p in ((a, b), (b, c))])
        return "tests/topology_ref.py union-find", time.perf_counter() - t0, int((root == range(V)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--min-obs", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU connected-components pass")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    build.ensure()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topology.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    depths, colors, K, M = make(a.frames, dev)
    origin, dims = I.fusion_grid(K, M, H, W, a.voxel, MAX_DEPTH)
    unit = _args.f32(a.voxel)
    volume = I.fuse_tsdf(depths, K, M, voxel_size=a.voxel, colors=colors, max_depth=MAX_DEPTH, origin=origin, dims=dims)
    mesh = I.extract_mesh(volume, min_obs=a.min_obs)
    topo = I.mesh_topology(mesh, unit=unit)
    ph = Phases(mesh, unit)
    c = topo.components
    with_faces = c[:, 2] > 0
    sides = torch.cat([mesh.faces[:, [0, 1]], mesh.faces[:, [1, 2]], mesh.faces[:, [2, 0]]]).long()
    out = dict(bench="mesh_topology", N=a.frames, H=H, W=W, voxel=a.voxel, min_obs=a.min_obs, V=ph.V, F=ph.F, n_open=mesh.n_open,
               C=int(c.shape[0]), C_with_faces=int(with_faces.sum()), faceless_vertices=int((~with_faces).sum()), L=int(topo.loops.shape[0]),
               largest_faces=int(c[:, 2].max()), largest_face_share=round(float(c[:, 2].max()) / max(ph.F, 1), 6),
               components_under_4_faces=int((with_faces & (c[:, 2] < 4)).sum()),
               edges=int(c[:, 3].sum()), boundary_edges=int(c[:, 4].sum()), nonmanifold_edges=int(c[:, 5].sum()),
               closed_components=int(topo.closed.sum()), area=float(topo.area.sum()), loop_length=float(topo.length.sum()),
               longest_loop_edges=int(topo.loops[:, 2].max()) if topo.loops.shape[0] else 0,
               n_dead_faces=topo.n_dead_faces, n_unmeasured=topo.n_unmeasured,
               max_sides_per_lower_endpoint=int(torch.bincount(sides.min(1).values).max()),
               scratch_mb=round(ph.scratch.numel() / 2 ** 20, 1), iters=a.iters, warmup=a.warmup)
    print(json.dumps(out), flush=True)
    for name, fn in (("components", ph.components), ("edges", ph.edges), ("loops", ph.loops), ("clean_plan", ph.clean_plan),
                     ("clean_write", ph.clean_write)):
        if name == "loops" and ph.L == 0:
            continue
        out[name + "_us"] = round(time_us(fn, a.iters, a.warmup), 1)
    out["mesh_topology_us"] = round(time_us(lambda: I.mesh_topology(mesh, unit=unit), a.iters, a.warmup), 1)
    out["clean_mesh_us"] = round(time_us(lambda: I.clean_mesh(mesh, topo, min_faces=1), a.iters, a.warmup), 1)
    cleaned = I.clean_mesh(mesh, topo, min_faces=1)
    out["cleaned_V"], out["cleaned_F"] = int(cleaned.mesh.vertices.shape[0]), int(cleaned.mesh.faces.shape[0])
    out["extract_mesh_us"] = round(time_us(lambda: I.extract_mesh(volume, min_obs=a.min_obs), a.iters, a.warmup), 1)
    if not a.no_cpu:
        what, seconds, n = cpu_components(mesh.faces, ph.V)
        assert n == out["C"], (n, out["C"])
        out["cpu_components"], out["cpu_components_us"] = what, round(seconds * 1e6, 1)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
