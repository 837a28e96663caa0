"""Time inference.fuse_tsdf / extract_mesh (csrc/tsdf.hip) per phase on one GPU, with hip events after a warm-up, beside
fuse_point_cloud on the same input and beside a plain torch composition of the voxel-centric update over the same allocated voxels.

    python tools/bench_tsdf.py [--frames N] [--voxel V] [--iters K] [--warmup W] [--torch-frames F] [--out PATH]

tools/bench_fuse.py's scene: N frames of 256x320 from coivo_amd.synth along a random trajectory, stride 1, with colours, max_depth
4.5, four voxels of truncation.  Event windows: plan, integrate (tuning entry tsdf_cull on and off), mesh count + vertices (which
includes counting and scanning the triangles) and the face write.  Also: allocated bricks, frames each brick walked after the cull
(mean and maximum), V and F.  The torch composition evaluates the contract's per-frame update with torch ops (one kernel per
operation, float32 sums of the quanta as int64 index-free adds) for --torch-frames frames only -- it visits every allocated voxel for
every frame, as the unculled kernel does -- and is reported per frame beside the unculled kernel's time per frame.  Prints one JSON
line and, with --out, writes it to that file.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coivo_amd import _args, _lib, build, inference as I  # noqa: E402
from bench_fuse import H, MAX_DEPTH, W, make, time_us  # noqa: E402

T = 4


class Phases:
    """The C calls of fuse_tsdf and extract_mesh on buffers sized once (what the wrappers do between their read-backs)."""

    def __init__(self, depths, colors, K, M, origin, dims, vs, min_obs):
        self.lib = lib = _lib.load()
        N = depths.shape[0]
        dev = depths.device
        self.t = (depths, colors, K, M)
        self.N, self.grid, self.dims, self.min_obs = N, (*origin, vs, *dims), dims, min_obs
        total = dims[0] * dims[1] * dims[2] // 512
        self.scratch = torch.empty(int(lib.colvo_tsdf_plan_scratch_bytes(N, H, W, 1, *dims)), device=dev, dtype=torch.uint8)
        self.table = torch.empty(total, device=dev, dtype=torch.int32)
        self.list = torch.empty(min(total, 1 << 22), device=dev, dtype=torch.int32)
        self.stats = torch.empty(3, device=dev, dtype=torch.int32)
        self.plan()
        self.n_input, self.n_outside, self.n_bricks = (int(x) for x in self.stats.tolist())
        self.pool = torch.empty(self.n_bricks * 512, 2, device=dev, dtype=torch.int32)
        self.sums = torch.empty(self.n_bricks * 512, 4, device=dev, dtype=torch.int32)
        self.survivors = torch.empty(self.n_bricks, device=dev, dtype=torch.int32)
        self.integrate()
        self.mscratch = torch.empty(int(lib.colvo_tsdf_mesh_scratch_bytes(self.n_bricks)), device=dev, dtype=torch.uint8)
        self.stats2 = torch.empty(3, device=dev, dtype=torch.int32)
        self.count()
        self.V, self.n_open = (int(x) for x in self.stats2[:2].tolist())
        self.vertices = torch.empty(self.V, 3, device=dev, dtype=torch.float32)
        self.colors = torch.empty(self.V, 3, device=dev, dtype=torch.float32)
        self.normals = torch.empty(self.V, 3, device=dev, dtype=torch.float32)
        self.cells = torch.empty(self.V, 3, device=dev, dtype=torch.int32)
        self.vid = torch.empty(self.n_bricks * 512, device=dev, dtype=torch.int32)
        self.write_vertices()
        self.F = int(self.stats2[2].item())
        self.faces = torch.empty(self.F, 3, device=dev, dtype=torch.int32)

    def plan(self):
        d, c, K, M = self.t
        _lib.check(self.lib.colvo_tsdf_plan(_lib.ptr(d), _lib.ptr(K), _lib.ptr(M), self.N, H, W, 1, MAX_DEPTH, *self.grid, T,
                                            _lib.ptr(self.scratch), _lib.ptr(self.table), _lib.ptr(self.list), _lib.ptr(self.stats),
                                            _lib.stream_ptr()), "colvo_tsdf_plan")

    def integrate(self):
        d, c, K, M = self.t
        _lib.check(self.lib.colvo_tsdf_integrate(_lib.ptr(d), _lib.ptr(c), _lib.ptr(K), _lib.ptr(M), self.N, H, W, MAX_DEPTH, *self.grid,
                                                 T, _lib.ptr(self.list), self.n_bricks, _lib.ptr(self.pool), _lib.ptr(self.sums),
                                                 _lib.ptr(self.survivors), _lib.stream_ptr()), "colvo_tsdf_integrate")

    def count(self):
        _lib.check(self.lib.colvo_tsdf_mesh_count(_lib.ptr(self.pool), _lib.ptr(self.table), _lib.ptr(self.list), self.n_bricks,
                                                  self.min_obs, *self.dims, _lib.ptr(self.mscratch), _lib.ptr(self.stats2),
                                                  _lib.stream_ptr()), "colvo_tsdf_mesh_count")

    def write_vertices(self):
        _lib.check(self.lib.colvo_tsdf_mesh_vertices(_lib.ptr(self.pool), _lib.ptr(self.sums), _lib.ptr(self.table), _lib.ptr(self.list),
                                                     self.n_bricks, self.min_obs, *self.grid, _lib.ptr(self.mscratch), self.V,
                                                     _lib.ptr(self.vertices), _lib.ptr(self.colors), _lib.ptr(self.normals),
                                                     _lib.ptr(self.cells), _lib.ptr(self.vid), self.stats2[2:].data_ptr(),
                                                     _lib.stream_ptr()), "colvo_tsdf_mesh_vertices")

    def count_vertices(self):
        self.count()
        self.write_vertices()

    def write_faces(self):
        _lib.check(self.lib.colvo_tsdf_mesh_faces(_lib.ptr(self.pool), _lib.ptr(self.table), _lib.ptr(self.list), self.n_bricks,
                                                  *self.dims, _lib.ptr(self.mscratch), _lib.ptr(self.vid), self.F, _lib.ptr(self.faces),
                                                  _lib.stream_ptr()), "colvo_tsdf_mesh_faces")


def torch_integrate(depths, K, M, origin, dims, vs, brick_list, frames):
    """The contract's voxel-centric update in torch ops over every voxel of the allocated bricks, for the given frames:
    (sum q, n) as int64 tensors."""
    dev = depths.device
    nb = [d // 8 for d in dims]
    b = brick_list.long()
    loc = torch.arange(512, device=dev)
    idx = [(b % nb[0])[:, None] * 8 + (loc & 7)[None], ((b // nb[0]) % nb[1])[:, None] * 8 + ((loc >> 3) & 7)[None],
           (b // (nb[0] * nb[1]))[:, None] * 8 + (loc >> 6)[None]]
    c = [origin[a] + (idx[a].reshape(-1).float() + 0.5) * vs for a in range(3)]
    trunc = T * vs
    sq = torch.zeros_like(c[0], dtype=torch.int64)
    n = torch.zeros_like(sq)
    for f in frames:
        r, t = M[f, :3, :3], M[f, :3, 3]
        q = [c[a] - t[a] for a in range(3)]
        P = [(r[0, a] * q[0] + r[1, a] * q[1]) + r[2, a] * q[2] for a in range(3)]
        x = torch.floor((K[f, 0, 0] * P[0]) / P[2] + K[f, 0, 2] + 0.5)
        y = torch.floor((K[f, 1, 1] * P[1]) / P[2] + K[f, 1, 2] + 0.5)
        ok = (P[2] > 1e-3) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
        d = depths[f, 0][torch.where(ok, y, 0).long(), torch.where(ok, x, 0).long()]
        sdf = d - P[2]
        ok &= (d > 0) & (d < MAX_DEPTH) & ~(sdf < -trunc)
        sq += torch.where(ok, torch.round(torch.clamp(sdf, max=trunc) * (4096.0 / trunc)), 0).long()
        n += ok
    return sq, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--min-obs", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-frames", type=int, default=8, help="frames the torch composition walks (0: skip it)")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    build.ensure()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    N = a.frames
    depths, colors, K, M = make(N, dev)
    origin, dims = I.fusion_grid(K, M, H, W, a.voxel, MAX_DEPTH)
    vs = _args.f32(a.voxel)
    ph = Phases(depths, colors, K, M, origin, dims, vs, a.min_obs)
    surv = ph.survivors.float()
    out = dict(bench="fuse_tsdf", N=N, H=H, W=W, stride=1, voxel=a.voxel, T=T, min_obs=a.min_obs, dims=list(dims),
               bricks_in_grid=dims[0] * dims[1] * dims[2] // 512, n_input=ph.n_input, n_outside=ph.n_outside, n_bricks=ph.n_bricks,
               pool_mb=round((ph.pool.numel() + ph.sums.numel()) * 4 / 2 ** 20, 1), V=ph.V, F=ph.F, n_open=ph.n_open,
               frames_walked_per_brick_mean=round(float(surv.mean()), 2), frames_walked_per_brick_max=int(surv.max()),
               iters=a.iters, warmup=a.warmup)
    print(json.dumps(out), flush=True)
    saved = _lib.tune_get("tsdf_cull")
    try:
        for name, fn in (("plan", ph.plan), ("integrate", ph.integrate), ("count_vertices", ph.count_vertices), ("faces", ph.write_faces)):
            out[name + "_us"] = round(time_us(fn, a.iters, a.warmup), 1)
        # the same walk without the three colour gathers per observation (what the depth gather and the arithmetic alone cost)
        held, ph.t, ph.sums = (ph.t, ph.sums), (depths, None, K, M), None
        out["integrate_no_colors_us"] = round(time_us(ph.integrate, a.iters, a.warmup), 1)
        ph.t, ph.sums = held
        _lib.tune_set("tsdf_cull", 0)
        out["integrate_no_cull_us"] = round(time_us(ph.integrate, max(2, a.iters // 3), 1), 1)
    finally:
        _lib.tune_set("tsdf_cull", saved)
    voxel_frames = float(surv.sum()) * 512
    out["integrate_voxel_frames"] = voxel_frames
    out["integrate_voxel_frames_per_s"] = round(voxel_frames / out["integrate_us"] * 1e6, 0)
    out["integrate_no_cull_voxel_frames_per_s"] = round(ph.n_bricks * 512.0 * N / out["integrate_no_cull_us"] * 1e6, 0)
    out["whole_us"] = round(time_us(lambda: I.extract_mesh(I.fuse_tsdf(depths, K, M, voxel_size=a.voxel, colors=colors, max_depth=MAX_DEPTH,
                                                                       origin=origin, dims=dims), min_obs=a.min_obs), a.iters, a.warmup), 1)
    out["fuse_point_cloud_us"] = round(time_us(lambda: I.fuse_point_cloud(depths, K, M, voxel_size=a.voxel, colors=colors, stride=1,
                                                                          max_depth=MAX_DEPTH, origin=origin, dims=dims), a.iters,
                                               a.warmup), 1)
    if a.torch_frames > 0:
        frames = list(range(min(a.torch_frames, N)))
        t_us = time_us(lambda: torch_integrate(depths, K, M, origin, dims, vs, ph.list[:ph.n_bricks], frames), 2, 1)
        out["torch_frames"] = len(frames)
        out["torch_us_per_frame"] = round(t_us / len(frames), 1)
        out["integrate_no_cull_us_per_frame"] = round(out["integrate_no_cull_us"] / N, 1)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
