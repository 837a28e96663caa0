"""Time inference.cloud_normals (csrc/normals.hip) beside fuse_point_cloud, and inference.render_surfels (csrc/surfels.hip) beside
render_cloud, on one GPU with hip events around the whole call after a warm-up, the two calls of a pair alternating call by call in
one process (the way tools/bench_render.py alternates its two forms).

    python tools/bench_surfels.py [--frames N] [--voxel V] [--radius R] [--max-splat S] [--iters K] [--warmup W]

The scene is tools/bench_render.py's: N frames of 256x320 of the tube (tests/consistency_ref.py tube_scene, seed 3), max_depth 4.5,
fused at voxel V with colours; the cloud is drawn into the same N cameras with radius R (default: the voxel size), squares against
discs with the cloud's own normals.  fuse_point_cloud reads two counts back between its phases, so its time holds two host round
trips; cloud_normals reads nothing back.  Prints us per call with min and max, then one JSON line with the same figures.
Byte model: the normals' accumulate pass reads 4 B per sample and up to four neighbours (cache hits at stride 1),
about log2(M) 8-byte keys per sample with a normal (the top of the search tree stays in cache) and issues four 8-byte atomic adds
into one 32-byte sector; the surfel splat reads 24 B per point and frame group and, per pixel of a footprint, does one division and
at most one 8-byte load and one atomic minimum.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coivo_amd import build, inference as I  # noqa: E402

H, W = 256, 320
MAX_DEPTH = 4.5


def alternate(calls, iters, warmup):
    """{name: sorted us per call} of the calls given, warmed up one after the other and then timed alternating call by call."""
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(iters):
        for name, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e3)
    return {name: sorted(t) for name, t in times.items()}


def summary(t):
    return dict(us=round(sum(t) / len(t), 1), us_min=round(t[0], 1), us_max=round(t[-1], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--radius", type=float, default=None)
    ap.add_argument("--max-splat", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    build.ensure()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surfels.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    from tests import consistency_ref as R
    N = a.frames
    depths, K, M = (torch.from_numpy(x).to(dev).contiguous() for x in R.tube_scene(N, H, W, 3))
    g = torch.Generator().manual_seed(5)
    frames = torch.rand(N, 3, H, W, generator=g).to(dev)
    fuse = lambda: I.fuse_point_cloud(depths, K, M, voxel_size=a.voxel, colors=frames, max_depth=MAX_DEPTH)
    fused = fuse()
    normals = lambda: I.cloud_normals(fused, depths, K, M, max_depth=MAX_DEPTH)
    cn = normals()
    m = fused.points.shape[0]
    radius = fused.voxel_size if a.radius is None else a.radius
    out = dict(bench="surfels", N=N, H=H, W=W, voxel=a.voxel, radius=radius, max_splat=a.max_splat, points=m, iters=a.iters, warmup=a.warmup,
               normals_stats=cn.stats.tolist(), rows_with_a_normal=int((cn.counts > 0).sum()),
               coherence_min=float(cn.coherence.min()), coherence_median=float(cn.coherence.median()))
    t = alternate(dict(fuse_point_cloud=fuse, cloud_normals=normals), a.iters, a.warmup)
    for name in t:
        out[name] = summary(t[name])
        print(f"{name:18s}: {out[name]['us']:9.1f} us per call (min {out[name]['us_min']:.1f}, max {out[name]['us_max']:.1f})", flush=True)
    out["cloud_normals"]["samples_per_s"] = round(cn.stats[0].item() / out["cloud_normals"]["us"] * 1e6)
    del frames
    kw = dict(radius=radius, colors=fused.colors, max_splat=a.max_splat, max_depth=MAX_DEPTH)
    squares = lambda: I.render_cloud(fused.points, K, M, H, W, **kw)
    discs = lambda: I.render_surfels(fused.points, cn.normals, K, M, H, W, **kw)
    shaded = lambda: I.render_surfels(fused.points, cn.normals, K, M, H, W, want_normals=True, **kw)
    t = alternate(dict(render_cloud=squares, render_surfels=discs, render_surfels_with_normal_planes=shaded), a.iters, a.warmup)
    for name in t:
        out[name] = summary(t[name])
        print(f"{name:34s}: {out[name]['us']:9.1f} us per call (min {out[name]['us_min']:.1f}, max {out[name]['us_max']:.1f})", flush=True)
    out["discs_over_squares"] = round(out["render_surfels"]["us"] / out["render_cloud"]["us"], 3)
    sq, di = squares(), discs()
    out.update(squares_stats=sq.stats.sum(0).tolist(), discs_stats=di.stats.sum(0).tolist())
    # what the discs buy: the model's depth against the scene's exact depth, over the pixels both forms cover
    both = (sq.index >= 0) & (di.index >= 0) & (depths < MAX_DEPTH)
    for name, r in (("squares", sq), ("discs", di)):
        rel = ((r.depth[both] - depths[both]).abs() / depths[both])
        out[f"{name}_rel_err_median"] = float(rel.median())
        print(f"{name}: median relative error of the rendered depth {100 * out[f'{name}_rel_err_median']:.4f} % over {int(both.sum())} pixels",
              flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
