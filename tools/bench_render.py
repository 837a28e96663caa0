"""Time inference.render_cloud (csrc/render.hip) on one GPU with hip events around the whole call after a warm-up, with the
load-before-atomic form of the splat kernel (tuning entry render_load_first) against the plain form, alternating call by call, and
beside the torch composition a user would otherwise write (projection in torch ops frame by frame, footprints expanded with
repeat_interleave, scatter_reduce_('amin') on int64 keys), whose result is checked equal on every pixel.

    python tools/bench_render.py [--frames N] [--voxel V] [--radius R] [--max-splat S] [--iters K] [--warmup W] [--quick]

The cloud is the fused cloud (fuse_point_cloud, voxel V, with colours) of N frames of 256x320 of the tube scene
(tests/consistency_ref.py tube_scene), max_depth 4.5; it is rendered into the same N cameras with radius R (default: the voxel
size).  Prints us per call, G (point, frame) pairs per second and the atomic minimums issued per second, then one JSON line with
the same figures.  Byte model: the splat kernel reads the cloud once per group of 16 frames (12 B per point and group) and issues
one 8-byte atomic minimum per covered (point, pixel) pair; clear and resolve move 8 B + 8 B + (4 + 4 + 12) B per pixel and frame.
--quick: the native calls only (a profiler run).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coivo_amd import _lib, build, inference as I  # noqa: E402

H, W = 256, 320
MAX_DEPTH = 4.5
I64_MAX = torch.iinfo(torch.int64).max


def torch_render(points, colors, K, M, H, W, radius, max_splat, max_depth):
    """The contract of include/colvo.h colvo_render_cloud in torch ops (one kernel per operation: nothing is contracted), one frame
    at a time.  -> (depth [N,1,H,W], index [N,1,H,W] int32, colors [N,3,H,W], stats [N,4] int32)."""
    dev = points.device
    N, m = M.shape[0], points.shape[0]
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    ms, lo = f(float(max_splat)), f(-(max_splat + 1.0))
    x_hi, y_hi = f(float(W + max_splat)), f(float(H + max_splat))
    rad, md, eps, half, zero = f(radius), f(max_depth), f(1e-3), f(0.5), f(0.0)
    rows = torch.arange(m, device=dev, dtype=torch.int64)
    depth = torch.empty(N, 1, H, W, device=dev, dtype=torch.float32)
    index = torch.empty(N, 1, H, W, device=dev, dtype=torch.int32)
    out_c = torch.zeros(N, 3, H, W, device=dev, dtype=torch.float32)
    stats = torch.zeros(N, 4, device=dev, dtype=torch.int64)
    for n in range(N):
        q = [points[:, a] - M[n, a, 3] for a in range(3)]
        P = [(M[n, 0, a] * q[0] + M[n, 1, a] * q[1]) + M[n, 2, a] * q[2] for a in range(3)]
        front = (P[2] > eps) & (P[2] < md)
        x = (K[n, 0, 0] * P[0]) / P[2] + K[n, 0, 2]
        y = (K[n, 1, 1] * P[1]) / P[2] + K[n, 1, 2]
        hx = (K[n, 0, 0] * rad) / P[2]
        hy = (K[n, 1, 1] * rad) / P[2]
        clipped = front & ((hx > ms) | (hy > ms))
        hx, hy = torch.where(hx > ms, ms, hx), torch.where(hy > ms, ms, hy)
        on = front & (x >= lo) & (x <= x_hi) & (y >= lo) & (y <= y_hi)
        sel = on.nonzero().squeeze(1)
        xs, ys, hxs, hys = x[sel], y[sel], hx[sel], hy[sel]
        ucf, vcf = torch.floor(xs + half), torch.floor(ys + half)
        u_lo = torch.minimum(torch.ceil(xs - hxs), ucf).to(torch.int64).clamp_(min=0)
        u_hi = torch.maximum(torch.floor(xs + hxs), ucf).to(torch.int64).clamp_(max=W - 1)
        v_lo = torch.minimum(torch.ceil(ys - hys), vcf).to(torch.int64).clamp_(min=0)
        v_hi = torch.maximum(torch.floor(ys + hys), vcf).to(torch.int64).clamp_(max=H - 1)
        drawn = (u_lo <= u_hi) & (v_lo <= v_hi)
        sel, u_lo, u_hi, v_lo, v_hi = sel[drawn], u_lo[drawn], u_hi[drawn], v_lo[drawn], v_hi[drawn]
        key = (P[2][sel].view(torch.int32).to(torch.int64) << 32) | rows[sel]
        wu = u_hi - u_lo + 1
        area = wu * (v_hi - v_lo + 1)
        owner = torch.repeat_interleave(torch.arange(sel.shape[0], device=dev), area)
        off = torch.arange(owner.shape[0], device=dev) - (torch.cumsum(area, 0) - area)[owner]
        pix = (v_lo[owner] + off // wu[owner]) * W + u_lo[owner] + off % wu[owner]
        keys = torch.full((H * W,), I64_MAX, device=dev, dtype=torch.int64)
        keys.scatter_reduce_(0, pix, key[owner], "amin")
        hit = keys != I64_MAX
        idx = keys & 0xFFFFFFFF
        depth[n, 0] = torch.where(hit, (keys >> 32).to(torch.int32).view(torch.float32), float("inf")).view(H, W)
        index[n, 0] = torch.where(hit, idx, -1).to(torch.int32).view(H, W)
        if colors is not None:
            out_c[n] = torch.where(hit[None], colors[torch.where(hit, idx, 0)].t(), zero).view(3, H, W)
        stats[n, 0], stats[n, 1], stats[n, 2], stats[n, 3] = front.sum(), sel.shape[0], clipped.sum(), hit.sum()
    return depth, index, (out_c if colors is not None else None), stats.to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--radius", type=float, default=None)
    ap.add_argument("--max-splat", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="native calls only (no torch composition): a profiler run")
    a = ap.parse_args()
    build.ensure()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    from tests import consistency_ref as R
    N = a.frames
    depths, K, M = (torch.from_numpy(x).to(dev).contiguous() for x in R.tube_scene(N, H, W, 3))
    g = torch.Generator().manual_seed(5)
    frames = torch.rand(N, 3, H, W, generator=g).to(dev)
    fused = I.fuse_point_cloud(depths, K, M, voxel_size=a.voxel, colors=frames, max_depth=MAX_DEPTH)
    del depths, frames
    radius = fused.voxel_size if a.radius is None else a.radius
    m = fused.points.shape[0]
    kw = dict(radius=radius, colors=fused.colors, max_splat=a.max_splat, max_depth=MAX_DEPTH)
    call = lambda: I.render_cloud(fused.points, K, M, H, W, **kw)
    out = dict(bench="render_cloud", N=N, H=H, W=W, voxel=a.voxel, radius=radius, max_splat=a.max_splat, points=m, iters=a.iters,
               warmup=a.warmup)
    saved = _lib.tune_get("render_load_first")
    times = {0: [], 1: []}
    try:
        for form in (0, 1):
            _lib.tune_set("render_load_first", form)
            for _ in range(a.warmup):
                r = call()
        torch.cuda.synchronize()
        for k in range(2 * a.iters):                                # alternating call by call
            form = k & 1
            _lib.tune_set("render_load_first", form)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            r = call()
            t1.record()
            t1.synchronize()
            times[form].append(t0.elapsed_time(t1) * 1e3)
    finally:
        _lib.tune_set("render_load_first", saved)
    stats = r.stats.sum(0).tolist()
    out.update(front=stats[0], drawn=stats[1], clipped=stats[2], covered=stats[3], covered_fraction=round(stats[3] / (N * H * W), 4),
               default_form=int(saved))
    pairs = m * N
    for form, name in ((0, "plain"), (1, "load_first")):
        t = sorted(times[form])
        us = sum(t) / len(t)
        out[name] = dict(us=round(us, 1), us_min=round(t[0], 1), us_max=round(t[-1], 1), pairs_per_s=round(pairs / us * 1e6),
                         drawn_per_s=round(stats[1] / us * 1e6))
        print(f"{name:10s}: {us:9.1f} us per call (min {t[0]:.1f}, max {t[-1]:.1f})  {pairs / us * 1e-3:7.2f} G (point, frame) pairs/s  "
              f"{stats[1] / us:7.1f} M drawn points/s", flush=True)
    print(f"{m} points into {N} views of {H}x{W}: front {stats[0]}, drawn {stats[1]}, clipped {stats[2]}, covered pixels {stats[3]} "
          f"({100.0 * stats[3] / (N * H * W):.1f} %)", flush=True)
    if not a.quick:
        ours = call()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        theirs = torch_render(fused.points, fused.colors, K, M, H, W, radius, a.max_splat, MAX_DEPTH)         # warm-up and the check
        t0.record()
        for _ in range(2):
            torch_render(fused.points, fused.colors, K, M, H, W, radius, a.max_splat, MAX_DEPTH)
        t1.record()
        t1.synchronize()
        t_us = t0.elapsed_time(t1) * 1e3 / 2
        bits = lambda t: t.contiguous().view(torch.int32)
        px = N * H * W
        same = dict(depth=int((bits(ours.depth) == bits(theirs[0])).sum()) / px, index=int((ours.index == theirs[1]).sum()) / px,
                    colors=int((bits(ours.colors) == bits(theirs[2])).sum()) / (3 * px), stats=bool(torch.equal(ours.stats, theirs[3])))
        ref_us = out["load_first" if saved else "plain"]["us"]
        out.update(torch_us=round(t_us, 1), speedup_vs_torch=round(t_us / ref_us, 2), equal_fraction_vs_torch=same)
        print(f"torch composition {t_us:.1f} us: x{out['speedup_vs_torch']:.2f}; equal pixels: {same}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
