"""Time evaluate.depth_metrics (csrc/evaluate.hip) against the torch composition of the same measures (torch.nanmedian over
[N, H*W] plus elementwise ops), on one GPU, with hip events after a warm-up.

    python tools/bench_eval.py [--iters K] [--warmup W] [--quick]

Prints one line per case: us per call, GB/s on the byte model of DESIGN.md §3.6b (three median passes and the metric pass,
each reading pred and gt, 8 B per pixel, +1 B with a mask: 32 / 36 B per pixel), its fraction of 8 TB/s, the torch
composition's us and the ratio; then one JSON line with the same figures.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coivo_amd import build, evaluate as E  # noqa: E402

LO, HI = 0.1, 10.0
PEAK = 8e12


def make(N, H, W, with_mask, dev, seed=0):
    """Smooth depth maps as a depth network gives them (a product of sinusoids per image, 0.5..5), a prediction off by a
    scale and 10 % noise, a strip beyond max_depth; the mask keeps 90 %."""
    g = torch.Generator(device=dev).manual_seed(seed)
    v = torch.arange(H, device=dev, dtype=torch.float32).view(1, 1, H, 1)
    u = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, 1, W)
    r = torch.rand(N, 4, 1, 1, generator=g, device=dev)
    fu, fv = 2 * math.pi * (0.5 + r[:, 0:1]) / W, 2 * math.pi * (0.5 + r[:, 1:2]) / W
    gt = 2.75 + 2.25 * torch.sin(fu * u + 6.28 * r[:, 2:3]) * torch.cos(fv * v + 6.28 * r[:, 3:4])
    gt[:, :, : H // 32] = 12.0
    pred = 0.4 * gt * torch.exp(0.1 * torch.randn(gt.shape, generator=g, device=dev))
    mask = torch.rand(gt.shape, generator=g, device=dev) < 0.9 if with_mask else None
    return pred.contiguous(), gt.contiguous(), mask


def torch_metrics(pred, gt, mask):
    """The same measures in torch: nanmedian per image, float32 terms, float64 sums."""
    N = pred.shape[0]
    P, G = pred.view(N, -1), gt.view(N, -1)
    valid = (G > LO) & (G < HI)
    if mask is not None:
        valid &= mask.view(N, -1)
    nan = torch.tensor(float("nan"), device=pred.device)
    mg = torch.nanmedian(torch.where(valid, G, nan), dim=1).values
    mp = torch.nanmedian(torch.where(valid, P, nan), dim=1).values
    p = ((mg / mp)[:, None] * P).clamp(LO, HI)
    n = valid.sum(dim=1).double()
    d = G - p
    th = torch.maximum(G / p, p / G)
    terms = (d.abs() / G, d * d / G, d * d, (torch.log(G) - torch.log(p)) ** 2, (th < 1.25).float(), (th < 1.5625).float(),
             (th < 1.953125).float())
    out = torch.stack([torch.where(valid, t, 0.0).sum(dim=1, dtype=torch.float64) / n for t in terms], dim=1)
    out[:, 2:4] = out[:, 2:4].sqrt()
    return out


def time_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="native calls only (no torch composition): a profiler run")
    a = ap.parse_args()
    build.ensure()
    dev = torch.device("cuda:0")
    rows = []
    for N, H, W in ((512, 256, 320), (64, 512, 640)):
        for with_mask in (False, True):
            pred, gt, mask = make(N, H, W, with_mask, dev)
            us = time_us(lambda: E.depth_metrics(pred, gt, mask), a.iters, a.warmup)
            model = N * H * W * (36 if with_mask else 32)
            row = dict(N=N, H=H, W=W, mask=with_mask, us=round(us, 1), model_bytes=model, gbps=round(model / us * 1e-3, 1),
                       frac_of_8tbs=round(model / us * 1e6 / PEAK, 3))
            if not a.quick:
                t_us = time_us(lambda: torch_metrics(pred, gt, mask), max(3, a.iters // 4), 1)
                ours = E.depth_metrics(pred, gt, mask).per_image
                ref = torch_metrics(pred, gt, mask)
                row.update(torch_us=round(t_us, 1), speedup=round(t_us / us, 2),
                           max_rel_vs_torch=float(((ours - ref).abs() / ref.abs().clamp_min(1e-12)).max()))
            rows.append(row)
            print(f"N={N:4d} {H}x{W} mask={int(with_mask)}: {us:9.1f} us  {row['gbps']:7.1f} GB/s  "
                  f"{100 * row['frac_of_8tbs']:5.1f} % of 8 TB/s" +
                  ("" if a.quick else f"  | torch {row['torch_us']:10.1f} us  x{row['speedup']:.1f}"), flush=True)
            del pred, gt, mask
            torch.cuda.empty_cache()
    print(json.dumps({"bench": "depth_metrics", "rows": rows}))


if __name__ == "__main__":
    main()
