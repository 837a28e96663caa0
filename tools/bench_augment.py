"""Time the augmenting conversion kernel (csrc/augment.hip, colvo_frames_u8_augment) beside the plain one (csrc/frames.hip,
colvo_frames_u8_to_f32) on one GPU, with hip events after a warm-up, the variants alternating round by round:

    python tools/bench_augment.py [--frames 16] [--iters K] [--rounds R]

Two sizes: `frames` frames 256x320 native (no resize) and 1080x1350 -> 256x320.  Three variants: plain, augment (rows drawn by
data.Augment(): crop, mirror, colour, gamma), augment with gamma fixed at 1 (no powf).  Prints per variant the median and the spread
of the rounds in us and the rate of the byte model -- the source rectangle read once plus 12 B per output pixel (the plain pass reads
the whole frame, a crop of zoom s 1/s^2 of it) -- then one JSON line with the same figures.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coivo_amd import _lib, build, data as D  # noqa: E402

H, W = 256, 320


def time_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    build.ensure()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n = a.frames
    result = dict(bench="frames_u8_augment", frames=n, H=H, W=W, iters=a.iters, rounds=a.rounds, sizes={})
    for h, w in ((256, 320), (1080, 1350)):
        g = torch.Generator().manual_seed(h)
        u8 = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
        out = torch.empty(n, 3, H, W, device=dev)
        tabs, src_bytes = {}, {"plain": n * h * w * 3}
        for name, aug in (("augment", D.Augment()), ("augment_gamma1", D.Augment(gamma=(1.0, 1.0)))):
            recs = [aug.params(0, 0, i, (h, w)) for i in range(n // 2)]
            tabs[name] = torch.from_numpy(D.aug_table([r.tgt for r in recs] + [r.ref for r in recs], H, W)).to(dev)
            src_bytes[name] = int(sum(2 * 3 * r.ch * r.cw for r in recs))
        fns = {"plain": lambda: _lib.check(lib.colvo_frames_u8_to_f32(_lib.ptr(u8), n, h, w, H, W, _lib.ptr(out), _lib.stream_ptr()),
                                           "colvo_frames_u8_to_f32")}
        for name, tab in tabs.items():
            fns[name] = lambda tab=tab: _lib.check(lib.colvo_frames_u8_augment(_lib.ptr(u8), n, h, w, H, W, _lib.ptr(tab), _lib.ptr(out),
                                                                              _lib.stream_ptr()), "colvo_frames_u8_augment")
        iters = a.iters if h == H else max(1, a.iters // 4)
        for fn in fns.values():
            time_us(fn, max(1, iters // 10))                        # warm-up
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append(time_us(fn, iters))
        rows = {}
        for k, t in times.items():
            med = statistics.median(t)
            nbytes = src_bytes[k] + n * 12 * H * W
            rows[k] = dict(us_median=round(med, 2), us_min=round(min(t), 2), us_max=round(max(t), 2), model_bytes=nbytes,
                           model_gb_per_s=round(nbytes / med * 1e-3, 1))
            print(f"{n} x {h}x{w} -> {H}x{W} {k:15s}: {med:8.2f} us (rounds {min(t):.2f} .. {max(t):.2f}), {nbytes / 1e6:.2f} MB of the "
                  f"byte model = {rows[k]['model_gb_per_s']:.0f} GB/s, x{med / statistics.median(times['plain']):.3f} of plain", flush=True)
        result["sizes"][f"{h}x{w}"] = rows
    print(json.dumps(result))


if __name__ == "__main__":
    main()
