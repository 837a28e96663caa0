"""Time inference.filter_depths (csrc/consistency.hip) beside the same check written in torch ops, on one GPU, with hip events
after a warm-up, the two alternating call by call in one process.

    python tools/bench_consistency.py [--frames N] [--iters K] [--warmup W] [--windows 1,2,4] [--out FILE] [--quick]

N frames of 256x320 of the tube scene (tests/consistency_ref.py tube_scene: the inside of a unit cylinder, 0.05 advance per
frame), step 1, rel_tol 0.01, max_depth 4.5.  Byte model of the call: every pixel's depth is read once as the centre and once
per frame that takes it as a neighbour, (1 + neighbours) * 4 B, and 4 + 3 B are written (27 B per pixel at window 2, a little
less at the ends of the sequence, which the figure below accounts for); reported as TB/s and as a share of the 8 TB/s of HBM.
The torch composition (torch_filter) is what a user would otherwise write: one batched pass per frame offset, every operation
a kernel of its own.  Also timed: the statistics with every workgroup of a frame adding to one counter line and to one of
eight (tuning entry consist_stat_lines).  Prints one JSON line; --out also writes it to a file.
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
REL_TOL = 0.01
HBM_BYTES_PER_S = 8e12


def torch_filter(depths, K, M, *, window, step, rel_tol, min_agree, max_violated, max_depth):
    """The contract in torch ops, batched over the frames that have the neighbour at each offset.  -> (depths, votes)."""
    N, _, Hh, Ww = depths.shape
    dev = depths.device
    d = depths[:, 0]
    cand = (d > 0) & (d < max_depth)
    v = torch.arange(Hh, device=dev, dtype=torch.float32).view(1, -1, 1)
    u = torch.arange(Ww, device=dev, dtype=torch.float32).view(1, 1, -1)
    k_ = lambda Kx, i, j: Kx[:, i, j].view(-1, 1, 1)
    px = ((u - k_(K, 0, 2)) / k_(K, 0, 0)) * d
    py = ((v - k_(K, 1, 2)) / k_(K, 1, 1)) * d
    votes = torch.zeros(N, 3, Hh, Ww, device=dev, dtype=torch.uint8)
    M64 = M.double()
    flat = depths.reshape(N, Hh * Ww)
    for k in [o for o in range(-window, window + 1) if o != 0]:
        off = k * step
        lo, hi = max(0, -off), min(N, N - off)
        if lo >= hi:
            continue
        i, j = slice(lo, hi), slice(lo + off, hi + off)
        Rj, Ri = M64[j, :3, :3], M64[i, :3, :3]
        R = (Rj.transpose(1, 2) @ Ri).float()
        t = (Rj.transpose(1, 2) @ (M64[i, :3, 3] - M64[j, :3, 3]).unsqueeze(-1)).squeeze(-1).float()
        r = lambda a, b: R[:, a, b].view(-1, 1, 1)
        P = [((r(a, 0) * px[i] + r(a, 1) * py[i]) + r(a, 2) * d[i]) + t[:, a].view(-1, 1, 1) for a in range(3)]
        Kj = K[j]
        x = (k_(Kj, 0, 0) * P[0]) / P[2] + k_(Kj, 0, 2)
        y = (k_(Kj, 1, 1) * P[1]) / P[2] + k_(Kj, 1, 2)
        seen = cand[i] & (P[2] > 1e-3) & (x >= 0) & (x <= Ww - 1) & (y >= 0) & (y <= Hh - 1)
        x0f, y0f = torch.floor(x), torch.floor(y)
        wx, wy = x - x0f, y - y0f
        x0 = torch.where(seen, x0f, torch.zeros_like(x0f)).long()
        y0 = torch.where(seen, y0f, torch.zeros_like(y0f)).long()
        x1, y1 = (x0 + 1).clamp(max=Ww - 1), (y0 + 1).clamp(max=Hh - 1)
        src = flat[j]
        tap = lambda yy, xx: torch.gather(src, 1, (yy * Ww + xx).view(hi - lo, -1)).view(hi - lo, Hh, Ww)
        t00, t01, t10, t11 = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
        visible = seen
        for tp in (t00, t01, t10, t11):
            visible = visible & (tp > 0) & (tp < max_depth)
        s = (((t00 * (1 - wx)) + (t01 * wx)) * (1 - wy)) + (((t10 * (1 - wx)) + (t11 * wx)) * wy)
        rel = (P[2] - s).abs() / (P[2] + s)
        ok, occ = rel < rel_tol, s < P[2]
        votes[i, 0] += (visible & ok).to(torch.uint8)
        votes[i, 1] += (visible & ~ok & occ).to(torch.uint8)
        votes[i, 2] += (visible & ~ok & ~occ).to(torch.uint8)
    kept = cand & (votes[:, 0] >= min_agree) & (votes[:, 2] <= max_violated)
    out = torch.where(kept, d, torch.full_like(d, float("inf"))).unsqueeze(1)
    return out, votes


def alternate_us(fns, iters, warmup):
    """Mean microseconds of each callable, the callables taking turns call by call (the same clocks and thermal state)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    total = [0.0] * len(fns)
    for _ in range(iters):
        for n, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            total[n] += a.elapsed_time(b) * 1e3
    return [t / iters for t in total]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", default="1,2,4")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--quick", action="store_true", help="the native call only (no torch composition, no counter-line comparison): a profiler run")
    a = ap.parse_args()
    build.ensure()
    if not torch.cuda.is_available():
        raise SystemExit("bench_consistency.py measures on the GPU; none found")
    from tests import consistency_ref as R
    dev = torch.device("cuda:0")
    N = a.frames
    depths, K, M = (torch.from_numpy(x).to(dev).contiguous() for x in R.tube_scene(N, H, W, 3))
    out = dict(bench="filter_depths", N=N, H=H, W=W, step=1, rel_tol=REL_TOL, max_depth=MAX_DEPTH, iters=a.iters, warmup=a.warmup,
               hbm_bytes_per_s=HBM_BYTES_PER_S, stat_lines_default=_lib.tune_get("consist_stat_lines"), windows={})
    default_lines = _lib.tune_get("consist_stat_lines")
    for window in (int(w) for w in a.windows.split(",")):
        kw = dict(window=window, step=1, rel_tol=REL_TOL, min_agree=1, max_violated=0, max_depth=MAX_DEPTH)
        neighbours = sum(min(window, i) + min(window, N - 1 - i) for i in range(N))
        model_bytes = H * W * (4 * (N + neighbours) + 7 * N)
        row = dict(neighbours_per_frame=round(neighbours / N, 3), model_bytes_per_pixel=round(model_bytes / (N * H * W), 2))
        ours = I.filter_depths(depths, K, M, **kw)
        st = ours.stats.sum(0).tolist()
        row["stats"] = dict(zip(("candidates", "kept", "no_view", "few_agree", "violated_out"), st))
        fns = [lambda: I.filter_depths(depths, K, M, **kw)]
        if not a.quick:
            fns.append(lambda: torch_filter(depths, K, M, **kw))
        us = alternate_us(fns, a.iters, a.warmup)
        row["kernel_us"] = round(us[0], 1)
        row["model_tb_per_s"] = round(model_bytes / us[0] * 1e6 / 1e12, 3)
        row["share_of_hbm"] = round(model_bytes / us[0] * 1e6 / HBM_BYTES_PER_S, 3)
        line = (f"window {window}: filter_depths {us[0]:9.1f} us  {row['model_tb_per_s']:.2f} TB/s of the byte model "
                f"({100 * row['share_of_hbm']:.0f} % of 8 TB/s, {row['model_bytes_per_pixel']} B per pixel)")
        if not a.quick:
            td, tv = torch_filter(depths, K, M, **kw)
            row["torch_us"] = round(us[1], 1)
            row["speedup_vs_torch"] = round(us[1] / us[0], 2)
            row["votes_equal_to_torch"] = float((tv == ours.votes).float().mean())
            row["kept_equal_to_torch"] = float((torch.isfinite(td) == torch.isfinite(ours.depths)).float().mean())
            line += (f"  | torch composition {us[1]:9.1f} us: x{row['speedup_vs_torch']:.2f}; votes equal on "
                     f"{100 * row['votes_equal_to_torch']:.4f} % of the entries")
            del td, tv
        print(line, flush=True)
        out["windows"][str(window)] = row
        del ours
    if not a.quick:
        # the statistics: one counter line per frame against eight, the two taking turns (the result's bits do not depend on it)
        kw = dict(window=2, step=1, rel_tol=REL_TOL, max_depth=MAX_DEPTH)
        try:
            def with_lines(n):
                def fn():
                    _lib.tune_set("consist_stat_lines", n)
                    I.filter_depths(depths, K, M, **kw)
                return fn
            us = alternate_us([with_lines(1), with_lines(8)], a.iters, a.warmup)
        finally:
            _lib.tune_set("consist_stat_lines", default_lines)
        out["stat_lines_us_window2"] = {"1": round(us[0], 1), "8": round(us[1], 1)}
        print(f"window 2, workgroups of a frame adding to 1 counter line {us[0]:.1f} us, to one of 8 {us[1]:.1f} us", flush=True)
    text = json.dumps(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    # the yardstick must do the same work: its votes are those of the kernel but for samples at a decision boundary (torch's own
    # kernels need not round as the contract does)
    for window, row in out["windows"].items():
        if min(row.get("votes_equal_to_torch", 1.0), row.get("kept_equal_to_torch", 1.0)) < 0.999:
            raise SystemExit(f"window {window}: the torch composition disagrees with filter_depths: {row}")


if __name__ == "__main__":
    main()
