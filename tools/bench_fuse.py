"""Time inference.fuse_point_cloud (csrc/fuse.hip) per phase and as a whole, beside stitch_point_cloud on the same input (what
merely reading the depths and writing one point per sample costs) and beside the torch composition a user would otherwise write
(pinned point in torch ops, torch.unique(return_inverse=True) over the voxel keys, index_add_ of count, positions and colours),
on one GPU, with hip events after a warm-up.

    python tools/bench_fuse.py [--frames N] [--voxel V] [--iters K] [--warmup W] [--quick]

N frames of 256x320 from coivo_amd.synth along a random trajectory (steps of 0.05 in translation, 0.03 rad in rotation), stride 1,
with colours, max_depth 4.5.  Prints us, samples per second and added atomic bytes per second for plan / accumulate / extract and
the whole call, with the wave aggregation (tuning entry fuse_agg_rounds) and the row-wise adds (fuse_row_adds) on and off and a
sweep of the round count;
then one JSON line with the same figures.  Byte model of the accumulate phase: every inside sample adds four 64-bit words = 32 B
(two words = 16 B without colours); with the aggregation the lanes of a wave that share a voxel add once, so the bytes that reach
memory lie between 32 B x (distinct (wave, voxel) pairs) and 32 B x samples; both are reported, beside the 1.3 TB/s that
MI355X sustains for float atomics in 256-B wave-instructions.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coivo_amd import _args, _lib, build, inference as I, synth  # noqa: E402

H, W = 256, 320
MAX_DEPTH = 4.5
FLOAT_ATOMIC_RATE = 1.3e12


def make(N, dev, seed=5, chunk=64):
    """depths [N,1,H,W], colours [N,3,H,W], K [N,3,3], cam2world [N,4,4] on `dev`."""
    depths, colors, Ks = [], [], []
    for i in range(0, N, chunk):
        b = synth.make_batch(min(chunk, N - i), H, W, seed=seed + i)
        depths.append(b["gt_depth"].to(dev))
        colors.append(b["tgt"].to(dev))
        Ks.append(b["K"].to(dev))
    g = torch.Generator().manual_seed(seed)
    rel = torch.cat([0.05 * torch.randn(N, 3, generator=g), 0.03 * torch.randn(N, 3, generator=g)], dim=1)
    M = I.integrate_trajectory(rel)[1:].to(dev, torch.float32)
    return torch.cat(depths).contiguous(), torch.cat(colors).contiguous(), torch.cat(Ks).contiguous(), M.contiguous()


def torch_keys(depths, K, M, origin, dims, vs, stride, max_depth):
    """The contract's point and voxel in torch ops (one kernel per operation: nothing is contracted).  -> inside mask
    [N,Hs,Ws], world points [S,3] and linear voxel keys [S] (int64) of the inside samples."""
    dev = depths.device
    d = depths[:, 0, ::stride, ::stride]
    v = torch.arange(0, depths.shape[2], stride, device=dev, dtype=torch.float32).view(1, -1, 1)
    u = torch.arange(0, depths.shape[3], stride, device=dev, dtype=torch.float32).view(1, 1, -1)
    k = lambda i, j: K[:, i, j].view(-1, 1, 1)
    m = lambda i, j: M[:, i, j].view(-1, 1, 1)
    px = (u - k(0, 2)) / k(0, 0) * d
    py = (v - k(1, 2)) / k(1, 1) * d
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(vs, dtype=torch.float32)
    inside = (d > 0) & (d < max_depth)
    X, g = [], []
    for a in range(3):
        X.append(((m(a, 0) * px + m(a, 1) * py) + m(a, 2) * d) + m(a, 3))
        g.append((X[a] - origin[a]) * inv.item())
        inside &= (g[a] >= 0) & (g[a] < float(dims[a]))
    idx = [torch.floor(g[a][inside]).to(torch.int64) for a in range(3)]
    key = (idx[2] * dims[1] + idx[1]) * dims[0] + idx[0]
    return inside, torch.stack([X[a][inside] for a in range(3)], 1), key


def torch_fuse(depths, colors, K, M, origin, dims, vs, stride=1, max_depth=MAX_DEPTH, min_obs=1):
    """Mean position, mean colour and count per occupied voxel, in ascending linear voxel order (float32 sums in arrival order)."""
    inside, pts, key = torch_keys(depths, K, M, origin, dims, vs, stride, max_depth)
    uniq, inverse = torch.unique(key, return_inverse=True)
    n = uniq.shape[0]
    cnt = torch.zeros(n, device=key.device, dtype=torch.float32).index_add_(0, inverse, torch.ones_like(inverse, dtype=torch.float32))
    pos = torch.zeros(n, 3, device=key.device, dtype=torch.float32).index_add_(0, inverse, pts)
    col = colors[:, :, ::stride, ::stride].permute(0, 2, 3, 1)[inside]
    csum = torch.zeros(n, 3, device=key.device, dtype=torch.float32).index_add_(0, inverse, col)
    rows = cnt >= min_obs
    return pos[rows] / cnt[rows, None], csum[rows] / cnt[rows, None], cnt[rows].to(torch.int32), uniq[rows]


def wave_voxel_pairs(depths, K, M, origin, dims, vs):
    """Distinct (wave, voxel) pairs at stride 1: a wave owns an 8x8 pixel tile of one frame.  The fewest groups of adds the
    aggregation can issue (reached when no wave holds more distinct voxels than fuse_agg_rounds)."""
    inside, _, key = torch_keys(depths, K, M, origin, dims, vs, 1, MAX_DEPTH)
    N, Hs, Ws = inside.shape
    n = torch.arange(N, device=key.device).view(-1, 1, 1)
    ty = (torch.arange(Hs, device=key.device) // 8).view(1, -1, 1)
    tx = (torch.arange(Ws, device=key.device) // 8).view(1, 1, -1)
    tile = ((n * ((Hs + 7) // 8) + ty) * ((Ws + 7) // 8) + tx).expand(N, Hs, Ws)[inside]
    return int(torch.unique(tile * (dims[0] * dims[1] * dims[2]) + key).shape[0])      # < 2^20 tiles a frame-set, < 2^31 voxels


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


class Phases:
    """The four C calls of fuse_point_cloud on buffers sized once (what the wrapper does between its two read-backs)."""

    def __init__(self, depths, colors, K, M, origin, dims, vs, min_obs):
        self.lib = lib = _lib.load()
        N = depths.shape[0]
        dev = depths.device
        self.t = (depths, colors, K, M)
        self.geom = (N, H, W, 1, MAX_DEPTH, *origin, vs, *dims)
        self.grid = (*origin, vs, *dims)
        self.min_obs = min_obs
        self.ws = torch.empty(int(lib.colvo_fuse_plan_workspace_bytes(N, H, W, 1, *dims)), device=dev, dtype=torch.uint8)
        self.stats = torch.empty(3, device=dev, dtype=torch.int32)
        self.plan()
        self.n_input, self.n_outside, self.n_bricks = (int(x) for x in self.stats.tolist())
        self.pool = torch.empty(int(lib.colvo_fuse_pool_bytes(self.n_bricks)), device=dev, dtype=torch.uint8)
        self.ews = torch.empty(int(lib.colvo_fuse_extract_workspace_bytes(self.n_bricks)), device=dev, dtype=torch.uint8)
        self.stats2 = torch.empty(3, device=dev, dtype=torch.int32)
        self.accumulate()
        self.count()
        self.n_voxels, self.m, overflow = (int(x) for x in self.stats2.tolist())
        assert not overflow
        self.points = torch.empty(self.m, 3, device=dev, dtype=torch.float32)
        self.colors = torch.empty(self.m, 3, device=dev, dtype=torch.float32)
        self.counts = torch.empty(self.m, device=dev, dtype=torch.int32)
        self.voxels = torch.empty(self.m, 3, device=dev, dtype=torch.int32)

    def plan(self):
        d, c, K, M = self.t
        _lib.check(self.lib.colvo_fuse_plan(_lib.ptr(d), _lib.ptr(K), _lib.ptr(M), *self.geom, _lib.ptr(self.ws), _lib.ptr(self.stats),
                                            _lib.stream_ptr()), "colvo_fuse_plan")

    def accumulate(self):
        d, c, K, M = self.t
        _lib.check(self.lib.colvo_fuse_accumulate(_lib.ptr(d), _lib.ptr(c), _lib.ptr(K), _lib.ptr(M), *self.geom, _lib.ptr(self.ws),
                                                  self.n_bricks, _lib.ptr(self.pool), _lib.stream_ptr()), "colvo_fuse_accumulate")

    def count(self):
        _lib.check(self.lib.colvo_fuse_count(_lib.ptr(self.pool), self.n_bricks, self.min_obs, _lib.ptr(self.ews), _lib.ptr(self.stats2),
                                             _lib.stream_ptr()), "colvo_fuse_count")

    def write(self):
        _lib.check(self.lib.colvo_fuse_write(_lib.ptr(self.ws), _lib.ptr(self.pool), self.n_bricks, self.min_obs, *self.grid,
                                             _lib.ptr(self.ews), self.m, _lib.ptr(self.points), _lib.ptr(self.colors), _lib.ptr(self.counts),
                                             _lib.ptr(self.voxels), _lib.stream_ptr()), "colvo_fuse_write")

    def extract(self):
        self.count()
        self.write()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--min-obs", type=int, default=1)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="native calls only (no torch composition, no pair count): a profiler run")
    a = ap.parse_args()
    build.ensure()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fuse.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    N = a.frames
    depths, colors, K, M = make(N, dev)
    origin, dims = I.fusion_grid(K, M, H, W, a.voxel, MAX_DEPTH)
    vs = _args.f32(a.voxel)
    ph = Phases(depths, colors, K, M, origin, dims, vs, a.min_obs)
    inside = ph.n_input - ph.n_outside
    out = dict(bench="fuse_point_cloud", N=N, H=H, W=W, stride=1, voxel=a.voxel, min_obs=a.min_obs, dims=list(dims),
               bricks_in_grid=dims[0] * dims[1] * dims[2] // 512, n_input=ph.n_input, n_outside=ph.n_outside, n_bricks=ph.n_bricks,
               n_voxels=ph.n_voxels, rows=ph.m, pool_mb=round(ph.pool.numel() / 2 ** 20, 1), iters=a.iters, warmup=a.warmup)
    print(json.dumps({k: out[k] for k in ("dims", "bricks_in_grid", "n_input", "n_outside", "n_bricks", "n_voxels", "rows", "pool_mb")}),
          flush=True)
    default_rounds, default_rows = _lib.tune_get("fuse_agg_rounds"), _lib.tune_get("fuse_row_adds")
    samples = N * H * W

    def rate(us, n):
        return round(n / us * 1e6, 0)

    phases = {}
    try:
        for name, rounds, rows in (("default", default_rounds, default_rows), ("aggregated_lane_adds", default_rounds, 0),
                                   ("single_row_adds", 0, 1), ("single_lane_adds", 0, 0)):
            _lib.tune_set("fuse_agg_rounds", rounds)
            _lib.tune_set("fuse_row_adds", rows)
            row = dict(rounds=rounds, row_adds=rows)
            for phase, fn in (("plan", ph.plan), ("accumulate", ph.accumulate), ("extract", ph.extract)):
                row[phase + "_us"] = round(time_us(fn, a.iters, a.warmup), 1)
            row["whole_us"] = round(time_us(lambda: I.fuse_point_cloud(depths, K, M, voxel_size=a.voxel, colors=colors, stride=1,
                                                                       max_depth=MAX_DEPTH, min_obs=a.min_obs, origin=origin,
                                                                       dims=dims), a.iters, a.warmup), 1)
            row["samples_per_s"] = {p: rate(row[p + "_us"], samples) for p in ("plan", "accumulate", "extract", "whole")}
            row["accumulate_sample_bytes_per_s"] = rate(row["accumulate_us"], inside * 32)
            phases[name] = row
            print(f"{name:20s} (rounds {rounds:g}, row adds {rows:g}): plan {row['plan_us']:8.1f} us  accumulate {row['accumulate_us']:8.1f} us  "
                  f"extract {row['extract_us']:8.1f} us  whole {row['whole_us']:9.1f} us  | {row['samples_per_s']['whole'] / 1e9:6.2f} G samples/s, "
                  f"accumulate {row['accumulate_sample_bytes_per_s'] / 1e12:5.2f} TB/s of sample bytes "
                  f"({row['accumulate_sample_bytes_per_s'] / FLOAT_ATOMIC_RATE:4.2f} x the float-atomic rate)", flush=True)
        sweep = {}
        for rows in (1, 0):
            _lib.tune_set("fuse_row_adds", rows)
            for rounds in (0, 1, 2, 4, 8, 16, 32, 48, 64):
                _lib.tune_set("fuse_agg_rounds", rounds)
                sweep[f"rows{rows}_rounds{rounds}"] = round(time_us(ph.accumulate, a.iters, a.warmup), 1)
        print("accumulate us by fuse_row_adds / fuse_agg_rounds:", sweep, flush=True)
        out["accumulate_us_sweep"] = sweep
    finally:
        _lib.tune_set("fuse_agg_rounds", default_rounds)
        _lib.tune_set("fuse_row_adds", default_rows)
    out["phases"] = phases
    out["pool_clear_us"] = round(time_us(lambda: ph.pool.zero_(), a.iters, a.warmup), 1)
    out["stitch_us"] = round(time_us(lambda: I.stitch_point_cloud(depths, K, M, stride=1, max_depth=MAX_DEPTH), a.iters, a.warmup), 1)
    print(f"pool clear alone {out['pool_clear_us']:.1f} us ({out['pool_mb']} MB); stitch_point_cloud {out['stitch_us']:.1f} us", flush=True)
    if not a.quick:
        pairs = wave_voxel_pairs(depths, K, M, origin, dims, vs)
        out["wave_voxel_pairs"] = pairs
        agg = phases["default"]
        agg["accumulate_issued_bytes_per_s_min"] = rate(agg["accumulate_us"], pairs * 32)
        print(f"distinct (wave, voxel) pairs {pairs} of {inside} inside samples ({inside / pairs:.2f} samples per pair): the aggregated "
              f"pass issues at least {agg['accumulate_issued_bytes_per_s_min'] / 1e12:.2f} TB/s of atomic bytes", flush=True)
        t_us = time_us(lambda: torch_fuse(depths, colors, K, M, origin, dims, vs, min_obs=a.min_obs), max(2, a.iters // 4), 1)
        ours = I.fuse_point_cloud(depths, K, M, voxel_size=a.voxel, colors=colors, max_depth=MAX_DEPTH, min_obs=a.min_obs,
                                  origin=origin, dims=dims)
        pos, col, cnt, uniq = torch_fuse(depths, colors, K, M, origin, dims, vs, min_obs=a.min_obs)
        # same voxels, same counts (the composition's rows are in linear voxel order: sort ours the same way)
        key = (ours.voxels[:, 2].long() * dims[1] + ours.voxels[:, 1].long()) * dims[0] + ours.voxels[:, 0].long()
        order = torch.argsort(key)
        same = bool(cnt.shape[0] == ours.counts.shape[0] and torch.equal(key[order], uniq) and torch.equal(ours.counts[order], cnt))
        out.update(torch_us=round(t_us, 1), speedup_vs_torch=round(t_us / phases["default"]["whole_us"], 2),
                   same_voxels_and_counts_as_torch=same,
                   max_point_diff_vs_torch_voxels=float((ours.points[order] - pos).abs().max() / vs) if same else None,
                   max_colour_diff_vs_torch=float((ours.colors[order] - col).abs().max()) if same else None)
        print(f"torch composition {t_us:.1f} us: x{out['speedup_vs_torch']:.2f}; same voxels and counts: {same}; largest mean-position "
              f"difference {out['max_point_diff_vs_torch_voxels']} voxel, colour {out['max_colour_diff_vs_torch']}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
