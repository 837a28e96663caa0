"""Time the point-cloud evaluation (csrc/cloud.hip, coivo_amd.evaluate.cloud_metrics) per phase and as a whole on one GPU, with hip
events after a warm-up, beside scipy's cKDTree on the CPU for the same distances.

    python tools/bench_cloud.py [--frames N] [--voxel V] [--max-dist D] [--iters K] [--warmup W] [--kdtree-queries Q] [--out PATH]

Ground truth: the cloud fused at `--voxel` (2 cm) from N (512) frames of 256x320 from coivo_amd.synth along a random trajectory
(tools/bench_fuse.py's input).  Prediction: the cloud fused from the same depths multiplied by a smooth per-frame factor within
+-2 % (1 + 0.02 sin(2 pi i / 64)).  max_dist 8 cm, thresholds 2 and 4 cm.  A second query set is the stitched, unfused cloud of the
predicted depths (every sample, in frame order) against the ground truth.

Reported: us by hip events for the index build, the query each way and the whole cloud_metrics call (two builds, two queries, its
allocations and the read-back); query points per second; mean reference records examined per valid query (the kernel counts them);
the measures themselves.  Baseline outside the library: cKDTree(gt).query(sample of pred, distance_upper_bound=max_dist, workers=16)
on `--kdtree-queries` predicted points, tree construction timed apart; its rate stands beside the GPU's with the subsample size, and
the largest difference between its float64 distances and ours is recorded.  One JSON line, also written to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fuse import H, W, MAX_DEPTH, make, time_us  # noqa: E402
from coivo_amd import _args, _lib, build, cloud_eval, evaluate as E, inference as I  # noqa: E402


class Search:
    """The two C calls of nearest_neighbors on buffers sized once."""

    def __init__(self, query, ref, md, th):
        import ctypes
        self.lib = lib = _lib.load()
        self.q, self.r, self.md = query, ref, md
        dev = query.device
        n, m = query.shape[0], ref.shape[0]
        self.ws = torch.empty(int(lib.colvo_cloud_workspace_bytes(n, m)), device=dev, dtype=torch.uint8)
        self.dist = torch.empty(n, device=dev, dtype=torch.float32)
        self.dist2 = torch.empty(n, device=dev, dtype=torch.float32)
        self.nearest = torch.empty(n, device=dev, dtype=torch.int32)
        self.stats = torch.empty(len(E.CLOUD_STATS), device=dev, dtype=torch.int64)
        self.tau = (ctypes.c_float * E.MAX_THRESHOLDS)(*th)
        self.tau_ptr, self.n_tau = ctypes.addressof(self.tau), len(th)

    def build(self):
        _lib.check(self.lib.colvo_cloud_index_build(_lib.ptr(self.r), self.r.shape[0], self.md, _lib.ptr(self.ws), _lib.stream_ptr()),
                   "colvo_cloud_index_build")

    def query(self):
        _lib.check(self.lib.colvo_cloud_query(_lib.ptr(self.q), self.q.shape[0], self.r.shape[0], self.md, self.tau_ptr, self.n_tau,
                                              _lib.ptr(self.ws), _lib.ptr(self.dist), _lib.ptr(self.dist2), _lib.ptr(self.nearest),
                                              _lib.ptr(self.stats), _lib.stream_ptr()), "colvo_cloud_query")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--max-dist", type=float, default=0.08)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kdtree-queries", type=int, default=200000, help="predicted points searched by cKDTree on the CPU (0: skip)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "cloud_bench_line.json"))
    a = ap.parse_args()
    build.ensure()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    N = a.frames
    depths, _, K, M = make(N, dev)
    factor = 1.0 + 0.02 * torch.sin(2.0 * torch.pi * torch.arange(N, device=dev, dtype=torch.float32) / 64.0)
    pred_depths = (depths * factor.view(-1, 1, 1, 1)).contiguous()
    gt = I.fuse_point_cloud(depths, K, M, voxel_size=a.voxel, max_depth=MAX_DEPTH).points
    pred = I.fuse_point_cloud(pred_depths, K, M, voxel_size=a.voxel, max_depth=MAX_DEPTH).points
    stitched = I.stitch_point_cloud(pred_depths, K, M, stride=1, max_depth=MAX_DEPTH)
    md, th = _args.reach("bench_cloud", a.max_dist, (a.max_dist / 4, a.max_dist / 2))
    out = dict(bench="cloud_metrics", N=N, H=H, W=W, voxel=a.voxel, max_dist=md, thresholds=list(th), n_gt=gt.shape[0],
               n_pred=pred.shape[0], n_stitched=stitched.shape[0], iters=a.iters, warmup=a.warmup, query_form="lane per query")
    print(json.dumps({k: out[k] for k in ("n_gt", "n_pred", "n_stitched", "max_dist")}), flush=True)

    def rate(us, n):
        return round(n / us * 1e6, 0)

    rows = {}
    for name, q, r in (("pred_to_gt", pred, gt), ("gt_to_pred", gt, pred), ("stitched_to_gt", stitched, gt)):
        s = Search(q, r, md, th)
        row = dict(queries=q.shape[0], refs=r.shape[0])
        row["build_us"] = round(time_us(s.build, a.iters, a.warmup), 1)
        row["query_us"] = round(time_us(s.query, a.iters, a.warmup), 1)
        st = s.stats.tolist()
        row["stats"] = dict(zip(E.CLOUD_STATS, st))
        row["examined_per_query"] = round(st[11] / max(st[0], 1), 2)
        row["query_points_per_s"] = rate(row["query_us"], q.shape[0])
        row["build_points_per_s"] = rate(row["build_us"], r.shape[0])
        row["mean_distance"] = cloud_eval.mean_truncated_distance(st, md)
        rows[name] = row
        print(f"{name:15s}: {q.shape[0]:9d} queries, {r.shape[0]:9d} refs: build {row['build_us']:9.1f} us  query {row['query_us']:10.1f} us  "
              f"| {row['query_points_per_s'] / 1e9:6.3f} G queries/s, {row['examined_per_query']:7.2f} records examined per query, "
              f"mean distance {row['mean_distance']:.5f}", flush=True)
        del s
    out["searches"] = rows
    whole = time_us(lambda: E.cloud_metrics(pred, gt, max_dist=md, thresholds=th), a.iters, a.warmup)
    m = E.cloud_metrics(pred, gt, max_dist=md, thresholds=th)
    out["cloud_metrics_us"] = round(whole, 1)
    out["cloud_metrics_points_per_s"] = rate(whole, pred.shape[0] + gt.shape[0])
    out["measures"] = {k: getattr(m, k) for k in ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore", "n_pred", "n_gt",
                                                  "n_pred_reached", "n_gt_reached")}
    print(f"cloud_metrics(pred, gt) whole call {whole:.1f} us = {out['cloud_metrics_points_per_s'] / 1e9:.3f} G points/s; "
          f"accuracy {m.accuracy:.5f} completeness {m.completeness:.5f} F {m.fscore}", flush=True)
    if a.kdtree_queries > 0:
        from scipy.spatial import cKDTree
        g = torch.Generator().manual_seed(1)
        pick = torch.randperm(pred.shape[0], generator=g)[:a.kdtree_queries].sort().values
        ref64 = gt.cpu().numpy().astype(np.float64)
        q64 = pred[pick.to(dev)].cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(ref64)
        t1 = time.perf_counter()
        d, _ = tree.query(q64, k=1, distance_upper_bound=md, workers=16)
        t2 = time.perf_counter()
        ours = m.pred_to_gt.dist[pick.to(dev)].cpu().numpy().astype(np.float64)
        diff = float(np.abs(np.minimum(d, md) - ours).max())
        out["kdtree"] = dict(queries=int(q64.shape[0]), refs=int(ref64.shape[0]), workers=16, build_s=round(t1 - t0, 3),
                             query_s=round(t2 - t1, 4), query_points_per_s=round(q64.shape[0] / (t2 - t1), 0),
                             max_abs_distance_difference=diff)
        print(f"cKDTree on the CPU: build {t1 - t0:.2f} s over {ref64.shape[0]} points; {q64.shape[0]} queries in {t2 - t1:.3f} s with 16 "
              f"workers = {out['kdtree']['query_points_per_s'] / 1e6:.2f} M queries/s; largest distance difference {diff:.2e}", flush=True)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
