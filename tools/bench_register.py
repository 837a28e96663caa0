"""Time the point-cloud registration (csrc/register.hip, coivo_amd.evaluate.register_clouds) on one GPU with hip events around whole
calls, beside the nearest-neighbour query it is built on, and score a drifted reconstruction before and after.

    python tools/bench_register.py [--frames N] [--voxel V] [--max-dist D] [--iters K] [--warmup W] [--skip-drift] [--out PATH]

Clouds: tools/bench_cloud.py's.  Ground truth: the cloud fused at `--voxel` (2 cm) from N (512) frames of 256x320 from coivo_amd.synth
along a random trajectory, with the normals of inference.cloud_normals.  Prediction: the cloud fused from the same depths multiplied
by a smooth per-frame factor within +-2 %.  max_dist 8 cm.

Timed, alternated call by call in one process, K (10) calls after W (2): register_clouds at 1 iteration and at 20 (each call
builds the target's index and allocates its outputs, as a user's call does), and nearest_neighbors of the same clouds.  An iteration
is one walk plus the sums: the difference of the two registration times over 19 is the cost of an iteration, and the figure of
interest is that over the query's time (index build excluded: it is timed apart and subtracted).  Also recorded: the pairs used and
the cost per valid point F of the first and last evaluation.

Drift: the ground-truth depths fused at stride 2 along a trajectory that drifts away from the true one -- frame i is turned by
i / N * 1.5 degrees about a fixed axis and pushed by i / N * 6 cm -- scored by reconstruction_metrics against the ground truth with
register=None and with register=Registration(): accuracy, completeness and F-scores of both.  One JSON line, also written to --out.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fuse import H, W, MAX_DEPTH, make  # noqa: E402
from coivo_amd import _args, _lib, build, evaluate as E, inference as I  # noqa: E402


def alternate_us(fns, iters, warmup):
    """Mean and extremes in us of each call of `fns` (name -> callable), timed one call at a time with its own pair of events, the
    calls alternated round by round."""
    times = {k: [] for k in fns}
    for r in range(warmup + iters):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                times[name].append(a.elapsed_time(b) * 1e3)
    return {k: dict(mean=round(sum(v) / len(v), 1), min=round(min(v), 1), max=round(max(v), 1)) for k, v in times.items()}


def drifted(M, degrees, shift):
    """cam2world [N,4,4] float64 with frame i turned by i / N * degrees about (1, 2, 3) / sqrt(14) and pushed by i / N * shift along
    (2, -1, 1) / sqrt(6), both in the world frame."""
    N = M.shape[0]
    out = M.clone()
    ax = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64) / math.sqrt(14.0)
    d = torch.tensor([2.0, -1.0, 1.0], dtype=torch.float64) / math.sqrt(6.0)
    Wm = torch.tensor([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]], dtype=torch.float64)
    for i in range(N):
        th = math.radians(degrees) * i / N
        R = torch.eye(3, dtype=torch.float64) + math.sin(th) * Wm + (1.0 - math.cos(th)) * (Wm @ Wm)
        out[i, :3, :3] = R @ M[i, :3, :3]
        out[i, :3, 3] = R @ M[i, :3, 3] + shift * i / N * d
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--max-dist", type=float, default=0.08)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-drift", action="store_true", help="timings only")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "register_bench_line.json"))
    a = ap.parse_args()
    build.ensure()
    if not torch.cuda.is_available():
        raise SystemExit("bench_register.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    N = a.frames
    depths, _, K, M = make(N, dev)
    factor = 1.0 + 0.02 * torch.sin(2.0 * torch.pi * torch.arange(N, device=dev, dtype=torch.float32) / 64.0)
    pred_depths = (depths * factor.view(-1, 1, 1, 1)).contiguous()
    gt_fused = I.fuse_point_cloud(depths, K, M, voxel_size=a.voxel, max_depth=MAX_DEPTH)
    gt = gt_fused.points
    normals = I.cloud_normals(gt_fused, depths, K, M, stride=1, max_depth=MAX_DEPTH).normals
    pred = I.fuse_point_cloud(pred_depths, K, M, voxel_size=a.voxel, max_depth=MAX_DEPTH).points
    del pred_depths
    md, _ = _args.reach("bench_register", a.max_dist, ())
    with_normal = int(((normals != 0).any(dim=1)).sum())
    out = dict(bench="register_clouds", N=N, H=H, W=W, voxel=a.voxel, max_dist=md, n_gt=gt.shape[0], n_pred=pred.shape[0],
               n_gt_with_normal=with_normal, iters=a.iters, warmup=a.warmup, mode="sim3", metric="plane")
    print(json.dumps({k: out[k] for k in ("n_gt", "n_pred", "n_gt_with_normal", "max_dist")}), flush=True)

    lib = _lib.load()
    index = torch.empty(int(lib.colvo_cloud_workspace_bytes(0, gt.shape[0])), device=dev, dtype=torch.uint8)

    def index_build():
        _lib.check(lib.colvo_cloud_index_build(_lib.ptr(gt), gt.shape[0], md, _lib.ptr(index), _lib.stream_ptr()), "colvo_cloud_index_build")

    kw = dict(target_normals=normals, max_dist=md)
    t = alternate_us(dict(register_1=lambda: E.register_clouds(pred, gt, iterations=1, **kw),
                          register_20=lambda: E.register_clouds(pred, gt, iterations=20, **kw),
                          nearest_neighbors=lambda: E.nearest_neighbors(pred, gt, max_dist=md),
                          index_build=index_build), a.iters, a.warmup)
    out["calls_us"] = t
    per_iteration = (t["register_20"]["mean"] - t["register_1"]["mean"]) / 19.0
    query = t["nearest_neighbors"]["mean"] - t["index_build"]["mean"]
    out["iteration_us"] = round(per_iteration, 1)
    out["query_us"] = round(query, 1)
    out["iteration_over_query"] = round(per_iteration / query, 3)
    res = E.register_clouds(pred, gt, iterations=20, **kw)
    h = res.history.cpu()
    R, tr, s = res.transform()
    out["status"] = int(res.status)
    out["pairs_used"] = [int(h[0, 2]), int(h[-1, 2])]
    out["F"] = [float(h[0, 3] / h[0, 0]), float(h[-1, 3] / h[-1, 0])]
    out["scale"] = s
    out["translation"] = [float(v) for v in tr]
    print(f"register_clouds: 1 iteration {t['register_1']['mean']:.1f} us, 20 iterations {t['register_20']['mean']:.1f} us: "
          f"{per_iteration:.1f} us per iteration; nearest_neighbors {t['nearest_neighbors']['mean']:.1f} us of which index build "
          f"{t['index_build']['mean']:.1f} us: query {query:.1f} us; iteration / query = {out['iteration_over_query']}", flush=True)
    print(f"status {out['status']}, pairs used {out['pairs_used']}, F {out['F']}, scale {s:.6f}", flush=True)

    if not a.skip_drift:
        Md = M.cpu().double()
        drift = drifted(Md, 1.5, 0.06)
        pred_d = I.fuse_point_cloud(depths, K, drift.to(dev, torch.float32), voxel_size=a.voxel, stride=2, max_depth=MAX_DEPTH)
        rows = {}
        for name, policy in (("trajectory_alignment", None), ("registered", E.Registration())):
            m = E.reconstruction_metrics(pred_d, drift, depths, K, Md, voxel_size=a.voxel, max_dist=md, max_depth=MAX_DEPTH,
                                         register=policy)
            rows[name] = dict(accuracy=m.accuracy, completeness=m.completeness, chamfer=m.chamfer, precision=m.precision,
                              recall=m.recall, fscore=m.fscore, n_pred=m.n_pred, n_gt=m.n_gt)
            if m.registration is not None:
                hh = m.registration.history.cpu()
                rows[name].update(status=int(m.registration.status), pairs_used=[int(hh[0, 2]), int(hh[-1, 2])],
                                  F=[float(hh[0, 3] / hh[0, 0]), float(hh[-1, 3] / hh[-1, 0])])
            print(f"drift 1.5 degrees / 6 cm, {name}: accuracy {m.accuracy:.5f} completeness {m.completeness:.5f} F {m.fscore}", flush=True)
        out["drift"] = dict(degrees=1.5, shift=0.06, stride=2, **rows)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
