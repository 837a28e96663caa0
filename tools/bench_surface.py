"""Time the point-to-surface evaluation (csrc/surface.hip, coivo_amd.evaluate.point_to_surface / surface_metrics) per phase on one GPU,
with hip events after a warm-up, and put the point-to-point and the point-to-surface measures of the same pair side by side.

    python tools/bench_surface.py [--frames N] [--voxel V] [--max-dist D] [--iters K] [--warmup W] [--out PATH]

Ground truth: the surface meshed (fuse_tsdf + extract_mesh, min_obs 2) at `--voxel` (2 cm) from N (512) frames of 256x320 from
coivo_amd.synth along a random trajectory -- the mesh of DESIGN.md 3.6m.  Prediction: the surface meshed the same way from the same
depths multiplied by a smooth per-frame factor within +-2 % (tools/bench_cloud.py's pair).  Both are cleaned with clean_mesh's
defaults, as surface_metrics does; max_dist 8 cm, thresholds 2 and 4 cm.

Reported per direction and for both record forms of the index (tuning.h surface_copy_records: the face index alone, or the face
copied into the record): us by hip events for the index plan, the fill and the query; (cell, face) pairs per face; faces examined per
valid query; the oversize count; and, for scale, nearest_neighbors' build and query for the same queries against the same mesh's
vertices.  Then the measures of surface_metrics beside those of cloud_metrics on the very same vertices: their difference is the
sampling floor of point-to-point scoring.  One JSON line, also written to --out.  No rate or ratio is promised.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_cloud import Search  # noqa: E402
from bench_fuse import H, W, MAX_DEPTH, make, time_us  # noqa: E402
from coivo_amd import _args, _lib, build, cloud_eval, evaluate as E, inference as I, surface_eval  # noqa: E402


class Index:
    """The three C calls of point_to_surface on buffers sized once (the records by a first plan's read-back), with the record form of
    the tuning entry surface_copy_records at construction."""

    def __init__(self, query, mesh, md, th):
        self.lib = lib = _lib.load()
        self.q, self.v, self.f, self.md = query, mesh.vertices, mesh.faces, md
        dev = query.device
        n, self.V, self.F = query.shape[0], mesh.vertices.shape[0], mesh.faces.shape[0]
        self.ws = torch.empty(int(lib.colvo_surface_scratch_bytes(self.V, self.F)), device=dev, dtype=torch.uint8)
        self.counts = torch.empty(8, device=dev, dtype=torch.int64)
        self.plan()
        self.pairs, _, _, _, self.record_bytes = (int(c) for c in self.counts[:5].tolist())
        self.records = torch.empty(max(self.pairs, 1) * self.record_bytes, device=dev, dtype=torch.uint8)
        self.dist2 = torch.empty(n, device=dev, dtype=torch.float64)
        self.dist = torch.empty(n, device=dev, dtype=torch.float32)
        self.face = torch.empty(n, device=dev, dtype=torch.int32)
        self.closest = torch.empty(n, 3, device=dev, dtype=torch.float32)
        self.side = torch.empty(n, device=dev, dtype=torch.int8)
        self.stats = torch.empty(len(E.SURFACE_STATS), device=dev, dtype=torch.int64)
        self.tau = (ctypes.c_float * E.MAX_THRESHOLDS)(*th)
        self.tau_ptr, self.n_tau = ctypes.addressof(self.tau), len(th)

    def plan(self):
        _lib.check(self.lib.colvo_surface_index_plan(_lib.ptr(self.v), _lib.ptr(self.f), self.V, self.F, self.md, _lib.ptr(self.ws),
                                                     _lib.ptr(self.counts), _lib.stream_ptr()), "colvo_surface_index_plan")

    def fill(self):
        _lib.check(self.lib.colvo_surface_index_fill(_lib.ptr(self.v), _lib.ptr(self.f), self.V, self.F, _lib.ptr(self.ws), self.pairs,
                                                     self.record_bytes, _lib.ptr(self.records), _lib.stream_ptr()),
                   "colvo_surface_index_fill")

    def query(self):
        _lib.check(self.lib.colvo_surface_query(_lib.ptr(self.q), self.q.shape[0], _lib.ptr(self.v), _lib.ptr(self.f), self.V, self.F,
                                                self.md, self.tau_ptr, self.n_tau, _lib.ptr(self.ws), _lib.ptr(self.records), self.pairs,
                                                self.record_bytes, _lib.ptr(self.dist2), _lib.ptr(self.dist), _lib.ptr(self.face), _lib.ptr(self.closest),
                                                _lib.ptr(self.side), _lib.ptr(self.stats), _lib.stream_ptr()), "colvo_surface_query")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--max-dist", type=float, default=0.08)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "surface_bench_line.json"))
    a = ap.parse_args()
    build.ensure()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    N = a.frames
    depths, _, K, M = make(N, dev)
    factor = 1.0 + 0.02 * torch.sin(2.0 * torch.pi * torch.arange(N, device=dev, dtype=torch.float32) / 64.0)
    pred_depths = (depths * factor.view(-1, 1, 1, 1)).contiguous()

    def surface(d):
        raw = I.extract_mesh(I.fuse_tsdf(d, K, M, voxel_size=a.voxel, max_depth=MAX_DEPTH), min_obs=2)
        return raw, surface_eval.cleaned(raw)

    gt_raw, gt = surface(depths)
    pred_raw, pred = surface(pred_depths)
    del depths, pred_depths
    md, th = _args.reach("bench_surface", a.max_dist, (a.max_dist / 4, a.max_dist / 2))
    out = dict(bench="surface_metrics", N=N, H=H, W=W, voxel=a.voxel, max_dist=md, thresholds=list(th),
               gt=dict(V=gt_raw.vertices.shape[0], F=gt_raw.faces.shape[0], V_clean=gt.vertices.shape[0], F_clean=gt.faces.shape[0]),
               pred=dict(V=pred_raw.vertices.shape[0], F=pred_raw.faces.shape[0], V_clean=pred.vertices.shape[0],
                         F_clean=pred.faces.shape[0]),
               iters=a.iters, warmup=a.warmup, query_form="lane per query")
    print(json.dumps({k: out[k] for k in ("gt", "pred", "max_dist")}), flush=True)
    rows = {}
    default_form = int(_lib.tune_get("surface_copy_records"))
    out["default_copy_records"] = default_form
    for name, q, m in (("pred_to_gt", pred.vertices, gt), ("gt_to_pred", gt.vertices, pred)):
        for copy in (0, 1):
            _lib.tune_set("surface_copy_records", copy)
            s = Index(q, m, md, th)
            _lib.tune_set("surface_copy_records", default_form)
            row = dict(queries=q.shape[0], faces=s.F, pairs=s.pairs, record_bytes=s.record_bytes)
            row["plan_us"] = round(time_us(s.plan, a.iters, a.warmup), 1)
            row["fill_us"] = round(time_us(s.fill, a.iters, a.warmup), 1)
            row["build_us"] = round(row["plan_us"] + row["fill_us"], 1)
            row["query_us"] = round(time_us(s.query, a.iters, a.warmup), 1)
            st = s.stats.tolist()
            row["stats"] = dict(zip(E.SURFACE_STATS, st))
            row["pairs_per_face"] = round(st[17] / max(s.F, 1), 3)
            row["examined_per_query"] = round(st[11] / max(st[0], 1), 2)
            row["oversize"] = st[18]
            row["mean_distance"] = cloud_eval.mean_truncated_distance(st, md)
            rows[name + ("_copied" if copy else "")] = row
            print(f"{name:11s} records of {s.record_bytes:2d} B: {q.shape[0]:8d} queries, {s.F:8d} faces, {s.pairs:8d} pairs ({row['pairs_per_face']:.3f} a "
                  f"face), {st[18]} oversize: plan {row['plan_us']:8.1f} us  fill {row['fill_us']:8.1f} us  query {row['query_us']:9.1f} us, "
                  f"{row['examined_per_query']:7.2f} faces examined per query, mean distance {row['mean_distance']:.5f}", flush=True)
            del s
        c = Search(q, m.vertices, md, th)
        row = dict(build_us=round(time_us(c.build, a.iters, a.warmup), 1), query_us=round(time_us(c.query, a.iters, a.warmup), 1))
        cst = c.stats.tolist()
        row["examined_per_query"] = round(cst[11] / max(cst[0], 1), 2)
        row["mean_distance"] = cloud_eval.mean_truncated_distance(cst, md)
        rows[name + "_vertices"] = row
        print(f"{name:11s} to the vertices (nearest_neighbors): build {row['build_us']:8.1f} us  query {row['query_us']:8.1f} us, "
              f"{row['examined_per_query']:6.2f} points per query, mean distance {row['mean_distance']:.5f}", flush=True)
        del c
    out["searches"] = rows
    keys = ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore", "n_pred", "n_gt", "n_pred_reached", "n_gt_reached")
    whole = time_us(lambda: E.surface_metrics(pred, gt, max_dist=md, thresholds=th), max(a.iters // 5, 1), 1)
    sm = E.surface_metrics(pred, gt, max_dist=md, thresholds=th)
    cm = E.cloud_metrics(pred.vertices, gt.vertices, max_dist=md, thresholds=th)
    out["surface_metrics_us"] = round(whole, 1)
    out["point_to_surface"] = dict({k: getattr(sm, k) for k in keys}, in_front=sm.in_front, behind=sm.behind)
    out["point_to_point"] = {k: getattr(cm, k) for k in keys}
    print(f"surface_metrics whole call (two cleanings, two indices, read-backs) {whole:.1f} us", flush=True)
    for name, m in (("point to point  ", cm), ("point to surface", sm)):
        print(f"{name}: accuracy {m.accuracy:.5f} completeness {m.completeness:.5f} chamfer {m.chamfer:.5f} precision {m.precision} "
              f"recall {m.recall} F {m.fscore}", flush=True)
    print(f"pred vertices in front of / behind the ground-truth surface: {sm.in_front:.4f} / {sm.behind:.4f}", flush=True)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
