"""Time localize.localize_polyps (csrc/localize.hip) per pass and as a whole, beside the torch composition a user would otherwise
write (pinned point in torch ops, one float64 index_add_ / scatter_reduce_ per field over label + L * frame keys, then the means),
on one GPU, with hip events after a warm-up.

    python tools/bench_localize.py [--frames N] [--polyps P] [--radius R] [--iters K] [--warmup W] [--quick]

N frames of 256x320 from coivo_amd.synth along a random trajectory (steps of 0.05 in translation, 0.03 rad in rotation), P spheres
implanted in front of every camera (a sphere keeps its place in the camera frame up to a seeded jitter per frame, so every frame
shows all of them: the densest case for the pass), stride 1, max_depth 4.5.  Prints us for the first accumulate, the bounds, the
clipped accumulate, the finish and the whole call with and without clip; the share of labelled pixels and of 32-byte depth sectors
that hold one; the rate on the byte model 1 B x pixels + 32 B x (depth sectors holding a labelled pixel); the same for the torch
composition; then one JSON line with the same figures.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coivo_amd import _lib, build, inference as I, localize as Z, synth  # noqa: E402

H, W = 256, 320
MAX_DEPTH = 4.5


def make(N, P, radius, dev, seed=5, chunk=64):
    """depths [N,1,H,W], labels [N,1,H,W] uint8, K [N,3,3], cam2world [N,4,4] on `dev`."""
    depths, Ks = [], []
    for i in range(0, N, chunk):
        b = synth.make_batch(min(chunk, N - i), H, W, seed=seed + i)
        depths.append(b["gt_depth"].to(dev))
        Ks.append(b["K"].to(dev))
    g = torch.Generator().manual_seed(seed)
    rel = torch.cat([0.05 * torch.randn(N, 3, generator=g), 0.03 * torch.randn(N, 3, generator=g)], dim=1)
    M = I.integrate_trajectory(rel)[1:].to(dev, torch.float32).contiguous()
    depths, K = torch.cat(depths).contiguous(), torch.cat(Ks).contiguous()
    labels = torch.zeros(N, 1, H, W, dtype=torch.uint8, device=dev)
    # sphere centres in the camera frame: a P-point ring at z = 0.4 (the synthetic depth is at least 0.5), jittered per frame
    ang = torch.arange(P, dtype=torch.float64) * (2 * torch.pi / P)
    base = torch.stack([0.17 * torch.cos(ang), 0.11 * torch.sin(ang), torch.full_like(ang, 0.4)], 1)
    centres = (base[None] + 0.01 * torch.randn(N, P, 3, generator=g, dtype=torch.float64)).to(dev)
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    Kd = K.double()
    ray = torch.stack([(u[None] - Kd[:, 0, 2, None, None]) / Kd[:, 0, 0, None, None],
                       (v[None] - Kd[:, 1, 2, None, None]) / Kd[:, 1, 1, None, None], torch.ones(N, H, W, device=dev, dtype=torch.float64)], -1)
    a = (ray * ray).sum(-1)
    for p in range(P):
        c = centres[:, p, None, None, :]
        b = -(ray * c).sum(-1)
        disc = b * b - a * ((c * c).sum(-1) - radius * radius)
        s = (-b - torch.sqrt(disc)) / a
        hit = (disc > 0) & (s > 0) & (s < depths[:, 0])
        depths[:, 0][hit] = s[hit].float()
        labels[:, 0][hit] = p + 1
    return depths, labels, K, M


def torch_localize(depths, labels, K, M, L, max_depth=MAX_DEPTH):
    """The composition: per (frame, label) count, samples, pixel sums, point sums and products (float64 index_add_), the bounding box
    (scatter_reduce_), then means, covariances, world centres and the per-polyp weighted means.  No clip."""
    N = depths.shape[0]
    dev = depths.device
    lab = labels[:, 0].long()
    labelled = (lab >= 1) & (lab <= L)
    n_idx, v_idx, u_idx = labelled.nonzero(as_tuple=True)
    key = lab[labelled] - 1 + L * n_idx
    d = depths[:, 0][labelled]
    sample = (d > 0) & (d < max_depth)
    uf, vf = u_idx.float(), v_idx.float()
    px = (uf - K[n_idx, 0, 2]) / K[n_idx, 0, 0] * d
    py = (vf - K[n_idx, 1, 2]) / K[n_idx, 1, 1] * d
    p = torch.stack([px, py, d], 1).double()
    ks = key[sample]
    ps = p[sample]
    z = lambda *s: torch.zeros(N * L, *s, device=dev, dtype=torch.float64)
    n_pix = z().index_add_(0, key, torch.ones_like(key, dtype=torch.float64))
    n = z().index_add_(0, ks, torch.ones_like(ks, dtype=torch.float64))
    su = z().index_add_(0, ks, u_idx[sample].double())
    sv = z().index_add_(0, ks, v_idx[sample].double())
    sp = [z().index_add_(0, ks, ps[:, a]) for a in range(3)]
    spp = [z().index_add_(0, ks, ps[:, a] * ps[:, b]) for a in range(3) for b in range(a, 3)]
    box = [torch.full((N * L,), W + H, device=dev, dtype=torch.long).scatter_reduce_(0, key, c, "amin") for c in (u_idx, v_idx)] + \
          [torch.full((N * L,), -1, device=dev, dtype=torch.long).scatter_reduce_(0, key, c, "amax") for c in (u_idx, v_idx)]
    m = torch.stack(sp, 1) / n[:, None]
    pairs = [(a, b) for a in range(3) for b in range(a, 3)]
    cov = torch.stack([spp[e] / n - m[:, a] * m[:, b] for e, (a, b) in enumerate(pairs)], 1)
    Md = M.double().repeat_interleave(L, dim=0)
    cw = torch.einsum("nab,nb->na", Md[:, :3, :3], m) + Md[:, :3, 3]
    C = torch.zeros(N * L, 3, 3, device=dev, dtype=torch.float64)
    for e, (a, b) in enumerate(pairs):
        C[:, a, b] = C[:, b, a] = cov[:, e]
    S = Md[:, :3, :3] @ C @ Md[:, :3, :3].transpose(1, 2) + cw[:, :, None] * cw[:, None, :]
    seen = n > 0
    wgt = torch.where(seen, n, torch.zeros_like(n)).view(N, L)
    tot = wgt.sum(0)
    pos = (torch.nan_to_num(cw).view(N, L, 3) * wgt[..., None]).sum(0) / tot[:, None]
    covw = (torch.nan_to_num(S).view(N, L, 3, 3) * wgt[..., None, None]).sum(0) / tot[:, None, None] - pos[:, :, None] * pos[:, None, :]
    return n_pix.view(N, L), n.view(N, L), torch.stack(box, 1), torch.stack([su / n, sv / n], 1), m, cov, cw, pos, covw


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


class Passes:
    """The C calls of localize_polyps on buffers sized once."""

    def __init__(self, depths, labels, K, M, L, clip_sigma):
        self.lib = lib = _lib.load()
        N = depths.shape[0]
        dev = depths.device
        self.t = (depths, labels, K, M)
        self.N, self.L, self.clip = N, L, clip_sigma
        self.records = torch.empty(int(lib.colvo_localize_workspace_bytes(N, L)), device=dev, dtype=torch.uint8)
        self.bounds_t = torch.empty(N, L, 2, device=dev, dtype=torch.float64)
        i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
        f64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float64)
        self.out = (i32(N, L), i32(N, L), i32(N, L, 4), f64(N, L, 2), f64(N, L, 3), f64(N, L, 6), f64(N, L, 3), i32(L),
                    torch.empty(L, device=dev, dtype=torch.int64), i32(L), i32(L), f64(L, 3), f64(L, 6),
                    torch.empty(2, device=dev, dtype=torch.int64))

    def accumulate(self, clipped=False):
        d, lab, K, M = self.t
        _lib.check(self.lib.colvo_localize_accumulate(_lib.ptr(d), _lib.ptr(lab), _lib.ptr(K), self.N, H, W, 1, MAX_DEPTH, self.L,
                                                      _lib.ptr(self.bounds_t) if clipped else 0, _lib.ptr(self.records),
                                                      _lib.stream_ptr()), "colvo_localize_accumulate")

    def bounds(self):
        _lib.check(self.lib.colvo_localize_bounds(_lib.ptr(self.records), self.N, self.L, self.clip, _lib.ptr(self.bounds_t),
                                                  _lib.stream_ptr()), "colvo_localize_bounds")

    def finish(self):
        _lib.check(self.lib.colvo_localize_finish(_lib.ptr(self.records), _lib.ptr(self.t[3]), self.N, self.L, 1,
                                                  *(_lib.ptr(t) for t in self.out), _lib.stream_ptr()), "colvo_localize_finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--polyps", type=int, default=8)
    ap.add_argument("--radius", type=float, default=0.03)
    ap.add_argument("--clip-sigma", type=float, default=1.5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="native calls only (no torch composition): a profiler run")
    a = ap.parse_args()
    build.ensure()
    if not torch.cuda.is_available():
        raise SystemExit("bench_localize.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    N, L = a.frames, a.polyps
    depths, labels, K, M = make(N, L, a.radius, dev)
    pixels = N * H * W
    labelled = labels != 0
    n_labelled = int(labelled.sum())
    sectors = int(labelled.view(N, H * W // 8, 8).any(-1).sum())
    model_bytes = pixels + 32 * sectors
    out = dict(bench="localize_polyps", N=N, H=H, W=W, stride=1, polyps=L, radius=a.radius, clip_sigma=a.clip_sigma, iters=a.iters,
               warmup=a.warmup, pixels=pixels, labelled_share=round(n_labelled / pixels, 5),
               depth_sector_share=round(sectors / (pixels // 8), 5), model_bytes=model_bytes)
    print(json.dumps(out), flush=True)
    ps = Passes(depths, labels, K, M, L, a.clip_sigma)
    ps.accumulate()
    ps.bounds()
    t = dict(accumulate_us=time_us(ps.accumulate, a.iters, a.warmup), bounds_us=time_us(ps.bounds, a.iters, a.warmup),
             accumulate_clipped_us=time_us(lambda: ps.accumulate(True), a.iters, a.warmup), finish_us=time_us(ps.finish, a.iters, a.warmup))
    kw = dict(num_labels=L, max_depth=MAX_DEPTH)
    t["whole_us"] = time_us(lambda: Z.localize_polyps(depths, labels, K, M, **kw), a.iters, a.warmup)
    t["whole_clipped_us"] = time_us(lambda: Z.localize_polyps(depths, labels, K, M, clip_sigma=a.clip_sigma, **kw), a.iters, a.warmup)
    out.update({k: round(v, 1) for k, v in t.items()})
    out["accumulate_model_tb_per_s"] = round(model_bytes / t["accumulate_us"] * 1e6 / 1e12, 3)
    out["accumulate_clipped_model_tb_per_s"] = round(model_bytes / t["accumulate_clipped_us"] * 1e6 / 1e12, 3)
    print(f"accumulate {t['accumulate_us']:.1f} us ({out['accumulate_model_tb_per_s']:.2f} TB/s on the byte model)  bounds {t['bounds_us']:.1f} us  "
          f"clipped accumulate {t['accumulate_clipped_us']:.1f} us ({out['accumulate_clipped_model_tb_per_s']:.2f} TB/s)  finish {t['finish_us']:.1f} us  | "
          f"whole call {t['whole_us']:.1f} us, with clip {t['whole_clipped_us']:.1f} us; labelled {out['labelled_share']:.2%} of the pixels, "
          f"{out['depth_sector_share']:.2%} of the depth sectors", flush=True)
    if not a.quick:
        t_us = time_us(lambda: torch_localize(depths, labels, K, M, L), max(2, a.iters // 2), 1)
        ours = Z.localize_polyps(depths, labels, K, M, **kw)
        ref = torch_localize(depths, labels, K, M, L)
        same_counts = bool(torch.equal(ours.n_pixels.double(), ref[0]) and torch.equal(ours.n_samples.double(), ref[1]) and
                           torch.equal(ours.bbox.long()[ours.n_pixels > 0], ref[2][ours.n_pixels.view(-1) > 0].view(-1, 4)))
        out.update(torch_us=round(t_us, 1), torch_model_tb_per_s=round(model_bytes / t_us * 1e6 / 1e12, 4),
                   speedup_vs_torch=round(t_us / t["whole_us"], 2), speedup_clipped_vs_torch=round(t_us / t["whole_clipped_us"], 2),
                   same_counts_and_boxes_as_torch=same_counts,
                   max_center_diff_vs_torch=float((ours.center_cam.view(-1, 3) - ref[4]).abs().nan_to_num().max()),
                   max_position_diff_vs_torch=float((ours.position - ref[7]).abs().nan_to_num().max()))
        print(f"torch composition (no clip) {t_us:.1f} us ({out['torch_model_tb_per_s']:.3f} TB/s on the byte model): this call x{out['speedup_vs_torch']:.2f}, "
              f"with clip x{out['speedup_clipped_vs_torch']:.2f}; same counts and boxes: {same_counts}; largest centre difference "
              f"{out['max_center_diff_vs_torch']:.2e}, position {out['max_position_diff_vs_torch']:.2e}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
