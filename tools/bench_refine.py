"""Time inference.refine_edges (csrc/refine.hip) beside the same loop written in torch ops, on one GPU, with hip events around the
whole call after a warm-up, the two alternating call by call in one process.

    python tools/bench_refine.py [--frames N] [--iters K] [--warmup W] [--out FILE] [--quick]

N frames of 256x320 of the textured tube (tests/refine_ref.py textured_tube), the N - 1 consecutive edges started from the truth
perturbed by 0.01 / 0.005 rad per axis, the defaults of inference.Refinement, max_depth 4.5.  Byte model of one evaluation of the
sums: 16 B read per pixel and edge (depth and grey of both frames) plus one row of 52 doubles written per workgroup of 1024 pixels and
read back once; the call makes iterations + 1 evaluations, and once reads the frames (12 B per pixel) and writes the grey planes (4 B).
Reported as TB/s and as a share of the 8 TB/s of HBM.  The time (`call_us`) is of the whole Python call -- the wrapper's
allocations, the upload of the edge list (a blocking host-to-device copy) and the 16 launches -- not of the kernels alone.  The
torch composition (torch_refine) is what a user would otherwise write: every operation a kernel of its own, the sums by einsum in
float64, the solve by torch.linalg.  Prints one JSON line; --out also writes it to a file.
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
HBM_BYTES_PER_S = 8e12


def _hat(w):
    z = torch.zeros_like(w[:, 0])
    return torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], 1), torch.stack([w[:, 2], z, -w[:, 0]], 1),
                        torch.stack([-w[:, 1], w[:, 0], z], 1)], 1)


def torch_rows(depths, grey, K, ei, ej, T, a, b, p):
    """Rows and residuals of every pixel of every edge, float32: (visible, J_g [E,6,HW], e_g, use_g, J_p [E,8,HW], e_p, use_p)."""
    E = ei.shape[0]
    Hh, Ww = depths.shape[2:]
    dev = depths.device
    T32, a32, b32 = T.float(), a.float().view(E, 1, 1), b.float().view(E, 1, 1)
    d = depths[ei, 0]
    Ki, Kj = K[ei], K[ej]
    k_ = lambda Kx, r, c: Kx[:, r, c].view(-1, 1, 1)
    v = torch.arange(Hh, device=dev, dtype=torch.float32).view(1, -1, 1)
    u = torch.arange(Ww, device=dev, dtype=torch.float32).view(1, 1, -1)
    cand = (d > 0) & (d < p["max_depth"])
    px = ((u - k_(Ki, 0, 2)) / k_(Ki, 0, 0)) * d
    py = ((v - k_(Ki, 1, 2)) / k_(Ki, 1, 1)) * d
    r = lambda m, n: T32[:, m, n].view(-1, 1, 1)
    P = [((r(m, 0) * px + r(m, 1) * py) + r(m, 2) * d) + r(m, 3) for m in range(3)]
    fx, fy = k_(Kj, 0, 0), k_(Kj, 1, 1)
    x = (fx * P[0]) / P[2] + k_(Kj, 0, 2)
    y = (fy * P[1]) / P[2] + k_(Kj, 1, 2)
    seen = cand & (P[2] > 1e-3) & (x >= 0) & (x <= Ww - 1) & (y >= 0) & (y <= Hh - 1)
    x0f, y0f = torch.floor(x), torch.floor(y)
    wx, wy = x - x0f, y - y0f
    x0 = torch.where(seen, x0f, torch.zeros_like(x0f)).long()
    y0 = torch.where(seen, y0f, torch.zeros_like(y0f)).long()
    x1, y1 = (x0 + 1).clamp(max=Ww - 1), (y0 + 1).clamp(max=Hh - 1)
    src_d, src_g = depths.reshape(-1, Hh * Ww)[ej], grey.reshape(-1, Hh * Ww)[ej]
    tap = lambda src, yy, xx: torch.gather(src, 1, (yy * Ww + xx).view(E, -1)).view(E, Hh, Ww)
    t00, t01, t10, t11 = (tap(src_d, yy, xx) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    c00, c01, c10, c11 = (tap(src_g, yy, xx) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    visible = seen
    for tp in (t00, t01, t10, t11):
        visible = visible & (tp > 0) & (tp < p["max_depth"])
    ax, ay = 1 - wx, 1 - wy
    s = (((t00 * ax) + (t01 * wx)) * ay) + (((t10 * ax) + (t11 * wx)) * wy)
    c = (((c00 * ax) + (c01 * wx)) * ay) + (((c10 * ax) + (c11 * wx)) * wy)
    sx, sy = ((t01 - t00) * ay) + ((t11 - t10) * wy), ((t10 - t00) * ax) + ((t11 - t01) * wx)
    gx, gy = ((c01 - c00) * ay) + ((c11 - c10) * wy), ((c10 - c00) * ax) + ((c11 - c01) * wx)
    iz = 1 / P[2]

    def grad_P(qx, qy):
        A, B = qx * fx, qy * fy
        return [A * iz, B * iz, -((((A * P[0]) + (B * P[1])) * iz) * iz)]

    cross = lambda g: [(P[1] * g[2]) - (P[2] * g[1]), (P[2] * g[0]) - (P[0] * g[2]), (P[0] * g[1]) - (P[1] * g[0])]
    den = P[2] + s
    rel = (P[2] - s) / den
    k2 = 2 / (den * den)
    G = grad_P(sx, sy)
    g_r = [-(k2 * (P[2] * G[0])), -(k2 * (P[2] * G[1])), k2 * (s - (P[2] * G[2]))]
    wg, wp = 1 / p["sigma_geo"], 1 / p["sigma_photo"]
    use_g = visible & (rel.abs() < p["gate_geo"])
    J_g = torch.stack([q * wg for q in g_r + cross(g_r)], 1).reshape(E, 6, -1)
    r_I = ((a32 * c) + b32) - grey[ei]
    h = [a32 * q for q in grad_P(gx, gy)]
    use_p = visible & (r_I.abs() < p["gate_photo"])
    J_p = torch.stack([q * wp for q in h + cross(h) + [c, torch.ones_like(c)]], 1).reshape(E, 8, -1)
    flat = lambda q: q.reshape(E, -1)
    return flat(visible), J_g, flat(rel * wg), flat(use_g), J_p, flat(r_I * wp), flat(use_p)


def torch_sums(depths, grey, K, ei, ej, T, a, b, p):
    """-> (Hm [E,8,8], g [E,8], F [E], n_visible [E]) float64."""
    visible, J_g, e_g, use_g, J_p, e_p, use_p = torch_rows(depths, grey, K, ei, ej, T, a, b, p)
    E = ei.shape[0]
    Hm = torch.zeros(E, 8, 8, device=depths.device, dtype=torch.float64)
    g = torch.zeros(E, 8, device=depths.device, dtype=torch.float64)
    Jg = torch.where(use_g[:, None], J_g, torch.zeros_like(J_g)).double()
    Jp = torch.where(use_p[:, None], J_p, torch.zeros_like(J_p)).double()
    Hm[:, :6, :6] += torch.einsum("ekp,elp->ekl", Jg, Jg)
    Hm += torch.einsum("ekp,elp->ekl", Jp, Jp)
    g[:, :6] += torch.einsum("ekp,ep->ek", Jg, torch.where(use_g, e_g, torch.zeros_like(e_g)).double())
    g += torch.einsum("ekp,ep->ek", Jp, torch.where(use_p, e_p, torch.zeros_like(e_p)).double())
    cap_g, cap_p = (p["gate_geo"] / p["sigma_geo"]) ** 2, (p["gate_photo"] / p["sigma_photo"]) ** 2
    zero = torch.zeros((), device=depths.device, dtype=torch.float64)
    C = (torch.where(visible, (e_g.double() ** 2).clamp(max=cap_g), zero).sum(1) +
         torch.where(visible, (e_p.double() ** 2).clamp(max=cap_p), zero).sum(1))
    n = visible.sum(1).double()
    return Hm, g, C / n, n


def torch_refine(depths, frames, K, ei, ej, T_init, p):
    """The loop of colvo_refine_edges in torch ops (both terms and the brightness on) -> (T [E,4,4], gain, offset, status)."""
    grey = ((frames[:, 0] + frames[:, 1]) + frames[:, 2]) * (1.0 / 3.0)
    E = ei.shape[0]
    dev = depths.device
    T = T_init.clone()
    a = torch.ones(E, device=dev, dtype=torch.float64)
    b = torch.zeros(E, device=dev, dtype=torch.float64)
    status = torch.zeros(E, device=dev, dtype=torch.int32)
    F0 = None
    eye = torch.eye(8, device=dev, dtype=torch.float64)
    for _ in range(p["iterations"]):
        Hm, g, F, n = torch_sums(depths, grey, K, ei, ej, T, a, b, p)
        F0 = F if F0 is None else F0
        Hd = Hm + p["damping"] * Hm * eye
        L, info = torch.linalg.cholesky_ex(Hd)
        few = (n < p["min_samples"]) & (status == 0)
        notpd = (info != 0) & ~few & (status == 0)
        status = torch.where(few, torch.ones_like(status), torch.where(notpd, torch.full_like(status, 2), status))
        live = status == 0
        Ls = torch.where(live.view(E, 1, 1), L, eye.expand(E, 8, 8))
        delta = -torch.cholesky_solve(g.unsqueeze(-1), Ls).squeeze(-1)
        xi = torch.zeros(E, 4, 4, device=dev, dtype=torch.float64)
        xi[:, :3, :3] = _hat(delta[:, 3:6])
        xi[:, :3, 3] = delta[:, :3]
        Tn = torch.linalg.matrix_exp(xi) @ T
        T = torch.where(live.view(E, 1, 1), Tn, T_init)
        a = torch.where(live, a + delta[:, 6], torch.ones_like(a))
        b = torch.where(live, b + delta[:, 7], torch.zeros_like(b))
    _, _, F1, _ = torch_sums(depths, grey, K, ei, ej, T, a, b, p)
    worse = (F1 > F0) & (status == 0)
    status = torch.where(worse, torch.full_like(status, 3), status)
    T = torch.where(worse.view(E, 1, 1), T_init, T)
    a = torch.where(worse, torch.ones_like(a), a)
    b = torch.where(worse, torch.zeros_like(b), b)
    return T, a, b, status


def alternate_us(fns, iters, warmup):
    """Mean microseconds of each callable, the callables taking turns call by call (the same clocks and thermal state)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    total = [0.0] * len(fns)
    for _ in range(iters):
        for n, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            total[n] += s.elapsed_time(e) * 1e3
    return [t / iters for t in total]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=64, help="edges per call of the torch composition (its intermediates are [E,8,H*W] float64)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--quick", action="store_true", help="the native call only (no torch composition): a profiler run")
    a = ap.parse_args()
    build.ensure()
    if not torch.cuda.is_available():
        raise SystemExit("bench_refine.py measures on the GPU; none found")
    import numpy as np
    from tests import refine_ref as R
    dev = torch.device("cuda:0")
    N = a.frames
    depths, frames, K, M, _, _ = R.textured_tube(N, H, W, 3)
    pairs = [(k, k + 1) for k in range(N - 1)]
    E = len(pairs)
    Tt = R.true_edges(M, pairs)
    T0 = R.perturb(Tt, 10)
    depths, frames, K = (torch.from_numpy(x).to(dev).contiguous() for x in (depths, frames, K))
    T_init = torch.from_numpy(T0).to(dev)
    policy = I.Refinement()
    p = dict(policy._asdict(), max_depth=MAX_DEPTH)
    its = policy.iterations
    strips = -(-((H + 7) // 8) * ((W + 7) // 8) // 16)
    eval_bytes = E * (16 * H * W + 2 * strips * 52 * 8)
    model_bytes = (its + 1) * eval_bytes + N * H * W * 16
    out = dict(bench="refine_edges", N=N, E=E, H=H, W=W, max_depth=MAX_DEPTH, policy=policy._asdict(), iters=a.iters, warmup=a.warmup,
               hbm_bytes_per_s=HBM_BYTES_PER_S, evaluations=its + 1, model_bytes_per_evaluation=eval_bytes,
               model_bytes_per_pixel_edge_evaluation=round(eval_bytes / (E * H * W), 2), model_bytes=model_bytes)
    ours = I.refine_edges(depths, frames, K, pairs, T_init, max_depth=MAX_DEPTH, **policy._asdict())
    t0, r0 = R.pose_error(T0, Tt)
    t1, r1 = R.pose_error(ours.T.cpu().numpy(), Tt)
    status = ours.status.cpu().numpy()
    out.update(status_counts=[int((status == s).sum()) for s in range(5)],
               translation_error=dict(start_max=float(t0.max()), end_max=float(t1.max()), end_median=float(np.median(t1))),
               rotation_error_deg=dict(start_max=float(r0.max()), end_max=float(r1.max()), end_median=float(np.median(r1))),
               n_visible_mean=float(ours.history[:, 0, 0].mean()))
    ei = torch.tensor([i for i, _ in pairs], device=dev)
    ej = torch.tensor([j for _, j in pairs], device=dev)

    def composition():
        outs = [torch_refine(depths, frames, K, ei[c:c + a.chunk], ej[c:c + a.chunk], T_init[c:c + a.chunk], p) for c in range(0, E, a.chunk)]
        return [torch.cat(q) for q in zip(*outs)]

    fns = [lambda: I.refine_edges(depths, frames, K, pairs, T_init, max_depth=MAX_DEPTH, **policy._asdict())]
    if not a.quick:
        fns.append(composition)
    us = alternate_us(fns, a.iters, a.warmup)
    out["call_us"] = round(us[0], 1)          # the whole wrapper call: allocations, edge upload, 16 launches
    out["model_tb_per_s"] = round(model_bytes / us[0] * 1e6 / 1e12, 3)
    out["share_of_hbm"] = round(model_bytes / us[0] * 1e6 / HBM_BYTES_PER_S, 4)
    out["call_us_per_evaluation"] = round(us[0] / (its + 1), 1)
    line = (f"refine_edges {us[0]:9.1f} us for {E} edges, {its + 1} evaluations: {out['model_tb_per_s']:.3f} TB/s of the byte model "
            f"({100 * out['share_of_hbm']:.1f} % of 8 TB/s)")
    if not a.quick:
        Tc, _, _, sc = composition()
        out["torch_us"] = round(us[1], 1)
        out["speedup_vs_torch"] = round(us[1] / us[0], 2)
        out["torch_status_equal"] = float((sc == ours.status).float().mean())
        out["torch_T_max_abs_diff"] = float((Tc - ours.T).abs().max())
        line += (f"  | torch composition {us[1]:9.1f} us: x{out['speedup_vs_torch']:.2f}; largest |T - T_torch| "
                 f"{out['torch_T_max_abs_diff']:.2e}, status equal on {100 * out['torch_status_equal']:.2f} % of the edges")
    print(line, flush=True)
    text = json.dumps(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    # the yardstick must do the same work: it ends where the kernel ends but for samples at a gate (torch's own kernels need not
    # round as the contract does)
    if not a.quick and (out["torch_status_equal"] < 0.99 or out["torch_T_max_abs_diff"] > 1e-3):
        raise SystemExit(f"the torch composition disagrees with refine_edges: {out}")


if __name__ == "__main__":
    main()
