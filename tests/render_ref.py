"""NumPy replica of the cloud rendering contract (include/colvo.h colvo_render_cloud) -- test infrastructure in
the manner of tests/consistency_ref.py.  The contract, restated:

  inputs      points [M,3] float32 in the world frame, colors [M,3] float32 or None, K [N,3,3], cam2world [N,4,4] float32 (rotation
              block r taken as orthonormal, t its translation), H, W, radius (finite, >= 0), max_splat (0..32), max_depth.
  arithmetic  float32, one rounding per operation in the order written (NumPy never contracts a multiply and an add), plain `/`.
  per frame n and point i (X):
    camera      q_a = X_a - t_a,  P_a = (r_0a * q_0 + r_1a * q_1) + r_2a * q_2.
    front       iff P_z > 1e-3f and P_z < max_depth (NaN falls out).
    centre      x = (fx * P_x) / P_z + cx, y likewise;  hx = (fx * radius) / P_z, hy = (fy * radius) / P_z;  clipped iff
                hx > max_splat or hy > max_splat, then hx = hx > max_splat ? max_splat : hx, the same for hy.
    on screen   iff x >= -(max_splat + 1), x <= float32(W + max_splat), and the same in y with H.
    footprint   uc = floor(x + 0.5f), u_lo = max(int(min(ceil(x - hx), uc)), 0), u_hi = min(int(max(floor(x + hx), uc)), W - 1),
                the same in v;  drawn iff front, on screen, u_lo <= u_hi and v_lo <= v_hi.
    key         (uint64(bits(P_z)) << 32) | uint32(i); every pixel of the footprint takes the minimum key.
  outputs     depth [N,1,H,W] float32 (+inf where empty), index [N,1,H,W] int32 (-1 where empty), colors [N,3,H,W] float32
              (colors[index], 0 where empty; only with colours), stats [N,4] int32: front, drawn, front and clipped, covered pixels.

`dtype=np.float64` evaluates the same expressions in float64 (the CPU tests compare the pixel rectangles of the two).  The GPU
tests demand equality with the float32 evaluation to the bit.
"""
import numpy as np

f32 = np.float32
Z_EPS = f32(1e-3)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def project(points, K, M, n, H, W, radius, max_splat, max_depth, dtype=f32):
    """Steps 1 to 5 of the contract for frame n and every point: dict of Pz, x, y, hx, hy (hx, hy before the clip), front, clipped,
    on, drawn (bool) and u_lo, u_hi, v_lo, v_hi (int64; 0 where the point is not on screen)."""
    ft = dtype
    X = np.asarray(points, dtype=f32).astype(ft).reshape(-1, 3)
    k, m = np.asarray(K, dtype=f32)[n].astype(ft), np.asarray(M, dtype=f32)[n].astype(ft)
    radius, max_depth, ms = ft(f32(radius)), ft(f32(max_depth)), ft(max_splat)
    with np.errstate(all="ignore"):
        q = [X[:, a] - m[a, 3] for a in range(3)]
        P = [(m[0, a] * q[0] + m[1, a] * q[1]) + m[2, a] * q[2] for a in range(3)]
        front = (P[2] > ft(Z_EPS)) & (P[2] < max_depth)
        x = (k[0, 0] * P[0]) / P[2] + k[0, 2]
        y = (k[1, 1] * P[1]) / P[2] + k[1, 2]
        hx0 = (k[0, 0] * radius) / P[2]
        hy0 = (k[1, 1] * radius) / P[2]
        assert x.dtype == ft and hx0.dtype == ft
        clipped = front & ((hx0 > ms) | (hy0 > ms))
        hx, hy = np.where(hx0 > ms, ms, hx0), np.where(hy0 > ms, ms, hy0)
        lo = -(ms + ft(1))
        on = front & (x >= lo) & (x <= ft(f32(W + max_splat))) & (y >= lo) & (y <= ft(f32(H + max_splat)))
        zero = ft(0)
        xs, ys, hxs, hys = np.where(on, x, zero), np.where(on, y, zero), np.where(on, hx, zero), np.where(on, hy, zero)
        ucf, vcf = np.floor(xs + ft(0.5)), np.floor(ys + ft(0.5))
        u_lo = np.maximum(np.minimum(np.ceil(xs - hxs), ucf).astype(np.int64), 0)
        u_hi = np.minimum(np.maximum(np.floor(xs + hxs), ucf).astype(np.int64), W - 1)
        v_lo = np.maximum(np.minimum(np.ceil(ys - hys), vcf).astype(np.int64), 0)
        v_hi = np.minimum(np.maximum(np.floor(ys + hys), vcf).astype(np.int64), H - 1)
    drawn = on & (u_lo <= u_hi) & (v_lo <= v_hi)
    return dict(Pz=P[2], x=x, y=y, hx=hx, hy=hy, front=front, clipped=clipped, on=on, drawn=drawn, u_lo=u_lo, u_hi=u_hi, v_lo=v_lo,
                v_hi=v_hi)


def render(points, K, M, H, W, *, radius, colors=None, max_splat=8, max_depth=10.0):
    """-> dict(depth [N,1,H,W] f32, index [N,1,H,W] i32, colors [N,3,H,W] f32 or None, stats [N,4] i32)."""
    points = np.asarray(points, dtype=f32).reshape(-1, 3)
    K, M = np.asarray(K, dtype=f32), np.asarray(M, dtype=f32)
    N = M.shape[0]
    if K.ndim == 2:
        K = np.broadcast_to(K, (N, 3, 3))
    depth = np.full((N, 1, H, W), np.inf, f32)
    index = np.full((N, 1, H, W), -1, np.int32)
    out_c = None if colors is None else np.zeros((N, 3, H, W), f32)
    stats = np.zeros((N, 4), np.int32)
    for n in range(N):
        p = project(points, K, M, n, H, W, radius, max_splat, max_depth)
        keys = np.full(H * W, EMPTY, np.uint64)
        rows = np.nonzero(p["drawn"])[0]
        if rows.size:
            key = (p["Pz"][rows].astype(f32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
            u_lo, u_hi, v_lo, v_hi = (p[k][rows] for k in ("u_lo", "u_hi", "v_lo", "v_hi"))
            for dv in range(int((v_hi - v_lo).max()) + 1):
                for du in range(int((u_hi - u_lo).max()) + 1):
                    u, v = u_lo + du, v_lo + dv
                    sel = (u <= u_hi) & (v <= v_hi)
                    np.minimum.at(keys, (v * W + u)[sel], key[sel])
        hit = keys != EMPTY
        idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        depth[n, 0] = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(f32), f32(np.inf)).reshape(H, W)
        index[n, 0] = np.where(hit, idx, -1).astype(np.int32).reshape(H, W)
        if colors is not None:
            c = np.asarray(colors, dtype=f32).reshape(-1, 3)
            safe = np.where(hit, idx, 0)
            out_c[n] = np.where(hit[None], c[safe].T if c.shape[0] else np.zeros((3, H * W), f32), f32(0)).reshape(3, H, W)
        stats[n] = [p["front"].sum(), p["drawn"].sum(), p["clipped"].sum(), hit.sum()]
    return dict(depth=depth, index=index, colors=out_c, stats=stats)


def tube_points(N, H, W, seed, max_depth=None):
    """The tube scene of tests/consistency_ref.py as a cloud: every frame's samples (finite depth; below max_depth if given) as
    float32 world points, computed in float64 and rounded once.  -> (points [M,3] f32, depths, K, cam2world)."""
    from tests import consistency_ref as C
    d, K, M = C.tube_scene(N, H, W, seed)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = []
    for n in range(N):
        k, m, z = K[n].astype(np.float64), M[n].astype(np.float64), d[n, 0].astype(np.float64)
        keep = np.isfinite(z) if max_depth is None else (z < float(max_depth))
        cam = np.stack([(u - k[0, 2]) / k[0, 0] * z, (v - k[1, 2]) / k[1, 1] * z, z], -1)[keep]
        out.append((cam @ m[:3, :3].T + m[:3, 3]).astype(f32))
    return np.concatenate(out), d, K, M
