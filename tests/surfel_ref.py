"""NumPy replica of the oriented-disc rendering contract (include/colvo.h colvo_render_surfels) -- test infrastructure
beside tests/render_ref.py, whose `project` (steps 1 to 5 of colvo_render_cloud's contract) it imports.  float32, one rounding per
operation in the order written, plain `/`.  What differs from render_ref.render, per frame n and point i with world normal N:

  has a normal   iff (N_0^2 + N_1^2) + N_2^2 > 0 (NaN fails); without one the point is a square with one depth (flat when in front).
  camera normal  m_a = (r_0a N_0 + r_1a N_1) + r_2a N_2, num = (m_x P_x + m_y P_y) + m_z P_z; in front, with a normal and num >= 0:
                 culled, draws nothing.
  per pixel      dx = (float(u) - cx) / fx, dy = (float(v) - cy) / fy, den = (m_x dx + m_y dy) + m_z, z = num / den,
                 e = (dx z - P_x, dy z - P_y, z - P_z); hit iff den < 0, z > 1e-3, z < max_depth, (e_x^2 + e_y^2) + e_z^2 <= radius^2.
                 A hit offers (bits(z) << 32) | i; the nearest pixel, not hit, offers (bits(P_z) << 32) | i; other pixels nothing.
  outputs        normal [N,3,H,W]: the winner's m (0 where empty or the winner has no normal); stats [N,6]: front, drawn (offered a
                 key), clipped, covered, culled, flat.

`squares=True` replaces the disc path by render_ref's squares (every normal ignored): what the bias test must fail with.
"""
import numpy as np

from tests import render_ref as R

f32 = np.float32
EMPTY = R.EMPTY


def _bits(z):
    return z.astype(f32).view(np.uint32).astype(np.uint64) << np.uint64(32)


def render(points, normals, K, M, H, W, *, radius, colors=None, max_splat=8, max_depth=10.0, squares=False):
    """-> dict(depth [N,1,H,W] f32, index [N,1,H,W] i32, colors [N,3,H,W] f32 or None, normal [N,3,H,W] f32, stats [N,6] i32)."""
    points = np.asarray(points, dtype=f32).reshape(-1, 3)
    normals = np.asarray(normals, dtype=f32).reshape(-1, 3)
    if squares:
        normals = np.zeros_like(normals)
    assert normals.shape == points.shape
    K, M = np.asarray(K, dtype=f32), np.asarray(M, dtype=f32)
    N = M.shape[0]
    if K.ndim == 2:
        K = np.broadcast_to(K, (N, 3, 3))
    depth = np.full((N, 1, H, W), np.inf, f32)
    index = np.full((N, 1, H, W), -1, np.int32)
    out_c = None if colors is None else np.zeros((N, 3, H, W), f32)
    out_n = np.zeros((N, 3, H, W), f32)
    stats = np.zeros((N, 6), np.int32)
    max_depth32 = f32(max_depth)
    with np.errstate(all="ignore"):
        r2 = f32(radius) * f32(radius)                                    # (+inf for a radius above 1.8e19)
        has = (normals[:, 0] * normals[:, 0] + normals[:, 1] * normals[:, 1]) + normals[:, 2] * normals[:, 2] > 0
    for n in range(N):
        p = R.project(points, K, M, n, H, W, radius, max_splat, max_depth)
        k, m4 = K[n], M[n]
        with np.errstate(all="ignore"):
            q = [points[:, a] - m4[a, 3] for a in range(3)]
            P = [(m4[0, a] * q[0] + m4[1, a] * q[1]) + m4[2, a] * q[2] for a in range(3)]
            assert np.array_equal(P[2].view(np.uint32), p["Pz"].view(np.uint32))
            mc = [(m4[0, a] * normals[:, 0] + m4[1, a] * normals[:, 1]) + m4[2, a] * normals[:, 2] for a in range(3)]
            num = (mc[0] * P[0] + mc[1] * P[1]) + mc[2] * P[2]
            culled = p["front"] & has & (num >= 0)
            flat = p["front"] & ~has
            xs, ys = np.where(p["on"], p["x"], f32(0)), np.where(p["on"], p["y"], f32(0))
            uc, vc = np.floor(xs + f32(0.5)).astype(np.int64), np.floor(ys + f32(0.5)).astype(np.int64)
        keys = np.full(H * W, EMPTY, np.uint64)
        rows = np.nonzero(p["drawn"] & ~culled)[0]
        drawn = np.zeros(len(points), bool)
        if rows.size:
            centre = _bits(P[2][rows]) | rows.astype(np.uint64)
            u_lo, u_hi, v_lo, v_hi = (p[key][rows] for key in ("u_lo", "u_hi", "v_lo", "v_hi"))
            hs, Px, Py, Pz, mx, my, mz, nm = (a[rows] for a in (has, P[0], P[1], P[2], mc[0], mc[1], mc[2], num))
            for dv in range(int((v_hi - v_lo).max()) + 1):
                for du in range(int((u_hi - u_lo).max()) + 1):
                    u, v = u_lo + du, v_lo + dv
                    sel = (u <= u_hi) & (v <= v_hi)
                    with np.errstate(all="ignore"):
                        dx = (u.astype(f32) - k[0, 2]) / k[0, 0]
                        dy = (v.astype(f32) - k[1, 2]) / k[1, 1]
                        den = (mx * dx + my * dy) + mz
                        z = nm / den
                        ex, ey, ez = dx * z - Px, dy * z - Py, z - Pz
                        ee = (ex * ex + ey * ey) + ez * ez
                        assert ee.dtype == f32
                        hit = hs & (den < 0) & (z > R.Z_EPS) & (z < max_depth32) & (ee <= r2)
                    offer = sel & (~hs | hit | ((u == uc[rows]) & (v == vc[rows])))
                    key = np.where(hit, _bits(np.where(hit, z, f32(1))) | rows.astype(np.uint64), centre)
                    np.minimum.at(keys, (v * W + u)[offer], key[offer])
                    drawn[rows[offer]] = True
        hitp = keys != EMPTY
        idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        safe = np.where(hitp, idx, 0)
        depth[n, 0] = np.where(hitp, (keys >> np.uint64(32)).astype(np.uint32).view(f32), f32(np.inf)).reshape(H, W)
        index[n, 0] = np.where(hitp, idx, -1).astype(np.int32).reshape(H, W)
        if len(points):
            if colors is not None:
                c = np.asarray(colors, dtype=f32).reshape(-1, 3)
                out_c[n] = np.where(hitp[None], c[safe].T, f32(0)).reshape(3, H, W)
            mcs = np.stack(mc)                                            # [3,M]
            out_n[n] = np.where((hitp & has[safe])[None], mcs[:, safe], f32(0)).reshape(3, H, W)
        stats[n] = [p["front"].sum(), drawn.sum(), p["clipped"].sum(), hitp.sum(), culled.sum(), flat.sum()]
    return dict(depth=depth, index=index, colors=out_c, normal=out_n, stats=stats)
