"""NumPy replica of the pose refinement contract (include/colvo.h colvo_refine_*) -- test infrastructure in the
manner of tests/consistency_ref.py.  Every per-sample value is float32 with one rounding per operation, in the contract's order
(NumPy never contracts a multiply and an add); the sums are float64 sums of exact products; the 8x8 solve and the SE(3)
exponential are float64.  Also the scene the tests use: consistency_ref.tube_scene with a smooth texture painted on the wall and
a gain and an offset per frame.
"""
import math

import numpy as np

from tests import consistency_ref as CR

f32 = np.float32
Z_EPS = f32(1e-3)
THIRD = f32(1) / f32(3)
N_SUMS = 46                                  # 36 upper-triangle entries of sum J^T J (row-major), 8 of sum J^T e, C_g, C_p
OK, TOO_FEW, NOT_PD, REVERTED, BAD_EDGE = 0, 1, 2, 3, 4
DEFAULTS = dict(iterations=6, sigma_geo=0.01, sigma_photo=0.02, gate_geo=0.05, gate_photo=0.1, damping=1e-6, min_samples=256,
                geometric=True, photometric=True, brightness=True)
UPPER = [(k, l) for k in range(8) for l in range(k, 8)]


# ---- the scene --------------------------------------------------------------------------------------------------------- #
def wall_texture(theta, z):
    """Smooth brightness of the wall point at angle theta and height z, in [0.1, 0.9]; angular wavenumbers 2..4, axial 2..3."""
    return (0.5 + 0.15 * np.sin(3.0 * theta + 0.7) * np.cos(2.5 * z) + 0.15 * np.cos(2.0 * theta - 0.3 + 3.0 * z)
            + 0.1 * np.sin(4.0 * theta + 1.1 + 2.0 * z))


def textured_tube(N, H, W, seed, K=None, brightness=True):
    """consistency_ref.tube_scene and what its cameras see of wall_texture: frame n is gain_n * texture + offset_n (gain in
    0.9..1.1, offset in -0.03..0.03; 1 and 0 without `brightness`), its three channels the same value times 1.0 / 0.9 / 0.8.  A pixel
    that looks down the lumen is black.  -> (depths [N,1,H,W], frames [N,3,H,W], K [N,3,3], cam2world [N,4,4]) float32, and
    (gain, offset) float64 [N]."""
    depths, K, M = CR.tube_scene(N, H, W, seed, K=K)
    rng = np.random.default_rng(seed + 1000)
    gain = rng.uniform(0.9, 1.1, N) if brightness else np.ones(N)
    offset = rng.uniform(-0.03, 0.03, N) if brightness else np.zeros(N)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    frames = np.zeros((N, 3, H, W), f32)
    for n in range(N):
        k, m = K[n].astype(np.float64), M[n].astype(np.float64)
        ray = np.stack([(u - k[0, 2]) / k[0, 0], (v - k[1, 2]) / k[1, 1], np.ones_like(u)], -1) @ m[:3, :3].T
        z = depths[n, 0].astype(np.float64)
        ok = np.isfinite(z)
        p = m[:3, 3] + ray * np.where(ok, z, 0.0)[..., None]
        tex = wall_texture(np.arctan2(p[..., 1], p[..., 0]), p[..., 2])
        val = np.where(ok, gain[n] * tex + offset[n], 0.0)
        for c, scale in enumerate((1.0, 0.9, 0.8)):
            frames[n, c] = (scale * val).astype(f32)
    return depths, frames, K, M, gain, offset


def true_edges(M, pairs):
    """[E,4,4] float64: T = inv(M_j) M_i of the float32 cam2world, for every (i, j)."""
    M = np.asarray(M, dtype=np.float64)
    return np.stack([np.linalg.inv(M[j]) @ M[i] for i, j in pairs])


def perturb(T, seed, sigma_t=0.01, sigma_r=0.005):
    """exp(xi) T with xi ~ N(0, sigma_t) per translation axis and N(0, sigma_r) rad per rotation axis."""
    rng = np.random.default_rng(seed)
    out = np.array(T, dtype=np.float64, copy=True)
    for e in range(out.shape[0]):
        xi = np.concatenate([sigma_t * rng.standard_normal(3), sigma_r * rng.standard_normal(3)])
        out[e] = se3_exp(xi) @ out[e]
    return out


def pose_error(T, T_true):
    """(translation error, rotation error in degrees) of each edge."""
    T, T_true = np.asarray(T, np.float64), np.asarray(T_true, np.float64)
    dt = np.linalg.norm(T[:, :3, 3] - T_true[:, :3, 3], axis=1)
    D = T[:, :3, :3] @ np.swapaxes(T_true[:, :3, :3], 1, 2)
    # the angle from the skew part: the float32 cam2world is orthonormal to 1e-7 only, which an arccos of the trace turns into 0.03
    # degrees of noise and the skew part does not see to first order
    w = 0.5 * np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], 1)
    return dt, np.degrees(np.arctan2(np.linalg.norm(w, axis=1), (np.trace(D, axis1=1, axis2=2) - 1.0) / 2.0))


def integrate(M0, T):
    """cam2world of frames 0..E from frame 0's and the consecutive edges k -> k+1: M_{k+1} = M_k inv(T_k)."""
    out = [np.asarray(M0, np.float64)]
    for k in range(T.shape[0]):
        R, t = T[k, :3, :3], T[k, :3, 3]
        inv = np.eye(4)
        inv[:3, :3] = R.T
        inv[:3, 3] = -(R.T @ t)
        out.append(out[-1] @ inv)
    return np.stack(out)


def ate(M, M_true):
    """Root mean square distance of the camera centres (no alignment: both start at the same frame 0)."""
    d = np.asarray(M, np.float64)[:, :3, 3] - np.asarray(M_true, np.float64)[:, :3, 3]
    return float(np.sqrt((d * d).sum(1).mean()))


# ---- the contract ------------------------------------------------------------------------------------------------------ #
def grey(frames):
    fr = np.asarray(frames, dtype=f32)
    return ((fr[:, 0] + fr[:, 1]) + fr[:, 2]) * THIRD


def state32(T, a, b):
    """The float32 rounding of an edge state: (R row-major then t [12], a, b)."""
    T = np.asarray(T, np.float64)
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]).astype(f32), f32(a), f32(b)


def _cross(P, g):
    return [(P[1] * g[2]) - (P[2] * g[1]), (P[2] * g[0]) - (P[0] * g[2]), (P[0] * g[1]) - (P[1] * g[0])]


def _grad_P(gx, gy, fx, fy, P, iz):
    A, B = gx * fx, gy * fy
    return [A * iz, B * iz, -((((A * P[0]) + (B * P[1])) * iz) * iz)]


def sample_terms(depths, gr, K, i, j, T, a, b, *, sigma_geo, sigma_photo, gate_geo, gate_photo, max_depth):
    """Every pixel of frame i under the edge state (T [4,4] float64, a, b): dict of visible [H,W] bool, P [3], x, y, wx, wy, rel, e_g,
    J_g [8,H,W], use_g, r_I, e_p, J_p [8,H,W], use_p -- float32 (garbage where not visible)."""
    depths, K = np.asarray(depths, dtype=f32), np.asarray(K, dtype=f32)
    _, _, H, W = depths.shape
    t, a, b = state32(T, a, b)
    max_depth, gate_geo, gate_photo = f32(max_depth), f32(gate_geo), f32(gate_photo)
    inv_sg, inv_sp = f32(1) / f32(sigma_geo), f32(1) / f32(sigma_photo)
    v, u = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    with np.errstate(all="ignore"):
        d = depths[i, 0]
        cand = (d > 0) & (d < max_depth)
        px = ((u - K[i, 0, 2]) / K[i, 0, 0]) * d
        py = ((v - K[i, 1, 2]) / K[i, 1, 1]) * d
        P = [((t[3 * r] * px + t[3 * r + 1] * py) + t[3 * r + 2] * d) + t[9 + r] for r in range(3)]
        fx, fy = K[j, 0, 0], K[j, 1, 1]
        x = (fx * P[0]) / P[2] + K[j, 0, 2]
        y = (fy * P[1]) / P[2] + K[j, 1, 2]
        seen = cand & (P[2] > Z_EPS) & (x >= 0) & (x <= f32(W - 1)) & (y >= 0) & (y <= f32(H - 1))
        x0f, y0f = np.floor(x), np.floor(y)
        wx, wy = x - x0f, y - y0f
        x0 = np.where(seen, x0f, 0).astype(np.int64)
        y0 = np.where(seen, y0f, 0).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        dj, gj = depths[j, 0], gr[j]
        t00, t01, t10, t11 = dj[y0, x0], dj[y0, x1], dj[y1, x0], dj[y1, x1]
        c00, c01, c10, c11 = gj[y0, x0], gj[y0, x1], gj[y1, x0], gj[y1, x1]
        visible = seen
        for tap in (t00, t01, t10, t11):
            visible = visible & (tap > 0) & (tap < max_depth)
        ax, ay = f32(1) - wx, f32(1) - wy
        s = (((t00 * ax) + (t01 * wx)) * ay) + (((t10 * ax) + (t11 * wx)) * wy)
        c = (((c00 * ax) + (c01 * wx)) * ay) + (((c10 * ax) + (c11 * wx)) * wy)
        sx = ((t01 - t00) * ay) + ((t11 - t10) * wy)
        sy = ((t10 - t00) * ax) + ((t11 - t01) * wx)
        cx = ((c01 - c00) * ay) + ((c11 - c10) * wy)
        cy = ((c10 - c00) * ax) + ((c11 - c01) * wx)
        iz = f32(1) / P[2]
        # geometric
        den = P[2] + s
        rel = (P[2] - s) / den
        k2 = f32(2) / (den * den)
        G = _grad_P(sx, sy, fx, fy, P, iz)
        g_r = [-(k2 * (P[2] * G[0])), -(k2 * (P[2] * G[1])), k2 * (s - (P[2] * G[2]))]
        zero = np.zeros((H, W), f32)
        J_g = [q * inv_sg for q in g_r + _cross(P, g_r)] + [zero, zero]
        e_g = rel * inv_sg
        use_g = visible & (np.abs(rel) < gate_geo)
        # photometric
        r_I = ((a * c) + b) - gr[i]
        Gc = _grad_P(cx, cy, fx, fy, P, iz)
        aG = [a * q for q in Gc]
        J_p = [q * inv_sp for q in aG + _cross(P, aG) + [c, np.ones((H, W), f32)]]
        e_p = r_I * inv_sp
        use_p = visible & (np.abs(r_I) < gate_photo)
    for q in J_g + J_p + [e_g, e_p, rel, r_I]:
        assert q.dtype == f32
    return dict(visible=visible, P=P, x=x, y=y, wx=wx, wy=wy, rel=rel, e_g=e_g, J_g=np.stack(J_g), use_g=use_g, r_I=r_I, e_p=e_p,
                J_p=np.stack(J_p), use_p=use_p)


def accumulate(depths, gr, K, i, j, T, a, b, *, sigma_geo=0.01, sigma_photo=0.02, gate_geo=0.05, gate_photo=0.1, max_depth=10.0,
               geometric=True, photometric=True, **_):
    """-> (sums [46] float64, abs [46] float64: the sum of the terms' magnitudes, terms [46] int: how many are not zero, counts [3]:
    n_visible, n_geo, n_photo).  A disabled term contributes nothing: its count and its C are 0.  Every term is an exact float64
    product of two float32 values and the sums are math.fsum's, correctly rounded: whatever order an implementation adds the n
    terms of a sum in, it lands within n * 2^-53 * (sum of magnitudes) of these."""
    st = sample_terms(depths, gr, K, i, j, T, a, b, sigma_geo=sigma_geo, sigma_photo=sigma_photo, gate_geo=gate_geo,
                      gate_photo=gate_photo, max_depth=max_depth)
    vis = st["visible"]
    parts = [[] for _ in range(N_SUMS)]
    counts = [int(vis.sum()), 0, 0]
    inv = (f32(1) / f32(sigma_geo), f32(1) / f32(sigma_photo))
    for w, (on, J, e, use, gate) in enumerate(((geometric, st["J_g"], st["e_g"], st["use_g"], gate_geo),
                                               (photometric, st["J_p"], st["e_p"], st["use_p"], gate_photo))):
        if not on:
            continue
        counts[1 + w] = int(use.sum())
        Ju, eu = J[:, use].astype(np.float64), e[use].astype(np.float64)
        for n, (k, l) in enumerate(UPPER):
            parts[n].append(Ju[k] * Ju[l])
        for k in range(8):
            parts[36 + k].append(Ju[k] * eu)
        cap = np.float64(f32(gate) * inv[w]) ** 2
        ev = e[vis].astype(np.float64)
        parts[44 + w].append(np.fmin(ev * ev, cap))
    sums, mags, terms = np.zeros(N_SUMS), np.zeros(N_SUMS), np.zeros(N_SUMS, np.int64)
    for n, ps in enumerate(parts):
        if ps:
            allp = np.concatenate(ps)
            sums[n], mags[n], terms[n] = math.fsum(allp), math.fsum(np.abs(allp)), int(np.count_nonzero(allp))
    return sums, mags, terms, np.array(counts, np.int64)


def cholesky_solve(Hm, g):
    """x with Hm x = -g by Cholesky, in the kernel's order of operations; None at a pivot that is not positive."""
    n = len(g)
    L = np.zeros((n, n))
    for k in range(n):
        s = Hm[k, k]
        for m in range(k):
            s -= L[k, m] * L[k, m]
        if not s > 0.0:
            return None
        L[k, k] = np.sqrt(s)
        for r in range(k + 1, n):
            q = Hm[k, r]
            for m in range(k):
                q -= L[r, m] * L[k, m]
            L[r, k] = q / L[k, k]
    y = np.zeros(n)
    for k in range(n):
        q = -g[k]
        for m in range(k):
            q -= L[k, m] * y[m]
        y[k] = q / L[k, k]
    x = np.zeros(n)
    for k in range(n - 1, -1, -1):
        q = y[k]
        for m in range(k + 1, n):
            q -= L[m, k] * x[m]
        x[k] = q / L[k, k]
    return x


def normal_matrix(sums, n):
    Hm = np.zeros((8, 8))
    for idx, (k, l) in enumerate(UPPER):
        Hm[k, l] = Hm[l, k] = sums[idx]
    return Hm[:n, :n]


def solve(sums, n, damping):
    Hm = normal_matrix(sums, n).copy()
    for k in range(n):
        Hm[k, k] = Hm[k, k] + damping * Hm[k, k]
    return cholesky_solve(Hm, sums[36:36 + n])


def se3_exp(xi):
    """Closed-form exponential of xi = (upsilon, omega) -> [4,4]; series below |omega|^2 = 1e-8."""
    ups, om = np.asarray(xi[:3], np.float64), np.asarray(xi[3:6], np.float64)
    th2 = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]
    if th2 < 1e-8:
        A, B, C = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        th = np.sqrt(th2)
        A, B, C = np.sin(th) / th, (1.0 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    Wm = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    W2 = Wm @ Wm
    out = np.eye(4)
    out[:3, :3] = np.eye(3) + A * Wm + B * W2
    out[:3, 3] = (np.eye(3) + B * Wm + C * W2) @ ups
    return out


def n_unknowns(photometric, brightness):
    return 8 if (photometric and brightness) else 6


def refine_edges(depths, frames, K, edges, T_init, *, iterations=6, sigma_geo=0.01, sigma_photo=0.02, gate_geo=0.05, gate_photo=0.1,
                 damping=1e-6, min_samples=256, geometric=True, photometric=True, brightness=True, max_depth=10.0):
    """The whole loop -> dict(T [E,4,4], gain [E], offset [E], history [E, iterations+1, 5], status [E] int32)."""
    gr = grey(frames)
    kw = dict(sigma_geo=sigma_geo, sigma_photo=sigma_photo, gate_geo=gate_geo, gate_photo=gate_photo, max_depth=max_depth,
              geometric=geometric, photometric=photometric)
    E = len(edges)
    n = n_unknowns(photometric, brightness)
    T_out = np.array(T_init, dtype=np.float64, copy=True)
    gain, offset = np.ones(E), np.zeros(E)
    history = np.zeros((E, iterations + 1, 5))
    status = np.zeros(E, np.int32)

    def record(e, it, sums, counts):
        history[e, it] = [counts[0], counts[1], sums[44], counts[2], sums[45]]

    for e, (i, j) in enumerate(edges):
        T, a, b = T_out[e].copy(), 1.0, 0.0
        for it in range(iterations):
            sums, _, _, counts = accumulate(depths, gr, K, i, j, T, a, b, **kw)
            record(e, it, sums, counts)
            if status[e] != OK:
                continue
            delta = None
            if counts[0] < min_samples:
                status[e] = TOO_FEW
            else:
                delta = solve(sums, n, damping)
                if delta is None:
                    status[e] = NOT_PD
            if delta is None:
                T, a, b = np.array(T_init[e], np.float64), 1.0, 0.0
                continue
            T = se3_exp(delta[:6]) @ T
            T[3] = [0.0, 0.0, 0.0, 1.0]
            if n == 8:
                a, b = a + delta[6], b + delta[7]
        sums, _, _, counts = accumulate(depths, gr, K, i, j, T, a, b, **kw)
        record(e, iterations, sums, counts)
        if status[e] == OK:
            h0, h1 = history[e, 0], history[e, iterations]
            with np.errstate(all="ignore"):
                if (h1[2] + h1[4]) / h1[0] > (h0[2] + h0[4]) / h0[0]:
                    status[e] = REVERTED
                    T, a, b = np.array(T_init[e], np.float64), 1.0, 0.0
        T_out[e], gain[e], offset[e] = T, a, b
    return dict(T=T_out, gain=gain, offset=offset, history=history, status=status)


# ---- starts that end in every status (tests/test_refine_cpu.py pins the replica's answers, tests/test_refine_gpu.py the kernel's) -- #
# 3 frames of 17x23, edges (0,1), (1,2), (0,2), truth perturbed by 0.2 / 0.1 rad per axis with the seed that is the key
STATUS_CASES = {102: [REVERTED, TOO_FEW, OK], 104: [OK, NOT_PD, TOO_FEW]}
STATUS_KW = dict(iterations=3, photometric=False, min_samples=16, max_depth=4.5)
STATUS_EDGES = [(0, 1), (1, 2), (0, 2)]


def status_case(seed):
    depths, frames, K, M, _, _ = textured_tube(3, 17, 23, 3)
    return depths, frames, K, perturb(true_edges(M, STATUS_EDGES), seed, sigma_t=0.2, sigma_r=0.1)
