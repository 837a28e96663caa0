"""NumPy replica of the registration contract (include/colvo.h colvo_register_*) -- test infrastructure in the manner
of tests/refine_ref.py.  Every per-sample value is float32 with one rounding per operation, in the contract's order (NumPy never
contracts a multiply and an add); the transform and the nearest neighbour are tests/cloud_ref.py's, brute force and gridless; the
sums are float64 sums of exact products; the 6x6 / 7x7 solve and the update are float64.  Also the scenes the tests use: an analytic
corrugated, bent tube, and the starts that end in every status.
"""
import functools
import math

import numpy as np

from tests import cloud_ref as CR
from tests import refine_ref as RR

f32 = np.float32
N_SUMS = 37                                  # 28 upper-triangle entries of sum J^T J (row-major), 7 of sum J^T r, C, sum r^2
OK, TOO_FEW, NOT_PD, REVERTED = 0, 1, 2, 3
UPPER = [(k, l) for k in range(7) for l in range(k, 7)]
IDENTITY = (np.eye(3), np.zeros(3), 1.0)


# ---- the scene --------------------------------------------------------------------------------------------------------- #
def surface(theta, z):
    """S(theta, z) of the corrugated, bent tube, float64 [..., 3]."""
    r = 1.0 + 0.08 * np.sin(6.0 * z) + 0.05 * np.cos(3.0 * theta + z)
    return np.stack([0.3 * np.sin(0.8 * z) + r * np.cos(theta), 0.2 * np.cos(0.5 * z) + r * np.sin(theta), z], -1)


def surface_normals(theta, z, h=1e-5):
    """The normalised cross product of central differences, turned towards the centreline."""
    n = np.cross((surface(theta + h, z) - surface(theta - h, z)) / (2 * h), (surface(theta, z + h) - surface(theta, z - h)) / (2 * h))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    centre = np.stack([0.3 * np.sin(0.8 * z), 0.2 * np.cos(0.5 * z), z], -1)
    flip = ((centre - surface(theta, z)) * n).sum(-1) < 0
    n[flip] = -n[flip]
    return n


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Wm = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * Wm + (1.0 - np.cos(angle)) * (Wm @ Wm)


def moved(points, R, t, s):
    """The points whose image under x' = s R x + t is `points` (float64)."""
    return ((np.asarray(points, np.float64) - t) / s) @ R          # row-wise R^T (p - t) / s


@functools.lru_cache(maxsize=None)
def tube(small=False, s_true=1.03, seed=5):
    """Target: a grid over theta in [0, 2 pi), z in [0, 3) (126 x 60; small: 64 x 30), rounded to float32, with its normals.  Source:
    a grid over z in [0.2, 2.8) (119 x 57; small: 57 x 27), offset by 0.37 of a step with Gaussian jitter of 0.2 of a step, moved by
    the inverse of a known Sim(3): 2 degrees about a seeded axis, t = (0.03, -0.02, 0.04), s = s_true.  `truth` holds the source
    points where they belong, float64.  max_dist 0.2 (small: 0.3)."""
    nt, nz, mt, mz, md = (64, 30, 57, 27, 0.3) if small else (126, 60, 119, 57, 0.2)
    rng = np.random.default_rng(seed)
    th, z = np.meshgrid(2 * np.pi * np.arange(nt) / nt, 3.0 * np.arange(nz) / nz, indexing="ij")
    target = surface(th.ravel(), z.ravel()).astype(f32)
    normals = surface_normals(th.ravel(), z.ravel()).astype(f32)
    i, j = np.meshgrid(np.arange(mt, dtype=np.float64), np.arange(mz, dtype=np.float64), indexing="ij")
    th = 2 * np.pi * (i + 0.37 + 0.2 * rng.standard_normal(i.shape)) / mt
    z = 0.2 + 2.6 * (j + 0.37 + 0.2 * rng.standard_normal(j.shape)) / mz
    truth = surface(th.ravel(), z.ravel())
    R = rodrigues(rng.standard_normal(3), np.radians(2.0))
    t = np.array([0.03, -0.02, 0.04])
    source = moved(truth, R, t, s_true).astype(f32)
    for a in (target, normals, source, truth):
        a.setflags(write=False)
    return dict(target=target, normals=normals, source=source, truth=truth, R=R, t=t, s=s_true, max_dist=md)


def true_error(source, truth, R, t, s):
    """Distance of every source point under x' = s R x + t from where it belongs, float64."""
    x = float(s) * (np.asarray(source, np.float64) @ np.asarray(R, np.float64).T) + np.asarray(t, np.float64)
    return np.linalg.norm(x - truth, axis=1)


def bad_start(seed, degrees, shift):
    """(R, t, s): a rotation by `degrees` about a seeded axis and a translation of length `shift` in a seeded direction."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal(3)
    return rodrigues(rng.standard_normal(3), np.radians(degrees)), shift * d / np.linalg.norm(d), 1.0


# ---- the contract ------------------------------------------------------------------------------------------------------ #
def pivot_of(P):
    """The centre of the box of the finite points, float32: 0.5 * lo + 0.5 * hi; zeros without a finite point."""
    P = np.asarray(P, f32).reshape(-1, 3)
    P = P[CR.valid(P)]
    if not len(P):
        return np.zeros(3, f32)
    with np.errstate(all="ignore"):
        c = f32(0.5) * P.min(axis=0) + f32(0.5) * P.max(axis=0)
    return np.where(np.isfinite(c), c, f32(0)).astype(f32)


def sample_terms(Q, P, Nrm, state, c, max_dist, metric):
    """Every source point under the state (R, t, s) float64: dict of valid, reached, used [N] bool, the rows J [rows, 7, N] and
    residuals r [rows, N] float32 (rows: 1 plane, 3 point; garbage where not used), cost [N] float64 (of the valid ones), md2."""
    P = np.ascontiguousarray(P, f32).reshape(-1, 3)
    c = np.asarray(c, f32)
    X = CR.transform(Q, *state)
    nn = CR.nearest(X, P, max_dist)
    md2 = np.float64(nn["md2"])
    valid = CR.valid(X)
    reached = valid & (nn["nearest"] >= 0)
    idx = np.where(reached, nn["nearest"], 0)
    with np.errstate(all="ignore"):
        p = P[idx] if len(P) else np.zeros_like(X)
        e = [X[:, a] - p[:, a] for a in range(3)]
        y = [X[:, a] - c[a] for a in range(3)]
        zero, one = np.zeros(len(X), f32), np.ones(len(X), f32)
        if metric == "plane":
            n = np.asarray(Nrm, f32).reshape(-1, 3)[idx] if len(P) else np.zeros_like(X)
            n = [n[:, a] for a in range(3)]
            n2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
            used = reached & (n2 > 0)
            r = [(n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]]
            J = [[n[0], n[1], n[2], (y[1] * n[2]) - (y[2] * n[1]), (y[2] * n[0]) - (y[0] * n[2]), (y[0] * n[1]) - (y[1] * n[0]),
                  (n[0] * y[0] + n[1] * y[1]) + n[2] * y[2]]]
            r64 = r[0].astype(np.float64)
            cost = np.where(used, np.fmin(r64 * r64, md2), md2)
        elif metric == "point":
            used = reached
            r = e
            J = [[one, zero, zero, zero, y[2], -y[1], y[0]], [zero, one, zero, -y[2], zero, y[0], y[1]],
                 [zero, zero, one, y[1], -y[0], zero, y[2]]]
            cost = np.where(used, nn["dist2"].astype(np.float64), md2)
        else:
            raise ValueError(metric)
    J, r = np.stack([np.stack(row) for row in J]), np.stack(r)
    assert J.dtype == f32 and r.dtype == f32
    return dict(valid=valid, reached=reached, used=used, J=J, r=r, cost=cost, md2=md2, X=X, nearest=nn["nearest"], dist2=nn["dist2"])


def accumulate(Q, P, Nrm, state, c, max_dist, metric="plane"):
    """-> (sums [37] float64, abs [37] float64: the sum of the terms' magnitudes, terms [37] int: how many are not zero, counts [3]:
    n_valid, n_reached, n_used).  Every term is an exact float64 product of two float32 values (the costs: exact squares, md2 or a
    float32 d2) and the sums are math.fsum's, correctly rounded: whatever order an implementation adds the n terms of a sum in, it
    lands within n * 2^-53 * (sum of magnitudes) of these."""
    st = sample_terms(Q, P, Nrm, state, c, max_dist, metric)
    used = st["used"]
    J, r = st["J"][:, :, used].astype(np.float64), st["r"][:, used].astype(np.float64)
    parts = [np.concatenate([J[w, k] * J[w, l] for w in range(J.shape[0])]) for k, l in UPPER]
    parts += [np.concatenate([J[w, k] * r[w] for w in range(J.shape[0])]) for k in range(7)]
    parts += [st["cost"][st["valid"]], (r * r).ravel()]
    sums, mags, terms = np.zeros(N_SUMS), np.zeros(N_SUMS), np.zeros(N_SUMS, np.int64)
    for n, p in enumerate(parts):
        sums[n], mags[n], terms[n] = math.fsum(p), math.fsum(np.abs(p)), int(np.count_nonzero(p))
    counts = np.array([int(st["valid"].sum()), int(st["reached"].sum()), int(used.sum())], np.int64)
    return sums, mags, terms, counts


def normal_matrix(sums):
    Hm = np.zeros((7, 7))
    for idx, (k, l) in enumerate(UPPER):
        Hm[k, l] = Hm[l, k] = sums[idx]
    return Hm


def step(sums, state, c, mode, damping):
    """One Gauss-Newton step about the pivot c; None at a pivot of the factor that is not positive."""
    n = 7 if mode == "sim3" else 6
    Hm = normal_matrix(sums)[:n, :n].copy()
    for k in range(n):
        Hm[k, k] = Hm[k, k] + damping * Hm[k, k]
    d = RR.cholesky_solve(Hm, sums[28:28 + n])
    if d is None:
        return None
    R, t, s = state
    Rx = RR.se3_exp(np.concatenate([np.zeros(3), d[3:6]]))[:3, :3]
    es = np.exp(d[6]) if n == 7 else 1.0
    c = np.asarray(c, f32).astype(np.float64)
    return Rx @ R, (es * (Rx @ (t - c)) + c) + d[:3], es * s if n == 7 else s


def register(Q, P, Nrm, *, init=None, pivot=None, max_dist, mode="sim3", metric="plane", iterations=20, damping=1e-9, min_pairs=64):
    """The whole loop -> dict(R, t, s, history [iterations+1, 5], status, normal_matrix [7,7])."""
    init = IDENTITY if init is None else init
    first = (np.array(init[0], np.float64), np.array(init[1], np.float64), float(init[2]))
    c = pivot_of(P) if pivot is None else np.asarray(pivot, f32)
    state, status = first, OK
    history = np.zeros((iterations + 1, 5))
    for it in range(iterations + 1):
        sums, _, _, counts = accumulate(Q, P, Nrm, state, c, max_dist, metric)
        history[it] = [counts[0], counts[1], counts[2], sums[35], sums[36]]
        if status != OK:
            continue
        if it == iterations:
            with np.errstate(all="ignore"):
                if history[it, 3] / history[it, 0] > history[0, 3] / history[0, 0]:
                    status, state = REVERTED, first
            continue
        new = None
        if counts[2] < min_pairs:
            status = TOO_FEW
        else:
            new = step(sums, state, c, mode, damping)
            if new is None:
                status = NOT_PD
        state = first if new is None else new
    return dict(R=state[0], t=state[1], s=state[2], history=history, status=status, normal_matrix=normal_matrix(sums))


# ---- starts that end in every status (tests/test_register_cpu.py pins the replica's answers, tests/test_register_gpu.py the kernel's) -- #
def cylinder(nt=48, nz=20):
    """An exact cylinder of radius 1 about the z axis with analytic inward normals (n_z = 0), float32, and a source on it."""
    th, z = np.meshgrid(2 * np.pi * np.arange(nt) / nt, 2.0 * np.arange(nz) / nz, indexing="ij")
    th, z = th.ravel(), z.ravel()
    P = np.stack([np.cos(th), np.sin(th), z], -1).astype(f32)
    Nrm = np.stack([-np.cos(th), -np.sin(th), np.zeros_like(th)], -1).astype(f32)
    Q = (np.stack([np.cos(th + 0.03), np.sin(th + 0.03), 0.9 * z + 0.1], -1) + np.array([0.01, -0.02, 0.0])).astype(f32)
    return Q, P, Nrm


def status_cases():
    """name -> (Q, P, Nrm, kwargs of register, the status it must end in).  Each returns its input state."""
    Q, P, Nrm = cylinder()
    sc = tube(small=True)
    far = (sc["source"] + f32(50.0)).astype(f32)
    kw = dict(max_dist=0.3, iterations=3)
    start = bad_start(3, 1.0, 0.01)
    # ... and one whose normals lean along the axis by noise of 0.01: nearly singular, it steps far along the axis; the final cost per
    # point is twice the first (3.4e-4 against 1.7e-4)
    leaning = Nrm.copy()
    leaning[:, 2] = (0.01 * np.random.default_rng(1).standard_normal(len(Nrm))).astype(f32)
    return {
        "cylinder": (Q, P, Nrm, dict(kw, init=start), NOT_PD),
        "nearly_cylinder": (Q, P, leaning, dict(kw, init=start), REVERTED),
        "empty_target": (sc["source"], np.zeros((0, 3), f32), np.zeros((0, 3), f32), dict(kw, init=start), TOO_FEW),
        "out_of_reach": (far, sc["target"], sc["normals"], dict(kw, init=start), TOO_FEW),
        "min_pairs": (sc["source"], sc["target"], sc["normals"], dict(kw, init=start, min_pairs=len(sc["source"]) + 1), TOO_FEW),
    }


# ---- the fused scene: fuse_ref.scene(6, 48, 64, 5) at 5 cm --------------------------------------------------------------------- #
FUSED_VOXEL = 0.05
FUSED_MOVE = (1.5, (0.04, -0.03, 0.05), 1.02)          # degrees about a seeded axis, t, s


@functools.lru_cache(maxsize=None)
def fused_scene():
    """Target: the scene fused at 5 cm, stride 1, with tests/normals_ref.py's normals.  Source: the stride-2 fusion, moved by the
    inverse of FUSED_MOVE; `truth` is the stride-2 fusion itself.  max_dist 4 voxels.  Also what the scene was made of."""
    import torch
    from coivo_amd import inference as I
    from tests import fuse_ref, normals_ref
    depths, _, K, M = fuse_ref.scene(6, 48, 64, 5)
    vs = float(f32(FUSED_VOXEL))
    origin, dims = I.fusion_grid(torch.from_numpy(K), torch.from_numpy(M), 48, 64, vs)
    kw = dict(max_depth=10.0, voxel_size=vs, origin=origin, dims=dims)
    gt = fuse_ref.fuse(depths, None, K, M, stride=1, **kw)
    normals = normals_ref.cloud_normals(depths, K, M, gt["voxels"], stride=1, **kw)["normals"]
    truth = fuse_ref.fuse(depths, None, K, M, stride=2, **kw)["points"]
    deg, t, s = FUSED_MOVE
    R = rodrigues(np.random.default_rng(5).standard_normal(3), np.radians(deg))
    t = np.array(t)
    source = moved(truth, R, t, s).astype(f32)
    return dict(target=gt["points"], normals=normals, source=source, truth=truth.astype(np.float64), R=R, t=t, s=s,
                max_dist=float(f32(4.0 * vs)), voxel_size=vs, depths=depths, K=K, M=M)
