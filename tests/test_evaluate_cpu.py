"""CPU checks of the evaluation side (coivo_amd/evaluate.py, csrc/evaluate.hip): the C-ABI refuses bad arguments before any
HIP call, the workspace size, and the float64 trajectory measures against an independent NumPy Umeyama."""
import ctypes as C
import math

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.build()
    return _lib.load()


def test_depth_metrics_entry_point_refuses_bad_arguments(lib):
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    args = dict(pred=p, gt=p, mask=None, N=2, H=8, W=8, lo=0.1, hi=10.0, ms=1, ws=p, per=p, scale=p, nv=p)

    def call(**kw):
        a = dict(args, **kw)
        return lib.colvo_depth_metrics(a["pred"], a["gt"], a["mask"], a["N"], a["H"], a["W"], a["lo"], a["hi"], a["ms"], a["ws"],
                                       a["per"], a["scale"], a["nv"], None)

    for name in ("pred", "gt", "ws", "per", "scale", "nv"):
        lib.colvo_abi_version()
        assert call(**{name: None}) != 0, name
        assert lib.colvo_last_error().startswith(b"colvo_depth_metrics: null pointer"), name
    for shape in (dict(N=0), dict(N=-1), dict(N=65536), dict(H=0), dict(W=-3), dict(H=1 << 15, W=1 << 15)):
        assert call(**shape) != 0, shape
        assert lib.colvo_last_error().startswith(b"colvo_depth_metrics: bad shape"), shape
    assert call(lo=10.0, hi=0.1) != 0 and b"depth range" in lib.colvo_last_error()
    assert call(ws=p + 8) != 0 and b"16-byte aligned" in lib.colvo_last_error()


def test_depth_metrics_workspace_bytes(lib):
    f = lib.colvo_depth_metrics_workspace_bytes
    for bad in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, 1 << 15, 1 << 15)):
        assert f(*bad) == 0, bad
    for H, W in ((1, 1), (17, 23), (256, 320), (512, 640)):
        sizes = [f(n, H, W) for n in (1, 2, 3, 64, 512, 65535)]
        assert all(s > 0 and s % 16 == 0 for s in sizes), (H, W, sizes)
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (H, W, sizes)
    assert f(8, 512, 640) > f(8, 256, 320)


def test_depth_metrics_refuses_cpu_tensors():
    from coivo_amd import evaluate as E
    t = torch.ones(2, 1, 8, 8)
    with pytest.raises(ValueError):
        E.depth_metrics(t, t)
    with pytest.raises(ValueError):
        E.depth_metrics(torch.ones(2, 3, 8, 8), t)


# ---- trajectories ------------------------------------------------------------------------------------------------------ #
def _rot(axis_angle):
    a = np.asarray(axis_angle, dtype=np.float64)
    th = np.linalg.norm(a)
    if th == 0:
        return np.eye(3)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def _random_traj(M, seed):
    rng = np.random.default_rng(seed)
    T = np.zeros((M, 4, 4))
    pos = np.cumsum(rng.normal(0, 0.3, size=(M, 3)), axis=0)
    for i in range(M):
        T[i, :3, :3] = _rot(rng.normal(0, 0.8, size=3))
        T[i, :3, 3] = pos[i]
        T[i, 3, 3] = 1
    return T


def _np_umeyama(x, y, with_scale):
    """The textbook algorithm (Umeyama 1991), written independently of the module: y ~ c R x + t."""
    n = x.shape[0]
    mx, my = x.mean(0), y.mean(0)
    sx = ((x - mx) ** 2).sum() / n
    cov = (y - my).T @ (x - mx) / n
    U, d, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(cov) < 0 or (np.linalg.det(cov) == 0 and np.linalg.det(U) * np.linalg.det(Vt) < 0):
        S[2, 2] = -1
    R = U @ S @ Vt
    c = np.trace(np.diag(d) @ S) / sx if with_scale else 1.0
    return R, my - c * R @ mx, c


def _np_ate(P, G, with_scale):
    R, t, c = _np_umeyama(P[:, :3, 3], G[:, :3, 3], with_scale)
    e = G[:, :3, 3] - (c * P[:, :3, 3] @ R.T + t)
    return math.sqrt((e ** 2).sum(1).mean()), c


def _np_rpe(P, G, c, delta):
    P = P.copy()
    P[:, :3, 3] *= c
    te, re = [], []
    for i in range(len(P) - delta):
        dg = np.linalg.inv(G[i]) @ G[i + delta]
        dp = np.linalg.inv(P[i]) @ P[i + delta]
        E = np.linalg.inv(dg) @ dp
        te.append(np.linalg.norm(E[:3, 3]))
        re.append(math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(E[:3, :3]) - 1) / 2)))))
    return math.sqrt(np.mean(np.square(te))), math.sqrt(np.mean(np.square(re)))


def _sim3(T, R, t, s):
    """Map a camera-to-world trajectory through the world transform x -> s R x + t."""
    out = T.copy()
    out[:, :3, :3] = R @ T[:, :3, :3]
    out[:, :3, 3] = s * T[:, :3, 3] @ R.T + t
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("mode", ["sim3", "se3"])
def test_ate_and_rpe_match_numpy_umeyama(seed, mode):
    from coivo_amd import evaluate as E
    G = _random_traj(20, seed)
    P = _sim3(G, _rot([0.3, -0.2, 0.9]), np.array([1.0, -2.0, 0.5]), 0.4)
    rng = np.random.default_rng(seed + 10)
    P[:, :3, 3] += rng.normal(0, 0.05, size=(20, 3))       # noise: non-trivial residuals (and rotation errors well away from 0)
    for i in range(20):
        P[i, :3, :3] = P[i, :3, :3] @ _rot(rng.normal(0, 0.05, size=3))
    want, c = _np_ate(P, G, mode == "sim3")
    got = E.ate(torch.from_numpy(P), torch.from_numpy(G), mode=mode)
    assert want > 1e-3 and abs(got - want) < 1e-9, (got, want)
    _, _, s = E.align_trajectory(torch.from_numpy(P), torch.from_numpy(G), mode)
    assert abs(s - c) < 1e-9
    for delta in (1, 3):
        wt, wr = _np_rpe(P, G, c, delta)
        gt_, gr = E.rpe(torch.from_numpy(P), torch.from_numpy(G), delta=delta, mode=mode)
        assert abs(gt_ - wt) < 1e-9 and abs(gr - wr) < 1e-9, (delta, gt_, wt, gr, wr)


def test_reflection_fix_gives_a_rotation():
    from coivo_amd import evaluate as E
    G = _random_traj(12, 4)
    P = G.copy()
    P[:, :3, 3] = G[:, :3, 3] * np.array([1.0, 1.0, -1.0])         # a mirror image: the best orthogonal map is a reflection
    R, _, _ = E.align_trajectory(torch.from_numpy(P), torch.from_numpy(G))
    assert abs(float(torch.det(R)) - 1.0) < 1e-12
    assert float((R.t() @ R - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12


@pytest.mark.parametrize("scale", [0.37, 1.0, 5.0])
def test_sim3_image_of_gt_has_zero_ate(scale):
    from coivo_amd import evaluate as E
    G = _random_traj(15, 7)
    P = _sim3(G, _rot([-1.1, 0.4, 0.2]), np.array([3.0, 0.1, -7.0]), scale)
    assert E.ate(P, G, mode="sim3") < 1e-9
    se3 = E.ate(P, G, mode="se3")
    if scale == 1.0:
        assert se3 < 1e-9
    else:
        assert se3 > 1e-3
    assert E.ate(P, G, mode="none") > 1e-3
    t, r = E.rpe(P, G, mode="sim3")
    assert t < 1e-9 and r < 1e-5


def test_halved_translations_have_zero_sim3_ate():
    """A trajectory integrated from the ground truth's relative poses with every translation halved is the ground truth at
    half scale: zero under sim3 (scale 2 recovered), not under se3."""
    from coivo_amd import evaluate as E, inference as I
    g = torch.Generator().manual_seed(3)
    rel = torch.cat([0.2 * torch.randn(12, 3, generator=g), 0.1 * torch.randn(12, 3, generator=g)], dim=1).double()
    G = I.integrate_trajectory(rel)
    half = rel.clone()
    half[:, :3] *= 0.5
    P = I.integrate_trajectory(half)
    assert E.ate(P, G, mode="sim3") < 1e-9
    assert abs(E.align_trajectory(P, G)[2] - 2.0) < 1e-9
    assert E.ate(P, G, mode="se3") > 1e-3
    t, r = E.rpe(P, G)
    assert t < 1e-9 and r < 1e-5


def test_rpe_of_identical_trajectories_is_zero():
    from coivo_amd import evaluate as E
    G = torch.from_numpy(_random_traj(10, 9))
    for mode in ("sim3", "se3", "none"):
        for delta in (1, 4):
            t, r = E.rpe(G, G.clone(), delta=delta, mode=mode)
            assert t < 1e-12 and r < 1e-5, (mode, delta, t, r)     # (arccos near 1: the angle is sqrt(eps)-resolved)
    assert E.ate(G, G) < 1e-12


def test_trajectory_arguments_are_checked():
    from coivo_amd import evaluate as E
    G = torch.from_numpy(_random_traj(6, 1))
    with pytest.raises(ValueError):
        E.align_trajectory(G, G, mode="affine")
    with pytest.raises(ValueError):
        E.ate(G[:5], G)
    with pytest.raises(ValueError):
        E.rpe(G, G, delta=6)
    with pytest.raises(ValueError):
        E.ate(G[:, :3, :3], G[:, :3, :3])
