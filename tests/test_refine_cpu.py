"""No GPU: the pose refinement contract (include/colvo.h colvo_refine_*) as tests/refine_ref.py restates it.  The
replica's rows are held to float64 autograd through the oracle's own project / bilinear_sample; its loop recovers the pose on the
textured tube; the geometric term alone is shown to be ill-conditioned there (the reason both terms are on by default); freeze and
revert; and the argument checks of the Python wrappers and of the C entry points."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import refine_ref as R

MAX_DEPTH = 4.5
SEED = 3


@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _scene(N, H, W, seed=SEED):
    return R.textured_tube(N, H, W, seed)


def _pairs(N):
    return [(k, k + 1) for k in range(N - 1)]


# ---- the rows against float64 autograd ------------------------------------------------------------------------------------ #
def _twist(xi):
    z = torch.zeros((), dtype=torch.float64)
    return torch.stack([torch.stack([z, -xi[5], xi[4], xi[0]]), torch.stack([xi[5], z, -xi[3], xi[1]]),
                        torch.stack([-xi[4], xi[3], z, xi[2]]), torch.stack([z, z, z, z])])


def _oracle_residuals(S, monkeypatch, depths, gr, K, i, j, T0, params):
    """(rel, r_I) [2,H,W] float64 of params = (xi [6], a, b) at the pose exp(xi) T0, composed from the oracle's project and
    bilinear_sample.  project() builds its transform from a pose vector; the left perturbation of a general T has none, so the
    module's pose_vec2mat is replaced for the call by one that returns exp(xi) T0 -- back-projection, projection, validity and the
    four-tap sampling are the oracle's own code."""
    d64 = torch.from_numpy(depths).double()
    g64 = torch.from_numpy(gr).double()
    k = torch.from_numpy(K[i:i + 1]).double()
    H, W = depths.shape[2:]
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    T = (torch.linalg.matrix_exp(_twist(params[:6])) @ torch.from_numpy(T0))[:3]
    monkeypatch.setattr(S, "pose_vec2mat", lambda pose: T[None])
    d = d64[i:i + 1]
    x, y, valid = S.project(d, torch.zeros(1, 6, dtype=torch.float64), k)
    X, Y = (u - k[0, 0, 2]) / k[0, 0, 0] * d[0, 0], (v - k[0, 1, 2]) / k[0, 1, 1] * d[0, 0]
    Pz = T[2, 0] * X + T[2, 1] * Y + T[2, 2] * d[0, 0] + T[2, 3]
    s = S.bilinear_sample(d64[j:j + 1], x, y, valid)[0, 0]
    c = S.bilinear_sample(g64[j:j + 1, None], x, y, valid)[0, 0]
    rel = (Pz - s) / (Pz + s)
    r_I = (params[6] * c + params[7]) - g64[i]
    return torch.stack([rel, r_I])


def test_rows_equal_float64_autograd_through_the_oracle(monkeypatch):
    """J_g and J_p of every visible sample farther than 1e-3 pixel from a tap boundary.  Bound: the float32 sample position is off by
    a few ulp of W (2e-5 pixel), which moves a bilinear gradient by that fraction of its change across a cell -- on this smooth scene
    below ten times the gradient itself, 2e-4 -- and the float32 chain of some twenty operations adds 1e-5 with the cancellation in
    P x g; so every entry is held to 5e-4 of the row's largest entry (pose part) or of itself (brightness part)."""
    from oracle import colvo_spec as S
    N, H, W = 3, 33, 47
    depths, frames, K, M, _, _ = _scene(N, H, W)
    finite = np.where(np.isfinite(depths), depths, np.float32(100.0))       # (the lumen: far away, never visible at max_depth 4.5)
    gr = R.grey(frames)
    i, j = 0, 1
    T0 = R.perturb(R.true_edges(M, [(i, j)]), 11)[0]
    a, b = 1.05, -0.02
    kw = dict(sigma_geo=0.01, sigma_photo=0.02, gate_geo=0.05, gate_photo=0.1, max_depth=MAX_DEPTH)
    st = R.sample_terms(finite, gr, K, i, j, T0, a, b, **kw)
    # T0 exactly as the replica sees it: its float32 rounding (the oracle then differentiates the same function)
    t32, a32, b32 = R.state32(T0, a, b)
    T32 = np.eye(4)
    T32[:3, :3], T32[:3, 3] = t32[:9].reshape(3, 3), t32[9:]
    p0 = torch.tensor([0.0] * 6 + [float(a32), float(b32)], dtype=torch.float64)
    f = lambda p: _oracle_residuals(S, monkeypatch, finite, gr, K, i, j, T32, p)
    val = f(p0)
    jac = torch.stack([torch.autograd.functional.jvp(f, p0, torch.eye(8, dtype=torch.float64)[q])[1] for q in range(8)]).numpy()
    inv = (float(np.float32(1) / np.float32(0.01)), float(np.float32(1) / np.float32(0.02)))
    fx_, fy_ = st["x"] - np.floor(st["x"]), st["y"] - np.floor(st["y"])
    away = (np.minimum(fx_, 1 - fx_) > 1e-3) & (np.minimum(fy_, 1 - fy_) > 1e-3)
    sel = st["visible"] & away
    assert sel.sum() > 800
    assert np.abs(st["rel"][sel] - val[0].numpy()[sel]).max() < 1e-5 and np.abs(st["r_I"][sel] - val[1].numpy()[sel]).max() < 1e-5
    worst = 0.0
    for w, name in enumerate(("J_g", "J_p")):
        want = jac[:, w] * inv[w]                                  # [8,H,W]
        got = st[name].astype(np.float64)
        scale = np.abs(want[:6]).max(0)
        for q in range(8):
            ref = scale if q < 6 else np.abs(want[q])
            err = np.abs(got[q] - want[q])[sel]
            worst = max(worst, float((err / np.maximum(ref[sel], 1e-30)).max()) if ref[sel].max() > 0 else float(err.max()))
            assert (err <= 5e-4 * ref[sel]).all(), (name, q, float(err.max()), float(ref[sel].max()))
        assert np.abs(want[:6, sel]).max() > 1.0                   # the comparison is not empty
    assert not st["J_g"][6:].any()
    print("largest row error relative to the row's largest entry:", worst)


# ---- the loop ----------------------------------------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def _refined(H, W, seed, **kw):
    N = 5
    depths, frames, K, M, _, _ = _scene(N, H, W, seed)
    Tt = R.true_edges(M, _pairs(N))
    T0 = R.perturb(Tt, seed + 7)
    return Tt, T0, R.refine_edges(depths, frames, K, _pairs(N), T0, max_depth=MAX_DEPTH, **kw), M


@pytest.mark.parametrize("H,W,factor", [(48, 64, 1.0), (33, 47, 2.0)])
@pytest.mark.parametrize("seed", [3, 4, 5])
def test_loop_recovers_the_pose_on_the_tube(H, W, seed, factor):
    """Truth perturbed by sigma_t = 0.01 and sigma_r = 0.005 rad per axis (expected norms 0.017 and 0.5 degrees): at the defaults
    every pair ends below a fifth of those at 48x64 -- 3.5e-3 and 0.1 degrees -- and below twice that at 33x47, where a pixel is 1.4
    times as large and the wall's interpolation error about twice.  Measured: <= 1.72e-3 / 0.062 degrees and <= 2.7e-3 / 0.163
    degrees."""
    Tt, T0, out, M = _refined(H, W, seed)
    (t0, r0), (t1, r1) = R.pose_error(T0, Tt), R.pose_error(out["T"], Tt)
    print(H, W, seed, "translation", t0, "->", t1, "rotation", r0, "->", r1)
    assert (out["status"] == R.OK).all()
    assert t1.max() <= factor * 0.01 * np.sqrt(3) / 5 and r1.max() <= factor * np.degrees(0.005 * np.sqrt(3)) / 5
    assert t1.max() < t0.max() / 4 and r1.max() < r0.max() / 3
    h = out["history"]
    assert ((h[:, -1, 2] + h[:, -1, 4]) / h[:, -1, 0] < 0.1 * (h[:, 0, 2] + h[:, 0, 4]) / h[:, 0, 0]).all()     # its own measure
    assert R.ate(R.integrate(M[0], out["T"]), M) < 0.3 * R.ate(R.integrate(M[0], T0), M)
    # exp(delta) is a rotation to the last place: the update leaves the determinant where the float32 cam2world put it
    assert np.allclose(out["T"][:, 3], [0, 0, 0, 1])
    assert np.abs(np.linalg.det(out["T"][:, :3, :3]) - np.linalg.det(T0[:, :3, :3])).max() < 1e-12


def test_the_geometric_term_alone_is_ill_conditioned_in_a_tube():
    """A tube lets the camera slide along the axis and spin about it without changing a depth: the geometric normal matrix has a
    condition number in the tens of thousands, the photometric term brings it to hundreds, and the geometric-only loop moves the
    translation away from the truth where both terms recover it.  This is why Refinement() has both terms on."""
    N, H, W = 5, 48, 64
    depths, frames, K, M, _, _ = _scene(N, H, W)
    gr = R.grey(frames)
    Tt = R.true_edges(M, _pairs(N))
    T0 = R.perturb(Tt, SEED + 7)
    conds = {}
    for name, kw in (("geo", dict(photometric=False)), ("both", dict())):
        sums = R.accumulate(depths, gr, K, 0, 1, T0[0], 1.0, 0.0, max_depth=MAX_DEPTH, **kw)[0]
        conds[name] = np.linalg.cond(R.normal_matrix(sums, 6))
    print(conds)
    assert conds["geo"] > 1e4 and conds["both"] < 2e3 and conds["geo"] > 30 * conds["both"]
    _, _, geo, _ = _refined(H, W, SEED, photometric=False)
    _, _, both, _ = _refined(H, W, SEED)
    t0 = R.pose_error(T0, Tt)[0]
    tg, tb = R.pose_error(geo["T"], Tt)[0], R.pose_error(both["T"], Tt)[0]
    assert tg.max() > t0.max() and tg.max() > 10 * tb.max(), (t0, tg, tb)
    # by its own measure the geometric-only result is no worse than its input (or it would have been reverted)
    h = geo["history"]
    assert (geo["status"] == R.OK).all() and (h[:, -1, 2] / h[:, -1, 0] <= h[:, 0, 2] / h[:, 0, 0]).all()


@pytest.mark.parametrize("seed", sorted(R.STATUS_CASES))
def test_freeze_and_revert(seed):
    depths, frames, K, T0 = R.status_case(seed)
    out = R.refine_edges(depths, frames, K, R.STATUS_EDGES, T0, **R.STATUS_KW)
    assert out["status"].tolist() == R.STATUS_CASES[seed]
    h = out["history"]
    for e, st in enumerate(out["status"]):
        F0, F1 = (h[e, 0, 2] + h[e, 0, 4]) / h[e, 0, 0], (h[e, -1, 2] + h[e, -1, 4]) / h[e, -1, 0]
        if st == R.OK:
            assert not np.array_equal(out["T"][e], T0[e]) and F1 <= F0
            continue
        assert np.array_equal(out["T"][e], T0[e]) and out["gain"][e] == 1.0 and out["offset"][e] == 0.0
        if st == R.REVERTED:
            assert F1 > F0 and h[e, :, 0].min() >= 16               # it ran to the end, and ended worse by its own measure
        if st == R.TOO_FEW:
            assert h[e, :, 0].min() < 16
        if st in (R.TOO_FEW, R.NOT_PD):                              # frozen: the evaluations after the freeze are of the initial state
            assert np.array_equal(h[e, -1], h[e, 0])


def test_too_few_samples_and_flat_frames_freeze():
    N, H, W = 3, 17, 23
    depths, frames, K, M, _, _ = _scene(N, H, W)
    T0 = R.perturb(R.true_edges(M, _pairs(N)), 5)
    out = R.refine_edges(depths, frames, K, _pairs(N), T0, max_depth=MAX_DEPTH, min_samples=100000)
    assert (out["status"] == R.TOO_FEW).all() and np.array_equal(out["T"], T0)
    flat = np.full_like(frames, 0.5)                                # no image gradient: the photometric pose block is zero
    out = R.refine_edges(depths, flat, K, _pairs(N), T0, max_depth=MAX_DEPTH, min_samples=16, geometric=False)
    assert (out["status"] == R.NOT_PD).all() and np.array_equal(out["T"], T0)


def test_se3_exponential():
    rng = np.random.default_rng(0)
    for scale in (1e-9, 1e-5, 9e-5, 1.1e-4, 1e-2, 1.0):
        xi = scale * rng.standard_normal(6)
        E = R.se3_exp(xi)
        A = _twist(torch.from_numpy(xi)).numpy()
        want, term = np.eye(4), np.eye(4)
        for n in range(1, 40):                                      # the power series itself (|xi| <= 3: it converges to the last place)
            term = term @ A / n
            want = want + term
        assert np.abs(E - want).max() < 4e-16 * max(1.0, np.abs(want).max()), scale
        assert np.abs(E[:3, :3] @ E[:3, :3].T - np.eye(3)).max() < 1e-15


# ---- the boundary ------------------------------------------------------------------------------------------------------- #
def test_workspace_query(lib):
    f = lib.colvo_refine_workspace_bytes
    for bad in ((0, 4, 8, 8, 6), (65536, 4, 8, 8, 6), (3, 0, 8, 8, 6), (3, 65536, 8, 8, 6), (3, 4, 0, 8, 6), (3, 4, 8, -1, 6),
                (3, 4, 1 << 15, 1 << 15, 6), (3, 4, 8, 8, 65), (3, 4, 8, 8, -1)):
        assert f(*bad) == 0, bad
    # one row of 52 doubles per 16 tiles of 8x8 and edge; a grey plane per frame; 64 B of state and 4 B of status per edge
    assert f(3, 4, 48, 64, 6) == 3 * 3 * 52 * 8 + 4 * 48 * 64 * 4 + 3 * 64 + 16
    assert f(511, 512, 256, 320, 6) == 511 * 80 * 52 * 8 + 512 * 256 * 320 * 4 + 511 * 64 + 2048
    assert f(3, 4, 48, 64, 1) == f(3, 4, 48, 64, 64)


def test_c_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    base = dict(N=3, H=8, W=8, E=2, iterations=6, sg=0.01, sp=0.02, gg=0.05, gp=0.1, damping=1e-6, min_samples=16, terms=7,
                max_depth=4.5, ws=p, null=None)

    def edges(**kw):
        a = dict(base, **kw)
        ptrs = [p] * 12
        if a["null"] is not None:
            ptrs[a["null"]] = 0
        d, f, k, e, t, oT, og, oo, h, s = ptrs[:10]
        return lib.colvo_refine_edges(d, f, k, a["N"], a["H"], a["W"], e, a["E"], t, a["iterations"], a["sg"], a["sp"], a["gg"],
                                      a["gp"], a["damping"], a["min_samples"], a["terms"], a["max_depth"], a["ws"], oT + 256 if oT else 0, og, oo,
                                      h, s, 0)

    def accum(**kw):
        a = dict(base, **kw)
        ptrs = [p] * 8
        if a["null"] is not None:
            ptrs[a["null"]] = 0
        d, f, k, e, t, os_, oc = ptrs[:7]
        return lib.colvo_refine_accumulate(d, f, k, a["N"], a["H"], a["W"], e, a["E"], t, 0, 0, a["sg"], a["sp"], a["gg"], a["gp"],
                                           a["terms"], a["max_depth"], a["ws"], os_, oc, 0)

    def refused(call, msg, **kw):
        assert call(**kw) != 0, kw
        err = lib.colvo_last_error().decode()
        assert msg in err and err.startswith("colvo_refine_"), (kw, err)

    for call, n in ((edges, 10), (accum, 7)):
        for k in range(n):
            refused(call, "null pointer", null=k)
        refused(call, "null pointer", ws=0)
        for s in (dict(E=0), dict(E=65536), dict(N=0), dict(N=65536), dict(H=0), dict(W=-2), dict(H=1 << 15, W=1 << 15)):
            refused(call, "bad shape", **s)
        for name in ("sg", "sp", "gg", "gp", "max_depth"):
            for v in (0.0, -1.0, float("nan"), float("inf")):
                refused(call, "finite and positive", **{name: v})
        for v in (0, 4, 8, -1):
            refused(call, "bad terms", terms=v)
        refused(call, "16-byte aligned", ws=p + 8)
    for v in (0, -1, 65):
        refused(edges, "bad iterations", iterations=v)
    for s in (dict(damping=-1e-9), dict(damping=float("nan")), dict(damping=float("inf")), dict(min_samples=0)):
        refused(edges, "bad damping", **s)
    assert lib.colvo_refine_edges(p, p, p, 3, 8, 8, p, 2, p, 6, 0.01, 0.02, 0.05, 0.1, 1e-6, 16, 7, 4.5, p, p, p, p, p, p, 0) != 0
    assert b"alias" in lib.colvo_last_error()


def test_kernels_use_no_scratch(lib, tmp_path):
    """The resource metadata of the four kernels: no private segment, no spilled register -- the 46 float64 accumulators of
    k_refine_accum stay in registers."""
    import re
    from coivo_amd import build
    asm = open(build.emit_asm("refine.hip", str(tmp_path / "refine.s"))).read()
    kernels = set(re.findall(r"\.name:\s+(\S*k_refine_\w+)", asm))
    assert len(kernels) == 4 and all(any(f"k_refine_{n}" in k for k in kernels) for n in ("grey", "init", "accum", "solve")), kernels
    for key in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count"):
        vals = re.findall(rf"\.{key}:\s+(\d+)", asm)
        assert len(vals) == 4 and all(int(v) == 0 for v in vals), (key, vals)
    assert re.findall(r"\.agpr_count:\s+(\d+)", asm) in ([], ["0"] * 4)      # ... and are not parked in accumulation registers


def test_python_wrappers_refuse_bad_arguments(lib):
    from coivo_amd import inference as I
    depths, frames, K, M, _, _ = _scene(3, 17, 23)
    d, f, k = (torch.from_numpy(a) for a in (depths, frames, K))
    T = torch.from_numpy(R.true_edges(M, _pairs(3)))
    ok = [(0, 1), (1, 2)]
    for bad in (dict(iterations=0), dict(iterations=65), dict(iterations=2.0), dict(iterations=True), dict(sigma_geo=0.0),
                dict(sigma_photo=-1.0), dict(gate_geo=float("nan")), dict(gate_photo=float("inf")), dict(sigma_geo=1e-50),
                dict(max_depth=0.0), dict(max_depth=1e39), dict(damping=-1.0), dict(damping=float("nan")), dict(damping=None),
                dict(min_samples=0), dict(min_samples=1.5), dict(sigma_geo=None)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            I.refine_edges(d, f, k, ok, T, **bad)
    with pytest.raises(ValueError, match="at least one"):
        I.refine_edges(d, f, k, ok, T, geometric=False, photometric=False)
    # these tensors live on the CPU: the policy above was refused before that mattered
    with pytest.raises(ValueError, match="CUDA"):
        I.refine_edges(d, f, k, ok, T)
    with pytest.raises(ValueError, match=r"\[N,1,H,W\]"):
        I.refine_edges(d[0], f, k, ok, T)
    with pytest.raises(ValueError, match="at least one"):
        I.refine_accumulate(d, f, k, ok, T, geometric=False, photometric=False)
    with pytest.raises(ValueError, match="CUDA"):
        I.refine_accumulate(d, f, k, ok, T)
    with pytest.raises(ValueError, match="cam2world"):
        I.refine_trajectory(d, f, k, torch.eye(4))
    with pytest.raises(ValueError, match="two frames"):
        I.refine_trajectory(d, f, k, torch.eye(4)[None])
    with pytest.raises(TypeError):
        I.refine_trajectory(d, f, k, torch.from_numpy(M), window=2)
    with pytest.raises(ValueError, match="iterations"):
        I.refine_trajectory(d, f, k, torch.from_numpy(M), iterations=0)
    # the edge list and T are checked before anything is uploaded (the checks of the device tensors come first: fake them)
    fake = lambda who, name, t, shape: t
    import unittest.mock as mock
    from coivo_amd import _args, refine
    with mock.patch.object(_args, "device_f32", fake), mock.patch.object(refine, "device_f32", fake):
        for edges in ([(0, 0)], [(0, 3)], [(-1, 1)], [], [(0, 1, 2)], [0, 1], torch.tensor([[0, 1]]).float(), None):
            with pytest.raises(ValueError, match="edge|edges_ij|E="):
                I._refine_inputs("refine_edges", d, f, k, edges, T[:1])
        for bad_T in (T.float(), T[:1], T[:, :3], None):
            with pytest.raises(ValueError, match="T must be"):
                I._refine_inputs("refine_edges", d, f, k, ok, bad_T)


def test_policy_and_result_types():
    from coivo_amd import inference as I
    assert I.Refinement() == (6, 0.01, 0.02, 0.05, 0.1, 1e-6, 256, True, True, True)
    assert I.Refinement._fields == tuple(R.DEFAULTS) and I.Refinement()._asdict() == R.DEFAULTS
    assert "not" in I.Refinement.__doc__ and "tuned" in I.Refinement.__doc__
    assert I.RefinementResult._fields == ("T", "gain", "offset", "history", "status")
    assert (I.REFINE_OK, I.REFINE_TOO_FEW, I.REFINE_NOT_PD, I.REFINE_REVERTED, I.REFINE_BAD_EDGE) == (R.OK, R.TOO_FEW, R.NOT_PD, R.REVERTED,
                                                                                                    R.BAD_EDGE)
    r = I.Reconstruction(1, 2, 3, 4)
    assert len(r) == 5 and r.refinement is None and r.consistency is None and r.polyps is None
    r2 = r._replace(points=7, refinement="x")
    assert r2.points == 7 and r2.refinement == "x" and r2.consistency is None
    import inspect
    assert inspect.signature(I.reconstruct_sequence).parameters["refine"].default is None
