"""-m gpu: the pose refinement (coivo_amd.inference.refine_edges / refine_trajectory, csrc/refine.hip) against its NumPy replica
(tests/refine_ref.py).  The per-sample arithmetic is pinned float32 and every term of a sum is an exact float64 product, so one
evaluation of the sums is held to the replica's correctly rounded sums by the bound any order of addition obeys; the loop, whose
float64 sin / cos may differ from NumPy's in the last place, to 1e-6."""
import functools

import numpy as np
import pytest
import torch

from tests import refine_ref as R
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

MAX_DEPTH = 4.5
SEED = 3
U = 2.0 ** -53


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _pairs(N):
    return [(k, k + 1) for k in range(N - 1)]


@functools.lru_cache(maxsize=None)
def _scene(N, H, W, seed=SEED):
    return R.textured_tube(N, H, W, seed)


@functools.lru_cache(maxsize=None)
def _start(H, W, seed=SEED):
    """The recovery start: 5 frames, truth perturbed by sigma_t = 0.01 and sigma_r = 0.005 rad per axis."""
    depths, frames, K, M, _, _ = _scene(5, H, W, seed)
    Tt = R.true_edges(M, _pairs(5))
    return depths, frames, K, M, Tt, R.perturb(Tt, seed + 7)


@functools.lru_cache(maxsize=None)
def _replica_loop(H, W, switches=()):
    depths, frames, K, M, Tt, T0 = _start(H, W)
    return R.refine_edges(depths, frames, K, _pairs(5), T0, max_depth=MAX_DEPTH, **dict(switches))


# ---- 1. one evaluation of the sums ---------------------------------------------------------------------------------------- #
def _check_accumulate(depths, frames, K, edges, T, gain, offset, **kw):
    from coivo_amd import inference as I
    sums, counts = I.refine_accumulate(_t(depths), _t(frames), _t(K), edges, _t(T), gain=_t(gain), offset=_t(offset),
                                       max_depth=MAX_DEPTH, **kw)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (len(edges), 48) and counts.dtype == torch.int32
    sums, counts = sums.cpu().numpy(), counts.cpu().numpy()
    gr = R.grey(frames)
    used = 0
    for e, (i, j) in enumerate(edges):
        want, mags, terms, wc = R.accumulate(depths, gr, K, i, j, T[e], gain[e], offset[e], max_depth=MAX_DEPTH, **kw)
        print("edge", (i, j), "counts", counts[e, :3], "want", wc)
        assert counts[e, :3].tolist() == wc.tolist() and counts[e, 3] == 0, (e, counts[e], wc)
        err = np.abs(sums[e, :46] - want)
        bound = terms * U * mags
        worst = int(np.argmax(err - bound))
        print("   largest error over bound: entry", worst, "error", err[worst], "bound", bound[worst])
        assert (err <= bound).all(), (e, worst, sums[e, worst], want[worst], err[worst], bound[worst])
        assert not sums[e, 46:].any()
        used += int(wc[1] + wc[2])
    return used


def test_accumulate_one_edge_smaller_than_a_strip():
    depths, frames, K, M, _, _ = _scene(2, 17, 23)
    T = R.perturb(R.true_edges(M, [(0, 1)]), 21)
    for kw in (dict(), dict(photometric=False), dict(geometric=False)):
        assert _check_accumulate(depths, frames, K, [(0, 1)], T, np.array([1.03]), np.array([-0.01]), **kw) > 100


def test_accumulate_with_intrinsics_that_differ_per_frame():
    N, H, W = 4, 33, 47
    rng = np.random.default_rng(11)
    K = np.zeros((N, 3, 3), np.float32)
    zoom = rng.uniform(0.9, 1.25, N)
    K[:, 0, 0] = 0.8 * W * zoom
    K[:, 1, 1] = 0.8 * W * zoom * rng.uniform(0.97, 1.03, N)
    K[:, 0, 2] = (W - 1) / 2 + rng.uniform(-4, 4, N)
    K[:, 1, 2] = (H - 1) / 2 + rng.uniform(-3, 3, N)
    K[:, 2, 2] = 1
    depths, frames, K, M, _, _ = R.textured_tube(N, H, W, SEED, K=K)
    edges = _pairs(N) + [(2, 0), (3, 1)]                              # (backwards and across two frames: the edge list is general)
    T = R.perturb(R.true_edges(M, edges), 22)
    gain, offset = rng.uniform(0.95, 1.05, len(edges)), rng.uniform(-0.02, 0.02, len(edges))
    assert _check_accumulate(depths, frames, K, edges, T, gain, offset) > 5000
    same_K = np.broadcast_to(K[0], K.shape).copy()                    # (the per-frame values matter)
    gr = R.grey(frames)
    a = R.accumulate(depths, gr, K, 0, 1, T[0], 1.0, 0.0, max_depth=MAX_DEPTH)
    b = R.accumulate(depths, gr, same_K, 0, 1, T[0], 1.0, 0.0, max_depth=MAX_DEPTH)
    assert a[3].tolist() != b[3].tolist()


def test_accumulate_with_infinite_and_nan_depths():
    N, H, W = 5, 48, 64
    depths, frames, K, M, _, _ = _scene(N, H, W)
    depths = depths.copy()
    rng = np.random.default_rng(5)
    hit = rng.random(depths.shape) < 0.06
    depths[hit] = np.array([np.inf, np.nan, 0.0, -1.0], np.float32)[rng.integers(0, 4, int(hit.sum()))]     # as filter_depths leaves them, and worse
    edges = _pairs(N)
    T = R.perturb(R.true_edges(M, edges), 23)
    used = _check_accumulate(depths, frames, K, edges, T, np.ones(4), np.zeros(4))
    assert used > 8000
    clean = R.accumulate(_scene(N, H, W)[0], R.grey(frames), K, 0, 1, T[0], 1.0, 0.0, max_depth=MAX_DEPTH)[3]
    dirty = R.accumulate(depths, R.grey(frames), K, 0, 1, T[0], 1.0, 0.0, max_depth=MAX_DEPTH)[3]
    assert dirty[0] < 0.85 * clean[0]                                 # (a bad tap hides a sample: the special values do reach the taps)


# ---- 2. determinism ------------------------------------------------------------------------------------------------------- #
def _bits_equal(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                                                  y.view(torch.int64) if y.dtype == torch.float64 else y)


def test_deterministic_across_calls_and_streams():
    from coivo_amd import inference as I
    depths, frames, K, M, Tt, T0 = _start(48, 64)
    args = (_t(depths), _t(frames), _t(K), _pairs(5), _t(T0))
    a, sa = I.refine_edges(*args, max_depth=MAX_DEPTH), I.refine_accumulate(*args, max_depth=MAX_DEPTH)
    b, sb = I.refine_edges(*args, max_depth=MAX_DEPTH), I.refine_accumulate(*args, max_depth=MAX_DEPTH)
    _bits_equal(a, b)
    _bits_equal(sa, sb)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        c, sc = I.refine_edges(*args, max_depth=MAX_DEPTH), I.refine_accumulate(*args, max_depth=MAX_DEPTH)
    side.synchronize()
    _bits_equal(a, c)
    _bits_equal(sa, sc)
    assert not torch.isnan(a.T).any() and (a.status == 0).all()


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("switches", [(), (("photometric", False),), (("geometric", False),), (("brightness", False),)],
                         ids=["both", "geometric", "photometric", "no-brightness"])
def test_loop_equals_the_replica(switches):
    from coivo_amd import inference as I
    depths, frames, K, M, Tt, T0 = _start(48, 64)
    want = _replica_loop(48, 64, switches)
    got = I.refine_edges(_t(depths), _t(frames), _t(K), _pairs(5), _t(T0), max_depth=MAX_DEPTH, **dict(switches))
    assert got.T.is_cuda and got.T.dtype == torch.float64 and tuple(got.T.shape) == (4, 4, 4)
    assert tuple(got.history.shape) == (4, 7, 5) and got.history.dtype == torch.float64 and got.status.dtype == torch.int32
    dT = np.abs(got.T.cpu().numpy() - want["T"])
    print(dict(switches), "largest |T - replica|", dT.max(), "status", got.status.tolist())
    assert got.status.cpu().tolist() == want["status"].tolist()
    assert dT.max() <= 1e-6
    assert np.array_equal(got.T.cpu().numpy()[:, 3], np.broadcast_to([0.0, 0.0, 0.0, 1.0], (4, 4)))
    assert np.abs(got.gain.cpu().numpy() - want["gain"]).max() <= 1e-6 and np.abs(got.offset.cpu().numpy() - want["offset"]).max() <= 1e-6
    h, hw = got.history.cpu().numpy(), want["history"]
    assert np.array_equal(h[:, 0, [0, 1, 3]], hw[:, 0, [0, 1, 3]])                        # the first evaluation: the same counts,
    assert np.allclose(h[:, 0, [2, 4]], hw[:, 0, [2, 4]], rtol=1e-12, atol=0)             # the same costs
    assert (h[:, :, 0] >= h[:, :, 1]).all() and (h[:, :, 0] >= h[:, :, 3]).all()
    # every later evaluation, the final one included, is of a state within 1e-6 of the replica's: a sample at a gate or at the
    # image border may fall on the other side (at most 4 of some 1900 allowed), each such sample moves a cost by at most its cap
    # (gate / sigma)^2 = 25, and the rest of a cost moves with the residuals, far below 1e-3 of it
    dn = np.abs(h[:, :, [0, 1, 3]] - hw[:, :, [0, 1, 3]])
    print("   history: largest count difference", dn.max(), "largest relative cost difference",
          (np.abs(h[:, :, [2, 4]] - hw[:, :, [2, 4]]) / np.maximum(hw[:, :, [2, 4]], 1e-300)).max())
    assert dn.max() <= 4
    flips = dn.sum(2, keepdims=True)
    assert (np.abs(h[:, :, [2, 4]] - hw[:, :, [2, 4]]) <= 1e-3 * hw[:, :, [2, 4]] + 25.0 * flips).all()
    assert not np.array_equal(h[:, -1], h[:, 0]) and not np.array_equal(h[:, 1], h[:, 0])          # (the rows are distinct evaluations)
    if not dict(switches).get("brightness", True) or not dict(switches).get("photometric", True):
        assert (got.gain == 1).all() and (got.offset == 0).all()


@pytest.mark.parametrize("seed", sorted(R.STATUS_CASES))
def test_freeze_and_revert_equal_the_replica(seed):
    from coivo_amd import inference as I
    depths, frames, K, T0 = R.status_case(seed)
    want = R.refine_edges(depths, frames, K, R.STATUS_EDGES, T0, **R.STATUS_KW)
    assert want["status"].tolist() == R.STATUS_CASES[seed]
    got = I.refine_edges(_t(depths), _t(frames), _t(K), R.STATUS_EDGES, _t(T0), **R.STATUS_KW)
    assert got.status.cpu().tolist() == want["status"].tolist()
    T = got.T.cpu().numpy()
    for e, st in enumerate(want["status"]):
        if st == R.OK:
            assert np.abs(T[e] - want["T"][e]).max() <= 1e-6
        else:                                                         # frozen or reverted: the input, to the bit
            assert np.array_equal(T[e], T0[e]) and float(got.gain[e]) == 1.0 and float(got.offset[e]) == 0.0


# ---- 4. recovery ---------------------------------------------------------------------------------------------------------- #
def test_recovers_the_pose_as_the_replica_does():
    """From truth perturbed by sigma_t = 0.01 and sigma_r = 0.005 rad, at the defaults: every pair's translation and rotation error
    against the scene's true relative pose is at most twice what the replica reaches from the same start (a rounding difference must
    not fail it; the bar is the replica's, never the kernel's own output), and the re-integrated trajectory is closer to the truth
    than the perturbed one."""
    from coivo_amd import inference as I
    depths, frames, K, M, Tt, T0 = _start(48, 64)
    want = _replica_loop(48, 64)
    tw, rw = R.pose_error(want["T"], Tt)
    perturbed = R.integrate(M[0], T0)
    traj, res = I.refine_trajectory(_t(depths), _t(frames), _t(K), torch.from_numpy(perturbed), max_depth=MAX_DEPTH)
    assert traj.dtype == torch.float64 and not traj.is_cuda and tuple(traj.shape) == (5, 4, 4) and (res.status == 0).all()
    tg, rg = R.pose_error(res.T.cpu().numpy(), Tt)
    t0, r0 = R.pose_error(T0, Tt)
    print("translation: start", t0, "replica", tw, "kernel", tg)
    print("rotation (degrees): start", r0, "replica", rw, "kernel", rg)
    assert (tg <= 2 * tw).all() and (rg <= 2 * rw).all()
    assert tw.max() <= 2e-3 and rw.max() <= 0.08                      # (the replica's own figures, DESIGN.md §3.6g: 1.52e-3, 0.062 degrees)
    ate0, ate1 = R.ate(perturbed, M), R.ate(traj.numpy(), M)
    print("ATE: perturbed", ate0, "refined", ate1)
    assert ate1 < ate0
    assert np.abs(traj.numpy() - R.integrate(M[0], res.T.cpu().numpy())).max() < 1e-12
    assert torch.equal(traj[0], torch.from_numpy(perturbed[0]))


# ---- 5. wiring ------------------------------------------------------------------------------------------------------------ #
def test_reconstruct_sequence_refines_when_asked(monkeypatch):
    from coivo_amd import inference as I, localize as Z, nn as hnn, synth
    from oracle import colvo_spec as S
    dn_o, pn_o = S.make_models(31)
    dn, pn = hnn.DepthNet(), hnn.PoseNet()
    dn.load_state_dict(dn_o.state_dict())
    pn.load_state_dict(pn_o.state_dict())
    b = synth.make_batch(5, 64, 96, seed=31)
    frames, K = b["tgt"].to(dev()), b["K"].to(dev())
    labels = torch.zeros(5, 1, 64, 96, dtype=torch.uint8, device=dev())
    labels[:, :, 20:40, 30:60] = 1
    kw = dict(stride=2, chunk=2, voxel_size=0.25, labels=labels, num_labels=1, consistency=I.Consistency(window=1, rel_tol=0.05))
    plain = I.reconstruct_sequence(dn, pn, frames, K, **kw)                               # as a caller from before would call it
    none = I.reconstruct_sequence(dn, pn, frames, K, refine=None, **kw)
    assert plain.refinement is None and none.refinement is None and len(plain) == 5
    for a, c in ((plain.depths, none.depths), (plain.rel_poses, none.rel_poses), (plain.cam2world, none.cam2world),
                 (plain.points, none.points), (plain.fused.points, none.fused.points), (plain.fused.counts, none.fused.counts),
                 (plain.consistency.depths, none.consistency.depths), (plain.polyps.position, none.polyps.position)):
        assert a.dtype == c.dtype and torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a.view(torch.int32),
                                                  c.view(torch.int64) if c.dtype == torch.float64 else c.view(torch.int32))
    # with a policy: what did the consumers receive?
    seen = {}
    for mod, name in ((I, "filter_depths"), (I, "stitch_point_cloud"), (I, "fuse_point_cloud"), (Z, "localize_polyps")):
        def spy(*args, _f=getattr(mod, name), _n=name, **kwargs):
            seen[_n] = (args[3] if _n == "localize_polyps" else args[2]).clone()
            return _f(*args, **kwargs)
        monkeypatch.setattr(mod, name, spy)
    policy = I.Refinement(iterations=4, min_samples=64)
    rec = I.reconstruct_sequence(dn, pn, frames, K, refine=policy, **kw)
    depths, rel, traj, points, fused = rec                                                # still five fields
    assert isinstance(rec.refinement, I.RefinementResult) and tuple(rec.refinement.T.shape) == (4, 4, 4)
    assert tuple(rec.refinement.history.shape) == (4, 5, 5)
    assert torch.equal(rec.depths, plain.depths) and torch.equal(rec.rel_poses, plain.rel_poses)
    Kn = K.to(torch.float32).contiguous()
    want_traj, want = I.refine_trajectory(rec.depths, frames.to(torch.float32).contiguous(), Kn, I.integrate_trajectory(rec.rel_poses),
                                          max_depth=I.MAX_DEPTH, **policy._asdict())
    _bits_equal(rec.refinement, want)
    assert torch.equal(rec.cam2world, want_traj)
    traj32 = rec.cam2world.to(dev(), torch.float32)
    assert sorted(seen) == ["filter_depths", "fuse_point_cloud", "localize_polyps", "stitch_point_cloud"]
    for name, got in seen.items():
        assert torch.equal(got, traj32), name
    status = rec.refinement.status.cpu().tolist()
    print("status", status)
    # on these seeded networks and frames every pair refines under this policy: what the consumers received is not the integrated
    # trajectory
    assert status == [I.REFINE_OK] * 4
    assert not torch.equal(rec.cam2world, plain.cam2world) and not torch.equal(traj32, plain.cam2world.to(dev(), torch.float32))
    with pytest.raises(ValueError, match="iterations"):
        I.reconstruct_sequence(dn, pn, frames, K, refine=I.Refinement(iterations=0))


# ---- the boundary on the device ------------------------------------------------------------------------------------------- #
def test_a_bad_edge_on_the_device_is_a_status_and_reads_nothing():
    """The C entry takes the edge list on the device and cannot refuse a bad edge: the kernels mark it and go nowhere through it."""
    from coivo_amd import _lib
    lib = _lib.load()
    depths, frames, K, M, _, _ = _scene(3, 17, 23)
    d, f, k = _t(depths), _t(frames), _t(K)
    pairs = [(0, 1), (1, 1), (0, 3), (-1, 2), (2, 1)]
    E = len(pairs)
    edges = torch.tensor(pairs, dtype=torch.int64).to(torch.int32).to(dev())
    T0 = np.stack([R.perturb(R.true_edges(M, [(0, 1)]), 9)[0]] * E)
    T0[-1] = R.perturb(R.true_edges(M, [(2, 1)]), 9)[0]
    T_init = _t(T0)
    it = 2
    ws = torch.empty(int(lib.colvo_refine_workspace_bytes(E, 3, 17, 23, it)), device=dev(), dtype=torch.uint8)
    T = torch.full((E, 4, 4), float("nan"), device=dev(), dtype=torch.float64)
    gain, offset = torch.empty(E, device=dev(), dtype=torch.float64), torch.empty(E, device=dev(), dtype=torch.float64)
    history = torch.full((E, it + 1, 5), float("nan"), device=dev(), dtype=torch.float64)
    status = torch.full((E,), -1, device=dev(), dtype=torch.int32)
    _lib.check(lib.colvo_refine_edges(_lib.ptr(d), _lib.ptr(f), _lib.ptr(k), 3, 17, 23, _lib.ptr(edges), E, _lib.ptr(T_init), it, 0.01,
                                      0.02, 0.05, 0.1, 1e-6, 16, 7, MAX_DEPTH, _lib.ptr(ws), _lib.ptr(T), _lib.ptr(gain),
                                      _lib.ptr(offset), _lib.ptr(history), _lib.ptr(status), _lib.stream_ptr()), "colvo_refine_edges")
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [R.OK, R.BAD_EDGE, R.BAD_EDGE, R.BAD_EDGE, R.OK]
    want = R.refine_edges(depths, frames, K, [(0, 1), (2, 1)], T0[[0, 4]], iterations=it, min_samples=16, max_depth=MAX_DEPTH)
    assert np.abs(T.cpu().numpy()[[0, 4]] - want["T"]).max() <= 1e-6
    for e in range(1, 4):
        assert np.array_equal(T[e].cpu().numpy(), T0[e]) and float(gain[e]) == 1.0 and float(offset[e]) == 0.0
        assert not history[e].any()


def test_argument_errors_on_the_device():
    from coivo_amd import inference as I
    depths, frames, K, M, _, _ = _scene(3, 17, 23)
    d, f, k = _t(depths), _t(frames), _t(K)
    T = _t(R.true_edges(M, _pairs(3)))
    ok = _pairs(3)
    for bad in ((d.cpu(), f, k), (d, f.cpu(), k), (d.double(), f, k), (d, f[:, :1], k), (d, f, k[:2]), (d[:, 0], f, k)):
        with pytest.raises(ValueError):
            I.refine_edges(*bad, ok, T)
    for edges in ([(0, 0)], [(0, 3)], [(-1, 0)], [], torch.tensor(ok).to(dev())):
        with pytest.raises(ValueError):
            I.refine_edges(d, f, k, edges, T[:max(1, len(edges))] if not isinstance(edges, torch.Tensor) else T)
    for bad_T in (T.float(), T[:1], T[:, :3]):
        with pytest.raises(ValueError, match="T must be"):
            I.refine_edges(d, f, k, ok, bad_T)
    out = I.refine_edges(d, f, k, torch.tensor(ok), T.cpu(), iterations=1, min_samples=16, max_depth=MAX_DEPTH)     # host T, tensor edges
    assert tuple(out.T.shape) == (2, 4, 4) and out.T.is_cuda


# ---- memory discipline ------------------------------------------------------------------------------------------------------ #
def test_memory_discipline():
    """refine_edges (six iterations) and refine_accumulate under tests/guarded.py: depths, frames, intrinsics and the starting edges
    between guard bands; the workspace (colvo_refine_workspace_bytes for that many iterations), T, gain, offset, the history and the
    status from the pool under both poisons.  The loop meets the replica as in test_loop_equals_the_replica, every output is the same
    bytes under either poison, and no guard byte changes.  Launches reached, at 5 frames of 48 x 64 and 4 edges: the strip sums, their
    fixed-order reduction and the float64 solve of every iteration, the final evaluation and the revert decision."""
    from coivo_amd import _lib, inference as I
    from tests import guarded as G
    lib = _lib.load()
    depths, frames, K, M, Tt, T0 = _start(48, 64)
    want = _replica_loop(48, 64, ())

    def run(pool):
        args = (pool.place(_t(depths)), pool.place(_t(frames)), pool.place(_t(K)), _pairs(5), pool.place(_t(T0)))
        return I.refine_edges(*args, max_depth=MAX_DEPTH), I.refine_accumulate(*args, max_depth=MAX_DEPTH)
    outs, pools = G.under_both_poisons(dev(), run, "refine_edges")
    for (got, (sums, counts)), pool in zip(outs, pools):
        assert got.status.cpu().tolist() == want["status"].tolist() and tuple(got.history.shape) == (4, 7, 5)
        assert np.abs(got.T.cpu().numpy() - want["T"]).max() <= 1e-6
        assert np.abs(got.gain.cpu().numpy() - want["gain"]).max() <= 1e-6 and np.abs(got.offset.cpu().numpy() - want["offset"]).max() <= 1e-6
        h, hw = got.history.cpu().numpy(), want["history"]
        assert np.array_equal(h[:, 0, [0, 1, 3]], hw[:, 0, [0, 1, 3]]) and np.allclose(h[:, 0, [2, 4]], hw[:, 0, [2, 4]], rtol=1e-12, atol=0)
        assert bool(torch.isfinite(sums).all()) and not bool(sums[:, 46:].any()) and not bool(counts[:, 3].any())
        G.assert_served(pool, 0, lib.colvo_refine_workspace_bytes(4, 5, 48, 64, 6), "refine_edges")
        G.assert_served(pool, 0, lib.colvo_refine_workspace_bytes(4, 5, 48, 64, 1), "refine_accumulate")
