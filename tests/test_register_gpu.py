"""-m gpu: the registration (coivo_amd.evaluate.register_clouds / register_accumulate, csrc/register.hip) against its NumPy replica
(tests/register_ref.py).  The per-sample arithmetic is pinned float32, the nearest neighbour is the query's own exact rule and every
term of a sum is an exact float64 product, so one evaluation of the sums is held to the replica's correctly rounded sums by the
bound any order of addition obeys, and the counts exactly; the loop, whose float64 sin / cos / exp may differ from NumPy's in the
last place, to 1e-6."""
import functools

import numpy as np
import pytest
import torch

from tests import register_ref as G
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ITER = 8
START = G.bad_start(3, 1.0, 0.01)[:2] + (1.01,)                  # the perturbed state of the single evaluations


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev())              # (a copy: the scenes are read-only)


def _init(state):
    return tuple(torch.from_numpy(np.asarray(v, np.float64)) for v in state[:2]) + (float(state[2]),)


# ---- 1. one evaluation of the sums ---------------------------------------------------------------------------------------- #
def _check_accumulate(Q, P, Nrm, max_dist, metric, state=START, pivot=None):
    from coivo_amd import evaluate as E
    sums, counts = E.register_accumulate(_t(Q), _t(P), target_normals=_t(Nrm) if metric == "plane" else None, init=_init(state),
                                         pivot=pivot, max_dist=max_dist, metric=metric)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (40,) and counts.dtype == torch.int64 and tuple(counts.shape) == (4,)
    sums, counts = sums.cpu().numpy(), counts.cpu().numpy()
    c = G.pivot_of(P) if pivot is None else np.asarray(pivot, np.float32)
    want, mags, terms, wc = G.accumulate(Q, P, Nrm, state, c, max_dist, metric)
    print(metric, "N", len(Q), "M", len(P), "counts", counts[:3], "want", wc)
    assert counts[:3].tolist() == wc.tolist() and counts[3] == 0
    err = np.abs(sums[:37] - want)
    bound = terms * U * mags
    worst = int(np.argmax(err - bound))
    print("   largest error over bound: entry", worst, "error", err[worst], "bound", bound[worst])
    assert (err <= bound).all(), (worst, sums[worst], want[worst], err[worst], bound[worst])
    assert not sums[37:].any()
    return wc


@pytest.mark.parametrize("metric", ["plane", "point"])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_accumulate_below_a_wave_below_a_workgroup_and_one_over(n, metric):
    sc = G.tube(small=True)
    wc = _check_accumulate(sc["source"][100:100 + n], sc["target"], sc["normals"], sc["max_dist"], metric)
    assert wc.tolist() == [n, n, n]


@pytest.mark.parametrize("metric", ["plane", "point"])
def test_accumulate_the_full_scene(metric):
    """6 783 source points: 7 partial rows for the 4 groups of the row reduction, the last one ragged."""
    sc = G.tube()
    wc = _check_accumulate(sc["source"], sc["target"], sc["normals"], sc["max_dist"], metric)
    assert wc.tolist() == [6783] * 3


def _hostile():
    sc = G.tube(small=True)
    rng = np.random.default_rng(17)
    Q, P, Nrm = sc["source"].copy(), sc["target"].copy(), sc["normals"].copy()
    special = np.array([np.nan, np.inf, -np.inf], np.float32)
    for A, share in ((Q, 0.05), (P, 0.05)):
        hit = rng.random(len(A)) < share
        A[hit, rng.integers(0, 3, int(hit.sum()))] = special[rng.integers(0, 3, int(hit.sum()))]
    tenth = rng.random(len(P)) < 0.1
    Nrm[tenth] = 0.0
    nan_n = tenth & (rng.random(len(P)) < 0.5)
    Nrm[nan_n, rng.integers(0, 3, int(nan_n.sum()))] = np.nan
    Q[7] = [9.0, 0.0, 1.0]                                       # more than a cell (of at least 0.3) outside the target's box
    Q[8] = [0.0, 0.0, -4.0]
    return Q, P, Nrm, sc["max_dist"]


@pytest.mark.parametrize("metric", ["plane", "point"])
def test_accumulate_with_hostile_inputs(metric):
    Q, P, Nrm, md = _hostile()
    wc = _check_accumulate(Q, P, Nrm, md, metric)
    assert wc[0] < len(Q) and wc[1] < wc[0] and (wc[2] < wc[1] if metric == "plane" else wc[2] == wc[1]) and wc[2] > 1000
    sc = G.tube(small=True)
    clean = G.accumulate(sc["source"], sc["target"], sc["normals"], START, G.pivot_of(sc["target"]), md, metric)[3]
    assert clean.tolist() == [len(Q)] * 3                        # (the special values do reach the pairs)


@pytest.mark.parametrize("metric", ["plane", "point"])
def test_accumulate_empty_sides_and_a_box_that_is_not_finite(metric):
    sc = G.tube(small=True)
    none = np.zeros((0, 3), np.float32)
    assert _check_accumulate(none, sc["target"], sc["normals"], 0.3, metric).tolist() == [0, 0, 0]
    assert _check_accumulate(sc["source"], none, none, 0.3, metric).tolist() == [len(sc["source"]), 0, 0]
    assert _check_accumulate(none, none, none, 0.3, metric).tolist() == [0, 0, 0]
    # two finite points 6e38 apart: the extent is not finite, the index is one cell, searched whole
    P, Nrm = sc["target"].copy(), sc["normals"].copy()
    P[3], P[4] = [3e38, 0.0, 0.0], [-3e38, 0.0, 0.0]
    wc = _check_accumulate(sc["source"], P, Nrm, 0.3, metric)
    assert wc.tolist() == [len(sc["source"])] * 3


# ---- 2. determinism ------------------------------------------------------------------------------------------------------- #
def _bits_equal(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                                                  y.view(torch.int64) if y.dtype == torch.float64 else y)


@pytest.mark.parametrize("metric", ["plane", "point"])
def test_deterministic_across_calls_and_streams(metric):
    from coivo_amd import evaluate as E
    sc = G.tube()
    args = (_t(sc["source"]), _t(sc["target"]))
    kw = dict(target_normals=_t(sc["normals"]), init=_init(START), max_dist=sc["max_dist"], metric=metric)
    run = lambda: (E.register_clouds(*args, iterations=4, **kw), E.register_accumulate(*args, **kw))
    a, sa = run()
    b, sb = run()
    _bits_equal(a, b)
    _bits_equal(sa, sb)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        c, sc_ = run()
    side.synchronize()
    _bits_equal(a, c)
    _bits_equal(sa, sc_)
    assert int(a.status) == G.OK and not torch.isnan(a.R).any()


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def _replica_loop(small, mode, metric):
    sc = G.tube(small=small, s_true=1.03 if mode == "sim3" else 1.0)
    return sc, G.register(sc["source"], sc["target"], sc["normals"], max_dist=sc["max_dist"], mode=mode, metric=metric, iterations=ITER)


@functools.lru_cache(maxsize=None)
def _kernel_loop(small, mode, metric):
    from coivo_amd import evaluate as E
    sc = G.tube(small=small, s_true=1.03 if mode == "sim3" else 1.0)
    return E.register_clouds(_t(sc["source"]), _t(sc["target"]), target_normals=_t(sc["normals"]), max_dist=sc["max_dist"], mode=mode,
                             metric=metric, iterations=ITER)


@pytest.mark.parametrize("metric", ["plane", "point"])
@pytest.mark.parametrize("mode", ["sim3", "se3"])
@pytest.mark.parametrize("small", [True, False], ids=["small", "full"])
def test_loop_equals_the_replica(small, mode, metric):
    sc, want = _replica_loop(small, mode, metric)
    got = _kernel_loop(small, mode, metric)
    assert got.R.is_cuda and got.R.dtype == torch.float64 and tuple(got.R.shape) == (3, 3) and tuple(got.t.shape) == (3,)
    assert got.s.dim() == 0 and got.status.dim() == 0 and got.status.dtype == torch.int32
    assert tuple(got.history.shape) == (ITER + 1, 5) and tuple(got.normal_matrix.shape) == (7, 7)
    assert int(got.status) == want["status"] == G.OK
    h, hw = got.history.cpu().numpy(), want["history"]
    assert np.array_equal(h[0, :3], hw[0, :3])                                    # the first evaluation: the same counts,
    assert np.allclose(h[0, 3:], hw[0, 3:], rtol=1e-12, atol=0)                  # the same costs
    dR = np.abs(got.R.cpu().numpy() - want["R"]).max()
    dt = np.abs(got.t.cpu().numpy() - want["t"]).max()
    ds = abs(float(got.s) - want["s"])
    print(small, mode, metric, "|R - replica|", dR, "|t - replica|", dt, "|s - replica|", ds)
    assert max(dR, dt, ds) <= 1e-6
    # no query of this input is near the reach (every point is reached at every evaluation of the replica, with room): every later
    # count is equal too
    assert np.array_equal(h[:, :3], hw[:, :3])
    assert not np.array_equal(h[-1, 3:], h[0, 3:]) and not np.array_equal(h[1, 3:], h[0, 3:])     # (the rows are distinct evaluations)
    nm = got.normal_matrix.cpu().numpy()
    assert np.array_equal(nm, nm.T) and np.allclose(nm, want["normal_matrix"], rtol=1e-6, atol=1e-6 * np.abs(want["normal_matrix"]).max())
    if mode == "se3":
        assert float(got.s) == 1.0
    R, t, s = got.transform()
    assert not R.is_cuda and R.dtype == torch.float64 and torch.equal(R, got.R.cpu()) and torch.equal(t, got.t.cpu()) and s == float(got.s)


# ---- 4. recovery ---------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("mode", ["sim3", "se3"])
def test_recovers_the_motion_as_the_replica_does(mode):
    """The kernel's largest true point error is at most twice the replica's from the same start (a rounding difference must not fail
    it; the bar is the replica's, never the kernel's own output), and the replica's own is 1/50 of the start's."""
    sc, want = _replica_loop(False, mode, "plane")
    got = _kernel_loop(False, mode, "plane")
    before = G.true_error(sc["source"], sc["truth"], *G.IDENTITY).max()
    e_want = G.true_error(sc["source"], sc["truth"], want["R"], want["t"], want["s"]).max()
    e_got = G.true_error(sc["source"], sc["truth"], got.R.cpu().numpy(), got.t.cpu().numpy(), float(got.s)).max()
    print(mode, "largest true error: start", before, "replica", e_want, "kernel", e_got)
    assert e_want <= before / 50
    assert e_got <= 2 * e_want


# ---- 5. status cases ------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("name", ["cylinder", "nearly_cylinder", "empty_target", "out_of_reach", "min_pairs"])
def test_freeze_and_revert_return_the_input_to_the_bit(name):
    from coivo_amd import evaluate as E
    Q, P, Nrm, kw, want = G.status_cases()[name]
    kw = dict(kw)
    init = kw.pop("init")
    assert G.register(Q, P, Nrm, init=init, **kw)["status"] == want
    got = E.register_clouds(_t(Q), _t(P), target_normals=_t(Nrm), init=_init(init), **kw)
    print(name, "status", int(got.status), "history", got.history.cpu().numpy()[:, :3].tolist())
    assert int(got.status) == want
    assert np.array_equal(got.R.cpu().numpy(), init[0]) and np.array_equal(got.t.cpu().numpy(), init[1]) and float(got.s) == init[2]
    if name == "cylinder":
        assert float(got.normal_matrix[2, 2]) == 0.0


# ---- 6. the reconstruction score ------------------------------------------------------------------------------------------ #
def test_reconstruction_metrics_registers_when_asked():
    from coivo_amd import _args, evaluate as E, inference as I
    sc = G.fused_scene()
    d, K, M = _t(sc["depths"]), _t(sc["K"]), _t(sc["M"])
    traj = torch.from_numpy(sc["M"]).double()
    vs = sc["voxel_size"]
    pred = _t(sc["source"])
    plain = E.reconstruction_metrics(pred, traj, d, K, traj, voxel_size=vs)           # as a caller from before would call it
    none = E.reconstruction_metrics(pred, traj, d, K, traj, voxel_size=vs, register=None)
    A = E.align_trajectory(traj, traj, "sim3")
    gt = I.fuse_point_cloud(d, K, M, voxel_size=vs)
    direct = E.cloud_metrics(pred, gt.points, max_dist=4.0 * _args.f32(vs), thresholds=(_args.f32(vs), 2.0 * _args.f32(vs)), transform=A)
    for m in (plain, none):
        assert m.registration is None and len(m) == 12
        assert tuple(m[:10]) == tuple(direct[:10])
        for a, b in ((m.pred_to_gt, direct.pred_to_gt), (m.gt_to_pred, direct.gt_to_pred)):
            assert torch.equal(a.dist2.view(torch.int32), b.dist2.view(torch.int32)) and torch.equal(a.nearest, b.nearest)
            assert torch.equal(a.stats, b.stats) and a.max_dist == b.max_dist and a.thresholds == b.thresholds
    reg = E.reconstruction_metrics(pred, traj, d, K, traj, voxel_size=vs, register=E.Registration())
    accuracy, completeness, chamfer, precision, recall, fscore, *_ = reg                  # still twelve fields
    assert isinstance(reg.registration, E.RegistrationResult) and len(reg) == 12
    assert int(reg.registration.status) == E.REGISTER_OK and tuple(reg.registration.history.shape) == (21, 5)
    print("accuracy", plain.accuracy, "->", reg.accuracy, "fscore", plain.fscore, "->", reg.fscore)
    assert reg.accuracy < plain.accuracy
    assert torch.equal(gt.points, _t(sc["target"]))                                       # (the replica's scene is the call's)
    want = G.register(sc["source"], sc["target"], sc["normals"], init=tuple(np.asarray(v, np.float64) for v in A[:2]) + (A[2],),
                      max_dist=sc["max_dist"])
    R, t, s = reg.registration.transform()
    diff = max(np.abs(R.numpy() - want["R"]).max(), np.abs(t.numpy() - want["t"]).max(), abs(s - want["s"]))
    print("|transform - replica|", diff, "status", want["status"])
    assert want["status"] == G.OK and diff <= 1e-6
    # the measures are those of the refined transform
    again = E.cloud_metrics(pred, gt.points, max_dist=4.0 * _args.f32(vs), thresholds=(_args.f32(vs), 2.0 * _args.f32(vs)), transform=(R, t, s))
    assert tuple(again[:10]) == tuple(reg[:10])


# ---- 7. argument errors that reach the device wrappers -------------------------------------------------------------------- #
def test_argument_errors_on_the_device():
    from coivo_amd import evaluate as E
    sc = G.tube(small=True)
    q, p, n = _t(sc["source"]), _t(sc["target"]), _t(sc["normals"])
    for f in (E.register_clouds, E.register_accumulate):
        with pytest.raises(ValueError, match="needs target_normals"):
            f(q, p, max_dist=0.3)
        with pytest.raises(ValueError, match="target_normals"):
            f(q, p, target_normals=n[:-1], max_dist=0.3)
        for bad in (n.cpu(), n.double(), n[:, :2]):
            with pytest.raises(ValueError):
                f(q, p, target_normals=bad, max_dist=0.3)
        for bad in ((q.cpu(), p), (q, p.cpu()), (q.double(), p), (q[:, :2], p)):
            with pytest.raises(ValueError):
                f(*bad, target_normals=n, max_dist=0.3)
        for md in (0.0, -1.0, float("nan"), float("inf"), 1e-30):
            with pytest.raises(ValueError, match="max_dist"):
                f(q, p, target_normals=n, max_dist=md)
        for init in ((np.eye(4), np.zeros(3), 1.0), (np.eye(3), np.zeros(4), 1.0), (np.eye(3), np.zeros(3)), 5,
                     (np.eye(3), np.zeros(3), float("nan")), (np.full((3, 3), np.inf), np.zeros(3), 1.0)):
            with pytest.raises(ValueError, match="init"):
                f(q, p, target_normals=n, max_dist=0.3, init=init)
        for pivot in ((0.0, 1.0), "c", np.zeros((2, 3))):
            with pytest.raises(ValueError, match="pivot"):
                f(q, p, target_normals=n, max_dist=0.3, pivot=pivot)
        with pytest.raises(ValueError, match="metric"):
            f(q, p, target_normals=n, max_dist=0.3, metric="colour")
    with pytest.raises(ValueError, match="needs target_normals"):
        E.cloud_metrics(q, p, max_dist=0.3, thresholds=(0.1,), register=E.Registration())
    # the point metric needs no normals; a pivot may be given as numbers or as a tensor
    out = E.register_clouds(q, p, max_dist=0.3, metric="point", iterations=1, pivot=(0.0, 0.0, 1.5))
    out2 = E.register_clouds(q, p, max_dist=0.3, metric="point", iterations=1, pivot=torch.tensor([0.0, 0.0, 1.5], device=dev()))
    assert int(out.status) == E.REGISTER_OK and torch.equal(out.R, out2.R) and tuple(out.history.shape) == (2, 5)
    m = E.cloud_metrics(q, p, max_dist=0.3, thresholds=(0.1,), register=E.Registration(metric="point", iterations=2))
    assert int(m.registration.status) == E.REGISTER_OK and tuple(m.registration.history.shape) == (3, 5)


# ---- memory discipline ---------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("mode", ["se3", "sim3"])
def test_memory_discipline(mode):
    """register_clouds (point to plane, eight iterations) under tests/guarded.py on the small tube: source, target and normals between
    guard bands; the target's index (colvo_cloud_workspace_bytes(0, M)), the scratch (colvo_register_scratch_bytes), the state, the
    history, the status and the normal matrix from the pool under both poisons.  The loop meets the replica as in
    test_loop_equals_the_replica, every output is the same bytes under either poison, and no guard byte changes.  Launches reached:
    colvo_cloud_index_build, and per iteration the pair search with its partial rows, the row reduction and the float64 solve, with
    the scale column in sim3."""
    from coivo_amd import _lib, evaluate as E
    from tests import guarded
    lib = _lib.load()
    sc, want = _replica_loop(True, mode, "plane")
    run = lambda pool: E.register_clouds(pool.place(_t(sc["source"])), pool.place(_t(sc["target"])), target_normals=pool.place(_t(sc["normals"])),
                                         max_dist=sc["max_dist"], mode=mode, metric="plane", iterations=ITER)
    outs, pools = guarded.under_both_poisons(dev(), run, f"register_clouds {mode}")
    for got, pool in zip(outs, pools):
        assert int(got.status) == want["status"] == G.OK
        h, hw = got.history.cpu().numpy(), want["history"]
        assert np.array_equal(h[:, :3], hw[:, :3]) and np.allclose(h[0, 3:], hw[0, 3:], rtol=1e-12, atol=0)
        d = max(np.abs(got.R.cpu().numpy() - want["R"]).max(), np.abs(got.t.cpu().numpy() - want["t"]).max(), abs(float(got.s) - want["s"]))
        assert d <= 1e-6, d
        nm = got.normal_matrix.cpu().numpy()
        assert np.array_equal(nm, nm.T) and np.allclose(nm, want["normal_matrix"], rtol=1e-6, atol=1e-6 * np.abs(want["normal_matrix"]).max())
        guarded.assert_served(pool, 0, lib.colvo_cloud_workspace_bytes(0, len(sc["target"])), "the target's index")
        guarded.assert_served(pool, 0, lib.colvo_register_scratch_bytes(len(sc["source"])), "register_clouds")
