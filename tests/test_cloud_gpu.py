"""-m gpu: the truncated nearest-neighbour search and the cloud measures (coivo_amd.evaluate, csrc/cloud.hip) against their NumPy
replica (tests/cloud_ref.py).  The arithmetic is pinned (float32, one rounding per operation), the minimum does not depend on the
order it is taken in and every sum is an integer, so every comparison here is equality to the bit: no tolerance, no excused point."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import cloud_ref as R
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

f32 = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _nn(Q, P, md, th=()):
    from coivo_amd import evaluate as E
    return E.nearest_neighbors(_t(np.asarray(Q, f32).reshape(-1, 3)), _t(np.asarray(P, f32).reshape(-1, 3)), max_dist=md, thresholds=th)


def _assert_equal(got, want, what=""):
    """CloudNN against the replica's dict: dist2 and dist bit for bit, nearest, every count and the 64-bit sum."""
    n = want["dist2"].shape[0]
    assert got.dist2.shape == (n,) and got.dist2.dtype == torch.float32, what
    assert got.dist.shape == (n,) and got.dist.dtype == torch.float32, what
    assert got.nearest.shape == (n,) and got.nearest.dtype == torch.int32, what
    assert got.stats.shape == (12,) and got.stats.dtype == torch.int64, what
    assert torch.equal(_bits(got.dist2).cpu(), _bits(torch.from_numpy(want["dist2"]))), what
    assert torch.equal(_bits(got.dist).cpu(), _bits(torch.from_numpy(want["dist"]))), what
    assert torch.equal(got.nearest.cpu(), torch.from_numpy(want["nearest"])), what
    assert torch.equal(got.stats[:R.STATS].cpu(), torch.from_numpy(want["stats"])), (what, got.stats.tolist(), want["stats"].tolist())


def _same(a, b):
    """Two CloudNNs: identical bits, the cost figure included."""
    for x, y in zip(a[:3], b[:3]):
        assert x.shape == y.shape and torch.equal(_bits(x), _bits(y))
    assert torch.equal(a.stats, b.stats)


def _check(Q, P, md, th=(), what=""):
    want = R.nearest(Q, P, md, th)
    got = _nn(Q, P, md, th)
    _assert_equal(got, want, what)
    return got, want


# ---- random clouds --------------------------------------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=1)
def _random_clouds():
    rng = np.random.default_rng(3)
    return rng.random((3000, 3)).astype(f32), rng.random((2500, 3)).astype(f32)


def test_random_clouds_equal_the_replica_both_ways():
    """20^3 = 8000 cells: more than one 4096-entry scan chunk.  Expected unreached share exp(-2500 * 4 pi / 3 * 0.05^3) = 27 %."""
    Q, P = _random_clouds()
    th = (0.02, 0.035, 0.05)
    for a, b in ((Q, P), (P, Q)):
        got, want = _check(a, b, 0.05, th)
        unreached = 1.0 - want["stats"][1] / want["stats"][0]
        assert 0.1 < unreached < 0.9, unreached                   # both branches carry weight
        assert want["stats"][0] == len(a) and want["stats"][2] < want["stats"][3] < want["stats"][4] == want["stats"][1]
        assert int(got.stats[11]) > 0


# ---- lattice: a cell edge of exactly max_dist fails here --------------------------------------------------------------------- #
@pytest.mark.parametrize("md", R.LATTICE_MAX_DISTS)
def test_lattice_at_the_reach_boundary(md):
    """tests/test_cloud_cpu.py shows, by emulating the cell rule, that at 0.013 and 0.083 a cell edge of exactly max_dist puts the
    nearest point of 160 of these queries two cells away."""
    Q, P, empty = R.lattice(md, 7)
    got, want = _check(Q, P, md, (md / 2, md))
    reached = want["nearest"] >= 0
    # the replica puts a fair part of the boundary queries on either side, so a missed neighbour cell cannot hide
    assert 0.05 < reached[empty].mean() < 0.95, reached[empty].mean()
    assert reached[~empty].mean() > 0.5
    got2, _ = _check(P, Q, md, (md,))
    assert int(got2.stats[0]) == len(P)


# ---- ties and zeros --------------------------------------------------------------------------------------------------------- #
def test_ties_return_the_smallest_index_and_equal_points_give_zero():
    rng = np.random.default_rng(5)
    base = rng.random((500, 3)).astype(f32)
    P = np.concatenate([base, base[::3], base[:100]])             # every third point twice, the first hundred up to three times
    Q = np.concatenate([base[:200], rng.random((300, 3)).astype(f32)])
    got, want = _check(Q, P, 0.1, (0.05, 0.1))
    assert want["nearest"][:200].tolist() == list(range(200))
    assert torch.equal(got.nearest[:200].cpu(), torch.arange(200, dtype=torch.int32))
    assert torch.count_nonzero(got.dist2[:200]) == 0 and torch.count_nonzero(got.dist[:200]) == 0


def test_one_point_repeated_fills_one_cell_beyond_a_workgroup():
    rng = np.random.default_rng(6)
    p = np.array([0.3, -0.2, 1.5], f32)
    P = np.tile(p, (5000, 1))
    Q = np.concatenate([p[None], p[None] + (rng.random((700, 3)).astype(f32) - f32(0.5)) * f32(0.3)])
    got, want = _check(Q, P, 0.1, (0.1,))
    reached = want["nearest"] >= 0
    assert 0.05 < reached.mean() < 0.95 and set(want["nearest"][reached].tolist()) == {0}
    assert float(got.dist2[0]) == 0.0 and int(got.nearest[0]) == 0
    examined = int(got.stats[11])                                  # a query walks the one cell whole or not at all
    assert examined % 5000 == 0 and 5000 * int(reached.sum()) <= examined <= 5000 * len(Q)
    _check(P[:300], Q, 0.1, (0.05,))


# ---- shapes that break indexing ---------------------------------------------------------------------------------------------- #
def test_a_grid_of_one_cell():
    rng = np.random.default_rng(8)
    P = (f32(0.5) + (rng.random((400, 3)).astype(f32) - f32(0.5)) * f32(0.01)).astype(f32)
    Q = (f32(0.5) + (rng.random((500, 3)).astype(f32) - f32(0.5)) * f32(0.2)).astype(f32)
    got, want = _check(Q, P, 0.05, (0.01, 0.05))
    assert 0 < want["stats"][1] < want["stats"][0]
    _check(P, P[:1], 0.05)                                        # a reference cloud of one point: a box of no extent
    _check(P[:1], P, 0.05)


def test_a_flat_grid():
    """4 x 4 x 0.02 at max_dist 0.05: 80 x 80 cells, one cell thick."""
    rng = np.random.default_rng(9)
    size = np.array([4.0, 4.0, 0.02], f32)
    P = rng.random((3000, 3)).astype(f32) * size
    Q = rng.random((3100, 3)).astype(f32) * size
    for perm in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):                 # the thin axis in every place
        got, want = _check(Q[:, perm], P[:, perm], 0.05, (0.025,))
        assert 0.1 < want["stats"][1] / want["stats"][0] < 0.9


@functools.lru_cache(maxsize=1)
def _large_clouds():
    rng = np.random.default_rng(10)
    Q, P = rng.random((65537, 3)).astype(f32), rng.random((70001, 3)).astype(f32)
    return Q, P, R.nearest(Q, P, 0.02, (0.01, 0.02))


def test_sizes_across_2_16_and_no_multiple_of_the_workgroup():
    Q, P, want = _large_clouds()
    got = _nn(Q, P, 0.02, (0.01, 0.02))
    _assert_equal(got, want)
    assert 0.1 < want["stats"][1] / want["stats"][0] < 0.9
    assert int(want["nearest"].max()) > 65536


def test_queries_far_outside_the_reference_box():
    rng = np.random.default_rng(12)
    md = 0.05
    P = rng.random((800, 3)).astype(f32)
    Q = []
    for off in (0.5 * md, 0.99 * md, 1.5 * md, 2.5 * md, 10.0, 1e6, 1e30, 3e38):
        for a in range(3):
            for side in (-1.0, 1.0):
                q = rng.random((40, 3)).astype(f32)
                q[:, a] = (q[:, a] * f32(0.02) + (f32(1.0 + off) if side > 0 else f32(-off) - f32(0.02))).astype(f32)
                Q.append(q)
    Q.append(np.full((5, 3), 3e38, f32) * np.array([[1, 1, 1], [-1, 1, 1], [1, -1, -1], [-1, -1, -1], [1, -1, 1]], f32))
    Q = np.concatenate(Q)
    got, want = _check(Q, P, md, (md,))
    assert 0 < want["stats"][1] < 0.5 * want["stats"][0]
    _check(P, Q, md, (md,))                                        # ... and as the reference: a box of 6e38, searched as one cell


def test_empty_clouds():
    rng = np.random.default_rng(13)
    Q = rng.random((300, 3)).astype(f32)
    none = np.zeros((0, 3), f32)
    md = 0.05
    got, want = _check(Q, none, md, (0.01,))
    assert torch.all(got.nearest == -1) and torch.all(got.dist2 == float(f32(md) * f32(md)))
    assert got.stats.tolist() == [300, 0, 0, 0, 0, 0, 0, 0, 0, 0, 300 * 2 ** 20, 0]
    got, want = _check(none, Q, md, (0.01,))
    assert got.dist.shape == (0,) and got.stats.tolist() == [0] * 12
    got, want = _check(none, none, md)
    assert got.stats.tolist() == [0] * 12


# ---- non-finite points ------------------------------------------------------------------------------------------------------- #
def test_non_finite_points_are_counted_and_take_no_part():
    rng = np.random.default_rng(14)
    Q, P = rng.random((1500, 3)).astype(f32), rng.random((1200, 3)).astype(f32)
    bad = [np.nan, np.inf, -np.inf]
    qb, pb = rng.choice(len(Q), 90, replace=False), rng.choice(len(P), 120, replace=False)
    for n, i in enumerate(qb):
        Q[i, n % 3] = bad[(n // 3) % 3]
    for n, i in enumerate(pb):
        P[i, n % 3] = bad[(n // 3) % 3]
    P[pb[0]] = np.nan
    Q[qb[0]] = -np.inf
    md, th = 0.06, (0.03, 0.06)
    got, want = _check(Q, P, md, th)
    assert int(got.stats[0]) == len(Q) - 90
    assert not np.isin(got.nearest.cpu().numpy(), pb).any()
    assert torch.all(got.nearest[_t(qb)] == -1) and torch.all(_bits(got.dist2[_t(qb)]) == int(f32(f32(md) * f32(md)).view(np.int32)))
    # the same clouds with those rows removed: everything else unchanged, the indices mapped
    keep_q, keep_p = np.setdiff1d(np.arange(len(Q)), qb), np.setdiff1d(np.arange(len(P)), pb)
    clean = _nn(Q[keep_q], P[keep_p], md, th)
    kq = _t(keep_q)
    assert torch.equal(_bits(clean.dist2), _bits(got.dist2[kq])) and torch.equal(_bits(clean.dist), _bits(got.dist[kq]))
    mapped = torch.where(clean.nearest >= 0, _t(keep_p.astype(np.int32))[clean.nearest.clamp(min=0).long()], clean.nearest)
    assert torch.equal(mapped, got.nearest[kq])
    assert torch.equal(clean.stats[:11], got.stats[:11])
    got, want = _check(P, Q, md, th)                               # the other direction
    assert int(got.stats[0]) == len(P) - 120


# ---- determinism ------------------------------------------------------------------------------------------------------------ #
def test_two_calls_a_side_stream_and_a_permuted_reference_give_the_same_bits():
    rng = np.random.default_rng(15)
    Q = rng.random((5000, 3)).astype(f32)
    P = np.unique(rng.random((4000, 3)).astype(f32), axis=0)      # no duplicates: no query can have tied candidates of one point
    md, th = 0.05, (0.02, 0.05)
    want = R.nearest(Q, P, md, th)
    a = _nn(Q, P, md, th)
    _assert_equal(a, want)
    b = _nn(Q, P, md, th)
    _same(a, b)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = _nn(Q, P, md, th)
    side.synchronize()
    _same(a, c)
    perm = rng.permutation(len(P))
    d = _nn(Q, P[perm], md, th)
    # exact only where no query has two nearest candidates at the same d2: the replica says which
    want_p = R.nearest(Q, P[perm], md, th)
    no_tie = torch.from_numpy(np.where(want_p["nearest"] >= 0, perm[np.maximum(want_p["nearest"], 0)], -1) == want["nearest"])
    assert no_tie.float().mean() > 0.999
    mapped = torch.where(d.nearest >= 0, _t(perm.astype(np.int32))[d.nearest.clamp(min=0).long()], d.nearest).cpu()
    assert torch.equal(mapped[no_tie], a.nearest.cpu()[no_tie])
    assert torch.equal(_bits(d.dist2), _bits(a.dist2)) and torch.equal(_bits(d.dist), _bits(a.dist)) and torch.equal(d.stats, a.stats)


# ---- measures --------------------------------------------------------------------------------------------------------------- #
MEASURES = ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore", "n_pred", "n_gt", "n_pred_reached", "n_gt_reached")


def _assert_metrics(got, want, what=""):
    for k in MEASURES:
        g, w = getattr(got, k), want[k]
        g, w = (g, w) if isinstance(w, tuple) else ((g,), (w,))
        assert len(g) == len(w), (what, k, g, w)
        for x, y in zip(g, w):                                     # equal, NaN where the replica has NaN
            assert x == y or (isinstance(y, float) and math.isnan(y) and math.isnan(x)), (what, k, g, w)
    _assert_equal(got.pred_to_gt, want["pred_to_gt"], what)
    _assert_equal(got.gt_to_pred, want["gt_to_pred"], what)


def test_cloud_metrics_equal_the_replica_and_are_symmetric():
    from coivo_amd import evaluate as E
    Q, P = _random_clouds()
    A, B = Q[:1700], (P[:1500] + f32(0.004)).astype(f32)
    th = (0.01, 0.03, 0.05)
    ab = E.cloud_metrics(_t(A), _t(B), max_dist=0.05, thresholds=th)
    ba = E.cloud_metrics(_t(B), _t(A), max_dist=0.05, thresholds=th)
    _assert_metrics(ab, R.metrics(A, B, 0.05, th))
    assert ab.accuracy == ba.completeness and ab.completeness == ba.accuracy and ab.chamfer == ba.chamfer
    assert ab.precision == ba.recall and ab.recall == ba.precision and ab.fscore == ba.fscore
    assert 0.0 < ab.accuracy < 0.05 and 0.0 < ab.precision[0] < ab.precision[2] < 1.0
    # an empty side
    none = torch.zeros(0, 3, device=dev())
    e = E.cloud_metrics(none, _t(B), max_dist=0.05, thresholds=th)
    _assert_metrics(e, R.metrics(np.zeros((0, 3), f32), B, 0.05, th))
    assert math.isnan(e.accuracy) and math.isnan(e.chamfer) and abs(e.completeness - 0.05) < 1e-7 and e.recall == (0.0, 0.0, 0.0)
    assert all(math.isnan(v) for v in e.precision + e.fscore)


def _sim3():
    ax = np.array([0.3, -0.5, 0.8])
    ax /= np.linalg.norm(ax)
    ang = 0.7
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + math.sin(ang) * Kx + (1 - math.cos(ang)) * Kx @ Kx
    return Rm, np.array([0.4, -1.1, 2.3]), 1.37


def test_cloud_metrics_with_a_transform_equal_the_replica_on_its_pinned_transform():
    from coivo_amd import evaluate as E
    Q, P = _random_clouds()
    Rm, t, s = _sim3()
    gt = P[:1500]
    # pred: gt, perturbed, seen through the inverse map, so that the transform brings it back
    rng = np.random.default_rng(16)
    near = gt.astype(np.float64) + rng.normal(0, 0.01, gt.shape)
    pred = (((near - t) / s) @ Rm).astype(f32)                   # R^T (x - t) / s
    th = (0.01, 0.02)
    want = R.metrics(pred, gt, 0.04, th, transform_=(Rm, t, s))
    got = E.cloud_metrics(_t(pred), _t(gt), max_dist=0.04, thresholds=th, transform=(torch.from_numpy(Rm), torch.from_numpy(t), s))
    _assert_metrics(got, want)
    assert 0.2 < got.precision[0] < 0.99
    moved = E.transform_cloud(_t(pred), Rm, t, s)
    assert torch.equal(_bits(moved).cpu(), _bits(torch.from_numpy(R.transform(pred, Rm, t, s))))


# ---- end to end ------------------------------------------------------------------------------------------------------------- #
def test_reconstruction_metrics_end_to_end():
    from coivo_amd import _args, evaluate as E, inference as I
    from tests import fuse_ref
    depths, _, K, M = fuse_ref.scene(6, 32, 40, 5)
    vs = 0.1
    d, Kt, Mt = _t(depths), _t(K), _t(M)
    traj = torch.from_numpy(M).double()
    gt = I.fuse_point_cloud(d, Kt, Mt, voxel_size=vs)
    assert gt.points.shape[0] > 1000
    # the ground truth against itself
    m = E.reconstruction_metrics(gt, traj, d, Kt, traj, voxel_size=vs)
    assert m.accuracy == 0.0 and m.completeness == 0.0 and m.chamfer == 0.0
    assert m.precision == (1.0, 1.0) and m.recall == (1.0, 1.0) and m.fscore == (1.0, 1.0)
    assert m.n_pred == m.n_gt == m.n_pred_reached == m.n_gt_reached == gt.points.shape[0]
    assert m.pred_to_gt.max_dist == _args.f32(4 * _args.f32(vs)) and m.pred_to_gt.thresholds == (_args.f32(vs), _args.f32(2 * _args.f32(vs)))
    # depths 3 % too deep, no alignment
    pred = I.fuse_point_cloud((d * 1.03).contiguous(), Kt, Mt, voxel_size=vs)
    m = E.reconstruction_metrics(pred, traj, d, Kt, traj, voxel_size=vs, align="none")
    want = R.metrics(pred.points.cpu().numpy(), gt.points.cpu().numpy(), _args.f32(4 * _args.f32(vs)), (_args.f32(vs), _args.f32(2 * _args.f32(vs))))
    _assert_metrics(m, want)
    assert 0.0 < m.accuracy < 0.4 and 0.0 < m.fscore[0] < 1.0
    # the prediction in another Sim(3) frame: trajectory and cloud moved by the same map
    Rm, t, s = _sim3()
    inv_s = 1.0 / s
    moved_traj = traj.clone()
    Rt = torch.from_numpy(Rm)
    moved_traj[:, :3, :3] = Rt.T @ traj[:, :3, :3]
    moved_traj[:, :3, 3] = ((traj[:, :3, 3] - torch.from_numpy(t)) * inv_s) @ Rt
    moved = ((pred.points.cpu().double() - torch.from_numpy(t)) * inv_s) @ Rt
    moved = moved.float().contiguous()
    m = E.reconstruction_metrics(moved.to(dev()), moved_traj, d, Kt, traj, voxel_size=vs)
    A = E.align_trajectory(moved_traj, traj, "sim3")
    assert abs(A[2] - s) < 1e-9
    want = R.metrics(moved.numpy(), gt.points.cpu().numpy(), _args.f32(4 * _args.f32(vs)), (_args.f32(vs), _args.f32(2 * _args.f32(vs))),
                     transform_=(A[0].numpy(), A[1].numpy(), A[2]))
    _assert_metrics(m, want)
    assert 0.0 < m.accuracy < 0.4


# ---- memory discipline ------------------------------------------------------------------------------------------------------- #
def test_memory_discipline():
    """nearest_neighbors under tests/guarded.py, both directions of the random clouds (3000 and 2500 points, 8000 cells: more than one
    scan chunk): query and reference between guard bands; the workspace (colvo_cloud_workspace_bytes: the grid, the cell offsets, the
    sorted points), dist, dist2, nearest and the statistics from the pool under both poisons.  Outputs equal the replica, are the same
    bytes under either poison, and no guard byte changes.  Launches reached: the bounding box, the cell count, the scan over two
    chunks, the scatter and the query with three thresholds."""
    from coivo_amd import _lib, evaluate as E
    from tests import guarded as G
    Q, P = _random_clouds()
    th = (0.02, 0.035, 0.05)
    for a, b in ((Q, P), (P, Q)):
        want = R.nearest(a, b, 0.05, th)
        outs, pools = G.under_both_poisons(dev(), lambda pool: E.nearest_neighbors(pool.place(_t(a)), pool.place(_t(b)), max_dist=0.05,
                                                                                  thresholds=th), f"nearest_neighbors {len(a)} -> {len(b)}")
        for got, pool in zip(outs, pools):
            _assert_equal(got, want, len(a))
            G.assert_served(pool, 0, _lib.load().colvo_cloud_workspace_bytes(len(a), len(b)), "nearest_neighbors")
