"""No GPU: the point-cloud replica (tests/cloud_ref.py) against a float64 k-d tree, the argument checks of the colvo_cloud_* entry
points and of the Python functions, and the host arithmetic that turns the integer statistics into measures."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import cloud_ref as R

U = 2.0 ** -24            # float32 unit roundoff


@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.ensure()
    return _lib.load()


def test_replica_agrees_with_a_float64_kd_tree():
    """The replica's float32 distances against scipy's cKDTree on the same points in float64.

    Bound.  The inputs are float32 values, exact in float64.  dx = fl(qx - px) carries a relative error <= u = 2^-24 whatever the
    coordinates' magnitude (a difference of two floats is rounded once), so dx*dx carries (1+u)^3, the two sums add one factor
    each: d2_32 = d2 * (1 + t), |t| <= (1+u)^5 - 1; the correctly rounded square root halves that and adds u:
    |dist32 - dist| <= ((1+u)^3.5 - 1) * dist < 4 u dist <= 4 u max_dist for every distance the truncation keeps, and
    sqrt(fl(md*md)) lies within u * max_dist of max_dist for the ones it does not.  The tree's own float64 error at coordinates
    of magnitude 100 (1e-14) is covered by 1e-12.  BOUND = 4 u max_dist + 1e-12 = 1.19e-8 + 1e-12 at max_dist = 0.05.
    Worst observed on this input: 3.9e-9 (printed below; 0.33 of the bound).
    The reached / not reached decision may differ only where the float64 distance lies within BOUND of max_dist; the share of
    queries in that band is asserted to be below 1 % (it is 0 of 4000 here)."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(11)
    md = 0.05
    shift = np.array([100.0, -37.0, 0.001])
    P = (rng.random((3000, 3)) + shift).astype(np.float32)
    Q = (rng.random((4000, 3)) + shift).astype(np.float32)
    md32 = float(np.float32(md))
    bound = 4 * U * md32 + 1e-12
    got = R.nearest(Q, P, md, (0.02, 0.05))
    d64, i64 = cKDTree(P.astype(np.float64)).query(Q.astype(np.float64), k=1)
    reach32, reach64 = got["nearest"] >= 0, d64 < md32
    band = np.abs(d64 - md32) <= bound
    share = float(band.mean())
    print(f"queries within {bound:.3e} of max_dist: {int(band.sum())} of {len(Q)}")
    assert share < 0.01
    assert not np.any((reach32 != reach64) & ~band)
    err = np.abs(got["dist"].astype(np.float64) - np.minimum(d64, md32))[~band]
    print(f"worst |dist32 - dist64| = {err.max():.3e}, bound {bound:.3e}")
    assert err.max() <= bound
    both = reach32 & reach64
    assert 0.1 < both.mean() < 0.9
    # where float64 has one clear winner the index agrees too (near-ties may legitimately resolve differently)
    d64_at = np.linalg.norm(Q[both].astype(np.float64) - P[got["nearest"][both]].astype(np.float64), axis=1)
    assert np.all(d64_at - d64[both] <= 2 * bound)
    # the counts follow from the distances
    assert got["stats"][0] == len(Q) and got["stats"][1] == int(reach32.sum()) and got["stats"][3] == int(reach32.sum())
    assert got["stats"][2] == int((got["dist2"] < np.float32(0.02) * np.float32(0.02)).sum())


def test_replica_tie_rule_invalid_points_and_transform():
    P = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0], [np.nan, 0, 0], [0, 0, np.inf], [5, 5, 5]], np.float32)
    Q = np.array([[0, 0, 0], [1, 0, 0], [np.inf, 0, 0], [9, 9, 9], [0.5, 0.5, 0]], np.float32)
    got = R.nearest(Q, P, 1.5, (0.5, 1.0, 1.5))
    assert got["nearest"].tolist() == [0, 0, -1, -1, 0]                 # ties: the smallest index; invalid and far queries: -1
    assert got["dist2"].tolist() == [1.0, 0.0, 2.25, 2.25, 0.5]
    assert got["stats"][:5].tolist() == [4, 3, 1, 2, 3]                  # valid, reached, < 0.25, < 1 (strict), < 2.25
    s = np.float32(2 ** 20) / np.float32(1.5)
    want = sum(int(np.rint(np.float32(np.sqrt(np.float32(d)) * s))) for d in (1.0, 0.0, 2.25, 0.5))
    assert got["stats"][10] == want
    out = R.transform(np.array([[1, 2, 3]], np.float32), np.eye(3), [1, 1, 1], 2.0)
    assert out.tolist() == [[3.0, 5.0, 7.0]]


def _refused(lib, rc, *words):
    msg = lib.colvo_last_error()
    assert rc != 0, msg
    for w in words:
        assert w in msg, msg


def test_cloud_entry_points_validate_their_arguments(lib):
    """Refused before any launch, with a message (without a GPU a call that got as far as a launch would report a HIP error
    instead of the check's message)."""
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert p % 16 == 0 or (p + 8) % 16 == 0
    p = p if p % 16 == 0 else p + 8
    tau = (C.c_float * 9)(0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09)
    t = C.addressof(tau)
    # sizes
    assert lib.colvo_cloud_workspace_bytes(100, 100) > 0
    assert lib.colvo_cloud_workspace_bytes(0, 0) > 0
    assert lib.colvo_cloud_workspace_bytes(100, 1000) - lib.colvo_cloud_workspace_bytes(100, 0) == 1000 * 20
    for n, m in ((2 ** 30, 1), (1, 2 ** 30), (-1, 1), (1, -1)):
        assert lib.colvo_cloud_workspace_bytes(n, m) == 0
    # build
    _refused(lib, lib.colvo_cloud_index_build(0, 8, 0.1, p, 0), b"colvo_cloud_index_build", b"null pointer")
    _refused(lib, lib.colvo_cloud_index_build(p, 8, 0.1, 0, 0), b"colvo_cloud_index_build", b"null pointer")
    _refused(lib, lib.colvo_cloud_index_build(p, 2 ** 30, 0.1, p, 0), b"bad shape")
    _refused(lib, lib.colvo_cloud_index_build(p, -1, 0.1, p, 0), b"bad shape")
    for bad in (0.0, -1.0, math.inf, math.nan, 1e-30, 1e30):                    # 1e-30, 1e30: the square leaves float32
        _refused(lib, lib.colvo_cloud_index_build(p, 8, bad, p, 0), b"bad max_dist")
    _refused(lib, lib.colvo_cloud_index_build(p, 8, 0.1, p + 4, 0), b"16-byte aligned")
    # query
    q = lambda **kw: lib.colvo_cloud_query(*[kw.get(k, d) for k, d in (
        ("query", p), ("N", 4), ("M", 4), ("max_dist", 0.1), ("tau", t), ("n_tau", 3), ("ws", p), ("dist", p), ("dist2", p),
        ("nearest", p), ("stats", p), ("stream", 0))])
    for name in ("query", "ws", "dist", "dist2", "nearest", "stats", "tau"):
        _refused(lib, q(**{name: 0}), b"colvo_cloud_query", b"null pointer")
    _refused(lib, q(N=2 ** 30), b"bad shape")
    _refused(lib, q(M=2 ** 30), b"bad shape")
    for bad in (0.0, -0.1, math.inf, math.nan):
        _refused(lib, q(max_dist=bad), b"bad max_dist")
    _refused(lib, q(n_tau=9), b"bad thresholds")
    _refused(lib, q(n_tau=-1), b"bad thresholds")
    _refused(lib, q(max_dist=0.025), b"bad thresholds", b"tau[2]")                # 0.03 above max_dist
    _refused(lib, q(tau=C.addressof((C.c_float * 3)(0.02, 0.01, 0.03))), b"bad thresholds", b"tau[1]")       # descending
    _refused(lib, q(tau=C.addressof((C.c_float * 3)(0.0, 0.01, 0.03))), b"bad thresholds", b"tau[0]")        # not positive
    _refused(lib, q(tau=C.addressof((C.c_float * 3)(0.01, math.nan, 0.03))), b"bad thresholds", b"tau[1]")
    _refused(lib, q(ws=p + 4), b"16-byte aligned")
    # transform
    _refused(lib, lib.colvo_cloud_transform(p, 4, 0, p, 0), b"colvo_cloud_transform", b"null pointer")
    _refused(lib, lib.colvo_cloud_transform(0, 4, p, p, 0), b"null pointer")
    _refused(lib, lib.colvo_cloud_transform(p, 4, p, 0, 0), b"null pointer")
    _refused(lib, lib.colvo_cloud_transform(p, 2 ** 30, p, p, 0), b"bad shape")
    # an empty cloud to transform needs neither pointer nor device
    assert lib.colvo_cloud_transform(0, 0, p, 0, 0) == 0


def test_python_functions_refuse_what_the_kernels_cannot_take():
    from coivo_amd import _args, evaluate as E
    ok = torch.zeros(4, 3)
    for bad in (ok, ok.double(), torch.zeros(4, 2), torch.zeros(3), torch.zeros(2, 4, 3), [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError, match="float32 CUDA tensor of shape"):
            E.nearest_neighbors(bad, bad, max_dist=0.1)
        with pytest.raises(ValueError, match="float32 CUDA tensor of shape"):
            E.cloud_metrics(bad, bad, max_dist=0.1, thresholds=(0.05,))
        with pytest.raises(ValueError, match="float32 CUDA tensor of shape"):
            E.transform_cloud(bad, torch.eye(3), torch.zeros(3), 1.0)
        with pytest.raises(ValueError, match="float32 CUDA tensor of shape"):
            E.reconstruction_metrics(bad, torch.eye(4)[None], torch.zeros(1, 1, 8, 8), torch.eye(3)[None], torch.eye(4)[None],
                                     voxel_size=0.1)
    assert _args.reach("x", 0.08, (0.02, 0.04, 0.08)) == (_args.f32(0.08), (_args.f32(0.02), _args.f32(0.04), _args.f32(0.08)))
    assert _args.reach("x", 1, ()) == (1.0, ())
    for md in (0.0, -1.0, math.inf, math.nan, 1e-30, 1e30, 1e300, "a", None):
        with pytest.raises(ValueError, match="max_dist"):
            _args.reach("x", md, ())
    for th in ((0.02, 0.01), (0.0,), (-0.1,), (0.2,), (math.nan,), tuple([0.01] * 9), ("a",)):
        with pytest.raises(ValueError, match="thresholds"):
            _args.reach("x", 0.1, th)


def test_measures_from_hand_made_statistics():
    from coivo_amd import _args, evaluate as E
    md = _args.f32(0.08)
    s = float(np.float32(2 ** 20) / np.float32(0.08))
    assert _args.f32(1048576.0 / md) == s                  # the Python side's scale is the float32 quotient
    pred = [10, 8, 2, 5, 0, 0, 0, 0, 0, 0, 3 * 2 ** 20, 123]
    gt = [20, 20, 5, 20, 0, 0, 0, 0, 0, 0, 5 * 2 ** 20, 456]
    m = E.metrics_from_stats(pred, gt, md, 2)
    assert m["accuracy"] == (3 * 2 ** 20) / (s * 10) and m["completeness"] == (5 * 2 ** 20) / (s * 20)
    assert abs(m["accuracy"] - 0.3 * 0.08) < 1e-8
    assert m["chamfer"] == 0.5 * (m["accuracy"] + m["completeness"])
    assert m["precision"] == (0.2, 0.5) and m["recall"] == (0.25, 1.0)
    assert m["fscore"] == (2.0 * 0.2 * 0.25 / (0.2 + 0.25), 2.0 * 0.5 * 1.0 / (0.5 + 1.0))
    assert (m["n_pred"], m["n_gt"], m["n_pred_reached"], m["n_gt_reached"]) == (10, 20, 8, 20)
    # nothing under a threshold on either side: F-score 0, not 0 / 0
    z = E.metrics_from_stats([10, 0] + [0] * 8 + [10 * 2 ** 20, 0], [4, 0] + [0] * 8 + [4 * 2 ** 20, 0], md, 1)
    assert z["precision"] == (0.0,) and z["recall"] == (0.0,) and z["fscore"] == (0.0,)
    assert abs(z["accuracy"] - 0.08) < 1e-8 and abs(z["chamfer"] - 0.08) < 1e-8
    # an empty side: NaN for what divides by its count, the other side's measures stand
    e = E.metrics_from_stats([0] * 12, gt, md, 2)
    assert math.isnan(e["accuracy"]) and math.isnan(e["chamfer"]) and e["completeness"] == m["completeness"]
    assert all(math.isnan(v) for v in e["precision"]) and e["recall"] == (0.25, 1.0) and all(math.isnan(v) for v in e["fscore"])
    e = E.metrics_from_stats(pred, [0] * 12, md, 2)
    assert math.isnan(e["completeness"]) and e["accuracy"] == m["accuracy"] and all(math.isnan(v) for v in e["recall"])
    assert E.metrics_from_stats(pred, gt, md, 0)["fscore"] == ()
    # the replica's host arithmetic is the same
    assert R.mean_distance(np.array(pred[:11]), np.float32(s)) == m["accuracy"]


def _emulated_misses(Q, P, md, margin):
    """The kernel's cell rule in NumPy -- origin = the box's lower corner, edge = max(max_dist * margin, extent / 126),
    cell = floor((x - o) * (1 / edge)), all float32 -- and how many reached queries have their nearest point (the gridless
    replica's) more than one cell away on some axis: those a walk over the 27 cells around the query's would miss."""
    f32 = np.float32
    want = R.nearest(Q, P, md)
    o = P.min(axis=0)
    edge = max(f32(f32(md) * f32(margin)), f32((P.max(axis=0) - o).max() / f32(126)))
    inv = f32(1) / edge
    cq, cp = np.floor((Q - o) * inv).astype(np.int64), np.floor((P - o) * inv).astype(np.int64)
    reached = want["nearest"] >= 0
    return int((np.abs(cq[reached] - cp[want["nearest"][reached]]).max(axis=1) > 1).sum()), int(reached.sum())


@pytest.mark.parametrize("md", R.LATTICE_MAX_DISTS)
def test_lattice_catches_a_cell_edge_of_exactly_max_dist(md):
    """The GPU lattice test has teeth: with a cell edge of exactly max_dist the float32 cell index puts the nearest point of some
    queries two cells away at max_dist 0.013 and 0.083 (160 queries each; none at 0.0625, where 1 / edge is exact, nor at 0.05),
    and with the library's margin of 2^-10 at none of the four."""
    Q, P, _ = R.lattice(md, 7)
    missed, reached = _emulated_misses(Q, P, md, 1.0)
    print(f"max_dist {md}: {missed} of {reached} reached queries miss their nearest point at edge = max_dist")
    assert (missed > 0) == (md in (0.013, 0.083))
    assert _emulated_misses(Q, P, md, 1.0 + 2.0 ** -10)[0] == 0
