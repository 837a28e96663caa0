"""No GPU: the point-to-surface replica (tests/surface_ref.py) against exact rational arithmetic, points made on the faces, the cell
rule of csrc/surface.hip emulated in NumPy against the gridless search, the host arithmetic from the statistics to the measures, and
the argument checks of the colvo_surface_* entry points and of the Python functions."""
import ctypes as C
import math
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

from tests import cloud_ref
from tests import surface_ref as S
from tests import topology_ref as T

f32, f64 = np.float32, np.float64
U64 = 2.0 ** -53
U32 = 2.0 ** -24


# ---- 1. exact rational check --------------------------------------------------------------------------------------------------------- #
def _fr(v):
    return tuple(Fr(float(x)) for x in v)


def _fsub(u, v):
    return tuple(x - y for x, y in zip(u, v))


def _fdot(u, v):
    return sum(x * y for x, y in zip(u, v))


def _fcross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _exact_segment(p, a, b):
    ab = _fsub(b, a)
    ee = _fdot(ab, ab)
    t = Fr(0) if ee == 0 else min(max(_fdot(_fsub(p, a), ab) / ee, Fr(0)), Fr(1))
    d = _fsub(p, tuple(x + t * e for x, e in zip(a, ab)))
    return _fdot(d, d)


def exact_d2(p, a, b, c):
    """The true squared distance from p to triangle (a, b, c), exact: the region-by-region closest point (Ericson, Real-Time Collision
    Detection 5.1.5: vertex, edge and face regions from six dot products) -- not the replica's candidates.  A triangle without area has
    no regions: the minimum over its three segments."""
    p, a, b, c = _fr(p), _fr(a), _fr(b), _fr(c)
    ab, ac, ap = _fsub(b, a), _fsub(c, a), _fsub(p, a)
    if all(x == 0 for x in _fcross(ab, ac)):
        return min(_exact_segment(p, a, b), _exact_segment(p, b, c), _exact_segment(p, c, a))
    d1, d2 = _fdot(ab, ap), _fdot(ac, ap)
    if d1 <= 0 and d2 <= 0:
        q = a
    else:
        bp = _fsub(p, b)
        d3, d4 = _fdot(ab, bp), _fdot(ac, bp)
        cp = _fsub(p, c)
        d5, d6 = _fdot(ab, cp), _fdot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        if d3 >= 0 and d4 <= d3:
            q = b
        elif vc <= 0 and d1 >= 0 and d3 <= 0:
            q = tuple(x + (d1 / (d1 - d3)) * e for x, e in zip(a, ab))
        elif d6 >= 0 and d5 <= d6:
            q = c
        elif vb <= 0 and d2 >= 0 and d6 <= 0:
            q = tuple(x + (d2 / (d2 - d6)) * e for x, e in zip(a, ac))
        elif va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
            w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
            q = tuple(x + w * (y - x) for x, y in zip(b, c))
        else:
            den = va + vb + vc
            v, w = vb / den, vc / den
            q = tuple(x + v * e + w * g for x, e, g in zip(a, ab, ac))
    d = _fsub(p, q)
    return _fdot(d, d)


def _up(x):
    """an upper bound of sqrt(x) for a Fraction x, as a Fraction"""
    return Fr(math.sqrt(float(x)) * (1.0 + 2.0 ** -40) + 5e-324)


def distance_bound(p, a, b, c):
    """B with |sqrt(d2_replica) - D| <= B, D the true distance, for float32 inputs whose differences are exact in float64 (asserted by the
    caller).  u = 2^-53.  L = max(|p - a|, |p - b|, |p - c|) bounds every w and, doubled, every edge; M = the largest coordinate
    magnitude.

    Segment candidates.  ee carries 3 roundings on positive terms, we an absolute error <= 3u |w||e|, the quotient one more rounding:
    |t^ - t*| <= 7u |w| / |e|, and t^ lies in [0, 1] exactly, so q(t^) is a point of the segment within 7u |w| of the true closest one.
    q^_j = fl(u_j + fl(t^ e_j)) is within 2u (M + |e|) of q(t^)_j, d_j = fl(p_j - q^_j) and the three-term sum add 2.5u relative on the
    distance: <= 8u (L + M) in all, counting |e| <= 2L.

    Plane candidate.  Each component of n = ab x ac is two rounded products and a rounded difference: |dn| <= 6u |ab||ac|.  With
    kappa = max_ij |e_i||e_j| / |n| (1 / the sine of the sharpest corner, >= 1) the computed normal is tilted by at most 12u kappa, which
    moves the plane distance n.pa / |n| by at most 12u kappa L; h and s add 3u L each from their own roundings, the product and the
    quotient 2u relative: (12 kappa + 8) u L.  The edge tests T_i = |n||e_i| rho_i (rho_i: the in-plane distance of p's projection
    from edge line i) carry an error of (6 kappa + 4) u |n||e_i||w|, so the plane candidate can be taken or dropped wrongly only with
    |rho_i| <= (6 kappa + 4) u L; such a projection lies within rho_i * kappa of the triangle (a wedge of opening alpha holds it within
    rho / sin alpha of the corner), so the true distance differs from the plane distance by at most (6 kappa + 4) kappa u L.
    Sum: (6 kappa^2 + 16 kappa + 12) u L <= 16 (kappa^2 + 1) u L for kappa >= 1.

    B = 8u (2 kappa^2 + 3) (L + M); kappa = 0 for a triangle whose exact normal is zero (the computed one is then zero too: equal
    products round alike)."""
    P, A, Bv, Cv = _fr(p), _fr(a), _fr(b), _fr(c)
    e = (_fsub(Bv, A), _fsub(Cv, Bv), _fsub(A, Cv))
    n2 = _fdot(_fcross(e[0], _fsub(Cv, A)), _fcross(e[0], _fsub(Cv, A)))
    k2 = Fr(0)
    if n2 != 0:
        l2 = [_fdot(x, x) for x in e]
        k2 = max(l2[0] * l2[1], l2[1] * l2[2], l2[0] * l2[2]) / n2
    L = max(_up(_fdot(_fsub(P, v), _fsub(P, v))) for v in (A, Bv, Cv))
    M = max(abs(x) for v in (P, A, Bv, Cv) for x in v)
    return 8 * Fr(U64) * (2 * k2 + 3) * (L + M)


def _differences_exact(p, a, b, c):
    pts = [np.asarray(v, f32).astype(f64) for v in (p, a, b, c)]
    for i in range(4):
        for j in range(i):
            for x, y in zip(pts[i], pts[j]):
                if Fr(float(x)) - Fr(float(y)) != Fr(float(x - y)):
                    return False
    return True


def _cases():
    """(p, a, b, c) float32 rows: random triangles of every size around random points, and the adversarial ones"""
    rng = np.random.default_rng(21)
    out = []
    for k in range(240):
        centre = rng.uniform(-1, 1, 3) * (100.0 if k % 3 == 0 else 1.0)
        size = 10.0 ** rng.uniform(-3, 0)
        tri = centre + rng.normal(0, size, (3, 3))
        p = centre + rng.normal(0, size * 10.0 ** rng.uniform(-2, 0.5), 3)
        out.append((p, *tri))
    for k in range(40):                                                      # needles: a short side of 1e-5 .. 1e-2 of the long ones
        a = rng.uniform(-1, 1, 3)
        d = rng.normal(0, 1, 3)
        b = a + d
        c = a + d * rng.uniform(0.2, 0.9) + rng.normal(0, 10.0 ** rng.uniform(-5, -2), 3)
        out.append((a + d * rng.uniform(-0.2, 1.2) + rng.normal(0, 0.05, 3), a, b, c))
    g = lambda *v: np.array(v, f64)
    a, b, c = g(0, 0, 0), g(1, 0, 0), g(0, 1, 0)
    out += [(g(0.25, 0.25, 0), a, b, c), (g(0.25, 0.25, 0.5), a, b, c), (g(0.5, 0, 0), a, b, c), (g(0.5, 0.5, 0), a, b, c),
            (g(0, 0, 0), a, b, c), (g(1, 0, 0), a, b, c), (g(0, 1, 0), a, b, c), (g(2, 2, 0), a, b, c), (g(-1, -1, 3), a, b, c),
            (g(0.5, -1, 0), a, b, c), (g(-1, 0.5, 1), a, b, c), (g(2, -1, 0), a, b, c), (g(-1, 2, 0), a, b, c)]
    line = (g(0, 0, 0), g(1, 1, 1), g(3, 3, 3))                              # collinear
    out += [(g(0.5, 0.5, 0.5), *line), (g(2, 2, 2.5), *line), (g(-1, 0, 0), *line), (g(4, 4, 4), *line), (g(1, 0, 0), *line)]
    twin = (g(1, 2, 3), g(1, 2, 3), g(2, 2, 3))                              # two coincident vertices (under distinct indices)
    out += [(g(1.5, 2, 3), *twin), (g(1.5, 3, 3), *twin), (g(0, 0, 0), *twin)]
    dot = (g(1, 2, 3), g(1, 2, 3), g(1, 2, 3))
    out += [(g(1, 2, 3), *dot), (g(0, 2, 3), *dot)]
    for k in range(60):                                                      # magnitude 100, everything within 0.05
        centre = np.array([100.0, -37.0, 64.0]) + rng.uniform(-1, 1, 3)
        tri = centre + rng.normal(0, 0.02, (3, 3))
        out.append((centre + rng.normal(0, 0.03, 3), *tri))
    return [tuple(np.asarray(v, f32) for v in row) for row in out]


def _replica_d2(p, a, b, c):
    cols = lambda v: tuple(f64(x) for x in v)
    return float(S.point_triangle(cols(p), cols(a), cols(b), cols(c))[0])


def test_replica_against_exact_rational_arithmetic():
    """The replica's d2 for 363 (point, triangle) pairs -- random, needles, collinear, coincident vertices, a single point, the point on
    the plane, an edge and a vertex, every region, coordinates of magnitude 100 with everything within 0.05 -- against the true squared
    distance in exact rationals.  With D the true distance and B = distance_bound (derived there from the operation count, scaled by
    the triangle's conditioning): |d2 - D^2| <= 2 D B + B^2, both ways."""
    cases = _cases()
    assert len(cases) >= 300
    worst, n_degenerate = 0.0, 0
    for p, a, b, c in cases:
        assert _differences_exact(p, a, b, c)
        truth = exact_d2(p, a, b, c)
        got = Fr(_replica_d2(p, a, b, c))
        B = distance_bound(p, a, b, c)
        allowed = 2 * _up(truth) * B + B * B
        assert abs(got - truth) <= allowed, (p, a, b, c, float(got), float(truth), float(allowed))
        if allowed > 0:
            worst = max(worst, float(abs(got - truth) / allowed))
        n_degenerate += all(x == 0 for x in _fcross(_fsub(_fr(b), _fr(a)), _fsub(_fr(c), _fr(a))))
    print(f"{len(cases)} pairs, {n_degenerate} without area; worst |d2 - D^2| / (2 D B + B^2) = {worst:.3g}")
    assert n_degenerate >= 10


def test_replica_winner_against_exact_rational_arithmetic():
    """Six random triangles and forty points at a time: the winning face agrees with the exact one wherever the exact gap between the
    best and the second best squared distance exceeds what their two bounds allow together; ties and truncation follow the contract."""
    rng = np.random.default_rng(22)
    checked = 0
    for trial in range(5):
        shift = np.array([100.0, -37.0, 0.001]) if trial % 2 else np.zeros(3)
        v = (rng.uniform(0, 1, (18, 3)) + shift).astype(f32)
        faces = np.arange(18, dtype=np.int32).reshape(6, 3)
        Q = (rng.uniform(-0.2, 1.2, (40, 3)) + shift).astype(f32)
        got = S.nearest(Q, v, faces, 10.0)
        for i, p in enumerate(Q):
            exact = [exact_d2(p, *v[f]) for f in faces]
            order = sorted(range(6), key=lambda k: exact[k])
            slack = sum(2 * _up(exact[k]) * B + B * B for k in order[:2] for B in [distance_bound(p, *v[faces[k]])])
            if exact[order[1]] - exact[order[0]] > slack:
                assert got["face"][i] == order[0]
                checked += 1
    print(f"{checked} of 200 queries have a clear exact winner")
    assert checked >= 150
    # ties go to the smallest index, a dead or skipped face never wins, the reach is strict
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]], f32)
    faces = np.array([[0, 1, 3], [0, 0, 1], [0, 1, 2], [0, 1, 2], [0, 1, 7]], np.int32)
    got = S.nearest(np.array([[0.25, 0.25, 0.5], [0.25, 0.25, -0.5], [0.25, 0.25, 0.0], [np.inf, 0, 0]], f32), v, faces, 0.5)
    assert got["face"].tolist() == [-1, -1, 2, -1] and got["side"].tolist() == [0, 0, 0, 0]
    assert got["dist"].tolist() == [0.5, 0.5, 0.0, 0.5] and got["closest"][3].tolist() == [0, 0, 0]
    assert got["stats"][[0, 1, 15, 16]].tolist() == [3, 1, 2, 1]
    got = S.nearest(np.array([[0.25, 0.25, 0.25], [0.25, 0.25, -0.25]], f32), v, faces, 0.5)
    assert got["face"].tolist() == [2, 2] and got["side"].tolist() == [1, -1] and got["stats"][[12, 13, 14]].tolist() == [1, 1, 2]


# ---- 2. points on the faces ---------------------------------------------------------------------------------------------------------- #
def test_points_made_on_the_faces_are_on_the_surface():
    """Barycentric combinations of the sphere scene's faces, computed in float64 and rounded to float32.  The float64 combination is
    within 4 * 2^-53 |p| of the face, the rounding to float32 moves each coordinate by at most 2^-24 of itself, so the point by at most
    2^-24 |p|; the replica's own error and the float32 rounding of dist are relative 2^-24 of that: dist <= 2^-24 |p| (1 + 2^-10).
    For the same points the nearest VERTEX (tests/cloud_ref.py) is a fraction of a voxel away: the floor of point-to-point scoring."""
    mesh, (_, _, _, kw) = T.sphere_mesh()
    v, faces = mesh["vertices"], mesh["faces"]
    assert v.shape == (730, 3) and faces.shape == (1456, 3)
    rng = np.random.default_rng(23)
    w = rng.dirichlet((1, 1, 1), (len(faces), 2))                            # two points per face
    w[::7, 0] = (1, 0, 0)                                                    # ... some at a vertex
    w[3::7, 0] = (0.5, 0.5, 0)                                               # ... some on an edge
    tri = v[faces.astype(np.int64)].astype(f64)                              # [F,3,3]
    P = np.einsum("fkc,fpk->fpc", tri, w).reshape(-1, 3).astype(f32)
    md = 4 * kw["voxel_size"]
    got = S.nearest(P, v, faces, md, (kw["voxel_size"],))
    bound = U32 * np.linalg.norm(P.astype(f64), axis=1) * (1 + 2.0 ** -10)
    assert (got["face"] >= 0).all() and (got["dist"].astype(f64) <= bound).all(), float((got["dist"] / bound).max())
    cloud = cloud_ref.nearest(P, v, md)
    vox = kw["voxel_size"]
    print(f"{len(P)} points on the faces: point to surface max {got['dist'].max():.3e} (bound {bound.max():.3e}); nearest vertex mean "
          f"{cloud['dist'].mean():.5f} = {cloud['dist'].mean() / vox:.3f} voxels, max {cloud['dist'].max() / vox:.3f} voxels")
    assert cloud["dist"].mean() > 0.25 * vox and got["dist"].max() < 1e-6 * vox


# ---- 3. the cell rule ---------------------------------------------------------------------------------------------------------------- #
def lattice_mesh(md):
    """cloud_ref.lattice's queries, and a mesh on its reference points (the even sites 0..7 of a lattice of pitch max_dist): every
    occupied site s with room carries the triangle (s, s + (1,1,0), s + (1,0,1)) -- vertices on even sites, bounds that end exactly on
    multiples of the pitch.  Queries at the sites beyond the lattice have a vertex, and nothing else, within a few ulps of max_dist."""
    Q, P, _ = cloud_ref.lattice(md, 7)
    g = np.arange(0, 8)
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    sites = sites[sites.sum(axis=1) % 2 == 0]
    index = {tuple(s): i for i, s in enumerate(sites)}
    pos = (sites.astype(f32) * f32(md) + cloud_ref.SHIFT).astype(f32)
    assert np.array_equal(np.sort(pos, axis=0), np.sort(P, axis=0))
    faces = [(index[tuple(s)], index[tuple(s + (1, 1, 0))], index[tuple(s + (1, 0, 1))]) for s in sites
             if tuple(s + (1, 1, 0)) in index and tuple(s + (1, 0, 1)) in index]
    return Q, pos, np.array(faces, np.int32)


def _misses(Q, v, faces, md, margin, want):
    g = S.grid_emulation(Q, v, faces, md, margin=margin)
    reached = want["face"] >= 0
    seen = g["seen"](np.maximum(want["face"], 0))
    return int((reached & ~seen).sum()), int(reached.sum())


@pytest.mark.parametrize("md", cloud_ref.LATTICE_MAX_DISTS)
def test_cell_rule_finds_every_winner_on_the_lattice(md):
    """The emulated index (binning by bounds, the 27-cell walk) holds the brute-force winner of every reached query at the library's
    margin of 2^-10.  The point lattice loses winners at 0.013 and 0.083 with a cell edge of exactly max_dist (tests/test_cloud_cpu.py);
    for faces that half does NOT reproduce: no winner is lost at any of the four values without the margin either (printed).  A point is
    within reach there by a float32 d2 that rounds below md2 although it is a hair beyond max_dist; here reach is decided in float64
    on exact differences, so a vertex within reach is nearer than max_dist by at least an ulp of a float32 coordinate, which these
    lattices' cell coordinates resolve.  The margin stays: the argument of DESIGN.md 3.6p needs it for coordinates whose ulp is finer
    than 2^-24 max_dist.  Only the positive half is asserted."""
    Q, v, faces = lattice_mesh(md)
    want = S.nearest(Q, v, faces, md)
    missed, reached = _misses(Q, v, faces, md, 1.0 + 2.0 ** -10, want)
    assert reached > 0.5 * len(Q) and (want["face"] < 0).sum() > 0
    bare, _ = _misses(Q, v, faces, md, 1.0, want)
    print(f"max_dist {md}: {bare} of {reached} reached queries lose their winner at edge = max_dist, {missed} at the margin")
    assert missed == 0


def test_cell_rule_finds_every_winner_on_an_extracted_mesh():
    mesh, (_, _, _, kw) = T.sphere_mesh()
    v, faces = mesh["vertices"], mesh["faces"]
    rng = np.random.default_rng(24)
    Q = (v[rng.integers(0, len(v), 1500)] + rng.normal(0, 0.6 * kw["voxel_size"], (1500, 3))).astype(f32)
    md = 1.5 * kw["voxel_size"]
    want = S.nearest(Q, v, faces, md)
    missed, reached = _misses(Q, v, faces, md, 1.0 + 2.0 ** -10, want)
    assert 0 < reached < len(Q) and missed == 0
    g = S.grid_emulation(Q, v, faces, md)
    assert g["pairs"] >= len(faces) and not g["oversize"].any() and g["examined"] > 0
    # one face across the whole box: oversize, seen by every query
    big = np.concatenate([v, [v.min(axis=0), [v[:, 0].max(), v[:, 1].min(), v[:, 2].min()], v.max(axis=0)]]).astype(f32)
    f2 = np.concatenate([faces, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)
    g2 = S.grid_emulation(Q, big, f2, md)
    assert g2["oversize"].tolist() == [False] * len(faces) + [True] and g2["pairs"] == g["pairs"]
    assert g2["examined"] == g["examined"] + len(Q)


# ---- 4. metrics_from_stats layout ---------------------------------------------------------------------------------------------------- #
def _patch(k, z=0.0):
    """a flat k x k patch of unit squares / 8 in the plane z, wound so that the normal points to +z"""
    g = np.arange(k + 1)
    x, y = np.meshgrid(g, g, indexing="ij")
    v = np.stack([x.ravel() / 8.0, y.ravel() / 8.0, np.full(x.size, z)], 1).astype(f32)
    i = (x[:-1, :-1] * (k + 1) + y[:-1, :-1]).ravel()
    faces = np.concatenate([np.stack([i, i + k + 1, i + k + 2], 1), np.stack([i, i + k + 2, i + 1], 1)]).astype(np.int32)
    return v, faces


def test_measures_from_the_replica_statistics():
    from coivo_amd import _args, evaluate as E
    assert E.SURFACE_STATS == S.STATS and E.SURFACE_STATS[:12] == E.CLOUD_STATS
    v, faces = _patch(6)
    md, th = 0.25, (0.05, 0.125)
    same = S.nearest(v, v, faces, md, th)
    m = E.metrics_from_stats(same["stats"][:12], same["stats"][:12], _args.f32(md), 2)
    assert m["accuracy"] == 0.0 and m["completeness"] == 0.0 and m["chamfer"] == 0.0
    assert m["precision"] == (1.0, 1.0) and m["recall"] == (1.0, 1.0) and m["fscore"] == (1.0, 1.0)
    assert m["n_pred"] == m["n_pred_reached"] == len(v)
    # a copy 1/16 above the patch: every vertex is exactly 1/16 from the plane candidate of a face below it, in front of it
    up, _ = _patch(6, 0.0625)
    a, b = S.nearest(up, v, faces, md, th), S.nearest(v, up, faces, md, th)
    assert (a["dist"] == 0.0625).all() and (a["side"] == 1).all() and (b["side"] == -1).all()
    assert a["stats"][10] == len(v) * 2 ** 18 and a["stats"][12] == len(v) and b["stats"][13] == len(v)
    assert a["stats"][14] == len(v)                                          # (an edge candidate at the same d2 never replaces the plane one)
    m = E.metrics_from_stats(a["stats"][:12], b["stats"][:12], _args.f32(md), 2)
    assert m["accuracy"] == 0.0625 and m["completeness"] == 0.0625 and m["precision"] == (0.0, 1.0) and m["recall"] == (0.0, 1.0)
    assert m["fscore"] == (0.0, 1.0)
    r = S.metrics((up, faces), (v, faces), md, th)
    assert r["accuracy"] == 0.0625 and r["in_front"] == 1.0 and r["behind"] == 0.0


# ---- the entry points refuse what they cannot take ----------------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.ensure()
    return _lib.load()


def _refused(lib, rc, *words):
    msg = lib.colvo_last_error()
    assert rc != 0, msg
    for w in words:
        assert w in msg, msg


def test_surface_entry_points_validate_their_arguments(lib):
    from coivo_amd import _lib
    assert lib.colvo_abi_version() == _lib.ABI_VERSION >= 27 and _lib.tune_get("surface_span_limit") == S.SPAN_LIMIT
    assert _lib.tune_get("surface_copy_records") in (0, 1)
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p = p if p % 16 == 0 else p + 8
    assert p % 16 == 0
    tau = (C.c_float * 3)(0.01, 0.02, 0.03)
    t = C.addressof(tau)
    assert lib.colvo_surface_scratch_bytes(0, 0) > 0
    assert lib.colvo_surface_scratch_bytes(10, 1000) - lib.colvo_surface_scratch_bytes(10, 0) == 4000
    for V, F in ((-1, 0), (0, -1), (0, 2 ** 29)):
        assert lib.colvo_surface_scratch_bytes(V, F) == 0
    plan = lambda **kw: lib.colvo_surface_index_plan(*[kw.get(k, d) for k, d in (
        ("vertices", p), ("faces", p), ("V", 4), ("F", 4), ("max_dist", 0.1), ("scratch", p), ("counts", p), ("stream", 0))])
    for name in ("vertices", "faces", "scratch", "counts"):
        _refused(lib, plan(**{name: 0}), b"colvo_surface_index_plan:", b"null pointer")
    _refused(lib, plan(F=2 ** 29), b"colvo_surface_index_plan: bad shape")
    _refused(lib, plan(V=-1), b"bad shape")
    for bad in (0.0, -1.0, math.inf, math.nan, 1e-30, 1e30):
        _refused(lib, plan(max_dist=bad), b"colvo_surface_index_plan: bad max_dist")
    _refused(lib, plan(scratch=p + 4), b"16-byte aligned")
    fill = lambda **kw: lib.colvo_surface_index_fill(*[kw.get(k, d) for k, d in (
        ("vertices", p), ("faces", p), ("V", 4), ("F", 4), ("scratch", p), ("pairs", 4), ("record_bytes", 4), ("records", p), ("stream", 0))])
    _refused(lib, fill(pairs=2 ** 30), b"colvo_surface_index_fill:", b"pairs")
    _refused(lib, fill(pairs=-1), b"pairs")
    _refused(lib, fill(records=0), b"colvo_surface_index_fill: null pointer")
    _refused(lib, fill(F=2 ** 29), b"bad shape")
    for bad in (0, 5, 40, -4):
        _refused(lib, fill(record_bytes=bad), b"colvo_surface_index_fill: bad record_bytes")
    _refused(lib, fill(records=p + 4), b"16-byte aligned")
    assert fill(pairs=0, records=0) == 0 and fill(pairs=0, records=0, record_bytes=48) == 0     # nothing to fill: no launch
    q = lambda **kw: lib.colvo_surface_query(*[kw.get(k, d) for k, d in (
        ("query", p), ("N", 4), ("vertices", p), ("faces", p), ("V", 4), ("F", 4), ("max_dist", 0.1), ("tau", t), ("n_tau", 3),
        ("scratch", p), ("records", p), ("pairs", 4), ("record_bytes", 48), ("dist2", p), ("dist", p), ("face", p), ("closest", p), ("side", p), ("stats", p),
        ("stream", 0))])
    for name in ("query", "vertices", "faces", "tau", "scratch", "records", "dist2", "dist", "face", "closest", "side", "stats"):
        _refused(lib, q(**{name: 0}), b"colvo_surface_query:", b"null pointer")
    _refused(lib, q(N=2 ** 30), b"colvo_surface_query: bad shape")
    _refused(lib, q(F=2 ** 29), b"bad shape")
    _refused(lib, q(pairs=2 ** 30), b"pairs")
    _refused(lib, q(record_bytes=8), b"colvo_surface_query: bad record_bytes")
    for bad in (0.0, -0.1, math.inf, math.nan):
        _refused(lib, q(max_dist=bad), b"bad max_dist")
    _refused(lib, q(n_tau=9), b"bad thresholds")
    _refused(lib, q(max_dist=0.025), b"bad thresholds", b"tau[2]")
    down = (C.c_float * 3)(0.02, 0.01, 0.03)
    _refused(lib, q(tau=C.addressof(down)), b"bad thresholds", b"tau[1]")
    _refused(lib, q(scratch=p + 4), b"16-byte aligned")


def test_python_functions_refuse_cpu_tensors_and_bad_reach():
    from coivo_amd import evaluate as E
    ok = torch.zeros(4, 3)
    faces = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="point_to_surface: points"):
        E.point_to_surface(ok, ok, faces, max_dist=0.1)
    with pytest.raises(ValueError, match="surface_metrics: max_dist"):
        E.surface_metrics((ok, faces), (ok, faces), max_dist=-1.0, thresholds=())
    with pytest.raises(ValueError, match="surface_metrics: thresholds"):
        E.surface_metrics((ok, faces), (ok, faces), max_dist=1.0, thresholds=(0.5, 0.25))
    with pytest.raises(ValueError, match="surface_metrics: pred must be a Mesh"):
        E.surface_metrics(ok, (ok, faces), max_dist=1.0, thresholds=())
    with pytest.raises(ValueError, match="surface_metrics"):
        E.surface_metrics((ok, faces), (ok, faces), max_dist=1.0, thresholds=())       # CPU vertices
    with pytest.raises(ValueError, match="surface_reconstruction_metrics: pred_mesh"):
        E.surface_reconstruction_metrics(ok, torch.eye(4)[None], torch.zeros(1, 1, 8, 8), torch.eye(3)[None], torch.eye(4)[None],
                                         voxel_size=0.1)
