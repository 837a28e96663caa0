"""-m gpu: point_to_surface / surface_metrics / surface_reconstruction_metrics (coivo_amd.evaluate, csrc/surface.hip) against their
gridless NumPy replica (tests/surface_ref.py).  The distance is float64 in a written association, the winner the least (d2, face) and
the statistics integer sums, so every comparison here is equality to the bit, of every output."""
import functools

import numpy as np
import pytest
import torch

from tests import cloud_ref
from tests import surface_ref as S
from tests import topology_ref as T
from tests.gpu_util import dev
from tests.test_surface_cpu import lattice_mesh

pytestmark = pytest.mark.gpu

f32 = np.float32
BITS = {torch.float32: torch.int32, torch.float64: torch.int64}


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _run(Q, v, f, md, th=()):
    from coivo_amd import evaluate as E
    return E.point_to_surface(_t(np.asarray(Q, f32).reshape(-1, 3)), _t(np.asarray(v, f32).reshape(-1, 3)),
                              _t(np.asarray(f, np.int32).reshape(-1, 3)), max_dist=md, thresholds=th)


def _bits(t):
    return t.view(BITS[t.dtype]) if t.dtype in BITS else t


def _assert_equal(got, want, what="", stats=True):
    """every per-query output to the bit (signed zeros included), and the statistics"""
    from coivo_amd import evaluate as E
    assert isinstance(got, E.SurfaceNN)
    for k, dtype in (("dist2", torch.float64), ("dist", torch.float32), ("face", torch.int32), ("closest", torch.float32),
                     ("side", torch.int8)):
        g, w = getattr(got, k).cpu(), torch.from_numpy(np.ascontiguousarray(want[k]))
        assert g.dtype == dtype and g.shape == w.shape, (what, k, g.dtype, tuple(g.shape), tuple(w.shape))
        assert torch.equal(_bits(g), _bits(w)), (what, k, int((_bits(g) != _bits(w)).sum()))
    if stats:
        assert got.stats.dtype == torch.int64 and torch.equal(got.stats.cpu(), torch.from_numpy(want["stats"])), \
            (what, got.stats.tolist(), want["stats"].tolist())


def _same(a, b):
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y))
        else:
            assert x == y


def _check(Q, v, f, md, th=(), what=""):
    want = S.full_stats(Q, v, f, md, th)
    got = _run(Q, v, f, md, th)
    _assert_equal(got, want, what)
    return got, want


# ---- 1. one hand mesh ---------------------------------------------------------------------------------------------------------------- #
def test_hand_mesh_equals_the_replica():
    nan, inf = np.nan, np.inf
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0],              # 0-3: two triangles on the edge (0, 1)
                  [4, 0, 0], [5, 1, 1], [7, 3, 3],                           # 4-6: collinear
                  [0, 4, 0], [0, 4, 0], [1, 4, 0],                           # 7-9: two coincident vertices under distinct indices
                  [nan, 8, 8], [0, 8, 8], [1, 8, 8]], f32)                   # 10-12: a NaN vertex
    V = len(v)
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 2], [4, 5, 6], [7, 8, 9], [0, 0, 1], [0, 1, -1], [0, 1, V], [10, 11, 12]], np.int32)
    below = np.nextafter(f32(0.5), f32(0))
    Q = np.array([[0.25, 0.25, 0.3],                                          # the face region, in front
                  [0.25, 0.25, -0.3],                                         # ... behind
                  [0.5, -0.2, 0.1], [0.7, 0.7, 0.1], [-0.2, 0.5, 0.1],        # beyond each edge (face 1 takes the first)
                  [-0.2, -0.2, 0.1], [1.3, -0.1, 0.1], [-0.1, 1.3, 0.1],      # beyond each vertex
                  [0.25, 0.25, 0.0], [0.5, 0.5, 0.0], [1.0, 0.0, 0.0],        # on the plane, on an edge, at a vertex
                  [0.25, 0.25, below], [0.25, 0.25, 0.5], [0.25, 0.25, -0.5], # just inside, and exactly at, max_dist
                  [0.5, 0.0, 0.3],                                            # equidistant from faces 0, 1 and 2 through their shared edge
                  [4.5, 0.5, 0.6], [6.0, 2.0, 2.1], [8.0, 4.0, 4.0],          # the collinear face: a segment
                  [0.5, 4.0, 0.2], [0.0, 4.1, 0.0], [-0.1, 4.0, 0.0],         # the face with coincident vertices: a segment
                  [0.5, 8.0, 8.1],                                            # the skipped face: nothing
                  [nan, 0, 0], [0, inf, 0], [0, 0, -inf], [-0.0, 0.2, 0.1]], f32)
    got, want = _check(Q, v, f, 0.5, (0.1, 0.3, 0.5), "hand")
    face = want["face"].tolist()
    assert face[:2] == [0, 0] and want["side"][:2].tolist() == [1, -1]
    assert face[11:15] == [0, -1, -1, 0] and face[8:11] == [0, 0, 0]         # strict reach; the smallest index of a tie
    assert face[15:18] == [3, 3, -1] and face[18:21] == [4, 4, 4] and face[21:25] == [-1, -1, -1, -1]
    assert want["side"][15:21].tolist() == [0] * 6                            # no area: no side
    st = want["stats"]
    assert st[0] == len(Q) - 3 and st[15] == 3 and st[16] == 1 and st[17] >= 4
    assert st[18] == 1                                                       # the collinear face spans seven cells of 0.5: oversize
    assert got.closest[22:25].tolist() == [[0.0, 0.0, 0.0]] * 3 and got.dist[22].item() == 0.5
    # a Mesh is taken apart the same way
    from coivo_amd import evaluate as E, inference as I
    mesh = I.Mesh(_t(v), _t(f), None, _t(v), torch.zeros(V, 3, device=dev(), dtype=torch.int32), 0)
    _assert_equal(E.point_to_surface(_t(Q), mesh, max_dist=0.5, thresholds=(0.1, 0.3, 0.5)), want, "Mesh")


# ---- 2. the project's own meshes ---------------------------------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def _scene(name):
    """(vertices, faces, voxel size) of the replica's mesh: shared by the tests, do not write to it"""
    if name == "sphere":
        mesh, (_, _, _, kw) = T.sphere_mesh()
    else:
        shape, Tv, min_obs = {"thin": ((5, 17, 23), 1, 2), "tube2": ((5, 24, 32), 4, 2)}[name]
        mesh, (_, _, _, kw) = T.tube_mesh(*shape, Tv, min_obs)
    return mesh["vertices"], mesh["faces"], kw["voxel_size"]


@functools.lru_cache(maxsize=None)
def _scene_case(name):
    v, f, vox = _scene(name)
    other = _scene("sphere" if name == "tube2" else "tube2")[0]
    rng = np.random.default_rng(31)
    jit = (v[rng.integers(0, len(v), 2500)] + rng.normal(0, 0.6 * vox, (2500, 3))).astype(f32)
    Q = np.concatenate([other, jit])
    md, th = 1.5 * vox, (0.5 * vox, vox)
    return Q, v, f, md, th, S.full_stats(Q, v, f, md, th)


@pytest.mark.parametrize("name", ["tube2", "sphere"])
def test_extracted_meshes_equal_the_replica(name):
    Q, v, f, md, th, want = _scene_case(name)
    assert {"tube2": (2054, 3498), "sphere": (730, 1456)}[name] == (len(v), len(f))
    st = want["stats"]
    assert 0.3 * 2500 < st[1] < len(Q) and st[12] > 100 and st[13] > 100 and 0 < st[14] < st[1] and st[17] > len(f)
    _assert_equal(_run(Q, v, f, md, th), want, name)


# ---- 3. the lattice ------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("md", cloud_ref.LATTICE_MAX_DISTS)
def test_lattice_equals_the_gridless_replica(md):
    """Queries within a few ulps of a cell border in every coordinate, vertices within a few ulps of max_dist from them (the CPU test
    of the same lattice checks the emulated rule)"""
    Q, v, f = lattice_mesh(md)
    got, want = _check(Q, v, f, md, (md,), f"lattice {md}")
    assert 0 < want["stats"][1] < want["stats"][0] == len(Q)


# ---- 4. the oversize list ------------------------------------------------------------------------------------------------------------- #
def test_oversize_list_and_a_face_just_below_the_limit():
    from coivo_amd import _lib
    assert _lib.tune_get("surface_span_limit") == S.SPAN_LIMIT
    v, f, vox = _scene("thin")
    md = 1.5 * vox
    rng = np.random.default_rng(32)
    Q = (v[rng.integers(0, len(v), 1500)] + rng.normal(0, 0.8 * vox, (1500, 3))).astype(f32)
    lo, hi = v.min(axis=0), v.max(axis=0)
    # one triangle across the whole bounding box
    v1 = np.concatenate([v, [lo, [hi[0], lo[1], lo[2]], hi]]).astype(f32)
    f1 = np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)
    got, want = _check(Q, v1, f1, md, (vox,), "oversize")
    assert want["stats"][18] == 1 and (want["face"] == len(f)).sum() > 0
    # a long, thin diagonal triangle whose box spans exactly the limit on every axis: entered through the grid, 64 pairs
    g = S.grid_emulation(Q, v, f, md)
    assert (g["n"] > S.SPAN_LIMIT).all()
    e, o = np.float64(g["edge"]), g["o"].astype(np.float64)
    tri = np.array([o + e * 0.5, o + e * (S.SPAN_LIMIT - 0.5), o + e * np.array([0.6, 0.5, 0.5])]).astype(f32)
    v2 = np.concatenate([v, tri]).astype(f32)
    g2 = S.grid_emulation(Q, v2, f1, md)
    assert (g2["hi"][-1] - g2["lo"][-1] + 1).tolist() == [S.SPAN_LIMIT] * 3 and not g2["oversize"].any()
    assert g2["pairs"] == g["pairs"] + S.SPAN_LIMIT ** 3
    got, want = _check(Q, v2, f1, md, (vox,), "below the limit")
    assert want["stats"][18] == 0 and (want["face"] == len(f)).sum() > 0
    # ... and one cell more on one axis puts it on the list
    v3 = v2.copy()
    v3[-2, 0] = f32(o[0] + e * (S.SPAN_LIMIT + 0.5))
    got, want = _check(Q, v3, f1, md, (vox,), "above the limit")
    assert want["stats"][18] == 1


def _record_bytes():
    """what a plan reports for a one-face mesh under the current tuning"""
    from coivo_amd import _lib
    lib = _lib.load()
    v, f = _t(np.eye(3, dtype=f32)), _t(np.array([[0, 1, 2]], np.int32))
    scratch = torch.empty(int(lib.colvo_surface_scratch_bytes(3, 1)), device=dev(), dtype=torch.uint8)
    counts = torch.empty(8, device=dev(), dtype=torch.int64)
    _lib.check(lib.colvo_surface_index_plan(_lib.ptr(v), _lib.ptr(f), 3, 1, 0.5, _lib.ptr(scratch), _lib.ptr(counts), _lib.stream_ptr()),
               "colvo_surface_index_plan")
    return counts.tolist()


@pytest.mark.parametrize("copy", [0, 1])
def test_both_record_forms_give_the_same_bits(copy):
    """tuning.h surface_copy_records: the face index alone, or the face copied into the record.  The plan reports the form; the
    extracted mesh, the lattice and the oversize list give the replica's bits with either."""
    from coivo_amd import _lib
    saved = _lib.tune_get("surface_copy_records")
    try:
        _lib.tune_set("surface_copy_records", copy)
        counts = _record_bytes()
        assert counts[0] >= 1 and counts[1:] == [0, 0, 0, 48 if copy else 4, 0, 0, 0]
        Q, v, f, md, th, want = _scene_case("sphere")
        _assert_equal(_run(Q, v, f, md, th), want, f"sphere, copy {copy}")
        Q, v, f = lattice_mesh(0.083)
        _check(Q[::5], v, f, 0.083, (), f"lattice, copy {copy}")
        v, f, vox = _scene("thin")
        lo, hi = v.min(axis=0), v.max(axis=0)
        v1 = np.concatenate([v, [lo, [hi[0], lo[1], lo[2]], hi]]).astype(f32)
        f1 = np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2], [0, 0, 1], [len(v), 1, 2]]]).astype(np.int32)
        got, want = _check(v[::3] + f32(0.01), v1, f1, 1.5 * vox, (vox,), f"oversize, copy {copy}")
        assert want["stats"][18] >= 1 and want["stats"][15] == 1
    finally:
        _lib.tune_set("surface_copy_records", saved)                         # the tests share one process
    assert _lib.tune_get("surface_copy_records") == saved


# ---- 5. identical bits ---------------------------------------------------------------------------------------------------------------- #
def test_identical_bits_between_calls_streams_and_orders():
    from coivo_amd import evaluate as E
    Q, v, f, md, th, _ = _scene_case("tube2")
    q, tv, tf = _t(Q), _t(v), _t(f)
    a = E.point_to_surface(q, tv, tf, max_dist=md, thresholds=th)
    _same(a, E.point_to_surface(q, tv, tf, max_dist=md, thresholds=th))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        b = E.point_to_surface(q, tv, tf, max_dist=md, thresholds=th)
    side.synchronize()
    _same(a, b)
    perm = torch.from_numpy(np.random.default_rng(33).permutation(len(Q))).to(dev())
    c = E.point_to_surface(q[perm].contiguous(), tv, tf, max_dist=md, thresholds=th)
    for k in ("dist", "dist2", "face", "closest", "side"):
        assert torch.equal(_bits(getattr(c, k)), _bits(getattr(a, k)[perm])), k
    assert torch.equal(c.stats, a.stats)


def test_a_permutation_of_the_faces_moves_only_the_face_index():
    """300 separate random triangles and 600 points: tie-free (checked on the replica's full matrix of d2), so the winner is the same
    triangle under any order of the faces."""
    from coivo_amd import evaluate as E
    rng = np.random.default_rng(34)
    v = (rng.uniform(0, 1, (300, 1, 3)) + rng.normal(0, 0.05, (300, 3, 3))).reshape(-1, 3).astype(f32)
    f = np.arange(900, dtype=np.int32).reshape(300, 3)
    Q = rng.uniform(0, 1, (600, 3)).astype(f32)
    md = 0.2
    tri = v[f.astype(np.int64)].astype(np.float64)
    d2 = S.point_triangle(tuple(Q[:, None, j].astype(np.float64) for j in range(3)), *(tuple(tri[None, :, k, j] for j in range(3))
                                                                                       for k in range(3)))[0]
    two = np.sort(d2, axis=1)[:, :2]
    assert (two[:, 0] < two[:, 1]).all()                                     # tie-free
    a = _run(Q, v, f, md)
    _assert_equal(a, S.full_stats(Q, v, f, md), "separate triangles")
    perm = rng.permutation(300)
    b = _run(Q, v, f[perm], md)
    for k in ("dist", "dist2", "closest", "side"):
        assert torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k))), k
    new_row = np.empty(300, np.int64)
    new_row[np.arange(300)] = np.argsort(perm)                               # old face -> its row after the permutation
    fa = a.face.cpu().numpy()
    assert np.array_equal(np.where(fa >= 0, new_row[np.maximum(fa, 0)], -1), b.face.cpu().numpy())
    assert torch.equal(a.stats[:17], b.stats[:17])


# ---- 6. degenerate inputs ------------------------------------------------------------------------------------------------------------- #
def test_empty_sides_and_refusals():
    from coivo_amd import evaluate as E
    v, f, vox = _scene("sphere")
    Q = v[:50]
    z3 = np.zeros((0, 3), f32)
    zf = np.zeros((0, 3), np.int32)
    got, want = _check(z3, v, f, 0.1, (0.05,), "N = 0")
    assert got.dist.shape == (0,) and got.closest.shape == (0, 3) and want["stats"][17] > 0
    got, want = _check(Q, v, zf, 0.1, (0.05,), "F = 0")
    assert (got.face == -1).all() and torch.equal(got.closest.cpu(), torch.from_numpy(Q)) and want["stats"][:2].tolist() == [50, 0]
    got, want = _check(Q, z3, f, 0.1, (), "V = 0")
    assert want["stats"][15] == len(f) and want["stats"][17] == 0 and (got.dist == np.float32(0.1)).all()
    dead = np.stack([f[:, 0], f[:, 0], f[:, 2]], 1)
    dead[::2] = -1
    got, want = _check(Q, v, dead, 0.1, (), "all faces dead")
    assert want["stats"][15] == len(f) and (got.side == 0).all() and (got.dist2 == float(np.float32(0.1)) ** 2).all()
    _check(z3, z3, zf, 0.1, (), "everything empty")
    q, tv, tf = _t(Q), _t(v), _t(f)
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-30, 1e30):
        with pytest.raises(ValueError, match="point_to_surface: max_dist"):
            E.point_to_surface(q, tv, tf, max_dist=bad)
    with pytest.raises(ValueError, match="point_to_surface: thresholds"):
        E.point_to_surface(q, tv, tf, max_dist=0.1, thresholds=(0.05, 0.02))
    with pytest.raises(ValueError, match="point_to_surface: thresholds"):
        E.point_to_surface(q, tv, tf, max_dist=0.1, thresholds=(0.2,))
    with pytest.raises(ValueError, match="point_to_surface: points"):
        E.point_to_surface(q.double(), tv, tf, max_dist=0.1)
    with pytest.raises(ValueError, match="point_to_surface: points"):
        E.point_to_surface(q.cpu(), tv, tf, max_dist=0.1)
    with pytest.raises(ValueError, match="point_to_surface: vertices"):
        E.point_to_surface(q, tv.double(), tf, max_dist=0.1)
    with pytest.raises(ValueError, match="point_to_surface: faces"):
        E.point_to_surface(q, tv, tf.long(), max_dist=0.1)
    with pytest.raises(ValueError, match="point_to_surface: faces"):
        E.point_to_surface(q, tv, tf.cpu(), max_dist=0.1)


# ---- 7. surface_metrics ---------------------------------------------------------------------------------------------------------------- #
MEASURES = ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore", "n_pred", "n_gt", "n_pred_reached", "n_gt_reached",
            "in_front", "behind")


def _assert_metrics(got, want, what=""):
    from coivo_amd import evaluate as E
    assert isinstance(got, E.SurfaceMetrics)
    for k in MEASURES:
        assert getattr(got, k) == want[k], (what, k, getattr(got, k), want[k])
    _assert_equal(got.pred_to_gt, want["pred_to_gt"], what + " pred -> gt", stats=False)
    _assert_equal(got.gt_to_pred, want["gt_to_pred"], what + " gt -> pred", stats=False)
    for g, w in ((got.pred_to_gt, want["pred_to_gt"]), (got.gt_to_pred, want["gt_to_pred"])):
        keep = [k for k in range(S.N_STATS) if k not in (11, 17, 18)]         # (the index's cost figures: compared in the tests above)
        assert got is not None and g.stats.cpu()[keep].tolist() == w["stats"][keep].tolist(), what
    assert torch.equal(got.pred.vertices.cpu(), torch.from_numpy(want["pred"][0])) and torch.equal(got.gt.faces.cpu(), torch.from_numpy(want["gt"][1]))


def _gpu_tube(scale=1.0):
    from coivo_amd import inference as I
    _, (depths, K, M, kw) = T.tube_mesh(5, 24, 32, 4, 2)
    vol = I.fuse_tsdf(_t(depths * f32(scale)), _t(K), _t(M), **{**kw, "colors": _t(kw["colors"])})
    return I.extract_mesh(vol, min_obs=2)


def test_surface_metrics_of_a_mesh_against_itself_and_against_a_scaled_one():
    from coivo_amd import evaluate as E
    mesh = _gpu_tube()
    v, f, vox = _scene("tube2")
    assert torch.equal(mesh.faces.cpu(), torch.from_numpy(f))
    md, th = 4 * vox, (vox, 2 * vox)
    m = E.surface_metrics(mesh, mesh, max_dist=md, thresholds=th)
    assert m.accuracy == 0.0 and m.completeness == 0.0 and m.chamfer == 0.0
    assert m.precision == (1.0, 1.0) and m.recall == (1.0, 1.0) and m.fscore == (1.0, 1.0)
    assert 0 < m.n_pred == m.n_gt == m.n_pred_reached < len(v)               # the face-less vertices are no queries
    _assert_metrics(m, S.metrics((v, f), (v, f), md, th), "self")
    # against the surface fused from the depths scaled by 1.02, as (vertices, faces) pairs and under a small transform
    far = _gpu_tube(1.02)
    fv, ff = far.vertices.cpu().numpy(), far.faces.cpu().numpy()
    tr = (np.eye(3), np.array([0.004, -0.003, 0.002]), 1.001)
    got = E.surface_metrics((mesh.vertices, mesh.faces), far, max_dist=md, thresholds=th, transform=tr)
    want = S.metrics((v, f), (fv, ff), md, th, tr)
    assert 0.0 < want["accuracy"] < vox and want["precision"][0] < 1.0 and want["in_front"] > want["behind"] > 0.0
    _assert_metrics(got, want, "scaled")


# ---- 8. surface_reconstruction_metrics ----------------------------------------------------------------------------------------------- #
def test_surface_reconstruction_metrics_equals_the_pipeline_of_the_replicas():
    from coivo_amd import evaluate as E, inference as I
    gt_mesh, (depths, K, M, kw) = T.tube_mesh(5, 24, 32, 4, 2)
    pred = _gpu_tube(1.02)                                                    # a reconstruction 2 % too large ...
    P = M.astype(np.float64).copy()
    P[:, :3, 3] *= 1.02                                                       # ... along a trajectory 2 % too long: sim3 takes both out
    got = E.surface_reconstruction_metrics(pred, torch.from_numpy(P), _t(depths), _t(K), torch.from_numpy(M), voxel_size=kw["voxel_size"],
                                           meshing=I.Meshing(), max_depth=T.TUBE_MAX_DEPTH)
    tr = E.align_trajectory(torch.from_numpy(P), torch.from_numpy(M), "sim3")
    assert abs(tr[2] - 1 / 1.02) < 1e-6
    vs = float(f32(kw["voxel_size"]))
    want = S.metrics((pred.vertices.cpu().numpy(), pred.faces.cpu().numpy()), (gt_mesh["vertices"], gt_mesh["faces"]), 4.0 * vs,
                     (vs, 2.0 * vs), tuple(np.asarray(x) for x in tr))
    assert got.pred_to_gt.max_dist == float(f32(4.0 * vs)) and got.pred_to_gt.thresholds == (vs, float(f32(2.0 * vs)))
    assert want["precision"][1] > 0.9 and want["accuracy"] < 0.5 * vs
    _assert_metrics(got, want, "reconstruction")
    none = E.surface_reconstruction_metrics(pred, torch.from_numpy(P), _t(depths), _t(K), torch.from_numpy(M), voxel_size=kw["voxel_size"],
                                            max_depth=T.TUBE_MAX_DEPTH, align="none")
    _assert_metrics(none, S.metrics((pred.vertices.cpu().numpy(), pred.faces.cpu().numpy()), (gt_mesh["vertices"], gt_mesh["faces"]),
                                    4.0 * vs, (vs, 2.0 * vs)), "align none")


# ---- memory discipline ---------------------------------------------------------------------------------------------------------------- #
def test_memory_discipline():
    """point_to_surface under tests/guarded.py: queries, vertices and faces between guard bands, the scratch of
    colvo_surface_scratch_bytes, the index and every output from the pool under both poisons, with both record forms.  Outputs equal the
    replica, are the same bytes under either poison, and no guard byte changes.  Launches reached: the thin tube's mesh with one
    triangle across its bounding box runs colvo_surface_index_plan, the index fill and the query with a non-empty oversize list
    (stats[18] = 1) and three threshold counts."""
    from coivo_amd import _lib, evaluate as E
    from tests import guarded as G
    lib = _lib.load()
    v, f, vox = _scene("thin")
    md = 1.5 * vox
    rng = np.random.default_rng(32)
    Q = (v[rng.integers(0, len(v), 1500)] + rng.normal(0, 0.8 * vox, (1500, 3))).astype(f32)
    lo, hi = v.min(axis=0), v.max(axis=0)
    v1 = np.concatenate([v, [lo, [hi[0], lo[1], lo[2]], hi]]).astype(f32)
    f1 = np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)
    th = (0.5 * vox, vox, md)
    want = S.full_stats(Q, v1, f1, md, th)
    assert want["stats"][18] == 1 and (want["face"] == len(f)).sum() > 0
    saved = _lib.tune_get("surface_copy_records")
    try:
        for copy in (0, 1):
            _lib.tune_set("surface_copy_records", copy)
            outs, pools = G.under_both_poisons(dev(), lambda pool: E.point_to_surface(pool.place(_t(Q)), pool.place(_t(v1)), pool.place(_t(f1)),
                                                                                     max_dist=md, thresholds=th), f"point_to_surface, copy {copy}")
            for got, pool in zip(outs, pools):
                _assert_equal(got, want, f"oversize, copy {copy}")
                G.assert_served(pool, 0, lib.colvo_surface_scratch_bytes(len(v1), len(f1)), f"point_to_surface, copy {copy}")
    finally:
        _lib.tune_set("surface_copy_records", saved)
