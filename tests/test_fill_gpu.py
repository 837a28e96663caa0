"""-m gpu: fill_holes (coivo_amd.holes, csrc/fill.hip) against its NumPy replica (tests/fill_ref.py).  Rings are numbered from the
loop's smallest vertex, sums are integer adds and the measures are float64 in a written association, so every comparison here is
equality to the bit of every field, float fields as int32 views, dtypes and shapes included."""
import functools

import numpy as np
import pytest
import torch

from tests import fill_ref as R
from tests import topology_ref as T
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

f32 = np.float32


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _gpu(mesh):
    """the dict of tests/fill_ref.py as a Mesh on the device"""
    from coivo_amd import inference as I
    return I.Mesh(_t(mesh["vertices"]), _t(mesh["faces"]), _t(mesh.get("colors")), _t(mesh["normals"]), _t(mesh["cells"]), mesh["n_open"])


def _assert_fill(got, want, what=""):
    from coivo_amd import inference as I
    assert isinstance(got, I.HoleFill) and isinstance(got.mesh, I.Mesh) and len(got) == 8
    for k, dtype in (("status", torch.int32), ("hole", torch.int64), ("ring_offsets", torch.int32), ("ring_vertices", torch.int32),
                     ("face_loop", torch.int32), ("new_vertex_loop", torch.int32)):
        g, w = getattr(got, k), torch.from_numpy(np.ascontiguousarray(want[k]))
        assert g.dtype == dtype and g.shape == w.shape, (what, k, g.dtype, tuple(g.shape), tuple(w.shape))
        assert torch.equal(g.cpu(), w), (what, k)
    for k, dtype in (("faces", torch.int32), ("cells", torch.int32)):
        g, w = getattr(got.mesh, k), torch.from_numpy(np.ascontiguousarray(want[k]))
        assert g.dtype == dtype and g.shape == w.shape and torch.equal(g.cpu(), w), (what, k)
    for k in ("vertices", "normals", "colors"):
        g, w = getattr(got.mesh, k), want[k]
        assert (g is None) == (w is None), (what, k)
        if g is not None:
            w = torch.from_numpy(np.ascontiguousarray(w))
            assert g.dtype == torch.float32 and g.shape == w.shape and torch.equal(_bits(g).cpu(), _bits(w)), (what, k)
    assert got.mesh.n_open == want["n_open"] and got.unit == want["unit"], what
    assert torch.equal(got.hole_area.cpu(), torch.from_numpy(R.hole_area(want))) and got.hole_area.dtype == torch.float64
    assert torch.equal(got.filled.cpu(), torch.from_numpy(want["status"] == R.FILLED))
    assert torch.equal(got.simple.cpu(), torch.from_numpy(want["status"] != R.NOT_SIMPLE))


def _same(a, b):
    assert type(a) is type(b)
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x) if x.dtype == torch.float32 else x,
                                                                           _bits(y) if y.dtype == torch.float32 else y)
        elif isinstance(x, tuple):
            _same(x, y)
        else:
            assert x == y


def _fill(mesh, unit, max_edges):
    """(GPU HoleFill, GPU topology, the Mesh) of a replica-style mesh dict"""
    from coivo_amd import inference as I
    m = _gpu(mesh)
    topo = I.mesh_topology(m, unit=unit)
    return I.fill_holes(m, topo, max_edges=max_edges), topo, m


# ---- 1. the hand meshes in one --------------------------------------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def _hand_mesh():
    names = sorted(R.hand_meshes())
    v, f = T.concatenate([R.hand_meshes()[k] for k in names])
    v = np.concatenate([v, [[9, 9, 9]]]).astype(f32)                          # a lone vertex
    V = len(v)
    f = np.concatenate([f, [[0, 1, -1]], [[0, 1, V]], [[2, 2, 3]]]).astype(np.int32)       # dead faces: they are copied as they are
    v, f = T.renumber(v, f, 13)
    return R.as_mesh(v, f, seed=2), T.mesh_topology(v, f, 0.5)


@pytest.mark.parametrize("max_edges", [8, 66])
def test_hand_meshes_equal_the_replica(max_edges):
    mesh, wt = _hand_mesh()
    want = R.fill_holes(mesh, wt, max_edges)
    assert sorted(want["status"].tolist()) == sorted([0, 0, 0, 0, 2, 2, 2, 3] + [0 if max_edges == 66 else 1]) and wt["n_dead_faces"] == 3
    got, _, _ = _fill(mesh, 0.5, max_edges)
    _assert_fill(got, want, max_edges)
    # without colours the same, and no colours come back
    plain = dict(mesh, colors=None)
    _assert_fill(_fill(plain, 0.5, max_edges)[0], R.fill_holes(plain, wt, max_edges), "no colours")


# ---- 2. one long ring ------------------------------------------------------------------------------------------------------------------ #
@functools.lru_cache(maxsize=None)
def _strip(shuffled):
    v, f = T.triangle_strip(20000)
    if shuffled:
        v, f = T.renumber(v, f, 3)
        f = f[np.random.default_rng(4).permutation(len(f))]
    mesh = R.as_mesh(v, f, seed=6)
    topo = T.mesh_topology(v, f, 1.0)
    return mesh, topo, R.fill_holes(mesh, topo, 20002), R.fill_holes(mesh, topo, 3)


@pytest.mark.parametrize("shuffled", [False, True])
def test_a_ring_of_20002_edges(shuffled):
    mesh, wt, want, want3 = _strip(shuffled)
    assert wt["loops"][:, 2].tolist() == [20002] and int(np.ceil(np.log2(20002))) == 15
    assert want["status"].tolist() == [R.FILLED] and want["hole"][0, 0] == 20002 and len(want["vertices"]) == 20003
    assert len(want["ring_vertices"]) == 20002 and len(want["faces"]) == 40002
    got, _, _ = _fill(mesh, 1.0, 20002)
    _assert_fill(got, want, shuffled)
    assert want3["status"].tolist() == [R.TOO_LONG] and want3["hole"].tolist() == [[0, int(want["hole"][0, 1])]]
    got3, _, _ = _fill(mesh, 1.0, 3)
    _assert_fill(got3, want3, shuffled)
    assert torch.equal(got3.ring_vertices, got.ring_vertices)


# ---- 3. more loops than one scan chunk ------------------------------------------------------------------------------------------------ #
def test_5000_separate_triangles_and_5000_separate_squares():
    v, f = T.separate_triangles(5000)
    mesh, wt = R.as_mesh(v, f, seed=7), T.mesh_topology(v, f, 1.0)
    want = R.fill_holes(mesh, wt, 8)
    assert (want["status"] == R.FILLED).all() and len(want["status"]) == 5000 and len(want["vertices"]) == len(v)
    assert (want["hole"] == [1, 32768]).all() and len(want["faces"]) == 10000
    _assert_fill(_fill(mesh, 1.0, 8)[0], want, "triangles")
    v, f = R.separate_squares(5000)
    mesh, wt = R.as_mesh(v, f, seed=8), T.mesh_topology(v, f, 1.0)
    want = R.fill_holes(mesh, wt, 8)
    assert (want["hole"] == [4, 65536]).all() and len(want["vertices"]) == len(v) + 5000 and 5000 > 4096
    _assert_fill(_fill(mesh, 1.0, 8)[0], want, "squares")


# ---- 4. the project's own meshes ------------------------------------------------------------------------------------------------------ #
MAX_EDGES = {"thin": 8, "tube2": 12, "tube1": 8, "sphere": 8}                  # DESIGN.md §3.6q's table


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "sphere":
        return (*T.sphere_mesh(), 1)
    shape, Tv, min_obs = {"thin": ((5, 17, 23), 1, 2), "tube2": ((5, 24, 32), 4, 2), "tube1": ((5, 24, 32), 4, 1)}[name]
    return (*T.tube_mesh(*shape, Tv, min_obs), min_obs)


def _gpu_mesh(scene):
    from coivo_amd import inference as I
    wm, (depths, K, M, kw), min_obs = scene
    vol = I.fuse_tsdf(_t(depths), _t(K), _t(M), **{**kw, "colors": _t(kw.get("colors"))})
    return I.extract_mesh(vol, min_obs=min_obs)


def _assert_topology(got, want, what=""):
    for k in ("vertex_component", "face_component", "vertex_loop", "components", "loops"):
        g, w = getattr(got, k), torch.from_numpy(np.ascontiguousarray(want[k]))
        assert g.shape == w.shape and torch.equal(g.cpu(), w), (what, k)
    assert got.n_dead_faces == want["n_dead_faces"] and got.n_unmeasured == want["n_unmeasured"] and got.unit == want["unit"], what


@pytest.mark.parametrize("name", ["thin", "tube2", "tube1", "sphere"])
def test_extracted_meshes_equal_the_replica(name):
    from coivo_amd import inference as I
    scene = _scene(name)
    wm, unit = scene[0], scene[1][3]["voxel_size"]
    wt = T.mesh_topology(wm["vertices"], wm["faces"], unit)
    want = R.fill_holes(wm, wt, MAX_EDGES[name])
    mesh = _gpu_mesh(scene)
    topo = I.mesh_topology(mesh, unit=unit)
    got = I.fill_holes(mesh, topo, max_edges=MAX_EDGES[name])
    _assert_fill(got, want, name)
    assert (name == "sphere") == (len(want["status"]) == 0) and (name == "sphere" or int((want["status"] == R.FILLED).sum()) >= 10)
    after = I.mesh_topology(got.mesh, unit=unit)
    _assert_topology(after, T.mesh_topology(want["vertices"], want["faces"], unit), name)
    assert after.loops.shape[0] == topo.loops.shape[0] - int(got.filled.sum())


# ---- 5. schedule independence --------------------------------------------------------------------------------------------------------- #
def test_identical_bits_between_calls_streams_and_face_orders():
    from coivo_amd import inference as I
    wm = _scene("tube2")[0]
    mesh = _gpu(wm)
    topo = I.mesh_topology(mesh, unit=0.1)
    a = I.fill_holes(mesh, topo, max_edges=12)
    _same(a, I.fill_holes(mesh, topo, max_edges=12))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        b = I.fill_holes(mesh, topo, max_edges=12)
    side.synchronize()
    _same(a, b)
    F = mesh.faces.shape[0]
    perm = torch.from_numpy(np.random.default_rng(5).permutation(F)).to(dev())
    pmesh = mesh._replace(faces=mesh.faces[perm].contiguous())
    p = I.fill_holes(pmesh, I.mesh_topology(pmesh, unit=0.1), max_edges=12)
    assert torch.equal(p.mesh.faces[:F], a.mesh.faces[:F][perm]) and torch.equal(p.mesh.faces[F:], a.mesh.faces[F:])
    _same(a._replace(mesh=a.mesh._replace(faces=p.mesh.faces)), p)
    # the long ring too: 15 rounds of pointer jumping
    sm = _gpu(_strip(True)[0])
    st = I.mesh_topology(sm, unit=1.0)
    x = I.fill_holes(sm, st, max_edges=20002)
    fm = sm._replace(faces=sm.faces.flip(0).contiguous())
    y = I.fill_holes(fm, I.mesh_topology(fm, unit=1.0), max_edges=20002)
    _same(x._replace(mesh=x.mesh._replace(faces=y.mesh.faces)), y)
    assert torch.equal(x.mesh.faces[20000:], y.mesh.faces[20000:])


# ---- 6. the filled mesh downstream ---------------------------------------------------------------------------------------------------- #
def test_render_and_point_to_surface_take_the_filled_mesh():
    from coivo_amd import evaluate as E, inference as I
    scene = _scene("tube2")
    depths, K, M, _ = scene[1]
    mesh = _gpu_mesh(scene)
    topo = I.mesh_topology(mesh, unit=0.1)
    fill = I.fill_holes(mesh, topo, max_edges=12)
    F = mesh.faces.shape[0]
    assert fill.mesh.faces.shape[0] > F
    H, W = depths.shape[2:]
    opened = I.render_mesh(mesh, _t(K), _t(M), H, W, max_depth=T.TUBE_MAX_DEPTH)
    closed = I.render_mesh(fill.mesh, _t(K), _t(M), H, W, max_depth=T.TUBE_MAX_DEPTH)
    assert int((closed.index >= 0).sum()) >= int((opened.index >= 0).sum())
    won = closed.index >= F                                                  # the pixels a fill face wins
    print("pixels covered open / filled / won by a fill face:", int((opened.index >= 0).sum()), int((closed.index >= 0).sum()), int(won.sum()))
    assert bool(((opened.index[won] < 0) | (opened.depth[won] > closed.depth[won])).all())
    assert torch.equal(closed.index[~won], opened.index[~won]) and torch.equal(_bits(closed.depth)[~won], _bits(opened.depth)[~won])
    # point to surface: the new vertices lie on the filled surface, on their own fans; no point is farther from it than from the open one
    centres = fill.mesh.vertices[mesh.vertices.shape[0]:].contiguous()
    assert centres.shape[0] == fill.new_vertex_loop.shape[0] > 0
    on = E.point_to_surface(centres, fill.mesh, max_dist=0.4)
    assert bool((on.dist2 <= 1e-12).all()) and bool((on.face >= 0).all())
    own = on.face >= F                                                       # (an old face through a centre may tie with its fan)
    assert int(own.sum()) > 0 and torch.equal(fill.face_loop[on.face.long()][own], fill.new_vertex_loop[own])
    points = (mesh.vertices[::7] + 0.03).contiguous()
    a, b = E.point_to_surface(points, mesh, max_dist=0.4), E.point_to_surface(points, fill.mesh, max_dist=0.4)
    assert bool((b.dist2 <= a.dist2).all()) and bool((b.face >= 0).any())


def test_surface_reconstruction_metrics_fills_the_ground_truth_mesh():
    from coivo_amd import _args, evaluate as E, inference as I
    scene = _scene("tube2")
    depths, K, M, kw = scene[1]
    pred = _gpu_mesh(scene)
    G = torch.from_numpy(M)
    args = (pred, G, _t(depths), _t(K), G)
    common = dict(voxel_size=kw["voxel_size"], max_depth=T.TUBE_MAX_DEPTH, align="none")
    got = E.surface_reconstruction_metrics(*args, meshing=I.Meshing(fill_edges=12), **common)
    # the ground truth here is fused without colours, from the same depths: pred's geometry, filled
    gt = I.extract_mesh(I.fuse_tsdf(_t(depths), _t(K), _t(M), voxel_size=kw["voxel_size"], max_depth=T.TUBE_MAX_DEPTH), min_obs=2)
    assert torch.equal(gt.faces, pred.faces)
    fill = I.fill_holes(gt, I.mesh_topology(gt, unit=kw["voxel_size"]), max_edges=12)
    vs = _args.f32(kw["voxel_size"])
    _same(got, E.surface_metrics(pred, fill.mesh, max_dist=4.0 * vs, thresholds=(vs, 2.0 * vs)))
    plain = E.surface_reconstruction_metrics(*args, **common)
    assert got.n_gt == plain.n_gt + int(fill.new_vertex_loop.shape[0]) > plain.n_gt and got.n_pred == plain.n_pred


# ---- 7. degenerate inputs --------------------------------------------------------------------------------------------------------------- #
def test_nothing_launches_without_vertices_or_loops():
    from coivo_amd import inference as I
    empty = _gpu(R.as_mesh(np.zeros((0, 3)), np.zeros((0, 3))))
    r = I.fill_holes(empty, I.mesh_topology(empty, unit=1.0), max_edges=8)
    assert r.mesh is empty and r.status.shape == (0,) and r.hole.shape == (0, 2) and r.ring_offsets.tolist() == [0]
    assert r.ring_vertices.shape == (0,) and r.face_loop.shape == (0,) and r.new_vertex_loop.shape == (0,)
    closed = _gpu(R.as_mesh(*T.tetrahedron()))
    r = I.fill_holes(closed, I.mesh_topology(closed, unit=1.0), max_edges=8)
    assert r.mesh is closed and r.face_loop.tolist() == [-1] * 4 and r.status.dtype == torch.int32 and r.hole.dtype == torch.int64
    # a topology of another mesh is refused, by shape or by what the kernels find
    cube, tet = _gpu(R.as_mesh(*R.open_cube())), _gpu(R.as_mesh(*R.open_tetrahedron()))
    with pytest.raises(ValueError, match="topology is not this mesh's"):
        I.fill_holes(cube, I.mesh_topology(tet, unit=1.0), max_edges=8)
    shifted = I.mesh_topology(cube, unit=1.0)
    shifted = shifted._replace(vertex_loop=shifted.vertex_loop.roll(1))      # the right shapes, the wrong vertices
    with pytest.raises(RuntimeError, match="topology is not this mesh's"):
        I.fill_holes(cube, shifted, max_edges=8)


# ---- 8. the whole pipeline ------------------------------------------------------------------------------------------------------------- #
def test_reconstruct_sequence_fills_and_returns_the_holes():
    # reconstruct_sequence takes frames and networks, not depth maps, so the tubes of tests/topology_ref.py cannot go through it: this
    # is the network scene of tests/test_topology_gpu.py's pipeline test, whose mesh has small simple holes as well
    from coivo_amd import inference as I, nn as hnn, synth
    from oracle import colvo_spec as S
    dn_o, pn_o = S.make_models(31)
    dn, pn = hnn.DepthNet(), hnn.PoseNet()
    dn.load_state_dict(dn_o.state_dict())
    pn.load_state_dict(pn_o.state_dict())
    b = synth.make_batch(5, 64, 96, seed=31)
    frames, K = b["tgt"].to(dev()), b["K"].to(dev())
    kw = dict(stride=2, chunk=2, voxel_size=0.005, max_depth=0.5)            # tests/test_tsdf_gpu.py's scene
    plain = I.reconstruct_sequence(dn, pn, frames, K, mesh=I.Meshing(0.02, 2), **kw)
    zero = I.reconstruct_sequence(dn, pn, frames, K, mesh=I.Meshing(0.02, 2, fill_edges=0), **kw)
    assert plain.holes is None and zero.holes is None
    _same(plain.mesh, zero.mesh)
    _same(plain.topology, zero.topology)
    _same(tuple(plain), tuple(zero))
    rec = I.reconstruct_sequence(dn, pn, frames, K, mesh=I.Meshing(0.02, 2, fill_edges=12), render=I.Render(mesh=True), **kw)
    assert len(rec) == 5 and isinstance(rec.holes, I.HoleFill) and rec.mesh is rec.holes.mesh
    _same(rec.holes, I.fill_holes(plain.mesh, plain.topology, max_edges=12))
    _same(rec.topology, I.mesh_topology(rec.mesh, unit=0.005))
    assert int(rec.holes.filled.sum()) > 0 and rec.topology.loops.shape[0] == plain.topology.loops.shape[0] - int(rec.holes.filled.sum())
    assert rec.mesh.faces.shape[0] == plain.mesh.faces.shape[0] + int(rec.holes.hole[:, 0].sum())
    assert int(rec.rendered.index.max()) < rec.mesh.faces.shape[0]
    drawn = I.render_mesh(rec.mesh, K, rec.cam2world.to(dev(), torch.float32), 64, 96, max_depth=0.5)
    assert torch.equal(rec.rendered.index, drawn.index)


# ---- 9. memory discipline -------------------------------------------------------------------------------------------------------------- #
def test_memory_discipline():
    """fill_holes under tests/guarded.py: the mesh and its topology between guard bands, the scratch of colvo_mesh_fill_scratch_bytes, the
    ring tables and the filled mesh from the pool under both poisons.  Outputs equal the replica, are the same bytes under either poison,
    and no guard byte changes.  Launches reached: the hand meshes with max_edges = 8 run colvo_mesh_fill_plan and colvo_mesh_fill_write
    with every status (filled with and without a new vertex, too long, not simple), colours and dead faces; 5000 separate squares take
    the loops, the new vertices and the new faces past one scan chunk of 4096."""
    from coivo_amd import _lib, inference as I
    from tests import guarded as G
    lib = _lib.load()
    mesh, wt = _hand_mesh()
    v, f = R.separate_squares(5000)
    for name, mesh, wt, unit in (("hand meshes", mesh, wt, 0.5), ("5000 squares", R.as_mesh(v, f, seed=8), T.mesh_topology(v, f, 1.0), 1.0)):
        want = R.fill_holes(mesh, wt, 8)
        assert int((want["status"] == R.FILLED).sum()) > 0 and len(want["vertices"]) > len(mesh["vertices"])
        m = _gpu(mesh)
        topo = I.mesh_topology(m, unit=unit)
        outs, pools = G.under_both_poisons(dev(), lambda pool: I.fill_holes(pool.place_tree(m), pool.place_tree(topo), max_edges=8),
                                           f"fill_holes {name}")
        V, F, L = m.vertices.shape[0], m.faces.shape[0], topo.loops.shape[0]
        for got, pool in zip(outs, pools):
            _assert_fill(got, want, name)
            G.assert_served(pool, 0, lib.colvo_mesh_fill_scratch_bytes(V, F, L), name)
