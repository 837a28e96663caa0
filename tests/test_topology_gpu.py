"""-m gpu: mesh_topology / clean_mesh (coivo_amd.topology, csrc/topology.hip) against their NumPy replica (tests/topology_ref.py).
Labels are numbered by smallest vertex, counts and quanta are integer sums and the measures are float64 in a written association, so
every comparison here is equality to the bit, of every output."""
import functools

import numpy as np
import pytest
import torch

from tests import topology_ref as T
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

f32 = np.float32


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _topo(v, f, unit):
    from coivo_amd import inference as I
    return I.mesh_topology(_t(v), _t(f), unit=unit)


def _assert_topology(got, want, what=""):
    from coivo_amd import inference as I
    assert isinstance(got, I.MeshTopology)
    for k, dtype in (("vertex_component", torch.int32), ("face_component", torch.int32), ("vertex_loop", torch.int32),
                     ("components", torch.int64), ("loops", torch.int64)):
        g, w = getattr(got, k), torch.from_numpy(np.ascontiguousarray(want[k]))
        assert g.dtype == dtype and g.shape == w.shape, (what, k, g.dtype, tuple(g.shape), tuple(w.shape))
        assert torch.equal(g.cpu(), w), (what, k)
    assert got.n_dead_faces == want["n_dead_faces"] and got.n_unmeasured == want["n_unmeasured"], what
    assert got.unit == want["unit"], what
    assert torch.equal(got.euler.cpu(), torch.from_numpy(T.euler(want))) and torch.equal(got.closed.cpu(), torch.from_numpy(T.closed(want)))
    assert torch.equal(got.area.cpu(), torch.from_numpy(want["components"][:, 7].astype(np.float64) * T.quanta(want["unit"])[0]))


def _same(a, b):
    assert type(a) is type(b)
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y)
        else:
            assert x == y


# ---- 1. one hand mesh ---------------------------------------------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def _hand_mesh():
    v, f = T.concatenate([T.tetrahedron(), T.square_strip(4), T.annulus(8), T.book(3), T.right_triangle()])
    v = np.concatenate([v, [[9, 9, 9]]]).astype(f32)                          # a lone vertex
    V = len(v)
    f = np.concatenate([f, f[-1:], [[0, 1, -1]], [[0, 1, V]], [[2, 2, 3]], [[2 ** 31 - 1, 0, 1]]]).astype(np.int32)
    return T.renumber(v, f, 11)


def test_hand_mesh_equals_the_replica():
    v, f = _hand_mesh()
    want = T.mesh_topology(v, f, 0.25)
    c = want["components"]
    assert len(c) == 6 and want["n_dead_faces"] == 4 and len(want["loops"]) == 4
    assert sorted(c[:, 2].tolist()) == [0, 2, 3, 4, 8, 16] and int(c[:, 5].sum()) == 1     # (the triangle and its duplicate: 2 faces)
    assert sorted(T.euler(want).tolist()) == [0, 1, 1, 1, 2, 2] and int(T.closed(want).sum()) == 2
    assert (np.diff(want["vertex_component"]) < 0).any()                                # the components interleave
    _assert_topology(_topo(v, f, 0.25), want)
    # a Mesh is taken apart the same way
    from coivo_amd import inference as I
    mesh = I.Mesh(_t(v), _t(f), None, _t(v), torch.zeros(len(v), 3, device=dev(), dtype=torch.int32), 0)
    _assert_topology(I.mesh_topology(mesh, unit=0.25), want)


# ---- 2. deep chains ------------------------------------------------------------------------------------------------------------------ #
@functools.lru_cache(maxsize=None)
def _strip(shuffled):
    v, f = T.triangle_strip(20000)
    if shuffled:
        v, f = T.renumber(v, f, 3)
        f = f[np.random.default_rng(4).permutation(len(f))]
    return v, f, T.mesh_topology(v, f, 1.0)


@pytest.mark.parametrize("shuffled", [False, True])
def test_a_strip_of_20000_triangles_is_one_component_and_one_loop(shuffled):
    v, f, want = _strip(shuffled)
    assert want["components"].tolist() == [[0, 20002, 20000, 40001, 20002, 0, 1, 10000 * 65536]]
    assert want["loops"].tolist() == [[0, 0, 20002, 20002 * 65536]]
    _assert_topology(_topo(v, f, 1.0), want, shuffled)


# ---- 3. more roots than one scan chunk ----------------------------------------------------------------------------------------------- #
def test_5000_separate_triangles():
    v, f = T.separate_triangles(5000)
    want = T.mesh_topology(v, f, 1.0)
    assert len(want["components"]) == len(want["loops"]) == 5000 > 4096
    assert (want["components"][:, 1:] == [3, 1, 3, 3, 0, 1, 32768]).all()
    _assert_topology(_topo(v, f, 1.0), want)


# ---- 4. one high-degree vertex -------------------------------------------------------------------------------------------------------- #
def test_a_fan_of_64_triangles():
    v, f = T.fan(64)
    want = T.mesh_topology(v, f, 0.5)
    assert want["components"][0, :7].tolist() == [0, 66, 64, 129, 66, 0, 1]
    _assert_topology(_topo(v, f, 0.5), want)
    # ... and with the hub as the LARGER endpoint of every spoke
    v2, f2 = v[::-1].copy(), (len(v) - 1 - f).astype(np.int32)
    _assert_topology(_topo(v2, f2, 0.5), T.mesh_topology(v2, f2, 0.5))


# ---- 5. the project's own meshes ------------------------------------------------------------------------------------------------------ #
def _gpu_mesh(scene):
    from coivo_amd import inference as I
    wm, (depths, K, M, kw), min_obs = scene
    vol = I.fuse_tsdf(_t(depths), _t(K), _t(M), **{**kw, "colors": _t(kw.get("colors"))})
    return I.extract_mesh(vol, min_obs=min_obs)


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "sphere":
        return (*T.sphere_mesh(), 1)
    shape, Tv, min_obs = {"thin": ((5, 17, 23), 1, 2), "tube2": ((5, 24, 32), 4, 2), "tube1": ((5, 24, 32), 4, 1)}[name]
    return (*T.tube_mesh(*shape, Tv, min_obs), min_obs)


@pytest.mark.parametrize("name", ["thin", "tube2", "tube1", "sphere"])
def test_extracted_meshes_equal_the_replica(name):
    from coivo_amd import inference as I
    scene = _scene(name)
    wm, unit = scene[0], scene[1][3]["voxel_size"]
    want = T.mesh_topology(wm["vertices"], wm["faces"], unit)
    c = want["components"]
    if name == "sphere":
        assert int((c[:, 2] > 0).sum()) == 1 and T.closed(want)[c[:, 2] > 0].all() and len(want["loops"]) == 0
    else:
        assert int((c[:, 2] == 0).sum()) > 0 and len(want["loops"]) >= 13                 # face-less vertices, holes
    if name == "thin":
        assert int((c[:, 2] > 0).sum()) >= 33
    mesh = _gpu_mesh(scene)
    assert torch.equal(mesh.faces.cpu(), torch.from_numpy(wm["faces"]))
    got = I.mesh_topology(mesh, unit=unit)
    _assert_topology(got, want, name)


# ---- 6. schedule independence --------------------------------------------------------------------------------------------------------- #
def test_identical_bits_between_calls_streams_and_face_orders():
    from coivo_amd import inference as I
    wm = _scene("tube2")[0]
    v, f = _t(wm["vertices"]), _t(wm["faces"])
    a = I.mesh_topology(v, f, unit=0.1)
    _same(a, I.mesh_topology(v, f, unit=0.1))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        b = I.mesh_topology(v, f, unit=0.1)
    side.synchronize()
    _same(a, b)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(len(wm["faces"]))).to(dev())
    p = I.mesh_topology(v, f[perm].contiguous(), unit=0.1)
    assert torch.equal(p.face_component, a.face_component[perm])
    _same(a._replace(face_component=p.face_component), p)
    # the deep strip too: its unions race along one chain
    sv, sf, _ = _strip(True)
    sv, sf = _t(sv), _t(sf)
    _same(I.mesh_topology(sv, sf, unit=1.0), I.mesh_topology(sv, sf.flip(0).contiguous(), unit=1.0))     # (every face is in component 0)


# ---- 7. clean_mesh -------------------------------------------------------------------------------------------------------------------- #
def _bits(t):
    return t.contiguous().view(torch.int32)


def _small_area(topo):
    """an area between the smallest and the second smallest fragment with faces"""
    c = topo["components"]
    a = np.unique(c[c[:, 2] > 0, 7]).astype(np.float64) * T.quanta(topo["unit"])[0]
    return float(a[0] + a[1]) / 2


@pytest.mark.parametrize("case", ["min_faces_1", "min_faces_5", "largest_1", "min_area"])
def test_clean_mesh_equals_the_replica(case):
    from coivo_amd import inference as I
    scene = _scene("thin")
    wm = scene[0]
    wt = T.mesh_topology(wm["vertices"], wm["faces"], 0.1)
    kw = {"min_faces_1": {}, "min_faces_5": dict(min_faces=5), "largest_1": dict(largest=1),
          "min_area": dict(min_area=_small_area(wt))}[case]
    want = T.clean_mesh(wm, wt, **kw)
    assert 0 < int(want["kept"].sum()) < len(wt["components"]) and 0 < len(want["faces"]) <= len(wm["faces"])
    if case != "min_faces_1":
        assert len(want["faces"]) < len(wm["faces"])
    mesh = _gpu_mesh(scene)
    topo = I.mesh_topology(mesh, unit=0.1)
    got = I.clean_mesh(mesh, topo, **kw)
    assert isinstance(got, I.CleanedMesh) and isinstance(got.mesh, I.Mesh) and got.mesh.n_open == mesh.n_open
    assert got.kept.dtype == torch.bool and torch.equal(got.kept.cpu(), torch.from_numpy(want["kept"]))
    assert got.vertex_index.dtype == torch.int32 and torch.equal(got.vertex_index.cpu(), torch.from_numpy(want["vertex_index"]))
    assert got.face_index.dtype == torch.int32 and torch.equal(got.face_index.cpu(), torch.from_numpy(want["face_index"]))
    assert got.mesh.faces.dtype == torch.int32 and torch.equal(got.mesh.faces.cpu(), torch.from_numpy(want["faces"]))
    assert torch.equal(got.mesh.cells.cpu(), torch.from_numpy(want["cells"]))
    for k in ("vertices", "normals", "colors"):
        assert torch.equal(_bits(getattr(got.mesh, k)).cpu(), _bits(torch.from_numpy(want[k]))), k
        # the gathered rows are the old rows' bits
        assert torch.equal(_bits(getattr(got.mesh, k)), _bits(getattr(mesh, k)[got.vertex_index.long()])), k
    # the result's own topology: nothing below the threshold, no face-less vertex, no dead face
    t2 = I.mesh_topology(got.mesh, unit=0.1)
    _assert_topology(t2, T.mesh_topology(want["vertices"], want["faces"], 0.1), case)
    assert int(t2.components[:, 2].min()) >= max(kw.get("min_faces", 1), 1) and t2.n_dead_faces == 0
    assert t2.components.shape[0] == int(want["kept"].sum())
    assert torch.equal(t2.components[:, 1:], topo.components[got.kept][:, 1:])


def test_render_of_the_cleaned_mesh_draws_the_faces_face_index_names():
    from coivo_amd import inference as I
    scene = _scene("thin")
    depths, K, M, _ = scene[1]
    mesh = _gpu_mesh(scene)
    topo = I.mesh_topology(mesh, unit=0.1)
    cleaned = I.clean_mesh(mesh, topo, min_faces=5)
    H, W = depths.shape[2:]
    full = I.render_mesh(mesh, _t(K), _t(M), H, W, max_depth=T.TUBE_MAX_DEPTH)
    part = I.render_mesh(cleaned.mesh, _t(K), _t(M), H, W, max_depth=T.TUBE_MAX_DEPTH)
    new_row = torch.full((mesh.faces.shape[0],), -1, device=dev(), dtype=torch.int64)
    new_row[cleaned.face_index.long()] = torch.arange(cleaned.face_index.shape[0], device=dev())
    won, won2 = full.index.long(), part.index.long()
    kept_winner = (won >= 0) & (new_row[won.clamp(min=0)] >= 0)
    dropped_winner = (won >= 0) & ~kept_winner
    assert int(kept_winner.sum()) > 0 and int(dropped_winner.sum()) > 0
    old_of_won2 = torch.where(won2 >= 0, cleaned.face_index.long()[won2.clamp(min=0)], won2)
    assert torch.equal(old_of_won2[kept_winner], won[kept_winner])
    assert torch.equal(_bits(part.depth)[kept_winner], _bits(full.depth)[kept_winner])
    assert (new_row[old_of_won2[won2 >= 0]] >= 0).all()                        # nothing else is ever drawn


# ---- 8. degenerate inputs -------------------------------------------------------------------------------------------------------------- #
def test_degenerate_inputs_give_empty_well_formed_results():
    from coivo_amd import inference as I
    z3 = torch.zeros(0, 3, device=dev())
    no_faces = torch.zeros(0, 3, device=dev(), dtype=torch.int32)
    # V = 0, with and without faces (all dead)
    for f in (no_faces, torch.tensor([[0, 1, 2], [-1, 0, 0]], device=dev(), dtype=torch.int32)):
        t = I.mesh_topology(z3, f, unit=1.0)
        _assert_topology(t, T.mesh_topology(np.zeros((0, 3), f32), f.cpu().numpy(), 1.0))
        assert t.components.shape == (0, 8) and t.loops.shape == (0, 4) and t.n_dead_faces == f.shape[0]
        assert t.euler.shape == (0,) and t.closed.shape == (0,) and t.area.shape == (0,)
        mesh = I.Mesh(z3, f, None, z3, torch.zeros(0, 3, device=dev(), dtype=torch.int32), 3)
        c = I.clean_mesh(mesh, t)
        assert c.mesh.vertices.shape == (0, 3) and c.mesh.faces.shape == (0, 3) and c.mesh.faces.dtype == torch.int32
        assert c.mesh.n_open == 3 and c.mesh.colors is None and c.kept.shape == (0,) and c.vertex_index.shape == (0,) == c.face_index.shape
    # F = 0 with V > 0: V components of one vertex; all faces dead: the same
    v = np.random.default_rng(1).random((5, 3)).astype(f32)
    for f in (np.zeros((0, 3), np.int32), np.array([[0, 0, 1], [0, 1, 5], [-1, 2, 3]], np.int32)):
        want = T.mesh_topology(v, f, 1.0)
        assert want["components"].tolist() == [[i, 1, 0, 0, 0, 0, 0, 0] for i in range(5)] and want["loops"].shape == (0, 4)
        got = _topo(v, f, 1.0)
        _assert_topology(got, want)
        mesh = I.Mesh(_t(v), _t(f), _t(v), _t(v), torch.zeros(5, 3, device=dev(), dtype=torch.int32), 0)
        c = I.clean_mesh(mesh, got)                                           # everything goes
        assert c.mesh.vertices.shape == (0, 3) and c.mesh.colors.shape == (0, 3) and c.mesh.faces.shape == (0, 3)
        assert not c.kept.any() and c.kept.shape == (5,)
        c = I.clean_mesh(mesh, got, min_faces=0)                              # everything stays, but for the dead faces
        assert torch.equal(_bits(c.mesh.vertices), _bits(mesh.vertices)) and c.mesh.faces.shape == (0, 3) and c.kept.all()
        assert c.vertex_index.tolist() == [0, 1, 2, 3, 4]


# ---- 9. the whole pipeline ------------------------------------------------------------------------------------------------------------- #
def test_reconstruct_sequence_returns_the_topology_and_cleans():
    from coivo_amd import _args, inference as I, nn as hnn, synth
    from oracle import colvo_spec as S
    dn_o, pn_o = S.make_models(31)
    dn, pn = hnn.DepthNet(), hnn.PoseNet()
    dn.load_state_dict(dn_o.state_dict())
    pn.load_state_dict(pn_o.state_dict())
    b = synth.make_batch(5, 64, 96, seed=31)
    frames, K = b["tgt"].to(dev()), b["K"].to(dev())
    kw = dict(stride=2, chunk=2, voxel_size=0.005, max_depth=0.5)            # tests/test_tsdf_gpu.py's scene
    plain = I.reconstruct_sequence(dn, pn, frames, K, mesh=I.Meshing(0.02, 2), **kw)
    assert I.Meshing(0.02, 2).min_faces == 0
    vol = I.fuse_tsdf(plain.depths, K, plain.cam2world.to(dev(), torch.float32), voxel_size=0.005, trunc=0.02,
                      colors=frames.float().contiguous(), stride=2, max_depth=0.5)
    raw = I.extract_mesh(vol, min_obs=2)
    _same(plain.mesh, raw)
    assert isinstance(plain.topology, I.MeshTopology) and plain.topology.unit == _args.f32(0.005)
    _same(plain.topology, I.mesh_topology(raw, unit=0.005))
    rec = I.reconstruct_sequence(dn, pn, frames, K, mesh=I.Meshing(0.02, 2, min_faces=4), render=I.Render(mesh=True), **kw)
    assert len(rec) == 5 and isinstance(rec.topology, I.MeshTopology) and rec.mesh.faces.shape[0] > 0
    assert int(rec.topology.components[:, 2].min()) >= 4 and rec.topology.n_dead_faces == 0
    _same(rec.mesh, I.clean_mesh(raw, plain.topology, min_faces=4).mesh)
    _same(rec.topology, I.mesh_topology(rec.mesh, unit=0.005))
    assert rec.topology.vertex_component.shape[0] == rec.mesh.vertices.shape[0] < raw.vertices.shape[0]
    assert int(rec.rendered.index.max()) < rec.mesh.faces.shape[0]


# ---- 10. memory discipline -------------------------------------------------------------------------------------------------------------- #
def test_memory_discipline():
    """mesh_topology and clean_mesh under tests/guarded.py: inputs between guard bands, every tensor the wrappers allocate (the scratch of
    colvo_mesh_topology_scratch_bytes / colvo_mesh_clean_scratch_bytes, the label arrays, the tables, the gathered mesh) from the pool
    under both poisons.  Outputs equal the replica, are the same bytes under either poison, and no guard byte changes.
    Launches reached: the hand mesh runs colvo_mesh_topology_components, _edges and _loops (4 loops, dead faces, a lone vertex); 5000
    separate triangles take the roots and the loops past one scan chunk of 4096; clean_mesh(min_faces=5) on the thin tube's mesh runs
    colvo_mesh_clean_plan and colvo_mesh_clean_write with colours."""
    from coivo_amd import _lib, inference as I
    from tests import guarded as G
    lib = _lib.load()
    for name, (v, f), unit in (("hand mesh", _hand_mesh(), 0.25), ("5000 triangles", T.separate_triangles(5000), 1.0)):
        want = T.mesh_topology(v, f, unit)
        outs, pools = G.under_both_poisons(dev(), lambda pool: I.mesh_topology(pool.place(_t(v)), pool.place(_t(f)), unit=unit),
                                           f"mesh_topology {name}")
        for got, pool in zip(outs, pools):
            _assert_topology(got, want, name)
            G.assert_served(pool, 0, lib.colvo_mesh_topology_scratch_bytes(len(v), len(f)), name)
    scene = _scene("thin")
    wm = scene[0]
    want = T.clean_mesh(wm, T.mesh_topology(wm["vertices"], wm["faces"], 0.1), min_faces=5)
    mesh = _gpu_mesh(scene)
    topo = I.mesh_topology(mesh, unit=0.1)
    assert mesh.colors is not None and 0 < len(want["faces"]) < len(wm["faces"])
    outs, pools = G.under_both_poisons(dev(), lambda pool: I.clean_mesh(pool.place_tree(mesh), pool.place_tree(topo), min_faces=5),
                                       "clean_mesh")
    for got, pool in zip(outs, pools):
        G.assert_served(pool, 0, lib.colvo_mesh_clean_scratch_bytes(mesh.vertices.shape[0], mesh.faces.shape[0]), "clean_mesh")
        for g, k in ((got.kept, "kept"), (got.vertex_index, "vertex_index"), (got.face_index, "face_index"), (got.mesh.faces, "faces"),
                     (got.mesh.cells, "cells")):
            assert torch.equal(g.cpu(), torch.from_numpy(want[k])), k
        for k in ("vertices", "normals", "colors"):
            assert torch.equal(_bits(getattr(got.mesh, k)).cpu(), _bits(torch.from_numpy(want[k]))), k
