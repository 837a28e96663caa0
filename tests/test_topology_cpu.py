"""No GPU: the mesh topology replica (tests/topology_ref.py) on meshes whose every number is known by hand and on the project's own
meshes (the replica of extract_mesh, tests/tsdf_ref.py); what mesh_topology / clean_mesh and the colvo_mesh_* entry points refuse; the
Meshing policy's third field and the new names of coivo_amd.inference."""
import importlib

import numpy as np
import pytest
import torch

from tests import topology_ref as T


def _row(topo, c=0):
    return [int(x) for x in topo["components"][c]]


# ---- 1. hand meshes ------------------------------------------------------------------------------------------------------------------ #
def test_tetrahedron_is_closed_with_euler_two():
    t = T.mesh_topology(*T.tetrahedron(), 1.0)
    assert _row(t)[:7] == [0, 4, 4, 6, 0, 0, 0] and len(t["loops"]) == 0
    assert T.euler(t).tolist() == [2] and T.closed(t).tolist() == [True]
    assert (t["vertex_component"] == 0).all() and (t["face_component"] == 0).all() and (t["vertex_loop"] == -1).all()
    # three right triangles of area 1/2 and one equilateral of side sqrt 2: sqrt(3)/2
    assert _row(t)[7] == 3 * 32768 + int(np.rint(np.sqrt(3.0) / 2 * 65536))
    assert t["n_dead_faces"] == 0 and t["n_unmeasured"] == 0


def test_square_strip_has_one_loop():
    n = 5
    t = T.mesh_topology(*T.square_strip(n), 1.0)
    # 2 n triangles over 2 n + 2 vertices: 4 n + 1 edges, 2 n + 2 of them on the one boundary loop, whose length is 2 n + 2
    assert _row(t) == [0, 2 * n + 2, 2 * n, 4 * n + 1, 2 * n + 2, 0, 1, n * 65536]
    assert t["loops"].tolist() == [[0, 0, 2 * n + 2, (2 * n + 2) * 65536]]
    assert T.euler(t).tolist() == [1] and T.closed(t).tolist() == [False] and (t["vertex_loop"] == 0).all()


def test_annulus_has_two_loops_and_euler_zero():
    k = 8
    t = T.mesh_topology(*T.annulus(k), 1.0)
    assert _row(t)[:7] == [0, 2 * k, 2 * k, 4 * k, 2 * k, 0, 2]
    assert t["loops"][:, :3].tolist() == [[0, 0, k], [k, 0, k]]
    assert T.euler(t).tolist() == [0]
    assert t["vertex_loop"].tolist() == [0] * k + [1] * k
    # the rings are regular octagons of circumradius 1 and 2: side 2 r sin(pi / 8); float32 coordinates move a side by < 1e-6
    side = 2 * np.sin(np.pi / k) * 65536
    assert abs(int(t["loops"][0, 3]) - k * side) < k and abs(int(t["loops"][1, 3]) - 2 * k * side) < 2 * k


def test_three_triangles_on_one_edge_make_it_non_manifold():
    t = T.mesh_topology(*T.book(3), 1.0)
    # 5 vertices, 3 faces, 1 + 6 edges; the shared edge has three sides, the six others one each
    assert _row(t)[:7] == [0, 5, 3, 7, 6, 1, 1]
    assert T.closed(t).tolist() == [False] and T.euler(t).tolist() == [1]
    assert t["vertex_loop"].tolist() == [0] * 5 and t["loops"][0, :3].tolist() == [0, 0, 6]
    two = T.mesh_topology(*T.book(2), 1.0)
    assert _row(two)[:7] == [0, 4, 2, 5, 4, 0, 1]


def test_unit_right_triangle_measures_exactly():
    t = T.mesh_topology(*T.right_triangle(), 1.0)
    hyp = int(np.rint(np.sqrt(2.0) * 65536))
    assert hyp == 92682
    assert _row(t) == [0, 3, 1, 3, 3, 0, 1, 32768]
    assert t["loops"].tolist() == [[0, 0, 3, 2 * 65536 + hyp]]
    # another unit: the quanta scale with it (0.5 -> areas x 4, lengths x 2)
    h = T.mesh_topology(*T.right_triangle(), 0.5)
    assert _row(h)[7] == 4 * 32768 and int(h["loops"][0, 3]) == 4 * 65536 + int(np.rint(np.sqrt(2.0) * 131072))


def test_dead_faces_lone_vertices_duplicates_and_unmeasured():
    v, f = T.right_triangle()
    v = np.concatenate([v, [[5, 5, 5]], [[np.inf, 0, 0]]]).astype(np.float32)           # a lone vertex (3), a vertex at infinity (4)
    f = np.concatenate([f, f, [[0, 1, -1]], [[0, 1, 5]], [[0, 1, 1]], [[0, 1, 4]]]).astype(np.int32)
    t = T.mesh_topology(v, f, 1.0)
    assert t["n_dead_faces"] == 3 and t["face_component"].tolist() == [0, 0, -1, -1, -1, 0]
    assert t["vertex_component"].tolist() == [0, 0, 0, 1, 0]
    # edges: (0,1) three sides; (1,2), (0,2) two each (the duplicate); (1,4), (0,4) one each
    assert _row(t, 0)[:7] == [0, 4, 3, 5, 2, 1, 1] and _row(t, 1) == [3, 1, 0, 0, 0, 0, 0, 0]
    assert _row(t, 0)[7] == 2 * 32768                                                    # the face at infinity adds nothing
    assert t["n_unmeasured"] == 1 + 2 and t["loops"].tolist() == [[0, 0, 2, 0]]
    assert t["vertex_loop"].tolist() == [0, 0, -1, -1, 0]


def test_renumbering_and_face_order_only_permute():
    v, f = T.concatenate([T.tetrahedron(), T.annulus(), T.book(3), T.square_strip(4)])
    a = T.mesh_topology(v, f, 0.25)
    assert [int(x) for x in a["components"][:, 6]] == [0, 2, 1, 1] and len(a["loops"]) == 4
    v2, f2 = T.renumber(v, f, 7)
    order = np.random.default_rng(8).permutation(len(f2))
    b = T.mesh_topology(v2, f2[order], 0.25)
    key = lambda t: sorted(tuple(int(x) for x in r[1:]) for r in t["components"])
    assert key(a) == key(b)
    assert sorted(tuple(r[2:]) for r in a["loops"].tolist()) == sorted(tuple(r[2:]) for r in b["loops"].tolist())


# ---- 2. the project's meshes --------------------------------------------------------------------------------------------------------- #
tube_mesh, sphere_mesh, SPHERE = T.tube_mesh, T.sphere_mesh, T.SPHERE


# (N, H, W), T, min_obs -> V, F, components, with faces, largest (faces), face-less vertices, boundary edges, loops, non-manifold edges
TUBES = [((5, 17, 23), 1, 2, (507, 114, 363, 33, 26, 330, 174, 33, 0)),
         ((5, 24, 32), 4, 2, (2054, 3498, 66, 1, 3498, 65, 538, 23, 0)),
         ((5, 24, 32), 4, 1, (2397, 4328, 54, 1, 4328, 53, 384, 13, 0))]


@pytest.mark.parametrize("shape,Tv,min_obs,want", TUBES)
def test_tubes_have_the_recorded_topology(shape, Tv, min_obs, want):
    m, _ = tube_mesh(*shape, Tv, min_obs)
    t = T.mesh_topology(m["vertices"], m["faces"], 0.1)
    c = t["components"]
    with_faces = c[:, 2] > 0
    got = (len(m["vertices"]), len(m["faces"]), len(c), int(with_faces.sum()), int(c[:, 2].max()), int((~with_faces).sum()),
           int(c[:, 4].sum()), len(t["loops"]), int(c[:, 5].sum()))
    assert got == want
    assert t["n_dead_faces"] == 0 and t["n_unmeasured"] == 0
    assert (c[~with_faces, 1] == 1).all()                                    # a face-less vertex is a component of one vertex
    assert int(c[:, 6].sum()) == len(t["loops"]) and int(t["loops"][:, 2].sum()) == int(c[:, 4].sum())
    # the sides of one smaller endpoint: what the kernel's bucket scan is quadratic in
    f = m["faces"].astype(np.int64)
    sides = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    assert np.bincount(sides.min(1)).max() == (8 if Tv == 1 else 12)


def test_sphere_is_one_closed_component():
    m, _ = sphere_mesh()
    t = T.mesh_topology(m["vertices"], m["faces"], SPHERE["voxel"])
    c = t["components"]
    with_faces = c[:, 2] > 0
    assert int(with_faces.sum()) == 1 and len(m["faces"]) > 1000
    assert T.euler(t)[with_faces].tolist() == [2] and T.closed(t)[with_faces].tolist() == [True] and len(t["loops"]) == 0
    assert (c[~with_faces, 1] == 1).all() and (t["vertex_loop"] == -1).all()
    # a polyhedron with its vertices within a voxel of the sphere: its area is within (1 +- 1 / r)^2 of 4 pi r^2, r in voxels
    r = SPHERE["radius_voxels"]
    area = int(c[with_faces, 7][0]) / 65536
    assert 4 * np.pi * (r - 1) ** 2 < area < 4 * np.pi * (r + 1) ** 2


def test_replica_clean_mesh_on_the_thin_tube():
    m, _ = tube_mesh(5, 17, 23, 1, 2)
    t = T.mesh_topology(m["vertices"], m["faces"], 0.1)
    c = T.clean_mesh(m, t)
    assert len(c["vertices"]) == 507 - 330 and len(c["faces"]) == 114 and int(c["kept"].sum()) == 33
    t2 = T.mesh_topology(c["vertices"], c["faces"], 0.1)
    assert len(t2["components"]) == 33 and (t2["components"][:, 2] > 0).all()
    assert (t2["components"][:, 1:] == t["components"][c["kept"]][:, 1:]).all()
    assert np.array_equal(c["vertices"], m["vertices"][c["vertex_index"]])
    one = T.clean_mesh(m, t, largest=1)
    assert len(one["faces"]) == 26 and int(one["kept"].sum()) == 1
    five = T.clean_mesh(m, t, min_faces=5)
    assert 0 < int(five["kept"].sum()) < 33 and (t["components"][five["kept"], 2] >= 5).all()


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.ensure()
    return _lib.load()


def test_python_entry_points_refuse_bad_arguments():
    from coivo_amd import inference as I
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    for unit in (0.0, -1.0, float("nan"), float("inf"), None, 1e39):
        with pytest.raises(ValueError, match="mesh_topology: unit"):
            I.mesh_topology(v, f, unit=unit)
    with pytest.raises(TypeError):
        I.mesh_topology(v, f)                                                # unit is required
    with pytest.raises(ValueError, match=r"vertices must be \[V,3\]"):
        I.mesh_topology(torch.zeros(3, 2), f, unit=1.0)
    with pytest.raises(ValueError, match=r"faces must be \[F,3\] int32"):
        I.mesh_topology(v, f.long(), unit=1.0)
    with pytest.raises(ValueError, match=r"faces must be \[F,3\] int32"):
        I.mesh_topology(v, None, unit=1.0)
    with pytest.raises(ValueError, match="expected a float32 CUDA tensor"):
        I.mesh_topology(v, f, unit=1.0)                                      # no CPU path
    mesh = I.Mesh(v, f, None, v, torch.zeros(3, 3, dtype=torch.int32), 0)
    with pytest.raises(ValueError, match="with a Mesh give no faces"):
        I.mesh_topology(mesh, f, unit=1.0)
    topo = I.MeshTopology(torch.zeros(3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(3, dtype=torch.int32),
                          torch.zeros(1, 8, dtype=torch.int64), torch.zeros(0, 4, dtype=torch.int64), 0, 0, 1.0)
    with pytest.raises(ValueError, match="mesh must be a Mesh"):
        I.clean_mesh(v, topo)
    with pytest.raises(ValueError, match="topology must be a MeshTopology"):
        I.clean_mesh(mesh, None)
    for kw in (dict(min_faces=-1), dict(min_faces=1.5), dict(min_faces=True), dict(largest=0), dict(largest=2.0)):
        with pytest.raises(ValueError, match="must be an int"):
            I.clean_mesh(mesh, topo, **kw)
    for bad in (-1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="min_area must be finite"):
            I.clean_mesh(mesh, topo, min_area=bad)


def test_topology_properties_are_plain_arithmetic():
    from coivo_amd import inference as I
    comps = torch.tensor([[0, 4, 4, 6, 0, 0, 0, 65536], [4, 3, 1, 3, 3, 0, 1, 32768], [7, 1, 0, 0, 0, 0, 0, 0]])
    loops = torch.tensor([[4, 1, 3, 3 * 65536]])
    z = torch.zeros(0, dtype=torch.int32)
    t = I.MeshTopology(z, z, z, comps, loops, 0, 0, 0.5)
    assert t.euler.tolist() == [2, 1, 1] and t.closed.tolist() == [True, False, False]
    assert t.area.dtype == torch.float64 and t.area.tolist() == [0.25, 0.125, 0.0] and t.length.tolist() == [1.5]
    assert t.area_quantum == 0.25 / 65536 and t.length_quantum == 0.5 / 65536 and len(t) == 8


def test_entry_points_refuse_before_any_hip_call(lib):
    import ctypes as C
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert lib.colvo_mesh_topology_scratch_bytes(0, 0) == 0 and lib.colvo_mesh_topology_scratch_bytes(-1, 4) == 0
    assert lib.colvo_mesh_topology_scratch_bytes(4, -1) == 0 and lib.colvo_mesh_topology_scratch_bytes(4, 2 ** 29) == 0
    assert lib.colvo_mesh_topology_scratch_bytes(2 ** 31 - 1, 2 ** 29 - 1) > 0 and lib.colvo_mesh_topology_scratch_bytes(1, 0) > 0
    assert lib.colvo_mesh_clean_scratch_bytes(0, 0) == 0 and lib.colvo_mesh_clean_scratch_bytes(4, 2 ** 29) == 0
    assert lib.colvo_mesh_clean_scratch_bytes(4, 4) > 0

    def refused(name, *args):
        assert getattr(lib, name)(*args) != 0, name
        msg = lib.colvo_last_error().decode()
        assert msg.startswith(name + ":"), msg
        return msg

    for V, F in ((0, 1), (-3, 1), (4, -1), (4, 2 ** 29)):
        assert "bad shape" in refused("colvo_mesh_topology_components", p, V, F, p, p, p, p, 0)
        assert "bad shape" in refused("colvo_mesh_topology_edges", p, p, V, F, 1.0, 1, p, p, p, p, p, p, 0)
        assert "bad shape" in refused("colvo_mesh_topology_loops", p, V, F, 1.0, 1, 1, p, p, p, p, p, p, 0)
        assert "bad shape" in refused("colvo_mesh_clean_plan", p, p, p, V, F, 1, p, p, p, p, p, 0)
        assert "bad shape" in refused("colvo_mesh_clean_write", p, p, p, p, p, V, F, p, p, p, 1, 1, p, p, p, p, p, 0)
    assert "null pointer" in refused("colvo_mesh_topology_components", 0, 4, 2, p, p, p, p, 0)
    assert "null pointer" in refused("colvo_mesh_topology_components", p, 4, 2, 0, p, p, p, 0)
    assert "16-byte aligned" in refused("colvo_mesh_topology_components", p, 4, 2, p + 4, p, p, p, 0)
    for C_ in (0, 5):
        assert "C = " in refused("colvo_mesh_topology_edges", p, p, 4, 2, 1.0, C_, p, p, p, p, p, p, 0)
        assert "C = " in refused("colvo_mesh_clean_plan", p, p, p, 4, 2, C_, p, p, p, p, p, 0)
    for unit in (0.0, -1.0, float("nan"), float("inf")):
        assert "unit" in refused("colvo_mesh_topology_edges", p, p, 4, 2, unit, 1, p, p, p, p, p, p, 0)
        assert "unit" in refused("colvo_mesh_topology_loops", p, 4, 2, unit, 1, 1, p, p, p, p, p, p, 0)
    assert "null pointer" in refused("colvo_mesh_topology_edges", 0, p, 4, 2, 1.0, 1, p, p, p, p, p, p, 0)
    assert "L = " in refused("colvo_mesh_topology_loops", p, 4, 2, 1.0, 1, 0, p, p, p, p, p, p, 0)
    assert "L = " in refused("colvo_mesh_topology_loops", p, 4, 2, 1.0, 1, 5, p, p, p, p, p, p, 0)
    assert "null pointer" in refused("colvo_mesh_topology_loops", p, 4, 2, 1.0, 1, 1, p, p, p, p, 0, p, 0)
    assert "null pointer" in refused("colvo_mesh_clean_plan", p, p, 0, 4, 2, 1, p, p, p, p, p, 0)
    assert "bad shape" in refused("colvo_mesh_clean_write", p, p, p, p, p, 4, 2, p, p, p, 5, 1, p, p, p, p, p, 0)
    assert "bad shape" in refused("colvo_mesh_clean_write", p, p, p, p, p, 4, 2, p, p, p, 0, 0, p, p, p, p, p, 0)
    assert "null pointer" in refused("colvo_mesh_clean_write", p, 0, p, p, p, 4, 2, p, p, p, 1, 1, p, p, p, p, p, 0)   # colors without out_colors


def test_abi_is_26(lib):
    from coivo_amd import _lib
    assert lib.colvo_abi_version() == _lib.ABI_VERSION >= 26


# ---- 4. the policy and the names ----------------------------------------------------------------------------------------------------- #
def test_meshing_keeps_its_positional_form():
    from coivo_amd import inference as I
    # the pair it was: it still unpacks into two and equals them; min_faces rides behind, third positionally or by keyword
    assert I.Meshing() == (None, 2) and I.Meshing(0.4, 3) == (0.4, 3) and len(I.Meshing(0.4, 3, 5)) == 2
    trunc, min_obs = I.Meshing(0.4, 3, 5)
    assert (trunc, min_obs) == (0.4, 3)
    assert I.Meshing().min_faces == 0 and I.Meshing(0.4, 3).min_faces == 0 and I.Meshing(0.4, 3, 5).min_faces == 5
    assert I.Meshing(min_faces=2).min_obs == 2 and I.Meshing(min_faces=2).min_faces == 2
    m = I.Meshing(0.4, 3, 5)
    assert m._replace(min_obs=1).min_faces == 5 and m._replace(min_faces=7) == (0.4, 3) and m._replace(min_faces=7).min_faces == 7
    assert "min_faces=5" in repr(m)
    r = I.Reconstruction(1, 2, 3, 4, mesh=7, topology=8)
    assert len(r) == 5 and r.mesh == 7 and r.topology == 8 and r._replace(points=0).topology == 8 and r._replace(topology=9).mesh == 7
    assert I.Reconstruction(1, 2, 3, 4).topology is None


def test_reconstruct_sequence_checks_min_faces_before_any_work():
    from coivo_amd import inference as I
    frames = torch.zeros(2, 3, 8, 8)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="mesh.min_faces must be an int >= 0"):
            I.reconstruct_sequence(None, None, frames, torch.eye(3), voxel_size=0.1, mesh=I.Meshing(None, 2, bad))
        with pytest.raises(ValueError, match="mesh.min_faces must be an int >= 0"):
            I.reconstruct_sequence(None, None, frames, torch.eye(3), voxel_size=0.1, mesh=(None, 2, bad))          # a plain tuple


@pytest.mark.parametrize("name", ["MeshTopology", "CleanedMesh", "mesh_topology", "clean_mesh"])
def test_name_is_importable_from_inference_and_is_topologys_object(name):
    from coivo_amd import inference
    assert getattr(inference, name) is getattr(importlib.import_module("coivo_amd.topology"), name)
