"""No GPU: the hole-filling replica (tests/fill_ref.py) against first principles -- on hand meshes whose every loop is known and on the
project's own meshes (the replica of extract_mesh) the filled mesh's topology, Euler characteristic and area must change by exactly
what the fill says --; what fill_holes and the colvo_mesh_fill_* entry points refuse; the Meshing policy's fourth field."""
import functools
import importlib

import numpy as np
import pytest
import torch

from tests import fill_ref as R
from tests import topology_ref as T

f64 = np.float64


@functools.lru_cache(maxsize=None)
def _tube(name):
    shape, Tv, min_obs = {"thin": ((5, 17, 23), 1, 2), "tube2": ((5, 24, 32), 4, 2), "tube1": ((5, 24, 32), 4, 1)}[name]
    mesh = T.tube_mesh(*shape, Tv, min_obs)[0]
    return mesh, T.mesh_topology(mesh["vertices"], mesh["faces"], 0.1)


@functools.lru_cache(maxsize=None)
def _sphere():
    mesh = T.sphere_mesh()[0]
    return mesh, T.mesh_topology(mesh["vertices"], mesh["faces"], T.SPHERE["voxel"])


def _directed_sides(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lf = f[T.live_faces(f, V)]
    return np.concatenate([lf[:, [0, 1]], lf[:, [1, 2]], lf[:, [2, 0]]]) if len(lf) else np.zeros((0, 2), np.int64)


def _check(mesh, topo, max_edges):
    """every identity the issue lists, for one mesh and policy -> (result, topology of the result)"""
    r = R.fill_holes(mesh, topo, max_edges)
    V, F, L = len(mesh["vertices"]), len(mesh["faces"]), len(topo["loops"])
    st, hole, loops = r["status"], r["hole"], topo["loops"]
    filled = st == R.FILLED
    # the old rows are the input's bits; shapes and numbering
    assert np.array_equal(r["vertices"][:V].view(np.int32), np.asarray(mesh["vertices"], np.float32).view(np.int32))
    assert np.array_equal(r["faces"][:F], mesh["faces"]) and np.array_equal(r["cells"][:V], mesh["cells"])
    assert (r["cells"][V:] == -1).all() and r["n_open"] == mesh["n_open"] and (r["colors"] is None) == (mesh.get("colors") is None)
    n = loops[:, 2]
    assert np.array_equal(hole[:, 0], np.where(filled, np.where(n == 3, 1, n), 0))
    assert len(r["vertices"]) == V + int((filled & (n > 3)).sum()) == len(r["normals"]) == len(r["cells"])
    assert len(r["faces"]) == F + int(hole[:, 0].sum()) == len(r["face_loop"])
    assert np.array_equal(r["new_vertex_loop"], np.nonzero(filled & (n > 3))[0])
    assert (r["face_loop"][:F] == -1).all() and np.array_equal(r["face_loop"][F:], np.repeat(np.arange(L), hole[:, 0]))
    assert (hole[(st == R.NOT_SIMPLE) | (st == R.UNMEASURED), 1] == 0).all()
    assert ((st == R.TOO_LONG) == ((st != R.NOT_SIMPLE) & (st != R.UNMEASURED) & (n > max_edges))).all()
    # rings: from the smallest vertex along boundary half-edges, closed
    src, dst = R.boundary_half_edges(mesh["faces"], V)
    half = set(zip(src.tolist(), dst.tolist()))
    off = r["ring_offsets"]
    assert np.array_equal(np.diff(off), np.where(st != R.NOT_SIMPLE, n, 0)) and off[0] == 0 and off[-1] == len(r["ring_vertices"])
    for l in np.nonzero(st != R.NOT_SIMPLE)[0]:
        ring = r["ring_vertices"][off[l]:off[l + 1]].tolist()
        assert ring[0] == loops[l, 0] == min(ring) and len(set(ring)) == len(ring)
        assert all((a, b) in half for a, b in zip(ring, ring[1:] + ring[:1]))
        assert (topo["vertex_loop"][ring] == l).all()
    # the centre: within q / 2 plus one float32 ulp of the float64 mean
    ql = T.quanta(topo["unit"])[1]
    for k, l in enumerate(r["new_vertex_loop"]):
        ring = r["ring_vertices"][off[l]:off[l + 1]]
        mean = np.asarray(mesh["vertices"], np.float32)[ring].astype(f64).mean(0)
        c = r["vertices"][V + k].astype(f64)
        assert (np.abs(c - mean) <= ql / 2 + np.spacing(np.abs(c).astype(np.float32)).astype(f64)).all(), (l, c, mean)
        nrm = r["normals"][V + k].astype(f64)
        assert abs(np.linalg.norm(nrm) - 1.0) < 1e-6 or not nrm.any()
    # the topology of the result: exactly the unfilled loops are left, no new non-manifold edge, chi + 1 and area + hole per filled loop
    after = T.mesh_topology(r["vertices"], r["faces"], topo["unit"])
    assert len(after["loops"]) == L - int(filled.sum())
    assert np.array_equal(after["loops"][:, [0, 2, 3]], loops[~filled][:, [0, 2, 3]])
    assert int(after["components"][:, 5].sum()) == int(topo["components"][:, 5].sum())
    assert int(T.euler(after).sum()) == int(T.euler(topo).sum()) + int(filled.sum())
    assert int(after["components"][:, 7].sum()) == int(topo["components"][:, 7].sum()) + int(hole[filled, 1].sum())
    assert after["n_dead_faces"] == topo["n_dead_faces"] and after["n_unmeasured"] == topo["n_unmeasured"]
    # no directed side twice among the live faces that was not so before
    def repeats(faces, nv):
        s = _directed_sides(faces, nv)
        return len(s) - len(np.unique(s[:, 0] * nv + s[:, 1]))
    assert repeats(r["faces"], len(r["vertices"])) == repeats(mesh["faces"], V)
    # a permutation of the faces moves the first F face rows and nothing else
    if F > 1:
        perm = np.random.default_rng(F).permutation(F)
        pm = dict(mesh, faces=np.asarray(mesh["faces"])[perm])
        pt = T.mesh_topology(pm["vertices"], pm["faces"], topo["unit"])
        p = R.fill_holes(pm, pt, max_edges)
        assert np.array_equal(p["faces"][:F], r["faces"][:F][perm])
        for k in r:
            a, b = (r[k][F:], p[k][F:]) if k == "faces" else (r[k], p[k])
            if isinstance(a, np.ndarray):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
            else:
                assert a == b, k
    return r, after


def _hand(name, unit=1.0, colors=True):
    v, f = R.hand_meshes()[name]
    return R.as_mesh(v, f, seed=5 if colors else None), T.mesh_topology(v, f, unit)


# ---- 1. hand meshes ------------------------------------------------------------------------------------------------------------------ #
def test_a_cube_less_one_face_is_closed_by_four_faces():
    mesh, topo = _hand("cube")
    assert topo["loops"][:, [0, 2]].tolist() == [[4, 4]] and T.euler(topo).tolist() == [1]
    r, after = _check(mesh, topo, 8)
    assert r["status"].tolist() == [R.FILLED] and r["hole"].tolist() == [[4, 65536]]           # the unit square, in quanta of 2^-16
    assert T.closed(after).tolist() == [True] and T.euler(after).tolist() == [2]
    assert r["vertices"][8].tolist() == [0.5, 0.5, 1.0] and r["normals"][8].tolist() == [0.0, 0.0, 1.0]       # outward: the top
    assert r["ring_vertices"].tolist() == [4, 6, 7, 5]
    assert r["faces"][10:].tolist() == [[6, 4, 8], [7, 6, 8], [5, 7, 8], [4, 5, 8]]
    ring_colors = mesh["colors"][[4, 5, 7, 6]].astype(f64)
    assert np.abs(r["colors"][8].astype(f64) - ring_colors.mean(0)).max() < 2.0 ** -16


def test_a_tetrahedron_less_one_face_gets_that_face_and_no_vertex():
    mesh, topo = _hand("tetrahedron", colors=False)
    r, after = _check(mesh, topo, 3)
    assert r["status"].tolist() == [R.FILLED] and r["hole"][:, 0].tolist() == [1] and len(r["vertices"]) == 4 and r["colors"] is None
    assert T.closed(after).tolist() == [True] and T.euler(after).tolist() == [2]
    assert sorted(r["faces"][3].tolist()) == [0, 2, 3] and int(r["hole"][0, 1]) == 32768
    full = T.mesh_topology(*T.tetrahedron(), 1.0)
    assert int(after["components"][0, 7]) == int(full["components"][0, 7])


def test_an_annulus_has_two_simple_rings():
    mesh, topo = _hand("annulus")
    r, after = _check(mesh, topo, 8)
    assert r["status"].tolist() == [R.FILLED, R.FILLED] and r["hole"][:, 0].tolist() == [8, 8]
    assert T.closed(after).tolist() == [True] and T.euler(after).tolist() == [2]
    # regular octagons of circumradius 1 and 2: area 2 sqrt 2 r^2.  The inner fan continues the annulus (its faces look along +z); the
    # outer one is wound like the annulus across its border and lies folded back over it: it looks along -z
    assert np.allclose(R.hole_area(r), [2 * np.sqrt(2.0), 8 * np.sqrt(2.0)], rtol=1e-4)
    assert r["normals"][16].tolist() == [0.0, 0.0, 1.0] and r["normals"][17].tolist() == [0.0, 0.0, -1.0]
    r7, after7 = _check(mesh, topo, 7)
    assert r7["status"].tolist() == [R.TOO_LONG] * 2 and np.array_equal(r7["hole"][:, 1], r["hole"][:, 1]) and len(after7["loops"]) == 2


@pytest.mark.parametrize("max_edges,status", [(66, R.FILLED), (65, R.TOO_LONG)])
def test_a_fan_of_64_is_one_ring_of_66(max_edges, status):
    mesh, topo = _hand("fan")
    assert topo["loops"][:, [0, 2]].tolist() == [[0, 66]]
    r, _ = _check(mesh, topo, max_edges)
    assert r["status"].tolist() == [status] and int(r["hole"][0, 1]) > 0


@pytest.mark.parametrize("name", ["book", "corner", "clash"])
def test_what_is_not_simple_is_skipped_whole(name):
    mesh, topo = _hand(name)
    assert len(topo["loops"]) == 1
    r, after = _check(mesh, topo, 1000)
    assert r["status"].tolist() == [R.NOT_SIMPLE] and r["hole"].tolist() == [[0, 0]] and len(r["ring_vertices"]) == 0
    assert np.array_equal(r["faces"], mesh["faces"]) and len(after["loops"]) == 1


def test_a_ring_with_a_coordinate_of_1e30_is_unmeasured():
    mesh, topo = _hand("far")
    r, _ = _check(mesh, topo, 8)
    assert r["status"].tolist() == [R.UNMEASURED] and r["hole"].tolist() == [[0, 0]] and r["ring_vertices"].tolist() == [0, 1, 2, 3]


def test_all_hand_meshes_in_one():
    names = sorted(R.hand_meshes())
    v, f = T.renumber(*T.concatenate([R.hand_meshes()[k] for k in names]), 13)
    mesh, topo = R.as_mesh(v, f, seed=2), T.mesh_topology(v, f, 0.5)
    for max_edges in (8, 66):
        r, _ = _check(mesh, topo, max_edges)
        assert sorted(r["status"].tolist()) == sorted([0, 0, 0, 0, 2, 2, 2, 3] + [0 if max_edges == 66 else 1])


def test_empty_meshes():
    empty = R.as_mesh(np.zeros((0, 3)), np.zeros((0, 3)))
    r = R.fill_holes(empty, T.mesh_topology(empty["vertices"], empty["faces"], 1.0), 8)
    assert len(r["vertices"]) == 0 and len(r["status"]) == 0 and r["ring_offsets"].tolist() == [0]
    mesh = R.as_mesh(*T.tetrahedron())
    r, _ = _check(mesh, T.mesh_topology(mesh["vertices"], mesh["faces"], 1.0), 8)
    assert len(r["status"]) == 0 and np.array_equal(r["faces"], mesh["faces"])


# ---- 2. the project's own meshes ----------------------------------------------------------------------------------------------------- #
# (tube, max_edges) -> filled / too long / not simple, loops before -> after, hole area of all simple loops / mesh area
TUBES = [("thin", 8, (32, 1, 0), (33, 1), 1.137), ("tube2", 12, (19, 0, 4), (23, 4), 0.0251), ("tube2", 6, (16, 3, 4), (23, 7), 0.0251),
         ("tube1", 8, (10, 1, 2), (13, 3), 0.0147)]


@pytest.mark.parametrize("name,max_edges,counts,loops,share", TUBES)
def test_tube_meshes(name, max_edges, counts, loops, share):
    mesh, topo = _tube(name)
    r, after = _check(mesh, topo, max_edges)
    st = r["status"]
    assert (int((st == R.FILLED).sum()), int((st == R.TOO_LONG).sum()), int((st == R.NOT_SIMPLE).sum())) == counts
    assert int((st == R.UNMEASURED).sum()) == 0 and (len(topo["loops"]), len(after["loops"])) == loops
    got = float(r["hole"][:, 1].sum()) / float(topo["components"][:, 7].sum())
    assert abs(got - share) <= 0.5 * 10.0 ** -(len(str(share).split(".")[1])), got        # the table's digits, rounded
    simple = topo["loops"][st != R.NOT_SIMPLE, 2]
    assert 4 <= simple.min() and simple.max() <= 22
    ends = topo["loops"][:, 2] >= 128                                                       # the tube's open ends: none is simple
    assert (st[ends] == R.NOT_SIMPLE).all() and int(ends.sum()) == min(counts[2], 2) and topo["loops"][:, 2].max() <= 242


def test_the_sphere():
    mesh, topo = _sphere()
    assert len(topo["loops"]) == 0
    r, after = _check(mesh, topo, 8)
    assert len(r["faces"]) == len(mesh["faces"]) and len(after["loops"]) == 0


# ---- 3. the surface ------------------------------------------------------------------------------------------------------------------ #
@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.ensure()
    return _lib.load()


def test_python_entry_point_refuses_bad_arguments():
    from coivo_amd import inference as I
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    mesh = I.Mesh(v, f, None, v, torch.zeros(3, 3, dtype=torch.int32), 0)
    topo = I.MeshTopology(torch.zeros(3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(3, dtype=torch.int32),
                          torch.zeros(1, 8, dtype=torch.int64), torch.zeros(1, 4, dtype=torch.int64), 0, 0, 1.0)
    with pytest.raises(ValueError, match="fill_holes: mesh must be a Mesh"):
        I.fill_holes(v, topo, max_edges=8)
    with pytest.raises(ValueError, match="fill_holes: topology must be a MeshTopology"):
        I.fill_holes(mesh, None, max_edges=8)
    for bad in (2, 0, -1, 8.0, True, None, 2 ** 31):
        with pytest.raises(ValueError, match="fill_holes: max_edges must be an int in 3.."):
            I.fill_holes(mesh, topo, max_edges=bad)
    with pytest.raises(TypeError):
        I.fill_holes(mesh, topo)                                             # max_edges is a choice the caller makes
    with pytest.raises(ValueError, match="expected a float32 CUDA tensor"):
        I.fill_holes(mesh, topo, max_edges=8)                                # no CPU path


def test_hole_fill_properties_are_plain_arithmetic():
    from coivo_amd import inference as I
    z = torch.zeros(0, dtype=torch.int32)
    h = I.HoleFill(None, torch.tensor([0, 1, 2, 3], dtype=torch.int32), torch.tensor([[4, 65536], [0, 32768], [0, 0], [0, 0]]), z, z, z, z, 0.5)
    assert h.hole_area.dtype == torch.float64 and h.hole_area.tolist() == [0.25, 0.125, 0.0, 0.0]
    assert h.filled.tolist() == [True, False, False, False] and h.simple.tolist() == [True, True, False, True] and len(h) == 8


def test_entry_points_refuse_before_any_hip_call(lib):
    import ctypes as C
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    q = lib.colvo_mesh_fill_scratch_bytes
    assert q(0, 1, 1) == 0 and q(4, 0, 1) == 0 and q(4, 2, 0) == 0 and q(4, 2, 5) == 0 and q(2 ** 30, 2, 1) == 0 and q(4, 2 ** 29, 1) == 0
    assert q(4, 2, 1) > 0 and q(2 ** 30 - 1, 2 ** 29 - 1, 2 ** 30 - 1) > q(2 ** 30 - 1, 2 ** 29 - 1, 1) > 0

    def refused(name, *args):
        assert getattr(lib, name)(*args) != 0, name
        msg = lib.colvo_last_error().decode()
        assert msg.startswith(name + ":"), msg
        return msg

    def plan(V=4, F=2, L=1, unit=1.0, max_edges=8, vertices=p, scratch=p):
        return refused("colvo_mesh_fill_plan", vertices, p, p, V, F, L, unit, max_edges, p, p, scratch, p, p, p, p, p, 0)

    def write(V=4, F=2, L=1, R=4, nv=1, nf=4, colors=p, out_colors=p, scratch=p):
        return refused("colvo_mesh_fill_write", p, colors, p, p, p, V, F, L, R, nv, nf, scratch, p, p, p, p, p, out_colors, p, p, p, p, p, 0)

    for V, F, L in ((0, 2, 1), (2 ** 30, 2, 1), (4, 0, 1), (4, 2 ** 29, 1), (4, 2, 0), (4, 2, 5)):
        assert "bad shape" in plan(V, F, L) and "bad shape" in write(V, F, L)
    for unit in (0.0, -1.0, float("nan"), float("inf")):
        assert "unit" in plan(unit=unit)
    assert "max_edges" in plan(max_edges=2) and "max_edges" in plan(max_edges=-1)
    assert "null pointer" in plan(vertices=0) and "16-byte aligned" in plan(scratch=p + 4)
    assert "bad shape" in write(R=5) and "bad shape" in write(nv=2) and "bad shape" in write(nf=5)
    assert "null pointer" in write(out_colors=0) and "16-byte aligned" in write(scratch=p + 4)


def test_abi_is_29(lib):
    from coivo_amd import _lib
    assert lib.colvo_abi_version() == _lib.ABI_VERSION >= 29


def test_meshing_has_a_fourth_value():
    from coivo_amd import inference as I
    assert I.Meshing() == (None, 2) and len(I.Meshing(0.4, 3, 5, 12)) == 2 and I.Meshing(0.4, 3, 5, 12) == (0.4, 3)
    trunc, min_obs = I.Meshing(0.4, 3, 5, 12)
    assert (trunc, min_obs) == (0.4, 3)
    assert I.Meshing().fill_edges == 0 and I.Meshing(0.4, 3, 5).fill_edges == 0 and I.Meshing(0.4, 3, 5, 12).fill_edges == 12
    assert I.Meshing(fill_edges=6).min_obs == 2 and I.Meshing(fill_edges=6).min_faces == 0 and I.Meshing(fill_edges=6).fill_edges == 6
    m = I.Meshing(0.4, 3, 5, 12)
    assert m._replace(min_obs=1).fill_edges == 12 and m._replace(min_faces=7).fill_edges == 12 and m._replace(fill_edges=4).min_faces == 5
    assert m._replace(fill_edges=4) == (0.4, 3) and m._replace(fill_edges=4).fill_edges == 4
    assert "min_faces=5" in repr(m) and "fill_edges=12" in repr(m)
    r = I.Reconstruction(1, 2, 3, 4, mesh=7, topology=8, holes=9)
    assert len(r) == 5 and r.holes == 9 and r._replace(points=0).holes == 9 and r._replace(holes=1).topology == 8
    assert I.Reconstruction(1, 2, 3, 4).holes is None and I.Reconstruction(1, 2, 3, 4, None, 5, 6, 7, 8, 9, 10, 11, 12).holes == 12


def test_reconstruct_sequence_checks_fill_edges_before_any_work():
    from coivo_amd import inference as I
    frames = torch.zeros(2, 3, 8, 8)
    for bad in (1, 2, -1, 8.0, True, None):
        with pytest.raises(ValueError, match="mesh.fill_edges .* must be an int >= 3"):
            I.reconstruct_sequence(None, None, frames, torch.eye(3), voxel_size=0.1, mesh=I.Meshing(None, 2, 0, bad))
        with pytest.raises(ValueError, match="mesh.fill_edges .* must be an int >= 3"):
            I.reconstruct_sequence(None, None, frames, torch.eye(3), voxel_size=0.1, mesh=(None, 2, 0, bad))          # a plain tuple


def test_surface_reconstruction_metrics_checks_fill_edges_before_any_work():
    from coivo_amd import evaluate as E, inference as I
    mesh = I.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), None, torch.zeros(3, 3), torch.zeros(3, 3, dtype=torch.int32), 0)
    for bad in (1, 2, -1, 8.0, True, None):
        with pytest.raises(ValueError, match="surface_reconstruction_metrics: meshing.fill_edges .* must be an int >= 3"):
            E.surface_reconstruction_metrics(mesh, None, None, None, None, voxel_size=0.1, meshing=I.Meshing(fill_edges=bad))


@pytest.mark.parametrize("name", ["HoleFill", "fill_holes"])
def test_name_is_importable_from_inference_and_is_holes_object(name):
    from coivo_amd import inference
    assert getattr(inference, name) is getattr(importlib.import_module("coivo_amd.holes"), name)
