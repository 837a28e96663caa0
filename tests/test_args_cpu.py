"""coivo_amd/_args.py, the argument checks of the post-training entry points: what each helper lets through and gives back, and that
every refusal is a ValueError whose message names the entry point (`who`) and the argument."""
import math
import struct

import pytest
import torch

from coivo_amd import _args as A

WHO = "some_entry_point"


def _refused(call, name, exc=ValueError):
    with pytest.raises(exc) as e:
        call()
    assert WHO in str(e.value) and name in str(e.value), str(e.value)


# ---- numbers ----------------------------------------------------------------------------------------------------------- #
def test_f32_rounds_to_float32():
    assert A.f32(0.1) == struct.unpack("f", struct.pack("f", 0.1))[0] != 0.1
    assert A.f32(1) == 1.0 and isinstance(A.f32(1), float) and A.f32(A.f32(0.1)) == A.f32(0.1)


@pytest.mark.parametrize("val", [math.nan, math.inf, -math.inf, 1e39, 0, 0.0, -1, -1e-3, 1e-50, "x", None, [1.0]])
def test_finite_pos32_refuses(val):
    _refused(lambda: A.finite_pos32(WHO, "max_depth", val), "max_depth")


@pytest.mark.parametrize("val", [math.nan, math.inf, 1e39, -1, -1e-3, "x", None])
def test_finite_nonneg32_refuses(val):
    _refused(lambda: A.finite_nonneg32(WHO, "radius", val), "radius")


def test_finite32_accepts_and_returns_the_float32_value():
    assert A.finite_pos32(WHO, "v", 0.1) == A.f32(0.1) and A.finite_pos32(WHO, "v", 3) == 3.0 and A.finite_pos32(WHO, "v", 1e38) > 0
    assert A.finite_nonneg32(WHO, "v", 0) == 0.0 and A.finite_nonneg32(WHO, "v", 1e-50) == 0.0     # (rounds to zero: not negative)
    assert A.finite_nonneg32(WHO, "v", 0.02) == A.f32(0.02)


@pytest.mark.parametrize("val,lo,hi", [(True, 0, None), (False, 0, None), (1.0, 1, None), ("1", 1, None), (None, 1, None), (0, 1, None),
                                       (-1, 0, 32), (33, 0, 32), (16385, 1, 16384), (torch.tensor(2), 1, None)])
def test_int_range_refuses(val, lo, hi):
    _refused(lambda: A.int_range(WHO, "stride", val, lo, hi), "stride")


def test_int_range_accepts_and_names_the_range():
    assert A.int_range(WHO, "n", 1, 1) == 1 and A.int_range(WHO, "n", 0, 0, 32) == 0 and A.int_range(WHO, "n", 32, 0, 32) == 32
    assert A.int_range(WHO, "n", 1 << 40, 1) == 1 << 40
    with pytest.raises(ValueError, match=r"1\.\.16384"):
        A.int_range(WHO, "H", 8.0, 1, 16384)
    with pytest.raises(ValueError, match=">= 1"):
        A.int_range(WHO, "stride", 0, 1)


# ---- tensors (no GPU here: what is refused before one is needed) --------------------------------------------------------- #
@pytest.mark.parametrize("t", [torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.float64), torch.zeros(3, 2), None, [[0.0] * 3] * 2],
                         ids=["cpu", "dtype", "shape", "none", "list"])
def test_device_f32_refuses(t):
    _refused(lambda: A.device_f32(WHO, "points", t, (2, 3)), "points")


def test_device_f32_says_what_it_wants_and_what_it_got():
    with pytest.raises(ValueError, match=r"float32 CUDA tensor of shape \(2, 3\), got torch.float64 \(3, 2\) on cpu"):
        A.device_f32(WHO, "points", torch.zeros(3, 2, dtype=torch.float64), (2, 3))


def test_depth_views_checks_the_trio_in_order():
    d, K, M = torch.ones(2, 1, 4, 5), torch.eye(3).expand(2, 3, 3), torch.eye(4).expand(2, 4, 4)
    assert A.frames_shape(WHO, "depths", d) == (2, 4, 5)
    for bad in (d[0], None, torch.ones(2, 4, 5)):
        _refused(lambda: A.frames_shape(WHO, "depths", bad), "depths")
        _refused(lambda: A.depth_views(WHO, bad, K, M), "depths")
    _refused(lambda: A.depth_views(WHO, d[0], K, M, name="depth"), "depth")
    _refused(lambda: A.depth_views(WHO, d, K, M), "depths")                                      # on the CPU: the first of the three
    import unittest.mock as mock
    real = A.device_f32

    def shapes_only(who, name, t, shape):                                                         # device_f32 without the device
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
            return real(who, name, t, shape)
        return t.contiguous()

    with mock.patch.object(A, "device_f32", shapes_only):
        out = A.depth_views(WHO, d, K, M)
        assert out[3:] == (2, 4, 5) and all(t.is_contiguous() for t in out[:3]) and torch.equal(out[1], K)
        assert A.depth_views(WHO, d, K)[2] is None                                                # cam2world may be left out
        _refused(lambda: A.depth_views(WHO, d, K[:1], M), "K")
        _refused(lambda: A.depth_views(WHO, d, torch.eye(3), M), "K")
        _refused(lambda: A.depth_views(WHO, d, K, M[:, :3]), "cam2world")
        _refused(lambda: A.depth_views(WHO, d, K, M.double()), "cam2world")


def test_per_view_K_expands_a_single_matrix_only():
    K = torch.arange(9.0).reshape(3, 3)
    out = A.per_view_K(K, 4)
    assert tuple(out.shape) == (4, 3, 3) and all(torch.equal(out[n], K) for n in range(4))
    many = K.expand(2, 3, 3)
    assert A.per_view_K(many, 4) is many and A.per_view_K(None, 4) is None


# ---- the voxel grid ---------------------------------------------------------------------------------------------------- #
def test_voxel_grid_normalises():
    origin, dims, vs = A.voxel_grid(WHO, [0.1, -0.2, 3], [8, 16.0, 24], 0.02)
    assert origin == (A.f32(0.1), A.f32(-0.2), 3.0) and dims == (8, 16, 24) and all(isinstance(d, int) for d in dims)
    assert vs == A.f32(0.02)
    assert A.voxel_grid(WHO, None, None, 0.02) == (None, None, A.f32(0.02))                       # the grid is the caller's to choose


@pytest.mark.parametrize("origin,dims,vs,name", [
    ((0.0, 0.0, 0.0), (8, 8, 7), 0.02, "dims"), ((0.0, 0.0, 0.0), (8, 8, 0), 0.02, "dims"), ((0.0, 0.0, 0.0), (8, 8, -8), 0.02, "dims"),
    ((0.0, 0.0, 0.0), (8, 8), 0.02, "dims"), ((0.0, 0.0), (8, 8, 8), 0.02, "origin"), ((0.0, 0.0, 0.0), None, 0.02, "dims"),
    (None, (8, 8, 8), 0.02, "origin"), ((0.0, 0.0, 0.0), (8, 8, 8), 0.0, "voxel_size"), ((0.0, 0.0, 0.0), (8, 8, 8), math.nan, "voxel_size"),
    (None, None, 1e39, "voxel_size"), (None, None, "x", "voxel_size")])
def test_voxel_grid_refuses(origin, dims, vs, name):
    _refused(lambda: A.voxel_grid(WHO, origin, dims, vs), name)


# ---- clouds, reach, Sim(3) --------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("t", [torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 2), None],
                         ids=["cpu", "dtype", "last_dim", "none"])
def test_cloud_refuses(t):
    _refused(lambda: A.cloud(WHO, "query", t), "query")


def test_reach_returns_float32_values():
    assert A.reach(WHO, 0.08, (0.02, 0.08)) == (A.f32(0.08), (A.f32(0.02), A.f32(0.08))) and A.reach(WHO, 1, ()) == (1.0, ())
    _refused(lambda: A.reach(WHO, -1.0, ()), "max_dist")
    _refused(lambda: A.reach(WHO, 0.1, (0.2,)), "thresholds")
    _refused(lambda: A.reach(WHO, 0.1, [0.01] * (A.MAX_THRESHOLDS + 1)), "thresholds")


def test_sim3_gives_host_float64_and_refuses_the_rest():
    R, t, s = A.sim3(WHO, "init", (torch.eye(3), [1, 2, 3], torch.tensor([2.0])))
    assert R.dtype == t.dtype == torch.float64 and tuple(R.shape) == (3, 3) and t.tolist() == [1.0, 2.0, 3.0] and s == 2.0
    assert isinstance(s, float)
    bad_R = torch.eye(3).clone()
    bad_R[1, 1] = math.nan
    for bad in ((torch.eye(4), torch.zeros(3), 1.0), (torch.eye(3), torch.zeros(4), 1.0), (torch.eye(3), torch.zeros(3), [1.0, 2.0]),
                (bad_R, torch.zeros(3), 1.0), (torch.eye(3), torch.zeros(3), math.inf), (torch.eye(3), torch.zeros(3)), 5, None,
                (torch.eye(3), "x", 1.0)):
        _refused(lambda: A.sim3(WHO, "init", bad), "init")


def test_finite_nonneg64_does_not_round():
    assert A.finite_nonneg64(WHO, "damping", 1e-50) == 1e-50 and A.finite_nonneg64(WHO, "damping", 0) == 0.0
    for bad in (-1e-300, math.nan, math.inf, "x", None):
        _refused(lambda: A.finite_nonneg64(WHO, "damping", bad), "damping")


# ---- meshes ------------------------------------------------------------------------------------------------------------ #
def test_mesh_arrays_refuses():
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    _refused(lambda: A.mesh_arrays(WHO, v, f), "vertices")                                        # on the CPU
    _refused(lambda: A.mesh_arrays(WHO, v.double(), f), "vertices")
    _refused(lambda: A.mesh_arrays(WHO, torch.zeros(4, 2), f), "vertices")
    _refused(lambda: A.mesh_arrays(WHO, v, f.long()), "faces")
    _refused(lambda: A.mesh_arrays(WHO, v, torch.zeros(2, 4, dtype=torch.int32)), "faces")
    mesh = A.Mesh(v, f, None, v, torch.zeros(4, 3, dtype=torch.int32), 0)
    _refused(lambda: A.mesh_arrays(WHO, mesh, f), "faces")                                        # with a Mesh give no faces
    _refused(lambda: A.mesh_arrays(WHO, mesh, None), "vertices")


def test_mesh_attributes_refuses_cells_of_the_wrong_dtype_or_shape():
    import unittest.mock as mock
    v = torch.zeros(4, 3)
    with mock.patch.object(A, "device_f32", lambda who, name, t, shape: t):                       # (no device here)
        for cells in (torch.zeros(4, 3, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), None):
            _refused(lambda: A.mesh_attributes(WHO, A.Mesh(v, None, None, v, cells, 0), 4, v.device), "mesh.cells")
        colors, normals, cells = A.mesh_attributes(WHO, A.Mesh(v, None, None, v, torch.zeros(4, 3, dtype=torch.int32), 0), 4, v.device)
        assert colors is None and normals is v and cells.is_contiguous()


def test_own_topology_checks_the_tables_the_caller_reads():
    from types import SimpleNamespace
    dev = torch.device("cpu")
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    topo = SimpleNamespace(vertex_component=i32(4), face_component=i32(2), vertex_loop=i32(4),
                           components=torch.zeros(1, 8, dtype=torch.int64), loops=torch.zeros(1, 4, dtype=torch.int64))
    A.own_topology(WHO, topo, 4, 2, dev, ("components",))
    A.own_topology(WHO, topo, 4, 2, dev, ("loops",))
    for V, F in ((5, 2), (4, 3)):
        for tables in (("components",), ("loops",)):
            _refused(lambda: A.own_topology(WHO, topo, V, F, dev, tables), "topology")
    topo.loops = topo.loops.to(torch.int32)                                                       # clean_mesh does not read the loops
    A.own_topology(WHO, topo, 4, 2, dev, ("components",))
    _refused(lambda: A.own_topology(WHO, topo, 4, 2, dev, ("loops",)), "topology")
    topo.vertex_component = i32(3)                                                                # fill_holes does not read the components
    _refused(lambda: A.own_topology(WHO, topo, 4, 2, dev, ("components",)), "topology")
