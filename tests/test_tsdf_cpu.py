"""No GPU: the NumPy replica of the TSDF fusion and the surface-net meshing (tests/tsdf_ref.py) on scenes whose answer is known, the
host-only entry points of csrc/tsdf.hip (every refusal with its message, the size queries) and write_ply's faces."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from coivo_amd.inference import Mesh, Meshing, TsdfVolume, extract_mesh, fuse_tsdf, write_ply  # noqa: F401  (what this file is about)
from tests import consistency_ref as CR
from tests import tsdf_ref as R

f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.build()
    return _lib.load()


def _edges(faces, V):
    """directed edges of a triangle list as keys a * V + b"""
    F = faces.astype(np.int64)
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    return e[:, 0] * V + e[:, 1], e[:, 1] * V + e[:, 0]


def _same_mesh(a, b):
    for k in ("vertices", "cells", "normals", "faces", "colors"):
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    assert a["n_open"] == b["n_open"]


# ---- 1. the hand scene --------------------------------------------------------------------------------------------------------- #
def test_replica_gives_the_hand_computed_answer():
    """One camera at the origin looks along +z at the plane z = 2.125: 64 x 64 pixels, fx = fy = 8, principal point 31.5.  One brick of
    0.5 voxels from (-2, -2, 0): the voxel layers lie at z = 0.25, 0.75, ..., 3.75, T = 1 so trunc = 0.5.  The distance of a voxel is
    2.125 - z whatever its pixel: layers 0..2 are free space (+4096), layer 3 (z = 1.75) has 0.375 / 0.5 * 4096 = 3072, layer 4
    (z = 2.25) has -0.125 / 0.5 * 4096 = -1024 and layers 5..7 are hidden (below -trunc).  Every quantity is exact in float32.  The
    surface crosses the edges between layers 3 and 4 at 3072 / (3072 + 1024) = 0.75 of a voxel: z = 1.75 + 0.375 = 2.125."""
    depths = np.full((1, 1, 64, 64), 2.125, f32)
    K = np.array([[[8.0, 0, 31.5], [0, 8.0, 31.5], [0, 0, 1]]], f32)
    M = np.eye(4, dtype=f32)[None]
    colors = np.broadcast_to(np.array([51, 102, 255], f32)[None, :, None, None] / f32(255), (1, 3, 64, 64))
    vol = R.fuse_tsdf(depths, K, M, voxel_size=0.5, trunc=0.5, colors=colors, origin=(-2.0, -2.0, 0.0), dims=(8, 8, 8), max_depth=10.0)
    assert vol["T"] == 1 and vol["trunc"] == f32(0.5) and vol["n_bricks"] == 1 and vol["brick_list"].tolist() == [0]
    # X = (u - 31.5) / 8 * 2.125 lies in [-2, 2) for u = 24 .. 39: 16 x 16 samples inside
    assert vol["n_input"] == 64 * 64 and vol["n_outside"] == 64 * 64 - 16 * 16
    pool = vol["pool"].reshape(8, 8, 8, 2)                          # [z][y][x]
    # layers 3 and 4 project into the image everywhere (|x| / z <= 1.75 / 1.75 -> 8 pixels from the centre)
    assert (pool[3, :, :, 0] == 3072).all() and (pool[3, :, :, 1] == 1).all()
    assert (pool[4, :, :, 0] == -1024).all() and (pool[4, :, :, 1] == 1).all()
    assert (pool[5:, :, :, 1] == 0).all() and (pool[5:, :, :, 0] == 0).all()
    seen = pool[:3, :, :, 1] == 1
    assert (pool[:3, :, :, 0][seen] == 4096).all() and (pool[:3, :, :, 0][~seen] == 0).all() and seen[2, 3:5, 3:5].all()
    assert (vol["color_sums"].reshape(8, 8, 8, 4)[3] == np.array([51, 102, 255, 0])).all()
    mesh = R.extract_mesh(vol, min_obs=1)
    # cells (i, j, 3), i, j = 0 .. 6, have their eight corners; those with i = 7 or j = 7 reach outside the grid: open
    assert mesh["vertices"].shape == (49, 3) and mesh["n_open"] == 15
    assert (mesh["cells"][:, 2] == 3).all() and mesh["cells"][:, :2].tolist() == [[i, j] for j in range(7) for i in range(7)]
    assert (mesh["vertices"][:, 2] == f32(2.125)).all()
    assert np.array_equal(mesh["vertices"][:, :2], (-2.0 + (mesh["cells"][:, :2] + 1.0) * 0.5).astype(f32))
    assert np.array_equal(mesh["normals"], np.broadcast_to(np.array([0, 0, -1], f32), (49, 3)))      # towards free space: the camera
    assert np.array_equal(mesh["colors"], np.broadcast_to(np.array([51, 102, 255], np.float64) / 255.0, (49, 3)).astype(f32))
    # one quad per z-edge (i, j, 3) -> (i, j, 4) with i, j = 1 .. 6
    assert mesh["faces"].shape == (72, 3) and mesh["faces"].dtype == np.int32
    v = mesh["vertices"].astype(np.float64)[mesh["faces"]]
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    assert (nrm[:, 2] < 0).all() and (nrm[:, :2] == 0).all()        # wound towards the camera
    assert np.isclose(0.5 * np.linalg.norm(nrm, axis=1).sum(), 36 * 0.25)
    # min_obs above every count: nothing is observed
    empty = R.extract_mesh(vol, min_obs=2)
    assert empty["vertices"].shape == (0, 3) and empty["faces"].shape == (0, 3) and empty["n_open"] == 0


# ---- 2. a sphere seen from its centre ------------------------------------------------------------------------------------------ #
SPHERE = dict(radius_voxels=12.0, voxel=0.05, S=64, n=48)


def test_replica_sphere_is_closed_oriented_and_near_the_sphere():
    """Six 90-degree cameras at the centre of a sphere of 12 voxels radius.  The grid's origin differs per axis so that no voxel centre
    lies on a seam |x| = |y| between two cameras (there the half-open pixel ranges decide, not the geometry)."""
    vs, n, S = SPHERE["voxel"], SPHERE["n"], SPHERE["S"]
    rad = SPHERE["radius_voxels"] * vs
    depths, K, M = R.sphere_scene(rad, S)
    origin = (-n / 2 * vs + 0.013, -n / 2 * vs + 0.021, -n / 2 * vs + 0.006)
    vol = R.fuse_tsdf(depths, K, M, voxel_size=vs, origin=origin, dims=(n, n, n))
    assert vol["T"] == 4 and vol["n_outside"] == 0
    mesh = R.extract_mesh(vol)
    V, F = len(mesh["vertices"]), len(mesh["faces"])
    assert V > 2000 and mesh["n_open"] == 0
    # closed and consistently oriented: every directed edge once, its reverse once
    key, rkey = _edges(mesh["faces"], V)
    assert len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rkey))
    assert V - len(key) // 2 + F == 2
    # a vertex is a mean of points on its cell's edges: inside the closed box of the cell, exactly (float64 of the float32 outputs:
    # the conversion to float32 is monotone and the box's corners are evaluated by the same expression)
    o64 = np.array([np.float64(f32(o)) for o in origin])
    lo = (o64 + (mesh["cells"].astype(np.float64) + 0.5) * np.float64(f32(vs))).astype(f32)
    hi = (o64 + (mesh["cells"].astype(np.float64) + 1.5) * np.float64(f32(vs))).astype(f32)
    assert (mesh["vertices"] >= lo).all() and (mesh["vertices"] <= hi).all()
    r = np.linalg.norm(mesh["vertices"].astype(np.float64), axis=1)
    err = np.abs(r - rad).max() / vs
    print(f"sphere: V = {V}, F = {F}, largest | |v| - R | = {err:.4f} voxels")
    # The bound that needs no measurement.  A voxel p is classified by the sign of d(pixel) - Pz = cos(t_p) (R - |p|) + R (cos(t_pix) -
    # cos(t_p)), t the angle to the optical axis.  cos(t) = (1 + x^2 + y^2)^-1/2 has a gradient of at most 0.385 in the image-plane
    # coordinates (x, y), which differ by at most sqrt(2) * 0.5 / fx between a voxel's ray and its nearest pixel's, and cos(t_p) >=
    # 1 / sqrt(3) inside a 90-degree field: the sign is that of R - |p| unless | |p| - R | <= eps = R * 0.385 * sqrt(2) * 0.5 / fx *
    # sqrt(3).  An active cell has a corner classified outside (|p| <= R + eps) and one classified inside (|p| >= R - eps), and the
    # vertex lies in the cell's box, within its diagonal sqrt(3) voxels of both: | |v| - R | <= sqrt(3) voxels + eps.
    eps = rad * 0.385 * np.sqrt(2.0) * 0.5 / (S / 2.0) * np.sqrt(3.0)
    assert err * vs <= np.sqrt(3.0) * vs + eps
    # measured on the replica at this size: 0.1190 voxels.  Asserted with a quarter on top -- the replica is deterministic, the margin
    # only allows for another libm's last bit in the scene's depths.
    assert err <= 0.15
    # normals point to free space: towards the centre
    assert ((mesh["normals"].astype(np.float64) * mesh["vertices"]).sum(1) < 0).all()


# ---- 3. carving ---------------------------------------------------------------------------------------------------------------- #
def test_free_space_votes_remove_a_floater():
    """Five cameras, shifted sideways, see a wall at z = 2; frame 0 also has an 8 x 8 patch at z = 1 in front of it.  Alone, frame 0
    gives the patch a surface.  The other four look through it: +4096 each against at most -4096."""
    N, S, vs = 5, 32, 0.125
    depths = np.full((N, 1, S, S), 2.0, f32)
    depths[0, 0, 12:20, 12:20] = 1.0
    K = np.broadcast_to(np.array([[32.0, 0, 15.5], [0, 32.0, 15.5], [0, 0, 1]], f32), (N, 3, 3)).copy()
    M = np.broadcast_to(np.eye(4, dtype=f32), (N, 4, 4)).copy()
    M[:, 0, 3] = 0.03 * np.arange(N)
    kw = dict(voxel_size=vs, trunc=2 * vs, origin=(-1.5, -1.5, 0.0), dims=(24, 24, 24), max_depth=10.0)
    alone = R.extract_mesh(R.fuse_tsdf(depths[:1], K[:1], M[:1], **kw), min_obs=1)
    assert (alone["vertices"][:, 2] < 1.5).sum() >= 4 and (alone["vertices"][:, 2] > 1.5).sum() > 0
    together = R.extract_mesh(R.fuse_tsdf(depths, K, M, **kw), min_obs=1)
    assert (together["vertices"][:, 2] < 1.5).sum() == 0 and (together["vertices"][:, 2] > 1.5).sum() > 0


# ---- 4. frame order ------------------------------------------------------------------------------------------------------------ #
def test_replica_does_not_depend_on_the_frame_order():
    depths, K, M = CR.tube_scene(5, 24, 32, 3)
    colors = np.random.default_rng(1).random((5, 3, 24, 32)).astype(f32)
    kw = dict(voxel_size=0.1, stride=2, max_depth=4.5, origin=(-1.6, -1.6, -0.8), dims=(32, 32, 64))
    a = R.fuse_tsdf(depths, K, M, colors=colors, **kw)
    assert a["n_bricks"] > 8
    perm = np.array([3, 0, 4, 2, 1])
    b = R.fuse_tsdf(depths[perm], K[perm], M[perm], colors=colors[perm], **kw)
    for k in ("pool", "color_sums", "brick_list", "table"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["n_input"], a["n_outside"]) == (b["n_input"], b["n_outside"])
    ma, mb = R.extract_mesh(a, min_obs=2), R.extract_mesh(b, min_obs=2)
    assert len(ma["vertices"]) > 100 and len(ma["faces"]) > 100
    _same_mesh(ma, mb)


# ---- 5. the host-only entries --------------------------------------------------------------------------------------------------- #
def test_size_queries(lib):
    q = lib.colvo_tsdf_plan_scratch_bytes
    assert q(1, 1, 1, 1, 8, 8, 8) == 16384 + 16                     # 256 counter lines of 64 bytes, one chunk sum
    assert q(8, 256, 320, 1, 1024, 1024, 1024) == 16384 + 4 * 512   # 2^21 bricks: 512 scan chunks
    for bad in ((0, 8, 8, 1, 8, 8, 8), (65536, 8, 8, 1, 8, 8, 8), (2, 0, 8, 1, 8, 8, 8), (2, 8, 8, 0, 8, 8, 8),
                (2, 32768, 32768, 1, 8, 8, 8), (65535, 256, 320, 1, 8, 8, 8), (2, 8, 8, 1, 12, 8, 8), (2, 8, 8, 1, 8, 8, 0),
                (2, 8, 8, 1, 8192, 8192, 8192)):
        assert q(*bad) == 0, bad
    m = lib.colvo_tsdf_mesh_scratch_bytes
    assert m(1) == 64 and m(4096) == 2 * (16384 + 16) and m(4097) == 2 * (16400 + 16)
    for bad in (0, -3, 1 << 22):
        assert m(bad) == 0, bad
    assert m((1 << 22) - 1) > 0
    from coivo_amd import _lib
    assert _lib.tune_get("tsdf_cull") == 1 and _lib.ABI_VERSION >= 23


def test_entry_points_refuse_bad_arguments_before_any_hip_call(lib):
    """Every refusal carries the entry's name and its reason.  The pointers are host memory or NULL: nothing may be launched."""
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 15) & ~15                               # 16-byte aligned, never dereferenced

    def refused(rc, entry, what):
        msg = lib.colvo_last_error().decode()
        assert rc != 0 and msg.startswith(entry + ":") and what in msg, (entry, what, msg)

    grid = (10.0, 0.0, 0.0, 0.0, 0.1, 8, 8, 8)                      # max_depth, origin, voxel_size, dims
    ok_shape = (2, 8, 8, 1)

    def plan(shape=ok_shape, grid=grid, T=4, ptrs=(p, p, p), out=(p, p, p, p)):
        return lib.colvo_tsdf_plan(*ptrs, *shape, *grid, T, *out, 0)

    e = "colvo_tsdf_plan"
    refused(plan(ptrs=(0, p, p)), e, "null pointer")
    refused(plan(out=(p, 0, p, p)), e, "null pointer")
    refused(plan(out=(p, p, p, 0)), e, "null pointer")
    for shape in ((0, 8, 8, 1), (65536, 8, 8, 1), (2, 0, 8, 1), (2, 8, 8, 0), (2, 32768, 32768, 1), (65535, 256, 320, 1)):
        refused(plan(shape=shape), e, "bad shape")
    for g in ((10.0, 0.0, 0.0, 0.0, 0.1, 12, 8, 8), (10.0, 0.0, 0.0, 0.0, 0.1, 8, 8, 0), (10.0, 0.0, 0.0, 0.0, 0.1, 8192, 8192, 8192),
              (10.0, 0.0, 0.0, 0.0, 0.0, 8, 8, 8), (10.0, float("nan"), 0.0, 0.0, 0.1, 8, 8, 8),
              (10.0, 0.0, 0.0, 0.0, float("inf"), 8, 8, 8)):
        refused(plan(grid=g), e, "bad grid")
    for T in (0, 8, -1):
        refused(plan(T=T), e, "bad truncation")
    refused(plan(out=(p + 4, p, p, p)), e, "16-byte aligned")
    refused(plan(out=(p, p + 8, p, p)), e, "16-byte aligned")

    def integrate(shape=(2, 8, 8), grid=grid, T=4, n_bricks=1, ptrs=(p, 0, p, p), bricks=p, pool=p, sums=0):
        return lib.colvo_tsdf_integrate(*ptrs, *shape, *grid, T, bricks, n_bricks, pool, sums, 0, 0)

    e = "colvo_tsdf_integrate"
    refused(integrate(ptrs=(0, 0, p, p)), e, "null pointer")
    refused(integrate(pool=0), e, "null pointer")
    refused(integrate(ptrs=(p, p, p, p)), e, "go together")          # colours without their sums
    refused(integrate(sums=p), e, "go together")
    for shape in ((0, 8, 8), (65536, 8, 8), (2, 32768, 32768)):
        refused(integrate(shape=shape), e, "bad shape")
    refused(integrate(grid=(10.0, 0.0, 0.0, 0.0, 0.1, 8, 8, 20)), e, "bad grid")
    for nb in (0, 2, 1 << 22):
        refused(integrate(n_bricks=nb), e, "n_bricks")
    refused(integrate(n_bricks=1 << 22, grid=(10.0, 0.0, 0.0, 0.0, 0.1, 2048, 2048, 2048)), e, "n_bricks")
    for T in (0, 8):
        refused(integrate(T=T), e, "bad truncation")
    refused(integrate(pool=p + 8), e, "16-byte aligned")
    refused(integrate(ptrs=(p, p, p, p), sums=p + 4), e, "16-byte aligned")

    e = "colvo_tsdf_mesh_count"
    refused(lib.colvo_tsdf_mesh_count(0, p, p, 1, 1, 8, 8, 8, p, p, 0), e, "null pointer")
    refused(lib.colvo_tsdf_mesh_count(p, p, p, 1, 1, 8, 8, 12, p, p, 0), e, "bad grid")
    refused(lib.colvo_tsdf_mesh_count(p, p, p, 2, 1, 8, 8, 8, p, p, 0), e, "n_bricks")
    refused(lib.colvo_tsdf_mesh_count(p, p, p, 1, 0, 8, 8, 8, p, p, 0), e, "min_obs")
    refused(lib.colvo_tsdf_mesh_count(p, p, p, 1, 1, 8, 8, 8, p + 4, p, 0), e, "16-byte aligned")

    def vertices(pool=p, sums=0, n_bricks=1, min_obs=1, vs=0.1, dims=(8, 8, 8), scratch=p, V=5, colors=0, out=p):
        return lib.colvo_tsdf_mesh_vertices(pool, sums, p, p, n_bricks, min_obs, 0.0, 0.0, 0.0, vs, *dims, scratch, V, out, colors, p, p,
                                            p, p, 0)

    e = "colvo_tsdf_mesh_vertices"
    refused(vertices(out=0), e, "null pointer")
    refused(vertices(colors=p), e, "go together")
    refused(vertices(dims=(8, 4, 8)), e, "bad grid")
    refused(vertices(vs=-1.0), e, "bad grid")
    refused(vertices(n_bricks=0), e, "n_bricks")
    refused(vertices(min_obs=0), e, "min_obs")
    for V in (0, 513):
        refused(vertices(V=V), e, "n_vertices")
    refused(vertices(scratch=p + 8), e, "16-byte aligned")

    e = "colvo_tsdf_mesh_faces"
    refused(lib.colvo_tsdf_mesh_faces(p, p, p, 1, 8, 8, 8, p, 0, 2, p, 0), e, "null pointer")
    refused(lib.colvo_tsdf_mesh_faces(p, p, p, 1, 8, 8, 9, p, p, 2, p, 0), e, "bad grid")
    refused(lib.colvo_tsdf_mesh_faces(p, p, p, 3, 8, 8, 8, p, p, 2, p, 0), e, "n_bricks")
    for F in (0, 3, 6 * 512 + 2):
        refused(lib.colvo_tsdf_mesh_faces(p, p, p, 1, 8, 8, 8, p, p, F, p, 0), e, "n_faces")
    refused(lib.colvo_tsdf_mesh_faces(p + 4, p, p, 1, 8, 8, 8, p, p, 2, p, 0), e, "16-byte aligned")


def test_python_calls_refuse_what_they_must():
    from coivo_amd import inference as I
    depths, K, M = (torch.from_numpy(a) for a in CR.tube_scene(2, 8, 8, 3))
    for trunc in (0.05, 0.3 + 0.04, 0.8, 0.0, -0.1, float("nan"), "x", True):        # half a voxel, 3.4 voxels, 8 voxels, ...
        with pytest.raises(ValueError, match="whole number of voxels"):
            I.fuse_tsdf(depths, K, M, voxel_size=0.1, trunc=trunc)
    with pytest.raises(ValueError, match="voxel_size"):
        I.fuse_tsdf(depths, K, M, voxel_size=0.0)
    with pytest.raises(ValueError, match="stride"):
        I.fuse_tsdf(depths, K, M, voxel_size=0.1, stride=0)
    with pytest.raises(ValueError, match="max_depth"):
        I.fuse_tsdf(depths, K, M, voxel_size=0.1, max_depth=float("inf"))
    with pytest.raises(ValueError, match=r"\[N,1,H,W\]"):
        I.fuse_tsdf(depths[0], K, M, voxel_size=0.1)
    with pytest.raises(ValueError):                                  # CPU tensors: there is no fallback
        I.fuse_tsdf(depths, K, M, voxel_size=0.1, trunc=0.3)
    with pytest.raises(ValueError, match="TsdfVolume"):
        I.extract_mesh(depths)
    vol = I.TsdfVolume(torch.zeros(0, 2, dtype=torch.int32), None, torch.zeros(0, dtype=torch.int32), torch.full((1,), -1, dtype=torch.int32),
                       (0.0, 0.0, 0.0), (8, 8, 8), 0.1, 0.4, False, 0, 0, 0)
    with pytest.raises(ValueError, match="min_obs"):
        I.extract_mesh(vol, min_obs=0)
    frames = torch.zeros(3, 3, 8, 8)
    with pytest.raises(ValueError, match="voxel_size"):
        I.reconstruct_sequence(None, None, frames, torch.eye(3), mesh=I.Meshing())
    with pytest.raises(ValueError, match="whole number of voxels"):
        I.reconstruct_sequence(None, None, frames, torch.eye(3), voxel_size=0.05, mesh=I.Meshing(trunc=0.07))
    with pytest.raises(ValueError, match="min_obs"):
        I.reconstruct_sequence(None, None, frames, torch.eye(3), voxel_size=0.05, mesh=I.Meshing(min_obs=0))
    assert I.Meshing() == (None, 2)
    r = I.Reconstruction(1, 2, 3, 4, mesh=7)
    assert r.mesh == 7 and tuple(r) == (1, 2, 3, 4, None) and r._replace(points=9).mesh == 7 and r._replace(mesh=8).mesh == 8
    depths_, rel, traj, points, fused = r                            # still five to unpack
    assert I.Reconstruction(1, 2, 3, 4).mesh is None


# ---- 6. write_ply ---------------------------------------------------------------------------------------------------------------- #
def _read_ply(path):
    """A small reader: -> (vertex rows as a structured array, faces [F,3] or None)."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")[:-2]
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    types = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    n_vertex, n_face, fields, in_face = 0, None, [], False
    for line in lines[2:]:
        w = line.split()
        if w[0] == "element":
            in_face = w[1] == "face"
            if in_face:
                n_face = int(w[2])
            else:
                assert w[1] == "vertex"
                n_vertex = int(w[2])
        elif in_face:
            assert w == ["property", "list", "uchar", "int", "vertex_indices"]
        else:
            assert w[0] == "property"
            fields.append((w[2], types[w[1]]))
    dt = np.dtype(fields)
    body = raw[end:]
    rows = np.frombuffer(body[:n_vertex * dt.itemsize], dtype=dt)
    rest = body[n_vertex * dt.itemsize:]
    if n_face is None:
        assert rest == b""
        return rows, None
    tri = np.frombuffer(rest, dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert len(tri) == n_face and (tri["n"] == 3).all()
    return rows, tri["v"]


def test_write_ply_with_faces_round_trips(tmp_path):
    from coivo_amd import inference as I
    g = torch.Generator().manual_seed(4)
    pts, nrm, col = torch.randn(9, 3, generator=g), torch.randn(9, 3, generator=g), torch.rand(9, 3, generator=g)
    faces = torch.tensor([[0, 1, 2], [2, 1, 3], [8, 7, 6], [4, 5, 0]], dtype=torch.int32)
    path = os.path.join(tmp_path, "mesh.ply")
    I.write_ply(path, pts, col, nrm, faces=faces)
    rows, tri = _read_ply(path)
    assert rows.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
    assert np.array_equal(np.stack([rows["x"], rows["y"], rows["z"]], 1), pts.numpy())
    assert np.array_equal(np.stack([rows["nx"], rows["ny"], rows["nz"]], 1), nrm.numpy())
    assert np.array_equal(np.stack([rows["red"], rows["green"], rows["blue"]], 1), np.rint(col.numpy() * f32(255)).astype(np.uint8))
    assert np.array_equal(tri, faces.numpy())
    I.write_ply(path, pts, faces=faces[:0])
    rows, tri = _read_ply(path)
    assert len(rows) == 9 and tri.shape == (0, 3)
    I.write_ply(path, pts, faces=faces.long())
    assert np.array_equal(_read_ply(path)[1], faces.numpy())
    for bad in (faces.float(), faces[:, :2], faces + 6, faces - 1):
        with pytest.raises(ValueError, match="faces"):
            I.write_ply(path, pts, faces=bad)
    # without faces: the bytes of the writer as it was before faces existed (header and rows spelled out here)
    for c, n in ((None, None), (col, None), (col, nrm)):
        I.write_ply(path, pts, c, n)
        head = ["ply", "format binary_little_endian 1.0", "element vertex 9", "property float x", "property float y", "property float z"]
        parts = [pts.numpy().astype("<f4")]
        if n is not None:
            head += ["property float nx", "property float ny", "property float nz"]
            parts.append(n.numpy().astype("<f4"))
        body = np.concatenate(parts, 1)
        if c is not None:
            head += ["property uchar red", "property uchar green", "property uchar blue"]
            q = np.clip(np.rint(c.numpy() * 255.0), 0, 255).astype(np.uint8)
            body = b"".join(body[i].tobytes() + q[i].tobytes() for i in range(9))
        else:
            body = body.tobytes()
        assert open(path, "rb").read() == ("\n".join(head + ["end_header"]) + "\n").encode("ascii") + body
