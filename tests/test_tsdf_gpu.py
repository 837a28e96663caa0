"""-m gpu: the TSDF fusion and the surface-net meshing (coivo_amd.inference.fuse_tsdf / extract_mesh, csrc/tsdf.hip) against their
NumPy replica (tests/tsdf_ref.py).  What decides a brick, a pixel or a quantum is pinned float32, every sum is an integer and the
vertices are float64 in a written association, so every comparison here -- the normals included -- is equality to the bit."""
import functools

import numpy as np
import pytest
import torch

from tests import consistency_ref as CR
from tests import tsdf_ref as R
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

MAX_DEPTH = 4.5
f32 = np.float32


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _fuse(depths, K, M, colors=None, **kw):
    from coivo_amd import inference as I
    return I.fuse_tsdf(_t(depths), _t(K), _t(M), colors=_t(colors), **kw)


def _mesh(vol, min_obs):
    from coivo_amd import inference as I
    return I.extract_mesh(vol, min_obs=min_obs)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_volume(got, want, what=""):
    for k in ("n_input", "n_outside", "n_bricks"):
        assert getattr(got, k) == want[k], (what, k, getattr(got, k), want[k])
    assert got.trunc == float(want["trunc"]) and got.voxel_size == float(want["voxel_size"]), what
    assert got.origin == tuple(float(o) for o in want["origin"]) and got.dims == tuple(want["dims"]), what
    assert got.brick_list.dtype == torch.int32 and torch.equal(got.brick_list.cpu(), torch.from_numpy(want["brick_list"])), what
    assert torch.equal(got.table.cpu(), torch.from_numpy(want["table"])), what
    assert got.pool.dtype == torch.int32 and got.pool.shape == want["pool"].shape, what
    assert torch.equal(got.pool.cpu(), torch.from_numpy(want["pool"])), what
    assert got.has_colors == (want["color_sums"] is not None)
    if want["color_sums"] is None:
        assert got.color_sums is None, what
    else:
        assert torch.equal(got.color_sums.cpu(), torch.from_numpy(want["color_sums"])), what


def _assert_mesh(got, want, what=""):
    V, F = want["vertices"].shape[0], want["faces"].shape[0]
    assert got.vertices.shape == (V, 3) and got.vertices.dtype == torch.float32, (what, got.vertices.shape, V)
    assert got.faces.shape == (F, 3) and got.faces.dtype == torch.int32, (what, got.faces.shape, F)
    assert got.normals.shape == (V, 3) and got.cells.shape == (V, 3) and got.cells.dtype == torch.int32
    assert got.n_open == want["n_open"], (what, got.n_open, want["n_open"])
    assert torch.equal(got.cells.cpu(), torch.from_numpy(want["cells"])), what
    assert torch.equal(_bits(got.vertices).cpu(), _bits(torch.from_numpy(want["vertices"]))), what
    assert torch.equal(_bits(got.normals).cpu(), _bits(torch.from_numpy(want["normals"]))), what
    assert torch.equal(got.faces.cpu(), torch.from_numpy(want["faces"])), what
    if want["colors"] is None:
        assert got.colors is None, what
    else:
        assert torch.equal(_bits(got.colors).cpu(), _bits(torch.from_numpy(want["colors"]))), what


def _same(a, b):
    """two TsdfVolumes or two Meshes: identical bits"""
    assert type(a) is type(b)
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y))
        else:
            assert x == y


@functools.lru_cache(maxsize=4)
def _tube(N, H, W):
    depths, K, M = CR.tube_scene(N, H, W, 3)
    colors = np.random.default_rng(N * H + W).random((N, 3, H, W)).astype(f32)
    colors[0, :, 0, 0] = (np.nan, -0.5, 1.5)
    return depths, colors, K, M


def _default_grid(K, M, H, W, voxel):
    from coivo_amd import inference as I
    return I.fusion_grid(torch.from_numpy(K), torch.from_numpy(M), H, W, voxel, MAX_DEPTH)


# ---- 1. the small tube ----------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("T", [1, 4, 7])
@pytest.mark.parametrize("with_colors", [True, False])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("H,W", [(24, 32), (17, 23)])
def test_volume_and_mesh_equal_the_replica(H, W, stride, with_colors, T):
    depths, colors, K, M = _tube(5, H, W)
    voxel = 0.1
    origin, dims = _default_grid(K, M, H, W, voxel)
    col = colors if with_colors else None
    trunc = None if T == 4 else T * voxel
    want = R.fuse_tsdf(depths, K, M, voxel_size=voxel, trunc=trunc, colors=col, stride=stride, max_depth=MAX_DEPTH, origin=origin, dims=dims)
    got = _fuse(depths, K, M, col, voxel_size=voxel, trunc=trunc, stride=stride, max_depth=MAX_DEPTH)        # the default grid
    assert want["T"] == T and want["n_bricks"] > 8 and want["n_outside"] == 0
    _assert_volume(got, want, (H, W, stride, with_colors, T))
    for min_obs in (1, 2):
        wm = R.extract_mesh(want, min_obs=min_obs)
        assert len(wm["vertices"]) > 100 and len(wm["faces"]) > 50 and wm["n_open"] > 0
        _assert_mesh(_mesh(got, min_obs), wm, (H, W, stride, with_colors, T, min_obs))


# ---- 2. brick boundaries ----------------------------------------------------------------------------------------------------------- #
def test_surface_across_brick_faces_edges_and_corners():
    """A sphere of sqrt(192) voxels about the centre of a 48^3 grid passes through the eight brick corners (+-8, +-8, +-8) and crosses
    brick faces and edges in all three axes; T = 1 and a marking stride of 8 leave bricks of the band unallocated, so cells reach
    into +neighbour bricks that do not exist: they are open."""
    vs, n = 0.05, 48
    depths, K, M = R.sphere_scene(np.sqrt(192.0) * vs, 32)
    kw = dict(voxel_size=vs, trunc=vs, stride=8, origin=(-n / 2 * vs,) * 3, dims=(n, n, n))
    want = R.fuse_tsdf(depths, K, M, **kw)
    wm = R.extract_mesh(want)
    on_face = (wm["cells"] % 8 == 7).sum(1)                        # cells that span 2, 4 and 8 bricks
    assert (on_face == 1).sum() > 0 and (on_face == 2).sum() > 0 and (on_face == 3).sum() > 0
    for a in range(3):
        assert ((wm["cells"][:, a] % 8 == 7) & (on_face == 1)).any()
    nb = n // 8
    b = want["brick_list"].astype(np.int64)
    missing = 0
    for step, coord in ((1, b % nb), (nb, (b // nb) % nb), (nb * nb, b // (nb * nb))):
        has = coord < nb - 1
        missing += int((want["table"][(b + step)[has]] < 0).sum())
    assert missing > 0 and want["n_bricks"] < nb ** 3 and wm["n_open"] > 0
    got = _fuse(depths, K, M, **kw)
    _assert_volume(got, want)
    _assert_mesh(_mesh(got, 1), wm)


# ---- 3. culling -------------------------------------------------------------------------------------------------------------------- #
def test_culled_and_unculled_integration_give_the_same_bits():
    """70 frames of 8 x 8 along the tube cross the 64-frame cull group; the cameras advance 3.5 tube radii, so every brick is behind
    some cameras, beyond max_depth + trunc of others and only partly inside the image of others."""
    from coivo_amd import _lib, inference as I
    N = 70
    depths, K, M = CR.tube_scene(N, 8, 8, 7)
    colors = np.random.default_rng(2).random((N, 3, 8, 8)).astype(f32)
    kw = dict(voxel_size=0.05, trunc=0.1, max_depth=1.5, colors=colors)
    origin, dims = I.fusion_grid(torch.from_numpy(K), torch.from_numpy(M), 8, 8, 0.05, 1.5)
    want = R.fuse_tsdf(depths, K, M, origin=origin, dims=dims, **kw)
    lib = _lib.load()
    saved = _lib.tune_get("tsdf_cull")
    walked = {}
    try:
        for cull in (1, 0):
            _lib.tune_set("tsdf_cull", cull)
            got = _fuse(depths, K, M, **kw)
            _assert_volume(got, want, f"cull={cull}")
            # the frames each brick walked, through the entry point's optional output
            surv = torch.full((got.n_bricks,), -1, device=dev(), dtype=torch.int32)
            pool = torch.empty_like(got.pool)
            sums = torch.empty_like(got.color_sums)
            d, k, m, c = _t(depths), _t(K), _t(M), _t(colors)
            _lib.check(lib.colvo_tsdf_integrate(d.data_ptr(), c.data_ptr(), k.data_ptr(), m.data_ptr(), N, 8, 8, 1.5, *got.origin,
                                                got.voxel_size, *got.dims, 2, got.brick_list.data_ptr(), got.n_bricks, pool.data_ptr(),
                                                sums.data_ptr(), surv.data_ptr(), _lib.stream_ptr()), "colvo_tsdf_integrate")
            assert torch.equal(pool, got.pool) and torch.equal(sums, got.color_sums)
            walked[cull] = surv.cpu().numpy()
    finally:
        _lib.tune_set("tsdf_cull", saved)
    assert (walked[0] == N).all()
    # per brick, the frames that add to any of its voxels (replica, frame by frame) must all have been walked
    contributing = np.zeros(want["n_bricks"], np.int64)
    for f in range(N):
        p, _ = R.integrate(depths, None, K, M, max_depth=1.5, voxel_size=0.05, T=2, origin=origin, dims=dims,
                           brick_list=want["brick_list"], frames=[f])
        contributing += p[:, 1].reshape(-1, 512).any(1)
    assert (walked[1] >= contributing).all() and (walked[1] <= N).all()
    assert walked[1].max() < N and walked[1].mean() < 0.8 * N, (walked[1].mean(), walked[1].max())       # the cull does cull


# ---- 4. scan chunk boundary -------------------------------------------------------------------------------------------------------- #
def test_more_bricks_than_one_scan_chunk():
    depths, _, K, M = _tube(3, 32, 40)
    voxel = 0.01
    origin, dims = _default_grid(K, M, 32, 40, voxel)
    kw = dict(voxel_size=voxel, trunc=7 * voxel, max_depth=MAX_DEPTH)
    want = R.fuse_tsdf(depths, K, M, origin=origin, dims=dims, **kw)
    assert want["n_bricks"] > 4096
    got = _fuse(depths, K, M, **kw)
    _assert_volume(got, want)
    _assert_mesh(_mesh(got, 1), R.extract_mesh(want, min_obs=1))


# ---- 5. calls and streams ---------------------------------------------------------------------------------------------------------- #
def test_identical_bits_between_calls_and_streams():
    depths, colors, K, M = _tube(5, 24, 32)
    kw = dict(voxel_size=0.1, stride=2, max_depth=MAX_DEPTH)
    a = _fuse(depths, K, M, colors, **kw)
    ma = _mesh(a, 2)
    b = _fuse(depths, K, M, colors, **kw)
    _same(a, b)
    _same(ma, _mesh(b, 2))
    args = [_t(x) for x in (depths, K, M, colors)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    from coivo_amd import inference as I
    with torch.cuda.stream(side):
        c = I.fuse_tsdf(args[0], args[1], args[2], colors=args[3], **kw)
        mc = I.extract_mesh(c, min_obs=2)
    side.synchronize()
    _same(a, c)
    _same(ma, mc)
    perm = np.array([3, 0, 4, 2, 1])
    origin, dims = a.origin, a.dims
    d = _fuse(depths[perm], K[perm], M[perm], colors[perm], origin=origin, dims=dims, **kw)
    _same(a, d)
    _same(ma, _mesh(d, 2))


# ---- 6. degenerate inputs ---------------------------------------------------------------------------------------------------------- #
def _assert_empty_mesh(m, colours):
    assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and m.normals.shape == (0, 3) and m.cells.shape == (0, 3)
    assert m.faces.dtype == torch.int32 and m.cells.dtype == torch.int32 and m.n_open == 0
    assert (m.colors is not None) == colours and (m.colors is None or m.colors.shape == (0, 3))


def test_degenerate_inputs_give_empty_well_formed_results():
    depths, colors, K, M = _tube(5, 17, 23)
    bad = np.empty_like(depths)
    bad[0], bad[1], bad[2], bad[3], bad[4] = 0.0, np.nan, np.inf, MAX_DEPTH, -1.0
    vol = _fuse(bad, K, M, colors, voxel_size=0.1, max_depth=MAX_DEPTH)
    assert (vol.n_input, vol.n_outside, vol.n_bricks) == (0, 0, 0) and vol.pool.shape == (0, 2) and vol.color_sums.shape == (0, 4)
    assert vol.brick_list.shape == (0,) and int((vol.table >= 0).sum()) == 0
    _assert_empty_mesh(_mesh(vol, 1), True)
    # a grid the scene misses entirely
    vol = _fuse(depths, K, M, voxel_size=0.1, max_depth=MAX_DEPTH, origin=(50.0, 50.0, 50.0), dims=(16, 8, 24))
    assert vol.n_input > 0 and vol.n_outside == vol.n_input and vol.n_bricks == 0
    _assert_empty_mesh(_mesh(vol, 1), False)
    # min_obs above every count
    vol = _fuse(depths, K, M, colors, voxel_size=0.1, max_depth=MAX_DEPTH)
    assert vol.n_bricks > 0 and int(vol.pool[:, 1].max()) <= 5
    _assert_empty_mesh(_mesh(vol, 6), True)


# ---- 7. the whole pipeline --------------------------------------------------------------------------------------------------------- #
def test_reconstruct_sequence_also_meshes():
    from coivo_amd import inference as I, nn as hnn, synth
    from oracle import colvo_spec as S
    dn_o, pn_o = S.make_models(31)
    dn, pn = hnn.DepthNet(), hnn.PoseNet()
    dn.load_state_dict(dn_o.state_dict())
    pn.load_state_dict(pn_o.state_dict())
    b = synth.make_batch(5, 64, 96, seed=31)
    frames, K = b["tgt"].to(dev()), b["K"].to(dev())
    # the untrained networks put everything at a depth of about 0.17: voxels of 5 mm, and a grid sized for max_depth = 0.5
    kw = dict(stride=2, chunk=2, voxel_size=0.005, max_depth=0.5)
    plain = I.reconstruct_sequence(dn, pn, frames, K, **kw)
    assert plain.mesh is None
    rec = I.reconstruct_sequence(dn, pn, frames, K, mesh=I.Meshing(trunc=0.02), **kw)
    depths, rel, traj, points, fused = rec                           # still five to unpack
    assert torch.equal(depths, plain.depths) and torch.equal(points, plain.points) and torch.equal(fused.points, plain.fused.points)
    vol = I.fuse_tsdf(depths, K, traj.to(dev(), torch.float32), voxel_size=0.005, trunc=0.02, colors=frames.float().contiguous(), stride=2,
                      max_depth=0.5)
    want = I.extract_mesh(vol, min_obs=2)
    assert isinstance(rec.mesh, I.Mesh) and rec.mesh.vertices.shape[0] > 0 and rec.mesh.faces.shape[0] > 0 and rec.mesh.colors is not None
    _same(rec.mesh, want)


# ---- 8. memory discipline ---------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", ["tube_5x17x23_colours", "more_bricks_than_one_scan_chunk"])
def test_memory_discipline(case):
    """fuse_tsdf and extract_mesh under tests/guarded.py: depths, colours, intrinsics and poses between guard bands; the plan's scratch
    (colvo_tsdf_plan_scratch_bytes), the table, the brick list, the voxel pool, the colour sums, the meshing scratch
    (colvo_tsdf_mesh_scratch_bytes), the vertex ids and every output from the pool under both poisons.  Volume and mesh equal the
    replica, are the same bytes under either poison, and no guard byte changes.  Launches reached: colvo_tsdf_plan, colvo_tsdf_integrate
    (with colours in the first case), colvo_tsdf_mesh_count, _vertices and _faces; the second case's 4096+ bricks take the plan's and
    the meshing's scans past one chunk."""
    from coivo_amd import _lib, inference as I
    from tests import guarded as G
    lib = _lib.load()
    if case == "tube_5x17x23_colours":
        (depths, colors, K, M), voxel, trunc, stride, min_obs = _tube(5, 17, 23), 0.1, None, 2, 2
    else:
        (depths, _, K, M), colors, voxel, trunc, stride, min_obs = _tube(3, 32, 40), None, 0.01, 7 * 0.01, 1, 1
    N, H, W = depths.shape[0], depths.shape[-2], depths.shape[-1]
    origin, dims = _default_grid(K, M, H, W, voxel)
    kw = dict(voxel_size=voxel, trunc=trunc, stride=stride, max_depth=MAX_DEPTH)
    want = R.fuse_tsdf(depths, K, M, colors=colors, origin=origin, dims=dims, **kw)
    wm = R.extract_mesh(want, min_obs=min_obs)
    assert len(wm["faces"]) > 50 and (case.startswith("tube") or want["n_bricks"] > 4096)

    def run(pool):
        vol = I.fuse_tsdf(pool.place(_t(depths)), pool.place(_t(K)), pool.place(_t(M)), colors=pool.place(_t(colors)), **kw)
        return vol, I.extract_mesh(vol, min_obs=min_obs)
    outs, pools = G.under_both_poisons(dev(), run, case)
    for (vol, mesh), pool in zip(outs, pools):
        _assert_volume(vol, want, case)
        _assert_mesh(mesh, wm, case)
        G.assert_served(pool, 0, lib.colvo_tsdf_plan_scratch_bytes(N, H, W, stride, *dims), case + " plan")
        G.assert_served(pool, 0, lib.colvo_tsdf_mesh_scratch_bytes(want["n_bricks"]), case + " mesh")
