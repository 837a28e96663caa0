"""-m gpu: the mesh renderer (coivo_amd.inference.render_mesh, csrc/raster.hip) against its NumPy replica (tests/raster_ref.py).  The
float32 arithmetic is pinned, the edge functions are integers, depth, colour and normal are float64 in a written association, the
minimum is taken on an integer key and every sum is an integer, so every comparison here is equality to the bit -- in both draw
forms (a lane walks its own face / the wave strides a large face together) and both forms of the key offer."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests import raster_ref as R
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

MAX_DEPTH = 4.5
FRAME_GROUP = 16         # csrc/render_common.h: frames a workgroup of the draw kernel walks
f32 = np.float32


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev())    # (a copy: the shared scenes are read-only)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _render(v, f, K, M, H, W, colors=None, **kw):
    from coivo_amd import inference as I
    return I.render_mesh(_t(np.asarray(v, f32).reshape(-1, 3)), _t(np.asarray(f, np.int32).reshape(-1, 3)), _t(K), _t(M), H, W,
                         colors=_t(colors), **kw)


def _assert_equal(got, want, what=""):
    """MeshViews against the replica's dict: every tensor that was asked for, bit for bit."""
    d, i, s = (torch.from_numpy(want[k]) for k in ("depth", "index", "stats"))
    assert got.depth.is_cuda and got.depth.dtype == torch.float32 and got.depth.shape == d.shape, what
    assert got.index.dtype == torch.int32 and got.index.shape == i.shape and got.stats.dtype == torch.int32 and got.stats.shape == s.shape, what
    assert torch.equal(got.stats.cpu(), s), (what, got.stats.cpu(), s)
    assert torch.equal(got.index.cpu(), i), (what, int((got.index.cpu() != i).sum()))
    assert torch.equal(_bits(got.depth.cpu()), _bits(d)), (what, int((_bits(got.depth.cpu()) != _bits(d)).sum()))
    for name in ("colors", "normal", "face_pixels"):
        g = getattr(got, name)
        if g is not None:
            w = torch.from_numpy(want[name])
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
            assert torch.equal(_bits(g.cpu()), _bits(w)), (what, name, int((_bits(g.cpu()) != _bits(w)).sum()))


def _same(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        assert x is None or (x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y)))


@contextlib.contextmanager
def _tuned(name, value):
    from coivo_amd import _lib
    saved = _lib.tune_get(name)
    try:
        _lib.tune_set(name, value)
        yield
    finally:
        _lib.tune_set(name, saved)           # the tests share one process: later ones must see the library's default


@functools.lru_cache(maxsize=None)
def _tube(H, W):
    """-> (vertices, faces, colours, depths, K, cam2world): the tube's mesh at 5 x HxW, voxel 0.1"""
    mesh, d, K, M = R.tube_mesh(5, H, W, 0.1)
    return mesh["vertices"], mesh["faces"], mesh["colors"], d, K, M


@functools.lru_cache(maxsize=None)
def _tube_want(H, W, cull_back):
    """the replica's answer with everything asked for: computed once, shared by the cases below"""
    v, f, c, _, K, M = _tube(H, W)
    return R.render(v, f, K, M, H, W, colors=c, cull_back=cull_back, max_depth=MAX_DEPTH, want_normals=True, want_face_pixels=True)


def _cameras(K, M, N):
    """N cameras: the scene's own, repeated with a small shift each round"""
    n = M.shape[0]
    Kn, Mn = np.stack([K[i % n] for i in range(N)]), np.stack([M[i % n] for i in range(N)]).copy()
    Mn[:, :3, 3] += (np.arange(N) // n)[:, None].astype(f32) * np.array([0.01, -0.02, 0.03], f32)
    return Kn, Mn


# ---- the tube ---------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("want_face_pixels", [False, True])
@pytest.mark.parametrize("want_normals", [False, True])
@pytest.mark.parametrize("cull_back", [False, True])
@pytest.mark.parametrize("with_colors", [False, True])
@pytest.mark.parametrize("H,W", [(24, 32), (17, 23)])
def test_tube_mesh_equals_the_replica(H, W, with_colors, cull_back, want_normals, want_face_pixels):
    v, f, c, _, K, M = _tube(H, W)
    want = dict(_tube_want(H, W, cull_back))
    if not with_colors:
        want["colors"] = None
    got = _render(v, f, K, M, H, W, colors=c if with_colors else None, cull_back=cull_back, max_depth=MAX_DEPTH,
                  want_normals=want_normals, want_face_pixels=want_face_pixels)
    assert (got.colors is not None) == with_colors and (got.normal is not None) == want_normals
    assert (got.face_pixels is not None) == want_face_pixels
    _assert_equal(got, want, (H, W, with_colors, cull_back, want_normals, want_face_pixels))
    s = want["stats"]
    assert len(f) > 2000 and s[:, 0].min() > 500 and s[:, 7].min() > 100 and s[:, 4].sum() > 0 and s[:, 5].sum() > 0
    if want_face_pixels:
        assert int(got.face_pixels.sum()) == int(got.stats[:, 7].sum()) == int(s[:, 7].sum())


@pytest.mark.parametrize("N", [1, FRAME_GROUP, FRAME_GROUP + 1, 2 * FRAME_GROUP + 1])
def test_frame_groups(N):
    H, W = 17, 23
    v, f, c, _, K, M = _tube(H, W)
    Kn, Mn = _cameras(K, M, N)
    kw = dict(colors=c, max_depth=MAX_DEPTH, want_normals=True, want_face_pixels=True)
    _assert_equal(_render(v, f, Kn, Mn, H, W, **kw), R.render(v, f, Kn, Mn, H, W, **kw), N)
    if N > 1:                                                                # one K for every camera
        got = _render(v, f, Kn[0], Mn, H, W, max_depth=MAX_DEPTH)
        _assert_equal(got, R.render(v, f, Kn[0], Mn, H, W, max_depth=MAX_DEPTH), (N, "K [3,3]"))


@pytest.mark.parametrize("F", [0, 1, 255, 256, 257])
def test_face_counts_around_a_workgroup(F):
    H, W = 24, 32
    v, f, c, _, K, M = _tube(H, W)
    seen = np.nonzero(R.setup(v, f, K, M, 2, H, W, MAX_DEPTH, False)["drawn"])[0]
    sub = f[seen[:F]]
    kw = dict(colors=c, max_depth=MAX_DEPTH, want_normals=True, want_face_pixels=True)
    want = R.render(v, sub, K, M, H, W, **kw)
    got = _render(v, sub, K, M, H, W, **kw)
    _assert_equal(got, want, F)
    assert got.face_pixels.shape == (F,) and (want["stats"][2, 1] == F)
    if F == 0:
        assert torch.isinf(got.depth).all() and (got.index == -1).all() and not got.colors.any() and not got.stats.any()
        empty = _render(np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), K, M, H, W, max_depth=MAX_DEPTH, want_face_pixels=True)
        assert (empty.index == -1).all() and not empty.stats.any() and empty.face_pixels.shape == (0,)
        dead = _render(np.zeros((0, 3), f32), [[0, 1, 2]], K, M, H, W, max_depth=MAX_DEPTH)      # faces, no vertices
        assert (dead.index == -1).all() and not dead.stats.any()


# ---- the two draw forms ------------------------------------------------------------------------------------------------ #
def _large_and_small_faces():
    """A 40x40 image (fx = 20, principal point 19.5): two faces that tile more than the image at depth 2, a slanted one in front of
    part of it, one that leaves the image on two sides, and 400 faces of less than a pixel -- the large ones spread over the lanes
    of three waves of two workgroups."""
    rng = np.random.default_rng(17)
    K = np.array([[[20, 0, 19.5], [0, 20, 19.5], [0, 0, 1]]], f32)

    def at(x, y, z):
        return [(x - 19.5) / 20 * z, (y - 19.5) / 20 * z, z]

    verts, faces = [], []
    for _ in range(400):
        x, y, z = rng.uniform(-1, 41), rng.uniform(-1, 41), rng.uniform(1.0, 3.0)
        faces.append([len(verts) + k for k in ((0, 1, 2) if rng.random() < 0.5 else (0, 2, 1))])
        verts += [at(x + rng.uniform(-0.7, 0.7), y + rng.uniform(-0.7, 0.7), z + rng.uniform(-0.05, 0.05)) for _ in range(3)]
    b = len(verts)
    verts += [at(-2, -2, 2.0), at(42, -2, 2.0), at(-2, 42, 2.0), at(42, 42, 2.0),                 # the two halves of a wall
              at(5, 8, 1.2), at(33, 3, 1.9), at(12, 37, 1.6),                                     # slanted, nearer
              at(25, 25, 1.5), at(300, 20, 1.5), at(30, 500, 1.4)]                                # leaves the image
    large = [[b, b + 2, b + 1], [b + 1, b + 2, b + 3], [b + 4, b + 6, b + 5], [b + 7, b + 9, b + 8]]
    for pos, face in zip((0, 70, 130, 300), large):
        faces.insert(pos, face)
    col = rng.random((len(verts), 3), dtype=f32)
    return np.array(verts, f32), np.array(faces, np.int32), col, K, np.eye(4, dtype=f32)[None]


def test_lane_walk_and_wave_walk_give_the_replica_bits():
    v, f, c, K, M = _large_and_small_faces()
    H = W = 40
    kw = dict(colors=c, max_depth=MAX_DEPTH, want_normals=True, want_face_pixels=True)
    want = R.render(v, f, K, M, H, W, **kw)
    assert want["stats"][0, 7] == H * W and want["stats"][0, 6] > H * W + 500          # covered everywhere, a third of it more than once
    boxes = R.setup(v, f, K, M, 0, H, W, MAX_DEPTH, False)
    area = ((boxes["u_hi"] - boxes["u_lo"] + 1) * (boxes["v_hi"] - boxes["v_lo"] + 1))[boxes["drawn"]]
    assert (area >= 256).sum() == 4 and (area <= 4).sum() > 100                          # both sides of the default threshold
    got = {}
    for coop in (0, 1e18, 256, 2):                                                       # every face / none / the default / nearly every
        for load_first in (1, 0):
            with _tuned("raster_coop_min_pixels", coop), _tuned("render_load_first", load_first):
                got[coop, load_first] = _render(v, f, K, M, H, W, **kw)
            _assert_equal(got[coop, load_first], want, (coop, load_first))
    from coivo_amd import _lib
    assert _lib.tune_get("raster_coop_min_pixels") == 256 and _lib.tune_get("render_load_first") == 1
    # the tube: small faces only, drawn by the wave walk
    v, f, c, _, K, M = _tube(24, 32)
    with _tuned("raster_coop_min_pixels", 0):
        _assert_equal(_render(v, f, K, M, 24, 32, colors=c, max_depth=MAX_DEPTH, want_normals=True, want_face_pixels=True),
                      _tube_want(24, 32, False), "tube, wave walk")


def test_deterministic_across_calls_and_streams():
    from coivo_amd import inference as I
    H, W = 24, 32
    v, f, c, _, K, M = _tube(H, W)
    args = (_t(v), _t(f), _t(K), _t(M), H, W)
    kw = dict(colors=_t(c), max_depth=MAX_DEPTH, want_normals=True, want_face_pixels=True)
    a = I.render_mesh(*args, **kw)
    _same(a, I.render_mesh(*args, **kw))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        b = I.render_mesh(*args, **kw)
        b2 = I.render_mesh(*args, **kw)
    side.synchronize()
    _same(a, b)
    _same(a, b2)
    mesh = I.Mesh(args[0], args[1], kw["colors"], args[0], torch.zeros(len(v), 3, dtype=torch.int32, device=dev()), 0)
    _same(a, I.render_mesh(mesh, args[2], args[3], H, W, max_depth=MAX_DEPTH, want_normals=True, want_face_pixels=True))
    _same(a, I.render_mesh(mesh, K=args[2], cam2world=args[3], H=H, W=W, max_depth=MAX_DEPTH, want_normals=True, want_face_pixels=True))
    _assert_equal(a, _tube_want(H, W, False))


# ---- edges ------------------------------------------------------------------------------------------------------------- #
def test_one_pixel_nothing_in_front_and_bad_indices():
    v, f, c, _, K, M = _tube(24, 32)
    K1 = K.copy()
    K1[:, 0, 2] -= 4                                                         # the one pixel is pixel (4, 12) of the 24x32 image: the wall
    K1[:, 1, 2] -= 12
    kw = dict(colors=c, max_depth=MAX_DEPTH, want_normals=True, want_face_pixels=True)
    want = R.render(v, f, K1, M, 1, 1, **kw)
    assert (want["index"] >= 0).all()
    _assert_equal(_render(v, f, K1, M, 1, 1, **kw), want, "1x1")
    for H, W in ((1, 70), (70, 1)):
        _assert_equal(_render(v, f, K, M, H, W, **kw), R.render(v, f, K, M, H, W, **kw), (H, W))
    kw["max_depth"] = 1e-3                                                   # nothing is nearer than that and beyond 1e-3
    want = R.render(v, f, K, M, 24, 32, **kw)
    assert not want["stats"].any() and (want["index"] == -1).all()
    _assert_equal(_render(v, f, K, M, 24, 32, **kw), want, "nothing in front")
    kw["max_depth"] = 2.0                                                    # the limit cuts through the wall: faces straddle it
    want = R.render(v, f, K, M, 24, 32, **kw)
    assert want["stats"][:, 2].min() > 100 and want["stats"][:, 0].min() > 300
    _assert_equal(_render(v, f, K, M, 24, 32, **kw), want, "straddling")
    kw["max_depth"] = MAX_DEPTH
    bad = np.array([[0, 1, len(v)], [-1, 2, 3], [4, 2 ** 31 - 1, 5], [-2 ** 31, 0, 1]], np.int32)
    f2 = np.concatenate([bad[:2], f, bad[2:]])
    want = R.render(v, f2, K, M, 24, 32, **kw)
    assert np.array_equal(want["stats"], _tube_want(24, 32, False)["stats"])
    _assert_equal(_render(v, f2, K, M, 24, 32, **kw), want, "indices out of range")


def test_hostile_vertices_and_cameras():
    v, f, c, _, K, M = _tube(17, 23)
    v2 = v.copy()
    v2[50] = np.nan
    v2[60, 2] = np.inf
    v2[70, 0] = -np.inf
    v2[80] = 1e30
    v2[90] = M[2, :3, 3]                                                     # a vertex in the camera centre of frame 2
    kw = dict(colors=c, max_depth=MAX_DEPTH, want_normals=True, want_face_pixels=True)
    _assert_equal(_render(v2, f, K, M, 17, 23, **kw), R.render(v2, f, K, M, 17, 23, **kw), "hostile vertices")
    K2, M2 = K.copy(), M.copy()
    K2[0, 0, 0] = np.nan                                                     # every front face of frame 0 leaves the guard band
    K2[1, 0, 0] = 1e7                                                        # ... most of frame 1's
    K2[3, 1, 1] = -K2[3, 1, 1]                                               # mirrored: the windings flip
    M2[4, 0, 3] = np.inf
    want = R.render(v, f, K2, M2, 17, 23, **kw)
    assert want["stats"][0, 3] == want["stats"][0, 0] > 0 and want["stats"][1, 3] > 100 and want["stats"][3, 4] > 500
    assert not want["stats"][4].any()
    _assert_equal(_render(v, f, K2, M2, 17, 23, **kw), want, "hostile cameras")
    want = R.render(v, f, K2, M2, 17, 23, cull_back=True, **kw)
    _assert_equal(_render(v, f, K2, M2, 17, 23, cull_back=True, **kw), want, "hostile cameras, culled")


def test_ties_go_to_the_smaller_face():
    H, W = 24, 32
    v, f, c, _, K, M = _tube(H, W)
    once = _tube_want(H, W, False)
    want = R.render(v, np.concatenate([f, f]), K, M, H, W, colors=c, max_depth=MAX_DEPTH, want_face_pixels=True)
    assert want["index"].max() < len(f) and np.array_equal(want["index"], once["index"])
    assert np.array_equal(want["stats"][:, :7], 2 * once["stats"][:, :7]) and np.array_equal(want["stats"][:, 7], once["stats"][:, 7])
    assert not want["face_pixels"][len(f):].any()
    _assert_equal(_render(v, np.concatenate([f, f]), K, M, H, W, colors=c, max_depth=MAX_DEPTH, want_face_pixels=True), want)


# ---- consumers --------------------------------------------------------------------------------------------------------- #
def test_rendered_depth_feeds_the_consumers():
    from coivo_amd import evaluate as E, inference as I
    H, W = 24, 32
    v, f, _, d, K, M = _tube(H, W)
    Kt, Mt = _t(K), _t(M)
    r = I.render_mesh(_t(v), _t(f), Kt, Mt, H, W, max_depth=MAX_DEPTH)
    assert r.normal is None and r.colors is None and r.face_pixels is None
    covered = r.index >= 0
    n_cov = int(covered.sum())
    assert 0 < n_cov < covered.numel() and int(r.stats[:, 7].sum()) == n_cov
    m = E.depth_metrics(r.depth, _t(d), mask=covered, max_depth=MAX_DEPTH, median_scaling=False)
    print(f"abs_rel of the mesh's depth against ground truth at 24x32, voxel 0.1: {m.per_image[:, 0].tolist()}")
    assert torch.isfinite(m.per_image).all() and (m.per_image[:, 0] < 0.02).all()
    cloud = I.stitch_point_cloud(r.depth, Kt, Mt, stride=1, max_depth=MAX_DEPTH)
    assert cloud.shape[0] == n_cov                                           # +inf is dropped, nothing else
    fused = I.fuse_point_cloud(r.depth, Kt, Mt, voxel_size=0.125, max_depth=MAX_DEPTH)
    assert fused.n_input == n_cov
    filt = I.filter_depths(r.depth, Kt, Mt, max_depth=MAX_DEPTH)
    assert int(filt.stats[:, 0].sum()) == n_cov


def test_reconstruct_sequence_draws_the_mesh_when_asked():
    from coivo_amd import inference as I, nn as hnn, synth
    from oracle import colvo_spec as S
    dn_o, pn_o = S.make_models(31)
    dn, pn = hnn.DepthNet(), hnn.PoseNet()
    dn.load_state_dict(dn_o.state_dict())
    pn.load_state_dict(pn_o.state_dict())
    b = synth.make_batch(5, 64, 96, seed=31)
    frames, K = b["tgt"].to(dev()), b["K"].to(dev())
    # the untrained networks put everything at a depth of about 0.17: voxels of 5 mm, and a grid sized for max_depth = 0.5
    kw = dict(stride=2, chunk=2, voxel_size=0.005, max_depth=0.5, mesh=I.Meshing(trunc=0.02))
    plain = I.reconstruct_sequence(dn, pn, frames, K, **kw)
    assert plain.rendered is None and plain.mesh is not None
    cloud = I.reconstruct_sequence(dn, pn, frames, K, render=I.Render(), **kw)
    assert isinstance(cloud.rendered, I.RenderedViews)                      # mesh=False: the cloud, as before
    rec = I.reconstruct_sequence(dn, pn, frames, K, render=I.Render(mesh=True), **kw)
    assert len(rec) == 5 and isinstance(rec.rendered, I.MeshViews) and rec.normals is None
    assert torch.equal(rec.depths, plain.depths) and torch.equal(rec.mesh.faces, plain.mesh.faces)
    traj32 = rec.cam2world.to(dev(), torch.float32)
    vol = I.fuse_tsdf(rec.depths, K, traj32, voxel_size=0.005, trunc=0.02, colors=frames.float().contiguous(), stride=2, max_depth=0.5)
    want = I.render_mesh(I.extract_mesh(vol, min_obs=2), K.to(torch.float32).contiguous(), traj32, 64, 96, max_depth=0.5)
    _same(rec.rendered, want)
    assert rec.rendered.depth.shape == (5, 1, 64, 96) and rec.rendered.colors.shape == (5, 3, 64, 96) and rec.rendered.stats.shape == (5, 8)
    assert int((rec.rendered.index >= 0).sum()) > 1000
    with pytest.raises(ValueError, match="Meshing"):
        I.reconstruct_sequence(dn, pn, frames, K, stride=2, chunk=2, voxel_size=0.005, max_depth=0.5, render=I.Render(mesh=True))


# ---- refusals ---------------------------------------------------------------------------------------------------------- #
def test_argument_errors_on_the_device_path_launch_nothing():
    from coivo_amd import inference as I
    v, f, c, _, K, M = (_t(a) for a in _tube(17, 23))
    for bad in ((v.cpu(), f, K, M), (v, f.cpu(), K, M), (v, f, K.cpu(), M), (v, f, K, M.cpu()), (v.double(), f, K, M),
                (v, f.long(), K, M), (v, f, K[:2], M), (v, f.t(), K, M)):
        with pytest.raises(ValueError):
            I.render_mesh(*bad, 17, 23)
    with pytest.raises(ValueError, match="colors"):
        I.render_mesh(v, f, K, M, 17, 23, colors=c[:-1])
    out = I.render_mesh(v[::2], f, K, M, 17, 23, colors=c[::2], max_depth=MAX_DEPTH)             # non-contiguous input: taken as it reads
    assert out.depth.shape == (5, 1, 17, 23) and out.colors.shape == (5, 3, 17, 23)
    assert int(out.stats[:, 0].sum()) < int(I.render_mesh(v, f, K, M, 17, 23, max_depth=MAX_DEPTH).stats[:, 0].sum())   # half the faces are dead


# ---- memory discipline ------------------------------------------------------------------------------------------------- #
def test_memory_discipline():
    """render_mesh under tests/guarded.py: vertices, faces, colours, intrinsics and the pose between guard bands; the scratch
    (colvo_render_scratch_bytes), depth, index, colours, normals, the per-face pixel counts and the statistics from the pool under both
    poisons.  Outputs equal the replica, are the same bytes under either poison, and no guard byte changes.  Launches reached: the
    clearing of the keys, the draw kernel in both forms -- 400 faces below a pixel on the lane walk, four large ones (two larger than
    the 40 x 40 image, one leaving it on two sides: their clamped boxes end on the image's last row) on the wave walk, at the default
    threshold and with every face on the wave walk -- and the resolve with colours, normals and face counts; then the tube's 5 views
    of 17 x 23 with back-face culling."""
    from coivo_amd import _lib, inference as I
    from tests import guarded as G
    lib = _lib.load()
    v, f, c, K, M = _large_and_small_faces()
    kw = dict(max_depth=MAX_DEPTH, want_normals=True, want_face_pixels=True)
    want = R.render(v, f, K, M, 40, 40, colors=c, **kw)
    run = lambda pool: I.render_mesh(pool.place(_t(v)), pool.place(_t(f)), pool.place(_t(K)), pool.place(_t(M)), 40, 40,
                                     colors=pool.place(_t(c)), **kw)
    for coop in (256, 0):
        with _tuned("raster_coop_min_pixels", coop):
            outs, pools = G.under_both_poisons(dev(), run, f"render_mesh, wave walk from {coop} pixels")
        for got, pool in zip(outs, pools):
            _assert_equal(got, want, coop)
            G.assert_served(pool, 0, lib.colvo_render_scratch_bytes(1, 40, 40), "render_mesh")
    v, f, c, _, K, M = _tube(17, 23)
    want = _tube_want(17, 23, True)
    run = lambda pool: I.render_mesh(pool.place(_t(v)), pool.place(_t(f)), pool.place(_t(K)), pool.place(_t(M)), 17, 23,
                                     colors=pool.place(_t(c)), cull_back=True, **kw)
    outs, pools = G.under_both_poisons(dev(), run, "render_mesh, the tube")
    for got, pool in zip(outs, pools):
        _assert_equal(got, want, "tube")
        G.assert_served(pool, 0, lib.colvo_render_scratch_bytes(M.shape[0], 17, 23), "render_mesh")
