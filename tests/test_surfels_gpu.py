"""-m gpu: the oriented-disc renderer (coivo_amd.inference.render_surfels / render_fused, csrc/surfels.hip) against its NumPy replica
(tests/surfel_ref.py).  The arithmetic is pinned (float32, one rounding per operation), the minimum is taken on an integer key and every
sum is an integer, so every comparison here is equality to the bit -- the one exception being WHICH NaN a normal plane holds where
the winner's normal is not finite: a NaN must be a NaN in the same place."""
import functools

import numpy as np
import pytest
import torch

from tests import consistency_ref as CR
from tests import normals_ref as NR
from tests import render_ref as R
from tests import surfel_ref as S
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

MAX_DEPTH = 4.5
SEED = 5
FRAME_GROUP = 16         # csrc/render_common.h: frames a workgroup of a splat kernel walks


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _render(points, normals, K, M, H, W, colors=None, want_normals=True, **kw):
    from coivo_amd import inference as I
    return I.render_surfels(_t(points), _t(normals), _t(K), _t(M), H, W, colors=None if colors is None else _t(colors),
                            want_normals=want_normals, **kw)


def _assert_equal(got, want, what=""):
    """SurfelViews against the replica's dict: every tensor bit for bit."""
    d, i, s = (torch.from_numpy(want[k]) for k in ("depth", "index", "stats"))
    assert got.depth.is_cuda and got.depth.dtype == torch.float32 and got.depth.shape == d.shape, what
    assert got.index.dtype == torch.int32 and got.index.shape == i.shape and got.stats.dtype == torch.int32 and got.stats.shape == s.shape, what
    assert torch.equal(got.stats.cpu(), s), (what, got.stats.cpu(), s)
    assert torch.equal(got.index.cpu(), i), (what, int((got.index.cpu() != i).sum()))
    assert torch.equal(_bits(got.depth.cpu()), _bits(d)), (what, int((_bits(got.depth.cpu()) != _bits(d)).sum()))
    if want["colors"] is None:
        assert got.colors is None, what
    else:
        c = torch.from_numpy(want["colors"])
        assert got.colors.dtype == torch.float32 and got.colors.shape == c.shape and torch.equal(_bits(got.colors.cpu()), _bits(c)), what
    if got.normal is not None:
        n, g = torch.from_numpy(want["normal"]), got.normal.cpu()
        assert g.dtype == torch.float32 and g.shape == n.shape and torch.equal(torch.isnan(g), torch.isnan(n)), what
        ok = ~torch.isnan(n)
        assert torch.equal(_bits(g)[ok], _bits(n)[ok]), (what, "normal", int((_bits(g)[ok] != _bits(n)[ok]).sum()))


def _same(a, b):
    assert torch.equal(_bits(a.depth), _bits(b.depth)) and torch.equal(a.index, b.index) and torch.equal(a.stats, b.stats)
    assert (a.colors is None) == (b.colors is None) and (a.colors is None or torch.equal(_bits(a.colors), _bits(b.colors)))
    assert (a.normal is None) == (b.normal is None) and (a.normal is None or torch.equal(_bits(a.normal), _bits(b.normal)))


def _check(points, normals, K, M, H, W, colors=None, what="", want_normals=True, **kw):
    want = S.render(points, normals, K, M, H, W, colors=colors, **kw)
    _assert_equal(_render(points, normals, K, M, H, W, colors=colors, want_normals=want_normals, **kw), want, what)
    return want


@functools.lru_cache(maxsize=None)
def _tube(N, H, W):
    """-> (points, normals, colours, depths, K, cam2world) of the tube: every frame's samples with the replica's own normals."""
    pts, d, K, M = R.tube_points(N, H, W, SEED)
    s = NR.sample_normals(d, K, M, max_depth=np.inf, rel_edge=0.05 if H >= 64 else 0.2)
    nrm = (s["q"][np.isfinite(d[:, 0])] / 16384.0).astype(np.float32)
    col = np.random.default_rng(1).random(pts.shape, dtype=np.float32)
    return pts, nrm, col, d, K, M


def _cams(N, H, W, per_frame_K=False):
    K = None
    if per_frame_K:
        rng = np.random.default_rng(11)
        K = np.zeros((N, 3, 3), np.float32)
        zoom = rng.uniform(0.9, 1.25, N)
        K[:, 0, 0] = 0.8 * W * zoom
        K[:, 1, 1] = 0.8 * W * zoom * rng.uniform(0.97, 1.03, N)
        K[:, 0, 2] = (W - 1) / 2 + rng.uniform(-4, 4, N)
        K[:, 1, 2] = (H - 1) / 2 + rng.uniform(-3, 3, N)
        K[:, 2, 2] = 1
    return CR.tube_scene(N, H, W, SEED, K=K)


def _frustum_points(m, seed, K, M, H, W):
    """m points spread over (and a little around) the views of the cameras given, depths on both sides of MAX_DEPTH, with normals that
    mostly face the camera they were placed in (a third are random: some face away, some are zero)."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, M.shape[0], m)
    z = rng.uniform(0.2, 1.2 * MAX_DEPTH, m)
    u, v = rng.uniform(-3, W + 2, m), rng.uniform(-3, H + 2, m)
    k, c = K[n].astype(np.float64), M[n].astype(np.float64)
    cam = np.stack([(u - k[:, 0, 2]) / k[:, 0, 0] * z, (v - k[:, 1, 2]) / k[:, 1, 1] * z, z], -1)
    nc = rng.normal(size=(m, 3)) * 0.5 + np.array([0, 0, -1.0])
    nc /= np.linalg.norm(nc, axis=1, keepdims=True)
    rnd = rng.normal(size=(m, 3))
    nc = np.where((np.arange(m) % 3 == 0)[:, None], rnd / np.linalg.norm(rnd, axis=1, keepdims=True), nc)
    nc[np.arange(m) % 7 == 3] = 0
    pts = (np.einsum("nij,nj->ni", c[:, :3, :3], cam) + c[:, :3, 3]).astype(np.float32)
    return pts, np.einsum("nij,nj->ni", c[:, :3, :3], nc).astype(np.float32)


# ---- the tube ---------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("radius,max_splat", [(0.02, 8), (0.05, 4), (0.0, 8), (0.05, 2)])
@pytest.mark.parametrize("H,W", [(17, 23), (64, 96)])
def test_tube_equals_the_replica(H, W, radius, max_splat):
    pts, nrm, col, _, K, M = _tube(3, H, W)
    want = _check(pts, nrm, K[1:2], M[1:2], H, W, colors=col, radius=radius, max_splat=max_splat, max_depth=MAX_DEPTH,
                  what=(H, W, radius, max_splat))
    front, drawn, clipped, covered, culled, flat = want["stats"][0].tolist()
    assert front > drawn > 0 and covered > 0 and flat < front // 4 and culled < front // 20
    assert want["normal"].any()
    if (radius, max_splat, H) == (0.05, 2, 64):
        assert clipped > 0
    if radius > 0:
        sq = R.render(pts, K[1:2], M[1:2], H, W, radius=radius, max_splat=max_splat, max_depth=MAX_DEPTH)
        assert not np.array_equal(sq["depth"], want["depth"])                 # the discs do carry their own depths


# ---- tails ------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("H,W", [(1, 1), (1, 70), (17, 23)])
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 257])
def test_tails(m, H, W):
    _, K, M = _cams(2, H, W)
    pts, nrm = _frustum_points(m, 100 + m, K, M, H, W)
    col = np.random.default_rng(m).random((m, 3), dtype=np.float32)
    want = _check(pts, nrm, K, M, H, W, colors=col, radius=0.03, max_splat=3, max_depth=MAX_DEPTH, what=(m, H, W))
    if m >= 63:
        assert (want["stats"][:, 0] < m).all() and want["stats"][:, 5].min() > 0
        assert want["stats"][:, 1].min() > 0 or H * W == 1                   # (one pixel: a frame's few discs may all miss its centre)
    if m >= 257:
        assert want["stats"][:, 4].min() > 0
    if m == 0:
        assert not want["stats"].any() and (want["index"] == -1).all()
    _check(pts, nrm, K, M, H, W, radius=0.03, max_splat=3, max_depth=MAX_DEPTH, want_normals=False, what=(m, H, W, "no colours"))


@pytest.mark.parametrize("N", [1, 3, 37])
def test_frame_groups_with_intrinsics_that_differ_per_frame(N):
    assert 37 > 2 * FRAME_GROUP and 37 % FRAME_GROUP
    H, W = 17, 23
    _, K, M = _cams(N, H, W, per_frame_K=True)
    pts, nrm = _frustum_points(500, 7, K, M, H, W)
    col = np.random.default_rng(3).random((500, 3), dtype=np.float32)
    want = _check(pts, nrm, K, M, H, W, colors=col, radius=0.04, max_splat=8, max_depth=MAX_DEPTH, what=N)
    assert want["stats"][:, 1].min() > 0
    if N > 1:
        wrong = S.render(pts, nrm, np.broadcast_to(K[0], K.shape), M, H, W, radius=0.04, max_splat=8, max_depth=MAX_DEPTH)
        assert not np.array_equal(wrong["index"], want["index"])
        one = _render(pts, nrm, K[0], M, H, W, radius=0.04, max_splat=8, max_depth=MAX_DEPTH)           # K [3,3] serves every frame
        _assert_equal(one, wrong)


# ---- borders, culling, hostile values ----------------------------------------------------------------------------------- #
_K = np.array([[[8, 0, 3], [0, 8, 5], [0, 0, 1]]], np.float32)      # x = 8 X / Z + 3, y = 8 Y / Z + 5: exact at Z = 2
_I = np.eye(4, dtype=np.float32)[None]


def _at(x, y, z=2.0):
    return [(x - 3) * z / 8, (y - 5) * z / 8, z]


def test_footprints_that_cross_every_edge_and_corner():
    H, W = 11, 7                                               # radius 0.5 at Z = 2: half-width 2 pixels
    xs, ys = (-1.0, 3.0, 7.0), (-1.5, 5.0, 11.5)
    pts = np.array([_at(x, y) for y in ys for x in xs], np.float32)
    for normal in ([0, 0, -1], [0.3, -0.2, -1], [0, 0, 0]):
        nrm = np.tile(np.array(normal, np.float32), (9, 1))
        want = _check(pts, nrm, _K, _I, H, W, radius=0.5, max_splat=8, max_depth=MAX_DEPTH, what=normal)
        assert want["stats"].tolist()[0][:3:2] == [9, 0]
        if normal[0] == 0:                                                    # (a tilted disc beside the image may miss every pixel centre)
            assert want["stats"][0, 1] == 9 and set(range(9)) <= set(np.unique(want["index"]).tolist())
        else:
            assert 5 <= want["stats"][0, 1] < 9
    far = np.array([_at(-3.0, 5.0), _at(10.0, 5.0), _at(3.0, -3.5), _at(3.0, 14.0)], np.float32)
    want = _check(far, np.tile(np.array([0, 0, -1], np.float32), (4, 1)), _K, _I, H, W, radius=0.5, max_splat=8, max_depth=MAX_DEPTH)
    assert want["stats"].tolist() == [[4, 0, 0, 0, 0, 0]]


def test_zero_normals_reproduce_render_cloud():
    from coivo_amd import inference as I
    H, W = 64, 96
    pts, nrm, col, _, K, M = _tube(3, H, W)
    kw = dict(radius=0.03, colors=_t(col), max_splat=6, max_depth=MAX_DEPTH)
    sq = I.render_cloud(_t(pts), _t(K), _t(M), H, W, **kw)
    for normals, radius in ((np.zeros_like(nrm), 0.03), (np.full_like(nrm, np.nan), 0.03)):
        got = I.render_surfels(_t(pts), _t(normals), _t(K), _t(M), H, W, want_normals=True, **kw)
        assert torch.equal(_bits(got.depth), _bits(sq.depth)) and torch.equal(got.index, sq.index) and torch.equal(_bits(got.colors), _bits(sq.colors))
        assert torch.equal(got.stats[:, :4], sq.stats) and not got.stats[:, 4].any() and torch.equal(got.stats[:, 5], got.stats[:, 0])
        assert not got.normal.any()
    # radius 0 with normals that face the cameras: the nearest pixel alone, as render_cloud
    kw["radius"] = 0.0
    sq = I.render_cloud(_t(pts), _t(K), _t(M), H, W, **kw)
    got = I.render_surfels(_t(pts), _t(nrm), _t(K), _t(M), H, W, **kw)
    assert not got.stats[:, 4].any()
    assert torch.equal(_bits(got.depth), _bits(sq.depth)) and torch.equal(got.index, sq.index) and torch.equal(got.stats[:, :4], sq.stats)


def test_back_facing_points_are_culled_and_counted():
    H, W = 64, 96
    pts, nrm, col, _, K, M = _tube(3, H, W)
    want = _check(pts, -nrm, K, M, H, W, colors=col, radius=0.02, max_splat=8, max_depth=MAX_DEPTH, what="all normals turned away")
    front, drawn, _, covered, culled, flat = want["stats"].sum(0).tolist()
    assert culled + flat == front and drawn <= flat and culled > 0.9 * front
    half = nrm.copy()
    half[::2] *= -1
    want = _check(pts, half, K, M, H, W, colors=col, radius=0.02, max_splat=8, max_depth=MAX_DEPTH, what="every other normal turned away")
    assert (want["index"][want["index"] >= 0] % 2 == 1).mean() > 0.95        # what shows faces the camera (or has no normal)


def test_hostile_normals():
    H, W = 11, 7
    nan, inf = np.nan, np.inf
    nrm = np.array([[nan, 0, -1], [0, nan, 0], [inf, 0, -1], [0, 0, -inf], [-inf, inf, -inf], [0, 0, -1e-30], [0, 0, -1e-20], [1e-20, 0, -1e-20],
                    [0, 0, -3], [2, 1, -3], [0, 0, -3e38], [3e38, 0, -3e38], [0, 0, -0.0], [1e-45, 0, 0], [0, 0, -1]], np.float32)
    m = len(nrm)
    rng = np.random.default_rng(9)
    pts = np.array([_at(rng.uniform(0, 6), rng.uniform(0, 10), rng.uniform(1.5, 3.0)) for _ in range(m)], np.float32)
    col = rng.random((m, 3), dtype=np.float32)
    for radius, ms in ((0.25, 8), (0.0, 8), (0.25, 0), (3e38, 32)):
        want = _check(pts, nrm, _K, _I, H, W, colors=col, radius=radius, max_splat=ms, max_depth=MAX_DEPTH, what=(radius, ms))
        assert want["stats"][0, 0] == m and want["stats"][0, 5] >= 4          # NaN, 1e-30 (its square is zero) and -0.0 count as flat
    # hostile points with good normals, and a camera whose own entries are hostile
    bad = np.array([[nan, 0, 2], [0, 0, inf], [1e30, 0, 2], [0, 0, -2], [0, 0, 0], [0, 0, 1e-3], _at(1.0, 2.0), _at(5.0, 9.0, 3.0)], np.float32)
    nb = np.tile(np.array([0.1, 0.2, -1], np.float32), (len(bad), 1))
    _check(bad, nb, _K, _I, H, W, radius=0.25, max_splat=8, max_depth=MAX_DEPTH, what="hostile points")
    K2, M2 = np.repeat(_K, 3, 0), np.repeat(_I, 3, 0)
    K2[0, 0, 0] = nan
    M2[2, 0, 3] = inf
    want = _check(bad, nb, K2, M2, H, W, radius=0.25, max_splat=8, max_depth=MAX_DEPTH, what="hostile cameras")
    assert (want["index"][[0, 2]] == -1).all() and want["stats"][1, 1] == 2
    K3 = _K.copy()
    K3[0, 0, 0] = -8
    _check(bad[-2:], nb[-2:], K3, _I, H, W, radius=0.25, max_splat=8, max_depth=MAX_DEPTH, what="negative focal length")


def test_ties_go_to_the_smaller_index():
    H, W = 64, 96
    pts, nrm, col, _, K, M = _tube(3, H, W)
    m = pts.shape[0]
    want = _check(np.concatenate([pts, pts]), np.concatenate([nrm, nrm]), K[1:2], M[1:2], H, W, colors=np.concatenate([col, 1 - col]),
                  radius=0.02, max_splat=8, max_depth=MAX_DEPTH)
    once = S.render(pts, nrm, K[1:2], M[1:2], H, W, colors=col, radius=0.02, max_splat=8, max_depth=MAX_DEPTH)
    assert want["index"].max() < m and np.array_equal(want["index"], once["index"]) and np.array_equal(want["colors"], once["colors"])
    assert np.array_equal(want["stats"][:, [0, 1, 2, 4, 5]], 2 * once["stats"][:, [0, 1, 2, 4, 5]])
    assert np.array_equal(want["stats"][:, 3], once["stats"][:, 3])


# ---- determinism ------------------------------------------------------------------------------------------------------- #
def test_deterministic_across_calls_streams_and_splat_forms():
    from coivo_amd import _lib, inference as I
    H, W = 64, 96
    pts, nrm, col, _, K, M = _tube(3, H, W)
    args = (_t(pts), _t(nrm), _t(K), _t(M), H, W)
    kw = dict(radius=0.03, colors=_t(col), max_splat=6, max_depth=MAX_DEPTH, want_normals=True)
    a = I.render_surfels(*args, **kw)
    _same(a, I.render_surfels(*args, **kw))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        c = I.render_surfels(*args, **kw)
    side.synchronize()
    _same(a, c)
    saved = _lib.tune_get("render_load_first")
    try:
        for form in (1, 0):
            _lib.tune_set("render_load_first", form)
            _same(a, I.render_surfels(*args, **kw))
    finally:
        _lib.tune_set("render_load_first", saved)
    _assert_equal(a, S.render(pts, nrm, K, M, H, W, colors=col, radius=0.03, max_splat=6, max_depth=MAX_DEPTH))


# ---- consumers --------------------------------------------------------------------------------------------------------- #
def test_rendered_depth_feeds_the_consumers_and_is_less_biased_than_the_squares():
    from coivo_amd import evaluate as E, inference as I
    H, W = 64, 96
    pts, nrm, _, d, K, M = _tube(3, H, W)
    Kt, Mt = _t(K), _t(M)
    r = I.render_surfels(_t(pts), _t(nrm), Kt, Mt, H, W, radius=0.02, max_depth=MAX_DEPTH)
    assert r.normal is None and r.colors is None
    covered = r.index >= 0
    n_cov = int(covered.sum())
    assert 0 < n_cov < covered.numel() and int(r.stats[:, 3].sum()) == n_cov
    m = E.depth_metrics(r.depth, _t(d), mask=covered, max_depth=MAX_DEPTH, median_scaling=False)
    sq = I.render_cloud(_t(pts), Kt, Mt, H, W, radius=0.02, max_depth=MAX_DEPTH)
    m_sq = E.depth_metrics(sq.depth, _t(d), mask=sq.index >= 0, max_depth=MAX_DEPTH, median_scaling=False)
    print(f"abs_rel against ground truth, radius 0.02 at 64x96: discs {m.per_image[:, 0].tolist()}, squares {m_sq.per_image[:, 0].tolist()}")
    assert torch.isfinite(m.per_image).all() and (m.per_image[:, 0] < m_sq.per_image[:, 0]).all()
    cloud = I.stitch_point_cloud(r.depth, Kt, Mt, stride=1, max_depth=MAX_DEPTH)
    assert cloud.shape[0] == n_cov                                           # +inf is dropped, nothing else
    fused = I.fuse_point_cloud(r.depth, Kt, Mt, voxel_size=0.125, max_depth=MAX_DEPTH)
    assert fused.n_input == n_cov
    filt = I.filter_depths(r.depth, Kt, Mt, max_depth=MAX_DEPTH)
    assert int(filt.stats[:, 0].sum()) == n_cov


def test_render_fused_with_cloud_normals():
    from coivo_amd import inference as I
    H, W = 64, 96
    d, K, M = CR.tube_scene(5, H, W, SEED)
    dt, Kt, Mt = _t(d), _t(K), _t(M)
    fused = I.fuse_point_cloud(dt, Kt, Mt, voxel_size=0.02, max_depth=MAX_DEPTH)
    cn = I.cloud_normals(fused, dt, Kt, Mt, max_depth=MAX_DEPTH)
    a = I.render_fused(fused, Kt, Mt, H, W, max_depth=MAX_DEPTH, normals=cn, want_normals=True)
    b = I.render_fused(fused, Kt, Mt, H, W, max_depth=MAX_DEPTH, normals=cn.normals, want_normals=True)
    _same(a, b)
    assert isinstance(a, I.SurfelViews) and isinstance(I.render_fused(fused, Kt, Mt, H, W, max_depth=MAX_DEPTH), I.RenderedViews)
    want = S.render(fused.points.cpu().numpy(), cn.normals.cpu().numpy(), K, M, H, W, radius=fused.voxel_size, max_splat=8, max_depth=MAX_DEPTH)
    assert a.colors is None
    _assert_equal(a, want)
    # the fused cloud with its own normals: the median error of the model's depth in frame 2 falls well below the squares' 1.5 %
    gt = dt[2, 0]
    keep = (gt < MAX_DEPTH) & (a.index[2, 0] >= 0)
    rel = ((a.depth[2, 0][keep] - gt[keep]).abs() / gt[keep]).median()
    print(f"fused cloud, discs of one voxel: median relative error in frame 2 {100 * float(rel):.4f} %")
    assert float(rel) < 1e-3


# ---- reconstruct_sequence ---------------------------------------------------------------------------------------------- #
def test_reconstruct_sequence_draws_surfels_when_asked():
    from coivo_amd import inference as I, nn as hnn, synth
    from oracle import colvo_spec as Sp
    dn_o, pn_o = Sp.make_models(31)
    dn, pn = hnn.DepthNet(), hnn.PoseNet()
    dn.load_state_dict(dn_o.state_dict())
    pn.load_state_dict(pn_o.state_dict())
    b = synth.make_batch(4, 64, 96, seed=31)
    frames, K = b["tgt"].to(dev()), b["K"].to(dev())
    plain = I.reconstruct_sequence(dn, pn, frames, K, stride=2, chunk=2, voxel_size=0.25, render=I.Render())
    assert plain.normals is None and isinstance(plain.rendered, I.RenderedViews) and len(plain) == 5
    assert I.reconstruct_sequence(dn, pn, frames, K, stride=2, chunk=2, voxel_size=0.25).normals is None
    rec = I.reconstruct_sequence(dn, pn, frames, K, stride=2, chunk=2, voxel_size=0.25, render=I.Render(surfels=True))
    assert torch.equal(rec.depths, plain.depths) and torch.equal(rec.fused.points, plain.fused.points) and len(rec) == 5
    assert isinstance(rec.normals, I.CloudNormals) and isinstance(rec.rendered, I.SurfelViews)
    Kn, traj32 = K.to(torch.float32).contiguous(), rec.cam2world.to(dev(), torch.float32)
    cn = I.cloud_normals(rec.fused, rec.depths, Kn, traj32, stride=2)
    assert torch.equal(_bits(cn.normals), _bits(rec.normals.normals)) and torch.equal(cn.stats, rec.normals.stats)
    assert int(cn.stats[3]) == 0 and int(cn.stats[2]) > 0                   # the same depths, stride and trajectory: every normal finds its row
    _same(rec.rendered, I.render_fused(rec.fused, Kn, traj32, 64, 96, normals=cn))
    assert rec.rendered.depth.shape == (4, 1, 64, 96) and rec.rendered.colors.shape == (4, 3, 64, 96) and rec.rendered.stats.shape == (4, 6)
    with pytest.raises(ValueError, match="voxel_size"):
        I.reconstruct_sequence(dn, pn, frames, K, render=I.Render(surfels=True))


# ---- refusals ---------------------------------------------------------------------------------------------------------- #
def test_argument_errors_on_the_device_path_launch_nothing():
    from coivo_amd import _lib, inference as I
    lib = _lib.load()
    pts, nrm, col, _, K, M = _tube(3, 17, 23)
    pts, nrm, col, K, M = _t(pts), _t(nrm), _t(col), _t(K), _t(M)
    m = pts.shape[0]
    scratch = torch.empty(int(lib.colvo_render_scratch_bytes(3, 17, 23)), device=dev(), dtype=torch.uint8)
    depth = torch.full((3, 1, 17, 23), 7.0, device=dev())
    index = torch.full((3, 1, 17, 23), 7, device=dev(), dtype=torch.int32)
    stats = torch.full((3, 6), 7, device=dev(), dtype=torch.int32)

    def call(M_=m, N=3, H=17, W=23, radius=0.02, max_splat=8, max_depth=MAX_DEPTH, normals=nrm.data_ptr(), colors=0, scr=scratch.data_ptr()):
        return lib.colvo_render_surfels(pts.data_ptr(), normals, colors, M_, K.data_ptr(), M.data_ptr(), N, H, W, radius, max_splat, max_depth,
                                        scr, depth.data_ptr(), index.data_ptr(), 0, 0, stats.data_ptr(), _lib.stream_ptr())

    for kw in (dict(M_=-1), dict(N=0), dict(N=65536), dict(H=0), dict(H=1 << 15, W=1 << 15), dict(max_splat=33), dict(max_splat=-1),
               dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(max_depth=0.0), dict(max_depth=float("inf")),
               dict(normals=0), dict(colors=col.data_ptr()), dict(scr=0), dict(scr=scratch.data_ptr() + 8)):
        assert call(**kw) != 0 and lib.colvo_last_error().startswith(b"colvo_render_surfels:"), (kw, lib.colvo_last_error())
    torch.cuda.synchronize()
    assert bool((depth == 7).all()) and bool((index == 7).all()) and bool((stats == 7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(stats, I.render_surfels(pts, nrm, K, M, 17, 23, radius=0.02, max_depth=MAX_DEPTH).stats)
    for bad in ((pts.cpu(), nrm, K, M), (pts, nrm.cpu(), K, M), (pts, nrm.double(), K, M), (pts, nrm[:-1], K, M), (pts, nrm, K[:2], M),
                (pts, nrm, K, M[:, :3, :])):
        with pytest.raises(ValueError):
            I.render_surfels(*bad, 17, 23, radius=0.02)
    with pytest.raises(ValueError):
        I.render_surfels(pts, nrm, K, M, 17, 23, radius=0.02, colors=col[:-1])
    out = I.render_surfels(pts[::2], nrm[::2], K, M, 17, 23, radius=0.02, colors=col[::2], max_depth=MAX_DEPTH)     # non-contiguous: taken as it reads
    assert out.depth.shape == (3, 1, 17, 23) and out.colors.shape == (3, 3, 17, 23) and out.normal is None


# ---- memory discipline ------------------------------------------------------------------------------------------------- #
def test_memory_discipline():
    """render_surfels under tests/guarded.py, 500 discs (a third with random normals, a seventh with none) in 37 views of 17 x 23 with
    per-frame intrinsics: points, normals, colours, intrinsics and poses between guard bands; the scratch (colvo_render_scratch_bytes),
    depth, index, colours, the normal planes and the statistics from the pool under both poisons.  Outputs equal the replica, are the
    same bytes under either poison, and no guard byte changes.  Launches reached: the clearing of the keys, the disc kernel (three frame
    groups, the last ragged; culled, flat and clipped points) and the resolve with colours and normals."""
    from coivo_amd import _lib, inference as I
    from tests import guarded as G
    H, W = 17, 23
    _, K, M = _cams(37, H, W, per_frame_K=True)
    pts, nrm = _frustum_points(500, 7, K, M, H, W)
    col = np.random.default_rng(3).random((500, 3), dtype=np.float32)
    kw = dict(radius=0.04, max_splat=8, max_depth=MAX_DEPTH)
    want = S.render(pts, nrm, K, M, H, W, colors=col, **kw)
    assert want["stats"][:, 1].min() > 0 and want["stats"][:, 4].max() > 0 and want["stats"][:, 5].max() > 0
    run = lambda pool: I.render_surfels(pool.place(_t(pts)), pool.place(_t(nrm)), pool.place(_t(K)), pool.place(_t(M)), H, W,
                                        colors=pool.place(_t(col)), want_normals=True, **kw)
    outs, pools = G.under_both_poisons(dev(), run, "render_surfels")
    for got, pool in zip(outs, pools):
        _assert_equal(got, want, "guarded")
        G.assert_served(pool, 0, _lib.load().colvo_render_scratch_bytes(37, H, W), "render_surfels")
