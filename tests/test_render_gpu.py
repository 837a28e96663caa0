"""-m gpu: the cloud renderer (coivo_amd.inference.render_cloud / render_fused, csrc/render.hip) against its NumPy replica
(tests/render_ref.py).  The arithmetic is pinned (float32, one rounding per operation), the minimum is taken on an integer key and
every sum is an integer, so every comparison here is equality to the bit: no tolerance, no excused pixel."""
import functools

import numpy as np
import pytest
import torch

from tests import render_ref as R
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

MAX_DEPTH = 4.5
SEED = 5
FRAME_GROUP = 16         # csrc/render.hip: frames a workgroup of the splat kernel walks


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _render(points, K, M, H, W, colors=None, **kw):
    from coivo_amd import inference as I
    return I.render_cloud(_t(points), _t(K), _t(M), H, W, colors=None if colors is None else _t(colors), **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_equal(got, want, what=""):
    """RenderedViews against the replica's dict: every tensor bit for bit."""
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


def _same(a, b):
    assert torch.equal(_bits(a.depth), _bits(b.depth)) and torch.equal(a.index, b.index) and torch.equal(a.stats, b.stats)
    assert (a.colors is None) == (b.colors is None) and (a.colors is None or torch.equal(_bits(a.colors), _bits(b.colors)))


def _check(points, K, M, H, W, colors=None, what="", **kw):
    want = R.render(points, K, M, H, W, colors=colors, **kw)
    _assert_equal(_render(points, K, M, H, W, colors=colors, **kw), want, what)
    return want


@functools.lru_cache(maxsize=None)
def _tube(N, H, W):
    """-> (points, colours, depths, K, cam2world) of the tube, every frame's samples."""
    pts, d, K, M = R.tube_points(N, H, W, SEED)
    col = np.random.default_rng(1).random(pts.shape, dtype=np.float32)
    return pts, col, d, K, M


def _frustum_points(m, seed, K, M, H, W):
    """m points spread over (and a little around) the views of the cameras given, depths on both sides of MAX_DEPTH."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, M.shape[0], m)
    z = rng.uniform(0.2, 1.2 * MAX_DEPTH, m)
    u, v = rng.uniform(-3, W + 2, m), rng.uniform(-3, H + 2, m)
    k, c = K[n].astype(np.float64), M[n].astype(np.float64)
    cam = np.stack([(u - k[:, 0, 2]) / k[:, 0, 0] * z, (v - k[:, 1, 2]) / k[:, 1, 1] * z, z], -1)
    return (np.einsum("nij,nj->ni", c[:, :3, :3], cam) + c[:, :3, 3]).astype(np.float32)


# ---- the tube ---------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("radius,max_splat", [(0.02, 8), (0.05, 4), (0.0, 8), (0.05, 2)])
@pytest.mark.parametrize("H,W", [(17, 23), (64, 96)])
def test_tube_equals_the_replica(H, W, radius, max_splat):
    pts, col, _, K, M = _tube(3, H, W)
    want = _check(pts, K[1:2], M[1:2], H, W, colors=col, radius=radius, max_splat=max_splat, max_depth=MAX_DEPTH, what=(H, W, radius, max_splat))
    front, drawn, clipped, covered = want["stats"][0].tolist()
    assert front > drawn > 0 and covered > 0
    if (radius, max_splat, H) == (0.05, 2, 64):
        # the clip path runs: at 64x96 (fx = 76.8) a wall point nearer than 1.92 has a half-width above 2 pixels.  (At 17x23,
        # fx = 18.4, no point of the wall is nearer than 0.46, so nothing can be clipped there.)
        assert clipped > 0


# ---- tails ------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("H,W", [(1, 1), (1, 70), (17, 23)])
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 257, 1000])
def test_tails(m, H, W):
    _, K, M = _cams(2, H, W)
    pts = _frustum_points(m, 100 + m, K, M, H, W)
    col = np.random.default_rng(m).random((m, 3), dtype=np.float32)
    want = _check(pts, K, M, H, W, colors=col, radius=0.03, max_splat=3, max_depth=MAX_DEPTH, what=(m, H, W))
    if m >= 63:
        assert want["stats"][:, 1].min() > 0 and (want["stats"][:, 0] < m).all()
    if m == 0:
        assert not want["stats"].any() and (want["index"] == -1).all()
    _check(pts, K, M, H, W, radius=0.03, max_splat=3, max_depth=MAX_DEPTH, what=(m, H, W, "no colours"))


def _cams(N, H, W, per_frame_K=False):
    """(depths, K, cam2world) of the tube's cameras; per_frame_K: intrinsics that differ from frame to frame."""
    from tests import consistency_ref as C
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
    return C.tube_scene(N, H, W, SEED, K=K)


# ---- frame groups ------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("N", [1, 3, 37])
def test_frame_groups_with_intrinsics_that_differ_per_frame(N):
    assert 37 > 2 * FRAME_GROUP and 37 % FRAME_GROUP
    H, W = 17, 23
    _, K, M = _cams(N, H, W, per_frame_K=True)
    pts = _frustum_points(500, 7, K, M, H, W)
    col = np.random.default_rng(3).random((500, 3), dtype=np.float32)
    want = _check(pts, K, M, H, W, colors=col, radius=0.04, max_splat=8, max_depth=MAX_DEPTH, what=N)
    assert want["stats"][:, 1].min() > 0                                      # every frame draws something
    if N > 1:
        wrong = R.render(pts, np.broadcast_to(K[0], K.shape), M, H, W, radius=0.04, max_splat=8, max_depth=MAX_DEPTH)
        assert not np.array_equal(wrong["index"], want["index"])              # (the per-frame values matter)
        one = _render(pts, K[0], M, H, W, radius=0.04, max_splat=8, max_depth=MAX_DEPTH)         # K [3,3] serves every frame
        _assert_equal(one, wrong)


# ---- borders, bounds, hostile values ------------------------------------------------------------------------------------ #
_K = np.array([[[8, 0, 3], [0, 8, 5], [0, 0, 1]]], np.float32)      # x = 8 X / Z + 3, y = 8 Y / Z + 5: exact at Z = 2
_I = np.eye(4, dtype=np.float32)[None]


def _at(x, y, z=2.0):
    """The point that lands at pixel coordinates (x, y) of the camera above, at depth z (exact for dyadic values)."""
    return [(x - 3) * z / 8, (y - 5) * z / 8, z]


def test_footprints_that_cross_every_edge_and_corner():
    H, W = 11, 7                                               # radius 0.5 at Z = 2: half-width 2 pixels
    xs, ys = (-1.0, 3.0, 7.0), (-1.5, 5.0, 11.5)              # left of / inside / right of the image; above / inside / below
    pts = np.array([_at(x, y) for y in ys for x in xs], np.float32)       # all at depth 2: where two overlap the smaller index wins
    want = _check(pts, _K, _I, H, W, radius=0.5, max_splat=8, max_depth=MAX_DEPTH)
    assert want["stats"].tolist()[0][:3] == [9, 9, 0]
    idx = want["index"][0, 0]
    assert idx[0, 0] == 0 and idx[0, W - 1] == 2 and idx[H - 1, 0] == 6 and idx[H - 1, W - 1] == 8 and idx[5, 3] == 4
    assert set(range(9)) <= set(np.unique(idx).tolist())                     # every one of the nine shows
    # two pixels further out nothing reaches the image any more
    far = np.array([_at(-3.0, 5.0), _at(10.0, 5.0), _at(3.0, -3.5), _at(3.0, 14.0)], np.float32)
    want = _check(far, _K, _I, H, W, radius=0.5, max_splat=8, max_depth=MAX_DEPTH)
    assert want["stats"].tolist() == [[4, 0, 0, 0]]


@pytest.mark.parametrize("max_splat", [0, 2, 8, 32])
def test_the_on_screen_bounds(max_splat):
    H, W = 11, 7
    f = np.float32
    lo, x_hi, y_hi = f(-(max_splat + 1)), f(W + max_splat), f(H + max_splat)
    xs = [lo, np.nextafter(lo, f(-1e9)), np.nextafter(lo, f(0)), x_hi, np.nextafter(x_hi, f(1e9)), np.nextafter(x_hi, f(0))]
    ys = [lo, np.nextafter(lo, f(-1e9)), np.nextafter(lo, f(0)), y_hi, np.nextafter(y_hi, f(1e9)), np.nextafter(y_hi, f(0))]
    K0 = np.array([[[8, 0, 0], [0, 8, 0], [0, 0, 1]]], np.float32)          # x = 8 X / 2 = 4 X: exact for every float32 x
    at = lambda x, y: [float(x) / 4, float(y) / 4, 2.0]
    pts = np.array([at(x, 5.0) for x in xs] + [at(3.0, y) for y in ys] + [at(xs[0], ys[3])], np.float32)
    p = R.project(pts, K0, _I, 0, H, W, 100.0, max_splat, MAX_DEPTH)
    assert np.array_equal(p["x"][:6], np.array(xs, f)) and np.array_equal(p["y"][6:12], np.array(ys, f))
    assert p["on"].tolist() == [True, False, True, True, False, True] * 2 + [True] and p["clipped"].all()
    _check(pts, K0, _I, H, W, radius=100.0, max_splat=max_splat, max_depth=MAX_DEPTH, what=max_splat)     # half-width max_splat exactly
    _check(pts, K0, _I, H, W, radius=0.0, max_splat=max_splat, max_depth=MAX_DEPTH, what=max_splat)


def test_hostile_values():
    H, W = 11, 7
    f = np.float32
    nan, inf = np.nan, np.inf
    eps, md = f(1e-3), f(MAX_DEPTH)
    pts = [[nan, 0, 2], [0, nan, 2], [0, 0, nan], [inf, 0, 2], [0, -inf, 2], [0, 0, inf], [0, 0, -inf], [inf, inf, inf],
           [1e30, 0, 2], [0, -1e30, 2], [0, 0, 1e30], [1e30, 1e30, 1e30], [-1e30, 0, 1e-2],
           [0, 0, -2], [0.25, 0.25, -0.5], [0, 0, 0], [0, 0, -0.0],
           [0, 0, eps], [0.25, 0, md], [0, 0, np.nextafter(eps, f(1))], [0.25, 0, np.nextafter(md, f(0))],
           _at(1.0, 2.0), _at(5.0, 9.0, 3.0)]
    pts = np.array(pts, np.float32)
    p = R.project(pts, _K, _I, 0, H, W, 0.25, 8, MAX_DEPTH)
    assert p["front"][17:21].tolist() == [False, False, True, True] and p["drawn"][17:21].tolist() == [False, False, True, True]
    assert not p["front"][:8].any() and not p["front"][13:17].any() and p["front"][8:10].all() and not p["drawn"][:17].any()
    col = np.random.default_rng(0).random(pts.shape, dtype=np.float32)
    for radius, ms in ((0.25, 8), (0.0, 8), (0.25, 0), (3e38, 32)):
        want = _check(pts, _K, _I, H, W, colors=col, radius=radius, max_splat=ms, max_depth=MAX_DEPTH, what=(radius, ms))
        assert want["stats"][0, 1] == 4
    # a camera whose own entries are hostile: the frame comes out empty, the one beside it is untouched
    K2, M2 = np.repeat(_K, 3, 0), np.repeat(_I, 3, 0)
    K2[0, 0, 0] = nan
    M2[2, 0, 3] = inf
    want = _check(pts, K2, M2, H, W, radius=0.25, max_splat=8, max_depth=MAX_DEPTH)
    assert want["stats"][:, 1].tolist() == [0, 4, 0] and (want["index"][[0, 2]] == -1).all()
    # a negative focal length makes the half-width negative: the nearest pixel is still drawn, nothing else
    K3 = _K.copy()
    K3[0, 0, 0] = -8
    want = _check(pts[-2:], K3, _I, H, W, radius=0.25, max_splat=8, max_depth=MAX_DEPTH)
    assert want["stats"][0, 1] == 2


def test_ties_go_to_the_smaller_index():
    H, W = 64, 96
    pts, col, _, K, M = _tube(3, H, W)
    m = pts.shape[0]
    twice = np.concatenate([pts, pts])
    want = _check(twice, K[1:2], M[1:2], H, W, colors=np.concatenate([col, 1 - col]), radius=0.02, max_splat=8, max_depth=MAX_DEPTH)
    once = R.render(pts, K[1:2], M[1:2], H, W, colors=col, radius=0.02, max_splat=8, max_depth=MAX_DEPTH)
    assert want["index"].max() < m and np.array_equal(want["index"], once["index"]) and np.array_equal(want["colors"], once["colors"])
    assert np.array_equal(want["stats"][:, :3], 2 * once["stats"][:, :3]) and np.array_equal(want["stats"][:, 3], once["stats"][:, 3])


# ---- through the existing API ------------------------------------------------------------------------------------------ #
def test_a_stitched_frame_renders_back_into_its_own_depth_map():
    from coivo_amd import inference as I
    H, W = 64, 96
    d, K, _ = _cams(2, H, W)
    d, K = _t(d[:1]), _t(K[:1])
    eye = torch.eye(4, device=dev())[None].contiguous()
    cloud = I.stitch_point_cloud(d, K, eye, stride=1, max_depth=MAX_DEPTH)
    r = I.render_cloud(cloud, K, eye, H, W, radius=0.0, max_depth=MAX_DEPTH)
    keep = d < MAX_DEPTH
    assert 0 < int(keep.sum()) == cloud.shape[0] < H * W
    assert torch.equal(_bits(r.depth)[keep], _bits(d)[keep]) and torch.isposinf(r.depth[~keep]).all()
    row = (torch.cumsum(keep.flatten().to(torch.int32), 0) - 1).to(torch.int32).view_as(r.index)
    assert torch.equal(r.index[keep], row[keep]) and (r.index[~keep] == -1).all()
    n = cloud.shape[0]
    assert r.stats.tolist() == [[n, n, 0, n]] and r.colors is None


# ---- determinism ------------------------------------------------------------------------------------------------------- #
def test_deterministic_across_calls_streams_and_splat_forms():
    from coivo_amd import _lib, inference as I
    H, W = 64, 96
    pts, col, _, K, M = _tube(3, H, W)
    args = (_t(pts), _t(K), _t(M), H, W)
    kw = dict(radius=0.03, colors=_t(col), max_splat=6, max_depth=MAX_DEPTH)
    a = I.render_cloud(*args, **kw)
    b = I.render_cloud(*args, **kw)
    _same(a, b)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        c = I.render_cloud(*args, **kw)
    side.synchronize()
    _same(a, c)
    saved = _lib.tune_get("render_load_first")
    try:
        for form in (1, 0):
            _lib.tune_set("render_load_first", form)
            _same(a, I.render_cloud(*args, **kw))
    finally:
        _lib.tune_set("render_load_first", saved)
    _assert_equal(a, R.render(pts, K, M, H, W, colors=col, radius=0.03, max_splat=6, max_depth=MAX_DEPTH))


# ---- consumers --------------------------------------------------------------------------------------------------------- #
def test_rendered_depth_feeds_the_consumers():
    from coivo_amd import evaluate as E, inference as I
    H, W = 64, 96
    pts, _, d, K, M = _tube(3, H, W)
    Kt, Mt = _t(K), _t(M)
    r = I.render_cloud(_t(pts), Kt, Mt, H, W, radius=0.02, max_depth=MAX_DEPTH)
    covered = r.index >= 0
    n_cov = int(covered.sum())
    assert 0 < n_cov < covered.numel() and torch.equal(r.stats[:, 3].sum().cpu(), torch.tensor(n_cov))
    m = E.depth_metrics(r.depth, _t(d), mask=covered, max_depth=MAX_DEPTH, median_scaling=False)
    assert int(m.n_valid.sum()) > 0.5 * n_cov and torch.isfinite(m.per_image).all()
    abs_rel = float(m.per_image[:, 0].max())
    print(f"rendered against ground truth, radius 0.02 at 64x96: abs_rel {m.per_image[:, 0].tolist()}")
    assert abs_rel < 0.1                                                     # the grazing-angle bias is a few per cent
    cloud = I.stitch_point_cloud(r.depth, Kt, Mt, stride=1, max_depth=MAX_DEPTH)
    assert cloud.shape[0] == n_cov                                           # +inf is dropped, nothing else
    fused = I.fuse_point_cloud(r.depth, Kt, Mt, voxel_size=0.125, max_depth=MAX_DEPTH)
    assert fused.n_input == n_cov
    filt = I.filter_depths(r.depth, Kt, Mt, max_depth=MAX_DEPTH)
    assert int(filt.stats[:, 0].sum()) == n_cov


# ---- reconstruct_sequence ---------------------------------------------------------------------------------------------- #
def test_reconstruct_sequence_renders_when_asked():
    from coivo_amd import inference as I, nn as hnn, synth
    from oracle import colvo_spec as S
    dn_o, pn_o = S.make_models(31)
    dn, pn = hnn.DepthNet(), hnn.PoseNet()
    dn.load_state_dict(dn_o.state_dict())
    pn.load_state_dict(pn_o.state_dict())
    b = synth.make_batch(4, 64, 96, seed=31)
    frames, K = b["tgt"].to(dev()), b["K"].to(dev())
    plain = I.reconstruct_sequence(dn, pn, frames, K, stride=2, chunk=2, voxel_size=0.25)
    assert plain.rendered is None and len(plain) == 5
    rec = I.reconstruct_sequence(dn, pn, frames, K, stride=2, chunk=2, voxel_size=0.25, render=I.Render())
    assert torch.equal(rec.depths, plain.depths) and torch.equal(rec.points, plain.points) and torch.equal(rec.fused.points, plain.fused.points)
    Kn, traj32 = K.to(torch.float32).contiguous(), rec.cam2world.to(dev(), torch.float32)
    want = I.render_fused(rec.fused, Kn, traj32, 64, 96)
    _same(rec.rendered, want)
    assert rec.rendered.depth.shape == (4, 1, 64, 96) and rec.rendered.colors.shape == (4, 3, 64, 96)
    assert int(rec.rendered.stats[:, 3].sum()) > 0
    ref = R.render(rec.fused.points.cpu().numpy(), Kn.cpu().numpy(), traj32.cpu().numpy(), 64, 96, colors=rec.fused.colors.cpu().numpy(),
                   radius=rec.fused.voxel_size, max_splat=8, max_depth=I.MAX_DEPTH)
    _assert_equal(rec.rendered, ref)
    small = I.reconstruct_sequence(dn, pn, frames, K, stride=2, chunk=2, voxel_size=0.25, render=I.Render(radius=0.05, max_splat=2))
    _same(small.rendered, I.render_fused(small.fused, Kn, traj32, 64, 96, radius=0.05, max_splat=2))
    assert not torch.equal(small.rendered.index, rec.rendered.index)
    with pytest.raises(ValueError, match="voxel_size"):
        I.reconstruct_sequence(dn, pn, frames, K, render=I.Render())


def test_argument_errors_on_the_device():
    from coivo_amd import inference as I
    pts, col, _, K, M = _tube(3, 17, 23)
    pts, col, K, M = _t(pts), _t(col), _t(K), _t(M)
    for bad in ((pts.cpu(), K, M), (pts.double(), K, M), (pts[:, :2], K, M), (pts, K[:2], M), (pts, K, M[:, :3, :]), (pts, K.cpu(), M)):
        with pytest.raises(ValueError):
            I.render_cloud(*bad, 17, 23, radius=0.02)
    with pytest.raises(ValueError):
        I.render_cloud(pts, K, M, 17, 23, radius=0.02, colors=col[:-1])
    for bad in (dict(radius=-1.0), dict(max_splat=33), dict(max_depth=float("inf"))):
        kw = dict(radius=0.02)
        kw.update(bad)
        with pytest.raises(ValueError):
            I.render_cloud(pts, K, M, 17, 23, **kw)
    out = I.render_cloud(pts[::2], K, M, 17, 23, radius=0.02, colors=col[::2], max_depth=MAX_DEPTH)      # non-contiguous input: taken as it reads
    assert out.depth.shape == (3, 1, 17, 23) and out.colors.shape == (3, 3, 17, 23)


# ---- memory discipline ------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", ["37_views_17x23", "tube_64x96_clipped"])
def test_memory_discipline(case):
    """render_cloud under tests/guarded.py: points, colours, intrinsics and poses between guard bands; the scratch
    (colvo_render_scratch_bytes: the 64-bit keys), depth, index, colours and statistics from the pool under both poisons.  Outputs
    equal the replica, are the same bytes under either poison, and no guard byte changes -- a square that hangs over the image's first or
    last row of view 0 or N - 1 would land in one.  Launches reached: the clearing of the keys, the splat kernel and the resolve; 37
    views are three frame groups, the last ragged, with per-frame intrinsics; the 64 x 96 tube at max_splat 2 runs the clip path."""
    from coivo_amd import _lib, inference as I
    from tests import guarded as G
    if case == "37_views_17x23":
        H, W = 17, 23
        _, K, M = _cams(37, H, W, per_frame_K=True)
        pts = _frustum_points(500, 7, K, M, H, W)
        col = np.random.default_rng(3).random((500, 3), dtype=np.float32)
        kw = dict(radius=0.04, max_splat=8, max_depth=MAX_DEPTH)
    else:
        H, W = 64, 96
        pts, col, _, K, M = _tube(3, H, W)
        K, M = K[1:2], M[1:2]
        kw = dict(radius=0.05, max_splat=2, max_depth=MAX_DEPTH)
    want = R.render(pts, K, M, H, W, colors=col, **kw)
    assert want["stats"][:, 1].min() > 0 and (case.startswith("37") or want["stats"][0, 2] > 0)
    run = lambda pool: I.render_cloud(pool.place(_t(pts)), pool.place(_t(K)), pool.place(_t(M)), H, W, colors=pool.place(_t(col)), **kw)
    outs, pools = G.under_both_poisons(dev(), run, case)
    for got, pool in zip(outs, pools):
        _assert_equal(got, want, case)
        G.assert_served(pool, 0, _lib.load().colvo_render_scratch_bytes(M.shape[0], H, W), case)
