"""CPU checks of the cloud renderer (coivo_amd.inference.render_cloud, csrc/render.hip): the NumPy replica the GPU tests compare
with (tests/render_ref.py) against hand-computed scenes, against an identity round trip and against the same contract evaluated in
float64; the C ABI's refusals before any HIP call; the size query; the Python wrappers' argument errors."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import render_ref as R

MAX_DEPTH = 4.5
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.build()
    return _lib.load()


# ---- hand-computed scenes ---------------------------------------------------------------------------------------------- #
# 7 x 7 pixels, fx = fy = 8, principal point (3, 3), identity camera: a point (X, Y, Z) lands at x = 8 X / Z + 3, and with radius
# 0.25 its half-width is 2 / Z pixels -- every value below is exact in float32.
_K = np.array([[[8, 0, 3], [0, 8, 3], [0, 0, 1]]], np.float32)
_M = np.eye(4, dtype=np.float32)[None]


def _hand(points, radius, **kw):
    return R.render(np.array(points, np.float32), _K, _M, 7, 7, radius=radius, max_depth=10.0, **kw)


def test_hand_scene_one_pixel():
    r = _hand([[0, 0, 2]], 0.0)
    want_d = np.full((7, 7), INF)
    want_d[3, 3] = 2
    want_i = np.full((7, 7), -1, np.int32)
    want_i[3, 3] = 0
    assert np.array_equal(r["depth"][0, 0], want_d) and np.array_equal(r["index"][0, 0], want_i)
    assert r["stats"].tolist() == [[1, 1, 0, 1]] and r["colors"] is None
    assert r["depth"].dtype == np.float32 and r["index"].dtype == np.int32 and r["stats"].dtype == np.int32
    # a centre between pixels, radius 0: the nearest pixel (x = 3.25 -> 3, y = 3.5 -> floor(4.0) = 4)
    r = _hand([[0.0625, 0.125, 2]], 0.0)
    assert np.argwhere(r["index"][0, 0] == 0).tolist() == [[4, 3]]


def test_hand_scene_three_by_three_footprint_with_colours():
    r = _hand([[0, 0, 2]], 0.25, colors=np.array([[0.25, 0.5, 0.75]], np.float32))       # hx = hy = 1
    want_d = np.full((7, 7), INF)
    want_d[2:5, 2:5] = 2
    assert np.array_equal(r["depth"][0, 0], want_d) and np.array_equal(r["index"][0, 0] == 0, want_d == 2)
    assert r["stats"].tolist() == [[1, 1, 0, 9]]
    for k, c in enumerate((0.25, 0.5, 0.75)):
        assert np.array_equal(r["colors"][0, k], np.where(want_d == 2, np.float32(c), np.float32(0)))
    # the same point with max_splat 0: clipped to its one pixel
    r = _hand([[0, 0, 2]], 0.25, max_splat=0)
    assert r["stats"].tolist() == [[1, 1, 1, 1]] and r["index"][0, 0, 3, 3] == 0


def test_hand_scene_nearer_point_hides_farther():
    # 0: far, x = 3, half-width 0.5 -> the pixel (3, 3);  1: near, x = 4, half-width 1 -> u 3..5, v 2..4;  2: far, x = 1 -> (1, 3)
    r = _hand([[0, 0, 4], [0.25, 0, 2], [-1, 0, 4]], 0.25)
    want_i = np.full((7, 7), -1, np.int32)
    want_i[2:5, 3:6] = 1
    want_i[3, 1] = 2
    assert np.array_equal(r["index"][0, 0], want_i)
    assert np.array_equal(r["depth"][0, 0], np.where(want_i == 1, np.float32(2), np.where(want_i == 2, np.float32(4), INF)))
    assert r["stats"].tolist() == [[3, 3, 0, 10]]
    # listed the other way round the answer is the same surface: order decides nothing but ties
    r2 = _hand([[0.25, 0, 2], [0, 0, 4], [-1, 0, 4]], 0.25)
    assert np.array_equal(r2["depth"], r["depth"])


def test_hand_scene_equal_depths_go_to_the_smaller_index():
    r = _hand([[0.25, 0, 2], [0, 0, 2]], 0.25)               # 0 covers u 3..5, 1 covers u 2..4, both v 2..4, both at depth 2
    want_i = np.full((7, 7), -1, np.int32)
    want_i[2:5, 2] = 1
    want_i[2:5, 3:6] = 0
    assert np.array_equal(r["index"][0, 0], want_i)
    r = _hand([[0, 0, 2], [0, 0, 2]], 0.25)
    assert set(np.unique(r["index"])) == {-1, 0} and r["stats"].tolist() == [[2, 2, 0, 9]]


def test_points_that_are_not_in_front_or_not_on_screen():
    nf = np.nextafter
    pts = [[0, 0, 1e-3], [0, 0, nf(np.float32(1e-3), np.float32(1))], [0, 0, 10.0], [0, 0, nf(np.float32(10), np.float32(0))],
           [0, 0, -2], [np.nan, 0, 2], [0, np.inf, 2], [1e30, 0, 2], [0, 0, np.nan], [0, 0, np.inf]]
    p = R.project(np.array(pts, np.float32), _K, _M, 0, 7, 7, 0.0, 8, 10.0)
    assert p["front"].tolist() == [False, True, False, True, False, False, False, True, False, False]
    assert p["drawn"].tolist() == [False, True, False, True, False, False, False, False, False, False]
    r = _hand(pts, 0.0)
    assert r["stats"].tolist() == [[3, 2, 0, 1]] and r["index"][0, 0, 3, 3] == 1          # the nearer of the two that land


# ---- identity round trip ----------------------------------------------------------------------------------------------- #
def test_identity_round_trip_returns_the_depth_map_bit_for_bit():
    H, W = 17, 23
    rng = np.random.default_rng(2)
    d = rng.uniform(0.3, 4.0, (H, W)).astype(np.float32)
    fx, fy, cx, cy = (np.float32(v) for v in (18.4, 17.9, 11.0, 8.0))
    v, u = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    pts = np.stack([((u - cx) / fx) * d, ((v - cy) / fy) * d, d], -1).reshape(-1, 3)
    assert pts.dtype == np.float32
    K = np.array([[[fx, 0, cx], [0, fy, cy], [0, 0, 1]]], np.float32)
    r = R.render(pts, K, _M, H, W, radius=0.0, max_depth=10.0)
    assert np.array_equal(r["depth"][0, 0].view(np.int32), d.view(np.int32))
    assert np.array_equal(r["index"][0, 0], np.arange(H * W, dtype=np.int32).reshape(H, W))
    assert r["stats"].tolist() == [[H * W, H * W, 0, H * W]]


# ---- the replica against the same contract in float64 ------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def _tube(H, W):
    return R.tube_points(3, H, W, 5)


@pytest.mark.parametrize("radius,max_splat", [(0.02, 8), (0.05, 4)])
@pytest.mark.parametrize("H,W", [(17, 23), (64, 96)])
def test_replica_rectangles_agree_with_float64(H, W, radius, max_splat):
    """Every drawn point has the same pixel rectangle in float32 and in float64, unless one of the values a floor or a ceiling is
    taken of lies within 1e-3 pixel of an integer in float64; at most 3 % of the drawn points may be excused that way."""
    pts, _, K, M = _tube(H, W)
    a = R.project(pts, K, M, 1, H, W, radius, max_splat, MAX_DEPTH)
    b = R.project(pts, K, M, 1, H, W, radius, max_splat, MAX_DEPTH, dtype=np.float64)
    drawn = a["drawn"] | b["drawn"]
    same = a["drawn"] == b["drawn"]
    for k in ("u_lo", "u_hi", "v_lo", "v_hi"):
        same &= a[k] == b[k]

    def near(z):
        return np.abs(z - np.rint(z)) < 1e-3

    with np.errstate(all="ignore"):
        excused = near(b["x"] - b["hx"]) | near(b["x"] + b["hx"]) | near(b["y"] - b["hy"]) | near(b["y"] + b["hy"]) | \
            near(b["x"] + 0.5) | near(b["y"] + 0.5)
    n, n_exc, n_diff = int(drawn.sum()), int((drawn & excused).sum()), int((drawn & ~same).sum())
    print(f"{H}x{W} radius {radius} max_splat {max_splat}: {n} drawn, {n_exc} excused ({100.0 * n_exc / n:.2f} %), {n_diff} rectangles differ")
    assert n > 900
    assert not (drawn & ~same & ~excused).any()
    assert n_exc <= 0.03 * n


def test_replica_bookkeeping_on_the_tube():
    H, W = 64, 96
    pts, d, K, M = _tube(H, W)
    rng = np.random.default_rng(0)
    col = rng.random(pts.shape, dtype=np.float32)
    r = R.render(pts, K[1:2], M[1:2], H, W, radius=0.05, colors=col, max_splat=2, max_depth=MAX_DEPTH)
    front, drawn, clipped, covered = r["stats"][0].tolist()
    assert front >= drawn > 0 and 0 < clipped <= front and covered == int((r["index"] >= 0).sum())
    hit = r["index"][0, 0] >= 0
    assert np.array_equal(np.isfinite(r["depth"][0, 0]), hit) and (r["depth"][0, 0][~hit] == INF).all()
    assert np.array_equal(r["colors"][0][:, hit], col[r["index"][0, 0][hit]].T) and not r["colors"][0][:, ~hit].any()
    assert hit[d[1, 0] < np.float32(MAX_DEPTH)].all()                        # every pixel of the frame's own valid depth is covered


# ---- the C ABI --------------------------------------------------------------------------------------------------------- #
def test_scratch_size_query(lib):
    from coivo_amd import _lib
    f = lib.colvo_render_scratch_bytes
    assert lib.colvo_abi_version() == _lib.ABI_VERSION >= 20
    assert f(1, 1, 1) == 16 + 8 * 16 * 4                                      # one key padded to 16 bytes, eight counter lines
    assert f(3, 17, 23) == (3 * 17 * 23 * 8 + 15) // 16 * 16 + 3 * 8 * 16 * 4
    assert f(512, 256, 320) == 512 * 256 * 320 * 8 + 512 * 512
    assert f(65535, 1, 1) > 0 and f(1, 1, (1 << 30) - 1) > 0 and f(2, 1 << 15, (1 << 15) - 1) > 0
    for bad in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, -2), (1, 1 << 15, 1 << 15), (2, 1 << 15, 1 << 15),
                (4, 1 << 14, 1 << 15), (65535, 256, 320)):
        assert f(*bad) == 0, bad


def test_entry_point_refuses_bad_arguments_before_any_hip_call(lib):
    buf = (C.c_double * 66)()
    p = (C.addressof(buf) + 15) & ~15                                       # no call below gets past its checks to touch it
    base = dict(points=p, colors=p, M=4, K=p, cam=p, N=2, H=8, W=8, radius=0.02, max_splat=8, max_depth=10.0, scratch=p, out_d=p,
                out_i=p, out_c=p, out_s=p)
    order = ("points", "colors", "M", "K", "cam", "N", "H", "W", "radius", "max_splat", "max_depth", "scratch", "out_d", "out_i",
             "out_c", "out_s")

    def refused(what, **kw):
        a = dict(base)
        a.update(kw)
        assert lib.colvo_render_cloud(*(a[k] for k in order), None) != 0, kw
        msg = lib.colvo_last_error().decode()
        assert msg.startswith("colvo_render_cloud: ") and what in msg, (kw, msg)

    for k in ("points", "K", "cam", "scratch", "out_d", "out_i", "out_s"):
        refused("null pointer", **{k: None})
    refused("null pointer", colors=None)                                     # colours without their output, and the reverse
    refused("null pointer", out_c=None)
    refused("bad point count", M=-1)
    for s in (dict(max_splat=33), dict(max_splat=-1)):
        refused("bad max_splat", **s)
    for s in (dict(radius=-0.5), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius=-float("inf"))):
        refused("bad radius", **s)
    for s in (dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=float("nan")), dict(max_depth=float("inf"))):
        refused("bad max_depth", **s)
    for s in (dict(N=0), dict(N=65536), dict(N=-3), dict(H=0), dict(W=-3), dict(N=1, H=1 << 15, W=1 << 15),
              dict(N=2, H=1 << 15, W=1 << 15), dict(N=4, H=1 << 14, W=1 << 15)):
        refused("bad shape", **s)
    refused("16-byte aligned", scratch=p + 8)


def test_kernels_use_no_scratch_and_a_native_minimum(lib, tmp_path):
    """The resource metadata of the kernels (the splat kernel in both its forms): no private segment, no spilled register; the
    64-bit minimum is one instruction."""
    import re
    from coivo_amd import build
    asm = open(build.emit_asm("render.hip", str(tmp_path / "render.s"))).read()
    kernels = set(re.findall(r"\.name:\s+(\S*k_render_\w+)", asm))
    assert len(kernels) == 5 and all(any(f"k_render_{n}" in k for k in kernels) for n in ("clear", "splat", "resolve", "stats")), kernels
    for key in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count"):
        vals = re.findall(rf"\.{key}:\s+(\d+)", asm)
        assert len(vals) == 5 and all(int(v) == 0 for v in vals), (key, vals)
    assert "global_atomic_umin_x2" in asm and "cmpswap" not in asm


# ---- Python ------------------------------------------------------------------------------------------------------------ #
def test_render_cloud_argument_errors(lib):
    from coivo_amd import inference as I
    pts = torch.zeros(5, 3)
    K, M = torch.eye(3), torch.eye(4)[None]
    for bad in (dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius=None), dict(radius=1e39),
                dict(max_splat=33), dict(max_splat=-1), dict(max_splat=2.0), dict(max_splat=True), dict(max_depth=0.0),
                dict(max_depth=float("inf")), dict(max_depth=float("nan"))):
        kw = dict(radius=0.02)
        kw.update(bad)
        with pytest.raises(ValueError, match=next(iter(bad))):
            I.render_cloud(pts, K, M, 8, 8, **kw)
    with pytest.raises(TypeError):
        I.render_cloud(pts, K, M, 8, 8)                                      # radius has no default
    for H, W in ((0, 8), (8, -1), (8.0, 8), (1 << 15, 1 << 15)):
        with pytest.raises(ValueError):
            I.render_cloud(pts, K, M, H, W, radius=0.02)
    with pytest.raises(ValueError, match="limits"):
        I.render_cloud(pts, K, torch.eye(4).expand(4, 4, 4), 1 << 14, 1 << 15, radius=0.02)      # N*H*W = 2^31
    with pytest.raises(ValueError, match="limits"):
        I.render_cloud(pts, K, torch.zeros(0, 4, 4), 8, 8, radius=0.02)
    with pytest.raises(ValueError, match=r"\[M,3\]"):
        I.render_cloud(pts[:, :2], K, M, 8, 8, radius=0.02)
    with pytest.raises(ValueError, match=r"\[N,4,4\]"):
        I.render_cloud(pts, K, M[0], 8, 8, radius=0.02)
    # these tensors live on the CPU: refused the way the neighbouring functions refuse them
    with pytest.raises(ValueError, match="CUDA"):
        I.render_cloud(pts, K, M, 8, 8, radius=0.02)
    with pytest.raises(ValueError, match="CUDA"):
        I.render_cloud(pts, K[None], M, 8, 8, radius=0.02, colors=pts)
    fused = I.FusedCloud(pts, None, torch.zeros(5, dtype=torch.int32), torch.zeros(5, 3, dtype=torch.int32), (0.0, 0.0, 0.0), (8, 8, 8),
                         0.05, 5, 0, 1, 5)
    with pytest.raises(ValueError, match="CUDA"):
        I.render_fused(fused, K, M, 8, 8)
    with pytest.raises(ValueError, match="radius"):
        I.render_fused(fused, K, M, 8, 8, radius=-1.0)
    with pytest.raises(ValueError, match="FusedCloud"):
        I.render_fused(pts, K, M, 8, 8)


def test_reconstruct_sequence_render_needs_a_voxel_size():
    from coivo_amd import inference as I
    frames = torch.zeros(3, 3, 8, 8)
    with pytest.raises(ValueError, match="voxel_size"):
        I.reconstruct_sequence(None, None, frames, torch.eye(3), render=I.Render())
    with pytest.raises(ValueError, match="max_splat"):
        I.reconstruct_sequence(None, None, frames, torch.eye(3), voxel_size=0.05, render=I.Render(max_splat=40))
    with pytest.raises(ValueError, match="radius"):
        I.reconstruct_sequence(None, None, frames, torch.eye(3), voxel_size=0.05, render=I.Render(radius=-1.0))


def test_policy_and_result_types():
    import inspect
    from coivo_amd import inference as I
    assert I.Render() == (None, 8) and I.Render._fields == ("radius", "max_splat")
    assert I.RenderedViews._fields == ("depth", "index", "colors", "stats")
    r = I.Reconstruction(1, 2, 3, 4)
    assert len(r) == 5 and r.rendered is None and r.refinement is None
    r = I.Reconstruction(1, 2, 3, 4, 5, 6, 7, 8, 9)
    assert tuple(r) == (1, 2, 3, 4, 5) and (r.polyps, r.consistency, r.refinement, r.rendered) == (6, 7, 8, 9)
    r2 = r._replace(points=0)
    assert tuple(r2) == (1, 2, 3, 0, 5) and (r2.polyps, r2.consistency, r2.refinement, r2.rendered) == (6, 7, 8, 9)
    assert r._replace(rendered=None).rendered is None and r._replace(rendered=None).refinement == 8
    sig = inspect.signature(I.reconstruct_sequence).parameters
    assert sig["render"].default is None
    sig = inspect.signature(I.render_cloud).parameters
    assert sig["max_splat"].default == 8 and sig["max_depth"].default == I.MAX_DEPTH and sig["colors"].default is None
    assert inspect.signature(I.render_fused).parameters["radius"].default is None
