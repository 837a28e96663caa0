"""-m gpu: the voxel fusion (coivo_amd.inference.fuse_point_cloud, csrc/fuse.hip) against its NumPy replica (tests/fuse_ref.py).
The arithmetic that decides a sample's voxel is pinned (float32, one rounding per operation) and every sum is an integer, so
every comparison here is equality to the bit: no tolerance, no excused samples."""
import functools

import numpy as np
import pytest
import torch

from tests import fuse_ref as R
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

MAX_DEPTH = 4.5          # the synthetic depths span 0.5 .. 5: a tenth of the samples is dropped


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _fuse(depths, colors, K, M, **kw):
    from coivo_amd import inference as I
    return I.fuse_point_cloud(_t(depths), _t(K), _t(M), colors=None if colors is None else _t(colors), **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_equal(got, want, what=""):
    """FusedCloud against the replica's dict: every tensor bit for bit, every statistic."""
    for k in ("n_input", "n_outside", "n_bricks", "n_voxels"):
        assert getattr(got, k) == want[k], (what, k, getattr(got, k), want[k])
    m = want["points"].shape[0]
    assert got.points.shape == (m, 3) and got.points.dtype == torch.float32, (what, got.points.shape, m)
    assert got.counts.shape == (m,) and got.counts.dtype == torch.int32
    assert got.voxels.shape == (m, 3) and got.voxels.dtype == torch.int32
    assert torch.equal(got.counts.cpu(), torch.from_numpy(want["counts"])), what
    assert torch.equal(got.voxels.cpu(), torch.from_numpy(want["voxels"])), what
    assert torch.equal(_bits(got.points).cpu(), _bits(torch.from_numpy(want["points"]))), what
    if want["colors"] is None:
        assert got.colors is None, what
    else:
        assert got.colors.shape == (m, 3) and got.colors.dtype == torch.float32
        assert torch.equal(_bits(got.colors).cpu(), _bits(torch.from_numpy(want["colors"]))), what
    assert got.n_input - got.n_outside == int(want["sum_counts"]), what


def _same(a, b):
    """Two FusedClouds: identical bits."""
    assert a[4:] == b[4:]
    for x, y in zip(a[:4], b[:4]):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.shape == y.shape and torch.equal(_bits(x), _bits(y))


def _ref(depths, colors, K, M, **kw):
    want = R.fuse(depths, colors, K, M, **kw)
    want["sum_counts"] = R.fuse(depths, None, K, M, **dict(kw, min_obs=1))["counts"].astype(np.int64).sum()
    return want


@functools.lru_cache(maxsize=2)
def _scene(N, H, W):
    return R.scene(N, H, W, 5)


def _default_grid(K, M, H, W, voxel):
    from coivo_amd import inference as I
    return I.fusion_grid(torch.from_numpy(K), torch.from_numpy(M), H, W, voxel, MAX_DEPTH)


CASES = [(3, 17, 23, 1, 0.25), (4, 64, 96, 2, 0.125), (8, 256, 320, 1, 0.05), (8, 256, 320, 1, 0.02), (8, 256, 320, 4, 0.05),
         (2, 5, 7, 9, 0.5)]


@pytest.mark.parametrize("min_obs", [1, 2, 5])
@pytest.mark.parametrize("with_colors", [True, False])
@pytest.mark.parametrize("N,H,W,stride,voxel", CASES)
def test_fused_cloud_equals_the_replica(N, H, W, stride, voxel, with_colors, min_obs):
    depths, colors, K, M = _scene(N, H, W)
    origin, dims = _default_grid(K, M, H, W, voxel)
    col = colors if with_colors else None
    want = _ref(depths, col, K, M, stride=stride, max_depth=MAX_DEPTH, voxel_size=voxel, origin=origin, dims=dims, min_obs=min_obs)
    got = _fuse(depths, col, K, M, voxel_size=voxel, stride=stride, max_depth=MAX_DEPTH, min_obs=min_obs)   # the default grid
    assert got.origin == tuple(origin) and got.dims == tuple(dims)
    assert want["n_outside"] == 0 and want["n_input"] > 0
    _assert_equal(got, want, (N, H, W, stride, voxel, with_colors, min_obs))


def test_user_grid_tighter_than_the_scene():
    depths, colors, K, M = _scene(4, 64, 96)
    kw = dict(stride=1, max_depth=MAX_DEPTH, voxel_size=0.125, origin=(-1.0, -0.5, 1.0), dims=(16, 8, 24), min_obs=1)
    want = _ref(depths, colors, K, M, **kw)
    assert 0 < want["n_outside"] < want["n_input"]
    _assert_equal(_fuse(depths, colors, K, M, **kw), want)


def test_samples_exactly_on_the_faces_of_the_grid():
    """Identity pose, fx = fy = 64, cx = cy = 0: X = u / 64 * d, Z = d, every quantity exact.  Grid z from 1 to 2 in 8 voxels:
    depth 1 sits on the lower face (inside, voxel 0, quantum 0), depth 2 on the upper face (outside), x = 0.125 = origin on
    the lower x face."""
    H = W = 16
    depths = np.full((1, 1, H, W), 1.5, np.float32)
    depths[0, 0, 0::3] = 1.0
    depths[0, 0, 1::3] = 2.0
    K = np.array([[[64.0, 0, 0], [0, 64.0, 0], [0, 0, 1]]], np.float32)
    M = np.eye(4, dtype=np.float32)[None].copy()
    kw = dict(stride=1, max_depth=10.0, voxel_size=0.125, origin=(0.125, 0.0, 1.0), dims=(8, 8, 8), min_obs=1)
    want = _ref(depths, None, K, M, **kw)
    # rows at depth 2 (5 of 16) are outside; so are the samples left of x = 0.125: u < 8 at depth 1, u < 6 (u / 64 * 1.5) at depth 1.5
    assert want["n_input"] == 256 and want["n_outside"] == 5 * 16 + 6 * 8 + 5 * 6
    got = _fuse(depths, None, K, M, **kw)
    _assert_equal(got, want)
    assert int(got.voxels[:, 2].min()) == 0 and int(got.voxels[:, 0].min()) == 0


def test_special_values_in_depths_and_colours():
    depths, colors, K, M = (a.copy() for a in _scene(4, 64, 96))
    d, c = depths.reshape(-1), colors.reshape(-1)
    for i, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, MAX_DEPTH, np.nextafter(np.float32(MAX_DEPTH), np.float32(0)))):
        d[i * 7::997] = v
    for i, v in enumerate((np.nan, np.inf, -np.inf, -0.5, 1.5, 255.0, 0.5 / 255.0, 1.5 / 255.0, 2.5 / 255.0)):
        c[i * 5::991] = v
    origin, dims = _default_grid(K, M, 64, 96, 0.125)
    kw = dict(stride=1, max_depth=MAX_DEPTH, voxel_size=0.125, origin=origin, dims=dims, min_obs=1)
    want = _ref(depths, colors, K, M, **kw)
    assert want["n_input"] < depths.size - 6 * (depths.size // 997)
    _assert_equal(_fuse(depths, colors, K, M, **kw), want)


def test_nothing_kept_gives_empty_outputs():
    depths, colors, K, M = _scene(3, 17, 23)
    got = _fuse(np.full_like(depths, 20.0), colors, K, M, voxel_size=0.25, max_depth=MAX_DEPTH)
    assert (got.n_input, got.n_outside, got.n_bricks, got.n_voxels) == (0, 0, 0, 0)
    assert got.points.shape == (0, 3) and got.points.dtype == torch.float32 and got.points.is_cuda
    assert got.colors.shape == (0, 3) and got.colors.dtype == torch.float32
    assert got.counts.shape == (0,) and got.counts.dtype == torch.int32
    assert got.voxels.shape == (0, 3) and got.voxels.dtype == torch.int32
    assert _fuse(np.full_like(depths, 20.0), None, K, M, voxel_size=0.25, max_depth=MAX_DEPTH).colors is None
    # kept, but all outside the grid
    out = _fuse(depths, colors, K, M, voxel_size=0.25, max_depth=MAX_DEPTH, origin=(50.0, 50.0, 50.0), dims=(8, 8, 8))
    assert out.n_input > 0 and out.n_outside == out.n_input and out.n_bricks == 0 and out.points.shape == (0, 3)
    # min_obs above every count
    none = _fuse(depths, colors, K, M, voxel_size=0.25, max_depth=MAX_DEPTH, min_obs=10 ** 6)
    assert none.n_voxels > 0 and none.points.shape == (0, 3) and none.colors.shape == (0, 3)


def test_one_voxel_fed_by_everything():
    """64 identical frames of constant depth seen through a narrow K into a coarse voxel: every lane of every wave agrees."""
    N, H, W = 64, 16, 16
    depths = np.full((N, 1, H, W), 1.0, np.float32)
    colors = np.broadcast_to(_scene(3, 17, 23)[1][:1, :, :H, :W], (N, 3, H, W)).copy()
    K = np.broadcast_to(np.array([[1e4, 0, -1.0], [0, 1e4, -1.0], [0, 0, 1]], np.float32), (N, 3, 3)).copy()
    M = np.broadcast_to(np.eye(4, dtype=np.float32), (N, 4, 4)).copy()
    kw = dict(stride=1, max_depth=10.0, voxel_size=1.0, origin=(-4.0, -4.0, -4.0), dims=(8, 8, 8), min_obs=1)
    want = _ref(depths, colors, K, M, **kw)
    assert want["n_voxels"] == 1 and want["max_count"] == N * H * W
    _assert_equal(_fuse(depths, colors, K, M, **kw), want)


def test_no_two_samples_share_a_voxel():
    """A voxel far smaller than a pixel's footprint: no two lanes agree, every sample adds on its own."""
    depths, colors, K, M = _scene(3, 17, 23)
    _, g = R.grid_coords(depths, K, M, 1, (0.0, 0.0, 0.0), 1.0)
    centre = [float(np.median(x)) for x in g]
    kw = dict(stride=1, max_depth=MAX_DEPTH, voxel_size=0.002, origin=tuple(c - 1.024 for c in centre), dims=(1024, 1024, 1024),
              min_obs=1)
    want = _ref(depths, colors, K, M, **kw)
    assert want["max_count"] == 1 and want["n_voxels"] >= 20 and want["n_outside"] > 0
    _assert_equal(_fuse(depths, colors, K, M, **kw), want)


def test_brick_table_of_more_than_256_chunks():
    """1024^3 voxels are 128^3 = 2 097 152 bricks: 512 chunks of 4096 table entries, so every thread of the scan's one top-level
    workgroup takes two chunk sums (no other case here has more than 256 chunks, where it takes at most one).  The marked bricks lie
    in chunks on both sides of entry 256 of the sums."""
    depths, colors, K, M = _scene(3, 17, 23)
    kw = dict(stride=1, max_depth=MAX_DEPTH, voxel_size=0.0078125, origin=(-4.0, -4.0, -1.0), dims=(1024, 1024, 1024), min_obs=1)
    want = _ref(depths, colors, K, M, **kw)
    assert (want["n_input"], want["n_outside"], want["n_bricks"], want["n_voxels"]) == (1076, 0, 1066, 1076)
    b = want["voxels"] >> 3
    chunks = np.unique(((b[:, 2] * 128 + b[:, 1]) * 128 + b[:, 0]) // 4096)
    assert len(chunks) == 131 and chunks.min() == 90 and chunks.max() == 358
    _assert_equal(_fuse(depths, colors, K, M, **kw), want)


@pytest.mark.parametrize("with_colors", [True, False])
@pytest.mark.parametrize("rounds,row_adds", [(0, 0), (0, 1), (1, 1), (8, 0), (32, 1), (32, 0)])
def test_result_does_not_depend_on_how_the_adds_are_issued(rounds, row_adds, with_colors):
    """The developer switches tools/bench_fuse.py compares: lanes matched on the voxel (0, 1, 32 distinct voxels per wave), a
    record's words added by one lane or by four adjacent ones."""
    from coivo_amd import _lib
    depths, colors, K, M = _scene(4, 64, 96)
    col = colors if with_colors else None
    origin, dims = _default_grid(K, M, 64, 96, 0.125)
    kw = dict(stride=1, max_depth=MAX_DEPTH, voxel_size=0.125, origin=origin, dims=dims, min_obs=1)
    want = _ref(depths, col, K, M, **kw)
    saved = _lib.tune_get("fuse_agg_rounds"), _lib.tune_get("fuse_row_adds")
    try:
        _lib.tune_set("fuse_agg_rounds", rounds)
        _lib.tune_set("fuse_row_adds", row_adds)
        got = _fuse(depths, col, K, M, **kw)
    finally:
        _lib.tune_set("fuse_agg_rounds", saved[0])
        _lib.tune_set("fuse_row_adds", saved[1])
    _assert_equal(got, want)


def test_overflow_flag_raises():
    """The limit is 2^24 samples per voxel; the tuning table lets a test lower it instead of feeding 16 million samples."""
    from coivo_amd import _lib
    depths, colors, K, M = _scene(3, 17, 23)
    origin, dims = _default_grid(K, M, 17, 23, 0.25)
    kw = dict(stride=1, max_depth=MAX_DEPTH, voxel_size=0.25, origin=origin, dims=dims)
    top = R.fuse(depths, None, K, M, **kw)["max_count"]
    assert top >= 3
    saved = _lib.tune_get("fuse_count_limit")
    assert saved == 2 ** 24
    try:
        _lib.tune_set("fuse_count_limit", top)
        with pytest.raises(RuntimeError, match="overflow"):
            _fuse(depths, colors, K, M, **kw)
        _lib.tune_set("fuse_count_limit", top + 1)
        _fuse(depths, colors, K, M, **kw)
    finally:
        _lib.tune_set("fuse_count_limit", saved)


def test_deterministic_across_calls_streams_and_frame_order():
    depths, colors, K, M = _scene(8, 256, 320)
    kw = dict(voxel_size=0.05, stride=1, max_depth=MAX_DEPTH, min_obs=2)
    origin, dims = _default_grid(K, M, 256, 320, 0.05)
    a = _fuse(depths, colors, K, M, **kw)
    b = _fuse(depths, colors, K, M, **kw)
    _same(a, b)
    side = torch.cuda.Stream()
    args = [_t(x) for x in (depths, colors, K, M)]
    torch.cuda.synchronize()
    from coivo_amd import inference as I
    with torch.cuda.stream(side):
        c = I.fuse_point_cloud(args[0], args[2], args[3], colors=args[1], **kw)
    side.synchronize()
    _same(a, c)
    perm = np.random.default_rng(3).permutation(depths.shape[0])
    assert not np.array_equal(perm, np.arange(len(perm)))
    d = _fuse(depths[perm], colors[perm], K[perm], M[perm], origin=origin, dims=dims, **kw)
    _same(a, d)


def test_reconstruct_sequence_also_fuses():
    from coivo_amd import inference as I, nn as hnn, synth
    from oracle import colvo_spec as S
    dn_o, pn_o = S.make_models(31)
    dn, pn = hnn.DepthNet(), hnn.PoseNet()
    dn.load_state_dict(dn_o.state_dict())
    pn.load_state_dict(pn_o.state_dict())
    b = synth.make_batch(5, 64, 96, seed=31)
    frames, K = b["tgt"].to(dev()), b["K"].to(dev())
    plain = I.reconstruct_sequence(dn, pn, frames, K, stride=2, chunk=2)
    assert plain.fused is None
    rec = I.reconstruct_sequence(dn, pn, frames, K, stride=2, chunk=2, voxel_size=0.1, min_obs=2)
    assert torch.equal(rec.depths, plain.depths) and torch.equal(rec.rel_poses, plain.rel_poses)
    assert torch.equal(rec.cam2world, plain.cam2world) and torch.equal(_bits(rec.points), _bits(plain.points))
    want = I.fuse_point_cloud(rec.depths, K, rec.cam2world.to(dev(), torch.float32), voxel_size=0.1, colors=frames, stride=2,
                              min_obs=2)
    assert rec.fused.n_voxels > 0 and rec.fused.points.shape[0] > 0
    _same(rec.fused, want)
    # ... and that cloud is the replica's
    ref = _ref(rec.depths.cpu().numpy(), frames.cpu().numpy(), K.cpu().numpy(), rec.cam2world.float().numpy(), stride=2,
               max_depth=I.MAX_DEPTH, voxel_size=0.1, origin=rec.fused.origin, dims=rec.fused.dims, min_obs=2)
    _assert_equal(rec.fused, ref)


def test_argument_errors():
    from coivo_amd import inference as I
    depths, colors, K, M = _scene(3, 17, 23)
    d, c, k, m = (_t(x) for x in (depths, colors, K, M))
    with pytest.raises(ValueError):
        I.fuse_point_cloud(torch.from_numpy(depths), k, m, voxel_size=0.25)          # CPU tensor: no fallback
    with pytest.raises(ValueError):
        I.fuse_point_cloud(d, k, m, voxel_size=0.25, colors=torch.from_numpy(colors))
    with pytest.raises(ValueError):
        I.fuse_point_cloud(d, k[:1], m, voxel_size=0.25)
    with pytest.raises(ValueError):
        I.fuse_point_cloud(d, k, m, voxel_size=0.25, colors=c[:, :1])
    for bad in (dict(voxel_size=0.0), dict(voxel_size=float("nan")), dict(voxel_size=0.25, stride=0), dict(voxel_size=0.25, min_obs=0),
                dict(voxel_size=0.25, origin=(0.0, 0.0, 0.0)), dict(voxel_size=0.25, origin=(0.0, 0.0, 0.0), dims=(8, 8, 12)),
                dict(voxel_size=0.25, origin=(0.0, 0.0, 0.0), dims=(8, 8, 0))):
        with pytest.raises(ValueError):
            I.fuse_point_cloud(d, k, m, **bad)


@pytest.mark.parametrize("case", ["3x17x23_colours_min_obs_2", "more_than_256_scan_chunks"])
def test_memory_discipline(case):
    """fuse_point_cloud under tests/guarded.py: depths, colours, intrinsics and poses between guard bands; the plan's workspace
    (colvo_fuse_plan_workspace_bytes), the voxel pool (colvo_fuse_pool_bytes), the extraction workspace
    (colvo_fuse_extract_workspace_bytes) and every output from the pool under both poisons.  The cloud equals the replica, is the same
    bytes under either poison, and no guard byte changes.  Launches reached: colvo_fuse_plan, colvo_fuse_accumulate, colvo_fuse_count
    and colvo_fuse_write, with colours and min_obs = 2 in the first case; the second case's 1024^3 grid is a brick table of 512 scan
    chunks, where the scan's top-level workgroup takes two chunk sums per thread."""
    from coivo_amd import _lib, inference as I
    from tests import guarded as G
    lib = _lib.load()
    depths, colors, K, M = _scene(3, 17, 23)
    if case == "3x17x23_colours_min_obs_2":
        origin, dims = _default_grid(K, M, 17, 23, 0.25)
        kw = dict(stride=1, max_depth=MAX_DEPTH, voxel_size=0.25, origin=origin, dims=dims, min_obs=2)
    else:
        kw = dict(stride=1, max_depth=MAX_DEPTH, voxel_size=0.0078125, origin=(-4.0, -4.0, -1.0), dims=(1024, 1024, 1024), min_obs=1)
    want = _ref(depths, colors, K, M, **kw)
    assert want["n_bricks"] > 0 and 0 < want["points"].shape[0] and (kw["min_obs"] == 1 or want["points"].shape[0] < want["n_voxels"])
    outs, pools = G.under_both_poisons(dev(), lambda pool: I.fuse_point_cloud(pool.place(_t(depths)), pool.place(_t(K)), pool.place(_t(M)),
                                                                              colors=pool.place(_t(colors)), **kw), case)
    for got, pool in zip(outs, pools):
        _assert_equal(got, want, case)
        for nbytes in (lib.colvo_fuse_plan_workspace_bytes(3, 17, 23, 1, *kw["dims"]), lib.colvo_fuse_pool_bytes(want["n_bricks"]),
                       lib.colvo_fuse_extract_workspace_bytes(want["n_bricks"])):
            G.assert_served(pool, 0, nbytes, case)
