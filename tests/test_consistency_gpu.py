"""-m gpu: the multi-view depth consistency filter (coivo_amd.inference.filter_depths, csrc/consistency.hip) against its NumPy
replica (tests/consistency_ref.py).  The arithmetic is pinned (float32, one rounding per operation, float64 relative transforms
rounded once) and every sum is an integer, so every comparison here is equality to the bit: no tolerance."""
import functools

import numpy as np
import pytest
import torch

from tests import consistency_ref as R
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

MAX_DEPTH = 4.5
SEED = 3
REL_TOL = 0.002          # between the clean tube's interpolation error at 17x23 (3.6e-3) and at 64x96 (3.6e-4): all classes occur


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _filter(depths, K, M, **kw):
    from coivo_amd import inference as I
    return I.filter_depths(_t(depths), _t(K), _t(M), **kw)


def _assert_equal(got, want, what=""):
    """ConsistencyResult against the replica's dict: every tensor bit for bit."""
    d, v, s = (torch.from_numpy(want[k]) for k in ("depths", "votes", "stats"))
    assert got.depths.is_cuda and got.depths.dtype == torch.float32 and got.depths.shape == d.shape, what
    assert got.votes.dtype == torch.uint8 and got.votes.shape == v.shape and got.stats.dtype == torch.int32 and got.stats.shape == s.shape, what
    assert torch.equal(got.stats.cpu(), s), (what, got.stats.cpu(), s)
    assert torch.equal(got.votes.cpu(), v), (what, int((got.votes.cpu() != v).sum()))
    assert torch.equal(got.depths.cpu().view(torch.int32), d.view(torch.int32)), (what, int((got.depths.cpu().view(torch.int32) != d.view(torch.int32)).sum()))


def _same(a, b):
    assert torch.equal(a.depths.view(torch.int32), b.depths.view(torch.int32)) and torch.equal(a.votes, b.votes) and torch.equal(a.stats, b.stats)


@functools.lru_cache(maxsize=None)
def _scene(N, H, W):
    """The tube with the corrupted blocks in its middle frame."""
    d, K, M = R.tube_scene(N, H, W, SEED)
    return R.corrupt(d, N // 2), K, M


# smaller than a tile; ragged in both directions; several workgroups per frame; the sequence ends -- each at every window and step
# (window * step reaches past N in most of them: at (2,5,7) from window 2 or step 2 on, at (6,64,96) with 3 * 2); and N = 1
SHAPES = [(2, 5, 7), (3, 17, 23), (4, 33, 47), (6, 64, 96), (4, 130, 200)]
CASES = [(N, H, W, window, step) for (N, H, W) in SHAPES for window in (1, 2, 3) for step in (1, 2)] + [(1, 17, 23, 2, 1)]


# where the comparison is known not to be empty (kept pixels and every class in the replica's answer): everything from 33x47 on,
# and (3,17,23) at step 1 -- at step 2 its corrupted middle frame has no neighbour
def _all_classes(N, H, W, window, step):
    return H >= 33 or (N, H, W, step) == (3, 17, 23, 1)


@pytest.mark.parametrize("N,H,W,window,step", CASES)
def test_filter_equals_the_replica(N, H, W, window, step):
    d, K, M = _scene(N, H, W)
    kw = dict(window=window, step=step, rel_tol=REL_TOL, max_depth=MAX_DEPTH)
    want = R.filter_depths(d, K, M, **kw)
    _assert_equal(_filter(d, K, M, **kw), want, (N, H, W, window, step))
    if _all_classes(N, H, W, window, step):
        assert want["stats"][:, 1].sum() > 0 and all(want["votes"][:, k].any() for k in range(3))


def test_identical_frames_land_on_integer_pixels():
    """Two identical frames with identical (identity) poses, fx = fy = 16 and depths with few mantissa bits: every product and
    quotient is exact, so every sample lands on its own pixel with wx = wy = 0 -- at u = W - 1 and v = H - 1 on the clamped
    tap -- and agrees with rel = 0."""
    H, W = 9, 13
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.broadcast_to((1.0 + 0.5 * ((u + 2 * v) % 5)).astype(np.float32), (2, 1, H, W)).copy()
    K = np.broadcast_to(np.array([[16.0, 0, 6.0], [0, 16.0, 4.0], [0, 0, 1]], np.float32), (2, 3, 3)).copy()
    M = np.broadcast_to(np.eye(4, dtype=np.float32), (2, 4, 4)).copy()
    kw = dict(window=1, rel_tol=1e-6, max_depth=MAX_DEPTH)
    want = R.filter_depths(d, K, M, detail=True, **kw)
    assert (want["votes"][:, 0] == 1).all() and not want["votes"][:, 1:].any() and np.array_equal(want["depths"], d)
    assert np.array_equal(want["x0"][0, 1], u) and np.array_equal(want["y0"][0, 1], v) and np.nanmax(want["rel"]) == 0.0
    _assert_equal(_filter(d, K, M, **kw), want)


def test_intrinsics_that_differ_per_frame():
    N, H, W = 4, 33, 47
    rng = np.random.default_rng(11)
    K = np.zeros((N, 3, 3), np.float32)
    zoom = rng.uniform(0.9, 1.25, N)
    K[:, 0, 0] = 0.8 * W * zoom
    K[:, 1, 1] = 0.8 * W * zoom * rng.uniform(0.97, 1.03, N)
    K[:, 0, 2] = (W - 1) / 2 + rng.uniform(-4, 4, N)
    K[:, 1, 2] = (H - 1) / 2 + rng.uniform(-3, 3, N)
    K[:, 2, 2] = 1
    d, K, M = R.tube_scene(N, H, W, SEED, K=K)
    d = R.corrupt(d, 1)
    kw = dict(window=2, rel_tol=REL_TOL, max_depth=MAX_DEPTH)
    want = R.filter_depths(d, K, M, **kw)
    assert want["stats"][:, 1].min() > 0 and want["votes"][:, 0].max() >= 2
    _assert_equal(_filter(d, K, M, **kw), want)
    wrong = R.filter_depths(d, np.broadcast_to(K[0], K.shape), M, **kw)           # (the per-frame values matter)
    assert not np.array_equal(wrong["votes"], want["votes"])


def test_special_values_in_the_depth_maps():
    N, H, W = 4, 33, 47
    d, K, M = _scene(N, H, W)
    d = d.copy()
    rng = np.random.default_rng(5)
    specials = np.array([0.0, -0.0, -1.5, np.nan, np.inf, -np.inf, MAX_DEPTH, 2 * MAX_DEPTH, np.nextafter(np.float32(MAX_DEPTH), np.float32(0))],
                        np.float32)
    hit = rng.random(d.shape) < 0.08
    d[hit] = specials[rng.integers(0, len(specials), int(hit.sum()))]
    kw = dict(window=2, rel_tol=REL_TOL, max_depth=MAX_DEPTH)
    want = R.filter_depths(d, K, M, detail=True, **kw)
    bad = ~((d > 0) & (d < np.float32(MAX_DEPTH)))
    assert np.isinf(want["depths"][bad]).all() and (want["depths"][bad] > 0).all() and not want["votes"][np.repeat(bad, 3, 1)].any()
    assert (want["cls"] == R.INVISIBLE).sum() > 1000 and want["stats"][:, 1].min() > 0
    got = _filter(d, K, M, **kw)
    _assert_equal(got, want)
    assert not torch.isnan(got.depths).any() and not (got.depths <= 0).any()


@pytest.mark.parametrize("max_violated", [0, 1])
@pytest.mark.parametrize("min_agree", [0, 1, 4])
def test_policy_grid(min_agree, max_violated):
    d, K, M = _scene(6, 17, 23)
    kw = dict(window=2, rel_tol=REL_TOL, min_agree=min_agree, max_violated=max_violated, max_depth=MAX_DEPTH)
    want = R.filter_depths(d, K, M, **kw)
    _assert_equal(_filter(d, K, M, **kw), want, (min_agree, max_violated))
    assert want["stats"][:, 1].sum() > 0


def test_deterministic_across_calls_streams_and_counter_lines():
    from coivo_amd import _lib, inference as I
    args = [_t(x) for x in _scene(4, 130, 200)]
    kw = dict(window=2, rel_tol=REL_TOL, max_depth=MAX_DEPTH)
    a = I.filter_depths(*args, **kw)
    b = I.filter_depths(*args, **kw)
    _same(a, b)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        c = I.filter_depths(*args, **kw)
    side.synchronize()
    _same(a, c)
    saved = _lib.tune_get("consist_stat_lines")
    try:
        for lines in (1, 3, 8):
            _lib.tune_set("consist_stat_lines", lines)
            _same(a, I.filter_depths(*args, **kw))
    finally:
        _lib.tune_set("consist_stat_lines", saved)


def test_filtered_depths_feed_the_consumers_unchanged():
    """fuse_point_cloud, stitch_point_cloud and localize_polyps on ConsistencyResult.depths: +inf is dropped by all three, and
    the answers are those of the replicas on the replica's filtered depths."""
    from coivo_amd import inference as I, localize as Z
    from tests import fuse_ref, localize_ref
    N, H, W = 6, 64, 96
    d, K, M = _scene(N, H, W)
    kw = dict(window=2, rel_tol=REL_TOL, max_depth=MAX_DEPTH)
    want = R.filter_depths(d, K, M, **kw)
    got = _filter(d, K, M, **kw)
    _assert_equal(got, want)
    fd = want["depths"]
    kept = np.isfinite(fd)
    assert 0 < kept.sum() < ((d > 0) & (d < np.float32(MAX_DEPTH))).sum()
    Kt, Mt = _t(K), _t(M)
    # stitch: exactly the kept pixels, in order; nothing at a camera centre
    pts = I.stitch_point_cloud(got.depths, Kt, Mt, stride=1, max_depth=MAX_DEPTH)
    ref_pts = I.stitch_point_cloud(_t(fd), Kt, Mt, stride=1, max_depth=MAX_DEPTH)
    assert pts.shape == (int(kept.sum()), 3) and torch.equal(pts.view(torch.int32), ref_pts.view(torch.int32))
    raw_pts = I.stitch_point_cloud(_t(d), Kt, Mt, stride=1, max_depth=MAX_DEPTH)
    sel = torch.from_numpy(kept[(d < np.float32(MAX_DEPTH))]).to(dev())
    assert torch.equal(pts.view(torch.int32), raw_pts[sel].view(torch.int32))
    # fuse: its own replica on the replica's depths
    voxel = 0.125
    origin, dims = I.fusion_grid(Kt, Mt, H, W, voxel, MAX_DEPTH)
    fkw = dict(stride=1, max_depth=MAX_DEPTH, voxel_size=voxel, origin=origin, dims=dims)
    fused = I.fuse_point_cloud(got.depths, Kt, Mt, min_obs=1, **fkw)
    fw = fuse_ref.fuse(fd, None, K, M, min_obs=1, **fkw)
    assert (fused.n_input, fused.n_outside, fused.n_bricks, fused.n_voxels) == (int(kept.sum()), fw["n_outside"], fw["n_bricks"], fw["n_voxels"])
    assert torch.equal(fused.counts.cpu(), torch.from_numpy(fw["counts"])) and torch.equal(fused.voxels.cpu(), torch.from_numpy(fw["voxels"]))
    assert torch.equal(fused.points.cpu().view(torch.int32), torch.from_numpy(fw["points"]).view(torch.int32))
    # localize: its own replica on the replica's depths
    labels = np.zeros((N, 1, H, W), np.uint8)
    (a0, a1, b0, b1), _ = R.blocks(H, W)
    labels[:, :, a0 - 4:a1 + 4, b0 - 4:b1 + 4] = 1                              # around the floater: part of it is rejected
    labels[:, :, 40:60, 50:90] = 2
    pol = Z.localize_polyps(got.depths, _t(labels), Kt, Mt, num_labels=2, max_depth=MAX_DEPTH)
    lw = localize_ref.localize(fd, labels, K, M, num_labels=2, max_depth=MAX_DEPTH)
    assert (pol.n_labelled, pol.n_ignored) == (lw["n_labelled"], lw["n_ignored"])
    for k in ("n_pixels", "n_samples", "center_cam", "cov_cam", "center_world", "position", "cov_world", "n_samples_total"):
        g, w = getattr(pol, k).cpu().contiguous(), torch.from_numpy(np.ascontiguousarray(lw[k]))
        bits = (lambda t: t.view(torch.int64)) if g.dtype == torch.float64 else (lambda t: t)
        assert g.dtype == w.dtype and torch.equal(bits(g), bits(w)), k
    n_kept_lab = torch.from_numpy(np.stack([(kept[:, 0] & (labels[:, 0] == l)).reshape(N, -1).sum(1) for l in (1, 2)], 1))
    assert torch.equal(pol.n_samples.cpu().long(), n_kept_lab)


def test_reconstruct_sequence_filters_when_asked():
    from coivo_amd import inference as I, nn as hnn, synth
    from oracle import colvo_spec as S
    dn_o, pn_o = S.make_models(31)
    dn, pn = hnn.DepthNet(), hnn.PoseNet()
    dn.load_state_dict(dn_o.state_dict())
    pn.load_state_dict(pn_o.state_dict())
    b = synth.make_batch(5, 64, 96, seed=31)
    frames, K = b["tgt"].to(dev()), b["K"].to(dev())
    plain = I.reconstruct_sequence(dn, pn, frames, K, stride=2, chunk=2, voxel_size=0.25)      # as a caller from before would call it
    none = I.reconstruct_sequence(dn, pn, frames, K, stride=2, chunk=2, voxel_size=0.25, consistency=None)
    assert plain.consistency is None and none.consistency is None and len(plain) == 5
    assert torch.equal(plain.points, none.points) and torch.equal(plain.depths, none.depths)
    assert torch.equal(plain.fused.points, none.fused.points) and torch.equal(plain.fused.counts, none.fused.counts)
    policy = I.Consistency(window=2, rel_tol=0.01, min_agree=1)       # (on these seeded networks about a third of the pixels pass)
    rec = I.reconstruct_sequence(dn, pn, frames, K, stride=2, chunk=2, voxel_size=0.25, consistency=policy)
    depths, rel, traj, points, fused = rec                                                       # still five fields
    assert torch.equal(rec.depths, plain.depths) and torch.equal(rec.rel_poses, plain.rel_poses) and torch.equal(rec.cam2world, plain.cam2world)
    Kn, traj32 = K.to(torch.float32).contiguous(), rec.cam2world.to(dev(), torch.float32)
    want = I.filter_depths(rec.depths, Kn, traj32, **policy._asdict(), max_depth=I.MAX_DEPTH)
    _same(rec.consistency, want)
    ref = R.filter_depths(rec.depths.cpu().numpy(), Kn.cpu().numpy(), traj32.cpu().numpy(), **policy._asdict(), max_depth=I.MAX_DEPTH)
    _assert_equal(rec.consistency, ref)
    kept = int(want.stats[:, 1].sum())
    assert 0 < kept < int(want.stats[:, 0].sum())
    assert torch.equal(rec.points, I.stitch_point_cloud(want.depths, Kn, traj32, stride=2, max_depth=I.MAX_DEPTH))
    assert rec.points.shape[0] < plain.points.shape[0]
    f2 = I.fuse_point_cloud(want.depths, Kn, traj32, voxel_size=0.25, colors=frames.to(torch.float32).contiguous(), stride=2,
                            max_depth=I.MAX_DEPTH)
    assert torch.equal(rec.fused.points, f2.points) and torch.equal(rec.fused.counts, f2.counts) and rec.fused.n_input == rec.points.shape[0]
    with pytest.raises(ValueError):
        I.reconstruct_sequence(dn, pn, frames, K, consistency=I.Consistency(window=0))


def test_argument_errors_on_the_device():
    from coivo_amd import inference as I
    d, K, M = (_t(x) for x in _scene(3, 17, 23))
    for bad in ((d.cpu(), K, M), (d.double(), K, M), (d[:, 0], K, M), (d, K[:2], M), (d, K, M[:, :3, :]), (d, K.cpu(), M)):
        with pytest.raises(ValueError):
            I.filter_depths(*bad)
    for bad in (dict(window=0), dict(window=17), dict(step=0), dict(min_agree=5), dict(max_violated=-1), dict(rel_tol=0.0), dict(max_depth=float("inf"))):
        with pytest.raises(ValueError):
            I.filter_depths(d, K, M, **bad)
    out = I.filter_depths(d[:, :, ::2][:, :, :, ::2], K, M, max_depth=MAX_DEPTH)        # non-contiguous input: taken as it reads
    assert out.depths.shape == (3, 1, 9, 12)


@pytest.mark.parametrize("N,H,W,window,step", [(3, 17, 23, 2, 1), (4, 33, 47, 3, 2)])
def test_memory_discipline(N, H, W, window, step):
    """filter_depths under tests/guarded.py: depths, intrinsics and poses between guard bands -- the bilinear taps of a sample that lands
    on the first or last row of frame 0 or N - 1 border a guard --; the workspace (colvo_consistency_workspace_bytes), the filtered
    depths, the votes and the statistics from the pool under both poisons.  Outputs equal the replica, are the same bytes under either
    poison, and no guard byte changes.  Launches reached: the transform set-up and the filter kernel of colvo_consistency_filter, at
    a frame smaller than one tile row (17 x 23, window * step past the sequence's ends) and at one with several ragged tiles
    (33 x 47, step 2)."""
    from coivo_amd import _lib, inference as I
    from tests import guarded as G
    d, K, M = _scene(N, H, W)
    kw = dict(window=window, step=step, rel_tol=REL_TOL, max_depth=MAX_DEPTH)
    want = R.filter_depths(d, K, M, **kw)
    assert want["stats"][:, 1].sum() > 0
    outs, pools = G.under_both_poisons(dev(), lambda pool: I.filter_depths(pool.place(_t(d)), pool.place(_t(K)), pool.place(_t(M)), **kw),
                                       f"filter_depths {N}x{H}x{W}")
    for got, pool in zip(outs, pools):
        _assert_equal(got, want, (N, H, W, window, step))
        G.assert_served(pool, 0, _lib.load().colvo_consistency_workspace_bytes(N, window), "filter_depths")
