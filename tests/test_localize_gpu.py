"""-m gpu: the polyp localisation (coivo_amd.localize.localize_polyps, csrc/localize.hip) against its NumPy replica
(tests/localize_ref.py).  The point arithmetic is pinned (float32, one rounding per operation), every sum is an integer and
every float64 output has its association written down, so every comparison here is equality to the bit: no tolerance."""
import functools

import numpy as np
import pytest
import torch

from tests import localize_ref as R
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

TENSORS = ("n_pixels", "n_samples", "bbox", "pixel", "center_cam", "cov_cam", "center_world", "n_frames", "n_samples_total",
           "first_frame", "last_frame", "position", "cov_world", "radius")
PER_OBSERVATION = TENSORS[:7]
DTYPES = dict(n_pixels=torch.int32, n_samples=torch.int32, bbox=torch.int32, n_frames=torch.int32, n_samples_total=torch.int64,
              first_frame=torch.int32, last_frame=torch.int32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _localize(depths, labels, K, M, **kw):
    from coivo_amd import localize as Z
    return Z.localize_polyps(_t(depths), _t(labels), _t(K), _t(M), **kw)


def _assert_equal(got, want, what=""):
    """PolypLocalization against the replica's dict: every tensor bit for bit, both statistics."""
    assert (got.n_labelled, got.n_ignored) == (want["n_labelled"], want["n_ignored"]), (what, got.n_labelled, got.n_ignored)
    for k in TENSORS:
        g, w = getattr(got, k), torch.from_numpy(np.ascontiguousarray(want[k]))
        assert g.is_cuda and g.dtype == DTYPES.get(k, torch.float64) and g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape)
        assert torch.equal(_bits(g).cpu(), _bits(w)), (what, k, g.cpu(), w)


def _same(a, b):
    assert a[-2:] == b[-2:]
    for k in TENSORS:
        assert torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k))), k


@functools.lru_cache(maxsize=None)
def _scene(key):
    N, H, W, stride, L = key
    seed, spheres = R.SCENES[key]
    return R.scene(N, H, W, seed, spheres)


@functools.lru_cache(maxsize=None)
def _want(key, clip, min_samples):
    N, H, W, stride, L = key
    d, lab, K, M = _scene(key)
    return R.localize(d, lab, K, M, num_labels=L, stride=stride, max_depth=R.MAX_DEPTH, clip_sigma=clip, min_samples=min_samples)


@pytest.mark.parametrize("min_samples", [1, 40])
@pytest.mark.parametrize("clip", [None, R.CLIP_SIGMA])
@pytest.mark.parametrize("key", list(R.SCENES))
def test_localization_equals_the_replica(key, clip, min_samples):
    N, H, W, stride, L = key
    d, lab, K, M = _scene(key)
    want = _want(key, clip, min_samples)
    assert want["n_labelled"] > 0
    got = _localize(d, lab, K, M, num_labels=L, stride=stride, max_depth=R.MAX_DEPTH, clip_sigma=clip, min_samples=min_samples)
    _assert_equal(got, want, (key, clip, min_samples))


def test_clip_scene_equals_the_replica():
    c = R.CLIP_SCENE
    d, lab, K, M = R.scene(c["N"], c["H"], c["W"], c["seed"], c["spheres"], wall=c["wall"], dilate=c["dilate"])
    for clip in (None, R.CLIP_SIGMA, 0.0):
        want = R.localize(d, lab, K, M, num_labels=1, max_depth=R.MAX_DEPTH, clip_sigma=clip)
        _assert_equal(_localize(d, lab, K, M, num_labels=1, max_depth=R.MAX_DEPTH, clip_sigma=clip), want, clip)


def test_largest_sums_the_guards_admit_at_this_size():
    """One label over every pixel of 256x320, depth just below max_depth = 10, fx = fy = 0.25 W: |q_x| up to 81 600, 81 920 samples a
    frame, sum q^2 about 2^48; 10 workgroups of 8192 pixels add into one record."""
    N, H, W = 2, 256, 320
    d = np.full((N, 1, H, W), np.nextafter(np.float32(10.0), np.float32(0)), np.float32)
    d[1] = np.float32(9.75)
    lab = np.ones((N, 1, H, W), np.uint8)
    K = np.broadcast_to(np.array([[0.25 * W, 0, (W - 1) / 2], [0, 0.25 * W, (H - 1) / 2], [0, 0, 1]], np.float32), (N, 3, 3)).copy()
    M = _scene((3, 17, 23, 1, 3))[3][:N]
    for clip in (None, 1.0):
        want = R.localize(d, lab, K, M, num_labels=1, max_depth=10.0, clip_sigma=clip)
        assert want["n_samples"].tolist() == [[H * W]] * N
        _assert_equal(_localize(d, lab, K, M, num_labels=1, max_depth=10.0, clip_sigma=clip), want, clip)


def test_every_lane_carries_a_different_label():
    """L = 255 and a seeded random label per pixel: the leader loop's worst case, and every record of the LDS table in use."""
    N, H, W = 2, 64, 96
    d, _, K, M = _scene((4, 64, 96, 2, 4))
    d, K, M = d[:N], K[:N], M[:N]
    lab = np.random.default_rng(11).integers(1, 256, size=(N, 1, H, W), dtype=np.uint8)
    for L in (255, 200):                                                        # 200: a fifth of the pixels is ignored
        for clip in (None, 1.0):
            want = R.localize(d, lab, K, M, num_labels=L, max_depth=R.MAX_DEPTH, clip_sigma=clip)
            assert (want["n_pixels"] > 0).all() and (want["n_ignored"] > 0) == (L < 255)
            _assert_equal(_localize(d, lab, K, M, num_labels=L, max_depth=R.MAX_DEPTH, clip_sigma=clip), want, (L, clip))


def test_labels_above_num_labels_are_ignored_and_counted():
    key = (8, 256, 320, 1, 8)
    d, lab, K, M = _scene(key)
    want = R.localize(d, lab, K, M, num_labels=5, max_depth=R.MAX_DEPTH)
    full = _want(key, None, 1)
    assert want["n_ignored"] == int(full["n_pixels"][:, 5:].sum()) > 0 and want["n_labelled"] == int(full["n_pixels"][:, :5].sum())
    got = _localize(d, lab, K, M, num_labels=5, max_depth=R.MAX_DEPTH)
    _assert_equal(got, want)
    assert torch.equal(got.n_pixels.cpu(), torch.from_numpy(full["n_pixels"][:, :5].copy()))         # ... and in no record


def test_labelled_pixels_without_a_usable_depth():
    """Frame 1's depths under label 2 are 0, negative, NaN, +inf or >= max_depth: pixels and a box, no sample, NaN centres; label 3
    is in no frame."""
    key = (3, 17, 23, 1, 3)
    d, lab, K, M = (a.copy() for a in _scene(key))
    lab[lab == 3] = 0
    under = np.argwhere(lab[1, 0] == 2)
    assert len(under) >= 10
    for i, (v, u) in enumerate(under):
        d[1, 0, v, u] = (0.0, -0.0, -1.5, np.nan, np.inf, -np.inf, R.MAX_DEPTH, 7.0)[i % 8]
    want = R.localize(d, lab, K, M, num_labels=3, max_depth=R.MAX_DEPTH)
    assert want["n_pixels"][1, 1] == len(under) and want["n_samples"][1, 1] == 0 and (want["bbox"][1, 1] >= 0).all()
    assert np.isnan(want["center_cam"][1, 1]).all() and np.isnan(want["center_world"][1, 1]).all() and want["n_frames"][1] == 2
    assert (want["bbox"][:, 2] == -1).all() and want["first_frame"][2] == -1 and want["last_frame"][2] == -1 and want["n_frames"][2] == 0
    assert np.isnan(want["position"][2]).all() and np.isnan(want["radius"][2])
    for clip in (None, R.CLIP_SIGMA):
        want = R.localize(d, lab, K, M, num_labels=3, max_depth=R.MAX_DEPTH, clip_sigma=clip)
        _assert_equal(_localize(d, lab, K, M, num_labels=3, max_depth=R.MAX_DEPTH, clip_sigma=clip), want, clip)


def test_deterministic_across_calls_and_streams():
    from coivo_amd import localize as Z
    key = (8, 256, 320, 1, 8)
    args = [_t(x) for x in _scene(key)]
    kw = dict(num_labels=8, max_depth=R.MAX_DEPTH, clip_sigma=R.CLIP_SIGMA, min_samples=40)
    a = Z.localize_polyps(*args, **kw)
    b = Z.localize_polyps(*args, **kw)
    _same(a, b)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        c = Z.localize_polyps(*args, **kw)
    side.synchronize()
    _same(a, c)


def test_permuting_the_frames_permutes_the_observations():
    key = (8, 256, 320, 1, 8)
    d, lab, K, M = _scene(key)
    kw = dict(num_labels=8, max_depth=R.MAX_DEPTH, clip_sigma=R.CLIP_SIGMA)
    a = _localize(d, lab, K, M, **kw)
    perm = np.random.default_rng(3).permutation(8)
    assert not np.array_equal(perm, np.arange(8))
    b = _localize(d[perm], lab[perm], K[perm], M[perm], **kw)
    index = torch.from_numpy(perm).to(dev())
    for k in PER_OBSERVATION:
        assert torch.equal(_bits(getattr(a, k))[index], _bits(getattr(b, k))), k
    assert (a.n_labelled, a.n_ignored) == (b.n_labelled, b.n_ignored)
    assert torch.equal(a.n_frames, b.n_frames) and torch.equal(a.n_samples_total, b.n_samples_total)     # integers: no order in them


def test_reconstruct_sequence_also_localizes():
    from coivo_amd import inference as I, localize as Z, nn as hnn, synth
    from oracle import colvo_spec as S
    dn_o, pn_o = S.make_models(31)
    dn, pn = hnn.DepthNet(), hnn.PoseNet()
    dn.load_state_dict(dn_o.state_dict())
    pn.load_state_dict(pn_o.state_dict())
    b = synth.make_batch(5, 64, 96, seed=31)
    frames, K = b["tgt"].to(dev()), b["K"].to(dev())
    labels = torch.zeros(5, 1, 64, 96, dtype=torch.uint8, device=dev())
    labels[:, :, 10:30, 20:50] = 1
    labels[1:4, :, 40:60, 60:90] = 2
    labels[0, :, 0:4, 0:4] = 9
    plain = I.reconstruct_sequence(dn, pn, frames, K, stride=2, chunk=2)                 # as a caller from before would call it
    assert plain.polyps is None and plain.fused is None and len(plain) == 5
    rec = I.reconstruct_sequence(dn, pn, frames, K, stride=2, chunk=2, labels=labels, num_labels=2)
    assert torch.equal(rec.depths, plain.depths) and torch.equal(rec.rel_poses, plain.rel_poses)
    assert torch.equal(rec.cam2world, plain.cam2world) and torch.equal(rec.points, plain.points) and rec.fused is None
    Kn = K.to(torch.float32).contiguous()
    want = Z.localize_polyps(rec.depths, labels, Kn, rec.cam2world.to(dev(), torch.float32), num_labels=2)
    _same(rec.polyps, want)
    assert rec.polyps.n_ignored == 16 and rec.polyps.n_labelled == 5 * 600 + 3 * 600
    assert rec.polyps.n_pixels.tolist() == [[600, 0], [600, 600], [600, 600], [600, 600], [600, 0]]
    # ... and that is the replica's answer
    ref = R.localize(rec.depths.cpu().numpy(), labels.cpu().numpy(), Kn.cpu().numpy(), rec.cam2world.float().numpy(), num_labels=2,
                     max_depth=I.MAX_DEPTH)
    _assert_equal(rec.polyps, ref)
    with pytest.raises(ValueError):
        I.reconstruct_sequence(dn, pn, frames, K, labels=labels)


def test_argument_errors():
    from coivo_amd import localize as Z
    d, lab, K, M = (_t(x) for x in _scene((3, 17, 23, 1, 3)))
    for bad in ((d.cpu(), lab, K, M), (d, lab.cpu(), K, M), (d, lab.to(torch.int32), K, M), (d, lab[:2], K, M), (d, lab, K[:1], M),
                (d, lab, K, M[:, :3])):
        with pytest.raises(ValueError):
            Z.localize_polyps(*bad, num_labels=3)
    narrow = K.clone()
    narrow[:, 0, 0] = 1e-4
    with pytest.raises(ValueError, match="2\\^31"):
        Z.localize_polyps(d, lab, narrow, M, num_labels=3)
    with pytest.raises(ValueError, match="2\\^62"):
        Z.localize_polyps(d, lab, K, M, num_labels=3, max_depth=2.0 ** 18)


@pytest.mark.parametrize("clip", [None, R.CLIP_SIGMA], ids=["plain", "clip_sigma"])
def test_memory_discipline(clip):
    """localize_polyps under tests/guarded.py on 4 frames of 64 x 96 at stride 2 with four labels, min_samples 40: depths, labels,
    intrinsics and poses between guard bands; the records (colvo_localize_workspace_bytes), the clip bounds and every per-observation
    and per-label output from the pool under both poisons.  Outputs equal the replica, are the same bytes under either poison, and no
    guard byte changes.  Launches reached: the clearing of the records, the accumulation pass and the write-out; with clip_sigma the
    bounds pass and the second, clipped accumulation as well."""
    from coivo_amd import _lib, localize as Z
    from tests import guarded as G
    key = (4, 64, 96, 2, 4)
    d, lab, K, M = _scene(key)
    want = _want(key, clip, 40)
    assert want["n_labelled"] > 0
    run = lambda pool: Z.localize_polyps(pool.place(_t(d)), pool.place(_t(lab)), pool.place(_t(K)), pool.place(_t(M)), num_labels=4, stride=2,
                                         max_depth=R.MAX_DEPTH, clip_sigma=clip, min_samples=40)
    outs, pools = G.under_both_poisons(dev(), run, f"localize_polyps clip {clip}")
    for got, pool in zip(outs, pools):
        _assert_equal(got, want, clip)
        G.assert_served(pool, 0, _lib.load().colvo_localize_workspace_bytes(4, 4), "localize_polyps")
