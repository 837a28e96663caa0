"""CPU checks of the polyp localisation (coivo_amd.localize, csrc/localize.hip): the NumPy replica the GPU tests compare with
(tests/localize_ref.py) against an answer written down by hand and against the spheres implanted in its scenes, what those
scenes show, the clip, the C ABI's refusals before any HIP call, the wrapper's guards and localization_error."""
import ctypes as C
import functools
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

from coivo_amd import localize as Z
from tests import localize_ref as R


@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _scene(key):
    N, H, W, stride, L = key
    seed, spheres = R.SCENES[key]
    return R.scene(N, H, W, seed, spheres)


@functools.lru_cache(maxsize=None)
def _located(key, clip):
    N, H, W, stride, L = key
    d, lab, K, M = _scene(key)
    return R.localize(d, lab, K, M, num_labels=L, stride=stride, max_depth=R.MAX_DEPTH, clip_sigma=clip)


# ---- the replica ------------------------------------------------------------------------------------------------------- #
def _hand_scene():
    """Two 4x4 frames, fx = fy = 64, cx = cy = 0, identity rotation; frame 1 is frame 0 moved by (0.125, 0, 0.25).
        labels  1 1 1 1     depths  1   1   1.5 1.5
                0 2 2 0             1   1.5 1.5 1
                0 0 0 0             1   1   1   1
                0 0 0 7             1   1   1   1          (7 is above num_labels = 2: ignored)
    px = u / 64 * d, so q_x = 64 u d, q_y = 64 v d, q_z = 4096 d: every quantity is a small dyadic number, exact in float32
    and float64."""
    labels = np.zeros((2, 1, 4, 4), np.uint8)
    labels[:, 0, 0] = 1
    labels[:, 0, 1, 1:3] = 2
    labels[:, 0, 3, 3] = 7
    depths = np.ones((2, 1, 4, 4), np.float32)
    depths[:, 0, 0, 2:] = 1.5
    depths[:, 0, 1, 1:3] = 1.5
    K = np.broadcast_to(np.array([[64.0, 0, 0], [0, 64.0, 0], [0, 0, 1]], np.float32), (2, 3, 3)).copy()
    M = np.broadcast_to(np.eye(4, dtype=np.float32), (2, 4, 4)).copy()
    M[1, :3, 3] = (0.125, 0.0, 0.25)
    return depths, labels, K, M


def test_replica_gives_the_hand_computed_answer():
    depths, labels, K, M = _hand_scene()
    r = R.localize(depths, labels, K, M, num_labels=2, stride=1, max_depth=10.0)
    assert (r["n_labelled"], r["n_ignored"]) == (12, 2)
    assert r["n_pixels"].tolist() == [[4, 2], [4, 2]] and r["n_samples"].tolist() == [[4, 2], [4, 2]]
    assert r["bbox"].tolist() == [[[0, 0, 3, 0], [1, 1, 2, 1]]] * 2
    assert r["pixel"].tolist() == [[[1.5, 0.0], [1.5, 1.0]]] * 2
    # label 1: q_x = 0, 64, 192, 288 (sum 544), q_y = 0, q_z = 4096, 4096, 6144, 6144 (sum 20480)
    #   sum q_x^2 = 123904, sum q_x q_z = 3211264, sum q_z^2 = 109051904
    # label 2: q_x = 96, 192 (sum 288), q_y = 96, 96, q_z = 6144, 6144
    #   sum q_x^2 = 46080, sum q_x q_y = 27648, sum q_x q_z = 1769472, sum q_y^2 = 18432, sum q_y q_z = 1179648, sum q_z^2 = 75497472
    m1 = [Fr(544, 4096 * 4), Fr(0), Fr(20480, 4096 * 4)]
    m2 = [Fr(288, 4096 * 2), Fr(192, 4096 * 2), Fr(12288, 4096 * 2)]
    assert [float(x) for x in m1] == [0.033203125, 0.0, 1.25] and [float(x) for x in m2] == [0.03515625, 0.0234375, 1.5]
    s1 = [123904, 0, 3211264, 0, 0, 109051904]
    s2 = [46080, 27648, 1769472, 18432, 1179648, 75497472]
    cov = lambda s, m, n: [Fr(s[e], 2 ** 24 * n) - m[a] * m[b] for e, (a, b) in enumerate(R.PAIRS)]
    c1, c2 = cov(s1, m1, 4), cov(s2, m2, 2)
    assert float(c1[5]) == 0.0625 and float(c1[2]) == 0.00634765625 and float(c2[5]) == 0.0 and float(c2[3]) == 0.0   # var{1, 1, 1.5, 1.5}
    for f in range(2):
        assert r["center_cam"][f].tolist() == [[float(x) for x in m1], [float(x) for x in m2]]
        assert r["cov_cam"][f].tolist() == [[float(x) for x in c1], [float(x) for x in c2]]
    t = [Fr(1, 8), Fr(0), Fr(1, 4)]
    assert r["center_world"][1].tolist() == [[float(m[a] + t[a]) for a in range(3)] for m in (m1, m2)]
    assert r["center_world"][0].tolist() == r["center_cam"][0].tolist()
    # two frames of equal weight: the position is the midpoint, the covariance gains the spread of the two centres, t t^T / 4
    assert r["position"].tolist() == [[float(m[a] + t[a] / 2) for a in range(3)] for m in (m1, m2)]
    want = [[float(c[e] + t[a] * t[b] / 4) for e, (a, b) in enumerate(R.PAIRS)] for c in (c1, c2)]
    assert r["cov_world"].tolist() == want
    assert r["radius"].tolist() == [float(np.sqrt(w[0] + w[3] + w[5])) for w in want]
    assert r["n_frames"].tolist() == [2, 2] and r["n_samples_total"].tolist() == [8, 4]
    assert r["first_frame"].tolist() == [0, 0] and r["last_frame"].tolist() == [1, 1]
    # min_samples = 3 leaves label 2 unseen; the per-observation rows do not change
    r3 = R.localize(depths, labels, K, M, num_labels=2, stride=1, max_depth=10.0, min_samples=3)
    assert r3["n_frames"].tolist() == [2, 0] and r3["first_frame"].tolist() == [0, -1] and r3["n_samples_total"].tolist() == [8, 0]
    assert np.isnan(r3["position"][1]).all() and np.isnan(r3["cov_world"][1]).all() and np.isnan(r3["radius"][1])
    assert np.array_equal(r3["center_cam"], r["center_cam"]) and r3["position"][0].tolist() == r["position"][0].tolist()
    # max_depth = 1.5 drops the far half: label 1 keeps u = 0, 1, label 2 keeps nothing but its pixels and its box
    r4 = R.localize(depths, labels, K, M, num_labels=2, stride=1, max_depth=1.5)
    assert r4["n_samples"].tolist() == [[2, 0], [2, 0]] and r4["n_pixels"].tolist() == [[4, 2], [4, 2]]
    assert r4["bbox"].tolist() == r["bbox"].tolist() and r4["pixel"][0].tolist()[0] == [0.5, 0.0] and np.isnan(r4["pixel"][0, 1]).all()
    assert r4["center_cam"][0, 0].tolist() == [32 / 4096, 0.0, 1.0] and r4["cov_cam"][0, 0, 5] == 0.0
    # the clip: label 1's depths are 1, 1, 1.5, 1.5 (mean 1.25, deviation 0.25 each): k = 1 keeps all four, k = 0.5 none
    assert R.localize(depths, labels, K, M, num_labels=2, max_depth=10.0, clip_sigma=1.0)["n_samples"].tolist() == [[4, 2], [4, 2]]
    assert R.localize(depths, labels, K, M, num_labels=2, max_depth=10.0, clip_sigma=0.5)["n_samples"].tolist() == [[0, 2], [0, 2]]
    # stride 2 walks (0, 0), (2, 0), (0, 2), (2, 2): two pixels of label 1, none of label 2
    r5 = R.localize(depths, labels, K, M, num_labels=2, stride=2, max_depth=10.0)
    assert r5["n_pixels"].tolist() == [[2, 0], [2, 0]] and r5["bbox"][0].tolist() == [[0, 0, 2, 0], [-1, -1, -1, -1]] and r5["n_ignored"] == 0


@pytest.mark.parametrize("key", list(R.SCENES))
def test_scenes_show_their_polyps_and_the_replica_finds_them(key):
    """Cap points lie on the sphere, so their mean lies inside it: the replica's position is within the sphere's radius (+ 1e-3
    for the 1/4096 quanta) of the implanted centre.  A scene with at least three frames of more than 300 walked pixels shows
    every polyp in at least three frames with at least 30 samples each; the two 5x7 scenes (one or two frames, one walked
    pixel a frame at stride 9) cannot, and show their first polyp in every frame."""
    N, H, W, stride, L = key
    _, spheres = R.SCENES[key]
    for clip in (None, R.CLIP_SIGMA):
        r = _located(key, clip)
        big = N >= 3
        if big:
            assert ((r["n_samples"] >= 30).sum(axis=0) >= 3).all(), r["n_samples"]
            seen = range(L)
        else:
            assert (r["n_samples"][:, 0] >= 1).all()
            seen = [0]
        for l in seen:
            centre, radius = spheres[l]
            dist = float(np.linalg.norm(r["position"][l] - np.asarray(centre)))
            print(f"{key} clip {clip} polyp {l}: {dist:.4f} from the centre of a sphere of radius {radius}, extent {r['radius'][l]:.4f}")
            assert dist <= radius + 1e-3
            assert r["radius"][l] <= radius + 1e-3                             # the RMS extent of points on a sphere of that radius


def test_clip_brings_a_spilt_mask_back_to_the_polyp():
    c = R.CLIP_SCENE
    d, lab, K, M = R.scene(c["N"], c["H"], c["W"], c["seed"], c["spheres"], wall=c["wall"], dilate=c["dilate"])
    tight = R.scene(c["N"], c["H"], c["W"], c["seed"], c["spheres"], wall=c["wall"])[1]
    assert 0.05 < 1.0 - (tight != 0).sum() / (lab != 0).sum() < 0.6           # the ring the dilation added
    assert np.array_equal(d, R.scene(c["N"], c["H"], c["W"], c["seed"], c["spheres"], wall=c["wall"])[0])   # ... leaves the depth alone
    plain = R.localize(d, lab, K, M, num_labels=1, max_depth=R.MAX_DEPTH)
    clipped = R.localize(d, lab, K, M, num_labels=1, max_depth=R.MAX_DEPTH, clip_sigma=R.CLIP_SIGMA)
    centre, radius = c["spheres"][0]
    e0, e1 = (float(np.linalg.norm(x["position"][0] - np.asarray(centre))) for x in (plain, clipped))
    dropped = 1.0 - clipped["n_samples"].sum() / plain["n_pixels"].sum()
    print(f"distance from the sphere's centre: {e0:.4f} without clip, {e1:.4f} with; {dropped:.1%} of the labelled pixels dropped")
    assert e1 < e0 and e1 <= radius + 1e-3
    assert 0.05 <= dropped <= 0.6
    assert np.array_equal(plain["n_pixels"], clipped["n_pixels"]) and np.array_equal(plain["bbox"], clipped["bbox"])
    # a region of constant depth keeps all of its samples whatever k is: double(n q) / (4096 n) is exact
    flat = np.full_like(d, 1.2345)
    for k in (0.0, 1.5):
        r = R.localize(flat, lab, K, M, num_labels=1, max_depth=R.MAX_DEPTH, clip_sigma=k)
        assert np.array_equal(r["n_samples"], r["n_pixels"]) and (r["cov_cam"][..., 5] == 0.0).all()


# ---- the C ABI --------------------------------------------------------------------------------------------------------- #
def test_workspace_size(lib):
    f = lib.colvo_localize_workspace_bytes
    for bad in ((0, 1), (-1, 1), (65536, 1), (1, 0), (1, 256), (1, -3)):
        assert f(*bad) == 0, bad
    assert f(1, 1) == 128 + 16 and f(2, 3) == 6 * 128 + 16 and f(3, 255) == 3 * 255 * 128 + 32       # records, then a count per frame
    assert f(65535, 255) == 65535 * 255 * 128 + 65535 * 8 + 8
    assert all(f(n, l) % 16 == 0 for n in (1, 2, 3, 7) for l in (1, 2, 255))


def test_entry_points_refuse_bad_arguments_before_any_hip_call(lib):
    buf = (C.c_double * 66)()
    p = (C.addressof(buf) + 15) & ~15                                       # no call below gets past its checks to touch it

    def accumulate(**kw):
        a = dict(depths=p, labels=p, K=p, N=2, H=8, W=8, stride=1, max_depth=10.0, L=3, bounds=None, records=p)
        a.update(kw)
        return lib.colvo_localize_accumulate(a["depths"], a["labels"], a["K"], a["N"], a["H"], a["W"], a["stride"], a["max_depth"], a["L"],
                                             a["bounds"], a["records"], None)

    def bounds(**kw):
        a = dict(records=p, N=2, L=3, k=1.5, bounds=p)
        a.update(kw)
        return lib.colvo_localize_bounds(a["records"], a["N"], a["L"], a["k"], a["bounds"], None)

    outs = ("n_pixels", "n_samples", "bbox", "pixel", "center_cam", "cov_cam", "center_world", "n_frames", "n_samples_total",
            "first_frame", "last_frame", "position", "cov_world", "stats")

    def finish(**kw):
        a = dict({k: p for k in outs}, records=p, M=p, N=2, L=3, min_samples=1)
        a.update(kw)
        return lib.colvo_localize_finish(a["records"], a["M"], a["N"], a["L"], a["min_samples"], *(a[k] for k in outs), None)

    def refused(fn, name, what, **kw):
        assert fn(**kw) != 0, (name, kw)
        msg = lib.colvo_last_error().decode()
        assert msg.startswith(name + ": ") and what in msg, (name, kw, msg)

    for fn, name, ptrs in ((accumulate, "colvo_localize_accumulate", ("depths", "labels", "K", "records")),
                           (bounds, "colvo_localize_bounds", ("records", "bounds")),
                           (finish, "colvo_localize_finish", ("records", "M") + outs)):
        for k in ptrs:
            refused(fn, name, "null pointer", **{k: None})
        for s in (dict(N=0), dict(N=-1), dict(N=65536)):
            refused(fn, name, "bad shape", **s)
        for l in (0, -1, 256):
            refused(fn, name, "num_labels", L=l)
        refused(fn, name, "16-byte aligned", records=p + 8)
    for s in (dict(H=0), dict(W=-3), dict(stride=0), dict(stride=-2), dict(H=1 << 15, W=1 << 15)):
        refused(accumulate, "colvo_localize_accumulate", "bad shape", **s)
    for m in (0.0, -1.0, float("nan"), float("inf")):
        refused(accumulate, "colvo_localize_accumulate", "max_depth", max_depth=m)
    refused(accumulate, "colvo_localize_accumulate", "16-byte aligned", bounds=p + 8)
    refused(bounds, "colvo_localize_bounds", "16-byte aligned", bounds=p + 8)
    for k in (-0.5, float("nan"), float("inf")):
        refused(bounds, "colvo_localize_bounds", "clip_sigma", k=k)
    for m in (0, -4):
        refused(finish, "colvo_localize_finish", "min_samples", min_samples=m)


# ---- Python ------------------------------------------------------------------------------------------------------------ #
def test_wrapper_refuses_cpu_tensors_and_bad_arguments():
    d, lab, K, M = (torch.from_numpy(a) for a in _scene((3, 17, 23, 1, 3)))
    with pytest.raises(ValueError):
        Z.localize_polyps(d, lab, K, M, num_labels=3)                          # CPU tensors: no fallback
    with pytest.raises(ValueError):
        Z.localize_polyps(d[0], lab, K, M, num_labels=3)
    for bad in (dict(num_labels=0), dict(num_labels=256), dict(num_labels=2.0), dict(num_labels=3, stride=0),
                dict(num_labels=3, min_samples=0), dict(num_labels=3, max_depth=0.0), dict(num_labels=3, max_depth=float("inf")),
                dict(num_labels=3, clip_sigma=-1.0), dict(num_labels=3, clip_sigma=float("nan"))):
        with pytest.raises(ValueError):
            Z.localize_polyps(d, lab, K, M, **bad)
    assert Z.PolypLocalization._fields == ("n_pixels", "n_samples", "bbox", "pixel", "center_cam", "cov_cam", "center_world", "n_frames",
                                           "n_samples_total", "first_frame", "last_frame", "position", "cov_world", "radius",
                                           "n_labelled", "n_ignored")


def test_overflow_bounds():
    """max_depth * ray_max * 4096 < 2^31 and its square times the walked pixels < 2^62, in float64 from K alone."""
    from coivo_amd import synth
    K = synth.intrinsics(2, 256, 320)
    b = Z.quantum_bound(K, 256, 320, 10.0)
    assert b == 10.0 * 4096.0                                                  # fx = 0.8 W: no corner ray component exceeds 1
    assert 46.5 < np.log2(b * b * 256 * 320) < 48.5                            # 2^47: far below the 2^62 guard
    Z.check_sum_bounds(K, 256, 320, 1, 10.0)
    wide = K.clone()
    wide[1, 0, 0] = 0.25 * 320                                                 # one frame with a wide field of view
    assert Z.quantum_bound(wide, 256, 320, 10.0) == 10.0 * (159.5 / 80.0) * 4096.0
    Z.check_sum_bounds(wide, 256, 320, 1, 10.0)
    # the first bound: a quantum beyond int32
    with pytest.raises(ValueError, match="2\\^31"):
        Z.check_sum_bounds(K, 256, 320, 1, 2.0 ** 19)
    Z.check_sum_bounds(K, 4, 4, 4, 2.0 ** 19 * (1 - 2.0 ** -20))
    narrow = K.clone()
    narrow[:, 1, 1] = 1e-3                                                     # |(v - cy) / fy| = 127 500
    with pytest.raises(ValueError, match="2\\^31"):
        Z.check_sum_bounds(narrow, 256, 320, 1, 10.0)
    # the second: b = 2^30 passes the first, b^2 * walked = 2^60 * walked needs fewer than 4 walked pixels
    with pytest.raises(ValueError, match="2\\^62"):
        Z.check_sum_bounds(K, 256, 320, 1, 2.0 ** 18)
    with pytest.raises(ValueError, match="2\\^62"):
        Z.check_sum_bounds(K, 256, 320, 128, 2.0 ** 18)                        # 2 x 3 walked pixels
    Z.check_sum_bounds(K, 256, 320, 256, 2.0 ** 18)                            # 1 x 2


def test_localization_error():
    g = torch.Generator().manual_seed(7)
    from coivo_amd import inference as I
    traj = I.integrate_trajectory(torch.cat([0.05 * torch.randn(12, 3, generator=g), 0.03 * torch.randn(12, 3, generator=g)], dim=1))
    P = torch.randn(5, 3, generator=g, dtype=torch.float64)
    # ground truth = a known similarity of the prediction: x -> s R x + t (camera poses: rotation R R_i, position s R p_i + t)
    R0 = I.pose_to_matrix4(torch.tensor([[0.3, -0.2, 0.5, 0.4, -0.3, 0.2]]))[0]
    Rm, t, s = R0[:3, :3], R0[:3, 3], 1.7
    gt_traj = traj.clone()
    gt_traj[:, :3, :3] = Rm @ traj[:, :3, :3]
    gt_traj[:, :3, 3] = s * (traj[:, :3, 3] @ Rm.t()) + t
    G = s * (P @ Rm.t()) + t
    e = Z.localization_error(P, G, traj, gt_traj)
    assert e.shape == (5,) and e.dtype == torch.float64 and float(e.max()) < 1e-9
    assert float(Z.localization_error(P, G, traj, gt_traj, mode="se3").max()) > 1e-2      # a rigid fit cannot absorb the scale
    assert float(Z.localization_error(P, P, mode="none").max()) == 0.0
    assert torch.allclose(Z.localization_error(P, P + torch.tensor([3.0, 0.0, 4.0]), mode="none"), torch.full((5,), 5.0, dtype=torch.float64))
    assert torch.equal(Z.localization_error(P, G, traj, gt_traj, mode="none"), Z.localization_error(P, G, mode="none"))
    Pn = P.clone()
    Pn[2] = float("nan")
    en = Z.localization_error(Pn, G, traj, gt_traj)
    assert torch.isnan(en[2]) and float(en[[0, 1, 3, 4]].max()) < 1e-9
    for mode in ("sim3", "se3"):
        with pytest.raises(ValueError, match="none"):
            Z.localization_error(P, G, mode=mode)
    with pytest.raises(ValueError):
        Z.localization_error(P, G)                                             # the default mode aligns: it needs the trajectories
    with pytest.raises(ValueError):
        Z.localization_error(P, G, traj, None, mode="none")
    with pytest.raises(ValueError):
        Z.localization_error(P, G[:4], mode="none")
    with pytest.raises(ValueError):
        Z.localization_error(P, G, traj, gt_traj, mode="affine")


def test_reconstruction_keeps_its_shape():
    from coivo_amd import inference as I
    r = I.Reconstruction(1, 2, 3, 4)
    assert r.polyps is None and r.fused is None and tuple(r) == (1, 2, 3, 4, None)
    depths, rel, traj, points, fused = r                                     # still five to unpack
    full = I.Reconstruction(1, 2, 3, 4, 5, 6)
    assert full.fused == 5 and full.polyps == 6 and I.Reconstruction(1, 2, 3, 4, polyps=6).polyps == 6
    assert full._replace(points=9).polyps == 6 and full._replace(polyps=7).polyps == 7 and full._replace(polyps=7)[:5] == full[:5]
    import inspect
    sig = inspect.signature(I.reconstruct_sequence)
    assert sig.parameters["labels"].default is None and sig.parameters["num_labels"].default is None
