"""CPU checks of the loader's augmentation (coivo_amd/data.py Augment, csrc/augment.hip's C entry): the float64 reference against the
oracle's resize and against itself mirrored, the intrinsics of a cropped / mirrored frame, the purity and the ranges of the seeded
draws, constructor validation, and the C entry's refusals before any launch."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from coivo_amd import data as D
from oracle import colvo_spec as S
from tests import augment_ref as R

PIXEL_TOL = 2e-6                 # tests/test_data_gpu.py
SHAPES = [(48, 64, 48, 64), (48, 64, 96, 160), (100, 130, 64, 96), (270, 350, 256, 320), (7, 5, 32, 32), (1080, 1350, 256, 320)]


def _frames(h, w, W, n=3):
    g = torch.Generator().manual_seed(h * 7 + W)
    return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)


def _identity(h, w):
    return D.FrameAug(0.0, 0.0, h, w, 0, 1.0)


@pytest.mark.parametrize("h,w,H,W", SHAPES)
def test_reference_at_identity_matches_the_oracle(h, w, H, W):
    n = 1 if h > 1000 else 3
    u8 = _frames(h, w, W, n)
    want = S.resize_frames_u8(u8, H, W).double().numpy()
    got = R.augment_frames(u8.numpy(), [_identity(h, w)] * n, H, W)
    err = np.abs(got - want).max()
    exact = np.abs(R.augment_frames(u8.numpy(), [_identity(h, w)] * n, H, W, coords="float64") - want).max()
    print(f"{h}x{w} -> {H}x{W}: reference vs oracle {err:.3e} (with exact coordinates {exact:.3e})")
    assert got.shape == want.shape and err < PIXEL_TOL


@pytest.mark.parametrize("h,w,H,W", [(100, 130, 64, 96), (7, 5, 32, 32)])
def test_reference_under_a_flip_is_the_exact_mirror(h, w, H, W):
    u8 = _frames(h, w, W).numpy()
    A = D.compose_colour(1.1, 0.9, 1.2, 0.05, 1.05, -0.02)
    recs = [D.FrameAug(1.25, 2.5, h / 1.15, w / 1.15, f, 1.25, A) for f in (0, 1, 0)]
    out = R.augment_frames(u8[[0, 0, 1]], recs, H, W)
    assert np.array_equal(out[1], out[0][..., ::-1])
    assert not np.array_equal(out[2], out[0])


def test_intrinsics_follow_the_crop_and_the_mirror():
    rng = np.random.default_rng(11)
    (h, w), (H, W) = (270, 350), (256, 320)
    K = np.array([[301.5, 0.0, 171.25], [0.0, 298.0, 133.5], [0.0, 0.0, 1.0]])
    P = np.stack([rng.uniform(-2, 2, 64), rng.uniform(-2, 2, 64), rng.uniform(0.5, 6.0, 64)])        # Z > 0
    for flip in (0, 1):
        rec = D.FrameAug(13.375, 21.140625, h / 1.15, w / 1.15, flip)
        uvw = K @ P
        u, v = uvw[0] / uvw[2], uvw[1] / uvw[2]
        u2 = (u + 0.5 - float(rec.ox)) * W / float(rec.cw) - 0.5
        v2 = (v + 0.5 - float(rec.oy)) * H / float(rec.ch) - 0.5
        if flip:
            u2 = W - 1 - u2
        Pm = P * np.array([[-1.0 if flip else 1.0], [1.0], [1.0]])       # a mirrored image shows the scene with X -> -X
        for Kp, tol in ((R.augment_intrinsics(K, rec, (h, w), (H, W)), 1e-9),):
            q = Kp @ Pm
            assert np.abs(q[0] / q[2] - u2).max() < tol and np.abs(q[1] / q[2] - v2).max() < tol
        # the float32 K' the loader ships: every entry within 4 float32 ulps of K's largest entry of the float64 one
        K32 = D.augment_intrinsics(torch.from_numpy(K), rec, (h, w), (H, W)).to(torch.float32)
        K64 = R.augment_intrinsics(K, rec, (h, w), (H, W))
        ulp = float(np.spacing(np.float32(np.abs(K64).max())))
        assert np.abs(K32.double().numpy() - K64).max() <= 4 * ulp
        assert np.array_equal(D.augment_intrinsics(torch.from_numpy(K), rec, (h, w), (H, W)).numpy(), K64)     # data.py == the reference


@pytest.mark.parametrize("hw,HW", [((48, 64), (96, 160)), ((60, 80), (64, 96)), ((270, 350), (256, 320))])
def test_identity_crop_reproduces_resize_intrinsics(hw, HW):
    K = torch.tensor([[50.0, 0, 31.0], [0, 52.0, 23.0], [0, 0, 1]], dtype=torch.float64)
    rec = _identity(*hw)
    assert torch.equal(D.augment_intrinsics(K, rec, hw, HW), S.resize_intrinsics(K, hw, HW))
    assert np.array_equal(R.augment_intrinsics(K.numpy(), rec, hw, HW), D.resize_intrinsics(K, hw, HW).numpy())
    K32 = D.augment_intrinsics(K.float(), rec, hw, HW).to(torch.float32)
    ulp = float(np.spacing(np.float32(K32.abs().max().item())))
    assert (K32 - D.resize_intrinsics(K.float(), hw, HW)).abs().max().item() <= 4 * ulp


@pytest.mark.parametrize("hw,HW", [((48, 64), (96, 160)), ((60, 80), (64, 96)), ((270, 350), (256, 320))])
def test_loader_intrinsics_of_an_uncropped_pair_are_resize_intrinsics_bit_for_bit(hw, HW):
    """What PairLoader ships (float32): an identity record gives augment=None's K exactly; any other record the float64 formula
    rounded once, pair by pair in a mixed batch."""
    Ks = torch.stack([torch.tensor([[50.0 + i, 0, 31.3], [0, 52.7, 23.0 + i], [0, 0, 1]]) for i in range(4)])
    ident = D.Augment.identity().params(1, 2, 3, hw)
    drawn = [D.Augment().params(1, 2, i, hw) for i in range(3)]
    recs = [drawn[0], ident, drawn[1], drawn[2]]
    K = D.batch_intrinsics(Ks, recs, hw, HW)
    assert K.dtype == torch.float32 and K.shape == (4, 3, 3)
    assert torch.equal(K[1], D.resize_intrinsics(Ks, hw, HW)[1])
    assert torch.equal(D.batch_intrinsics(Ks, [ident] * 4, hw, HW), D.resize_intrinsics(Ks, hw, HW))
    for j in (0, 2, 3):
        assert np.array_equal(K[j].numpy(), R.augment_intrinsics(Ks[j].numpy(), recs[j], hw, HW).astype(np.float32))


def test_params_is_a_pure_function_of_its_key():
    a = D.Augment()
    keys = [(s, e, i) for s in (0, 3) for e in (0, 1, 2) for i in (0, 1, 17, 2 ** 40)]
    first = {k: a.params(*k, (60, 80)) for k in keys}
    assert all(a.params(*k, (60, 80)) == first[k] for k in reversed(keys))         # again, in another order
    assert all(D.Augment().params(*k, (60, 80)) == first[k] for k in keys)         # ... and from another object
    assert len(set(first.values())) == len(keys)                                   # seed, epoch and index all matter
    import threading
    got = {}
    th = [threading.Thread(target=lambda k=k: got.__setitem__(k, a.params(*k, (60, 80)))) for k in keys]
    [t.start() for t in th]
    [t.join() for t in th]
    assert got == first
    # the draws are numpy's Philox keyed on (seed, epoch) at counter (0, index, 0, 0)
    u = np.random.Generator(np.random.Philox(key=[3, 1], counter=[0, 17, 0, 0])).random(13)
    assert D._uniforms(3, 1, 17, 13) == u.tolist()
    r = first[(3, 1, 17)]
    assert r.flip == int(u[0] < 0.5) and r.terms["zoom"] == 1.0 + u[1] * (1.15 - 1.0)


def test_draws_stay_inside_their_ranges():
    a = D.Augment()
    h, w = 270, 350
    seen_flip = set()
    lo = dict(zoom=1.0, brightness=0.8, contrast=0.8, saturation=0.8, hue=-0.1, a_tgt=0.9, a_ref=0.9, b_tgt=-0.05, b_ref=-0.05)
    hi = dict(zoom=1.15, brightness=1.2, contrast=1.2, saturation=1.2, hue=0.1, a_tgt=1.1, a_ref=1.1, b_tgt=0.05, b_ref=0.05)
    span = {k: [math.inf, -math.inf] for k in lo}
    for i in range(2000):
        r = a.params(1, i % 3, i, (h, w))
        seen_flip.add(r.flip)
        assert r.flip in (0, 1) and np.float32(0.8) <= np.float32(r.gamma) <= np.float32(1.25)
        assert 0.0 <= r.oy and r.oy + r.ch <= h and 0.0 <= r.ox and r.ox + r.cw <= w          # float64 sums of the float32 values
        assert r.ch == float(np.float32(h / r.terms["zoom"])) and r.cw == float(np.float32(w / r.terms["zoom"]))
        for k in lo:
            assert lo[k] <= r.terms[k] <= hi[k], (k, r.terms[k])
            span[k][0], span[k][1] = min(span[k][0], r.terms[k]), max(span[k][1], r.terms[k])
        t = r.terms
        for A, f in ((r.A_tgt, "tgt"), (r.A_ref, "ref")):
            want = D.compose_colour(t["brightness"], t["contrast"], t["saturation"], t["hue"], t[f"a_{f}"], t[f"b_{f}"])
            assert np.array_equal(A, want.astype(np.float32))
        assert not np.array_equal(r.A_tgt, r.A_ref)                   # the illumination term is drawn per frame
    assert seen_flip == {0, 1}
    for k in lo:                                                       # ... and the ranges are used, not just respected
        assert span[k][0] < lo[k] + 0.05 * (hi[k] - lo[k]) and span[k][1] > hi[k] - 0.05 * (hi[k] - lo[k]), k


def test_colour_terms_compose_in_the_documented_order():
    lum = np.array(D.LUMA)
    x = np.array([0.2, 0.5, 0.9])
    g, c, s, hue, a, b = 1.1, 0.85, 1.2, 0.07, 1.05, -0.03
    y = g * x
    y = c * (y - 0.5) + 0.5
    y = (lum @ y) + s * (y - lum @ y)
    th, n = 2 * math.pi * hue, np.ones(3) / math.sqrt(3)
    y = y * math.cos(th) + np.cross(n, y) * math.sin(th) + n * (n @ y) * (1 - math.cos(th))       # Rodrigues, about the grey axis
    y = a * y + b
    A = D.compose_colour(g, c, s, hue, a, b)
    assert np.abs(A[:, :3] @ x + A[:, 3] - y).max() < 1e-15
    grey = D.compose_colour(1.0, 1.0, 0.3, 0.2) @ np.array([0.4, 0.4, 0.4, 1.0])                   # saturation and hue leave greys alone
    assert np.abs(grey - 0.4).max() < 1e-15


def test_identity_augment_yields_the_identity_record():
    ident = D.Augment.identity()
    for key in ((0, 0, 0), (5, 3, 1234567), (2 ** 63, 7, 9)):
        r = ident.params(*key, (60, 80))
        assert (r.oy, r.ox, r.ch, r.cw, r.flip, r.gamma) == (0.0, 0.0, 60.0, 80.0, 0, 1.0)
        assert np.array_equal(r.A_tgt, D.IDENTITY_A) and np.array_equal(r.A_ref, D.IDENTITY_A)
        t = D.aug_table([r.tgt, r.ref], 64, 96)
        assert t.shape == (2, 20) and t.dtype == np.float32
        assert t[0, :4].tolist() == [0.0, 0.0, float(np.float32(60 / 64)), float(np.float32(80 / 96))]
        assert t[:, 4].view(np.int32).tolist() == [0, 0] and np.array_equal(t[0, 6:18].reshape(3, 4), D.IDENTITY_A)


@pytest.mark.parametrize("kw", [dict(p_flip=-0.1), dict(p_flip=1.5), dict(max_zoom=0.9), dict(max_zoom=math.inf), dict(gamma=(0.0, 1.0)),
                                dict(gamma=(1.2, 0.9)), dict(gamma=(0.8, math.nan)), dict(brightness=math.nan), dict(contrast=-0.1),
                                dict(saturation=1.0), dict(hue=0.6), dict(illum_gain=math.inf), dict(illum_offset=-0.01),
                                dict(gamma=1.0)])
def test_bad_ranges_are_refused(kw):
    with pytest.raises(ValueError):
        D.Augment(**kw)


def test_c_entry_refuses_bad_arguments_without_a_gpu():
    from coivo_amd import _lib, build
    build.ensure()
    lib = _lib.load()
    buf = (C.c_char * 272)()
    p = (C.addressof(buf) + 15) // 16 * 16                # a 16-byte aligned address inside buf; no call below gets to dereference it
    ok = (p, 2, 8, 8, 32, 32, p, p, 0)
    for bad, msg in (((0,) + ok[1:], b"null pointer"), (ok[:6] + (0, p, 0), b"null pointer"), (ok[:7] + (0, 0), b"null pointer"),
                     (ok[:6] + (p + 4, p, 0), b"16-byte aligned"),
                     ((p, 0) + ok[2:], b"bad shape"), ((p, 70000) + ok[2:], b"bad shape"), ((p, 2, 0) + ok[3:], b"bad shape"),
                     ((p, 2, 8, 8, 32, 0) + ok[6:], b"bad shape"), ((p, 2, 1 << 14, 1 << 14) + ok[4:], b"bad shape"),
                     ((p, 2, 8, 8, 4 * 65536, 32) + ok[6:], b"bad shape")):
        rc = lib.colvo_frames_u8_augment(*bad)
        err = lib.colvo_last_error()
        assert rc != 0 and err.startswith(b"colvo_frames_u8_augment:") and msg in err, (bad, err)


def test_loader_refuses_a_non_augment(tmp_path):
    from tests.test_data_cpu import make_tree
    ds = D.SequenceFolder(make_tree(str(tmp_path)))
    with pytest.raises(ValueError):
        D.PairLoader(ds, 2, (64, 96), augment="yes")
