"""-m gpu checks of the augmenting conversion pass (csrc/augment.hip) and of PairLoader(augment=...): identity rows against the plain
conversion kernel bit for bit, the mirror, native-scale crops and a power-of-two gain exactly, general geometry / colour / gamma
against the float64 reference (tests/augment_ref.py), a hostile table, and the loader end to end."""
import functools

import numpy as np
import pytest
import torch

from tests import augment_ref as R
from tests.gpu_util import dev
from tests.test_data_cpu import make_tree

pytestmark = pytest.mark.gpu

SHAPES = [(48, 64, 48, 64), (48, 64, 96, 160), (100, 130, 64, 96), (7, 5, 32, 32), (270, 350, 256, 320)]
N = 3
# powf against float64 pow of the same float32 value, gamma 0.8 and 1.25, every 8-bit level: twice the largest error measured on an
# MI355X (GAMMA_MEASURED), and in any case <= 1e-6 -- a condition, not a measurement: a 1 % error in gamma
# moves mid-grey by 3e-3
GAMMA_MEASURED = 4.946e-8        # gamma 0.8 (4.311e-8 at gamma 1.25), gfx950, ROCm's powf
GAMMA_BAR = min(2 * GAMMA_MEASURED, 1e-6)


@functools.lru_cache(maxsize=None)
def _frames(h, w):
    g = torch.Generator().manual_seed(h * 131 + w)
    return torch.randint(0, 256, (N, h, w, 3), generator=g, dtype=torch.uint8)


def _plain(u8, H, W):
    from coivo_amd import _lib
    lib = _lib.load()
    n, h, w, _ = u8.shape
    out = torch.empty(n, 3, H, W, device=dev())
    _lib.check(lib.colvo_frames_u8_to_f32(_lib.ptr(u8), n, h, w, H, W, _lib.ptr(out), _lib.stream_ptr()), "frames")
    return out


def _augment(u8, table, H, W):
    """u8 [n,h,w,3] on the device, table [n,20] float32 (numpy) -> [n,3,H,W] on the device."""
    from coivo_amd import _lib
    lib = _lib.load()
    n, h, w, _ = u8.shape
    assert table.shape == (n, _lib.AUG_ROW_FLOATS) and table.dtype == np.float32
    tab = torch.from_numpy(table).to(dev())
    out = torch.full((n, 3, H, W), float("nan"), device=dev())
    _lib.check(lib.colvo_frames_u8_augment(_lib.ptr(u8), n, h, w, H, W, _lib.ptr(tab), _lib.ptr(out), _lib.stream_ptr()), "augment")
    torch.cuda.synchronize()
    return out


def _run(u8, recs, H, W):
    from coivo_amd import data as D
    return _augment(u8.to(dev()), D.aug_table(recs, H, W), H, W)


def _identity_rows(h, w):
    from coivo_amd import data as D
    return [D.FrameAug(0.0, 0.0, h, w, 0, 1.0) for _ in range(N)]


def _general_rows(h, w, gamma=1.0):
    """Three DIFFERENT rows: fractional origins, zoom 1.15, the odd frame mirrored, every colour term active and strong enough that
    a good share of the 8-bit noise lands on each clamp."""
    from coivo_amd import data as D
    ch, cw = h / 1.15, w / 1.15
    rows = []
    for i, (fy, fx) in enumerate(((0.31, 0.77), (1.0, 0.0), (0.5, 0.13))):
        A = D.compose_colour(1.0 + 0.05 * i, 1.9 - 0.1 * i, 1.3, 0.08 - 0.07 * i, 1.1 - 0.1 * i, 0.05 - 0.04 * i)
        oy = np.floor(fy * (h - float(np.float32(ch))) * 64) / 64
        ox = np.floor(fx * (w - float(np.float32(cw))) * 64) / 64
        rows.append(D.FrameAug(oy, ox, ch, cw, i % 2, gamma, A))
    return rows


@pytest.mark.parametrize("h,w,H,W", SHAPES)
def test_identity_rows_equal_the_plain_kernel(h, w, H, W):
    u8 = _frames(h, w).to(dev())
    assert torch.equal(_run(u8, _identity_rows(h, w), H, W), _plain(u8, H, W))


def test_flip_mirrors_bit_for_bit():
    from coivo_amd import data as D
    (h, w), (H, W) = (100, 130), (64, 96)
    rows = _general_rows(h, w, gamma=1.25)
    a = _run(_frames(h, w), [D.FrameAug(r.oy, r.ox, r.ch, r.cw, 0, r.gamma, r.A) for r in rows], H, W)
    b = _run(_frames(h, w), [D.FrameAug(r.oy, r.ox, r.ch, r.cw, 1, r.gamma, r.A) for r in rows], H, W)
    assert torch.equal(b, a.flip(-1)) and not torch.equal(b, a)


@pytest.mark.parametrize("h,w,H,W", [(100, 130, 64, 96), (270, 350, 256, 320)])
def test_native_scale_crop_is_exact(h, w, H, W):
    from coivo_amd import data as D
    u8 = _frames(h, w)
    origins = [(0, 0), (h - H, w - W), (7, 3)]             # the second touches the bottom-right corner: oy + ch == h, ox + cw == w
    got = _run(u8, [D.FrameAug(oy, ox, H, W, 0, 1.0) for oy, ox in origins], H, W).cpu()
    for i, (oy, ox) in enumerate(origins):
        want = u8[i, oy:oy + H, ox:ox + W].permute(2, 0, 1).float() / 255.0
        assert torch.equal(got[i], want), (oy, ox)


def test_power_of_two_gain_is_exact():
    from coivo_amd import data as D
    (h, w), (H, W) = (48, 64), (96, 160)
    half = np.concatenate([0.5 * np.eye(3), np.zeros((3, 1))], axis=1)
    got = _run(_frames(h, w), [D.FrameAug(0.0, 0.0, h, w, 0, 1.0, half) for _ in range(N)], H, W)
    assert torch.equal(got, 0.5 * _plain(_frames(h, w).to(dev()), H, W))


def _check_against_reference(h, w, H, W, gamma, bar_extra):
    rows = _general_rows(h, w, gamma)
    got = _run(_frames(h, w), rows, H, W).cpu().double().numpy()
    want = R.augment_frames(_frames(h, w).numpy(), rows, H, W)
    worst = 0.0
    for i, r in enumerate(rows):
        bar = gamma * R.channel_bound(r.A) + bar_extra
        err = np.abs(got[i] - want[i]).max(axis=(1, 2))
        print(f"{h}x{w} -> {H}x{W} gamma {gamma} frame {i}: max error per channel {err}, bar {bar}; at 0: {(want[i] == 0).mean():.3f}, "
              f"at 1: {(want[i] == 1).mean():.3f}")
        assert (want[i] == 0).mean() > 0.05 and (want[i] == 1).mean() > 0.05 and ((want[i] > 0) & (want[i] < 1)).mean() > 0.3
        worst = max(worst, (err / bar).max())
    assert worst <= 1.0, worst
    assert not np.array_equal(got[0], got[2])


@pytest.mark.parametrize("h,w,H,W", SHAPES)
def test_general_geometry_and_colour_match_the_reference(h, w, H, W):
    _check_against_reference(h, w, H, W, 1.0, 0.0)


@pytest.mark.parametrize("gamma", [0.8, 1.25])
def test_gamma_on_exact_inputs(gamma):
    """Identity geometry and colour at the native size: the value before the power is exactly u8/255 in float32."""
    from coivo_amd import data as D
    h, w = 48, 64
    u8 = _frames(h, w).clone()
    u8[0, 0, :, 0] = torch.arange(64, dtype=torch.uint8) * 4           # every level is there, 0 and 255 included
    u8[0, 1, :, 0] = torch.arange(64, dtype=torch.uint8) * 4 + 3
    u8[0, 2, :4, 0] = torch.tensor([0, 1, 254, 255], dtype=torch.uint8)
    got = _run(u8, [D.FrameAug(0.0, 0.0, h, w, 0, gamma) for _ in range(N)], h, w).cpu().double()
    base = (u8.permute(0, 3, 1, 2).float() / 255.0).double()
    err = (got - base ** gamma).abs().max().item()
    print(f"gamma {gamma}: largest error of powf against float64 pow {err:.3e} (bar {GAMMA_BAR:.3e})")
    assert err <= GAMMA_BAR
    assert got.min().item() == 0.0 and got.max().item() == 1.0


@pytest.mark.parametrize("h,w,H,W", [(100, 130, 64, 96), (270, 350, 256, 320)])
def test_gamma_after_general_geometry_and_colour(h, w, H, W):
    _check_against_reference(h, w, H, W, 1.25, GAMMA_BAR)


def test_hostile_table_reads_stay_inside_the_frame():
    """Any bit pattern is defined behaviour: a NaN coordinate reads pixel 0, a coordinate far outside reads the nearest edge pixel,
    flip = 7 is a flip, and the output is finite and in [0,1] whatever the colour entries hold."""
    (h, w), (H, W) = (100, 130), (64, 96)
    u8 = _frames(h, w)[:1].expand(6, -1, -1, -1).contiguous()
    nan, inf = float("nan"), float("inf")
    ident = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    t = np.zeros((6, 20), dtype=np.float32)
    t[0] = [nan, nan, nan, nan, 0, 1.0] + ident + [nan, nan]                       # NaN geometry -> pixel (0, 0)
    t[1] = [0.0, 0.0, inf, inf, 0, 1.0] + ident + [0, 0]                           # +inf step -> the last pixel
    t[2] = [-inf, -inf, 1.0, 1.0, 0, 1.0] + ident + [0, 0]                         # -inf origin -> pixel (0, 0)
    t[3] = [3e9, 3e9, 1e6, 1e6, 0, 1.0] + ident + [0, 0]                           # a crop far outside, mirrored with flip = 7
    t[4] = [inf, 0.0, -inf, 1e30, 0, 1.0] + ident + [0, 0]                         # inf - inf: NaN in y (row 0), far right in x
    t[5] = [1.0, 2.0, 1.2, 1.1, 0, nan] + [nan, inf, -inf, 0, 1e38, 1e38, 1e38, 1e38, -1e38, 0, 0, nan] + [0, 0]
    t[:, 4].view(np.int32)[:] = [0, 0, 0, 7, 0x7fc00000, -1]
    got = _augment(u8.to(dev()), t, H, W).cpu()
    assert torch.isfinite(got).all() and got.min().item() >= 0.0 and got.max().item() <= 1.0
    px = lambda y, x: (u8[0, y, x].float() / 255.0).view(3, 1, 1).expand(3, H, W)
    for i, (y, x) in enumerate([(0, 0), (h - 1, w - 1), (0, 0), (h - 1, w - 1), (0, w - 1)]):
        assert torch.equal(got[i], px(y, x)), i


# ---- the loader ------------------------------------------------------------------------------------------------------------------ #
HW, SIZE = (60, 80), (64, 96)


def _tree(tmp_path):
    from coivo_amd import data as D
    return D.SequenceFolder(make_tree(str(tmp_path), seqs=(("a", 9, HW), ("b", 6, HW))))


def _collect(ds, batch, augment, *, epoch=1, seed=3, rank=0, world=1, prefetch=2):
    """{dataset index: (tgt, ref, K, record)} of one pass, tensors on the CPU."""
    from coivo_amd import data as D
    ld = D.PairLoader(ds, batch, SIZE, rank=rank, world_size=world, shuffle=True, seed=seed, workers=2, prefetch=prefetch, augment=augment)
    ld.set_epoch(epoch)
    idx = D.shard_indices(len(ds), batch, rank, world, shuffle=True, seed=seed, epoch=epoch)
    out = {}
    try:
        for step, b in enumerate(ld):
            assert ("aug" in b) == (augment is not None) and b["frames"].data_ptr() == b["tgt"].data_ptr()
            for j, i in enumerate(idx[step * batch:(step + 1) * batch]):
                out[i] = (b["tgt"][j].cpu(), b["ref"][j].cpu(), b["K"][j].cpu(), b["aug"][j] if augment is not None else None)
    finally:
        ld.close()
    assert len(out) == len(idx)
    return out


def test_loader_batches_match_the_reference(tmp_path):
    from coivo_amd import data as D
    ds = _tree(tmp_path)
    aug = D.Augment(gamma=(1.0, 1.25))                  # gamma < 1 has an unbounded slope at 0: held to the reference on exact inputs only
    got = _collect(ds, 3, aug)
    assert len(got) == 12
    flips = set()
    for i, (tgt, ref, K, rec) in got.items():
        assert rec == aug.params(3, 1, i, HW)
        flips.add(rec.flip)
        item = ds[i]
        for name, t, fr in (("tgt", tgt, rec.tgt), ("ref", ref, rec.ref)):
            want = R.augment_frames(item[name][None], [fr], *SIZE)[0]
            bar = float(rec.gamma) * R.channel_bound(fr.A) + (GAMMA_BAR if rec.gamma != 1.0 else 0.0)
            err = np.abs(t.double().numpy() - want).max(axis=(1, 2))
            assert (err <= bar).all(), (i, name, err, bar)
        K64 = R.augment_intrinsics(item["K"].double().numpy(), rec, HW, SIZE)
        assert np.abs(K.double().numpy() - K64).max() <= 4 * float(np.spacing(np.float32(np.abs(K64).max())))
    assert flips == {0, 1}


def test_loader_draws_repeat_change_with_the_epoch_and_ignore_the_sharding(tmp_path):
    from coivo_amd import data as D
    ds = _tree(tmp_path)
    aug = D.Augment()
    one = _collect(ds, 2, aug, prefetch=1)                                                  # 1 rank, batches of 2, prefetch 1
    again = _collect(ds, 2, D.Augment(), prefetch=1)
    assert one.keys() == again.keys() and len(one) == 12
    for i in one:
        assert all(torch.equal(a, b) for a, b in zip(one[i][:3], again[i][:3])) and one[i][3] == again[i][3]
    other = _collect(ds, 2, aug, epoch=2, prefetch=1)
    for i in one.keys() & other.keys():
        assert one[i][3] != other[i][3] and not torch.equal(one[i][0], other[i][0])
    assert len(one.keys() & other.keys()) >= 10
    two = {}
    for rank in range(2):                                                                   # 2 ranks, batches of 3, prefetch 2
        two.update(_collect(ds, 3, aug, rank=rank, world=2, prefetch=2))
    common = one.keys() & two.keys()
    assert len(two) == 12 and len(common) >= 11
    for i in common:
        assert one[i][3] == two[i][3] and all(torch.equal(a, b) for a, b in zip(one[i][:3], two[i][:3])), i


def test_identity_augment_equals_no_augment(tmp_path):
    from coivo_amd import data as D
    ds = _tree(tmp_path)
    plain = _collect(ds, 3, None)
    ident = _collect(ds, 3, D.Augment.identity())
    assert plain.keys() == ident.keys()
    for i in plain:
        assert torch.equal(plain[i][0], ident[i][0]) and torch.equal(plain[i][1], ident[i][1])
        assert torch.equal(plain[i][2], ident[i][2])            # an uncropped, unmirrored pair takes resize_intrinsics itself


def test_augmented_batches_feed_a_training_step(tmp_path):
    from coivo_amd import data as D, nn as hnn, optim
    ds = D.SequenceFolder(make_tree(str(tmp_path), seqs=(("a", 5, (64, 96)),)))
    ld = D.PairLoader(ds, 2, (64, 96), shuffle=False, augment=D.Augment())
    dn, pn = hnn.DepthNet(), hnn.PoseNet()
    opt = optim.FusedAdam([dn, pn])
    losses = []
    for batch in ld:
        assert len(batch["aug"]) == 2 and batch["frames"].shape[0] == 4
        loss = hnn.dcdp_forward(dn, pn, None, None, batch["K"], frames=batch["frames"])[0]
        loss.backward()
        opt.step()
        losses.append(loss.item())
    ld.close()
    assert len(losses) == 2 and all(np.isfinite(losses))


@pytest.mark.parametrize("h,w,H,W", [(7, 5, 32, 32), (100, 130, 64, 96)])
def test_memory_discipline(h, w, H, W):
    """colvo_frames_u8_augment with the source frames and the parameter table between guard bands and the destination from
    tests/guarded.py's pool, under both poisons: general rows (fractional crop origins, zoom 1.15, a mirrored frame, gamma 1.25 at 100 x 130) held
    to the float64 reference as in _check_against_reference, and native-scale crops that touch the source's bottom-right corner, exact.
    No tap may leave the source, every output element must be written, nothing may be written outside the destination.  One launch:
    the augmenting conversion kernel."""
    from coivo_amd import _lib, data as D
    from tests import guarded as G
    lib = _lib.load()
    u8 = _frames(h, w)
    gamma, bar_extra = (1.25, GAMMA_BAR) if (h, w) == (100, 130) else (1.0, 0.0)      # the shapes each bar is stated for above
    rows = _general_rows(h, w, gamma)
    cases = [("general", rows)]
    if h >= H and w >= W:
        cases.append(("corner crops", [D.FrameAug(oy, ox, H, W, 0, 1.0) for oy, ox in ((0, 0), (h - H, w - W), (7, 3))]))
    for what, recs in cases:
        table = D.aug_table(recs, H, W)
        outs = []
        for poison in G.POISONS:
            pool = G.Pool(dev(), poison)
            src, tab = pool.place(u8.to(dev()), "frames"), pool.place(torch.from_numpy(table).to(dev()), "table")
            out = pool.empty((N, 3, H, W), torch.float32, label="out")
            _lib.check(lib.colvo_frames_u8_augment(_lib.ptr(src), N, h, w, H, W, _lib.ptr(tab), _lib.ptr(out), _lib.stream_ptr()), "augment")
            pool.check(f"colvo_frames_u8_augment {what} {h}x{w} -> {H}x{W}, poison {poison:#04x}")
            assert torch.equal(src.cpu(), u8) and torch.equal(tab.cpu(), torch.from_numpy(table))
            outs.append(out)
        G.assert_same_bits(outs[0], outs[1], what)
        got = outs[0].cpu()
        if what == "general":
            want = R.augment_frames(u8.numpy(), recs, H, W)
            for i, r in enumerate(recs):
                err = np.abs(got[i].double().numpy() - want[i]).max(axis=(1, 2))
                assert (err <= gamma * R.channel_bound(r.A) + bar_extra).all(), (what, i, err)
        else:
            for i, r in enumerate(recs):
                oy, ox = int(r.oy), int(r.ox)
                assert torch.equal(got[i], u8[i, oy:oy + H, ox:ox + W].permute(2, 0, 1).float() / 255.0), (oy, ox)
