"""-m gpu: the fused loss kernels against the chunked float64 reference (tests/loss_ref.py) at every march geometry.

march_plan() gives each wave a strip of columns and a segment of `seg_rows` rows (4..64, chosen from the shape).  The
other loss tests run at seg_rows = 4 only; here the TUNE knobs march_rows_fwd / march_rows_bwd force every height on shapes
that end a segment exactly at the last row, one row past it, one row short, or inside a segment longer than the image, with
strips that end at, one column past and one column short of the border and batches that leave the last workgroup partial;
then the benchmark shapes run with production tuning.  Frames carry i.i.d. per-pixel noise, so a one-row or one-column slip
of a window or a tap changes the result by the noise.

Bars against float64, per case:
  * d_depth / d_r: outside the decision margin (loss_ref: validity flips, tap cells, |.| signs, SSIM clamp) NO element beyond
    rtol 2e-3 + 2e-4 x max; elements the fp32 oracle itself misses by a quarter of that bar (ill-conditioned at fp32
    coordinates) are counted and reported, not judged;
  * d_pose, d_a, d_b: gpu_util.grad_parity_failures against the fp32 oracle's own distance from float64; where that fails,
    every element within GRAD_K x the oracle's largest error plus what the margin's decisions can move it by (loss_ref);
  * loss within 1e-5;
  * the kernel's valid count (an exact integer in fp32) inside [n_sure, n_sure + n_doubt] per level: a strip segment dropped
    or counted twice by a finalize shows here whatever the tolerances.
"""
import pytest
import torch

from tests import loss_ref as R
from tests.gpu_util import GRAD_K, dev, grad_parity_failures, grad_parity_table

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-5
RTOL, ATOL_SCALE = 2e-3, 2e-4
KNOBS = ("march_rows_fwd", "march_rows_bwd")
# decisions of the margin the kernel may take the other way in one image (a handful is what fp32 rounding flips: see
# tests/test_loss_ref_cpu.py; a dropped strip segment or a lost channel moves hundreds of pixels)
DECISION_FLIPS = 4


@pytest.fixture
def march_rows():
    """-> set(fwd, bwd): force the rows per strip segment of the two marches; the production values are restored after."""
    from coivo_amd import _lib
    saved = {n: _lib.tune_get(n) for n in KNOBS}

    def set_rows(fwd=0, bwd=0):
        _lib.tune_set("march_rows_fwd", fwd)
        _lib.tune_set("march_rows_bwd", bwd)

    yield set_rows
    for n, v in saved.items():
        _lib.tune_set(n, v)


@pytest.fixture
def fused(monkeypatch):
    from coivo_amd import functional as Fh

    def set_fused(on):
        monkeypatch.setattr(Fh, "FUSE_TRAINING_PASS", on)
    set_fused(True)
    return set_fused


# ---------------------------------------------------------------------------------------------------------------------- #
# the HIP side                                                                                                              #
# ---------------------------------------------------------------------------------------------------------------------- #
def _photometric(t, form):
    """form: 'grad' (fused or two-pass, as FUSE_TRAINING_PASS says), 'fwd' (no_grad: the forward-only march) or 'handover'
    (DepthNet.forward_pair_split's form: d_depth raw, times the posted scales).  -> dict(loss, count [1, B] summed, grads)"""
    from coivo_amd import functional as Fh
    d = {k: v.to(dev()) for k, v in t.items()}
    if form == "fwd":
        with torch.no_grad():
            loss = Fh.photometric_loss(d["tgt"], d["ref"], d["depth"], d["pose"], d["K"], d["lcc_a"], d["lcc_b"])
        return dict(loss=loss.item(), count=[loss._base[2].item()])
    leaves = [d[k].clone().requires_grad_(True) for k in ("depth", "pose", "lcc_a", "lcc_b")]
    hand = None
    if form == "handover":
        hand = Fh.GradHandover()
        leaves[0]._colvo_handover = hand
    loss = Fh.photometric_loss(d["tgt"], d["ref"], leaves[0], leaves[1], d["K"], leaves[2], leaves[3])
    count = loss._base[2].item()                  # loss_state = [loss, 1 / max(3 n, 1), n, masked sum]; loss is its [0]
    grads = list(torch.autograd.grad(loss, leaves))
    if hand is not None:
        sa, sb = hand.take((grads[0],))
        assert sa is not None and sb is not None, "the hand-over form did not run"
        grads[0] = grads[0] * (sa * sb)
    out = dict(loss=loss.item(), count=[count])
    out.update({k: g.cpu() for k, g in zip(("d_depth", "d_pose", "d_a", "d_b"), grads)})
    return out


def _full(t, kw):
    from coivo_amd import functional as Fh
    d = {k: v.to(dev()) for k, v in t.items()}
    leaves = [d[k].clone().requires_grad_(True) for k in ("depth", "d_r", "pose", "lcc_a", "lcc_b")]
    loss = Fh.dcdp_full_loss(d["tgt"], d["ref"], leaves[0], leaves[1], leaves[2], d["K"], leaves[3], leaves[4], **kw)
    terms = Fh.full_objective_terms(loss).cpu()
    count = [terms[4 + 4 * s + 2].item() for s in range(kw["num_scales"])]
    grads = torch.autograd.grad(loss, leaves)
    out = dict(loss=loss.item(), count=count)
    out.update({k: g.cpu() for k, g in zip(("d_depth", "d_r", "d_pose", "d_a", "d_b"), grads)})
    return out


# ---------------------------------------------------------------------------------------------------------------------- #
# the bars                                                                                                                 #
# ---------------------------------------------------------------------------------------------------------------------- #
def _elements(got, r64, r32, margin, what):
    got, ref, o32 = got.double(), r64.double(), r32.double()
    bar = ATOL_SCALE * max(ref.abs().max().item(), 1e-30) + RTOL * ref.abs()
    err = (got - ref).abs()
    ill = (o32 - ref).abs() > 0.25 * bar                     # the fp32 oracle itself is this far off: rounding-bound
    bad = (err > bar) & ~margin & ~ill
    n = int(bad.sum())
    if n:
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {n} element(s) beyond rtol {RTOL} + {ATOL_SCALE} x max outside the margin, first at "
                             f"{i}: got {got[tuple(i)].item():.6e}, float64 {ref[tuple(i)].item():.6e}, fp32 oracle "
                             f"{o32[tuple(i)].item():.6e}")
    return int((ill & ~margin).sum())


def _check(h, t, tag, **kw):
    """h: the HIP result (_photometric / _full); kw: loss_ref.evaluate's objective arguments."""
    r64 = R.evaluate(t, margins=True, **kw)
    assert abs(h["loss"] - r64["loss"]) < LOSS_TOL, (tag, h["loss"], r64["loss"])
    for s, c in enumerate(h["count"]):
        lo, hi = r64["n_sure"][s].sum().item(), (r64["n_sure"][s] + r64["n_doubt"][s]).sum().item()
        assert c == int(c) and lo <= c <= hi, f"{tag}: level {s} valid count {c} outside [{lo:.0f}, {hi:.0f}]"
    if "d_depth" not in h:
        print(f"{tag}: loss |d| {abs(h['loss'] - r64['loss']):.1e}, counts {h['count']}")
        return
    r32 = R.evaluate(t, dtype=torch.float32, **kw)
    ill = _elements(h["d_depth"], r64["d_depth"], r32["d_depth"], r64["m_depth"], tag + " d_depth")
    if r64["d_r"] is not None:
        ill += _elements(h["d_r"], r64["d_r"], r32["d_r"], r64["m_r"], tag + " d_r")
    names = ("d_pose", "d_a", "d_b")
    rows = grad_parity_table([(n, h[n]) for n in names], [(n, r32[n]) for n in names], [(n, r64[n]) for n in names])
    bad = grad_parity_failures(rows)
    if bad:
        # one decision taken the other way in the margin (an L1 sign, a tap cell) moves a cancelling sum over a small image
        # by more than rounding does: beyond the fp32 oracle's distance, an element may differ by what DECISION_FLIPS
        # decisions of the margin can move it (loss_ref `allow`: the largest move of one), and by no more
        allow = {"d_pose": r64["allow"][:, :6], "d_a": r64["allow"][:, 6:7], "d_b": r64["allow"][:, 7:8]}
        for n in names:
            g64 = r64[n].double()
            lim = GRAD_K * (r32[n].double() - g64).abs().max() + DECISION_FLIPS * allow[n]
            over = (h[n].double() - g64).abs() > lim
            assert not over.any(), f"{tag}: {n} beyond the fp32 oracle's distance and the margin's decisions: " + "; ".join(bad)
        print(f"{tag}: reduced gradients inside the margin's decision allowance: " + "; ".join(bad))
    print(f"{tag}: loss |d| {abs(h['loss'] - r64['loss']):.1e}, counts {h['count']}, margin {R.margin_fraction(r64):.2%} of "
          f"d_depth (d_r {r64['m_r'].double().mean().item():.2%}), {ill} rounding-bound elements")
    return r64


# ---------------------------------------------------------------------------------------------------------------------- #
# (a) every segment height                                                                                                 #
# ---------------------------------------------------------------------------------------------------------------------- #
# (rows, B, H, W): one-pass strips are 60 columns wide (BCOLS), forward-only strips 62 (MCOLS); items = B x segments x strips
# per launch, in workgroups of 4 waves.  H % rows runs over 0, 1, rows - 1 and H < rows.
ONE_PASS = [(4, 3, 8, 60), (5, 1, 2, 121), (7, 2, 13, 120), (16, 3, 33, 61), (31, 1, 62, 181), (47, 2, 5, 119), (63, 1, 125, 62),
            (64, 3, 65, 63)]
TWO_PASS = [(4, 2, 7, 121), (7, 3, 15, 60), (31, 1, 31, 63), (64, 2, 5, 181)]
FORWARD = [(5, 3, 11, 62), (16, 1, 15, 63), (47, 2, 94, 61), (63, 1, 2, 120), (4, 2, 9, 124), (64, 1, 64, 61)]
# (rows, B, H, W, scales): every level's plan takes the knob (level heights in the comments)
FULL = [(4, 2, 40, 120, 4),        # 40 20 10 5
        (5, 3, 26, 62, 2),         # 26 13
        (7, 3, 48, 64, 4),         # 48 24 12 6
        (16, 1, 68, 180, 3),       # 68 34 17
        (31, 2, 62, 122, 2),       # 62 31
        (47, 2, 93, 119, 1),
        (63, 1, 126, 62, 2),       # 126 63
        (64, 1, 130, 122, 2)]      # 130 65


def _motion(H):
    return 0.0 if H <= 2 else 2.0          # (a two-row image keeps valid pixels only under a small motion)


def _id(c):
    return "r{}-B{}-{}x{}".format(*c[:4]) + (f"-s{c[4]}" if len(c) > 4 else "")


@pytest.mark.parametrize("case", ONE_PASS, ids=_id)
def test_one_pass(case, march_rows, fused):
    rows, B, H, W = case
    march_rows(bwd=rows)
    t = R.noisy_case(B, H, W, seed=500 + rows, pose_scale=_motion(H))
    _check(_photometric(t, "grad"), t, "one-pass " + _id(case))


@pytest.mark.parametrize("case", TWO_PASS, ids=_id)
def test_two_pass(case, march_rows, fused):
    rows, B, H, W = case
    fused(False)
    march_rows(fwd=rows, bwd=rows)
    t = R.noisy_case(B, H, W, seed=520 + rows, pose_scale=_motion(H))
    _check(_photometric(t, "grad"), t, "two-pass " + _id(case))


@pytest.mark.parametrize("case", FORWARD, ids=_id)
def test_forward_only(case, march_rows):
    rows, B, H, W = case
    march_rows(fwd=rows)
    t = R.noisy_case(B, H, W, seed=540 + rows, pose_scale=_motion(H))
    _check(_photometric(t, "fwd"), t, "forward " + _id(case))


@pytest.mark.parametrize("case", FULL, ids=_id)
def test_full_objective(case, march_rows):
    rows, B, H, W, S = case
    march_rows(bwd=rows)
    t = R.noisy_case(B, H, W, seed=560 + rows, pose_scale=_motion(H))
    kw = dict(num_scales=S, geo_weight=0.5, smooth_weight=0.1)
    _check(_full(t, kw), t, "full " + _id(case), **kw)


def test_more_strip_segments_than_finalize_threads(march_rows, fused):
    """1 x 1024 x 1280 at seg_rows 4: 256 x 22 = 5 632 one-pass strip segments per image (256 x 21 forward-only), more than
    the 1 024 threads of the finalize that adds them up per image."""
    B, H, W = 1, 1024, 1280
    march_rows(fwd=4, bwd=4)
    t = R.noisy_case(B, H, W, seed=580)
    _check(_photometric(t, "grad"), t, "one-pass 1x1024x1280 r4")
    _check(_photometric(t, "fwd"), t, "forward 1x1024x1280 r4")
    kw = dict(num_scales=2, geo_weight=0.5, smooth_weight=0.1)
    _check(_full(t, kw), t, "full 1x1024x1280 r4 s2", **kw)


# ---------------------------------------------------------------------------------------------------------------------- #
# (b) the benchmark shapes with production tuning                                                                          #
# ---------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("B,H,W", [(8, 256, 320), (32, 256, 320), (64, 256, 320), (32, 512, 640)])
def test_benchmark_shapes(B, H, W, fused):
    from coivo_amd import _lib
    assert all(_lib.tune_get(n) == 0 for n in KNOBS), "the production march_plan must choose the rows"
    t = R.noisy_case(B, H, W, seed=600 + B + H)
    _check(_photometric(t, "handover"), t, f"hand-over B{B} {H}x{W}")
    kw = dict(num_scales=3, geo_weight=0.5, smooth_weight=0.1)
    _check(_full(t, kw), t, f"full B{B} {H}x{W}", **kw)


# ---------------------------------------------------------------------------------------------------------------------- #
# (c) an image with nothing valid among valid ones                                                                         #
# ---------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("form", ["one-pass", "two-pass", "full"])
def test_image_behind_the_camera(form, fused):
    B, H, W = 3, 64, 124
    t = R.noisy_case(B, H, W, seed=620)
    t["pose"] = t["pose"].clone()
    t["pose"][1] = torch.tensor([0.0, 0.0, -100.0, 0.0, 0.0, 0.0])      # every point of image 1 behind the camera
    if form == "full":
        kw = dict(num_scales=2, geo_weight=0.5, smooth_weight=0.0)
        h = _full(t, kw)
    else:
        fused(form == "one-pass")
        kw = {}
        h = _photometric(t, "grad")
    r64 = _check(h, t, f"image 1 behind the camera, {form}", **kw)
    assert (r64["n_valid"][:, 1] == 0).all() and (r64["n_valid"][:, [0, 2]] > 0).all()
    for k in ("d_pose", "d_a", "d_b"):
        assert torch.count_nonzero(h[k][1]) == 0, f"{form}: {k} of the image with no valid pixel is not exactly zero"
        assert torch.count_nonzero(h[k][[0, 2]]) > 0, k
    assert torch.count_nonzero(h["d_depth"][1]) == 0
