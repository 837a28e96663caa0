"""The chunked float64 reference of the loss kernels (tests/loss_ref.py) and the evidence for its decision margins; no GPU.

* Chunked == unchunked: `evaluate` combines per-chunk sums with the spec's global normalisers; at small shapes it must equal
  the spec evaluated in one piece, for one chunk, several, and a split that leaves a short last chunk.
* The margins are wide enough: wherever fp32 and fp64 evaluations of the spec's `project` decide validity or the bilinear
  cell (floor of x or y) differently, and wherever the L1 term's sign differs, the float64 margin holds the pixel; and the
  validity + tap margin stays below 1 % of the pixels, so the GPU tests still check nearly every element.
"""
import pytest
import torch

from oracle import colvo_spec as S
from tests import loss_ref as R

FULL3 = dict(num_scales=3, geo_weight=0.5, smooth_weight=0.1)
FULL4 = dict(num_scales=4, geo_weight=0.7, smooth_weight=0.2)


@pytest.mark.parametrize("B,H,W,chunk,kw", [
    (3, 33, 47, 1, {}),
    (3, 33, 47, 2, {}),             # 2 + 1
    (3, 33, 47, 3, {}),
    (5, 2, 5, 2, {}),               # 2 + 2 + 1, two-row images
    (3, 40, 56, 2, FULL3),
    (4, 48, 64, 3, FULL4),          # 3 + 1
    (2, 36, 52, 1, dict(num_scales=2, geo_weight=0.5, smooth_weight=0.0)),
])
def test_chunked_equals_spec(B, H, W, chunk, kw):
    t = R.noisy_case(B, H, W, seed=400 + B * H + chunk, pose_scale=2.0)
    got = R.evaluate(t, chunk=chunk, **kw)
    want = R.spec_value_and_grads(t, **kw)
    assert abs(got["loss"] - want["loss"]) <= 1e-12 * abs(want["loss"]), (got["loss"], want["loss"])
    for k in ("d_depth", "d_pose", "d_a", "d_b", "d_r"):
        if want[k] is None:
            assert got[k] is None
            continue
        scale = want[k].abs().max().item()
        assert scale > 0, k
        err = (got[k] - want[k]).abs().max().item()
        assert err <= 1e-10 * scale, (k, err, scale)
    # the counts are the spec's validity, level by level
    lv = R._levels(t["tgt"].double(), t["ref"].double(), t["depth"].double(), t["K"].double(), kw.get("num_scales", 1))
    for s, (_, _, dp, K) in enumerate(lv):
        assert torch.equal(got["n_valid"][s], S.project(dp, t["pose"].double(), K)[2].sum(dim=(1, 2)).double())


def test_float32_evaluation_is_the_fp32_oracle():
    t = R.noisy_case(2, 32, 48, seed=431)
    got = R.evaluate(t, dtype=torch.float32, chunk=1)
    leaves = [t[k].clone().requires_grad_(True) for k in ("depth", "pose", "lcc_a", "lcc_b")]
    loss = S.photometric_loss(t["tgt"], t["ref"], leaves[0], leaves[1], t["K"], leaves[2], leaves[3])
    grads = torch.autograd.grad(loss, leaves)
    assert got["d_depth"].dtype == torch.float32
    assert abs(got["loss"] - loss.item()) < 1e-6
    for k, g in zip(("d_depth", "d_pose", "d_a", "d_b"), grads):
        assert (got[k] - g).abs().max().item() <= 1e-5 * g.abs().max().item(), k


def test_chunk_size_bounds_the_graph():
    assert R.default_chunk(512, 640) >= 1 and R.default_chunk(512, 640) * 512 * 640 * R.GRAPH_BYTES_PER_PX <= R.CHUNK_BYTES
    assert R.default_chunk(1024, 1280) == 1
    assert R.default_chunk(4, 4) > 1000


def _pixels(t, dtype):
    c = {k: v.to(dtype) for k, v in t.items()}
    x, y, valid = S.project(c["depth"], c["pose"], c["K"])
    recal = S.lcc_recalibrate(S.bilinear_sample(c["ref"], x, y, valid), c["lcc_a"], c["lcc_b"])
    return x.double(), y.double(), valid, (c["tgt"] - recal).double()


def _strong_turn(t):
    """a yaw of 1.5 rad: z crosses Z_EPS inside the image (the z bound decides), most points leave the frame."""
    t = dict(t)
    p = t["pose"].clone()
    p[:, 4] = 1.5
    t["pose"] = p
    return t


@pytest.mark.parametrize("B,H,W,seed,ps,turn", [
    (4, 256, 320, 440, 1.0, False),
    (2, 512, 640, 441, 1.0, False),
    (1, 1024, 1280, 442, 1.0, False),
    (8, 128, 128, 443, 4.0, False),     # large motion: a quarter of the pixels leave the frame
    (4, 96, 128, 444, 8.0, False),
    (2, 128, 160, 445, 1.0, True),
])
def test_margin_holds_every_fp32_decision_flip(B, H, W, seed, ps, turn):
    t = R.noisy_case(B, H, W, seed=seed, pose_scale=ps)
    if turn:
        t = _strong_turn(t)
    x32, y32, v32, l32 = _pixels(t, torch.float32)
    x64, y64, v64, l64 = _pixels(t, torch.float64)
    c = {k: v.double() for k, v in t.items()}
    Pz, xr, yr = R._camera_z_and_pixel(c["depth"], c["pose"], c["K"])
    sure, doubt = R.validity_margin(xr, yr, Pz, H, W)
    # validity: sure -> valid in both, outside sure | doubt -> invalid in both
    vflip = v32 != v64
    assert not (vflip & ~doubt).any(), f"{int((vflip & ~doubt).sum())} validity flips outside the margin"
    assert v64[sure].all() and v32[sure].all() and not v64[~(sure | doubt)].any()
    # the bilinear cell, where both evaluations sample
    both = v32 & v64
    cell = both & ((x32.floor() != x64.floor()) | (y32.floor() != y64.floor()))
    tap = R.tap_margin(x64, y64)
    assert not (cell & ~tap).any(), f"{int((cell & ~tap).sum())} cell changes outside the margin"
    # the L1 term's sign
    sign = both.unsqueeze(1) & (l32.sign() != l64.sign())
    near = l64.abs() < R.L1_EPS
    assert not (sign & ~near).any(), f"{int((sign & ~near).sum())} L1 sign flips outside the margin"
    frac = ((doubt | tap) & (sure | doubt)).double().mean().item()
    assert frac < 1e-2, f"validity + tap margin covers {frac:.3%} of the pixels"
    print(f"B{B} {H}x{W} ps {ps}{' turn' if turn else ''}: {int(vflip.sum())} validity flips, {int(cell.sum())} cell changes, "
          f"{int(sign.sum())} L1 sign flips; margin {frac:.3%} (validity {doubt.double().mean().item():.3%})")


def test_margin_masks_of_the_reference():
    """`evaluate(margins=True)`: the count interval holds the fp32 count; the d_depth mask holds the dilated validity doubt."""
    t = R.noisy_case(4, 64, 64, seed=450, pose_scale=4.0)
    r64 = R.evaluate(t, margins=True)
    r32 = R.evaluate(t, dtype=torch.float32)
    assert (r64["n_sure"] <= r64["n_valid"]).all() and (r64["n_valid"] <= r64["n_sure"] + r64["n_doubt"]).all()
    assert (r64["n_sure"] <= r32["n_valid"]).all() and (r32["n_valid"] <= r64["n_sure"] + r64["n_doubt"]).all()
    assert r64["n_doubt"].sum() > 0, "the case should put some pixels on a validity bound"
    m = r64["m_depth"]
    assert m.dtype == torch.bool and m.shape == t["depth"].shape and 0 < m.double().mean().item() < 0.1
