"""The sliced oracle step of tests/gpu_util.py, checked before it judges anything (tests/test_step_shapes_gpu.py); no GPU.

* Sliced == whole: the coupled step evaluated `slice_pairs` pairs at a time (valid-pixel count of the batch from a first sweep,
  one backward per slice) is the spec's step -- float64 loss and all 58 parameter gradients to 1e-12, free and with forced ReLU
  decisions, whose mask rows are s.. and B+s.. of DepthNet's 2B frames.
* Sensitivity of the step-level bar (grad_parity_failures: fp64 truth, fp32 oracle as the noise scale, matched decisions), on the
  reference alone: the sliced fp32 step stands in for the HIP path and passes; with one image's contribution missing from one
  mid layer's weight gradient that layer's two tensors fail and no other, and with the normaliser taken from one slice instead of
  the whole batch all 58 do.

What this level of test CANNOT see: one dropped 8x16 output tile of one image at 64 pairs of 256x320 is 128 of 5.2 M pixels of a
full-resolution layer and moves that layer's weight gradient by ~1e-5 of its norm, under the fp32 oracle's own distance from
float64 at that size (5e-4).  That is what the exact layer tests are for (tests/test_conv_exact_gpu.py).
"""
import pytest
import torch

from coivo_amd import synth
from oracle import colvo_spec as S
from tests import gpu_util as U

B, H, W, SEED = 6, 32, 64, 2024
MID = "iconv3"                                  # DepthNet, 1/4 resolution: 64 + 64 -> 64 channels


@pytest.fixture(scope="module")
def batch():
    return synth.make_batch(B, H, W, seed=SEED)


def _rel(a, b):
    return (a.double() - b.double()).norm().item() / max(b.double().norm().item(), 1e-300)


def _spec_masks(batch, per_row_flips=0):
    """ReLU decisions of the unsliced fp32 oracle, in hip_relu_masks' layout; per_row_flips: that many of the most marginal
    decisions of EVERY batch row of every layer turned over by hand, so that every slice has rows to select."""
    dn, pn = S.make_models(SEED)
    masks = {}
    for tag, net, skip in (("depth", dn, "head"), ("pose", pn, "pred")):
        for name, mod in net.named_children():
            if name != skip:
                mod.register_forward_hook(lambda mod, inp, out, key=f"{tag}.{name}": masks.__setitem__(key, out.detach().clone()))
    with torch.no_grad():
        S.dcdp_forward(dn, pn, batch["tgt"], batch["ref"], batch["K"])
    out = {}
    for key, pre in masks.items():
        m = pre > 0
        if per_row_flips:
            flat = pre.abs().flatten(1)
            idx = flat.topk(min(per_row_flips, flat.shape[1]), dim=1, largest=False).indices
            mf = m.flatten(1).clone()
            mf.scatter_(1, idx, ~mf.gather(1, idx))
            m = mf.view_as(m)
        out[key] = m
    return out


@pytest.fixture(scope="module")
def free_masks(batch):
    return _spec_masks(batch)


@pytest.mark.parametrize("slice_pairs", [2, 4])          # 2 + 2 + 2, and 4 + 2: a short last slice
@pytest.mark.parametrize("forced", [False, True])
def test_sliced_equals_whole(batch, slice_pairs, forced):
    masks = _spec_masks(batch, per_row_flips=3) if forced else None
    whole = U.oracle_step(SEED, batch, torch.float64, masks)
    part = U.oracle_step(SEED, batch, torch.float64, masks, slice_pairs=slice_pairs)
    worst = max(_rel(g, w) for (_, g), (_, w) in zip(part["grads"], whole["grads"]))
    print(f"float64, slices of {slice_pairs}, forced {forced}: loss difference {abs(part['loss'] - whole['loss']):.1e}, "
          f"worst of {len(whole['grads'])} gradient tensors {worst:.1e} relL2; {whole['flips']} decisions forced")
    assert len(whole["grads"]) == 58 and [n for n, _ in part["grads"]] == [n for n, _ in whole["grads"]]
    assert abs(part["loss"] - whole["loss"]) <= 1e-12
    for (n, g), (_, w) in zip(part["grads"], whole["grads"]):
        assert w.abs().max().item() > 0, n
        assert _rel(g, w) <= 1e-12, (n, _rel(g, w))
    for k in ("d_t", "d_r", "pose", "a", "b"):
        assert part[k].shape == whole[k].shape and (part[k] - whole[k]).abs().max().item() <= 1e-12, k
    if forced:
        # 3 per row and layer by hand, of which float64 takes a few by itself (they are the most marginal of the fp32 run), plus
        # what it decides the other way than fp32 anyway; counted once, not once per sweep
        by_hand = 3 * (2 * B * 20 + B * 7)
        assert by_hand // 2 <= whole["flips"] == part["flips"] <= 2 * by_hand, (whole["flips"], part["flips"])
        assert part["flip_worst"] == whole["flip_worst"] > 0
    else:
        assert whole["flips"] == part["flips"] == 0
    # float32: the same sums in another order (and, unforced, the odd ReLU decided the other way) -- printed, not asserted
    w32 = U.oracle_step(SEED, batch, torch.float32, masks)
    p32 = U.oracle_step(SEED, batch, torch.float32, masks, slice_pairs=slice_pairs)
    print(f"float32 sliced vs whole: loss {abs(p32['loss'] - w32['loss']):.1e}, worst tensor "
          f"{max(_rel(g, w) for (_, g), (_, w) in zip(p32['grads'], w32['grads'])):.1e} relL2")


def test_bf16_oracle_sliced_equals_whole(batch, free_masks):
    """The bf16 target and its emulated-storage noise run take the same path: same step in slices, to float32 summation order."""
    for emulate in (False, True):
        whole = U.oracle_step_bf16(SEED, batch, free_masks, emulate=emulate)
        part = U.oracle_step_bf16(SEED, batch, free_masks, emulate=emulate, slice_pairs=2)
        worst = max(_rel(g, w) for (_, g), (_, w) in zip(part["grads"], whole["grads"]))
        print(f"bf16 oracle (emulate {emulate}) sliced vs whole: loss {abs(part['loss'] - whole['loss']):.1e}, worst tensor {worst:.1e}")
        # Not emulated: float32 sums in another order, ~1e-6 of a tensor's norm (the fp32 oracle's own distance from float64 at
        # this size); 1e-4 is a hundred times that.  Emulated: a last-bit difference in front of a bf16 rounding point moves that
        # element by a whole bf16 step (2^-8 of it), so the two runs are two partly different draws of the storage noise the run
        # exists to measure (0.5-1.5 % of a tensor's norm): 1e-3, a tenth of it.  A wrong mask row or normaliser moves a tensor by
        # tens of percent (below).
        assert abs(part["loss"] - whole["loss"]) <= 1e-6 and worst <= (1e-3 if emulate else 1e-4)


def test_full_loss_is_unsliced_only(batch):
    with pytest.raises(ValueError):
        U.oracle_step(SEED, batch, torch.float64, slice_pairs=2, full_loss=True)
    whole = U.oracle_step(SEED, batch, torch.float64, full_loss=True)
    dn, pn = S.make_models(SEED, dtype=torch.float64)
    t = lambda v: v.double()
    loss = S.dcdp_forward(dn, pn, t(batch["tgt"]), t(batch["ref"]), t(batch["K"]), full_loss=True)[0]
    assert abs(whole["loss"] - loss.item()) <= 1e-12 and abs(whole["loss"] - U.oracle_step(SEED, batch, torch.float64)["loss"]) > 1e-3


def _stand_in(batch, masks, normaliser=None, drop=None):
    """The sliced fp32 step as the path under test.  drop = (layer of DepthNet, frame): that frame's contribution is taken out of
    the layer's weight and bias gradient -- exactly what a weight-gradient kernel that skips one image leaves -- and nothing else
    changes (the input gradient still flows)."""
    dn, pn = S.make_models(SEED)
    rows = U._Rows()
    seen = {}
    for tag, net in (("depth", dn), ("pose", pn)):
        for name, mod in net.named_children():
            m = masks.get(f"{tag}.{name}")
            if m is None:
                continue

            def hook(mod, inp, out, m=m, tag=tag, name=name):
                mm = rows.of(m, tag)
                flip = (out > 0) != mm
                out = U._forced(out, mm, flip) if bool(flip.any()) else out
                if drop is not None and rows.count and (tag, name) == ("depth", drop[0]):
                    k = rows.k
                    frames = list(range(rows.s, rows.s + k)) + list(range(B + rows.s, B + rows.s + k))
                    if drop[1] in frames:
                        j = frames.index(drop[1])
                        seen["x"] = inp[0][j:j + 1].detach()
                        out.register_hook(lambda g: seen.__setitem__("dy", g[j:j + 1].detach()))
                return out
            mod.register_forward_hook(hook)
    loss = U._coupled_step(dn, pn, batch["tgt"], batch["ref"], batch["K"], rows, 2, False, normaliser)[0]
    if drop is not None:
        mod = getattr(dn, drop[0])
        dw = torch.nn.grad.conv2d_weight(seen["x"], mod.weight.shape, seen["dy"], stride=mod.stride, padding=mod.padding)
        mod.weight.grad -= dw
        mod.bias.grad -= seen["dy"].sum(dim=(0, 2, 3))
    return loss, U._named_grads(dn, pn)


@pytest.fixture(scope="module")
def yardsticks(batch, free_masks):
    return U.oracle_step(SEED, batch, torch.float32, free_masks), U.oracle_step(SEED, batch, torch.float64, free_masks)


def test_the_bar_passes_the_sliced_step_and_sees_a_missing_image_and_a_wrong_normaliser(batch, free_masks, yardsticks):
    o32, o64 = yardsticks
    failing = lambda grads: {line.split(":")[0] for line in U.grad_parity_failures(U.grad_parity_table(grads, o32["grads"], o64["grads"]))}
    rows = U.grad_parity_table(_stand_in(batch, free_masks)[1], o32["grads"], o64["grads"])
    print(f"control: sliced fp32 step, worst tensor {max(r[5] for r in rows):.2e} relL2 from float64 (whole fp32 oracle "
          f"{max(r[6] for r in rows):.2e}); failing: {U.grad_parity_failures(rows)}")
    assert not U.grad_parity_failures(rows)

    # one of the 12 frames (target frame of pair 3: second slice) missing from one mid layer's weight gradient
    _, grads = _stand_in(batch, free_masks, drop=(MID, 3))
    moved = {n: _rel(g, w) for (n, g), (_, w) in zip(grads, o64["grads"])}
    bad = failing(grads)
    print(f"one frame of {2 * B} missing from depth.{MID}'s weight gradient: weight {moved[f'depth.{MID}.weight']:.2e}, bias "
          f"{moved[f'depth.{MID}.bias']:.2e} relL2 from float64; failing: {sorted(bad)}")
    assert bad == {f"depth.{MID}.weight", f"depth.{MID}.bias"}

    # the normaliser of slice 0 alone instead of the batch's: every gradient ~3 x too large
    loss, grads = _stand_in(batch, free_masks, normaliser=lambda counts, i: counts[0])
    bad = failing(grads)
    print(f"normaliser from slice 0 alone: loss {loss:.6f} vs {o64['loss']:.6f}; {len(bad)} of 58 tensors fail")
    assert len(bad) == 58
