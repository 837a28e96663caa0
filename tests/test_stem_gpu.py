"""-m gpu: DepthNet's stem as one launch (csrc/stem.hip, tuning `stem_fused`) against the three launches it replaces:
colvo_pack_stem_pose, enc1a (8 -> 32, stride 2) and enc1b (32 -> 32) through colvo_conv_fwd.

The launch must give the same BITS in all four tensors it writes -- the packed stem input, the frame channels of PoseNet's input,
enc1a and enc1b -- torch.equal against the plain launches in one process.  Every destination comes from tests/guarded.py's pool:
poisoned with 0xFF bytes (NaN in bf16) between guard bands, so an element the kernel leaves unwritten shows, and so does a byte
written outside the tensor; the frames, weights and biases are guarded copies, so a tap outside a frame reads NaN.  The plain calls' form
counters say that the references are the forms the bits are tied to.  Frame sizes (2 and 3 pairs of each):
    32 x 48     enc1 maps of 16 x 24: several tiles, none ragged
    36 x 52     18 x 26: the planner's tile adapts to it (9 x 13: odd tile width, 117 pixels, the last fragments partly empty)
    46 x 58     23 x 29: 8 x 16 tiles, ragged in both directions
    16 x 16     8 x 8: one tile, every halo pixel outside the image
each with the planner's grid (one round) and with `stem_max_wgs` lowered to 3 workgroups, where the persistent walk and the register
prefetch take a second and third round wherever there are more pair tiles than that.
Frames have both signs, and a third of their elements sit exactly half way between two bf16 values (round-to-nearest-even ties, with
even and odd neighbours).  enc1a's bias is about +2 in every channel: enc1a evaluated one pixel off the map -- on a patch of zeros
-- would be relu(bias) > 0, so a halo that is computed instead of zeroed changes enc1b's border pixels."""
import pytest
import torch

from coivo_amd import _lib, ops
from tests import conv_exact as X
from tests import guarded
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

SIZES = [(32, 48), (36, 52), (46, 58), (16, 16)]
PAIRS = (2, 3)


class _tune:
    """tuning entries set for a block; what they were afterwards (the tests share one process)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.saved = {k: _lib.tune_get(k) for k in self.kv}
        for k, v in self.kv.items():
            _lib.tune_set(k, v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            _lib.tune_set(k, v)
        return False


def _descs(pairs, H, W):
    da = ops.conv_desc(torch.bfloat16, 2 * pairs, H, W, 8, 32, stride=2)
    return da, ops.conv_desc(torch.bfloat16, 2 * pairs, da.Ho, da.Wo, 32, 32)


def _pack(wm):
    cout, _, cin = wm.shape
    w_fwd = torch.empty(cout, 9, cin, device=wm.device, dtype=torch.bfloat16)
    w_bwd = torch.empty(cin, 9, cout, device=wm.device, dtype=torch.bfloat16)
    ops.pack_weights(wm, torch.bfloat16, w_fwd, w_bwd)
    return w_fwd


def _dests(pairs, H, W, da):
    """(pool, the four destinations): bf16 tensors of NaN between guard bands."""
    B = 2 * pairs
    pool = guarded.Pool(dev())
    shapes = ((B, H, W, 8), (pairs, H, W, 8), (B, da.Ho, da.Wo, 32), (B, da.Ho, da.Wo, 32))
    return pool, [pool.empty(shape, torch.bfloat16, label=name) for shape, name in zip(shapes, NAMES)]


NAMES = ("stem input", "PoseNet input", "enc1a", "enc1b")
OPERANDS = ("frames", "enc1a weights", "enc1a bias", "enc1b weights", "enc1b bias")


def _plain(da, db, frames, w1, b1, w2, b2):
    """The three launches, into guarded poisoned destinations; the form counters of the two conv calls."""
    pairs, (_, _, H, W) = da.B // 2, frames.shape
    pool, out = _dests(pairs, H, W, da)
    frames, w1, b1, w2, b2 = (pool.place(t, n) for t, n in zip((frames, w1, b1, w2, b2), OPERANDS))
    ops.pack_stem_pose(frames, out[0], out[1])
    forms = []
    for d, x, w, b, y in ((da, out[0], w1, b1, out[2]), (db, out[2], w2, b2, out[3])):
        before = _lib.form_counts()
        ops.conv_fwd(d, x, None, w, b, y)
        torch.cuda.synchronize()
        forms.append(X.forms_diff(before, _lib.form_counts()))
    pool.check("the three launches")
    return out, forms


def _fused(da, frames, w1, b1, w2, b2):
    pairs, (_, _, H, W) = da.B // 2, frames.shape
    pool, out = _dests(pairs, H, W, da)
    frames, w1, b1, w2, b2 = (pool.place(t, n) for t, n in zip((frames, w1, b1, w2, b2), OPERANDS))
    before = _lib.form_counts()
    ops.stem_fused(da, frames, out[0], out[1], w1, b1, out[2], w2, b2, out[3])
    torch.cuda.synchronize()
    assert _lib.form_counts() == before                                 # the launch counts no form
    pool.check("the fused stem")                                         # no byte outside a destination or an operand was written
    return out


def _bits_equal(ref, got, what):
    for name, r, y in zip(NAMES, ref, got):
        assert not bool(torch.isnan(y).any()) and not bool(torch.isnan(r).any()), f"{what}: {name} has unwritten elements"
        ri, yi = r.view(torch.int16), y.view(torch.int16)
        assert torch.equal(ri, yi), f"{what}: {name}: {int((ri != yi).sum())} of {ri.numel()} elements differ"


def _frames(pairs, H, W, g):
    """fp32 frames with both signs; every third element is an exact tie between two bf16 values (low 16 bits 0x8000)."""
    f = torch.randn(2 * pairs, 3, H, W, generator=g, device=dev())
    bits = f.view(torch.int32)
    tie = (torch.arange(f.numel(), device=dev()).view(f.shape) % 3) == 0
    bits.copy_(torch.where(tie, (bits & -65536) | 0x8000, bits))
    assert bool((f < 0).any()) and bool((f > 0).any())
    hi = (bits[tie] >> 16) & 1
    assert bool((hi == 0).any()) and bool((hi == 1).any())              # ties with an even and with an odd neighbour below
    return f


def _operands(g, bias1=2.0):
    w1 = _pack(torch.randn(32, 9, 8, generator=g, device=dev()) * (2.0 / 27) ** 0.5)
    w2 = _pack(torch.randn(32, 9, 32, generator=g, device=dev()) * (2.0 / 288) ** 0.5)
    b1 = torch.randn(32, generator=g, device=dev()) * 0.3 + bias1
    b2 = torch.randn(32, generator=g, device=dev()) * 0.3 - 1.0
    return w1, b1, w2, b2


@pytest.mark.parametrize("wgs", [0, 3])
@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("H,W", SIZES)
def test_the_launch_gives_the_bits_of_the_three_launches(H, W, pairs, wgs):
    g = torch.Generator(device=dev()).manual_seed(1000 * pairs + H + W)
    da, db = _descs(pairs, H, W)
    frames = _frames(pairs, H, W, g)
    w1, b1, w2, b2 = _operands(g)
    assert float(b1.min()) > 0.5                                         # enc1a off the map would be relu(bias) > 0 in every channel
    ref, forms = _plain(da, db, frames, w1, b1, w2, b2)
    # the references really are the forms the bits are tied to
    assert forms[0] in ({"conv_tile": 1}, {"conv_res_s2": 1}) and forms[1] in ({"conv_tile": 1}, {"conv_res": 1}), forms
    with _tune(**({"stem_max_wgs": wgs} if wgs else {})):
        plan = ops.stem_plan(da)
        assert plan is not None and plan[3] <= 160 * 1024, plan
        nwg, toh, tow, _ = plan
        items = pairs * (-(-da.Ho // toh)) * (-(-da.Wo // tow))
        print(f"stem {pairs} pairs of {H}x{W}: tile {toh}x{tow}, {items} pair tiles on {nwg} workgroups, LDS {plan[3]}")
        if wgs:
            assert nwg <= wgs
            if (H, W) != (16, 16):
                assert items > nwg                                           # a second round of the walk (a third for most)
        else:
            assert nwg == items
        if (H, W) == (16, 16):
            assert toh * tow == 64 and items == pairs                       # one tile: the whole halo lies outside the image
        if (H, W) == (36, 52):
            assert toh * tow < 128 and tow % 2                               # an odd, partly filled tile
        if (H, W) == (46, 58):
            assert da.Ho % toh and da.Wo % tow                               # ragged in both directions
        got = _fused(da, frames, w1, b1, w2, b2)
    _bits_equal([r for r in ref], got, f"{pairs} pairs of {H}x{W}, {nwg} workgroups")
    # the border of enc1b depends on the halo being zero: with a halo of relu(bias) it would differ from this reference
    frac = float((ref[3] == 0).float().mean())
    assert 0.02 < frac < 0.98, f"enc1b's ReLU mask is not mixed ({frac:.2f} zeros)"


def test_the_frame_channels_are_the_rounded_frames():
    """The packed tensors by their definition (independent of colvo_pack_stem_pose): round-to-nearest-even of the frames, ties included;
    channels 3..7 of the stem input and 6, 7 of PoseNet's input are zero."""
    pairs, H, W = 2, 32, 48
    g = torch.Generator(device=dev()).manual_seed(5)
    da, _ = _descs(pairs, H, W)
    frames = _frames(pairs, H, W, g)
    got = _fused(da, frames, *_operands(g))
    want = frames.to(torch.bfloat16).permute(0, 2, 3, 1)                  # torch rounds to nearest even
    assert torch.equal(got[0][..., :3], want) and not bool(got[0][..., 3:].any())
    assert torch.equal(got[1][..., :3], want[:pairs]) and torch.equal(got[1][..., 3:6], want[pairs:])
    assert not bool(got[1][..., 6:].any())


@pytest.mark.parametrize("pairs,H,W", [(2, 36, 52), (3, 32, 48)])
def test_both_layers_are_exact_on_exact_data(pairs, H, W):
    """tests/conv_exact.py's sources, weights, biases, float64 reference and comparison.  enc1a's weights are drawn from [-2, 2]
    quanta: its pre-activations are then at most 9 x 3 x 3 x 2 + 16 = 178 < 256 quanta of 2^-6, so the stored bf16 map is EXACT and
    enc1b's input is exact data again -- 9 x 32 products of at most 178 x 8 quanta of 2^-10 plus the bias, far below 2^24."""
    g = torch.Generator(device=dev()).manual_seed(11 + pairs)
    da, db = _descs(pairs, H, W)
    B = 2 * pairs
    frames = X.make_source((B, 3, H, W), g, dev())
    wm1 = torch.randint(-2, 3, (32, 9, 8), generator=g, device=dev(), dtype=torch.int32).float() * X.QW
    wm2 = X.make_weights(32, 32, g, dev())
    b1, b2 = X.make_bias(32, g, dev()), X.make_bias(32, g, dev())
    assert 9 * 3 * X.X_MAX * 2 + X.B_MAX < 256 and 9 * 32 * 178 * X.W_MAX + X.B_MAX * 16 < 2 ** 24
    x8 = torch.zeros(B, H, W, 8, device=dev())
    x8[..., :3] = frames.permute(0, 2, 3, 1)
    want1 = X.Layer.of_desc(da).ref_fwd(x8, None, wm1, b1, 0, B)
    got = _fused(da, frames, _pack(wm1), b1, _pack(wm2), b2)
    X.expect_exact(got[2], want1, X.QB, "enc1a inside the fused stem")
    assert torch.equal(got[2].double(), want1)                          # ... and exact in bf16: enc1b's input is exact data
    want2 = X.Layer.of_desc(db).ref_fwd(got[2].float(), None, wm2, b2, 0, B)
    X.expect_exact(got[3], want2, X.QB * X.QW, "enc1b inside the fused stem")
    ref, _ = _plain(da, db, frames, _pack(wm1), b1, _pack(wm2), b2)
    _bits_equal(ref, got, "exact data")


def _depth_step(dn, frames, entry, seed):
    """One DepthNet pair pass forward + backward with fixed output gradients -> (outputs, PoseNet's input, the whole gradient arena)."""
    g = torch.Generator(device=dev()).manual_seed(seed)
    B = frames.shape[0] // 2
    dn.zero_grad()
    if entry == "forward_pair":
        d_t, d_r = dn.forward_pair(frames)
        outs = [d_t, d_r]
    else:
        d = dn(frames)
        outs = [d[:B], d[B:]]
    pose_in = outs[0]._colvo_pose_in[0]                                  # (the pass filled it: both entries are pair passes)
    grads = [torch.randn(o.shape, generator=g, device=dev()) for o in outs]
    torch.autograd.backward(outs, grads)
    dn.join_side()
    torch.cuda.synchronize()
    return [o.detach().clone() for o in outs] + [pose_in.clone()], dn.flat_grad.clone()


@pytest.mark.parametrize("entry", ["forward_pair", "forward"])
def test_depthnet_step_is_the_same_with_the_stem(entry):
    """nn level, deterministic mode, 2 pairs of 64 x 96: outputs, PoseNet's input and the whole gradient arena with the switch on and
    off, and two runs with it on.  The recorded forward pass is keyed by the planner's answer: with the switch on its first command
    is the stem form of CMD_PACK_STEM_POSE and enc1a's and enc1b's CMD_CONV_FWD are gone."""
    from coivo_amd import nn as hnn
    pairs, H, W = 2, 64, 96
    g = torch.Generator(device=dev()).manual_seed(17)
    dn = hnn.DepthNet(compute_dtype=torch.bfloat16)
    dn.deterministic = True
    with torch.no_grad():
        dn.flat_param.copy_(torch.randn(dn.flat_param.shape, generator=g, device=dev()) * 0.05)
    dn.mark_params_changed()
    frames = torch.rand(2 * pairs, 3, H, W, generator=g, device=dev())
    with _tune(stem_fused=0):
        off = _depth_step(dn, frames, entry, 3)
    with _tune(stem_fused=1):
        on1 = _depth_step(dn, frames, entry, 3)
        on2 = _depth_step(dn, frames, entry, 3)
    assert sorted(k[5] for k in dn._insts) == [False, True]
    listing = {}
    for key, insts in dn._insts.items():
        pr = insts[0].passes["fwd"][0]
        listing[key[5]] = [(pr._arr[ci].op, bool(pr._arr[ci].p[3]), pr._arr[ci].desc.C0, pr._arr[ci].desc.Cout) for ci in range(len(pr))]
    head_on, head_off = listing[True][0], listing[False][0]
    assert head_on[:2] == (_lib.CMD_PACK_STEM_POSE, True) and head_off[:2] == (_lib.CMD_PACK_STEM_POSE, False)
    conv = lambda rows: [r[2:] for r in rows if r[0] == _lib.CMD_CONV_FWD]
    assert conv(listing[False])[:2] == [(8, 32), (32, 32)] and conv(listing[False])[2:] == conv(listing[True])
    assert len(listing[True]) == len(listing[False]) - 2
    assert float(off[1].abs().max()) > 0
    for name, a, b in (("off / on", off, on1), ("on / on", on1, on2)):
        for x, y in zip(a[0] + [a[1]], b[0] + [b[1]]):
            assert torch.equal(x, y), name


def test_a_request_is_refused_where_the_stem_is_not_selected():
    """No quiet fall-back: a request at a shape the planner does not select is an error."""
    pairs, H, W = 2, 32, 48
    g = torch.Generator(device=dev()).manual_seed(23)
    da, _ = _descs(pairs, H, W)
    frames = _frames(pairs, H, W, g)
    ops_ = _operands(g)
    pool, out = _dests(pairs, H, W, da)
    with _tune(stem_fused=0):
        assert ops.stem_plan(da) is None
        with pytest.raises(RuntimeError, match="the fused stem is not selected"):
            ops.stem_fused(da, frames, out[0], out[1], ops_[0], ops_[1], out[2], ops_[2], ops_[3], out[3])
    pool.check("a refused request")
    assert all(bool((o.view(torch.uint8) == guarded.GUARD_BYTE).all()) for o in out)           # ... and nothing inside them either
