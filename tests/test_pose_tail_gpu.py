"""-m gpu: PoseNet's conv5-conv7 as whole-K resident launches (csrc/pose_tail.hip, tuning `pose_tail` / `pose_tail_bwd`) against the
launches they replace.

The form must give the same BITS: torch.equal with the request on and the plain call in one process, on random data with both signs
(mixed ReLU masks), random weights and non-zero biases; destinations are pre-filled with a sentinel so that an element the kernel
leaves unwritten shows.  The plain call's form counters say that the reference really is the form the bits are tied to: k_conv3x3
(one chunk in flight or the two-chunk ring) forward; k_dgrad_s2, or k_conv3x3 over the zero-dilated dy, backward.  Inputs are conv4's
output maps for these image sizes (pairs x H x W):
    1 x 32 x 32     maps 2x2 -> 1x1 -> 1x1 -> 1x1: everything is padding
    2 x 64 x 96     4x6 -> 2x3 -> 1x2 -> 1x1
    3 x 96 x 160    6x10 -> 3x5 -> 2x3 -> 1x2: odd batch, odd widths; with several images per workgroup a fragment spans images and
                    the last workgroup's group of images is ragged
    8 x 256 x 320   the benchmark's maps, 16x20 -> 8x10 -> 4x5 -> 2x3
    24 x 256 x 320  the largest pair count under the ceiling (tuning `pose_tail_max_pairs`): 384 workgroups at one image each, so
                    the planner takes two images per workgroup where they fit
Every case runs with the planner's own images per workgroup and with 2, 3 and 8 forced (tuning `pose_tail_images`) wherever those fit.
On exact data (tests/conv_exact.py) every sum is representable, so the forward form must also match the float64 reference bit for
bit."""
import pytest
import torch

from coivo_amd import _lib, ops
from tests import conv_exact as X
from tests import guarded
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

_guarded = guarded.fixture(dev)          # every test here allocates from tests/guarded.py's pool; the guards are checked at its end

SHAPES = [(1, 32, 32), (2, 64, 96), (3, 96, 160), (8, 256, 320), (24, 256, 320)]
CH = (128, 256, 256, 256)                 # conv4's output, conv5, conv6, conv7
SENTINEL = 77.0
IMAGES = (0, 2, 3, 8)                     # 0: the planner's choice


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


def _switch(on):
    return _tune(pose_tail=1 if on else 0)


def _descs(B, H, W):
    out, h, w = [], H // 16, W // 16
    for i in range(3):
        out.append(ops.conv_desc(torch.bfloat16, B, h, w, CH[i], CH[i + 1], stride=2))
        h, w = out[-1].Ho, out[-1].Wo
    return out


def _pack(wm):
    cout, _, cin = wm.shape
    w_fwd = torch.empty(cout, 9, cin, device=wm.device, dtype=torch.bfloat16)
    w_bwd = torch.empty(cin, 9, cout, device=wm.device, dtype=torch.bfloat16)
    ops.pack_weights(wm, torch.bfloat16, w_fwd, w_bwd)
    return w_fwd, w_bwd


def _bits_equal(r, y, what):
    assert not bool((r == SENTINEL).any()), what
    assert torch.equal(r.view(torch.int16), y.view(torch.int16)), \
        f"{what}: {int((r.view(torch.int16) != y.view(torch.int16)).sum())} of {r.numel()} elements differ"


def _fwd_both(d, x, w_fwd, bias):
    """(the plain colvo_conv_fwd launch, [(images per workgroup, the whole-K launch)]), every destination pre-filled."""
    mk = lambda: torch.full((d.B, d.Ho, d.Wo, d.Cout), SENTINEL, device=x.device, dtype=torch.bfloat16)
    ref = mk()
    before = _lib.form_counts()
    ops.conv_fwd(d, x, None, w_fwd, bias, ref)
    torch.cuda.synchronize()
    diff = X.forms_diff(before, _lib.form_counts())
    assert diff in ({"conv_tile": 1}, {"conv_ring": 1}), diff          # the reference really is the form the bits are tied to
    got = []
    for images in IMAGES:
        with _tune(pose_tail_images=images):
            plan = ops.pose_tail_plan(d)
            if images == 0:
                assert plan is not None and plan[2] <= 160 * 1024
            if plan is None:                                            # that many images do not fit in LDS
                continue
            y = mk()
            before = _lib.form_counts()
            ops.conv_fwd(d, x, None, w_fwd, bias, y, whole_k=True)
            torch.cuda.synchronize()
            assert _lib.form_counts() == before                         # the form counts nothing
            got.append((plan[1], y))
    return ref, got


@pytest.mark.parametrize("layer", [5, 6, 7])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_forward_gives_the_bits_of_the_plain_launch(B, H, W, layer):
    g = torch.Generator(device=dev()).manual_seed(B * 1000 + H + layer)
    d = _descs(B, H, W)[layer - 5]
    cin, cout = d.C0, d.Cout
    x = torch.randn(B, d.Hi, d.Wi, cin, generator=g, device=dev()).to(torch.bfloat16)
    w_fwd, _ = _pack(torch.randn(cout, 9, cin, generator=g, device=dev()) * (2.0 / (9 * cin)) ** 0.5)
    bias = torch.randn(cout, generator=g, device=dev()) * 0.3
    ref, got = _fwd_both(d, x, w_fwd, bias)
    frac = float((ref == 0).float().mean())
    assert 0.05 < frac < 0.95, f"conv{layer}: the ReLU mask is not mixed ({frac:.2f} zeros)"
    assert got and got[0][0] >= 1
    for images, y in got:
        _bits_equal(ref, y, f"conv{layer} forward at {B}x{H}x{W}, {images} images per workgroup")


@pytest.mark.parametrize("layer", [5, 6, 7])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_input_gradient_gives_the_bits_of_the_plain_launch(B, H, W, layer):
    """dx = dgrad(dy) masked by the producing activation > 0 (random, both signs), as nn.PoseNet calls it."""
    g = torch.Generator(device=dev()).manual_seed(B * 1000 + W + layer)
    d = _descs(B, H, W)[layer - 5]
    cin, cout = d.C0, d.Cout
    dy = torch.randn(B, d.Ho, d.Wo, cout, generator=g, device=dev()).to(torch.bfloat16)
    act = torch.randn(B, d.Hi, d.Wi, cin, generator=g, device=dev()).to(torch.bfloat16)
    _, w_bwd = _pack(torch.randn(cout, 9, cin, generator=g, device=dev()) * 0.1)
    ref = torch.full_like(act, SENTINEL)
    before = _lib.form_counts()
    ops.conv_dgrad(d, 0, dy, w_bwd, act, ref, False)
    torch.cuda.synchronize()
    diff = X.forms_diff(before, _lib.form_counts())
    plan0 = ops.pose_tail_plan(d, 1)
    assert plan0 is not None and plan0[2] <= 160 * 1024
    # the reference really is the form the bits are tied to, and the planner read the same one
    even = d.Hi == 2 * d.Ho and d.Wi == 2 * d.Wo
    assert diff in (({"dgrad_s2": 1}, {"dgrad_s2_ring": 1}) if even else ({"conv_tile": 1}, {"conv_ring": 1})), diff
    assert plan0[3] == (1 if even else 0)
    frac = float((ref == 0).float().mean())
    assert 0.2 < frac < 0.8, f"conv{layer}: the ReLU mask is not mixed ({frac:.2f} zeros)"
    ran = 0
    for images in IMAGES:
        with _tune(pose_tail_images=images):
            plan = ops.pose_tail_plan(d, 1)
            if plan is None:
                continue
            dx = torch.full_like(act, SENTINEL)
            before = _lib.form_counts()
            ops.conv_dgrad(d, 0, dy, w_bwd, act, dx, False, whole_k=True)
            torch.cuda.synchronize()
            assert _lib.form_counts() == before
            _bits_equal(ref, dx, f"conv{layer} input gradient at {B}x{H}x{W}, {plan[1]} images per workgroup")
            ran += 1
    assert ran >= 1


@pytest.mark.parametrize("B,H,W", [(3, 96, 160), (8, 256, 320)])
def test_forward_is_exact_on_exact_data(B, H, W):
    """tests/conv_exact.py's sources, weights, biases, float64 reference and comparison, each layer on a fresh exact source: at most
    9 x 256 products of at most 24 quanta and a bias of at most 16 (bound_fwd), far below 2^24, so every partial sum is exact in fp32
    whatever the order and the stored bf16 is one rounding of the exact value."""
    g = torch.Generator(device=dev()).manual_seed(7 + B)
    for layer, d in zip((5, 6, 7), _descs(B, H, W)):
        assert X.bound_fwd(d.C0) < 2 ** 24
        xf = X.make_source((B, d.Hi, d.Wi, d.C0), g, dev())
        wm = X.make_weights(d.Cout, d.C0, g, dev())
        bias = X.make_bias(d.Cout, g, dev())
        ref, got = _fwd_both(d, xf.to(torch.bfloat16), _pack(wm)[0], bias)
        want = X.Layer.of_desc(d).ref_fwd(xf, None, wm, bias, 0, B)
        for images, y in got:
            X.expect_exact(y, want, X.QB, f"conv{layer} whole-K forward, {images} images per workgroup")
            assert torch.equal(ref, y)


# The mask decision every bf16 input gradient shares (csrc/conv_lane.h relu_mask_keep): the producer's value is > 0, read off its
# bits.  Real activations are >= 0, so the tests above never show the kernels a set sign bit, a denormal or a NaN.
MASK_PATTERNS = (0x0000, 0x8000, 0x0001, 0x8001, 0x3F80, 0xBF80, 0x7FC0, 0xFFC0)      # +0, -0, +-denormal, +-1, +-NaN


def _mask_case(name):
    """(descriptor, whole-K request, the form counters one plain launch moves or the whole-K kernel kind) at the smallest shape
    where the form is selected."""
    bf = torch.bfloat16
    if name == "k_conv3x3":                     # one tile, one 32-channel chunk
        return ops.conv_desc(bf, 1, 8, 8, 32, 32), False, ({"conv_tile": 1},)
    if name == "k_dgrad_s2":
        return ops.conv_desc(bf, 1, 8, 8, 32, 32, stride=2), False, ({"dgrad_s2": 1},)
    if name == "k_conv_rt":                     # 16 x 16 tiles x 64 channels x 4 images = rt_min_wgs workgroups, two chunks
        assert _lib.tune_get("rt_min_wgs") == 1024 and _lib.tune_get("rt_min_chunks") == 2
        return ops.conv_desc(bf, 4, 256, 256, 64, 64), False, ({"conv_rt": 1},)
    t = _descs(*SHAPES[0])                      # conv5: 2 x 2 -> 1 x 1, k_dgrad_s2's order; conv6: 1 x 1 -> 1 x 1, k_conv3x3's
    return (t[0], True, 1) if name == "k_conv_wholek dgrad_s2" else (t[1], True, 0)


@pytest.mark.parametrize("name", ["k_conv3x3", "k_dgrad_s2", "k_conv_rt", "k_conv_wholek conv", "k_conv_wholek dgrad_s2"])
def test_the_relu_mask_keeps_exactly_the_positive_bit_patterns(name):
    """One input gradient with a mask that cycles through MASK_PATTERNS and one without a mask: the masked result has the unmasked
    bits where the mask's pattern has the sign clear and a non-zero magnitude (numpy, from the mask's uint16 view) and +0 elsewhere."""
    import numpy as np
    d, whole_k, form = _mask_case(name)
    g = torch.Generator(device=dev()).manual_seed(len(name))
    dy = torch.randn(d.B, d.Ho, d.Wo, d.Cout, generator=g, device=dev()).to(torch.bfloat16)
    _, w_bwd = _pack(torch.randn(d.Cout, 9, d.C0, generator=g, device=dev()) * 0.1)
    n = d.B * d.Hi * d.Wi * d.C0
    flat = np.arange(n, dtype=np.int64)
    pat = np.array(MASK_PATTERNS, dtype=np.uint16)[(flat + flat // d.C0) % len(MASK_PATTERNS)]     # shifts by one from pixel to pixel
    mask = torch.from_numpy(pat.view(np.int16)).to(dev()).view(torch.bfloat16).view(d.B, d.Hi, d.Wi, d.C0)
    if whole_k:
        plan = ops.pose_tail_plan(d, 1)
        assert plan is not None and plan[3] == form, plan
    out = []
    for m in (None, mask):
        dx = torch.full((d.B, d.Hi, d.Wi, d.C0), SENTINEL, device=dev(), dtype=torch.bfloat16)
        before = _lib.form_counts()
        ops.conv_dgrad(d, 0, dy, w_bwd, m, dx, False, whole_k=whole_k)
        torch.cuda.synchronize()
        diff = X.forms_diff(before, _lib.form_counts())
        assert (diff == {}) if whole_k else (diff in form), diff
        out.append(dx.view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1))
    plain, masked = out
    u = mask.view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)
    keep = ((u & 0x8000) == 0) & ((u & 0x7FFF) != 0)
    assert np.unique(u).tolist() == sorted(MASK_PATTERNS) and 0 < keep.sum() < n
    sentinel = np.uint16(torch.tensor(SENTINEL, dtype=torch.bfloat16).view(torch.int16).item() & 0xFFFF)
    assert not (plain == sentinel).any() and not (masked == sentinel).any()
    for p in MASK_PATTERNS:                     # every pattern decides over some non-zero gradients
        assert ((plain[u == p] & 0x7FFF) != 0).any(), hex(p)
    want = np.where(keep, plain, np.uint16(0))
    bad = np.flatnonzero(masked != want)
    assert bad.size == 0, f"{name}: {bad.size} of {n} elements; first at {bad[0]}: mask {u[bad[0]]:#06x}, unmasked " \
                          f"{plain[bad[0]]:#06x}, masked {masked[bad[0]]:#06x}"


def _pose_step(pn, batch, seed):
    """One PoseNet forward + backward with fixed output gradients -> (outputs, depth gradients, the whole gradient arena)."""
    g = torch.Generator(device=dev()).manual_seed(seed)
    tgt, ref, d_t, d_r = batch
    d_t = d_t.clone().requires_grad_(True)
    d_r = d_r.clone().requires_grad_(True)
    pn.zero_grad()
    pose, a, b = pn(tgt, ref, d_t, d_r)
    gp = torch.randn(pose.shape, generator=g, device=dev())
    ga = torch.randn(a.shape, generator=g, device=dev())
    gb = torch.randn(b.shape, generator=g, device=dev())
    torch.autograd.backward([pose, a, b], [gp, ga, gb])
    pn.join_side()
    torch.cuda.synchronize()
    return ([t.detach().clone() for t in (pose, a, b)], [d_t.grad.clone(), d_r.grad.clone()], pn.flat_grad.clone())


@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (8, 256, 320)])
def test_posenet_step_is_the_same_with_the_form(B, H, W):
    """nn level, deterministic mode: outputs, depth gradients and the whole gradient arena with the switch on and off, and two runs
    with it on.  The recorded passes are keyed by the planner's answers, so one network serves both settings."""
    from coivo_amd import nn as hnn
    g = torch.Generator(device=dev()).manual_seed(13)
    pn = hnn.PoseNet(compute_dtype=torch.bfloat16)
    pn.deterministic = True
    with torch.no_grad():
        pn.flat_param.copy_(torch.randn(pn.flat_param.shape, generator=g, device=dev()) * 0.08)
    pn.mark_params_changed()
    batch = (torch.rand(B, 3, H, W, generator=g, device=dev()), torch.rand(B, 3, H, W, generator=g, device=dev()),
             torch.rand(B, 1, H, W, generator=g, device=dev()) * 5 + 0.1, torch.rand(B, 1, H, W, generator=g, device=dev()) * 5 + 0.1)
    with _switch(False):
        off = _pose_step(pn, batch, 3)
    with _switch(True):
        on1 = _pose_step(pn, batch, 3)
        on2 = _pose_step(pn, batch, 3)
    # both settings were recorded, forward and backward: all three layers whole-K with the switch on, none with it off
    assert sorted(k[5] for k in pn._insts) == [(False, False, False), (True, True, True)]
    marks = {k[5][0]: [w for inst in v for w in inst.passes if w.startswith("bwd")] for k, v in pn._insts.items()}
    assert all(",tail111" in w for w in marks[True]) and all(",tail000" in w for w in marks[False]) and marks[True] and marks[False]
    assert float(off[2].abs().max()) > 0 and float(off[1][0].abs().max()) > 0
    for name, a, b in (("off / on", off, on1), ("on / on", on1, on2)):
        for x, y in zip(a[0] + a[1] + [a[2]], b[0] + b[1] + [b[2]]):
            assert torch.equal(x, y), name


def test_a_request_is_refused_where_the_form_is_not_selected():
    """No quiet fall-back: a whole-K request at a shape the planner does not select is an error; the plain call never takes the form."""
    B = 32
    assert max(s[0] for s in SHAPES) == int(_lib.tune_get("pose_tail_max_pairs")) < B      # SHAPES' last entry is the ceiling itself
    d = _descs(B, 256, 320)[2]
    assert ops.pose_tail_plan(d) is None and ops.pose_tail_plan(d, 1) is None
    x = torch.zeros(B, d.Hi, d.Wi, 256, device=dev(), dtype=torch.bfloat16)
    w = torch.zeros(256, 9, 256, device=dev(), dtype=torch.bfloat16)
    y = torch.zeros(B, d.Ho, d.Wo, 256, device=dev(), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="colvo_conv_fwd: the whole-K form is not selected"):
        ops.conv_fwd(d, x, None, w, torch.zeros(256, device=dev()), y, whole_k=True)
    with pytest.raises(RuntimeError, match="colvo_conv_dgrad: the whole-K form is not selected"):
        ops.conv_dgrad(d, 0, y, w, x, torch.zeros_like(x), False, whole_k=True)
    d8 = _descs(8, 256, 320)[2]
    with _switch(False):
        with pytest.raises(RuntimeError, match="colvo_conv_fwd: the whole-K form is not selected"):
            ops.conv_fwd(d8, x[:8], None, w, torch.zeros(256, device=dev()), y[:8], whole_k=True)
