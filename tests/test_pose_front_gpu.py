"""-m gpu: PoseNet's front layers as one launch per direction (csrc/pose_front.hip, tuning `pose_front` / `pose_front_bwd`) against the
three launches each replaces.

The chains must give the same BITS: torch.equal with the switch on and off in one process, on random data with both signs (mixed
ReLU masks), random weights and non-zero biases; destinations are pre-filled with a sentinel so that an element the chain leaves
unwritten shows.  Shapes (pairs x H x W):
    1 x 32 x 32     conv3's map is 4 x 4: one partial tile, every level's border inside one workgroup
    2 x 64 x 96     several tiles, tile edges on image borders
    3 x 96 x 160    odd batch; conv3's 12 x 20 map leaves the last 4 x 8 tile column ragged
    8 x 256 x 320   the benchmark's shape: the planner's 4 x 10 tile (256 workgroups), the other compiled tile width
On exact data (tests/conv_exact.py) every sum is representable, so the forward chain must also match the float64 reference bit for
bit."""
import pytest
import torch

from coivo_amd import _lib, ops
from tests import conv_exact as X
from tests import guarded
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

_guarded = guarded.fixture(dev)          # every test here allocates from tests/guarded.py's pool; the guards are checked at its end

SHAPES = [(1, 32, 32), (2, 64, 96), (3, 96, 160), (8, 256, 320)]
CH = (8, 16, 32, 64)
SENTINEL = 77.0


class _switch:
    """tuning `pose_front` set for a block; the library's default afterwards (the tests share one process)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.saved = _lib.tune_get("pose_front")
        _lib.tune_set("pose_front", 1 if self.on else 0)

    def __exit__(self, *exc):
        _lib.tune_set("pose_front", self.saved)
        return False


def _descs(B, H, W):
    out, h, w = [], H, W
    for i in range(3):
        out.append(ops.conv_desc(torch.bfloat16, B, h, w, CH[i], CH[i + 1], stride=2))
        h, w = out[-1].Ho, out[-1].Wo
    return out


def _pack(wm):
    cout, _, cin = wm.shape
    w_fwd = torch.empty(cout, 9, cin, device=wm.device, dtype=torch.bfloat16)
    w_bwd = torch.empty(cin, 9, cout, device=wm.device, dtype=torch.bfloat16)
    ops.pack_weights(wm, torch.bfloat16, w_fwd, w_bwd)
    return w_fwd


def _run_both(descs, x, weights, biases):
    """(acts of three colvo_conv_fwd launches, acts of the chain launch), every destination pre-filled with the sentinel."""
    mk = lambda d: torch.full((d.B, d.Ho, d.Wo, d.Cout), SENTINEL, device=x.device, dtype=torch.bfloat16)
    with _switch(False):
        assert ops.pose_front_plan(descs[0]) is None
        ref, src = [mk(d) for d in descs], x
        before = _lib.form_counts()
        for d, w, b, y in zip(descs, weights, biases, ref):
            ops.conv_fwd(d, src, None, w, b, y)
            src = y
        torch.cuda.synchronize()
        # the reference really is the one-tile form the chain's bits are tied to
        assert X.forms_diff(before, _lib.form_counts()) == {"conv_tile": 3}
    with _switch(True):
        assert ops.pose_front_plan(descs[0]) is not None
        got = [mk(d) for d in descs]
        before = _lib.form_counts()
        ops.conv_fwd_chain(descs[0], x, list(zip(weights, biases, got)))
        torch.cuda.synchronize()
        assert _lib.form_counts() == before                      # the chain counts nothing
    return ref, got


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_chain_gives_the_bits_of_three_launches(B, H, W):
    g = torch.Generator(device=dev()).manual_seed(B * 1000 + H)
    descs = _descs(B, H, W)
    x = torch.randn(B, H, W, 8, generator=g, device=dev()).to(torch.bfloat16)
    weights = [_pack(torch.randn(CH[i + 1], 9, CH[i], generator=g, device=dev()) * (2.0 / (9 * CH[i])) ** 0.5) for i in range(3)]
    biases = [torch.randn(CH[i + 1], generator=g, device=dev()) * 0.3 for i in range(3)]
    ref, got = _run_both(descs, x, weights, biases)
    for i, (r, y) in enumerate(zip(ref, got), start=1):
        frac = float((r == 0).float().mean())
        assert 0.05 < frac < 0.95, f"act{i}: the ReLU mask is not mixed ({frac:.2f} zeros)"
        assert not bool((r == SENTINEL).any())
        assert torch.equal(r.view(torch.int16), y.view(torch.int16)), \
            f"act{i} at {B}x{H}x{W}: {int((r.view(torch.int16) != y.view(torch.int16)).sum())} of {r.numel()} elements differ"


def _pack_bwd(wm):
    cout, _, cin = wm.shape
    w_fwd = torch.empty(cout, 9, cin, device=wm.device, dtype=torch.bfloat16)
    w_bwd = torch.empty(cin, 9, cout, device=wm.device, dtype=torch.bfloat16)
    ops.pack_weights(wm, torch.bfloat16, w_fwd, w_bwd)
    return w_bwd


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_input_gradient_chain_gives_the_bits_of_three_launches(B, H, W):
    """g2, g1 and the two depth planes d_tr against conv3's and conv2's colvo_conv_dgrad and colvo_conv_dgrad_planes, destinations
    pre-filled with a sentinel.  The activations only serve as ReLU masks here: random, both signs."""
    g = torch.Generator(device=dev()).manual_seed(B * 1000 + W)
    d1, d2, d3 = _descs(B, H, W)
    rnd = lambda *shape: torch.randn(*shape, generator=g, device=dev())
    act1, act2 = rnd(B, d1.Ho, d1.Wo, 16).to(torch.bfloat16), rnd(B, d2.Ho, d2.Wo, 32).to(torch.bfloat16)
    g3 = rnd(B, d3.Ho, d3.Wo, 64).to(torch.bfloat16)
    wm1 = rnd(16, 9, 8) * 0.2
    wb2, wb3 = _pack_bwd(rnd(32, 9, 16) * 0.1), _pack_bwd(rnd(64, 9, 32) * 0.1)
    mk = lambda: (torch.full_like(act2, SENTINEL), torch.full_like(act1, SENTINEL),
                  torch.full((2, B, 1, H, W), SENTINEL, device=dev()))
    with _switch(False):
        assert ops.pose_front_plan(d1, 1) is None
        r2, r1, rtr = mk()
        before = _lib.form_counts()
        ops.conv_dgrad(d3, 0, g3, wb3, act2, r2, False)
        ops.conv_dgrad(d2, 0, r2, wb2, act1, r1, False)
        ops.conv_dgrad_planes(d1, r1, wm1, 6, 2, rtr)
        torch.cuda.synchronize()
        # the reference really is the three forms the chain's bits are tied to
        assert X.forms_diff(before, _lib.form_counts()) == {"dgrad_s2": 2, "dgrad_planes_mfma": 1}
    with _switch(True):
        assert ops.pose_front_plan(d1, 1) is not None
        c2, c1, ctr = mk()
        before = _lib.form_counts()
        ops.conv_dgrad_chain(d1, g3, wb3, wb2, act2, act1, c2, c1, wm1, 6, 2, ctr)
        torch.cuda.synchronize()
        assert _lib.form_counts() == before
    for name, r, c in (("g2", r2, c2), ("g1", r1, c1)):
        frac = float((r == 0).float().mean())
        assert 0.2 < frac < 0.8, f"{name}: the ReLU mask is not mixed ({frac:.2f} zeros)"
        assert not bool((r == SENTINEL).any())
        assert torch.equal(r.view(torch.int16), c.view(torch.int16)), \
            f"{name} at {B}x{H}x{W}: {int((r.view(torch.int16) != c.view(torch.int16)).sum())} of {r.numel()} elements differ"
    assert not bool((rtr == SENTINEL).any()) and float(rtr.abs().max()) > 0
    assert torch.equal(rtr.view(torch.int32), ctr.view(torch.int32)), \
        f"d_tr at {B}x{H}x{W}: {int((rtr.view(torch.int32) != ctr.view(torch.int32)).sum())} of {rtr.numel()} elements differ"


def test_chain_is_exact_on_exact_data():
    """tests/conv_exact.py's sources, biases, float64 reference and comparison at 2 x 64 x 96.  conv2 and conv3 read the previous
    layer's stored bf16 map, so each layer's reference is taken on the map in front of it, and the weights are drawn from
    {-1, 0, 1} * 2^-4 instead of conv_exact's [-8, 8] * 2^-4 to keep all THREE levels in the exact regime, in quanta of 2^-6:
    conv1 sums 72 products of at most 3 and a bias of at most 16 -- at most 232 < 2^8, stored exactly in bf16; conv2 sums 144
    products of at most 232 -- at most 33 424, one rounding to bf16; conv3 sums 288 products of at most 33 424 -- below 2^23.2, exact
    in fp32 whatever the order.  expect_exact checks that the reference itself survives the trip through fp32."""
    B, H, W = 2, 64, 96
    g = torch.Generator(device=dev()).manual_seed(5)
    descs = _descs(B, H, W)
    xf = X.make_source((B, H, W, 8), g, dev())
    wms = [torch.randint(-1, 2, (CH[i + 1], 9, CH[i]), generator=g, device=dev(), dtype=torch.int32).float() * X.QW for i in range(3)]
    biases = [X.make_bias(CH[i + 1], g, dev()) for i in range(3)]
    weights = [_pack(w) for w in wms]
    ref, got = _run_both(descs, xf.to(torch.bfloat16), weights, biases)
    src = xf
    for i, (d, y) in enumerate(zip(descs, got)):
        lay = X.Layer.of_desc(d)
        X.expect_exact(y, lay.ref_fwd(src, None, wms[i], biases[i], 0, B), X.QB, f"chain act{i + 1}")
        assert torch.equal(ref[i], y)
        src = y.float()


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


@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (3, 96, 160)])
def test_posenet_step_is_the_same_with_the_chain(B, H, W):
    """nn level, deterministic mode: outputs, depth gradients and the whole gradient arena with the switch on and off, and two runs
    with it on.  The recorded pass is keyed by the planner's answer, so one network serves both settings."""
    from coivo_amd import nn as hnn
    g = torch.Generator(device=dev()).manual_seed(11)
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
    assert any(k[4] for k in pn._insts) and any(not k[4] for k in pn._insts)      # both forms were recorded, in both directions
    chained = {k[4]: [w.endswith(",chain") for inst in v for w in inst.passes if w.startswith("bwd")] for k, v in pn._insts.items()}
    assert chained == {True: [True], False: [False]}
    assert float(off[2].abs().max()) > 0 and float(off[1][0].abs().max()) > 0
    for name, a, b in (("off / on", off, on1), ("on / on", on1, on2)):
        for x, y in zip(a[0] + a[1] + [a[2]], b[0] + b[1] + [b[2]]):
            assert torch.equal(x, y), name


def test_chain_is_refused_where_it_is_not_selected():
    """No quiet fall-back: a chain command at a shape the planner does not select is an error of colvo_conv_fwd."""
    B, H, W = 1, 36, 44
    descs = _descs(B, H, W)
    x = torch.zeros(B, H, W, 8, device=dev(), dtype=torch.bfloat16)
    lays = [(torch.zeros(CH[i + 1], 9, CH[i], device=dev(), dtype=torch.bfloat16), torch.zeros(CH[i + 1], device=dev()),
             torch.zeros(B, d.Ho, d.Wo, CH[i + 1], device=dev(), dtype=torch.bfloat16)) for i, d in enumerate(descs)]
    with pytest.raises(RuntimeError, match="colvo_conv_fwd: the three-layer chain is not selected"):
        ops.conv_fwd_chain(descs[0], x, lays)
    g1, g2, g3 = (torch.zeros_like(lays[i][2]) for i in range(3))
    with pytest.raises(RuntimeError, match="colvo_conv_dgrad_planes: the input-gradient chain is not selected"):
        ops.conv_dgrad_chain(descs[0], g3, torch.zeros(32, 9, 64, device=dev(), dtype=torch.bfloat16),
                             torch.zeros(16, 9, 32, device=dev(), dtype=torch.bfloat16), lays[1][2], lays[0][2], g2, g1,
                             torch.zeros(16, 9, 8, device=dev()), 6, 2, torch.zeros(2, B, 1, H, W, device=dev()))
