"""-m gpu unit parity of the conv-stack kernels (a1/a2) against torch CPU ops (F.conv2d autograd).

f32 mode uses the exact-f32 MFMA and is held to fp32 round-off; bf16 mode is compared against the same
torch computation on bf16-rounded operands with a bf16-sized tolerance.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import guarded
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

_guarded = guarded.fixture(dev, allocates_nothing=("test_every_kernel_form_is_covered",))          # every test here allocates from tests/guarded.py's pool; the guards are checked at its end


def _nhwc(t):   # NCHW -> NHWC contiguous
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _ref_conv(x0, x1, up0, up1, w_master, bias, stride, relu):
    """x0/x1: NCHW fp32 (stored resolution), w_master [Cout, 9, Cin]."""
    xs = []
    for x, up in ((x0, up0), (x1, up1)):
        if x is None:
            continue
        xs.append(F.interpolate(x, scale_factor=2, mode="nearest") if up else x)
    x = torch.cat(xs, dim=1)
    Cout, _, Cin = w_master.shape
    w = w_master.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    y = F.conv2d(x, w, bias, stride=stride, padding=1)
    return F.relu(y) if relu else y


CASES = [
    # B, Hi, Wi, C0, C1, up0, up1, Cout, stride
    (2, 16, 24, 32, 0, False, False, 64, 1),
    (2, 16, 24, 32, 0, False, False, 32, 2),
    (1, 13, 21, 8, 0, False, False, 16, 2),       # stem-like: Cin 8, odd size
    (2, 16, 20, 64, 0, True, False, 32, 1),       # up-sampled source
    (2, 16, 20, 32, 32, False, False, 32, 1),     # concat
    (1, 8, 12, 16, 0, False, False, 16, 1),       # Cin = Cout = 16
    (3, 8, 10, 128, 0, False, False, 128, 1),     # deep small image, 2 N tiles
    (2, 5, 5, 64, 0, False, False, 64, 2),        # PoseNet tail sizes
    (1, 32, 40, 16, 16, True, False, 16, 1),      # up + concat, narrow
    (2, 9, 7, 24, 0, False, False, 40, 1),        # channel counts that are only multiples of 8
    (2, 16, 24, 8, 0, False, False, 8, 1),        # narrower than the smallest channel tile (rows beyond N read as zero)
    (2, 8, 10, 256, 0, False, False, 64, 1),      # 8 chunks, <= 256 workgroups: the two-chunk register ring
    (4, 256, 320, 16, 0, False, False, 16, 1),    # >= 2048 tiles, single chunk: weights-resident persistent kernel
    (4, 256, 288, 32, 0, True, False, 16, 1),     # ... its dgrad with the 2x2 sum-pool of an up-sampled source (form0: 2304 tiles, and the
                                                  #     k_dgrad_up2 grid below dgrad_up2_min_wgs; form1 / form2 lower that: k_dgrad_up2)
    (13, 128, 160, 32, 0, False, False, 32, 1),   # ... 32-wide (bf16: one chunk; 2080 tiles); f32: two chunks, the one-tile kernel
    # stride 2 with an even input: the parity-decomposed input gradient (k_dgrad_s2)
    (2, 32, 40, 64, 0, False, False, 128, 2),     # 4 chunks (bf16), two N tiles, ragged tiles (16 x 20 positions)
    (2, 16, 20, 128, 0, False, False, 256, 2),    # 8 chunks, few workgroups: unrolled two-chunk ring
    (1, 16, 20, 256, 0, False, False, 512, 2),    # 16 chunks
    (2, 64, 80, 8, 0, False, False, 32, 2),       # 8 input channels: narrower than the 16-wide channel tile
    (3, 12, 18, 40, 0, False, False, 64, 2),      # channel count that is only a multiple of 8; 6 x 9 positions
    (2, 2, 2, 32, 0, False, False, 32, 2),        # one position per image
    # single up-sampled source, >= 2 chunks: four output pixels per source position (k_conv_up2)
    (2, 64, 80, 128, 0, True, False, 64, 1),      # 4 chunks, several tiles, two N tiles
    (2, 16, 20, 256, 0, True, False, 128, 1),     # 8 chunks: unrolled two-chunk ring
    (1, 16, 20, 512, 0, True, False, 256, 1),     # 16 chunks
    (3, 10, 14, 64, 0, True, False, 24, 1),       # 5 x 7 source positions, ragged N
    (2, 2, 2, 64, 0, True, False, 16, 1),         # a single source pixel per image
    (1, 8, 10, 32, 0, True, False, 512, 1),       # k_dgrad_up2 with 16 chunks of dy
    (2, 24, 40, 32, 0, True, False, 64, 1),       # ... 12 x 20 source positions: ragged tiles
    # stride 1, direct sources, >= 2 chunks: the quad-tile kernel (k_conv_q) in the form1 runs
    (2, 32, 64, 64, 64, False, False, 64, 1),     # concat of two sources, exact 16 x 32 quad tiles, two N tiles
    (1, 40, 72, 128, 0, False, False, 48, 1),     # ragged quad tiles and ragged N
    (2, 20, 12, 64, 32, False, False, 32, 1),     # sources of different width, narrow image (8-wide sub-tiles, padded rows)
    # deep layers on few workgroups (the shapes of enc5b / iconv5 / enc4b at small batch)
    (1, 8, 10, 512, 0, False, False, 512, 1),     # 16 chunks (bf16)
    (2, 16, 20, 256, 256, False, False, 256, 1),  # concat, 16 chunks from two sources
    (2, 16, 20, 256, 0, False, False, 256, 1),    # 8 chunks
    (1, 8, 10, 288, 0, False, False, 64, 1),      # 9 (bf16) / 18 (f32) chunks: odd count on the two-chunk ring
    # stride 2, ONE chunk (32 bf16 / 16 f32 channels): the stride-2 form of the weights-resident persistent kernel in the form2 runs
    (3, 32, 48, 32, 0, False, False, 64, 2),      # 64-wide channel tile (bf16), several tiles per image and per workgroup; f32: two chunks
    (2, 40, 112, 16, 0, False, False, 32, 2),     # f32: one chunk of 16; bf16: two-granule chunks; 20 x 56 outputs
    (5, 16, 64, 32, 0, False, False, 48, 2),      # N = 48 (bf16): two 32-wide channel tiles, rows beyond N of the second read as zero
    # stride 1, direct sources: the register-tiled kernel (k_conv_rt) in the form2 runs -- 16 x 16 tiles x 64 / 32 channels
    (2, 32, 48, 64, 0, False, False, 64, 1),      # exact tiles, one 64-wide channel tile, 2 chunks
    (1, 48, 32, 64, 64, False, False, 128, 1),    # concat 64 + 64 (two-output input gradient, 64-wide tiles), two N tiles
    (2, 40, 56, 32, 32, False, False, 32, 1),     # concat 32 + 32 (two-output input gradient, 32-wide tiles), ragged 16 x 16 tiles
    (1, 33, 17, 96, 0, False, False, 80, 1),      # ragged everything: 3 chunks, N = 80 in 64-wide tiles, one-pixel tile rows / columns
    # the register-tiled weight gradient (k_wgrad_rt): image groups and long walks
    (7, 8, 10, 64, 0, False, False, 64, 1),       # 8 x 10 maps: tiles of several whole images, the last group cut short by the batch
    (2, 64, 80, 32, 32, False, False, 32, 1),     # concat at 1/4 resolution: several tiles per image, two ci tiles from two sources
    (3, 32, 40, 128, 0, False, False, 128, 1),    # 4 x 4 (co, ci) tiles
]


def _tols(dtype):
    """(rtol, atol as a fraction of max|ref|) for outputs ACCUMULATED in fp32 and stored in fp32 (weight / bias gradients) or, in
    f32 mode, everything.  The operands of every case are exactly representable in `dtype`, so the products are exact in fp32 and
    only the summation order differs from torch's (up to 3e5 terms per element, split across workgroups): 1e-4 of the largest
    element in f32 mode (as in rounds 1-4) and 2e-4 for the bf16 kernels' fp32 outputs (round 4 allowed 0.1)."""
    return (1e-4, 1e-4) if dtype == torch.float32 else (2e-4, 2e-4)


def _close_out(got, ref, dtype, what, atol_scale=2e-5):
    """Feature-map outputs (forward, input gradients).  f32 mode: fp32 round-off.  bf16 mode: the kernel accumulates in fp32 and
    rounds ONCE, at the store -- every element within one bf16 ulp of the fp32 reference (2^-7 relative: half an ulp of rounding,
    the other half for a sum that lands on the other side of a rounding boundary), and all but 0.1 % of them within the rounding
    itself (2^-8 relative); the absolute part covers fp32 summation order on elements that cancel to ~0.  Round 4 allowed 2e-2 of
    the LARGEST element everywhere: a dropped tile row of a 20-tile walk would have passed."""
    if dtype == torch.float32:
        return _close(got, ref, 2e-5, 2e-5, what)
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    atol = atol_scale * max(ref.abs().max().item(), 1e-20)
    err = (got - ref).abs()
    bad = err > atol + 2.0 ** -7 * ref.abs()
    assert not bad.any(), f"{what}: max err {err.max().item():.3e} beyond one bf16 ulp, {int(bad.sum())} bad of {bad.numel()}"
    loose = err > atol + (2.0 ** -8) * (1 + 1e-3) * ref.abs()
    assert loose.float().mean().item() < 1e-3, f"{what}: {int(loose.sum())} of {loose.numel()} elements beyond a bf16 rounding"


def _close(got, ref, rtol, atol_scale, what):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    atol = atol_scale * max(ref.abs().max().item(), 1e-20)
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{what}: max err {err.max().item():.3e} (atol {atol:.3e}), {int(bad.sum())} bad of {bad.numel()}"


_FORM_TUNING = ("dgrad_up2_min_wgs", "quad_min_wgs", "quad_max_chunks", "rt_min_wgs", "rt_bn32_min_wgs", "rt_min_fill_pct", "rt_min_chunks",
                "rt_tiles_per_wg", "res_s2_min_tiles", "wgrad_rt", "wgrad_rt_min_c", "wgrad_rt_over_up2", "wgrad_rt_wgs", "wgrad_rt_max_px")


def _set_form(form, dtype):
    """The fat-workgroup kernels (k_conv_q: quad tiles for stride-1 layers; k_dgrad_up2: sum-pool in the K loop) are selected
    only for large grids (>= 2048 / 640 workgroups); the parametrised cases are small, so form1 / form2 lower the thresholds
    in the library's tuning table (colvo_tune_set, csrc/tuning.h) to reach them -- form0 exercises the production dispatch on the
    same shapes.  Returns the entries to restore."""
    from coivo_amd import _lib
    saved = {n: _lib.tune_get(n) for n in _FORM_TUNING}
    # The register-tiled weight gradient (k_wgrad_rt, csrc/wgrad_rt.hip; bf16 stride-1 layers; measured level alone and a loss in the step,
    # so production leaves it off -- profiles/r6_wgrad_rt.md -- and form0 is the production dispatch): form1 runs it on EVERY bf16 stride-1
    # case (8-, 16-, 24-, 40-channel tensors in 32-wide tiles, up-sampled sources read through its staging addresses) with tiles of
    # at most 48 pixels and three workgroups per (co, ci) tile -- long walks over both staging buffers, ragged tiles, image groups cut
    # short by the batch; form2 the same tensors in full-size tiles on 256-workgroup grids.
    if form == "form1":
        _lib.tune_set("wgrad_rt", 1)
        _lib.tune_set("wgrad_rt_min_c", 8)
        _lib.tune_set("wgrad_rt_over_up2", 1)
        _lib.tune_set("wgrad_rt_max_px", 48)
        _lib.tune_set("wgrad_rt_wgs", 3)
        _lib.tune_set("dgrad_up2_min_wgs", 0)
        _lib.tune_set("quad_min_wgs", 0)
        _lib.tune_set("quad_max_chunks", 64)
    if form == "form2":
        _lib.tune_set("wgrad_rt", 1)
        _lib.tune_set("wgrad_rt_min_c", 8)
        _lib.tune_set("wgrad_rt_over_up2", 1)
        # the register-tiled stride-1 kernel (k_conv_rt, csrc/conv_rt.hip: selected from 1024 workgroups on and where its 16 x 16
        # tiles cover the image well): every stride-1 case with direct sources and whole chunks, ragged images included
        _lib.tune_set("dgrad_up2_min_wgs", 0)
        _lib.tune_set("rt_min_wgs", 0)
        _lib.tune_set("rt_bn32_min_wgs", 0)
        _lib.tune_set("rt_min_fill_pct", 0)
        _lib.tune_set("rt_min_chunks", 1)
        _lib.tune_set("res_s2_min_tiles", 2)       # the stride-2 form of the weights-resident persistent kernel (single-chunk layers)
        # ... bf16 runs with workgroups that WALK three consecutive tiles (across channel tiles, tile rows and images; the last
        # workgroup a shorter walk), f32 runs with one tile per workgroup, the production setting
        _lib.tune_set("rt_tiles_per_wg", 3 if dtype == torch.bfloat16 else 0)
    return saved


def _restore(saved):
    from coivo_amd import _lib
    for n, v in saved.items():
        _lib.tune_set(n, v)


@pytest.fixture(autouse=True)
def _both_kernel_forms(request):
    """Runs test_conv_fwd_dgrad_wgrad and its exact-data twin in form0 / form1 / form2 (_set_form) and restores the table."""
    params = getattr(getattr(request.node, "callspec", None), "params", {})
    form = next((f for f in ("form0", "form1", "form2") if f in request.node.name), "form0")
    saved = _set_form(form, params.get("dtype"))
    yield
    _restore(saved)


@pytest.mark.parametrize("form", ["form0", "form1", "form2"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CASES)
def test_conv_fwd_dgrad_wgrad(case, dtype, form):
    from coivo_amd import ops
    B, Hi, Wi, C0, C1, up0, up1, Cout, stride = case
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    rt, at = _tols(dtype)

    def rnd(*s):
        t = torch.randn(*s, generator=g)
        return t.to(dtype).float()      # values exactly representable in `dtype`

    def stored(C, up):
        return (B, C, Hi // 2, Wi // 2) if up else (B, C, Hi, Wi)

    x0 = F.relu(rnd(*stored(C0, up0)))             # sources are ReLU outputs (>= 0, many exact zeros)
    x1 = F.relu(rnd(*stored(C1, up1))) if C1 else None
    Cin = C0 + C1
    w = (rnd(Cout, 9, Cin) * (2.0 / (9 * Cin)) ** 0.5).to(dtype).float()
    bias = torch.randn(Cout, generator=g) * 0.1

    x0r = x0.clone().requires_grad_(True)
    x1r = x1.clone().requires_grad_(True) if C1 else None
    wr = w.clone().requires_grad_(True)
    br = bias.clone().requires_grad_(True)
    y_ref = _ref_conv(x0r, x1r, up0, up1, wr, br, stride, True)
    dy = rnd(*y_ref.shape)
    dpre = (dy * (y_ref > 0)).to(dtype).float()    # gradient w.r.t. the pre-activation, as the kernels expect
    pre = _ref_conv(x0r, x1r, up0, up1, wr, br, stride, False)
    pre.backward(dpre)

    d = dev()
    desc = ops.conv_desc(dtype, B, Hi, Wi, C0, Cout, stride=stride, relu=True, C1=C1, up0=up0, up1=up1)
    x0d = _nhwc(x0).to(d, dtype)
    x1d = _nhwc(x1).to(d, dtype) if C1 else None
    wm = w.to(d)
    w_fwd = torch.empty(Cout, 9, Cin, device=d, dtype=dtype)
    w_bwd = torch.empty(Cin, 9, Cout, device=d, dtype=dtype)
    ops.pack_weights(wm, dtype, w_fwd, w_bwd)
    assert torch.equal(w_fwd.float().cpu(), w)
    yd = torch.empty(B, desc.Ho, desc.Wo, Cout, device=d, dtype=dtype)
    ops.conv_fwd(desc, x0d, x1d, w_fwd, bias.to(d), yd)
    _close_out(_nchw(yd), y_ref, dtype, "fwd")

    dyd = _nhwc(dpre).to(d, dtype)
    # dgrad of each source: plain, then with the producer's ReLU mask + accumulate on top of a base
    for si, (xs, xr, Cs) in enumerate(((x0d, x0r, C0), (x1d, x1r, C1))):
        if xs is None:
            continue
        dx = torch.full_like(xs, 7.0)
        ops.conv_dgrad(desc, si, dyd, w_bwd, None, dx, False)
        _close_out(_nchw(dx), xr.grad, dtype, f"dgrad src{si}")
        base = torch.randn(xs.shape, generator=g).to(dtype)
        dx2 = guarded.active_pool().place(base.to(d), "accumulate base")
        ops.conv_dgrad(desc, si, dyd, w_bwd, xs, dx2, True)
        ref2 = _nchw(base.float()) + xr.grad * (xr > 0)
        _close_out(_nchw(dx2), ref2, dtype, f"dgrad src{si} masked+accumulate", atol_scale=4e-5)

    dw = torch.zeros(Cout, 9, Cin, device=d)
    db = torch.zeros(Cout, device=d)
    ops.conv_wgrad(desc, x0d, x1d, dyd, dw, db)
    _close(dw, wr.grad, rt, at, "wgrad")
    _close(db, br.grad, rt, at, "bgrad")
    # wgrad accumulates
    ops.conv_wgrad(desc, x0d, x1d, dyd, dw, db)
    _close(dw, 2 * wr.grad, rt, at, "wgrad accumulate")
    # the caller vouches for a zero arena (colvo_conv_wgrad_clean): single-split layers store instead of adding -- same values; a
    # second, ordinary call accumulates on top
    dwc, dbc = torch.zeros_like(dw), torch.zeros_like(db)
    ops.conv_wgrad(desc, x0d, x1d, dyd, dwc, dbc, arena_is_zero=True)
    _close(dwc, wr.grad, rt, at, "wgrad (zero arena vouched for)")
    _close(dbc, br.grad, rt, at, "bgrad (zero arena vouched for)")
    ops.conv_wgrad(desc, x0d, x1d, dyd, dwc, dbc)
    _close(dwc, 2 * wr.grad, rt, at, "wgrad (zero arena vouched for) accumulate")
    # deterministic form (per-split slabs + a fixed-order second launch instead of float atomics): same values, bitwise
    # repeatable, accumulates like the plain form
    scr = ops.conv_wgrad_scratch(desc, d)
    dws, dbs = [], []
    for _ in range(2):
        dwd, dbd = torch.zeros_like(dw), torch.zeros_like(db)
        ops.conv_wgrad(desc, x0d, x1d, dyd, dwd, dbd, scr)
        dws.append(dwd); dbs.append(dbd)
    _close(dws[0], wr.grad, rt, at, "wgrad (deterministic form)")
    _close(dbs[0], br.grad, rt, at, "bgrad (deterministic form)")
    assert torch.equal(dws[0], dws[1]) and torch.equal(dbs[0], dbs[1])
    ops.conv_wgrad(desc, x0d, x1d, dyd, dws[0], dbs[0], scr)
    _close(dws[0], 2 * wr.grad, rt, at, "wgrad (deterministic form) accumulate")


# The kernels the comments of CASES name, by case index: (forms, dtypes, acceptable forms) -- at least one pass of the exact twin counts one
# of them (include/colvo.h colvo_form_counts).  bf16 / f32 differ where the chunk width does (32 / 16 channels).
_BF, _F32, _ALL = (torch.bfloat16,), (torch.float32,), (torch.bfloat16, torch.float32)
CASE_FORMS = {
    11: [("form0", _ALL, {"conv_ring"})],                                   # the two-chunk register ring
    12: [("form0", _ALL, {"conv_res"})],                                    # weights-resident persistent kernel
    13: [("form0", _ALL, {"conv_res"}), ("form1", _ALL, {"dgrad_up2"})],   # ... its input gradient with the sum-pool
    14: [("form0", _BF, {"conv_res"}), ("form1", _BF, {"conv_res"}), ("form0", _F32, {"conv_tile"})],
    15: [("form0", _BF, {"dgrad_s2"})],                                     # 4 chunks (f32: 8, the ring)
    16: [("form0", _ALL, {"dgrad_s2_ring"})],                               # unrolled two-chunk ring
    17: [("form0", _BF, {"dgrad_s2_ring"})],                                # 16 chunks (f32: 32, one chunk in flight)
    18: [("form0", _ALL, {"dgrad_s2"})],
    19: [("form0", _ALL, {"dgrad_s2"})],
    20: [("form0", _ALL, {"dgrad_s2"})],
    21: [("form0", _ALL, {"conv_up2_bn16", "conv_up2_bn32"})],
    22: [("form0", _ALL, {"conv_up2_bn16", "conv_up2_bn32"})],
    23: [("form0", _ALL, {"conv_up2_bn16", "conv_up2_bn32"})],
    24: [("form0", _ALL, {"conv_up2_bn16", "conv_up2_bn32"})],
    25: [("form0", _ALL, {"conv_up2_bn16", "conv_up2_bn32"})],
    26: [("form1", _ALL, {"dgrad_up2"}), ("form2", _ALL, {"dgrad_up2"})],
    27: [("form1", _ALL, {"dgrad_up2"}), ("form2", _ALL, {"dgrad_up2"})],
    28: [("form1", _ALL, {"conv_q"})],
    29: [("form1", _ALL, {"conv_q"})],
    30: [("form1", _ALL, {"conv_q"})],
    31: [("form0", _ALL, {"conv_ring"})],                                   # deep layers on few workgroups: the two-chunk ring
    32: [("form0", _ALL, {"conv_ring"})],
    33: [("form0", _ALL, {"conv_ring"})],
    34: [("form0", _ALL, {"conv_ring"})],
    35: [("form2", _BF, {"conv_res_s2"}), ("form2", _BF, {"conv_bn64"})],
    36: [("form2", _ALL, {"conv_res_s2"})],
    37: [("form2", _BF, {"conv_res_s2"})],
    35: [("form2", _BF, {"conv_res_s2"})],
    38: [("form2", _ALL, {"conv_rt"})],
    39: [("form2", _ALL, {"conv_rt"})],
    40: [("form2", _ALL, {"conv_rt"}), ("form2", _ALL, {"conv_rt_bn32"})],   # 32-wide tiles
    41: [("form2", _ALL, {"conv_rt"})],
    42: [("form1", _BF, {"wgrad_rt"}), ("form2", _BF, {"wgrad_rt"})],
    43: [("form1", _BF, {"wgrad_rt"}), ("form2", _BF, {"wgrad_rt"})],
    44: [("form1", _BF, {"wgrad_rt"}), ("form2", _BF, {"wgrad_rt"})],
}
_EXACT_SEEN = {}         # (case index, dtype, form) -> {form: launches} of the exact twin in this process


def _exact_case(ci, dtype, form):
    from tests import conv_exact as X
    B, Hi, Wi, C0, C1, up0, up1, Cout, stride = CASES[ci]
    lay = X.Layer(B, Hi, Wi, C0, C1, up0, up1, Cout, stride)
    g = torch.Generator(device=dev()).manual_seed(1000 * ci + 7)
    forms = X.check_layer(lay, dtype, g, dev())
    X.check_forms(lay, dtype, forms)
    hit = {}
    for f in forms.values():
        for k, v in f.items():
            hit[k] = hit.get(k, 0) + v
    for want_form, dts, names in CASE_FORMS.get(ci, ()):
        if want_form == form and dtype in dts:
            assert any(hit.get(n, 0) for n in names), f"case {ci} {CASES[ci]} {dtype} {form}: none of {sorted(names)} ran; {forms}"
    _EXACT_SEEN[(ci, dtype, form)] = hit
    return hit


@pytest.mark.parametrize("form", ["form0", "form1", "form2"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_conv_exact_data_bit_for_bit(ci, dtype, form):
    """test_conv_fwd_dgrad_wgrad's cases, dtypes and kernel forms on exact data (tests/conv_exact.py): every pass -- forward, input
    gradients plain / masked + accumulate / both sources in one launch, weight gradient in the atomic, clean-arena, deterministic and
    slab forms and accumulating -- equal BY VALUE to the float64 reference rounded once to the output dtype; and the kernel each case's
    comment names ran (CASE_FORMS)."""
    _exact_case(ci, dtype, form)


def test_conv_exact_data_wide_form():
    """The one-tile kernel's 512-thread / 256-pixel form (tuning `wide`, off by default -- no production shape and no case above reaches
    it): on, from any grid, at a two-chunk stride-1 layer whose 256-pixel tiles fit; bit for bit as above."""
    from coivo_amd import _lib
    from tests import conv_exact as X
    saved = {n: _lib.tune_get(n) for n in ("wide", "wide_min_wgs")}
    try:
        _lib.tune_set("wide", 1)
        _lib.tune_set("wide_min_wgs", 0)
        for dtype in (torch.bfloat16, torch.float32):
            lay = X.Layer(2, 32, 48, 64, 0, False, False, 64, 1)
            forms = X.check_layer(lay, dtype, torch.Generator(device=dev()).manual_seed(9), dev())
            X.check_forms(lay, dtype, forms)
            assert forms["fwd"].get("conv_wide") == 1, (dtype, forms)
            _EXACT_SEEN[("wide", dtype)] = forms["fwd"]
    finally:
        for n, v in saved.items():
            _lib.tune_set(n, v)


def test_every_kernel_form_is_covered():
    """The forms the exact small cases reach, with those the production sweep asserts (test_conv_exact_gpu.PRODUCTION_FORMS), are
    every counter the library reports.  Cases not yet run in this process are run here."""
    from coivo_amd import _lib
    from tests.test_conv_exact_gpu import PRODUCTION_FORMS
    for ci in range(len(CASES)):
        for dtype in (torch.float32, torch.bfloat16):
            for form in ("form0", "form1", "form2"):
                if (ci, dtype, form) not in _EXACT_SEEN:
                    saved = _set_form(form, dtype)
                    try:
                        _exact_case(ci, dtype, form)
                    finally:
                        _restore(saved)
    if ("wide", torch.bfloat16) not in _EXACT_SEEN:
        test_conv_exact_data_wide_form()
    small = set()
    for hit in _EXACT_SEEN.values():
        small |= {k for k, v in hit.items() if v}
    every = set(_lib.form_counts())
    assert len(every) == 27
    assert small | PRODUCTION_FORMS == every, sorted(every - small - PRODUCTION_FORMS)
    print(f"forms only the production sweep reaches: {sorted(PRODUCTION_FORMS - small)}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pack_roundtrip_and_relu_bwd(dtype):
    from coivo_amd import ops
    d = dev()
    a = torch.rand(2, 3, 6, 10)
    b = torch.rand(2, 1, 6, 10)
    p = ops.pack_nchw([a.to(d), b.to(d)], 8, dtype)
    assert p.shape == (2, 6, 10, 8)
    ref = torch.cat([a, b, torch.zeros(2, 4, 6, 10)], 1).to(dtype)
    assert torch.equal(_nchw(p).cpu(), ref)
    out = torch.full((2, 1, 6, 10), 5.0, device=d)
    ops.unpack_nhwc_grad(p, 3, 1, out, False)
    assert torch.equal(out.cpu(), b.to(dtype).float())
    ops.unpack_nhwc_grad(p, 3, 1, out, True)
    assert torch.allclose(out.cpu(), 2 * b.to(dtype).float())
    y = torch.randn(1000).clamp(min=0).to(d, dtype)
    dy = torch.randn(1000).to(d, dtype)
    ref = dy.clone() * (y > 0)
    ops.relu_bwd_inplace(y, dy)
    assert torch.equal(dy, ref)


def test_pair_conversion_to_bf16_is_torchs_rounding_bit_for_bit():
    """pack2bf (csrc/common.h: one v_cvt_pk_bf16_f32 per pair, in every bf16 epilogue of the library since round 5) against
    Tensor.to(bfloat16) through colvo_cast_f32_bf16, whose vector body uses it and whose tail uses the scalar f2bf(): random values over
    the whole exponent range, exact ties to even in both directions, the largest finite values (rounding to infinity), denormals,
    signed zeros, infinities and NaNs; a length that leaves a scalar tail; and the way back."""
    import ctypes as C
    from coivo_amd import _lib
    g = torch.Generator().manual_seed(5)
    n = 4 * 4099 + 3
    x = torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 12.0)
    bits = torch.randint(0, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    x[: n // 2] = bits[: n // 2].view(torch.float32)                 # arbitrary bit patterns (NaNs, denormals, huge values included)
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,
                            -(1.0 + 2.0 ** -8), 3.3895313892515355e38, 3.4028234663852886e38, 1e-40, -1e-40, 2.0 ** -133])
    x[-special.numel():] = special
    xd = x.to(dev())
    ref = xd.to(torch.bfloat16)
    out = torch.empty(n, device=dev(), dtype=torch.bfloat16)
    lib = _lib.load()
    _lib.check(lib.colvo_cast_f32_bf16(_lib.ptr(xd), _lib.ptr(out), n, 1, _lib.stream_ptr()), "colvo_cast_f32_bf16")
    torch.cuda.synchronize()
    a, b = out.view(torch.int16), ref.view(torch.int16)
    nan = torch.isnan(ref.float())
    assert torch.equal(torch.isnan(out.float()), nan)
    assert torch.equal(a[~nan], b[~nan]), f"{int((a[~nan] != b[~nan]).sum())} of {n} values round differently"
    back = torch.empty(n, device=dev(), dtype=torch.float32)
    _lib.check(lib.colvo_cast_f32_bf16(_lib.ptr(out), _lib.ptr(back), n, 0, _lib.stream_ptr()), "colvo_cast_f32_bf16")
    torch.cuda.synchronize()
    assert torch.equal(back[~nan], ref.float()[~nan])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_depth_head(dtype):
    from coivo_amd import ops
    from oracle import colvo_spec as S
    B, H, W, Cc = 2, 12, 20, 16
    g = torch.Generator().manual_seed(5)
    x = F.relu(torch.randn(B, Cc, H, W, generator=g)).to(dtype).float()
    w = torch.randn(1, 9, Cc, generator=g) * 0.2
    bias = torch.tensor([0.1])
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    pre = F.conv2d(xr, wr.view(1, 3, 3, Cc).permute(0, 3, 1, 2), br, padding=1)
    depth_ref = S.disp_to_depth(torch.sigmoid(pre))
    dd = torch.randn(B, 1, H, W, generator=g)
    depth_ref.backward(dd)
    d = dev()
    xd = _nhwc(x).to(d, dtype)
    depth = torch.empty(B, 1, H, W, device=d)
    ops.depth_head_fwd(xd, w.to(d), bias.to(d), depth)
    tol = 1e-5 if dtype == torch.float32 else 1e-5
    _close(depth, depth_ref, tol, tol, "depth head fwd")
    dx = torch.empty_like(xd)
    dw = torch.zeros(1, 9, Cc, device=d)
    db = torch.zeros(1, device=d)
    scratch = torch.empty(B * H * W, device=d)
    ops.depth_head_bwd(xd, w.to(d), depth, dd.to(d), scratch, dx, dw, db)
    if dtype == torch.float32:
        _close(_nchw(dx), xr.grad * (x > 0), 1e-4, 1e-4, "depth head dx")
    else:       # fp32 arithmetic, one rounding at the bf16 store (round 4: 2e-2 of the largest element)
        _close_out(_nchw(dx), xr.grad * (x > 0), dtype, "depth head dx", atol_scale=1e-4)
    _close(dw, wr.grad, 1e-4, 1e-4, "depth head dw")
    _close(db, br.grad, 1e-4, 1e-4, "depth head db")
    # split form (dx first, then the weight gradient from the d(pre) plane): atomics and the deterministic table form
    outs = []
    for det in (False, True, True):
        dw2, db2 = torch.zeros(1, 9, Cc, device=d), torch.zeros(1, device=d)
        ops.depth_head_bwd(xd, w.to(d), depth, dd.to(d), scratch, dx, None, None)
        ops.depth_head_wgrad(xd, scratch, dw2, db2, det)
        _close(dw2, wr.grad, 1e-4, 1e-4, f"depth head dw (wgrad call, det={det})")
        _close(db2, br.grad, 1e-4, 1e-4, f"depth head db (wgrad call, det={det})")
        outs.append((dw2, db2))
    assert torch.equal(outs[1][0], outs[2][0]) and torch.equal(outs[1][1], outs[2][1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pose_head(dtype):
    from coivo_amd import ops
    from oracle import colvo_spec as S
    B, H, W, Cc = 3, 2, 3, 256
    g = torch.Generator().manual_seed(6)
    x = F.relu(torch.randn(B, Cc, H, W, generator=g)).to(dtype).float()
    w = torch.randn(8, 1, Cc, generator=g) * 0.1
    bias = torch.randn(8, generator=g) * 0.1
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    o = F.conv2d(xr, wr.view(8, Cc, 1, 1), br).mean(dim=(2, 3))
    out_ref = torch.cat([S.POSE_SCALE * o[:, :6], 1 + S.LCC_SCALE * o[:, 6:7], S.LCC_SCALE * o[:, 7:8]], 1)
    do = torch.randn(B, 8, generator=g)
    out_ref.backward(do)
    d = dev()
    xd = _nhwc(x).to(d, dtype)
    out = torch.empty(8 * B, device=d)
    ops.pose_head_fwd(xd, w.to(d), bias.to(d), out)
    got = torch.cat([out[:6 * B].view(B, 6), out[6 * B:7 * B].view(B, 1), out[7 * B:].view(B, 1)], 1)   # planar -> [B,8]
    _close(got, out_ref, 1e-5, 1e-5, "pose head fwd")
    dx = torch.empty_like(xd)
    dw = torch.zeros(8, 1, Cc, device=d)
    db = torch.zeros(8, device=d)
    dod = do.to(d)
    ops.pose_head_bwd(xd, w.to(d), dod[:, :6].contiguous(), dod[:, 6:7].contiguous(), dod[:, 7:8].contiguous(), dx, dw, db)
    if dtype == torch.float32:
        _close(_nchw(dx), xr.grad * (x > 0), 1e-4, 1e-4, "pose head dx")
    else:
        _close_out(_nchw(dx), xr.grad * (x > 0), dtype, "pose head dx", atol_scale=1e-4)
    _close(dw, wr.grad, 1e-4, 1e-4, "pose head dw")
    _close(db, br.grad, 1e-4, 1e-4, "pose head db")
    # deterministic form: no atomics, one thread per weight column walks the images in order
    dx2 = torch.empty_like(xd)
    dw2, db2 = torch.zeros(8, 1, Cc, device=d), torch.zeros(8, device=d)
    ops.pose_head_bwd(xd, w.to(d), dod[:, :6].contiguous(), dod[:, 6:7].contiguous(), dod[:, 7:8].contiguous(), dx2, dw2, db2,
                      deterministic=True)
    assert torch.equal(dx2, dx)
    _close(dw2, wr.grad, 1e-4, 1e-4, "pose head dw (deterministic form)")
    _close(db2, br.grad, 1e-4, 1e-4, "pose head db (deterministic form)")


def test_adam_matches_torch():
    from coivo_amd import ops
    from oracle import colvo_spec as S
    d = dev()
    g = torch.Generator().manual_seed(7)
    n = 100003
    p0 = torch.randn(n, generator=g)
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], **S.ADAM_KW)
    p = p0.to(d)
    m = torch.zeros(n, device=d)
    v = torch.zeros(n, device=d)
    step = torch.zeros(1, dtype=torch.int32, device=d)
    for it in range(3):
        gr = torch.randn(n, generator=g) * 10 ** (it - 1)
        pr.grad = gr.clone()
        opt.step()
        ops.adam_step(p, gr.to(d), m, v, step, lr=S.ADAM_KW["lr"], beta1=S.ADAM_KW["betas"][0],
                      beta2=S.ADAM_KW["betas"][1], eps=S.ADAM_KW["eps"])
    assert int(step.item()) == 3
    assert torch.allclose(p.cpu(), pr.detach(), rtol=1e-6, atol=1e-7)


def test_multi_arena_adam_and_zero_match_the_single_arena_calls():
    """colvo_adam_step_multi / colvo_zero_multi: up to four arenas of ragged lengths in one launch == one call per arena, bit for
    bit; lengths that are not multiples of four take the scalar tail."""
    from coivo_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(11)
    sizes = [100003, 64, 7, 4096 * 5 + 4]
    kw = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=0.5)
    for count in (1, 2, 4):
        arenas_a, arenas_b = [], []
        for n in sizes[:count]:
            base = [torch.randn(n, generator=g), torch.randn(n, generator=g), torch.rand(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01]
            arenas_a.append([t.to(d) for t in base])
            arenas_b.append([t.to(d) for t in base])
        for t in (1, 2, 7):
            ops.adam_step_multi([tuple(a) for a in arenas_a], t, **kw)
            for a in arenas_b:
                ops.adam_step_t(a[0], a[1], a[2], a[3], t, **kw)
        for a, b in zip(arenas_a, arenas_b):
            for x, y in zip(a, b):
                assert torch.equal(x, y)
    bufs = [torch.full((n,), 3.0, device=d) for n in (64, 4096 * 3 + 16, 1 << 20, 4)]
    guard = [torch.full((8,), 5.0, device=d) for _ in bufs]
    ops.zero_multi(bufs)
    assert all(float(b.abs().max()) == 0.0 for b in bufs) and all(float(gd.min()) == 5.0 for gd in guard)
    odd = [torch.full((6,), 1.0, device=d)[1:], torch.full((64,), 1.0, device=d)]      # misaligned / not a multiple of 16 bytes
    ops.zero_multi(odd)                                                                 # falls back to one memset each
    assert all(float(b.abs().max()) == 0.0 for b in odd)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pack_weights_multi_matches_permute(dtype):
    """One-launch packing of several layers (ragged against the 32 x 64 transpose tile) == cast / permute + tap flip."""
    import numpy as np
    from coivo_amd import ops
    d = torch.device("cuda:0")
    shapes = [(32, 8), (40, 72), (16, 16), (136, 200), (8, 64)]        # (Cout, Cin)
    g = torch.Generator().manual_seed(5)
    total = sum(co * 9 * ci for co, ci in shapes)
    master = torch.randn(total + 64, generator=g)                       # 64 spare floats in front: non-zero w_off
    tab = np.zeros(len(shapes), dtype=np.dtype([("w_off", "<i8"), ("fwd_off", "<i8"), ("bwd_off", "<i8"),
                                                ("Cout", "<i4"), ("kk", "<i4"), ("Cin", "<i4"), ("blk", "<i4")]))
    off, blk = 0, 0
    for i, (co, ci) in enumerate(shapes):
        tab[i] = (64 + off, off, off, co, 9, ci, blk)
        off += co * 9 * ci
        blk += 9 * ((co + 31) // 32) * ((ci + 63) // 64)
    fwd = torch.full((total,), 3.0, device=d, dtype=dtype)
    bwd = torch.full((total,), 3.0, device=d, dtype=dtype)
    table = torch.from_numpy(tab.view(np.uint8).copy()).to(d)
    ops.pack_weights_multi(master.to(d), table, len(shapes), blk, dtype, fwd, bwd)
    off = 0
    for co, ci in shapes:
        n = co * 9 * ci
        w = master[64 + off:64 + off + n].view(co, 9, ci)
        assert torch.equal(fwd[off:off + n].cpu().view(co, 9, ci), w.to(dtype)), (co, ci, "fwd")
        ref_b = w.flip(1).permute(2, 1, 0).contiguous().to(dtype)
        assert torch.equal(bwd[off:off + n].cpu().view(ci, 9, co), ref_b), (co, ci, "bwd")
        off += n


@pytest.mark.parametrize("kernel", ["one_tile", "register_tiled"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,C0,C1,Cout", [(2, 16, 20, 32, 32, 32), (2, 32, 40, 64, 64, 64), (1, 24, 24, 64, 32, 48),
                                              (2, 16, 16, 24, 40, 32)])
def test_dgrad_both_sources_equals_two_calls(B, H, W, C0, C1, Cout, dtype, kernel):
    """colvo_conv_dgrad_both (one launch, two outputs) against colvo_conv_dgrad per source; the last case (C0 not a
    multiple of 32) takes the documented fallback.  `register_tiled`: all three launches through k_conv_rt (same summation order
    whatever the channel-tile width, so the two forms stay bit-identical there too)."""
    from coivo_amd import _lib, ops
    if kernel == "register_tiled":      # (the autouse fixture restores the entries)
        _lib.tune_set("rt_min_wgs", 0)
        _lib.tune_set("rt_bn32_min_wgs", 0)
        _lib.tune_set("rt_min_fill_pct", 0)
        _lib.tune_set("rt_min_chunks", 1)
    d = dev()
    g = torch.Generator().manual_seed(B * 1000 + C0 + C1)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dtype)
    x0 = torch.relu(rnd(B, H, W, C0)).to(d)
    x1 = torch.relu(rnd(B, H, W, C1)).to(d)
    dy = rnd(B, H, W, Cout).to(d)
    w = (torch.randn(Cout, 9, C0 + C1, generator=g) * (2.0 / (9 * (C0 + C1))) ** 0.5).to(d)
    w_fwd = torch.empty(Cout, 9, C0 + C1, device=d, dtype=dtype)
    w_bwd = torch.empty(C0 + C1, 9, Cout, device=d, dtype=dtype)
    ops.pack_weights(w, dtype, w_fwd, w_bwd)
    desc = ops.conv_desc(dtype, B, H, W, C0, Cout, C1=C1)
    for masks in ((None, None), (x0, x1)):
        a0, a1 = torch.full_like(x0, 3.0), torch.full_like(x1, 3.0)
        ops.conv_dgrad(desc, 0, dy, w_bwd, masks[0], a0, False)
        ops.conv_dgrad(desc, 1, dy, w_bwd, masks[1], a1, False)
        b0, b1 = torch.full_like(x0, 5.0), torch.full_like(x1, 5.0)
        ops.conv_dgrad_both(desc, dy, w_bwd, masks[0], masks[1], b0, b1)
        assert torch.equal(a0, b0) and torch.equal(a1, b1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", [
    # B, Hi, Wi, C0, Cout, stride, c_begin, c_count
    (2, 64, 96, 8, 16, 2, 6, 2),       # PoseNet conv1: the two depth channels of the 8-channel input
    (1, 13, 21, 8, 16, 2, 6, 2),       # odd extent: ragged last output row / column
    (2, 32, 40, 8, 16, 2, 6, 2),       # (bf16: the MFMA form, 16 blocks per wave step) a block row that ends inside a group of 16
    (3, 4, 2, 8, 16, 2, 0, 2),         # ... a single block column; the first two channels
    (2, 16, 24, 16, 32, 1, 3, 4),      # stride 1, four channels from the middle
    (3, 9, 7, 8, 8, 2, 0, 1),          # one channel
])
def test_input_gradient_of_a_few_channels_as_planes(case, dtype):
    """colvo_conv_dgrad_planes against torch autograd of F.conv2d: the input gradient w.r.t. channels [c_begin, c_begin + c_count)
    only, as fp32 planes [c_count, B, 1, H, W]; fp32 weights in both modes, dy in the feature-map dtype; accumulate adds."""
    from coivo_amd import ops
    B, Hi, Wi, C0, Cout, stride, c_begin, c_count = case
    g = torch.Generator().manual_seed(17)
    d = ops.conv_desc(dtype, B, Hi, Wi, C0, Cout, stride=stride)
    w = torch.randn(Cout, 9, C0, generator=g) * 0.1
    dy = torch.randn(B, Cout, d.Ho, d.Wo, generator=g)
    dy_q = dy.to(dtype).float()                                # what the kernel sees
    x = torch.zeros(B, C0, Hi, Wi, requires_grad=True)
    y = F.conv2d(x, w.view(Cout, 3, 3, C0).permute(0, 3, 1, 2), None, stride=stride, padding=1)
    y.backward(dy_q)
    ref = x.grad[:, c_begin:c_begin + c_count].permute(1, 0, 2, 3).unsqueeze(2).contiguous()       # [c, B, 1, H, W]
    dst = torch.full((c_count, B, 1, Hi, Wi), 7.0, device=dev())
    ops.conv_dgrad_planes(d, _nhwc(dy).to(dev()).to(dtype), w.to(dev()), c_begin, c_count, dst)
    torch.cuda.synchronize()
    scale = ref.abs().max().item()
    assert (dst.cpu() - ref).abs().max().item() < 2e-6 * scale + 1e-6
    ops.conv_dgrad_planes(d, _nhwc(dy).to(dev()).to(dtype), w.to(dev()), c_begin, c_count, dst, accumulate=True)
    torch.cuda.synchronize()
    assert (dst.cpu() - 2 * ref).abs().max().item() < 4e-6 * scale + 2e-6


def test_grouped_weight_gradient_equals_the_per_layer_deterministic_form():
    """colvo_conv_wgrad_slabs + colvo_wgrad_reduce_group (several layers, one second launch) against colvo_conv_wgrad_det per layer:
    the same slabs added in the same order up to the reduction tree -- compared to fp32 round-off -- and bitwise repeatable."""
    from coivo_amd import ops
    g = torch.Generator().manual_seed(23)
    layers = [(2, 16, 24, 32, 0, False, 64, 1), (2, 16, 20, 64, 0, True, 32, 1), (2, 32, 40, 64, 0, False, 128, 2),
              (1, 8, 10, 512, 0, False, 512, 1), (2, 64, 80, 8, 0, False, 32, 2), (2, 16, 20, 32, 32, False, 32, 1)]
    for dtype in (torch.float32, torch.bfloat16):
        sets, refs, outs = [], [], []
        for (B, Hi, Wi, C0, C1, up0, Cout, stride) in layers:
            d = ops.conv_desc(dtype, B, Hi, Wi, C0, Cout, stride=stride, C1=C1, up0=up0)
            hs, ws = (Hi // 2, Wi // 2) if up0 else (Hi, Wi)
            x0 = torch.randn(B, hs, ws, C0, generator=g).to(dev()).to(dtype)
            x1 = torch.randn(B, Hi, Wi, C1, generator=g).to(dev()).to(dtype) if C1 else None
            dy = torch.randn(B, d.Ho, d.Wo, Cout, generator=g).to(dev()).to(dtype)
            dw_ref = torch.ones(Cout, 9, C0 + C1, device=dev())
            db_ref = torch.ones(Cout, device=dev())
            ops.conv_wgrad(d, x0, x1, dy, dw_ref, db_ref, ops.conv_wgrad_scratch(d, dev()))
            dw, db = torch.ones(Cout, 9, C0 + C1, device=dev()), torch.ones(Cout, device=dev())
            scr = ops.conv_wgrad_scratch(d, dev())
            ops.conv_wgrad_slabs(d, x0, x1, dy, scr)
            sets.append((scr, dw, db, ops.conv_wgrad_splits(d), Cout, C0 + C1))
            refs.append((dw_ref, db_ref)); outs.append((dw, db))
        ops.wgrad_reduce_group(sets)
        first = [(a.clone(), b.clone()) for a, b in outs]
        for (a, b), (ra, rb) in zip(outs, refs):
            assert (a - ra).abs().max().item() <= 2e-5 * ra.abs().max().item(), dtype
            assert (b - rb).abs().max().item() <= 2e-5 * rb.abs().max().item() + 1e-6, dtype
        # ... and adding the same slabs again gives exactly twice the increment's bits every time
        for a, b in outs:
            a.fill_(1.0); b.fill_(1.0)
        ops.wgrad_reduce_group(sets)
        torch.cuda.synchronize()
        for (a, b), (fa, fb) in zip(outs, first):
            assert torch.equal(a, fa) and torch.equal(b, fb), dtype


@pytest.mark.parametrize("shape", [(2, 64, 96), (1, 13, 37), (3, 8, 16), (2, 256, 320)])
@pytest.mark.parametrize("relu_mask", [True, False])
def test_fused_backward_of_the_narrow_layer_equals_the_two_kernels(shape, relu_mask):
    """colvo_conv_bwd_fused (bf16, 16 -> 16, stride 1): dx and dw / db against the separate input-gradient and weight-gradient
    kernels on the same operands -- fp32 accumulation in both, so dx agrees to a bf16 rounding of the last bit and dw / db to the
    summation order -- and against torch autograd on the bf16-rounded operands; ragged shapes (tiles are 8 x 16) included."""
    from coivo_amd import ops
    B, H, W = shape
    g = torch.Generator().manual_seed(31)
    dt = torch.bfloat16
    d = ops.conv_desc(dt, B, H, W, 16, 16)
    assert ops.conv_bwd_fused_ok(d)
    x = torch.randn(B, H, W, 16, generator=g).relu().to(dev()).to(dt)           # post-ReLU input: ~half zeros
    dy = torch.randn(B, H, W, 16, generator=g).to(dev()).to(dt)
    w = torch.randn(16, 9, 16, generator=g) * 0.1                               # [Cout][9][Cin]
    w_bwd = w.view(16, 9, 16).flip(1).permute(2, 1, 0).contiguous().to(dev()).to(dt)     # [Cin][9 flipped][Cout]
    # reference: the two kernels
    dx_ref = torch.empty_like(x)
    ops.conv_dgrad(d, 0, dy, w_bwd, x if relu_mask else None, dx_ref, False)
    dw_ref, db_ref = torch.zeros(16, 9, 16, device=dev()), torch.zeros(16, device=dev())
    ops.conv_wgrad(d, x, None, dy, dw_ref, db_ref)
    dx = torch.full_like(x, 3.0)
    dw, db = torch.zeros(16, 9, 16, device=dev()), torch.zeros(16, device=dev())
    ops.conv_bwd_fused(d, dy, w_bwd, x, relu_mask, dx, dw, db)
    torch.cuda.synchronize()
    sx = dx_ref.float().abs().max().item()
    assert (dx.float() - dx_ref.float()).abs().max().item() <= 2.0 ** -7 * sx       # one bf16 ulp of the largest element
    assert ((dx.float() - dx_ref.float()).abs() > 1e-3 * sx).float().mean().item() < 1e-3
    assert (dw - dw_ref).abs().max().item() <= 1e-4 * dw_ref.abs().max().item()
    assert (db - db_ref).abs().max().item() <= 1e-4 * db_ref.abs().max().item() + 1e-4
    # torch autograd on the same bf16-rounded operands
    xt = x.float().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    wt = w.to(dt).float().view(16, 3, 3, 16).permute(0, 3, 1, 2).requires_grad_(True)
    bt = torch.zeros(16, requires_grad=True)
    y = F.conv2d(xt, wt, bt, padding=1)
    y.backward(dy.float().cpu().permute(0, 3, 1, 2))
    gx = xt.grad.permute(0, 2, 3, 1)
    if relu_mask:
        gx = gx * (x.float().cpu() > 0)
    assert (dx.float().cpu() - gx).abs().max().item() <= 2.0 ** -6 * gx.abs().max().item()
    gw = wt.grad.permute(0, 2, 3, 1).reshape(16, 9, 16)
    assert (dw.cpu() - gw).abs().max().item() <= 2e-4 * gw.abs().max().item()
    assert (db.cpu() - bt.grad).abs().max().item() <= 2e-4 * bt.grad.abs().max().item() + 1e-4
    # accumulation into dw / db
    ops.conv_bwd_fused(d, dy, w_bwd, x, relu_mask, dx, dw, db)
    torch.cuda.synchronize()
    assert (dw - 2 * dw_ref).abs().max().item() <= 2e-4 * dw_ref.abs().max().item()


@pytest.mark.parametrize("shape", [(2, 64, 96), (1, 13, 37), (2, 256, 320)])
def test_fused_backward_with_the_depth_head_gradient_made_on_the_fly(shape):
    """colvo_conv_bwd_fused, HEAD form: `dy` is the layer's OUTPUT y and the gradient g = (y > 0) * (dpre (*) head_w) is made inside the
    kernel from the depth head's d(pre) plane -- against the same call fed with g computed by torch (conv of dpre with the flipped head
    weights, masked, rounded to bf16 as the head's own input-gradient kernel stores it)."""
    from coivo_amd import ops
    B, H, W = shape
    gen = torch.Generator().manual_seed(37)
    dt = torch.bfloat16
    d = ops.conv_desc(dt, B, H, W, 16, 16)
    x = torch.randn(B, H, W, 16, generator=gen).relu().to(dev()).to(dt)
    y = torch.randn(B, H, W, 16, generator=gen).relu().to(dev()).to(dt)                 # the layer's output (post-ReLU)
    dpre = torch.randn(B, H, W, generator=gen).to(dev())
    wh = (torch.randn(1, 9, 16, generator=gen) * 0.2).to(dev())                          # head weights [1][9][16]
    w = torch.randn(16, 9, 16, generator=gen) * 0.1
    w_bwd = w.flip(1).permute(2, 1, 0).contiguous().to(dev()).to(dt)
    # g[b, p, c] = sum_t wh[t][c] * dpre[p + 1 - t]  ==  conv2d(dpre, kernel[c][0][ky][kx] = wh[(2 - ky) * 3 + (2 - kx)][c], padding 1)
    k = wh[0].view(3, 3, 16).flip(0, 1).permute(2, 0, 1).unsqueeze(1).contiguous()       # [16, 1, 3, 3]
    g = F.conv2d(dpre.unsqueeze(1), k, padding=1).permute(0, 2, 3, 1)                      # [B, H, W, 16] fp32
    g = (g * (y.float() > 0)).to(dt).contiguous()
    dx_ref, dw_ref, db_ref = torch.empty_like(x), torch.zeros(16, 9, 16, device=dev()), torch.zeros(16, device=dev())
    ops.conv_bwd_fused(d, g, w_bwd, x, True, dx_ref, dw_ref, db_ref)
    dx, dw, db = torch.full_like(x, 5.0), torch.zeros(16, 9, 16, device=dev()), torch.zeros(16, device=dev())
    ops.conv_bwd_fused(d, y, w_bwd, x, True, dx, dw, db, dpre, wh)
    torch.cuda.synchronize()
    sx = dx_ref.float().abs().max().item()
    # g itself may differ in the last bf16 bit where the two summation orders round differently: a few elements, one ulp each
    assert (dx.float() - dx_ref.float()).abs().max().item() <= 2.0 ** -6 * sx
    assert ((dx.float() - dx_ref.float()).abs() > 2e-3 * sx).float().mean().item() < 2e-3
    assert (dw - dw_ref).abs().max().item() <= 2e-3 * dw_ref.abs().max().item()
    assert (db - db_ref).abs().max().item() <= 2e-3 * db_ref.abs().max().item() + 1e-3


@pytest.mark.parametrize("shape", [(2, 64, 96), (1, 13, 37), (2, 256, 320)])
def test_fused_backward_carries_the_depth_heads_weight_gradient(shape):
    """colvo_conv_bwd_fused with head_partials: the head's dw [9][16] / db [1] from the partial rows (colvo_depth_head_wgrad_reduce)
    against colvo_depth_head_wgrad on the same y and d(pre) (the fold rounds d(pre) to bf16 for its MFMA: 2^-9 per term), and dx / dw
    of the layer unchanged by the extra output (bitwise dx)."""
    from coivo_amd import _lib, ops
    import ctypes as C
    B, H, W = shape
    gen = torch.Generator().manual_seed(41)
    dt = torch.bfloat16
    d = ops.conv_desc(dt, B, H, W, 16, 16)
    x = torch.randn(B, H, W, 16, generator=gen).relu().to(dev()).to(dt)
    y = torch.randn(B, H, W, 16, generator=gen).relu().to(dev()).to(dt)
    dpre = torch.randn(B, H, W, generator=gen).to(dev())
    wh = (torch.randn(1, 9, 16, generator=gen) * 0.2).to(dev())
    w_bwd = (torch.randn(16, 9, 16, generator=gen) * 0.1).to(dev()).to(dt)
    dx0, dw0, db0 = torch.empty_like(x), torch.zeros(16, 9, 16, device=dev()), torch.zeros(16, device=dev())
    ops.conv_bwd_fused(d, y, w_bwd, x, True, dx0, dw0, db0, dpre, wh)
    rows = ops.conv_bwd_fused_head_rows(d)
    assert rows >= 4 and rows % 4 == 0
    hp = torch.full((rows * 145,), float("nan"), device=dev())
    dx1, dw1, db1 = torch.empty_like(x), torch.zeros(16, 9, 16, device=dev()), torch.zeros(16, device=dev())
    ops.conv_bwd_fused(d, y, w_bwd, x, True, dx1, dw1, db1, dpre, wh, hp)
    hdw, hdb = torch.zeros(1, 9, 16, device=dev()), torch.zeros(1, device=dev())
    ops.depth_head_wgrad_reduce(hp, rows, hdw, hdb)
    rdw, rdb = torch.zeros(1, 9, 16, device=dev()), torch.zeros(1, device=dev())
    ops.depth_head_wgrad(y, dpre, rdw, rdb)
    torch.cuda.synchronize()
    assert torch.equal(dx0, dx1)
    assert (dw0 - dw1).abs().max().item() <= 1e-4 * dw0.abs().max().item()
    assert torch.isfinite(hp).all()
    assert (hdw - rdw).abs().max().item() <= 4e-3 * rdw.abs().max().item(), ((hdw - rdw).abs().max().item(), rdw.abs().max().item())
    assert abs(hdb.item() - rdb.item()) <= 1e-4 * max(1.0, abs(rdb.item())) + 1e-3 * dpre.abs().sum().item() * 1e-4


@pytest.mark.parametrize("shape", [(2, 64, 96), (1, 13, 37), (3, 8, 16), (2, 256, 320)])
def test_fused_layer_and_depth_head_forward_equals_the_two_kernels(shape):
    """colvo_conv_head_fused (bf16, 16 -> 16 + the 3x3 16 -> 1 depth head): y against colvo_conv_fwd (same fp32 accumulation up to the
    summation order: a bf16 rounding of the last bit on a few elements), depth against colvo_depth_head_fwd on that y."""
    from coivo_amd import ops
    B, H, W = shape
    gen = torch.Generator().manual_seed(43)
    dt = torch.bfloat16
    d = ops.conv_desc(dt, B, H, W, 16, 16)
    assert ops.conv_head_fused_ok(d)
    x = torch.randn(B, H, W, 16, generator=gen).relu().to(dev()).to(dt)
    w = (torch.randn(16, 9, 16, generator=gen) * 0.15).to(dev()).to(dt)                  # [Cout][9][Cin]
    bias = (torch.randn(16, generator=gen) * 0.1).to(dev())
    wh = (torch.randn(1, 9, 16, generator=gen) * 0.2).to(dev())
    bh = torch.tensor([0.3], device=dev())
    y_ref = torch.empty(B, H, W, 16, device=dev(), dtype=dt)
    ops.conv_fwd(d, x, None, w, bias, y_ref)
    depth_ref = torch.empty(B, 1, H, W, device=dev())
    ops.depth_head_fwd(y_ref, wh, bh, depth_ref)
    y = torch.full_like(y_ref, 9.0)
    depth = torch.full_like(depth_ref, -1.0)
    ops.conv_head_fused(d, x, w, bias, wh, bh, y, depth)
    torch.cuda.synchronize()
    sy = y_ref.float().abs().max().item()
    assert (y.float() - y_ref.float()).abs().max().item() <= 2.0 ** -7 * sy
    assert ((y.float() - y_ref.float()).abs() > 0).float().mean().item() < 2e-3
    # depth in (0.1, 10): compare 1 / depth (the sigmoid's scale); the few y elements that differ by one bf16 ulp move it by ~1e-3 relative
    inv, inv_ref = 1.0 / depth, 1.0 / depth_ref
    assert (depth > 0.0999).all() and (depth < 10.001).all()
    assert (inv - inv_ref).abs().max().item() <= 2e-2 and ((inv - inv_ref).abs() > 1e-4).float().mean().item() < 5e-3


@pytest.mark.parametrize("shape", [(1, 64, 96), (3, 8, 16), (2, 13, 37)])
def test_pose_input_filled_by_stem_pack_and_depth_head_is_bit_identical(shape):
    """colvo_pack_stem_pose + the pose_in argument of colvo_conv_head_fused assemble PoseNet's input [tgt rgb | ref rgb | depth_t |
    depth_r] (bf16): bit for bit what colvo_pack_nchw makes from the frames and the depth this pass wrote; the stem input too."""
    from coivo_amd import ops
    Bp, H, W = shape                                     # pairs
    gen = torch.Generator().manual_seed(53)
    dt = torch.bfloat16
    frames = torch.rand(2 * Bp, 3, H, W, generator=gen).to(dev())
    stem = torch.full((2 * Bp, H, W, 8), 7.0, device=dev(), dtype=dt)
    pose_in = torch.full((Bp, H, W, 8), 5.0, device=dev(), dtype=dt)
    ops.pack_stem_pose(frames, stem, pose_in)
    assert torch.equal(stem, ops.pack_nchw([frames], 8, dt))
    d = ops.conv_desc(dt, 2 * Bp, H, W, 16, 16)
    x = torch.randn(2 * Bp, H, W, 16, generator=gen).relu().to(dev()).to(dt)
    w = (torch.randn(16, 9, 16, generator=gen) * 0.15).to(dev()).to(dt)
    bias = (torch.randn(16, generator=gen) * 0.1).to(dev())
    wh = (torch.randn(1, 9, 16, generator=gen) * 0.2).to(dev())
    bh = torch.tensor([0.3], device=dev())
    y, depth = torch.empty_like(x), torch.empty(2 * Bp, 1, H, W, device=dev())
    y0, depth0 = torch.empty_like(x), torch.empty_like(depth)
    ops.conv_head_fused(d, x, w, bias, wh, bh, y0, depth0)
    ops.conv_head_fused(d, x, w, bias, wh, bh, y, depth, pose_in)
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and torch.equal(depth, depth0)
    want = ops.pack_nchw([frames[:Bp].contiguous(), frames[Bp:].contiguous(), depth[:Bp].contiguous(), depth[Bp:].contiguous()], 8, dt)
    assert torch.equal(pose_in.view(torch.int16), want.view(torch.int16))
    with pytest.raises(RuntimeError):                    # an odd image count is not a pair batch
        d3 = ops.conv_desc(dt, 3, H, W, 16, 16)
        ops.conv_head_fused(d3, x[:3].contiguous(), w, bias, wh, bh, y[:3].contiguous(), depth[:3].contiguous(), pose_in)


@pytest.mark.parametrize("shape", [(2, 64, 96), (1, 13, 37), (2, 256, 320)])
def test_depth_head_weight_gradient_by_mfma(shape):
    """colvo_depth_head_wgrad_mfma (+ the table reduction) against the VALU kernel colvo_depth_head_wgrad on the same y and d(pre):
    the MFMA form rounds d(pre) to bf16 (2^-9 per term); added to dw / db, bitwise repeatable."""
    from coivo_amd import ops
    B, H, W = shape
    gen = torch.Generator().manual_seed(47)
    y = torch.randn(B, H, W, 16, generator=gen).relu().to(dev()).to(torch.bfloat16)
    dpre = torch.randn(B, H, W, generator=gen).to(dev())
    rdw, rdb = torch.ones(1, 9, 16, device=dev()), torch.ones(1, device=dev())
    ops.depth_head_wgrad(y, dpre, rdw, rdb)
    outs = []
    for _ in range(2):
        dw, db = torch.ones(1, 9, 16, device=dev()), torch.ones(1, device=dev())
        ops.depth_head_wgrad_mfma(y, dpre, dw, db)
        torch.cuda.synchronize()
        outs.append((dw, db))
    dw, db = outs[0]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    scale = (rdw - 1).abs().max().item()
    assert (dw - rdw).abs().max().item() <= 4e-3 * scale, ((dw - rdw).abs().max().item(), scale)
    assert abs(db.item() - rdb.item()) <= 1e-4 * abs(rdb.item() - 1) + 2e-3
