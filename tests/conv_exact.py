"""Exact-data checks of the conv kernels: operands that are small integers times a power-of-two quantum, so that every product
and every partial sum is exact in fp32 whatever the summation order -- as long as the sum of |terms| of each output element,
counted in quanta, stays below 2^24.  Any correct kernel (MFMA tiling, split-K, pixel-range splits, fp32 atomics, slabs, image
slices) then returns the exact result bit for bit, a float64 reference is exact as well, and a bf16 output is one round-to-nearest-
even of that exact value.  The bar is equality by value (-0.0 == +0.0), no tolerance.

Value sets (quanta):
    sources x        {0, 1, 2, 3} * 2^-2, drawn from {-3..3} clamped at 0 (4 / 7 zeros, like ReLU outputs)
    master weights   [-8, 8] * 2^-4       (exact in bf16)
    bias             [-16, 16] * 2^-6     (the product quantum: pre-activations are multiples of 2^-6, many exactly 0)
    dy               {-2, -1, 1, 2} * 2^-3 with density rho (dense: rho = 1/2)
    accumulate base  [-64, 64] * 2^-7
The weight gradient sums B * Ho * Wo products per element: rho is chosen from that pixel count so that
max|x| * sum_p |dy[p, co]| stays within 2^22 quanta (headroom for the accumulating second call and for the bf16 MFMA, whose exact
addition of representable partial sums is assumed, not documented).  bound_* state the bounds analytically (tests/test_abi_cpu.py
checks them for every production descriptor); check_wgrad_bound measures the drawn tensors before anything is compared."""
import ctypes
import math

import torch
import torch.nn.functional as F

QX, QW, QB, QDY, QBASE = 2.0 ** -2, 2.0 ** -4, 2.0 ** -6, 2.0 ** -3, 2.0 ** -7
X_MAX, W_MAX, B_MAX, DY_MAX, BASE_MAX = 3, 8, 16, 2, 64        # largest |value| of each set, in its quantum
BOUND = 2 ** 22                                                 # quanta; fp32 is exact below 2^24
RHO_MAX = 0.5


def dy_density(npix: int) -> float:
    """Density of the non-zero dy elements of a weight-gradient check over npix = B * Ho * Wo output pixels: the expected
    sum_p |dy_q| * X_MAX is at most 3 / 4 of BOUND (E|dy_q| <= DY_MAX)."""
    return min(RHO_MAX, BOUND / (X_MAX * DY_MAX * npix) * 0.75)


def bound_wgrad(npix: int) -> float:
    """Worst sum of |terms| (quanta of QX * QDY) of a weight-gradient element: every non-zero dy at DY_MAX and a count of non-zeros six
    standard deviations above its mean (binomial), times X_MAX; the bias gradient's sum is smaller (no X_MAX)."""
    rho = dy_density(npix)
    n = rho * npix + 6.0 * math.sqrt(rho * (1 - rho) * npix) + 1
    return X_MAX * DY_MAX * n


def bound_fwd(cin: int) -> int:
    """Pre-activation, quanta of QX * QW = QB: 9 taps x Cin products and the bias."""
    return 9 * cin * X_MAX * W_MAX + B_MAX


def bound_dgrad(cout: int, up: bool) -> int:
    """Input gradient, quanta of QDY * QW = QBASE: 9 taps x Cout products (x 4 output pixels per stored pixel of an up-sampled
    source) and the accumulate base."""
    return (4 if up else 1) * 9 * cout * DY_MAX * W_MAX + BASE_MAX


def _ints(lo, hi, shape, g, device):
    return torch.randint(lo, hi + 1, shape, generator=g, device=device, dtype=torch.int32).float()


def make_source(shape, g, device):
    return _ints(-X_MAX, X_MAX, shape, g, device).clamp_(min=0) * QX


def make_weights(cout, cin, g, device):
    return _ints(-W_MAX, W_MAX, (cout, 9, cin), g, device) * QW


def make_bias(cout, g, device):
    return _ints(-B_MAX, B_MAX, (cout,), g, device) * QB


def make_dy(shape, rho, g, device):
    v = _ints(1, DY_MAX, shape, g, device) * torch.where(torch.rand(shape, generator=g, device=device) < 0.5, -1.0, 1.0)
    keep = torch.rand(shape, generator=g, device=device) < rho
    return (v * keep) * QDY


def make_base(shape, g, device):
    return _ints(-BASE_MAX, BASE_MAX, shape, g, device) * QBASE


def check_wgrad_bound(x_list, dy, what):
    """The measured bound of a weight-gradient check: max|x| (quanta) * max over co of sum_p |dy[., co]| (quanta) <= BOUND."""
    xm = max(float(x.abs().max()) for x in x_list if x is not None) / QX
    col = dy.abs().sum(dim=tuple(range(dy.dim() - 1)), dtype=torch.float64) / QDY
    worst = xm * float(col.max())
    assert worst <= BOUND, f"{what}: weight-gradient sum of |terms| {worst:.0f} quanta > 2^22 -- outside the exact regime"
    return worst


# ------------------------------------------------------------------------------------------------------------------------------- #
# float64 reference (NHWC in, NHWC / [Cout][9][Cin] out), processed in image slices: fp64 sums of exact slices stay exact           #
# ------------------------------------------------------------------------------------------------------------------------------- #
def _nchw64(t):
    return t.permute(0, 3, 1, 2).double()


def _up(t):
    return t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def _w4(w):                                  # [Cout][9][Cin] -> [Cout][Cin][3][3]
    co, _, ci = w.shape
    return w.double().view(co, 3, 3, ci).permute(0, 3, 1, 2)


def image_slices(B, per_image_elems, cap=1 << 27):
    n = max(1, cap // max(1, per_image_elems))
    return [(b, min(B, b + n)) for b in range(0, B, n)]


class Layer:
    """One conv layer: B, Hi, Wi, C0, C1, up0, up1, Cout, stride (Hi / Wi: the conv input's extent, an up-sampled source is stored at
    half of it)."""

    def __init__(self, B, Hi, Wi, C0, C1, up0, up1, Cout, stride):
        self.B, self.Hi, self.Wi, self.C0, self.C1, self.up0, self.up1 = B, Hi, Wi, C0, C1, bool(up0), bool(up1)
        self.Cout, self.stride = Cout, stride
        self.Ho, self.Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
        self.Cin = C0 + C1

    @staticmethod
    def of_desc(d):
        return Layer(d.B, d.Hi, d.Wi, d.C0, d.C1, d.up0, d.up1, d.Cout, d.stride)

    def stored(self, src):
        C, up = (self.C0, self.up0) if src == 0 else (self.C1, self.up1)
        return (self.B, self.Hi // 2, self.Wi // 2, C) if up else (self.B, self.Hi, self.Wi, C)

    def _input(self, x0, x1, b0, b1):
        xs = [_up(_nchw64(x0[b0:b1])) if self.up0 else _nchw64(x0[b0:b1])]
        if self.C1:
            xs.append(_up(_nchw64(x1[b0:b1])) if self.up1 else _nchw64(x1[b0:b1]))
        return torch.cat(xs, 1) if len(xs) > 1 else xs[0]

    def slices(self):
        return image_slices(self.B, max(self.Hi * self.Wi * self.Cin, self.Ho * self.Wo * self.Cout))

    def ref_fwd(self, x0, x1, w, bias, b0, b1):
        """ReLU(conv) of images [b0, b1), NHWC float64."""
        y = F.conv2d(self._input(x0, x1, b0, b1), _w4(w), bias.double(), stride=self.stride, padding=1)
        return y.clamp_(min=0).permute(0, 2, 3, 1)

    def ref_dgrad(self, dy, w, b0, b1):
        """(dx0, dx1) of images [b0, b1) at the stored resolution of each source, NHWC float64, unmasked."""
        g = torch.nn.grad.conv2d_input((b1 - b0, self.Cin, self.Hi, self.Wi), _w4(w), _nchw64(dy[b0:b1]), stride=self.stride,
                                       padding=1)
        out = []
        for gs, up in ((g[:, :self.C0], self.up0), (g[:, self.C0:], self.up1)):
            if gs.shape[1] == 0:
                out.append(None)
                continue
            if up:
                n, c, h, wd = gs.shape
                gs = gs.reshape(n, c, h // 2, 2, wd // 2, 2).sum(dim=(3, 5))
            out.append(gs.permute(0, 2, 3, 1))
        return out

    def ref_wgrad(self, x0, x1, dy):
        """(dw [Cout][9][Cin], db [Cout]) float64 over the whole batch."""
        dw = torch.zeros(self.Cout, self.Cin, 3, 3, dtype=torch.float64, device=dy.device)
        db = torch.zeros(self.Cout, dtype=torch.float64, device=dy.device)
        for b0, b1 in self.slices():
            g = _nchw64(dy[b0:b1])
            dw += torch.nn.grad.conv2d_weight(self._input(x0, x1, b0, b1), dw.shape, g, stride=self.stride, padding=1)
            db += g.sum(dim=(0, 2, 3))
        return dw.permute(0, 2, 3, 1).reshape(self.Cout, 9, self.Cin), db


def layers(net, B, H, W):
    """(name, Layer) of every conv of DepthNet (DepthNet._plan) or of PoseNet's stride-2 chain at batch B (frames / pairs)."""
    import types
    from coivo_amd import nn as hnn
    if net == "depth":
        plan = hnn.DepthNet._plan(types.SimpleNamespace(compute_dtype=torch.bfloat16, _plans={}), B, H, W)
        return [(name, Layer.of_desc(d)) for name, d in plan.items()]
    out, h, w, cin = [], H, W, 8
    for i, c in enumerate(hnn.POSE_CH, start=1):
        lay = Layer(B, h, w, cin, 0, False, False, c, 2)
        out.append((f"conv{i}", lay))
        h, w, cin = lay.Ho, lay.Wo, c
    return out


# The inference batch sizes of tests/test_conv_exact_small_batch_gpu.py (why each: its docstring); tests/test_abi_cpu.py holds the
# exact-regime bounds for them.
SMALL_BATCH_SHAPES = [("depth", 1, 256, 320), ("pose", 1, 256, 320), ("depth", 3, 256, 320), ("pose", 3, 256, 320),
                      ("depth", 5, 256, 320), ("depth", 13, 256, 320), ("pose", 13, 256, 320),
                      ("depth", 1, 512, 640), ("depth", 3, 512, 640), ("pose", 1, 512, 640)]


def expect_exact(got, ref, quantum, what):
    """got (kernel dtype) == ref (float64, exact) rounded once to got's dtype, by value.  On failure: the number of mismatching
    elements, the largest difference in quanta and the first bad index (NHWC: b, y, x, c)."""
    r32 = ref.float()
    assert torch.equal(r32.double(), ref), f"{what}: the reference left the exact fp32 regime"
    want = r32.to(got.dtype) if got.dtype == torch.bfloat16 else r32
    bad = got != want
    if bool(bad.any()):
        n = int(bad.sum())
        diff = (got.double() - want.double()).abs()
        diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
        first = [int(i) for i in bad.nonzero()[0].tolist()]
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ; largest difference {float(diff.max()) / quantum:.6g} "
                             f"quanta of {quantum:g}; first bad index {tuple(first)} (got {float(got[tuple(first)])}, "
                             f"want {float(want[tuple(first)])})")


def forms_diff(before, after):
    return {k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)}


FWD_LEAVES = {"conv_rt", "conv_q", "conv_up2_bn16", "conv_up2_bn32", "conv_tile", "conv_ring", "conv_wide", "conv_res", "conv_res_s2"}
DGRAD_LEAVES = {"dgrad_s2", "dgrad_s2_ring", "dgrad_up2", "conv_rt", "conv_q", "conv_tile", "conv_ring", "conv_wide", "conv_res"}
WGRAD_LEAVES = {"wgrad_rt", "wgrad_up2", "wgrad_teams", "wgrad_tail"}


def leaves(forms, kinds):
    return {k: v for k, v in forms.items() if k in kinds}


def wgrad_slices(lay, dtype):
    """How many image slices colvo_conv_wgrad processes (csrc/wgrad.hip wgrad_impl: every tensor below 1 GiB)."""
    es = 4 if dtype == torch.float32 else 2
    per_img = max(lay.Ho * lay.Wo * lay.Cout, lay.Hi * lay.Wi * max(lay.C0, lay.C1)) * es
    bmax = max(1, (2 ** 30 - 1) // per_img)
    return 1 if lay.B <= bmax else -(-lay.B // bmax)


def _ref(data, key, fn):
    """The float64 reference `key` of a layer, computed once and shared between the dtypes that use the same operands."""
    refs = data.setdefault("refs", {})
    if key not in refs:
        refs[key] = fn()
    return refs[key]


def check_layer(lay, dtype, g, dev, fused=True, data=None):
    """Every pass of `lay` in `dtype` on exact data against the float64 reference: forward with ReLU, input gradient of each source
    plain and masked + accumulate, both sources in one launch (concat layers), weight / bias gradient in the atomic, clean-arena,
    deterministic (twice) and slab + grouped-reduction forms, plus the accumulating second call; the fused kernels where their _ok
    allows them.  Returns {pass: forms counted}.  `data`: operands shared between the dtypes of one layer (made here when None).
    Every operand is a guarded copy (tests/guarded.py Pool.place) and every destination and scratch comes from the pool, poisoned with
    0xFF bytes (NaN): an element a kernel leaves unwritten fails the comparison, a load from outside an operand that reaches a sum makes
    it NaN, and the guards of everything live are checked after each pass."""
    from coivo_amd import _lib, ops
    from tests import guarded
    pool = guarded.Pool(dev)
    data = data if data is not None else make_data(lay, g, dev)
    x0f, x1f, wm, bias, dyd_f, dyw_f, hw = (data[k] for k in ("x0", "x1", "w", "bias", "dy_dense", "dy_wgrad", "head_w"))
    desc = ops.conv_desc(dtype, lay.B, lay.Hi, lay.Wi, lay.C0, lay.Cout, stride=lay.stride, relu=True, C1=lay.C1, up0=lay.up0,
                         up1=lay.up1)
    cast = lambda t: None if t is None else t.to(dtype)
    x0, x1, dyd, dyw = (pool.place(cast(t), n) for t, n in ((x0f, "x0"), (x1f, "x1"), (dyd_f, "dy dense"), (dyw_f, "dy wgrad")))
    wm_g, bias, hw = pool.place(wm, "master weights"), pool.place(bias, "bias"), pool.place(hw, "head weights")
    w_fwd = pool.empty((lay.Cout, 9, lay.Cin), dtype, label="w_fwd")
    w_bwd = pool.empty((lay.Cin, 9, lay.Cout), dtype, label="w_bwd")
    ops.pack_weights(wm_g, dtype, w_fwd, w_bwd)
    tag = f"{lay.__dict__} {dtype}"
    pool.check(f"pack_weights {tag}", release=False)
    assert torch.equal(w_fwd.float(), wm)
    forms = {}
    poisoned = lambda like, label: pool.empty(like.shape, like.dtype, label=label)

    def run(name, fn):
        torch.cuda.synchronize()
        before = _lib.form_counts()
        fn()
        torch.cuda.synchronize()
        forms[name] = forms_diff(before, _lib.form_counts())
        pool.check(f"{name} {tag}", release=False)

    # ---- forward ----
    y = pool.empty((lay.B, lay.Ho, lay.Wo, lay.Cout), dtype, label="y")
    run("fwd", lambda: ops.conv_fwd(desc, x0, x1, w_fwd, bias, y))
    yh = None
    if fused and ops.conv_head_fused_ok(desc):
        yh = poisoned(y, "conv_head_fused y")
        depth = pool.empty((lay.B, 1, lay.Ho, lay.Wo), torch.float32, label="conv_head_fused depth")
        hb = pool.filled((1,), 0.0, label="head bias")
        run("fwd16_head", lambda: ops.conv_head_fused(desc, x0, w_fwd, bias, hw, hb, yh, depth))
        assert bool(torch.isfinite(depth).all()), f"conv_head_fused depth {tag}: elements left unwritten"
        pool.forget(depth, hb)
        del depth, hb
    for b0, b1 in lay.slices():
        r = _ref(data, ("fwd", b0), lambda: lay.ref_fwd(x0f, x1f, wm, bias, b0, b1))
        expect_exact(y[b0:b1], r, QB, f"fwd {tag} images {b0}..{b1}")
        if yh is not None:
            expect_exact(yh[b0:b1], r, QB, f"conv_head_fused y {tag} images {b0}..{b1}")
    pool.forget(y, yh)
    del y, yh

    # ---- input gradients ----
    srcs = [(0, x0, x0f), (1, x1, x1f)] if lay.C1 else [(0, x0, x0f)]
    outs = {}
    for si, xs, _ in srcs:
        dx = poisoned(xs, f"dx{si}")
        run(f"dgrad{si}", lambda: ops.conv_dgrad(desc, si, dyd, w_bwd, None, dx, False))
        base = make_base(xs.shape, g, dev).to(dtype)
        dxm = pool.place(base, f"dx{si} masked + accumulate")
        run(f"dgrad{si}_masked_acc", lambda: ops.conv_dgrad(desc, si, dyd, w_bwd, xs, dxm, True))
        outs[si] = (dx, base, dxm)
    both = None
    if lay.C1:
        both = (poisoned(x0, "dgrad_both dx0"), poisoned(x1, "dgrad_both dx1"))
        run("dgrad_both", lambda: ops.conv_dgrad_both(desc, dyd, w_bwd, x0, x1, both[0], both[1]))
    planes = None
    if fused and lay.stride == 2 and lay.C0 == 8 and lay.C1 == 0 and lay.Cout == 16:      # PoseNet conv1: the two depth channels
        planes = pool.empty((2, lay.B, 1, lay.Hi, lay.Wi), torch.float32, label="planes")
        run("dgrad_planes", lambda: ops.conv_dgrad_planes(desc, dyd, wm_g, 6, 2, planes))
    for b0, b1 in lay.slices():
        refs = _ref(data, ("dgrad", b0), lambda: lay.ref_dgrad(dyd_f, wm, b0, b1))
        for si, xs, xsf in srcs:
            dx, base, dxm = outs[si]
            expect_exact(dx[b0:b1], refs[si], QBASE, f"dgrad src{si} {tag} images {b0}..{b1}")
            masked = base[b0:b1].double() + refs[si] * (xsf[b0:b1] > 0)
            expect_exact(dxm[b0:b1], masked, QBASE, f"dgrad src{si} masked+accumulate {tag} images {b0}..{b1}")
            if both is not None:
                expect_exact(both[si][b0:b1], refs[si] * (xsf[b0:b1] > 0), QBASE, f"dgrad_both src{si} {tag} images {b0}..{b1}")
        if planes is not None:
            expect_exact(planes[:, b0:b1, 0], refs[0][..., 6:8].permute(3, 0, 1, 2), QBASE,
                         f"conv_dgrad_planes {tag} images {b0}..{b1}")
    pool.forget(planes, *(both or ()), *(t for dx, _, dxm in outs.values() for t in (dx, dxm)))
    del outs, both, planes

    # ---- weight / bias gradient ----
    check_wgrad_bound([x0f, x1f], dyw_f, tag)
    rdw, rdb = _ref(data, "wgrad", lambda: lay.ref_wgrad(x0f, x1f, dyw_f))
    qw = QX * QDY
    zeros = lambda: (pool.filled((lay.Cout, 9, lay.Cin), 0.0, label="dw"), pool.filled((lay.Cout,), 0.0, label="db"))
    dw, db = zeros()
    run("wgrad", lambda: ops.conv_wgrad(desc, x0, x1, dyw, dw, db))
    expect_exact(dw, rdw, qw, f"wgrad (atomics) {tag}")
    expect_exact(db, rdb, QDY, f"bgrad (atomics) {tag}")
    run("wgrad_acc", lambda: ops.conv_wgrad(desc, x0, x1, dyw, dw, db))
    expect_exact(dw, 2 * rdw, qw, f"wgrad (atomics) accumulate {tag}")
    expect_exact(db, 2 * rdb, QDY, f"bgrad (atomics) accumulate {tag}")
    dwc, dbc = zeros()
    run("wgrad_clean", lambda: ops.conv_wgrad(desc, x0, x1, dyw, dwc, dbc, arena_is_zero=True))
    expect_exact(dwc, rdw, qw, f"wgrad (clean arena) {tag}")
    expect_exact(dbc, rdb, QDY, f"bgrad (clean arena) {tag}")
    with guarded.guarded_allocations(pool):          # the slabs: colvo_conv_wgrad_scratch_bytes and not a byte more
        served = len(pool.served)
        scr = ops.conv_wgrad_scratch(desc, dev)
    nb = _lib.load().colvo_conv_wgrad_scratch_bytes(ctypes.byref(desc))
    guarded.assert_served(pool, served, (nb + 3) // 4 * 4, f"conv_wgrad_scratch {tag}")
    dets = []
    for i in range(2):
        dwd, dbd = zeros()
        run(f"wgrad_det{i}", lambda: ops.conv_wgrad(desc, x0, x1, dyw, dwd, dbd, scr))
        expect_exact(dwd, rdw, qw, f"wgrad (deterministic, call {i}) {tag}")
        expect_exact(dbd, rdb, QDY, f"bgrad (deterministic, call {i}) {tag}")
        dets.append((dwd, dbd))
    assert torch.equal(dets[0][0], dets[1][0]) and torch.equal(dets[0][1], dets[1][1]), tag
    if wgrad_slices(lay, dtype) == 1:          # (colvo_conv_wgrad_slabs refuses a batch it would slice)
        dwg, dbg = zeros()

        def grouped():
            ops.conv_wgrad_slabs(desc, x0, x1, dyw, scr)
            ops.wgrad_reduce_group([(scr, dwg, dbg, ops.conv_wgrad_splits(desc), lay.Cout, lay.Cin)])
        run("wgrad_slabs", grouped)
        expect_exact(dwg, rdw, qw, f"wgrad (slabs + grouped reduction) {tag}")
        expect_exact(dbg, rdb, QDY, f"bgrad (slabs + grouped reduction) {tag}")
    pool.forget(dw, db, dwc, dbc, scr, *(t for d in dets for t in d))
    del dw, db, dwc, dbc, dets, scr
    if fused and ops.conv_bwd_fused_ok(desc):
        # the 16 -> 16 layer's input and weight gradient in one pass (without the head term), on the sparse dy of the weight gradient
        dx = poisoned(x0, "conv_bwd_fused dx")
        dwf, dbf = zeros()
        run("bwd16", lambda: ops.conv_bwd_fused(desc, dyw, w_bwd, x0, True, dx, dwf, dbf))
        expect_exact(dwf, rdw, qw, f"conv_bwd_fused dw {tag}")
        expect_exact(dbf, rdb, QDY, f"conv_bwd_fused db {tag}")
        for b0, b1 in lay.slices():
            r = _ref(data, ("dgrad_sparse", b0), lambda: lay.ref_dgrad(dyw_f, wm, b0, b1)[0]) * (x0f[b0:b1] > 0)
            expect_exact(dx[b0:b1], r, QBASE, f"conv_bwd_fused dx {tag} images {b0}..{b1}")
    pool.check(f"end {tag}")
    return forms


def make_data(lay, g, dev):
    """Operands of one layer (fp32 tensors holding values exact in bf16): the dense dy of the input gradients, the sparse one of the
    weight gradient (density dy_density of the pixel count), the depth head's weights of colvo_conv_head_fused; the float64
    references are cached in it (key "refs") by check_layer."""
    ysh = (lay.B, lay.Ho, lay.Wo, lay.Cout)
    return dict(x0=make_source(lay.stored(0), g, dev), x1=make_source(lay.stored(1), g, dev) if lay.C1 else None,
                w=make_weights(lay.Cout, lay.Cin, g, dev), bias=make_bias(lay.Cout, g, dev),
                dy_dense=make_dy(ysh, RHO_MAX, g, dev), dy_wgrad=make_dy(ysh, dy_density(lay.B * lay.Ho * lay.Wo), g, dev),
                head_w=make_weights(1, 16, g, dev))


def check_forms(lay, dtype, forms):
    """What every pass must have counted, from the dispatch trees (csrc/conv.hip, conv_rt.hip, wgrad.hip): one forward leaf, one
    input-gradient leaf per source, colvo_conv_dgrad_both's merged launch beside its leaf or two single-source leaves, one
    weight-gradient leaf per image slice and the slicing itself where a tensor reaches 1 GiB."""
    what = f"{lay.__dict__} {dtype}: {forms}"
    assert sum(leaves(forms["fwd"], FWD_LEAVES).values()) == 1, what
    for si in range(2 if lay.C1 else 1):
        for p in (f"dgrad{si}", f"dgrad{si}_masked_acc"):
            assert sum(leaves(forms[p], DGRAD_LEAVES).values()) == 1, (p, what)
    if lay.C1:
        fb = forms["dgrad_both"]
        n = sum(leaves(fb, DGRAD_LEAVES).values())
        assert (fb.get("dgrad_both", 0) == 1 and n == 1) or (fb.get("dgrad_both", 0) == 0 and n == 2), what
    ns = wgrad_slices(lay, dtype)
    for p in ("wgrad", "wgrad_acc", "wgrad_clean", "wgrad_det0", "wgrad_det1"):
        f = forms[p]
        assert sum(leaves(f, WGRAD_LEAVES).values()) == ns, (p, what)
        assert f.get("wgrad_sliced", 0) == (1 if ns > 1 else 0), (p, what)
