"""-m gpu: the depth and pose heads, and the glue around them, against float64 at the benchmark's own shapes (tests/head_exact.py):
exact where the arithmetic is exact (pre-activations, weight gradients, the HEAD form of k_bwd16, PoseNet's input), within a bound
derived from the kernel's fp32 operations where it is not (depth, d(pre), the heads' input gradients, the pose head).

Shapes: the DepthNet head at 16 / 64 / 128 frames of 256x320 and 64 frames of 512x640 (configs[1], [3], [4], [2] per GPU), the pose
head at 8 / 32 / 64 pairs of 256x320 and 32 pairs of 512x640, and ragged extents (H not a multiple of 4 or 8, W not a multiple of
16 or 64) for every op-level kernel.  Every form is reached through the tuning switch that selects it (restored afterwards); the
production values of those switches are asserted.  Each check prints a HEAD-ERR line: the largest error in fp32 ulps of the float64
value next to the derived bound, and their largest ratio."""
import contextlib
import gc
import zlib

import pytest
import torch

from tests import conv_exact as CX
from tests import head_exact as HX
from tests import guarded
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

_guarded = guarded.fixture(dev, allocates_nothing=("test_production_tuning_of_the_head_switches",))          # every test here allocates from tests/guarded.py's pool; the guards are checked at its end

DEPTH_SHAPES = [(16, 256, 320), (64, 256, 320), (128, 256, 320), (64, 512, 640)]
POSE_SHAPES = [(8, 256, 320), (32, 256, 320), (64, 256, 320), (32, 512, 640)]
RAGGED = [(2, 13, 37), (3, 33, 47)]
DTYPES = (torch.bfloat16, torch.float32)
PRODUCTION = {"head_fwd_lds": 1, "head_dgrad_generic": 0, "head_wgrad_rows": 1, "fwd16": 1, "bwd16": 1, "head_wgrad_wgs": 1024}


def _free():
    gc.collect()
    if guarded._ACTIVE:                      # check the guards of everything allocated so far and let go of what the test has dropped
        guarded.active_pool().check("before freeing", release=False)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def tuned(**kv):
    from coivo_amd import _lib
    old = {k: _lib.tune_get(k) for k in kv}
    try:
        for k, v in kv.items():
            _lib.tune_set(k, v)
        yield
    finally:
        torch.cuda.synchronize()
        for k, v in old.items():
            _lib.tune_set(k, v)


def _record(shape, form, stats):
    err, bnd, ratio = stats
    print(f"HEAD-ERR {shape} {form}: max err {err:.3g} ulp, bound {bnd:.3g} ulp, err/bound {ratio:.3g}")


def _exact(shape, form, got, ref, quantum):
    CX.expect_exact(got, ref, quantum, f"{form} {shape}")
    print(f"HEAD-ERR {shape} {form}: exact (bit for bit)")


def _gen(*key):
    return torch.Generator(device=dev()).manual_seed(zlib.crc32(repr(key).encode()))


def _label(B, H, W, dtype=None):
    return f"B={B} {H}x{W}" + (f" {str(dtype)[6:]}" if dtype is not None else "")


def _op_shapes():
    return [(s, dt) for s in DEPTH_SHAPES + RAGGED for dt in DTYPES]


def test_production_tuning_of_the_head_switches():
    from coivo_amd import _lib
    assert {k: _lib.tune_get(k) for k in PRODUCTION} == PRODUCTION


# --------------------------------------------------------------------------------------------------------------------------- #
# depth head forward                                                                                                           #
# --------------------------------------------------------------------------------------------------------------------------- #
def _p(t, label=""):
    """A guarded copy of an operand (tests/guarded.py): what a kernel loads past its end is NaN."""
    return guarded.active_pool().place(t, label)


def _head_inputs(B, H, W, C, g, d, y_max=HX.Y_FWD):
    y = HX.make_y((B, H, W, C), y_max, g, d)
    w = HX.make_head_w_saturating(C, g, d) if C == 16 else HX.make_head_w(C, g, d)
    b = HX.make_head_b(g, d)
    if C == 16:
        HX.saturate(y, w, g, 4)
    assert HX.bound_pre(y_max, C) <= CX.BOUND
    return y, w, b


@pytest.mark.parametrize("shape,dtype", _op_shapes())
def test_depth_head_forward(shape, dtype):
    from coivo_amd import ops
    _free()
    B, H, W = shape
    d, g = dev(), _gen("fwd", shape)
    forms = [("C16", 16, {})] if dtype == torch.float32 else [("C16 lds", 16, {"head_fwd_lds": 1}), ("C16 global", 16, {"head_fwd_lds": 0})]
    if shape in RAGGED:
        forms.append(("generic C=8", 8, {}))
    lab = _label(B, H, W, dtype)
    for form, C, sw in forms:
        y, w, b = _head_inputs(B, H, W, C, g, d)
        pre = HX.ref_pre(y, w, b)
        assert torch.equal(pre.float().double(), pre), "pre left the exact regime"
        if C == 16:
            assert bool((pre > HX.SAT_PRE).any()) and bool((pre < -HX.SAT_PRE).any()), "no saturated pixel"
        ref = HX.ref_depth(pre)
        depth = torch.full((B, 1, H, W), 7.0, device=d)
        with tuned(**sw):
            ops.depth_head_fwd(_p(y.to(dtype), "y"), _p(w, "w"), _p(b, "b"), depth)
        _record(lab, f"depth fwd {form}", HX.expect_within(depth[:, 0], ref, HX.depth_rel_bound(pre) * ref, f"depth fwd {form} {lab}"))
        del y, pre, ref, depth
        _free()


# --------------------------------------------------------------------------------------------------------------------------- #
# d(pre) and the head's input gradient                                                                                         #
# --------------------------------------------------------------------------------------------------------------------------- #
def _check_dgrad(lab, form, y, w, dpre, dx):
    ref, absum = HX.ref_head_dgrad(dpre, w, y.shape[-1])
    mask = (y > 0).double()
    _record(lab, form, HX.expect_within(dx, ref * mask, HX.dgrad_bound(absum, dx.dtype) * mask, f"{form} {lab}"))


@pytest.mark.parametrize("shape,dtype", _op_shapes())
def test_depth_head_dpre_and_input_gradient(shape, dtype):
    from coivo_amd import ops
    _free()
    B, H, W = shape
    d, g = dev(), _gen("bwd", shape)
    C = 16
    y, w, b = _head_inputs(B, H, W, C, g, d)
    pre = HX.ref_pre(y, w, b)
    yk, wk, bk = _p(y.to(dtype), "y"), _p(w, "w"), _p(b, "b")
    depth = torch.empty(B, 1, H, W, device=d)
    ops.depth_head_fwd(yk, wk, bk, depth)
    lab = _label(B, H, W, dtype)
    n = B * H * W
    dd = _p(HX.make_d_depth((B, 1, H, W), g, d), "d depth")
    scratch = torch.full((n,), 7.0, device=d)
    # plain form: k_depth_head_dpre, then the granule form (production), the generic form by its switch, and a misaligned view
    for form, sw, view in (("granule", {}, False), ("generic (switch)", {"head_dgrad_generic": 1}, False), ("generic (misaligned)", {}, True)):
        if view:
            buf = torch.empty(n * C + 1, device=d, dtype=dtype)
            dx = buf[1:].view(B, H, W, C)
        else:
            dx = torch.full_like(yk, 5.0)
        with tuned(**sw):
            ops.depth_head_bwd(yk, wk, depth, dd, scratch, dx, None, None)
        dpre = scratch.view(B, H, W).clone()
        _record(lab, "d(pre)", HX.expect_within(dpre, HX.ref_dpre(pre, dd[:, 0].double()), HX.dpre_bound(pre, dd[:, 0].double()),
                                                f"d(pre) {lab}"))
        _check_dgrad(lab, f"head dgrad {form}", y, w, dpre, dx)
        del dx
    # parts form (the training step's): device scales a power of two (exact) and general; g_raw on both halves
    Bh = B // 2
    if B % 2 == 0:
        gf, gsec, gr, gr2 = (_p(HX.make_d_depth((Bh, 1, H, W), g, d), "gradient part") for _ in range(4))
        for sa, sb in ((0.5, 0.125), (0.3, 0.7)):
            ta, tb = _p(torch.tensor([sa], device=d), "scale a"), _p(torch.tensor([sb], device=d), "scale b")
            sa32, sb32 = float(ta), float(tb)
            dx = torch.full_like(yk, 5.0)
            ops.depth_head_bwd_parts(yk, wk, depth, gf, gsec, gr, ta, tb, scratch, dx, gr2)
            g0 = torch.cat([gf, gsec])[:, 0]
            graw = torch.cat([gr, gr2])[:, 0]
            gdd, gerr = HX.parts_g(g0, graw, sa32, sb32)
            dpre = scratch.view(B, H, W).clone()
            _record(lab, f"d(pre) parts s={sa}*{sb}", HX.expect_within(dpre, HX.ref_dpre(pre, gdd), HX.dpre_bound(pre, gdd, gerr),
                                                                     f"d(pre) parts {lab}"))
            _check_dgrad(lab, f"head dgrad parts s={sa}*{sb}", y, w, dpre, dx)
            del dx
    if shape in RAGGED:            # the generic C != 16 kernels
        y2, w2, b2 = _head_inputs(B, H, W, 8, g, d)
        yk2, wk2 = _p(y2.to(dtype), "y C=8"), _p(w2, "w C=8")
        dep2 = torch.empty(B, 1, H, W, device=d)
        ops.depth_head_fwd(yk2, wk2, _p(b2, "b C=8"), dep2)
        pre2 = HX.ref_pre(y2, w2, b2)
        dx = torch.full_like(yk2, 5.0)
        ops.depth_head_bwd(yk2, wk2, dep2, dd, scratch, dx, None, None)
        dpre = scratch.view(B, H, W).clone()
        _record(lab, "d(pre) C=8", HX.expect_within(dpre, HX.ref_dpre(pre2, dd[:, 0].double()), HX.dpre_bound(pre2, dd[:, 0].double()),
                                                     f"d(pre) C=8 {lab}"))
        _check_dgrad(lab, "head dgrad generic C=8", y2, w2, dpre, dx)
    _free()


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("shape,dtype", [(s, dt) for s in [(2, 5, 7), (2, 13, 37)] for dt in DTYPES])
def test_depth_head_bwd_equals_bwd_parts(shape, dtype):
    """Both entry points make d(pre) and hand it to one input-gradient launch: with the incoming gradient as the two halves and no
    raw parts, scratch and dx are the same bits -- granule form, generic form by its switch, and C = 8."""
    from coivo_amd import ops
    B, H, W = shape
    d, g = dev(), _gen("bwd = parts", shape)
    dd = _p(HX.make_d_depth((B, 1, H, W), g, d), "d depth")
    lo, hi = _p(dd[:B // 2].contiguous(), "first half"), _p(dd[B // 2:].contiguous(), "second half")
    for form, C, sw in (("granule", 16, {"head_dgrad_generic": 0}), ("generic (switch)", 16, {"head_dgrad_generic": 1}), ("C=8", 8, {})):
        y, w, b = _head_inputs(B, H, W, C, g, d)
        yk, w, b = _p(y.to(dtype), "y"), _p(w, "w"), _p(b, "b")
        depth = torch.empty(B, 1, H, W, device=d)
        ops.depth_head_fwd(yk, w, b, depth)
        s1, s2 = torch.full((B * H * W,), 7.0, device=d), torch.full((B * H * W,), 9.0, device=d)
        dx1, dx2 = torch.full_like(yk, 5.0), torch.full_like(yk, 3.0)
        with tuned(**sw):
            ops.depth_head_bwd(yk, w, depth, dd, s1, dx1, None, None)
            ops.depth_head_bwd_parts(yk, w, depth, lo, hi, None, None, None, s2, dx2)
        lab = f"{form} {_label(B, H, W, dtype)}"
        assert _same_bits(s1, s2), f"d(pre) of depth_head_bwd and depth_head_bwd_parts differ: {lab}"
        assert _same_bits(dx1, dx2), f"dx of depth_head_bwd and depth_head_bwd_parts differ: {lab}"


# --------------------------------------------------------------------------------------------------------------------------- #
# the head's weight gradient                                                                                                   #
# --------------------------------------------------------------------------------------------------------------------------- #
def _wgrad_operands(B, H, W, C, g, d):
    y = HX.make_y((B, H, W, C), CX.X_MAX, g, d)
    dpre = CX.make_dy((B, H, W), CX.dy_density(B * H * W), g, d)
    worst = float(y.abs().max()) / HX.QY * float(dpre.abs().sum(dtype=torch.float64)) / CX.QDY
    assert worst <= CX.BOUND, f"head weight gradient: {worst:.0f} quanta > 2^22"
    assert worst <= CX.bound_wgrad(B * H * W)
    return y, _p(dpre, "d(pre)")


def _wgrad_atomic(y, dpre, dw, db):
    """colvo_depth_head_wgrad without scratch: the fp32-atomics form (ops.depth_head_wgrad takes the table form)."""
    from coivo_amd import _lib, ops
    B, H, W, C = y.shape
    ops._issue(_lib.CMD_DEPTH_HEAD_WGRAD, None, (y, dpre, dw, db, None), (ops.dt_code(y.dtype), B, H, W, C, 0))


def _zeros(C, d):
    return torch.zeros(1, 9, C, device=d), torch.zeros(1, device=d)


@pytest.mark.parametrize("shape,dtype", _op_shapes())
def test_depth_head_weight_gradient_exact(shape, dtype):
    from coivo_amd import ops
    _free()
    B, H, W = shape
    d, g = dev(), _gen("wgrad", shape)
    lab = _label(B, H, W, dtype)
    y, dpre = _wgrad_operands(B, H, W, 16, g, d)
    rdw, rdb = HX.ref_head_wgrad(y, dpre)
    q = HX.QY * CX.QDY
    yk = _p(y.to(dtype), "y")
    for rows in (1, 3):
        with tuned(head_wgrad_rows=rows):
            dw, db = _zeros(16, d)
            _wgrad_atomic(yk, dpre, dw, db)
            _exact(lab, f"head wgrad atomics rows={rows}", dw, rdw, q)
            _exact(lab, f"head bgrad atomics rows={rows}", db, rdb, CX.QDY)
            dets = []
            for i in range(2):
                dw, db = _zeros(16, d)
                ops.depth_head_wgrad(yk, dpre, dw, db, deterministic=True)
                _exact(lab, f"head wgrad table rows={rows} call {i}", dw, rdw, q)
                _exact(lab, f"head bgrad table rows={rows} call {i}", db, rdb, CX.QDY)
                dets.append((dw, db))
            assert torch.equal(dets[0][0], dets[1][0]) and torch.equal(dets[0][1], dets[1][1])
    if dtype == torch.bfloat16:
        assert ops.depth_head_wgrad_mfma_ok(B, H, W)
        for i in range(2):
            dw, db = _zeros(16, d)
            dw.fill_(0.25)           # (the reduction adds)
            ops.depth_head_wgrad_mfma(yk, dpre, dw, db)
            _exact(lab, f"head wgrad MFMA call {i}", dw, rdw + 0.25, q)
            _exact(lab, f"head bgrad MFMA call {i}", db, rdb, CX.QDY)
    if shape in RAGGED:
        y2, dp2 = _wgrad_operands(B, H, W, 8, g, d)
        rdw2, rdb2 = HX.ref_head_wgrad(y2, dp2)
        dw, db = _zeros(8, d)
        ops.depth_head_wgrad(_p(y2.to(dtype), "y C=8"), dp2, dw, db)
        _exact(lab, "head wgrad generic C=8", dw, rdw2, q)
        _exact(lab, "head bgrad generic C=8", db, rdb2, CX.QDY)
    _free()


def test_depth_head_weight_gradient_above_2_25_pixels():
    """128 frames of 512x640 (2^25 pixels or more): the MFMA form refuses the shape (32-bit offsets); the table form DepthNet falls
    back to is exact there."""
    from coivo_amd import ops
    _free()
    B, H, W = 128, 512, 640
    assert B * H * W >= 2 ** 25 and not ops.depth_head_wgrad_mfma_ok(B, H, W)
    d, g = dev(), _gen("wgrad-big")
    y, dpre = _wgrad_operands(B, H, W, 16, g, d)
    yk = y.bfloat16()
    del y
    rdw, rdb = HX.ref_head_wgrad(yk, dpre)
    dw, db = _zeros(16, d)
    ops.depth_head_wgrad(yk, dpre, dw, db, deterministic=True)
    lab = _label(B, H, W, torch.bfloat16)
    _exact(lab, "head wgrad table (fallback of the MFMA form)", dw, rdw, HX.QY * CX.QDY)
    _exact(lab, "head bgrad table (fallback of the MFMA form)", db, rdb, CX.QDY)
    with pytest.raises(RuntimeError):
        ops.depth_head_wgrad_mfma(yk, dpre, dw, db)
    _free()


# --------------------------------------------------------------------------------------------------------------------------- #
# k_bwd16, HEAD form                                                                                                           #
# --------------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", DEPTH_SHAPES + RAGGED)
def test_fused_backward_head_form_exact(shape):
    from coivo_amd import ops
    _free()
    B, H, W = shape
    d, g = dev(), _gen("bwd16", shape)
    lab = _label(B, H, W)
    lay = CX.Layer(B, H, W, 16, 0, False, False, 16, 1)
    desc = ops.conv_desc(torch.bfloat16, B, H, W, 16, 16)
    assert ops.conv_bwd_fused_ok(desc)
    npix = B * H * W
    assert CX.bound_wgrad(npix) <= CX.BOUND and HX.bound_head_g_wgrad(npix) <= CX.BOUND and HX.head_g_bound() <= 255
    x = CX.make_source(lay.stored(0), g, d)
    wm = CX.make_weights(16, 16, g, d)
    y = HX.make_y((B, H, W, 16), CX.X_MAX, g, d)
    dpre = CX.make_dy((B, H, W), HX.head_g_density(npix), g, d)
    wh = HX.make_head_w(16, g, d)
    # g = (y > 0) * (d(pre) (*) head weights): exact in bf16 by head_g_bound
    gref = HX.ref_head_dgrad(dpre, wh, 16)[0] * (y > 0)
    assert torch.equal(gref.float().bfloat16().double(), gref)
    measured = float(x.abs().max()) / CX.QX * float(gref.abs().sum(dim=(0, 1, 2)).max()) / (CX.QDY * HX.QH_OP)
    assert measured <= CX.BOUND, measured
    rdw, rdb = lay.ref_wgrad(x, None, gref)
    hdw, hdb = HX.ref_head_wgrad(y, dpre)
    w_fwd = torch.empty(16, 9, 16, device=d, dtype=torch.bfloat16)
    w_bwd = torch.empty(16, 9, 16, device=d, dtype=torch.bfloat16)
    ops.pack_weights(wm, torch.bfloat16, w_fwd, w_bwd)
    xb, yb = _p(x.bfloat16(), "x"), _p(y.bfloat16(), "y")
    dpre_k, wh_k = _p(dpre, "d(pre)"), _p(wh, "head weights")
    qg = CX.QDY * HX.QH_OP
    for form in ("HEAD", "HEAD + head partials"):
        dx = torch.full_like(xb, 3.0)
        dw, db = torch.zeros(16, 9, 16, device=d), torch.zeros(16, device=d)
        if form == "HEAD":
            ops.conv_bwd_fused(desc, yb, w_bwd, xb, True, dx, dw, db, dpre_k, wh_k)
        else:
            rows = ops.conv_bwd_fused_head_rows(desc)
            hp = torch.full((rows * 145,), float("nan"), device=d)
            ops.conv_bwd_fused(desc, yb, w_bwd, xb, True, dx, dw, db, dpre_k, wh_k, hp)
            hw_, hb_ = _zeros(16, d)
            ops.depth_head_wgrad_reduce(hp, rows, hw_, hb_)
            _exact(lab, "bwd16 head partials: head wgrad", hw_, hdw, HX.QY * CX.QDY)
            _exact(lab, "bwd16 head partials: head bgrad", hb_, hdb, CX.QDY)
        _exact(lab, f"bwd16 {form}: layer dw", dw, rdw, CX.QX * qg)
        _exact(lab, f"bwd16 {form}: layer db", db, rdb, qg)
        for b0, b1 in lay.slices():
            r = lay.ref_dgrad(gref, wm, b0, b1)[0] * (x[b0:b1] > 0)
            CX.expect_exact(dx[b0:b1], r, qg * CX.QW, f"bwd16 {form}: dx {lab} images {b0}..{b1}")
        print(f"HEAD-ERR {lab} bwd16 {form}: dx exact (bit for bit)")
        del dx
    _free()


# --------------------------------------------------------------------------------------------------------------------------- #
# the fused layer + head forward, PoseNet's input                                                                              #
# --------------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", DEPTH_SHAPES + RAGGED[:1])
def test_fused_forward_depth_and_pose_input(shape):
    from coivo_amd import ops
    _free()
    B, H, W = shape
    d, g = dev(), _gen("fwd16", shape)
    lab = _label(B, H, W)
    lay = CX.Layer(B, H, W, 16, 0, False, False, 16, 1)
    desc = ops.conv_desc(torch.bfloat16, B, H, W, 16, 16)
    assert ops.conv_head_fused_ok(desc)
    x, wm, bias = CX.make_source(lay.stored(0), g, d), CX.make_weights(16, 16, g, d), CX.make_bias(16, g, d)
    x[:, H // 3:H // 3 + 6, W // 4:W // 4 + 6] = CX.X_MAX * CX.QX            # a bright patch: large layer outputs
    wh, hb = HX.make_head_w(16, g, d, HX.QH_FUSED), HX.make_head_b(g, d, HX.QH_FUSED)
    w_fwd = torch.empty(16, 9, 16, device=d, dtype=torch.bfloat16)
    ops.pack_weights(wm, torch.bfloat16, w_fwd, torch.empty_like(w_fwd))
    yref = torch.cat([lay.ref_fwd(x, None, wm, bias, b0, b1) for b0, b1 in lay.slices()])
    ybf = yref.float().bfloat16().float()
    pre = HX.ref_pre(ybf, wh, hb)
    assert float(ybf.max()) <= HX.Y_FWD * HX.QY and torch.equal(pre.float().double(), pre)
    ref = HX.ref_depth(pre)
    bound = HX.depth_rel_bound(pre) * ref
    print(f"HEAD-ERR {lab} fused fwd: |pre| max {float(pre.abs().max()):.3g}, saturated pixels {int((pre.abs() > HX.SAT_PRE).sum())}")
    xb, bias_k, wh_k, hb_k = _p(x.bfloat16(), "x"), _p(bias, "bias"), _p(wh, "head weights"), _p(hb, "head bias")
    depths = []
    for with_pose in ((True, False) if B % 2 == 0 else (False,)):
        y = torch.full((B, H, W, 16), 9.0, device=d, dtype=torch.bfloat16)
        depth = torch.full((B, 1, H, W), 7.0, device=d)
        pose_in = None
        if with_pose:
            frames = _p(torch.rand(B, 3, H, W, generator=g, device=d), "frames")
            stem = torch.full((B, H, W, 8), 3.0, device=d, dtype=torch.bfloat16)
            pose_in = torch.full((B // 2, H, W, 8), 3.0, device=d, dtype=torch.bfloat16)
            ops.pack_stem_pose(frames, stem, pose_in)
            want = torch.cat([frames.permute(0, 2, 3, 1), torch.zeros(B, H, W, 5, device=d)], 3).bfloat16()
            assert torch.equal(stem.view(torch.int16), want.view(torch.int16)), "pack_stem_pose: stem"
        ops.conv_head_fused(desc, xb, w_fwd, bias_k, wh_k, hb_k, y, depth, pose_in)
        form = "fused fwd + pose_in" if with_pose else "fused fwd"
        for b0, b1 in lay.slices():
            CX.expect_exact(y[b0:b1], yref[b0:b1], CX.QB, f"{form} y {lab}")
        _record(lab, f"{form} depth", HX.expect_within(depth[:, 0], ref, bound, f"{form} depth {lab}"))
        if with_pose:
            HX.check_pose_in(pose_in, frames, depth)
            print(f"HEAD-ERR {lab} pose_in ({B // 2} pairs): exact (bit for bit)")
        depths.append(depth)
        del y
    assert all(torch.equal(depths[0], t) for t in depths)
    _free()


# --------------------------------------------------------------------------------------------------------------------------- #
# pose head                                                                                                                    #
# --------------------------------------------------------------------------------------------------------------------------- #
def _pose_hw(H, W):
    from coivo_amd import nn as hnn
    for _ in hnn.POSE_CH:
        H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return H, W


@pytest.mark.parametrize("shape,dtype", [(s, dt) for s in POSE_SHAPES + [(5, 3, 7)] for dt in DTYPES])
def test_pose_head(shape, dtype):
    from coivo_amd import ops
    B, H0, W0 = shape
    H, W = _pose_hw(H0, W0) if shape in POSE_SHAPES else (H0, W0)
    C = 256
    d, g = dev(), _gen("pose", shape)
    lab = _label(B, H, W, dtype)
    x = CX.make_source((B, H, W, C), g, d)
    w = CX._ints(-CX.W_MAX, CX.W_MAX, (8, 1, C), g, d) * CX.QW
    b = CX.make_bias(8, g, d)
    pool = guarded.active_pool()
    xk, w, b = pool.place(x.to(dtype), "x"), pool.place(w, "w"), pool.place(b, "b")         # a load past the end of x or w reads NaN
    out = torch.full((8 * B,), 7.0, device=d)
    ops.pose_head_fwd(xk, w, b, out)
    got = torch.cat([out[:6 * B].view(B, 6), out[6 * B:7 * B].view(B, 1), out[7 * B:].view(B, 1)], 1)
    ref, bnd = HX.pose_ref(x, w, b)
    _record(lab, f"pose fwd (HW={H * W})", HX.expect_within(got, ref, bnd, f"pose fwd {lab}"))
    dout = CX._ints(-4, 4, (B, 8), g, d) * 2.0 ** -4
    results = {}
    for sa, sb in ((None, None), (0.5, 0.125), (0.3, 0.7)):
        ta = None if sa is None else torch.tensor([sa], device=d)
        tb = None if sb is None else torch.tensor([sb], device=d)
        sa32, sb32 = (1.0, 1.0) if sa is None else (float(ta), float(tb))
        r = HX.pose_bwd_refs(x, w, dout, sa32, sb32)
        parts = [pool.place(dout[:, lo:hi].contiguous(), f"d_out[:, {lo}:{hi}]") for lo, hi in ((0, 6), (6, 7), (7, 8))]
        # the atomic form, then the deterministic one in both of its forms: the parallel one (the default) twice, then the serial walk
        # (tuning pose_head_det_parallel = 0), which must give the parallel form's bits
        for det, pars in ((False, (None,)), (True, (1, 1, 0))):
            outs = []
            for par in pars:
                dx = torch.full_like(xk, 5.0)
                dw, db = torch.zeros(8, 1, C, device=d), torch.zeros(8, device=d)
                with contextlib.nullcontext() if par is None else tuned(pose_head_det_parallel=par):
                    ops.pose_head_bwd(xk, w, parts[0], parts[1], parts[2], dx, dw, db, ta, tb, deterministic=det)
                    torch.cuda.synchronize()
                outs.append((dx, dw, db))
            if det:
                assert all(torch.equal(a, c) for a, c in zip(outs[0], outs[1])), "deterministic pose head: not repeatable"
                assert all(_same_bits(a, c) for a, c in zip(outs[0], outs[2])), "pose head: the serial walk and the parallel form differ"
            dx, dw, db = outs[0]
            dxb, dwb, dbb = HX.pose_bwd_bounds(r, B, dtype, det)
            form = f"pose bwd {'det' if det else 'atomics'} s={sa}*{sb}"
            _record(lab, f"{form} dx", HX.expect_within(dx, r["dx"], dxb, f"{form} dx {lab}"))
            _record(lab, f"{form} dw", HX.expect_within(dw.view(8, C), r["dw"], dwb, f"{form} dw {lab}"))
            _record(lab, f"{form} db", HX.expect_within(db, r["db"], dbb, f"{form} db {lab}"))
            results[(sa, det)] = outs[0]
    # power-of-two device scales: exactly gs times the unscaled result (deterministic form, bit for bit)
    gs = 0.5 * 0.125
    for a, c in zip(results[(0.5, True)], results[(None, True)]):
        assert torch.equal(a.float(), (c.float() * gs)), "pose head: a power-of-two scale is not exact"


@pytest.mark.parametrize("C,dtype", [(C, dt) for C in (8, 264) for dt in DTYPES])
def test_pose_head_backward_forms_share_dx(C, dtype):
    """The atomic and the ordered form run one per-channel function: dx bit-equal; dw, db of the ordered form repeatable.  C = 264
    is the smallest multiple of 8 past one 256-thread pass: a second workgroup (ordered), a second trip of the channel loop (atomic)."""
    from coivo_amd import ops
    B, H, W = 3, 1, 5
    d, g = dev(), _gen("pose forms", C)
    xk = CX.make_source((B, H, W, C), g, d).to(dtype)
    w = CX._ints(-CX.W_MAX, CX.W_MAX, (8, 1, C), g, d) * CX.QW
    dout = CX._ints(-4, 4, (B, 8), g, d) * 2.0 ** -4
    outs = []
    for det in (False, True, True):
        dx = torch.full_like(xk, 5.0)
        dw, db = torch.zeros(8, 1, C, device=d), torch.zeros(8, device=d)
        ops.pose_head_bwd(xk, w, dout[:, :6].contiguous(), dout[:, 6:7].contiguous(), dout[:, 7:8].contiguous(), dx, dw, db, None, None,
                          deterministic=det)
        outs.append((dx, dw, db))
    assert _same_bits(outs[0][0], outs[1][0]), "pose head: dx of the atomic and of the ordered form differ"
    assert all(_same_bits(a, c) for a, c in zip(outs[1], outs[2])), "ordered pose head: not repeatable"


# --------------------------------------------------------------------------------------------------------------------------- #
# DepthNet at 2^25 pixels or more                                                                                              #
# --------------------------------------------------------------------------------------------------------------------------- #
def test_depthnet_bf16_backward_above_2_25_pixels():
    """bf16 DepthNet forward + backward at 128 frames of 512x640: the head's weight gradient takes the table form where the MFMA form
    refuses the shape; the pass ends with finite, non-zero head gradients."""
    from coivo_amd import nn as hnn
    _free()
    B, H, W = 128, 512, 640
    d = dev()
    dn = hnn.DepthNet(compute_dtype=torch.bfloat16, device=d)
    g = torch.Generator(device=d).manual_seed(11)
    with torch.no_grad():                                   # (a new network's weights are zero: so would be every activation)
        for name, p in dn.named_parameters():
            if name.endswith("weight"):
                p.copy_(torch.randn(p.shape, generator=g, device=d) * (2.0 / (p.shape[1] * 9)) ** 0.5)
    img = torch.rand(B, 3, H, W, generator=g, device=d)
    depth = dn.forward(img)
    assert torch.isfinite(depth).all()
    dd = torch.randn(B, 1, H, W, generator=g, device=d)
    (depth * dd).sum().backward()
    dn.join_side()
    torch.cuda.synchronize()
    hg, hb = dn.head.g_master, dn.head.g_bias
    assert torch.isfinite(hg).all() and torch.isfinite(hb).all()
    assert float(hg.abs().max()) > 0 and float(hb.abs().max()) > 0
    assert torch.isfinite(dn.flat_grad).all()
    del dn, depth, img, dd
    _free()
