"""-m gpu: the deterministic form of the fused full-resolution backward (colvo_conv_bwd_fused_det, csrc/bwd16.hip): k_bwd16 with the
slab way-out -- every workgroup stores its weight / bias sums into its own row of a scratch -- and the fixed-tree reduction that adds
the rows to dw / db behind it; and the deterministic training step that runs it.

Kernel level, bf16, mode 0 (dy given) and the HEAD form: bit for bit the float64 reference on exact data (tests/conv_exact.py,
tests/head_exact.py) at a grid of 4 rows with 8 tiles per workgroup, a short last workgroup and a workgroup that crosses the image
boundary, and at the production grid of one tile per workgroup; adds to dw / db; repeatable on random data, the atomic form's dx bit
for bit and its dw to fp32 summation order; a scratch full of NaN changes nothing.  Step level (2 pairs of 64x96): the kernel is in
the recorded backward pass, three optimizer steps repeat bit for bit, two passes share the slab scratch, and the gradients agree
with the three-kernel deterministic path the step took before within the bound tests/test_nets_gpu.py uses for this pair of forms."""
import contextlib
import functools
import zlib

import pytest
import torch

from coivo_amd import synth
from tests import conv_exact as CX
from tests import head_exact as HX
from tests import guarded
from tests.gpu_util import bf16_rounded_state, dev, to_dev

pytestmark = pytest.mark.gpu

_guarded = guarded.fixture(dev)          # every test here allocates from tests/guarded.py's pool; the guards are checked at its end

ROW = 16 * 9 * 16 + 16                    # floats of one workgroup's row: the weight slab and the bias slab
# (shape, bwd16_wgs, rows): 15 tiles per image of 33x47 -> 30 tiles over 4 workgroups = 8, 8, 8, 6; 64x96 at the production tuning
CASES = [((2, 33, 47), 4, 4), ((2, 64, 96), None, 96)]
MODES = ["dy", "HEAD"]


@contextlib.contextmanager
def _wgs(n):
    from coivo_amd import _lib
    old = _lib.tune_get("bwd16_wgs")
    try:
        if n is not None:
            _lib.tune_set("bwd16_wgs", n)
        yield
    finally:
        torch.cuda.synchronize()
        _lib.tune_set("bwd16_wgs", old)


def _gen(*key):
    return torch.Generator(device=dev()).manual_seed(zlib.crc32(repr(key).encode()))


def _packed(wm):
    from coivo_amd import ops
    w_fwd = torch.empty(16, 9, 16, device=wm.device, dtype=torch.bfloat16)
    w_bwd = torch.empty(16, 9, 16, device=wm.device, dtype=torch.bfloat16)
    ops.pack_weights(wm, torch.bfloat16, w_fwd, w_bwd)
    return w_bwd


@functools.lru_cache(maxsize=None)
def _exact_case(shape, mode):
    """Operands in the exact regime and the float64 references of one (shape, mode), made once: dict(args = what conv_bwd_fused takes
    behind the descriptor, rdw, rdb, rdx, qw, qb, qx)."""
    B, H, W = shape
    d, g = dev(), _gen("bwd16_det", shape, mode)
    lay = CX.Layer(B, H, W, 16, 0, False, False, 16, 1)
    npix = B * H * W
    x = CX.make_source(lay.stored(0), g, d)
    wm = CX.make_weights(16, 16, g, d)
    w_bwd = _packed(wm)
    if mode == "dy":
        assert CX.bound_wgrad(npix) <= CX.BOUND
        dy = CX.make_dy((B, H, W, 16), CX.dy_density(npix), g, d)
        CX.check_wgrad_bound([x], dy, f"{shape}")
        gref, qg, qx = dy.double(), CX.QDY, CX.QBASE
        args = (dy.bfloat16(), w_bwd, x.bfloat16(), True)
        head = ()
    else:
        assert CX.bound_wgrad(npix) <= CX.BOUND and HX.bound_head_g_wgrad(npix) <= CX.BOUND and HX.head_g_bound() <= 255
        y = HX.make_y((B, H, W, 16), CX.X_MAX, g, d)
        dpre = CX.make_dy((B, H, W), HX.head_g_density(npix), g, d)
        wh = HX.make_head_w(16, g, d)
        gref = HX.ref_head_dgrad(dpre, wh, 16)[0] * (y > 0)               # exact in bf16 by head_g_bound
        assert torch.equal(gref.float().bfloat16().double(), gref)
        qg = CX.QDY * HX.QH_OP
        measured = float(x.abs().max()) / CX.QX * float(gref.abs().sum(dim=(0, 1, 2)).max()) / qg
        assert measured <= CX.BOUND, measured
        qx = qg * CX.QW
        args = (y.bfloat16(), w_bwd, x.bfloat16(), True)
        head = (dpre, wh)
    rdw, rdb = lay.ref_wgrad(x, None, gref)
    rdx = lay.ref_dgrad(gref, wm, 0, B)[0] * (x > 0)
    return dict(args=args, head=head, rdw=rdw, rdb=rdb, rdx=rdx, qw=CX.QX * qg, qb=qg, qx=qx)


def _desc(shape):
    from coivo_amd import ops
    desc = ops.conv_desc(torch.bfloat16, *shape, 16, 16)
    assert ops.conv_bwd_fused_ok(desc)
    return desc


def _scratch(desc, mode, rows, fill=None):
    import ctypes
    from coivo_amd import _lib, ops
    pool = guarded.active_pool()
    served = len(pool.served)
    scr = ops.conv_bwd_fused_scratch(desc, 0 if mode == "dy" else 1, dev())
    assert scr.numel() == rows * ROW, (scr.numel(), rows)
    # the rows come from the pool, of the size the query gives and not a byte more: a row written past the last one lands in a guard
    nbytes = _lib.load().colvo_conv_bwd_fused_scratch_bytes(ctypes.byref(desc), 0 if mode == "dy" else 1)
    guarded.assert_served(pool, served, nbytes, f"conv_bwd_fused_scratch mode {mode}")
    if fill is not None:
        scr.fill_(fill)
    return scr


def _call(desc, c, dx, dw, db, scratch):
    from coivo_amd import ops
    pool = guarded.active_pool()             # the operands as guarded copies: a load past the end of dy, x, d(pre) or the weights reads NaN
    ops.conv_bwd_fused(desc, *pool.place_tree(c["args"]), dx, dw, db, *pool.place_tree(c["head"]), scratch=scratch)


def _zeros():
    return torch.zeros(16, 9, 16, device=dev()), torch.zeros(16, device=dev())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,wgs,rows", CASES)
def test_det_form_is_exact(shape, wgs, rows, mode):
    """dw, db and dx of the slab form against float64 on exact data, bit for bit."""
    from coivo_amd import _lib
    c, desc = _exact_case(shape, mode), _desc(shape)
    with _wgs(wgs):
        scr = _scratch(desc, mode, rows)
        dx = torch.full_like(c["args"][2], 3.0)
        dw, db = _zeros()
        before = _lib.form_counts()
        _call(desc, c, dx, dw, db, scr)
        torch.cuda.synchronize()
        assert CX.forms_diff(before, _lib.form_counts()) == {"bwd16": 1}
    CX.expect_exact(dw, c["rdw"], c["qw"], f"bwd16 det {mode} dw {shape}")
    CX.expect_exact(db, c["rdb"], c["qb"], f"bwd16 det {mode} db {shape}")
    CX.expect_exact(dx, c["rdx"], c["qx"], f"bwd16 det {mode} dx {shape}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,wgs,rows", CASES)
def test_det_form_adds_to_dw_and_db(shape, wgs, rows, mode):
    """Two calls into the same dw / db give exactly twice the single call; a call into a pre-filled dw / db keeps the addend."""
    c, desc = _exact_case(shape, mode), _desc(shape)
    g = _gen("addend", shape, mode)
    base_w = CX._ints(-64, 64, (16, 9, 16), g, dev()) * c["qw"]
    base_b = CX._ints(-64, 64, (16,), g, dev()) * c["qb"]
    with _wgs(wgs):
        scr = _scratch(desc, mode, rows)
        dx = torch.empty_like(c["args"][2])
        dw, db = _zeros()
        _call(desc, c, dx, dw, db, scr)
        _call(desc, c, dx, dw, db, scr)
        fw, fb = base_w.clone(), base_b.clone()
        _call(desc, c, dx, fw, fb, scr)
        torch.cuda.synchronize()
    CX.expect_exact(dw, 2 * c["rdw"], c["qw"], f"bwd16 det {mode} dw, two calls {shape}")
    CX.expect_exact(db, 2 * c["rdb"], c["qb"], f"bwd16 det {mode} db, two calls {shape}")
    CX.expect_exact(fw, base_w.double() + c["rdw"], c["qw"], f"bwd16 det {mode} dw, pre-filled {shape}")
    CX.expect_exact(fb, base_b.double() + c["rdb"], c["qb"], f"bwd16 det {mode} db, pre-filled {shape}")


@functools.lru_cache(maxsize=None)
def _random_case(shape, mode):
    B, H, W = shape
    gen = torch.Generator().manual_seed(zlib.crc32(repr(("random", shape, mode)).encode()))
    dt = torch.bfloat16
    x = torch.randn(B, H, W, 16, generator=gen).relu().to(dev()).to(dt)
    w_bwd = (torch.randn(16, 9, 16, generator=gen) * 0.1).to(dev()).to(dt)
    if mode == "dy":
        dy = torch.randn(B, H, W, 16, generator=gen).to(dev()).to(dt)
        return dict(args=(dy, w_bwd, x, True), head=())
    y = torch.randn(B, H, W, 16, generator=gen).relu().to(dev()).to(dt)
    dpre = torch.randn(B, H, W, generator=gen).to(dev())
    wh = (torch.randn(1, 9, 16, generator=gen) * 0.2).to(dev())
    return dict(args=(y, w_bwd, x, True), head=(dpre, wh))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,wgs,rows", CASES)
def test_det_form_is_repeatable_and_agrees_with_the_atomic_form(shape, wgs, rows, mode):
    """Random bf16 data: three calls, identical bits; a scratch full of NaN beforehand changes nothing (every row is written in full
    before it is read); dx is the atomic form's bit for bit (the way-out does not touch it) and dw its dw within 1e-5 of the largest
    element (fp32 summation order only).  db: both forms sum the same bf16 terms in fp32, each along chains of fewer than 256 adds, so
    each is within 256 * 2^-24 * sum|terms| of the exact sum -- the two differ by at most twice that."""
    c, desc = _random_case(shape, mode), _desc(shape)
    with _wgs(wgs):
        outs = []
        for fill in (None, 0.0, float("nan")):
            scr = _scratch(desc, mode, rows, fill)
            dx = torch.full_like(c["args"][2], 3.0)
            dw, db = _zeros()
            _call(desc, c, dx, dw, db, scr)
            outs.append((dx, dw, db))
        ax = torch.full_like(c["args"][2], 5.0)
        aw, ab = _zeros()
        _call(desc, c, ax, aw, ab, None)
        torch.cuda.synchronize()
    for dx, dw, db in outs[1:]:
        assert torch.equal(dx, outs[0][0]) and torch.equal(dw, outs[0][1]) and torch.equal(db, outs[0][2])
    dx, dw, db = outs[0]
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
    assert torch.equal(dx, ax)
    ew, sw = (dw - aw).abs().max().item(), aw.abs().max().item()
    print(f"bwd16 det {mode} {shape}: max|dw - atomic dw| = {ew:.3e} = {ew / sw:.3e} of max|dw|")
    assert ew <= 1e-5 * sw
    # sum over the pixels of |g[., co]|, at most: of |dy| itself (mode 0), or -- the HEAD form's g is not materialised -- through the
    # atomic form's db, which sums the same g: bound it by the pixel count times the largest |g| a pixel can take
    if mode == "dy":
        terms = c["args"][0].float().abs().sum(dim=(0, 1, 2)).max().item()
    else:
        dpre, wh = c["head"]
        terms = dpre.numel() * dpre.abs().max().item() * wh.abs().sum(dim=1).max().item() * (1 + 2.0 ** -8)
    eb = (db - ab).abs().max().item()
    print(f"bwd16 det {mode} {shape}: max|db - atomic db| = {eb:.3e}, bound {2 * 256 * 2.0 ** -24 * terms:.3e}")
    assert eb <= 2 * 256 * 2.0 ** -24 * terms


@pytest.mark.parametrize("mode", MODES)
def test_rows_left_to_a_later_reduction_give_the_det_form_bit_for_bit(mode):
    """The _det form without dw + wgrad_reduce_group: db untouched by the first call, then the _det form's bits."""
    from coivo_amd import ops
    shape = (2, 64, 96)
    c, desc = _random_case(shape, mode), _desc(shape)
    scr = _scratch(desc, mode, 96, float("nan"))
    dx0, (dw0, db0) = torch.empty_like(c["args"][2]), _zeros()
    _call(desc, c, dx0, dw0, db0, scr)
    dx1, (dw1, db1) = torch.empty_like(c["args"][2]), _zeros()
    scr.fill_(float("nan"))
    ops.conv_bwd_fused(desc, *c["args"], dx1, None, db1, *c["head"], scratch=scr)
    torch.cuda.synchronize()
    assert float(db1.abs().max()) == 0.0 and scr.numel() == 96 * ROW
    ops.wgrad_reduce_group([(scr, dw1, db1, 96, 16, 16)])
    torch.cuda.synchronize()
    assert torch.equal(dx0, dx1) and torch.equal(dw0, dw1) and torch.equal(db0, db1)


def test_det_form_refuses_a_short_scratch_and_head_partials():
    from coivo_amd import ops
    shape = (2, 64, 96)
    c, desc = _random_case(shape, "HEAD"), _desc(shape)
    dx = torch.empty_like(c["args"][2])
    dw, db = _zeros()
    short = torch.empty(96 * ROW - 4, device=dev())
    with pytest.raises(RuntimeError, match="colvo_conv_bwd_fused_det: scratch"):
        _call(desc, c, dx, dw, db, short)
    hp = torch.empty(ops.conv_bwd_fused_head_rows(desc) * 145, device=dev())
    with pytest.raises(RuntimeError, match="colvo_conv_bwd_fused_det: the head's own weight gradient"):
        ops.conv_bwd_fused(desc, *c["args"], dx, dw, db, *c["head"], hp, scratch=_scratch(desc, "HEAD", 96))
    torch.cuda.synchronize()
    assert float(dw.abs().max()) == 0.0 and float(db.abs().max()) == 0.0       # refused before any launch


# --------------------------------------------------------------------------------------------------------------------------- #
# the deterministic step                                                                                                       #
# --------------------------------------------------------------------------------------------------------------------------- #
B, H, W, SEED = 2, 64, 96, 57


def _nets():
    from coivo_amd import nn as hnn
    from oracle import colvo_spec as S
    dn_o, pn_o = S.make_models(SEED)
    dn, pn = hnn.DepthNet(compute_dtype=torch.bfloat16), hnn.PoseNet(compute_dtype=torch.bfloat16)
    dn.load_state_dict(bf16_rounded_state(dn_o))
    pn.load_state_dict(bf16_rounded_state(pn_o))
    dn.deterministic = pn.deterministic = True
    return dn, pn


def _batch(seed=SEED):
    return to_dev(synth.make_batch(B, H, W, seed=seed))


def _pass(dn, pn, b):
    from coivo_amd import nn as hnn
    hnn.dcdp_forward(dn, pn, b["tgt"], b["ref"], b["K"])[0].backward()


def _grads(dn, pn):
    dn.join_side(); pn.join_side()
    torch.cuda.synchronize()
    return dn.flat_grad.clone(), pn.flat_grad.clone()


def test_deterministic_step_runs_the_fused_backward():
    from coivo_amd import _lib
    dn, pn = _nets()
    b = _batch()
    dn.zero_grad(); pn.zero_grad()
    torch.cuda.synchronize()
    _lib.form_counts(reset=True)
    _pass(dn, pn, b)
    _grads(dn, pn)
    forms = _lib.form_counts()
    assert forms["bwd16"] == 1, forms
    bwd = [pr for which, (pr, _) in next(iter(dn._insts.values()))[-1].passes.items() if which.startswith("bwd")]
    assert len(bwd) == 1
    cmds = [bwd[0]._arr[i] for i in range(len(bwd[0]))]
    fused = [c for c in cmds if c.op == _lib.CMD_CONV_BWD_FUSED]
    assert len(fused) == 1 and fused[0].stream == 0
    # mode 0 (the head's input gradient comes from the head's own kernel: nn.DepthNet._backward_impl says why) with the slab scratch:
    # 4 frames of 64x96 = 192 tiles, one per workgroup
    assert not fused[0].p[6] and not fused[0].p[7] and not fused[0].p[8] and fused[0].p[9] and fused[0].i[1] == 192 * ROW * 4
    # ... run without dw: one reduction on a weight-gradient stream adds the rows to the arena
    assert not fused[0].p[4] and fused[0].p[5] and [c.stream for c in cmds if c.op == _lib.CMD_WGRAD_REDUCE_GROUP] == [1]


def test_deterministic_steps_repeat_bit_for_bit():
    from coivo_amd.optim import FusedAdam
    b = _batch()

    def run():
        dn, pn = _nets()
        opt = FusedAdam([dn, pn], lr=1e-3)
        for _ in range(3):
            opt.zero_grad()
            _pass(dn, pn, b)
            opt.step()
        torch.cuda.synchronize()
        return dn.flat_param.clone(), pn.flat_param.clone()

    first, second = run(), run()
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


def test_two_passes_share_the_slab_scratch():
    """Two backward passes of one step without a join between them (the second replays the recorded pass, slab scratch included,
    while nothing on the host has waited for the first) against the same two passes with join_side() between them."""
    b1, b2 = _batch(), _batch(SEED + 1)

    def run(join):
        dn, pn = _nets()
        dn.zero_grad(); pn.zero_grad()
        _pass(dn, pn, b1)
        if join:
            dn.join_side(); pn.join_side()
            torch.cuda.synchronize()
        _pass(dn, pn, b2)
        return _grads(dn, pn)

    apart, together = run(True), run(False)
    assert torch.equal(apart[0], together[0]) and torch.equal(apart[1], together[1])
    single = run(True)
    assert torch.equal(apart[0], single[0])


def test_deterministic_step_agrees_with_the_three_kernel_path(monkeypatch):
    """The path the deterministic step took before (head input gradient, plain input gradient, k_wgrad3x3 + k_wgrad_reduce; developer
    switch COLVO_NO_BWD16) in the same process, and the HEAD form in deterministic mode (developer switch COLVO_DET_BWD16_HEAD).
    The reduction inside the command on the main stream (developer switch COLVO_DET_BWD16_MAIN) adds the same rows in the same order:
    bit for bit the default placement.
    iconv1's dw is summed in another order, its dx comes from another kernel (a bf16 rounding of the last bit on a few elements) and
    the HEAD form makes the head's input gradient by split-bf16 MFMA before the bf16 rounding: the pair of forms tests/test_nets_gpu.py
    test_grouped_slab_weight_gradients_equal_the_default_form bounds at 4e-3 of an arena's largest element."""
    from coivo_amd import _lib
    b = _batch()

    def run(old, head=False, main=False):
        monkeypatch.setenv("COLVO_DEV", "1")
        for name, on in (("COLVO_NO_BWD16", old), ("COLVO_DET_BWD16_HEAD", head), ("COLVO_DET_BWD16_MAIN", main)):
            if on:
                monkeypatch.setenv(name, "1")
            else:
                monkeypatch.delenv(name, raising=False)
        dn, pn = _nets()
        dn.zero_grad(); pn.zero_grad()
        torch.cuda.synchronize()
        _lib.form_counts(reset=True)
        _pass(dn, pn, b)
        g = _grads(dn, pn)
        return g, _lib.form_counts()["bwd16"]

    (new, n_new), (old, n_old), (head, n_head) = run(False), run(True), run(False, head=True)
    assert n_new == 1 and n_old == 0 and n_head == 1
    (main, n_main) = run(False, main=True)
    assert n_main == 1 and torch.equal(main[0], new[0]) and torch.equal(main[1], new[1])
    for form, got in (("fused", new), ("fused, HEAD form", head)):
        for a, c, name in zip(got, old, ("DepthNet", "PoseNet")):
            scale = c.abs().max().item()
            err = (a - c).abs().max().item()
            print(f"{name}: max|{form} - three-kernel| = {err:.3e} = {err / scale:.3e} of the arena's largest element")
            assert err <= 4e-3 * scale
