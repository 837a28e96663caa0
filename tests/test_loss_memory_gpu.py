"""-m gpu: the loss kernels held to their own memory (tests/guarded.py).

Every case of tests/test_loss_geometry_gpu.py listed below runs through coivo_amd.functional inside guarded_allocations, once per
poison: the workspaces (colvo_warp_loss_workspace_floats, colvo_geo_loss_workspace_floats, colvo_full_objective_workspace_floats), the
loss state, the raw planes and every gradient output are allocated by the wrappers from the pool, between guard bands and filled with
0xFF bytes (NaN) or 0x55 bytes (a large finite number).  The inputs -- tgt, ref, depth, d_r, pose, K, lcc_a, lcc_b -- are guarded
copies: a tap above the first or below the last plane reads NaN.  The B = 1 cases are there so that the first and the last image row
border a guard.

Per case: loss, valid counts and every gradient are the same bytes under the two poisons (a kernel that reads workspace it never wrote,
needs it zeroed, or leaves part of an output unwritten differs, or gives NaN); they meet test_loss_geometry_gpu's bars against float64
(same march_rows knobs, same seeds, same reference: loss_ref.evaluate); no guard byte changed; and one allocation had exactly the size
the workspace query returns."""
import pytest
import torch

from tests import guarded as G
from tests import loss_ref as R
from tests.gpu_util import assert_close_frac, dev
from tests.test_loss_geometry_gpu import _check, _id, _motion, fused, march_rows  # noqa: F401  (the last two are fixtures)

pytestmark = pytest.mark.gpu

ONE_PASS = [(4, 3, 8, 60), (5, 1, 2, 121), (16, 3, 33, 61)]
TWO_PASS = [(4, 2, 7, 121)]
FORWARD = [(5, 3, 11, 62), (63, 1, 2, 120)]
FULL = [(5, 3, 26, 62, 2), (4, 2, 40, 120, 4), (16, 1, 68, 180, 3)]


def _state(loss):
    """The four floats of the loss state `loss` is element 0 of (functional._WarpLoss: [loss, 1 / max(3 n, 1), n, masked sum]).  Under the
    patch the state is itself a view into the pool's byte buffer, which is then what `_base` names."""
    base = loss._base
    if base.dtype == torch.uint8:
        off = loss.storage_offset() * 4
        base = base[off:off + 16].view(torch.float32)
    return base


def _photometric(t, form, pool):
    """tests/test_loss_geometry_gpu.py's _photometric with guarded inputs, under the patch."""
    from coivo_amd import functional as Fh
    d = {k: pool.place(v.to(dev()), k) for k, v in t.items()}
    if form == "fwd":
        with torch.no_grad():
            loss = Fh.photometric_loss(d["tgt"], d["ref"], d["depth"], d["pose"], d["K"], d["lcc_a"], d["lcc_b"])
        return dict(loss=loss.clone(), count=[_state(loss)[2].clone()])
    leaves = [d[k].requires_grad_(True) for k in ("depth", "pose", "lcc_a", "lcc_b")]
    hand = None
    if form == "handover":
        hand = Fh.GradHandover()
        leaves[0]._colvo_handover = hand
    loss = Fh.photometric_loss(d["tgt"], d["ref"], leaves[0], leaves[1], d["K"], leaves[2], leaves[3])
    out = dict(loss=loss.detach().clone(), count=[_state(loss)[2].clone()])
    grads = list(torch.autograd.grad(loss, leaves))
    if hand is not None:
        sa, sb = hand.take((grads[0],))
        assert sa is not None and sb is not None, "the hand-over form did not run"
        out["d_depth_raw"] = grads[0]
        grads[0] = grads[0] * (sa * sb)
    out.update(zip(("d_depth", "d_pose", "d_a", "d_b"), grads))
    return out


def _full(t, kw, pool):
    from coivo_amd import functional as Fh
    d = {k: pool.place(v.to(dev()), k) for k, v in t.items()}
    leaves = [d[k].requires_grad_(True) for k in ("depth", "d_r", "pose", "lcc_a", "lcc_b")]
    loss = Fh.dcdp_full_loss(d["tgt"], d["ref"], leaves[0], leaves[1], leaves[2], d["K"], leaves[3], leaves[4], **kw)
    # (of the 32 floats of the view, four per pyramid level behind the first four are written; the rest belongs to levels this call has not)
    terms = Fh.full_objective_terms(loss)[:4 + 4 * kw["num_scales"]].clone()
    out = dict(loss=loss.detach().clone(), count=[terms[4 + 4 * s + 2] for s in range(kw["num_scales"])], terms=terms)
    out.update(zip(("d_depth", "d_r", "d_pose", "d_a", "d_b"), torch.autograd.grad(loss, leaves)))
    return out


def _host(h):
    """the result in the form test_loss_geometry_gpu._check takes"""
    out = {k: v.cpu() for k, v in h.items() if k.startswith("d_") and k != "d_depth_raw"}
    out.update(loss=h["loss"].item(), count=[c.item() for c in h["count"]])
    return out


def _both(run, t, tag, ws_floats, **kw):
    """run(pool) under both poisons -> (the result on the host, the float64 reference _check returns: None for forward-only cases)."""
    outs, pools = G.under_both_poisons(dev(), run, tag)
    for h, pool in zip(outs, pools):
        for k, v in h.items():
            if torch.is_tensor(v):
                assert bool(torch.isfinite(v).all()), f"{tag}: {k} is not finite"
        G.assert_served(pool, 0, 4 * int(ws_floats), tag)
    return _host(outs[0]), _check(_host(outs[0]), t, tag, **kw)


def _warp_ws(B, H, W):
    from coivo_amd import _lib
    return _lib.load().colvo_warp_loss_workspace_floats(B, H, W)


def _full_ws(B, H, W, S):
    from coivo_amd import _lib
    return _lib.load().colvo_full_objective_workspace_floats(B, H, W, S)


@pytest.mark.parametrize("case", ONE_PASS, ids=_id)
def test_one_pass(case, march_rows, fused):
    rows, B, H, W = case
    march_rows(bwd=rows)
    t = R.noisy_case(B, H, W, seed=500 + rows, pose_scale=_motion(H))
    _both(lambda pool: _photometric(t, "grad", pool), t, "one-pass " + _id(case), _warp_ws(B, H, W))


@pytest.mark.parametrize("case", TWO_PASS, ids=_id)
def test_two_pass(case, march_rows, fused):
    rows, B, H, W = case
    fused(False)
    march_rows(fwd=rows, bwd=rows)
    t = R.noisy_case(B, H, W, seed=520 + rows, pose_scale=_motion(H))
    _both(lambda pool: _photometric(t, "grad", pool), t, "two-pass " + _id(case), _warp_ws(B, H, W))


@pytest.mark.parametrize("case", FORWARD, ids=_id)
def test_forward_only(case, march_rows):
    rows, B, H, W = case
    march_rows(fwd=rows)
    t = R.noisy_case(B, H, W, seed=540 + rows, pose_scale=_motion(H))
    _both(lambda pool: _photometric(t, "fwd", pool), t, "forward " + _id(case), _warp_ws(B, H, W))


@pytest.mark.parametrize("case", FULL, ids=_id)
def test_full_objective(case, march_rows):
    rows, B, H, W, S = case
    march_rows(bwd=rows)
    t = R.noisy_case(B, H, W, seed=560 + rows, pose_scale=_motion(H))
    kw = dict(num_scales=S, geo_weight=0.5, smooth_weight=0.1)
    _both(lambda pool: _full(t, kw, pool), t, "full " + _id(case), _full_ws(B, H, W, S), **kw)


def test_hand_over_form(fused):
    """DepthNet.forward_pair_split's form with production tuning: d_depth stays raw and the scales are posted.  2 x 13 x 120: two strips
    of 60 columns, a last segment one row long."""
    B, H, W = 2, 13, 120
    t = R.noisy_case(B, H, W, seed=607)
    _both(lambda pool: _photometric(t, "handover", pool), t, f"hand-over B{B} {H}x{W}", _warp_ws(B, H, W))


@pytest.mark.parametrize("form", ["one-pass", "two-pass", "full"])
def test_image_behind_the_camera(form, fused):
    B, H, W = 3, 64, 124
    t = R.noisy_case(B, H, W, seed=620)
    t["pose"] = t["pose"].clone()
    t["pose"][1] = torch.tensor([0.0, 0.0, -100.0, 0.0, 0.0, 0.0])      # every point of image 1 behind the camera
    if form == "full":
        kw = dict(num_scales=2, geo_weight=0.5, smooth_weight=0.0)
        h, r64 = _both(lambda pool: _full(t, kw, pool), t, f"image 1 behind the camera, {form}", _full_ws(B, H, W, 2), **kw)
    else:
        fused(form == "one-pass")
        h, r64 = _both(lambda pool: _photometric(t, "grad", pool), t, f"image 1 behind the camera, {form}", _warp_ws(B, H, W))
    assert (r64["n_valid"][:, 1] == 0).all() and (r64["n_valid"][:, [0, 2]] > 0).all()
    for k in ("d_pose", "d_a", "d_b"):
        assert torch.count_nonzero(h[k][1]) == 0, f"{form}: {k} of the image with no valid pixel is not exactly zero"
    assert torch.count_nonzero(h["d_depth"][1]) == 0


# ---------------------------------------------------------------------------------------------------------------------- #
# the standalone terms, against the oracle with tests/test_terms_gpu.py's data recipes and bars                            #
# ---------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("B,H,W,seed", [(2, 33, 47, 62), (3, 17, 23, 64)])
def test_standalone_terms(B, H, W, seed):
    """geometric_consistency_loss, smoothness_loss, downsample2 (on the even part of the frame: it refuses odd sizes) and
    dcdp_full_loss_composite at one scale, each forward and backward under both poisons: guards intact, the oracle's value and
    gradients within test_terms_gpu's bars under either poison, and the same bits under both wherever the term has no float atomics."""
    from coivo_amd import _lib, functional as Fh, synth
    from oracle import colvo_spec as S
    b = synth.make_batch(B, H, W, seed=seed)
    g = torch.Generator().manual_seed(seed)
    d_t = (b["gt_depth"] * (1 + 0.05 * torch.randn(B, 1, H, W, generator=g))).clamp(0.2, 9.0)
    d_r = (b["gt_depth"] * (1 + 0.05 * torch.randn(B, 1, H, W, generator=g))).clamp(0.2, 9.0)
    He, We = H - H % 2, W - W % 2
    x = b["tgt"][:, :, :He, :We].contiguous()
    gy = torch.rand(B, 3, He // 2, We // 2, generator=g)

    def leaves_of(ts, place):
        return [place(t).requires_grad_(True) for t in ts]

    def geo(fn, place):
        lv = leaves_of((d_t, d_r, b["gt_pose"]), place)
        loss = fn(*lv, place(b["K"]))
        return (loss.detach().clone(),) + tuple(torch.autograd.grad(loss, lv))

    def smooth(fn, place):
        lv = leaves_of((b["gt_depth"],), place)
        loss = fn(lv[0], place(b["tgt"]))
        return (loss.detach().clone(),) + tuple(torch.autograd.grad(loss, lv))

    def pool2(fn, place):
        lv = leaves_of((x,), place)
        y = fn(lv[0])
        return (y.detach().clone(),) + tuple(torch.autograd.grad(y, lv, place(gy)))

    def composite(fn, place):
        lv = leaves_of((b["gt_depth"], b["gt_depth"] * 1.07 + 0.05, b["gt_pose"], b["gt_a"], b["gt_b"]), place)
        loss = fn(place(b["tgt"]), place(b["ref"]), lv[0], lv[1], lv[2], place(b["K"]), lv[3], lv[4], geo_weight=0.5, smooth_weight=0.1,
                  num_scales=1)
        return (loss.detach().clone(),) + tuple(torch.autograd.grad(loss, lv))

    lib = _lib.load()
    cases = (("geo", geo, Fh.geometric_consistency_loss, S.geometric_consistency_loss, 4 * lib.colvo_geo_loss_workspace_floats(B, H, W)),
             ("smooth", smooth, Fh.smoothness_loss, S.smoothness_loss, 4 * 2 * B * ((H * W + 255) // 256)),
             ("avgpool2", pool2, Fh.downsample2, S.downsample2, 4 * B * 3 * (He // 2) * (We // 2)),
             ("composite", composite, Fh.dcdp_full_loss_composite, S.dcdp_full_loss, 4 * lib.colvo_warp_loss_workspace_floats(B, H, W)))
    for name, run, hip, oracle, nbytes in cases:
        want = run(oracle, lambda t: t.clone())
        # the reference depth's gradient of the geometric term is scattered with float atomics (functional.geometric_consistency_loss):
        # it moves in its last bits from run to run, so it is held to the bars under either poison and left out of the bit comparison
        outs, pools = [], []
        for poison in G.POISONS:
            pool = G.Pool(dev(), poison)
            with G.guarded_allocations(pool):
                outs.append(run(hip, lambda t: pool.place(t.to(dev()))))
            pool.check(f"{name} {B}x{H}x{W}, poison {poison:#04x}")
            pools.append(pool)
        atomic = {"geo": 2, "composite": 2}.get(name)
        G.assert_same_bits(*([o for i, o in enumerate(out) if i != atomic] for out in outs), f"{name} {B}x{H}x{W}")
        for got, pool in zip(outs, pools):
            G.assert_served(pool, 0, nbytes, name)
            if name == "avgpool2":
                assert torch.allclose(got[0].cpu(), want[0], atol=1e-7) and torch.allclose(got[1].cpu(), want[1], atol=1e-7)
                continue
            assert abs(got[0].item() - want[0].item()) < (1e-6 if name == "smooth" else 1e-5), name
            for i, (a, c) in enumerate(zip(got[1:], want[1:])):
                plane = a.dim() == 4
                if name == "smooth":
                    assert_close_frac(a, c, rtol=1e-3, atol_scale=1e-4, max_bad_frac=1e-4, what="smooth d_depth")
                elif name == "geo":
                    assert_close_frac(a, c, rtol=2e-3, atol_scale=2e-4 if plane else 3e-3, max_bad_frac=5e-4 if plane else 0, what=f"geo grad {i}")
            if name == "composite":
                # every gradient against float64 with the bars of the main cases (test_loss_geometry_gpu._check on loss_ref.evaluate): the
                # per-image gradients (pose, a, b) are cancelling sums of a few 1e-4 here, which one L1 sign or tap cell taken the other
                # way inside the decision margin moves by more than rounding does -- _check allows for exactly that and for no more
                t = dict(tgt=b["tgt"], ref=b["ref"], depth=b["gt_depth"], d_r=b["gt_depth"] * 1.07 + 0.05, pose=b["gt_pose"], K=b["K"],
                         lcc_a=b["gt_a"], lcc_b=b["gt_b"])
                h = dict(zip(("d_depth", "d_r", "d_pose", "d_a", "d_b"), (x.cpu() for x in got[1:])), loss=got[0].item(), count=[])
                _check(h, t, f"composite {B}x{H}x{W}", num_scales=1, geo_weight=0.5, smooth_weight=0.1)
