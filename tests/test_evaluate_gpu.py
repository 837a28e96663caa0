"""-m gpu checks of the depth measures (coivo_amd/evaluate.py, csrc/evaluate.hip) against references computed here: the medians
by torch.nanmedian on the CPU (invalid pixels set to NaN), the rest by a NumPy float32 / float64 replica of the definitions in
evaluate.py's docstring."""
import math

import numpy as np
import pytest
import torch

from coivo_amd import synth
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

LO, HI = 0.1, 10.0
FLT_MAX = float(np.finfo(np.float32).max)
REL = 1e-5          # abs_rel, sq_rel, rmse, rmse_log against the float64 reference
ATOL = 1e-6         # ... for measures that are ~0 (a prediction equal to gt up to rounding)


def _valid(gt, mask, lo=LO, hi=HI):
    v = (gt > float(np.float32(lo))) & (gt < float(np.float32(hi)))          # the float32 bounds the kernel compares with
    return v if mask is None else v & (mask != 0)


def _reference(pred, gt, mask=None, lo=LO, hi=HI, scaling=True):
    """-> (medians of gt and pred [N] float32 by torch.nanmedian, scale [N] float32, n [N], per_image [N,7] float64)"""
    N = pred.shape[0]
    P = pred.reshape(N, -1).float()
    G = gt.reshape(N, -1).float()
    M = None if mask is None else mask.reshape(N, -1)
    valid = _valid(G, M, lo, hi)
    nan = torch.tensor(float("nan"))
    med_g = torch.nanmedian(torch.where(valid, G, nan), dim=1).values
    med_p = torch.nanmedian(torch.where(valid, P, nan), dim=1).values
    lo32, hi32 = np.float32(lo), np.float32(hi)
    scale = np.full(N, np.nan, dtype=np.float32)
    out = np.full((N, 7), np.nan)
    n = valid.sum(dim=1).numpy()
    for i in range(N):
        if n[i] == 0:
            continue
        v = valid[i].numpy()
        s = np.float32(med_g[i].item()) / np.float32(med_p[i].item()) if scaling else np.float32(1.0)
        scale[i] = s
        g = G[i].numpy()[v]
        p = np.minimum(np.maximum(s * P[i].numpy()[v], lo32), hi32)
        assert g.dtype == np.float32 and p.dtype == np.float32
        th = np.maximum(g / p, p / g)
        g64, p64 = g.astype(np.float64), p.astype(np.float64)
        d = g64 - p64
        out[i, 0] = np.mean(np.abs(d) / g64)
        out[i, 1] = np.mean(d * d / g64)
        out[i, 2] = math.sqrt(np.mean(d * d))
        out[i, 3] = math.sqrt(np.mean((np.log(g64) - np.log(p64)) ** 2))
        for j, t in enumerate((1.25, 1.5625, 1.953125)):
            out[i, 4 + j] = int((th < np.float32(t)).sum()) / int(n[i])
    return med_g, med_p, scale, n, out


def _gpu_medians(pred, gt, mask, lo=LO, hi=HI):
    """The kernel's exact medians through the public call: with pred == 1 the scale IS med(gt); with the roles swapped (pred as
    gt, the original valid set as the mask, a range that admits every positive finite value) it is med(pred)."""
    from coivo_amd import evaluate as E
    ones = torch.ones_like(pred)
    med_g = E.depth_metrics(ones, gt, mask, min_depth=lo, max_depth=hi).scale
    valid = _valid(gt, mask, lo, hi)
    med_p = E.depth_metrics(ones, pred, valid, min_depth=0.0, max_depth=FLT_MAX).scale
    return med_g.cpu(), med_p.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(torch.int64)


def _smooth(N, H, W, seed):
    return synth.make_batch(N, H, W, seed=seed)["gt_depth"]


def _case(name):
    g = torch.Generator().manual_seed(sum(map(ord, name)))

    def u(*shape, a=0.0, b=1.0):
        return a + (b - a) * torch.rand(*shape, generator=g)

    mask = None
    if name == "odd":
        gt, pred = u(2, 1, 5, 7, a=0.5, b=5.0), u(2, 1, 5, 7, a=0.2, b=3.0)
    elif name == "even":
        gt, pred = u(2, 1, 4, 4, a=0.5, b=5.0), u(2, 1, 4, 4, a=0.2, b=3.0)
    elif name == "ties":
        gt = torch.round(u(3, 1, 64, 64, a=0.5, b=2.0) * 256) / 256
        pred = torch.round(u(3, 1, 64, 64, a=0.2, b=1.0) * 256) / 256
    elif name == "constant":
        gt, pred = torch.full((2, 1, 16, 24), 2.5), torch.full((2, 1, 16, 24), 0.7)
    elif name == "one_valid":
        gt, pred = torch.full((2, 1, 9, 11), 20.0), u(2, 1, 9, 11, a=0.2, b=3.0)
        gt[0, 0, 4, 5], gt[1, 0, 0, 0] = 3.0, 0.25
    elif name == "exponents":
        pred = torch.exp2(u(4, 1, 32, 48, a=-60.0, b=60.0))
        gt = torch.pow(10.0, u(4, 1, 32, 48, a=-1.5, b=1.5))
    elif name == "mask":
        gt, pred = u(3, 1, 40, 56, a=0.05, b=12.0), u(3, 1, 40, 56, a=0.2, b=3.0)
        mask = torch.rand(3, 1, 40, 56, generator=g) < 0.3
    elif name == "nonfinite":
        gt, pred = u(3, 1, 32, 32, a=0.5, b=5.0), u(3, 1, 32, 32, a=0.2, b=3.0)
        r = torch.rand(gt.shape, generator=g)
        gt[r < 0.05] = float("nan")
        gt[(r >= 0.05) & (r < 0.10)] = float("inf")
        gt[(r >= 0.10) & (r < 0.15)] = -float("inf")
        gt[(r >= 0.15) & (r < 0.20)] = -1.0
    elif name == "ragged":
        gt, pred = u(3, 1, 17, 23, a=0.05, b=11.0), u(3, 1, 17, 23, a=0.2, b=3.0)
    elif name in ("n64_256x320", "n8_512x640"):
        N, H, W = (64, 256, 320) if name == "n64_256x320" else (8, 512, 640)
        gt = _smooth(N, H, W, 11)
        pred = 0.37 * gt * torch.exp(0.15 * torch.randn(gt.shape, generator=g))
        gt[:, :, :8] = 12.0                                           # some rows beyond max_depth
        mask = torch.rand(gt.shape, generator=g) < 0.9 if name == "n8_512x640" else None
    else:
        raise KeyError(name)
    return pred.float().contiguous(), gt.float().contiguous(), mask


CASES = ["odd", "even", "ties", "constant", "one_valid", "exponents", "mask", "nonfinite", "ragged", "n64_256x320", "n8_512x640"]


def _check(res, ref):
    _, _, scale, n, want = ref
    assert torch.equal(res.n_valid.cpu(), torch.from_numpy(n.astype(np.int32)))
    got_s = res.scale.cpu()
    ok = n > 0
    okt = torch.from_numpy(ok)
    assert torch.equal(_bits(got_s[okt]), _bits(torch.from_numpy(scale)[okt])), (got_s, scale)
    assert torch.isnan(got_s[~okt]).all()
    got = res.per_image.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[ok, 4:], want[ok, 4:]), "delta fractions differ from the float32 replica"
    err = np.abs(got[ok, :4] - want[ok, :4])
    bound = REL * np.abs(want[ok, :4]) + ATOL
    assert (err <= bound).all(), (np.max(err / np.maximum(np.abs(want[ok, :4]), 1e-30)), got[ok, :4][err > bound][:5])


@pytest.mark.parametrize("name", CASES)
def test_medians_are_bit_exact(name):
    from coivo_amd import evaluate as E
    pred, gt, mask = _case(name)
    ref = _reference(pred, gt, mask)
    d = dev()
    mk = None if mask is None else mask.to(d)
    med_g, med_p = _gpu_medians(pred.to(d), gt.to(d), mk)
    ok = torch.from_numpy(ref[3] > 0)
    assert torch.equal(_bits(med_g[ok]), _bits(ref[0][ok])), "med(gt)"
    assert torch.equal(_bits(med_p[ok]), _bits(ref[1][ok])), "med(pred)"
    assert torch.isnan(med_g[~ok]).all()
    _check(E.depth_metrics(pred.to(d), gt.to(d), mk), ref)


def test_uint8_mask_equals_bool_mask():
    from coivo_amd import evaluate as E
    pred, gt, mask = _case("mask")
    d = dev()
    a = E.depth_metrics(pred.to(d), gt.to(d), mask.to(d))
    b = E.depth_metrics(pred.to(d), gt.to(d), mask.to(d, torch.uint8) * 7)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x) if x.is_floating_point() else x, _bits(y) if y.is_floating_point() else y)


def test_empty_images_are_nan_and_skipped():
    from coivo_amd import evaluate as E
    pred, gt, _ = _case("ragged")
    gt[1] = 50.0                                   # no valid pixel
    d = dev()
    res = E.depth_metrics(pred.to(d), gt.to(d))
    _check(res, _reference(pred, gt))
    assert int(res.n_valid[1]) == 0 and math.isnan(float(res.scale[1])) and torch.isnan(res.per_image[1]).all()
    summ = E.summarize(res)
    assert summ["images"] == 2 and summ["skipped"] == 1
    keep = res.per_image.cpu()[[0, 2]].mean(dim=0)
    for i, name in enumerate(E.METRICS):
        assert summ[name] == float(keep[i])
    # all images empty: NaN means, nothing counted
    none = E.summarize(E.depth_metrics(pred.to(d), torch.full_like(gt, 50.0).to(d)))
    assert none["images"] == 0 and none["skipped"] == 3 and math.isnan(none["abs_rel"])


def test_summarize_streams_batches():
    from coivo_amd import evaluate as E
    pred, gt, mask = _case("mask")
    d = dev()
    whole = E.depth_metrics(pred.to(d), gt.to(d), mask.to(d))
    parts = [E.depth_metrics(pred[i:i + 1].to(d), gt[i:i + 1].to(d), mask[i:i + 1].to(d)) for i in range(3)]
    assert E.summarize(*parts) == E.summarize(whole)


def test_without_median_scaling_the_scale_is_one():
    from coivo_amd import evaluate as E
    pred, gt, mask = _case("mask")
    d = dev()
    res = E.depth_metrics(pred.to(d), gt.to(d), mask.to(d), median_scaling=False)
    assert (res.scale.cpu() == 1.0).all()
    _check(res, _reference(pred, gt, mask, scaling=False))


def test_scale_only_prediction_has_no_error():
    from coivo_amd import evaluate as E
    gt = _smooth(4, 64, 96, 5)
    d = dev()
    res = E.depth_metrics((3.0 * gt).to(d), gt.to(d))
    assert (res.per_image[:, 0] < 1e-6).all() and (res.per_image[:, 4] == 1.0).all()
    assert (res.scale.cpu() - 1.0 / 3.0).abs().max() < 1e-6


def test_deterministic_and_on_any_stream():
    from coivo_amd import evaluate as E
    pred, gt, mask = _case("n8_512x640")
    d = dev()
    pred, gt, mask = pred.to(d), gt.to(d), mask.to(d)
    a = E.depth_metrics(pred, gt, mask)
    b = E.depth_metrics(pred, gt, mask)
    s = torch.cuda.Stream(device=d)
    s.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(s):
        c = E.depth_metrics(pred, gt, mask)
    torch.cuda.current_stream(d).wait_stream(s)
    for r in (b, c):
        assert torch.equal(_bits(a.per_image), _bits(r.per_image))
        assert torch.equal(_bits(a.scale), _bits(r.scale))
        assert torch.equal(a.n_valid, r.n_valid)


def test_evaluate_sequence_agrees_with_its_parts():
    """evaluate_sequence on a 5-frame synthetic sequence: its measures are depth_metrics / ate / rpe of its own outputs, and its
    networks' outputs are reconstruct_sequence's (the two share inference.run_networks)."""
    from coivo_amd import evaluate as E, inference as I, nn as hnn
    torch.manual_seed(21)
    dn, pn = hnn.DepthNet(), hnn.PoseNet()
    n, H, W = 5, 64, 96
    b = synth.make_batch(n, H, W, seed=21)
    d = dev()
    frames, K, gt_depths = b["tgt"].to(d), b["K"].to(d), b["gt_depth"].to(d)
    g = torch.Generator().manual_seed(4)
    G = I.integrate_trajectory(torch.cat([0.05 * torch.randn(n - 1, 3, generator=g), 0.02 * torch.randn(n - 1, 3, generator=g)], 1))
    ev = E.evaluate_sequence(dn, pn, frames, gt_depths=gt_depths, gt_cam2world=G, chunk=2)
    assert ev.depths.shape == (n, 1, H, W) and ev.rel_poses.shape == (n - 1, 6) and ev.cam2world.shape == (n, 4, 4)
    direct = E.depth_metrics(ev.depths, gt_depths)
    assert torch.equal(_bits(ev.depth.per_image), _bits(direct.per_image))
    assert torch.equal(_bits(ev.depth.scale), _bits(direct.scale)) and torch.equal(ev.depth.n_valid, direct.n_valid)
    assert ev.summary == E.summarize(direct)
    assert ev.ate == E.ate(ev.cam2world, G) and ev.rpe == E.rpe(ev.cam2world, G)
    assert torch.equal(ev.cam2world, I.integrate_trajectory(ev.rel_poses))
    only_depth = E.evaluate_sequence(dn, pn, frames, gt_depths=gt_depths, chunk=3, median_scaling=False)
    assert only_depth.ate is None and only_depth.rpe is None and (only_depth.depth.scale == 1.0).all()

    rec = I.reconstruct_sequence(dn, pn, frames, K, stride=4, chunk=2)
    assert torch.equal(rec.depths, ev.depths) and torch.equal(rec.rel_poses, ev.rel_poses)
    assert torch.equal(rec.cam2world, ev.cam2world)
    cloud = I.stitch_point_cloud(ev.depths, K, ev.cam2world.to(d, torch.float32), stride=4)
    assert torch.equal(rec.points, cloud)


def test_argument_errors():
    from coivo_amd import evaluate as E
    d = dev()
    t = torch.ones(2, 1, 8, 8, device=d)
    with pytest.raises(ValueError):
        E.depth_metrics(t, torch.ones(2, 1, 8, 9, device=d))
    with pytest.raises(ValueError):
        E.depth_metrics(t, t.double())
    with pytest.raises(ValueError):
        E.depth_metrics(t, t, torch.ones(2, 1, 8, 8, device=d))                  # float mask
    with pytest.raises(ValueError):
        E.depth_metrics(t, t, min_depth=5.0, max_depth=1.0)


@pytest.mark.parametrize("name", ["ragged", "mask", "one_valid", "ragged_one_empty"])
def test_memory_discipline(name):
    """depth_metrics under tests/guarded.py: prediction, ground truth and mask between guard bands; the workspace
    (colvo_depth_metrics_workspace_bytes: the histogram levels of the exact median and the sums), per_image, scale and n_valid from the
    pool under both poisons.  Outputs meet the reference as in _check, are the same bytes under either poison, and no guard byte
    changes.  Launches reached: k_eval_init, the radix passes of both medians and the sums, at a ragged 17 x 23 (one image of it with
    no valid pixel in the last case), with a mask, and with a single valid pixel per image."""
    from coivo_amd import _lib, evaluate as E
    from tests import guarded as G
    pred, gt, mask = _case(name.split("_one_empty")[0])
    if name == "ragged_one_empty":
        gt[1] = 50.0
    ref = _reference(pred, gt, mask)
    d = dev()
    run = lambda pool: E.depth_metrics(pool.place(pred.to(d)), pool.place(gt.to(d)), None if mask is None else pool.place(mask.to(d)))
    outs, pools = G.under_both_poisons(d, run, f"depth_metrics {name}")
    N, _, H, W = pred.shape
    for res, pool in zip(outs, pools):
        _check(res, ref)
        G.assert_served(pool, 0, _lib.load().colvo_depth_metrics_workspace_bytes(N, H, W), "depth_metrics")
    if name == "ragged_one_empty":
        assert int(outs[0].n_valid[1]) == 0 and torch.isnan(outs[0].per_image[1]).all()
