"""-m gpu: every conv layer of DepthNet and PoseNet at the benchmark's own shapes, production tuning, held BIT-EXACTLY to a float64
reference on exact data (tests/conv_exact.py: operands that are small integers times a power-of-two quantum, so that every
summation order gives the exact answer).  A dropped or doubled pixel tile, a wrong tap, a wrong ReLU tie or a mis-masked gradient
fails; test_conv_gpu.py's relative bars (2e-4 of the largest weight-gradient element, one bf16 ulp of a feature map) cannot see a
small local mistake at these sizes.

Shapes: DepthNet at 16 / 64 / 128 frames of 256x320 and 64 frames of 512x640 (configs[1], [3], [4], [2] per GPU), PoseNet's
stride-2 chain at 8 / 32 / 64 pairs of 256x320 and 32 pairs of 512x640 (its odd deep extents included); bf16 and f32 each.  Around
every pass the kernel-form counters are read: the test asserts the structure of each dispatch (one leaf per launch) and the forms
the planner picks at these shapes (csrc/tuning.h), and prints the forms reached per shape."""
import gc

import pytest
import torch

from tests import conv_exact as X
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float32)
SHAPES = [("depth", 16, 256, 320), ("depth", 64, 256, 320), ("depth", 128, 256, 320), ("depth", 64, 512, 640),
          ("pose", 8, 256, 320), ("pose", 32, 256, 320), ("pose", 64, 256, 320), ("pose", 32, 512, 640)]

# Forms the production sweep reaches (asserted by test_the_sweep_reaches_its_forms; test_conv_gpu.py's coverage test adds the small
# cases' forms to these and expects every counter of the library).  Not among them, a finding of this sweep: k_conv_q (conv_q) runs
# at NO benchmark shape under the production tuning -- k_conv_rt is tried first and takes every grid large enough for quad_min_wgs,
# configs[2]'s iconv2 included (tuning.h) -- and neither do the off-by-default k_wgrad_rt and 512-thread one-tile form; the small
# cases of test_conv_gpu.py reach all three.
PRODUCTION_FORMS = {"conv_rt", "conv_rt_bn32", "wgrad_full_grid", "wgrad_halved_grid", "wgrad_up2", "wgrad_store_clean", "conv_res_s2", "conv_up2_bn16",
                    "conv_up2_bn32", "dgrad_s2", "dgrad_s2_ring", "dgrad_up2", "dgrad_both", "conv_tile", "conv_ring", "conv_res", "conv_bn64",
                    "wgrad_teams", "wgrad_tail", "wgrad_mt4", "wgrad_sliced", "bwd16", "fwd16_head", "dgrad_planes_mfma"}

_SEEN = {}          # shape -> {form: launches} of the sweep in this process


def _free():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def sweep(net, B, H, W):
    """Every layer x dtype of one shape; returns {form: launches} and checks the per-layer form claims."""
    from coivo_amd import _lib
    assert _lib.tune_get("wgrad_rt") == 0 and _lib.tune_get("quad_min_wgs") == 8192, "production tuning expected"
    d = dev()
    g = torch.Generator(device=d).manual_seed(B * 100003 + H * 7 + (net == "pose"))
    total = {dt: {} for dt in DTYPES}
    for name, lay in X.layers(net, B, H, W):
        data = X.make_data(lay, g, d)
        for dt in DTYPES:
            forms = X.check_layer(lay, dt, g, d, data=data)
            X.check_forms(lay, dt, forms)
            _layer_claims(net, name, lay, dt, forms)
            line = {p: f for p, f in forms.items() if f}
            print(f"FORMS {net} B={B} {H}x{W} {name} {str(dt)[6:]}: {line}")
            for f in forms.values():
                for k, v in f.items():
                    total[dt][k] = total[dt].get(k, 0) + v
        del data
        _free()
    return total


def _layer_claims(net, name, lay, dt, forms):
    """Forms the planner must pick for this layer at production tuning (csrc/conv.hip, wgrad.hip, tuning.h)."""
    what = f"{net} {name} {lay.__dict__} {dt}: {forms}"
    wg = forms["wgrad"]
    assert wg.get("wgrad_rt", 0) == 0, what                             # wgrad_rt = 0: the register-tiled weight gradient stays off
    if net == "depth" and name == "iconv2" and lay.B >= 64:
        assert forms["fwd"].get("conv_rt_bn32") == 1, what              # N = 32: k_conv_rt's 32-channel form (rt_bn32_min_wgs)
    if lay.up0 and not lay.C1:                                           # the five up-sampled layers: the four-class weight gradient
        assert wg.get("wgrad_up2", 0) == X.wgrad_slices(lay, dt), what
    if lay.C0 == 16 and lay.Cout == 16 and not lay.up0 and lay.stride == 1:
        # iconv1, the 16 -> 16 full-resolution layer: the teams form (one co tile, one chunk); bf16: the fused kernels
        assert wg.get("wgrad_teams", 0) == X.wgrad_slices(lay, dt), what
        if dt == torch.bfloat16:
            assert forms["fwd16_head"].get("fwd16_head") == 1 and forms["bwd16"].get("bwd16") == 1, what
    if net == "pose" and name == "conv1" and dt == torch.bfloat16:
        assert forms["dgrad_planes"].get("dgrad_planes_mfma") == 1, what
    if forms["wgrad_clean"].get("wgrad_store_clean"):
        assert forms["wgrad"].get("wgrad_store_clean", 0) == 0, what     # only the vouched-for call stores


@pytest.mark.parametrize("net,B,H,W", SHAPES)
def test_every_layer_bit_exact_at_the_production_shape(net, B, H, W):
    _free()
    total = sweep(net, B, H, W)
    _SEEN[(net, B, H, W)] = total
    print(f"FORMS-TOTAL {net} B={B} {H}x{W}: " + "; ".join(f"{str(dt)[6:]} {sorted(f.items())}" for dt, f in total.items()))
    bf, f32 = total[torch.bfloat16], total[torch.float32]
    if net == "depth" and B >= 64:
        for t in (bf, f32):
            assert t.get("wgrad_mt4", 0) > 0, t                     # 64-wide co tiles from a walk of wgrad_mt4_min_walk tiles on
            assert t.get("conv_rt", 0) > 0, t
            assert t.get("conv_rt_bn32", 0) > 0, t                  # the 32-channel form from rt_bn32_min_wgs workgroups on (iconv2)
            assert t.get("conv_q", 0) == 0, t
    if (net, B, H, W) == ("depth", 64, 512, 640):
        # the image-sliced weight gradient (which layers: X.wgrad_slices, checked per call by X.check_forms) -- in f32 the 16-channel
        # full-resolution layers themselves pass 1 GiB
        assert f32.get("wgrad_sliced", 0) > bf.get("wgrad_sliced", 0) > 0, (bf, f32)
    _free()


def test_the_sweep_reaches_its_forms():
    """The union of the forms the sweep counted is PRODUCTION_FORMS (shapes not yet swept in this process are swept here)."""
    union = set()
    for shape in SHAPES:
        if shape not in _SEEN:
            _SEEN[shape] = sweep(*shape)
            _free()
        for t in _SEEN[shape].values():
            union |= {k for k, v in t.items() if v}
    assert union == PRODUCTION_FORMS, (sorted(union - PRODUCTION_FORMS), sorted(PRODUCTION_FORMS - union))


def test_gpu_reference_is_the_cpu_float64_reference():
    """The float64 reference on the GPU (the one the sweep uses) against the same functions on the CPU at a small shape with odd
    extents, an up-sampled source, a concat and a stride-2 layer."""
    g = torch.Generator().manual_seed(3)
    for lay in (X.Layer(2, 10, 14, 16, 8, True, False, 24, 1), X.Layer(3, 13, 11, 8, 0, False, False, 16, 2)):
        data = X.make_data(lay, g, "cpu")
        gd = {k: (v.to(dev()) if v is not None else None) for k, v in data.items()}
        args = lambda t: (t["x0"], t["x1"], t["w"], t["bias"], 0, lay.B)
        assert torch.equal(lay.ref_fwd(*args(gd)).cpu(), lay.ref_fwd(*args(data)))
        for a, b in zip(lay.ref_dgrad(gd["dy_dense"], gd["w"], 0, lay.B), lay.ref_dgrad(data["dy_dense"], data["w"], 0, lay.B)):
            assert (a is None and b is None) or torch.equal(a.cpu(), b)
        for a, b in zip(lay.ref_wgrad(gd["x0"], gd["x1"], gd["dy_wgrad"]), lay.ref_wgrad(data["x0"], data["x1"], data["dy_wgrad"])):
            assert torch.equal(a.cpu(), b)
        # ... and the CPU reference is plain arithmetic: one output element of each pass by hand
        x = torch.cat([data["x0"].repeat_interleave(2, 1).repeat_interleave(2, 2) if lay.up0 else data["x0"]]
                      + ([data["x1"]] if lay.C1 else []), dim=3).double()
        w, s = data["w"].double(), lay.stride
        b, oy, ox, co = 1, lay.Ho - 1, 1, lay.Cout - 1
        acc = float(data["bias"][co])
        for t in range(9):
            iy, ix = oy * s + t // 3 - 1, ox * s + t % 3 - 1
            if 0 <= iy < lay.Hi and 0 <= ix < lay.Wi:
                acc += float((x[b, iy, ix] * w[co, t]).sum())
        assert float(lay.ref_fwd(*args(data))[b, oy, ox, co]) == max(acc, 0.0)
        dy = data["dy_wgrad"].double()
        t, ci = 4, 3
        dwv = sum(float(dy[bb, yy, xx, co] * x[bb, yy * s, xx * s, ci]) for bb in range(lay.B) for yy in range(lay.Ho)
                  for xx in range(lay.Wo))
        assert float(lay.ref_wgrad(data["x0"], data["x1"], data["dy_wgrad"])[0][co, t, ci]) == dwv


def test_a_dropped_tile_or_image_changes_the_exact_answer():
    """Sensitivity, in torch on the reference alone: remove one 128-pixel tile's (8 x 16 pixels) or one image's contribution from a
    production-shape weight gradient (enc3b at 64 frames of 256x320) -- torch.equal fails on either.  On this data test_conv_gpu.py's
    relative bar (2e-4 of the largest element + 2e-4 relative) fails too: dy has random signs, so dw is a random walk over ~3e5
    pixels and 128 of them move it by a few percent of max|dw|; the exact bar does not depend on that."""
    lay = dict(X.layers("depth", 64, 256, 320))["enc3b"]
    g = torch.Generator(device=dev()).manual_seed(5)
    data = X.make_data(lay, g, dev())
    X.check_wgrad_bound([data["x0"]], data["dy_wgrad"], "enc3b")
    ref, _ = lay.ref_wgrad(data["x0"], None, data["dy_wgrad"])
    results = {}
    for what in ("tile", "image"):
        dy = data["dy_wgrad"].clone()
        if what == "tile":
            dy[17, 8:16, 16:32] = 0
        else:
            dy[17] = 0
        got, _ = lay.ref_wgrad(data["x0"], None, dy)
        assert not torch.equal(got.float(), ref.float()), what
        err = (got - ref).abs()
        old_bar_passes = bool((err <= 2e-4 * ref.abs().max() + 2e-4 * ref.abs()).all())
        results[what] = (float(err.max() / ref.abs().max()), old_bar_passes)
        assert not old_bar_passes, (what, results[what])
    print(f"SENSITIVITY enc3b 64x256x320 wgrad: {results} (max err / max |dw|, passes the 2e-4 bar)")
