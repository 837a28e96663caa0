"""-m gpu: every conv layer of DepthNet and PoseNet at the batch sizes of INFERENCE, production tuning, bit for bit against the float64
reference on exact data (tests/conv_exact.py) -- the sweep of tests/test_conv_exact_gpu.py at the shapes that sweep cannot reach.

inference.run_networks calls the networks with `chunk` frames (16 by default), the last call of a sequence with whatever is left
(1 to 15), a live stream with one frame.  The benchmark's batch sizes (16 k frames) share three things those do not: every
persistent walk is a whole number of rounds, every layer has more tiles than the chip has workgroup slots (every csrc/tuning.h
decision falls on its large side), and every image shares its deep layers with many others.  All passes of check_layer run, the
backward ones too: they cost little here and fine-tuning on a few frames reaches them.

Shapes (X.SMALL_BATCH_SHAPES) and why each is there.  Tile counts, grids and walks are derived from the planning code, not assumed:
plan_conv_t / plan_conv_res / res_s2_fits (csrc/conv.hip), conv_rt_plan (conv_rt.hip), colvo_conv_head_fused's grid (fwd16.hip),
bwd16_grid (bwd16.hip), wgrad_grid_floor / set_wgrad_grid (wgrad.hip).  A map whose extents are multiples of 8 x 16 is tiled in 8 x 16
pixels by pick_tile (an exact cover of 128-pixel tiles, conflict-free rows, 173 cost units per tile; a tile of fewer than 127 pixels
costs more per pixel), so a 256x320 map is 640 tiles, 128x160 is 160, 512x640 is 2560.  The two full-resolution layers are up1 and
iconv1; enc1a is stride 2, so enc1b sits at half resolution.  k_conv3x3_res walks `tile += gridDim.x` over a grid of min(1024, tiles):
its rounds are tiles / 1024.  k_fwd16_head and k_bwd16 walk consecutive tiles: grid 1024 / 768, tiles_per_wg = ceil(tiles / grid), then
grid = ceil(tiles / tiles_per_wg), and the LAST workgroup walks what is left.

  ("depth", 1, 256, 320), ("pose", 1, 256, 320)
      The deep maps are smaller than one tile: 8x10 (enc5, one 8x10 tile) and 16x20 (three 16x7 tiles); PoseNet's chain runs down to
      4x5 and 2x3, one tile each.  Every grid is below 256 workgroups x 4: at most 640 tiles (iconv1: fwd16 640 x 1, bwd16 640 x 1).
      No weights-resident or register-tiled kernel can be chosen (_layer_claims).
  ("depth", 3, 256, 320), ("pose", 3, 256, 320)
      An odd batch.  1920 full-resolution tiles, just below res_min_tiles = 2048: iconv1 stays with the one-tile kernel.  fwd16 960 x 2,
      bwd16 640 x 3, both even.  The weight gradients' last split is short in places (enc3b bf16: 30 tiles, 8 splits of 4, last 2).
  ("depth", 5, 256, 320)
      3200 full-resolution tiles = 3 rounds of 1024 + 128: k_conv3x3_res (iconv1, forward and input gradient, both dtypes) walks a
      short last round.  The fused kernels do NOT here: fwd16 800 x 4 and bwd16 640 x 5 divide evenly (their raggedness is the next
      shape's and one frame of 512x640's); enc1a in f32 takes the stride-2 resident kernel at exactly one round (800 tiles).  The
      raggedness claimed for this shape is the resident kernel's and it is there, so 5 stays.
  ("depth", 13, 256, 320), ("pose", 13, 256, 320)
      8320 tiles = 8 rounds + 128.  fwd16: ceil(8320 / 1024) = 9 tiles per workgroup, 925 workgroups, the last walks 4.  bwd16:
      ceil(8320 / 768) = 11, 757 workgroups, the last walks 4.  enc1b (bf16): 2080 tiles >= 2048, the resident kernel at 2 rounds + 32;
      enc1a (f32) the stride-2 one likewise; enc2a (bf16, 64-wide tiles: 84 KB of LDS, one workgroup per CU) walks its 520 tiles on 256
      workgroups, 2 rounds + 8.  Weight gradients of 2080 tiles in 64 splits of 33 leave ONE tile to the last split.
      PoseNet's conv2 has 520 tiles >= res_s2_min_tiles = 512: the stride-2 resident kernel, in bf16 one round of 520, in f32 (64 KB of
      LDS, two workgroups per CU) 512 workgroups and 8 tiles more; conv3 has 130 (one-tile kernel).  conv1's input gradient over the
      256x320 input (bf16) is the resident kernel at 8 rounds + 128.
  ("depth", 1, 512, 640), ("depth", 3, 512, 640), ("pose", 1, 512, 640)
      2560 and 7680 full-resolution tiles: 2.5 and 7.5 rounds of the resident kernel (iconv1); fwd16 at one frame 854 x 3 with the
      last workgroup walking 1 (three frames: 960 x 8, even; bwd16 640 x 4 and 768 x 10, even).  enc1a (f32) at three frames: 1920
      tiles on the 1024 workgroups of the stride-2 resident kernel, 1.875 rounds.  This is the set of forms small batches select at the large resolution, which
      tests/test_step_shapes_gpu.py records as different from configs[2]'s and which nothing held to a reference.

Asserted: X.check_layer (bit for bit), X.check_forms (one leaf per launch), per-layer claims that follow from tuning.h arithmetic
(_layer_claims), and the union of forms per shape and dtype as measured on the first run (FORMS; profiles/inference_shapes.md)."""
import gc
import time

import pytest
import torch

from tests import conv_exact as X
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float32)
SHAPES = X.SMALL_BATCH_SHAPES

# The forms each shape counts over all its layers and passes, per dtype, as measured on the first run with the production tuning
# (profiles/inference_shapes.md has the launch counts).  One to three frames of 256x320 run entirely on the small side of the table;
# the resident kernels come in at 5 frames (and at one frame of 512x640), the stride-2 one, k_conv_rt and the full grid floor at 13.
_D_BF16 = {"bwd16", "conv_ring", "conv_tile", "conv_up2_bn16", "dgrad_both", "dgrad_s2", "dgrad_s2_ring", "fwd16_head", "wgrad_halved_grid",
           "wgrad_store_clean", "wgrad_tail", "wgrad_teams", "wgrad_up2"}
_D_F32 = _D_BF16 - {"bwd16", "fwd16_head"}
_P_BF16 = {"conv_ring", "conv_tile", "dgrad_planes_mfma", "dgrad_s2", "dgrad_s2_ring", "wgrad_halved_grid", "wgrad_tail", "wgrad_teams"}
_P_F32 = {"conv_ring", "conv_tile", "dgrad_s2", "dgrad_s2_ring", "wgrad_halved_grid", "wgrad_store_clean", "wgrad_tail"}
_D_MID = {"bfloat16": _D_BF16 | {"conv_res", "dgrad_up2"}, "float32": _D_F32 | {"conv_res", "conv_res_s2", "dgrad_up2"}}
FORMS = {
    ("depth", 1, 256, 320): {"bfloat16": _D_BF16, "float32": _D_F32},
    ("depth", 3, 256, 320): {"bfloat16": _D_BF16, "float32": _D_F32},
    ("depth", 5, 256, 320): _D_MID,
    ("depth", 13, 256, 320): {"bfloat16": _D_BF16 | {"conv_res", "dgrad_up2", "conv_res_s2", "conv_bn64", "wgrad_full_grid"},
                              "float32": _D_F32 | {"conv_res", "dgrad_up2", "conv_res_s2", "conv_rt", "conv_rt_bn32", "wgrad_full_grid", "wgrad_mt4"}},
    ("depth", 1, 512, 640): _D_MID,
    ("depth", 3, 512, 640): _D_MID,
    ("pose", 1, 256, 320): {"bfloat16": _P_BF16 | {"wgrad_store_clean"}, "float32": _P_F32},
    ("pose", 3, 256, 320): {"bfloat16": _P_BF16, "float32": _P_F32},
    ("pose", 13, 256, 320): {"bfloat16": _P_BF16 | {"conv_res", "conv_res_s2"}, "float32": _P_F32 | {"conv_res_s2"}},
    ("pose", 1, 512, 640): {"bfloat16": _P_BF16 | {"conv_res", "wgrad_store_clean"}, "float32": _P_F32},
}

def _free():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _cdiv(a, b):
    return -(-a // b)


def _counted(forms, *names):
    return sum(f.get(n, 0) for f in forms.values() for n in names)


def _layer_claims(net, name, lay, dt, forms):
    """What the planner must pick for this layer at production tuning, each claim beside the arithmetic it follows from."""
    from coivo_amd import _lib
    what = f"{net} {name} {lay.__dict__} {dt}: {forms}"
    tune = lambda k: int(_lib.tune_get(k))
    bf = dt == torch.bfloat16
    G = 8 if bf else 4                                   # channels of a 16-byte granule; a chunk of the MFMA kernels is up to 4 of them
    wg = forms["wgrad"]
    # ---- the claims of tests/test_conv_exact_gpu.py that do not depend on the batch ----
    assert wg.get("wgrad_rt", 0) == 0, what
    if lay.up0 and not lay.C1:
        assert wg.get("wgrad_up2", 0) == X.wgrad_slices(lay, dt) == 1, what
    if lay.C0 == 16 and lay.Cout == 16 and not lay.up0 and lay.stride == 1:
        assert wg.get("wgrad_teams", 0) == 1, what
        if bf:
            assert forms["fwd16_head"].get("fwd16_head") == 1 and forms["bwd16"].get("bwd16") == 1, what
    if net == "pose" and name == "conv1" and bf:
        assert forms["dgrad_planes"].get("dgrad_planes_mfma") == 1, what
    assert _counted(forms, "wgrad_sliced") == 0, what                # no tensor here is near 1 GiB
    # ---- k_conv_rt: its grid is 16 x 16-pixel tiles x 32- or 64-wide channel tiles x images and must reach rt_min_wgs = 1024 (64-wide) or
    # rt_bn32_min_wgs = 2048.  The forward runs over the output map and Cout, an input gradient over the input map and C0 or C1, the
    # merged one of a concat layer over C0 + C1: the input map with the widest of these in 32-wide tiles bounds every pass's grid from
    # above.  (13 frames, f32: iconv2's merged input gradient has 13 * 80 * 2 = 2080 and is the one k_conv_rt launch of that sweep.)
    rt_bound = lay.B * _cdiv(lay.Hi, 16) * _cdiv(lay.Wi, 16) * _cdiv(max(lay.Cout, lay.C0 + lay.C1), 32)
    if rt_bound < min(tune("rt_min_wgs"), tune("rt_bn32_min_wgs")):
        assert _counted(forms, "conv_rt", "conv_rt_bn32") == 0, (rt_bound, what)
    # ---- the weights-resident kernels, forward pass.  plan_conv_t: one directly stored source of ONE chunk (C0 = ng * G, ng = 4, 2 or
    # 1: 32 / 16 / 8 channels in bf16, 16 / 8 / 4 in f32), stride 1 with Cout <= 32 from res_min_tiles = 2048 tiles on; stride 2
    # (res_s2_fits) with Cout >= 32 and ng of 2 or 4 from res_s2_min_tiles = 512 on.  Two-chunk layers are out; k_conv_rt and k_conv_q
    # want two chunks and k_conv_up2 an up-sampled source, so nothing is tried before it.  Tiles: 8 x 16 where the output map is a
    # multiple of that (the module's docstring); the claim is made for those maps only.
    if lay.Ho % 8 == 0 and lay.Wo % 16 == 0 and not lay.up0 and not lay.C1:
        tiles = lay.B * (lay.Ho // 8) * (lay.Wo // 16)
        ng = next((n for n in (4, 2, 1) if lay.C0 == n * G), 0)
        res = lay.stride == 1 and ng and lay.Cout <= 32 and tiles >= tune("res_min_tiles")
        res_s2 = lay.stride == 2 and ng in (2, 4) and lay.Cout >= 32 and tiles >= tune("res_s2_min_tiles")
        assert forms["fwd"].get("conv_res", 0) == (1 if res else 0), (tiles, ng, what)
        assert forms["fwd"].get("conv_res_s2", 0) == (1 if res_s2 else 0), (tiles, ng, what)
    if net == "depth" and name == "enc1b" and lay.B == 13 and (lay.Ho, lay.Wo) == (128, 160):
        # 13 * 160 = 2080 tiles >= 2048.  bf16: 32 channels are one chunk -- the resident kernel, two rounds of 1024 and 32 tiles more;
        # f32: two 16-channel chunks -- the one-tile kernel (k_conv_rt's 32-channel form would want 2048 of its 13 * 80 = 1040 tiles)
        assert forms["fwd"].get("conv_res", 0) == (1 if bf else 0) and forms["fwd"].get("conv_tile", 0) == (0 if bf else 1), what
    # ---- one frame of 256x320: no pass of any layer runs over more than 256x320 pixels = 640 tiles of 8 x 16 (pick_tile's cost grows with
    # the tile count: 173 units per 8 x 16 tile, at least 128 per tile of any shape, so never more than 640 * 173 / 128 = 865 tiles),
    # below res_min_tiles = 2048; the largest stride-2 output, 128x160, has 160 (at most 217), below res_s2_min_tiles = 512.
    if lay.B == 1 and lay.Hi * lay.Wi <= 256 * 320:
        assert _counted(forms, "conv_rt", "conv_rt_bn32", "conv_res", "conv_res_s2") == 0, what


def sweep(net, B, H, W):
    """Every layer x dtype of one shape; returns {dtype: {form: launches}} and checks the per-layer form claims."""
    from coivo_amd import _lib
    assert _lib.tune_get("wgrad_rt") == 0 and _lib.tune_get("quad_min_wgs") == 8192, "production tuning expected"
    assert _lib.tune_get("res_min_tiles") == 2048 and _lib.tune_get("res_s2_min_tiles") == 512 and _lib.tune_get("rt_min_wgs") == 1024 \
        and _lib.tune_get("fwd16_wgs") == 1024 and _lib.tune_get("bwd16_wgs") == 768, "production tuning expected"
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


def selected(total):
    return {str(dt)[6:]: {k for k, v in f.items() if v} for dt, f in total.items()}


@pytest.mark.parametrize("net,B,H,W", SHAPES)
def test_every_layer_bit_exact_at_the_inference_batch_size(net, B, H, W):
    _free()
    t0 = time.perf_counter()
    total = sweep(net, B, H, W)
    print(f"FORMS-TOTAL {net} B={B} {H}x{W}: " + "; ".join(f"{str(dt)[6:]} {sorted(f.items())}" for dt, f in total.items())
          + f"; {time.perf_counter() - t0:.1f} s")
    got = selected(total)
    assert got == FORMS.get((net, B, H, W)), {k: sorted(v) for k, v in got.items()}
    _free()


def test_a_dropped_last_tile_changes_the_exact_answer():
    """Sensitivity, in torch on the reference alone: enc1b's forward at 13 frames is 2080 tiles, two rounds of the resident kernel's 1024
    workgroups and 32 more.  Zero the last 8 x 16-pixel tile of the last image -- what a walk that drops its short last round would
    leave in a cleared buffer -- and torch.equal fails; so does it for ANY other content of that tile, since the bar is equality."""
    lay = dict(X.layers("depth", 13, 256, 320))["enc1b"]
    assert 13 * (lay.Ho // 8) * (lay.Wo // 16) == 2080 == 2 * 1024 + 32
    g = torch.Generator(device=dev()).manual_seed(13)
    data = X.make_data(lay, g, dev())
    ref = lay.ref_fwd(data["x0"], None, data["w"], data["bias"], 0, lay.B)
    got = ref.clone()
    got[lay.B - 1, lay.Ho - 8:, lay.Wo - 16:] = 0
    assert not torch.equal(got.float(), ref.float())
    n = int((got != ref).sum())
    print(f"SENSITIVITY enc1b 13x128x160 forward: {n} of {8 * 16 * lay.Cout} elements of the last tile are non-zero in the reference")
    assert n > 8 * 16 * lay.Cout // 8           # ReLU outputs of a zero-mean pre-activation: about half are positive


def test_what_the_inference_batch_sizes_add_to_the_production_sweep():
    """No single form is new: the union over the shapes here lies inside tests/test_conv_exact_gpu.py's PRODUCTION_FORMS (without
    conv_up2_bn32 and wgrad_sliced, which need large grids and 1 GiB tensors).  New are the walks (the module's docstring) and the
    COMBINATIONS: every training-step set pinned in tests/test_step_shapes_gpu.py holds conv_rt, wgrad_full_grid and wgrad_mt4, while one
    to five frames run a whole network without any of them -- every weight gradient on the halved grid floor, every multi-chunk layer on
    the one-tile kernel -- and from five frames on (one at 512x640) with the resident kernel beside that."""
    from tests.test_conv_exact_gpu import PRODUCTION_FORMS
    from tests.test_step_shapes_gpu import FORMS as STEP_FORMS
    union = set().union(*(s for v in FORMS.values() for s in v.values()))
    assert union == PRODUCTION_FORMS - {"conv_up2_bn32", "wgrad_sliced"}, sorted(union ^ PRODUCTION_FORMS)
    large_side = {"conv_rt", "wgrad_full_grid", "wgrad_mt4"}
    assert all(large_side <= s for s in STEP_FORMS.values())
    small = [k for k, v in FORMS.items() if not any(large_side & s for s in v.values())]
    assert {("depth", 1, 256, 320), ("depth", 3, 256, 320), ("depth", 5, 256, 320), ("depth", 1, 512, 640), ("depth", 3, 512, 640)} <= set(small)
    assert all("conv_res" in FORMS["depth", 5, 256, 320][dt] and "conv_res" in FORMS["depth", 1, 512, 640][dt] for dt in ("bfloat16", "float32"))
