"""The analytic bounds of tests/head_exact.py at every production shape, and proof that each comparison of
tests/test_heads_exact_gpu.py catches a small mistake: a reference with one 64-column tile's halo tap dropped, with one pixel range
left out of the weight gradient, with one pose_in pair swapped -- each must fail its check.  No GPU, no kernel."""
import pytest
import torch

from tests import conv_exact as CX
from tests import head_exact as HX

DEPTH_SHAPES = [(16, 256, 320), (64, 256, 320), (128, 256, 320), (64, 512, 640), (128, 512, 640)]


@pytest.mark.parametrize("B,H,W", DEPTH_SHAPES)
def test_head_bounds_stay_exact_at_every_production_shape(B, H, W):
    npix = B * H * W
    assert HX.bound_pre(HX.Y_FWD) <= CX.BOUND and HX.bound_pre(HX.Y_FWD, 8) <= CX.BOUND
    assert HX.Y_FWD * HX.QY == float(torch.tensor(HX.Y_FWD * HX.QY).bfloat16())        # the largest y is a bf16 value
    assert HX.head_g_bound() <= 255                                                   # g: at most 8 significant bits -> exact in bf16
    assert CX.bound_wgrad(npix) <= CX.BOUND                                           # the head's weight gradient (X_MAX, DY_MAX)
    assert HX.bound_head_g_wgrad(npix) <= CX.BOUND                                    # the layer's weight gradient in the HEAD form
    # d(pre) stays dense enough that every pixel range of the VALU weight gradient (at most 16384 pixels) holds non-zeros
    assert CX.dy_density(npix) * 2048 >= 10


def test_rounding_bounds_are_small_where_the_math_is_well_conditioned():
    pre = torch.tensor([-30.0, -8.0, -1.0, 0.0, 1.0, 8.0, 30.0], dtype=torch.float64)
    rel = HX.depth_rel_bound(pre)
    assert float(rel.max()) <= 12 * HX.U * (1 + 1e-4)
    g = torch.ones_like(pre)
    b = HX.dpre_bound(pre, g) / HX.ref_dpre(pre, g).abs()
    assert float(b[2:5].max()) < 128 * HX.U                      # mid-range: the rebuilt sigmoid and the depth squared, ~65 U
    assert float(b[0]) > 1e3 * HX.U and float(b[-1]) > 1e3 * HX.U  # saturated: the rebuilt sigmoid's amplification is in the bound


def _depth_from(y, w, b):
    return HX.ref_depth(HX.ref_pre(y, w, b)).float()


def test_a_dropped_halo_tap_at_a_tile_seam_fails_the_depth_check():
    """Two 64-column tiles; the mutant loses the tap that reaches across the seam (column 63 seen from column 64)."""
    g = torch.Generator().manual_seed(1)
    B, H, W = 1, 8, 128
    y = HX.make_y((B, H, W, 16), HX.Y_FWD, g, "cpu")
    w, b = HX.make_head_w(16, g, "cpu"), HX.make_head_b(g, "cpu")
    pre = HX.ref_pre(y, w, b)
    ref = HX.ref_depth(pre)
    bound = HX.depth_rel_bound(pre) * ref
    HX.expect_within(_depth_from(y, w, b), ref, bound, "correct")
    ym = y.clone()
    ym[:, :, 63] = 0                                           # the left halo of tile 1 ...
    got = _depth_from(ym, w, b)
    got[:, :, :63] = _depth_from(y, w, b)[:, :, :63]            # ... seen only from tile 1 (column 64): the left tile keeps its own
    got[:, :, 65:] = _depth_from(y, w, b)[:, :, 65:]
    with pytest.raises(AssertionError):
        HX.expect_within(got, ref, bound, "dropped halo tap")


def test_a_dropped_pixel_range_fails_the_weight_gradient_check():
    """One 2048-pixel range of one image left out of the head's weight gradient."""
    g = torch.Generator().manual_seed(2)
    B, H, W = 2, 16, 320
    y = HX.make_y((B, H, W, 16), CX.X_MAX, g, "cpu")
    dpre = CX.make_dy((B, H, W), CX.dy_density(B * H * W), g, "cpu")
    rdw, rdb = HX.ref_head_wgrad(y, dpre)
    CX.expect_exact(rdw.float(), rdw, HX.QY * CX.QDY, "correct")
    dm = dpre.clone().view(B, H * W)
    dm[1, 2048:4096] = 0
    mdw, mdb = HX.ref_head_wgrad(y, dm.view(B, H, W))
    with pytest.raises(AssertionError):
        CX.expect_exact(mdw.float(), rdw, HX.QY * CX.QDY, "dropped pixel range")
    with pytest.raises(AssertionError):
        CX.expect_exact(mdb.float(), rdb, CX.QDY, "dropped pixel range (bias)")


def test_a_swapped_pose_in_pair_fails_the_pose_in_check():
    g = torch.Generator().manual_seed(3)
    Bh, H, W = 3, 4, 5
    frames = torch.rand(2 * Bh, 3, H, W, generator=g)
    depth = 0.1 + 9.9 * torch.rand(2 * Bh, 1, H, W, generator=g)
    pose_in = torch.cat([frames[:Bh].permute(0, 2, 3, 1), frames[Bh:].permute(0, 2, 3, 1), depth[:Bh].permute(0, 2, 3, 1),
                         depth[Bh:].permute(0, 2, 3, 1)], dim=3).bfloat16()
    HX.check_pose_in(pose_in, frames, depth)
    swapped = pose_in.clone()
    swapped[0, ..., 6:8], swapped[1, ..., 6:8] = pose_in[1, ..., 6:8], pose_in[0, ..., 6:8]
    with pytest.raises(AssertionError):
        HX.check_pose_in(swapped, frames, depth)
    late = pose_in.clone()
    late[2, ..., 7] = pose_in[2, ..., 6]                      # the target's depth in the reference channel
    with pytest.raises(AssertionError):
        HX.check_pose_in(late, frames, depth)


def test_the_pose_bounds_on_exact_data():
    """On the CPU the float64 pose reference of integer data, evaluated in fp32 the kernel's way, stays within the derived bound."""
    g = torch.Generator().manual_seed(4)
    B, H, W, C = 4, 2, 3, 256
    x = CX.make_source((B, H, W, C), g, "cpu")
    w = CX._ints(-CX.W_MAX, CX.W_MAX, (8, 1, C), g, "cpu") * CX.QW
    b = CX.make_bias(8, g, "cpu")
    ref, bnd = HX.pose_ref(x, w, b)
    S = (x.sum(dim=(1, 2)) @ w.view(8, C).t())                       # exact in fp32 on this data
    s = torch.tensor([HX.POSE_S] * 6 + [HX.LCC_S] * 2)
    o = s * (b + S / float(H * W))
    o[:, 6] += 1.0
    HX.expect_within(o, ref, bnd, "fp32 evaluation")
