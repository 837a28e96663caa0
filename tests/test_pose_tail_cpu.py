"""The planner of PoseNet's whole-K resident launches (csrc/pose_tail.hip, include/colvo.h colvo_pose_tail_plan), without a GPU:
conv5-conv7 are selected in both directions at small batches, refused everywhere else, and the query moves no counter."""
import pytest
import torch

from coivo_amd import _lib, build, ops


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.ensure()
    return _lib.load()


CH = (128, 256, 256, 256)


def _descs(dtype, B, H, W):
    """conv5, conv6, conv7 behind B pairs of H x W frames (conv4's output map is H/16 x W/16)."""
    out, h, w = [], H // 16, W // 16
    for i in range(3):
        out.append(ops.conv_desc(dtype, B, h, w, CH[i], CH[i + 1], stride=2))
        h, w = out[-1].Ho, out[-1].Wo
    return out


def test_selected_in_both_directions_at_the_benchmark_shape():
    """8 pairs of 256x320: every layer one round of workgroups of 16 channels x whole images, operands within 160 KB of LDS; conv7's
    input gradient (5-wide input, not 2 x 3) keeps the conv order over the zero-dilated dy, conv6's and conv5's take k_dgrad_s2's."""
    kinds = []
    for d in _descs(torch.bfloat16, 8, 256, 320):
        for direction in (0, 1):
            plan = ops.pose_tail_plan(d, direction)
            assert plan is not None, (d.Hi, d.Wi, direction)
            nwg, images, lds, kind = plan
            n = d.Cout if direction == 0 else d.C0
            assert images >= 1 and nwg == -(-8 // images) * (n // 16) and nwg <= 256
            assert 0 < lds <= 160 * 1024
            kinds.append(kind)
    assert kinds == [0, 1, 0, 1, 0, 0]


@pytest.mark.parametrize("B,H,W", [(1, 32, 32), (2, 64, 96), (3, 96, 160), (16, 256, 320), (24, 256, 320)])
def test_selected_at_other_small_batches(B, H, W):
    for d in _descs(torch.bfloat16, B, H, W):
        for direction in (0, 1):
            plan = ops.pose_tail_plan(d, direction)
            assert plan is not None and 0 < plan[2] <= 160 * 1024


def test_refusals():
    for d in _descs(torch.float32, 8, 256, 320):
        assert ops.pose_tail_plan(d) is None and ops.pose_tail_plan(d, 1) is None                   # f32
    ceiling = int(_lib.tune_get("pose_tail_max_pairs"))
    for B in (ceiling + 1, 32, 64):                                                                   # above the ceiling; configs[3]
        for d in _descs(torch.bfloat16, B, 256, 320):
            assert ops.pose_tail_plan(d) is None and ops.pose_tail_plan(d, 1) is None, B
    d = _descs(torch.bfloat16, 8, 256, 320)[0]
    assert ops.pose_tail_plan(d, 2) is None
    assert ops.pose_tail_plan(ops.conv_desc(torch.bfloat16, 8, 16, 20, 128, 256, stride=1)) is None  # not stride 2
    assert ops.pose_tail_plan(ops.conv_desc(torch.bfloat16, 8, 32, 40, 64, 128, stride=2)) is None   # conv4: K = 64
    assert ops.pose_tail_plan(ops.conv_desc(torch.bfloat16, 8, 64, 80, 128, 256, stride=2)) is None  # the map does not fit in LDS


def test_tuning_entries_switch_it_off():
    descs = _descs(torch.bfloat16, 8, 256, 320)
    assert _lib.tune_get("pose_tail") == 1 and _lib.tune_get("pose_tail_bwd") == 1
    try:
        _lib.tune_set("pose_tail_bwd", 0)       # its own switch: the forward form stays
        for d in descs:
            assert ops.pose_tail_plan(d) is not None and ops.pose_tail_plan(d, 1) is None
        _lib.tune_set("pose_tail_bwd", 1)
        _lib.tune_set("pose_tail", 0)
        for d in descs:
            assert ops.pose_tail_plan(d) is None and ops.pose_tail_plan(d, 1) is None
        _lib.tune_set("pose_tail", 1)
        _lib.tune_set("pose_tail_max_pairs", 4)
        for d in descs:
            assert ops.pose_tail_plan(d) is None and ops.pose_tail_plan(d, 1) is None
    finally:                                    # the tests share one process: later ones must see the library's defaults
        _lib.tune_set("pose_tail", 1)
        _lib.tune_set("pose_tail_bwd", 1)
        _lib.tune_set("pose_tail_max_pairs", 24)
    assert all(ops.pose_tail_plan(d) is not None for d in descs)


def test_forced_images_per_workgroup_fill_fragments_across_images():
    """conv7 at 8 pairs has 48 pixels: eight images in one workgroup are three fragments, not 8 x 1."""
    d = _descs(torch.bfloat16, 8, 256, 320)[2]
    try:
        _lib.tune_set("pose_tail_images", 8)
        assert ops.pose_tail_plan(d)[:2] == (16, 8) and ops.pose_tail_plan(d)[2] <= 160 * 1024
        _lib.tune_set("pose_tail_images", 3)
        assert ops.pose_tail_plan(d)[:2] == (3 * 16, 3)
        d5 = _descs(torch.bfloat16, 8, 256, 320)[0]
        assert ops.pose_tail_plan(d5) is None   # three 16 x 20 x 128 maps do not fit beside the slab: refused, not clipped
    finally:
        _lib.tune_set("pose_tail_images", 0)


def test_queries_count_no_form():
    before = _lib.form_counts()
    for B, H, W in ((8, 256, 320), (1, 32, 32), (16, 256, 320), (64, 256, 320), (32, 512, 640)):
        for dt in (torch.bfloat16, torch.float32):
            for d in _descs(dt, B, H, W):
                for direction in (0, 1):
                    ops.pose_tail_plan(d, direction)
    assert _lib.form_counts() == before
    assert len(before) == 27


def test_kernel_closes_its_mfma_chains_with_the_guard(tmp_path):
    """The emitted ISA of csrc/pose_tail.hip, as tests/test_isa_cpu.py holds the other MFMA files to it: no rotated MFMA result is
    read early, accumulators live in VGPRs, every instantiation carries the in-place terminator of mfma_result_guard, and no scratch."""
    import os
    import re
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import isa_check_mfma
    asm = build.emit_asm("pose_tail.hip", str(tmp_path / "pose_tail.s"))
    nmfma, _, bad = isa_check_mfma.check(asm, 16, 12)
    assert nmfma >= 2 * (36 + 72), nmfma        # the (chunk, tap) products of the four instantiations
    assert not bad, bad[:5]
    text = open(asm).read()
    assert "v_accvgpr" not in text and " a[" not in text
    kernels = [k for k in re.split(r"\n(?=_Z\S+:)", text) if k.startswith("_Z") and "v_mfma" in k]
    assert len(kernels) == 4 and all("k_conv_wholek" in k.split(":")[0] for k in kernels)
    for k in kernels:
        assert len(re.findall(r";;#ASMSTART\s+s_nop 1\s+v_mfma\S+ (v\[\d+:\d+\]), (\S+), \2, \1", k)) == 1, k.split(":")[0]
        assert "scratch_" not in k, k.split(":")[0]
