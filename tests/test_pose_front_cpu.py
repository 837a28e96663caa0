"""The planner of PoseNet's front chain (csrc/pose_front.hip, include/colvo.h colvo_pose_front_plan), without a GPU: the chain is
selected exactly where every one of conv1-conv3 would otherwise be a one-tile launch -- its bits are that form's bits -- and the
query moves no counter."""
import pytest
import torch

from coivo_amd import _lib, build, ops


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.ensure()
    return _lib.load()


def _d1(dtype, B, H, W):
    return ops.conv_desc(dtype, B, H, W, 8, 16, stride=2)


@pytest.mark.parametrize("B,H,W", [(8, 256, 320), (1, 32, 32)])
def test_selected_for_bf16_at_small_batches(B, H, W):
    plan = ops.pose_front_plan(_d1(torch.bfloat16, B, H, W))
    assert plan is not None
    nwg, toh, tow, lds = plan
    assert toh == 4 and tow in (8, 10) and 0 < lds <= 160 * 1024
    assert nwg == B * -(-(H // 8) // toh) * -(-(W // 8) // tow)


def test_the_benchmark_shape_runs_one_round_of_workgroups():
    """8 pairs of 256x320: conv3's 32x40 map in 4 x 10 tiles is 256 workgroups, one per CU (4 x 8 tiles would be 320)."""
    assert ops.pose_front_plan(_d1(torch.bfloat16, 8, 256, 320))[:3] == (256, 4, 10)
    assert ops.pose_front_plan(_d1(torch.bfloat16, 1, 32, 32))[:3] == (1, 4, 8)


@pytest.mark.parametrize("dtype,B,H,W,why", [
    (torch.float32, 8, 256, 320, "f32"),
    (torch.bfloat16, 2, 36, 44, "H, W not multiples of 8"),
    (torch.bfloat16, 2, 64, 36, "W not a multiple of 8"),
    (torch.bfloat16, 13, 256, 320, "conv2 goes to the stride-2 resident kernel from res_s2_min_tiles on"),
    (torch.bfloat16, 64, 256, 320, "configs[3]"),
    (torch.bfloat16, 32, 512, 640, "configs[2]"),
])
def test_not_selected(dtype, B, H, W, why):
    for direction in (0, 1):
        assert ops.pose_front_plan(_d1(dtype, B, H, W), direction) is None, (why, direction)


def test_other_layers_are_not_the_chain():
    d = ops.conv_desc(torch.bfloat16, 8, 256, 320, 16, 32, stride=2)
    assert ops.pose_front_plan(d) is None
    d = ops.conv_desc(torch.bfloat16, 8, 256, 320, 8, 16, stride=1)
    assert ops.pose_front_plan(d) is None
    d = ops.conv_desc(torch.bfloat16, 8, 256, 320, 8, 16, stride=2, relu=False)
    assert ops.pose_front_plan(d) is None


@pytest.mark.parametrize("B,H,W", [(8, 256, 320), (1, 32, 32)])
def test_the_input_gradient_chain_is_selected_with_the_forward_chain(B, H, W):
    fwd, bwd = ops.pose_front_plan(_d1(torch.bfloat16, B, H, W)), ops.pose_front_plan(_d1(torch.bfloat16, B, H, W), direction=1)
    assert bwd is not None and bwd[:3] == fwd[:3] and 0 < bwd[3] <= 160 * 1024
    try:
        _lib.tune_set("pose_front_bwd", 0)      # its own switch: the forward chain stays
        assert ops.pose_front_plan(_d1(torch.bfloat16, B, H, W), direction=1) is None
        assert ops.pose_front_plan(_d1(torch.bfloat16, B, H, W)) == fwd
    finally:
        _lib.tune_set("pose_front_bwd", 1)
    assert ops.pose_front_plan(_d1(torch.bfloat16, B, H, W), direction=2) is None


def test_queries_count_no_form():
    before = _lib.form_counts()
    for B, H, W in ((8, 256, 320), (1, 32, 32), (13, 256, 320), (64, 256, 320), (32, 512, 640), (2, 36, 44)):
        for dt in (torch.bfloat16, torch.float32):
            for direction in (0, 1):
                ops.pose_front_plan(_d1(dt, B, H, W), direction)
    assert _lib.form_counts() == before
    assert len(before) == 27


def test_chain_kernel_closes_its_mfma_chains_with_the_guard(tmp_path):
    """The emitted ISA of csrc/pose_front.hip, as tests/test_isa_cpu.py holds the other MFMA files to it: no rotated MFMA result is
    read early, accumulators live in VGPRs, and the kernel carries the in-place terminator of mfma_result_guard."""
    import os
    import re
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import isa_check_mfma
    asm = build.emit_asm("pose_front.hip", str(tmp_path / "pose_front.s"))
    nmfma, _, bad = isa_check_mfma.check(asm, 16, 12)
    assert nmfma >= (3 + 5 + 9) + (18 + 9 + 6), nmfma           # the k-groups of the three forward and three backward levels
    assert not bad, bad[:5]
    text = open(asm).read()
    assert "v_accvgpr" not in text and " a[" not in text
    kernels = [k for k in re.split(r"\n(?=_Z\S+:)", text) if k.startswith("_Z") and "v_mfma" in k]
    assert sorted(re.search(r"k_pose_front_(fwd|bwd)", k.split(":")[0]).group(1) for k in kernels) == ["bwd", "fwd"]
    for k in kernels:
        assert len(re.findall(r";;#ASMSTART\s+s_nop 1\s+v_mfma\S+ (v\[\d+:\d+\]), (\S+), \2, \1", k)) == 3, k.split(":")[0]
        assert "scratch_" not in k, k.split(":")[0]


def test_switched_off_it_is_never_selected():
    assert _lib.tune_get("pose_front") == 1
    try:
        _lib.tune_set("pose_front", 0)
        for B, H, W in ((8, 256, 320), (1, 32, 32), (2, 64, 96), (3, 96, 160)):
            for direction in (0, 1):
                assert ops.pose_front_plan(_d1(torch.bfloat16, B, H, W), direction) is None
    finally:
        _lib.tune_set("pose_front", 1)          # the tests share one process: later ones must see the library's default
    assert ops.pose_front_plan(_d1(torch.bfloat16, 8, 256, 320)) is not None
