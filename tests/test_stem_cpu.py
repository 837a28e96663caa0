"""The planner of DepthNet's fused stem (csrc/stem.hip, include/colvo.h colvo_stem_plan) and its command, without a GPU: the benchmark
shape is selected, everything the kernel is not built for is refused, the query moves no counter, and the recorded command is the stem
form of CMD_PACK_STEM_POSE in the slot layout the decoder reads.  (A whole DepthNet pass cannot be recorded without a GPU -- the
weights are packed by a kernel --: tests/test_stem_gpu.py reads the recorded forward pass of a real network.)"""
import pytest
import torch

from coivo_amd import _lib, build, ops, program


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.ensure()
    return _lib.load()


def _enc1a(dtype, pairs, H, W, cin=8, cout=32, stride=2):
    return ops.conv_desc(dtype, 2 * pairs, H, W, cin, cout, stride=stride)


def test_selected_at_the_benchmark_shape():
    """8 pairs of 256 x 320: enc1b's 128 x 160 map in 128-pixel tiles, 160 a frame; the 1280 pair tiles are walked by one workgroup per
    resident slot, three to a CU."""
    plan = ops.stem_plan(_enc1a(torch.bfloat16, 8, 256, 320))
    assert plan is not None
    nwg, toh, tow, lds = plan
    assert toh * tow == 128 and 128 % toh == 0 and 160 % tow == 0
    items = 8 * (128 // toh) * (160 // tow)
    slots = int(_lib.tune_get("stem_max_wgs"))
    assert slots == 768 and 3 * lds <= 160 * 1024
    assert items == 1280 and nwg == min(items, slots)
    assert (2 * toh + 5) * (2 * tow + 5) <= 4 * 256                      # the frame patch fits the register prefetch


@pytest.mark.parametrize("pairs,H,W", [(1, 16, 16), (2, 32, 48), (3, 36, 52), (2, 64, 96), (64, 256, 320), (32, 512, 640)])
def test_selected_at_other_shapes(pairs, H, W):
    plan = ops.stem_plan(_enc1a(torch.bfloat16, pairs, H, W))
    assert plan is not None and 0 < plan[3] <= 160 * 1024 and 1 <= plan[0] <= 768


def test_refusals():
    bf = torch.bfloat16
    assert ops.stem_plan(_enc1a(torch.float32, 8, 256, 320)) is None                       # f32
    assert ops.stem_plan(_enc1a(bf, 8, 256, 320, cout=16)) is None                          # PoseNet's conv1: 8 -> 16
    assert ops.stem_plan(_enc1a(bf, 8, 256, 320, cout=64)) is None
    assert ops.stem_plan(_enc1a(bf, 8, 256, 320, cin=32)) is None                           # enc2a-like: 32 -> 32 at stride 2
    assert ops.stem_plan(_enc1a(bf, 8, 256, 320, stride=1)) is None
    assert ops.stem_plan(ops.conv_desc(bf, 15, 256, 320, 8, 32, stride=2)) is None          # an odd image count is no pair batch
    for H, W in ((8, 8), (8, 64), (64, 8), (14, 16)):                                       # too small
        assert ops.stem_plan(_enc1a(bf, 2, H, W)) is None, (H, W)
    assert ops.stem_plan(_enc1a(bf, 2, 33, 48)) is None                                     # odd extent
    assert ops.stem_plan(_enc1a(bf, 512, 512, 640)) is None                                 # tensors of 1 GiB and more


def test_tuning_entries():
    d = _enc1a(torch.bfloat16, 8, 256, 320)
    assert _lib.tune_get("stem_fused") in (0, 1)
    saved = {k: _lib.tune_get(k) for k in ("stem_fused", "stem_max_pairs", "stem_max_wgs")}
    try:
        _lib.tune_set("stem_fused", 1)
        assert ops.stem_plan(d) is not None
        _lib.tune_set("stem_max_pairs", 7)
        assert ops.stem_plan(d) is None and ops.stem_plan(_enc1a(torch.bfloat16, 7, 256, 320)) is not None
        _lib.tune_set("stem_max_pairs", saved["stem_max_pairs"])
        _lib.tune_set("stem_max_wgs", 3)                                  # what the GPU tests use to walk several rounds
        assert ops.stem_plan(_enc1a(torch.bfloat16, 2, 32, 48))[0] <= 3
        _lib.tune_set("stem_fused", 0)
        assert ops.stem_plan(d) is None
    finally:                                                              # the tests share one process
        for k, v in saved.items():
            _lib.tune_set(k, v)


def test_queries_count_no_form():
    before = _lib.form_counts()
    for pairs, H, W in ((8, 256, 320), (1, 16, 16), (3, 36, 52), (64, 256, 320), (32, 512, 640)):
        for dt in (torch.bfloat16, torch.float32):
            ops.stem_plan(_enc1a(dt, pairs, H, W))
    assert _lib.form_counts() == before
    assert len(before) == 27                                              # no new form counter


def test_the_recorded_command_is_the_stem_form(monkeypatch):
    """ops.stem_fused records ONE command: CMD_PACK_STEM_POSE with enc1a's descriptor, the nine pointers in the order program.hip's
    decoder reads (p[3] != NULL selects csrc/stem.hip) and i = frames, H, W -- where pack_stem_pose and two conv_fwd record three."""
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)             # (recording only takes addresses)
    pairs, H, W = 2, 32, 48
    d = _enc1a(torch.bfloat16, pairs, H, W)
    db = ops.conv_desc(torch.bfloat16, 2 * pairs, d.Ho, d.Wo, 32, 32)
    bf = torch.bfloat16
    frames = torch.zeros(2 * pairs, 3, H, W)
    stem, pose_in = torch.zeros(2 * pairs, H, W, 8, dtype=bf), torch.zeros(pairs, H, W, 8, dtype=bf)
    w1, b1, y1 = torch.zeros(32, 9, 8, dtype=bf), torch.zeros(32), torch.zeros(2 * pairs, d.Ho, d.Wo, 32, dtype=bf)
    w2, b2, y2 = torch.zeros(32, 9, 32, dtype=bf), torch.zeros(32), torch.zeros(2 * pairs, d.Ho, d.Wo, 32, dtype=bf)
    with program.Program() as fused:
        fused.external("img", frames)
        ops.stem_fused(d, frames, stem, pose_in, w1, b1, y1, w2, b2, y2)
    with program.Program() as plain:
        plain.external("img", frames)
        ops.pack_stem_pose(frames, stem, pose_in)
        ops.conv_fwd(d, stem, None, w1, b1, y1)
        ops.conv_fwd(db, y1, None, w2, b2, y2)
    assert len(fused) == 1 and len(plain) == 3
    c = fused._arr[0]
    assert c.op == _lib.CMD_PACK_STEM_POSE and c.stream == 0
    assert [c.p[k] for k in range(9)] == [t.data_ptr() for t in (frames, stem, pose_in, w1, b1, y1, w2, b2, y2)]
    assert not any(c.p[k] for k in range(9, _lib.NPTR))
    assert list(c.i)[:3] == [2 * pairs, H, W]
    assert (c.desc.B, c.desc.Hi, c.desc.Wi, c.desc.C0, c.desc.Cout, c.desc.stride) == (2 * pairs, H, W, 8, 32, 2)
    assert fused._slots["img"] == [(0, 0)]                                # the frames stay a per-call pointer
    assert [plain._arr[k].op for k in range(3)] == [_lib.CMD_PACK_STEM_POSE, _lib.CMD_CONV_FWD, _lib.CMD_CONV_FWD]
    assert not plain._arr[0].p[3]                                         # the plain form of the same command


def test_kernel_closes_its_mfma_chains_with_the_guard(tmp_path):
    """The emitted ISA of csrc/stem.hip, as tests/test_isa_cpu.py holds the other MFMA files to it: no rotated MFMA result is read
    early, accumulators live in VGPRs, both chains carry the in-place terminator of mfma_result_guard, and no scratch."""
    import os
    import re
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import isa_check_mfma
    asm = build.emit_asm("stem.hip", str(tmp_path / "stem.s"))
    nmfma, _, bad = isa_check_mfma.check(asm, 16, 12)
    assert nmfma >= 6 + 36, nmfma                # enc1a: 3 k-groups x 2 channel tiles; enc1b: 9 taps x 2 x 2
    assert not bad, bad[:5]
    text = open(asm).read()
    assert "v_accvgpr" not in text and " a[" not in text
    kernels = [k for k in re.split(r"\n(?=_Z\S+:)", text) if k.startswith("_Z") and "v_mfma" in k]
    assert len(kernels) == 1 and "k_stem" in kernels[0].split(":")[0]
    assert len(re.findall(r";;#ASMSTART\s+s_nop 1\s+v_mfma\S+ (v\[\d+:\d+\]), (\S+), \2, \1", kernels[0])) == 2
    assert "scratch_" not in kernels[0]
