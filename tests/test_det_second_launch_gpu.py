"""-m gpu: the two forms of the deterministic step's slab reduction and PoseNet head backward give the same bits.

tuning.h `wgrad_reduce_staged` chooses between k_wgrad_reduce (eight slab loads at a time) and k_wgrad_reduce_staged (every split's
load in flight, values parked in LDS, added in split order); `pose_head_det_parallel` between k_pose_head_bwd_det (one thread per
channel walks every image and pixel) and k_pose_head_bwd_det_par (threads over (image, channel) pairs).  Both switches promise
bitwise equality, so every comparison here is torch.equal on pre-filled (non-zero) destinations.
"""
import pytest
import torch

from tests import guarded
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

_guarded = guarded.fixture(dev)          # every test here allocates from tests/guarded.py's pool; the guards are checked at its end


class _tuned:
    """Set tuning entries for a block and put the former values back."""

    def __init__(self, **entries):
        self.entries = entries

    def __enter__(self):
        from coivo_amd import _lib
        self.saved = {k: _lib.tune_get(k) for k in self.entries}
        for k, v in self.entries.items():
            _lib.tune_set(k, v)

    def __exit__(self, *exc):
        from coivo_amd import _lib
        for k, v in self.saved.items():
            _lib.tune_set(k, v)


# (B, H, W, Cin, Cout, stride, up0) -> pixel-range splits the planner gives it in bf16.  In f32 a chunk is 16 channels instead of 32
# and the planner gives the two 64-channel layers fewer splits (F32_SPLITS); the slabs are fp32 either way.
REDUCE_CASES = [
    ((1, 16, 16, 16, 16, 1, False), 2),
    ((1, 32, 48, 16, 16, 2, False), 3),
    ((3, 32, 48, 8, 16, 2, False), 9),
    ((1, 32, 48, 16, 16, 1, False), 12),
    ((3, 64, 96, 64, 64, 1, False), 29),
    ((3, 96, 160, 64, 32, 1, True), 45),
    ((5, 96, 160, 32, 32, 2, False), 75),
    ((5, 96, 160, 16, 16, 2, False), 150),
]


F32_SPLITS = {29: 18, 45: 30}


def _reduce_both_forms(desc_args, nsplit, dtype, chunk=None, db_offset=0):
    from coivo_amd import ops
    B, H, W, Cin, Cout, stride, up0 = desc_args
    d = dev()
    desc = ops.conv_desc(dtype, B, H, W, Cin, Cout, stride=stride, up0=up0)
    if dtype == torch.float32:
        nsplit = F32_SPLITS.get(nsplit, nsplit)
    assert ops.conv_wgrad_splits(desc) == nsplit
    g = torch.Generator().manual_seed(1000 * nsplit + Cin)
    hs, ws = (H // 2, W // 2) if up0 else (H, W)
    x0 = torch.randn(B, hs, ws, Cin, generator=g).to(d).to(dtype)
    dy = torch.randn(B, desc.Ho, desc.Wo, Cout, generator=g).to(d).to(dtype)
    dw0 = (torch.randn(Cout, 9, Cin, generator=g) + 3.0).to(d)
    db0 = (torch.randn(Cout + db_offset, generator=g) + 3.0).to(d)
    scr = ops.conv_wgrad_scratch(desc, d)
    out = []
    for staged in (0, 1):
        entries = {"wgrad_reduce_staged": staged, "wgrad_reduce_staged_min": 1}      # the staged form for the few-split layers too
        if chunk is not None:
            entries["wgrad_reduce_chunk"] = chunk
        dw, dbf = dw0.clone(), db0.clone()
        with _tuned(**entries):
            ops.conv_wgrad(desc, x0, None, dy, dw, dbf[db_offset:], scr)
            torch.cuda.synchronize()
        out.append((dw, dbf))
    (dw_a, db_a), (dw_b, db_b) = out
    assert not torch.equal(dw_a, dw0) and not torch.equal(db_a, db0)        # something was added
    assert torch.equal(dw_a, dw_b), "dw: staged form differs from k_wgrad_reduce"
    assert torch.equal(db_a, db_b), "db: staged form differs from k_wgrad_reduce"
    if db_offset:
        assert torch.equal(db_b[:db_offset], db0[:db_offset])                # nothing written in front of the bias


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", REDUCE_CASES, ids=[f"nsplit{n}" for _, n in REDUCE_CASES])
def test_staged_slab_reduction_has_the_bits_of_the_eight_at_a_time_form(case, dtype):
    _reduce_both_forms(case[0], case[1], dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", [REDUCE_CASES[4], REDUCE_CASES[7]], ids=["nsplit29", "nsplit150"])
def test_staged_slab_reduction_in_chunks_of_eight_splits(case, dtype):
    """wgrad_reduce_chunk = 8: 4 (f32: 3) and 19 chunks, the last one short; the sum is carried from chunk to chunk in split order."""
    _reduce_both_forms(case[0], case[1], dtype, chunk=8)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_staged_slab_reduction_of_a_bias_that_is_not_16_byte_aligned(dtype):
    """db one float behind a 16-byte boundary: the bias part takes single floats instead of 16-byte vectors (the weights keep them)."""
    _reduce_both_forms(REDUCE_CASES[3][0], REDUCE_CASES[3][1], dtype, db_offset=1)
    _reduce_both_forms(REDUCE_CASES[4][0], REDUCE_CASES[4][1], dtype, chunk=8, db_offset=1)


# which of d_pose, d_a, d_b are given, and whether the two scale factors are
HEAD_COMBOS = [
    ((True, True, True), True),
    ((True, True, True), False),
    ((True, False, False), True),
    ((False, True, True), False),
    ((False, False, True), True),
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("C", [8, 40, 256, 264])
@pytest.mark.parametrize("HW", [1, 6, 20])
@pytest.mark.parametrize("B", [1, 3, 8, 11])
def test_parallel_pose_head_backward_has_the_bits_of_the_serial_walk(B, HW, C, dtype):
    from coivo_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(B * 10000 + HW * 100 + C)
    H, W = (4, 5) if HW == 20 else (2, 3) if HW == 6 else (1, 1)
    x = torch.randn(B, H, W, C, generator=g).to(d).to(dtype)           # both signs: the ReLU mask of dx is exercised
    w = torch.randn(8, C, generator=g).to(d)
    grads = [torch.randn(B, 6, generator=g).to(d), torch.randn(B, 1, generator=g).to(d), torch.randn(B, 1, generator=g).to(d)]
    sa, sb = torch.tensor([0.37], device=d), torch.tensor([1.9], device=d)
    dw0 = (torch.randn(8, C, generator=g) + 3.0).to(d)
    db0 = (torch.randn(8, generator=g) + 3.0).to(d)
    for present, scaled in HEAD_COMBOS:
        args = [t if p else None for t, p in zip(grads, present)]
        out = []
        for par in (0, 1):
            dx = torch.full_like(x, 7.0)
            dw, db = dw0.clone(), db0.clone()
            with _tuned(pose_head_det_parallel=par):
                ops.pose_head_bwd(x, w, args[0], args[1], args[2], dx, dw, db, sa if scaled else None, sb if scaled else None,
                                  deterministic=True)
                torch.cuda.synchronize()
            out.append((dx, dw, db))
        what = f"present={present} scaled={scaled}"
        assert not torch.equal(out[0][1], dw0), what                       # something was added
        for name, a, b in zip(("dx", "dw", "db"), out[0], out[1]):
            # bit patterns, so that a NaN or a zero of the other sign cannot pass as equal or differ unnoticed
            assert torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                               b.view(torch.int16 if b.element_size() == 2 else torch.int32)), f"{name}: {what}"
