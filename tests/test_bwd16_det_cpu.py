"""CPU-side checks of the deterministic fused backward's boundary (colvo_conv_bwd_fused_scratch_bytes, colvo_conv_bwd_fused_det through
its command): the scratch query is the launch's grid times one row, answers without a GPU and counts nothing; the command's scratch
slot selects the _det entry, whose argument check refuses NULL tensors before any launch."""
import ctypes as C

import pytest
import torch

ROW = 16 * 9 * 16 + 16


@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.build()
    return _lib.load()


def _rows(B, H, W, wgs=768, slots=1024):
    """csrc/bwd16.hip bwd16_grid for modes 0 and 1 (four workgroups per CU on 256 CUs) at the production tuning."""
    ntiles = B * ((W + 15) // 16) * ((H + 7) // 8)
    want = min(4 * wgs, ntiles // 40)
    if want > wgs:
        wgs = max(1, (want + slots // 2) // slots) * slots
    wgs = min(wgs, ntiles)
    tpw = -(-ntiles // wgs)
    return -(-ntiles // tpw)


def test_scratch_bytes_is_the_grid_times_one_row(lib):
    from coivo_amd import _lib, ops
    assert _lib.tune_get("bwd16_wgs") == 768
    assert _rows(16, 256, 320) == 732 and _rows(64, 256, 320) == 1024
    for B, H, W in ((16, 256, 320), (64, 256, 320), (128, 256, 320), (64, 512, 640)):
        d = ops.conv_desc(torch.bfloat16, B, H, W, 16, 16)              # DepthNet.iconv1
        assert lib.colvo_conv_bwd_fused_ok(C.byref(d))
        before = _lib.form_counts()
        for mode in (0, 1):
            assert lib.colvo_conv_bwd_fused_scratch_bytes(C.byref(d), mode) == _rows(B, H, W) * ROW * 4, (B, H, W, mode)
        assert lib.colvo_conv_bwd_fused_scratch_bytes(C.byref(d), 2) == 0        # the head's own weight gradient has no slab form
        assert _lib.form_counts() == before


def test_scratch_bytes_is_zero_for_a_layer_the_kernel_refuses(lib):
    from coivo_amd import _lib, ops
    before = _lib.form_counts()
    for d in (ops.conv_desc(torch.bfloat16, 2, 64, 96, 32, 16), ops.conv_desc(torch.float32, 2, 64, 96, 16, 16),
              ops.conv_desc(torch.bfloat16, 2, 64, 96, 16, 16, stride=2), ops.conv_desc(torch.bfloat16, 2048, 256, 320, 16, 16)):
        assert not lib.colvo_conv_bwd_fused_ok(C.byref(d))
        assert lib.colvo_conv_bwd_fused_scratch_bytes(C.byref(d), 0) == 0
    assert lib.colvo_conv_bwd_fused_scratch_bytes(None, 0) == 0
    assert _lib.form_counts() == before


def test_the_scratch_slot_selects_the_det_entry(lib):
    from coivo_amd import _lib, ops
    buf = (C.c_float * 16)()
    h = C.addressof(buf)
    d = ops.conv_desc(torch.bfloat16, 2, 16, 16, 16, 16)

    def refused(p, i=()):
        c = _lib.Cmd()
        c.op, c.stream, c.desc = _lib.CMD_CONV_BWD_FUSED, 0, d
        for k, v in p.items():
            c.p[k] = v
        for k, v in enumerate(i):
            c.i[k] = v
        before = _lib.form_counts()
        assert lib.colvo_run_command(C.byref(c), 0) != 0
        assert _lib.form_counts() == before
        return lib.colvo_last_error().decode()

    assert refused({}).startswith("colvo_conv_bwd_fused: null pointer")
    assert refused({9: h}, (1, 64)).startswith("colvo_conv_bwd_fused_det: null pointer")
    # without dw (p[4]) the same entry leaves the rows in the scratch: the same checks in front of the launch
    assert refused({0: h, 1: h, 2: h, 3: h, 9: h}, (1, 4 * ROW * 4 - 4)).startswith("colvo_conv_bwd_fused_det: scratch of")
    # every tensor given, a scratch too small for the grid (4 tiles, 4 rows): refused by size before any launch
    full = {k: h for k in (0, 1, 2, 3, 4, 5, 9)}
    msg = refused(full, (1, 4 * ROW * 4 - 4))
    assert msg.startswith("colvo_conv_bwd_fused_det: scratch of"), msg
    msg = refused({**full, 6: h, 7: h, 8: h}, (1, 4 * ROW * 4))
    assert msg.startswith("colvo_conv_bwd_fused_det: the head's own weight gradient"), msg
