"""CPU-side checks of the boundary: the C-ABI library builds, loads next to torch's HIP runtime and exports every
symbol include/colvo.h declares; argument validation fails loudly without touching a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.build()
    return _lib.load()


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "colvo.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(colvo_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported_and_bound(lib):
    from coivo_amd import _lib
    names = _declared_symbols()
    assert len(names) >= 19
    for n in names:
        assert hasattr(lib, n), f"libcolvo.so does not export {n}"
        assert n in _lib.SIGNATURES, f"{n} is declared in colvo.h but has no ctypes signature"
    assert sorted(_lib.SIGNATURES) == names


def test_abi_version_and_error_string(lib):
    from coivo_amd import _lib
    assert lib.colvo_abi_version() == _lib.ABI_VERSION
    assert isinstance(lib.colvo_last_error(), bytes)


def test_workspace_size_formula(lib):
    # max(backward: 14 partial sums per 60-column strip segment, forward: 2 per 62-column strip segment; >= 4 rows each)
    assert lib.colvo_warp_loss_workspace_floats(8, 256, 320) == max(8 * 6 * 64 * 16, 8 * 6 * 64 * 2)   # 16 = 14 gradient sums + loss + count (fused pass)
    assert lib.colvo_warp_loss_workspace_floats(2, 33, 47) == max(2 * 1 * 9 * 16, 2 * 1 * 9 * 2)
    assert lib.colvo_warp_loss_workspace_floats(0, 10, 10) == 0


def test_argument_validation_fails_loudly_without_gpu(lib):
    # null pointers / bad shapes are rejected before any launch
    rc = lib.colvo_warp_loss_fwd(0, 0, 0, 0, 0, 0, 0, 1, 8, 8, 0.85, 0, 0, 0)
    assert rc != 0 and b"null pointer" in lib.colvo_last_error()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    rc = lib.colvo_warp_loss_fwd(p, p, p, p, p, p, p, 1, 1, 8, 0.85, p, p, 0)   # H = 1 < 2
    assert rc != 0 and b"bad shape" in lib.colvo_last_error()
    from coivo_amd._lib import ConvDesc
    d = ConvDesc()
    d.dtype, d.B, d.Hi, d.Wi, d.Ho, d.Wo, d.Cout, d.ksize, d.stride, d.C0 = 0, 1, 8, 8, 8, 8, 16, 5, 1, 16
    rc = lib.colvo_conv_fwd(C.byref(d), p, 0, p, p, p, 0)
    assert rc != 0 and b"3x3" in lib.colvo_last_error()
    d.ksize, d.C0 = 3, 12
    rc = lib.colvo_conv_fwd(C.byref(d), p, 0, p, p, p, 0)
    assert rc != 0 and b"multiples of 8" in lib.colvo_last_error()


def test_round3_entry_points_validate_their_arguments(lib):
    """The widened objective, the multi-arena optimizer calls: rejected before any launch, with a message."""
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    # workspace size: 0 for shapes the call would refuse (H, W not divisible by 2^(scales-1); more than 4 scales)
    assert lib.colvo_full_objective_workspace_floats(2, 48, 64, 3) > 0
    assert lib.colvo_full_objective_workspace_floats(2, 48, 62, 3) == 0
    assert lib.colvo_full_objective_workspace_floats(2, 48, 64, 5) == 0
    assert lib.colvo_full_objective_workspace_floats(2, 48, 64, 1) < lib.colvo_full_objective_workspace_floats(2, 48, 64, 3)
    rc = lib.colvo_full_objective_fwd(p, p, p, 0, p, p, p, p, 2, 48, 64, 3, 0.85, 0.5, 0.1, p, p, 0)      # geo term without depth_r
    assert rc != 0 and b"reference depth" in lib.colvo_last_error()
    rc = lib.colvo_full_objective_fwd(p, p, p, p, p, p, p, p, 2, 48, 62, 3, 0.85, 0.5, 0.1, p, p, 0)
    assert rc != 0 and b"bad shape" in lib.colvo_last_error()
    rc = lib.colvo_full_objective_fwd(p, p, p, p, p, p, p, p, 2, 48, 64, 3, 0.85, 0.5, 0.1, p + 4, p, 0)  # misaligned workspace
    assert rc != 0 and b"16-byte aligned" in lib.colvo_last_error()
    rc = lib.colvo_full_objective_bwd(p, p, p, 2, 48, 64, 3, 0.5, 0.1, p, 0, p, p, p, 0)                   # geo term without d_depth_r
    assert rc != 0 and b"d_depth_r" in lib.colvo_last_error()
    rc = lib.colvo_adam_step_multi(0, 2, 1e-3, 0.9, 0.999, 1e-8, 1.0, 1, 0)
    assert rc != 0 and b"colvo_adam_step_multi" in lib.colvo_last_error()
    from coivo_amd._lib import AdamArena
    arr = (AdamArena * 1)()
    arr[0].param, arr[0].grad, arr[0].exp_avg, arr[0].exp_avg_sq, arr[0].n = p + 4, p, p, p, 8              # misaligned arena
    rc = lib.colvo_adam_step_multi(arr, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0, 1, 0)
    assert rc != 0 and b"16-byte aligned" in lib.colvo_last_error()
    rc = lib.colvo_adam_step_multi(arr, 5, 1e-3, 0.9, 0.999, 1e-8, 1.0, 1, 0)                               # more than COLVO_MAX_ARENAS
    assert rc != 0
    ptrs, sizes = (C.c_void_p * 1)(p), (C.c_size_t * 1)(20)                                                  # not a multiple of 16 bytes
    rc = lib.colvo_zero_multi(ptrs, sizes, 1, 0)
    assert rc != 0 and b"multiple of 16" in lib.colvo_last_error()
    rc = lib.colvo_adam_pack_step(0, 0, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0, 0, 1, 0)                         # no table
    assert rc != 0 and b"colvo_adam_pack_step" in lib.colvo_last_error()


# The size queries of the post-training calls (reconstruct, fuse, localize, consistency, refine, evaluate, cloud): arguments -> bytes
# (ints for the stitch), recorded from the library before the layouts moved onto the shared workspace carver (csrc/common.h).  Small,
# ragged and refused arguments for each; a refused shape answers 0 -- except that the stitch query answers for every positive shape.
# Every array that is not padded in today's layouts has a size that is a multiple of 16 bytes by its element (52 or 8 doubles, 32-byte
# states, 16-int lines), so the carver's uniform padding cannot move anything: the table pins that, and the 0 answers.
WORKSPACE_SIZES = {
    "colvo_stitch_workspace_ints": [((1, 1, 1, 1), 1), ((3, 17, 23, 1), 6), ((8, 256, 320, 4), 160), ((2, 5, 7, 9), 2),
                                    ((512, 256, 320, 1), 163840), ((70000, 8, 8, 1), 70000), ((0, 8, 8, 1), 0), ((2, 0, 8, 1), 0),
                                    ((2, 8, -3, 1), 0), ((2, 8, 8, 0), 0)],
    "colvo_fuse_plan_workspace_bytes": [((1, 1, 1, 1, 8, 8, 8), 16432), ((3, 17, 23, 1, 8, 16, 24), 16464),
                                        ((4, 64, 96, 2, 40, 24, 16), 16656), ((8, 256, 320, 1, 1024, 1024, 1024), 16795648),
                                        ((2, 5, 7, 9, 2048, 2048, 512), 33574912), ((3, 17, 23, 1, 12, 8, 8), 0),
                                        ((3, 17, 23, 1, 8, 8, 0), 0), ((0, 17, 23, 1, 8, 8, 8), 0), ((65536, 17, 23, 1, 8, 8, 8), 0),
                                        ((3, 17, 23, 0, 8, 8, 8), 0), ((3, 32768, 32768, 1, 8, 8, 8), 0),
                                        ((65535, 256, 320, 1, 8, 8, 8), 0), ((8, 256, 320, 1, 8192, 8192, 8192), 0)],
    "colvo_fuse_pool_bytes": [((1,), 16384), ((1066,), 17465344), ((4194303,), 68719460352), ((0,), 0), ((-1,), 0), ((4194304,), 0)],
    "colvo_fuse_extract_workspace_bytes": [((1,), 32), ((3,), 32), ((4096,), 16400), ((4097,), 16416), ((1066,), 4288),
                                           ((4194303,), 16781312), ((0,), 0), ((-5,), 0), ((4194304,), 0)],
    "colvo_localize_workspace_bytes": [((1, 1), 144), ((3, 5), 1952), ((7, 255), 228544), ((65535, 255), 2139586688), ((0, 1), 0),
                                       ((65536, 1), 0), ((1, 0), 0), ((1, 256), 0)],
    "colvo_consistency_workspace_bytes": [((1, 1), 608), ((5, 3), 4000), ((7, 16), 14336), ((65535, 16), 134215680), ((0, 1), 0),
                                          ((65536, 2), 0), ((1, 0), 0), ((1, 17), 0)],
    "colvo_refine_workspace_bytes": [((1, 2, 8, 8, 1), 1008), ((3, 5, 17, 23, 4), 9280), ((7, 8, 256, 320, 0), 2854880),
                                     ((5, 3, 33, 47, 64), 23136), ((65535, 2, 9, 9, 1), 31719600), ((0, 2, 8, 8, 1), 0),
                                     ((1, 65536, 8, 8, 1), 0), ((1, 2, 0, 8, 1), 0), ((1, 2, 32768, 32768, 1), 0), ((1, 2, 8, 8, 65), 0),
                                     ((1, 2, 8, 8, -1), 0)],
    "colvo_depth_metrics_workspace_bytes": [((1, 1, 1), 16480), ((3, 17, 23), 49440), ((8, 256, 320), 136448), ((2, 91, 91), 33088),
                                            ((65535, 5, 7), 1080016800), ((0, 8, 8), 0), ((65536, 8, 8), 0), ((2, 0, 8), 0),
                                            ((2, 8, -1), 0), ((1, 32768, 32768), 0)],
    "colvo_cloud_workspace_bytes": [((0, 0), 8423712), ((5, 0), 8423712), ((0, 7), 8423856), ((1000, 1001), 8443744),
                                    ((3, 1073741823), 21483260176), ((1073741823, 3), 8423776), ((-1, 0), 0), ((0, -1), 0),
                                    ((1073741824, 0), 0), ((0, 1073741824), 0)],
}


def test_post_training_workspace_sizes_are_the_recorded_ones(lib):
    """Host-only entries: no GPU.  Every size query include/colvo.h declares for these calls is in the table."""
    queries = [n for n in _declared_symbols() if re.search(r"_workspace_(bytes|ints)$|_pool_bytes$", n)]
    assert sorted(queries) == sorted(WORKSPACE_SIZES)
    for name, rows in WORKSPACE_SIZES.items():
        for args, size in rows:
            assert getattr(lib, name)(*args) == size, (name, args)


def test_stitch_refuses_a_cloud_whose_rows_leave_int32(lib):
    """A point's row is an int in k_stitch_write: N * ceil(H/stride) * ceil(W/stride) >= 2^31 is refused as a shape, and the shape is
    looked at before the pointers.  All pointers are NULL here: nothing can launch, with the check or without it."""
    N, H, W = 65535, 1024, 1024                          # 4096 blocks per frame: N * blocks < 2^30 passes, 6.9e10 rows do not fit
    assert lib.colvo_stitch_workspace_ints(N, H, W, 1) == N * 4096 < 2 ** 30 and N * H * W >= 2 ** 31
    rc = lib.colvo_stitch_point_cloud(0, 0, 0, N, H, W, 1, 10.0, 0, 0, 0, 0)
    assert rc != 0 and lib.colvo_last_error().startswith(b"colvo_stitch_point_cloud: bad shape"), lib.colvo_last_error()
    rc = lib.colvo_stitch_point_cloud(0, 0, 0, 32767, 256, 256, 1, 10.0, 0, 0, 0, 0)         # 2^31 - 65536 rows: the shape is accepted
    assert rc != 0 and b"null pointer" in lib.colvo_last_error(), lib.colvo_last_error()
    rc = lib.colvo_stitch_point_cloud(0, 0, 0, 32768, 256, 256, 1, 10.0, 0, 0, 0, 0)         # 2^31 rows exactly
    assert rc != 0 and b"bad shape" in lib.colvo_last_error(), lib.colvo_last_error()
    rc = lib.colvo_stitch_point_cloud(0, 0, 0, 32768, 256, 256, 2, 10.0, 0, 0, 0, 0)         # ... a quarter of them at stride 2
    assert rc != 0 and b"null pointer" in lib.colvo_last_error(), lib.colvo_last_error()


def test_python_ops_refuse_cpu_tensors():
    from coivo_amd import functional as Fh
    t = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        Fh.photometric_loss(t, t, torch.ones(1, 1, 8, 8), torch.zeros(1, 6), torch.eye(3)[None], torch.ones(1, 1),
                            torch.zeros(1, 1))
    with pytest.raises(RuntimeError, match="GPU only"):
        Fh.inverse_warp(t, torch.ones(1, 1, 8, 8), torch.zeros(1, 6), torch.eye(3)[None])


def test_product_package_does_not_import_the_oracle():
    """The oracle is test infrastructure: nothing under coivo_amd/ may reference it."""
    pkg = os.path.join(ROOT, "coivo_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f
                assert "colvo_spec" not in txt or f in ("nn.py", "functional.py", "optim.py", "inference.py", "data.py", "frames.hip", "heads.hip", "adam.hip",
                                                       "conv.hip", "conv_rt.hip", "wgrad_rt.hip", "warp_loss.hip", "reconstruct.hip"), f   # docstring citations only
    for f in ("nn.py", "functional.py", "optim.py", "ops.py", "ddp.py", "synth.py", "_lib.py", "build.py"):
        txt = open(os.path.join(pkg, f)).read()
        assert not re.search(r"^\s*(from|import)\s+oracle", txt, flags=re.M)


def test_tuning_table_hooks_and_no_stray_getenv(lib):
    """One table of dispatch thresholds (csrc/tuning.h): entries can be read / set by name, unknown names fail loudly, and no
    kernel source reads an environment variable of its own (the developer-build ablation switches excepted)."""
    from coivo_amd import _lib
    assert _lib.tune_get("bn64_min_wgs") == 4096 and _lib.tune_get("wgrad_atomic_mb") == 3
    saved = _lib.tune_get("quad_min_wgs")
    try:
        _lib.tune_set("quad_min_wgs", 7)
        assert _lib.tune_get("quad_min_wgs") == 7
    finally:
        _lib.tune_set("quad_min_wgs", saved)      # the tests share one process: later ones must see the library's default
    assert _lib.tune_get("quad_min_wgs") == saved
    assert lib.colvo_tune_set(b"no_such_entry", 1.0) != 0 and b"no tuning entry" in lib.colvo_last_error()
    csrc = os.path.join(ROOT, "coivo_amd", "csrc")
    for f in os.listdir(csrc):
        if f == "tuning.h":
            continue
        for line in open(os.path.join(csrc, f)):
            if "getenv(" in line:
                # (developer builds only: -DCOLVO_ABLATE of conv.hip, -DCOLVO_WTRACE of wgrad.hip; never the production library)
                    assert "COLVO_ABL" in line or "COLVO_TRACE" in line or "COLVO_WTRACE" in line, f"{f}: {line.strip()}"
    # the Python side honours its developer switches only under COLVO_DEV=1
    os.environ["COLVO_TEST_SWITCH"] = "x"
    dev = os.environ.pop("COLVO_DEV", None)
    try:
        assert _lib.dev_env("COLVO_TEST_SWITCH") is None
        os.environ["COLVO_DEV"] = "1"
        assert _lib.dev_env("COLVO_TEST_SWITCH") == "x"
    finally:
        os.environ.pop("COLVO_TEST_SWITCH")
        os.environ.pop("COLVO_DEV", None)
        if dev is not None:
            os.environ["COLVO_DEV"] = dev


def _network_conv_descs():
    """Every conv layer of DepthNet (the descriptors DepthNet._plan builds) and of PoseNet (its stride-2 chain, as
    PoseNet._forward_impl builds it) at 16, 64 and 128 frames of 256x320 and 64 frames of 512x640, bf16 and f32."""
    import types
    from coivo_amd import nn as hnn, ops
    for dt in (torch.bfloat16, torch.float32):
        for B, H, W in ((16, 256, 320), (64, 256, 320), (128, 256, 320), (64, 512, 640)):
            plan = hnn.DepthNet._plan(types.SimpleNamespace(compute_dtype=dt, _plans={}), B, H, W)
            for name, d in plan.items():
                yield f"DepthNet.{name} {dt} B={B} {H}x{W}", d
            h, w, cin = H, W, 8
            for i, c in enumerate(hnn.POSE_CH, start=1):
                d = ops.conv_desc(dt, B, h, w, cin, c, stride=2)
                yield f"PoseNet.conv{i} {dt} B={B} {H}x{W}", d
                h, w, cin = d.Ho, d.Wo, c


def test_wgrad_plan_queries_have_no_side_effects(lib):
    """colvo_conv_wgrad_splits / colvo_conv_wgrad_scratch_bytes run the weight-gradient planner alone: no HIP call (so they
    answer without a GPU), no kernel form counted, and the scratch size follows from the split count."""
    from coivo_amd import _lib
    n = 0
    for name, d in _network_conv_descs():
        before = _lib.form_counts()
        splits = lib.colvo_conv_wgrad_splits(C.byref(d))
        assert splits >= 1, f"{name}: {lib.colvo_last_error()}"
        scratch = lib.colvo_conv_wgrad_scratch_bytes(C.byref(d))
        assert scratch == splits * (d.Cout * 9 * (d.C0 + d.C1) + d.Cout) * 4, f"{name}: {lib.colvo_last_error()}"
        assert _lib.form_counts() == before, name
        n += 1
    assert n == 2 * 4 * (20 + 7)
    # a batch the call would process in image slices (a tensor of 1 GiB or more): the query is the largest of the slices' own
    # queries -- every slice re-uses the same scratch -- and still counts nothing, not even wgrad_sliced
    from coivo_amd import ops
    for dt, es in ((torch.float32, 4), (torch.bfloat16, 2)):
        per_img = 256 * 320 * 32 * es                       # enc1b at 256x320
        bmax = (2 ** 30 - 1) // per_img
        d = ops.conv_desc(dt, 2 * bmax + 3, 256, 320, 32, 32)
        assert d.B * per_img >= 2 ** 30
        before = _lib.form_counts()
        splits = lib.colvo_conv_wgrad_splits(C.byref(d))
        scratch = lib.colvo_conv_wgrad_scratch_bytes(C.byref(d))
        assert _lib.form_counts() == before, dt
        per_slice = []
        for b in (bmax, bmax, 3):                           # the sub-batches the call walks
            sub = ops.conv_desc(dt, b, 256, 320, 32, 32)
            per_slice.append(lib.colvo_conv_wgrad_splits(C.byref(sub)))
        assert min(per_slice) >= 1 and splits == max(per_slice), (dt, splits, per_slice)
        assert scratch == splits * (d.Cout * 9 * (d.C0 + d.C1) + d.Cout) * 4, dt


def test_every_command_reaches_its_entry_point(lib):
    """colvo_run_command runs one command through the decoder that eager ops and recorded passes share (csrc/program.hip run_one).
    Sent with NULL pointers, every recordable COLVO_CMD_* op, and every form of the ops that pick one from their slots, is refused
    by the argument check of the entry point it must reach, before any launch.  Commands that order streams are refused."""
    from coivo_amd import _lib, ops
    buf = (C.c_float * 16)()
    h = C.addressof(buf)                                 # non-NULL; no call below gets past its checks to dereference it
    d = ops.conv_desc(torch.bfloat16, 2, 16, 16, 16, 16)

    def refused(op, desc=d, p=(), i=(), stream=0):
        c = _lib.Cmd()
        c.op, c.stream, c.desc = op, stream, desc
        for k, v in enumerate(p):
            c.p[k] = v
        for k, v in enumerate(i):
            c.i[k] = v
        assert lib.colvo_run_command(C.byref(c), 0) != 0, op
        return lib.colvo_last_error().decode()

    entry = {_lib.CMD_CONV_FWD: "colvo_conv_fwd", _lib.CMD_CONV_DGRAD: "colvo_conv_dgrad", _lib.CMD_CONV_WGRAD: "colvo_conv_wgrad",
             _lib.CMD_PACK_NCHW: "colvo_pack_nchw", _lib.CMD_UNPACK_NHWC_GRAD: "colvo_unpack_nhwc_grad",
             _lib.CMD_DEPTH_HEAD_FWD: "colvo_depth_head_fwd", _lib.CMD_DEPTH_HEAD_BWD: "colvo_depth_head_bwd",
             _lib.CMD_DEPTH_HEAD_WGRAD: "colvo_depth_head_wgrad", _lib.CMD_POSE_HEAD_FWD: "colvo_pose_head_fwd",
             _lib.CMD_POSE_HEAD_BWD: "colvo_pose_head_bwd", _lib.CMD_DEPTH_HEAD_BWD_PARTS: "colvo_depth_head_bwd_parts",
             _lib.CMD_CONV_DGRAD_BOTH: "colvo_conv_dgrad_both", _lib.CMD_WGRAD_REDUCE_GROUP: "colvo_wgrad_reduce_group",
             _lib.CMD_CONV_DGRAD_PLANES: "colvo_conv_dgrad_planes", _lib.CMD_CONV_BWD_FUSED: "colvo_conv_bwd_fused",
             _lib.CMD_HEAD_WGRAD_REDUCE: "colvo_depth_head_wgrad_reduce", _lib.CMD_CONV_HEAD_FUSED: "colvo_conv_head_fused",
             _lib.CMD_PACK_STEM_POSE: "colvo_pack_stem_pose", _lib.CMD_HEAD_WGRAD_MFMA: "colvo_depth_head_wgrad_mfma"}
    control = {_lib.CMD_FORK, _lib.CMD_JOIN, _lib.CMD_SIDE_SYNC}
    assert set(entry) | control == {v for k, v in vars(_lib).items() if k.startswith("CMD_")}
    for op, name in entry.items():
        msg = refused(op)
        assert msg.startswith(name + ":"), (name, msg)

    # the forms: colvo_conv_wgrad_clean (i[2]) and _det (p[5]) share colvo_conv_wgrad's pointer check; _slabs (p[5] and i[1]) ignores
    # dw / db, so it is the one that gets to its own check -- a batch it would have to slice (512 MiB per image)
    big = ops.conv_desc(torch.bfloat16, 2, 1024, 1024, 256, 256)
    for form, cmd in (("colvo_conv_wgrad: null pointer", dict(i=(0, 0, 1))),
                      ("colvo_conv_wgrad: null pointer", dict(p=(0, 0, 0, 0, 0, h), i=(64, 0, 0))),
                      ("colvo_conv_wgrad_slabs: batch 2 would be sliced", dict(desc=big, p=(h, 0, h, 0, 0, h), i=(64, 1))),
                      ("colvo_conv_wgrad: null pointer", dict(desc=big, p=(h, 0, h, 0, 0, h), i=(64, 0)))):
        msg = refused(_lib.CMD_CONV_WGRAD, **cmd)
        assert msg.startswith(form), (form, msg)
    msg = refused(_lib.CMD_DEPTH_HEAD_WGRAD, p=(0, 0, 0, 0, h))                       # p[4]: scratch
    assert msg.startswith("colvo_depth_head_wgrad_det:"), msg
    msg = refused(_lib.CMD_POSE_HEAD_BWD, i=(0, 0, 0, 0, 1))                           # i[4]: det
    assert msg.startswith("colvo_pose_head_bwd_det:"), msg

    for op in control:
        msg = refused(op)
        assert msg.startswith("colvo_run_command:") and str(op) in msg, msg
    msg = refused(_lib.CMD_CONV_FWD, stream=1)
    assert msg.startswith("colvo_run_command:"), msg
    assert lib.colvo_run_command(None, 0) != 0 and lib.colvo_last_error().startswith(b"colvo_run_command:")

def test_every_kernel_form_has_a_distinct_name(lib):
    """colvo_form_counts / colvo_form_name: at most the 32 counters _lib.form_counts reads, every one named, no two alike, NULL beyond
    the last; the counters start at zero and a name lookup out of range does not crash."""
    from coivo_amd import _lib
    buf = (C.c_longlong * 32)()
    n = lib.colvo_form_counts(buf, 32)
    assert 8 <= n <= 32
    names = [lib.colvo_form_name(i) for i in range(n)]
    assert all(isinstance(x, bytes) and x for x in names), names
    assert len(set(names)) == n, names
    assert lib.colvo_form_name(n) is None and lib.colvo_form_name(-1) is None
    assert list(_lib.form_counts()) == [x.decode() for x in names]
    # the leaves the dispatch trees of csrc/conv.hip, conv_rt.hip, wgrad.hip, bwd16.hip and fwd16.hip count
    for leaf in ("conv_rt", "conv_q", "conv_up2_bn16", "conv_up2_bn32", "dgrad_s2", "dgrad_s2_ring", "dgrad_up2", "dgrad_both", "conv_tile",
                 "conv_ring", "conv_wide", "conv_res", "conv_res_s2", "conv_bn64", "wgrad_teams", "wgrad_tail", "wgrad_mt4", "wgrad_sliced",
                 "wgrad_up2", "wgrad_rt", "bwd16", "fwd16_head", "dgrad_planes_mfma", "conv_rt_bn32"):
        assert leaf.encode() in names, leaf


def test_exact_data_stays_in_the_exact_regime_at_every_production_shape():
    """tests/conv_exact.py's value sets and dy density rule keep every output element of every pass within 2^22 quanta (fp32 exact
    below 2^24, whatever the summation order) for every conv layer of the benchmark's shapes: the exact GPU tests cannot silently
    leave the exact regime at a future shape."""
    from tests import conv_exact as X
    n = 0
    for name, d in _network_conv_descs():
        cin = d.C0 + d.C1
        assert X.bound_fwd(cin) <= X.BOUND, name
        assert X.bound_dgrad(d.Cout, bool(d.up0 or d.up1)) <= X.BOUND, name
        npix = d.B * d.Ho * d.Wo
        assert X.bound_wgrad(npix) <= X.BOUND, (name, X.bound_wgrad(npix))
        assert X.dy_density(npix) * npix >= min(npix / 4, 1e5), name          # ... and dy is not so sparse that the check is empty
        n += 1
    assert n == 2 * 4 * (20 + 7)
    # the value sets: every magnitude in its quantum, representable in bf16
    g = torch.Generator().manual_seed(1)
    for t, q, m in ((X.make_source((4096,), g, "cpu"), X.QX, X.X_MAX), (X.make_weights(16, 16, g, "cpu"), X.QW, X.W_MAX),
                    (X.make_bias(4096, g, "cpu"), X.QB, X.B_MAX), (X.make_dy((4096,), 0.5, g, "cpu"), X.QDY, X.DY_MAX),
                    (X.make_base((4096,), g, "cpu"), X.QBASE, X.BASE_MAX)):
        assert torch.equal(t.to(torch.bfloat16).float(), t)
        assert torch.equal(t / q, (t / q).round()) and float((t / q).abs().max()) == m


def test_exact_data_stays_in_the_exact_regime_at_the_inference_shapes():
    """The same bounds for the descriptors of tests/test_conv_exact_small_batch_gpu.py (1 to 13 frames or pairs of 256x320, 1 and 3 of
    512x640).  Fewer pixels than at the benchmark's shapes and a dy density capped at RHO_MAX: the bounds should hold, and here they
    are computed, not assumed -- down to PoseNet's 2x3 last layer, where the weight gradient sums six pixels and dy must still
    hold something."""
    from tests import conv_exact as X
    n = 0
    for net, B, H, W in X.SMALL_BATCH_SHAPES:
        for name, lay in X.layers(net, B, H, W):
            what = f"{net} {name} B={B} {H}x{W}"
            assert X.bound_fwd(lay.Cin) <= X.BOUND, what
            assert X.bound_dgrad(lay.Cout, lay.up0 or lay.up1) <= X.BOUND, what
            npix = lay.B * lay.Ho * lay.Wo
            assert X.dy_density(npix) <= X.RHO_MAX, what
            assert X.bound_wgrad(npix) <= X.BOUND, (what, X.bound_wgrad(npix))
            assert X.dy_density(npix) * npix >= min(npix / 4, 1e5), what
            n += 1
    assert n == 6 * 20 + 4 * 7
    last = dict(X.layers("pose", 1, 256, 320))["conv7"]
    assert (last.Ho, last.Wo) == (2, 3)


def test_call_passes_pointers_and_raises_under_the_entry_points_name(lib):
    """_lib.call: tensors go as their addresses and None as NULL, the status is checked under the name that was called.  The native
    half uses colvo_mesh_topology_components, which refuses a scratch address that is not 16-byte aligned before its first HIP call."""
    import types
    import unittest.mock as mock
    from coivo_amd import _lib
    t = torch.zeros(5)
    seen = []
    stub = types.SimpleNamespace(colvo_x=lambda *a: seen.append(a) or 0, colvo_y=lambda *a: 7, colvo_last_error=lambda: b"why")
    with mock.patch.object(_lib, "load", lambda: stub):
        assert _lib.call("colvo_x", t, None, 3, 0.5, "s") is None
        assert seen == [(t.data_ptr(), 0, 3, 0.5, "s")]
        with pytest.raises(RuntimeError, match=r"colvo_y failed \(code 7\): why"):
            _lib.call("colvo_y", t)
    with pytest.raises(RuntimeError, match="colvo_mesh_topology_components failed .*scratch must be 16-byte aligned"):
        _lib.call("colvo_mesh_topology_components", 0x1000, 4, 2, 0x1008, 0x2000, 0x3000, 0x4000, None)
