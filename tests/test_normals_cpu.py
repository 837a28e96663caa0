"""CPU: the NumPy replica of the cloud-normals contract (tests/normals_ref.py) held to geometry -- planes whose normal is known, a depth
step that no finite difference may straddle, and the tube of tests/consistency_ref.py, whose wall has the analytic inward normal
(-x, -y, 0) / |.| -- and the host side of the call: the ISA metadata of csrc/normals.hip, the refusals of colvo_cloud_normals and the
ValueErrors of inference.cloud_normals, none of which needs a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import consistency_ref as CR
from tests import fuse_ref as F
from tests import normals_ref as NR

f32 = np.float32
U = 2.0 ** -24                       # unit roundoff of float32
MAX_DEPTH = 4.5
TUBE_GRID = dict(voxel_size=0.02, origin=(-1.28, -1.28, -0.64), dims=(128, 128, 320))     # holds every sample of the tube below 4.5


def _cams(N, H, W, fx):
    K = np.zeros((N, 3, 3), f32)
    K[:, 0, 0] = K[:, 1, 1] = fx
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = (W - 1) / 2, (H - 1) / 2, 1
    M = np.tile(np.eye(4, dtype=f32), (N, 1, 1))
    return K, M


def _plane_depth(n, c, K, H, W):
    """Exact z-depth of the plane n . X = c per pixel (float64), rounded once to float32."""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    k = K[0].astype(np.float64)
    ray = np.stack([(u - k[0, 2]) / k[0, 0], (v - k[1, 2]) / k[1, 1], np.ones_like(u)], -1)
    return (c / (ray @ np.asarray(n, np.float64))).astype(f32)[None, None]


def test_fronto_parallel_plane_is_exactly_minus_z():
    H, W = 9, 11
    K, M = _cams(1, H, W, 10.0)
    s = NR.sample_normals(np.full((1, 1, H, W), 2.0, f32), K, M, max_depth=MAX_DEPTH)
    assert s["kept"].all() and s["normal"].all()
    assert np.array_equal(s["cam"], np.broadcast_to(np.array([0, 0, -1], f32), (1, H, W, 3)))       # (-0.0 == 0.0)
    assert np.array_equal(s["q"], np.broadcast_to(np.array([0, 0, -16384]), (1, H, W, 3)))
    # borders use one-sided differences, a 1 x 1 image has none
    assert s["one_sided"][0, 0].all() and s["one_sided"][0, :, 0].all() and not s["one_sided"][0, 1:-1, 1:-1].any()
    s1 = NR.sample_normals(np.full((1, 1, 1, 1), 2.0, f32), *_cams(1, 1, 1, 10.0), max_depth=MAX_DEPTH)
    assert s1["kept"].all() and not s1["normal"].any() and not s1["q"].any()


def test_tilted_plane_equals_the_analytic_normal_to_float32_rounding():
    """A camera point has a relative error of at most 3 u (the depth's rounding, the division, the product), a tangent an absolute one
    of at most 2 * 3 u |P| + u |t|; a cross product of two vectors with relative errors e_u, e_v turns by at most (e_u + e_v) / sin of
    the angle between them (plus its own three roundings), and the normalisation and the comparison add a few u."""
    H, W, fx = 12, 14, 8.0
    K, M = _cams(1, H, W, fx)
    n = np.array([0.3, -0.2, -1.0])
    n /= np.linalg.norm(n)
    d = _plane_depth(n, -2.0, K, H, W)                                    # the plane faces the camera: n . P = -2 < 0
    assert (d > 1.0).all() and (d < 4.0).all()
    s = NR.sample_normals(d, K, M, max_depth=MAX_DEPTH)
    assert s["normal"].all()
    got = s["cam"].astype(np.float64)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    P = np.stack([(u - (W - 1) / 2) / fx, (v - (H - 1) / 2) / fx, np.ones_like(u)], -1) * d[0, 0][..., None].astype(np.float64)
    p_max = np.linalg.norm(P, axis=-1).max()
    t_min = d.min() / fx                                                  # a one-sided tangent is at least one pixel at the nearest depth
    sin_min = 0.5                                                         # tangents of a plane tilted by < 25 degrees: far from parallel
    bound = ((2 * (6 * U * p_max / t_min + U)) / sin_min + 8 * U)
    err = np.linalg.norm(got - n[None, None, None], axis=-1).max()
    print(f"tilted plane: largest deviation {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.abs(np.linalg.norm(got, axis=-1) - 1).max() <= 4 * U
    assert np.abs(s["q"] - np.rint(got * 16384)).max() <= 1


def test_no_difference_straddles_a_depth_step_larger_than_rel_edge():
    H, W, c0 = 7, 12, 6
    K, M = _cams(1, H, W, 10.0)
    d = np.full((1, 1, H, W), 1.0, f32)
    d[..., c0:] = 1.5                                                     # |1.5 - 1| / 2.5 = 0.2 > 0.05
    s = NR.sample_normals(d, K, M, max_depth=MAX_DEPTH, rel_edge=0.05)
    left, right = s["use"][0], s["use"][1]
    assert not right[0, :, c0 - 1].any() and not left[0, :, c0].any()     # the neighbour across the step is not usable
    assert right[0, :, :c0 - 1].all() and left[0, :, c0 + 1:].all()
    assert s["one_sided"][0, :, c0 - 1].all() and s["one_sided"][0, :, c0].all()
    # both sides are fronto-parallel: a tangent across the step would tilt the normal, a one-sided one keeps it exactly -z
    assert s["normal"].all() and np.array_equal(s["cam"], np.broadcast_to(np.array([0, 0, -1], f32), (1, H, W, 3)))
    # a step below rel_edge is differenced across: |1.05 - 1| / 2.05 = 0.024
    d[..., c0:] = 1.05
    s = NR.sample_normals(d, K, M, max_depth=MAX_DEPTH, rel_edge=0.05)
    assert s["use"][1][0, :, c0 - 1].all() and (s["cam"][0, :, c0 - 1, 2] > -1).all()
    # ... and with rel_edge below it, not
    s = NR.sample_normals(d, K, M, max_depth=MAX_DEPTH, rel_edge=0.02)
    assert not s["use"][1][0, :, c0 - 1].any() and np.array_equal(s["cam"][0, :, c0 - 1, 2], np.full(H, -1, f32))


def test_invalid_depths_give_no_normal_and_are_no_neighbours():
    H, W = 5, 6
    K, M = _cams(1, H, W, 10.0)
    d = np.full((1, 1, H, W), 2.0, f32)
    d[0, 0, 2, 2:4] = [np.nan, np.inf]
    d[0, 0, 0, 0], d[0, 0, 4, 5], d[0, 0, 4, 0] = 0.0, -1.0, 5.0          # 5.0 >= max_depth
    s = NR.sample_normals(d, K, M, max_depth=MAX_DEPTH)
    bad = ~((d[0, 0] > 0) & (d[0, 0] < MAX_DEPTH))
    assert np.array_equal(s["kept"][0], ~bad) and not s["normal"][0][bad].any() and s["normal"][0][~bad].all()
    assert not s["q"][0][bad].any()
    assert np.array_equal(s["cam"][0][~bad], np.broadcast_to(np.array([0, 0, -1], f32), (int((~bad).sum()), 3)))


@functools.lru_cache(maxsize=None)
def _tube(min_obs=1, stride=1):
    d, K, M = CR.tube_scene(5, 64, 96, 5)
    fu = F.fuse(d, None, K, M, stride=stride, max_depth=MAX_DEPTH, min_obs=min_obs, **TUBE_GRID)
    cn = NR.cloud_normals(d, K, M, fu["voxels"], stride=stride, max_depth=MAX_DEPTH, **TUBE_GRID)
    return fu, cn


def test_tube_every_voxel_has_a_normal_within_three_degrees_of_the_analytic_one():
    fu, cn = _tube()
    assert fu["n_outside"] == 0 and len(fu["points"]) > 18000
    assert (cn["counts"] > 0).all() and np.array_equal(cn["counts"], fu["counts"])
    assert cn["stats"].tolist() == [fu["n_input"]] * 3 + [0]
    p = fu["points"].astype(np.float64)
    want = np.stack([-p[:, 0], -p[:, 1], np.zeros(len(p))], 1)
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    got = cn["normals"].astype(np.float64)
    ang = np.degrees(np.arccos(np.clip((want * got).sum(1), -1, 1)))
    print(f"tube normals: median {np.median(ang):.4f} deg, 99th percentile {np.percentile(ang, 99):.4f}, max {ang.max():.4f}")
    assert ang.max() < 3.0
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 4 * U
    # the observations of a voxel of a smooth wall agree: coherence close to 1, and never above it by more than the quantisation
    assert cn["coherence"].min() > 0.999 and cn["coherence"].max() <= 1 + 2.0 ** -13


def test_tube_rows_below_min_obs_end_in_the_unmatched_count():
    fu1, cn1 = _tube()
    fu2, cn2 = _tube(min_obs=2)
    assert 0 < len(fu2["points"]) < len(fu1["points"])
    kept, normal, matched, unmatched = cn2["stats"].tolist()
    assert kept == normal == fu2["n_input"] and unmatched == int(fu1["counts"][fu1["counts"] < 2].sum()) > 0
    assert matched == int(cn2["counts"].sum()) == kept - unmatched
    rows = np.nonzero(fu1["counts"] >= 2)[0]
    assert np.array_equal(cn2["normals"].view(np.uint32), cn1["normals"][rows].view(np.uint32))


# ---- the library's host side ------------------------------------------------------------------------------------------------ #
@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.build()
    return _lib.load()


def test_kernels_use_no_scratch_and_native_integer_adds(lib, tmp_path):
    import re
    from coivo_amd import build
    asm = open(build.emit_asm("normals.hip", str(tmp_path / "normals.s"))).read()
    kernels = set(re.findall(r"\.name:\s+(\S*k_normals_\w+)", asm))
    assert len(kernels) == 4 and all(any(f"k_normals_{n}" in k for k in kernels) for n in ("keys", "accumulate", "write", "stats")), kernels
    for key in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count"):
        vals = re.findall(rf"\.{key}:\s+(\d+)", asm)
        assert len(vals) == 4 and all(int(v) == 0 for v in vals), (key, vals)
    assert "global_atomic_add_x2" in asm and "cmpswap" not in asm
    assert set(re.findall(r"float_denorm_mode_32 (\d)", asm)) == {"3"}          # float32 denormals are kept, as the contract says


GOOD = dict(N=2, H=8, W=8, stride=1, max_depth=4.5, o=(0.0, 0.0, 0.0), vs=0.02, dims=(8, 8, 8), M=4, rel_edge=0.05)


def _call(lib, p, **kw):
    a = dict(GOOD)
    a.update(kw)
    ptrs = a.pop("ptrs", [p] * 9)          # depths, K, cam2world | voxels | scratch, normals, counts, coherence, stats
    return lib.colvo_cloud_normals(ptrs[0], ptrs[1], ptrs[2], a["N"], a["H"], a["W"], a["stride"], a["max_depth"], *a["o"], a["vs"],
                                   *a["dims"], ptrs[3], a["M"], a["rel_edge"], *ptrs[4:9], 0)


def test_colvo_cloud_normals_refuses_before_any_hip_call(lib):
    """Host pointers: a call that got past its checks would fault or report a HIP error with another prefix."""
    buf = (C.c_float * 72)()
    p = (C.addressof(buf) + 15) // 16 * 16
    for what, kw in (("bad row count", dict(M=-1)), ("bad shape", dict(N=0)), ("bad shape", dict(N=65536)), ("bad shape", dict(H=0)),
                     ("bad shape", dict(stride=0)), ("bad shape", dict(H=1 << 15, W=1 << 15)), ("bad grid", dict(dims=(8, 12, 8))),
                     ("bad grid", dict(dims=(8, 8, 0))), ("bad grid", dict(vs=0.0)), ("bad grid", dict(vs=float("nan"))),
                     ("bad grid", dict(o=(float("inf"), 0.0, 0.0))), ("bad grid", dict(dims=(8192, 8192, 8192))),
                     ("bad max_depth", dict(max_depth=0.0)), ("bad max_depth", dict(max_depth=float("inf"))),
                     ("bad rel_edge", dict(rel_edge=0.0)), ("bad rel_edge", dict(rel_edge=-0.1)), ("bad rel_edge", dict(rel_edge=float("nan"))),
                     ("bad rel_edge", dict(rel_edge=float("inf"))), ("16-byte aligned", dict(ptrs=[p] * 4 + [p + 4] + [p] * 4)),
                     ("null pointer", dict(ptrs=[0] + [p] * 8)), ("null pointer", dict(ptrs=[p] * 3 + [0] + [p] * 5)),
                     ("null pointer", dict(ptrs=[p] * 8 + [0])), ("null pointer", dict(ptrs=[p] * 5 + [0] + [p] * 3))):
        rc = _call(lib, p, **kw)
        msg = lib.colvo_last_error()
        assert rc != 0 and msg.startswith(b"colvo_cloud_normals:") and what.encode() in msg, (what, kw, msg)
    assert lib.colvo_cloud_normals_scratch_bytes(-1) == 0
    assert lib.colvo_cloud_normals_scratch_bytes(0) == 256 * 16 * 4
    assert lib.colvo_cloud_normals_scratch_bytes(5) == 5 * 32 + 256 * 16 * 4 + 48          # keys padded to 16 bytes


def test_cloud_normals_argument_errors(lib):
    from coivo_amd import inference as I
    fused = I.FusedCloud(torch.zeros(2, 3), None, torch.ones(2, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32), (0.0, 0.0, 0.0),
                         (8, 8, 8), 0.02, 2, 0, 1, 2)
    d, K, M = torch.ones(1, 1, 4, 4), torch.eye(3)[None], torch.eye(4)[None]
    for bad in (dict(rel_edge=0.0), dict(rel_edge=-1.0), dict(rel_edge=float("nan")), dict(rel_edge=float("inf")), dict(rel_edge=None),
                dict(max_depth=0.0), dict(max_depth=float("inf")), dict(stride=0), dict(stride=1.0), dict(stride=True)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            I.cloud_normals(fused, d, K, M, **bad)
    with pytest.raises(ValueError, match="FusedCloud"):
        I.cloud_normals((fused.points,), d, K, M)
    with pytest.raises(ValueError, match="depths"):
        I.cloud_normals(fused, d[0], K, M)
    with pytest.raises(ValueError, match="grid"):
        I.cloud_normals(fused._replace(dims=(8, 12, 8)), d, K, M)
    with pytest.raises(ValueError, match="limits"):
        I.cloud_normals(fused._replace(dims=(8192, 8192, 8192)), d, K, M)
