"""CPU checks of the multi-view depth consistency filter (coivo_amd.inference.filter_depths, csrc/consistency.hip): the NumPy
replica the GPU tests compare with (tests/consistency_ref.py) against the float64 oracle and against what the filter is for on
a synthetic tube, its bookkeeping, the C ABI's refusals before any HIP call and the Python wrapper's argument errors."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import consistency_ref as R

MAX_DEPTH = 4.5
SHAPES = [(3, 17, 23), (6, 64, 96), (8, 256, 320)]
# The largest rel = |P_z - s| / (P_z + s) the replica reports on the clean tube (window 2, step 1, seed 3): the bilinear
# interpolation error of a curved wall, which shrinks with the resolution.  The property tests use four times it as rel_tol.
CLEAN_REL = {(3, 17, 23): 3.61e-3, (6, 64, 96): 3.6e-4, (8, 256, 320): 4.0e-5}
SEED = 3


@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _scene(N, H, W):
    return R.tube_scene(N, H, W, SEED)


@functools.lru_cache(maxsize=None)
def _filtered(N, H, W, corrupted, rel_tol, min_agree=1, max_violated=0):
    d, K, M = _scene(N, H, W)
    if corrupted:
        d = R.corrupt(d, N // 2)
    return R.filter_depths(d, K, M, window=2, step=1, rel_tol=rel_tol, min_agree=min_agree, max_violated=max_violated,
                           max_depth=MAX_DEPTH, detail=True)


# ---- the replica against the float64 oracle ---------------------------------------------------------------------------- #
def _pose_of(T):
    """(tx, ty, tz, rx, ry, rz) of a 4x4 [R|t] with R = Rz Ry Rx (the spec's pose_vec2mat), float64."""
    R_, t = T[:3, :3], T[:3, 3]
    ry = -math.asin(float(R_[2, 0]))
    rx = math.atan2(float(R_[2, 1]), float(R_[2, 2]))
    rz = math.atan2(float(R_[1, 0]), float(R_[0, 0]))
    return torch.tensor([float(t[0]), float(t[1]), float(t[2]), rx, ry, rz], dtype=torch.float64)


def _oracle_classes(depths, K, M, window, step, rel_tol, max_depth):
    """The contract composed from the float64 oracle's project / bilinear_sample (as its geometric_consistency_loss composes
    them) plus the tap-validity rule: class of every (frame, slot, pixel), shaped like the replica's."""
    from oracle import colvo_spec as S
    N, _, H, W = depths.shape
    assert np.all(K == K[0])                                        # the spec's project() has one K for both frames
    d64, K64, M64 = (torch.from_numpy(np.asarray(a)).double() for a in (depths, K, M))
    tol, md = float(np.float32(rel_tol)), float(np.float32(max_depth))
    nbr = R.neighbours(N, window, step)
    cls = np.full((N, 2 * window, H, W), R.NONE, np.int8)
    u = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    v = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    for i in range(N):
        d = d64[i:i + 1]
        cand = (d[0, 0] > 0) & (d[0, 0] < md)
        for s, j in enumerate(nbr[i]):
            if j < 0:
                continue
            pose = _pose_of(torch.linalg.inv(M64[j]) @ M64[i]).view(1, 6)
            k = K64[i:i + 1]
            x, y, valid = S.project(d, pose, k)
            T = S.pose_vec2mat(pose)
            X, Y = (u - k[0, 0, 2]) / k[0, 0, 0] * d[:, 0], (v - k[0, 1, 2]) / k[0, 1, 1] * d[:, 0]
            d_proj = T[0, 2, 0] * X + T[0, 2, 1] * Y + T[0, 2, 2] * d[:, 0] + T[0, 2, 3]
            dj = d64[j:j + 1]
            ok_j = ((dj > 0) & (dj < md)).double()
            clean_j = torch.where(ok_j > 0, dj, torch.ones_like(dj))          # (an infinite tap times a zero weight is NaN)
            d_samp = S.bilinear_sample(clean_j, x, y, valid)[:, 0]
            xs, ys = torch.where(valid, x, torch.zeros_like(x)), torch.where(valid, y, torch.zeros_like(y))
            x0, y0 = torch.floor(xs).long(), torch.floor(ys).long()
            x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
            m = ok_j[0, 0]
            taps = (m[y0, x0] * m[y0, x1] * m[y1, x0] * m[y1, x1]) > 0
            visible = (valid & taps)[0]
            rel = ((d_proj - d_samp).abs() / (d_proj + d_samp))[0]
            agree, occ = rel < tol, (d_samp < d_proj)[0]
            c = torch.where(~visible, R.INVISIBLE, torch.where(agree, R.AGREE, torch.where(occ, R.OCCLUDED, R.VIOLATED)))
            cls[i, s] = torch.where(cand, c, R.NONE).numpy().astype(np.int8)
    return cls


@pytest.mark.parametrize("rel_tol", [0.02, 0.0002])
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_replica_classes_agree_with_the_float64_oracle(N, H, W, rel_tol):
    """Every (pixel, neighbour) sample of the corrupted tube must get the class the float64 composition gives it; at most
    0.1 % of the samples may differ (float32 against float64 at a decision boundary)."""
    d, K, M = _scene(N, H, W)
    d = R.corrupt(d, N // 2)
    got = _filtered(N, H, W, True, rel_tol)["cls"]
    want = _oracle_classes(d, K, M, 2, 1, rel_tol, MAX_DEPTH)
    assert np.array_equal(got == R.NONE, want == R.NONE)
    samples = int((want != R.NONE).sum())
    differ = int((got != want).sum())
    counts = {name: int((want == c).sum()) for name, c in (("invisible", R.INVISIBLE), ("agree", R.AGREE), ("occluded", R.OCCLUDED),
                                                           ("violated", R.VIOLATED))}
    print(f"{(N, H, W)} rel_tol {rel_tol}: {differ} of {samples} samples differ; float64 classes {counts}")
    assert samples > 0 and min(counts.values()) > 0                         # every class occurs
    assert differ <= 0.001 * samples


# ---- what the filter is for -------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_clean_tube_every_visible_neighbour_agrees(N, H, W):
    probe = _filtered(N, H, W, False, 0.02)
    worst = float(np.nanmax(probe["rel"]))
    print(f"{(N, H, W)}: largest clean rel {worst:.3e} (recorded {CLEAN_REL[(N, H, W)]:.1e})")
    assert worst <= CLEAN_REL[(N, H, W)]                                    # the recorded figure still covers the scene
    r = _filtered(N, H, W, False, 4 * CLEAN_REL[(N, H, W)])
    votes = r["votes"].astype(np.int64)
    visible = votes.sum(1)
    assert np.array_equal(votes[:, 0], visible) and visible.max() > 0
    d = _scene(N, H, W)[0]
    cand = (d[:, 0] > 0) & (d[:, 0] < np.float32(MAX_DEPTH))
    assert 0.10 < 1.0 - cand.mean() < 0.16                                  # the lumen: the invalid-tap path is exercised
    assert np.array_equal(np.isfinite(r["depths"][:, 0]), cand & (visible > 0))
    assert (r["cls"] == R.INVISIBLE).sum() > 0


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_corrupted_blocks_are_rejected_and_nothing_else_in_their_frame(N, H, W):
    """No block pixel is kept, the 0.7 block is violated, the 1.4 block occluded, and outside the blocks exactly the same pixels
    are kept as on the clean scene -- asserted to the bit for the whole corrupted frame.

    Where this departs from the issue's wording ("exactly the same pixels outside the block are kept as on the clean scene", "no
    pixel outside the block is lost"): read over ALL frames that sentence cannot hold under the contract itself.  A pixel of another
    frame whose sample lands in the 1.4 block finds a surface behind its own point, which the contract classes as violated, and
    with max_violated = 0 it is rejected; one that lands in the 0.7 block is occluded and loses an agreeing view.  So for the other
    frames the test asserts the tightest statement that is true: a pixel's votes differ from the clean scene's only if one of its
    four taps in the corrupted frame lies in a block, and (so that this is not vacuous) some do differ in every frame within the
    window.  DESIGN.md 3.6f says the same."""
    tol = 4 * CLEAN_REL[(N, H, W)]
    frame = N // 2
    clean, bad = _filtered(N, H, W, False, tol), _filtered(N, H, W, True, tol)
    near, far = R.block_mask(H, W)                                          # scaled by 0.7, by 1.4
    kept = np.isfinite(bad["depths"][:, 0])
    assert not kept[frame][near | far].any()
    assert bad["votes"][frame, 0][near | far].max() == 0                    # no neighbour agrees with a block pixel
    assert (bad["votes"][frame, 2][near] > 0).all()                         # a floater: the neighbours see through it
    assert (bad["votes"][frame, 1][far] > 0).all()                          # a hole: the neighbours' wall is in front of it
    # in the corrupted frame nothing outside the blocks changes: not a vote, not a bit of the output
    outside = ~(near | far)
    assert np.array_equal(bad["votes"][frame][:, outside], clean["votes"][frame][:, outside])
    assert np.array_equal(bad["depths"][frame, 0][outside].view(np.int32), clean["depths"][frame, 0][outside].view(np.int32))
    assert np.array_equal(kept[frame][outside], np.isfinite(clean["depths"][frame, 0])[outside])
    # in the other frames a pixel changes only if one of its taps in the corrupted frame lies in a block
    for i in range(N):
        if i == frame:
            continue
        changed = (bad["votes"][i] != clean["votes"][i]).any(0)
        touches = np.zeros((H, W), bool)
        for s in np.nonzero(bad["neighbours"][i] == frame)[0]:
            x0, y0 = bad["x0"][i, s], bad["y0"][i, s]
            for (a0, a1, b0, b1) in R.blocks(H, W):
                touches |= (x0 >= 0) & (y0 + 1 >= a0) & (y0 < a1) & (x0 + 1 >= b0) & (x0 < b1)
        assert not (changed & ~touches).any(), i
        if abs(i - frame) <= 2:
            assert changed.any(), i                                          # (the check is not empty)


# ---- bookkeeping ------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("min_agree,max_violated", [(0, 0), (1, 0), (2, 1), (4, 0)])
def test_stats_rows_add_up(min_agree, max_violated):
    N, H, W = 6, 64, 96
    r = _filtered(N, H, W, True, 0.002, min_agree, max_violated)
    st = r["stats"].astype(np.int64)
    assert np.array_equal(st[:, 0], st[:, 1:].sum(1))
    d = R.corrupt(_scene(N, H, W)[0], N // 2)
    cand = (d[:, 0] > 0) & (d[:, 0] < np.float32(MAX_DEPTH))
    assert np.array_equal(st[:, 0], cand.reshape(N, -1).sum(1))
    assert np.array_equal(st[:, 1], np.isfinite(r["depths"]).reshape(N, -1).sum(1))
    votes = r["votes"].astype(np.int64)
    assert np.array_equal(st[:, 4], (cand & (votes[:, 2] > max_violated)).reshape(N, -1).sum(1))
    assert np.array_equal(np.isfinite(r["depths"][:, 0]), cand & (votes[:, 0] >= min_agree) & (votes[:, 2] <= max_violated))
    assert not votes[~cand[:, None].repeat(3, 1)].any()
    if min_agree == 0:
        assert st[:, 2].sum() == 0 and st[:, 3].sum() == 0                  # nothing can have too few
    else:
        assert st[:, 2].sum() > 0
    if (min_agree, max_violated) == (1, 0):
        assert st[N // 2, 4] > 0 and st[N // 2, 3] > 0                       # the floater is violated, the hole has too few


def test_a_single_frame_has_no_neighbour():
    d, K, M = R.tube_scene(1, 17, 23, SEED)
    cand = (d > 0) & (d < np.float32(MAX_DEPTH))
    a = R.filter_depths(d, K, M, window=2, min_agree=1, max_depth=MAX_DEPTH)
    assert not np.isfinite(a["depths"]).any() and not a["votes"].any()
    assert a["stats"].tolist() == [[int(cand.sum()), 0, int(cand.sum()), 0, 0]]
    b = R.filter_depths(d, K, M, window=2, min_agree=0, max_depth=MAX_DEPTH)
    assert np.array_equal(np.isfinite(b["depths"]), cand) and np.array_equal(b["depths"][cand].view(np.int32), d[cand].view(np.int32))
    assert b["stats"].tolist() == [[int(cand.sum()), int(cand.sum()), 0, 0, 0]]


def test_step_two_uses_every_second_frame():
    assert R.neighbours(9, 2, 2)[4].tolist() == [0, 2, 6, 8]
    assert R.neighbours(9, 2, 2)[1].tolist() == [-1, -1, 3, 5] and R.neighbours(9, 2, 2)[7].tolist() == [3, 5, -1, -1]
    assert R.neighbours(3, 2, 1).tolist() == [[-1, -1, 1, 2], [-1, 0, 2, -1], [0, 1, -1, -1]]
    d, K, M = R.tube_scene(7, 17, 23, SEED)
    kw = dict(window=2, rel_tol=0.01, max_depth=MAX_DEPTH)
    wide = R.filter_depths(d, K, M, step=2, **kw)
    even = R.filter_depths(d[::2], K[::2], M[::2], step=1, **kw)
    for k in ("depths", "votes", "stats"):                                  # the even frames see exactly the even frames
        assert np.array_equal(wide[k][::2], even[k]), k


@pytest.mark.parametrize("window,step", [(4, 1), (2, 3), (16, 1), (1, 1 << 20)])
def test_a_window_that_reaches_past_both_ends(window, step):
    N, H, W = 3, 17, 23
    d, K, M = R.tube_scene(N, H, W, SEED)
    r = R.filter_depths(d, K, M, window=window, step=step, rel_tol=0.02, max_depth=MAX_DEPTH)
    nbr = R.neighbours(N, window, step)
    exist = (nbr >= 0).sum(1)
    assert exist.tolist() == ([2, 2, 2] if step == 1 else [0, 0, 0])
    assert (r["votes"].astype(np.int64).sum(1).reshape(N, -1).max(1) <= exist).all()
    if step == 1:                                                           # the same neighbours as window 2: the same answer
        want = R.filter_depths(d, K, M, window=2, step=1, rel_tol=0.02, max_depth=MAX_DEPTH)
        assert all(np.array_equal(r[k], want[k]) for k in ("depths", "votes", "stats"))
    else:
        assert not np.isfinite(r["depths"]).any()
    assert np.array_equal(R.rel_table(M, window, step)[nbr < 0], np.zeros(((nbr < 0).sum(), 12), np.float32))


def test_relative_transform_maps_frame_i_into_frame_j():
    _, _, M = R.tube_scene(4, 5, 7, SEED)
    T = R.rel_table(M, 1, 1)
    M64 = M.astype(np.float64)
    for i, s, j in ((0, 1, 1), (2, 0, 1), (2, 1, 3)):
        want = np.linalg.inv(M64[j]) @ M64[i]
        got = np.concatenate([T[i, s, :9].reshape(3, 3), T[i, s, 9:].reshape(3, 1)], 1)
        assert np.abs(got - want[:3]).max() < 1e-6                          # (float32 rotations are orthonormal to ~1e-7)
    assert not T[0, 0].any() and not T[3, 1].any()


# ---- the C ABI --------------------------------------------------------------------------------------------------------- #
def test_library_exports_the_entry_points_and_sizes_the_workspace(lib):
    from coivo_amd import _lib
    assert hasattr(lib, "colvo_consistency_workspace_bytes") and hasattr(lib, "colvo_consistency_filter")
    assert lib.colvo_abi_version() == _lib.ABI_VERSION >= 16
    f = lib.colvo_consistency_workspace_bytes
    for bad in ((0, 2), (-1, 2), (65536, 2), (4, 0), (4, -1), (4, 17)):
        assert f(*bad) == 0, bad
    sizes = [f(n, w) for n, w in ((1, 1), (1, 16), (8, 2), (512, 2), (512, 4), (65535, 16))]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(set(sizes))
    assert f(8, 2) >= 8 * 4 * 12 * 4                                        # the transform table
    assert _lib.tune_get("consist_stat_lines") in (1.0, 8.0)


def test_entry_point_refuses_bad_arguments_before_any_hip_call(lib):
    buf = (C.c_double * 66)()
    p = (C.addressof(buf) + 15) & ~15                                       # no call below gets past its checks to touch it
    base = dict(depths=p, K=p, M=p, N=2, H=8, W=8, window=2, step=1, rel_tol=0.01, min_agree=1, max_violated=0, max_depth=10.0, ws=p,
                out_d=p, out_v=p, out_s=p)
    order = ("depths", "K", "M", "N", "H", "W", "window", "step", "rel_tol", "min_agree", "max_violated", "max_depth", "ws", "out_d",
             "out_v", "out_s")

    def refused(what, **kw):
        a = dict(base)
        a.update(kw)
        assert lib.colvo_consistency_filter(*(a[k] for k in order), None) != 0, kw
        msg = lib.colvo_last_error().decode()
        assert msg.startswith("colvo_consistency_filter: ") and what in msg, (kw, msg)

    for k in ("depths", "K", "M", "ws", "out_d", "out_v", "out_s"):
        refused("null pointer", **{k: None})
    for s in (dict(N=0), dict(N=65536), dict(H=0), dict(W=-3), dict(H=1 << 15, W=1 << 15)):
        refused("bad shape", **s)
    for s in (dict(window=0), dict(window=17), dict(window=-2), dict(step=0), dict(step=-1)):
        refused("bad window", **s)
    for s in (dict(min_agree=-1), dict(max_violated=-1), dict(min_agree=5), dict(window=1, min_agree=3)):
        refused("bad policy", **s)
    for s in (dict(rel_tol=0.0), dict(rel_tol=-0.1), dict(rel_tol=float("nan")), dict(rel_tol=float("inf")), dict(max_depth=0.0),
              dict(max_depth=-1.0), dict(max_depth=float("nan")), dict(max_depth=float("inf"))):
        refused("bad tolerance", **s)
    refused("16-byte aligned", ws=p + 8)


def test_kernels_use_no_scratch(lib, tmp_path):
    """The resource metadata of the three kernels: no private segment, no spilled register."""
    import re
    from coivo_amd import build
    asm = open(build.emit_asm("consistency.hip", str(tmp_path / "consistency.s"))).read()
    kernels = re.findall(r"\.name:\s+(\S*k_consist_\w+)", asm)
    assert len(set(kernels)) == 3 and all(any(f"k_consist_{n}" in k for k in kernels) for n in ("rel", "filter", "stats")), kernels
    for key in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count"):
        vals = re.findall(rf"\.{key}:\s+(\d+)", asm)
        assert len(vals) == 3 and all(int(v) == 0 for v in vals), (key, vals)


# ---- Python ------------------------------------------------------------------------------------------------------------ #
def test_filter_depths_argument_errors(lib):
    from coivo_amd import inference as I
    d, K, M = (torch.from_numpy(a) for a in R.tube_scene(2, 8, 8, SEED))
    for bad in (dict(window=0), dict(window=17), dict(window=2.0), dict(step=0), dict(step=-3), dict(min_agree=-1), dict(max_violated=-1),
                dict(min_agree=5), dict(window=1, min_agree=3), dict(rel_tol=0.0), dict(rel_tol=-1.0), dict(rel_tol=float("nan")),
                dict(rel_tol=float("inf")), dict(rel_tol=1e-50), dict(max_depth=0.0), dict(max_depth=float("inf")),
                dict(max_depth=float("nan")), dict(max_depth=1e39), dict(rel_tol=None)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            I.filter_depths(d, K, M, **bad)
    # wrong shapes, dtypes and devices (these tensors live on the CPU: the policy above was refused before that mattered)
    with pytest.raises(ValueError, match="CUDA"):
        I.filter_depths(d, K, M)
    with pytest.raises(ValueError, match=r"\[N,1,H,W\]"):
        I.filter_depths(d[0], K, M)
    with pytest.raises(ValueError):
        I.filter_depths(d.double(), K, M)
    with pytest.raises(ValueError):
        I.filter_depths(d, K[:1], M)
    with pytest.raises(ValueError):
        I.filter_depths(d, K, M[:, :3])


def test_policy_and_result_types():
    from coivo_amd import inference as I
    assert I.Consistency() == (2, 1, 0.01, 1, 0) and I.Consistency._fields == ("window", "step", "rel_tol", "min_agree", "max_violated")
    assert I.ConsistencyResult._fields == ("depths", "votes", "stats")
    r = I.Reconstruction(1, 2, 3, 4)
    assert len(r) == 5 and r.consistency is None and r.polyps is None
    r = I.Reconstruction(1, 2, 3, 4, 5, 6, 7)
    assert tuple(r) == (1, 2, 3, 4, 5) and (r.polyps, r.consistency) == (6, 7)
    r2 = r._replace(points=9)
    assert tuple(r2) == (1, 2, 3, 9, 5) and (r2.polyps, r2.consistency) == (6, 7)
    assert r._replace(consistency=None).consistency is None and r._replace(consistency=None).polyps == 6
    import inspect
    assert inspect.signature(I.reconstruct_sequence).parameters["consistency"].default is None
