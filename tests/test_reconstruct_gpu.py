"""-m gpu: csrc/reconstruct.hip (k_backproject, k_stitch_count, k_stitch_write) and the scan between the stitch's two kernels
(csrc/scan.hip k_scan_top through scan_sums) against the float64 replica tests/reconstruct_ref.py: every coordinate within the
derived bound of its reference, counts, shapes and block offsets exact, nothing written outside the buffers.

Every case prints  RECONSTRUCT_EXACT <kernel> [<case>]: worst error/bound <r> at <index>  (profiles/reconstruct_exact.md)."""
import numpy as np
import pytest
import torch

from tests import reconstruct_ref as R
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

CANARY = 0x7FC0DEAD            # a NaN pattern no arithmetic produces
CANARY_ROWS = 256              # rows of 3 floats behind the points; ints behind the workspace


def _d(a):
    return torch.tensor(np.asarray(a)).to(dev())          # (a copy: the cached cases are read-only)


def _canaried(n, dtype):
    """n elements followed by CANARY_ROWS * 3 canary words, all canary to begin with.  -> (whole int32 view, typed view)"""
    raw = torch.full((n + CANARY_ROWS * 3,), CANARY, dtype=torch.int32, device=dev())
    return raw, raw.view(dtype)


def _report(kernel, case, got, ref, bound):
    r, i = R.worst_ratio(got, ref, bound)
    print(f"RECONSTRUCT_EXACT {kernel} [{case}]: worst error/bound {r:.3f} at {i}")
    return r


def _hold(kernel, case, got, ref, bound):
    """got (float32 NumPy) against the reference: the bound where the reference is finite, the same class where it is not."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    r = _report(kernel, case, got, ref, bound)
    assert R.same_class(got, ref), f"{kernel} [{case}]: a non-finite reference element has another class on the device"
    assert r <= 1.0, f"{kernel} [{case}]: worst error/bound {r}"


# ---- back-projection ------------------------------------------------------------------------------------------------------------ #
def _backproject_entry(depth, K, M):
    """colvo_backproject into a canaried buffer -> points [B,HW,3] float32 NumPy; checks the canary and the inputs."""
    from coivo_amd import _lib
    lib = _lib.load()
    B, _, H, W = depth.shape
    d, k, m = _d(depth), _d(K), _d(M)
    raw, pts = _canaried(B * H * W * 3, torch.float32)
    _lib.check(lib.colvo_backproject(_lib.ptr(d), _lib.ptr(k), _lib.ptr(m), B, H, W, _lib.ptr(pts), _lib.stream_ptr()), "colvo_backproject")
    torch.cuda.synchronize()
    assert bool((raw[B * H * W * 3:] == CANARY).all()), "k_backproject wrote behind B*H*W*3 floats"
    for name, t, a in (("depth", d, depth), ("K", k, K), ("cam2world", m, M)):
        assert np.array_equal(t.cpu().numpy().view(np.int32), np.ascontiguousarray(a).view(np.int32)), f"{name} changed"
    return pts[:B * H * W * 3].cpu().numpy().reshape(B, H * W, 3)


@pytest.mark.parametrize("B,H,W", R.BACKPROJECT_SHAPES)
def test_backproject_within_the_bound(B, H, W):
    from coivo_amd import inference as I
    depth, K, M, ref, bound, _ = R.backproject_case(B, H, W)
    got = _backproject_entry(depth, K, M)
    _hold("k_backproject", f"{B}x{H}x{W}", got, ref, bound)
    wrapped = I.backproject(_d(depth), _d(K), _d(M))
    assert wrapped.shape == (B, H * W, 3) and np.array_equal(wrapped.cpu().numpy().view(np.int32), got.view(np.int32))


@pytest.mark.parametrize("kind", ["finite", "nonfinite"])
def test_backproject_special_depths(kind):
    """finite: 0, -0, negative and subnormal depths, frame 0 under the identity pose (a subnormal depth gives a subnormal point),
    all against the bound.  nonfinite: +inf, -inf, NaN -- the same class as the reference, the bound everywhere else."""
    depth, K, M, ref, bound, pos = R.backproject_case(3, 17, 23, kind)
    got = _backproject_entry(depth, K, M)
    if kind == "finite":
        assert np.isfinite(got).all()
    else:
        assert not np.isfinite(got.reshape(-1, 3)[pos.reshape(-1)]).all(axis=1).any()
    _hold("k_backproject", f"3x17x23 {kind} specials", got, ref, bound)


# ---- stitched cloud --------------------------------------------------------------------------------------------------------------- #
def _stitch_entry(c):
    """colvo_stitch_point_cloud on the case c with canaried points and workspace -> (count, rows [count,3] float32 NumPy,
    workspace [n_blocks] int64 NumPy) after the bounds checks."""
    from coivo_amd import _lib
    lib = _lib.load()
    N, _, H, W = c["depth"].shape
    d, k, m = _d(c["depth"]), _d(c["K"]), _d(c["M"])
    n_ws = int(lib.colvo_stitch_workspace_ints(N, H, W, c["stride"]))
    assert n_ws == c["n_blocks"]
    raw_p, pts = _canaried(c["cap"] * 3, torch.float32)
    raw_w, ws = _canaried(n_ws, torch.int32)
    count = torch.full((3,), CANARY, dtype=torch.int32, device=dev())
    _lib.check(lib.colvo_stitch_point_cloud(_lib.ptr(d), _lib.ptr(k), _lib.ptr(m), N, H, W, c["stride"], float(c["max_depth"]),
                                            _lib.ptr(ws), _lib.ptr(pts), _lib.ptr(count[1:]), _lib.stream_ptr()), "colvo_stitch_point_cloud")
    torch.cuda.synchronize()
    n = int(count[1].item())
    assert int(count[0].item()) == CANARY and int(count[2].item()) == CANARY, "the words around n_points changed"
    assert n == len(c["idx"]), f"n_points {n}, the reference keeps {len(c['idx'])}"
    assert bool((raw_p[n * 3:] == CANARY).all()), "rows >= n_points, or the block behind the cap, were written"
    assert bool((raw_w[n_ws:] == CANARY).all()), "the workspace's tail was written"
    for name, t, a in (("depths", d, c["depth"]), ("K", k, c["K"]), ("cam2world", m, c["M"])):
        assert np.array_equal(t.cpu().numpy().view(np.int32), np.ascontiguousarray(a).view(np.int32)), f"{name} changed"
    return n, pts[:n * 3].cpu().numpy().reshape(n, 3), ws[:n_ws].cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("name,variant,max_depth", R.STITCH_CASES, ids=["-".join(map(str, c)) for c in R.STITCH_CASES])
def test_stitched_cloud_within_the_bound(name, variant, max_depth):
    """The count, every block's offset and every row: row k is the reference's k-th kept sample (tests/test_reconstruct_cpu.py: two
    consecutive ones differ by more than their bounds, so a displaced row cannot pass)."""
    from coivo_amd import inference as I
    c = R.stitch_case(name, variant, max_depth)
    case = f"{name} {variant} max_depth={max_depth} n={c['n_blocks']} per={c['per']}"
    n, rows, ws = _stitch_entry(c)
    # the scan by itself: a wrong offset is named
    want_off = R.exclusive(c["counts"])
    wrong = np.flatnonzero(ws != want_off)
    assert wrong.size == 0, f"k_scan_top [{case}]: offset of block {wrong[0]} is {ws[wrong[0]]}, want {want_off[wrong[0]]} ({wrong.size} wrong)"
    _hold("k_stitch_write", case, rows, c["ref"], c["bound"])
    if variant == "none":
        assert rows.shape == (0, 3)
    if variant == "all":
        assert n == c["cap"]
    # the Python entry returns the same rows
    wrapped = I.stitch_point_cloud(_d(c["depth"]), _d(c["K"]), _d(c["M"]), stride=c["stride"], max_depth=max_depth)
    assert wrapped.shape == (n, 3) and np.array_equal(wrapped.cpu().numpy().view(np.int32), rows.view(np.int32))


# ---- wiring ------------------------------------------------------------------------------------------------------------------------ #
def _bits(t):
    return t.contiguous().view(torch.int32)


def test_views_calls_and_streams_give_the_same_bits():
    from coivo_amd import inference as I
    c = R.stitch_case("n600", "plain")
    depth, K, M = _d(c["depth"]), _d(c["K"]), _d(c["M"])
    N = depth.shape[0]
    want_s = I.stitch_point_cloud(depth, K, M, stride=1)
    want_b = I.backproject(depth, K, M)
    two = torch.stack([depth[:, 0], torch.full_like(depth[:, 0], float("nan"))], dim=1)        # [N,2,H,W]: channel 1 must not be read
    sliced = two[:, :1]
    Kt = K.transpose(1, 2).contiguous().transpose(1, 2)                                        # same values, column-major storage
    assert not sliced.is_contiguous() and not Kt.is_contiguous() and torch.equal(Kt, K)
    assert torch.equal(_bits(I.stitch_point_cloud(sliced, Kt, M, stride=1)), _bits(want_s))
    assert torch.equal(_bits(I.backproject(sliced, Kt, M)), _bits(want_b))
    K1 = K[7:8].expand(N, 3, 3)                                                                # one K for all frames, stride-0 view
    assert torch.equal(_bits(I.stitch_point_cloud(depth, K1, M, stride=1)), _bits(I.stitch_point_cloud(depth, K1.contiguous(), M, stride=1)))
    assert torch.equal(_bits(I.backproject(depth, K1, M)), _bits(I.backproject(depth, K1.contiguous(), M)))
    assert torch.equal(_bits(I.stitch_point_cloud(depth, K, M, stride=1)), _bits(want_s))     # a second call
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got_s = I.stitch_point_cloud(depth, K, M, stride=1)
        got_b = I.backproject(depth, K, M)
    side.synchronize()
    assert torch.equal(_bits(got_s), _bits(want_s)) and torch.equal(_bits(got_b), _bits(want_b))


def test_reconstruct_sequence_is_held_to_the_replica():
    """12 frames of 64x96 at stride 1: 12 * 24 = 288 blocks, per == 2 in the scan, per-frame K with fx != fy.  The cloud is within the
    bound of the replica evaluated on the depths, the K and the float32 trajectory the call itself used; with a Consistency policy
    the +inf of filter_depths reach the stitch through the real path."""
    from coivo_amd import inference as I, nn as hnn, synth
    from oracle import colvo_spec as S
    dn_o, pn_o = S.make_models(31)
    dn, pn = hnn.DepthNet(), hnn.PoseNet()
    dn.load_state_dict(dn_o.state_dict())
    pn.load_state_dict(pn_o.state_dict())
    n, H, W = 12, 64, 96
    frames = synth.make_batch(n, H, W, seed=31)["tgt"].to(dev())
    K = R.intrinsics(np.random.default_rng(31), n, H, W)
    assert R.n_blocks(n, H, W, 1) == 288
    for policy in (None, I.Consistency(window=2, rel_tol=0.01, min_agree=1)):
        rec = I.reconstruct_sequence(dn, pn, frames, _d(K), stride=1, chunk=4, consistency=policy)
        depths = rec.depths if policy is None else rec.consistency.depths
        M = rec.cam2world.float().numpy()
        idx, ref, bound = R.stitch(depths.cpu().numpy(), K, M, 1, I.MAX_DEPTH)
        got = rec.points.cpu().numpy()
        assert got.shape == ref.shape and got.shape[0] > 0
        if policy is not None:
            n_inf = int(torch.isinf(depths).sum().item())
            assert 0 < n_inf < depths.numel() and got.shape[0] < depths.numel()
        _hold("reconstruct_sequence", "12x64x96 stride 1" + ("" if policy is None else " consistency"), got, ref, bound)


def test_memory_discipline():
    """backproject and stitch_point_cloud under tests/guarded.py: depths, intrinsics and poses between guard bands; the points, the
    count and the block workspace (colvo_stitch_workspace_ints) from the pool under both poisons.  Outputs hold the replica's bound as
    above, are the same bytes under either poison, and no guard byte changes.  Launches reached: k_backproject at 3 x 17 x 23 (a ragged
    last block); k_stitch_count, k_scan_top and k_stitch_write at n600 (300 frames of 17 x 23: 600 blocks, three per thread of the
    scan's top-level workgroup, the last share ragged)."""
    from coivo_amd import _lib, inference as I
    from tests import guarded as G
    depth, K, M, ref, bound, _ = R.backproject_case(3, 17, 23)
    outs, pools = G.under_both_poisons(dev(), lambda pool: I.backproject(pool.place(_d(depth)), pool.place(_d(K)), pool.place(_d(M))),
                                       "backproject")
    for got, pool in zip(outs, pools):
        _hold("k_backproject", "3x17x23 guarded", got.cpu().numpy(), ref, bound)
        G.assert_served(pool, 0, 3 * 17 * 23 * 3 * 4, "backproject")
    c = R.stitch_case("n600", "plain")
    assert c["n_blocks"] == 600 > 256
    outs, pools = G.under_both_poisons(dev(), lambda pool: I.stitch_point_cloud(pool.place(_d(c["depth"])), pool.place(_d(c["K"])),
                                                                                pool.place(_d(c["M"])), stride=c["stride"],
                                                                                max_depth=c["max_depth"]), "stitch_point_cloud")
    N, _, H, W = c["depth"].shape
    for got, pool in zip(outs, pools):
        assert got.shape == (len(c["idx"]), 3)
        _hold("k_stitch_write", "n600 plain guarded", got.cpu().numpy(), c["ref"], c["bound"])
        G.assert_served(pool, 0, 4 * int(_lib.load().colvo_stitch_workspace_ints(N, H, W, c["stride"])), "stitch_point_cloud")
