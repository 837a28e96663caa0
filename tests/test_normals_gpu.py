"""-m gpu: the normals of a fused cloud (coivo_amd.inference.cloud_normals, csrc/normals.hip) against their NumPy replica
(tests/normals_ref.py).  The arithmetic is pinned (float32, one rounding per operation, denormals kept), the sums are integers and the
write-out is float64, so every comparison here is equality to the bit: no tolerance, no excused row."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import consistency_ref as CR
from tests import normals_ref as NR
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

MAX_DEPTH = 4.5
SEED = 5
TUBE_GRID = dict(voxel_size=0.02, origin=(-1.28, -1.28, -0.64), dims=(128, 128, 320))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _fuse(d, K, M, *, stride=1, min_obs=1, grid=TUBE_GRID, max_depth=MAX_DEPTH):
    from coivo_amd import inference as I
    return I.fuse_point_cloud(_t(d), _t(K), _t(M), stride=stride, max_depth=max_depth, min_obs=min_obs, **(grid or dict(voxel_size=0.05)))


def _want(fused, d, K, M, *, stride=1, rel_edge=0.05, max_depth=MAX_DEPTH):
    return NR.cloud_normals(d, K, M, fused.voxels.cpu().numpy(), stride=stride, max_depth=max_depth, voxel_size=fused.voxel_size,
                            origin=fused.origin, dims=fused.dims, rel_edge=rel_edge)


def _assert_equal(got, want, what=""):
    m = want["counts"].shape[0]
    assert got.normals.is_cuda and got.normals.dtype == torch.float32 and got.normals.shape == (m, 3), what
    assert got.counts.dtype == torch.int32 and got.counts.shape == (m,) and got.coherence.dtype == torch.float32, what
    assert got.coherence.shape == (m,) and got.stats.dtype == torch.int32 and got.stats.shape == (4,), what
    assert got.stats.cpu().tolist() == want["stats"].tolist(), (what, got.stats.cpu().tolist(), want["stats"].tolist())
    assert torch.equal(got.counts.cpu(), torch.from_numpy(want["counts"])), what
    for name in ("normals", "coherence"):
        g, w = _bits(getattr(got, name).cpu()), _bits(torch.from_numpy(want[name]))
        assert torch.equal(g, w), (what, name, int((g != w).sum()))


def _check(d, K, M, *, stride=1, min_obs=1, rel_edge=0.05, grid=TUBE_GRID, what=""):
    from coivo_amd import inference as I
    fused = _fuse(d, K, M, stride=stride, min_obs=min_obs, grid=grid)
    got = I.cloud_normals(fused, _t(d), _t(K), _t(M), stride=stride, max_depth=MAX_DEPTH, rel_edge=rel_edge)
    want = _want(fused, d, K, M, stride=stride, rel_edge=rel_edge)
    _assert_equal(got, want, what)
    return fused, got, want


@functools.lru_cache(maxsize=None)
def _tube(H, W):
    return CR.tube_scene(5, H, W, SEED)


# ---- the tube ---------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("min_obs", [1, 2])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("H,W", [(17, 23), (64, 96)])
def test_tube_equals_the_replica(H, W, stride, min_obs):
    d, K, M = _tube(H, W)
    rel_edge = 0.05 if H == 64 else 0.2          # 23 pixels across a tube: neighbouring depths differ by more than 5 %
    fused, got, want = _check(d, K, M, stride=stride, min_obs=min_obs, rel_edge=rel_edge, what=(H, W, stride, min_obs))
    kept, normal, matched, unmatched = want["stats"].tolist()
    assert kept == fused.n_input and normal > kept // 2 and matched + unmatched == normal and fused.n_outside == 0
    assert (unmatched > 0) == (min_obs == 2) and matched > 0
    if (H, stride, min_obs) == (64, 1, 1):
        # both ends of the binary search: the first and the last row of the cloud are hit
        assert want["counts"][0] > 0 and want["counts"][-1] > 0 and (want["counts"] > 0).all()
        assert float(got.coherence.min()) > 0.999


# ---- tails ------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("H,W", [(1, 1), (1, 70), (2, 2)])
def test_image_tails_where_every_difference_is_one_sided_or_missing(H, W):
    rng = np.random.default_rng(H * 100 + W)
    N = 3
    d = rng.uniform(1.0, 1.1, (N, 1, H, W)).astype(np.float32)
    K = np.zeros((N, 3, 3), np.float32)
    K[:, 0, 0] = K[:, 1, 1] = 30.0
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = (W - 1) / 2, (H - 1) / 2, 1
    _, _, M = CR.tube_scene(N, 8, 8, SEED)
    for stride in (1, 2):
        fused, got, want = _check(d, K, M, stride=stride, grid=None, what=(H, W, stride))
        assert want["stats"][0] == N * -(-H // stride) * -(-W // stride)
        # a row or a column of one pixel has no tangent along the other axis: no normal at all; 2 x 2 has one-sided ones everywhere
        assert (want["stats"][1] > 0) == ((H, W) == (2, 2))
        assert fused.points.shape[0] > 0 and (H > 1 or not want["counts"].any())


def test_clouds_of_no_row_and_of_one_row():
    from coivo_amd import inference as I
    d, K, M = _tube(64, 96)
    dt, Kt, Mt = _t(d), _t(K), _t(M)
    full = _fuse(d, K, M)
    none = _fuse(d, K, M, min_obs=1000)
    assert none.points.shape[0] == 0
    got = I.cloud_normals(none, dt, Kt, Mt, max_depth=MAX_DEPTH)
    want = _want(none, d, K, M)
    _assert_equal(got, want, "M = 0")
    assert want["stats"][2] == 0 and want["stats"][3] == want["stats"][1] > 0
    ref = _want(full, d, K, M)
    m = full.points.shape[0]
    for row in (0, m // 2, m - 1):
        one = full._replace(points=full.points[row:row + 1], counts=full.counts[row:row + 1], voxels=full.voxels[row:row + 1].contiguous())
        got = I.cloud_normals(one, dt, Kt, Mt, max_depth=MAX_DEPTH)
        _assert_equal(got, _want(one, d, K, M), ("M = 1", row))
        assert torch.equal(_bits(got.normals.cpu()), _bits(torch.from_numpy(ref["normals"][row:row + 1]))) and int(got.counts[0]) > 0


# ---- hostile values ---------------------------------------------------------------------------------------------------- #
def test_hostile_depths():
    d, K, M = _tube(64, 96)
    d = d.copy()
    nan, inf = np.nan, np.inf
    d[0, 0, 10, 10:17] = [nan, inf, -inf, 0.0, -0.0, -1.0, 1e-30]
    d[1, 0, 20:23, 30:33] = 1e-30          # every product underflows to zero: no normal
    d[2, 0, 30:34, 40:44] = 1e-8           # the squares of the cross product are float32 denormals: the build keeps them, as NumPy does
    d[3, 0, 0, 0], d[3, 0, 63, 95], d[3, 0, 0, 95] = nan, inf, 1e-30
    d[4, 0, 40:44, 50] = [3.4e38, 4.4999995, 4.5, 1e-45]
    fused, got, want = _check(d, K, M, what="hostile depths")
    s = NR.sample_normals(d, K, M, max_depth=MAX_DEPTH)
    assert not s["normal"][1, 20:23, 30:33].any() and s["kept"][1, 20:23, 30:33].all()
    assert s["normal"][2, 31:33, 41:43].all()
    assert want["stats"][1] < want["stats"][0] and torch.isfinite(got.normals).all() and torch.isfinite(got.coherence).all()


def test_a_negative_focal_length():
    d, K, M = _tube(64, 96)
    K = K.copy()
    K[1, 0, 0] = -K[1, 0, 0]               # the image is mirrored, the cross product changes sign, the facing rule turns it back
    K[3, 1, 1] = -K[3, 1, 1]
    _, _, want = _check(d, K, M, what="negative focal length")
    assert want["stats"][1] == want["stats"][0] and want["stats"][2] > 0


# ---- determinism ------------------------------------------------------------------------------------------------------- #
def test_two_streams_and_the_frame_order_reversed_give_the_same_bits():
    from coivo_amd import inference as I
    d, K, M = _tube(64, 96)
    fused = _fuse(d, K, M, min_obs=2)
    args = (_t(d), _t(K), _t(M))
    a = I.cloud_normals(fused, *args, max_depth=MAX_DEPTH)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        b = I.cloud_normals(fused, *args, max_depth=MAX_DEPTH)
    side.synchronize()
    rev = tuple(t.flip(0).contiguous() for t in args)
    fused_rev = _fuse(d[::-1], K[::-1], M[::-1], min_obs=2)
    assert torch.equal(fused_rev.voxels, fused.voxels)
    c = I.cloud_normals(fused_rev, *rev, max_depth=MAX_DEPTH)
    for other in (b, c):
        assert torch.equal(_bits(a.normals), _bits(other.normals)) and torch.equal(a.counts, other.counts)
        assert torch.equal(_bits(a.coherence), _bits(other.coherence)) and torch.equal(a.stats, other.stats)
    _assert_equal(a, _want(fused, d, K, M))


# ---- refusals ---------------------------------------------------------------------------------------------------------- #
def test_argument_errors_on_the_device_path_launch_nothing():
    from coivo_amd import _lib, inference as I
    lib = _lib.load()
    d, K, M = _tube(17, 23)
    dt, Kt, Mt = _t(d), _t(K), _t(M)
    fused = _fuse(d, K, M)
    m = fused.points.shape[0]
    scratch = torch.empty(int(lib.colvo_cloud_normals_scratch_bytes(m)), device=dev(), dtype=torch.uint8)
    outs = [torch.full((m, 3), 7.0, device=dev()), torch.full((m,), 7, device=dev(), dtype=torch.int32), torch.full((m,), 7.0, device=dev()),
            torch.full((4,), 7, device=dev(), dtype=torch.int32)]
    good = dict(N=5, H=17, W=23, stride=1, max_depth=MAX_DEPTH, vs=fused.voxel_size, dims=fused.dims, M=m, rel_edge=0.05, scratch=scratch.data_ptr(),
                voxels=fused.voxels.data_ptr())

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.colvo_cloud_normals(dt.data_ptr(), Kt.data_ptr(), Mt.data_ptr(), a["N"], a["H"], a["W"], a["stride"], a["max_depth"],
                                       *fused.origin, a["vs"], *a["dims"], a["voxels"], a["M"], a["rel_edge"], a["scratch"],
                                       *(o.data_ptr() for o in outs), _lib.stream_ptr())

    for kw in (dict(M=-1), dict(N=0), dict(N=65536), dict(stride=0), dict(dims=(8, 12, 8)), dict(vs=0.0), dict(max_depth=float("nan")),
               dict(rel_edge=0.0), dict(rel_edge=float("inf")), dict(rel_edge=float("nan")), dict(scratch=scratch.data_ptr() + 4),
               dict(voxels=0), dict(scratch=0)):
        assert call(**kw) != 0 and lib.colvo_last_error().startswith(b"colvo_cloud_normals:"), (kw, lib.colvo_last_error())
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    assert call() == 0
    torch.cuda.synchronize()
    assert outs[3].tolist() == I.cloud_normals(fused, dt, Kt, Mt, max_depth=MAX_DEPTH).stats.tolist()
    for bad in ((dt.cpu(), Kt, Mt), (dt.double(), Kt, Mt), (dt, Kt[:2], Mt), (dt, Kt, Mt[:, :3])):
        with pytest.raises(ValueError):
            I.cloud_normals(fused, *bad, max_depth=MAX_DEPTH)
    with pytest.raises(ValueError, match="voxels"):
        I.cloud_normals(fused._replace(voxels=fused.voxels.cpu()), dt, Kt, Mt, max_depth=MAX_DEPTH)


# ---- memory discipline ------------------------------------------------------------------------------------------------- #
def test_memory_discipline():
    """cloud_normals under tests/guarded.py on the 5 x 17 x 23 tube, stride 2, a cloud of min_obs = 2 (matched and unmatched samples):
    depths, intrinsics, poses and the cloud's tensors between guard bands -- a one-sided difference at the first or last image row of
    frame 0 or 4 borders a guard --; the scratch (colvo_cloud_normals_scratch_bytes: the integer sums per row), normals, counts,
    coherence and statistics from the pool under both poisons.  Outputs equal the replica, are the same bytes under either poison, and
    no guard byte changes.  Launches reached: the clearing of the sums, the sample pass with its binary search and the write-out."""
    from coivo_amd import _lib, inference as I
    from tests import guarded as G
    d, K, M = _tube(17, 23)
    fused = _fuse(d, K, M, stride=2, min_obs=2)
    want = _want(fused, d, K, M, stride=2, rel_edge=0.2)
    assert want["stats"][2] > 0 and want["stats"][3] > 0
    run = lambda pool: I.cloud_normals(pool.place_tree(fused), pool.place(_t(d)), pool.place(_t(K)), pool.place(_t(M)), stride=2,
                                       max_depth=MAX_DEPTH, rel_edge=0.2)
    outs, pools = G.under_both_poisons(dev(), run, "cloud_normals")
    for got, pool in zip(outs, pools):
        _assert_equal(got, want, "guarded")
        G.assert_served(pool, 0, _lib.load().colvo_cloud_normals_scratch_bytes(fused.voxels.shape[0]), "cloud_normals")
