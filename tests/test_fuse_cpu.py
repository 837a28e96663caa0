"""CPU checks of the voxel fusion (coivo_amd.inference.fuse_point_cloud, csrc/fuse.hip): the NumPy replica the GPU tests compare
with (tests/fuse_ref.py) against answers written down by hand and against the float64 oracle, the C ABI's refusals before any
HIP call, the default grid rule and the PLY writer."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from coivo_amd.inference import FusedCloud, fuse_point_cloud, fusion_grid, write_ply  # noqa: F401  (what this file is about)
from tests import fuse_ref as R

MAX_DEPTH = 4.5
SCENES = [(3, 17, 23, 0.25), (4, 64, 96, 0.125), (8, 256, 320, 0.05), (8, 256, 320, 0.02)]


@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.build()
    return _lib.load()


# ---- the replica ------------------------------------------------------------------------------------------------------- #
def _hand_scene():
    """Identity rotation, fx = fy = 64, cx = cy = 0, one row of 33 pixels walked with stride 8 (u = 0, 8, 16, 24, 32), depth 2:
    X = u / 32, Y = 0, Z = 2.  Frame 1 is shifted by (0.125, 0, 0.25).  Voxels of 0.5 from the origin: g_x = u / 16 (+ 0.25),
    g_z = 4 (4.5): every quantity is exact."""
    depths = np.full((2, 1, 1, 33), 2.0, np.float32)
    K = np.broadcast_to(np.array([[64.0, 0, 0], [0, 64.0, 0], [0, 0, 1]], np.float32), (2, 3, 3)).copy()
    M = np.broadcast_to(np.eye(4, dtype=np.float32), (2, 4, 4)).copy()
    M[1, :3, 3] = (0.125, 0.0, 0.25)
    colors = np.empty((2, 3, 1, 33), np.float32)
    colors[0] = np.array([51, 102, 255], np.float32)[:, None, None] / np.float32(255)
    colors[1] = np.array([0, 153, 255], np.float32)[:, None, None] / np.float32(255)
    return depths, colors, K, M, dict(stride=8, max_depth=10.0, voxel_size=0.5, origin=(0.0, 0.0, 0.0), dims=(8, 8, 8))


def test_replica_gives_the_hand_computed_answer():
    depths, colors, K, M, kw = _hand_scene()
    r = R.fuse(depths, colors, K, M, min_obs=1, **kw)
    assert (r["n_input"], r["n_outside"], r["n_bricks"], r["n_voxels"], r["max_count"]) == (10, 0, 1, 3, 4)
    # frame 0: g_x = 0, .5, 1, 1.5, 2 -> voxels 0 0 1 1 2, quanta 0 128 0 128 0; frame 1: + .25 -> same voxels, quanta 64 192 64 192 64
    # g_z = 4 (quantum 0) and 4.5 (quantum 128); g_y = 0
    assert r["voxels"].tolist() == [[0, 0, 4], [1, 0, 4], [2, 0, 4]]
    assert r["counts"].tolist() == [4, 4, 2]
    # mean = origin + (i + (sum q + n / 2) / (256 n)) * 0.5: sum q_x = 384, 384, 64; sum q_y = 0; sum q_z = 256, 256, 128
    want = [[(0 + 386 / 1024) * 0.5, (2 / 1024) * 0.5, (4 + 258 / 1024) * 0.5],
            [(1 + 386 / 1024) * 0.5, (2 / 1024) * 0.5, (4 + 258 / 1024) * 0.5],
            [(2 + 65 / 512) * 0.5, (1 / 512) * 0.5, (4 + 129 / 512) * 0.5]]
    assert r["points"].tolist() == want                                   # all exactly representable
    # colour sums: red 51 + 51 + 0 + 0 = 102 of 4 * 255, green 102 * 2 + 153 * 2 = 510, blue 4 * 255; last voxel one sample a frame
    wc = np.array([[102 / 1020, 510 / 1020, 1.0], [102 / 1020, 510 / 1020, 1.0], [51 / 510, 255 / 510, 1.0]]).astype(np.float32)
    assert np.array_equal(r["colors"], wc)
    r2 = R.fuse(depths, colors, K, M, min_obs=3, **kw)
    assert r2["voxels"].tolist() == [[0, 0, 4], [1, 0, 4]] and r2["n_voxels"] == 3
    # a tighter grid: x from 0.5 on loses the four samples of voxel 0 (counted outside), and what was voxel 1 is voxel 0
    r3 = R.fuse(depths, None, K, M, min_obs=1, **dict(kw, origin=(0.5, 0.0, 0.0)))
    assert (r3["n_input"], r3["n_outside"]) == (10, 4) and r3["voxels"].tolist() == [[0, 0, 4], [1, 0, 4]] and r3["colors"] is None
    assert r3["points"][:, 0].tolist() == [0.5 + (0 + 386 / 1024) * 0.5, 0.5 + (1 + 65 / 512) * 0.5]


def test_replica_drops_what_the_contract_drops():
    depths, colors, K, M, kw = _hand_scene()
    depths[0, 0, 0, 0] = np.nan
    depths[0, 0, 0, 8] = 0.0
    depths[0, 0, 0, 16] = -2.0
    depths[0, 0, 0, 24] = 10.0            # exactly max_depth
    depths[0, 0, 0, 32] = np.inf
    colors[1, 0] = np.nan                 # -> quantum 0
    colors[1, 1] = 7.0                    # -> 255
    colors[1, 2] = -3.0                   # -> 0
    r = R.fuse(depths, colors, K, M, min_obs=1, **kw)
    assert (r["n_input"], r["n_outside"]) == (5, 0) and r["counts"].tolist() == [2, 2, 1]
    assert np.array_equal(r["colors"], np.array([[0, 1, 0]] * 3, np.float32))


@pytest.mark.parametrize("N,H,W,voxel", SCENES[:3])
def test_replica_invariants(N, H, W, voxel):
    from coivo_amd import inference as I
    depths, colors, K, M = R.scene(N, H, W, 5)
    origin, dims = I.fusion_grid(torch.from_numpy(K), torch.from_numpy(M), H, W, voxel, MAX_DEPTH)
    kw = dict(stride=1, max_depth=MAX_DEPTH, voxel_size=voxel, origin=origin, dims=dims)
    a = R.fuse(depths, colors, K, M, min_obs=1, **kw)
    assert a["n_input"] - a["n_outside"] == int(a["counts"].astype(np.int64).sum())
    assert a["counts"].shape[0] == a["n_voxels"] and int(a["counts"].max()) == a["max_count"]
    nb = [d // 8 for d in dims]
    v = a["voxels"].astype(np.int64)
    key = (((v[:, 2] // 8) * nb[1] + v[:, 1] // 8) * nb[0] + v[:, 0] // 8) * 512 + ((v[:, 2] % 8) * 8 + v[:, 1] % 8) * 8 + v[:, 0] % 8
    assert np.all(np.diff(key) > 0)                                        # ascending (brick, local), no voxel twice
    lo = np.array(origin)[None] + v * np.float32(voxel).astype(np.float64)
    assert np.all(a["points"] >= lo.astype(np.float32)) and np.all(a["points"] <= (lo + np.float64(np.float32(voxel))).astype(np.float32))
    assert a["colors"].min() >= 0.0 and a["colors"].max() <= 1.0
    # min_obs only removes rows
    b = R.fuse(depths, colors, K, M, min_obs=2, **kw)
    keep = a["counts"] >= 2
    assert 0 < keep.sum() < keep.size
    for k in ("points", "colors", "counts", "voxels"):
        assert np.array_equal(a[k][keep].view(np.int32), b[k].view(np.int32)), k
    assert all(a[k] == b[k] for k in ("n_input", "n_outside", "n_bricks", "n_voxels"))
    # the order of the frames leaves every bit unchanged
    perm = np.random.default_rng(1).permutation(N)
    c = R.fuse(depths[perm], colors[perm], K[perm], M[perm], min_obs=1, **kw)
    for k in ("points", "colors", "counts", "voxels"):
        assert np.array_equal(a[k].view(np.int32), c[k].view(np.int32)), k


@pytest.mark.parametrize("N,H,W,voxel", SCENES)
def test_replica_voxels_agree_with_the_float64_oracle(N, H, W, voxel):
    """Something the replica shares no code with: the oracle's backproject in float64.  Every sample whose float64 grid
    coordinate lies at least 1e-3 voxel from a voxel face must land in floor() of it; the samples left out (nearer to a face
    than float32 can be trusted to resolve) may be at most 1 %."""
    from oracle import colvo_spec as S
    depths, _, K, M = R.scene(N, H, W, 5)
    origin = np.array([-6.0, -6.0, -6.0], np.float32)
    P64 = S.backproject(torch.from_numpy(depths).double(), torch.from_numpy(K).double(), torch.from_numpy(M).double()).numpy()
    g64 = (P64.reshape(-1, 3) - origin.astype(np.float64)) / np.float64(np.float32(voxel))
    _, g = R.grid_coords(depths, K, M, 1, origin, voxel)
    g32 = np.stack([x.reshape(-1) for x in g], 1)
    frac = g64 - np.floor(g64)
    near = (np.minimum(frac, 1.0 - frac) < 1e-3).any(1)
    print(f"{(N, H, W, voxel)}: {near.mean():.4%} of the samples within 1e-3 voxel of a face; largest |g32 - g64| "
          f"{np.abs(g32 - g64).max():.2e} voxel")
    assert near.mean() <= 0.01
    assert np.array_equal(np.floor(g32)[~near], np.floor(g64)[~near])


# ---- the grid rule ----------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("N,H,W,voxel", SCENES)
def test_default_grid_contains_every_sample(N, H, W, voxel):
    from coivo_amd import inference as I
    depths, _, K, M = R.scene(N, H, W, 5)
    origin, dims = I.fusion_grid(torch.from_numpy(K), torch.from_numpy(M), H, W, voxel, MAX_DEPTH)
    assert len(origin) == 3 and len(dims) == 3 and all(isinstance(d, int) and d > 0 and d % 8 == 0 for d in dims)
    assert all(float(np.float32(o)) == o for o in origin)
    r = R.fuse(depths, None, K, M, stride=1, max_depth=MAX_DEPTH, voxel_size=voxel, origin=origin, dims=dims)
    assert r["n_outside"] == 0 and r["n_input"] > 0.8 * depths.size
    # ... and is no larger than the cameras' span plus the reach of the farthest corner ray on either side (+ a voxel and a brick)
    span = M[:, :3, 3].max(0) - M[:, :3, 3].min(0)
    ray = np.sqrt(1 + (max(K[0, 0, 2], W - 1 - K[0, 0, 2]) / K[0, 0, 0]) ** 2 + (max(K[0, 1, 2], H - 1 - K[0, 1, 2]) / K[0, 1, 1]) ** 2)
    for a in range(3):
        assert dims[a] * voxel <= span[a] + 2 * (MAX_DEPTH * ray + voxel) + 2 * 8 * voxel + 1e-6
    with pytest.raises(ValueError):
        I.fusion_grid(torch.from_numpy(K), torch.from_numpy(M), H, W, 0.0, MAX_DEPTH)


# ---- the C ABI --------------------------------------------------------------------------------------------------------- #
def test_size_functions(lib):
    f = lib.colvo_fuse_plan_workspace_bytes
    for bad in ((0, 8, 8, 1, 8, 8, 8), (65536, 8, 8, 1, 8, 8, 8), (1, 0, 8, 1, 8, 8, 8), (1, 8, -1, 1, 8, 8, 8), (1, 8, 8, 0, 8, 8, 8),
                (1, 1 << 15, 1 << 15, 1, 8, 8, 8), (65535, 1 << 14, 1 << 14, 1, 8, 8, 8), (1, 8, 8, 1, 0, 8, 8), (1, 8, 8, 1, 8, 12, 8),
                (1, 8, 8, 1, 8, 8, -8), (1, 8, 8, 1, 1 << 13, 1 << 13, 1 << 11)):
        assert f(*bad) == 0, bad
    sizes = [f(2, 64, 96, 1, n, n, n) for n in (8, 16, 64, 512, 1024)]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(set(sizes))
    assert f(2, 64, 96, 1, 512, 512, 512) >= 4 * 64 ** 3                     # a table entry per brick
    assert f(1, 8, 8, 1, 1 << 12, 1 << 12, 1 << 10) > 0                      # 2^27 bricks: allowed
    for g in (lib.colvo_fuse_pool_bytes, lib.colvo_fuse_extract_workspace_bytes):
        assert g(0) == 0 and g(-1) == 0 and g(1 << 22) == 0
        s = [g(n) for n in (1, 100, 7428, 1 << 20, (1 << 22) - 1)]
        assert all(x > 0 and x % 16 == 0 for x in s) and s == sorted(set(s))
    assert lib.colvo_fuse_pool_bytes(7428) == 7428 * 512 * 32


def test_entry_points_refuse_bad_arguments_before_any_hip_call(lib):
    buf = (C.c_double * 66)()
    p = (C.addressof(buf) + 15) & ~15                                       # no call below gets past its checks to touch it
    geom = dict(N=2, H=8, W=8, stride=1, max_depth=10.0, ox=0.0, oy=0.0, oz=0.0, vs=0.1, nx=8, ny=16, nz=8)
    G = ("N", "H", "W", "stride", "max_depth", "ox", "oy", "oz", "vs", "nx", "ny", "nz")
    grid = ("ox", "oy", "oz", "vs", "nx", "ny", "nz")

    def plan(**kw):
        a = dict(geom, depths=p, K=p, M=p, ws=p, stats=p)
        a.update(kw)
        return lib.colvo_fuse_plan(a["depths"], a["K"], a["M"], *(a[k] for k in G), a["ws"], a["stats"], None)

    def accumulate(**kw):
        a = dict(geom, depths=p, colors=None, K=p, M=p, ws=p, n_bricks=1, pool=p)
        a.update(kw)
        return lib.colvo_fuse_accumulate(a["depths"], a["colors"], a["K"], a["M"], *(a[k] for k in G), a["ws"], a["n_bricks"], a["pool"], None)

    def count(**kw):
        a = dict(pool=p, n_bricks=1, min_obs=1, ews=p, stats=p)
        a.update(kw)
        return lib.colvo_fuse_count(a["pool"], a["n_bricks"], a["min_obs"], a["ews"], a["stats"], None)

    def write(**kw):
        a = dict(geom, ws=p, pool=p, n_bricks=1, min_obs=1, ews=p, n_rows=1, points=p, colors=None, counts=p, voxels=p)
        a.update(kw)
        return lib.colvo_fuse_write(a["ws"], a["pool"], a["n_bricks"], a["min_obs"], *(a[k] for k in grid), a["ews"], a["n_rows"], a["points"],
                                    a["colors"], a["counts"], a["voxels"], None)

    def refused(fn, name, what, **kw):
        assert fn(**kw) != 0, (name, kw)
        msg = lib.colvo_last_error().decode()
        assert msg.startswith(name + ": ") and what in msg, (name, kw, msg)

    shapes = (dict(N=0), dict(N=65536), dict(H=0), dict(W=-3), dict(stride=0), dict(H=1 << 15, W=1 << 15),
              dict(N=65535, H=1 << 14, W=1 << 14))
    grids = (dict(nx=0), dict(ny=12), dict(nz=-8), dict(vs=0.0), dict(vs=-1.0), dict(vs=float("nan")), dict(vs=float("inf")),
             dict(ox=float("nan")), dict(oz=float("inf")), dict(nx=1 << 13, ny=1 << 13, nz=1 << 11), dict(vs=1e-45))
    bricks = (dict(n_bricks=0), dict(n_bricks=-1), dict(n_bricks=1 << 22))
    for fn, name, ptrs in ((plan, "colvo_fuse_plan", ("depths", "K", "M", "ws", "stats")),
                           (accumulate, "colvo_fuse_accumulate", ("depths", "K", "M", "ws", "pool")),
                           (count, "colvo_fuse_count", ("pool", "ews", "stats")),
                           (write, "colvo_fuse_write", ("ws", "pool", "ews", "points", "counts", "voxels"))):
        for k in ptrs:
            refused(fn, name, "null pointer", **{k: None})
        for k in [x for x in ptrs if x in ("ws", "pool", "ews")]:
            refused(fn, name, "16-byte aligned", **{k: p + 8})
        if fn in (plan, accumulate):
            for s in shapes:
                refused(fn, name, "bad shape", **s)
        if fn is not count:
            for g in grids:
                refused(fn, name, "bad grid", **g)
        if fn is not plan:
            for b in bricks:
                refused(fn, name, "bad grid", **b)
        if fn in (count, write):
            refused(fn, name, "bad grid", min_obs=0)
    refused(accumulate, "colvo_fuse_accumulate", "bad grid", n_bricks=3, nx=8, ny=8, nz=16)      # more bricks than the grid has
    refused(write, "colvo_fuse_write", "bad grid", n_bricks=3, nx=8, ny=8, nz=16)
    for n_rows in (0, -1, 513):                                                                   # more rows than one brick has voxels
        refused(write, "colvo_fuse_write", "bad shape", n_rows=n_rows)


def test_tuning_entries_and_isa(lib, tmp_path):
    """The developer switches of the fusion live in the one tuning table; every add of fuse.hip is a native atomic (no
    compare-and-swap loop) and no kernel spills."""
    from coivo_amd import _lib, build
    assert _lib.tune_get("fuse_agg_rounds") == 64 and _lib.tune_get("fuse_row_adds") == 1 and _lib.tune_get("fuse_count_limit") == 2 ** 24
    asm = open(build.emit_asm("fuse.hip", str(tmp_path / "fuse.s"))).read()
    assert "cmpswap" not in asm
    assert asm.count("global_atomic_add_x2") >= 5 and "ds_add_u64" in asm
    # its own five kernels, and the four of the ordered scan it numbers bricks and rows with (csrc/scan.hip)
    for listing, prefix, n in ((asm, "k_fuse", 5), (open(build.emit_asm("scan.hip", str(tmp_path / "scan.s"))).read(), "k_scan", 4)):
        kernels = re.findall(rf"\.name:\s+(\S*{prefix}\S*)", listing)
        assert len(kernels) >= n, kernels
        for key in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count"):
            vals = re.findall(rf"\.{key}:\s+(\d+)", listing)
            assert len(vals) >= n and all(int(v) == 0 for v in vals), (key, vals)
        assert not re.search(r"\bscratch_(load|store)", listing)


# ---- Python ------------------------------------------------------------------------------------------------------------ #
def test_fuse_point_cloud_refuses_cpu_tensors():
    from coivo_amd import inference as I
    depths, colors, K, M = (torch.from_numpy(a) for a in R.scene(2, 8, 8, 5))
    with pytest.raises(ValueError):
        I.fuse_point_cloud(depths, K, M, voxel_size=0.25)
    with pytest.raises(ValueError):
        I.fuse_point_cloud(depths, K, M, voxel_size=0.25, colors=colors)
    with pytest.raises(ValueError):
        I.fuse_point_cloud(depths[0], K, M, voxel_size=0.25)
    assert I.Reconstruction._fields == ("depths", "rel_poses", "cam2world", "points", "fused")
    assert I.Reconstruction(1, 2, 3, 4).fused is None


def _parse_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-2] == "end_header" and lines[-1] == ""
    m = re.fullmatch(r"element vertex (\d+)", lines[2])
    props = [tuple(l.split()[1:]) for l in lines[3:-2]]
    assert all(l.startswith("property ") for l in lines[3:-2])
    return int(m.group(1)), props, raw[end:]


def test_write_ply_round_trip(tmp_path):
    from coivo_amd import inference as I
    g = torch.Generator().manual_seed(2)
    pts = torch.randn(37, 3, generator=g)
    col = torch.rand(37, 3, generator=g)
    col[0] = torch.tensor([-0.5, 1.5, float("nan")])
    col[1] = torch.tensor([0.0, 1.0, 0.25])
    path = os.path.join(tmp_path, "cloud.ply")
    I.write_ply(path, pts, col)
    n, props, payload = _parse_ply(path)
    assert n == 37 and props == [("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]
    assert len(payload) == 37 * 15
    rows = np.frombuffer(payload, dtype=np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    assert np.array_equal(rows["p"], pts.numpy())
    want = np.clip(np.rint(np.nan_to_num(col.numpy(), nan=0.0) * np.float32(255)), 0, 255).astype(np.uint8)
    assert np.array_equal(rows["c"], want) and rows["c"][0].tolist() == [0, 255, 0] and rows["c"][1].tolist() == [0, 255, 64]
    I.write_ply(path, pts)
    n, props, payload = _parse_ply(path)
    assert n == 37 and props == [("float", "x"), ("float", "y"), ("float", "z")]
    assert payload == pts.numpy().astype("<f4").tobytes()
    I.write_ply(path, pts[:0], col[:0])
    n, props, payload = _parse_ply(path)
    assert n == 0 and len(props) == 6 and payload == b""
    with pytest.raises(ValueError):
        I.write_ply(path, pts[:, :2])
    with pytest.raises(ValueError):
        I.write_ply(path, pts, col[:5])
