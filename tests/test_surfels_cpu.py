"""CPU: the NumPy replica of the oriented-disc renderer (tests/surfel_ref.py) held to geometry -- hand-computed discs, equality with
render_ref.render where the contract says so, and the grazing-angle bias on the scene behind DESIGN.md §3.6j's table --, write_ply
with normals, and the host side of colvo_render_surfels / inference.render_surfels, none of which needs a GPU."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest
import torch

from tests import consistency_ref as CR
from tests import normals_ref as NR
from tests import render_ref as R
from tests import surfel_ref as S

f32 = np.float32
MAX_DEPTH = 4.5


def _cam(H, W, fx):
    K = np.array([[[fx, 0, (W - 1) / 2], [0, fx, (H - 1) / 2], [0, 0, 1]]], f32)
    return K, np.eye(4, dtype=f32)[None]


def test_a_disc_facing_the_camera_is_round_and_keeps_its_depth():
    H = W = 11
    K, M = _cam(H, W, 100.0)
    o = S.render([[0, 0, 2]], [[0, 0, -1]], K, M, H, W, radius=0.05, max_splat=8, max_depth=MAX_DEPTH)      # 2.5 pixels at depth 2
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    inside = (u - 5) ** 2 + (v - 5) ** 2 <= 2.5 ** 2                     # 21 pixels: the 5 x 5 square without its corners and (+-2, +-2)...
    assert inside.sum() == 21
    assert np.array_equal(o["index"][0, 0] == 0, inside) and np.array_equal(o["depth"][0, 0][inside], np.full(21, 2, f32))
    assert np.isinf(o["depth"][0, 0][~inside]).all() and o["stats"].tolist() == [[1, 1, 0, 21, 0, 0]]
    assert np.array_equal(o["normal"][0][:, inside], np.broadcast_to(np.array([[0], [0], [-1]], f32), (3, 21)))
    assert not o["normal"][0][:, ~inside].any()
    # the square of the same point covers the corners too
    sq = R.render([[0, 0, 2]], K, M, H, W, radius=0.05, max_splat=8, max_depth=MAX_DEPTH)
    assert (sq["index"][0, 0] == 0).sum() == 25


def test_a_tilted_disc_carries_its_plane():
    H = W = 21
    K, M = _cam(H, W, 100.0)
    n = np.array([0.6, 0.0, -0.8])
    P = np.array([0.03, -0.02, 2.0])
    o = S.render([P], [n], K, M, H, W, radius=0.08, max_splat=8, max_depth=MAX_DEPTH)
    hit = o["index"][0, 0] == 0
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - 10) / 100, (v - 10) / 100, np.ones_like(u)], -1)
    z = (n @ P) / (ray @ n)                                              # the ray's depth on the disc's plane
    on_disc = np.linalg.norm(ray * z[..., None] - P, axis=-1)
    # away from the rim (by more than float32 rounding of a distance of 0.08) the hit set is the disc, and the nearest pixel is on it:
    # an ellipse of 4 by 4 * 0.8 pixels, pi * 4 * 3.2 = 40 pixels
    assert hit[on_disc < 0.08 - 1e-6].all() and not hit[on_disc > 0.08 + 1e-6].any() and 30 < hit.sum() < 50
    assert np.abs(o["depth"][0, 0][hit] - z[hit]).max() < 8 * 2.0 ** -24 * 2.2 / 0.8          # num / den: a few roundings over |den| >= 0.8
    assert o["depth"][0, 0][hit].max() - o["depth"][0, 0][hit].min() > 0.05                     # a square would carry ONE depth
    assert o["stats"].tolist() == [[1, 1, 0, int(hit.sum()), 0, 0]]


def test_back_facing_points_are_culled_and_zero_or_nan_normals_are_flat():
    H = W = 9
    K, M = _cam(H, W, 50.0)
    pts = np.array([[0, 0, 2], [0.02, 0, 1.5], [-0.04, 0.02, 1.0], [0, 0, -1]], f32)
    nrm = np.array([[0, 0, 1], [0, 0, 0], [np.nan, 0, 0], [0, 0, -1]], f32)                     # away, none, none, (behind the camera)
    o = S.render(pts, nrm, K, M, H, W, radius=0.03, max_splat=8, max_depth=MAX_DEPTH)
    assert o["stats"].tolist() == [[3, 2, 0, int((o["index"] >= 0).sum()), 1, 2]]
    assert set(np.unique(o["index"])) == {-1, 1, 2} and not o["normal"].any()
    sq = R.render(pts[1:3], K, M, H, W, radius=0.03, max_splat=8, max_depth=MAX_DEPTH)
    assert np.array_equal(o["depth"].view(np.uint32), sq["depth"].view(np.uint32))
    assert np.array_equal(o["index"], np.where(sq["index"] >= 0, sq["index"] + 1, -1))


def test_a_point_that_hits_no_pixel_centre_lands_on_its_nearest_pixel():
    H = W = 9
    K, M = _cam(H, W, 50.0)
    # a disc of 0.2 pixels radius between pixel centres, seen edge-on enough that no ray through a pixel centre meets it
    o = S.render([[0.012, 0.012, 2]], [[0.0, 0.0, -1.0]], K, M, H, W, radius=0.008, max_splat=8, max_depth=MAX_DEPTH)
    assert o["stats"].tolist() == [[1, 1, 0, 1, 0, 0]]
    assert o["index"][0, 0, 4, 4] == 0 and o["depth"][0, 0, 4, 4] == f32(2)


@functools.lru_cache(maxsize=None)
def _tube():
    pts, d, K, M = R.tube_points(3, 17, 23, 5)
    s = NR.sample_normals(d, K, M, max_depth=np.inf, rel_edge=0.2)           # (23 pixels across: neighbours differ by more than 5 %)
    nrm = (s["q"][np.isfinite(d[:, 0])] / 16384.0).astype(f32)
    col = np.random.default_rng(1).random(pts.shape, dtype=f32)
    return pts, nrm, col, K, M


def test_zero_normals_and_zero_radius_equal_render_cloud():
    pts, nrm, col, K, M = _tube()
    for radius, normals in ((0.05, np.zeros_like(nrm)), (0.0, nrm), (0.0, np.zeros_like(nrm))):
        o = S.render(pts, normals, K, M, 17, 23, radius=radius, colors=col, max_splat=4, max_depth=MAX_DEPTH)
        q = R.render(pts, K, M, 17, 23, radius=radius, colors=col, max_splat=4, max_depth=MAX_DEPTH)
        for k in ("depth", "colors"):
            assert np.array_equal(o[k].view(np.uint32), q[k].view(np.uint32)), (radius, k)
        assert np.array_equal(o["index"], q["index"]) and np.array_equal(o["stats"][:, :4], q["stats"])
        assert not o["stats"][:, 4].any()                                # the wall's normals face the cameras inside it: none culled
        # flat: every point in front without normals; with them only the few deep in the lumen whose neighbours lie beyond rel_edge
        assert np.array_equal(o["stats"][:, 5], o["stats"][:, 0]) if not normals.any() else (o["stats"][:, 5] < o["stats"][:, 0] // 4).all()


# ---- the bias, on the scene behind §3.6j's table ---------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def _bias_scene():
    """consistency_ref.tube_scene(5, 64, 96, 5): every frame's samples below 4.5 with their own quantised normals, drawn into frame 2."""
    pts, d, K, M = R.tube_points(5, 64, 96, 5, max_depth=MAX_DEPTH)
    s = NR.sample_normals(d, K, M, max_depth=MAX_DEPTH)
    kept = d[:, 0] < MAX_DEPTH
    assert s["normal"][kept].all()
    nrm = (s["q"][kept] / 16384.0).astype(f32)                            # (exact: |q| < 2^15)
    gt = d[2, 0]
    return pts, nrm, K[2:3], M[2:3], gt, gt < MAX_DEPTH


def _bias(radius, squares=False):
    pts, nrm, K, M, gt, mask = _bias_scene()
    o = S.render(pts, nrm, K, M, 64, 96, radius=radius, max_splat=8, max_depth=MAX_DEPTH, squares=squares)
    z = o["depth"][0, 0][mask]
    rel = np.abs(z.astype(np.float64) - gt[mask]) / gt[mask]
    return o, int(np.isfinite(z).sum()), float(np.median(rel)), float(rel.max())


@pytest.mark.parametrize("radius", [0.0, 0.01, 0.02, 0.04])
def test_discs_remove_the_grazing_angle_bias(radius):
    pts, nrm, K, M, gt, mask = _bias_scene()
    assert int(mask.sum()) == 5230
    o, covered, median, worst = _bias(radius)
    _, sq_covered, sq_median, sq_worst = _bias(radius, squares=True)
    print(f"radius {radius}: discs median {100 * median:.5f} % max {100 * worst:.3f} %, squares median {100 * sq_median:.5f} % "
          f"max {100 * sq_worst:.3f} %, stats {o['stats'][0].tolist()}")
    assert covered == sq_covered == 5230                                  # every scored pixel is covered
    if radius >= 0.02:
        assert median < 1e-3                                              # 0.1 %
        assert sq_median > 1.6e-2                                         # ... which the squares miss by a factor of sixteen and more
    if radius == 0.0:
        q = R.render(pts, K, M, 64, 96, radius=0.0, max_splat=8, max_depth=MAX_DEPTH)
        assert np.array_equal(o["depth"].view(np.uint32), q["depth"].view(np.uint32)) and np.array_equal(o["index"], q["index"])
        assert np.array_equal(o["stats"][:, :4], q["stats"]) and not o["stats"][:, 4:].any()


# ---- write_ply ---------------------------------------------------------------------------------------------------------------- #
def _read_ply(path):
    """A hand-written reader: (property names, rows as tuples)."""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    m = int(lines[2].split()[-1])
    props = [l.split()[1:] for l in lines[3:] if l.startswith("property")]
    fmt = "<" + "".join({"float": "f", "uchar": "B"}[t] for t, _ in props)
    size = struct.calcsize(fmt)
    assert len(body) == m * size
    return [n for _, n in props], [struct.unpack_from(fmt, body, i * size) for i in range(m)]


def test_write_ply_with_normals_round_trips_and_without_them_is_unchanged(tmp_path):
    from coivo_amd import inference as I
    g = torch.Generator().manual_seed(3)
    pts, col = torch.randn(7, 3, generator=g), torch.rand(7, 3, generator=g)
    nrm = torch.nn.functional.normalize(torch.randn(7, 3, generator=g), dim=1)
    I.write_ply(tmp_path / "n.ply", pts, col, nrm)
    names, rows = _read_ply(tmp_path / "n.ply")
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    want_c = np.clip(np.rint(col.numpy() * 255.0), 0, 255).astype(np.uint8)
    for i, r in enumerate(rows):
        assert r[:3] == tuple(pts[i].tolist()) and r[3:6] == tuple(nrm[i].tolist()) and r[6:] == tuple(want_c[i].tolist())
    I.write_ply(tmp_path / "n2.ply", pts, normals=nrm)
    names, rows = _read_ply(tmp_path / "n2.ply")
    assert names == ["x", "y", "z", "nx", "ny", "nz"] and rows[3] == tuple(pts[3].tolist()) + tuple(nrm[3].tolist())
    # without normals: the bytes of the writer before normals existed, built here by hand
    for colors in (None, col):
        I.write_ply(tmp_path / "p.ply", pts, colors)
        head = ["ply", "format binary_little_endian 1.0", "element vertex 7", "property float x", "property float y", "property float z"]
        if colors is not None:
            head += ["property uchar red", "property uchar green", "property uchar blue"]
        body = b"".join(struct.pack("<fff", *pts[i].tolist()) + (bytes(want_c[i].tolist()) if colors is not None else b"") for i in range(7))
        assert open(tmp_path / "p.ply", "rb").read() == ("\n".join(head + ["end_header"]) + "\n").encode("ascii") + body
    with pytest.raises(ValueError, match="normals"):
        I.write_ply(tmp_path / "bad.ply", pts, col, nrm[:3])


# ---- the library's host side -------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.build()
    return _lib.load()


def test_kernels_use_no_scratch_and_a_native_minimum(lib, tmp_path):
    import re
    from coivo_amd import build
    asm = open(build.emit_asm("surfels.hip", str(tmp_path / "surfels.s"))).read()
    kernels = set(re.findall(r"\.name:\s+(\S*k_(?:surfel|render)_\w+)", asm))
    assert len(kernels) == 5 and all(any(n in k for k in kernels) for n in ("k_render_clear", "k_surfel_splat", "k_surfel_resolve",
                                                                             "k_surfel_stats")), kernels
    for key in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count"):
        vals = re.findall(rf"\.{key}:\s+(\d+)", asm)
        assert len(vals) == 5 and all(int(v) == 0 for v in vals), (key, vals)
    assert "global_atomic_umin_x2" in asm and "cmpswap" not in asm


def test_colvo_render_surfels_refuses_before_any_hip_call(lib):
    """Host pointers: a call that got past its checks would fault or report a HIP error with another prefix."""
    buf = (C.c_float * 72)()
    p = (C.addressof(buf) + 15) // 16 * 16

    def call(M=4, N=1, H=8, W=8, radius=0.02, max_splat=8, max_depth=4.5, ptrs=None):
        # points, normals, colors | K, cam2world | scratch, out_depth, out_index, out_colors, out_normal, out_stats
        a = ptrs or [p, p, 0, p, p, p, p, p, 0, 0, p]
        return lib.colvo_render_surfels(a[0], a[1], a[2], M, a[3], a[4], N, H, W, radius, max_splat, max_depth, *a[5:], 0)

    for what, kw in (("bad point count", dict(M=-1)), ("bad shape", dict(N=0)), ("bad shape", dict(N=65536)), ("bad shape", dict(H=0)),
                     ("bad shape", dict(H=1 << 15, W=1 << 15)), ("bad shape", dict(N=1 << 15, H=1 << 8, W=1 << 8)),
                     ("bad max_splat", dict(max_splat=33)), ("bad max_splat", dict(max_splat=-1)), ("bad radius", dict(radius=-1.0)),
                     ("bad radius", dict(radius=float("nan"))), ("bad radius", dict(radius=float("inf"))),
                     ("bad max_depth", dict(max_depth=0.0)), ("bad max_depth", dict(max_depth=float("inf"))),
                     ("null pointer", dict(ptrs=[p, 0, 0, p, p, p, p, p, 0, 0, p])),                 # points without normals
                     ("null pointer", dict(ptrs=[0, p, 0, p, p, p, p, p, 0, 0, p])),
                     ("null pointer", dict(ptrs=[p, p, 0, p, p, 0, p, p, 0, 0, p])),
                     ("go together", dict(ptrs=[p, p, p, p, p, p, p, p, 0, 0, p])),
                     ("go together", dict(ptrs=[p, p, 0, p, p, p, p, p, p, 0, p])),
                     ("16-byte aligned", dict(ptrs=[p, p, 0, p, p, p + 4, p, p, 0, 0, p]))):
        rc = call(**kw)
        msg = lib.colvo_last_error()
        assert rc != 0 and msg.startswith(b"colvo_render_surfels:") and what.encode() in msg, (what, kw, msg)


def test_render_surfels_argument_errors(lib):
    from coivo_amd import inference as I
    pts = torch.zeros(5, 3)
    K, M = torch.eye(3), torch.eye(4)[None]
    for bad in (dict(radius=-1.0), dict(radius=float("nan")), dict(radius=None), dict(max_splat=33), dict(max_splat=2.0),
                dict(max_depth=0.0), dict(max_depth=float("nan"))):
        kw = dict(radius=0.02)
        kw.update(bad)
        with pytest.raises(ValueError, match=next(iter(bad))):
            I.render_surfels(pts, pts, K, M, 8, 8, **kw)
    with pytest.raises(TypeError):
        I.render_surfels(pts, pts, K, M, 8, 8)                           # radius has no default
    with pytest.raises(ValueError, match="normals"):
        I.render_surfels(pts, pts[:4], K, M, 8, 8, radius=0.02)
    with pytest.raises(ValueError, match="normals"):
        I.render_surfels(pts, None, K, M, 8, 8, radius=0.02)
    for H, W in ((0, 8), (8, -1), (8.0, 8), (1 << 15, 1 << 15)):
        with pytest.raises(ValueError):
            I.render_surfels(pts, pts, K, M, H, W, radius=0.02)
    fused = I.FusedCloud(pts, None, torch.ones(5, dtype=torch.int32), torch.zeros(5, 3, dtype=torch.int32), (0.0, 0.0, 0.0), (8, 8, 8), 0.02,
                         5, 0, 1, 5)
    with pytest.raises(ValueError, match="want_normals"):
        I.render_fused(fused, K, M, 8, 8, want_normals=True)
    assert I.Render() == (None, 8) and I.Render().surfels is False and I.Render(surfels=True).surfels is True
    assert I.Render(0.01, 4, True)._replace(max_splat=2) == (0.01, 2) and I.Render(0.01, 4, True)._replace(max_splat=2).surfels is True
