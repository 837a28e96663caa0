"""CPU checks of the mesh renderer (coivo_amd.inference.render_mesh, csrc/raster.hip): the NumPy replica the GPU tests compare with
(tests/raster_ref.py) against covered sets and depths written down by hand, against exact integer point-in-polygon counts on
tessellated rectangles, against the exact ray-plane depth, and against the tube's own depth maps; the C ABI's refusals before any
HIP call; the Python wrappers' argument errors."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import raster_ref as R

MAX_DEPTH = 4.5
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.build()
    return _lib.load()


# ---- hand scenes ------------------------------------------------------------------------------------------------------- #
# fx = fy = 1, principal point (0, 0), identity camera: a vertex (x * z, y * z, z) lands on pixel position (x, y) exactly when z is a
# power of two and x, y are multiples of 1/256.
_K = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]], f32)
_M = np.eye(4, dtype=f32)[None]


def _verts(pix, z=1.0):
    """pixel positions [(x, y), ...] at depth z (a number or one per vertex) -> camera = world points"""
    pix = np.asarray(pix, dtype=np.float64)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), pix.shape[:1])
    return np.stack([pix[:, 0] * z, pix[:, 1] * z, z], 1).astype(f32)


def _covered(out, n=0):
    v, u = np.nonzero(out["index"][n, 0] >= 0)
    return sorted(zip(u.tolist(), v.tolist()))


def test_hand_triangles_and_the_top_left_rule():
    """Two right triangles that tile the square [1, 5] x [1, 5]: the top edge y = 1 and the left edge x = 1 own their pixel centres,
    the right edge x = 5 and the bottom edge y = 5 do not, the shared hypotenuse x + y = 6 belongs to the lower-right face alone
    (of the upper-left face it is neither a top nor a left edge)."""
    v = _verts([(1, 1), (1, 5), (5, 1), (5, 5)])
    upper, lower = [0, 1, 2], [2, 1, 3]                  # both A < 0: front-facing
    want_upper = [(1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (2, 2), (3, 2), (1, 3), (2, 3), (1, 4)]
    want_lower = [(4, 2), (3, 3), (4, 3), (2, 4), (3, 4), (4, 4)]
    o = R.render(v, [upper], _K, _M, 8, 8)
    assert _covered(o) == sorted(want_upper) and o["stats"].tolist() == [[1, 1, 0, 0, 0, 0, 10, 10]]
    o = R.render(v, [lower], _K, _M, 8, 8)
    assert _covered(o) == sorted(want_lower) and o["stats"].tolist() == [[1, 1, 0, 0, 0, 0, 6, 6]]
    o = R.render(v, [upper, lower], _K, _M, 8, 8, want_face_pixels=True)
    assert _covered(o) == sorted(want_upper + want_lower) and o["stats"].tolist() == [[2, 2, 0, 0, 0, 0, 16, 16]]
    assert o["face_pixels"].tolist() == [10, 6]
    idx = o["index"][0, 0]
    assert all(idx[y, x] == 0 for x, y in want_upper) and all(idx[y, x] == 1 for x, y in want_lower)
    assert (o["depth"][0, 0][idx >= 0] == 1.0).all() and np.isposinf(o["depth"][0, 0][idx < 0]).all()
    # the other winding: back-facing, the same pixels; culled: nothing
    o = R.render(v, [upper[::-1], lower[::-1]], _K, _M, 8, 8)
    assert _covered(o) == sorted(want_upper + want_lower) and o["stats"].tolist() == [[2, 2, 0, 0, 2, 0, 16, 16]]
    o = R.render(v, [upper[::-1], lower[::-1]], _K, _M, 8, 8, cull_back=True)
    assert _covered(o) == [] and o["stats"].tolist() == [[2, 0, 0, 0, 2, 0, 0, 0]]
    assert R.render(v, [upper, lower], _K, _M, 8, 8, cull_back=True)["stats"].tolist() == [[2, 2, 0, 0, 0, 0, 16, 16]]


def test_hand_subpixel_positions():
    """Vertices on half and quarter pixels.  (0.5, 0.5), (3.5, 0.5), (0.5, 3.5): the centres with u, v >= 1 and u + v < 4 (those on
    the hypotenuse u + v = 4 are not owned).  Then faces narrower than a pixel: `drawn` says that the bounding box holds a pixel
    centre, `covered` that the face owns one."""
    o = R.render(_verts([(0.5, 0.5), (0.5, 3.5), (3.5, 0.5)]), [[0, 1, 2]], _K, _M, 6, 6)
    assert _covered(o) == [(1, 1), (1, 2), (2, 1)] and o["stats"].tolist() == [[1, 1, 0, 0, 0, 0, 3, 3]]
    # exactly one pixel centre, on the left edge of a face one quarter pixel wide: owned
    o = R.render(_verts([(2, 1.5), (2, 2.5), (2.25, 2)]), [[0, 1, 2]], _K, _M, 6, 6)
    assert _covered(o) == [(2, 2)] and o["stats"].tolist() == [[1, 1, 0, 0, 0, 0, 1, 1]]
    # ... on its right edge: not owned, but the box held the centre, so the face counts as drawn
    o = R.render(_verts([(2, 1.5), (1.75, 2), (2, 2.5)]), [[0, 1, 2]], _K, _M, 6, 6)
    assert _covered(o) == [] and o["stats"].tolist() == [[1, 1, 0, 0, 0, 0, 0, 0]]
    # between two columns: the box is empty
    o = R.render(_verts([(2.25, 1), (2.25, 4), (2.75, 2)]), [[0, 1, 2]], _K, _M, 6, 6)
    assert _covered(o) == [] and o["stats"].tolist() == [[1, 0, 0, 0, 0, 0, 0, 0]]
    # no area
    o = R.render(_verts([(1, 1), (2, 2), (3, 3)]), [[0, 1, 2]], _K, _M, 6, 6)
    assert o["stats"].tolist() == [[1, 0, 0, 0, 0, 1, 0, 0]]


@pytest.mark.parametrize("z", [1.0, 2.0, 0.5, 1.5, 0.7, 3.3])
def test_fronto_parallel_face_returns_its_depth_exactly(z):
    z = float(f32(z))
    K = np.array([[[8, 0, 3], [0, 8, 3], [0, 0, 1]]], f32)
    v = np.array([[-0.3 * z, -0.3 * z, z], [-0.2 * z, 0.6 * z, z], [0.55 * z, -0.1 * z, z]], f32)        # the same pixels at every depth
    o = R.render(v, [[0, 1, 2]], K, _M, 9, 9, want_fragments=True)
    assert o["stats"][0, 6] >= 5 and (o["fragments"]["z"] == f32(z)).all()


def test_slanted_face_returns_the_ray_plane_depth_within_one_ulp():
    """Vertices at depths 1, 2 and 4 that project onto the 1/256 grid, so snapping moves nothing and the face drawn is the face
    given.  The exact depth of the ray through pixel (u, v) -- direction (u, v, 1) -- on the plane through the three points, in
    rationals; the contract's float64 evaluation rounds at most a few 2^-53 away from it and then once to float32: 1 ulp allows the
    final rounding (0.5) and a double rounding."""
    pix, z = [(1, 1), (2.75, 13), (12.5, 1.25)], [1.0, 4.0, 2.0]
    v = _verts(pix, z)
    o = R.render(v, [[0, 1, 2]], _K, _M, 16, 16, want_fragments=True)
    fr = o["fragments"]
    assert o["stats"][0, 0] == 1 and fr["z"].size > 40
    P = [[Fraction(float(c)) for c in row] for row in v]
    a, b = [P[1][i] - P[0][i] for i in range(3)], [P[2][i] - P[0][i] for i in range(3)]
    nrm = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    num = sum(nrm[i] * P[0][i] for i in range(3))
    worst = 0.0
    for u, w, got in zip(fr["u"].tolist(), fr["v"].tolist(), fr["z"]):
        exact = num / (nrm[0] * u + nrm[1] * w + nrm[2])
        ulp = float(np.spacing(f32(float(exact))))
        worst = max(worst, abs(float(Fraction(float(got)) - exact)) / ulp)
    print(f"slanted face: {fr['z'].size} fragments, largest error {worst:.3f} ulp")
    assert worst <= 1.0
    assert len(set(fr["z"].tolist())) > 20                                  # (it is slanted)


# ---- watertightness ---------------------------------------------------------------------------------------------------- #
def _owned_exactly(poly):
    """Pixel centres owned by a convex polygon given in pixel units (multiples of 1/256, counter-clockwise in the contract's sense:
    interior on the positive side of every edge), by the contract's rule in Python integers."""
    q = [(int(round(x * 256)), int(round(y * 256))) for x, y in poly]
    assert all(abs(a * 256 - b[0]) == 0 and abs(c * 256 - b[1]) == 0 for (a, c), b in zip(poly, q))
    us = range(min(x for x, _ in q) // 256 - 1, max(x for x, _ in q) // 256 + 2)
    vs = range(min(y for _, y in q) // 256 - 1, max(y for _, y in q) // 256 + 2)
    n = 0
    for v in vs:
        for u in us:
            ok = True
            for (ax, ay), (bx, by) in zip(q, q[1:] + q[:1]):
                dx, dy = bx - ax, by - ay
                e = dx * (256 * v - ay) - dy * (256 * u - ax)
                ok = ok and (e > 0 or (e == 0 and (dy < 0 or (dy == 0 and dx > 0))))
            n += ok
    return n


def _fan(x0, y0, x1, y1, cx, cy):
    """the rectangle as eight faces about (cx, cy), through the corners and the points of the sides straight above, below and beside it"""
    ring = [(x0, y0), (cx, y0), (x1, y0), (x1, cy), (x1, y1), (cx, y1), (x0, y1), (x0, cy)]
    pts = [(cx, cy)] + ring
    return pts, [[0, 1 + i, 1 + (i + 1) % 8] for i in range(8)]


def _grid(xs, ys):
    pts = [(x, y) for y in ys for x in xs]
    faces = []
    for j in range(len(ys) - 1):
        for i in range(len(xs) - 1):
            a, b, c, d = j * len(xs) + i, j * len(xs) + i + 1, (j + 1) * len(xs) + i, (j + 1) * len(xs) + i + 1
            faces += [[a, b, d], [a, d, c]] if (i + j) % 2 else [[a, b, c], [b, d, c]]
    return pts, faces


@pytest.mark.parametrize("name,mesh,rect", [
    # a pixel centre on the shared vertex (5, 5), centres on the diagonals (2, 2) ... (8, 8) and on the axis-parallel spokes
    ("fan on centres", _fan(1, 1, 9, 9, 5, 5), (1, 1, 9, 9)),
    ("fan off centres", _fan(0.75, 1.25, 8.5, 9.0, 4.25, 6.5), (0.75, 1.25, 8.5, 9.0)),
    # every grid vertex is a pixel centre, shared by up to eight faces; every grid line runs through centres
    ("grid on centres", _grid([1, 3, 5, 7, 9], [1, 3, 5, 7, 9]), (1, 1, 9, 9)),
    ("grid off centres", _grid([0.5, 2, 3.25, 6, 9.75], [1.5, 2, 4.125, 9]), (0.5, 1.5, 9.75, 9)),
])
def test_a_tessellated_rectangle_is_owned_exactly_once(name, mesh, rect):
    pts, faces = mesh
    x0, y0, x1, y1 = rect
    want = _owned_exactly([(x0, y0), (x1, y0), (x1, y1), (x0, y1)])
    assert want > 30
    v = _verts(pts, 2.0)
    for winding in (1, -1):
        fs = [f[::winding] for f in faces]
        o = R.render(v, fs, _K, _M, 12, 12, want_face_pixels=True)
        s = dict(zip(R.STATS, o["stats"][0].tolist()))
        assert s["fragments"] == s["covered"] == want == int(o["face_pixels"].sum()), (name, winding, s, want)
        assert s["front"] == len(fs) and s["degenerate"] == 0 and s["back"] in (0, len(fs))
        culled = R.render(v, fs, _K, _M, 12, 12, cull_back=True)["stats"][0].tolist()
        if s["back"]:
            assert culled[1] == culled[6] == culled[7] == 0 and culled[4] == len(fs), name
        else:
            assert culled == o["stats"][0].tolist(), name
    assert {0, len(faces)} == {R.render(v, [f[::w] for f in faces], _K, _M, 12, 12)["stats"][0, 4] for w in (1, -1)}


# ---- depth bounds ------------------------------------------------------------------------------------------------------ #
def test_every_fragment_lies_between_its_face_depths():
    rng = np.random.default_rng(11)
    K = np.array([[[40, 0, 19.5], [0, 40, 14.5], [0, 0, 1]]], f32)
    F = 600
    z = np.exp(rng.uniform(np.log(0.01), np.log(60.0), (F, 3)))                # depths over nearly four decades within a face
    z[: F // 3] = z[: F // 3, :1] * (1 + 1e-6 * rng.standard_normal((F // 3, 3)))              # ... and nearly equal ones
    pix = rng.uniform(-4, 44, (F, 3, 2)) * [1.0, 0.75]
    v = np.stack([(pix[..., 0] - 19.5) / 40 * z, (pix[..., 1] - 14.5) / 40 * z, z], -1).reshape(-1, 3).astype(f32)
    o = R.render(v, np.arange(3 * F).reshape(F, 3), K, _M, 30, 40, max_depth=100.0, want_fragments=True)
    fr = o["fragments"]
    assert fr["z"].size > 20000 and o["stats"][0, 0] == F
    assert (fr["zmin"] <= fr["z"]).all() and (fr["z"] <= fr["zmax"]).all()
    assert (fr["z"] > 0).all() and (fr["zmin"] < fr["zmax"]).any()


# ---- the tube ---------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("H,W,voxel,proto", [(24, 32, 0.1, 0.979), (64, 96, 0.05, 0.991)])
def test_extract_mesh_winds_towards_the_camera(H, W, voxel, proto):
    """A < 0 is front-facing: of the front, non-degenerate faces of the tube's mesh in the frames' own cameras at least 95 %."""
    mesh, _, K, M = R.tube_mesh(5, H, W, voxel)
    neg = tot = 0
    for n in range(5):
        s = R.setup(mesh["vertices"], mesh["faces"], K, M, n, H, W, MAX_DEPTH, False)
        ok = s["front"] & ~s["outside"] & ~s["degenerate"]
        neg, tot = neg + int((ok & s["swapped"]).sum()), tot + int(ok.sum())
    print(f"{H}x{W}: {neg} of {tot} front faces have A < 0 ({neg / tot:.4f}; frame 2 alone in the prototype: {proto})")
    assert tot > 1000 and neg >= 0.95 * tot


def test_rendered_mesh_depth_against_the_exact_depth():
    """5 x 64x96, voxel 0.05, the mesh drawn into frame 2's camera against that frame's exact depth below 4.5: coverage at least 95 %
    (a cap on what the comparison leaves out), median relative error below 0.85 % (the squares' best figure at this size, DESIGN.md
    §3.6j).  Measured: coverage 97.19 %, median 0.128 %, p90 0.344 %, max 1.241 %."""
    H, W = 64, 96
    mesh, d, K, M = R.tube_mesh(5, H, W, 0.05)
    assert mesh["vertices"].shape == (9696, 3) and mesh["faces"].shape == (17974, 3)
    o = R.render(mesh["vertices"], mesh["faces"], K[2:3], M[2:3], H, W, max_depth=MAX_DEPTH)
    s = dict(zip(R.STATS, o["stats"][0].tolist()))
    gt = d[2, 0].astype(np.float64)
    valid = gt < MAX_DEPTH
    seen = valid & (o["index"][0, 0] >= 0)
    rel = np.abs(o["depth"][0, 0][seen].astype(np.float64) - gt[seen]) / gt[seen]
    print(f"stats {s}; covered {seen.sum()} of {valid.sum()} ({seen.sum() / valid.sum():.4f}); relative error median "
          f"{np.median(rel):.5f}, p90 {np.percentile(rel, 90):.5f}, max {rel.max():.5f}")
    assert s["straddling"] == 24 and s["back"] == 166
    assert seen.sum() >= 0.95 * valid.sum()
    assert np.median(rel) < 0.0085


# ---- robustness -------------------------------------------------------------------------------------------------------- #
def _small_tube():
    mesh, _, K, M = R.tube_mesh(5, 24, 32, 0.1)
    return np.array(mesh["vertices"]), np.array(mesh["faces"]), np.array(mesh["colors"]), K, M


def _same(a, b, keys=("depth", "index", "colors", "normal", "face_pixels", "stats")):
    for k in keys:
        if a[k] is None:
            assert b[k] is None, k
        else:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


def test_a_face_with_an_index_out_of_range_is_skipped():
    v, f, c, K, M = _small_tube()
    kw = dict(colors=c, max_depth=MAX_DEPTH, want_normals=True)
    want = R.render(v, f, K, M, 24, 32, **kw)
    bad = np.array([[0, 1, len(v)], [-1, 2, 3], [4, 2 ** 31 - 1, 5], [-2 ** 31, 0, 1]], np.int32)
    got = R.render(v, np.concatenate([f, bad]), K, M, 24, 32, **kw)
    _same(want, got)
    assert want["stats"][:, 0].min() > 1000


def test_nan_vertices_fall_out():
    v, f, c, K, M = _small_tube()
    want = R.render(v, f, K, M, 24, 32, max_depth=MAX_DEPTH)
    v2 = v.copy()
    v2[100] = np.nan
    v2[200, 0] = np.inf
    touched = (f == 100).any(1) | (f == 200).any(1)
    got = R.render(v2, f, K, M, 24, 32, max_depth=MAX_DEPTH)
    ref = R.render(v, f[~touched], K, M, 24, 32, max_depth=MAX_DEPTH)
    assert np.array_equal(got["depth"].view(np.int32), ref["depth"].view(np.int32))
    assert not np.isin(got["index"], np.nonzero(touched)[0]).any() and touched.sum() >= 6
    assert np.isfinite(got["depth"][got["index"] >= 0]).all()
    assert (got["stats"][:, 0] <= want["stats"][:, 0]).all() and got["stats"][:, 0].sum() < want["stats"][:, 0].sum()


def test_a_permutation_of_the_faces_moves_no_depth_bit_and_no_statistic():
    v, f, c, K, M = _small_tube()
    perm = np.random.default_rng(5).permutation(len(f))
    a = R.render(v, f, K, M, 24, 32, colors=c, max_depth=MAX_DEPTH, want_face_pixels=True)
    b = R.render(v, f[perm], K, M, 24, 32, colors=c, max_depth=MAX_DEPTH, want_face_pixels=True)
    _same(a, b, keys=("depth", "stats"))
    # (equal depths go to the smallest row, so the winner may change where two faces tie: the pixel totals do not)
    assert a["face_pixels"].sum() == b["face_pixels"].sum() == a["stats"][:, 7].sum()


def test_replica_products_are_consistent():
    v, f, c, K, M = _small_tube()
    o = R.render(v, f, K, M, 24, 32, colors=c, max_depth=MAX_DEPTH, want_normals=True, want_face_pixels=True, want_fragments=True)
    hit = o["index"][:, 0] >= 0
    assert (o["stats"][:, 7] == hit.reshape(5, -1).sum(1)).all() and (o["stats"][:, 6] >= o["stats"][:, 7]).all()
    assert o["fragments"]["z"].size == o["stats"][:, 6].sum()
    assert np.array_equal(o["face_pixels"], np.bincount(o["index"][o["index"] >= 0], minlength=len(f)))
    nn = np.moveaxis(o["normal"], 1, -1)[hit].astype(np.float64)
    assert np.abs(np.linalg.norm(nn, axis=1) - 1).max() < 1e-6 and not o["normal"][:, :, ~hit[0]][0].any()
    col = np.moveaxis(o["colors"], 1, -1)[hit]
    assert (col >= 0).all() and (col <= 1).all() and col.std() > 0.05         # a weighted mean of colours in [0, 1]
    # the normal faces the camera: n . ray < 0 for the pixel's ray
    vv, uu = np.meshgrid(np.arange(24.0), np.arange(32.0), indexing="ij")
    for n in range(5):
        ray = np.stack([(uu - K[n, 0, 2]) / K[n, 0, 0], (vv - K[n, 1, 2]) / K[n, 1, 1], np.ones_like(uu)], -1)[hit[n]]
        dots = (np.moveaxis(o["normal"][n], 0, -1)[hit[n]] * ray).sum(1)
        assert (dots < 1e-6).all()


# ---- the C ABI --------------------------------------------------------------------------------------------------------- #
def test_entry_point_refuses_bad_arguments_before_any_hip_call(lib):
    from coivo_amd import _lib
    assert lib.colvo_abi_version() == _lib.ABI_VERSION >= 24
    buf = (C.c_double * 66)()
    p = (C.addressof(buf) + 15) & ~15                                       # no call below gets past its checks to touch it
    base = dict(vertices=p, faces=p, colors=p, V=4, F=2, K=p, cam=p, N=2, H=8, W=8, max_depth=10.0, cull=0, scratch=p, out_d=p, out_i=p,
                out_c=p, out_n=p, out_f=p, out_s=p)
    order = tuple(base)

    def refused(what, **kw):
        a = dict(base)
        a.update(kw)
        assert lib.colvo_render_mesh(*(a[k] for k in order), None) != 0, kw
        msg = lib.colvo_last_error().decode()
        assert msg.startswith("colvo_render_mesh: ") and what in msg, (kw, msg)

    for k in ("vertices", "faces", "K", "cam", "scratch", "out_d", "out_i", "out_s"):
        refused("null pointer", **{k: None})
    refused("null pointer", colors=None)                                     # colours without their output, and the reverse
    refused("null pointer", out_c=None)
    refused("bad mesh", V=-1)
    refused("bad mesh", F=-1)
    for s in (dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=float("nan")), dict(max_depth=float("inf"))):
        refused("bad max_depth", **s)
    for s in (dict(cull=2), dict(cull=-1)):
        refused("bad cull_back", **s)
    for s in (dict(N=0), dict(N=65536), dict(N=-3), dict(H=0), dict(W=-3), dict(H=16385), dict(N=1, H=1, W=16385),
              dict(N=8, H=16384, W=16384), dict(N=65535, H=256, W=320)):
        refused("bad shape", **s)
    refused("16-byte aligned", scratch=p + 8)
    assert lib.colvo_render_scratch_bytes(7, 16384, 16384) > 0 and lib.colvo_render_scratch_bytes(8, 16384, 16384) == 0


def test_kernels_use_no_scratch_and_a_native_minimum(lib, tmp_path):
    """The resource metadata of raster.hip's kernels (the draw kernel in both its forms): no private segment, no spilled register;
    the 64-bit minimum is one instruction."""
    import re
    from coivo_amd import build
    asm = open(build.emit_asm("raster.hip", str(tmp_path / "raster.s"))).read()
    kernels = set(re.findall(r"\.name:\s+(\S*k_r(?:aster|ender)_\w+)", asm))
    assert len(kernels) == 6 and all(any(n in k for k in kernels) for n in ("k_render_clear", "k_raster_zero", "k_raster_draw",
                                                                             "k_raster_resolve", "k_raster_stats")), kernels
    for key in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count"):
        vals = re.findall(rf"\.{key}:\s+(\d+)", asm)
        assert len(vals) == 6 and all(int(v) == 0 for v in vals), (key, vals)
    assert "global_atomic_umin_x2" in asm and "cmpswap" not in asm


# ---- Python ------------------------------------------------------------------------------------------------------------ #
def test_render_mesh_argument_errors(lib):
    from coivo_amd import inference as I
    v, f = torch.zeros(5, 3), torch.zeros(2, 3, dtype=torch.int32)
    K, M = torch.eye(3), torch.eye(4)[None]
    for bad in (dict(max_depth=0.0), dict(max_depth=float("inf")), dict(max_depth=float("nan")), dict(max_depth=None),
                dict(cull_back=1), dict(cull_back=None), dict(want_normals=1), dict(want_face_pixels="yes")):
        with pytest.raises(ValueError, match=next(iter(bad))):
            I.render_mesh(v, f, K, M, 8, 8, **bad)
    for H, W in ((0, 8), (8, -1), (8.0, 8), (True, 8), (16385, 8), (8, 1 << 15)):
        with pytest.raises(ValueError, match="1..16384"):
            I.render_mesh(v, f, K, M, H, W)
    with pytest.raises(ValueError, match="limits"):
        I.render_mesh(v, f, K, torch.eye(4).expand(8, 4, 4), 1 << 14, 1 << 14)                   # N*H*W = 2^31
    with pytest.raises(ValueError, match="limits"):
        I.render_mesh(v, f, K, torch.zeros(0, 4, 4), 8, 8)
    with pytest.raises(ValueError, match=r"\[V,3\]"):
        I.render_mesh(v[:, :2], f, K, M, 8, 8)
    with pytest.raises(ValueError, match=r"\[F,3\] int32"):
        I.render_mesh(v, f.long(), K, M, 8, 8)
    with pytest.raises(ValueError, match=r"\[F,3\] int32"):
        I.render_mesh(v, None, K, M, 8, 8)
    with pytest.raises(ValueError, match=r"\[N,4,4\]"):
        I.render_mesh(v, f, K, M[0], 8, 8)
    # these tensors live on the CPU: refused the way the neighbouring functions refuse them, before any native call
    with pytest.raises(ValueError, match="CUDA"):
        I.render_mesh(v, f, K, M, 8, 8)
    mesh = I.Mesh(v, f, None, v, torch.zeros(5, 3, dtype=torch.int32), 0)
    for call in (lambda: I.render_mesh(mesh, K, M, 8, 8), lambda: I.render_mesh(mesh, K=K, cam2world=M, H=8, W=8)):
        with pytest.raises(ValueError, match="CUDA"):
            call()
    with pytest.raises(ValueError, match="with a Mesh"):
        I.render_mesh(mesh, f, K, M, 8, 8)
    with pytest.raises(ValueError, match="with a Mesh"):
        I.render_mesh(mesh, K, M, 8)


def test_reconstruct_sequence_refuses_what_it_must():
    from coivo_amd import inference as I
    frames = torch.zeros(3, 3, 8, 8)
    with pytest.raises(ValueError, match="Meshing"):
        I.reconstruct_sequence(None, None, frames, torch.eye(3), voxel_size=0.05, render=I.Render(mesh=True))
    with pytest.raises(ValueError, match="surfels"):
        I.reconstruct_sequence(None, None, frames, torch.eye(3), voxel_size=0.05, mesh=I.Meshing(),
                               render=I.Render(mesh=True, surfels=True))
    with pytest.raises(ValueError, match="render.mesh"):
        I.reconstruct_sequence(None, None, frames, torch.eye(3), voxel_size=0.05, mesh=I.Meshing(), render=I.Render(mesh=1))
    with pytest.raises(ValueError, match="voxel_size"):
        I.reconstruct_sequence(None, None, frames, torch.eye(3), mesh=I.Meshing(), render=I.Render(mesh=True))


def test_policy_and_result_types():
    from coivo_amd import inference as I
    assert I.MeshViews._fields == ("depth", "index", "colors", "normal", "stats", "face_pixels")
    assert I.Render() == (None, 8) and I.Render._fields == ("radius", "max_splat") and len(I.Render(mesh=True)) == 2
    assert I.Render().mesh is False and I.Render(mesh=True).mesh is True and I.Render(mesh=True).surfels is False
    r = I.Render(0.01, 4, mesh=True)._replace(max_splat=2)
    assert r == (0.01, 2) and r.mesh is True and r.surfels is False
    assert I.Render(surfels=True)._replace(mesh=True).mesh is True and I.Render(surfels=True)._replace(radius=1.0).surfels is True
    assert "mesh=True" in repr(I.Render(mesh=True)) and "surfels=False" in repr(I.Render(mesh=True))
    radius, max_splat = I.Render(mesh=True)
    assert (radius, max_splat) == (None, 8)
    assert I.Reconstruction._fields == ("depths", "rel_poses", "cam2world", "points", "fused") and len(I.Reconstruction(1, 2, 3, 4)) == 5
    from coivo_amd import _lib
    assert _lib.tune_get("raster_coop_min_pixels") == 256
