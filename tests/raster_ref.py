"""NumPy replica of the mesh rendering contract (include/colvo.h colvo_render_mesh) -- test infrastructure in the
manner of tests/render_ref.py.  The contract, restated:

  inputs      vertices [V,3] float32 in the world frame, faces [F,3] int32, colors [V,3] float32 or None, K [N,3,3], cam2world
              [N,4,4] float32, H, W, max_depth, cull_back.  Pixel u has its centre at x = u.
  arithmetic  float32 where the contract says float32, int64 for the snapped coordinates and the edge functions (|E| < 2^48),
              float64 in the written association for depth, colour and normal; one rounding per operation (NumPy never contracts).
  per frame n and face f:
    camera      each vertex as tests/render_ref.py's camera point; a face with an index outside [0, V) is dead.  A vertex is front
                iff 1e-3f < P_z < max_depth; the face is front iff all three are, straddling iff some are.
    projection  x = (fx * P_x) / P_z + cx, y likewise; in the guard band iff |x|, |y| <= 16384 for all three; X = int(rint(x * 256)).
    area        A = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0); 0: degenerate; < 0: front-facing; > 0: back-facing (dropped iff
                cull_back).  A < 0: vertices 1 and 2 are exchanged and A = -A (the oriented numbering, used from here on).
    coverage    u_lo = max((min X + 255) >> 8, 0), u_hi = min(max X >> 8, W - 1), the same in v.  E_k for the edge opposite vertex k
                (1 -> 2, 2 -> 0, 0 -> 1) at p = (256 u, 256 v): d_x (p_y - a_y) - d_y (p_x - a_x); covered iff every E_k > 0 or
                (E_k == 0 and the edge is top-left: d_y < 0 or (d_y == 0 and d_x > 0)).
    depth       iz_k = 1 / float64(P_z,k), w_k = float64(E_k) * iz_k, s = (w_0 + w_1) + w_2, z = float32(float64(A) / s).
    key         (uint64(bits(z)) << 32) | uint32(f); the pixel takes the minimum.
  outputs     depth [N,1,H,W] f32 (+inf where empty), index [N,1,H,W] i32 (-1), colors [N,3,H,W] f32
              (float32(((w_0 c_0 + w_1 c_1) + w_2 c_2) / s), 0 where empty), normal [N,3,H,W] f32 (unit (P_1 - P_0) x (P_2 - P_0) of
              the face's own numbering in float64, turned to the camera; 0 where empty), face_pixels [F] i32, stats [N,8] i32: front,
              drawn, straddling, outside, back-facing, degenerate, fragments, covered.

The GPU tests demand equality to the bit.
"""
import functools

import numpy as np

f32, f64, i64 = np.float32, np.float64, np.int64
Z_EPS = f32(1e-3)
GUARD = f32(16384.0)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
STATS = ("front", "drawn", "straddling", "outside", "back", "degenerate", "fragments", "covered")


def setup(vertices, faces, K, M, n, H, W, max_depth, cull_back):
    """Steps 1 to 4 of the contract up to the bounding box, for frame n and every face.  -> dict of live, front, straddling, outside,
    back, degenerate, drawn, swapped (bool [F]); P [F,3,3] f32 (camera points, the face's own numbering: P[f, k, axis]); X, Y [F,3]
    int64 and Pz [F,3] f32 in the oriented numbering; A [F] int64 (>= 0); u_lo, u_hi, v_lo, v_hi int64."""
    vertices = np.asarray(vertices, dtype=f32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3).astype(i64)
    V, F = vertices.shape[0], faces.shape[0]
    k, m = np.asarray(K, dtype=f32)[n], np.asarray(M, dtype=f32)[n]
    max_depth = f32(max_depth)
    live = ((faces >= 0) & (faces < V)).all(1)
    w = vertices[np.where(live[:, None], faces, 0)] if V else np.zeros((F, 3, 3), f32)
    with np.errstate(all="ignore"):
        q = [w[:, :, a] - m[a, 3] for a in range(3)]
        P = np.stack([(m[0, a] * q[0] + m[1, a] * q[1]) + m[2, a] * q[2] for a in range(3)], -1)
        assert P.dtype == f32
        vfront = live[:, None] & (P[:, :, 2] > Z_EPS) & (P[:, :, 2] < max_depth)
        nf = vfront.sum(1)
        front, straddling = nf == 3, (nf > 0) & (nf < 3)
        x = (k[0, 0] * P[:, :, 0]) / P[:, :, 2] + k[0, 2]
        y = (k[1, 1] * P[:, :, 1]) / P[:, :, 2] + k[1, 2]
        assert x.dtype == f32 and y.dtype == f32
        inb = front & ((np.abs(x) <= GUARD) & (np.abs(y) <= GUARD)).all(1)
        X = np.rint(np.where(inb[:, None], x, f32(0)) * f32(256.0)).astype(i64)
        Y = np.rint(np.where(inb[:, None], y, f32(0)) * f32(256.0)).astype(i64)
    A = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
    back, degenerate, swapped = inb & (A > 0), inb & (A == 0), A < 0
    order = np.where(swapped[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))
    X, Y, Pz = (np.take_along_axis(a, order, 1) for a in (X, Y, P[:, :, 2]))
    A = np.abs(A)
    u_lo, u_hi = np.maximum((X.min(1) + 255) >> 8, 0), np.minimum(X.max(1) >> 8, W - 1)
    v_lo, v_hi = np.maximum((Y.min(1) + 255) >> 8, 0), np.minimum(Y.max(1) >> 8, H - 1)
    drawn = inb & (A != 0) & ~(back & bool(cull_back)) & (u_lo <= u_hi) & (v_lo <= v_hi)
    return dict(live=live, front=front, straddling=straddling, outside=front & ~inb, back=back, degenerate=degenerate, drawn=drawn,
                swapped=swapped, order=order, P=P, X=X, Y=Y, Pz=Pz, A=A, u_lo=u_lo, u_hi=u_hi, v_lo=v_lo, v_hi=v_hi)


def edges(s, rows, u, v):
    """The three edge functions of faces `rows` of a setup at the pixel centres (u, v) (arrays of rows' length) -> (E [3, n] int64,
    covered [n] bool)."""
    X, Y = s["X"][rows], s["Y"][rows]
    px, py = np.asarray(u, dtype=i64) * 256, np.asarray(v, dtype=i64) * 256
    E, cov = [], np.ones(len(rows), bool)
    for a, b in ((1, 2), (2, 0), (0, 1)):
        dx, dy = X[:, b] - X[:, a], Y[:, b] - Y[:, a]
        e = dx * (py - Y[:, a]) - dy * (px - X[:, a])
        top_left = (dy < 0) | ((dy == 0) & (dx > 0))
        cov &= (e > 0) | ((e == 0) & top_left)
        E.append(e)
    return np.stack(E), cov


def weights(s, rows, E):
    """-> (w [3, n] float64, sum [n] float64) in the written association"""
    iz = f64(1.0) / s["Pz"][rows].astype(f64)                    # [n, 3]
    w = E.astype(f64) * iz.T
    return w, (w[0] + w[1]) + w[2]


def render(vertices, faces, K, M, H, W, *, colors=None, cull_back=False, max_depth=10.0, want_normals=False, want_face_pixels=False,
           want_fragments=False):
    """-> dict(depth, index, colors (or None), normal (or None), face_pixels (or None), stats [N,8]); with want_fragments also
    fragments: dict of n, f, u, v (int64), z (f32), zmin, zmax (f32: the face's smallest and largest P_z) per offer."""
    vertices = np.asarray(vertices, dtype=f32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    K, M = np.asarray(K, dtype=f32), np.asarray(M, dtype=f32)
    N, F = M.shape[0], faces.shape[0]
    if K.ndim == 2:
        K = np.broadcast_to(K, (N, 3, 3))
    depth = np.full((N, 1, H, W), np.inf, f32)
    index = np.full((N, 1, H, W), -1, np.int32)
    out_c = None if colors is None else np.zeros((N, 3, H, W), f32)
    out_n = np.zeros((N, 3, H, W), f32) if want_normals else None
    face_pixels = np.zeros(F, np.int32) if want_face_pixels else None
    stats = np.zeros((N, 8), np.int32)
    frag = {k: [] for k in ("n", "f", "u", "v", "z", "zmin", "zmax")}
    for n in range(N):
        s = setup(vertices, faces, K, M, n, H, W, max_depth, cull_back)
        keys = np.full(H * W, EMPTY, np.uint64)
        rows = np.nonzero(s["drawn"])[0]
        n_frag = 0
        if rows.size:
            bw, bh = (s["u_hi"] - s["u_lo"] + 1)[rows], (s["v_hi"] - s["v_lo"] + 1)[rows]
            for dv in range(int(bh.max())):
                for du in range(int(bw[bh > dv].max())):
                    act = rows[(bw > du) & (bh > dv)]
                    u, v = s["u_lo"][act] + du, s["v_lo"][act] + dv
                    E, cov = edges(s, act, u, v)
                    if not cov.any():
                        continue
                    act, u, v, E = act[cov], u[cov], v[cov], E[:, cov]
                    _, sw = weights(s, act, E)
                    z = (s["A"][act].astype(f64) / sw).astype(f32)
                    key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | act.astype(np.uint64)
                    np.minimum.at(keys, v * W + u, key)
                    n_frag += act.size
                    if want_fragments:
                        for name, val in (("n", np.full(act.size, n, i64)), ("f", act), ("u", u), ("v", v), ("z", z),
                                          ("zmin", s["Pz"][act].min(1)), ("zmax", s["Pz"][act].max(1))):
                            frag[name].append(val)
        hit = keys != EMPTY
        win = (keys & np.uint64(0xFFFFFFFF)).astype(i64)
        depth[n, 0] = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(f32), f32(np.inf)).reshape(H, W)
        index[n, 0] = np.where(hit, win, -1).astype(np.int32).reshape(H, W)
        pix = np.nonzero(hit)[0]
        wf = win[pix]
        if pix.size and colors is not None:
            c = np.asarray(colors, dtype=f32).reshape(-1, 3).astype(f64)
            E, _ = edges(s, wf, pix % W, pix // W)
            w, sw = weights(s, wf, E)
            vid = np.take_along_axis(faces[wf].astype(i64), s["order"][wf], 1)                   # oriented numbering
            for ch in range(3):
                val = ((w[0] * c[vid[:, 0], ch] + w[1] * c[vid[:, 1], ch]) + w[2] * c[vid[:, 2], ch]) / sw
                out_c[n, ch].reshape(-1)[pix] = val.astype(f32)
        if pix.size and want_normals:
            P = s["P"][wf].astype(f64)                           # [n, vertex, axis], the face's own numbering
            a, b = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
            m = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                          a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
            with np.errstate(all="ignore"):
                length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
                ok = (length > 0) & (length < np.inf)
                unit = m / length[:, None]
                away = (unit[:, 0] * P[:, 0, 0] + unit[:, 1] * P[:, 0, 1]) + unit[:, 2] * P[:, 0, 2]
                unit = np.where((away > 0)[:, None], -unit, unit)
                val = np.where(ok[:, None], unit, 0.0).astype(f32)
            for ch in range(3):
                out_n[n, ch].reshape(-1)[pix] = val[:, ch]
        if want_face_pixels and pix.size:
            np.add.at(face_pixels, wf, 1)
        stats[n] = [s["front"].sum(), s["drawn"].sum(), s["straddling"].sum(), s["outside"].sum(), s["back"].sum(),
                    s["degenerate"].sum(), n_frag, hit.sum()]
    out = dict(depth=depth, index=index, colors=out_c, normal=out_n, face_pixels=face_pixels, stats=stats)
    if want_fragments:
        empty = dict(n=i64, f=i64, u=i64, v=i64, z=f32, zmin=f32, zmax=f32)
        out["fragments"] = {k: (np.concatenate(val) if val else np.zeros(0, empty[k])) for k, val in frag.items()}
    return out


@functools.lru_cache(maxsize=4)
def tube_mesh(N, H, W, voxel, max_depth=4.5, min_obs=1):
    """The surface-net mesh (tests/tsdf_ref.py) of the tube scene of tests/consistency_ref.py, coloured -> (mesh dict, depths, K, M).
    Shared by the tests and left unchanged by them."""
    from coivo_amd import inference as I
    import torch
    from tests import consistency_ref as CR
    from tests import tsdf_ref as TR
    depths, K, M = CR.tube_scene(N, H, W, 3)
    colors = np.random.default_rng(N * H + W).random((N, 3, H, W)).astype(f32)
    origin, dims = I.fusion_grid(torch.from_numpy(K), torch.from_numpy(M), H, W, voxel, max_depth)
    vol = TR.fuse_tsdf(depths, K, M, voxel_size=voxel, colors=colors, max_depth=max_depth, origin=origin, dims=dims)
    mesh = TR.extract_mesh(vol, min_obs=min_obs)
    for a in mesh.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return mesh, depths, K, M
