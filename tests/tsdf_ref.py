"""NumPy replica of the TSDF fusion and surface-net meshing contract (include/colvo.h colvo_tsdf_*) -- test
infrastructure in the manner of tests/fuse_ref.py.  float32 with one rounding per operation for everything that decides a brick, a
pixel or a quantum (NumPy never contracts a multiply and an add), int64 sums, float64 in the written association for the vertices;
the GPU tests demand equality with it to the bit.  The replica does not cull frames: the sums are integers, so skipping a frame that
adds nothing cannot move a bit.
"""
import numpy as np

f32 = np.float32
f64 = np.float64
BRICK = 8
BRICK_VOX = 512
Z_EPS = f32(1e-3)
Q_ONE = 4096

# the cell's 12 edges in the contract's order: (axis, corner a, corner b), a corner being (x, y, z) in {0, 1}^3.  Per axis the two
# other coordinates run (0,0), (1,0), (0,1), (1,1), the lower axis fastest.
EDGES = []
for _axis in range(3):
    _o = [a for a in range(3) if a != _axis]
    for _p in range(4):
        _a = [0, 0, 0]
        _a[_o[0]], _a[_o[1]] = _p & 1, _p >> 1
        _b = list(_a)
        _b[_axis] = 1
        EDGES.append((_axis, tuple(_a), tuple(_b)))


def sphere_scene(radius, S):
    """A sphere of `radius` seen from its centre (the world origin) by six cameras of S x S pixels with 90-degree fields, one along
    each axis direction: (depths [6,1,S,S], K [6,3,3], cam2world [6,4,4]) float32.  A pixel column covers (u - cx) / fx in
    [-1, 1) -- half-open, so every direction belongs to exactly one camera; the rotations are signed permutations, exact in float32."""
    K = np.zeros((6, 3, 3), f32)
    K[:, 0, 0] = K[:, 1, 1] = S / 2.0
    K[:, 0, 2] = K[:, 1, 2] = S / 2.0 - 0.5
    K[:, 2, 2] = 1
    M = np.zeros((6, 4, 4), f32)
    M[:, 3, 3] = 1
    i = 0
    for axis in range(3):
        for sign in (1.0, -1.0):
            z = np.zeros(3); z[axis] = sign
            x = np.zeros(3); x[(axis + 1) % 3] = 1.0
            M[i, :3, 0], M[i, :3, 1], M[i, :3, 2] = x, np.cross(z, x), z
            i += 1
    v, u = np.meshgrid(np.arange(S, dtype=f64), np.arange(S, dtype=f64), indexing="ij")
    x, y = (u - (S / 2.0 - 0.5)) / (S / 2.0), (v - (S / 2.0 - 0.5)) / (S / 2.0)
    d = (radius / np.sqrt(x * x + y * y + 1.0)).astype(f32)
    return np.ascontiguousarray(np.broadcast_to(d, (6, 1, S, S))), K, M


def check_trunc(voxel_size, trunc):
    """-> (T, trunc as float32): trunc=None is four voxels; else a whole number of voxels 1..7."""
    vs = f32(voxel_size)
    if trunc is None:
        T = 4
    else:
        T = int(round(float(trunc) / float(vs)))
        if not 1 <= T <= 7 or abs(float(trunc) - T * float(vs)) > 1e-5 * float(trunc):
            raise ValueError("trunc must be a whole number of voxels, 1 to 7")
    return T, f32(T) * vs


def _locate(K, M, u, v, d, origin, voxel_size, dims):
    """voxel_grid::locate on samples (u, v [Hs,Ws] float32; d [N,Hs,Ws]): (inside [N,Hs,Ws], idx [3][N,Hs,Ws] int64, 0 outside)."""
    inv = f32(1) / f32(voxel_size)
    k = lambda i, j: K[:, i, j][:, None, None]
    m = lambda i, j: M[:, i, j][:, None, None]
    with np.errstate(all="ignore"):
        px = (u[None] - k(0, 2)) / k(0, 0) * d
        py = (v[None] - k(1, 2)) / k(1, 1) * d
        inside = np.ones(d.shape, bool)
        idx = []
        for a in range(3):
            X = ((m(a, 0) * px + m(a, 1) * py) + m(a, 2) * d) + m(a, 3)
            g = (X - f32(origin[a])) * inv
            assert g.dtype == f32
            inside = inside & (g >= 0) & (g < f32(dims[a]))
            idx.append(np.where(inside, np.floor(g), f32(0)).astype(np.int64))
    idx = [np.where(inside, i, 0) for i in idx]
    return inside, idx


def plan(depths, K, M, *, stride, max_depth, voxel_size, T, origin, dims):
    """-> dict(brick_list [n_bricks] ascending, table [bricks] slot or -1, n_input, n_outside)."""
    depths, K, M = (np.asarray(a, dtype=f32) for a in (depths, K, M))
    N, _, H, W = depths.shape
    vs = f32(voxel_size)
    nb = [x // BRICK for x in dims]
    d = depths[:, 0, ::stride, ::stride]
    v, u = np.meshgrid(np.arange(0, H, stride, dtype=f32), np.arange(0, W, stride, dtype=f32), indexing="ij")
    with np.errstate(all="ignore"):
        kept = (d > 0) & (d < f32(max_depth))
    marks = np.zeros(nb[0] * nb[1] * nb[2], bool)
    n_outside = 0
    for k in range(-(T + 1), T + 2):
        with np.errstate(all="ignore"):
            dk = d + f32(k) * vs
            ok = kept & (dk > 0)
        inside, idx = _locate(K, M, u, v, dk, origin, vs, dims)
        inside &= ok
        brick = ((idx[2] // BRICK) * nb[1] + idx[1] // BRICK) * nb[0] + idx[0] // BRICK
        marks[brick[inside]] = True
        if k == 0:
            n_outside = int((kept & ~inside).sum())
    brick_list = np.nonzero(marks)[0].astype(np.int32)
    table = np.full(marks.size, -1, np.int32)
    table[brick_list] = np.arange(len(brick_list), dtype=np.int32)
    return dict(brick_list=brick_list, table=table, n_input=int(kept.sum()), n_outside=n_outside)


def _voxel_index(brick_list, dims):
    """[n_bricks * 512, 3] int64: the grid index of every pool record, in (slot, local) order."""
    nb = [x // BRICK for x in dims]
    b = np.asarray(brick_list, np.int64)
    bx, by, bz = b % nb[0], (b // nb[0]) % nb[1], b // (nb[0] * nb[1])
    loc = np.arange(BRICK_VOX)
    i = np.stack([bx[:, None] * BRICK + (loc & 7)[None], by[:, None] * BRICK + ((loc >> 3) & 7)[None],
                  bz[:, None] * BRICK + (loc >> 6)[None]], -1)
    return i.reshape(-1, 3)


def integrate(depths, colors, K, M, *, max_depth, voxel_size, T, origin, dims, brick_list, frames=None):
    """-> (pool [n_bricks * 512, 2] int32: sum q and n; colour sums [n_bricks * 512, 4] int32 (last column 0) or None).  `frames`:
    the frame indices to integrate, in that order (default: all)."""
    depths, K, M = (np.asarray(a, dtype=f32) for a in (depths, K, M))
    N, _, H, W = depths.shape
    vs = f32(voxel_size)
    trunc = f32(T) * vs
    inv_trunc = f32(1) / trunc
    idx = _voxel_index(brick_list, dims)
    c = [f32(origin[a]) + (idx[:, a].astype(f32) + f32(0.5)) * vs for a in range(3)]
    assert all(x.dtype == f32 for x in c)
    sq = np.zeros(len(idx), np.int64)
    n = np.zeros(len(idx), np.int64)
    sc = np.zeros((len(idx), 4), np.int64) if colors is not None else None
    col = np.asarray(colors, dtype=f32) if colors is not None else None
    for f in (range(N) if frames is None else frames):
        r = M[f, :3, :3]
        t = M[f, :3, 3]
        fx, fy, cx, cy = K[f, 0, 0], K[f, 1, 1], K[f, 0, 2], K[f, 1, 2]
        with np.errstate(all="ignore"):
            q0, q1, q2 = c[0] - t[0], c[1] - t[1], c[2] - t[2]
            Px = (r[0, 0] * q0 + r[1, 0] * q1) + r[2, 0] * q2
            Py = (r[0, 1] * q0 + r[1, 1] * q1) + r[2, 1] * q2
            Pz = (r[0, 2] * q0 + r[1, 2] * q1) + r[2, 2] * q2
            x = (fx * Px) / Pz + cx
            y = (fy * Py) / Pz + cy
            xf = np.floor(x + f32(0.5))
            yf = np.floor(y + f32(0.5))
            ok = (Pz > Z_EPS) & (xf >= 0) & (xf < f32(W)) & (yf >= 0) & (yf < f32(H))
            uu = np.where(ok, xf, f32(0)).astype(np.int64)
            vv = np.where(ok, yf, f32(0)).astype(np.int64)
            d = depths[f, 0][vv, uu]
            ok &= (d > 0) & (d < f32(max_depth))
            sdf = d - Pz
            ok &= ~(sdf < -trunc)
            tt = np.minimum(sdf, trunc) * inv_trunc
            assert tt.dtype == f32
            q = np.where(ok, np.rint(tt * f32(Q_ONE)), f32(0)).astype(np.int64)
        assert np.abs(q).max(initial=0) <= Q_ONE
        sq += q
        n += ok
        if sc is not None:
            with np.errstate(all="ignore"):
                for k in range(3):
                    cq = np.clip(np.nan_to_num(np.rint(col[f, k][vv, uu] * f32(255)), nan=0.0, posinf=255.0, neginf=0.0), 0, 255)
                    sc[:, k] += np.where(ok, cq, 0).astype(np.int64)
    pool = np.stack([sq, n], 1).astype(np.int32)
    return pool, (sc.astype(np.int32) if sc is not None else None)


def fuse_tsdf(depths, K, M, *, voxel_size, trunc=None, colors=None, stride=1, max_depth=10.0, origin, dims, frames=None):
    """The whole volume: dict(pool, color_sums, brick_list, table, origin, dims, voxel_size, trunc, T, n_input, n_outside, n_bricks)."""
    dims = [int(x) for x in dims]
    assert all(x > 0 and x % BRICK == 0 for x in dims)
    T, tr = check_trunc(voxel_size, trunc)
    p = plan(depths, K, M, stride=stride, max_depth=max_depth, voxel_size=voxel_size, T=T, origin=origin, dims=dims)
    pool, sc = integrate(depths, colors, K, M, max_depth=max_depth, voxel_size=voxel_size, T=T, origin=origin, dims=dims,
                         brick_list=p["brick_list"], frames=frames)
    return dict(pool=pool, color_sums=sc, brick_list=p["brick_list"], table=p["table"], origin=tuple(f32(o) for o in origin),
                dims=tuple(dims), voxel_size=f32(voxel_size), trunc=tr, T=T, n_input=p["n_input"], n_outside=p["n_outside"],
                n_bricks=int(len(p["brick_list"])))


def _pool_index(vol, idx):
    """pool row of the voxels idx [..., 3] (int64), -1 outside the grid or in a brick that is not allocated"""
    dims = vol["dims"]
    nb = [x // BRICK for x in dims]
    x, y, z = (np.ascontiguousarray(idx[..., a]).astype(np.int32) for a in range(3))
    inside = (x >= 0) & (x < dims[0]) & (y >= 0) & (y < dims[1]) & (z >= 0) & (z < dims[2])
    x, y, z = (np.where(inside, c, 0) for c in (x, y, z))
    brick = ((z >> 3) * nb[1] + (y >> 3)) * nb[0] + (x >> 3)
    local = ((z & 7) * BRICK + (y & 7)) * BRICK + (x & 7)
    slot = vol["table"][brick]
    return np.where(inside & (slot >= 0), slot.astype(np.int64) * BRICK_VOX + local, -1)


def extract_mesh(vol, *, min_obs=1):
    """-> dict(vertices [V,3] f32, cells [V,3] i32, colors [V,3] f32 or None, normals [V,3] f32, faces [F,3] i32, n_open).
    Cells are those whose minimum corner lies in an allocated brick, in (slot, local) order of that corner."""
    pool = vol["pool"].astype(np.int64)
    sc = vol["color_sums"]
    idx = _voxel_index(vol["brick_list"], vol["dims"])                       # the cells' minimum corners
    n_cells = len(idx)
    corners = [(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)]    # corner c = x + 2 y + 4 z
    row = np.stack([_pool_index(vol, idx + np.array(c)) for c in corners], 1) if n_cells else np.zeros((0, 8), np.int64)
    safe = np.maximum(row, 0)
    cn = np.where(row >= 0, pool[safe, 1] if n_cells else 0, 0)
    obs = cn >= min_obs
    csq = np.where(obs, pool[safe, 0] if n_cells else 0, 0)
    neg = obs & (csq < 0)
    n_obs, n_neg = obs.sum(1), neg.sum(1)
    mixed = (n_neg > 0) & (n_neg < n_obs)
    active = mixed & (n_obs == 8)
    n_open = int((mixed & (n_obs < 8)).sum())
    act = np.nonzero(active)[0]
    V = len(act)
    vid = np.full(n_cells, -1, np.int64)
    vid[act] = np.arange(V)
    # ---- vertices ----
    phi = csq[act].astype(f64) / np.maximum(cn[act], 1).astype(f64)          # [V,8]
    ins = neg[act]
    cidx = lambda c: c[0] + 2 * c[1] + 4 * c[2]
    m = np.zeros((V, 3), f64)
    cnt = np.zeros(V, np.int64)
    grad = [None, None, None]
    for axis, a, b in EDGES:
        pa, pb = phi[:, cidx(a)], phi[:, cidx(b)]
        cross = ins[:, cidx(a)] != ins[:, cidx(b)]
        with np.errstate(all="ignore"):
            t = pa / (pa - pb)
        for ax in range(3):
            m[:, ax] += np.where(cross, t if ax == axis else f64(a[ax]), 0.0)
        cnt += cross
        dlt = pb - pa
        grad[axis] = dlt if grad[axis] is None else grad[axis] + dlt
    assert V == 0 or cnt.min() >= 1
    m = m / cnt.astype(f64)[:, None]
    o64 = np.array([f64(f32(o)) for o in vol["origin"]])
    vs64 = f64(f32(vol["voxel_size"]))
    cells = idx[act]
    vertices = (o64[None] + ((cells.astype(f64) + 0.5) + m) * vs64).astype(f32)
    g = np.stack(grad, 1) if V else np.zeros((0, 3), f64)
    length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    with np.errstate(all="ignore"):
        normals = np.where(length[:, None] > 0, g / length[:, None], 0.0).astype(f32)
    colors = None
    if sc is not None:
        csum = np.zeros((V, 3), f64)
        for c in range(8):
            r = row[act, c]
            csum += sc[r, :3].astype(f64) / (255.0 * cn[act, c].astype(f64))[:, None]
        colors = (csum / 8.0).astype(f32)
    # ---- faces: the owner voxel is a cell's minimum corner, and that cell (C below) must be active itself; axis 0..2 ----
    faces = []
    own_sq = pool[act, 0]
    idx = idx[act]
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        e = np.zeros(3, np.int64); e[axis] = 1
        du = np.zeros(3, np.int64); du[u] = 1
        dw = np.zeros(3, np.int64); dw[w] = 1
        quad = []
        for off in (-du - dw, -dw, np.zeros(3, np.int64), -du):           # A, B, C, D: counter-clockwise seen from +axis
            r = _pool_index(vol, idx + off)
            quad.append(np.where(r >= 0, vid[np.maximum(r, 0)], -1))
        quad = np.stack(quad, 1) if V else np.zeros((0, 4), np.int64)
        far = _pool_index(vol, idx + e)
        far_sq = np.where(far >= 0, pool[np.maximum(far, 0), 0], 0)
        has = (quad >= 0).all(1) & ((own_sq < 0) != (far_sq < 0))
        o = np.nonzero(has)[0]
        A, B, C, D = (quad[o, i] for i in range(4))
        fwd = own_sq[o] < 0                                               # inside at the owner: the normal points along +axis
        t1 = np.where(fwd[:, None], np.stack([A, B, C], 1), np.stack([A, C, B], 1))
        t2 = np.where(fwd[:, None], np.stack([A, C, D], 1), np.stack([A, D, C], 1))
        faces.append((act[o] * 3 + axis, t1, t2))
    key = np.concatenate([f[0] for f in faces])
    order = np.argsort(key, kind="stable")
    t1 = np.concatenate([f[1] for f in faces])[order]
    t2 = np.concatenate([f[2] for f in faces])[order]
    tri = np.stack([t1, t2], 1).reshape(-1, 3).astype(np.int32)
    return dict(vertices=vertices.reshape(-1, 3), cells=cells.astype(np.int32).reshape(-1, 3), colors=colors,
                normals=normals.reshape(-1, 3), faces=tri, n_open=n_open)
