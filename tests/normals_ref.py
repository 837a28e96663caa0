"""NumPy replica of the cloud-normals contract (include/colvo.h colvo_cloud_normals) -- test infrastructure in the
manner of tests/fuse_ref.py, whose pinned grid coordinates it imports.  float32 with one rounding per operation (NumPy never contracts
a multiply and an add, divides and takes square roots correctly rounded, and keeps denormals), int64 sums, float64 for the write-out;
the GPU tests demand equality with it to the bit.  The contract, restated, per walked sample c = (u, v) with 0 < d_c < max_depth:

  points    P = (((u - cx) / fx) * d, ((v - cy) / fy) * d, d) for c and its four neighbours one pixel away in the full-resolution map.
  usable    neighbour b: inside the image, 0 < d_b < max_depth, |d_b - d_c| < rel_edge * (d_b + d_c).
  tangents  P(u+1) - P(u-1), or one-sided with P(c) where one neighbour is not usable, or none; the same along v.
  normal    n = t_u x t_v; negated iff (n_x P_x + n_y P_y) + n_z P_z > 0;  L = sqrt((n_x^2 + n_y^2) + n_z^2); has a normal iff both
            tangents exist, L > 0 and L < inf.
  world     e = n / L, N_a = (r_a0 e_x + r_a1 e_y) + r_a2 e_z, q_a = int(rint(N_a * 16384)).
  row       the fusion's voxel of the sample, looked up among the cloud's rows by its key brick * 512 + local.
  write     len = sqrt((sx sx + sy sy) + sz sz) in float64; normal = s / len, coherence = len / (16384 n); 0 where n = 0 or len = 0.
"""
import numpy as np

from tests import fuse_ref as F

f32 = np.float32
BRICK = F.BRICK
QUANTUM = f32(16384.0)


def _shift(a, du, dv, fill):
    """a[..., v + dv, u + du] where that lies inside the map, `fill` elsewhere (a is [..., H, W])."""
    out = np.full_like(a, fill)
    H, W = a.shape[-2:]
    vs, vd = (slice(dv, H), slice(0, H - dv)) if dv >= 0 else (slice(0, H + dv), slice(-dv, H))
    us, ud = (slice(du, W), slice(0, W - du)) if du >= 0 else (slice(0, W + du), slice(-du, W))
    out[..., vd, ud] = a[..., vs, us]
    return out


def sample_normals(depths, K, M, *, stride=1, max_depth=10.0, rel_edge=0.05):
    """Per walked sample -> dict(kept, normal (bool [N,Hs,Ws]), one_sided (bool: a tangent that is a one-sided difference), cam (float32
    [N,Hs,Ws,3]: the unit normal in the camera frame, 0 without one), q (int64 [N,Hs,Ws,3]: the quantised world normal))."""
    depths, K, M = (np.asarray(a, dtype=f32) for a in (depths, K, M))
    N, _, H, W = depths.shape
    d = depths[:, 0]
    max_depth, rel_edge = f32(max_depth), f32(rel_edge)
    v, u = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    k = lambda i, j: K[:, i, j][:, None, None]
    with np.errstate(all="ignore"):
        valid = (d > 0) & (d < max_depth)
        P = np.stack([(u[None] - k(0, 2)) / k(0, 0) * d, (v[None] - k(1, 2)) / k(1, 1) * d, d])          # [3,N,H,W]
        assert P.dtype == f32
        use, Pn = [], []
        for du, dv in ((-1, 0), (1, 0), (0, -1), (0, 1)):                 # left, right, up, down
            db = _shift(d, du, dv, f32(0))
            use.append(_shift(valid, du, dv, False) & (np.abs(db - d) < rel_edge * (db + d)))
            Pn.append(_shift(P, du, dv, f32(0)))
        tu = np.where(use[1], Pn[1], P) - np.where(use[0], Pn[0], P)
        tv = np.where(use[3], Pn[3], P) - np.where(use[2], Pn[2], P)
        n = np.stack([tu[1] * tv[2] - tu[2] * tv[1], tu[2] * tv[0] - tu[0] * tv[2], tu[0] * tv[1] - tu[1] * tv[0]])
        away = (n[0] * P[0] + n[1] * P[1]) + n[2] * P[2] > 0
        n = np.where(away, -n, n)
        L = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        normal = valid & (use[0] | use[1]) & (use[2] | use[3]) & (L > 0) & (L < f32(np.inf))
        e = np.where(normal, n / L, f32(0))
        m = lambda a, b: M[:, a, b][:, None, None]
        Nw = np.stack([(m(a, 0) * e[0] + m(a, 1) * e[1]) + m(a, 2) * e[2] for a in range(3)])
        assert Nw.dtype == f32 and L.dtype == f32
        q = np.where(normal, np.rint(Nw * QUANTUM), f32(0)).astype(np.int64)
    one_sided = normal & ((use[0] ^ use[1]) | (use[2] ^ use[3]))
    s = (slice(None), slice(None, None, stride), slice(None, None, stride))
    return dict(kept=valid[s], normal=normal[s], one_sided=one_sided[s], cam=np.moveaxis(e, 0, -1)[s], q=np.moveaxis(q, 0, -1)[s],
                use=[x[s] for x in use])


def voxel_keys(voxels, dims):
    """brick * 512 + local of voxel indices [M,3], the order a fused cloud's rows are in."""
    vox = np.asarray(voxels).astype(np.int64).reshape(-1, 3)
    nb = [int(x) // BRICK for x in dims]
    brick = ((vox[:, 2] // BRICK) * nb[1] + vox[:, 1] // BRICK) * nb[0] + vox[:, 0] // BRICK
    local = ((vox[:, 2] % BRICK) * BRICK + vox[:, 1] % BRICK) * BRICK + vox[:, 0] % BRICK
    return brick * 512 + local


def sample_keys(depths, K, M, *, stride, max_depth, voxel_size, origin, dims):
    """(inside [N,Hs,Ws] bool, key int64 [N,Hs,Ws], -1 where not inside): the fusion's voxel of every walked sample."""
    d, g = F.grid_coords(depths, K, M, stride, origin, voxel_size)
    with np.errstate(all="ignore"):
        inside = (d > 0) & (d < f32(max_depth))
        for a in range(3):
            inside &= (g[a] >= 0) & (g[a] < f32(int(dims[a])))
        idx = np.stack([np.where(inside, np.floor(g[a]), 0).astype(np.int64) for a in range(3)], -1)
    return inside, np.where(inside, voxel_keys(idx.reshape(-1, 3), dims).reshape(inside.shape), -1)


def cloud_normals(depths, K, M, voxels, *, stride=1, max_depth=10.0, voxel_size, origin, dims, rel_edge=0.05):
    """-> dict(normals [M,3] f32, counts [M] i32, coherence [M] f32, stats [4] i32, sums [M,3] i64)."""
    s = sample_normals(depths, K, M, stride=stride, max_depth=max_depth, rel_edge=rel_edge)
    inside, key = sample_keys(depths, K, M, stride=stride, max_depth=max_depth, voxel_size=voxel_size, origin=origin, dims=dims)
    rows = voxel_keys(voxels, dims)
    n_rows = len(rows)
    pos = np.searchsorted(rows, key, side="left")
    found = s["normal"] & inside & (pos < n_rows)
    found &= rows[np.minimum(pos, max(n_rows - 1, 0))] == key if n_rows else False
    sums = np.zeros((n_rows, 3), np.int64)
    cnt = np.zeros(n_rows, np.int64)
    np.add.at(sums, pos[found], s["q"][found])
    np.add.at(cnt, pos[found], 1)
    sd = sums.astype(np.float64)
    ln = np.sqrt((sd[:, 0] * sd[:, 0] + sd[:, 1] * sd[:, 1]) + sd[:, 2] * sd[:, 2])
    some = (cnt > 0) & (ln > 0)
    with np.errstate(all="ignore"):
        normals = np.where(some[:, None], sd / ln[:, None], 0.0).astype(f32)
        coherence = np.where(some, ln / (16384.0 * cnt.astype(np.float64)), 0.0).astype(f32)
    stats = np.array([s["kept"].sum(), s["normal"].sum(), found.sum(), (s["normal"] & ~found).sum()], np.int32)
    return dict(normals=normals.reshape(-1, 3), counts=cnt.astype(np.int32), coherence=coherence, stats=stats, sums=sums)
