"""NumPy replica of the voxel fusion contract (include/colvo.h colvo_fuse_*) -- test infrastructure in the
manner of tests/loss_ref.py.  float32 with one rounding per operation for everything that decides a sample's voxel (NumPy
never contracts a multiply and an add), int64 sums, float64 for the means; the GPU tests demand equality with it to the bit.
"""
import numpy as np
import torch

f32 = np.float32
BRICK = 8


def scene(N, H, W, seed, step_t=0.05, step_r=0.03):
    """Synthetic depths and colours (coivo_amd.synth) along a random trajectory integrated by the float64 oracle:
    (depths [N,1,H,W], colors [N,3,H,W], K [N,3,3], cam2world [N,4,4]) as float32 arrays."""
    from coivo_amd import synth
    from oracle import colvo_spec as S
    b = synth.make_batch(N, H, W, seed=seed)
    g = torch.Generator().manual_seed(seed)
    rel = torch.cat([step_t * torch.randn(N, 3, generator=g), step_r * torch.randn(N, 3, generator=g)], dim=1)
    M = S.integrate_trajectory(rel.double())[1:].float()
    return (np.ascontiguousarray(b["gt_depth"].numpy()), np.ascontiguousarray(b["tgt"].numpy()),
            np.ascontiguousarray(b["K"].numpy()), np.ascontiguousarray(M.numpy()))


def grid_coords(depths, K, M, stride, origin, voxel_size):
    """(d [N,Hs,Ws], g [3][N,Hs,Ws]): the samples' depths and float32 grid coordinates, operation for operation as the
    contract orders them."""
    depths, K, M = (np.asarray(a, dtype=f32) for a in (depths, K, M))
    N, _, H, W = depths.shape
    inv = f32(1) / f32(voxel_size)
    d = depths[:, 0, ::stride, ::stride]
    v, u = np.meshgrid(np.arange(0, H, stride, dtype=f32), np.arange(0, W, stride, dtype=f32), indexing="ij")
    k = lambda i, j: K[:, i, j][:, None, None]
    m = lambda i, j: M[:, i, j][:, None, None]
    with np.errstate(all="ignore"):
        px = (u[None] - k(0, 2)) / k(0, 0) * d
        py = (v[None] - k(1, 2)) / k(1, 1) * d
        g = []
        for a in range(3):
            X = ((m(a, 0) * px + m(a, 1) * py) + m(a, 2) * d) + m(a, 3)
            g.append((X - f32(origin[a])) * inv)
    assert all(x.dtype == f32 for x in g)
    return d, g


def fuse(depths, colors, K, M, *, stride, max_depth, voxel_size, origin, dims, min_obs=1):
    """-> dict(points [M,3] f32, colors [M,3] f32 or None, counts [M] i32, voxels [M,3] i32, n_input, n_outside, n_bricks,
    n_voxels, max_count)."""
    dims = [int(x) for x in dims]
    assert all(x > 0 and x % BRICK == 0 for x in dims)
    d, g = grid_coords(depths, K, M, stride, origin, voxel_size)
    with np.errstate(all="ignore"):
        kept = (d > 0) & (d < f32(max_depth))
        inside = kept.copy()
        for a in range(3):
            inside &= (g[a] >= 0) & (g[a] < f32(dims[a]))
        fl = [np.floor(g[a][inside]) for a in range(3)]
        idx = [fl[a].astype(np.int64) for a in range(3)]
        q = np.stack([np.floor((g[a][inside] - fl[a]) * f32(256)).astype(np.int64) for a in range(3)], 1)
    assert q.size == 0 or (q.min() >= 0 and q.max() <= 255)
    nb = [x // BRICK for x in dims]
    brick = ((idx[2] // BRICK) * nb[1] + idx[1] // BRICK) * nb[0] + idx[0] // BRICK
    local = ((idx[2] % BRICK) * BRICK + idx[1] % BRICK) * BRICK + idx[0] % BRICK
    key = brick * 512 + local
    uk, first, inverse, cnt = np.unique(key, return_index=True, return_inverse=True, return_counts=True)   # ascending (brick, local)
    inverse = inverse.reshape(-1)
    sq = np.zeros((len(uk), 3), np.int64)
    np.add.at(sq, inverse, q)
    sc = None
    if colors is not None:
        col = np.asarray(colors, dtype=f32)[:, :, ::stride, ::stride]
        with np.errstate(all="ignore"):
            c = np.stack([np.clip(np.nan_to_num(np.rint(col[:, k][inside] * f32(255)), nan=0.0, posinf=255.0, neginf=0.0), 0, 255)
                          for k in range(3)], 1).astype(np.int64)
        sc = np.zeros((len(uk), 3), np.int64)
        np.add.at(sc, inverse, c)
    vox = np.stack([idx[a][first] for a in range(3)], 1) if len(uk) else np.zeros((0, 3), np.int64)
    rows = cnt >= min_obs
    n = cnt[rows].astype(np.float64)
    o64 = np.array([np.float64(f32(o)) for o in origin])
    vs64 = np.float64(f32(voxel_size))
    pts = (o64[None] + (vox[rows].astype(np.float64) + (sq[rows].astype(np.float64) + 0.5 * n[:, None]) / (256.0 * n[:, None])) * vs64)
    out = dict(points=pts.astype(f32).reshape(-1, 3), colors=None, counts=cnt[rows].astype(np.int32),
               voxels=vox[rows].astype(np.int32).reshape(-1, 3), n_input=int(kept.sum()), n_outside=int((kept & ~inside).sum()),
               n_bricks=int(len(np.unique(brick))), n_voxels=int(len(uk)), max_count=int(cnt.max()) if len(cnt) else 0)
    if sc is not None:
        out["colors"] = (sc[rows].astype(np.float64) / (255.0 * n[:, None])).astype(f32).reshape(-1, 3)
    return out
