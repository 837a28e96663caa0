"""NumPy replica of the multi-view depth consistency contract (include/colvo.h colvo_consistency_*) -- test
infrastructure in the manner of tests/fuse_ref.py.  float32 with one rounding per operation, in the contract's order, for
everything that decides a vote (NumPy never contracts a multiply and an add); float64 for the relative transforms; integer
sums.  The GPU tests demand equality with it to the bit.  Also the synthetic scene the tests use: the inside of a tube.
"""
import numpy as np

f32 = np.float32
Z_EPS = f32(1e-3)
NONE, INVISIBLE, AGREE, OCCLUDED, VIOLATED = -1, 0, 1, 2, 3       # class of a (pixel, neighbour slot) sample


# ---- the scene --------------------------------------------------------------------------------------------------------- #
def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                     [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                     [-sy, cy * sx, cy * cx]], np.float64)


def tube_scene(N, H, W, seed, advance=0.05, jitter_t=0.02, jitter_r=0.02, K=None):
    """The inside of a unit cylinder about the world z axis, seen by N cameras that sit near the axis, look along it and advance
    `advance` per frame, each with a small random rotation (R = Rz Ry Rx, angles ~ jitter_r) and offset (~ jitter_t).
    fx = fy = 0.8 W, principal point at the image centre (or the per-frame intrinsics K [N,3,3] given).  depths are the exact ray-cylinder z-depth of every pixel in float64,
    rounded to float32 (the pixels that look down the lumen are far away: with max_depth = 4.5 about 13 % are no candidates).
    -> (depths [N,1,H,W], K [N,3,3], cam2world [N,4,4]) float32; the depths belong to the float32 cam2world and K."""
    rng = np.random.default_rng(seed)
    if K is None:
        K = np.zeros((N, 3, 3), f32)
        K[:, 0, 0] = K[:, 1, 1] = f32(0.8 * W)
        K[:, 0, 2] = f32((W - 1) / 2)
        K[:, 1, 2] = f32((H - 1) / 2)
        K[:, 2, 2] = 1
    K = np.ascontiguousarray(K, dtype=f32)
    M = np.zeros((N, 4, 4), f32)
    for n in range(N):
        M[n, :3, :3] = _rot(*(jitter_r * rng.standard_normal(3)))
        M[n, :3, 3] = jitter_t * rng.standard_normal(3) + np.array([0.0, 0.0, advance * n])
        M[n, 3, 3] = 1
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depths = np.empty((N, 1, H, W), f32)
    for n in range(N):
        k, m = K[n].astype(np.float64), M[n].astype(np.float64)
        ray = np.stack([(u - k[0, 2]) / k[0, 0], (v - k[1, 2]) / k[1, 1], np.ones_like(u)], -1) @ m[:3, :3].T    # world, per unit z-depth
        o = m[:3, 3]
        a = ray[..., 0] ** 2 + ray[..., 1] ** 2
        b = 2.0 * (o[0] * ray[..., 0] + o[1] * ray[..., 1])
        c = o[0] ** 2 + o[1] ** 2 - 1.0                                    # < 0: the camera is inside
        with np.errstate(all="ignore"):
            z = (-b + np.sqrt(b * b - 4.0 * a * c)) / (2.0 * a)
        depths[n, 0] = np.where(a > 0, z, np.inf).astype(f32)
    return depths, K, M


def blocks(H, W):
    """The two blocks corrupt() scales: ((v0, v1, u0, u1) scaled by 0.7, (...) scaled by 1.4), half-open, in opposite corners
    of the image where the wall is near."""
    bh, bw = max(2, H // 6), max(2, W // 6)
    v0, u0 = H // 8, W // 8
    return (v0, v0 + bh, u0, u0 + bw), (H - v0 - bh, H - v0, W - u0 - bw, W - u0)


def block_mask(H, W):
    m = np.zeros((2, H, W), bool)
    for k, (v0, v1, u0, u1) in enumerate(blocks(H, W)):
        m[k, v0:v1, u0:u1] = True
    return m


def corrupt(depths, frame):
    """A copy of depths with one block of `frame` scaled by 0.7 (a floater in front of the wall) and another by 1.4 (a hole
    behind it)."""
    out = np.array(depths, dtype=f32, copy=True)
    for (v0, v1, u0, u1), scale in zip(blocks(*depths.shape[2:]), (f32(0.7), f32(1.4))):
        out[frame, 0, v0:v1, u0:u1] *= scale
    return out


# ---- the contract ------------------------------------------------------------------------------------------------------ #
def neighbours(N, window, step):
    """[N, 2 * window] frame index of every neighbour slot (k = -window..-1, 1..window: ascending), -1 where it does not exist."""
    k = np.concatenate([np.arange(-window, 0), np.arange(1, window + 1)])
    j = np.arange(N)[:, None] + k[None] * int(step)
    return np.where((j >= 0) & (j < N), j, -1)


def rel_table(M, window, step):
    """[N, 2 * window, 12] float32: R (row-major) and t of the transform frame i -> neighbour, float64 from the float32
    cam2world, every value rounded once; zeros where the neighbour does not exist."""
    M = np.asarray(M, dtype=f32).astype(np.float64)
    N = M.shape[0]
    nbr = neighbours(N, window, step)
    out = np.zeros((N, 2 * window, 12), f32)
    for i in range(N):
        for s, j in enumerate(nbr[i]):
            if j < 0:
                continue
            Ri, Rj, dt = M[i, :3, :3], M[j, :3, :3], M[i, :3, 3] - M[j, :3, 3]
            for a in range(3):
                for b in range(3):
                    out[i, s, a * 3 + b] = f32((Rj[0, a] * Ri[0, b] + Rj[1, a] * Ri[1, b]) + Rj[2, a] * Ri[2, b])
                out[i, s, 9 + a] = f32((Rj[0, a] * dt[0] + Rj[1, a] * dt[1]) + Rj[2, a] * dt[2])
    return out


def filter_depths(depths, K, M, *, window=2, step=1, rel_tol=0.01, min_agree=1, max_violated=0, max_depth=10.0, detail=False):
    """-> dict(depths [N,1,H,W] f32 (+inf where not kept), votes [N,3,H,W] u8, stats [N,5] i32).  With detail also, per
    (frame, slot, pixel): cls int8 (NONE for no candidate or no neighbour, else INVISIBLE / AGREE / OCCLUDED / VIOLATED), rel f32
    (NaN where not visible) and the first tap x0, y0 (int32, -1 where the point is not in front of and inside the neighbour)."""
    depths, K, M = (np.asarray(a, dtype=f32) for a in (depths, K, M))
    N, _, H, W = depths.shape
    rel_tol, max_depth = f32(rel_tol), f32(max_depth)
    nbr = neighbours(N, window, step)
    T = rel_table(M, window, step)
    v, u = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    out_d = np.full((N, 1, H, W), np.inf, f32)
    votes = np.zeros((N, 3, H, W), np.uint8)
    stats = np.zeros((N, 5), np.int32)
    if detail:
        cls = np.full((N, 2 * window, H, W), NONE, np.int8)
        rels = np.full((N, 2 * window, H, W), np.nan, f32)
        tx0 = np.full((N, 2 * window, H, W), -1, np.int32)
        ty0 = np.full((N, 2 * window, H, W), -1, np.int32)
    with np.errstate(all="ignore"):
        for i in range(N):
            d = depths[i, 0]
            cand = (d > 0) & (d < max_depth)
            px = ((u - K[i, 0, 2]) / K[i, 0, 0]) * d
            py = ((v - K[i, 1, 2]) / K[i, 1, 1]) * d
            cnt = np.zeros((3, H, W), np.int64)
            for s, j in enumerate(nbr[i]):
                if j < 0:
                    continue
                t = T[i, s]
                P = [((t[3 * a] * px + t[3 * a + 1] * py) + t[3 * a + 2] * d) + t[9 + a] for a in range(3)]
                x = (K[j, 0, 0] * P[0]) / P[2] + K[j, 0, 2]
                y = (K[j, 1, 1] * P[1]) / P[2] + K[j, 1, 2]
                assert x.dtype == f32 and y.dtype == f32
                seen = cand & (P[2] > Z_EPS) & (x >= 0) & (x <= f32(W - 1)) & (y >= 0) & (y <= f32(H - 1))
                x0f, y0f = np.floor(x), np.floor(y)
                wx, wy = x - x0f, y - y0f
                x0 = np.where(seen, x0f, 0).astype(np.int64)
                y0 = np.where(seen, y0f, 0).astype(np.int64)
                x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
                dj = depths[j, 0]
                t00, t01, t10, t11 = dj[y0, x0], dj[y0, x1], dj[y1, x0], dj[y1, x1]
                visible = seen
                for tap in (t00, t01, t10, t11):
                    visible = visible & (tap > 0) & (tap < max_depth)
                ax, ay = f32(1) - wx, f32(1) - wy
                sd = (((t00 * ax) + (t01 * wx)) * ay) + (((t10 * ax) + (t11 * wx)) * wy)
                rel = np.abs(P[2] - sd) / (P[2] + sd)
                assert rel.dtype == f32
                ok, occ = rel < rel_tol, sd < P[2]
                cnt[0] += visible & ok
                cnt[1] += visible & ~ok & occ
                cnt[2] += visible & ~ok & ~occ
                if detail:
                    cls[i, s] = np.where(~cand, NONE, np.where(~visible, INVISIBLE, np.where(ok, AGREE, np.where(occ, OCCLUDED, VIOLATED))))
                    rels[i, s] = np.where(visible, rel, np.nan)
                    tx0[i, s] = np.where(seen, x0, -1)
                    ty0[i, s] = np.where(seen, y0, -1)
            n_vis = cnt.sum(0)
            enough, clean = cnt[0] >= min_agree, cnt[2] <= max_violated
            kept = cand & enough & clean
            out_d[i, 0] = np.where(kept, d, f32(np.inf))
            votes[i] = cnt.astype(np.uint8)
            stats[i] = [cand.sum(), kept.sum(), (cand & ~kept & (n_vis == 0)).sum(), (cand & clean & ~enough & (n_vis > 0)).sum(),
                        (cand & ~clean).sum()]
    out = dict(depths=out_d, votes=votes, stats=stats)
    if detail:
        out.update(cls=cls, rel=rels, x0=tx0, y0=ty0, neighbours=nbr)
    return out
