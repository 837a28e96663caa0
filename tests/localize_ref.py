"""NumPy replica of the polyp localisation contract (include/colvo.h colvo_localize_*) and a scene maker --
test infrastructure in the manner of tests/fuse_ref.py.  float32 with one rounding per operation for the point and its quanta
(NumPy never contracts a multiply and an add), int64 for the sums, float64 in the header's association for every output; the
GPU tests demand equality with it to the bit.
"""
import numpy as np

from tests import fuse_ref

f32 = np.float32
f64 = np.float64
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))       # xx xy xz yy yz zz


# ---- the replica -------------------------------------------------------------------------------------------------------- #
def quanta(depths, K, stride):
    """(d [N,Hs,Ws] f32, u, v [Hs,Ws] int64, q [3][N,Hs,Ws] float32 = rint(p_a * 4096) before the cast)."""
    depths, K = np.asarray(depths, dtype=f32), np.asarray(K, dtype=f32)
    N, _, H, W = depths.shape
    d = depths[:, 0, ::stride, ::stride]
    v, u = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    k = lambda i, j: K[:, i, j][:, None, None]
    with np.errstate(all="ignore"):
        px = (u.astype(f32)[None] - k(0, 2)) / k(0, 0) * d
        py = (v.astype(f32)[None] - k(1, 2)) / k(1, 1) * d
        q = [np.rint(p * f32(4096.0)) for p in (px, py, d)]
    assert all(x.dtype == f32 for x in q)
    return d, u.astype(np.int64), v.astype(np.int64), q


def accumulate(depths, labels, K, *, num_labels, stride, max_depth, bounds=None):
    """The integer records: dict of int64 arrays [N,L] (n_pixels, n_samples, su, sv), [N,L,3] (sq), [N,L,6] (sqq), [N,L,4] (bbox,
    -1 where n_pixels = 0), and n_ignored."""
    L = int(num_labels)
    d, u, v, qf = quanta(depths, K, stride)
    N = d.shape[0]
    lab = np.asarray(labels)[:, 0, ::stride, ::stride].astype(np.int64)
    labelled = (lab >= 1) & (lab <= L)
    with np.errstate(all="ignore"):
        sample = labelled & (d > 0) & (d < f32(max_depth))
    key = (np.arange(N)[:, None, None] * L + lab - 1)
    q = [np.where(sample, x, f32(0)).astype(np.int64) for x in qf]
    if bounds is not None:
        b = np.asarray(bounds, dtype=f64).reshape(N * L, 2)
        kk = np.where(labelled, key, 0)
        with np.errstate(all="ignore"):
            dz = q[2].astype(f64) / 4096.0 - b[kk, 0]
            sample &= dz * dz <= b[kk, 1]
    U, V = np.broadcast_to(u, d.shape), np.broadcast_to(v, d.shape)

    def total(mask, values):
        out = np.zeros(N * L, np.int64)
        np.add.at(out, key[mask], values[mask])
        return out.reshape(N, L)

    one = np.ones(d.shape, np.int64)
    r = dict(n_pixels=total(labelled, one), n_samples=total(sample, one), su=total(sample, U), sv=total(sample, V))
    r["sq"] = np.stack([total(sample, q[a]) for a in range(3)], -1)
    r["sqq"] = np.stack([total(sample, q[a] * q[b]) for a, b in PAIRS], -1)
    big = np.iinfo(np.int64).max
    lo_u, lo_v = np.full(N * L, big), np.full(N * L, big)
    hi_u, hi_v = np.full(N * L, -1, np.int64), np.full(N * L, -1, np.int64)
    np.minimum.at(lo_u, key[labelled], U[labelled])
    np.minimum.at(lo_v, key[labelled], V[labelled])
    np.maximum.at(hi_u, key[labelled], U[labelled])
    np.maximum.at(hi_v, key[labelled], V[labelled])
    box = np.stack([lo_u, lo_v, hi_u, hi_v], -1).reshape(N, L, 4)
    r["bbox"] = np.where(r["n_pixels"][..., None] > 0, box, -1)
    r["n_ignored"] = int((lab > L).sum())
    return r


def clip_bounds(r, clip_sigma):
    """[N,L,2] float64 (mean_z, limit)."""
    n = r["n_samples"]
    dn = np.where(n >= 2, n, 1).astype(f64)
    mean = r["sq"][..., 2].astype(f64) / (4096.0 * dn)
    var = np.maximum(0.0, r["sqq"][..., 5].astype(f64) / (16777216.0 * dn) - mean * mean)
    k = f64(f32(clip_sigma))
    limit = (k * k) * var
    return np.stack([np.where(n >= 2, mean, 0.0), np.where(n >= 2, limit, np.inf)], -1)


def localize(depths, labels, K, M, *, num_labels, stride=1, max_depth=10.0, clip_sigma=None, min_samples=1):
    """-> dict with PolypLocalization's fields as NumPy arrays (n_labelled, n_ignored as ints)."""
    L = int(num_labels)
    kw = dict(num_labels=L, stride=stride, max_depth=max_depth)
    r = accumulate(depths, labels, K, **kw)
    if clip_sigma is not None:
        r = accumulate(depths, labels, K, bounds=clip_bounds(r, clip_sigma), **kw)
    M = np.asarray(M, dtype=f32).astype(f64)
    N = M.shape[0]
    n = r["n_samples"]
    seen = n > 0
    dn = np.where(seen, n, 1).astype(f64)
    nan = lambda x, m=seen: np.where(m if x.ndim == 2 else m[..., None], x, np.nan)
    pixel = np.stack([r["su"].astype(f64) / dn, r["sv"].astype(f64) / dn], -1)
    m = r["sq"].astype(f64) / (4096.0 * dn)[..., None]
    cov = np.stack([r["sqq"][..., e].astype(f64) / (16777216.0 * dn) - m[..., a] * m[..., b] for e, (a, b) in enumerate(PAIRS)], -1)
    R, t = M[:, None, :3, :3], M[:, None, :3, 3]
    cw = np.stack([((R[..., a, 0] * m[..., 0] + R[..., a, 1] * m[..., 1]) + R[..., a, 2] * m[..., 2]) + t[..., a] for a in range(3)], -1)
    out = dict(n_pixels=r["n_pixels"].astype(np.int32), n_samples=n.astype(np.int32), bbox=r["bbox"].astype(np.int32),
               pixel=nan(pixel), center_cam=nan(m), cov_cam=nan(cov), center_world=nan(cw))
    # per polyp: the frames in ascending order, one float64 addition at a time
    n_frames, total = np.zeros(L, np.int32), np.zeros(L, np.int64)
    first, last = np.full(L, -1, np.int32), np.full(L, -1, np.int32)
    position, cov_world = np.full((L, 3), np.nan), np.full((L, 6), np.nan)
    sym = {(a, b): e for e, (a, b) in enumerate(PAIRS)}
    sym.update({(b, a): e for e, (a, b) in enumerate(PAIRS)})
    for l in range(L):
        acc = [f64(0.0)] * 9
        for f in range(N):
            if n[f, l] < max(int(min_samples), 1):
                continue
            w = f64(n[f, l])
            Rf, c = M[f, :3, :3], cw[f, l]
            C = [[cov[f, l, sym[a, b]] for b in range(3)] for a in range(3)]
            T = [[(Rf[a, 0] * C[0][b] + Rf[a, 1] * C[1][b]) + Rf[a, 2] * C[2][b] for b in range(3)] for a in range(3)]
            for a in range(3):
                acc[a] = acc[a] + w * c[a]
            for e, (a, b) in enumerate(PAIRS):
                rcr = (T[a][0] * Rf[b, 0] + T[a][1] * Rf[b, 1]) + T[a][2] * Rf[b, 2]
                acc[3 + e] = acc[3 + e] + w * (rcr + c[a] * c[b])
            n_frames[l] += 1
            total[l] += n[f, l]
            first[l] = f if first[l] < 0 else first[l]
            last[l] = f
        if total[l] > 0:
            dt = f64(total[l])
            position[l] = [acc[a] / dt for a in range(3)]
            cov_world[l] = [acc[3 + e] / dt - position[l, a] * position[l, b] for e, (a, b) in enumerate(PAIRS)]
    out.update(n_frames=n_frames, n_samples_total=total, first_frame=first, last_frame=last, position=position, cov_world=cov_world,
               radius=np.sqrt(np.maximum(cov_world[:, 0] + cov_world[:, 3] + cov_world[:, 5], 0.0)),
               n_labelled=int(r["n_pixels"].sum()), n_ignored=r["n_ignored"])
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------- #
def scene(N, H, W, seed, spheres, dilate=0, wall=None, step_t=0.01, step_r=0.01):
    """fuse_ref.scene's depths, K and cam2world (a slow random trajectory) with spheres implanted: spheres = [((x, y, z), radius),
    ...] in the world frame, sphere i carrying label i + 1.  Per frame every pixel's ray is intersected with every sphere in
    float64; where the hit is nearer than what the pixel shows so far, the hit's z becomes the depth and the sphere's id the
    label.  wall: a constant background depth in place of the synthetic one.  dilate = p grows each mask by p pixels
    (4-neighbourhood, p times, lower ids first) onto background pixels without touching the depth.
    -> (depths [N,1,H,W] f32, labels [N,1,H,W] u8, K [N,3,3] f32, cam2world [N,4,4] f32)."""
    depths, _, K, M = fuse_ref.scene(N, H, W, seed, step_t=step_t, step_r=step_r)
    depths = depths.copy()
    if wall is not None:
        depths[:] = f32(wall)
    labels = np.zeros((N, 1, H, W), np.uint8)
    v, u = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    for n in range(N):
        Kd, Md = K[n].astype(f64), M[n].astype(f64)
        ray = np.stack([(u - Kd[0, 2]) / Kd[0, 0], (v - Kd[1, 2]) / Kd[1, 1], np.ones_like(u)], -1) @ Md[:3, :3].T   # world, z-depth 1
        for i, (centre, radius) in enumerate(spheres):
            oc = Md[:3, 3] - np.asarray(centre, f64)
            a = (ray * ray).sum(-1)
            b = ray @ oc
            disc = b * b - a * ((oc * oc).sum() - radius * radius)
            with np.errstate(all="ignore"):
                s = (-b - np.sqrt(disc)) / a                                   # the nearer root; NaN without a hit
                hit = (disc > 0) & (s > 0) & (s < depths[n, 0])
            depths[n, 0][hit] = s[hit].astype(f32)
            labels[n, 0][hit] = i + 1
        for _ in range(int(dilate)):
            lab = labels[n, 0]
            grown = lab.copy()
            for i in range(len(spheres), 0, -1):                               # lower ids written last: they win
                m = lab == i
                near = np.zeros_like(m)
                near[1:] |= m[:-1]
                near[:-1] |= m[1:]
                near[:, 1:] |= m[:, :-1]
                near[:, :-1] |= m[:, 1:]
                grown[near & (lab == 0)] = i
            labels[n, 0] = grown
    return depths, labels, K, M


# The scenes of the tests: (N, H, W, stride, L) -> (seed, spheres).  Centres and radii were chosen on the CPU (the cameras look
# down +z from near the origin with fx = 0.8 W, the synthetic depth is at least 0.5) so that every sphere lies in front of the
# scene and in view of every frame; tests/test_localize_cpu.py asserts what each scene shows.
def _row(xs, ys, z, r):
    return [((x, y, z), r) for y in ys for x in xs]


SCENES = {
    (1, 5, 7, 1, 1): (3, [((0.0, 0.0, 0.4), 0.1)]),
    (3, 17, 23, 1, 3): (5, _row((-0.17, 0.0, 0.17), (0.0,), 0.4, 0.085)),
    (4, 64, 96, 2, 4): (5, _row((-0.16, -0.05, 0.06, 0.17), (0.0,), 0.4, 0.05)),
    (8, 256, 320, 1, 8): (5, _row((-0.165, -0.055, 0.055, 0.165), (-0.07, 0.07), 0.4, 0.04)),
    (2, 5, 7, 9, 2): (3, [((-0.2, -0.12, 0.4), 0.12), ((0.5, 0.5, 0.4), 0.05)]),
}
CLIP_SCENE = dict(N=4, H=64, W=96, seed=5, spheres=[((0.0, 0.0, 0.4), 0.08)], wall=3.0, dilate=2)
CLIP_SIGMA = 1.5
MAX_DEPTH = 4.5
