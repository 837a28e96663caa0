"""NumPy replica of the point-cloud contract (include/colvo.h colvo_cloud_*, coivo_amd/evaluate.py) -- test
infrastructure in the manner of tests/fuse_ref.py.  Brute force over chunked N x M matrices of d2: float32 with one rounding per
operation (NumPy never contracts a multiply and an add), the minimum of the packed 64-bit key by a first-minimum argmin, integer sums.  It has no
grid, so it cannot share a grid bug with the kernel; the GPU tests demand equality with it to the bit.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

f32 = np.float32
CHUNK_ELEMS = 1 << 18          # pairs per chunk: three work arrays of it stay in cache
SHIFT = np.array([100.0, -37.0, 0.001], f32)      # the lattice's offset: the cell coordinate rounds
LATTICE_MAX_DISTS = (0.0625, 0.05, 0.013, 0.083)   # a power of two, one that is not, two at which an edge of max_dist fails
STATS = 11                     # n_valid, n_reached, eight threshold counts, the sum of the quanta (the kernel's 12th word is a cost figure)


def valid(P):
    return np.isfinite(np.asarray(P, dtype=f32)).all(axis=1)


def _chunk_min(Qc, Pv, idx64):
    """Minimum packed key (bits(d2) << 32) | original index over the reference points, for every row of Qc."""
    with np.errstate(over="ignore"):
        d = Qc[:, None, 0] - Pv[None, :, 0]
        np.multiply(d, d, out=d)
        acc = d
        d = Qc[:, None, 1] - Pv[None, :, 1]
        np.multiply(d, d, out=d)
        np.add(acc, d, out=acc)                      # (dx*dx + dy*dy)
        d = Qc[:, None, 2] - Pv[None, :, 2]
        np.multiply(d, d, out=d)
        np.add(acc, d, out=acc)                      # ... + dz*dz
    assert acc.dtype == f32
    # argmin returns the FIRST minimum and the columns are in ascending original index: the column it names carries the smallest
    # packed key of its row (d2 >= 0, never NaN between finite points, so the float order is the order of the bits)
    j = acc.argmin(axis=1)
    return (acc[np.arange(len(j)), j].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx64[j]


def nearest(Q, P, max_dist, thresholds=()):
    """-> dict(dist [N] f32, dist2 [N] f32, nearest [N] i32, stats [11] i64, md2, scale)."""
    Q = np.ascontiguousarray(Q, dtype=f32).reshape(-1, 3)
    P = np.ascontiguousarray(P, dtype=f32).reshape(-1, 3)
    md = f32(max_dist)
    md2 = f32(md * md)
    N = Q.shape[0]
    vq = valid(Q)
    idx = np.nonzero(valid(P))[0]
    Pv, idx64 = P[idx], idx.astype(np.uint64)
    best = np.full(N, (np.uint64(md2.view(np.uint32)) << np.uint64(32)) | np.uint64(0xffffffff), dtype=np.uint64)
    rows = np.nonzero(vq)[0]
    if len(idx) and len(rows):
        step = max(1, CHUNK_ELEMS // len(idx))
        parts = [rows[i:i + step] for i in range(0, len(rows), step)]
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            mins = list(ex.map(lambda r: _chunk_min(Q[r], Pv, idx64), parts))
        key = np.concatenate(mins)
        d2 = (key >> np.uint64(32)).astype(np.uint32).view(f32)
        reach = d2 < md2                                         # strict; NaN cannot occur between finite points, inf falls out
        best[rows[reach]] = key[reach]
    dist2 = (best >> np.uint64(32)).astype(np.uint32).view(f32)
    near = (best & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32)
    dist = np.sqrt(dist2)
    assert dist.dtype == f32
    scale = f32(f32(2 ** 20) / md)
    quanta = np.rint((dist * scale).astype(f32)).astype(np.uint64)
    stats = np.zeros(STATS, np.int64)
    stats[0] = int(vq.sum())
    stats[1] = int((vq & (near >= 0)).sum())
    for k, tau in enumerate(thresholds):
        t = f32(tau)
        stats[2 + k] = int((vq & (dist2 < f32(t * t))).sum())
    stats[10] = int(quanta[vq].sum())
    return dict(dist=dist, dist2=dist2, nearest=near, stats=stats, md2=md2, scale=scale)


def transform(P, R, t, s):
    """out = ((s * ((r0*x + r1*y) + r2*z)) + t) per axis, float32, one rounding per operation; R, t, s rounded to float32 first."""
    P = np.ascontiguousarray(P, dtype=f32).reshape(-1, 3)
    R = np.asarray(R, dtype=np.float64).astype(f32)
    t = np.asarray(t, dtype=np.float64).astype(f32)
    s = f32(np.float64(s))
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        out = np.stack([((s * ((R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z)) + t[a]) for a in range(3)], axis=1)
    assert out.dtype == f32
    return np.ascontiguousarray(out)


def mean_distance(stats, scale):
    n = int(stats[0])
    return float("nan") if n == 0 else float(int(stats[10])) / (float(scale) * n)


def metrics(pred, gt, max_dist, thresholds, transform_=None):
    """The measures of evaluate.cloud_metrics from two brute-force searches: dict with accuracy, completeness, chamfer, precision,
    recall, fscore (tuples), the four counts and the two searches (pred_to_gt, gt_to_pred)."""
    if transform_ is not None:
        pred = transform(pred, *transform_)
    a = nearest(pred, gt, max_dist, thresholds)
    b = nearest(gt, pred, max_dist, thresholds)
    acc, comp = mean_distance(a["stats"], a["scale"]), mean_distance(b["stats"], b["scale"])
    n_pred, n_gt = int(a["stats"][0]), int(b["stats"][0])
    precision, recall, fscore = [], [], []
    for k in range(len(thresholds)):
        p = int(a["stats"][2 + k]) / n_pred if n_pred else float("nan")
        r = int(b["stats"][2 + k]) / n_gt if n_gt else float("nan")
        precision.append(p)
        recall.append(r)
        fscore.append(0.0 if p == 0.0 and r == 0.0 else 2.0 * p * r / (p + r))
    return dict(accuracy=acc, completeness=comp, chamfer=0.5 * (acc + comp), precision=tuple(precision), recall=tuple(recall),
                fscore=tuple(fscore), n_pred=n_pred, n_gt=n_gt, n_pred_reached=int(a["stats"][1]), n_gt_reached=int(b["stats"][1]),
                pred_to_gt=a, gt_to_pred=b)


# ---- the lattice of the reach-boundary test ------------------------------------------------------------------------------ #
def nudge(x, k):
    """x moved by k float32 ulps (k < 0: downwards)."""
    x = np.asarray(x, f32).copy()
    for _ in range(abs(int(k))):
        x = np.nextafter(x, f32(np.inf if k > 0 else -np.inf))
    return x


def lattice(md, seed):
    """Reference points on the even sites of a lattice of pitch max_dist (sites 0..7 per axis), shifted by SHIFT so that the cell
    coordinate rounds; queries at every site -1..8, occupied or not, moved by -4..4 ulps along one axis and by random ulps
    along all three: within a few ulps of a pitch multiple in every coordinate, and, at the empty sites, within a few ulps of
    distance max_dist from up to six reference points -- on whichever side of the boundary the float32 arithmetic puts them."""
    md = f32(md)
    g = np.arange(-1, 9)
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    pos = (sites.astype(f32) * md + SHIFT).astype(f32)
    inner = ((sites >= 0) & (sites <= 7)).all(axis=1)
    occupied = inner & (sites.sum(axis=1) % 2 == 0)
    P = pos[occupied]
    Q = []
    for a in range(3):
        for k in range(-4, 5):
            q = pos.copy()
            q[:, a] = nudge(q[:, a], k)
            Q.append(q)
    rng = np.random.default_rng(seed)
    for _ in range(6):
        q = pos.copy()
        ks = rng.integers(-4, 5, size=q.shape)
        for k in range(-4, 5):
            q = np.where(ks == k, nudge(q, k), q)
        Q.append(q)
    Q = np.concatenate(Q)
    empty = np.tile(~occupied, len(Q) // len(pos))
    return Q, P, empty
