"""NumPy replica of the point-to-surface contract (include/colvo.h colvo_surface_*, coivo_amd/evaluate.py) -- test
infrastructure in the manner of tests/cloud_ref.py.  Brute force: every live, finite face against every valid query, in chunks of an
N x F matrix; float64 on coordinates widened from float32, one rounding per operation (NumPy never contracts a multiply and an add), in
the association the header writes.  The winner is the first minimum over the faces in ascending index.  `nearest` has no grid, so it
cannot share a grid bug with the kernel; `grid_emulation` is the cell rule in NumPy, for the cost figures that depend on the index and
for the CPU test of the rule itself.
"""
import numpy as np

f32, f64 = np.float32, np.float64
CHUNK_ELEMS = 1 << 18
N_STATS = 19
STATS = ("n_valid", "n_reached") + tuple(f"under_{k}" for k in range(8)) + (
    "sum_quanta", "examined", "in_front", "behind", "plane_winners", "dead_faces", "skipped_faces", "pairs", "oversize")
SPAN_LIMIT = 4                 # tuning.h surface_span_limit
EDGE_MARGIN = 1.0 + 2.0 ** -10
AXIS_LIMIT, AXIS_DIV = 128, 126.0


def _sub(u, v):
    return tuple(u[k] - v[k] for k in range(3))


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def classify(vertices, faces):
    """-> (live [F] bool, used [F] bool): live as tests/topology_ref.py's, used = live and all nine coordinates finite."""
    vertices = np.asarray(vertices, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(vertices)
    inside = ((faces >= 0) & (faces < V)).all(axis=1)
    live = inside & (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    used = live.copy()
    if live.any():
        used[live] = np.isfinite(vertices[faces[live]]).all(axis=(1, 2))
    return live, used


def point_triangle(p, a, b, c, points=False):
    """The contract's arithmetic on broadcastable float64 component tuples p, a, b, c -> (d2, plane winner?, h, area?) and, with
    points=True, the winning candidate's point as a component tuple behind them."""
    with np.errstate(all="ignore"):
        ab, ac, bc, ca = _sub(b, a), _sub(c, a), _sub(c, b), _sub(a, c)
        pa, pb, pc = _sub(p, a), _sub(p, b), _sub(p, c)
        n = _cross(ab, ac)
        s = _dot(n, n)
        h = _dot(n, pa)
        area = (s > 0.0) & np.isfinite(s)
        used = area & (_dot(n, _cross(ab, pa)) >= 0.0) & (_dot(n, _cross(bc, pb)) >= 0.0) & (_dot(n, _cross(ca, pc)) >= 0.0)
        k = h / s
        d2 = np.where(used, (h * h) / s, np.inf)
        plane = used
        q = tuple(np.where(used, p[j] - n[j] * k, 0.0) for j in range(3)) if points else None
        for u, e, w in ((a, ab, pa), (b, bc, pb), (c, ca, pc)):
            ee, we = _dot(e, e), _dot(w, e)
            t = np.where(ee > 0.0, np.minimum(np.maximum(we / ee, 0.0), 1.0), 0.0)
            cand = tuple(u[j] + t * e[j] for j in range(3))
            s2 = _dot(_sub(p, cand), _sub(p, cand))
            better = s2 < d2
            d2 = np.where(better, s2, d2)
            plane = plane & ~better
            if points:
                q = tuple(np.where(better, cand[j], q[j]) for j in range(3))
    out = (d2, plane, h, area)
    return out + (q,) if points else out


def _cols(A):
    return tuple(A[..., j] for j in range(3))


def nearest(Q, vertices, faces, max_dist, thresholds=()):
    """-> dict(dist2 [N] f64, dist [N] f32, face [N] i32, closest [N,3] f32, side [N] i8, stats [19] i64 with the three words that depend on
    the index -- examined, pairs, oversize -- left 0: grid_emulation gives them)."""
    Q = np.ascontiguousarray(Q, f32).reshape(-1, 3)
    vertices = np.ascontiguousarray(vertices, f32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    md = f32(max_dist)
    md2 = f64(md) * f64(md)
    N = len(Q)
    live, used = classify(vertices, faces)
    idx = np.nonzero(used)[0]
    vq = np.isfinite(Q).all(axis=1)
    dist2 = np.full(N, md2, f64)
    face = np.full(N, -1, np.int32)
    closest = np.where(vq[:, None], Q, f32(0)).astype(f32)
    side = np.zeros(N, np.int8)
    plane = np.zeros(N, bool)
    rows = np.nonzero(vq)[0]
    if len(idx) and len(rows):
        tri = vertices[faces[idx].astype(np.int64)].astype(f64)             # [m,3 corners,3]
        a, b, c = (tuple(tri[None, :, k, j] for j in range(3)) for k in range(3))
        step = max(1, CHUNK_ELEMS // len(idx))
        for i in range(0, len(rows), step):
            r = rows[i:i + step]
            P = Q[r].astype(f64)
            d2 = point_triangle(tuple(P[:, None, j] for j in range(3)), a, b, c)[0]
            j = d2.argmin(axis=1)                     # the FIRST minimum; the columns ascend in face index
            best = d2[np.arange(len(r)), j]
            hit = best < md2                          # strict
            r, j, P = r[hit], j[hit], P[hit]
            if not len(r):
                continue
            w = tri[j]
            d2w, pl, h, area, q = point_triangle(_cols(P), _cols(w[:, 0]), _cols(w[:, 1]), _cols(w[:, 2]), points=True)
            assert np.array_equal(d2w, best[hit])     # the same face evaluated twice gives the same bits
            dist2[r] = d2w
            face[r] = idx[j].astype(np.int32)
            closest[r] = np.stack(q, axis=1).astype(f32)
            side[r] = np.where(area, (h > 0.0).astype(np.int8) - (h < 0.0).astype(np.int8), 0).astype(np.int8)
            plane[r] = pl
    dist = np.where(face >= 0, np.sqrt(dist2).astype(f32), md).astype(f32)
    scale = f32(f32(2 ** 20) / md)
    quanta = np.rint((dist * scale).astype(f32)).astype(np.uint64)
    stats = np.zeros(N_STATS, np.int64)
    stats[0] = int(vq.sum())
    stats[1] = int((vq & (face >= 0)).sum())
    for k, tau in enumerate(thresholds):
        t = f64(f32(tau))
        stats[2 + k] = int((vq & (dist2 < t * t)).sum())
    stats[10] = int(quanta[vq].sum())
    stats[12] = int((side > 0).sum())
    stats[13] = int((side < 0).sum())
    stats[14] = int(plane.sum())
    stats[15] = int((~live).sum())
    stats[16] = int((live & ~used).sum())
    return dict(dist2=dist2, dist=dist, face=face, closest=closest, side=side, stats=stats, md2=md2, scale=scale)


def grid_emulation(Q, vertices, faces, max_dist, *, margin=EDGE_MARGIN, span=SPAN_LIMIT):
    """The kernel's cell rule in NumPy (float32, as cloud_grid.h): origin = the lower corner of the box of the used faces' vertices,
    edge = max(max_dist * margin, extent / 126), cell = clamp(floor((x - o) * (1 / edge))); a face is entered into the box of cells of
    its bounds, or is oversize where that box spans more than `span` cells on an axis; a query walks the 27 cells around its own.
    -> dict(lo, hi [F,3] cell boxes (-1 for faces not used), oversize [F] bool, pairs, cell [N,3] and walk [N] of the queries,
    seen(face index [N]) -> [N] bool: is that face in the query's walk or oversize, examined: the kernel's cost figure)."""
    Q = np.ascontiguousarray(Q, f32).reshape(-1, 3)
    vertices = np.ascontiguousarray(vertices, f32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    F = len(faces)
    _, used = classify(vertices, faces)
    lo = np.full((F, 3), -1, np.int64)
    hi = np.full((F, 3), -1, np.int64)
    vq = np.isfinite(Q).all(axis=1)
    out = dict(lo=lo, hi=hi, oversize=np.zeros(F, bool), pairs=0, examined=0, walk=np.zeros(len(Q), bool),
               cell=np.zeros((len(Q), 3), np.int64))
    if not used.any():
        out["seen"] = lambda f: np.zeros(len(Q), bool)
        return out
    tri = vertices[faces[used].astype(np.int64)]                            # [m,3,3] float32
    o, top = tri.min(axis=(0, 1)), tri.max(axis=(0, 1))
    with np.errstate(all="ignore"):
        ext = f32((top - o).max())
        edge = max(f32(f32(max_dist) * f32(margin)), f32(ext / f32(AXIS_DIV)))
        inv = f32(f32(1) / edge)
        single = not (np.isfinite(ext) and np.isfinite(edge) and np.isfinite(inv) and inv > 0)
        if single:
            inv = f32(0)
            n = np.ones(3, np.int64)
        else:
            n = np.clip(np.floor((top - o) * inv), 0, AXIS_LIMIT - 1).astype(np.int64) + 1

        def cell(x):
            g = np.nan_to_num(np.floor((x - o) * inv), nan=0.0)
            return np.minimum(np.maximum(g, 0.0), (n - 1).astype(f32)).astype(np.int64)

        lo[used], hi[used] = cell(tri.min(axis=1)), cell(tri.max(axis=1))
        over = used & ((hi - lo + 1) > span).any(axis=1)
        g = (Q - o) * inv
        walk = vq.copy()
        if not single:
            walk &= ((g >= -1.0) & (g < (n + 1).astype(f32))).all(axis=1)
        cq = np.where(walk[:, None] & (not single), np.floor(np.nan_to_num(g, nan=0.0, posinf=0.0, neginf=0.0)), 0.0).astype(np.int64)
    binned = used & ~over
    sizes = (hi - lo + 1)[binned]
    count = np.zeros(tuple(n[::-1]), np.int64)                              # [z, y, x]
    for f in np.nonzero(binned)[0]:
        count[lo[f, 2]:hi[f, 2] + 1, lo[f, 1]:hi[f, 1] + 1, lo[f, 0]:hi[f, 0] + 1] += 1
    integral = np.zeros(tuple(n[::-1] + 1), np.int64)
    integral[1:, 1:, 1:] = count.cumsum(0).cumsum(1).cumsum(2)
    b0 = np.clip(cq - 1, 0, None)
    b1 = np.minimum(cq + 1, n - 1) + 1                                       # exclusive
    ok = walk & (b0 < b1).all(axis=1)
    x0, y0, z0 = (b0[ok, j] for j in range(3))
    x1, y1, z1 = (b1[ok, j] for j in range(3))
    I = integral
    box = (I[z1, y1, x1] - I[z0, y1, x1] - I[z1, y0, x1] - I[z1, y1, x0] + I[z0, y0, x1] + I[z0, y1, x0] + I[z1, y0, x0] - I[z0, y0, x0])
    n_over = int(over.sum())

    def seen(f):
        f = np.asarray(f, np.int64)
        inside = ((lo[f] <= cq + 1) & (hi[f] >= cq - 1)).all(axis=1) & walk
        return over[f] | (inside & binned[f])

    out.update(oversize=over, pairs=int(sizes.prod(axis=1).sum()), examined=int(box.sum()) + n_over * int(vq.sum()), walk=walk, cell=cq,
               seen=seen, n=n, single=single, o=o, edge=edge)
    return out


def full_stats(Q, vertices, faces, max_dist, thresholds=(), want=None):
    """nearest(...) with the three index-dependent statistics filled in from grid_emulation."""
    want = nearest(Q, vertices, faces, max_dist, thresholds) if want is None else want
    g = grid_emulation(Q, vertices, faces, max_dist)
    st = want["stats"].copy()
    st[11], st[17], st[18] = g["examined"], g["pairs"], int(g["oversize"].sum())
    return dict(want, stats=st)


def used_vertices(vertices, faces):
    """The mesh as clean_mesh's defaults leave it: the vertices a live face uses, in their old order, and the live faces re-indexed."""
    vertices = np.ascontiguousarray(vertices, f32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    live, _ = classify(vertices, faces)
    keep = np.zeros(len(vertices), bool)
    keep[faces[live].astype(np.int64).reshape(-1)] = True
    new = np.cumsum(keep) - 1
    return vertices[keep], new[faces[live].astype(np.int64)].astype(np.int32).reshape(-1, 3)


def mean_distance(stats, scale):
    n = int(stats[0])
    return float("nan") if n == 0 else float(int(stats[10])) / (float(scale) * n)


def metrics(pred, gt, max_dist, thresholds, transform_=None):
    """The measures of evaluate.surface_metrics: pred, gt = (vertices, faces); both cleaned, pred moved by cloud_ref.transform, the
    vertices of each side against the other side's faces."""
    from tests import cloud_ref
    pv, pf = used_vertices(*pred)
    gv, gf = used_vertices(*gt)
    if transform_ is not None:
        pv = cloud_ref.transform(pv, *transform_)
    a = nearest(pv, gv, gf, max_dist, thresholds)
    b = nearest(gv, pv, pf, max_dist, thresholds)
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
                in_front=int(a["stats"][12]) / n_pred if n_pred else float("nan"),
                behind=int(a["stats"][13]) / n_pred if n_pred else float("nan"), pred_to_gt=a, gt_to_pred=b,
                pred=(pv, pf), gt=(gv, gf))
