"""NumPy replica of the mesh topology and cleaning contract (include/colvo.h colvo_mesh_topology_* / colvo_mesh_clean_*, DESIGN.md
§3.6o) -- test infrastructure in the manner of tests/tsdf_ref.py.  A sequential union-find, np.unique on the sorted vertex pairs,
float64 measures in the written association (NumPy never contracts a multiply and an add), np.rint, int64 sums; the GPU tests demand
equality with it to the bit.  Also the hand meshes the tests share.
"""
import functools

import numpy as np

f32 = np.float32
f64 = np.float64
Q_BITS = 16
Q_LIMIT = 2.0 ** 62


def quanta(unit):
    """(area quantum, length quantum) of a float32 unit, float64"""
    u = f64(f32(unit))
    return (u * u) * f64(2.0 ** -Q_BITS), u * f64(2.0 ** -Q_BITS)


def _union_find(n, pairs):
    """root [n] int64 of every element after uniting the pairs in order; a root is the smallest element of its class"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in pairs:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(n)], np.int64).reshape(n)


def _to_quanta(measure, quantum):
    with np.errstate(all="ignore"):
        t = measure / quantum
        ok = t < Q_LIMIT                                                    # NaN fails
        return np.where(ok, np.rint(np.where(ok, t, 0.0)), 0.0).astype(np.int64), ok


def live_faces(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((f >= 0) & (f < V)).all(1)
    return inside & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def mesh_topology(vertices, faces, unit):
    """-> dict(vertex_component [V] i32, face_component [F] i32, vertex_loop [V] i32, components [C,8] i64, loops [L,4] i64,
    n_dead_faces, n_unmeasured, unit)"""
    v = np.asarray(vertices, f32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = len(v), len(f)
    qa, ql = quanta(unit)
    live = live_faces(f, V)
    lf = f[live]
    root = _union_find(V, [p for a, b, c in lf.tolist() for p in ((a, b), (b, c))])
    roots = np.unique(root)
    C = len(roots)
    vc = np.searchsorted(roots, root)
    fc = np.full(F, -1, np.int64)
    fc[live] = vc[lf[:, 0]]
    comps = np.zeros((C, 8), np.int64)
    comps[:, 0] = roots
    comps[:, 1] = np.bincount(vc, minlength=C)
    comps[:, 2] = np.bincount(fc[live], minlength=C)
    # edges
    sides = np.concatenate([lf[:, [0, 1]], lf[:, [1, 2]], lf[:, [2, 0]]]) if len(lf) else np.zeros((0, 2), np.int64)
    lo, hi = sides.min(1), sides.max(1)
    key, m = np.unique(lo * max(V, 1) + hi, return_counts=True)
    elo, ehi = key // max(V, 1), key % max(V, 1)
    ec = vc[elo] if len(key) else np.zeros(0, np.int64)
    comps[:, 3] = np.bincount(ec, minlength=C)
    comps[:, 4] = np.bincount(ec[m == 1], minlength=C)
    comps[:, 5] = np.bincount(ec[m > 2], minlength=C)
    # areas
    p = v.astype(f64)
    with np.errstate(all="ignore"):
        a, b = p[lf[:, 1]] - p[lf[:, 0]], p[lf[:, 2]] - p[lf[:, 0]]
        nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        s = (nx * nx + ny * ny) + nz * nz
        q, ok = _to_quanta(0.5 * np.sqrt(s), qa)
    np.add.at(comps[:, 7], fc[live], q)
    n_unmeasured = int((~ok).sum())
    # loops
    blo, bhi = elo[m == 1], ehi[m == 1]
    on = np.zeros(V, bool)
    on[blo] = True
    on[bhi] = True
    root2 = _union_find(V, zip(blo.tolist(), bhi.tolist()))
    roots2 = np.unique(root2[on])
    L = len(roots2)
    vl = np.where(on, np.searchsorted(roots2, root2), -1)
    loops = np.zeros((L, 4), np.int64)
    loops[:, 0] = roots2
    loops[:, 1] = vc[roots2] if L else 0
    el = vl[blo]
    loops[:, 2] = np.bincount(el, minlength=L)
    with np.errstate(all="ignore"):
        d = p[bhi] - p[blo]
        q, ok = _to_quanta(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]), ql)
    np.add.at(loops[:, 3], el, q)
    n_unmeasured += int((~ok).sum())
    comps[:, 6] = np.bincount(loops[:, 1], minlength=C)
    return dict(vertex_component=vc.astype(np.int32), face_component=fc.astype(np.int32), vertex_loop=vl.astype(np.int32),
                components=comps, loops=loops, n_dead_faces=int(F - live.sum()), n_unmeasured=n_unmeasured, unit=float(f32(unit)))


def euler(topo):
    c = topo["components"]
    return c[:, 1] - c[:, 3] + c[:, 2]


def closed(topo):
    c = topo["components"]
    return (c[:, 2] > 0) & (c[:, 4] == 0) & (c[:, 5] == 0)


def keep_mask(topo, *, min_faces=1, min_area=0.0, largest=None):
    c = topo["components"]
    area = c[:, 7].astype(f64) * quanta(topo["unit"])[0]
    kept = (c[:, 2] >= min_faces) & (area >= f64(min_area))
    if largest is not None:
        order = sorted(range(len(c)), key=lambda i: (-(int(c[i, 2]) if kept[i] else -1), i))[:largest]
        top = np.zeros(len(c), bool)
        top[order] = True
        kept = kept & top
    return kept


def clean_mesh(mesh, topo, *, min_faces=1, min_area=0.0, largest=None):
    """mesh: dict(vertices, faces, colors or None, normals, cells, n_open) -> dict(the same keys, vertex_index, face_index, kept)"""
    kept = keep_mask(topo, min_faces=min_faces, min_area=min_area, largest=largest)
    vc, fc = topo["vertex_component"].astype(np.int64), topo["face_component"].astype(np.int64)
    vkeep = kept[vc] if len(vc) else np.zeros(0, bool)
    fkeep = (fc >= 0) & (kept[np.maximum(fc, 0)] if len(kept) else False)
    vi, fi = np.nonzero(vkeep)[0], np.nonzero(fkeep)[0]
    vmap = np.full(len(vc), -1, np.int64)
    vmap[vi] = np.arange(len(vi))
    faces = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    out = dict(vertices=mesh["vertices"][vi], normals=mesh["normals"][vi], cells=mesh["cells"][vi],
               colors=None if mesh.get("colors") is None else mesh["colors"][vi],
               faces=vmap[faces[fi]].astype(np.int32).reshape(-1, 3), n_open=mesh["n_open"],
               vertex_index=vi.astype(np.int32), face_index=fi.astype(np.int32), kept=kept)
    return out


# ---- hand meshes: (vertices [V,3] float32, faces [F,3] int32) ---------------------------------------------------------------------- #
def _mesh(v, f):
    return np.asarray(v, f32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)


def tetrahedron():
    return _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])


def right_triangle():
    return _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])


def triangle_strip(n):
    """n triangles (i, i+1, i+2) over two rows of vertices: one component, one loop of n + 2 edges, 2 n + 1 edges in all"""
    j = np.arange(n + 2)
    v = np.stack([(j // 2).astype(f64), (j % 2).astype(f64), np.zeros(n + 2)], 1)
    i = np.arange(n)
    f = np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], 1), np.stack([i + 1, i, i + 2], 1))
    return _mesh(v, f)


def square_strip(n):
    """n unit squares in a row, two triangles each"""
    return triangle_strip(2 * n)


def annulus(k=8):
    """k quads between two rings: 2 k vertices, 2 k faces, 4 k edges, two loops of k edges"""
    t = 2.0 * np.pi * np.arange(k) / k
    ring = lambda r: np.stack([r * np.cos(t), r * np.sin(t), np.zeros(k)], 1)
    v = np.concatenate([ring(1.0), ring(2.0)])
    i = np.arange(k)
    j = (i + 1) % k
    f = np.concatenate([np.stack([i, i + k, j + k], 1), np.stack([i, j + k, j], 1)])
    return _mesh(v, f)


def book(pages=3):
    """`pages` triangles on one edge (0, 1): that edge is non-manifold from three pages on"""
    v = [[0, 0, 0], [1, 0, 0]] + [[0.5, np.cos(0.7 * p), np.sin(0.7 * p)] for p in range(pages)]
    return _mesh(v, [[0, 1, 2 + p] for p in range(pages)])


def fan(n):
    """n triangles around vertex 0: the hub is the smaller endpoint of n + 1 edges"""
    t = np.pi * np.arange(n + 1) / n
    v = np.concatenate([np.zeros((1, 3)), np.stack([np.cos(t), np.sin(t), np.zeros(n + 1)], 1)])
    i = np.arange(n)
    return _mesh(v, np.stack([np.zeros(n, np.int64), i + 1, i + 2], 1))


def separate_triangles(n):
    """n triangles that share nothing"""
    i = np.arange(n)
    x = (i % 100).astype(f64) * 2.0
    y = (i // 100).astype(f64) * 2.0
    v = np.stack([np.stack([x, y, 0 * x], 1), np.stack([x + 1, y, 0 * x], 1), np.stack([x, y + 1, 0 * x], 1)], 1).reshape(-1, 3)
    return _mesh(v, np.arange(3 * n).reshape(n, 3))


def concatenate(meshes):
    """the meshes side by side in one vertex array (each shifted 4 along z per piece, so that nothing coincides)"""
    vs, fs, base = [], [], 0
    for k, (v, f) in enumerate(meshes):
        vs.append(v + np.array([0, 0, 4.0 * k], f32))
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs).astype(f32), np.concatenate(fs).astype(np.int32)


def renumber(v, f, seed):
    """the same mesh with its vertex numbers shuffled; face entries outside [0, V) stay as they are"""
    perm = np.random.default_rng(seed).permutation(len(v))                   # old -> new
    v2 = np.empty_like(v)
    v2[perm] = v
    inside = (f >= 0) & (f < len(v))
    f2 = np.where(inside, perm[np.clip(f, 0, max(len(v) - 1, 0))], f).astype(np.int32)
    return v2, f2


# ---- the project's own meshes: the replica of extract_mesh (tests/tsdf_ref.py) on small scenes -------------------------------------- #
TUBE_MAX_DEPTH = 4.5
SPHERE = dict(radius_voxels=6.3, T=3, S=32, n=32, voxel=0.05, shift=(0.011, -0.007, 0.004))


@functools.lru_cache(maxsize=None)
def tube_mesh(N, H, W, Tv, min_obs):
    """The replica's mesh of tests/test_tsdf_gpu.py's small tube at voxel 0.1 and a truncation of Tv voxels, with random colours, and
    the arguments of its volume: (mesh, (depths, K, M, fuse_tsdf keywords)).  Shared by the tests: do not write to it."""
    import torch
    from coivo_amd import inference as I
    from tests import consistency_ref as CR
    from tests import tsdf_ref as R
    depths, K, M = CR.tube_scene(N, H, W, 3)
    origin, dims = I.fusion_grid(torch.from_numpy(K), torch.from_numpy(M), H, W, 0.1, TUBE_MAX_DEPTH)
    colors = np.random.default_rng(N * H + W).random((N, 3, H, W)).astype(f32)
    kw = dict(voxel_size=0.1, trunc=None if Tv == 4 else Tv * 0.1, max_depth=TUBE_MAX_DEPTH, origin=origin, dims=dims, colors=colors)
    return R.extract_mesh(R.fuse_tsdf(depths, K, M, **kw), min_obs=min_obs), (depths, K, M, kw)


@functools.lru_cache(maxsize=None)
def sphere_mesh():
    """tsdf_ref.sphere_scene's mesh, the same way.  The grid is shifted off the sphere's centre: a voxel centre exactly on a diagonal
    of the cube of cameras (direction (1, 1, 1): on the half-open border of three images, inside none) is never observed, and the
    mesh has a hole there."""
    from tests import tsdf_ref as R
    s = SPHERE
    depths, K, M = R.sphere_scene(s["radius_voxels"] * s["voxel"], s["S"])
    origin = tuple(float(f32(-s["n"] / 2 * s["voxel"] + x)) for x in s["shift"])
    kw = dict(voxel_size=s["voxel"], trunc=s["T"] * s["voxel"], origin=origin, dims=(s["n"],) * 3)
    return R.extract_mesh(R.fuse_tsdf(depths, K, M, **kw), min_obs=1), (depths, K, M, kw)
