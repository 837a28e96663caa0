"""NumPy replica of the hole-filling contract (include/colvo.h colvo_mesh_fill_*) -- test infrastructure in the manner
of tests/topology_ref.py, on whose mesh_topology it stands.  Sequential: it walks succ around every simple loop, rounds with np.rint
and sums in int64; float64 measures in the written association (NumPy never contracts a multiply and an add).  The GPU tests demand
equality with it to the bit.  Also the hand meshes the tests share.

The contract.  A live face (a, b, c) has the directed sides a->b, b->c, c->a; a side whose unordered edge has multiplicity 1 is a boundary
half-edge; out[v] / in[v] count those that leave / enter v.  A loop of mesh_topology is simple iff every one of its vertices has out = in
= 1; its ring starts at loops[l, 0] and follows succ.  Centre: per ring vertex and coordinate t = double(x) / q with q = unit * 2^-16;
unmeasured if any t is NaN or |t| >= 2^32; else S = sum of rint(t) as int64 and the coordinate is float32((double(S) / double(n)) * q);
colours likewise with q = 2^-16, a bad colour adding 0.  Fan: for n > 3 ring edge k gives (ring[k+1 mod n], ring[k], centre), for n = 3
the one face (ring[0], ring[2], ring[1]).  Hole area: the sum of mesh_topology's face quanta over the fan (a face that fails makes the
loop unmeasured).  Centre normal: the three half cross-product components per fan face, each in area quanta under |t| < 2^62, summed as
int64, normalised in float64 as x / sqrt((x x + y y) + z z); zero where the sum is.  Status, the first that applies: 2 NOT_SIMPLE, 3
UNMEASURED, 1 TOO_LONG (n > max_edges), 0 FILLED.  hole[l] = (fan faces written, area in quanta -- 0 for a loop that is not simple or
unmeasured).
"""
import numpy as np

from tests import topology_ref as T

f32, f64 = np.float32, np.float64
FILLED, TOO_LONG, NOT_SIMPLE, UNMEASURED = 0, 1, 2, 3
T_LIMIT = 2.0 ** 32
COLOR_QUANTUM = f64(2.0 ** -16)


def boundary_half_edges(faces, V):
    """(src, dst) int64 arrays of the boundary half-edges of the live faces"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lf = f[T.live_faces(f, V)]
    if not len(lf):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    src = np.concatenate([lf[:, 0], lf[:, 1], lf[:, 2]])
    dst = np.concatenate([lf[:, 1], lf[:, 2], lf[:, 0]])
    key = np.minimum(src, dst) * V + np.maximum(src, dst)
    _, inverse, counts = np.unique(key, return_inverse=True, return_counts=True)
    b = counts[inverse.reshape(-1)] == 1
    return src[b], dst[b]


def _coordinate_quanta(x, quantum):
    with np.errstate(all="ignore"):
        t = np.asarray(x, f32).astype(f64) / quantum
        ok = np.abs(t) < T_LIMIT                                            # NaN fails
        return np.where(ok, np.rint(np.where(ok, t, 0.0)), 0.0).astype(np.int64), ok


def _signed_quanta(m, quantum):
    with np.errstate(all="ignore"):
        t = m / quantum
        ok = np.abs(t) < T.Q_LIMIT
        return np.where(ok, np.rint(np.where(ok, t, 0.0)), 0.0).astype(np.int64), ok


def _fan_measure(pi, pj, pk, qa):
    """faces (i, j, k) given by their float64 points [m,3] -> (area quanta sum, normal quanta sums [3], all measured)"""
    with np.errstate(all="ignore"):
        a, b = pj - pi, pk - pi
        nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        s = (nx * nx + ny * ny) + nz * nz
        q, ok = T._to_quanta(0.5 * np.sqrt(s), qa)
        comps = [_signed_quanta(0.5 * c, qa) for c in (nx, ny, nz)]
    measured = bool(ok.all()) and all(bool(o.all()) for _, o in comps)
    return int(q.sum()), np.array([int(c.sum()) for c, _ in comps], np.int64), measured


def fill_holes(mesh, topo, max_edges):
    """mesh: dict(vertices, faces, colors or None, normals, cells, n_open); topo: topology_ref.mesh_topology of it ->
    dict(vertices, faces, colors, normals, cells, n_open, status [L] i32, hole [L,2] i64, ring_offsets [L+1] i32, ring_vertices [R] i32,
    face_loop [F'] i32, new_vertex_loop [V'-V] i32, centres [L,3] f32 (of the simple measured loops, else 0), unit)"""
    assert isinstance(max_edges, int) and max_edges >= 3
    v = np.asarray(mesh["vertices"], f32).reshape(-1, 3)
    f = np.asarray(mesh["faces"], np.int32).reshape(-1, 3)
    colors = mesh.get("colors")
    V, F = len(v), len(f)
    loops = topo["loops"]
    L = len(loops)
    qa, ql = T.quanta(topo["unit"])
    vl = topo["vertex_loop"].astype(np.int64)
    src, dst = boundary_half_edges(f, V)
    out, inn = np.bincount(src, minlength=V), np.bincount(dst, minlength=V)
    succ = np.full(V, -1, np.int64)
    succ[src] = dst
    on = vl >= 0
    bad = np.bincount(vl[on & ((out != 1) | (inn != 1))], minlength=L) > 0
    p = v.astype(f64)

    status = np.zeros(L, np.int32)
    hole = np.zeros((L, 2), np.int64)
    ring_offsets = np.zeros(L + 1, np.int32)
    centres = np.zeros((L, 3), f32)
    rings, new_vertices, new_colors, new_normals, new_faces, face_loop, new_vertex_loop = [], [], [], [], [], [], []
    n_new = 0
    for l in range(L):
        n = int(loops[l, 2])
        ring_offsets[l + 1] = ring_offsets[l]
        if bad[l]:
            status[l] = NOT_SIMPLE
            continue
        assert n >= 3
        ring = [int(loops[l, 0])]
        for _ in range(n - 1):
            ring.append(int(succ[ring[-1]]))
        assert succ[ring[-1]] == ring[0] and len(set(ring)) == n and (vl[ring] == l).all(), "a simple loop is one cycle"
        ring = np.array(ring, np.int64)
        rings.append(ring)
        ring_offsets[l + 1] += n
        t, ok = _coordinate_quanta(v[ring], ql)
        if not ok.all():
            status[l] = UNMEASURED
            continue
        with np.errstate(all="ignore"):
            centre = ((t.sum(0).astype(f64) / f64(n)) * ql).astype(f32)
        if n > 3:
            k = np.arange(n)
            area, nq, measured = _fan_measure(p[ring[(k + 1) % n]], p[ring], np.broadcast_to(centre.astype(f64), (n, 3)), qa)
        else:
            area, nq, measured = _fan_measure(p[ring[[0]]], p[ring[[2]]], p[ring[[1]]], qa)
        if not measured:
            status[l] = UNMEASURED
            continue
        centres[l] = centre
        hole[l, 1] = area
        if n > max_edges:
            status[l] = TOO_LONG
            continue
        status[l] = FILLED
        if n == 3:
            hole[l, 0] = 1
            new_faces.append([ring[0], ring[2], ring[1]])
            face_loop.append(l)
            continue
        hole[l, 0] = n
        c = V + n_new
        n_new += 1
        new_vertices.append(centre)
        new_vertex_loop.append(l)
        x = nq.astype(f64)
        length = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
        new_normals.append((x / length).astype(f32) if length > 0 else np.zeros(3, f32))
        if colors is not None:
            cq, cok = _coordinate_quanta(np.asarray(colors, f32)[ring], COLOR_QUANTUM)
            new_colors.append(((np.where(cok, cq, 0).sum(0).astype(f64) / f64(n)) * COLOR_QUANTUM).astype(f32))
        for j in range(n):
            new_faces.append([ring[(j + 1) % n], ring[j], c])
            face_loop.append(l)

    def rows(old, new, dtype):
        old = np.asarray(old, dtype).reshape(-1, 3)
        return np.concatenate([old, np.asarray(new, dtype).reshape(-1, 3)]) if len(new) else old.copy()

    return dict(vertices=rows(v, new_vertices, f32), faces=rows(f, new_faces, np.int32),
                colors=None if colors is None else rows(colors, new_colors, f32),
                normals=rows(mesh["normals"], new_normals, f32), cells=rows(mesh["cells"], [[-1, -1, -1]] * n_new, np.int32),
                n_open=mesh["n_open"], status=status, hole=hole, ring_offsets=ring_offsets,
                ring_vertices=(np.concatenate(rings) if rings else np.zeros(0, np.int64)).astype(np.int32),
                face_loop=np.concatenate([np.full(F, -1, np.int64), np.asarray(face_loop, np.int64)]).astype(np.int32),
                new_vertex_loop=np.asarray(new_vertex_loop, np.int32).reshape(-1), centres=centres, unit=topo["unit"])


def hole_area(result):
    """[L] float64"""
    return result["hole"][:, 1].astype(f64) * T.quanta(result["unit"])[0]


# ---- hand meshes ------------------------------------------------------------------------------------------------------------------- #
def as_mesh(v, f, colors=None, seed=None):
    """(vertices, faces) -> the dict fill_holes takes: unit normals along z, cells counting up, random colours with a seed"""
    v = np.asarray(v, f32).reshape(-1, 3)
    if seed is not None:
        colors = np.random.default_rng(seed).random((len(v), 3)).astype(f32)
    normals = np.tile(np.array([0, 0, 1], f32), (len(v), 1))
    cells = np.stack([np.arange(len(v))] * 3, 1).astype(np.int32)
    return dict(vertices=v, faces=np.asarray(f, np.int32).reshape(-1, 3), colors=colors, normals=normals, cells=cells, n_open=7)


def open_cube():
    """a cube without its top: one simple 4-ring; filled it is closed with Euler characteristic 2"""
    v = [[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)]
    quads = [(0, 2, 3, 1), (0, 1, 5, 4), (1, 3, 7, 5), (3, 2, 6, 7), (2, 0, 4, 6)]      # bottom and four sides, outward
    return T._mesh(v, [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])


def open_tetrahedron():
    """a tetrahedron without one face: one simple 3-ring"""
    v, f = T.tetrahedron()
    return v, f[:3].copy()


def corner_squares():
    """two squares that share one corner: one loop, not simple"""
    v = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 1, 0], [2, 2, 0], [1, 2, 0]]
    return T._mesh(v, [[0, 1, 2], [0, 2, 3], [2, 4, 5], [2, 5, 6]])


def clashing_triangles():
    """two adjacent triangles wound against each other: the shared edge is interior, the ring's half-edges collide (in != out)"""
    return T._mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], [[0, 1, 2], [1, 2, 3]])


def far_ring():
    """a square whose ring has a coordinate of 1e30: unmeasured"""
    return T._mesh([[0, 0, 0], [1, 0, 0], [1e30, 1, 0], [0, 1, 0]], [[0, 1, 2], [0, 2, 3]])


def separate_squares(n):
    """n unit squares of two triangles each that share nothing: n simple 4-rings"""
    i = np.arange(n)
    x, y = (i % 100).astype(f64) * 2.0, (i // 100).astype(f64) * 2.0
    z = 0 * x
    v = np.stack([np.stack([x, y, z], 1), np.stack([x + 1, y, z], 1), np.stack([x + 1, y + 1, z], 1), np.stack([x, y + 1, z], 1)], 1)
    b = 4 * i
    f = np.stack([np.stack([b, b + 1, b + 2], 1), np.stack([b, b + 2, b + 3], 1)], 1)
    return T._mesh(v.reshape(-1, 3), f.reshape(-1, 3))


def hand_meshes():
    """name -> (vertices, faces)"""
    return dict(cube=open_cube(), tetrahedron=open_tetrahedron(), annulus=T.annulus(8), fan=T.fan(64), book=T.book(3),
                corner=corner_squares(), clash=clashing_triangles(), far=far_ring())
