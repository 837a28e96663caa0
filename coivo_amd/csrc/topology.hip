// topology.hip -- what an indexed triangle mesh is: its connected components, its edges (boundary, non-manifold), its boundary loops,
// their areas and lengths, and the mesh without the components a caller drops.  Contract: include/colvo.h
// (colvo_mesh_topology_*, colvo_mesh_clean_*); replica: tests/topology_ref.py.
//
//   components  k_unite_faces: a lock-free union-find over the vertices, one thread per face.  A root is only ever hung under a
//               SMALLER vertex (atomicCAS on the root's own word), so a parent chain strictly descends and the root that survives is
//               the smallest vertex of the class whatever the schedule.  k_flatten walks every vertex to its root; the roots are
//               numbered in ascending order by the ordered scan of csrc/scan.hip.
//   edges       the sides of the live faces are bucketed by their smaller endpoint (count, scan, fill through an atomic cursor; the
//               order inside a bucket is free); one thread per side scans its bucket for equal partners, and the side at the lowest
//               position of each edge counts it.  A bucket scan is quadratic in the edges at one lower endpoint.
//   loops       the same union-find over the edges of multiplicity one.
//   clean       marks, two ordered scans, ordered gathers.
//
// No thread waits on another thread's store: every loop has a bound known on entry (a chain descends, so it has at most V links;
// a failed atomicCAS returns the word's current value, which is smaller, and the walk goes on from there), and a thread that
// exhausts its bound sets stats[5] and leaves.  Parent words are read with agent-scope atomic loads and written with atomics only;
// a stale parent is still an older ancestor -- smaller and in the same class -- so it can cost steps, never correctness.
//
// Every sum is an int64 (or int32) integer add, so a call's bits depend on neither the schedule nor the stream.  The measures are
// float64 in the association the contract writes -- contraction is off for this whole file.
#include "mesh_common.h"

#pragma clang fp contract(off)

namespace colvo {
namespace {

constexpr int NT = 256;
constexpr int MAX_F = 1 << 29;             // 3 F half-edges stay below 2^31
enum { ST_C = 0, ST_DEAD, ST_L, ST_BAD_FACES, ST_BAD_EDGES, ST_GAVE_UP, ST_SIDES, ST_COUNT = 8 };
enum { COL_MIN = 0, COL_NV, COL_NF, COL_NE, COL_NB, COL_NNM, COL_NL, COL_AREA, COLS = 8 };
enum { LCOL_MIN = 0, LCOL_COMP, LCOL_NE, LCOL_LEN, LCOLS = 4 };

__device__ __forceinline__ int ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a, b in [0, V): their classes become one.  At most a + b + 1 < 2 V rounds: every round ends the call or lowers a or b.
__device__ __forceinline__ void unite(int32_t* __restrict__ parent, int a, int b, long long bound, int32_t* __restrict__ gave_up) {
    for (long long round = 0; round < bound; ++round) {
        const int pa = ld(parent + a);
        if (pa != a) {                                           // path halving: a's parent becomes its grandparent
            const int ga = ld(parent + pa);
            if (ga != pa) atomicMin(parent + a, ga);
            a = ga;
            continue;
        }
        const int pb = ld(parent + b);
        if (pb != b) {
            const int gb = ld(parent + pb);
            if (gb != pb) atomicMin(parent + b, gb);
            b = gb;
            continue;
        }
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        if (a == hi) a = old; else b = old;                      // no longer a root: old < hi, go on from there
    }
    atomicOr(gave_up, 1);
}

__global__ __launch_bounds__(NT) void k_identity(int32_t* __restrict__ a, int n) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) a[i] = i;
}

__global__ __launch_bounds__(NT) void k_unite_faces(const int32_t* __restrict__ faces, int V, int F, int32_t* __restrict__ parent,
                                                    int32_t* __restrict__ stats) {
    const int f = blockIdx.x * NT + threadIdx.x;
    int v[3];
    const bool live = f < F && live_face(faces, f, V, v);
    const int n_dead = (int)__popcll(__ballot(f < F && !live));
    if ((threadIdx.x & 63) == 0 && n_dead) atomicAdd(stats + ST_DEAD, n_dead);
    if (!live) return;
    const long long bound = 2ll * V + 2;
    unite(parent, v[0], v[1], bound, stats + ST_GAVE_UP);
    unite(parent, v[1], v[2], bound, stats + ST_GAVE_UP);
}

// root[v] = the root of v (or -1 where `only` is given and zero); marks[v] = is v such a root.  After the kernel that united.
__global__ __launch_bounds__(NT) void k_flatten(const int32_t* __restrict__ parent, const int32_t* __restrict__ only, int V,
                                                int32_t* __restrict__ root, int32_t* __restrict__ marks, int32_t* __restrict__ stats) {
    const int v = blockIdx.x * NT + threadIdx.x;
    if (v >= V) return;
    if (only != nullptr && only[v] == 0) {
        root[v] = -1;
        marks[v] = 0;
        return;
    }
    int r = v;
    bool done = false;
    for (long long step = 0; step <= (long long)V; ++step) {
        const int p = parent[r];
        if (p == r) { done = true; break; }
        r = p;
    }
    if (!done) atomicOr(stats + ST_GAVE_UP, 1);
    root[v] = r;
    marks[v] = (int)(r == v);
}

// label[v]: the root of v on entry (-1: none), the number of its root on exit
__global__ __launch_bounds__(NT) void k_number(int32_t* __restrict__ label, const int32_t* __restrict__ slots, int V) {
    const int v = blockIdx.x * NT + threadIdx.x;
    if (v >= V) return;
    const int r = label[v];
    label[v] = (unsigned)r < (unsigned)V ? slots[r] : -1;
}

__global__ __launch_bounds__(NT) void k_face_component(const int32_t* __restrict__ faces, const int32_t* __restrict__ vertex_component,
                                                       int V, int F, int32_t* __restrict__ face_component) {
    const int f = blockIdx.x * NT + threadIdx.x;
    if (f >= F) return;
    int v[3];
    face_component[f] = live_face(faces, f, V, v) ? vertex_component[v[0]] : -1;
}

__global__ __launch_bounds__(NT) void k_components_init(const int32_t* __restrict__ roots, int C, long long* __restrict__ components) {
    const int c = blockIdx.x * NT + threadIdx.x;
    if (c >= C) return;
#pragma unroll
    for (int k = 0; k < COLS; ++k) components[(size_t)c * COLS + k] = k == COL_MIN ? (long long)roots[c] : 0ll;
}

__global__ __launch_bounds__(NT) void k_count_vertices(const int32_t* __restrict__ vertex_component, int V, int C,
                                                       long long* __restrict__ components) {
    const int v = blockIdx.x * NT + threadIdx.x;
    int c = v < V ? vertex_component[v] : -1;
    if ((unsigned)c >= (unsigned)C) c = -1;
    const int col[1] = {COL_NV};
    const long long one[1] = {1ll};
    record_add(components, COLS, c, col, one);
}

// per face: its component's face count and area; the three sides into the count of their smaller endpoint
__global__ __launch_bounds__(NT) void k_faces_measure(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                      const int32_t* __restrict__ face_component, int V, int F, int C, float unit,
                                                      long long* __restrict__ components, int32_t* __restrict__ counts,
                                                      int32_t* __restrict__ stats) {
    const int f = blockIdx.x * NT + threadIdx.x;
    int v[3];
    int c = -1;
    if (f < F && live_face(faces, f, V, v)) c = face_component[f];
    if ((unsigned)c >= (unsigned)C) c = -1;
    long long add[2] = {1ll, 0ll};
    bool bad = false;
    if (c >= 0) {
        double p0[3], p1[3], p2[3];
        load_point(vertices, v[0], p0);
        load_point(vertices, v[1], p1);
        load_point(vertices, v[2], p2);
        const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        const double s = (nx * nx + ny * ny) + nz * nz;
        bad = !to_quanta(0.5 * sqrt(s), quanta_of(unit).area, add[1]);
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicAdd(counts + min(v[k], v[(k + 1) % 3]), 1);
    }
    const int n_bad = (int)__popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0 && n_bad) atomicAdd(stats + ST_BAD_FACES, n_bad);
    const int col[2] = {COL_NF, COL_AREA};
    record_add(components, COLS, c, col, add);
}

// the sides, into their buckets: side_lo / side_hi [start[lo] + cursor]
__global__ __launch_bounds__(NT) void k_sides_fill(const int32_t* __restrict__ faces, int V, int F, const int32_t* __restrict__ start,
                                                   int32_t* __restrict__ cursor, int cap, int32_t* __restrict__ side_lo,
                                                   int32_t* __restrict__ side_hi) {
    const int f = blockIdx.x * NT + threadIdx.x;
    int v[3];
    if (f >= F || !live_face(faces, f, V, v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = v[k], b = v[(k + 1) % 3];
        const int lo = min(a, b), hi = max(a, b);
        const int pos = start[lo] + atomicAdd(cursor + lo, 1);
        if ((unsigned)pos < (unsigned)cap) {                     // (never past the buffers)
            side_lo[pos] = lo;
            side_hi[pos] = hi;
        }
    }
}

// one thread per side: multiplicity m of its edge within the bucket; the side at the edge's lowest position counts the edge; an edge
// with m = 1 is boundary: kind[pos] = 1, its ends are marked and united in the loops' forest
__global__ __launch_bounds__(NT) void k_edges(const int32_t* __restrict__ side_lo, const int32_t* __restrict__ side_hi,
                                              const int32_t* __restrict__ start, const int32_t* __restrict__ counts,
                                              const int32_t* __restrict__ vertex_component, int V, int C, int cap,
                                              long long* __restrict__ components, uint8_t* __restrict__ kind,
                                              int32_t* __restrict__ on_boundary, int32_t* __restrict__ parent2, int32_t* __restrict__ stats) {
    const int pos = blockIdx.x * NT + threadIdx.x;
    const int n_sides = min(max(stats[ST_SIDES], 0), cap);
    int c = -1;
    long long add[3] = {0ll, 0ll, 0ll};
    bool boundary = false;
    int lo = 0, hi = 0;
    if (pos < n_sides) {
        lo = side_lo[pos];
        hi = side_hi[pos];
        const int b0 = start[lo], b1 = min(b0 + counts[lo], n_sides);
        int m = 0, first = pos;
        for (int i = b0; i < b1; ++i) {
            if (side_hi[i] == hi) {
                ++m;
                first = min(first, i);
            }
        }
        if (first == pos) {
            c = vertex_component[lo];
            if ((unsigned)c >= (unsigned)C) c = -1;
            boundary = m == 1;
            add[0] = 1ll;
            add[1] = (long long)boundary;
            add[2] = (long long)(m > 2);
        }
        kind[pos] = (uint8_t)boundary;
    }
    const int col[3] = {COL_NE, COL_NB, COL_NNM};
    record_add(components, COLS, c, col, add);
    if (boundary) {
        on_boundary[lo] = 1;                                     // idempotent same-value stores
        on_boundary[hi] = 1;
        unite(parent2, lo, hi, 2ll * V + 2, stats + ST_GAVE_UP);
    }
}

__global__ __launch_bounds__(NT) void k_loops_init(const int32_t* __restrict__ roots2, const int32_t* __restrict__ vertex_component, int V,
                                                   int C, int L, long long* __restrict__ loops, long long* __restrict__ components) {
    const int l = blockIdx.x * NT + threadIdx.x;
    int c = -1;
    if (l < L) {
        const int r = roots2[l];
        c = (unsigned)r < (unsigned)V ? vertex_component[r] : -1;
        if ((unsigned)c >= (unsigned)C) c = -1;
        loops[(size_t)l * LCOLS + LCOL_MIN] = r;
        loops[(size_t)l * LCOLS + LCOL_COMP] = c;
        loops[(size_t)l * LCOLS + LCOL_NE] = 0;
        loops[(size_t)l * LCOLS + LCOL_LEN] = 0;
    }
    const int col[1] = {COL_NL};
    const long long one[1] = {1ll};
    record_add(components, COLS, c, col, one);
}

__global__ __launch_bounds__(NT) void k_loops_measure(const float* __restrict__ vertices, const int32_t* __restrict__ side_lo,
                                                      const int32_t* __restrict__ side_hi, const uint8_t* __restrict__ kind,
                                                      const int32_t* __restrict__ vertex_loop, int L, int cap, float unit,
                                                      long long* __restrict__ loops, int32_t* __restrict__ stats) {
    const int pos = blockIdx.x * NT + threadIdx.x;
    const int n_sides = min(max(stats[ST_SIDES], 0), cap);
    int l = -1;
    long long add[2] = {1ll, 0ll};
    bool bad = false;
    if (pos < n_sides && kind[pos]) {
        const int lo = side_lo[pos], hi = side_hi[pos];
        l = vertex_loop[lo];
        if ((unsigned)l >= (unsigned)L) l = -1;
        if (l >= 0) {
            double p[3], q[3];
            load_point(vertices, lo, p);
            load_point(vertices, hi, q);
            const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
            bad = !to_quanta(sqrt((dx * dx + dy * dy) + dz * dz), quanta_of(unit).length, add[1]);
        }
    }
    const int n_bad = (int)__popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0 && n_bad) atomicAdd(stats + ST_BAD_EDGES, n_bad);
    const int col[2] = {LCOL_NE, LCOL_LEN};
    record_add(loops, LCOLS, l, col, add);
}

// ---- clean ------------------------------------------------------------------------------------------------------------------------ //
__global__ __launch_bounds__(NT) void k_clean_mark(const int32_t* __restrict__ component, const uint8_t* __restrict__ kept, int n, int C,
                                                   int32_t* __restrict__ marks) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int c = component[i];
    marks[i] = (unsigned)c < (unsigned)C ? (int)(kept[c] != 0) : 0;
}

// rows of three 32-bit words: dst[i] = src[index[i]]
__global__ __launch_bounds__(NT) void k_gather_rows(const int32_t* __restrict__ src, const int32_t* __restrict__ index, int n_src, int n,
                                                    int32_t* __restrict__ dst) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int r = index[i];
    const bool in = (unsigned)r < (unsigned)n_src;
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[(size_t)i * 3 + k] = in ? src[(size_t)r * 3 + k] : 0;
}

__global__ __launch_bounds__(NT) void k_gather_faces(const int32_t* __restrict__ faces, const int32_t* __restrict__ face_index,
                                                     const int32_t* __restrict__ vertex_map, int V, int F, int n,
                                                     int32_t* __restrict__ dst) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int r = face_index[i];
    const bool in = (unsigned)r < (unsigned)F;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int v = in ? faces[(size_t)r * 3 + k] : -1;
        dst[(size_t)i * 3 + k] = (unsigned)v < (unsigned)V ? vertex_map[v] : -1;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------ //
struct TopoWs {
    int32_t *parent, *parent2;             // the two forests
    int32_t *slots, *roots, *sums;         // marks -> numbers of the component roots, the roots in ascending order, the scan's chunk sums
    int32_t *slots2, *roots2;              // the same for the loops
    int32_t *start, *counts;               // bucket starts (counts before the scan), sides per smaller endpoint
    int32_t *on_boundary;
    int32_t *side_lo, *side_hi;
    uint8_t* kind;
    size_t bytes;
};

TopoWs topo_ws(void* base, int V, int F) {
    Carver c(base);
    TopoWs w;
    const size_t v = (size_t)V, s = 3 * (size_t)F;
    w.parent = c.take<int32_t>(v);
    w.parent2 = c.take<int32_t>(v);
    w.slots = c.take<int32_t>(v);
    w.roots = c.take<int32_t>(v);
    w.sums = c.take<int32_t>(scan_chunks(V));
    w.slots2 = c.take<int32_t>(v);
    w.roots2 = c.take<int32_t>(v);
    w.start = c.take<int32_t>(v);
    w.counts = c.take<int32_t>(v);
    w.on_boundary = c.take<int32_t>(v);
    w.side_lo = c.take<int32_t>(s);
    w.side_hi = c.take<int32_t>(s);
    w.kind = c.take<uint8_t>(s);
    w.bytes = c.bytes();
    return w;
}

struct CleanWs {
    int32_t *vsums, *fslots, *fsums;
    size_t bytes;
};

CleanWs clean_ws(void* base, int V, int F) {
    Carver c(base);
    CleanWs w;
    w.vsums = c.take<int32_t>(scan_chunks(V));
    w.fslots = c.take<int32_t>((size_t)F);
    w.fsums = c.take<int32_t>(scan_chunks(F));
    w.bytes = c.bytes();
    return w;
}

inline bool topo_shape(int V, int F) { return V >= 1 && F >= 0 && F < MAX_F; }      // (V < 2^31 by its type)

}  // namespace
}  // namespace colvo

using namespace colvo;

#define TOPO_CHECK_SHAPE(who) \
    COLVO_CHECK_ARG(topo_shape(V, F), who ": bad shape: V = %d (1 .. 2^31 - 1), F = %d (0 .. 2^29 - 1)", V, F)

extern "C" size_t colvo_mesh_topology_scratch_bytes(int V, int F) {
    if (!topo_shape(V, F)) return 0;
    return topo_ws(nullptr, V, F).bytes;
}

extern "C" int colvo_mesh_topology_components(const int32_t* faces, int V, int F, void* scratch, int32_t* vertex_component,
                                              int32_t* face_component, int32_t* stats, colvo_stream_t stream) {
    TOPO_CHECK_SHAPE("colvo_mesh_topology_components");
    COLVO_CHECK_ARG(scratch && vertex_component && stats && (F == 0 || (faces && face_component)),
                    "colvo_mesh_topology_components: null pointer argument");
    COLVO_CHECK_ARG(aligned16(scratch), "colvo_mesh_topology_components: scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const TopoWs w = topo_ws(scratch, V, F);
    const dim3 gv(blocks_of(V, NT)), gf(blocks_of(F, NT));
    COLVO_CHECK_HIP(hipMemsetAsync(stats, 0, ST_COUNT * sizeof(int32_t), s), "colvo_mesh_topology_components");
    colvo::launch(k_identity, gv, dim3(NT), 0, s, w.parent, V);
    COLVO_CHECK_LAUNCH("k_identity");
    if (F > 0) {
        colvo::launch(k_unite_faces, gf, dim3(NT), 0, s, faces, V, F, w.parent, stats);
        COLVO_CHECK_LAUNCH("k_unite_faces");
    }
    colvo::launch(k_flatten, gv, dim3(NT), 0, s, w.parent, (const int32_t*)nullptr, V, vertex_component, w.slots, stats);
    COLVO_CHECK_LAUNCH("k_flatten");
    const int rc = scan_exclusive(Scan{w.slots, V, nullptr, w.sums, stats + ST_C, w.roots, V}, s);
    if (rc != 0) return rc;
    colvo::launch(k_number, gv, dim3(NT), 0, s, vertex_component, w.slots, V);
    COLVO_CHECK_LAUNCH("k_number");
    if (F > 0) {
        colvo::launch(k_face_component, gf, dim3(NT), 0, s, faces, vertex_component, V, F, face_component);
        COLVO_CHECK_LAUNCH("k_face_component");
    }
    return 0;
}

extern "C" int colvo_mesh_topology_edges(const float* vertices, const int32_t* faces, int V, int F, float unit, int C, void* scratch,
                                         const int32_t* vertex_component, const int32_t* face_component, int64_t* components,
                                         int32_t* vertex_loop, int32_t* stats, colvo_stream_t stream) {
    TOPO_CHECK_SHAPE("colvo_mesh_topology_edges");
    COLVO_CHECK_ARG(C >= 1 && C <= V, "colvo_mesh_topology_edges: bad shape: C = %d (1 .. V = %d)", C, V);
    COLVO_CHECK_ARG(unit_ok(unit), "colvo_mesh_topology_edges: unit %g must be finite and positive", (double)unit);
    COLVO_CHECK_ARG(vertices && scratch && vertex_component && components && vertex_loop && stats && (F == 0 || (faces && face_component)),
                    "colvo_mesh_topology_edges: null pointer argument");
    COLVO_CHECK_ARG(aligned16(scratch), "colvo_mesh_topology_edges: scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const TopoWs w = topo_ws(scratch, V, F);
    const dim3 gv(blocks_of(V, NT)), gf(blocks_of(F, NT)), gs(blocks_of(3ll * F, NT));
    const int cap = 3 * F;
    long long* rec = reinterpret_cast<long long*>(components);
    colvo::launch(k_components_init, dim3(blocks_of(C, NT)), dim3(NT), 0, s, w.roots, C, rec);
    COLVO_CHECK_LAUNCH("k_components_init");
    colvo::launch(k_count_vertices, gv, dim3(NT), 0, s, vertex_component, V, C, rec);
    COLVO_CHECK_LAUNCH("k_count_vertices");
    COLVO_CHECK_HIP(hipMemsetAsync(w.on_boundary, 0, (size_t)V * 4, s), "colvo_mesh_topology_edges");
    colvo::launch(k_identity, gv, dim3(NT), 0, s, w.parent2, V);
    COLVO_CHECK_LAUNCH("k_identity");
    if (F > 0) {
        COLVO_CHECK_HIP(hipMemsetAsync(w.start, 0, (size_t)V * 4, s), "colvo_mesh_topology_edges");
        COLVO_CHECK_HIP(hipMemsetAsync(w.counts, 0, (size_t)V * 4, s), "colvo_mesh_topology_edges");
        colvo::launch(k_faces_measure, gf, dim3(NT), 0, s, vertices, faces, face_component, V, F, C, unit, rec, w.start, stats);
        COLVO_CHECK_LAUNCH("k_faces_measure");
        int rc = scan_exclusive(Scan{w.start, V, nullptr, w.sums, stats + ST_SIDES, nullptr, 0}, s);
        if (rc != 0) return rc;
        colvo::launch(k_sides_fill, gf, dim3(NT), 0, s, faces, V, F, w.start, w.counts, cap, w.side_lo, w.side_hi);
        COLVO_CHECK_LAUNCH("k_sides_fill");
        colvo::launch(k_edges, gs, dim3(NT), 0, s, w.side_lo, w.side_hi, w.start, w.counts, vertex_component, V, C, cap, rec, w.kind,
                      w.on_boundary, w.parent2, stats);
        COLVO_CHECK_LAUNCH("k_edges");
    }
    colvo::launch(k_flatten, gv, dim3(NT), 0, s, w.parent2, w.on_boundary, V, vertex_loop, w.slots2, stats);
    COLVO_CHECK_LAUNCH("k_flatten");
    const int rc = scan_exclusive(Scan{w.slots2, V, nullptr, w.sums, stats + ST_L, w.roots2, V}, s);
    if (rc != 0) return rc;
    colvo::launch(k_number, gv, dim3(NT), 0, s, vertex_loop, w.slots2, V);
    COLVO_CHECK_LAUNCH("k_number");
    return 0;
}

extern "C" int colvo_mesh_topology_loops(const float* vertices, int V, int F, float unit, int C, int L, const void* scratch,
                                         const int32_t* vertex_component, const int32_t* vertex_loop, int64_t* components,
                                         int64_t* loops, int32_t* stats, colvo_stream_t stream) {
    TOPO_CHECK_SHAPE("colvo_mesh_topology_loops");
    COLVO_CHECK_ARG(C >= 1 && C <= V && L >= 1 && L <= V && F >= 1, "colvo_mesh_topology_loops: bad shape: C = %d, L = %d (1 .. V = %d), F = %d (>= 1)",
                    C, L, V, F);
    COLVO_CHECK_ARG(unit_ok(unit), "colvo_mesh_topology_loops: unit %g must be finite and positive", (double)unit);
    COLVO_CHECK_ARG(vertices && scratch && vertex_component && vertex_loop && components && loops && stats,
                    "colvo_mesh_topology_loops: null pointer argument");
    COLVO_CHECK_ARG(aligned16(scratch), "colvo_mesh_topology_loops: scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const TopoWs w = topo_ws(const_cast<void*>(scratch), V, F);
    colvo::launch(k_loops_init, dim3(blocks_of(L, NT)), dim3(NT), 0, s, w.roots2, vertex_component, V, C, L,
                  reinterpret_cast<long long*>(loops), reinterpret_cast<long long*>(components));
    COLVO_CHECK_LAUNCH("k_loops_init");
    colvo::launch(k_loops_measure, dim3(blocks_of(3ll * F, NT)), dim3(NT), 0, s, vertices, w.side_lo, w.side_hi, w.kind, vertex_loop, L,
                  3 * F, unit, reinterpret_cast<long long*>(loops), stats);
    COLVO_CHECK_LAUNCH("k_loops_measure");
    return 0;
}

extern "C" size_t colvo_mesh_clean_scratch_bytes(int V, int F) {
    if (!topo_shape(V, F)) return 0;
    return clean_ws(nullptr, V, F).bytes;
}

extern "C" int colvo_mesh_clean_plan(const int32_t* vertex_component, const int32_t* face_component, const uint8_t* kept, int V, int F,
                                     int C, void* scratch, int32_t* vertex_map, int32_t* vertex_index, int32_t* face_index,
                                     int32_t* counts, colvo_stream_t stream) {
    TOPO_CHECK_SHAPE("colvo_mesh_clean_plan");
    COLVO_CHECK_ARG(C >= 1 && C <= V, "colvo_mesh_clean_plan: bad shape: C = %d (1 .. V = %d)", C, V);
    COLVO_CHECK_ARG(vertex_component && kept && scratch && vertex_map && vertex_index && counts && (F == 0 || (face_component && face_index)),
                    "colvo_mesh_clean_plan: null pointer argument");
    COLVO_CHECK_ARG(aligned16(scratch), "colvo_mesh_clean_plan: scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const CleanWs w = clean_ws(scratch, V, F);
    COLVO_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), s), "colvo_mesh_clean_plan");
    colvo::launch(k_clean_mark, dim3(blocks_of(V, NT)), dim3(NT), 0, s, vertex_component, kept, V, C, vertex_map);
    COLVO_CHECK_LAUNCH("k_clean_mark");
    int rc = scan_exclusive(Scan{vertex_map, V, nullptr, w.vsums, counts, vertex_index, V}, s);
    if (rc != 0 || F == 0) return rc;
    colvo::launch(k_clean_mark, dim3(blocks_of(F, NT)), dim3(NT), 0, s, face_component, kept, F, C, w.fslots);
    COLVO_CHECK_LAUNCH("k_clean_mark");
    return scan_exclusive(Scan{w.fslots, F, nullptr, w.fsums, counts + 1, face_index, F}, s);
}

extern "C" int colvo_mesh_clean_write(const float* vertices, const float* colors, const float* normals, const int32_t* cells,
                                      const int32_t* faces, int V, int F, const int32_t* vertex_map, const int32_t* vertex_index,
                                      const int32_t* face_index, int V2, int F2, float* out_vertices, float* out_colors,
                                      float* out_normals, int32_t* out_cells, int32_t* out_faces, colvo_stream_t stream) {
    TOPO_CHECK_SHAPE("colvo_mesh_clean_write");
    COLVO_CHECK_ARG(V2 >= 0 && V2 <= V && F2 >= 0 && F2 <= F && V2 + F2 > 0, "colvo_mesh_clean_write: bad shape: V2 = %d (0 .. %d), F2 = %d (0 .. %d), one of them positive",
                    V2, V, F2, F);
    COLVO_CHECK_ARG(vertex_map && (V2 == 0 || (vertices && vertex_index && out_vertices)) && (F2 == 0 || (faces && face_index && out_faces)) &&
                        (!colors == !out_colors) && (!normals == !out_normals) && (!cells == !out_cells),
                    "colvo_mesh_clean_write: null pointer argument (colors, normals and cells go with their outputs)");
    hipStream_t s = (hipStream_t)stream;
    if (V2 > 0) {
        const dim3 g(blocks_of(V2, NT));
        const int32_t* src[4] = {reinterpret_cast<const int32_t*>(vertices), reinterpret_cast<const int32_t*>(colors),
                                 reinterpret_cast<const int32_t*>(normals), cells};
        int32_t* dst[4] = {reinterpret_cast<int32_t*>(out_vertices), reinterpret_cast<int32_t*>(out_colors),
                           reinterpret_cast<int32_t*>(out_normals), out_cells};
        for (int k = 0; k < 4; ++k) {
            if (src[k] == nullptr) continue;
            colvo::launch(k_gather_rows, g, dim3(NT), 0, s, src[k], vertex_index, V, V2, dst[k]);
            COLVO_CHECK_LAUNCH("k_gather_rows");
        }
    }
    if (F2 > 0) {
        colvo::launch(k_gather_faces, dim3(blocks_of(F2, NT)), dim3(NT), 0, s, faces, face_index, vertex_map, V, F, F2, out_faces);
        COLVO_CHECK_LAUNCH("k_gather_faces");
    }
    return 0;
}
