// fill.hip -- the holes of an indexed triangle mesh: which boundary loops are simple rings, the ring of each in order, the area a fan
// to the ring's mean spans, and the mesh with the short rings closed by that fan.  Contract: include/colvo.h
// (colvo_mesh_fill_*); replica: tests/fill_ref.py.  It reads mesh_topology's vertex_loop and loops (csrc/topology.hip) and trusts
// neither: every index is checked against its buffer before a gather.
//
//   half-edges  the sides of the live faces are bucketed by their smaller endpoint as in topology.hip, here with a direction bit (the
//               buckets there drop it); one thread per side counts its edge's multiplicity in the bucket; a side of multiplicity one
//               is a boundary half-edge from -> to: out[from], in[to], succ[from] = to, and one more edge of from's loop.
//   classify    one thread per vertex: a loop with a vertex whose out or in is not 1 is not simple; the vertex's coordinates (and
//               colours) go, in quanta, into its loop's sums.  One thread per loop then decides, and writes the ring's length and centre.
//   rank        pointer jumping over (next, distance) pairs, double-buffered, one launch per doubling round: the cycle is cut at the
//               loop's smallest vertex (the vertex whose successor that is ends the list and points at itself with distance 0), so
//               after ceil(log2(n)) rounds every vertex holds its distance to the end, and its ring position is n - 1 - distance.
//               The host does not know the longest simple loop when it launches: it launches ceil(log2(min(V, 3 F))) rounds, and a
//               round beyond ceil(log2(longest simple loop)) -- a device word, counts[3] -- leaves at its first instruction.
//   measure     one thread per ring position: its fan face's area and half cross product, in quanta, into the loop's record.
//   number      status, faces and vertices per loop; three ordered scans (csrc/scan.hip) give the ring, vertex and face offsets.
//   write       copies of the old rows, one thread per loop for the new vertices, one per ring position for the new faces.
//
// No thread waits on another thread's store; every in-kernel loop has a bound known on entry (a bucket's size; the rounds are
// launches).  A thread that finds its inputs inconsistent sets counts[4] (a ranking that did not end where it must) or counts[7] (the
// topology is not this mesh's) and the wrapper raises.  Every sum is an integer add: a call's bits depend on neither the schedule nor
// the stream.  The measures are float64 in the association the contract writes -- contraction is off for this whole file.
#include "mesh_common.h"

#pragma clang fp contract(off)

namespace colvo {
namespace {

constexpr int NT = 256;
constexpr int MAX_F = 1 << 29;             // 3 F half-edges stay below 2^31
constexpr int MAX_V = 1 << 30;             // (hi << 1 | direction) stays in an int32, V + L in an int32
enum { CT_R = 0, CT_NV, CT_NF, CT_LONGEST, CT_GAVE_UP, CT_SIMPLE, CT_SIDES, CT_MISMATCH, CT_COUNT = 8 };
enum { SUM_NV = 0, SUM_X, SUM_Y, SUM_Z, SUM_R, SUM_G, SUM_B, SUM_COLS = 8 };
enum { MEAS_AREA = 0, MEAS_NX, MEAS_NY, MEAS_NZ, MEAS_COLS = 4 };
enum { FLAG_NOT_SIMPLE = 1, FLAG_UNMEASURED = 2 };
enum { FILL_FILLED = 0, FILL_TOO_LONG = 1, FILL_NOT_SIMPLE = 2, FILL_UNMEASURED = 3 };

__device__ __forceinline__ int loop_of(const int32_t* __restrict__ vertex_loop, int v, int L) {
    const int l = vertex_loop[v];
    return (unsigned)l < (unsigned)L ? l : -1;
}

// ---- boundary half-edges ---------------------------------------------------------------------------------------------------------- //
__global__ __launch_bounds__(NT) void k_fill_count(const int32_t* __restrict__ faces, int V, int F, int32_t* __restrict__ counts) {
    const int f = blockIdx.x * NT + threadIdx.x;
    int v[3];
    if (f >= F || !live_face(faces, f, V, v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(counts + min(v[k], v[(k + 1) % 3]), 1);
}

// side_lo / side_key [start[lo] + cursor]: key = hi << 1 | (the side runs hi -> lo)
__global__ __launch_bounds__(NT) void k_fill_sides(const int32_t* __restrict__ faces, int V, int F, const int32_t* __restrict__ start,
                                                   int32_t* __restrict__ cursor, int cap, int32_t* __restrict__ side_lo,
                                                   int32_t* __restrict__ side_key) {
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
            side_key[pos] = (hi << 1) | (int)(a > b);
        }
    }
}

// one thread per side: the multiplicity of its edge within the bucket; a side alone on its edge is a boundary half-edge
__global__ __launch_bounds__(NT) void k_fill_edges(const int32_t* __restrict__ side_lo, const int32_t* __restrict__ side_key,
                                                   const int32_t* __restrict__ start, const int32_t* __restrict__ cursor,
                                                   const int32_t* __restrict__ vertex_loop, int V, int L, int cap,
                                                   int32_t* __restrict__ out, int32_t* __restrict__ in, int32_t* __restrict__ succ,
                                                   int32_t* __restrict__ loop_edges, int32_t* __restrict__ counts) {
    const int pos = blockIdx.x * NT + threadIdx.x;
    const int n_sides = min(max(counts[CT_SIDES], 0), cap);
    if (pos >= n_sides) return;
    const int lo = side_lo[pos], key = side_key[pos];
    const int hi = key >> 1;
    if ((unsigned)lo >= (unsigned)V || (unsigned)hi >= (unsigned)V) return;
    const int b0 = max(start[lo], 0), b1 = min(b0 + max(cursor[lo], 0), n_sides);
    int m = 0;
    for (int i = b0; i < b1; ++i) m += (int)((side_key[i] >> 1) == hi);
    if (m != 1) return;
    const int from = (key & 1) ? hi : lo, to = (key & 1) ? lo : hi;
    atomicAdd(out + from, 1);
    atomicAdd(in + to, 1);
    succ[from] = to;                                             // (one writer wherever out[from] is 1: the only place it is read)
    const int l = loop_of(vertex_loop, from, L);
    if (l >= 0) atomicAdd(loop_edges + l, 1);
    else atomicOr(counts + CT_MISMATCH, 1);
}

// ---- classify ------------------------------------------------------------------------------------------------------------------- //
// llrint(x / quantum) and true, or 0 and false where the quotient is NaN or its magnitude 2^32 and more
__device__ __forceinline__ bool coordinate_quanta(float x, double quantum, long long& q) {
    const double t = (double)x / quantum;
    const bool ok = fabs(t) < 0x1p32;
    q = ok ? llrint(t) : 0ll;
    return ok;
}

__global__ __launch_bounds__(NT) void k_fill_vertices(const float* __restrict__ vertices, const float* __restrict__ colors,
                                                      const int32_t* __restrict__ vertex_loop, const long long* __restrict__ loops,
                                                      const int32_t* __restrict__ out, const int32_t* __restrict__ in, int V, int L,
                                                      float unit, long long* __restrict__ loop_sums, int32_t* __restrict__ loop_flags,
                                                      int32_t* __restrict__ counts) {
    const int v = blockIdx.x * NT + threadIdx.x;
    int l = -1;
    long long add[7] = {1ll, 0ll, 0ll, 0ll, 0ll, 0ll, 0ll};
    if (v < V) {
        l = loop_of(vertex_loop, v, L);
        const int o = out[v], i = in[v];
        if (l < 0) {
            if (o != 0 || i != 0) atomicOr(counts + CT_MISMATCH, 1);
        } else {
            int flags = (o != 1 || i != 1) ? FLAG_NOT_SIMPLE : 0;
            if ((long long)v < loops[(size_t)l * 4]) atomicOr(counts + CT_MISMATCH, 1);      // loops[l][0] is not the loop's smallest vertex
            const double ql = quanta_of(unit).length;
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if (!coordinate_quanta(vertices[(size_t)v * 3 + a], ql, add[SUM_X + a])) flags |= FLAG_UNMEASURED;
            if (colors != nullptr) {
#pragma unroll
                for (int a = 0; a < 3; ++a) coordinate_quanta(colors[(size_t)v * 3 + a], 0x1p-16, add[SUM_R + a]);
            }
            if (flags) atomicOr(loop_flags + l, flags);
        }
    }
    const int col[7] = {SUM_NV, SUM_X, SUM_Y, SUM_Z, SUM_R, SUM_G, SUM_B};
    record_add(loop_sums, SUM_COLS, l, col, add);
}

// one thread per loop (and one more: the entry behind the last): simple or not, the ring's length, the centre
__global__ __launch_bounds__(NT) void k_fill_loops(const long long* __restrict__ loops, const int32_t* __restrict__ vertex_loop,
                                                   const long long* __restrict__ loop_sums, const int32_t* __restrict__ loop_edges,
                                                   int32_t* __restrict__ loop_flags, int V, int L, float unit,
                                                   int32_t* __restrict__ ring_len, int32_t* __restrict__ ring_offsets,
                                                   float* __restrict__ centre, float* __restrict__ centre_color,
                                                   int32_t* __restrict__ counts) {
    const int l = blockIdx.x * NT + threadIdx.x;
    bool simple = false;
    if (l < L) {
        const long long head = loops[(size_t)l * 4], n = loops[(size_t)l * 4 + 2];
        const long long nv = loop_sums[(size_t)l * SUM_COLS + SUM_NV];
        const int flags = loop_flags[l];
        bool mismatch = (long long)loop_edges[l] != n || head < 0 || head >= (long long)V || n > (long long)V;
        if (!mismatch) mismatch = vertex_loop[head] != l;
        if (!mismatch && !(flags & FLAG_NOT_SIMPLE)) mismatch = nv != n;       // out = in = 1 throughout: as many edges as vertices
        if (mismatch) {
            atomicOr(counts + CT_MISMATCH, 1);
            atomicOr(loop_flags + l, FLAG_NOT_SIMPLE);
        }
        simple = !mismatch && !(flags & FLAG_NOT_SIMPLE) && n >= 3;
        if (!simple && !(flags & FLAG_NOT_SIMPLE)) atomicOr(loop_flags + l, FLAG_NOT_SIMPLE);
        const int len = simple ? (int)n : 0;
        ring_len[l] = len;
        ring_offsets[l] = len;
        const double ql = quanta_of(unit).length;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const long long s = loop_sums[(size_t)l * SUM_COLS + SUM_X + a], c = loop_sums[(size_t)l * SUM_COLS + SUM_R + a];
            centre[(size_t)l * 3 + a] = simple ? (float)(((double)s / (double)n) * ql) : 0.0f;
            centre_color[(size_t)l * 3 + a] = simple ? (float)(((double)c / (double)n) * 0x1p-16) : 0.0f;
        }
        if (simple) atomicMax(counts + CT_LONGEST, len);
    } else if (l == L) {
        ring_offsets[l] = 0;
    }
    const int n_simple = (int)__popcll(__ballot(simple));
    if ((threadIdx.x & 63) == 0 && n_simple) atomicAdd(counts + CT_SIMPLE, n_simple);
}

// ---- rank ------------------------------------------------------------------------------------------------------------------------ //
__global__ __launch_bounds__(NT) void k_rank_init(const int32_t* __restrict__ vertex_loop, const long long* __restrict__ loops,
                                                  const int32_t* __restrict__ ring_len, const int32_t* __restrict__ succ, int V, int L,
                                                  int2* __restrict__ pair, int32_t* __restrict__ counts) {
    const int v = blockIdx.x * NT + threadIdx.x;
    if (v >= V) return;
    int2 p = make_int2(-1, 0);
    const int l = loop_of(vertex_loop, v, L);
    if (l >= 0 && ring_len[l] > 0) {
        const int s = succ[v];
        if ((unsigned)s < (unsigned)V && vertex_loop[s] == l) p = (long long)s == loops[(size_t)l * 4] ? make_int2(v, 0) : make_int2(s, 1);
        else atomicOr(counts + CT_GAVE_UP, 1);
    }
    pair[v] = p;
}

// the rounds that the longest simple loop needs: ceil(log2(longest)), 2^rounds >= longest > the longest distance to a ring's end
__host__ __device__ __forceinline__ int doubling_rounds(int longest) {
    int r = 0;
    while (r < 31 && (1ll << r) < (long long)longest) ++r;
    return r;
}

// doubling round `round`: reads one buffer, writes the other (round 0 reads a); a round that the longest simple loop does not need
// leaves at once, the whole grid alike
__global__ __launch_bounds__(NT) void k_rank_round(int2* __restrict__ a, int2* __restrict__ b, int V, int round,
                                                   const int32_t* __restrict__ counts) {
    if ((1ll << round) >= (long long)counts[CT_LONGEST]) return;
    const int2* __restrict__ from = (round & 1) ? b : a;
    int2* __restrict__ to = (round & 1) ? a : b;
    const int v = blockIdx.x * NT + threadIdx.x;
    if (v >= V) return;
    int2 p = from[v];
    if ((unsigned)p.x < (unsigned)V) {
        const int2 q = from[p.x];
        p = (unsigned)q.x < (unsigned)V ? make_int2(q.x, (int)min((long long)p.y + q.y, 0x7fffffffll)) : make_int2(-1, 0);
    }
    to[v] = p;
}

// the vertex at distance d from its ring's end stands at position n - 1 - d
__global__ __launch_bounds__(NT) void k_rank_finish(const int2* __restrict__ a, const int2* __restrict__ b,
                                                    const int32_t* __restrict__ vertex_loop,
                                                    const long long* __restrict__ loops, const int32_t* __restrict__ ring_len,
                                                    const int32_t* __restrict__ ring_offsets, const int32_t* __restrict__ succ, int V,
                                                    int L, int32_t* __restrict__ ring_vertices, int32_t* __restrict__ counts) {
    const int v = blockIdx.x * NT + threadIdx.x;
    if (v >= V) return;
    const int l = loop_of(vertex_loop, v, L);
    if (l < 0) return;
    const int n = ring_len[l];
    if (n <= 0) return;
    const int2 p = (doubling_rounds(counts[CT_LONGEST]) & 1) ? b[v] : a[v];                  // where the last round that ran wrote
    bool ok = (unsigned)p.x < (unsigned)V && p.y >= 0 && p.y < n;
    if (ok) ok = vertex_loop[p.x] == l && (long long)succ[p.x] == loops[(size_t)l * 4];      // it ended at the ring's last vertex
    const long long slot = (long long)ring_offsets[l] + (n - 1 - p.y);
    if (ok && slot >= 0 && slot < (long long)V) ring_vertices[slot] = v;
    else atomicOr(counts + CT_GAVE_UP, 1);
}

// ---- measure --------------------------------------------------------------------------------------------------------------------- //
// the signed counterpart of to_quanta: llrint(m / quantum) and true, or 0 and false where the quotient is NaN or its magnitude 2^62 and more
__device__ __forceinline__ bool to_signed_quanta(double m, double quantum, long long& q) {
    const double t = m / quantum;
    const bool ok = fabs(t) < 0x1p62;
    q = ok ? llrint(t) : 0ll;
    return ok;
}

// Ring position i of loop l, k-th of its n: the fan face it stands for -- (ring[k+1 mod n], ring[k], centre) for n > 3, the one face
// (ring[0], ring[2], ring[1]) at k = 0 for n = 3 -- as vertex numbers (the centre: -1), or false where it stands for none or an index
// does not hold.
struct FanFace {
    int l, k, n, i, j, c;
};

__device__ __forceinline__ bool fan_face(const int32_t* __restrict__ ring_vertices, const int32_t* __restrict__ ring_offsets,
                                         const int32_t* __restrict__ ring_len, const int32_t* __restrict__ vertex_loop, int V, int L,
                                         int slot, int R, FanFace& f) {
    if (slot >= R || slot >= V) return false;
    const int v = ring_vertices[slot];
    if ((unsigned)v >= (unsigned)V) return false;
    f.l = loop_of(vertex_loop, v, L);
    if (f.l < 0) return false;
    const int off = ring_offsets[f.l];
    f.n = ring_len[f.l];
    f.k = slot - off;
    if (f.n < 3 || f.k < 0 || f.k >= f.n || off < 0 || (long long)off + f.n > (long long)min(R, V)) return false;
    if (f.n > 3) {
        f.i = ring_vertices[off + (f.k + 1 == f.n ? 0 : f.k + 1)];
        f.j = v;
        f.c = -1;
        return (unsigned)f.i < (unsigned)V;
    }
    if (f.k != 0) return false;
    f.i = v;
    f.j = ring_vertices[off + 2];
    f.c = ring_vertices[off + 1];
    return (unsigned)f.j < (unsigned)V && (unsigned)f.c < (unsigned)V;
}

__global__ __launch_bounds__(NT) void k_fan_measure(const float* __restrict__ vertices, const int32_t* __restrict__ ring_vertices,
                                                    const int32_t* __restrict__ ring_offsets, const int32_t* __restrict__ ring_len,
                                                    const int32_t* __restrict__ vertex_loop, const float* __restrict__ centre, int V,
                                                    int L, float unit, long long* __restrict__ loop_measures,
                                                    int32_t* __restrict__ loop_flags) {
    const int slot = blockIdx.x * NT + threadIdx.x;
    const int R = ring_offsets[L];
    FanFace f;
    int l = -1;
    long long add[4] = {0ll, 0ll, 0ll, 0ll};
    if (fan_face(ring_vertices, ring_offsets, ring_len, vertex_loop, V, L, slot, R, f)) {
        l = f.l;
        double p0[3], p1[3], p2[3];
        load_point(vertices, f.i, p0);
        load_point(vertices, f.j, p1);
        if (f.c >= 0) load_point(vertices, f.c, p2);
        else load_point(centre, l, p2);
        const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        const double s = (nx * nx + ny * ny) + nz * nz;
        const double qa = quanta_of(unit).area;
        bool ok = to_quanta(0.5 * sqrt(s), qa, add[MEAS_AREA]);
        ok = to_signed_quanta(0.5 * nx, qa, add[MEAS_NX]) && ok;
        ok = to_signed_quanta(0.5 * ny, qa, add[MEAS_NY]) && ok;
        ok = to_signed_quanta(0.5 * nz, qa, add[MEAS_NZ]) && ok;
        if (!ok) atomicOr(loop_flags + l, FLAG_UNMEASURED);
    }
    const int col[4] = {MEAS_AREA, MEAS_NX, MEAS_NY, MEAS_NZ};
    record_add(loop_measures, MEAS_COLS, l, col, add);
}

// ---- number ---------------------------------------------------------------------------------------------------------------------- //
__global__ __launch_bounds__(NT) void k_fill_number(const int32_t* __restrict__ ring_len, const int32_t* __restrict__ loop_flags,
                                                    const long long* __restrict__ loop_measures, int L, int max_edges,
                                                    int32_t* __restrict__ status, long long* __restrict__ hole,
                                                    int32_t* __restrict__ vertex_offsets, int32_t* __restrict__ face_offsets,
                                                    float* __restrict__ centre_normal) {
    const int l = blockIdx.x * NT + threadIdx.x;
    if (l > L) return;
    if (l == L) {
        vertex_offsets[l] = 0;
        face_offsets[l] = 0;
        return;
    }
    const int n = ring_len[l], flags = loop_flags[l];
    const int st = (n < 3 || (flags & FLAG_NOT_SIMPLE)) ? FILL_NOT_SIMPLE
                   : (flags & FLAG_UNMEASURED)          ? FILL_UNMEASURED
                   : n > max_edges                      ? FILL_TOO_LONG
                                                        : FILL_FILLED;
    const int n_faces = st != FILL_FILLED ? 0 : n > 3 ? n : 1;
    status[l] = st;
    hole[(size_t)l * 2] = n_faces;
    hole[(size_t)l * 2 + 1] = (st == FILL_FILLED || st == FILL_TOO_LONG) ? loop_measures[(size_t)l * MEAS_COLS + MEAS_AREA] : 0ll;
    vertex_offsets[l] = (int)(st == FILL_FILLED && n > 3);
    face_offsets[l] = n_faces;
    const double x = (double)loop_measures[(size_t)l * MEAS_COLS + MEAS_NX], y = (double)loop_measures[(size_t)l * MEAS_COLS + MEAS_NY],
                 z = (double)loop_measures[(size_t)l * MEAS_COLS + MEAS_NZ];
    const double len = sqrt((x * x + y * y) + z * z);
    const bool unit_normal = (st == FILL_FILLED || st == FILL_TOO_LONG) && len > 0.0;
    centre_normal[(size_t)l * 3] = unit_normal ? (float)(x / len) : 0.0f;
    centre_normal[(size_t)l * 3 + 1] = unit_normal ? (float)(y / len) : 0.0f;
    centre_normal[(size_t)l * 3 + 2] = unit_normal ? (float)(z / len) : 0.0f;
}

// ---- write ----------------------------------------------------------------------------------------------------------------------- //
__global__ __launch_bounds__(NT) void k_copy_words(const int32_t* __restrict__ src, size_t n, int32_t* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// one thread per loop: the centre of a filled ring of more than three edges becomes vertex V + vertex_offsets[l]
__global__ __launch_bounds__(NT) void k_fill_new_vertices(const int32_t* __restrict__ status, const int32_t* __restrict__ ring_len,
                                                          const int32_t* __restrict__ vertex_offsets, const float* __restrict__ centre,
                                                          const float* __restrict__ centre_color, const float* __restrict__ centre_normal,
                                                          int V, int L, int n_new, float* __restrict__ out_vertices,
                                                          float* __restrict__ out_colors, float* __restrict__ out_normals,
                                                          int32_t* __restrict__ out_cells, int32_t* __restrict__ new_vertex_loop) {
    const int l = blockIdx.x * NT + threadIdx.x;
    if (l >= L || status[l] != FILL_FILLED || ring_len[l] <= 3) return;
    const int r = vertex_offsets[l];
    if ((unsigned)r >= (unsigned)n_new) return;
    const size_t row = (size_t)V + r;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out_vertices[row * 3 + a] = centre[(size_t)l * 3 + a];
        if (out_colors != nullptr) out_colors[row * 3 + a] = centre_color[(size_t)l * 3 + a];
        if (out_normals != nullptr) out_normals[row * 3 + a] = centre_normal[(size_t)l * 3 + a];
        if (out_cells != nullptr) out_cells[row * 3 + a] = -1;
    }
    new_vertex_loop[r] = l;
}

// one thread per ring position: its fan face, if its loop is filled, becomes face F + face_offsets[l] + k
__global__ __launch_bounds__(NT) void k_fill_new_faces(const int32_t* __restrict__ status, const int32_t* __restrict__ ring_vertices,
                                                       const int32_t* __restrict__ ring_offsets, const int32_t* __restrict__ ring_len,
                                                       const int32_t* __restrict__ vertex_loop, const int32_t* __restrict__ vertex_offsets,
                                                       const int32_t* __restrict__ face_offsets, int V, int F, int L, int R, int n_new_v,
                                                       int n_new_f, int32_t* __restrict__ out_faces, int32_t* __restrict__ face_loop) {
    const int slot = blockIdx.x * NT + threadIdx.x;
    FanFace f;
    if (!fan_face(ring_vertices, ring_offsets, ring_len, vertex_loop, V, L, slot, R, f) || status[f.l] != FILL_FILLED) return;
    const long long r = (long long)face_offsets[f.l] + f.k;
    if (r < 0 || r >= (long long)n_new_f) return;
    int c = f.c;
    if (c < 0) {
        const int vr = vertex_offsets[f.l];
        if ((unsigned)vr >= (unsigned)n_new_v) return;
        c = V + vr;
    }
    const size_t row = (size_t)F + (size_t)r;
    out_faces[row * 3] = f.i;
    out_faces[row * 3 + 1] = f.j;
    out_faces[row * 3 + 2] = c;
    face_loop[row] = f.l;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------ //
struct FillWs {
    int32_t *start, *cursor;               // bucket starts (counts before the scan), sides per smaller endpoint
    int32_t *side_lo, *side_key;
    int32_t *out, *in, *succ;
    int2 *pair_a, *pair_b;                 // (next, distance), double-buffered
    int32_t* sums;                         // the scans' chunk sums
    long long *loop_sums, *loop_measures;  // [L][8], [L][4]
    int32_t *loop_flags, *loop_edges, *ring_len;
    int32_t *vertex_offsets, *face_offsets;                      // [L + 1]
    float *centre, *centre_color, *centre_normal;                // [L][3]
    size_t bytes;
};

FillWs fill_ws(void* base, int V, int F, int L) {
    Carver c(base);
    FillWs w;
    const size_t v = (size_t)V, s = 3 * (size_t)F, l = (size_t)L;
    w.start = c.take<int32_t>(v);
    w.cursor = c.take<int32_t>(v);
    w.side_lo = c.take<int32_t>(s);
    w.side_key = c.take<int32_t>(s);
    w.out = c.take<int32_t>(v);
    w.in = c.take<int32_t>(v);
    w.succ = c.take<int32_t>(v);
    w.pair_a = c.take<int2>(v);
    w.pair_b = c.take<int2>(v);
    w.sums = c.take<int32_t>(scan_chunks(max(V, L + 1)));
    w.loop_sums = c.take<long long>(l * SUM_COLS);
    w.loop_measures = c.take<long long>(l * MEAS_COLS);
    w.loop_flags = c.take<int32_t>(l);
    w.loop_edges = c.take<int32_t>(l);
    w.ring_len = c.take<int32_t>(l);
    w.vertex_offsets = c.take<int32_t>(l + 1);
    w.face_offsets = c.take<int32_t>(l + 1);
    w.centre = c.take<float>(l * 3);
    w.centre_color = c.take<float>(l * 3);
    w.centre_normal = c.take<float>(l * 3);
    w.bytes = c.bytes();
    return w;
}

inline bool fill_shape(int V, int F, int L) { return V >= 1 && V < MAX_V && F >= 1 && F < MAX_F && L >= 1 && L <= V; }

}  // namespace
}  // namespace colvo

using namespace colvo;

#define FILL_CHECK_SHAPE(who) \
    COLVO_CHECK_ARG(fill_shape(V, F, L), who ": bad shape: V = %d (1 .. 2^30 - 1), F = %d (1 .. 2^29 - 1), L = %d (1 .. V)", V, F, L)

extern "C" size_t colvo_mesh_fill_scratch_bytes(int V, int F, int L) {
    if (!fill_shape(V, F, L)) return 0;
    return fill_ws(nullptr, V, F, L).bytes;
}

extern "C" int colvo_mesh_fill_plan(const float* vertices, const int32_t* faces, const float* colors, int V, int F, int L, float unit,
                                    int max_edges, const int32_t* vertex_loop, const int64_t* loops, void* scratch,
                                    int32_t* status, int64_t* hole, int32_t* ring_offsets, int32_t* ring_vertices, int32_t* counts,
                                    colvo_stream_t stream) {
    FILL_CHECK_SHAPE("colvo_mesh_fill_plan");
    COLVO_CHECK_ARG(unit_ok(unit), "colvo_mesh_fill_plan: unit %g must be finite and positive", (double)unit);
    COLVO_CHECK_ARG(max_edges >= 3, "colvo_mesh_fill_plan: max_edges = %d must be 3 or more", max_edges);
    COLVO_CHECK_ARG(vertices && faces && vertex_loop && loops && scratch && status && hole && ring_offsets && ring_vertices && counts,
                    "colvo_mesh_fill_plan: null pointer argument");
    COLVO_CHECK_ARG(aligned16(scratch), "colvo_mesh_fill_plan: scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const FillWs w = fill_ws(scratch, V, F, L);
    const dim3 gv(blocks_of(V, NT)), gf(blocks_of(F, NT)), gs(blocks_of(3ll * F, NT)), gl(blocks_of(L + 1ll, NT));
    const int cap = 3 * F;
    const long long* lp = reinterpret_cast<const long long*>(loops);
    const char* who = "colvo_mesh_fill_plan";
    COLVO_CHECK_HIP(hipMemsetAsync(counts, 0, CT_COUNT * sizeof(int32_t), s), who);
    // start, cursor | out, in, succ | loop_sums .. ring_len are each consecutive in the scratch, padding included
    COLVO_CHECK_HIP(hipMemsetAsync(w.start, 0, (size_t)((char*)w.side_lo - (char*)w.start), s), who);
    COLVO_CHECK_HIP(hipMemsetAsync(w.out, 0, (size_t)((char*)w.pair_a - (char*)w.out), s), who);
    COLVO_CHECK_HIP(hipMemsetAsync(w.loop_sums, 0, (size_t)((char*)w.vertex_offsets - (char*)w.loop_sums), s), who);
    COLVO_CHECK_HIP(hipMemsetAsync(ring_vertices, 0, (size_t)V * 4, s), who);
    colvo::launch(k_fill_count, gf, dim3(NT), 0, s, faces, V, F, w.start);
    COLVO_CHECK_LAUNCH("k_fill_count");
    int rc = scan_exclusive(Scan{w.start, V, nullptr, w.sums, counts + CT_SIDES, nullptr, 0}, s);
    if (rc != 0) return rc;
    colvo::launch(k_fill_sides, gf, dim3(NT), 0, s, faces, V, F, w.start, w.cursor, cap, w.side_lo, w.side_key);
    COLVO_CHECK_LAUNCH("k_fill_sides");
    colvo::launch(k_fill_edges, gs, dim3(NT), 0, s, w.side_lo, w.side_key, w.start, w.cursor, vertex_loop, V, L, cap, w.out, w.in, w.succ,
                  w.loop_edges, counts);
    COLVO_CHECK_LAUNCH("k_fill_edges");
    colvo::launch(k_fill_vertices, gv, dim3(NT), 0, s, vertices, colors, vertex_loop, lp, w.out, w.in, V, L, unit, w.loop_sums,
                  w.loop_flags, counts);
    COLVO_CHECK_LAUNCH("k_fill_vertices");
    colvo::launch(k_fill_loops, gl, dim3(NT), 0, s, lp, vertex_loop, w.loop_sums, w.loop_edges, w.loop_flags, V, L, unit,
                  w.ring_len, ring_offsets, w.centre, w.centre_color, counts);
    COLVO_CHECK_LAUNCH("k_fill_loops");
    rc = scan_exclusive(Scan{ring_offsets, L + 1, nullptr, w.sums, counts + CT_R, nullptr, 0}, s);
    if (rc != 0) return rc;
    colvo::launch(k_rank_init, gv, dim3(NT), 0, s, vertex_loop, lp, w.ring_len, w.succ, V, L, w.pair_a, counts);
    COLVO_CHECK_LAUNCH("k_rank_init");
    // (a simple loop has at most min(V, 3 F) edges; the rounds beyond what the longest one needs leave at once)
    for (int round = 0, rounds = doubling_rounds((int)std::min<long long>(V, 3ll * F)); round < rounds; ++round) {
        colvo::launch(k_rank_round, gv, dim3(NT), 0, s, w.pair_a, w.pair_b, V, round, counts);
        COLVO_CHECK_LAUNCH("k_rank_round");
    }
    colvo::launch(k_rank_finish, gv, dim3(NT), 0, s, w.pair_a, w.pair_b, vertex_loop, lp, w.ring_len, ring_offsets, w.succ, V, L, ring_vertices, counts);
    COLVO_CHECK_LAUNCH("k_rank_finish");
    colvo::launch(k_fan_measure, gv, dim3(NT), 0, s, vertices, ring_vertices, ring_offsets, w.ring_len, vertex_loop, w.centre, V, L, unit,
                  w.loop_measures, w.loop_flags);
    COLVO_CHECK_LAUNCH("k_fan_measure");
    colvo::launch(k_fill_number, gl, dim3(NT), 0, s, w.ring_len, w.loop_flags, w.loop_measures, L, max_edges, status,
                  reinterpret_cast<long long*>(hole), w.vertex_offsets, w.face_offsets, w.centre_normal);
    COLVO_CHECK_LAUNCH("k_fill_number");
    rc = scan_exclusive(Scan{w.vertex_offsets, L + 1, nullptr, w.sums, counts + CT_NV, nullptr, 0}, s);
    if (rc != 0) return rc;
    return scan_exclusive(Scan{w.face_offsets, L + 1, nullptr, w.sums, counts + CT_NF, nullptr, 0}, s);
}

extern "C" int colvo_mesh_fill_write(const float* vertices, const float* colors, const float* normals, const int32_t* cells,
                                     const int32_t* faces, int V, int F, int L, int R, int n_new_vertices, int n_new_faces,
                                     const void* scratch, const int32_t* vertex_loop, const int32_t* status, const int32_t* ring_offsets,
                                     const int32_t* ring_vertices, float* out_vertices, float* out_colors, float* out_normals,
                                     int32_t* out_cells, int32_t* out_faces, int32_t* face_loop, int32_t* new_vertex_loop,
                                     colvo_stream_t stream) {
    FILL_CHECK_SHAPE("colvo_mesh_fill_write");
    COLVO_CHECK_ARG(R >= 0 && R <= V && n_new_vertices >= 0 && n_new_vertices <= L && n_new_faces >= 0 && n_new_faces <= R,
                    "colvo_mesh_fill_write: bad shape: R = %d (0 .. V = %d), new vertices = %d (0 .. L = %d), new faces = %d (0 .. R)", R, V,
                    n_new_vertices, L, n_new_faces);
    COLVO_CHECK_ARG(vertices && faces && scratch && vertex_loop && status && ring_offsets && ring_vertices && out_vertices && out_faces &&
                        face_loop && (n_new_vertices == 0 || new_vertex_loop) && (!colors == !out_colors) && (!normals == !out_normals) &&
                        (!cells == !out_cells),
                    "colvo_mesh_fill_write: null pointer argument (colors, normals and cells go with their outputs)");
    COLVO_CHECK_ARG(aligned16(scratch), "colvo_mesh_fill_write: scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const FillWs w = fill_ws(const_cast<void*>(scratch), V, F, L);
    const int32_t* src[5] = {reinterpret_cast<const int32_t*>(vertices), reinterpret_cast<const int32_t*>(colors),
                             reinterpret_cast<const int32_t*>(normals), cells, faces};
    int32_t* dst[5] = {reinterpret_cast<int32_t*>(out_vertices), reinterpret_cast<int32_t*>(out_colors),
                       reinterpret_cast<int32_t*>(out_normals), out_cells, out_faces};
    for (int k = 0; k < 5; ++k) {
        if (src[k] == nullptr) continue;
        const size_t n = 3 * (size_t)(k == 4 ? F : V);
        colvo::launch(k_copy_words, dim3(blocks_of((long long)n, NT)), dim3(NT), 0, s, src[k], n, dst[k]);
        COLVO_CHECK_LAUNCH("k_copy_words");
    }
    COLVO_CHECK_HIP(hipMemsetAsync(face_loop, 0xff, (size_t)F * 4, s), "colvo_mesh_fill_write");
    if (n_new_vertices > 0) {
        colvo::launch(k_fill_new_vertices, dim3(blocks_of(L, NT)), dim3(NT), 0, s, status, w.ring_len, w.vertex_offsets, w.centre,
                      w.centre_color, w.centre_normal, V, L, n_new_vertices, out_vertices, out_colors, out_normals, out_cells,
                      new_vertex_loop);
        COLVO_CHECK_LAUNCH("k_fill_new_vertices");
    }
    if (n_new_faces > 0) {
        colvo::launch(k_fill_new_faces, dim3(blocks_of(R, NT)), dim3(NT), 0, s, status, ring_vertices, ring_offsets, w.ring_len,
                      vertex_loop, w.vertex_offsets, w.face_offsets, V, F, L, R, n_new_vertices, n_new_faces, out_faces, face_loop);
        COLVO_CHECK_LAUNCH("k_fill_new_faces");
    }
    return 0;
}
