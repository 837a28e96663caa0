// surface.hip -- exact truncated point-to-surface distances: for every query point the squared distance to the nearest
// point OF THE TRIANGLES of a mesh within max_dist, which face that is, where on it the nearest point lies and on which side of it the
// query lies, and exact integer statistics over the queries.  Contract: include/colvo.h (colvo_surface_*); NumPy replica
// tests/surface_ref.py, which has no grid.  The sibling of cloud.hip: the same header, cell coordinate and margin (cloud_grid.h).
//
//   plan    k_surface_bounds: bounding box of the vertices of the live, finite faces (integer max on ordered float keys), and the counts
//           of dead and skipped faces.  k_surface_grid: one thread, cloud_grid::make_grid.  k_surface_count: one thread per face; a face
//           whose box of cells [c(min) .. c(max)] spans more than `surface_span_limit` cells on an axis goes onto the oversize list, any
//           other adds one to the count of every cell of its box.  The ordered scan of csrc/scan.hip turns the counts into starts.  The
//           pair total is a 64-bit sum of its own: the caller reads it back once and sizes the records with it.
//   fill    k_surface_fill: the same boxes again; a face's record goes to start[cell] + cursor[cell]++ for every cell of its box.  The
//           order inside a cell follows the atomics; no output depends on it.  A record is the face's index (4 bytes; the query
//           gathers through faces and vertices) or, with the tuning entry surface_copy_records, its nine coordinates and its index
//           (48 bytes, read as three 16-byte words): the plan says which, the caller passes it on.
//   query   k_surface_query: one lane per query; the 9 x-runs of up to 3 cells around the query's cell are contiguous in the records;
//           then the oversize list, whole.  The least (d2, face) stays in registers with its point and side.  A face that lies in
//           several of the cells is evaluated again to the same bits and cannot replace itself.  Statistics: cloud.hip's striped lines.
//
// Every loop has a bound known on entry, no thread waits on another's store, and every cell, record, face and vertex index is clamped
// or checked before it is used as an address, whatever the header, the records and the faces hold.  The arithmetic that decides a
// distance is float64 on coordinates widened from float32, every operation individually rounded in the order colvo.h writes --
// contraction is off for this whole file; division and square root are the correctly rounded ones.
#include "scene.h"
#include "tuning.h"

#pragma clang fp contract(off)

#include "cloud_grid.h"

namespace colvo {
namespace {

using namespace cloud_grid;

constexpr int NT = 256;
constexpr int N_QUERY_STATS = 15;          // the words the query counts; the build's four follow them in the stats block
constexpr int N_STATS = 19;
constexpr int MAX_THRESHOLDS = 8;
constexpr int BOUNDS_MAX_BLOCKS = 1024;
constexpr int MAX_F = 1 << 29;
constexpr long long MAX_PAIRS = 1ll << 30;
constexpr int REC_INDEX = 4, REC_COPY = 48;     // bytes of a record in the two forms
static_assert(N_QUERY_STATS <= COUNTER_PITCH, "a counter line holds the query's words");

struct SurfHeader {                        // the head of the workspace
    Header g;                              // the grid, as a cloud's
    unsigned long long pairs;              // (cell, face) pairs of the faces entered through the grid
    uint32_t n_over;                       // faces on the oversize list
    uint32_t dead, skipped;
    uint32_t span;                         // the span limit the plan was made with: the fill reads it here
    uint32_t pad_[10];
};
static_assert(sizeof(SurfHeader) == 128, "SurfHeader is 128 B");

struct Thresholds {
    double t2[MAX_THRESHOLDS];             // double(float32(tau))^2: exact
    int n;
};

enum { FACE_OK = 0, FACE_DEAD = 1, FACE_SKIPPED = 2 };

// the nine coordinates of face f, or why it takes no part: dead as in topology.hip (an index outside [0, V) or a repeated index), skipped
// where a coordinate of a live face is not finite.  f in [0, F).
__device__ __forceinline__ int load_face(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int f, int V, float (&p)[9]) {
    int v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = faces[(size_t)f * 3 + k];
    const bool in = (unsigned)v[0] < (unsigned)V && (unsigned)v[1] < (unsigned)V && (unsigned)v[2] < (unsigned)V;
    if (!(in && v[0] != v[1] && v[1] != v[2] && v[0] != v[2])) return FACE_DEAD;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[k * 3 + a] = vertices[(size_t)v[k] * 3 + a];
            fin = fin && finite_f(p[k * 3 + a]);
        }
    }
    return fin ? FACE_OK : FACE_SKIPPED;
}

// cell coordinate of one axis, clamped into the grid (the clamp never acts on a vertex of the box the grid was made from; it turns the
// NaN of an unbounded box into 0)
__device__ __forceinline__ int axis_cell(const Grid& G, int a, float x) {
    return (int)fminf(fmaxf(floorf(grid_coord(G, a, x)), 0.0f), (float)(G.n[a] - 1));
}

// the box of cells of a face's own axis-aligned bounds; true iff it spans more than `span` cells on some axis
__device__ __forceinline__ bool face_box(const Grid& G, const float (&p)[9], int span, int (&lo)[3], int (&hi)[3]) {
    bool over = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = axis_cell(G, a, fminf(fminf(p[a], p[3 + a]), p[6 + a]));
        hi[a] = axis_cell(G, a, fmaxf(fmaxf(p[a], p[3 + a]), p[6 + a]));
        over = over || hi[a] - lo[a] + 1 > span;
    }
    return over;
}

__device__ __forceinline__ int span_of(const SurfHeader* __restrict__ h) {
    return min(max(__builtin_amdgcn_readfirstlane((int)h->span), 1), AXIS_LIMIT);
}

// ---- plan -------------------------------------------------------------------------------------------------------------------------- //
// grid min(ceil(F / NT), BOUNDS_MAX_BLOCKS), grid-stride: six integer maxima and three counts per workgroup
__global__ __launch_bounds__(NT) void k_surface_bounds(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int V, int F,
                                                       SurfHeader* __restrict__ h) {
    __shared__ uint32_t sm[NT / 64][9];
    uint32_t k[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t n[3] = {0u, 0u, 0u};
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < F; i += (long long)gridDim.x * NT) {
        float p[9];
        const int kind = load_face(vertices, faces, (int)i, V, p);
        n[0] += (uint32_t)(kind == FACE_OK);
        n[1] += (uint32_t)(kind == FACE_DEAD);
        n[2] += (uint32_t)(kind == FACE_SKIPPED);
        if (kind != FACE_OK) continue;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const uint32_t q = float_key(p[j]);
            k[j % 3] = max(k[j % 3], ~q);
            k[3 + j % 3] = max(k[3 + j % 3], q);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int j = 0; j < 6; ++j) k[j] = max(k[j], (uint32_t)__shfl_xor((int)k[j], off));
#pragma unroll
        for (int j = 0; j < 3; ++j) n[j] += (uint32_t)__shfl_xor((int)n[j], off);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 6; ++j) sm[threadIdx.x >> 6][j] = k[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) sm[threadIdx.x >> 6][6 + j] = n[j];
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const int j = threadIdx.x;
        if (j < 6) {
            const uint32_t v = max(max(sm[0][j], sm[1][j]), max(sm[2][j], sm[3][j]));
            if ((sm[0][6] + sm[1][6]) + (sm[2][6] + sm[3][6]) != 0u) atomicMax(&h->g.key[j], v);
        } else {
            const uint32_t v = (sm[0][j] + sm[1][j]) + (sm[2][j] + sm[3][j]);
            uint32_t* dst = j == 6 ? &h->g.n_valid : j == 7 ? &h->dead : &h->skipped;
            if (v) atomicAdd(dst, v);
        }
    }
}

__global__ void k_surface_grid(SurfHeader* __restrict__ h, float max_dist, int span) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    h->span = (uint32_t)span;
    make_grid(&h->g, max_dist);
}

// one thread per face: oversize list, or count[cell] += 1 over its box
__global__ __launch_bounds__(NT) void k_surface_count(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int V, int F,
                                                      SurfHeader* __restrict__ h, int32_t* __restrict__ count, int32_t* __restrict__ over) {
    const Grid G = load_grid(&h->g);
    const int span = span_of(h);
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    float p[9];
    unsigned long long pairs = 0ull;
    if (i < F && G.cells > 0 && load_face(vertices, faces, (int)i, V, p) == FACE_OK) {
        int lo[3], hi[3];
        if (face_box(G, p, span, lo, hi)) {
            const uint32_t slot = atomicAdd(&h->n_over, 1u);
            if (slot < (uint32_t)F) over[slot] = (int)i;
        } else {
            for (int z = lo[2]; z <= hi[2]; ++z)
                for (int y = lo[1]; y <= hi[1]; ++y)
                    for (int x = lo[0]; x <= hi[0]; ++x) atomicAdd(&count[(z * G.n[1] + y) * G.n[0] + x], 1);       // < cells
            pairs = (unsigned long long)(hi[0] - lo[0] + 1) * (unsigned long long)((hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1));
        }
    }
    const unsigned long long total = wave_sum(pairs);
    if ((threadIdx.x & 63) == 0 && total) atomicAdd(&h->pairs, total);
}

// one thread: what the caller reads back
__global__ void k_surface_counts(const SurfHeader* __restrict__ h, int F, int record_bytes, long long* __restrict__ counts) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    counts[4] = record_bytes;
    counts[5] = counts[6] = counts[7] = 0;
    counts[0] = (long long)h->pairs;
    counts[1] = (long long)min(h->n_over, (uint32_t)F);
    counts[2] = (long long)h->dead;
    counts[3] = (long long)h->skipped;
}

// ---- fill -------------------------------------------------------------------------------------------------------------------------- //
template <bool COPY>
__global__ __launch_bounds__(NT) void k_surface_fill(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int V, int F,
                                                     const SurfHeader* __restrict__ h, const int32_t* __restrict__ start,
                                                     int32_t* __restrict__ cursor, int pairs, void* __restrict__ records) {
    const Grid G = load_grid(&h->g);
    const int span = span_of(h);
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    float p[9];
    if (i >= F || G.cells <= 0 || load_face(vertices, faces, (int)i, V, p) != FACE_OK) return;
    int lo[3], hi[3];
    if (face_box(G, p, span, lo, hi)) return;
    for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y)
            for (int x = lo[0]; x <= hi[0]; ++x) {
                const int cell = (z * G.n[1] + y) * G.n[0] + x;
                const long long pos = (long long)start[cell] + atomicAdd(&cursor[cell], 1);
                if (pos < 0 || pos >= pairs) continue;                         // (never, for the counts of this plan)
                if (COPY) {
                    float4* r = static_cast<float4*>(records) + pos * 3;
                    r[0] = make_float4(p[0], p[1], p[2], p[3]);
                    r[1] = make_float4(p[4], p[5], p[6], p[7]);
                    r[2] = make_float4(p[8], __int_as_float((int)i), 0.0f, 0.0f);
                } else {
                    static_cast<int32_t*>(records)[pos] = (int)i;
                }
            }
}

// ---- query ------------------------------------------------------------------------------------------------------------------------- //
struct Best {
    double d2;
    double c[3];
    int face, side, plane;
};

// the closest point of segment (u, u + e) to p: a candidate that replaces the running one only when strictly nearer
__device__ __forceinline__ void segment(const double (&p)[3], const double (&u)[3], const double (&w)[3], const double (&e)[3],
                                        double& d2, double (&c)[3], bool& plane) {
    const double ee = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    const double we = (w[0] * e[0] + w[1] * e[1]) + w[2] * e[2];
    double t = 0.0;
    if (ee > 0.0) t = fmin(fmax(we / ee, 0.0), 1.0);
    double q[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        q[a] = u[a] + t * e[a];
        d[a] = p[a] - q[a];
    }
    const double s2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    if (s2 < d2) {
        d2 = s2;
        plane = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = q[a];
    }
}

// n . (e x w)
__device__ __forceinline__ double edge_test(const double (&n)[3], const double (&e)[3], const double (&w)[3]) {
    const double cx = e[1] * w[2] - e[2] * w[1], cy = e[2] * w[0] - e[0] * w[2], cz = e[0] * w[1] - e[1] * w[0];
    return (n[0] * cx + n[1] * cy) + n[2] * cz;
}

// face f, given by its nine coordinates, against p
__device__ __forceinline__ void evaluate(const double (&p)[3], int f, const float (&r)[9], double md2, Best& B) {
    double a[3], ab[3], bc[3], ca[3], ac[3], pa[3], pb[3], pc[3], b[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = (double)r[k];
        b[k] = (double)r[3 + k];
        c[k] = (double)r[6 + k];
        ab[k] = b[k] - a[k];
        ac[k] = c[k] - a[k];
        bc[k] = c[k] - b[k];
        ca[k] = a[k] - c[k];
        pa[k] = p[k] - a[k];
        pb[k] = p[k] - b[k];
        pc[k] = p[k] - c[k];
    }
    const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
    const double s = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    const double h = (n[0] * pa[0] + n[1] * pa[1]) + n[2] * pa[2];
    const bool area = s > 0.0 && s < (double)__builtin_inff();
    double d2 = (double)__builtin_inff();
    double q[3] = {0.0, 0.0, 0.0};
    bool plane = false;
    if (area && edge_test(n, ab, pa) >= 0.0 && edge_test(n, bc, pb) >= 0.0 && edge_test(n, ca, pc) >= 0.0) {
        const double k = h / s;
        d2 = (h * h) / s;
        plane = true;
#pragma unroll
        for (int j = 0; j < 3; ++j) q[j] = p[j] - n[j] * k;
    }
    segment(p, a, pa, ab, d2, q, plane);
    segment(p, b, pb, bc, d2, q, plane);
    segment(p, c, pc, ca, d2, q, plane);
    if (d2 < md2 && (d2 < B.d2 || (d2 == B.d2 && f < B.face))) {
        B.d2 = d2;
        B.face = f;
        B.plane = (int)plane;
        B.side = area ? (int)(h > 0.0) - (int)(h < 0.0) : 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) B.c[j] = q[j];
    }
}

// face f against p through faces and vertices; f may be anything: it is checked against F, its indices against V
__device__ __forceinline__ void consider(const double (&p)[3], int f, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                         int V, int F, double md2, Best& B) {
    if ((unsigned)f >= (unsigned)F) return;
    float r[9];
    if (load_face(vertices, faces, f, V, r) != FACE_OK) return;
    evaluate(p, f, r, md2, B);
}

// record j of the copied form: whatever it holds, it is arithmetic and a face number in the output, never an address
__device__ __forceinline__ void consider_record(const double (&p)[3], const float4* __restrict__ rec, int j, double md2, Best& B) {
    const float4 r0 = rec[(size_t)j * 3], r1 = rec[(size_t)j * 3 + 1], r2 = rec[(size_t)j * 3 + 2];
    const float r[9] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x};
    evaluate(p, __float_as_int(r2.y), r, md2, B);
}

// grid ceil(N / NT), one lane per query
template <bool COPY>
__global__ __launch_bounds__(NT) void k_surface_query(const float* __restrict__ Q, int N, const float* __restrict__ vertices,
                                                      const int32_t* __restrict__ faces, int V, int F, const SurfHeader* __restrict__ h,
                                                      const int32_t* __restrict__ start, const void* __restrict__ rec, int pairs,
                                                      const int32_t* __restrict__ over, float md, double md2, float scale, Thresholds thr,
                                                      double* __restrict__ dist2, float* __restrict__ dist, int32_t* __restrict__ face,
                                                      float* __restrict__ closest, int8_t* __restrict__ side,
                                                      unsigned long long* __restrict__ counters) {
    __shared__ unsigned long long sm[NT / 64][N_QUERY_STATS];
    const Grid G = load_grid(&h->g);
    const int n_over = min(__builtin_amdgcn_readfirstlane((int)min(h->n_over, (uint32_t)MAX_F)), F);
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    const bool in = i < N;
    float q[3] = {0.0f, 0.0f, 0.0f};
    if (in) {
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = Q[i * 3 + a];
    }
    const bool valid = in && finite_f(q[0]) && finite_f(q[1]) && finite_f(q[2]);
    const double p[3] = {(double)q[0], (double)q[1], (double)q[2]};
    Best B;
    B.d2 = md2;
    B.face = 0x7fffffff;
    B.side = 0;
    B.plane = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) B.c[a] = valid ? p[a] : 0.0;
    unsigned long long examined = 0ull;
    bool walk = valid && G.cells > 0;
    int c[3] = {0, 0, 0};
    if (walk && !G.single) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float g = grid_coord(G, a, q[a]);
            // more than a cell outside the box: nothing of the grid within reach (and no integer is made of a coordinate out of range)
            walk = walk && g >= -1.0f && g < (float)G.n[a] + 1.0f;
            c[a] = walk ? (int)floorf(g) : 0;                   // -1 .. n
        }
    }
    if (walk) {
        const int x0 = max(c[0] - 1, 0), x1 = min(c[0] + 1, G.n[0] - 1);
        const int y0 = max(c[1] - 1, 0), y1 = min(c[1] + 1, G.n[1] - 1);
        const int z0 = max(c[2] - 1, 0), z1 = min(c[2] + 1, G.n[2] - 1);
        if (x0 <= x1) {
            for (int z = z0; z <= z1; ++z) {
                for (int y = y0; y <= y1; ++y) {
                    const int base = (z * G.n[1] + y) * G.n[0];          // < cells <= MAX_CELLS
                    const int b = max(start[base + x0], 0), e = min(start[base + x1 + 1], pairs);
                    for (int j = b; j < e; ++j) {
                        if (COPY) consider_record(p, static_cast<const float4*>(rec), j, md2, B);
                        else consider(p, static_cast<const int32_t*>(rec)[j], vertices, faces, V, F, md2, B);
                    }
                    if (e > b) examined += (unsigned long long)(e - b);
                }
            }
        }
    }
    if (valid) {
        for (int j = 0; j < n_over; ++j) consider(p, over[j], vertices, faces, V, F, md2, B);
        examined += (unsigned long long)n_over;
    }
    const bool reached = B.face != 0x7fffffff;
    const float dv = reached ? (float)sqrt(B.d2) : md;          // sqrt(md2) is max_dist itself: md2 is its exact square
    if (in) {
        dist2[i] = B.d2;
        dist[i] = dv;
        face[i] = reached ? B.face : -1;
        side[i] = (int8_t)B.side;
#pragma unroll
        for (int a = 0; a < 3; ++a) closest[i * 3 + a] = (float)B.c[a];
    }
    // statistics: per wave, per workgroup, then one add per word into this workgroup's counter line
    unsigned long long st[N_QUERY_STATS];
    st[0] = (unsigned long long)__popcll(__ballot(valid));
    st[1] = (unsigned long long)__popcll(__ballot(valid && reached));
#pragma unroll
    for (int k = 0; k < MAX_THRESHOLDS; ++k) st[2 + k] = (unsigned long long)__popcll(__ballot(valid && k < thr.n && B.d2 < thr.t2[k]));
    st[10] = wave_sum(valid ? (unsigned long long)(uint32_t)rintf(dv * scale) : 0ull);
    st[11] = wave_sum(examined);
    st[12] = (unsigned long long)__popcll(__ballot(valid && B.side > 0));
    st[13] = (unsigned long long)__popcll(__ballot(valid && B.side < 0));
    st[14] = (unsigned long long)__popcll(__ballot(valid && reached && B.plane != 0));
    striped_counter_add(st, sm, counters + (size_t)(blockIdx.x % COUNTER_LINES) * COUNTER_PITCH);
}

// one workgroup: stats[k] = sum over the counter lines; the build's four words behind them
__global__ void k_surface_stats(const unsigned long long* __restrict__ counters, const SurfHeader* __restrict__ h, int F,
                                unsigned long long* __restrict__ stats) {
    const int k = threadIdx.x;
    if (k >= N_STATS) return;
    unsigned long long s = 0ull;
    if (k < N_QUERY_STATS) {
        for (int l = 0; l < COUNTER_LINES; ++l) s += counters[(size_t)l * COUNTER_PITCH + k];
    } else {
        s = k == 15 ? h->dead : k == 16 ? h->skipped : k == 17 ? h->pairs : (unsigned long long)min(h->n_over, (uint32_t)F);
    }
    stats[k] = s;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------- //
struct SurfWs {                            // header, counter lines, cell starts, chunk sums, cursors, the oversize list [F]
    SurfHeader* header;
    unsigned long long* counters;
    int32_t* cells;
    int32_t* sums;
    int32_t* cursor;
    int32_t* over;
    size_t bytes;
};

SurfWs surf_ws(void* base, int F) {
    Carver c(base);
    SurfWs w;
    w.header = c.take<SurfHeader>(1, 256);
    w.counters = c.take<unsigned long long>((size_t)COUNTER_LINES * COUNTER_PITCH);
    w.cells = c.take<int32_t>(SCAN_ENTRIES);
    w.sums = c.take<int32_t>(scan_chunks(SCAN_ENTRIES));
    w.cursor = c.take<int32_t>(MAX_CELLS);
    w.over = c.take<int32_t>((size_t)F);
    w.bytes = c.bytes();
    return w;
}

inline bool surf_shape(int V, int F) { return V >= 0 && F >= 0 && F < MAX_F; }

}  // namespace
}  // namespace colvo

using namespace colvo;
using namespace colvo::cloud_grid;

#define SURF_CHECK_SHAPE(who) COLVO_CHECK_ARG(surf_shape(V, F), who ": bad shape: V = %d (0 .. 2^31 - 1), F = %d (0 .. 2^29 - 1)", V, F)
#define SURF_CHECK_MAX_DIST(who)                         \
    float md2f, scale;                                   \
    COLVO_CHECK_ARG(good_max_dist(max_dist, md2f, scale), \
                    who ": bad max_dist %g (finite, positive, with a finite positive float32 square)", (double)max_dist)

extern "C" size_t colvo_surface_scratch_bytes(int V, int F) {
    if (!surf_shape(V, F)) return 0;
    return surf_ws(nullptr, F).bytes;
}

extern "C" int colvo_surface_index_plan(const float* vertices, const int32_t* faces, int V, int F, float max_dist, void* scratch,
                                        int64_t* counts, colvo_stream_t stream) {
    SURF_CHECK_SHAPE("colvo_surface_index_plan");
    COLVO_CHECK_ARG(scratch && counts && (F == 0 || (faces && (vertices || V == 0))), "colvo_surface_index_plan: null pointer argument");
    SURF_CHECK_MAX_DIST("colvo_surface_index_plan");
    COLVO_CHECK_ARG(aligned16(scratch), "colvo_surface_index_plan: scratch must be 16-byte aligned");
    long span = TUNE(surface_span_limit);
    span = span < 1 ? 1 : span > AXIS_LIMIT ? AXIS_LIMIT : span;
    hipStream_t s = (hipStream_t)stream;
    const SurfWs w = surf_ws(scratch, F);
    COLVO_CHECK_HIP(hipMemsetAsync(w.header, 0, sizeof(SurfHeader), s), "colvo_surface_index_plan");
    if (F > 0) {                                                 // (F = 0: cells = 0, the query walks nothing)
        COLVO_CHECK_HIP(hipMemsetAsync(w.cells, 0, (size_t)SCAN_ENTRIES * 4, s), "colvo_surface_index_plan");
        const int nb = blocks_of(F, NT);
        colvo::launch(k_surface_bounds, dim3(nb < BOUNDS_MAX_BLOCKS ? nb : BOUNDS_MAX_BLOCKS), dim3(NT), 0, s, vertices, faces, V, F, w.header);
        COLVO_CHECK_LAUNCH("k_surface_bounds");
        colvo::launch(k_surface_grid, dim3(1), dim3(64), 0, s, w.header, max_dist, (int)span);
        COLVO_CHECK_LAUNCH("k_surface_grid");
        colvo::launch(k_surface_count, dim3(nb), dim3(NT), 0, s, vertices, faces, V, F, w.header, w.cells, w.over);
        COLVO_CHECK_LAUNCH("k_surface_count");
        if (int rc = scan_exclusive(Scan{w.cells, SCAN_ENTRIES, &w.header->g.cells, w.sums, nullptr, nullptr, 0}, s)) return rc;
    }
    colvo::launch(k_surface_counts, dim3(1), dim3(64), 0, s, (const SurfHeader*)w.header, F,
                  TUNE(surface_copy_records) != 0 ? REC_COPY : REC_INDEX, reinterpret_cast<long long*>(counts));
    COLVO_CHECK_LAUNCH("k_surface_counts");
    return 0;
}

#define SURF_CHECK_RECORDS(who)                                                                                                  \
    COLVO_CHECK_ARG(pairs >= 0 && pairs < MAX_PAIRS, who ": %lld (cell, face) pairs: the index holds fewer than 2^30", (long long)pairs); \
    COLVO_CHECK_ARG(record_bytes == REC_INDEX || record_bytes == REC_COPY, who ": bad record_bytes %d (%d: face index, %d: copied face)", \
                    record_bytes, REC_INDEX, REC_COPY)

extern "C" int colvo_surface_index_fill(const float* vertices, const int32_t* faces, int V, int F, void* scratch, int64_t pairs,
                                        int record_bytes, void* records, colvo_stream_t stream) {
    SURF_CHECK_SHAPE("colvo_surface_index_fill");
    SURF_CHECK_RECORDS("colvo_surface_index_fill");
    COLVO_CHECK_ARG(scratch && (pairs == 0 || (records && faces && vertices)), "colvo_surface_index_fill: null pointer argument");
    COLVO_CHECK_ARG(aligned16(scratch) && aligned16(records), "colvo_surface_index_fill: scratch and records must be 16-byte aligned");
    if (pairs == 0 || F == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const SurfWs w = surf_ws(scratch, F);
    COLVO_CHECK_HIP(hipMemsetAsync(w.cursor, 0, (size_t)MAX_CELLS * 4, s), "colvo_surface_index_fill");
    colvo::launch(record_bytes == REC_COPY ? k_surface_fill<true> : k_surface_fill<false>, dim3(blocks_of(F, NT)), dim3(NT), 0, s, vertices,
                  faces, V, F, (const SurfHeader*)w.header, (const int32_t*)w.cells, w.cursor, (int)pairs, records);
    COLVO_CHECK_LAUNCH("k_surface_fill");
    return 0;
}

extern "C" int colvo_surface_query(const float* query, int N, const float* vertices, const int32_t* faces, int V, int F, float max_dist,
                                   const float* thresholds, int n_thresholds, void* scratch, const void* records, int64_t pairs,
                                   int record_bytes, double* dist2, float* dist, int32_t* face, float* closest, int8_t* side, uint64_t* stats,
                                   colvo_stream_t stream) {
    SURF_CHECK_SHAPE("colvo_surface_query");
    COLVO_CHECK_ARG(N >= 0 && N < MAX_POINTS, "colvo_surface_query: bad shape: N = %d (0 .. 2^30 - 1)", N);
    SURF_CHECK_RECORDS("colvo_surface_query");
    COLVO_CHECK_ARG(scratch && stats && ((query && dist2 && dist && face && closest && side) || N == 0) &&
                        (F == 0 || (faces && (vertices || V == 0))) && (records || pairs == 0) && (thresholds || n_thresholds == 0),
                    "colvo_surface_query: null pointer argument");
    SURF_CHECK_MAX_DIST("colvo_surface_query");
    COLVO_CHECK_ARG(n_thresholds >= 0 && n_thresholds <= MAX_THRESHOLDS, "colvo_surface_query: bad thresholds: %d of them (0 .. %d)",
                    n_thresholds, MAX_THRESHOLDS);
    Thresholds thr;
    thr.n = n_thresholds;
    for (int k = 0; k < MAX_THRESHOLDS; ++k) {
        thr.t2[k] = 0.0;
        if (k >= n_thresholds) continue;
        const float t = thresholds[k];
        COLVO_CHECK_ARG(t > 0.0f && t <= max_dist && (k == 0 || t >= thresholds[k - 1]),
                        "colvo_surface_query: bad thresholds: tau[%d] = %g (positive, non-descending, <= max_dist %g)", k, (double)t,
                        (double)max_dist);
        thr.t2[k] = (double)t * (double)t;
    }
    COLVO_CHECK_ARG(aligned16(scratch) && aligned16(records), "colvo_surface_query: scratch and records must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const SurfWs w = surf_ws(scratch, F);
    COLVO_CHECK_HIP(hipMemsetAsync(w.counters, 0, (size_t)COUNTER_LINES * COUNTER_PITCH * 8, s), "colvo_surface_query");
    if (N > 0) {
        colvo::launch(record_bytes == REC_COPY ? k_surface_query<true> : k_surface_query<false>, dim3(blocks_of(N, NT)), dim3(NT), 0, s, query, N, vertices, faces, V, F, (const SurfHeader*)w.header,
                      (const int32_t*)w.cells, records, (int)pairs, (const int32_t*)w.over, max_dist, (double)max_dist * (double)max_dist,
                      scale, thr, dist2, dist, face, closest, side, w.counters);
        COLVO_CHECK_LAUNCH("k_surface_query");
    }
    colvo::launch(k_surface_stats, dim3(1), dim3(64), 0, s, (const unsigned long long*)w.counters, (const SurfHeader*)w.header, F,
                  reinterpret_cast<unsigned long long*>(stats));
    COLVO_CHECK_LAUNCH("k_surface_stats");
    return 0;
}
