// cloud_grid.h -- the index of a reference cloud and the walk of a query through it, shared by cloud.hip, which builds
// the index and answers plain queries, and register.hip, which walks it once per source point and iteration: both find the nearest
// point with the very same routine.  `nearest_key` below is PINNED -- float32, every operation individually rounded, in the order
// written -- against tests/cloud_ref.py.  A file that includes this header must have contraction off (`#pragma clang fp contract(off)`
// in front of the include); the pragma below repeats it, and since a file-scope pragma holds to the end of the translation unit,
// everything behind the include is compiled without contraction as well.
#pragma once
#include <float.h>

#include "scene.h"

#pragma clang fp contract(off)

namespace colvo {
namespace cloud_grid {

constexpr int AXIS_LIMIT = 128;                          // cells per axis, at most
constexpr float AXIS_DIV = 126.0f;                       // edge >= extent / AXIS_DIV: floor(126 * (1 + 3 * 2^-24)) + 1 <= 128
constexpr int MAX_CELLS = AXIS_LIMIT * AXIS_LIMIT * AXIS_LIMIT;
constexpr float EDGE_MARGIN = 1.0f + 1.0f / 1024.0f;     // edge >= max_dist * (1 + 2^-10): DESIGN.md §3.6h
constexpr int SCAN_ENTRIES = MAX_CELLS + 1;              // the cells and one entry behind them: its prefix is the record count
constexpr int COUNTER_LINES = 256;                       // the query's statistics: this many rows of N_STATS 64-bit words,
constexpr int COUNTER_PITCH = 16;                        // ... 128 bytes apart (one hot address measured 41 x slower: §3.6c (c))
constexpr int MAX_POINTS = 1 << 30;

struct Header {                            // the head of the workspace: written by the build, read by the query
    uint32_t key[6];                       // ordered keys: ~min x, y, z and max x, y, z (all of them gathered with atomicMax)
    uint32_t n_valid;                      // valid reference points
    uint32_t single;                       // the box has no finite grid: one cell, searched whole
    float o[3];                            // the box's lower corner
    float inv;                             // float32(1) / edge
    int n[3];                              // cells per axis
    int cells;                             // 0: no valid reference point
};
static_assert(sizeof(Header) == 64, "Header is 64 B");

struct Grid {                              // the header's geometry, wave-uniform
    float o[3], inv;
    int n[3], cells;
    bool single;
};

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ Grid load_grid(const Header* __restrict__ h) {
    Grid G;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        G.o[a] = uniform_f(h->o[a]);
        G.n[a] = __builtin_amdgcn_readfirstlane(h->n[a]);
    }
    G.inv = uniform_f(h->inv);
    G.cells = __builtin_amdgcn_readfirstlane(h->cells);
    G.single = __builtin_amdgcn_readfirstlane((int)h->single) != 0;
    // whatever the header holds, no index below leaves the cell arrays
    G.cells = min(max(G.cells, 0), MAX_CELLS);
#pragma unroll
    for (int a = 0; a < 3; ++a) G.n[a] = min(max(G.n[a], 1), AXIS_LIMIT);
    if ((long long)G.n[0] * G.n[1] * G.n[2] > (long long)G.cells) G.cells = 0;
    return G;
}

// One thread: the box of the header's keys -> origin, cell edge and dims, for the cloud's index and the surface's (csrc/surface.hip)
// alike.  edge = max(max_dist * EDGE_MARGIN, extent / AXIS_DIV), float32, every operation rounded once.
__device__ __forceinline__ void make_grid(Header* __restrict__ h, float max_dist) {
    if (h->n_valid == 0u) return;                                // the header was cleared: cells = 0
    float lo[3], hi[3], ext = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = float_key_inv(~h->key[a]);
        hi[a] = float_key_inv(h->key[3 + a]);
        ext = fmaxf(ext, hi[a] - lo[a]);
    }
    const float edge = fmaxf(max_dist * EDGE_MARGIN, __fdiv_rn(ext, AXIS_DIV));
    const float inv = __fdiv_rn(1.0f, edge);
    const bool single = !(finite_f(ext) && finite_f(edge) && finite_f(inv) && inv > 0.0f);
    int cells = 1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        h->o[a] = lo[a];
        int n = 1;
        if (!single) n = (int)fminf(fmaxf(floorf((hi[a] - lo[a]) * inv), 0.0f), (float)(AXIS_LIMIT - 1)) + 1;
        h->n[a] = n;
        cells *= n;
    }
    h->inv = single ? 0.0f : inv;
    h->single = single ? 1u : 0u;
    h->cells = cells;
}

// The pinned cell coordinate of one axis: ((x - o) * inv), floored by the callers.
__device__ __forceinline__ float grid_coord(const Grid& G, int a, float x) { return (x - G.o[a]) * G.inv; }

// The nearest valid reference point within reach of q: the minimum of the 64-bit keys (bits(d2) << 32) | original index over the
// records of the 9 x-runs of up to 3 cells around q's cell, d2 = ((dx*dx + dy*dy) + dz*dz) < md2 (strict); nothing within reach, or q
// not valid: (bits(md2) << 32) | 0xffffffff.  `examined` grows by the records looked at.  start [cells + 1] and rec [M] are the
// build's; every cell index is below G.cells and every record index is clamped to [0, M): whatever the header and the starts hold, no
// address leaves the two arrays.
__device__ __forceinline__ unsigned long long nearest_key(const Grid& G, const float (&q)[3], bool valid,
                                                          const int32_t* __restrict__ start, const float4* __restrict__ rec, int M,
                                                          float md2, unsigned long long& examined) {
    unsigned long long best = ((unsigned long long)__float_as_uint(md2) << 32) | 0xffffffffull;
    bool walk = valid && G.cells > 0;
    int c[3] = {0, 0, 0};
    if (walk && !G.single) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float g = grid_coord(G, a, q[a]);
            // more than a cell outside the box: nothing within reach (and no integer is made of a coordinate out of range)
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
                    const int b = max(start[base + x0], 0), e = min(start[base + x1 + 1], M);
                    for (int j = b; j < e; ++j) {
                        const float4 r = rec[j];
                        const float dx = q[0] - r.x, dy = q[1] - r.y, dz = q[2] - r.z;
                        const float d2 = ((dx * dx + dy * dy) + dz * dz);
                        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)__float_as_int(r.w);
                        if (d2 < md2 && key < best) best = key;
                    }
                    if (e > b) examined += (unsigned long long)(e - b);
                }
            }
        }
    }
    return best;
}

// ---- host side: the workspace of an index, and what both files refuse ------------------------------------------------------------ //
struct Ws {                                // header, counter lines, cell starts, chunk sums, records [M], ranks [M]
    Header* header;
    unsigned long long* counters;
    int32_t* cells;
    int32_t* sums;
    float4* rec;
    int32_t* rank;
    size_t bytes;
};

inline Ws layout(void* base, int M) {
    Carver c(base);
    Ws w;
    w.header = c.take<Header>(1, 256);
    w.counters = c.take<unsigned long long>((size_t)COUNTER_LINES * COUNTER_PITCH);
    w.cells = c.take<int32_t>(SCAN_ENTRIES);
    w.sums = c.take<int32_t>(scan_chunks(SCAN_ENTRIES));
    w.rec = c.take<float4>(M);
    w.rank = c.take<int32_t>(M);
    w.bytes = c.bytes();
    return w;
}

inline bool good_sizes(int N, int M) { return N >= 0 && M >= 0 && N < MAX_POINTS && M < MAX_POINTS; }

// max_dist finite and positive with a finite, normal square; md2 and the quantum scale, each rounded once
inline bool good_max_dist(float max_dist, float& md2, float& scale) {
    if (!(max_dist > 0.0f) || !(max_dist < __builtin_inff())) return false;
    md2 = max_dist * max_dist;
    scale = 1048576.0f / max_dist;
    return md2 >= FLT_MIN && md2 < __builtin_inff() && scale < __builtin_inff();
}

}  // namespace cloud_grid
}  // namespace colvo
