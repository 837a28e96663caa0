// cloud.hip -- exact truncated nearest neighbours between two point clouds: for every point of a query cloud the
// squared distance to, and the index of, the nearest point of a reference cloud within max_dist, and exact integer statistics over
// the query cloud.  Contract: include/colvo.h (colvo_cloud_*); NumPy replica tests/cloud_ref.py.
//
//   build   k_cloud_bounds: bounding box of the valid reference points, integer max on an order-preserving map of the float bits.
//           k_cloud_grid: one thread turns the box into origin, cell edge and dims, in a device header the later kernels read.
//           k_cloud_hist: one thread per point, 32-bit integer add into its cell's count; the value the add returns is the point's
//           rank in its cell.  The ordered scan of csrc/scan.hip over the cells, the entry count read from the device header
//           and clamped to the launches' bound.  k_cloud_scatter: 16-byte records (x, y, z, original index)
//           to start[cell] + rank.  The order inside a cell follows the atomics; no output depends on it.
//   query   k_cloud_query: one lane per query; the 9 x-runs of up to 3 cells around the query's cell are contiguous in the sorted
//           records; the minimum of the 64-bit keys (bits(d2) << 32) | index stays in registers.  Statistics are reduced per
//           workgroup and added to one of 256 counter lines; k_cloud_stats sums the lines.
//
// Every hand-off between phases is a kernel boundary.  The minimum of a set does not depend on the order it is taken in and every
// sum is an unsigned integer, so a call's bits do not depend on scheduling or on the stream.  The arithmetic that decides a distance,
// a cell or a quantum is pinned: float32, every operation individually rounded -- contraction is off for this whole file.
#include "scene.h"

#pragma clang fp contract(off)

#include "cloud_grid.h"

namespace colvo {
namespace {

using namespace cloud_grid;                              // Header, Grid, load_grid, grid_coord, nearest_key, the workspace's layout

constexpr int NT = 256;
constexpr int N_STATS = 12;
constexpr int MAX_THRESHOLDS = 8;
constexpr int BOUNDS_MAX_BLOCKS = 1024;

struct Thresholds {
    float t2[MAX_THRESHOLDS];              // float32(tau) * float32(tau)
    int n;
};

struct Sim3 {
    float r[9], t[3], s;
};

// cell of a VALID reference point; the clamp never acts on a point of the box the grid was made from (the dims come from the same
// routine, which is monotone) and turns the NaN of an unbounded box (G.single: inf * 0) into cell 0
__device__ __forceinline__ int ref_cell(const Grid& G, float x, float y, float z) {
    const float p[3] = {x, y, z};
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = (int)fminf(fmaxf(floorf(grid_coord(G, a, p[a])), 0.0f), (float)(G.n[a] - 1));
    return (c[2] * G.n[1] + c[1]) * G.n[0] + c[0];
}

// ---- build ------------------------------------------------------------------------------------------------------------------- //
// grid min(ceil(M / NT), BOUNDS_MAX_BLOCKS), grid-stride: six integer maxima and a count per workgroup
__global__ __launch_bounds__(NT) void k_cloud_bounds(const float* __restrict__ P, int M, Header* __restrict__ h) {
    __shared__ uint32_t sm[NT / 64][7];
    uint32_t k[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t n = 0u;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < M; i += (long long)gridDim.x * NT) {
        const float x = P[i * 3 + 0], y = P[i * 3 + 1], z = P[i * 3 + 2];
        if (!(finite_f(x) && finite_f(y) && finite_f(z))) continue;
        const float p[3] = {x, y, z};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t q = float_key(p[a]);
            k[a] = max(k[a], ~q);
            k[3 + a] = max(k[3 + a], q);
        }
        ++n;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int j = 0; j < 6; ++j) k[j] = max(k[j], (uint32_t)__shfl_xor((int)k[j], off));
        n += (uint32_t)__shfl_xor((int)n, off);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 6; ++j) sm[threadIdx.x >> 6][j] = k[j];
        sm[threadIdx.x >> 6][6] = n;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int j = threadIdx.x;
        if (j < 6) {
            const uint32_t v = max(max(sm[0][j], sm[1][j]), max(sm[2][j], sm[3][j]));
            if ((sm[0][6] + sm[1][6]) + (sm[2][6] + sm[3][6]) != 0u) atomicMax(&h->key[j], v);
        } else {
            const uint32_t v = (sm[0][6] + sm[1][6]) + (sm[2][6] + sm[3][6]);
            if (v) atomicAdd(&h->n_valid, v);
        }
    }
}

// one thread: the box -> origin, edge, dims (cloud_grid::make_grid)
__global__ void k_cloud_grid(Header* __restrict__ h, float max_dist) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    make_grid(h, max_dist);
}

// one thread per reference point: count[cell] += 1; the value before the add is the point's rank in its cell (-1: invalid point)
__global__ __launch_bounds__(NT) void k_cloud_hist(const float* __restrict__ P, int M, const Header* __restrict__ h,
                                                   int32_t* __restrict__ count, int32_t* __restrict__ rank) {
    const Grid G = load_grid(h);
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= M) return;
    const float x = P[i * 3 + 0], y = P[i * 3 + 1], z = P[i * 3 + 2];
    int r = -1;
    if (G.cells > 0 && finite_f(x) && finite_f(y) && finite_f(z)) r = atomicAdd(&count[ref_cell(G, x, y, z)], 1);
    rank[i] = r;
}

// one thread per reference point: its record goes to start[cell] + rank
__global__ __launch_bounds__(NT) void k_cloud_scatter(const float* __restrict__ P, int M, const Header* __restrict__ h,
                                                      const int32_t* __restrict__ start, const int32_t* __restrict__ rank,
                                                      float4* __restrict__ rec) {
    const Grid G = load_grid(h);
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= M) return;
    const int r = rank[i];
    if (r < 0 || G.cells <= 0) return;
    const float x = P[i * 3 + 0], y = P[i * 3 + 1], z = P[i * 3 + 2];
    const long long pos = (long long)start[ref_cell(G, x, y, z)] + r;
    if (pos >= 0 && pos < M) rec[pos] = make_float4(x, y, z, __int_as_float((int)i));       // (always, for the counts of this build)
}

// ---- query ------------------------------------------------------------------------------------------------------------------- //
// grid ceil(N / NT), one lane per query
__global__ __launch_bounds__(NT) void k_cloud_query(const float* __restrict__ Q, int N, const Header* __restrict__ h,
                                                    const int32_t* __restrict__ start, const float4* __restrict__ rec, int M,
                                                    float md2, float s, Thresholds thr, float* __restrict__ dist,
                                                    float* __restrict__ dist2, int32_t* __restrict__ nearest,
                                                    unsigned long long* __restrict__ counters) {
    __shared__ unsigned long long sm[NT / 64][N_STATS];
    const Grid G = load_grid(h);
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    const bool in = i < N;
    float q[3] = {0.0f, 0.0f, 0.0f};
    if (in) {
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = Q[i * 3 + a];
    }
    const bool valid = in && finite_f(q[0]) && finite_f(q[1]) && finite_f(q[2]);
    unsigned long long examined = 0ull;
    const unsigned long long best = nearest_key(G, q, valid, start, rec, M, md2, examined);
    const float d2v = __uint_as_float((uint32_t)(best >> 32));
    const float dv = sqrtf(d2v);                             // correctly rounded (the build keeps HIP's default for sqrt and division)
    const int idx = (int)(uint32_t)best;
    if (in) {
        dist[i] = dv;
        dist2[i] = d2v;
        nearest[i] = idx;
    }
    // statistics: per wave, per workgroup, then one add per word into this workgroup's counter line
    unsigned long long st[N_STATS];
    st[0] = (unsigned long long)__popcll(__ballot(valid));
    st[1] = (unsigned long long)__popcll(__ballot(valid && idx >= 0));
#pragma unroll
    for (int k = 0; k < MAX_THRESHOLDS; ++k) st[2 + k] = (unsigned long long)__popcll(__ballot(valid && k < thr.n && d2v < thr.t2[k]));
    st[10] = wave_sum(valid ? (unsigned long long)(uint32_t)rintf(dv * s) : 0ull);
    st[11] = wave_sum(examined);
    striped_counter_add(st, sm, counters + (size_t)(blockIdx.x % COUNTER_LINES) * COUNTER_PITCH);
}

// one workgroup: stats[k] = sum over the counter lines
__global__ void k_cloud_stats(const unsigned long long* __restrict__ counters, unsigned long long* __restrict__ stats) {
    if (threadIdx.x >= N_STATS) return;
    unsigned long long s = 0ull;
    for (int l = 0; l < COUNTER_LINES; ++l) s += counters[(size_t)l * COUNTER_PITCH + threadIdx.x];
    stats[threadIdx.x] = s;
}

// one thread per point
__global__ __launch_bounds__(NT) void k_cloud_transform(const float* P, int N, Sim3 T, float* out) {      // (out may be P)
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    const float x = P[i * 3 + 0], y = P[i * 3 + 1], z = P[i * 3 + 2];
    float o[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = ((T.s * ((T.r[a * 3 + 0] * x + T.r[a * 3 + 1] * y) + T.r[a * 3 + 2] * z)) + T.t[a]);
#pragma unroll
    for (int a = 0; a < 3; ++a) out[i * 3 + a] = o[a];
}

}  // namespace
}  // namespace colvo

using namespace colvo;
using namespace colvo::cloud_grid;

extern "C" size_t colvo_cloud_workspace_bytes(int N, int M) {
    if (!good_sizes(N, M)) return 0;
    return layout(nullptr, M).bytes;
}

extern "C" int colvo_cloud_index_build(const float* ref, int M, float max_dist, void* workspace, colvo_stream_t stream) {
    COLVO_CHECK_ARG(workspace && (ref || M == 0), "colvo_cloud_index_build: null pointer argument");
    COLVO_CHECK_ARG(good_sizes(0, M), "colvo_cloud_index_build: bad shape M=%d (0 .. 2^30 - 1)", M);
    float md2, scale;
    COLVO_CHECK_ARG(good_max_dist(max_dist, md2, scale),
                    "colvo_cloud_index_build: bad max_dist %g (finite, positive, with a finite positive float32 square)", (double)max_dist);
    COLVO_CHECK_ARG(aligned16(workspace), "colvo_cloud_index_build: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const Ws w = layout(workspace, M);
    COLVO_CHECK_HIP(hipMemsetAsync(w.header, 0, sizeof(Header), s), "colvo_cloud_index_build");
    if (M == 0) return 0;                                        // cells = 0: the query walks nothing
    COLVO_CHECK_HIP(hipMemsetAsync(w.cells, 0, (size_t)SCAN_ENTRIES * 4, s), "colvo_cloud_index_build");
    const int nb = blocks_of(M, NT);
    colvo::launch(k_cloud_bounds, dim3(nb < BOUNDS_MAX_BLOCKS ? nb : BOUNDS_MAX_BLOCKS), dim3(NT), 0, s, ref, M, w.header);
    COLVO_CHECK_LAUNCH("k_cloud_bounds");
    colvo::launch(k_cloud_grid, dim3(1), dim3(64), 0, s, w.header, max_dist);
    COLVO_CHECK_LAUNCH("k_cloud_grid");
    colvo::launch(k_cloud_hist, dim3(nb), dim3(NT), 0, s, ref, M, w.header, w.cells, w.rank);
    COLVO_CHECK_LAUNCH("k_cloud_hist");
    if (int rc = scan_exclusive(Scan{w.cells, SCAN_ENTRIES, &w.header->cells, w.sums, nullptr, nullptr, 0}, s)) return rc;
    colvo::launch(k_cloud_scatter, dim3(nb), dim3(NT), 0, s, ref, M, w.header, w.cells, w.rank, w.rec);
    COLVO_CHECK_LAUNCH("k_cloud_scatter");
    return 0;
}

extern "C" int colvo_cloud_query(const float* query, int N, int M, float max_dist, const float* thresholds, int n_thresholds,
                                 void* workspace, float* dist, float* dist2, int32_t* nearest, uint64_t* stats,
                                 colvo_stream_t stream) {
    COLVO_CHECK_ARG(workspace && stats && ((query && dist && dist2 && nearest) || N == 0) && (thresholds || n_thresholds == 0),
                    "colvo_cloud_query: null pointer argument");
    COLVO_CHECK_ARG(good_sizes(N, M), "colvo_cloud_query: bad shape N=%d M=%d (0 .. 2^30 - 1)", N, M);
    float md2, scale;
    COLVO_CHECK_ARG(good_max_dist(max_dist, md2, scale),
                    "colvo_cloud_query: bad max_dist %g (finite, positive, with a finite positive float32 square)", (double)max_dist);
    COLVO_CHECK_ARG(n_thresholds >= 0 && n_thresholds <= MAX_THRESHOLDS, "colvo_cloud_query: bad thresholds: %d of them (0 .. %d)",
                    n_thresholds, MAX_THRESHOLDS);
    Thresholds thr;
    thr.n = n_thresholds;
    for (int k = 0; k < MAX_THRESHOLDS; ++k) {
        thr.t2[k] = 0.0f;
        if (k >= n_thresholds) continue;
        const float t = thresholds[k];
        COLVO_CHECK_ARG(t > 0.0f && t <= max_dist && (k == 0 || t >= thresholds[k - 1]),
                        "colvo_cloud_query: bad thresholds: tau[%d] = %g (positive, non-descending, <= max_dist %g)", k, (double)t,
                        (double)max_dist);
        thr.t2[k] = t * t;
    }
    COLVO_CHECK_ARG(aligned16(workspace), "colvo_cloud_query: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const Ws w = layout(workspace, M);
    COLVO_CHECK_HIP(hipMemsetAsync(w.counters, 0, (size_t)COUNTER_LINES * COUNTER_PITCH * 8, s), "colvo_cloud_query");
    if (N > 0) {
        colvo::launch(k_cloud_query, dim3(blocks_of(N, NT)), dim3(NT), 0, s, query, N, (const Header*)w.header, (const int32_t*)w.cells,
                      (const float4*)w.rec, M, md2, scale, thr, dist, dist2, nearest, w.counters);
        COLVO_CHECK_LAUNCH("k_cloud_query");
    }
    colvo::launch(k_cloud_stats, dim3(1), dim3(64), 0, s, (const unsigned long long*)w.counters,
                  reinterpret_cast<unsigned long long*>(stats));
    COLVO_CHECK_LAUNCH("k_cloud_stats");
    return 0;
}

extern "C" int colvo_cloud_transform(const float* points, int N, const float* Rts, float* out, colvo_stream_t stream) {
    COLVO_CHECK_ARG(Rts && ((points && out) || N == 0), "colvo_cloud_transform: null pointer argument");
    COLVO_CHECK_ARG(good_sizes(N, 0), "colvo_cloud_transform: bad shape N=%d (0 .. 2^30 - 1)", N);
    if (N == 0) return 0;
    Sim3 T;
    for (int k = 0; k < 9; ++k) T.r[k] = Rts[k];
    for (int k = 0; k < 3; ++k) T.t[k] = Rts[9 + k];
    T.s = Rts[12];
    colvo::launch(k_cloud_transform, dim3(blocks_of(N, NT)), dim3(NT), 0, (hipStream_t)stream, points, N, T, out);
    COLVO_CHECK_LAUNCH("k_cloud_transform");
    return 0;
}
