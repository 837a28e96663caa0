// normals.hip -- surface normals of a fused cloud: every sample the fusion walked gets a finite-difference normal from
// its depth map, turned into the world frame and quantised; the normals of the samples of a voxel are summed as integers in the row
// the voxel has in the cloud, and the sum's direction is the row's normal, its length per sample the row's coherence.  Contract:
// include/colvo.h (colvo_cloud_normals).
//
//   k_normals_keys        one thread per row: voxel (ix, iy, iz) -> brick * 512 + local, the order the rows are in.
//   k_normals_accumulate  the fusion's walk and the fusion's `locate` (csrc/voxel_grid.h: the same routine, so the same voxel); the
//                         four neighbours one pixel away in the full-resolution map, one-sided where one is missing or lies across
//                         a depth edge; cross product, faced to the camera, normalised, rotated, quantised to 2^-14.  The row is
//                         found by binary search among the keys; the issuing lanes' records (sum qx, sum qy, sum qz, n: four 64-bit
//                         words, 32 bytes) are compacted through LDS and added a record per four adjacent lanes, as k_fuse_accumulate
//                         adds its records.
//   k_normals_write       one thread per row, float64: normal = sum / |sum|, coherence = |sum| / (16384 n).
//   k_normals_stats       one workgroup: the counter lines summed into stats[4].
//
// All sums are integers added with native atomics: a call's bits do not depend on scheduling, on the stream or on the order of the
// frames.  Float32 with every operation individually rounded -- contraction is off for this whole file.
#include "scene.h"

#pragma clang fp contract(off)

#include "voxel_grid.h"

namespace colvo {
namespace {

using namespace voxel_grid;

constexpr int COUNTER_LINES = 256;         // the sample counters: this many sets of four,
constexpr int COUNTER_PITCH = 16;          // ... one per 64-byte line
constexpr int N_STATS = 4;                 // kept, with a normal, ... in a row of the cloud, ... in no row
constexpr float QUANTUM = 16384.0f;        // a unit normal's components as integers of 2^-14

struct Sums {                              // sum qx, sum qy, sum qz (two's complement), n.  |q| <= 2^14 + 1 and n < 2^24: below 2^39
    unsigned long long w[4];
};
static_assert(sizeof(Sums) == 32, "Sums is 32 B");

// grid ceil(M / NT).  Unsigned arithmetic: whatever `voxels` holds, a key is a number and nothing else
__global__ __launch_bounds__(NT) void k_normals_keys(const int32_t* __restrict__ voxels, int M, Grid G, long long* __restrict__ keys) {
    const int m = blockIdx.x * NT + threadIdx.x;
    if (m >= M) return;
    const int32_t* x = voxels + (size_t)m * 3;
    const int ix = x[0], iy = x[1], iz = x[2];
    const unsigned long long brick =
        ((unsigned long long)(iz >> 3) * (unsigned long long)G.nb[1] + (unsigned long long)(iy >> 3)) * (unsigned long long)G.nb[0] +
        (unsigned long long)(ix >> 3);
    const unsigned long long local = (unsigned long long)((((iz & 7) * BRICK) + (iy & 7)) * BRICK + (ix & 7));
    keys[m] = (long long)(brick * (unsigned long long)BRICK_VOX + local);
}

// camera point of pixel (u, v) at depth d: (((u - cx) / fx) * d, ((v - cy) / fy) * d, d)
__device__ __forceinline__ void cam_point(const Cam& c, float u, float v, float d, float (&P)[3]) {
    P[0] = __fdiv_rn(u - c.cx, c.fx) * d;
    P[1] = __fdiv_rn(v - c.cy, c.fy) * d;
    P[2] = d;
}

// the tangent along one image axis from the neighbours one pixel before (a) and behind (b) the sample: both usable -> central
// difference, one -> one-sided, none -> false
__device__ __forceinline__ bool tangent(const Cam& c, const float (&Pc)[3], bool use_a, float ua, float va, float da, bool use_b,
                                        float ub, float vb, float db, float (&t)[3]) {
    float A[3], B[3];
    cam_point(c, ua, va, da, A);
    cam_point(c, ub, vb, db, B);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float hi = use_b ? B[k] : Pc[k];
        const float lo = use_a ? A[k] : Pc[k];
        t[k] = hi - lo;
    }
    return (int)use_a | (int)use_b;
}

// grid (blocks_per_frame, N)
__global__ __launch_bounds__(NT) void k_normals_accumulate(const float* __restrict__ depth, const float* __restrict__ K,
                                                           const float* __restrict__ M, Walk w, Grid G, float max_depth, float rel_edge,
                                                           const long long* __restrict__ keys, int n_rows, Sums* __restrict__ sums,
                                                           int32_t* __restrict__ counters) {
    __shared__ unsigned long long out_w[NT][4];
    __shared__ int out_row[NT];
    __shared__ int sm[NT / 64][N_STATS];
    const int b = blockIdx.y;
    int u = 0, v = 0;
    const bool in = walk_pixel(w, u, v);
    const float* frame = depth + (size_t)b * w.H * w.W;
    const float d = in ? frame[(size_t)v * w.W + u] : 0.0f;
    const bool kept = in && valid_depth(d, max_depth);
    const Cam c = load_cam(K, M, b);
    // the four neighbours, one pixel away in the full-resolution map whatever the stride: left, right, up, down
    const int nu[4] = {u - 1, u + 1, u, u}, nv[4] = {v, v, v - 1, v + 1};
    float nd[4];
    bool use[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool inside = kept && nu[k] >= 0 && nu[k] < w.W && nv[k] >= 0 && nv[k] < w.H;
        nd[k] = inside ? frame[(size_t)nv[k] * w.W + nu[k]] : 0.0f;
        // usable: inside, a valid depth, and not across a depth edge (the relative measure of the consistency filter)
        use[k] = (int)inside & (int)valid_depth(nd[k], max_depth) & (int)(fabsf(nd[k] - d) < rel_edge * (nd[k] + d));
    }
    float Pc[3], tu[3], tv[3];
    cam_point(c, (float)u, (float)v, d, Pc);
    const bool has_u = tangent(c, Pc, use[0], (float)nu[0], (float)nv[0], nd[0], use[1], (float)nu[1], (float)nv[1], nd[1], tu);
    const bool has_v = tangent(c, Pc, use[2], (float)nu[2], (float)nv[2], nd[2], use[3], (float)nu[3], (float)nv[3], nd[3], tv);
    float n[3] = {tu[1] * tv[2] - tu[2] * tv[1], tu[2] * tv[0] - tu[0] * tv[2], tu[0] * tv[1] - tu[1] * tv[0]};
    const bool away = (n[0] * Pc[0] + n[1] * Pc[1]) + n[2] * Pc[2] > 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = away ? -n[k] : n[k];
    const float L = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const bool normal = (int)kept & (int)has_u & (int)has_v & (int)(L > 0.0f) & (int)(L < __builtin_inff());       // NaN falls out
    int q[3] = {0, 0, 0};
    if (normal) {                                                // |N_a| <= sqrt(3) (1 + a few u): the product converts safely
        const float e[3] = {n[0] / L, n[1] / L, n[2] / L};
#pragma unroll
        for (int a = 0; a < 3; ++a)
            q[a] = (int)rintf(((c.r[a * 3 + 0] * e[0] + c.r[a * 3 + 1] * e[1]) + c.r[a * 3 + 2] * e[2]) * QUANTUM);
    }
    Voxel vx;
    const bool inside = kept && locate(c, G, (float)u, (float)v, d, vx);
    // the row: lower bound of the key among the rows' keys.  0 <= lo <= mid < hi <= n_rows: no index leaves keys[0..n_rows)
    int row = -1;
    if (normal && inside) {
        const long long key = (long long)vx.brick * BRICK_VOX + vx.local;
        int lo = 0, hi = n_rows;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        if (lo < n_rows && keys[lo] == key) row = lo;
    }
    const bool issuer = row >= 0;
    const int cnt[N_STATS] = {(int)__popcll(__ballot(kept)), (int)__popcll(__ballot(normal)), (int)__popcll(__ballot(issuer)),
                              (int)__popcll(__ballot(normal && !issuer))};
    // the issuing lanes' records, compacted, then a record per four adjacent lanes: one instruction covers the 32 contiguous bytes of
    // 16 records (csrc/fuse.hip measured lane-per-record at 3.3 to 3.8 times the time: the memory side works in requests)
    const int lane = threadIdx.x & 63, wave0 = threadIdx.x & ~63;
    const unsigned long long issuers = __ballot(issuer);
    const int n_issuers = __popcll(issuers);
    if (issuer) {
        const int r = wave0 + __popcll(issuers & ((1ull << lane) - 1ull));
        out_w[r][0] = (unsigned long long)(long long)q[0];
        out_w[r][1] = (unsigned long long)(long long)q[1];
        out_w[r][2] = (unsigned long long)(long long)q[2];
        out_w[r][3] = 1ull;
        out_row[r] = row;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // the LDS writes of this wave's lanes, visible to its other lanes
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int i = 0; i < n_issuers; i += 16) {
        const int r = i + (lane >> 2), word = lane & 3;
        if (r < n_issuers) {
            const unsigned long long val = out_w[wave0 + r][word];
            if (val != 0ull) atomicAdd(&sums[out_row[wave0 + r]].w[word], val);
        }
    }
    const unsigned line = (blockIdx.y * gridDim.x + blockIdx.x) % COUNTER_LINES;
    striped_counter_add(cnt, sm, counters + line * COUNTER_PITCH);
}

// grid ceil(M / NT): float64, every operation individually rounded
__global__ __launch_bounds__(NT) void k_normals_write(const Sums* __restrict__ sums, int M, float* __restrict__ normals,
                                                      int32_t* __restrict__ counts, float* __restrict__ coherence) {
    const int m = blockIdx.x * NT + threadIdx.x;
    if (m >= M) return;
    const Sums s = sums[m];
    const double sx = (double)(long long)s.w[0], sy = (double)(long long)s.w[1], sz = (double)(long long)s.w[2];
    const unsigned long long n = s.w[3];
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    const bool some = n != 0ull && len > 0.0;
    normals[(size_t)m * 3 + 0] = some ? (float)(sx / len) : 0.0f;
    normals[(size_t)m * 3 + 1] = some ? (float)(sy / len) : 0.0f;
    normals[(size_t)m * 3 + 2] = some ? (float)(sz / len) : 0.0f;
    coherence[m] = some ? (float)(len / (16384.0 * (double)n)) : 0.0f;
    counts[m] = (int32_t)n;
}

// one workgroup: stats[k] = sum over the counter lines
__global__ __launch_bounds__(NT) void k_normals_stats(const int32_t* __restrict__ counters, int32_t* __restrict__ stats) {
    __shared__ int sm[N_STATS][NT / 64];
    static_assert(COUNTER_LINES == NT, "one counter line per thread");
    int t[N_STATS];
#pragma unroll
    for (int k = 0; k < N_STATS; ++k) t[k] = block_sum(counters[threadIdx.x * COUNTER_PITCH + k], sm[k]);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N_STATS; ++k) stats[k] = t[k];
    }
}

struct Scratch {                           // the rows' sums [M] and the counter lines (cleared together), the rows' keys [M]
    Sums* sums;
    int32_t* counters;
    long long* keys;
    size_t clear_bytes, bytes;
};

Scratch layout(void* base, int M) {
    Carver c(base);
    Scratch s;
    s.sums = c.take<Sums>((size_t)M);
    s.counters = c.take<int32_t>((size_t)COUNTER_LINES * COUNTER_PITCH);
    s.clear_bytes = c.bytes();
    s.keys = c.take<long long>((size_t)M);
    s.bytes = c.bytes();
    return s;
}

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" size_t colvo_cloud_normals_scratch_bytes(int M) {
    if (M < 0) return 0;
    return layout(nullptr, M).bytes;
}

extern "C" int colvo_cloud_normals(const float* depths, const float* K, const float* cam2world, int N, int H, int W, int stride,
                                   float max_depth, float ox, float oy, float oz, float voxel_size, int nx, int ny, int nz,
                                   const int32_t* voxels, int M, float rel_edge, void* scratch, float* normals, int32_t* counts,
                                   float* coherence, int32_t* stats, colvo_stream_t stream) {
    COLVO_CHECK_ARG(M >= 0, "colvo_cloud_normals: bad row count M=%d (0 <= M < 2^31)", M);
    COLVO_CHECK_ARG(depths && K && cam2world && scratch && stats && ((voxels && normals && counts && coherence) || M == 0),
                    "colvo_cloud_normals: null pointer argument");
    Walk w;
    Grid G;
    COLVO_CHECK_ARG(walk_geom(N, H, W, stride, w), "colvo_cloud_normals: bad shape N=%d H=%d W=%d stride=%d", N, H, W, stride);
    COLVO_CHECK_ARG(grid_geom(ox, oy, oz, voxel_size, nx, ny, nz, G),
                    "colvo_cloud_normals: bad grid origin (%g, %g, %g) voxel_size %g dims %d x %d x %d", (double)ox, (double)oy, (double)oz,
                    (double)voxel_size, nx, ny, nz);
    COLVO_CHECK_ARG(max_depth > 0.0f && max_depth < __builtin_inff(), "colvo_cloud_normals: bad max_depth %g (finite and positive)",
                    (double)max_depth);
    COLVO_CHECK_ARG(rel_edge > 0.0f && rel_edge < __builtin_inff(), "colvo_cloud_normals: bad rel_edge %g (finite and positive)",
                    (double)rel_edge);
    COLVO_CHECK_ARG(aligned16(scratch), "colvo_cloud_normals: scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const Scratch sc = layout(scratch, M);
    COLVO_CHECK_HIP(hipMemsetAsync(sc.sums, 0, sc.clear_bytes, s), "colvo_cloud_normals");      // ... and the counter lines behind them
    if (M > 0) {
        colvo::launch(k_normals_keys, dim3(blocks_of(M, NT)), dim3(NT), 0, s, voxels, M, G, sc.keys);
        COLVO_CHECK_LAUNCH("k_normals_keys");
    }
    colvo::launch(k_normals_accumulate, dim3(w.blocks_per_frame, N), dim3(NT), 0, s, depths, K, cam2world, w, G, max_depth, rel_edge,
                  (const long long*)sc.keys, M, sc.sums, sc.counters);
    COLVO_CHECK_LAUNCH("k_normals_accumulate");
    if (M > 0) {
        colvo::launch(k_normals_write, dim3(blocks_of(M, NT)), dim3(NT), 0, s, (const Sums*)sc.sums, M, normals, counts, coherence);
        COLVO_CHECK_LAUNCH("k_normals_write");
    }
    colvo::launch(k_normals_stats, dim3(1), dim3(NT), 0, s, (const int32_t*)sc.counters, stats);
    COLVO_CHECK_LAUNCH("k_normals_stats");
    return 0;
}
