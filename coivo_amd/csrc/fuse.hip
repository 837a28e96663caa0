// fuse.hip -- depth maps + colours + trajectory -> one point per occupied voxel: mean position, mean colour and
// observation count of the samples that fell into each voxel of a regular grid.  Contract: include/colvo.h (colvo_fuse_*).
//
//   plan        k_fuse_mark: one thread per sample, marks the 8x8x8 brick it falls into.  The marks are numbered in ascending brick
//               order by the ordered scan of csrc/scan.hip -- no hash, so the output order is fixed.
//   accumulate  k_fuse_accumulate: the same walk and the same point routine (so the same bits), slot lookup, integer adds into the
//               brick's 512 records.  Lanes of a wave that hit the same voxel add once, through the first of them, and a record's
//               four words are added by four adjacent lanes of one instruction.
//   extract     rows per brick, the same scan, ordered write with the means evaluated in float64.
//
// Every hand-off between phases is a kernel boundary.  All sums are unsigned integers added with native atomics, so a call's bits do
// not depend on scheduling, on the stream or on the order of the frames.  The arithmetic that decides a sample's voxel is pinned:
// float32, every operation individually rounded -- contraction is off for this whole file.
#include "scene.h"
#include "tuning.h"

#pragma clang fp contract(off)

#include "voxel_grid.h"                    // Grid, Walk, Voxel and the pinned locate, shared with normals.hip

namespace colvo {
namespace {

using namespace voxel_grid;

constexpr int MAX_SLOTS = 1 << 22;         // n_bricks below this: a pool index (slot * 512 + local) stays below 2^31
constexpr int MAX_AGG_ROUNDS = 64;           // a wave holds at most 64 distinct voxels
constexpr int COUNTER_LINES = 256;         // k_fuse_mark's sample counters: this many pairs,
constexpr int COUNTER_PITCH = 16;          // ... one per 64-byte line

// one voxel: [n | sum qx] [sum qy | sum qz] [sum cr | sum cg] [sum cb | 0], high half first.  With n < 2^24 no low half can carry
// into its neighbour (255 * 2^24 < 2^32), so a sample costs four 64-bit adds into one 32-byte sector.
struct Record {
    unsigned long long w[4];
};
static_assert(sizeof(Record) == 32, "Record is 32 B");

// grid (blocks_per_frame, N).  The two sample counts are summed per workgroup and added to one of COUNTER_LINES pairs, each in a
// 64-byte line of its own (every wave adding to ONE address measured 7 ms for 42 M samples: 1.3 M adds queue up behind each other)
__global__ __launch_bounds__(NT) void k_fuse_mark(const float* __restrict__ depth, const float* __restrict__ K,
                                                  const float* __restrict__ M, Walk w, Grid G, float max_depth,
                                                  int32_t* __restrict__ brick_table, int32_t* __restrict__ counters) {
    __shared__ int sm[NT / 64][2];
    const int b = blockIdx.y;
    int u = 0, v = 0;
    const bool in = walk_pixel(w, u, v);
    const float d = in ? depth[((size_t)b * w.H + v) * w.W + u] : 0.0f;
    const bool kept = in && valid_depth(d, max_depth);
    const Cam c = load_cam(K, M, b);
    Voxel vx;
    const bool inside = kept && locate(c, G, (float)u, (float)v, d, vx);
    if (inside) brick_table[vx.brick] = 1;                       // idempotent same-value store
    const int n[2] = {(int)__popcll(__ballot(kept)), (int)__popcll(__ballot(kept && !inside))};
    const unsigned line = (blockIdx.y * gridDim.x + blockIdx.x) % COUNTER_LINES;
    striped_counter_add(n, sm, counters + line * COUNTER_PITCH);
}

// one workgroup: stats[0], stats[1] = sums over the counter lines
__global__ __launch_bounds__(NT) void k_fuse_stats(const int32_t* __restrict__ counters, int32_t* __restrict__ stats) {
    __shared__ int sm[NT / 64];
    __shared__ int sm2[NT / 64];
    static_assert(COUNTER_LINES == NT, "one counter line per thread");
    const int n_kept = block_sum(counters[threadIdx.x * COUNTER_PITCH], sm);
    const int n_out = block_sum(counters[threadIdx.x * COUNTER_PITCH + 1], sm2);
    if (threadIdx.x == 0) {
        stats[0] = n_kept;
        stats[1] = n_out;
    }
}

// ---- accumulate ------------------------------------------------------------------------------------------------------------- //
__device__ __forceinline__ void wave_lds_sync() {                // the LDS writes of this wave's lanes, visible to its other lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// grid (blocks_per_frame, N).  The result does not depend on either switch: integer sums.
//   agg_rounds > 0   up to that many distinct voxels of a wave are matched lane against lane; the lanes of a match add their sample,
//                    packed into two words of 16-bit fields (64 quanta of 8 bits stay below 2^14), to an LDS row owned by the first
//                    of them, which issues for all.  Lanes left unmatched issue their own sample.
//   row_adds         the issuing lanes' records are compacted through LDS and added a record per four adjacent lanes: one
//                    instruction covers the 32 contiguous bytes of 16 records, where lane-per-record takes four instructions that
//                    each touch 64 records (the memory side works in requests, not in lanes).
__global__ __launch_bounds__(NT) void k_fuse_accumulate(const float* __restrict__ depth, const float* __restrict__ colors,
                                                        const float* __restrict__ K, const float* __restrict__ M, Walk w, Grid G,
                                                        float max_depth, const int32_t* __restrict__ brick_table,
                                                        Record* __restrict__ pool, int n_bricks, int agg_rounds, int row_adds) {
    __shared__ unsigned long long row[NT][2];
    __shared__ unsigned long long out_w[NT][4];
    __shared__ int out_key[NT];
    const int b = blockIdx.y;
    int u = 0, v = 0;
    const bool in = walk_pixel(w, u, v);
    const size_t HW = (size_t)w.H * w.W;
    const size_t px = (size_t)v * w.W + u;
    const float d = in ? depth[(size_t)b * HW + px] : 0.0f;
    const bool kept = in && valid_depth(d, max_depth);
    const Cam c = load_cam(K, M, b);
    Voxel vx;
    bool inside = kept && locate(c, G, (float)u, (float)v, d, vx);
    const bool colour = colors != nullptr;
    uint32_t cq[3] = {0u, 0u, 0u};
    if (inside && colour) {
#pragma unroll
        for (int k = 0; k < 3; ++k) cq[k] = colour_quantum(colors[((size_t)b * 3 + k) * HW + px]);
    }
    int key = -1;
    if (inside) {
        const int slot = brick_table[vx.brick];
        inside = slot >= 0 && slot < n_bricks;                   // always true for the plan this pool was sized from
        key = slot * BRICK_VOX + vx.local;
    }
    const int lane = threadIdx.x & 63, wave0 = threadIdx.x & ~63;
    // this lane's sample, packed: [n | qx | qy | qz] and [cr | cg | cb] in 16-bit fields
    unsigned long long a = 0ull, cc = 0ull;
    if (inside) {
        a = 1ull | ((unsigned long long)vx.q[0] << 16) | ((unsigned long long)vx.q[1] << 32) | ((unsigned long long)vx.q[2] << 48);
        cc = (unsigned long long)cq[0] | ((unsigned long long)cq[1] << 16) | ((unsigned long long)cq[2] << 32);
    }
    bool issuer = inside;
    if (agg_rounds > 0) {
        int my_leader = -1;
        row[threadIdx.x][0] = 0ull;
        row[threadIdx.x][1] = 0ull;
        unsigned long long remaining = __ballot(inside);
        for (int r = 0; r < agg_rounds && remaining != 0ull; ++r) {
            const int leader = __builtin_ctzll(remaining);
            const int lead_key = __builtin_amdgcn_readlane(key, leader);
            const bool same = inside && my_leader < 0 && key == lead_key;
            if (same) my_leader = leader;
            remaining &= ~__ballot(same);
        }
        wave_lds_sync();                                         // a wave's rows are its own: no workgroup barrier
        if (my_leader >= 0) {
            atomicAdd(&row[wave0 + my_leader][0], a);
            if (colour) atomicAdd(&row[wave0 + my_leader][1], cc);
        }
        wave_lds_sync();
        if (my_leader == lane) {
            a = row[threadIdx.x][0];
            cc = row[threadIdx.x][1];
        }
        issuer = inside && (my_leader < 0 || my_leader == lane);
    }
    // the record's words: [n | sum qx] [sum qy | sum qz] [sum cr | sum cg] [sum cb | 0]
    const unsigned long long w0 = ((a & 0xffffull) << 32) | ((a >> 16) & 0xffffull);
    const unsigned long long w1 = (((a >> 32) & 0xffffull) << 32) | (a >> 48);
    const unsigned long long w2 = ((cc & 0xffffull) << 32) | ((cc >> 16) & 0xffffull);
    const unsigned long long w3 = ((cc >> 32) & 0xffffull) << 32;
    if (!row_adds) {
        if (issuer) {
            Record* rec = &pool[key];
            atomicAdd(&rec->w[0], w0);
            atomicAdd(&rec->w[1], w1);
            if (colour) {
                atomicAdd(&rec->w[2], w2);
                atomicAdd(&rec->w[3], w3);
            }
        }
        return;
    }
    const unsigned long long issuers = __ballot(issuer);
    const int n_issuers = __popcll(issuers);
    if (issuer) {
        const int r = wave0 + __popcll(issuers & ((1ull << lane) - 1ull));
        out_w[r][0] = w0;
        out_w[r][1] = w1;
        out_w[r][2] = w2;
        out_w[r][3] = w3;
        out_key[r] = key;
    }
    wave_lds_sync();
    for (int i = 0; i < n_issuers; i += 16) {
        const int r = i + (lane >> 2), word = lane & 3;
        if (r < n_issuers) {
            const unsigned long long val = out_w[wave0 + r][word];
            if (val != 0ull) atomicAdd(&pool[out_key[wave0 + r]].w[word], val);      // (no colours: words 2, 3 are zero)
        }
    }
}

// ---- extract ---------------------------------------------------------------------------------------------------------------- //
// grid n_bricks: rows[slot] = voxels of the brick with n >= min_obs; occupied voxels -> stats2[0]; a voxel at the limit -> stats2[2]
__global__ __launch_bounds__(NT) void k_fuse_count(const Record* __restrict__ pool, int min_obs, unsigned long long limit,
                                                   int32_t* __restrict__ rows, int32_t* __restrict__ stats2) {
    __shared__ int sm[NT / 64];
    __shared__ int sm2[NT / 64];
    const Record* rec = pool + (size_t)blockIdx.x * BRICK_VOX;
    int n_rows = 0, n_occ = 0;
    bool over = false;
#pragma unroll
    for (int r = 0; r < BRICK_VOX / NT; ++r) {
        const unsigned long long n = rec[r * NT + threadIdx.x].w[0] >> 32;
        n_occ += n > 0ull;
        n_rows += n >= (unsigned long long)min_obs;
        over = over || n >= limit;
    }
    n_rows = block_sum(n_rows, sm);
    n_occ = block_sum(n_occ, sm2);
    if (threadIdx.x == 0) {
        rows[blockIdx.x] = n_rows;
        if (n_occ) atomicAdd(&stats2[0], n_occ);
    }
    if (over) atomicOr(&stats2[2], 1);
}

// grid n_bricks: the brick's rows, in local order, from offsets[slot] on
__global__ __launch_bounds__(NT) void k_fuse_write(const Record* __restrict__ pool, const int32_t* __restrict__ brick_list,
                                                   const int32_t* __restrict__ offsets, int min_obs, Grid G, float voxel_size,
                                                   int n_rows, float* __restrict__ points, float* __restrict__ colors,
                                                   int32_t* __restrict__ counts, int32_t* __restrict__ voxels) {
    __shared__ int wsum[BRICK_VOX / 64];
    const int slot = blockIdx.x;
    const Record* rec = pool + (size_t)slot * BRICK_VOX;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    Record rc[BRICK_VOX / NT];
    unsigned long long mask[BRICK_VOX / NT];
#pragma unroll
    for (int r = 0; r < BRICK_VOX / NT; ++r) {
        rc[r] = rec[r * NT + threadIdx.x];
        mask[r] = __ballot((rc[r].w[0] >> 32) >= (unsigned long long)min_obs);
        if (lane == 0) wsum[r * (NT / 64) + wv] = __popcll(mask[r]);
    }
    __syncthreads();
    const int brick = brick_list[slot];
    const int bx = brick % G.nb[0], by = (brick / G.nb[0]) % G.nb[1], bz = brick / (G.nb[0] * G.nb[1]);
    const double vs = (double)voxel_size;
#pragma unroll
    for (int r = 0; r < BRICK_VOX / NT; ++r) {
        const uint32_t n = (uint32_t)(rc[r].w[0] >> 32);
        if (n < (uint32_t)min_obs) continue;
        int m = offsets[slot] + __popcll(mask[r] & ((1ull << lane) - 1ull));
        for (int i = 0; i < r * (NT / 64) + wv; ++i) m += wsum[i];
        if (m >= n_rows) continue;                               // (a min_obs other than the count's: never past the caller's buffers)
        const int local = r * NT + threadIdx.x;
        const int idx[3] = {bx * BRICK + (local & 7), by * BRICK + ((local >> 3) & 7), bz * BRICK + (local >> 6)};
        const uint32_t sq[3] = {(uint32_t)rc[r].w[0], (uint32_t)(rc[r].w[1] >> 32), (uint32_t)rc[r].w[1]};
        const double dn = (double)n;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            points[(size_t)m * 3 + a] = (float)((double)G.o[a] + ((double)idx[a] + ((double)sq[a] + 0.5 * dn) / (256.0 * dn)) * vs);
            voxels[(size_t)m * 3 + a] = idx[a];
        }
        if (colors != nullptr) {
            const uint32_t sc[3] = {(uint32_t)(rc[r].w[2] >> 32), (uint32_t)rc[r].w[2], (uint32_t)(rc[r].w[3] >> 32)};
#pragma unroll
            for (int k = 0; k < 3; ++k) colors[(size_t)m * 3 + k] = (float)((double)sc[k] / (255.0 * dn));
        }
        counts[m] = (int32_t)n;
    }
}

// ---- host side: geometry and workspace layouts ------------------------------------------------------------------------------- //
struct PlanWs {                            // sample counters, brick table [bricks], brick list [min(bricks, MAX_SLOTS)], chunk sums
    int32_t* counters;
    int32_t* table;
    int32_t* list;
    int32_t* sums;
    int list_cap;
    size_t bytes;
};

PlanWs plan_ws(void* base, const Grid& G) {
    const int tb = total_bricks(G);
    Carver c(base);
    PlanWs p;
    p.list_cap = tb < MAX_SLOTS ? tb : MAX_SLOTS;
    p.counters = c.take<int32_t>((size_t)COUNTER_LINES * COUNTER_PITCH);
    p.table = c.take<int32_t>(tb);                               // (cleared together with the counters: it lies right behind them)
    p.list = c.take<int32_t>(p.list_cap);
    p.sums = c.take<int32_t>(scan_chunks(tb));
    p.bytes = c.bytes();
    return p;
}

struct ExtractWs {                         // rows per brick [n_bricks] (offsets after the scan), chunk sums
    int32_t* rows;
    int32_t* sums;
    size_t bytes;
};

ExtractWs extract_ws(void* base, int n_bricks) {
    Carver c(base);
    ExtractWs e;
    e.rows = c.take<int32_t>(n_bricks);
    e.sums = c.take<int32_t>(scan_chunks(n_bricks));
    e.bytes = c.bytes();
    return e;
}

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" size_t colvo_fuse_plan_workspace_bytes(int N, int H, int W, int stride, int nx, int ny, int nz) {
    Walk w;
    Grid G;
    if (!walk_geom(N, H, W, stride, w) || !grid_dims(nx, ny, nz, G)) return 0;
    return plan_ws(nullptr, G).bytes;
}

extern "C" int colvo_fuse_plan(const float* depths, const float* K, const float* cam2world, int N, int H, int W, int stride,
                               float max_depth, float ox, float oy, float oz, float voxel_size, int nx, int ny, int nz,
                               void* workspace, int32_t* stats, colvo_stream_t stream) {
    COLVO_CHECK_ARG(depths && K && cam2world && workspace && stats, "colvo_fuse_plan: null pointer argument");
    Walk w;
    Grid G;
    COLVO_CHECK_ARG(walk_geom(N, H, W, stride, w), "colvo_fuse_plan: bad shape N=%d H=%d W=%d stride=%d", N, H, W, stride);
    COLVO_CHECK_ARG(grid_geom(ox, oy, oz, voxel_size, nx, ny, nz, G),
                    "colvo_fuse_plan: bad grid origin (%g, %g, %g) voxel_size %g dims %d x %d x %d", (double)ox, (double)oy, (double)oz,
                    (double)voxel_size, nx, ny, nz);
    COLVO_CHECK_ARG(aligned16(workspace), "colvo_fuse_plan: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const PlanWs p = plan_ws(workspace, G);
    const int tb = total_bricks(G);
    COLVO_CHECK_HIP(hipMemsetAsync(p.counters, 0, (size_t)COUNTER_LINES * COUNTER_PITCH * 4 + (size_t)tb * 4, s),     // ... and the table
                    "colvo_fuse_plan");
    colvo::launch(k_fuse_mark, dim3(w.blocks_per_frame, N), dim3(NT), 0, s, depths, K, cam2world, w, G, max_depth, p.table, p.counters);
    COLVO_CHECK_LAUNCH("k_fuse_mark");
    colvo::launch(k_fuse_stats, dim3(1), dim3(NT), 0, s, p.counters, stats);
    COLVO_CHECK_LAUNCH("k_fuse_stats");
    return scan_exclusive(Scan{p.table, tb, nullptr, p.sums, stats + 2, p.list, p.list_cap}, s);
}

extern "C" size_t colvo_fuse_pool_bytes(int n_bricks) {
    if (n_bricks <= 0 || n_bricks >= MAX_SLOTS) return 0;
    return (size_t)n_bricks * BRICK_VOX * sizeof(Record);
}

extern "C" int colvo_fuse_accumulate(const float* depths, const float* colors, const float* K, const float* cam2world, int N, int H,
                                     int W, int stride, float max_depth, float ox, float oy, float oz, float voxel_size, int nx,
                                     int ny, int nz, const void* workspace, int n_bricks, void* pool, colvo_stream_t stream) {
    COLVO_CHECK_ARG(depths && K && cam2world && workspace && pool, "colvo_fuse_accumulate: null pointer argument");
    Walk w;
    Grid G;
    COLVO_CHECK_ARG(walk_geom(N, H, W, stride, w), "colvo_fuse_accumulate: bad shape N=%d H=%d W=%d stride=%d", N, H, W, stride);
    COLVO_CHECK_ARG(grid_geom(ox, oy, oz, voxel_size, nx, ny, nz, G),
                    "colvo_fuse_accumulate: bad grid origin (%g, %g, %g) voxel_size %g dims %d x %d x %d", (double)ox, (double)oy,
                    (double)oz, (double)voxel_size, nx, ny, nz);
    COLVO_CHECK_ARG(n_bricks > 0 && n_bricks < MAX_SLOTS && n_bricks <= total_bricks(G),
                    "colvo_fuse_accumulate: bad grid: n_bricks %d (1 .. min(2^22 - 1, %d))", n_bricks, total_bricks(G));
    COLVO_CHECK_ARG(aligned16(workspace) && aligned16(pool), "colvo_fuse_accumulate: workspace and pool must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const PlanWs p = plan_ws(const_cast<void*>(workspace), G);
    long rounds = TUNE(fuse_agg_rounds);
    rounds = rounds < 0 ? 0 : rounds > MAX_AGG_ROUNDS ? MAX_AGG_ROUNDS : rounds;
    COLVO_CHECK_HIP(hipMemsetAsync(pool, 0, (size_t)n_bricks * BRICK_VOX * sizeof(Record), s), "colvo_fuse_accumulate");
    colvo::launch(k_fuse_accumulate, dim3(w.blocks_per_frame, N), dim3(NT), 0, s, depths, colors, K, cam2world, w, G, max_depth,
                  p.table, static_cast<Record*>(pool), n_bricks, (int)rounds, (int)(TUNE(fuse_row_adds) != 0));
    COLVO_CHECK_LAUNCH("k_fuse_accumulate");
    return 0;
}

extern "C" size_t colvo_fuse_extract_workspace_bytes(int n_bricks) {
    if (n_bricks <= 0 || n_bricks >= MAX_SLOTS) return 0;
    return extract_ws(nullptr, n_bricks).bytes;
}

extern "C" int colvo_fuse_count(const void* pool, int n_bricks, int min_obs, void* extract_workspace, int32_t* stats2,
                                colvo_stream_t stream) {
    COLVO_CHECK_ARG(pool && extract_workspace && stats2, "colvo_fuse_count: null pointer argument");
    COLVO_CHECK_ARG(n_bricks > 0 && n_bricks < MAX_SLOTS && min_obs >= 1, "colvo_fuse_count: bad grid: n_bricks %d (1 .. 2^22 - 1), min_obs %d (>= 1)",
                    n_bricks, min_obs);
    COLVO_CHECK_ARG(aligned16(pool) && aligned16(extract_workspace), "colvo_fuse_count: pool and workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const ExtractWs e = extract_ws(extract_workspace, n_bricks);
    double limit = TUNE_F(fuse_count_limit);
    limit = limit < 1.0 ? 1.0 : limit > 16777216.0 ? 16777216.0 : limit;
    COLVO_CHECK_HIP(hipMemsetAsync(stats2, 0, 3 * sizeof(int32_t), s), "colvo_fuse_count");
    colvo::launch(k_fuse_count, dim3(n_bricks), dim3(NT), 0, s, static_cast<const Record*>(pool), min_obs, (unsigned long long)limit,
                  e.rows, stats2);
    COLVO_CHECK_LAUNCH("k_fuse_count");
    return scan_exclusive(Scan{e.rows, n_bricks, nullptr, e.sums, stats2 + 1, nullptr, 0}, s);
}

extern "C" int colvo_fuse_write(const void* workspace, const void* pool, int n_bricks, int min_obs, float ox, float oy, float oz,
                                float voxel_size, int nx, int ny, int nz, const void* extract_workspace, int n_rows, float* points,
                                float* colors, int32_t* counts, int32_t* voxels, colvo_stream_t stream) {
    COLVO_CHECK_ARG(workspace && pool && extract_workspace && points && counts && voxels, "colvo_fuse_write: null pointer argument");
    Grid G;
    COLVO_CHECK_ARG(grid_geom(ox, oy, oz, voxel_size, nx, ny, nz, G),
                    "colvo_fuse_write: bad grid origin (%g, %g, %g) voxel_size %g dims %d x %d x %d", (double)ox, (double)oy, (double)oz,
                    (double)voxel_size, nx, ny, nz);
    COLVO_CHECK_ARG(n_bricks > 0 && n_bricks < MAX_SLOTS && n_bricks <= total_bricks(G) && min_obs >= 1,
                    "colvo_fuse_write: bad grid: n_bricks %d (1 .. min(2^22 - 1, %d)), min_obs %d (>= 1)", n_bricks, total_bricks(G),
                    min_obs);
    COLVO_CHECK_ARG(n_rows > 0 && (long long)n_rows <= (long long)n_bricks * BRICK_VOX, "colvo_fuse_write: bad shape: n_rows %d (1 .. %lld)",
                    n_rows, (long long)n_bricks * BRICK_VOX);
    COLVO_CHECK_ARG(aligned16(workspace) && aligned16(pool) && aligned16(extract_workspace),
                    "colvo_fuse_write: workspaces and pool must be 16-byte aligned");
    const PlanWs p = plan_ws(const_cast<void*>(workspace), G);
    const ExtractWs e = extract_ws(const_cast<void*>(extract_workspace), n_bricks);
    colvo::launch(k_fuse_write, dim3(n_bricks), dim3(NT), 0, (hipStream_t)stream, static_cast<const Record*>(pool), p.list, e.rows,
                  min_obs, G, voxel_size, n_rows, points, colors, counts, voxels);
    COLVO_CHECK_LAUNCH("k_fuse_write");
    return 0;
}
