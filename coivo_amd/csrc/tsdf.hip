// tsdf.hip -- depth maps + trajectory -> a truncated signed distance volume, and the volume -> an indexed triangle mesh by surface
// nets.  Contract: include/colvo.h (colvo_tsdf_*); replica: tests/tsdf_ref.py.
//
//   plan        k_tsdf_mark: one thread per walked sample marks the 8x8x8 bricks of 2 T + 3 points along its ray (the fusion's pinned
//               locate); the marks are numbered in ascending brick order by the ordered scan of csrc/scan.hip.
//   integrate   k_tsdf_integrate: one workgroup per allocated brick, a thread owns two voxels for the whole call and keeps their
//               integer sums in registers -- no atomics, no cleared pool.  Frames are tested 64 at a time against the brick (one lane
//               per frame) and only the survivors are walked.
//   mesh        count / scan / write twice: active cells -> vertices (and the cell -> vertex table), then grid edges -> quads.
//
// All sums are integers and every output row has a position fixed by the scans, so a call's bits do not depend on scheduling, on the
// stream or on the order of the frames.  What decides a brick, a pixel or a quantum is float32 with every operation individually
// rounded; the vertices are float64 in the association the contract writes -- contraction is off for this whole file.
//
// No overflow: a voxel receives at most one observation per frame, N <= 65535 and |q| <= 4096, so |sum q| <= 65535 * 4096 < 2.7e8
// < 2^31 and a colour sum is at most 65535 * 255 < 1.7e7: the sums are plain int32 and there is no overflow flag.
#include "scene.h"
#include "tuning.h"

#pragma clang fp contract(off)

#include "voxel_grid.h"                    // Grid, Walk, the pinned locate, colour_quantum
#include "render_common.h"                 // the pinned camera point (cam_point) and Z_EPS, shared with the renderers

namespace colvo {
namespace {

using namespace voxel_grid;
using render_common::Z_EPS;

constexpr int MAX_SLOTS = 1 << 22;         // n_bricks below this: a pool index (slot * 512 + local) stays below 2^31
constexpr int COUNTER_LINES = 256;         // k_tsdf_mark's sample counters: this many pairs,
constexpr int COUNTER_PITCH = 16;          // ... one per 64-byte line (csrc/fuse.hip measured why)
constexpr int MAX_T = 7;                   // a band of T + 1 <= 8 voxels never skips a brick
constexpr int FRAME_GROUP = 64;            // frames culled at a time, one lane each: 64 Cams of 64 bytes = 4 KiB of LDS
constexpr int HALO = BRICK + 1;            // a brick's cells reach one voxel into its +x / +y / +z neighbours
constexpr int HALO_VOX = HALO * HALO * HALO;
constexpr float Q_ONE = 4096.0f;
static_assert(sizeof(Cam) == 64, "a Cam is 64 bytes");

struct Tsdf {                              // the truncation, as the host computed it in float32
    float vs, trunc, inv_trunc;
};

// ---- plan ------------------------------------------------------------------------------------------------------------------- //
// grid (blocks_per_frame, N).  The sample's own point (k = 0) decides the outside count.
__global__ __launch_bounds__(NT) void k_tsdf_mark(const float* __restrict__ depth, const float* __restrict__ K,
                                                  const float* __restrict__ M, Walk w, Grid G, float vs, float max_depth, int T,
                                                  int32_t* __restrict__ brick_table, int32_t* __restrict__ counters) {
    __shared__ int sm[NT / 64][2];
    const int b = blockIdx.y;
    int u = 0, v = 0;
    const bool in = walk_pixel(w, u, v);
    const float d = in ? depth[((size_t)b * w.H + v) * w.W + u] : 0.0f;
    const bool kept = in && valid_depth(d, max_depth);
    const Cam c = load_cam(K, M, b);
    bool inside0 = false;
    for (int k = -(T + 1); k <= T + 1; ++k) {
        const float dk = d + (float)k * vs;
        Voxel vx;
        const bool inside = kept && dk > 0.0f && locate(c, G, (float)u, (float)v, dk, vx);
        if (inside) brick_table[vx.brick] = 1;                   // idempotent same-value store
        if (k == 0) inside0 = inside;
    }
    const int n[2] = {(int)__popcll(__ballot(kept)), (int)__popcll(__ballot(kept && !inside0))};
    const unsigned line = (blockIdx.y * gridDim.x + blockIdx.x) % COUNTER_LINES;
    striped_counter_add(n, sm, counters + line * COUNTER_PITCH);
}

// one workgroup: stats[0], stats[1] = sums over the counter lines
__global__ __launch_bounds__(NT) void k_tsdf_stats(const int32_t* __restrict__ counters, int32_t* __restrict__ stats) {
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

// ---- integrate -------------------------------------------------------------------------------------------------------------- //
__device__ __forceinline__ Cam load_cam_lane(const float* __restrict__ K, const float* __restrict__ M, int f) {     // per lane
    Cam c;
    const float* k = K + (size_t)f * 9;
    const float* m = M + (size_t)f * 16;
    c.fx = k[0]; c.fy = k[4]; c.cx = k[2]; c.cy = k[5];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c.r[i * 3 + j] = m[i * 4 + j];
        c.t[i] = m[i * 4 + 3];
    }
    return c;
}

// Does frame `c` provably add nothing to any voxel of the brick whose voxel centres lie in the box C -/+ h (h = 3.5 voxels per axis)?
//
// A voxel contributes only with  Z_EPS < Pz,  Pz <= d + trunc < max_depth + trunc,  and a nearest pixel inside the image:
// -0.5 <= x < W - 0.5 for x = fx Px / Pz + cx, and y likewise.  Its camera point is P = Pc + dP with Pc the centre's and
// |dP_a| <= s_a = h (|r_0a| + |r_1a| + |r_2a|), the image of the box under r^T -- for any matrix r; for a rotation s_a <= sqrt(3) h,
// the radius of the box's bounding sphere, so the test is never looser than the sphere's.  The float32 evaluation of P (six products,
// five sums of terms bounded by (|C|_1 + |t|_1 + 3 h) max|r|) errs by less than 16 u of that, u = 2^-24: E_a = 2^-20 (|C|_1 + |t|_1
// + 3 h) (|r_0a| + |r_1a| + |r_2a|) is added to s_a, for the centre's own evaluation and the voxel's together.
//   depth slab   culled if Pc_z + s_z < Z_EPS or Pc_z - s_z > (max_depth + trunc) (1 + 2^-20)  (the factor: the roundings of the sum
//                and of sdf = d - Pz).
//   image        with Pz > 0 and fx > 0, x >= -0.5 - g  <=>  fx Px + (cx + 0.5 + g) Pz >= 0: a half-space through the camera centre.
//                Its left side over the box is at most L = fx Pc_x + a Pc_z + fx s_x + |a| s_z; culled if L < -tol, tol = 2^-20 times
//                the sum of the four terms' magnitudes (four roundings of at most u each).  Right, top and bottom likewise.  The
//                pixel margin g = 1 + 2^-18 (|cx| + W) covers the voxel's own float32 evaluation of x, which errs by less than
//                4 u (|x - cx| + |cx|) < g near the image border and is monotone far from it.  fx <= 0 or fy <= 0: not culled.
// Every comparison culls on `true` only, so a NaN anywhere keeps the frame: the cull is conservative by construction, and since the
// sums are integers the result does not depend on which of the non-contributing frames were skipped.
__device__ __forceinline__ bool cull_frame(const Cam& c, const float (&C)[3], float h, int H, int W, float far) {
    const float q0 = C[0] - c.t[0], q1 = C[1] - c.t[1], q2 = C[2] - c.t[2];
    const float Px = (c.r[0] * q0 + c.r[3] * q1) + c.r[6] * q2;
    const float Py = (c.r[1] * q0 + c.r[4] * q1) + c.r[7] * q2;
    const float Pz = (c.r[2] * q0 + c.r[5] * q1) + c.r[8] * q2;
    const float mag = 0x1p-20f * ((((fabsf(C[0]) + fabsf(C[1])) + fabsf(C[2])) + ((fabsf(c.t[0]) + fabsf(c.t[1])) + fabsf(c.t[2]))) + 3.0f * h);
    const float nx = (fabsf(c.r[0]) + fabsf(c.r[3])) + fabsf(c.r[6]);
    const float ny = (fabsf(c.r[1]) + fabsf(c.r[4])) + fabsf(c.r[7]);
    const float nz = (fabsf(c.r[2]) + fabsf(c.r[5])) + fabsf(c.r[8]);
    const float sx = (h + mag) * nx, sy = (h + mag) * ny, sz = (h + mag) * nz;
    if (Pz + sz < Z_EPS) return true;
    if (Pz - sz > far * (1.0f + 0x1p-20f)) return true;
    if (!(c.fx > 0.0f) || !(c.fy > 0.0f)) return false;
    const float gx = 1.0f + 0x1p-18f * (fabsf(c.cx) + (float)W), gy = 1.0f + 0x1p-18f * (fabsf(c.cy) + (float)H);
    {
        const float a = c.cx + 0.5f + gx, b = ((float)W - 0.5f + gx) - c.cx;
        const float fs = c.fx * sx;
        const float left = ((c.fx * Px + a * Pz) + fs) + fabsf(a) * sz;
        if (left < -0x1p-20f * (((fabsf(c.fx * Px) + fabsf(a * Pz)) + fs) + fabsf(a) * sz)) return true;
        const float right = ((c.fx * Px - b * Pz) - fs) - fabsf(b) * sz;
        if (right > 0x1p-20f * (((fabsf(c.fx * Px) + fabsf(b * Pz)) + fs) + fabsf(b) * sz)) return true;
    }
    {
        const float a = c.cy + 0.5f + gy, b = ((float)H - 0.5f + gy) - c.cy;
        const float fs = c.fy * sy;
        const float top = ((c.fy * Py + a * Pz) + fs) + fabsf(a) * sz;
        if (top < -0x1p-20f * (((fabsf(c.fy * Py) + fabsf(a * Pz)) + fs) + fabsf(a) * sz)) return true;
        const float bottom = ((c.fy * Py - b * Pz) - fs) - fabsf(b) * sz;
        if (bottom > 0x1p-20f * (((fabsf(c.fy * Py) + fabsf(b * Pz)) + fs) + fabsf(b) * sz)) return true;
    }
    return false;
}

// grid n_bricks.  pool[slot * 512 + local] = (sum q, n); csum[...] = (sum r, sum g, sum b, 0) with colours.  survivors (or NULL):
// frames the brick walked, for tools/bench_tsdf.py.
__global__ __launch_bounds__(NT) void k_tsdf_integrate(const float* __restrict__ depth, const float* __restrict__ colors,
                                                       const float* __restrict__ K, const float* __restrict__ M, int N, int H, int W,
                                                       Grid G, Tsdf t, float max_depth, const int32_t* __restrict__ brick_list,
                                                       int2* __restrict__ pool, int4* __restrict__ csum, int cull,
                                                       int32_t* __restrict__ survivors) {
    __shared__ Cam cams[FRAME_GROUP];
    __shared__ unsigned long long s_mask;
    const int slot = blockIdx.x;
    const int brick = brick_list[slot];
    const int b3[3] = {brick % G.nb[0], (brick / G.nb[0]) % G.nb[1], brick / (G.nb[0] * G.nb[1])};
    float centre[3];                                             // of the brick's voxel centres: o + (8 b + 4) vs
#pragma unroll
    for (int a = 0; a < 3; ++a) centre[a] = G.o[a] + ((float)(b3[a] * BRICK) + 4.0f) * t.vs;
    constexpr int PER = BRICK_VOX / NT;
    float vc[PER][3];                                            // this thread's voxel centres
    int sq[PER], n[PER], sc[PER][3];
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int local = r * NT + threadIdx.x;
        const int l3[3] = {local & 7, (local >> 3) & 7, local >> 6};
#pragma unroll
        for (int a = 0; a < 3; ++a) vc[r][a] = G.o[a] + ((float)(b3[a] * BRICK + l3[a]) + 0.5f) * t.vs;
        sq[r] = n[r] = sc[r][0] = sc[r][1] = sc[r][2] = 0;
    }
    const size_t HW = (size_t)H * W;
    const float Wf = (float)W, Hf = (float)H;
    const render_common::Geom no_far{0, 0, 0, 0, 0, 0.0f, __builtin_inff()};
    int walked = 0;
    for (int f0 = 0; f0 < N; f0 += FRAME_GROUP) {
        if (threadIdx.x < FRAME_GROUP) {                         // wave 0: one lane per frame of the group
            const int f = f0 + threadIdx.x;
            bool keep = f < N;
            if (keep) {
                const Cam c = load_cam_lane(K, M, f);
                cams[threadIdx.x] = c;
                if (cull) keep = !cull_frame(c, centre, 3.5f * t.vs, H, W, max_depth + t.trunc);
            }
            const unsigned long long m = __ballot(keep);
            if (threadIdx.x == 0) s_mask = m;
        }
        __syncthreads();
        unsigned long long mask = s_mask;
        mask = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(mask >> 32)) << 32) |
               (unsigned)__builtin_amdgcn_readfirstlane((int)mask);
        walked += __popcll(mask);
        while (mask != 0ull) {
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            const int f = f0 + j;
            Cam c;
            c.fx = uniform_f(cams[j].fx); c.fy = uniform_f(cams[j].fy); c.cx = uniform_f(cams[j].cx); c.cy = uniform_f(cams[j].cy);
#pragma unroll
            for (int i = 0; i < 9; ++i) c.r[i] = uniform_f(cams[j].r[i]);
#pragma unroll
            for (int i = 0; i < 3; ++i) c.t[i] = uniform_f(cams[j].t[i]);
            const float* dmap = depth + (size_t)f * HW;
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const render_common::CamPoint p = render_common::cam_point(c, no_far, true, vc[r][0], vc[r][1], vc[r][2]);
                const float x = (c.fx * p.Px) / p.Pz + c.cx;
                const float y = (c.fy * p.Py) / p.Pz + c.cy;
                const float xf = floorf(x + 0.5f), yf = floorf(y + 0.5f);
                const bool on = (int)(p.Pz > Z_EPS) & (int)(xf >= 0.0f) & (int)(xf < Wf) & (int)(yf >= 0.0f) & (int)(yf < Hf);      // NaN fails
                if (!on) continue;
                const size_t px = (size_t)(int)yf * W + (int)xf;
                const float d = dmap[px];
                if (!valid_depth(d, max_depth)) continue;
                const float sdf = d - p.Pz;
                if (sdf < -t.trunc) continue;                    // hidden behind the surface
                const float tt = fminf(sdf, t.trunc) * t.inv_trunc;
                sq[r] += (int)rintf(tt * Q_ONE);
                n[r] += 1;
                if (colors != nullptr) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) sc[r][k] += (int)colour_quantum(colors[((size_t)f * 3 + k) * HW + px]);
                }
            }
        }
        __syncthreads();                                         // before the next group overwrites the cameras
    }
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const size_t row = (size_t)slot * BRICK_VOX + r * NT + threadIdx.x;
        pool[row] = make_int2(sq[r], n[r]);
        if (csum != nullptr) csum[row] = make_int4(sc[r][0], sc[r][1], sc[r][2], 0);
    }
    if (survivors != nullptr && threadIdx.x == 0) survivors[slot] = walked;
}

// ---- mesh: cells and vertices ------------------------------------------------------------------------------------------------- //
// pool row of voxel (x, y, z): -1 outside the grid or in a brick that is not allocated
__device__ __forceinline__ int pool_row(const Grid& G, const int32_t* __restrict__ table, int n_bricks, int x, int y, int z) {
    if ((unsigned)x >= (unsigned)G.n[0] || (unsigned)y >= (unsigned)G.n[1] || (unsigned)z >= (unsigned)G.n[2]) return -1;
    const int slot = table[((z >> 3) * G.nb[1] + (y >> 3)) * G.nb[0] + (x >> 3)];
    if (slot < 0 || slot >= n_bricks) return -1;
    return slot * BRICK_VOX + (((z & 7) * BRICK + (y & 7)) * BRICK + (x & 7));
}

struct Halo {                              // the brick's 9 x 9 x 9 corners: sum q, n (0: not observed), pool row (-1: not observed)
    int sq[HALO_VOX], n[HALO_VOX], row[HALO_VOX];
};

__device__ __forceinline__ void load_halo(const int2* __restrict__ pool, const int32_t* __restrict__ table, int n_bricks, const Grid& G,
                                          const int (&b3)[3], int min_obs, Halo& h) {
    for (int i = threadIdx.x; i < HALO_VOX; i += NT) {
        const int x = i % HALO, y = (i / HALO) % HALO, z = i / (HALO * HALO);
        const int row = pool_row(G, table, n_bricks, b3[0] * BRICK + x, b3[1] * BRICK + y, b3[2] * BRICK + z);
        int2 rec = make_int2(0, 0);
        if (row >= 0) rec = pool[row];
        const bool obs = row >= 0 && rec.y >= min_obs;           // (min_obs >= 1)
        h.sq[i] = obs ? rec.x : 0;
        h.n[i] = obs ? rec.y : 0;
        h.row[i] = obs ? row : -1;
    }
    __syncthreads();
}

__device__ __forceinline__ int halo_index(int local, int corner) {
    const int x = (local & 7) + (corner & 1), y = ((local >> 3) & 7) + ((corner >> 1) & 1), z = (local >> 6) + (corner >> 2);
    return (z * HALO + y) * HALO + x;
}

// a cell: bit 0 active (eight observed corners, mixed signs), bit 1 open (mixed signs among the observed, one or more not observed)
__device__ __forceinline__ int classify(const Halo& h, int local) {
    int n_obs = 0, n_neg = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int i = halo_index(local, c);
        const bool obs = h.n[i] > 0;
        n_obs += obs;
        n_neg += obs && h.sq[i] < 0;
    }
    const bool mixed = n_neg > 0 && n_neg < n_obs;
    return (int)(mixed && n_obs == 8) | ((int)(mixed && n_obs < 8) << 1);
}

struct Bricks {                            // what every mesh kernel gets
    const int2* pool;
    const int32_t* table;
    const int32_t* list;
    int n_bricks;
    Grid G;
};

__device__ __forceinline__ void brick_coords(const Bricks& B, int slot, int (&b3)[3]) {
    const int brick = B.list[slot];
    b3[0] = brick % B.G.nb[0];
    b3[1] = (brick / B.G.nb[0]) % B.G.nb[1];
    b3[2] = brick / (B.G.nb[0] * B.G.nb[1]);
}

// grid n_bricks: rows[slot] = active cells; open cells -> stats2[1]
__global__ __launch_bounds__(NT) void k_mesh_count(Bricks B, int min_obs, int32_t* __restrict__ rows, int32_t* __restrict__ stats2) {
    __shared__ Halo h;
    __shared__ int sm[NT / 64];
    __shared__ int sm2[NT / 64];
    int b3[3];
    brick_coords(B, blockIdx.x, b3);
    load_halo(B.pool, B.table, B.n_bricks, B.G, b3, min_obs, h);
    int n_act = 0, n_open = 0;
#pragma unroll
    for (int r = 0; r < BRICK_VOX / NT; ++r) {
        const int k = classify(h, r * NT + threadIdx.x);
        n_act += k & 1;
        n_open += k >> 1;
    }
    n_act = block_sum(n_act, sm);
    n_open = block_sum(n_open, sm2);
    if (threadIdx.x == 0) {
        rows[blockIdx.x] = n_act;
        if (n_open) atomicAdd(&stats2[1], n_open);
    }
}

// grid n_bricks: the brick's vertices, in local order, from offsets[slot] on; vid[slot * 512 + local] = the cell's vertex or -1
__global__ __launch_bounds__(NT) void k_mesh_vertices(Bricks B, const int4* __restrict__ csum, int min_obs,
                                                      const int32_t* __restrict__ offsets, float voxel_size, int n_vertices,
                                                      float* __restrict__ vertices, float* __restrict__ colors,
                                                      float* __restrict__ normals, int32_t* __restrict__ cells,
                                                      int32_t* __restrict__ vid) {
    __shared__ Halo h;
    __shared__ int wsum[BRICK_VOX / 64];
    const int slot = blockIdx.x;
    int b3[3];
    brick_coords(B, slot, b3);
    load_halo(B.pool, B.table, B.n_bricks, B.G, b3, min_obs, h);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    constexpr int PER = BRICK_VOX / NT;
    bool active[PER];
    unsigned long long mask[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        active[r] = classify(h, r * NT + threadIdx.x) & 1;
        mask[r] = __ballot(active[r]);
        if (lane == 0) wsum[r * (NT / 64) + wv] = __popcll(mask[r]);
    }
    __syncthreads();
    const double vs = (double)voxel_size;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int local = r * NT + threadIdx.x;
        int m = -1;
        if (active[r]) {
            m = offsets[slot] + __popcll(mask[r] & ((1ull << lane) - 1ull));
            for (int i = 0; i < r * (NT / 64) + wv; ++i) m += wsum[i];
            if (m >= n_vertices) m = -1;                         // (a min_obs other than the count's: never past the caller's buffers)
        }
        vid[(size_t)slot * BRICK_VOX + local] = m;
        if (m < 0) continue;
        double phi[8];
        bool in[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int i = halo_index(local, c);
            phi[c] = (double)h.sq[i] / (double)h.n[i];
            in[c] = h.sq[i] < 0;
        }
        // the 12 edges: per axis the two other coordinates run (0,0), (1,0), (0,1), (1,1), the lower axis fastest
        double sum[3] = {0.0, 0.0, 0.0}, grad[3] = {0.0, 0.0, 0.0};
        int crossings = 0;
#pragma unroll
        for (int axis = 0; axis < 3; ++axis) {
            const int o0 = axis == 0 ? 1 : 0, o1 = axis == 2 ? 1 : 2;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int a = ((p & 1) << o0) | ((p >> 1) << o1), b = a | (1 << axis);
                if (in[a] != in[b]) {
                    const double t = phi[a] / (phi[a] - phi[b]);
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) sum[ax] += ax == axis ? t : (double)((a >> ax) & 1);
                    ++crossings;
                }
                const double d = phi[b] - phi[a];
                grad[axis] = p == 0 ? d : grad[axis] + d;
            }
        }
        const int l3[3] = {local & 7, (local >> 3) & 7, local >> 6};
        const double dn = (double)crossings;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int idx = b3[a] * BRICK + l3[a];
            vertices[(size_t)m * 3 + a] = (float)((double)B.G.o[a] + (((double)idx + 0.5) + sum[a] / dn) * vs);
            cells[(size_t)m * 3 + a] = idx;
        }
        const double len = sqrt((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) normals[(size_t)m * 3 + a] = len > 0.0 ? (float)(grad[a] / len) : 0.0f;
        if (colors != nullptr) {
            double cs[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int i = halo_index(local, c);
                const int4 s = csum[h.row[i]];
                const double den = 255.0 * (double)h.n[i];
                cs[0] += (double)s.x / den;
                cs[1] += (double)s.y / den;
                cs[2] += (double)s.z / den;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) colors[(size_t)m * 3 + k] = (float)(cs[k] / 8.0);
        }
    }
}

// ---- mesh: faces ------------------------------------------------------------------------------------------------------------ //
// The quad of the grid edge from voxel v to v + e_axis: the vertices of the four cells around it, A = v - e_u - e_w, B = v - e_w,
// C = v, D = v - e_u with u = axis + 1, w = axis + 2 (cyclic): counter-clockwise seen from +axis.  It exists iff all four cells are
// active (which makes both ends observed) and the ends differ in sign; fwd: the owner is the inside end, the normal points along +axis.
struct Quad {
    int v[4];
    bool has, fwd;
};

__device__ __forceinline__ Quad quad_of(const Bricks& B, const int32_t* __restrict__ vid, const int (&x)[3], int axis, int own_vid, int own_sq) {
    Quad q;
    const int u = (axis + 1) % 3, w = (axis + 2) % 3;
    q.has = true;
    q.fwd = own_sq < 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int y[3] = {x[0], x[1], x[2]};
        if (k == 0 || k == 3) y[u] -= 1;
        if (k == 0 || k == 1) y[w] -= 1;
        int v = own_vid;
        if (k != 2) {
            const int row = q.has ? pool_row(B.G, B.table, B.n_bricks, y[0], y[1], y[2]) : -1;
            v = row >= 0 ? vid[row] : -1;
        }
        q.v[k] = v;
        q.has = q.has && v >= 0;
    }
    if (q.has) {
        int y[3] = {x[0], x[1], x[2]};
        y[axis] += 1;
        const int far = pool_row(B.G, B.table, B.n_bricks, y[0], y[1], y[2]);
        q.has = far >= 0 && (B.pool[far].x < 0) != q.fwd;
    }
    return q;
}

// grid n_bricks.  WRITE = false: rows[slot] = triangles the brick's voxels own.  WRITE = true: the triangles, in (local, axis) order,
// from offsets[slot] on.
template <bool WRITE>
__global__ __launch_bounds__(NT) void k_mesh_faces(Bricks B, const int32_t* __restrict__ vid, int32_t* __restrict__ rows, int n_faces,
                                                   int32_t* __restrict__ faces) {
    __shared__ int sm[NT / 64];
    __shared__ int wsum[BRICK_VOX / 64];
    const int slot = blockIdx.x;
    int b3[3];
    brick_coords(B, slot, b3);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    constexpr int PER = BRICK_VOX / NT;
    Quad q[PER][3];
    unsigned long long mask[PER][3];
    int total = 0;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int local = r * NT + threadIdx.x;
        const size_t row = (size_t)slot * BRICK_VOX + local;
        const int own_vid = vid[row];
        const int x[3] = {b3[0] * BRICK + (local & 7), b3[1] * BRICK + ((local >> 3) & 7), b3[2] * BRICK + (local >> 6)};
        const int own_sq = own_vid >= 0 ? B.pool[row].x : 0;
        int wave_quads = 0;
#pragma unroll
        for (int axis = 0; axis < 3; ++axis) {
            q[r][axis].has = false;
            if (own_vid >= 0) q[r][axis] = quad_of(B, vid, x, axis, own_vid, own_sq);
            mask[r][axis] = __ballot(q[r][axis].has);
            wave_quads += __popcll(mask[r][axis]);
            total += q[r][axis].has;
        }
        if (WRITE && lane == 0) wsum[r * (NT / 64) + wv] = wave_quads;
    }
    if (!WRITE) {
        total = block_sum(total, sm);
        if (threadIdx.x == 0) rows[slot] = 2 * total;
        return;
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        int m = 0;
        for (int i = 0; i < r * (NT / 64) + wv; ++i) m += wsum[i];
        m += (__popcll(mask[r][0] & below) + __popcll(mask[r][1] & below)) + __popcll(mask[r][2] & below);
        m = rows[slot] + 2 * m;
#pragma unroll
        for (int axis = 0; axis < 3; ++axis) {
            const Quad& f = q[r][axis];
            if (!f.has) continue;
            if (m + 1 < n_faces) {                               // (never past the caller's buffer)
                int32_t* o = faces + (size_t)m * 3;
                o[0] = f.v[0]; o[1] = f.fwd ? f.v[1] : f.v[2]; o[2] = f.fwd ? f.v[2] : f.v[1];
                o[3] = f.v[0]; o[4] = f.fwd ? f.v[2] : f.v[3]; o[5] = f.fwd ? f.v[3] : f.v[2];
            }
            m += 2;
        }
    }
}

// ---- host side: geometry and scratch layouts -------------------------------------------------------------------------------- //
struct PlanWs {                            // sample counters, chunk sums of the brick table
    int32_t* counters;
    int32_t* sums;
    size_t bytes;
};

PlanWs plan_ws(void* base, const Grid& G) {
    Carver c(base);
    PlanWs p;
    p.counters = c.take<int32_t>((size_t)COUNTER_LINES * COUNTER_PITCH);
    p.sums = c.take<int32_t>(scan_chunks(total_bricks(G)));
    p.bytes = c.bytes();
    return p;
}

struct MeshWs {                            // vertices per brick and triangles per brick (offsets after their scans), chunk sums of each
    int32_t* rows;
    int32_t* sums;
    int32_t* face_rows;
    int32_t* face_sums;
    size_t bytes;
};

MeshWs mesh_ws(void* base, int n_bricks) {
    Carver c(base);
    MeshWs m;
    m.rows = c.take<int32_t>(n_bricks);
    m.sums = c.take<int32_t>(scan_chunks(n_bricks));
    m.face_rows = c.take<int32_t>(n_bricks);
    m.face_sums = c.take<int32_t>(scan_chunks(n_bricks));
    m.bytes = c.bytes();
    return m;
}

bool tsdf_geom(float voxel_size, int T, Tsdf& t) {
    if (T < 1 || T > MAX_T) return false;
    t.vs = voxel_size;
    t.trunc = (float)T * voxel_size;
    t.inv_trunc = 1.0f / t.trunc;
    return t.trunc > 0.0f && t.trunc < __builtin_inff() && t.inv_trunc > 0.0f && t.inv_trunc < __builtin_inff();
}

}  // namespace
}  // namespace colvo

using namespace colvo;

#define TSDF_CHECK_GRID(who)                                                                                                          \
    COLVO_CHECK_ARG(grid_geom(ox, oy, oz, voxel_size, nx, ny, nz, G), who ": bad grid origin (%g, %g, %g) voxel_size %g dims %d x %d x %d", \
                    (double)ox, (double)oy, (double)oz, (double)voxel_size, nx, ny, nz)
#define TSDF_CHECK_BRICKS(who)                                                                                    \
    COLVO_CHECK_ARG(n_bricks > 0 && n_bricks < MAX_SLOTS && n_bricks <= total_bricks(G),                          \
                    who ": bad grid: n_bricks %d (1 .. min(2^22 - 1, %d))", n_bricks, total_bricks(G))

extern "C" size_t colvo_tsdf_plan_scratch_bytes(int N, int H, int W, int stride, int nx, int ny, int nz) {
    Walk w;
    Grid G;
    if (!walk_geom(N, H, W, stride, w) || !grid_dims(nx, ny, nz, G)) return 0;
    return plan_ws(nullptr, G).bytes;
}

extern "C" int colvo_tsdf_plan(const float* depths, const float* K, const float* cam2world, int N, int H, int W, int stride,
                               float max_depth, float ox, float oy, float oz, float voxel_size, int nx, int ny, int nz, int T,
                               void* scratch, int32_t* table, int32_t* brick_list, int32_t* stats, colvo_stream_t stream) {
    COLVO_CHECK_ARG(depths && K && cam2world && scratch && table && brick_list && stats, "colvo_tsdf_plan: null pointer argument");
    Walk w;
    Grid G;
    Tsdf t;
    COLVO_CHECK_ARG(walk_geom(N, H, W, stride, w), "colvo_tsdf_plan: bad shape N=%d H=%d W=%d stride=%d", N, H, W, stride);
    TSDF_CHECK_GRID("colvo_tsdf_plan");
    COLVO_CHECK_ARG(tsdf_geom(voxel_size, T, t), "colvo_tsdf_plan: bad truncation: T = %d voxels (1 .. %d)", T, MAX_T);
    COLVO_CHECK_ARG(aligned16(scratch) && aligned16(table) && aligned16(brick_list),
                    "colvo_tsdf_plan: scratch, table and brick_list must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const PlanWs p = plan_ws(scratch, G);
    const int tb = total_bricks(G);
    COLVO_CHECK_HIP(hipMemsetAsync(p.counters, 0, (size_t)COUNTER_LINES * COUNTER_PITCH * 4, s), "colvo_tsdf_plan");
    COLVO_CHECK_HIP(hipMemsetAsync(table, 0, (size_t)tb * 4, s), "colvo_tsdf_plan");
    colvo::launch(k_tsdf_mark, dim3(w.blocks_per_frame, N), dim3(NT), 0, s, depths, K, cam2world, w, G, voxel_size, max_depth, T, table,
                  p.counters);
    COLVO_CHECK_LAUNCH("k_tsdf_mark");
    colvo::launch(k_tsdf_stats, dim3(1), dim3(NT), 0, s, p.counters, stats);
    COLVO_CHECK_LAUNCH("k_tsdf_stats");
    return scan_exclusive(Scan{table, tb, nullptr, p.sums, stats + 2, brick_list, tb < MAX_SLOTS ? tb : MAX_SLOTS}, s);
}

extern "C" int colvo_tsdf_integrate(const float* depths, const float* colors, const float* K, const float* cam2world, int N, int H,
                                    int W, float max_depth, float ox, float oy, float oz, float voxel_size, int nx, int ny, int nz,
                                    int T, const int32_t* brick_list, int n_bricks, void* pool, void* color_sums, int32_t* survivors,
                                    colvo_stream_t stream) {
    COLVO_CHECK_ARG(depths && K && cam2world && brick_list && pool && (!colors == !color_sums),
                    "colvo_tsdf_integrate: null pointer argument (colors and color_sums go together)");
    StridedFrame fr;
    Grid G;
    Tsdf t;
    COLVO_CHECK_ARG(strided_frame(N, H, W, 1, fr), "colvo_tsdf_integrate: bad shape N=%d H=%d W=%d", N, H, W);
    TSDF_CHECK_GRID("colvo_tsdf_integrate");
    TSDF_CHECK_BRICKS("colvo_tsdf_integrate");
    COLVO_CHECK_ARG(tsdf_geom(voxel_size, T, t), "colvo_tsdf_integrate: bad truncation: T = %d voxels (1 .. %d)", T, MAX_T);
    COLVO_CHECK_ARG(aligned16(pool) && aligned16(color_sums) && aligned16(brick_list),
                    "colvo_tsdf_integrate: pool, color_sums and brick_list must be 16-byte aligned");
    colvo::launch(k_tsdf_integrate, dim3(n_bricks), dim3(NT), 0, (hipStream_t)stream, depths, colors, K, cam2world, N, H, W, G, t,
                  max_depth, brick_list, static_cast<int2*>(pool), static_cast<int4*>(color_sums), (int)(TUNE(tsdf_cull) != 0), survivors);
    COLVO_CHECK_LAUNCH("k_tsdf_integrate");
    return 0;
}

extern "C" size_t colvo_tsdf_mesh_scratch_bytes(int n_bricks) {
    if (n_bricks <= 0 || n_bricks >= MAX_SLOTS) return 0;
    return mesh_ws(nullptr, n_bricks).bytes;
}

extern "C" int colvo_tsdf_mesh_count(const void* pool, const int32_t* table, const int32_t* brick_list, int n_bricks, int min_obs,
                                     int nx, int ny, int nz, void* scratch, int32_t* stats2, colvo_stream_t stream) {
    COLVO_CHECK_ARG(pool && table && brick_list && scratch && stats2, "colvo_tsdf_mesh_count: null pointer argument");
    Grid G{};
    COLVO_CHECK_ARG(grid_dims(nx, ny, nz, G), "colvo_tsdf_mesh_count: bad grid dims %d x %d x %d", nx, ny, nz);
    TSDF_CHECK_BRICKS("colvo_tsdf_mesh_count");
    COLVO_CHECK_ARG(min_obs >= 1, "colvo_tsdf_mesh_count: min_obs %d (>= 1)", min_obs);
    COLVO_CHECK_ARG(aligned16(pool) && aligned16(scratch), "colvo_tsdf_mesh_count: pool and scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const MeshWs m = mesh_ws(scratch, n_bricks);
    COLVO_CHECK_HIP(hipMemsetAsync(stats2, 0, 2 * sizeof(int32_t), s), "colvo_tsdf_mesh_count");
    const Bricks B{static_cast<const int2*>(pool), table, brick_list, n_bricks, G};
    colvo::launch(k_mesh_count, dim3(n_bricks), dim3(NT), 0, s, B, min_obs, m.rows, stats2);
    COLVO_CHECK_LAUNCH("k_mesh_count");
    return scan_exclusive(Scan{m.rows, n_bricks, nullptr, m.sums, stats2, nullptr, 0}, s);
}

extern "C" int colvo_tsdf_mesh_vertices(const void* pool, const void* color_sums, const int32_t* table, const int32_t* brick_list,
                                        int n_bricks, int min_obs, float ox, float oy, float oz, float voxel_size, int nx, int ny,
                                        int nz, void* scratch, int n_vertices, float* vertices, float* colors, float* normals,
                                        int32_t* cells, int32_t* vertex_ids, int32_t* n_faces, colvo_stream_t stream) {
    COLVO_CHECK_ARG(pool && table && brick_list && scratch && vertices && normals && cells && vertex_ids && n_faces &&
                        (!colors == !color_sums),
                    "colvo_tsdf_mesh_vertices: null pointer argument (colors and color_sums go together)");
    Grid G;
    TSDF_CHECK_GRID("colvo_tsdf_mesh_vertices");
    TSDF_CHECK_BRICKS("colvo_tsdf_mesh_vertices");
    COLVO_CHECK_ARG(min_obs >= 1, "colvo_tsdf_mesh_vertices: min_obs %d (>= 1)", min_obs);
    COLVO_CHECK_ARG(n_vertices > 0 && (long long)n_vertices <= (long long)n_bricks * BRICK_VOX,
                    "colvo_tsdf_mesh_vertices: bad shape: n_vertices %d (1 .. %lld)", n_vertices, (long long)n_bricks * BRICK_VOX);
    COLVO_CHECK_ARG(aligned16(pool) && aligned16(color_sums) && aligned16(scratch),
                    "colvo_tsdf_mesh_vertices: pool, color_sums and scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const MeshWs m = mesh_ws(scratch, n_bricks);
    const Bricks B{static_cast<const int2*>(pool), table, brick_list, n_bricks, G};
    colvo::launch(k_mesh_vertices, dim3(n_bricks), dim3(NT), 0, s, B, static_cast<const int4*>(color_sums), min_obs, m.rows, voxel_size,
                  n_vertices, vertices, colors, normals, cells, vertex_ids);
    COLVO_CHECK_LAUNCH("k_mesh_vertices");
    colvo::launch(k_mesh_faces<false>, dim3(n_bricks), dim3(NT), 0, s, B, vertex_ids, m.face_rows, 0, (int32_t*)nullptr);
    COLVO_CHECK_LAUNCH("k_mesh_faces");
    return scan_exclusive(Scan{m.face_rows, n_bricks, nullptr, m.face_sums, n_faces, nullptr, 0}, s);
}

extern "C" int colvo_tsdf_mesh_faces(const void* pool, const int32_t* table, const int32_t* brick_list, int n_bricks, int nx, int ny,
                                     int nz, const void* scratch, const int32_t* vertex_ids, int n_faces, int32_t* faces,
                                     colvo_stream_t stream) {
    COLVO_CHECK_ARG(pool && table && brick_list && scratch && vertex_ids && faces, "colvo_tsdf_mesh_faces: null pointer argument");
    Grid G{};
    COLVO_CHECK_ARG(grid_dims(nx, ny, nz, G), "colvo_tsdf_mesh_faces: bad grid dims %d x %d x %d", nx, ny, nz);
    TSDF_CHECK_BRICKS("colvo_tsdf_mesh_faces");
    COLVO_CHECK_ARG(n_faces > 0 && n_faces % 2 == 0 && (long long)n_faces <= 6ll * n_bricks * BRICK_VOX,
                    "colvo_tsdf_mesh_faces: bad shape: n_faces %d (even, 2 .. %lld)", n_faces, 6ll * n_bricks * BRICK_VOX);
    COLVO_CHECK_ARG(aligned16(pool) && aligned16(scratch), "colvo_tsdf_mesh_faces: pool and scratch must be 16-byte aligned");
    const MeshWs m = mesh_ws(const_cast<void*>(scratch), n_bricks);
    const Bricks B{static_cast<const int2*>(pool), table, brick_list, n_bricks, G};
    colvo::launch(k_mesh_faces<true>, dim3(n_bricks), dim3(NT), 0, (hipStream_t)stream, B, vertex_ids, m.face_rows, n_faces, faces);
    COLVO_CHECK_LAUNCH("k_mesh_faces");
    return 0;
}
