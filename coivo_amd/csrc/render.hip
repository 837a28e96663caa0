// render.hip -- a point cloud drawn into camera views: every point projected into every requested camera as a small
// screen-aligned square, the nearest kept per pixel.  Contract: include/colvo.h (colvo_render_*).
//
//   k_render_clear    the key buffer to all-ones (two keys per thread, one 16-byte store), the per-frame counter lines to zero.
//   k_render_splat    one point per thread, held in registers, over a group of FRAME_GROUP frames: the cloud is read once per group, a
//                     frame's camera is wave-uniform (scalar loads).  A wave with no lane in front of the camera leaves the frame
//                     after the three products; the footprint loop runs only in the lanes that draw.  Per covered pixel one 64-bit
//                     atomic minimum without a return value on the packed key (depth bits, point index), as csrc/cloud.hip packs its
//                     keys; optionally behind a relaxed load that skips it (tuning.h render_load_first).  The front / drawn / clipped
//                     counts are ballots and go through striped_counter_add, whose LDS rows alternate between two sets so that one
//                     barrier per frame is enough.
//   k_render_resolve  one thread per pixel: key -> depth, index, gathered colour; covered pixels counted by ballot.
//   k_render_stats    one wave per frame: the counter lines summed into out_stats[N][4].
//
// Every float32 operation is individually rounded -- contraction is off for this whole file --, the minimum is an integer minimum and
// every sum is an integer: a call's bits do not depend on scheduling or on the stream.
#include "scene.h"
#include "tuning.h"

#pragma clang fp contract(off)

namespace colvo {
namespace {

constexpr int NT = 256;
constexpr int FRAME_GROUP = 16;            // frames a workgroup of the splat kernel walks with its 256 points in registers
constexpr int MAX_SPLAT = 32;
constexpr int N_STATS = 4;                 // front, drawn, clipped, covered
constexpr int MAX_LINES = 8;               // counter lines per frame,
constexpr int LINE_INTS = 16;              // ... 64 bytes each
constexpr float Z_EPS = 1e-3f;             // spec: Z_EPS
constexpr unsigned long long EMPTY = ~0ull;

struct Geom {
    int M, N, H, W, max_splat;
    float radius, max_depth;
};

// grid ceil(max(pairs + 1, n_counters) / NT); total = N * H * W keys, pairs = total / 2
__global__ __launch_bounds__(NT) void k_render_clear(unsigned long long* __restrict__ keys, long long total, int32_t* __restrict__ counters,
                                                     int n_counters) {
    const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
    const long long pairs = total >> 1;
    if (idx < pairs) reinterpret_cast<ulonglong2*>(keys)[idx] = make_ulonglong2(EMPTY, EMPTY);
    if (idx == pairs && (total & 1)) keys[total - 1] = EMPTY;
    if (idx < n_counters) counters[idx] = 0;
}

// grid (ceil(M / NT), ceil(N / FRAME_GROUP))
template <bool LOAD_FIRST>
__global__ __launch_bounds__(NT) void k_render_splat(const float* __restrict__ points, const float* __restrict__ K,
                                                     const float* __restrict__ M, Geom g, unsigned long long* __restrict__ keys,
                                                     int32_t* __restrict__ counters) {
    __shared__ int sm_stats[2][NT / 64][3];
    const int i = blockIdx.x * NT + threadIdx.x;                 // M < 2^31 and the grid covers M rounded up to NT <= 2^31: no overflow
    const bool live = i < g.M;
    float X0 = 0.0f, X1 = 0.0f, X2 = 0.0f;
    if (live) {
        const float* p = points + (size_t)i * 3;
        X0 = p[0];
        X1 = p[1];
        X2 = p[2];
    }
    const float ms = (float)g.max_splat;
    const float lo = -(ms + 1.0f), x_hi = (float)(g.W + g.max_splat), y_hi = (float)(g.H + g.max_splat);
    const size_t HW = (size_t)g.H * g.W;
    const int n0 = blockIdx.y * FRAME_GROUP, n1 = min(n0 + FRAME_GROUP, g.N);
    for (int n = n0; n < n1; ++n) {
        const Cam c = load_cam(K, M, n);
        const float q0 = X0 - c.t[0], q1 = X1 - c.t[1], q2 = X2 - c.t[2];
        const float Px = (c.r[0] * q0 + c.r[3] * q1) + c.r[6] * q2;
        const float Py = (c.r[1] * q0 + c.r[4] * q1) + c.r[7] * q2;
        const float Pz = (c.r[2] * q0 + c.r[5] * q1) + c.r[8] * q2;
        const bool front = (int)live & (int)(Pz > Z_EPS) & (int)(Pz < g.max_depth);                // (no short circuit: no branch)
        int cnt[3] = {(int)__popcll(__ballot(front)), 0, 0};
        if (cnt[0]) {                                            // wave-uniform
            const float x = (c.fx * Px) / Pz + c.cx;
            const float y = (c.fy * Py) / Pz + c.cy;
            float hx = (c.fx * g.radius) / Pz;
            float hy = (c.fy * g.radius) / Pz;
            const bool clipped = (int)front & ((int)(hx > ms) | (int)(hy > ms));
            hx = hx > ms ? ms : hx;
            hy = hy > ms ? ms : hy;
            const bool on = (int)front & (int)(x >= lo) & (int)(x <= x_hi) & (int)(y >= lo) & (int)(y <= y_hi);      // NaN, inf fail
            // from here on a lane that is not on screen computes with zeros: every conversion below sees a value within
            // [-(2 * max_splat + 2), 2^30 + 2 * max_splat + 1]
            const float xs = on ? x : 0.0f, ys = on ? y : 0.0f, hxs = on ? hx : 0.0f, hys = on ? hy : 0.0f;
            const float ucf = floorf(xs + 0.5f), vcf = floorf(ys + 0.5f);
            const int u_lo = max((int)fminf(ceilf(xs - hxs), ucf), 0);
            const int u_hi = min((int)fmaxf(floorf(xs + hxs), ucf), g.W - 1);
            const int v_lo = max((int)fminf(ceilf(ys - hys), vcf), 0);
            const int v_hi = min((int)fmaxf(floorf(ys + hys), vcf), g.H - 1);
            const bool drawn = (int)on & (int)(u_lo <= u_hi) & (int)(v_lo <= v_hi);
            cnt[1] = (int)__popcll(__ballot(drawn));
            cnt[2] = (int)__popcll(__ballot(clipped));
            if (drawn) {                                         // 0 <= u_lo <= u_hi < W, 0 <= v_lo <= v_hi < H, n < N: inside the key buffer
                const unsigned long long key = ((unsigned long long)__float_as_uint(Pz) << 32) | (unsigned)i;
                unsigned long long* frame = keys + (size_t)n * HW;
                for (int v = v_lo; v <= v_hi; ++v) {
                    unsigned long long* row = frame + (size_t)v * g.W;
                    for (int u = u_lo; u <= u_hi; ++u) {
                        if (LOAD_FIRST && __hip_atomic_load(row + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) continue;
                        atomicMin(row + u, key);
                    }
                }
            }
        }
        striped_counter_add(cnt, sm_stats[(n - n0) & 1],
                            counters + ((size_t)n * MAX_LINES + blockIdx.x % (unsigned)MAX_LINES) * LINE_INTS);
    }
}

// grid (ceil(H * W / NT), N)
__global__ __launch_bounds__(NT) void k_render_resolve(const unsigned long long* __restrict__ keys, const float* __restrict__ colors, Geom g,
                                                       float* __restrict__ out_depth, int32_t* __restrict__ out_index,
                                                       float* __restrict__ out_colors, int32_t* __restrict__ counters) {
    __shared__ int sm_stats[NT / 64][1];
    const int n = blockIdx.y;
    const size_t HW = (size_t)g.H * g.W;
    const size_t p = (size_t)blockIdx.x * NT + threadIdx.x;
    const bool in = p < HW;
    const unsigned long long key = in ? keys[(size_t)n * HW + p] : EMPTY;
    const bool hit = key != EMPTY;
    if (in) {
        const unsigned idx = (unsigned)key;                      // < M where hit
        out_depth[(size_t)n * HW + p] = hit ? __uint_as_float((unsigned)(key >> 32)) : __builtin_inff();
        out_index[(size_t)n * HW + p] = hit ? (int)idx : -1;
        if (out_colors) {
            float c[3] = {0.0f, 0.0f, 0.0f};
            if (hit) {                                           // (colors may be NULL when M = 0: nothing hits then)
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k] = colors[(size_t)idx * 3 + k];
            }
            float* o = out_colors + (size_t)n * 3 * HW + p;
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k * HW] = c[k];
        }
    }
    const int cnt[1] = {(int)__popcll(__ballot(hit))};
    striped_counter_add(cnt, sm_stats, counters + ((size_t)n * MAX_LINES + blockIdx.x % (unsigned)MAX_LINES) * LINE_INTS + 3);
}

// grid N, one wave: out_stats[n][k] = sum over the frame's counter lines
__global__ __launch_bounds__(64) void k_render_stats(const int32_t* __restrict__ counters, int32_t* __restrict__ out_stats) {
    const int n = blockIdx.x, k = threadIdx.x;
    if (k >= N_STATS) return;
    int t = 0;
#pragma unroll
    for (int l = 0; l < MAX_LINES; ++l) t += counters[((size_t)n * MAX_LINES + l) * LINE_INTS + k];
    out_stats[(size_t)n * N_STATS + k] = t;
}

bool render_shape(int N, int H, int W) {
    return N >= 1 && N <= 65535 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 30) && (long long)N * H * W < (1ll << 31);
}

struct Scratch {                           // the keys [N][H][W], the counter lines [N][MAX_LINES][LINE_INTS]
    unsigned long long* keys;
    int32_t* counters;
    size_t bytes;
};

Scratch layout(void* base, int N, int H, int W) {
    Carver c(base);
    Scratch s;
    s.keys = c.take<unsigned long long>((size_t)N * H * W);
    s.counters = c.take<int32_t>((size_t)N * MAX_LINES * LINE_INTS);
    s.bytes = c.bytes();
    return s;
}

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" size_t colvo_render_scratch_bytes(int N, int H, int W) {
    if (!render_shape(N, H, W)) return 0;
    return layout(nullptr, N, H, W).bytes;
}

extern "C" int colvo_render_cloud(const float* points, const float* colors, int M, const float* K, const float* cam2world, int N, int H,
                                  int W, float radius, int max_splat, float max_depth, void* scratch, float* out_depth,
                                  int32_t* out_index, float* out_colors, int32_t* out_stats, colvo_stream_t stream) {
    COLVO_CHECK_ARG(M >= 0, "colvo_render_cloud: bad point count M=%d (0 <= M < 2^31)", M);
    COLVO_CHECK_ARG((points || M == 0) && K && cam2world && scratch && out_depth && out_index && out_stats,
                    "colvo_render_cloud: null pointer argument");
    COLVO_CHECK_ARG(out_colors ? (colors || M == 0) : !colors,
                    "colvo_render_cloud: null pointer argument: colors and out_colors go together");
    COLVO_CHECK_ARG(render_shape(N, H, W), "colvo_render_cloud: bad shape N=%d H=%d W=%d (1 <= N <= 65535, H*W < 2^30, N*H*W < 2^31)", N, H,
                    W);
    COLVO_CHECK_ARG(max_splat >= 0 && max_splat <= MAX_SPLAT, "colvo_render_cloud: bad max_splat %d (0 .. %d)", max_splat, MAX_SPLAT);
    COLVO_CHECK_ARG(radius >= 0.0f && radius < __builtin_inff(), "colvo_render_cloud: bad radius %g (finite and >= 0)", (double)radius);
    COLVO_CHECK_ARG(max_depth > 0.0f && max_depth < __builtin_inff(), "colvo_render_cloud: bad max_depth %g (finite and positive)",
                    (double)max_depth);
    COLVO_CHECK_ARG(aligned16(scratch), "colvo_render_cloud: scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    Geom g;
    g.M = M; g.N = N; g.H = H; g.W = W; g.max_splat = max_splat; g.radius = radius; g.max_depth = max_depth;
    const Scratch w = layout(scratch, N, H, W);
    const long long total = (long long)N * H * W;
    const int n_counters = N * MAX_LINES * LINE_INTS;
    const long long clear_threads = (total >> 1) + 1 > n_counters ? (total >> 1) + 1 : n_counters;
    colvo::launch(k_render_clear, dim3(blocks_of(clear_threads, NT)), dim3(NT), 0, s, w.keys, total, w.counters, n_counters);
    COLVO_CHECK_LAUNCH("k_render_clear");
    if (M > 0) {
        const dim3 grid(blocks_of(M, NT), blocks_of(N, FRAME_GROUP));
        if (TUNE(render_load_first))
            colvo::launch(k_render_splat<true>, grid, dim3(NT), 0, s, points, K, cam2world, g, w.keys, w.counters);
        else
            colvo::launch(k_render_splat<false>, grid, dim3(NT), 0, s, points, K, cam2world, g, w.keys, w.counters);
        COLVO_CHECK_LAUNCH("k_render_splat");
    }
    colvo::launch(k_render_resolve, dim3(blocks_of((long long)H * W, NT), N), dim3(NT), 0, s, (const unsigned long long*)w.keys, colors, g,
                  out_depth, out_index, out_colors, w.counters);
    COLVO_CHECK_LAUNCH("k_render_resolve");
    colvo::launch(k_render_stats, dim3(N), dim3(64), 0, s, (const int32_t*)w.counters, out_stats);
    COLVO_CHECK_LAUNCH("k_render_stats");
    return 0;
}
