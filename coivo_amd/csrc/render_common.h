// render_common.h -- what the renderers share: render.hip draws screen-aligned squares, surfels.hip
// draws oriented discs, raster.hip triangles.  Steps 1 to 5 of colvo_render_cloud's contract (camera point, front, centre, half-widths,
// footprint) are ONE routine here, so a point without a normal is drawn by surfels.hip with the bits render.hip gives it; so are the
// key buffer's layout and clear, the decoding of a winning key, the frame of a resolve kernel, the stats kernel's body, and what the
// entry points check and launch alike.  A file that includes this header must have contraction off in front of the include.
#pragma once
#include "scene.h"
#include "tuning.h"

#pragma clang fp contract(off)

namespace colvo {
namespace render_common {

constexpr int NT = 256;
constexpr int FRAME_GROUP = 16;            // frames a workgroup of a splat kernel walks with its 256 points in registers
constexpr int MAX_SPLAT = 32;
constexpr int MAX_LINES = 8;               // counter lines per frame,
constexpr int LINE_INTS = 16;              // ... 64 bytes each
constexpr float Z_EPS = 1e-3f;             // spec: Z_EPS
constexpr unsigned long long EMPTY = ~0ull;

struct Geom {
    int M, N, H, W, max_splat;
    float radius, max_depth;
};

namespace {                                // (a kernel per including file: internal linkage)
// grid ceil(max(pairs + 1, n_counters) / NT); total = N * H * W keys, pairs = total / 2
__global__ __launch_bounds__(NT) void k_render_clear(unsigned long long* __restrict__ keys, long long total, int32_t* __restrict__ counters,
                                                     int n_counters) {
    const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
    const long long pairs = total >> 1;
    if (idx < pairs) reinterpret_cast<ulonglong2*>(keys)[idx] = make_ulonglong2(EMPTY, EMPTY);
    if (idx == pairs && (total & 1)) keys[total - 1] = EMPTY;
    if (idx < n_counters) counters[idx] = 0;
}
}  // namespace

// a point in the camera of one frame: steps 1 and 2 of the contract
struct CamPoint {
    float Px, Py, Pz;
    bool front;
};

__device__ __forceinline__ CamPoint cam_point(const Cam& c, const Geom& g, bool live, float X0, float X1, float X2) {
    CamPoint p;
    const float q0 = X0 - c.t[0], q1 = X1 - c.t[1], q2 = X2 - c.t[2];
    p.Px = (c.r[0] * q0 + c.r[3] * q1) + c.r[6] * q2;
    p.Py = (c.r[1] * q0 + c.r[4] * q1) + c.r[7] * q2;
    p.Pz = (c.r[2] * q0 + c.r[5] * q1) + c.r[8] * q2;
    p.front = (int)live & (int)(p.Pz > Z_EPS) & (int)(p.Pz < g.max_depth);                         // (no short circuit: no branch)
    return p;
}

// steps 3 to 5: the pixel rectangle of a point in front.  inside: 0 <= u_lo <= u_hi < W and 0 <= v_lo <= v_hi < H, so every pixel
// of the rectangle is inside the frame's keys; (uc, vc) is the nearest pixel, which may lie outside the image.
struct Footprint {
    int u_lo, u_hi, v_lo, v_hi, uc, vc;
    bool clipped, inside;
};

__device__ __forceinline__ Footprint footprint(const Cam& c, const Geom& g, const CamPoint& p) {
    const float ms = (float)g.max_splat;
    const float lo = -(ms + 1.0f), x_hi = (float)(g.W + g.max_splat), y_hi = (float)(g.H + g.max_splat);
    Footprint f;
    const float x = (c.fx * p.Px) / p.Pz + c.cx;
    const float y = (c.fy * p.Py) / p.Pz + c.cy;
    float hx = (c.fx * g.radius) / p.Pz;
    float hy = (c.fy * g.radius) / p.Pz;
    f.clipped = (int)p.front & ((int)(hx > ms) | (int)(hy > ms));
    hx = hx > ms ? ms : hx;
    hy = hy > ms ? ms : hy;
    const bool on = (int)p.front & (int)(x >= lo) & (int)(x <= x_hi) & (int)(y >= lo) & (int)(y <= y_hi);      // NaN, inf fail
    // from here on a lane that is not on screen computes with zeros: every conversion below sees a value within
    // [-(2 * max_splat + 2), 2^30 + 2 * max_splat + 1]
    const float xs = on ? x : 0.0f, ys = on ? y : 0.0f, hxs = on ? hx : 0.0f, hys = on ? hy : 0.0f;
    const float ucf = floorf(xs + 0.5f), vcf = floorf(ys + 0.5f);
    f.uc = (int)ucf;
    f.vc = (int)vcf;
    f.u_lo = max((int)fminf(ceilf(xs - hxs), ucf), 0);
    f.u_hi = min((int)fmaxf(floorf(xs + hxs), ucf), g.W - 1);
    f.v_lo = max((int)fminf(ceilf(ys - hys), vcf), 0);
    f.v_hi = min((int)fmaxf(floorf(ys + hys), vcf), g.H - 1);
    f.inside = (int)on & (int)(f.u_lo <= f.u_hi) & (int)(f.v_lo <= f.v_hi);
    return f;
}

__device__ __forceinline__ unsigned long long pack_key(float z, int i) {     // z > 0: its bits order as unsigned integers
    return ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)i;
}

// the pixel's minimum: optionally behind a relaxed load that skips it (keys only decrease: a stale read costs an atomic, never skips
// a needed one)
template <bool LOAD_FIRST>
__device__ __forceinline__ void offer_key(unsigned long long* p, unsigned long long key) {
    if (LOAD_FIRST && __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) return;
    atomicMin(p, key);
}

// the opening of a resolve kernel, grid (ceil(H * W / NT), N): the frame, the pixel, whether it is inside the image, its key
struct ResolvePixel {
    int n;
    size_t HW, p;
    bool in;
    unsigned long long key;
};

__device__ __forceinline__ ResolvePixel resolve_open(const unsigned long long* __restrict__ keys, const Geom& g) {
    ResolvePixel r;
    r.n = blockIdx.y;
    r.HW = (size_t)g.H * g.W;
    r.p = (size_t)blockIdx.x * NT + threadIdx.x;
    r.in = r.p < r.HW;
    r.key = r.in ? keys[(size_t)r.n * r.HW + r.p] : EMPTY;
    return r;
}

// one pixel inside the image: key -> depth, index and, with out_colors, the gathered colour of row idx of `colors` (a renderer that
// makes its colours otherwise passes none).  Returns whether something landed; idx is its row then.
__device__ __forceinline__ bool resolve_pixel(const ResolvePixel& r, const float* __restrict__ colors, float* __restrict__ out_depth,
                                              int32_t* __restrict__ out_index, float* __restrict__ out_colors, unsigned& idx) {
    const bool hit = r.key != EMPTY;
    const size_t frame_pixel = (size_t)r.n * r.HW + r.p;
    idx = (unsigned)r.key;
    out_depth[frame_pixel] = hit ? __uint_as_float((unsigned)(r.key >> 32)) : __builtin_inff();
    out_index[frame_pixel] = hit ? (int)idx : -1;
    if (out_colors) {
        float c[3] = {0.0f, 0.0f, 0.0f};
        if (hit) {                                               // (colors may be NULL when M = 0: nothing hits then)
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = colors[(size_t)idx * 3 + k];
        }
        float* o = out_colors + (size_t)r.n * 3 * r.HW + r.p;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k * r.HW] = c[k];
    }
    return hit;
}

// ... and its close: the covered pixels counted by ballot into slot line_covered of the frame's counter lines.  Every thread of the
// workgroup comes here.
__device__ __forceinline__ void resolve_close(bool hit, int n, int line_covered, int32_t* __restrict__ counters) {
    __shared__ int sm_stats[NT / 64][1];
    const int cnt[1] = {(int)__popcll(__ballot(hit))};
    striped_counter_add(cnt, sm_stats, counters + ((size_t)n * MAX_LINES + blockIdx.x % (unsigned)MAX_LINES) * LINE_INTS + line_covered);
}

// a stats kernel, grid N, one wave: out_stats[n][k] = sum over the frame's counter lines.  The draw kernel's counts keep their order;
// the covered pixels, slot LINE_COVERED of a counter line, go to column OUT_COVERED of the N_STATS columns.  A renderer's kernel is
// this one line under the renderer's own name (listings and profiles tell the renderers apart by it).
template <int N_STATS, int LINE_COVERED, int OUT_COVERED>
__device__ __forceinline__ void stats_row(const int32_t* __restrict__ counters, int32_t* __restrict__ out_stats) {
    const int n = blockIdx.x, k = threadIdx.x;
    if (k >= N_STATS) return;
    const int slot = k < OUT_COVERED ? k : k == OUT_COVERED ? LINE_COVERED : k - 1;
    int t = 0;
#pragma unroll
    for (int l = 0; l < MAX_LINES; ++l) t += counters[((size_t)n * MAX_LINES + l) * LINE_INTS + slot];
    out_stats[(size_t)n * N_STATS + k] = t;
}

inline bool render_shape(int N, int H, int W) {
    return N >= 1 && N <= 65535 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 30) && (long long)N * H * W < (1ll << 31);
}

struct Scratch {                           // the keys [N][H][W], the counter lines [N][MAX_LINES][LINE_INTS]
    unsigned long long* keys;
    int32_t* counters;
    size_t bytes;
};

inline Scratch layout(void* base, int N, int H, int W) {
    Carver c(base);
    Scratch s;
    s.keys = c.take<unsigned long long>((size_t)N * H * W);
    s.counters = c.take<int32_t>((size_t)N * MAX_LINES * LINE_INTS);
    s.bytes = c.bytes();
    return s;
}

// What the three entry points refuse and set up alike, under the entry point's own name `who`: the required pointers (`drawn`: what
// is drawn is there, or there is none of it), colours with their output, the shape, the policy, the scratch; then the Geom (rows:
// Geom::M), the scratch's layout and k_render_clear.  -> 0, or the error to return.
inline int begin_render(const char* who, bool drawn, bool colours_there, const void* colors, const void* K, const void* cam2world, int rows,
                        int N, int H, int W, float radius, int max_splat, float max_depth, void* scratch, const void* out_depth,
                        const void* out_index, const void* out_colors, const void* out_stats, hipStream_t s, Geom& g, Scratch& w) {
    COLVO_CHECK_ARG(drawn && K && cam2world && scratch && out_depth && out_index && out_stats, "%s: null pointer argument", who);
    COLVO_CHECK_ARG(out_colors ? colours_there : !colors, "%s: null pointer argument: colors and out_colors go together", who);
    COLVO_CHECK_ARG(render_shape(N, H, W), "%s: bad shape N=%d H=%d W=%d (1 <= N <= 65535, H*W < 2^30, N*H*W < 2^31)", who, N, H, W);
    COLVO_CHECK_ARG(max_splat >= 0 && max_splat <= MAX_SPLAT, "%s: bad max_splat %d (0 .. %d)", who, max_splat, MAX_SPLAT);
    COLVO_CHECK_ARG(radius >= 0.0f && radius < __builtin_inff(), "%s: bad radius %g (finite and >= 0)", who, (double)radius);
    COLVO_CHECK_ARG(max_depth > 0.0f && max_depth < __builtin_inff(), "%s: bad max_depth %g (finite and positive)", who, (double)max_depth);
    COLVO_CHECK_ARG(aligned16(scratch), "%s: scratch must be 16-byte aligned", who);
    g.M = rows; g.N = N; g.H = H; g.W = W; g.max_splat = max_splat; g.radius = radius; g.max_depth = max_depth;
    w = layout(scratch, N, H, W);
    const long long total = (long long)N * H * W;
    const int n_counters = N * MAX_LINES * LINE_INTS;
    const long long clear_threads = (total >> 1) + 1 > n_counters ? (total >> 1) + 1 : n_counters;
    colvo::launch(k_render_clear, dim3(blocks_of(clear_threads, NT)), dim3(NT), 0, s, w.keys, total, w.counters, n_counters);
    COLVO_CHECK_LAUNCH("k_render_clear");
    return 0;
}

// a draw kernel in the form tuning.h render_load_first selects: the relaxed load in front of the atomic minimum, or not
template <typename... P, typename... A>
inline void launch_draw(void (*load_first)(P...), void (*plain)(P...), dim3 grid, hipStream_t s, A&&... a) {
    colvo::launch(TUNE(render_load_first) ? load_first : plain, grid, dim3(NT), 0, s, static_cast<A&&>(a)...);
}

}  // namespace render_common
}  // namespace colvo
