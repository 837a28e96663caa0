// render_common.h -- what the two renderers share: render.hip draws screen-aligned squares, surfels.hip draws
// oriented discs.  Steps 1 to 5 of colvo_render_cloud's contract (camera point, front, centre, half-widths, footprint) are ONE routine
// here, so a point without a normal is drawn by surfels.hip with the bits render.hip gives it; so are the key buffer's layout and
// clear and the decoding of a winning key.  A file that includes this header must have contraction off in front of the include.
#pragma once
#include "scene.h"

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

// one pixel of k_render_resolve / k_surfel_resolve: key -> depth, index, gathered colour.  Returns whether a point landed; idx < M then.
__device__ __forceinline__ bool resolve_pixel(unsigned long long key, const float* __restrict__ colors, size_t HW, size_t frame_pixel,
                                              size_t colour_pixel, float* __restrict__ out_depth, int32_t* __restrict__ out_index,
                                              float* __restrict__ out_colors, unsigned& idx) {
    const bool hit = key != EMPTY;
    idx = (unsigned)key;
    out_depth[frame_pixel] = hit ? __uint_as_float((unsigned)(key >> 32)) : __builtin_inff();
    out_index[frame_pixel] = hit ? (int)idx : -1;
    if (out_colors) {
        float c[3] = {0.0f, 0.0f, 0.0f};
        if (hit) {                                               // (colors may be NULL when M = 0: nothing hits then)
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = colors[(size_t)idx * 3 + k];
        }
        float* o = out_colors + colour_pixel;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k * HW] = c[k];
    }
    return hit;
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

// k_render_clear for a call's scratch; the launch's error is the caller's to check
inline void launch_clear(const Scratch& w, int N, int H, int W, hipStream_t s) {
    const long long total = (long long)N * H * W;
    const int n_counters = N * MAX_LINES * LINE_INTS;
    const long long clear_threads = (total >> 1) + 1 > n_counters ? (total >> 1) + 1 : n_counters;
    colvo::launch(k_render_clear, dim3(blocks_of(clear_threads, NT)), dim3(NT), 0, s, w.keys, total, w.counters, n_counters);
}

}  // namespace render_common
}  // namespace colvo
