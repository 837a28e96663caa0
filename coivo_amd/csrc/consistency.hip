// consistency.hip -- multi-view depth consistency: a pixel of frame i keeps its depth only if neighbouring frames,
// through the trajectory, see the same surface there.  Contract: include/colvo.h (colvo_consistency_*).
//
//   k_consist_rel     one thread per (frame, neighbour slot): [R|t] frame i -> frame j in float64 from the float32 cam2world, rounded
//                     to float32, into the table [N][2 * window][12]; the same launch clears the per-frame counter lines.
//   k_consist_filter  one thread per pixel, a wave per 8x8 tile, a workgroup per 16x16; the neighbour loop is the outer loop and a
//                     neighbour's transform and intrinsics are wave-uniform.  The four taps of a neighbour are issued before the
//                     previous neighbour is judged.  No LDS for the data; five integer adds per workgroup for the statistics.
//   k_consist_stats   one workgroup per frame: the counter lines summed into out_stats[N][5].
//
// Every float32 operation that decides a vote is individually rounded -- contraction is off for this whole file -- and every sum is
// an integer: a call's bits do not depend on scheduling or on the stream.
#include "scene.h"
#include "tuning.h"

#pragma clang fp contract(off)

namespace colvo {
namespace {

constexpr int NT = 256;
constexpr int TILE = 8;                    // a wave owns TILE x TILE pixels: their taps land in a compact patch of the neighbour's map
constexpr int WG_TILE = 16;                // a workgroup owns 2 x 2 of them
constexpr int MAX_WINDOW = 16;
constexpr int REL_FLOATS = 12;             // R row-major, then t
constexpr int N_STATS = 5;                 // candidates, kept, no_view, few_agree, violated_out
constexpr int MAX_LINES = 8;               // counter lines per frame,
constexpr int LINE_INTS = 16;              // ... 64 bytes each
constexpr float Z_EPS = 1e-3f;             // spec: Z_EPS

struct Geom {
    int N, H, W, window, step, tiles_x, tiles;
};

// neighbour slot s of frame i: k = -window..-1 for s < window, 1..window from there on (ascending j); -1 where it does not exist
__host__ __device__ __forceinline__ int neighbour(int i, int s, int window, int step, int N) {
    const int k = s < window ? s - window : s - window + 1;
    const int j = i + k * step;                                  // step <= 65536 (colvo_consistency_filter clamps g.step), |k| <= 16: no overflow
    return j >= 0 && j < N ? j : -1;
}

// grid ceil(N * MAX_LINES * LINE_INTS / NT): clears the counters; the first N * 2 * window threads fill the table
__global__ __launch_bounds__(NT) void k_consist_rel(const float* __restrict__ M, int N, int window, int step, float* __restrict__ rel,
                                                    int32_t* __restrict__ counters) {
    const int idx = blockIdx.x * NT + threadIdx.x;
    if (idx < N * MAX_LINES * LINE_INTS) counters[idx] = 0;
    const int slots = 2 * window;
    if (idx >= N * slots) return;
    const int i = idx / slots, s = idx - i * slots;
    const int j = neighbour(i, s, window, step, N);
    float* out = rel + (size_t)idx * REL_FLOATS;
    if (j < 0) {
#pragma unroll
        for (int e = 0; e < REL_FLOATS; ++e) out[e] = 0.0f;
        return;
    }
    const float* mi = M + (size_t)i * 16;
    const float* mj = M + (size_t)j * 16;
    double Ri[3][3], Rj[3][3], dt[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Ri[r][c] = (double)mi[r * 4 + c];
            Rj[r][c] = (double)mj[r * 4 + c];
        }
        dt[r] = (double)mi[r * 4 + 3] - (double)mj[r * 4 + 3];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) out[a * 3 + b] = (float)((Rj[0][a] * Ri[0][b] + Rj[1][a] * Ri[1][b]) + Rj[2][a] * Ri[2][b]);
        out[9 + a] = (float)((Rj[0][a] * dt[0] + Rj[1][a] * dt[1]) + Rj[2][a] * dt[2]);
    }
}

struct Sample {                            // one neighbour's view of the pixel, its taps in flight
    float pz, wx, wy, t00, t01, t10, t11;
    bool seen;                             // front and inside (of a candidate)
};

// Projects the candidate into frame j and issues the four tap loads (from a safe address where the point is not seen).
__device__ __forceinline__ Sample issue(const float* __restrict__ dj, const float* __restrict__ T, const float* __restrict__ Kj, int H,
                                        int W, bool cand, float px, float py, float d) {
    const float fx = Kj[0], fy = Kj[4], cx = Kj[2], cy = Kj[5];
    const float Px = ((T[0] * px + T[1] * py) + T[2] * d) + T[9];
    const float Py = ((T[3] * px + T[4] * py) + T[5] * d) + T[10];
    const float Pz = ((T[6] * px + T[7] * py) + T[8] * d) + T[11];
    Sample sm;
    sm.pz = Pz;
    const bool front = Pz > Z_EPS;
    const float x = (fx * Px) / Pz + cx;
    const float y = (fy * Py) / Pz + cy;
    sm.seen = cand && front && x >= 0.0f && x <= (float)(W - 1) && y >= 0.0f && y <= (float)(H - 1);       // NaN fails
    const float x0f = floorf(x), y0f = floorf(y);
    sm.wx = x - x0f;
    sm.wy = y - y0f;
    const int x0 = sm.seen ? (int)x0f : 0, y0 = sm.seen ? (int)y0f : 0;         // in [0, W-1] x [0, H-1]
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float* r0 = dj + (size_t)y0 * W;
    const float* r1 = dj + (size_t)y1 * W;
    sm.t00 = r0[x0];
    sm.t01 = r0[x1];
    sm.t10 = r1[x0];
    sm.t11 = r1[x1];
    return sm;
}

__device__ __forceinline__ void judge(const Sample& sm, float rel_tol, float max_depth, int& agree, int& occluded, int& violated) {
    const bool visible = (int)sm.seen & (int)valid_depth(sm.t00, max_depth) & (int)valid_depth(sm.t01, max_depth) &
                         (int)valid_depth(sm.t10, max_depth) & (int)valid_depth(sm.t11, max_depth);      // (no short circuit: no branch)
    const float ax = 1.0f - sm.wx, ay = 1.0f - sm.wy;
    const float s = (((sm.t00 * ax) + (sm.t01 * sm.wx)) * ay) + (((sm.t10 * ax) + (sm.t11 * sm.wx)) * sm.wy);
    const float rel = fabsf(sm.pz - s) / (sm.pz + s);
    const bool ok = rel < rel_tol;
    const bool occ = s < sm.pz;
    agree += visible && ok;
    occluded += visible && !ok && occ;
    violated += visible && !ok && !occ;
}

// grid (tiles, N)
__global__ __launch_bounds__(NT) void k_consist_filter(const float* __restrict__ depth, const float* __restrict__ K,
                                                       const float* __restrict__ rel, Geom g, float rel_tol, int min_agree,
                                                       int max_violated, float max_depth, int lines, float* __restrict__ out_depth,
                                                       uint8_t* __restrict__ out_votes, int32_t* __restrict__ counters) {
    __shared__ int sm_stats[NT / 64][N_STATS];
    const int i = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ty = blockIdx.x / g.tiles_x, tx = blockIdx.x - ty * g.tiles_x;
    const int u = tx * WG_TILE + (wave & 1) * TILE + (lane & 7);
    const int v = ty * WG_TILE + (wave >> 1) * TILE + (lane >> 3);
    const bool in = u < g.W && v < g.H;
    const size_t HW = (size_t)g.H * g.W;
    const size_t pix = (size_t)v * g.W + u;
    const float d = in ? depth[(size_t)i * HW + pix] : 0.0f;
    const bool cand = in && valid_depth(d, max_depth);
    const float* Ki = K + (size_t)i * 9;
    const float px = (((float)u - Ki[2]) / Ki[0]) * d;
    const float py = (((float)v - Ki[5]) / Ki[4]) * d;

    int agree = 0, occluded = 0, violated = 0;
    const int slots = 2 * g.window;
    const float* Ti = rel + (size_t)i * slots * REL_FLOATS;
    // the slots whose frame exists are contiguous: [s_lo, s_hi).  Two samples take turns, so that a neighbour's taps are in flight
    // while the one before it is judged and the one after it is projected (uniform branches only).
    const int s_lo = max(0, g.window - i / g.step), s_hi = min(slots, g.window + (g.N - 1 - i) / g.step);
    auto sample = [&](int s) {
        const int j = neighbour(i, s, g.window, g.step, g.N);
        return issue(depth + (size_t)j * HW, Ti + s * REL_FLOATS, K + (size_t)j * 9, g.H, g.W, cand, px, py, d);
    };
    if (s_lo < s_hi) {
        Sample a = sample(s_lo);
        int s = s_lo;
        for (; s + 2 < s_hi; s += 2) {                           // straight-line body: no wait covers more than it needs
            const Sample b = sample(s + 1);
            judge(a, rel_tol, max_depth, agree, occluded, violated);
            a = sample(s + 2);
            judge(b, rel_tol, max_depth, agree, occluded, violated);
        }
        if (s + 1 < s_hi) {
            const Sample b = sample(s + 1);
            judge(a, rel_tol, max_depth, agree, occluded, violated);
            judge(b, rel_tol, max_depth, agree, occluded, violated);
        } else {
            judge(a, rel_tol, max_depth, agree, occluded, violated);
        }
    }
    const int n_seen = (agree + occluded) + violated;            // visible neighbours

    const bool enough = agree >= min_agree, clean = violated <= max_violated;
    const bool kept = cand && enough && clean;
    const bool viol_out = cand && !clean;
    const bool no_view = cand && clean && n_seen == 0 && !enough;          // (min_agree = 0 keeps a pixel nobody else sees)
    const bool few = cand && clean && n_seen > 0 && !enough;
    if (in) {
        out_depth[(size_t)i * HW + pix] = kept ? d : __builtin_inff();
        uint8_t* vp = out_votes + (size_t)i * 3 * HW + pix;
        vp[0] = (uint8_t)agree;
        vp[HW] = (uint8_t)occluded;
        vp[2 * HW] = (uint8_t)violated;
    }
    const int n[N_STATS] = {(int)__popcll(__ballot(cand)), (int)__popcll(__ballot(kept)), (int)__popcll(__ballot(no_view)),
                            (int)__popcll(__ballot(few)), (int)__popcll(__ballot(viol_out))};
    striped_counter_add(n, sm_stats, counters + ((size_t)i * MAX_LINES + blockIdx.x % (unsigned)lines) * LINE_INTS);
}

// grid N, one wave: out_stats[i][k] = sum over the frame's counter lines
__global__ __launch_bounds__(64) void k_consist_stats(const int32_t* __restrict__ counters, int32_t* __restrict__ out_stats) {
    const int i = blockIdx.x, k = threadIdx.x;
    if (k >= N_STATS) return;
    int t = 0;
#pragma unroll
    for (int l = 0; l < MAX_LINES; ++l) t += counters[((size_t)i * MAX_LINES + l) * LINE_INTS + k];
    out_stats[(size_t)i * N_STATS + k] = t;
}

bool ws_shape(int N, int window) { return N > 0 && N <= 65535 && window >= 1 && window <= MAX_WINDOW; }

struct Ws {                                // the transform table [N][2 * window][12], the counter lines [N][MAX_LINES][LINE_INTS]
    float* rel;
    int32_t* counters;
    size_t bytes;
};

Ws layout(void* base, int N, int window) {
    Carver c(base);
    Ws w;
    w.rel = c.take<float>((size_t)N * 2 * window * REL_FLOATS);
    w.counters = c.take<int32_t>((size_t)N * MAX_LINES * LINE_INTS);
    w.bytes = c.bytes();
    return w;
}

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" size_t colvo_consistency_workspace_bytes(int N, int window) {
    if (!ws_shape(N, window)) return 0;
    return layout(nullptr, N, window).bytes;
}

extern "C" int colvo_consistency_filter(const float* depths, const float* K, const float* cam2world, int N, int H, int W, int window,
                                        int step, float rel_tol, int min_agree, int max_violated, float max_depth, void* workspace,
                                        float* out_depths, uint8_t* out_votes, int32_t* out_stats, colvo_stream_t stream) {
    COLVO_CHECK_ARG(depths && K && cam2world && workspace && out_depths && out_votes && out_stats,
                    "colvo_consistency_filter: null pointer argument");
    COLVO_CHECK_ARG(N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 30),
                    "colvo_consistency_filter: bad shape N=%d H=%d W=%d", N, H, W);
    COLVO_CHECK_ARG(window >= 1 && window <= MAX_WINDOW && step >= 1,
                    "colvo_consistency_filter: bad window %d (1 .. %d) or step %d (>= 1)", window, MAX_WINDOW, step);
    COLVO_CHECK_ARG(min_agree >= 0 && min_agree <= 2 * window && max_violated >= 0,
                    "colvo_consistency_filter: bad policy min_agree %d (0 .. 2 * window = %d), max_violated %d (>= 0)", min_agree,
                    2 * window, max_violated);
    COLVO_CHECK_ARG(rel_tol > 0.0f && rel_tol < __builtin_inff() && max_depth > 0.0f && max_depth < __builtin_inff(),
                    "colvo_consistency_filter: bad tolerance rel_tol %g or max_depth %g (finite and positive)", (double)rel_tol,
                    (double)max_depth);
    COLVO_CHECK_ARG(aligned16(workspace), "colvo_consistency_filter: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    Geom g;
    g.N = N; g.H = H; g.W = W; g.window = window;
    g.step = step < 65536 ? step : 65536;                        // a step of N or more has no neighbour: any such step is the same
    g.tiles_x = blocks_of(W, WG_TILE);
    g.tiles = g.tiles_x * blocks_of(H, WG_TILE);
    const Ws w = layout(workspace, N, window);
    long lines = TUNE(consist_stat_lines);
    lines = lines < 1 ? 1 : lines > MAX_LINES ? MAX_LINES : lines;
    colvo::launch(k_consist_rel, dim3(blocks_of(N * MAX_LINES * LINE_INTS, NT)), dim3(NT), 0, s, cam2world, N, window, g.step, w.rel,
                  w.counters);
    COLVO_CHECK_LAUNCH("k_consist_rel");
    colvo::launch(k_consist_filter, dim3(g.tiles, N), dim3(NT), 0, s, depths, K, (const float*)w.rel, g, rel_tol, min_agree, max_violated,
                  max_depth, (int)lines, out_depths, out_votes, w.counters);
    COLVO_CHECK_LAUNCH("k_consist_filter");
    colvo::launch(k_consist_stats, dim3(N), dim3(64), 0, s, (const int32_t*)w.counters, out_stats);
    COLVO_CHECK_LAUNCH("k_consist_stats");
    return 0;
}
