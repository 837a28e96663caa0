// raster.hip -- a triangle mesh drawn into camera views: every face projected into every requested camera, snapped to
// a 1/256-pixel grid and rasterised with integer edge functions and the top-left rule; per covered pixel centre the perspective-correct
// depth in float64, the nearest kept per pixel in the point renderers' key buffer.  Contract: include/colvo.h (colvo_render_mesh).
//
//   k_render_clear       (render_common.h) the key buffer to all-ones, the counter lines to zero.
//   k_raster_zero        face_pixels to zero, when asked for.
//   k_raster_draw        one face per thread -- its three indices checked, its nine world coordinates held in registers -- over a group
//                        of FRAME_GROUP frames; a frame's camera is wave-uniform.  A wave with no front face leaves the set-up after the
//                        classification.  A lane walks the pixel centres of its own bounding box, unless the box holds at least
//                        raster_coop_min_pixels of them: those faces are then taken one by one in ascending lane order, the set-up
//                        broadcast by readlane and the box strided by all 64 lanes.  Both walks offer the same keys; the minimum decides,
//                        so the bits do not depend on the threshold.  Per covered pixel one 64-bit atomic minimum (both
//                        render_load_first forms).  Seven counts per frame through striped_counter_add.
//   k_raster_resolve     one thread per pixel: key -> depth, face; with colours or normals the winner is set up again by the routine
//                        that drew it (raster_common.h) for the interpolation weights; one integer add per covered pixel to
//                        face_pixels when asked.
//   k_raster_stats       one wave per frame: the counter lines summed into out_stats[N][8].
//
// Every float32 and float64 operation is individually rounded -- contraction is off for this whole file --, the edge functions are
// integers, the minimum is an integer minimum and every sum is an integer: a call's bits do not depend on scheduling or on the stream.
#include "scene.h"
#include "tuning.h"

#pragma clang fp contract(off)

#include "raster_common.h"

namespace colvo {
namespace {

using namespace raster;

constexpr int N_STATS = 8;                 // front, drawn, straddling, outside, back-facing, degenerate, fragments, covered
constexpr int N_DRAW_STATS = 7;            // a counter line: the first seven (the draw's), covered (the resolve's)
constexpr int LINE_COVERED = 7;

struct Mesh {
    int V, cull_back, coop_min;            // (the face count is Geom::M)
};

// the three indices of face f, checked: -> whether the face is live; idx is only to be used then
__device__ __forceinline__ bool load_face(const int32_t* __restrict__ faces, int f, int F, int V, int (&idx)[3]) {
    bool live = (int)(f >= 0) & (int)(f < F);
    idx[0] = idx[1] = idx[2] = 0;
    if (live) {
        const int32_t* q = faces + (size_t)f * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) idx[k] = q[k];
        live = (int)(idx[0] >= 0) & (int)(idx[0] < V) & (int)(idx[1] >= 0) & (int)(idx[1] < V) & (int)(idx[2] >= 0) & (int)(idx[2] < V);
    }
    return live;
}

__device__ __forceinline__ void load_corners(const float* __restrict__ vertices, bool live, const int (&idx)[3], float (&w)[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = 0.0f;
    if (live) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* p = vertices + (size_t)idx[k] * 3;
            w[3 * k] = p[0]; w[3 * k + 1] = p[1]; w[3 * k + 2] = p[2];
        }
    }
}

// one pixel centre of a drawn face; (u, v) inside the image, frame inside the key buffer
template <bool LOAD_FIRST>
__device__ __forceinline__ int shade(const Tri& t, const double (&iz)[3], int u, int v, int f, unsigned long long* __restrict__ frame,
                                     int W) {
    long long e[3];
    if (!fragment(t, u, v, e)) return 0;
    offer_key<LOAD_FIRST>(frame + (size_t)v * W + u, pack_key(depth(t, weights(e, iz)), f));
    return 1;
}

__device__ __forceinline__ Tri lane_tri(const Tri& t, int lane) {
    Tri b;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b.X[k] = lane_value(t.X[k], lane);
        b.Y[k] = lane_value(t.Y[k], lane);
        b.Pz[k] = __int_as_float(lane_value(__float_as_int(t.Pz[k]), lane));
    }
    b.A = lane_value(t.A, lane);
    b.u_lo = lane_value(t.u_lo, lane);
    b.u_hi = lane_value(t.u_hi, lane);
    b.v_lo = lane_value(t.v_lo, lane);
    b.v_hi = lane_value(t.v_hi, lane);
    b.flags = lane_value(t.flags, lane);
    b.swapped = false;                     // (the oriented numbering is what travels)
    return b;
}

// grid (ceil(F / NT), ceil(N / FRAME_GROUP))
template <bool LOAD_FIRST>
__global__ __launch_bounds__(NT) void k_raster_draw(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                    const float* __restrict__ K, const float* __restrict__ M, Geom g, Mesh mesh,
                                                    unsigned long long* __restrict__ keys, int32_t* __restrict__ counters) {
    __shared__ int sm_stats[2][NT / 64][N_DRAW_STATS];
    const int f = blockIdx.x * NT + threadIdx.x;                 // F < 2^31 and the grid covers F rounded up to NT <= 2^31: no overflow
    const int lane = threadIdx.x & 63;
    int idx[3];
    const bool live = load_face(faces, f, g.M, mesh.V, idx);
    float w[9];
    load_corners(vertices, live, idx, w);
    const size_t HW = (size_t)g.H * g.W;
    const int n0 = blockIdx.y * FRAME_GROUP, n1 = min(n0 + FRAME_GROUP, g.N);
    for (int n = n0; n < n1; ++n) {
        const Cam c = load_cam(K, M, n);
        CamPoint P[3];
        const Tri t = setup(c, g, live, w, mesh.cull_back, P);
        int cnt[N_DRAW_STATS] = {(int)__popcll(__ballot(t.flags & TRI_FRONT)), 0, (int)__popcll(__ballot(t.flags & TRI_STRADDLE)), 0, 0, 0, 0};
        if (cnt[0]) {                                            // wave-uniform
            const bool drawn = t.flags & TRI_DRAWN;
            const int bw = t.u_hi - t.u_lo + 1, pixels = bw * (t.v_hi - t.v_lo + 1);             // <= 2^28; 0 when not drawn
            const bool coop = (int)drawn & (int)(pixels >= mesh.coop_min);
            unsigned long long* frame = keys + (size_t)n * HW;   // n < N: inside the key buffer
            int fragments = 0;
            if ((int)drawn & (int)!coop) {
                double iz[3];
                inverse_depths(t, iz);
                for (int v = t.v_lo; v <= t.v_hi; ++v)
                    for (int u = t.u_lo; u <= t.u_hi; ++u) fragments += shade<LOAD_FIRST>(t, iz, u, v, f, frame, g.W);
            }
            for (unsigned long long todo = __ballot(coop); todo; todo &= todo - 1) {             // wave-uniform
                const int src = __ffsll(todo) - 1;
                const Tri b = lane_tri(t, src);
                const int bf = lane_value(f, src);
                const int b_bw = b.u_hi - b.u_lo + 1, b_pixels = b_bw * (b.v_hi - b.v_lo + 1);
                double iz[3];
                inverse_depths(b, iz);
                for (int p = lane; p < b_pixels; p += 64) {
                    const int row = p / b_bw;
                    fragments += shade<LOAD_FIRST>(b, iz, b.u_lo + (p - row * b_bw), b.v_lo + row, bf, frame, g.W);
                }
            }
            cnt[1] = (int)__popcll(__ballot(drawn));
            cnt[3] = (int)__popcll(__ballot(t.flags & TRI_OUTSIDE));
            cnt[4] = (int)__popcll(__ballot(t.flags & TRI_BACK));
            cnt[5] = (int)__popcll(__ballot(t.flags & TRI_DEGENERATE));
            cnt[6] = wave_sum(fragments);
        }
        striped_counter_add(cnt, sm_stats[(n - n0) & 1],
                            counters + ((size_t)n * MAX_LINES + blockIdx.x % (unsigned)MAX_LINES) * LINE_INTS);
    }
}

// grid ceil(F / NT)
__global__ __launch_bounds__(NT) void k_raster_zero(int32_t* __restrict__ face_pixels, int F) {
    const int f = blockIdx.x * NT + threadIdx.x;
    if (f < F) face_pixels[f] = 0;
}

// grid (ceil(H * W / NT), N)
__global__ __launch_bounds__(NT) void k_raster_resolve(const unsigned long long* __restrict__ keys, const float* __restrict__ vertices,
                                                       const int32_t* __restrict__ faces, const float* __restrict__ colors,
                                                       const float* __restrict__ K, const float* __restrict__ M, Geom g, Mesh mesh,
                                                       float* __restrict__ out_depth, int32_t* __restrict__ out_index,
                                                       float* __restrict__ out_colors, float* __restrict__ out_normal,
                                                       int32_t* __restrict__ face_pixels, int32_t* __restrict__ counters) {
    const ResolvePixel r = resolve_open(keys, g);
    const int n = r.n;
    const size_t HW = r.HW, p = r.p;
    bool hit = false;
    if (r.in) {
        unsigned row;
        hit = resolve_pixel(r, nullptr, out_depth, out_index, nullptr, row);                   // (the colours are interpolated below)
        const int f = (int)row;
        float col[3] = {0.0f, 0.0f, 0.0f}, nrm[3] = {0.0f, 0.0f, 0.0f};
        int idx[3];
        if ((int)hit & (int)(out_colors != nullptr || out_normal != nullptr) && load_face(faces, f, g.M, mesh.V, idx)) {
            float w[9];
            load_corners(vertices, true, idx, w);
            const Cam c = load_cam(K, M, n);
            CamPoint P[3];
            const Tri t = setup(c, g, true, w, 0, P);
            if (out_colors) {
                const int v = (int)(p / (size_t)g.W), u = (int)(p - (size_t)v * g.W);
                long long e[3];
                fragment(t, u, v, e);
                double iz[3];
                inverse_depths(t, iz);
                const Weights q = weights(e, iz);
                const float* c0 = colors + (size_t)idx[0] * 3;
                const float* c1 = colors + (size_t)idx[t.swapped ? 2 : 1] * 3;
                const float* c2 = colors + (size_t)idx[t.swapped ? 1 : 2] * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    col[k] = (float)(((q.w[0] * (double)c0[k] + q.w[1] * (double)c1[k]) + q.w[2] * (double)c2[k]) / q.s);
            }
            if (out_normal) {                                    // the face's own numbering: (P1 - P0) x (P2 - P0), turned to the camera
                const double a[3] = {(double)P[1].Px - (double)P[0].Px, (double)P[1].Py - (double)P[0].Py, (double)P[1].Pz - (double)P[0].Pz};
                const double b[3] = {(double)P[2].Px - (double)P[0].Px, (double)P[2].Py - (double)P[0].Py, (double)P[2].Pz - (double)P[0].Pz};
                const double m[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
                const double len = __builtin_sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
                if ((int)(len > 0.0) & (int)(len < __builtin_inf())) {
                    const double u0 = m[0] / len, u1 = m[1] / len, u2 = m[2] / len;
                    const double away = (u0 * (double)P[0].Px + u1 * (double)P[0].Py) + u2 * (double)P[0].Pz;
                    const bool flip = away > 0.0;
                    nrm[0] = (float)(flip ? -u0 : u0);
                    nrm[1] = (float)(flip ? -u1 : u1);
                    nrm[2] = (float)(flip ? -u2 : u2);
                }
            }
        }
        if (out_colors) {
            float* o = out_colors + (size_t)n * 3 * HW + p;
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k * HW] = col[k];
        }
        if (out_normal) {
            float* o = out_normal + (size_t)n * 3 * HW + p;
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k * HW] = nrm[k];
        }
        if (face_pixels && (int)hit & (int)(f >= 0) & (int)(f < g.M)) atomicAdd(face_pixels + f, 1);
    }
    resolve_close(hit, n, LINE_COVERED, counters);
}

// grid N, one wave: the draw's seven counts, then covered
__global__ __launch_bounds__(64) void k_raster_stats(const int32_t* __restrict__ counters, int32_t* __restrict__ out_stats) {
    stats_row<N_STATS, LINE_COVERED, 7>(counters, out_stats);
}

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" int colvo_render_mesh(const float* vertices, const int32_t* faces, const float* colors, int V, int F, const float* K,
                                 const float* cam2world, int N, int H, int W, float max_depth, int cull_back, void* scratch,
                                 float* out_depth, int32_t* out_index, float* out_colors, float* out_normal, int32_t* out_face_pixels,
                                 int32_t* out_stats, colvo_stream_t stream) {
    COLVO_CHECK_ARG(V >= 0 && F >= 0, "colvo_render_mesh: bad mesh V=%d F=%d (0 <= V, F < 2^31)", V, F);
    COLVO_CHECK_ARG(render_shape(N, H, W) && H <= 16384 && W <= 16384,
                    "colvo_render_mesh: bad shape N=%d H=%d W=%d (1 <= N <= 65535, 1 <= H, W <= 16384, N*H*W < 2^31)", N, H, W);
    COLVO_CHECK_ARG(cull_back == 0 || cull_back == 1, "colvo_render_mesh: bad cull_back %d (0 or 1)", cull_back);
    hipStream_t s = (hipStream_t)stream;
    Geom g;
    Scratch w;
    if (int e = begin_render("colvo_render_mesh", (vertices || V == 0) && (faces || F == 0), colors || V == 0, colors, K, cam2world, F, N, H,
                             W, 0.0f, 0, max_depth, scratch, out_depth, out_index, out_colors, out_stats, s, g, w))
        return e;
    const double coop = TUNE_F(raster_coop_min_pixels);
    Mesh mesh;
    mesh.V = V;
    mesh.cull_back = cull_back;
    mesh.coop_min = coop >= 2147483647.0 ? 2147483647 : coop >= 0.0 ? (int)coop : 0;             // (a NaN counts as 0)
    if (out_face_pixels && F > 0) {
        colvo::launch(k_raster_zero, dim3(blocks_of(F, NT)), dim3(NT), 0, s, out_face_pixels, F);
        COLVO_CHECK_LAUNCH("k_raster_zero");
    }
    if (F > 0 && V > 0) {
        launch_draw(k_raster_draw<true>, k_raster_draw<false>, dim3(blocks_of(F, NT), blocks_of(N, FRAME_GROUP)), s, vertices, faces, K,
                    cam2world, g, mesh, w.keys, w.counters);
        COLVO_CHECK_LAUNCH("k_raster_draw");
    }
    colvo::launch(k_raster_resolve, dim3(blocks_of((long long)H * W, NT), N), dim3(NT), 0, s, (const unsigned long long*)w.keys, vertices,
                  faces, colors, K, cam2world, g, mesh, out_depth, out_index, out_colors, out_normal, out_face_pixels, w.counters);
    COLVO_CHECK_LAUNCH("k_raster_resolve");
    colvo::launch(k_raster_stats, dim3(N), dim3(64), 0, s, (const int32_t*)w.counters, out_stats);
    COLVO_CHECK_LAUNCH("k_raster_stats");
    return 0;
}
