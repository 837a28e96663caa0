// surfels.hip -- a point cloud with normals drawn into camera views as oriented discs: render.hip's walk, key buffer
// and footprint (csrc/render_common.h), but a point that has a normal offers, per pixel of its footprint, the depth at which the
// pixel's ray meets the point's disc, instead of one depth for the whole square.  Contract: include/colvo.h (colvo_render_surfels).
//
//   k_render_clear    (render_common.h) the key buffer to all-ones, the counter lines to zero.
//   k_surfel_splat    one point per thread, point and normal in registers, over a group of FRAME_GROUP frames.  Per frame: the camera
//                     point and the footprint as in k_render_splat; the normal turned into the camera frame (six products); a point
//                     that faces away leaves.  Per pixel of the footprint one division (the ray's depth on the disc's plane), the
//                     offset from the disc's centre and the test against radius^2; a hit offers that depth, the nearest pixel offers
//                     the centre's depth when it is not hit, nothing else is offered.  A point without a normal offers the centre's
//                     depth on every pixel: render.hip's square.  Both splat forms (tuning.h render_load_first) as there.
//   k_surfel_resolve  one thread per pixel: key -> depth, index, gathered colour and, when asked, the winner's camera-frame normal.
//   k_surfel_stats    one wave per frame: the counter lines summed into out_stats[N][6].
//
// These kernels live in a file of their own, not in render.hip, because tests/test_render_cpu.py pins render.hip's listing to its
// five kernels.  Every float32 operation is individually rounded -- contraction is off for this whole file --, the minimum is an
// integer minimum and every sum is an integer: a call's bits do not depend on scheduling or on the stream.
#include "scene.h"
#include "tuning.h"

#pragma clang fp contract(off)

#include "render_common.h"

namespace colvo {
namespace {

using namespace render_common;

constexpr int N_STATS = 6;                 // out_stats: front, drawn, clipped, covered, culled, flat
constexpr int N_SPLAT_STATS = 5;           // a counter line: front, drawn, clipped, culled, flat (the splat's), covered (the resolve's)
constexpr int LINE_COVERED = 5;

// the world normal in the frame's camera: m_a = (r_0a * N_0 + r_1a * N_1) + r_2a * N_2
__device__ __forceinline__ void cam_normal(const Cam& c, float N0, float N1, float N2, float (&m)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = (c.r[a] * N0 + c.r[3 + a] * N1) + c.r[6 + a] * N2;
}

__device__ __forceinline__ bool has_normal(float N0, float N1, float N2) { return (N0 * N0 + N1 * N1) + N2 * N2 > 0.0f; }     // NaN fails

// grid (ceil(M / NT), ceil(N / FRAME_GROUP))
template <bool LOAD_FIRST>
__global__ __launch_bounds__(NT) void k_surfel_splat(const float* __restrict__ points, const float* __restrict__ normals,
                                                     const float* __restrict__ K, const float* __restrict__ M, Geom g,
                                                     unsigned long long* __restrict__ keys, int32_t* __restrict__ counters) {
    __shared__ int sm_stats[2][NT / 64][N_SPLAT_STATS];
    const int i = blockIdx.x * NT + threadIdx.x;                 // M < 2^31 and the grid covers M rounded up to NT <= 2^31: no overflow
    const bool live = i < g.M;
    float X0 = 0.0f, X1 = 0.0f, X2 = 0.0f, N0 = 0.0f, N1 = 0.0f, N2 = 0.0f;
    if (live) {
        const float* p = points + (size_t)i * 3;
        const float* q = normals + (size_t)i * 3;
        X0 = p[0]; X1 = p[1]; X2 = p[2];
        N0 = q[0]; N1 = q[1]; N2 = q[2];
    }
    const bool has = has_normal(N0, N1, N2);
    const float r2 = g.radius * g.radius;
    const size_t HW = (size_t)g.H * g.W;
    const int n0 = blockIdx.y * FRAME_GROUP, n1 = min(n0 + FRAME_GROUP, g.N);
    for (int n = n0; n < n1; ++n) {
        const Cam c = load_cam(K, M, n);
        const CamPoint p = cam_point(c, g, live, X0, X1, X2);
        int cnt[N_SPLAT_STATS] = {(int)__popcll(__ballot(p.front)), 0, 0, 0, 0};
        if (cnt[0]) {                                            // wave-uniform
            const Footprint f = footprint(c, g, p);
            float m[3];
            cam_normal(c, N0, N1, N2, m);
            const float num = (m[0] * p.Px + m[1] * p.Py) + m[2] * p.Pz;
            const bool culled = (int)p.front & (int)has & (int)(num >= 0.0f);                      // faces away; a NaN does not
            const bool flat = (int)p.front & (int)!has;
            bool drawn = false;
            if ((int)f.inside & (int)!culled) {                  // 0 <= u_lo <= u_hi < W, 0 <= v_lo <= v_hi < H, n < N: inside the key buffer
                const unsigned long long centre_key = pack_key(p.Pz, i);
                unsigned long long* frame = keys + (size_t)n * HW;
                for (int v = f.v_lo; v <= f.v_hi; ++v) {
                    unsigned long long* row = frame + (size_t)v * g.W;
                    const float dy = ((float)v - c.cy) / c.fy;
                    for (int u = f.u_lo; u <= f.u_hi; ++u) {
                        unsigned long long key = centre_key;
                        bool offer = !has;
                        if (has) {
                            const float dx = ((float)u - c.cx) / c.fx;
                            const float den = (m[0] * dx + m[1] * dy) + m[2];
                            const float z = num / den;
                            const float ex = dx * z - p.Px, ey = dy * z - p.Py, ez = z - p.Pz;
                            const float ee = (ex * ex + ey * ey) + ez * ez;
                            const bool hit = (int)(den < 0.0f) & (int)(z > Z_EPS) & (int)(z < g.max_depth) & (int)(ee <= r2);   // NaN, inf fail
                            offer = (int)hit | ((int)(u == f.uc) & (int)(v == f.vc));
                            if (hit) key = pack_key(z, i);
                        }
                        if (offer) {
                            drawn = true;
                            offer_key<LOAD_FIRST>(row + u, key);
                        }
                    }
                }
            }
            cnt[1] = (int)__popcll(__ballot(drawn));
            cnt[2] = (int)__popcll(__ballot(f.clipped));
            cnt[3] = (int)__popcll(__ballot(culled));
            cnt[4] = (int)__popcll(__ballot(flat));
        }
        striped_counter_add(cnt, sm_stats[(n - n0) & 1],
                            counters + ((size_t)n * MAX_LINES + blockIdx.x % (unsigned)MAX_LINES) * LINE_INTS);
    }
}

// grid (ceil(H * W / NT), N)
__global__ __launch_bounds__(NT) void k_surfel_resolve(const unsigned long long* __restrict__ keys, const float* __restrict__ colors,
                                                       const float* __restrict__ normals, const float* __restrict__ K,
                                                       const float* __restrict__ M, Geom g, float* __restrict__ out_depth,
                                                       int32_t* __restrict__ out_index, float* __restrict__ out_colors,
                                                       float* __restrict__ out_normal, int32_t* __restrict__ counters) {
    const ResolvePixel r = resolve_open(keys, g);
    bool hit = false;
    unsigned idx;
    if (r.in) {
        hit = resolve_pixel(r, colors, out_depth, out_index, out_colors, idx);
        if (out_normal) {
            float m[3] = {0.0f, 0.0f, 0.0f};
            if (hit) {
                const float* q = normals + (size_t)idx * 3;
                const float N0 = q[0], N1 = q[1], N2 = q[2];
                if (has_normal(N0, N1, N2)) cam_normal(load_cam(K, M, r.n), N0, N1, N2, m);
            }
            float* o = out_normal + (size_t)r.n * 3 * r.HW + r.p;
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k * r.HW] = m[k];
        }
    }
    resolve_close(hit, r.n, LINE_COVERED, counters);
}

// grid N, one wave: front, drawn, clipped, covered, culled, flat
__global__ __launch_bounds__(64) void k_surfel_stats(const int32_t* __restrict__ counters, int32_t* __restrict__ out_stats) {
    stats_row<N_STATS, LINE_COVERED, 3>(counters, out_stats);
}

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" int colvo_render_surfels(const float* points, const float* normals, const float* colors, int M, const float* K,
                                    const float* cam2world, int N, int H, int W, float radius, int max_splat, float max_depth,
                                    void* scratch, float* out_depth, int32_t* out_index, float* out_colors, float* out_normal,
                                    int32_t* out_stats, colvo_stream_t stream) {
    COLVO_CHECK_ARG(M >= 0, "colvo_render_surfels: bad point count M=%d (0 <= M < 2^31)", M);
    hipStream_t s = (hipStream_t)stream;
    Geom g;
    Scratch w;
    if (int e = begin_render("colvo_render_surfels", (points && normals) || M == 0, colors || M == 0, colors, K, cam2world, M, N, H, W,
                             radius, max_splat, max_depth, scratch, out_depth, out_index, out_colors, out_stats, s, g, w))
        return e;
    if (M > 0) {
        launch_draw(k_surfel_splat<true>, k_surfel_splat<false>, dim3(blocks_of(M, NT), blocks_of(N, FRAME_GROUP)), s, points, normals, K,
                    cam2world, g, w.keys, w.counters);
        COLVO_CHECK_LAUNCH("k_surfel_splat");
    }
    colvo::launch(k_surfel_resolve, dim3(blocks_of((long long)H * W, NT), N), dim3(NT), 0, s, (const unsigned long long*)w.keys, colors,
                  normals, K, cam2world, g, out_depth, out_index, out_colors, out_normal, w.counters);
    COLVO_CHECK_LAUNCH("k_surfel_resolve");
    colvo::launch(k_surfel_stats, dim3(N), dim3(64), 0, s, (const int32_t*)w.counters, out_stats);
    COLVO_CHECK_LAUNCH("k_surfel_stats");
    return 0;
}
