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
// The frame of the last two and the entry point's checks are render_common.h's, shared with surfels.hip and raster.hip.
//
// Every float32 operation is individually rounded -- contraction is off for this whole file --, the minimum is an integer minimum and
// every sum is an integer: a call's bits do not depend on scheduling or on the stream.
#include "scene.h"
#include "tuning.h"

#pragma clang fp contract(off)

#include "render_common.h"                 // Geom, the key buffer and its clear, steps 1 to 5 of the contract: shared with surfels.hip

namespace colvo {
namespace {

using namespace render_common;

constexpr int N_STATS = 4;                 // front, drawn, clipped, covered
constexpr int LINE_COVERED = 3;            // a counter line: front, drawn, clipped (the splat's), covered (the resolve's)

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
    const size_t HW = (size_t)g.H * g.W;
    const int n0 = blockIdx.y * FRAME_GROUP, n1 = min(n0 + FRAME_GROUP, g.N);
    for (int n = n0; n < n1; ++n) {
        const Cam c = load_cam(K, M, n);
        const CamPoint p = cam_point(c, g, live, X0, X1, X2);
        int cnt[3] = {(int)__popcll(__ballot(p.front)), 0, 0};
        if (cnt[0]) {                                            // wave-uniform
            const Footprint f = footprint(c, g, p);
            cnt[1] = (int)__popcll(__ballot(f.inside));
            cnt[2] = (int)__popcll(__ballot(f.clipped));
            if (f.inside) {                                      // drawn.  n < N: inside the key buffer
                const unsigned long long key = pack_key(p.Pz, i);
                unsigned long long* frame = keys + (size_t)n * HW;
                for (int v = f.v_lo; v <= f.v_hi; ++v) {
                    unsigned long long* row = frame + (size_t)v * g.W;
                    for (int u = f.u_lo; u <= f.u_hi; ++u) offer_key<LOAD_FIRST>(row + u, key);
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
    const ResolvePixel r = resolve_open(keys, g);
    bool hit = false;
    unsigned idx;
    if (r.in) hit = resolve_pixel(r, colors, out_depth, out_index, out_colors, idx);
    resolve_close(hit, r.n, LINE_COVERED, counters);
}

// grid N, one wave
__global__ __launch_bounds__(64) void k_render_stats(const int32_t* __restrict__ counters, int32_t* __restrict__ out_stats) {
    stats_row<N_STATS, LINE_COVERED, 3>(counters, out_stats);
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
    hipStream_t s = (hipStream_t)stream;
    Geom g;
    Scratch w;
    if (int e = begin_render("colvo_render_cloud", points || M == 0, colors || M == 0, colors, K, cam2world, M, N, H, W, radius, max_splat,
                             max_depth, scratch, out_depth, out_index, out_colors, out_stats, s, g, w))
        return e;
    if (M > 0) {
        launch_draw(k_render_splat<true>, k_render_splat<false>, dim3(blocks_of(M, NT), blocks_of(N, FRAME_GROUP)), s, points, K, cam2world,
                    g, w.keys, w.counters);
        COLVO_CHECK_LAUNCH("k_render_splat");
    }
    colvo::launch(k_render_resolve, dim3(blocks_of((long long)H * W, NT), N), dim3(NT), 0, s, (const unsigned long long*)w.keys, colors, g,
                  out_depth, out_index, out_colors, w.counters);
    COLVO_CHECK_LAUNCH("k_render_resolve");
    colvo::launch(k_render_stats, dim3(N), dim3(64), 0, s, (const int32_t*)w.counters, out_stats);
    COLVO_CHECK_LAUNCH("k_render_stats");
    return 0;
}
