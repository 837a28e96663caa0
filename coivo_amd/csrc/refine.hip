// refine.hip -- pose refinement by dense depth and intensity alignment: a few Gauss-Newton steps per edge (i, j, T) on
// the per-pixel geometric and photometric residuals of the pair, starting from the pose given.  Contract: include/colvo.h (colvo_refine_*).
//
//   k_refine_grey    one thread per pixel: the grey plane of every frame, g = ((r + g) + b) * (1/3).
//   k_refine_init    one thread per edge: checks the edge, rounds its float64 state to the float32 the per-pixel pass reads.
//   k_refine_accum   grid (strips, E), a wave per 8x8 tile, TILES_PER_WAVE tiles per wave: projection and taps as k_consist_filter, the
//                    two whitened rows and residuals in float32, the 46 sums in float64 per thread (products of two float32 values are
//                    exact in float64, so every fma is an exact product and one rounded addition), a fixed butterfly over the
//                    wave, the four waves added in a fixed tree: one row of 52 doubles per workgroup.  No atomics.
//   k_refine_solve   one workgroup per edge: the rows summed in a fixed order; then one thread: damped normal equations, Cholesky in
//                    LDS, closed-form SE(3) exponential, the update, the history row, freeze and revert.
//
// The sums' layout and reduction, the row summation, the solve and the rotation are gauss_newton.h's, shared with register.hip; the
// per-sample arithmetic, the history, the cost in the revert test and the state update are this file's.
//
// Every float32 operation of a sample is individually rounded -- contraction is off for this whole file -- and the order of every
// float64 addition is fixed by the code: a call's bits do not depend on scheduling or on the stream.
#include "scene.h"
#include "tuning.h"

#pragma clang fp contract(off)

#include "gauss_newton.h"

namespace colvo {
namespace {

constexpr int NT = 256;
constexpr int TILE = 8;                    // a wave owns TILE x TILE pixels at a time
constexpr int TILES_PER_WAVE = 4;          // ... and walks this many: a thread sums four samples before the reduction
constexpr int TILES_PER_WG = TILES_PER_WAVE * (NT / 64);
constexpr int N_SUMS = 46;                 // 36 upper-triangle entries of sum J^T J (row-major), 8 of sum J^T e, C_g, C_p
constexpr int ROW = 52;                    // doubles per partial row: the sums, three counts (as int64 bits), pad
constexpr int STATE = 16;                  // values per edge state: R row-major, t, a, b, pad
constexpr int NT_SOLVE = 512;
constexpr int GROUPS = NT_SOLVE / 64;
constexpr float Z_EPS = 1e-3f;
constexpr int ST_BAD_EDGE = 4;             // beside gn::OK .. gn::REVERTED
enum { FLAG_GEO = 1, FLAG_PHOTO = 2, FLAG_BRIGHT = 4 };

struct Geom {
    int N, H, W, E, tiles_x, tiles, strips;
};

struct Policy {
    float max_depth, inv_sg, inv_sp, gate_geo, gate_photo;
    int flags;
    double cap_g, cap_p;                   // (gate / sigma)^2 of the float32 quotient's stand-in gate * (1 / sigma)
};

// grid (ceil(HW / NT), N)
__global__ __launch_bounds__(NT) void k_refine_grey(const float* __restrict__ frames, int HW, float* __restrict__ grey) {
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= HW) return;
    const float* f = frames + (size_t)blockIdx.y * 3 * HW + p;
    grey[(size_t)blockIdx.y * HW + p] = ((f[0] + f[HW]) + f[2 * (size_t)HW]) * (1.0f / 3.0f);
}

// grid ceil(E / NT).  T [E][4][4] float64 (rows 0..2 are read), gain / offset [E] or NULL (1 and 0).  Writes the float32 state, the
// status (bad edge or ok) and -- where given -- the live float64 state the loop updates in place.
__global__ __launch_bounds__(NT) void k_refine_init(const int32_t* __restrict__ edges, const double* __restrict__ T,
                                                    const double* __restrict__ gain, const double* __restrict__ offset, int E, int N,
                                                    float* __restrict__ st32, int32_t* __restrict__ status, double* __restrict__ live_T,
                                                    double* __restrict__ live_gain, double* __restrict__ live_offset) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= E) return;
    const int i = edges[2 * e], j = edges[2 * e + 1];
    status[e] = (i >= 0 && i < N && j >= 0 && j < N && i != j) ? gn::OK : ST_BAD_EDGE;
    const double* t = T + (size_t)e * 16;
    float* s = st32 + (size_t)e * STATE;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[r * 3 + c] = (float)t[r * 4 + c];
        s[9 + r] = (float)t[r * 4 + 3];
    }
    const double a = gain ? gain[e] : 1.0, b = offset ? offset[e] : 0.0;
    s[12] = (float)a;
    s[13] = (float)b;
    s[14] = s[15] = 0.0f;
    if (live_T) {
#pragma unroll
        for (int k = 0; k < 12; ++k) live_T[(size_t)e * 16 + k] = t[k];
        live_T[(size_t)e * 16 + 12] = live_T[(size_t)e * 16 + 13] = live_T[(size_t)e * 16 + 14] = 0.0;
        live_T[(size_t)e * 16 + 15] = 1.0;
        live_gain[e] = a;
        live_offset[e] = b;
    }
}

// gradient of an image-plane quantity with respect to P: (gx fx / Pz, gy fy / Pz, -(gx fx Px + gy fy Py) / Pz^2)
__device__ __forceinline__ void grad_P(float gx, float gy, float fx, float fy, float Px, float Py, float iz, float* G) {
    const float A = gx * fx, B = gy * fy;
    G[0] = A * iz;
    G[1] = B * iz;
    G[2] = -((((A * Px) + (B * Py)) * iz) * iz);
}

// row[3..5] = P x row[0..2]
__device__ __forceinline__ void cross_P(float Px, float Py, float Pz, float* row) {
    row[3] = (Py * row[2]) - (Pz * row[1]);
    row[4] = (Pz * row[0]) - (Px * row[2]);
    row[5] = (Px * row[1]) - (Py * row[0]);
}

// grid (strips, E)
__global__ __launch_bounds__(NT) void k_refine_accum(const float* __restrict__ depth, const float* __restrict__ grey,
                                                     const float* __restrict__ K, const int32_t* __restrict__ edges,
                                                     const float* __restrict__ st32, const int32_t* __restrict__ status, Geom g, Policy p,
                                                     double* __restrict__ rows) {
    __shared__ double red[NT / 64][N_SUMS];
    __shared__ int cnt[NT / 64][3];
    const int e = blockIdx.y;
    if (status[e] == ST_BAD_EDGE) return;                        // uniform; k_refine_solve does not read this edge's rows
    const int i = __builtin_amdgcn_readfirstlane(edges[2 * e]), j = __builtin_amdgcn_readfirstlane(edges[2 * e + 1]);   // both in [0, N)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t HW = (size_t)g.H * g.W;
    const float* T = st32 + (size_t)e * STATE;
    const float a = T[12], b = T[13];
    const float* Ki = K + (size_t)i * 9;
    const float* Kj = K + (size_t)j * 9;
    const float fxi = Ki[0], fyi = Ki[4], cxi = Ki[2], cyi = Ki[5];
    const float fx = Kj[0], fy = Kj[4], cx = Kj[2], cy = Kj[5];
    const float* di = depth + (size_t)i * HW;
    const float* dj = depth + (size_t)j * HW;
    const float* gi = grey + (size_t)i * HW;
    const float* gj = grey + (size_t)j * HW;
    const bool geo_on = p.flags & FLAG_GEO, photo_on = p.flags & FLAG_PHOTO;

    double acc[N_SUMS];
#pragma unroll
    for (int k = 0; k < N_SUMS; ++k) acc[k] = 0.0;
    int n_vis = 0, n_geo = 0, n_photo = 0;                       // wave totals (uniform)

#pragma unroll 1
    for (int k = 0; k < TILES_PER_WAVE; ++k) {
        const int tile = (blockIdx.x * TILES_PER_WAVE + k) * (NT / 64) + wave;
        if (tile >= g.tiles) break;                              // uniform over the wave
        const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
        const int u = tx * TILE + (lane & 7), v = ty * TILE + (lane >> 3);
        const bool in = u < g.W && v < g.H;
        const size_t pix = in ? (size_t)v * g.W + u : 0;
        const float d = in ? di[pix] : 0.0f;
        const float Ii = gi[pix];
        const bool cand = in && valid_depth(d, p.max_depth);
        const float px = (((float)u - cxi) / fxi) * d;
        const float py = (((float)v - cyi) / fyi) * d;
        const float Px = ((T[0] * px + T[1] * py) + T[2] * d) + T[9];
        const float Py = ((T[3] * px + T[4] * py) + T[5] * d) + T[10];
        const float Pz = ((T[6] * px + T[7] * py) + T[8] * d) + T[11];
        const bool front = Pz > Z_EPS;
        const float x = (fx * Px) / Pz + cx;
        const float y = (fy * Py) / Pz + cy;
        const bool seen = cand && front && x >= 0.0f && x <= (float)(g.W - 1) && y >= 0.0f && y <= (float)(g.H - 1);      // NaN fails
        const float x0f = floorf(x), y0f = floorf(y);
        const float wx = x - x0f, wy = y - y0f;
        const int x0 = seen ? (int)x0f : 0, y0 = seen ? (int)y0f : 0;        // in [0, W-1] x [0, H-1]
        const int x1 = min(x0 + 1, g.W - 1), y1 = min(y0 + 1, g.H - 1);
        const size_t o00 = (size_t)y0 * g.W + x0, o01 = (size_t)y0 * g.W + x1, o10 = (size_t)y1 * g.W + x0, o11 = (size_t)y1 * g.W + x1;
        const float t00 = dj[o00], t01 = dj[o01], t10 = dj[o10], t11 = dj[o11];
        const float c00 = gj[o00], c01 = gj[o01], c10 = gj[o10], c11 = gj[o11];
        const bool visible = (int)seen & (int)valid_depth(t00, p.max_depth) & (int)valid_depth(t01, p.max_depth) &
                             (int)valid_depth(t10, p.max_depth) & (int)valid_depth(t11, p.max_depth);
        const float ax = 1.0f - wx, ay = 1.0f - wy;
        const float s = (((t00 * ax) + (t01 * wx)) * ay) + (((t10 * ax) + (t11 * wx)) * wy);
        const float c = (((c00 * ax) + (c01 * wx)) * ay) + (((c10 * ax) + (c11 * wx)) * wy);
        const float sx = ((t01 - t00) * ay) + ((t11 - t10) * wy);
        const float sy = ((t10 - t00) * ax) + ((t11 - t01) * wx);
        const float gcx = ((c01 - c00) * ay) + ((c11 - c10) * wy);
        const float gcy = ((c10 - c00) * ax) + ((c11 - c01) * wx);
        const float iz = 1.0f / Pz;
        n_vis += (int)__popcll(__ballot(visible));

        if (geo_on) {
            const float den = Pz + s;
            const float rel = (Pz - s) / den;
            const float k2 = 2.0f / (den * den);
            float G[3], J[6];
            grad_P(sx, sy, fx, fy, Px, Py, iz, G);
            J[0] = -(k2 * (Pz * G[0]));
            J[1] = -(k2 * (Pz * G[1]));
            J[2] = k2 * (s - (Pz * G[2]));
            cross_P(Px, Py, Pz, J);
            const float eg = rel * p.inv_sg;
            const bool use = visible && fabsf(rel) < p.gate_geo;
#pragma unroll
            for (int q = 0; q < 6; ++q) J[q] = use ? J[q] * p.inv_sg : 0.0f;
            n_geo += (int)__popcll(__ballot(use));
            gn::add_row<6, 8>(J, use ? eg : 0.0f, acc);          // an unused sample adds exact zeros; a branch around this
                                                                 // cost 116 AGPRs of copies at the join
            const double e2 = (double)eg * (double)eg;
            acc[44] += visible ? fmin(e2, p.cap_g) : 0.0;
        }
        if (photo_on) {
            const float rI = ((a * c) + b) - Ii;
            float G[3], J[8];
            grad_P(gcx, gcy, fx, fy, Px, Py, iz, G);
            J[0] = a * G[0];
            J[1] = a * G[1];
            J[2] = a * G[2];
            cross_P(Px, Py, Pz, J);
            J[6] = c;
            J[7] = 1.0f;
            const float ep = rI * p.inv_sp;
            const bool use = visible && fabsf(rI) < p.gate_photo;
#pragma unroll
            for (int q = 0; q < 8; ++q) J[q] = use ? J[q] * p.inv_sp : 0.0f;
            n_photo += (int)__popcll(__ballot(use));
            gn::add_row<8, 8>(J, use ? ep : 0.0f, acc);
            const double e2 = (double)ep * (double)ep;
            acc[45] += visible ? fmin(e2, p.cap_p) : 0.0;
        }
    }

    gn::write_partial_row<N_SUMS>(acc, n_vis, n_geo, n_photo, red, cnt, rows + ((size_t)e * g.strips + blockIdx.x) * ROW,
                                  gn::XorButterfly());
}

struct Solve {
    int iterations, it, min_samples, flags;
    double damping;
};

// grid E, NT_SOLVE threads: the rows of the edge summed by gn::sum_rows (none of a bad edge); thread 0 does the rest.  gn::SUMS: the
// totals to out_sums [E][48] / out_counts [E][4].  gn::STEP: history row `it`, one Gauss-Newton step on the live state.  gn::FINAL:
// history row `iterations`, the revert test.
__global__ __launch_bounds__(NT_SOLVE) void k_refine_solve(const double* __restrict__ rows, int strips, int mode, Solve sv,
                                                            const double* __restrict__ T_init, double* __restrict__ live_T,
                                                            double* __restrict__ live_gain, double* __restrict__ live_offset,
                                                            float* __restrict__ st32, double* __restrict__ history,
                                                            int32_t* __restrict__ status, double* __restrict__ out_sums,
                                                            int32_t* __restrict__ out_counts) {
    __shared__ double part[GROUPS][ROW];
    __shared__ double tot[ROW];
    __shared__ double A[8][8];                                   // the normal matrix, then its Cholesky factor (lower)
    __shared__ double xs[8];
    const int e = blockIdx.x;
    gn::sum_rows<N_SUMS, ROW, GROUPS>(rows + (size_t)e * strips * ROW, strips, status[e] == ST_BAD_EDGE, part, tot);
    if (mode == gn::SUMS) {
        if (threadIdx.x < 48) out_sums[(size_t)e * 48 + threadIdx.x] = threadIdx.x < N_SUMS ? tot[threadIdx.x] : 0.0;
        if (threadIdx.x < 4) out_counts[(size_t)e * 4 + threadIdx.x] = threadIdx.x < 3 ? (int)tot[N_SUMS + threadIdx.x] : 0;
        return;
    }
    if (threadIdx.x != 0) return;

    const double n_vis = tot[N_SUMS];
    double* h = history + ((size_t)e * (sv.iterations + 1) + sv.it) * 5;
    h[0] = n_vis;
    h[1] = tot[N_SUMS + 1];
    h[2] = tot[44];
    h[3] = tot[N_SUMS + 2];
    h[4] = tot[45];
    int st = status[e];
    if (st != gn::OK) return;                                    // frozen: the state is the initial one already

    double* Tl = live_T + (size_t)e * 16;
    bool restore = false;
    if (mode == gn::FINAL) {
        const double* h0 = history + (size_t)e * (sv.iterations + 1) * 5;
        const double F1 = (tot[44] + tot[45]) / n_vis, F0 = (h0[2] + h0[4]) / h0[0];
        if (F1 > F0) {                                           // (NaN: no revert)
            st = gn::REVERTED;
            restore = true;
        }
    } else if (n_vis < (double)sv.min_samples) {
        st = gn::TOO_FEW;
        restore = true;
    } else {
        const int n = ((sv.flags & FLAG_PHOTO) && (sv.flags & FLAG_BRIGHT)) ? 8 : 6;
        if (!gn::solve_damped<8>(A, xs, tot, n, sv.damping)) {
            st = gn::NOT_PD;
            restore = true;
        } else {
            // T <- exp(delta_1..6) T
            const double u0 = xs[0], u1 = xs[1], u2 = xs[2];
            double Rx[3][3], V[3][3];
            gn::rot_exp(xs[3], xs[4], xs[5], Rx, V);
            double Tn[12];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    Tn[r * 4 + c] = (Rx[r][0] * Tl[c] + Rx[r][1] * Tl[4 + c]) + Rx[r][2] * Tl[8 + c];
                Tn[r * 4 + 3] += (V[r][0] * u0 + V[r][1] * u1) + V[r][2] * u2;
            }
#pragma unroll
            for (int k = 0; k < 12; ++k) Tl[k] = Tn[k];
            if (n == 8) {
                live_gain[e] += xs[6];
                live_offset[e] += xs[7];
            }
        }
    }
    if (restore) {
        const double* t0 = T_init + (size_t)e * 16;
#pragma unroll
        for (int k = 0; k < 12; ++k) Tl[k] = t0[k];
        live_gain[e] = 1.0;
        live_offset[e] = 0.0;
    }
    status[e] = st;
    float* s32 = st32 + (size_t)e * STATE;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s32[r * 3 + c] = (float)Tl[r * 4 + c];
        s32[9 + r] = (float)Tl[r * 4 + 3];
    }
    s32[12] = (float)live_gain[e];
    s32[13] = (float)live_offset[e];
}

bool shape_ok(int E, int N, int H, int W) {
    return E > 0 && E <= 65535 && N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 30);
}

Geom make_geom(int E, int N, int H, int W) {
    Geom g;
    g.N = N; g.H = H; g.W = W; g.E = E;
    g.tiles_x = blocks_of(W, TILE);
    g.tiles = g.tiles_x * blocks_of(H, TILE);
    g.strips = blocks_of(g.tiles, TILES_PER_WG);
    return g;
}

struct Ws {
    double* rows;                          // [E][strips][ROW]
    float* grey;                           // [N][H*W]
    float* st32;                           // [E][STATE]
    int32_t* status;                       // [E] (colvo_refine_accumulate; the loop uses its own output)
    size_t bytes;
};

Ws carve(void* base, const Geom& g) {
    Carver c(base);
    Ws w;
    w.rows = c.take<double>((size_t)g.E * g.strips * ROW);
    w.grey = c.take<float>((size_t)g.N * g.H * g.W);
    w.st32 = c.take<float>((size_t)g.E * STATE);
    w.status = c.take<int32_t>(g.E);
    w.bytes = c.bytes();
    return w;
}

bool pos_finite(float v) { return v > 0.0f && v < __builtin_inff(); }

int check_policy(const char* who, float sigma_geo, float sigma_photo, float gate_geo, float gate_photo, float max_depth, int flags) {
    COLVO_CHECK_ARG(pos_finite(sigma_geo) && pos_finite(sigma_photo) && pos_finite(gate_geo) && pos_finite(gate_photo) &&
                        pos_finite(max_depth),
                    "%s: sigma_geo %g, sigma_photo %g, gate_geo %g, gate_photo %g and max_depth %g must be finite and positive", who,
                    (double)sigma_geo, (double)sigma_photo, (double)gate_geo, (double)gate_photo, (double)max_depth);
    COLVO_CHECK_ARG((flags & ~7) == 0 && (flags & (FLAG_GEO | FLAG_PHOTO)) != 0,
                    "%s: bad terms %d (bit 0 geometric, bit 1 photometric, bit 2 brightness; at least one term)", who, flags);
    return 0;
}

Policy make_policy(float sigma_geo, float sigma_photo, float gate_geo, float gate_photo, float max_depth, int flags) {
    Policy p;
    p.max_depth = max_depth;
    p.inv_sg = 1.0f / sigma_geo;
    p.inv_sp = 1.0f / sigma_photo;
    p.gate_geo = gate_geo;
    p.gate_photo = gate_photo;
    p.flags = flags;
    const float tg = gate_geo * p.inv_sg, tp = gate_photo * p.inv_sp;
    p.cap_g = (double)tg * (double)tg;
    p.cap_p = (double)tp * (double)tp;
    return p;
}

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" size_t colvo_refine_workspace_bytes(int E, int N, int H, int W, int iterations) {
    if (!shape_ok(E, N, H, W) || iterations < 0 || iterations > 64) return 0;
    return carve(nullptr, make_geom(E, N, H, W)).bytes;
}

extern "C" int colvo_refine_accumulate(const float* depths, const float* frames, const float* K, int N, int H, int W,
                                       const int32_t* edges, int E, const double* T, const double* gain, const double* offset,
                                       float sigma_geo, float sigma_photo, float gate_geo, float gate_photo, int terms, float max_depth,
                                       void* workspace, double* out_sums, int32_t* out_counts, colvo_stream_t stream) {
    COLVO_CHECK_ARG(depths && frames && K && edges && T && workspace && out_sums && out_counts,
                    "colvo_refine_accumulate: null pointer argument");
    COLVO_CHECK_ARG(shape_ok(E, N, H, W), "colvo_refine_accumulate: bad shape E=%d N=%d H=%d W=%d", E, N, H, W);
    if (int rc = check_policy("colvo_refine_accumulate", sigma_geo, sigma_photo, gate_geo, gate_photo, max_depth, terms)) return rc;
    COLVO_CHECK_ARG(aligned16(workspace), "colvo_refine_accumulate: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const Geom g = make_geom(E, N, H, W);
    const Ws w = carve(workspace, g);
    const Policy p = make_policy(sigma_geo, sigma_photo, gate_geo, gate_photo, max_depth, terms);
    const int HW = H * W;
    colvo::launch(k_refine_grey, dim3(blocks_of(HW, NT), N), dim3(NT), 0, s, frames, HW, w.grey);
    COLVO_CHECK_LAUNCH("k_refine_grey");
    colvo::launch(k_refine_init, dim3(blocks_of(E, NT)), dim3(NT), 0, s, edges, T, gain, offset, E, N, w.st32, w.status,
                  (double*)nullptr, (double*)nullptr, (double*)nullptr);
    COLVO_CHECK_LAUNCH("k_refine_init");
    colvo::launch(k_refine_accum, dim3(g.strips, E), dim3(NT), 0, s, depths, (const float*)w.grey, K, edges, (const float*)w.st32,
                  (const int32_t*)w.status, g, p, w.rows);
    COLVO_CHECK_LAUNCH("k_refine_accum");
    Solve sv{};
    colvo::launch(k_refine_solve, dim3(E), dim3(NT_SOLVE), 0, s, (const double*)w.rows, g.strips, gn::SUMS, sv,
                  (const double*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr, (float*)nullptr, (double*)nullptr,
                  w.status, out_sums, out_counts);
    COLVO_CHECK_LAUNCH("k_refine_solve");
    return 0;
}

extern "C" int colvo_refine_edges(const float* depths, const float* frames, const float* K, int N, int H, int W, const int32_t* edges,
                                  int E, const double* T_init, int iterations, float sigma_geo, float sigma_photo, float gate_geo,
                                  float gate_photo, double damping, int min_samples, int terms, float max_depth, void* workspace,
                                  double* out_T, double* out_gain, double* out_offset, double* history, int32_t* status,
                                  colvo_stream_t stream) {
    COLVO_CHECK_ARG(depths && frames && K && edges && T_init && workspace && out_T && out_gain && out_offset && history && status,
                    "colvo_refine_edges: null pointer argument");
    COLVO_CHECK_ARG(shape_ok(E, N, H, W), "colvo_refine_edges: bad shape E=%d N=%d H=%d W=%d", E, N, H, W);
    if (int rc = check_policy("colvo_refine_edges", sigma_geo, sigma_photo, gate_geo, gate_photo, max_depth, terms)) return rc;
    if (int rc = gn::check_loop("colvo_refine_edges", iterations, damping, "min_samples", min_samples)) return rc;
    COLVO_CHECK_ARG(aligned16(workspace), "colvo_refine_edges: workspace must be 16-byte aligned");
    COLVO_CHECK_ARG(out_T != T_init, "colvo_refine_edges: out_T must not alias T_init");
    hipStream_t s = (hipStream_t)stream;
    const Geom g = make_geom(E, N, H, W);
    const Ws w = carve(workspace, g);
    const Policy p = make_policy(sigma_geo, sigma_photo, gate_geo, gate_photo, max_depth, terms);
    const int HW = H * W;
    colvo::launch(k_refine_grey, dim3(blocks_of(HW, NT), N), dim3(NT), 0, s, frames, HW, w.grey);
    COLVO_CHECK_LAUNCH("k_refine_grey");
    colvo::launch(k_refine_init, dim3(blocks_of(E, NT)), dim3(NT), 0, s, edges, T_init, (const double*)nullptr, (const double*)nullptr,
                  E, N, w.st32, status, out_T, out_gain, out_offset);
    COLVO_CHECK_LAUNCH("k_refine_init");
    Solve sv;
    sv.iterations = iterations;
    sv.min_samples = min_samples;
    sv.flags = terms;
    sv.damping = damping;
    for (int it = 0; it <= iterations; ++it) {
        colvo::launch(k_refine_accum, dim3(g.strips, E), dim3(NT), 0, s, depths, (const float*)w.grey, K, edges, (const float*)w.st32,
                      (const int32_t*)status, g, p, w.rows);
        COLVO_CHECK_LAUNCH("k_refine_accum");
        sv.it = it;
        colvo::launch(k_refine_solve, dim3(E), dim3(NT_SOLVE), 0, s, (const double*)w.rows, g.strips,
                      it < iterations ? gn::STEP : gn::FINAL, sv, T_init, out_T, out_gain, out_offset, w.st32, history, status,
                      (double*)nullptr, (int32_t*)nullptr);
        COLVO_CHECK_LAUNCH("k_refine_solve");
    }
    return 0;
}
