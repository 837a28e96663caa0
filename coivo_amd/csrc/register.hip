// register.hip -- point-cloud registration: a few Gauss-Newton steps of point-to-plane (or point-to-point) ICP that move
// a source cloud onto a target cloud by a Sim(3) or SE(3), starting from the state given.  The target's index is the one
// colvo_cloud_index_build left in its workspace.  Contract: include/colvo.h (colvo_register_*); NumPy replica tests/register_ref.py.
//
//   k_register_init    one thread: the float64 state (R, t, s) to the live state the loop updates, and rounded to the float32 the
//                      per-point pass reads; status ok.
//   k_register_accum   one lane per source point, PER_LANE points per lane: the transform by k_cloud_transform's formula, the nearest
//                      target point by k_cloud_query's walk (cloud_grid.h nearest_key: the one routine), the Jacobian rows and residuals
//                      in float32, the 37 sums in float64 per thread (products of two float32 values are exact in float64, so every fma
//                      is an exact product and one rounded addition), a fixed reduction over the wave, the four waves added in a
//                      fixed tree: one row of 40 doubles per workgroup.  No atomics.
//   k_register_solve   one workgroup: the rows summed in a fixed order; then one thread: damped normal equations, Cholesky in LDS,
//                      closed-form rotation, the update about the pivot, the history row, freeze and revert.
//
// The sums' layout and reduction, the row summation, the solve and the rotation are gauss_newton.h's, shared with refine.hip; the
// per-point arithmetic, the history, the cost in the revert test and the state update are this file's.
//
// Every float32 operation of a sample is individually rounded -- contraction is off for this whole file -- and the order of every
// float64 addition is fixed by the code and a function of N alone: a call's bits do not depend on scheduling or on the stream.
#include "scene.h"

#pragma clang fp contract(off)

#include "cloud_grid.h"
#include "gauss_newton.h"

namespace colvo {
namespace {

using namespace cloud_grid;

constexpr int NT = 256;
constexpr int PER_LANE = 4;                // source points a thread sums before the reduction
constexpr int PER_WG = NT * PER_LANE;
constexpr int N_SUMS = 37;                 // 28 upper-triangle entries of sum J^T J (row-major), 7 of sum J^T r, C, sum r^2
constexpr int OUT_SUMS = 40;               // ... as colvo_register_accumulate delivers them: three zeros behind
constexpr int ROW = 40;                    // doubles per partial row: the sums and three counts (as int64 bits)
constexpr int STATE = 13;                  // R row-major, t, s
constexpr int ST32 = 16;                   // ... rounded to float32, padded
constexpr int NT_SOLVE = 256;
constexpr int GROUPS = NT_SOLVE / 64;
enum { UNKNOWNS_SE3 = 0, UNKNOWNS_SIM3 = 1 };
enum { METRIC_PLANE = 0, METRIC_POINT = 1 };

// one thread
__global__ void k_register_init(const double* __restrict__ state, double* __restrict__ live, float* __restrict__ st32,
                                int32_t* __restrict__ status) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < STATE; ++k) {
        st32[k] = (float)state[k];
        if (live) live[k] = state[k];
    }
    st32[13] = st32[14] = st32[15] = 0.0f;
    if (status) status[0] = gn::OK;
}

// a row of 7 into the sums, and r^2 into the last of them
__device__ __forceinline__ void add_row(const float* J, float r, double* acc) {
    gn::add_row<7, 7>(J, r, acc);
    acc[36] = __builtin_fma((double)r, (double)r, acc[36]);
}

// grid ceil(N / PER_WG).  P [M,3] and Nrm [M,3] are read at the index a record carries, and only where it lies in [0, M).
template <int METRIC>
__global__ __launch_bounds__(NT) void k_register_accum(const float* __restrict__ Q, int N, const float* __restrict__ P,
                                                       const float* __restrict__ Nrm, int M, const Header* __restrict__ h,
                                                       const int32_t* __restrict__ start, const float4* __restrict__ rec, float md2,
                                                       const float* __restrict__ st32, const float* __restrict__ pivot,
                                                       double* __restrict__ rows) {
    __shared__ double red[NT / 64][N_SUMS];
    __shared__ int cnt[NT / 64][3];
    const Grid G = load_grid(h);
    const float* T = st32;
    const float s = T[12];
    const float c[3] = {pivot[0], pivot[1], pivot[2]};
    const double cap = (double)md2;

    double acc[N_SUMS];
#pragma unroll
    for (int k = 0; k < N_SUMS; ++k) acc[k] = 0.0;
    int n_valid = 0, n_reached = 0, n_used = 0;                  // wave totals (uniform)

#pragma unroll 1
    for (int k = 0; k < PER_LANE; ++k) {
        const long long first = ((long long)blockIdx.x * PER_LANE + k) * NT;
        if (first >= N) break;                                   // uniform over the workgroup
        const long long i = first + threadIdx.x;
        const bool in = i < N;
        float x[3] = {0.0f, 0.0f, 0.0f};
        if (in) {
            const float qx = Q[i * 3 + 0], qy = Q[i * 3 + 1], qz = Q[i * 3 + 2];
#pragma unroll
            for (int a = 0; a < 3; ++a) x[a] = ((s * ((T[a * 3 + 0] * qx + T[a * 3 + 1] * qy) + T[a * 3 + 2] * qz)) + T[9 + a]);
        }
        const bool valid = in && finite_f(x[0]) && finite_f(x[1]) && finite_f(x[2]);
        unsigned long long examined = 0ull;
        const unsigned long long best = nearest_key(G, x, valid, start, rec, M, md2, examined);
        const float d2v = __uint_as_float((uint32_t)(best >> 32));
        const int idx = (int)(uint32_t)best;
        const bool reached = valid && idx >= 0 && idx < M;
        float p[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 0.0f, 0.0f};
        if (reached) {
#pragma unroll
            for (int a = 0; a < 3; ++a) p[a] = P[(size_t)idx * 3 + a];
            if (METRIC == METRIC_PLANE) {
#pragma unroll
                for (int a = 0; a < 3; ++a) n[a] = Nrm[(size_t)idx * 3 + a];
            }
        }
        float e[3], y[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            e[a] = x[a] - p[a];
            y[a] = x[a] - c[a];
        }
        n_valid += (int)__popcll(__ballot(valid));
        n_reached += (int)__popcll(__ballot(reached));
        if (METRIC == METRIC_PLANE) {
            const float n2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
            const bool use = reached && n2 > 0.0f;               // NaN fails
            const float r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2];
            float J[7];
            J[0] = n[0];
            J[1] = n[1];
            J[2] = n[2];
            J[3] = (y[1] * n[2]) - (y[2] * n[1]);
            J[4] = (y[2] * n[0]) - (y[0] * n[2]);
            J[5] = (y[0] * n[1]) - (y[1] * n[0]);
            J[6] = (n[0] * y[0] + n[1] * y[1]) + n[2] * y[2];
#pragma unroll
            for (int q = 0; q < 7; ++q) J[q] = use ? J[q] : 0.0f;
            n_used += (int)__popcll(__ballot(use));
            add_row(J, use ? r : 0.0f, acc);                     // an unused sample adds exact zeros
            const double r2 = (double)r * (double)r;
            acc[35] += valid ? (use ? fmin(r2, cap) : cap) : 0.0;
        } else {
            const bool use = reached;
            n_used += (int)__popcll(__ballot(use));
            const float yx = use ? y[0] : 0.0f, yy = use ? y[1] : 0.0f, yz = use ? y[2] : 0.0f, one = use ? 1.0f : 0.0f;
            const float J0[7] = {one, 0.0f, 0.0f, 0.0f, yz, -yy, yx};
            const float J1[7] = {0.0f, one, 0.0f, -yz, 0.0f, yx, yy};
            const float J2[7] = {0.0f, 0.0f, one, yy, -yx, 0.0f, yz};
            add_row(J0, use ? e[0] : 0.0f, acc);
            add_row(J1, use ? e[1] : 0.0f, acc);
            add_row(J2, use ? e[2] : 0.0f, acc);
            acc[35] += valid ? (use ? (double)d2v : cap) : 0.0;
        }
    }

    gn::write_partial_row<N_SUMS>(acc, n_valid, n_reached, n_used, red, cnt, rows + (size_t)blockIdx.x * ROW, gn::RowRotations());
}

struct Solve {
    int iterations, it, min_pairs, unknowns;
    double damping;
};

// one workgroup of NT_SOLVE threads: the rows summed by gn::sum_rows; thread 0 does the rest.  gn::SUMS: the totals to out_sums [40] /
// out_counts [4].  gn::STEP: history row `it`, one Gauss-Newton step on the live state.  gn::FINAL: history row `iterations`, the
// normal matrix, the revert test.
__global__ __launch_bounds__(NT_SOLVE) void k_register_solve(const double* __restrict__ rows, int nrows, int mode, Solve sv,
                                                              const double* __restrict__ init, double* __restrict__ live,
                                                              float* __restrict__ st32, const float* __restrict__ pivot,
                                                              double* __restrict__ history, int32_t* __restrict__ status,
                                                              double* __restrict__ normal, double* __restrict__ out_sums,
                                                              long long* __restrict__ out_counts) {
    __shared__ double part[GROUPS][ROW];
    __shared__ double tot[ROW];
    __shared__ double A[7][7];                                   // the normal matrix, then its Cholesky factor (lower)
    __shared__ double xs[7];
    gn::sum_rows<N_SUMS, ROW, GROUPS>(rows, nrows, false, part, tot);
    if (mode == gn::SUMS) {
        if (threadIdx.x < OUT_SUMS) out_sums[threadIdx.x] = threadIdx.x < N_SUMS ? tot[threadIdx.x] : 0.0;
        if (threadIdx.x < 4) out_counts[threadIdx.x] = threadIdx.x < 3 ? (long long)tot[N_SUMS + threadIdx.x] : 0ll;
        return;
    }
    if (threadIdx.x != 0) return;

    const double n_valid = tot[N_SUMS], n_used = tot[N_SUMS + 2];
    double* h = history + (size_t)sv.it * 5;
    h[0] = n_valid;
    h[1] = tot[N_SUMS + 1];
    h[2] = n_used;
    h[3] = tot[35];
    h[4] = tot[36];
    if (mode == gn::FINAL) {
        int idx = 0;
        for (int k = 0; k < 7; ++k)
            for (int l = k; l < 7; ++l, ++idx) normal[k * 7 + l] = normal[l * 7 + k] = tot[idx];
    }
    int st = status[0];
    if (st != gn::OK) return;                                    // frozen: the state is the initial one already

    bool restore = false;
    if (mode == gn::FINAL) {
        const double F1 = tot[35] / n_valid, F0 = history[3] / history[0];
        if (F1 > F0) {                                           // (NaN: no revert)
            st = gn::REVERTED;
            restore = true;
        }
    } else if (n_used < (double)sv.min_pairs) {
        st = gn::TOO_FEW;
        restore = true;
    } else {
        const int n = sv.unknowns == UNKNOWNS_SIM3 ? 7 : 6;
        if (!gn::solve_damped<7>(A, xs, tot, n, sv.damping)) {
            st = gn::NOT_PD;
            restore = true;
        } else {
            // R <- Exp(omega) R, t <- e^sigma Exp(omega) (t - c) + c + v, s <- e^sigma s
            double Rx[3][3];
            gn::rot_exp(xs[3], xs[4], xs[5], Rx, nullptr);
            const double es = n == 7 ? exp(xs[6]) : 1.0;
            const double piv[3] = {(double)pivot[0], (double)pivot[1], (double)pivot[2]};
            const double vv[3] = {xs[0], xs[1], xs[2]};
            double Rn[9], tn[3];
            const double d[3] = {live[9] - piv[0], live[10] - piv[1], live[11] - piv[2]};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) Rn[r * 3 + c] = (Rx[r][0] * live[c] + Rx[r][1] * live[3 + c]) + Rx[r][2] * live[6 + c];
                tn[r] = ((es * ((Rx[r][0] * d[0] + Rx[r][1] * d[1]) + Rx[r][2] * d[2])) + piv[r]) + vv[r];
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) live[k] = Rn[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) live[9 + k] = tn[k];
            if (n == 7) live[12] = es * live[12];
        }
    }
    if (restore) {
#pragma unroll
        for (int k = 0; k < STATE; ++k) live[k] = init[k];
    }
    status[0] = st;
#pragma unroll
    for (int k = 0; k < STATE; ++k) st32[k] = (float)live[k];
}

struct Scratch {
    double* rows;                          // [ceil(N / PER_WG)][ROW]
    float* st32;                           // [ST32]
    int32_t* status;                       // [4] (colvo_register_accumulate; the loop uses its own output)
    size_t bytes;
};

Scratch carve(void* base, int N) {
    Carver c(base);
    Scratch w;
    w.rows = c.take<double>((size_t)blocks_of(N, PER_WG) * ROW);
    w.st32 = c.take<float>(ST32);
    w.status = c.take<int32_t>(4);
    w.bytes = c.bytes();
    return w;
}

struct Clouds {
    const float *Q, *P, *Nrm;
    int N, M;
    float max_dist;
    const void* index;
    const float* pivot;
    int metric;
};

// what both calls refuse; md2 out
int check_clouds(const char* who, const Clouds& a, const void* workspace, float& md2) {
    COLVO_CHECK_ARG(a.index && a.pivot && workspace && (a.Q || a.N == 0) && (a.P || a.M == 0), "%s: null pointer argument", who);
    COLVO_CHECK_ARG(a.metric == METRIC_PLANE || a.metric == METRIC_POINT, "%s: bad metric %d (0 plane, 1 point)", who, a.metric);
    COLVO_CHECK_ARG(a.Nrm || a.M == 0 || a.metric == METRIC_POINT, "%s: null pointer argument: the plane metric needs the target's normals",
                    who);
    COLVO_CHECK_ARG(good_sizes(a.N, a.M), "%s: bad shape N=%d M=%d (0 .. 2^30 - 1)", who, a.N, a.M);
    float scale;
    COLVO_CHECK_ARG(good_max_dist(a.max_dist, md2, scale), "%s: bad max_dist %g (finite, positive, with a finite positive float32 square)",
                    who, (double)a.max_dist);
    COLVO_CHECK_ARG(aligned16(workspace) && aligned16(a.index), "%s: workspace and index must be 16-byte aligned", who);
    return 0;
}

int launch_accum(const Clouds& a, float md2, const Scratch& w, hipStream_t s) {
    if (a.N == 0) return 0;                                      // no row: the solve sums nothing
    const cloud_grid::Ws ix = layout(const_cast<void*>(a.index), a.M);
    const dim3 grid(blocks_of(a.N, PER_WG));
    if (a.metric == METRIC_PLANE)
        colvo::launch(k_register_accum<METRIC_PLANE>, grid, dim3(NT), 0, s, a.Q, a.N, a.P, a.Nrm, a.M, (const Header*)ix.header,
                      (const int32_t*)ix.cells, (const float4*)ix.rec, md2, (const float*)w.st32, a.pivot, w.rows);
    else
        colvo::launch(k_register_accum<METRIC_POINT>, grid, dim3(NT), 0, s, a.Q, a.N, a.P, a.Nrm, a.M, (const Header*)ix.header,
                      (const int32_t*)ix.cells, (const float4*)ix.rec, md2, (const float*)w.st32, a.pivot, w.rows);
    COLVO_CHECK_LAUNCH("k_register_accum");
    return 0;
}

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" size_t colvo_register_scratch_bytes(int N) {
    if (!good_sizes(N, 0)) return 0;
    return carve(nullptr, N).bytes;
}

extern "C" int colvo_register_accumulate(const float* source, int N, const float* target, const float* normals, int M, float max_dist,
                                         const void* index, const double* state, const float* pivot, int metric, void* workspace,
                                         double* out_sums, int64_t* out_counts, colvo_stream_t stream) {
    const Clouds a{source, target, normals, N, M, max_dist, index, pivot, metric};
    COLVO_CHECK_ARG(state && out_sums && out_counts, "colvo_register_accumulate: null pointer argument");
    float md2;
    if (int rc = check_clouds("colvo_register_accumulate", a, workspace, md2)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Scratch w = carve(workspace, N);
    colvo::launch(k_register_init, dim3(1), dim3(64), 0, s, state, (double*)nullptr, w.st32, w.status);
    COLVO_CHECK_LAUNCH("k_register_init");
    if (int rc = launch_accum(a, md2, w, s)) return rc;
    Solve sv{};
    colvo::launch(k_register_solve, dim3(1), dim3(NT_SOLVE), 0, s, (const double*)w.rows, blocks_of(N, PER_WG), gn::SUMS, sv,
                  (const double*)nullptr, (double*)nullptr, (float*)nullptr, pivot, (double*)nullptr, w.status, (double*)nullptr,
                  out_sums, reinterpret_cast<long long*>(out_counts));
    COLVO_CHECK_LAUNCH("k_register_solve");
    return 0;
}

extern "C" int colvo_register_clouds(const float* source, int N, const float* target, const float* normals, int M, float max_dist,
                                     const void* index, const double* state_init, const float* pivot, int mode, int metric,
                                     int iterations, double damping, int min_pairs, void* workspace, double* out_state, double* history,
                                     int32_t* status, double* normal_matrix, colvo_stream_t stream) {
    const Clouds a{source, target, normals, N, M, max_dist, index, pivot, metric};
    COLVO_CHECK_ARG(state_init && out_state && history && status && normal_matrix, "colvo_register_clouds: null pointer argument");
    float md2;
    if (int rc = check_clouds("colvo_register_clouds", a, workspace, md2)) return rc;
    COLVO_CHECK_ARG(mode == UNKNOWNS_SE3 || mode == UNKNOWNS_SIM3, "colvo_register_clouds: bad mode %d (0 se3, 1 sim3)", mode);
    if (int rc = gn::check_loop("colvo_register_clouds", iterations, damping, "min_pairs", min_pairs)) return rc;
    COLVO_CHECK_ARG(out_state != state_init, "colvo_register_clouds: out_state must not alias state_init");
    hipStream_t s = (hipStream_t)stream;
    const Scratch w = carve(workspace, N);
    colvo::launch(k_register_init, dim3(1), dim3(64), 0, s, state_init, out_state, w.st32, status);
    COLVO_CHECK_LAUNCH("k_register_init");
    Solve sv;
    sv.iterations = iterations;
    sv.min_pairs = min_pairs;
    sv.unknowns = mode;
    sv.damping = damping;
    for (int it = 0; it <= iterations; ++it) {
        if (int rc = launch_accum(a, md2, w, s)) return rc;
        sv.it = it;
        colvo::launch(k_register_solve, dim3(1), dim3(NT_SOLVE), 0, s, (const double*)w.rows, blocks_of(N, PER_WG),
                      it < iterations ? gn::STEP : gn::FINAL, sv, state_init, out_state, w.st32, pivot, history, status,
                      normal_matrix, (double*)nullptr, (long long*)nullptr);
        COLVO_CHECK_LAUNCH("k_register_solve");
    }
    return 0;
}
