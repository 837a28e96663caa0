// gauss_newton.h -- the Gauss-Newton core that refine.hip and register.hip (§3.6l) run around their own per-sample
// passes: the float64 sums of exact float32 products, their fixed-order reduction to one partial row per workgroup, the ordered sum of
// the rows, the damped Cholesky solve and the closed-form rotation.  Included by those two files only.  Every operation below is
// individually rounded in the order written, PINNED against tests/refine_ref.py (`solve`, `cholesky_solve`, `se3_exp`).
//
// The arithmetic part is plain C++: tests/cpp/gn_solve.cpp compiles it with g++, no HIP header, and holds it to the replica bit for
// bit.  Contraction: this header does not rely on its includer.  It carries the pragma itself (clang's at file scope, which holds for
// every function below and to the end of the translation unit; g++'s `optimize` pragma for the functions below) and does not compile
// with a compiler that has neither.
#pragma once
#include <math.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#else
#error "gauss_newton.h: no way to switch floating-point contraction off with this compiler"
#endif

#ifdef __HIPCC__
#include "common.h"
#define COLVO_GN_FN __host__ __device__ __forceinline__
#else
#define COLVO_GN_FN inline
#endif

namespace colvo {
namespace gn {

// status of a loop (refine.hip adds its own ST_BAD_EDGE = 4) and what a call of a solve kernel is for
constexpr int OK = 0, TOO_FEW = 1, NOT_PD = 2, REVERTED = 3;
constexpr int SUMS = 0, STEP = 1, FINAL = 2;

// x with (H + damping diag(H)) x = -g over the first n unknowns, by Cholesky.  tot: the LD (LD + 1) / 2 upper-triangle sums of H,
// row-major, then g.  A [LD][LD] and xs [LD] are the caller's (LDS on the device): A takes the matrix in its upper half and the factor
// in its lower half and diagonal, xs the solution.  false at the first pivot that is not positive (NaN included).
template <int LD>
COLVO_GN_FN bool solve_damped(double (*A)[LD], double* xs, const double* tot, int n, double damping) {
    int idx = 0;
    for (int k = 0; k < LD; ++k)
        for (int l = k; l < LD; ++l, ++idx) A[k][l] = tot[idx];
    for (int k = 0; k < n; ++k) A[k][k] = A[k][k] + damping * A[k][k];
    bool pd = true;
    for (int k = 0; k < n && pd; ++k) {
        double s = A[k][k];
        for (int m = 0; m < k; ++m) s -= A[k][m] * A[k][m];
        if (!(s > 0.0)) { pd = false; break; }
        const double lkk = sqrt(s);
        for (int r = k + 1; r < n; ++r) {
            double q = A[k][r];
            for (int m = 0; m < k; ++m) q -= A[r][m] * A[k][m];
            A[r][k] = q / lkk;
        }
        A[k][k] = lkk;                                           // (the diagonal of the matrix is not read again)
    }
    if (!pd) return false;
    const double* g = tot + LD * (LD + 1) / 2;
    for (int k = 0; k < n; ++k) {                                // L y = -g
        double q = -g[k];
        for (int m = 0; m < k; ++m) q -= A[k][m] * xs[m];
        xs[k] = q / A[k][k];
    }
    for (int k = n - 1; k >= 0; --k) {                           // L^T x = y
        double q = xs[k];
        for (int m = k + 1; m < n; ++m) q -= A[m][k] * xs[m];
        xs[k] = q / A[k][k];
    }
    return true;
}

// Rx = Exp(w) = (I + ca W) + cb W^2 and, where V is given, the SE(3) exponential's V = (I + cb W) + cc W^2 (else null: cc is not
// computed); W the cross-product matrix of w, the coefficients by their series below |w|^2 = 1e-8.
COLVO_GN_FN void rot_exp(double w0, double w1, double w2, double (*Rx)[3], double (*V)[3]) {
    const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
    double ca, cb, cc = 0.0;
    if (th2 < 1e-8) {
        ca = 1.0 - th2 / 6.0;
        cb = 0.5 - th2 / 24.0;
        if (V) cc = 1.0 / 6.0 - th2 / 120.0;
    } else {
        const double th = sqrt(th2);
        ca = sin(th) / th;
        cb = (1.0 - cos(th)) / th2;
        if (V) cc = (th - sin(th)) / (th2 * th);
    }
    const double Wm[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double W2 = (Wm[r][0] * Wm[0][c] + Wm[r][1] * Wm[1][c]) + Wm[r][2] * Wm[2][c];
            const double id = r == c ? 1.0 : 0.0;
            Rx[r][c] = (id + ca * Wm[r][c]) + cb * W2;
            if (V) V[r][c] = (id + cb * Wm[r][c]) + cc * W2;
        }
}

#ifdef __HIPCC__
// what both loop entry points refuse; `who` is the entry point, `count_name` its name for the minimum count
inline int check_loop(const char* who, int iterations, double damping, const char* count_name, int min_count) {
    COLVO_CHECK_ARG(iterations >= 1 && iterations <= 64, "%s: bad iterations %d (1 .. 64)", who, iterations);
    COLVO_CHECK_ARG(damping >= 0.0 && damping < (double)__builtin_inff() && min_count >= 1,
                    "%s: bad damping %g (finite, >= 0) or %s %d (>= 1)", who, damping, count_name, min_count);
    return 0;
}

// One sample's row into the sums: the NC x NC upper triangle of J^T J in the layout of an LD x LD one, and the NC products with e
// behind it.  Every fma is an exact product of two float32 values and one rounded addition.
template <int NC, int LD>
__device__ __forceinline__ void add_row(const float* J, float e, double* acc) {
    double Jd[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) Jd[k] = (double)J[k];
    const double ed = (double)e;
    int idx = 0;
#pragma unroll
    for (int k = 0; k < LD; ++k) {
#pragma unroll
        for (int l = k; l < LD; ++l, ++idx) {
            if (k < NC && l < NC) acc[idx] = __builtin_fma(Jd[k], Jd[l], acc[idx]);
        }
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[LD * (LD + 1) / 2 + k] = __builtin_fma(Jd[k], ed, acc[LD * (LD + 1) / 2 + k]);
}

// The two fixed orders of a sum over the 64 lanes.  Each kernel's bits depend on its own, so both stay (§3.6i).
struct XorButterfly {                      // xor-shuffles 32, 16, .. 1: the total in every lane (refine.hip)
    __device__ __forceinline__ double operator()(double v) const {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        return v;
    }
};
struct RowRotations {                      // row rotations by DPP on the two halves of the value, then the four row totals through
    __device__ __forceinline__ double operator()(double v) const {       // scalar registers, (0 + 16) + (32 + 48) (register.hip)
        v += __longlong_as_double(row_ror<8>(__double_as_longlong(v)));
        v += __longlong_as_double(row_ror<4>(__double_as_longlong(v)));
        v += __longlong_as_double(row_ror<2>(__double_as_longlong(v)));
        v += __longlong_as_double(row_ror<1>(__double_as_longlong(v)));
        const long long b = __double_as_longlong(v);
        return (__longlong_as_double(lane_value(b, 0)) + __longlong_as_double(lane_value(b, 16))) +
               (__longlong_as_double(lane_value(b, 32)) + __longlong_as_double(lane_value(b, 48)));
    }
};

// A workgroup of four waves writes its partial row: every sum over the wave in `wave_order`, the four waves in a fixed tree, then the
// three wave-uniform counts as int64 bits.  red [4][N_SUMS] and cnt [4][3] are LDS, row [N_SUMS + 3] the workgroup's row.  No atomics.
template <int N_SUMS, typename WaveOrder>
__device__ __forceinline__ void write_partial_row(const double* acc, int c0, int c1, int c2, double (*red)[N_SUMS], int (*cnt)[3],
                                                  double* row, WaveOrder wave_order) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < N_SUMS; ++k) {
        const double v = wave_order(acc[k]);
        if (lane == 0) red[wave][k] = v;
    }
    if (lane == 0) {
        cnt[wave][0] = c0;
        cnt[wave][1] = c1;
        cnt[wave][2] = c2;
    }
    __syncthreads();
    const int m = threadIdx.x;
    if (m < N_SUMS) {
        row[m] = (red[0][m] + red[1][m]) + (red[2][m] + red[3][m]);
    } else if (m < N_SUMS + 3) {
        const int q = m - N_SUMS;
        row[m] = __longlong_as_double((long long)((cnt[0][q] + cnt[1][q]) + (cnt[2][q] + cnt[3][q])));
    }
}

// The partial rows of one system into tot [N_SUMS + 3], by a workgroup of GROUPS x 64 threads: group w sums the rows w, w + GROUPS, ...
// of entry `lane` in order, then the GROUPS partial totals are added in order; the counts as int64, converted (a count is below 2^30:
// exact).  skip: the rows are not read and every total is zero.  part [GROUPS][ROW] and tot are LDS; ends behind a barrier.
template <int N_SUMS, int ROW, int GROUPS>
__device__ __forceinline__ void sum_rows(const double* __restrict__ rows, int nrows, bool skip, double (*part)[ROW], double* tot) {
    const int grp = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane < N_SUMS + 3) {
        const double* r = rows + lane;
        if (lane < N_SUMS) {
            double v = 0.0;
            if (!skip)
                for (int c = grp; c < nrows; c += GROUPS) v += r[(size_t)c * ROW];
            part[grp][lane] = v;
        } else {
            long long v = 0;
            if (!skip)
                for (int c = grp; c < nrows; c += GROUPS) v += __double_as_longlong(r[(size_t)c * ROW]);
            part[grp][lane] = __longlong_as_double(v);
        }
    }
    __syncthreads();
    if (threadIdx.x < N_SUMS) {
        double v = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < GROUPS; ++w) v += part[w][threadIdx.x];
        tot[threadIdx.x] = v;
    } else if (threadIdx.x < N_SUMS + 3) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < GROUPS; ++w) v += __double_as_longlong(part[w][threadIdx.x]);
        tot[threadIdx.x] = (double)v;
    }
    __syncthreads();
}
#endif  // __HIPCC__

}  // namespace gn
}  // namespace colvo

#undef COLVO_GN_FN
#if !defined(__clang__)
#pragma GCC pop_options
#endif
