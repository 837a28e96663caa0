// mesh_common.h -- what the kernels over an indexed triangle mesh share (topology.hip, fill.hip): which face
// is live, the quanta of the measures, and the wave-grouped integer adds into per-record tables.  Every file that includes it pins its
// own float64 association (contraction off for the whole file).
#pragma once
#include "scene.h"

namespace colvo {

__device__ __forceinline__ bool live_face(const int32_t* __restrict__ faces, int f, int V, int (&v)[3]) {
    v[0] = faces[(size_t)f * 3];
    v[1] = faces[(size_t)f * 3 + 1];
    v[2] = faces[(size_t)f * 3 + 2];
    const bool in = (unsigned)v[0] < (unsigned)V && (unsigned)v[1] < (unsigned)V && (unsigned)v[2] < (unsigned)V;
    return in && v[0] != v[1] && v[1] != v[2] && v[0] != v[2];
}

// ---- sums into the records ---------------------------------------------------------------------------------------------------- //
// Called by the whole wave (no lane has left): lanes with row >= 0 add v[0..K) to table[row * stride + col[k]].  Up to GROUP_ROUNDS
// times, the lanes that share the first remaining lane's row are summed over the wave and added once -- on the project's meshes a
// wave's faces and edges belong to one or two components, and nearly all of them to the same few records --; what remains after
// that adds for itself.
constexpr int GROUP_ROUNDS = 4;

template <int K>
__device__ __forceinline__ void record_add(long long* __restrict__ table, int stride, int row, const int (&col)[K], const long long (&v)[K]) {
    unsigned long long todo = __ballot(row >= 0);                // wave-uniform, as is the loop
#pragma unroll 1
    for (int round = 0; round < GROUP_ROUNDS && todo != 0ull; ++round) {
        const int first = __shfl(row, __builtin_ctzll(todo));
        const bool grouped = row == first;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const long long s = wave_sum(grouped ? v[k] : 0ll);
            if ((threadIdx.x & 63) == 0 && s != 0) atomicAdd((unsigned long long*)(table + (size_t)first * stride + col[k]), (unsigned long long)s);
        }
        todo &= ~__ballot(grouped);
    }
    if ((todo >> (threadIdx.x & 63)) & 1ull) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (v[k] != 0) atomicAdd((unsigned long long*)(table + (size_t)row * stride + col[k]), (unsigned long long)v[k]);
    }
}

struct Quanta {
    double area, length;                   // unit^2 * 2^-16, unit * 2^-16
};

__device__ __forceinline__ Quanta quanta_of(float unit) {
    const double u = (double)unit;
    return Quanta{(u * u) * 0x1p-16, u * 0x1p-16};
}

// llrint(m / quantum) and true, or 0 and false where the quotient is NaN or 2^62 and more
__device__ __forceinline__ bool to_quanta(double m, double quantum, long long& q) {
    const double t = m / quantum;
    const bool ok = t < 0x1p62;                                  // (m >= 0; NaN fails)
    q = ok ? llrint(t) : 0ll;
    return ok;
}

__device__ __forceinline__ void load_point(const float* __restrict__ vertices, int v, double (&p)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = (double)vertices[(size_t)v * 3 + a];
}

inline bool unit_ok(float unit) { return unit > 0.0f && unit < __builtin_inff(); }

}  // namespace colvo
