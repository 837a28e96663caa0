// elem.h -- what the memory-bound helper files (heads.hip, adam.hip, layout.hip, dgrad_planes.hip) share: the element type
// of a feature map as a template parameter, its 16-byte granule as floats, the dtype check and dispatch of an entry point,
// and the one-thread-per-element grid.  Included by those four files only: a helper that moves into common.h reaches
// every kernel of the library (profiles/scene_shared_ab.md).
#pragma once
#include "common.h"

namespace colvo {
namespace {

constexpr int NT = 256;

template <int ES> struct Elem;
template <> struct Elem<4> {
    static __device__ __forceinline__ float ld(const void* p, size_t i) { return reinterpret_cast<const float*>(p)[i]; }
    static __device__ __forceinline__ void st(void* p, size_t i, float v) { reinterpret_cast<float*>(p)[i] = v; }
};
template <> struct Elem<2> {
    static __device__ __forceinline__ float ld(const void* p, size_t i) { return bf2f(reinterpret_cast<const uint16_t*>(p)[i]); }
    static __device__ __forceinline__ void st(void* p, size_t i, float v) { reinterpret_cast<uint16_t*>(p)[i] = f2bf(v); }
};

// f(k, x) for element k = 0 .. 16 / ES - 1 of one 16-byte granule, in element order: x is the element as a float.  (A visitor, so
// that a caller's multiply-add follows each element's decode as it did when written out: the forward head kernels keep their listings.)
template <int ES, class F>
__device__ __forceinline__ void granule_each(const uint4 q, F f) {
    const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if constexpr (ES == 2) {
            f(2 * k, __uint_as_float(u[k] << 16));
            f(2 * k + 1, __uint_as_float(u[k] & 0xFFFF0000u));
        } else {
            f(k, __uint_as_float(u[k]));
        }
    }
}
template <int ES>
__device__ __forceinline__ void granule_floats(const uint4 q, float* v) {
    granule_each<ES>(q, [&](int k, float x) { v[k] = x; });
}

// eight consecutive elements at p (16-byte aligned; global memory or LDS) as floats: one granule (bf16) or two (f32)
template <int ES>
__device__ __forceinline__ void load8(const void* p, float (&v)[8]) {
#pragma unroll
    for (int q = 0; q < ES / 2; ++q) granule_floats<ES>(reinterpret_cast<const uint4*>(p)[q], v + q * (16 / ES));
}

inline unsigned nblk(size_t n) { return (unsigned)((n + NT - 1) / NT); }

}  // namespace
}  // namespace colvo

// ES = 4 / 2 for a dtype that has been checked; the check; and both as the opening of entry point `who`.  (Where another
// argument check of the entry point stands between the two, they stay apart: a call that is wrong twice keeps its message.)
#define DISPATCH_ES(dtype, ...)                                          \
    do {                                                                 \
        if ((dtype) == COLVO_F32) { constexpr int ES = 4; __VA_ARGS__; } \
        else { constexpr int ES = 2; __VA_ARGS__; }                      \
    } while (0)
#define COLVO_CHECK_DTYPE(dtype, who) COLVO_CHECK_ARG((dtype) == COLVO_F32 || (dtype) == COLVO_BF16, who ": bad dtype")
#define COLVO_DISPATCH_ES(dtype, who, ...)  \
    do {                                    \
        COLVO_CHECK_DTYPE(dtype, who);      \
        DISPATCH_ES(dtype, __VA_ARGS__);    \
    } while (0)
