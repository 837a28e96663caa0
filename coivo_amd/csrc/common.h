// common.h -- shared host/device helpers for libcolvo (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <mutex>
#include <utility>

#include "../../include/colvo.h"

namespace colvo {

void set_error(const char* fmt, ...);

#define COLVO_CHECK_ARG(cond, ...)                   \
    do {                                             \
        if (!(cond)) {                               \
            ::colvo::set_error(__VA_ARGS__);         \
            return (int)hipErrorInvalidValue;        \
        }                                            \
    } while (0)

#define COLVO_CHECK_LAUNCH(name)                                                    \
    do {                                                                            \
        hipError_t e_ = hipGetLastError();                                          \
        if (e_ != hipSuccess) {                                                     \
            ::colvo::set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); \
            return (int)e_;                                                         \
        }                                                                           \
    } while (0)

#define COLVO_CHECK_HIP(call, name)                                                       \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            ::colvo::set_error("%s: %s failed: %s", name, #call, hipGetErrorString(e_)); \
            return (int)e_;                                                               \
        }                                                                                 \
    } while (0)

// Every kernel launch of the library goes through launch(): a launch can then CARRY an event.  hipEventRecord puts a marker packet
// behind the kernel on its queue, and the next kernel of that queue waits for it: 2.8 us per record on the producing chain, 5.3 us
// when another queue already waits on the event -- the backward pass forks a weight-gradient kernel off every layer of its
// input-gradient chain (tools/ubench/fork_cost.hip: chain of 40 kernels of 18 us: 18.0 us per kernel alone, 20.8 with a record after
// each, 23.3 with record + waiter; 19.4 with the event as hipExtLaunchKernel's stopEvent, which rides on the kernel's own completion
// signal: no packet on the producer's queue).  colvo_run_commands arms the tap around a command that a FORK follows.
struct LaunchTap {
    hipEvent_t stop = nullptr;     // event to attach to launches on `stream` (nullptr: plain launches)
    hipStream_t stream = nullptr;
    int used = 0;                  // launches that carried it
};
extern thread_local LaunchTap g_launch_tap;      // program.hip (commands run on the thread that armed it)

template <typename... P, typename... A>
inline void launch(void (*kernel)(P...), dim3 grid, dim3 block, unsigned lds, hipStream_t s, A&&... a) {
    LaunchTap& t = g_launch_tap;
    if (t.stop != nullptr && t.stream == s) {
        ++t.used;
        hipExtLaunchKernelGGL(kernel, grid, block, lds, s, nullptr, t.stop, 0u, static_cast<P>(a)...);
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, s, static_cast<P>(a)...);
    }
}

// Dynamic-LDS opt-in: a launch of `Kernel` asks for `lds` bytes; above the default 48 KB the kernel must first be allowed `limit`
// bytes (its MaxDynamicSharedMemorySize attribute), once per kernel and process.  Safe under concurrent callers; once the
// attribute is set, a call is one atomic load.
template <auto Kernel>
inline int allow_dynamic_lds(size_t lds, int limit, const char* who) {
    static std::atomic<bool> done{false};
    if (lds <= 48 * 1024 || done.load(std::memory_order_acquire)) return 0;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (done.load(std::memory_order_relaxed)) return 0;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, limit);
    if (e != hipSuccess) { set_error("%s: dynamic LDS opt-in failed: %s", who, hipGetErrorString(e)); return (int)e; }
    done.store(true, std::memory_order_release);
    return 0;
}

// The launch of a resident kernel (one workgroup per CU, up to the whole 160 KB of LDS): opt-in, launch, check.  who: the caller's
// name for the opt-in's error; name: the kernel's for the launch's.
template <auto Kernel, typename... A>
inline int launch_resident(unsigned grid, int nt, int lds, hipStream_t s, const char* who, const char* name, A&&... args) {
    if (int e = allow_dynamic_lds<Kernel>((size_t)lds, 160 * 1024, who)) return e;
    colvo::launch(Kernel, dim3(grid), dim3((unsigned)nt), (unsigned)lds, s, std::forward<A>(args)...);
    COLVO_CHECK_LAUNCH(name);
    return 0;
}

// Host-side sizes and layouts.
inline size_t pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int blocks_of(long long n, int nt) { return (int)((n + nt - 1) / nt); }    // ceil(n / nt)

// A workspace laid out as consecutive arrays: take<T>(count) hands out the next `count` elements and advances by their size rounded up
// to `pad` bytes.  On a null base it only measures (every pointer it returns is null): bytes() is what the same takes need, so a
// layout is written once and serves both the size query and the call.
class Carver {
public:
    explicit Carver(void* base) : base_(static_cast<char*>(base)) {}
    template <typename T>
    T* take(size_t count, size_t pad = 16) {
        T* p = base_ ? reinterpret_cast<T*>(base_ + used_) : nullptr;
        used_ += (count * sizeof(T) + pad - 1) / pad * pad;
        return p;
    }
    size_t bytes() const { return used_; }

private:
    char* base_;
    size_t used_ = 0;
};

// Which kernel FORM a dispatcher chose, counted per process (colvo_form_counts: the tests of the grid-size-selected forms read it --
// a parity test at a small shape must be able to say that the large-grid kernel is what actually ran).  Every leaf of
// the forward / input-gradient / weight-gradient dispatch trees and every fused kernel has a counter; the grid and store attributes of
// the weight gradient (full / halved grid, clean-arena store, 64-wide co tile) and the 64-wide one-tile channel tile count beside their
// leaf.  Names: api.hip (same order).
enum { FORM_CONV_RT = 0, FORM_WGRAD_FULL_GRID, FORM_WGRAD_HALVED_GRID, FORM_WGRAD_UP2, FORM_WGRAD_RT, FORM_WGRAD_STORE_CLEAN, FORM_CONV_RES_S2,
       FORM_CONV_Q,
       FORM_CONV_UP2_BN16, FORM_CONV_UP2_BN32,    // k_conv_up2, 16- / 32-wide channel tiles
       FORM_DGRAD_S2, FORM_DGRAD_S2_RING,         // k_dgrad_s2, one chunk / two chunks in flight
       FORM_DGRAD_UP2,                            // k_dgrad_up2
       FORM_DGRAD_BOTH,                           // colvo_conv_dgrad_both's merged launch (beside the leaf it took: conv_rt or a one-tile form)
       FORM_CONV_TILE, FORM_CONV_RING,            // k_conv3x3 one-tile kernel (256 threads), its two-chunk register ring
       FORM_CONV_WIDE,                            // ... its 512-thread / 256-pixel form (tuning `wide`, off by default)
       FORM_CONV_RES,                             // k_conv3x3_res, stride 1
       FORM_CONV_BN64,                            // a one-tile (256- or 512-thread) or weights-resident launch with 64-wide channel tiles
       FORM_WGRAD_TEAMS, FORM_WGRAD_TAIL,         // k_wgrad3x3 with four pixel-tile teams / one team
       FORM_WGRAD_MT4,                            // ... one team, 64-wide co tile
       FORM_WGRAD_SLICED,                         // a weight-gradient call processed in image slices (tensors >= 1 GiB)
       FORM_BWD16, FORM_FWD16_HEAD, FORM_DGRAD_PLANES_MFMA,
       FORM_CONV_RT_BN32,                         // k_conv_rt's 32-channel form (beside conv_rt)
       FORM_COUNT };
static_assert(FORM_COUNT <= 32, "coivo_amd/_lib.py form_counts reads 32 counters");
void form_hit(int id);
constexpr uint32_t form_bit(int id) { return 1u << id; }
inline void form_hits(uint32_t mask) {          // every FORM_f whose form_bit is in mask
    for (; mask; mask &= mask - 1) form_hit(__builtin_ctz(mask));
}

// csrc/bwd16.hip: the MFMA form of colvo_conv_dgrad_planes (bf16, stride 2, 16 output channels, two input channels, even extents)
int launch_dgrad_planes_s2_mfma(const void* g, const float* w, int Cin, int c_begin, int B, int Hi, int Wi, int Ho, int Wo, float* dst,
                                int accumulate, hipStream_t stream);

// csrc/pose_front.hip: COLVO_CMD_CONV_FWD with a chain length in i[0] -- PoseNet's conv1-conv3 in one launch -- and
// COLVO_CMD_CONV_DGRAD_PLANES with g3 in p[3] -- their input-gradient chain down to the two depth planes in one launch
int pose_front_fwd(const ColvoCmd& c, hipStream_t stream);
int pose_front_bwd(const ColvoCmd& c, hipStream_t stream);

// csrc/pose_tail.hip: COLVO_CMD_CONV_FWD with i[0] = -1 and COLVO_CMD_CONV_DGRAD with i[2] = 1 -- one of PoseNet's conv5-conv7 as a
// whole-K resident launch (colvo_pose_tail_plan)
int pose_tail_fwd(const ColvoCmd& c, hipStream_t stream);
int pose_tail_dgrad(const ColvoCmd& c, hipStream_t stream);

// csrc/stem.hip: COLVO_CMD_PACK_STEM_POSE with enc1a's weights in p[3] -- the packing pass, enc1a and enc1b of DepthNet's stem in one
// launch (colvo_stem_plan)
int stem_fused(const ColvoCmd& c, hipStream_t stream);

__device__ __forceinline__ float uniform_f(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// Sum over the 64 lanes, result in every lane.  Row rotations by DPP (row_ror: VALU only, no LDS crossbar
// round trip as with ds_bpermute-based shuffles), then the four 16-lane row totals through scalar registers.
__device__ __forceinline__ float wave_sum(float v) {
#define COLVO_ROR(x, n) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x120 + (n), 0xf, 0xf, false))
    v += COLVO_ROR(v, 8);
    v += COLVO_ROR(v, 4);
    v += COLVO_ROR(v, 2);
    v += COLVO_ROR(v, 1);
#undef COLVO_ROR
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (r0 + r1) + (r2 + r3);
}

// The same for integers.  The rotations act on the two halves of a 64-bit value (VALU only; six xor-shuffles of a 64-bit value are
// twelve trips through the LDS crossbar, and csrc/localize.hip needs eleven such sums per group of lanes).  Called by the whole wave,
// result uniform.
template <int N>
__device__ __forceinline__ int row_ror(int x) {
    return __builtin_amdgcn_update_dpp(0, x, 0x120 + N, 0xf, 0xf, false);
}
template <int N>
__device__ __forceinline__ long long row_ror(long long x) {
    const unsigned lo = (unsigned)row_ror<N>((int)(unsigned)x), hi = (unsigned)row_ror<N>((int)(unsigned)((unsigned long long)x >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ int lane_value(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ long long lane_value(long long v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), lane);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ long long wave_sum(long long v) {
    v += row_ror<8>(v);
    v += row_ror<4>(v);
    v += row_ror<2>(v);
    v += row_ror<1>(v);
    return (lane_value(v, 0) + lane_value(v, 16)) + (lane_value(v, 32) + lane_value(v, 48));
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) { return (unsigned long long)wave_sum((long long)v); }
// (no caller yet: block_sum below keeps its xor-shuffles, so that the kernels using it keep the instructions they had)
__device__ __forceinline__ int wave_sum(int v) {
    v += row_ror<8>(v);
    v += row_ror<4>(v);
    v += row_ror<2>(v);
    v += row_ror<1>(v);
    return (lane_value(v, 0) + lane_value(v, 16)) + (lane_value(v, 32) + lane_value(v, 48));
}
__device__ __forceinline__ int wave_max(int v) {
    v = max(v, row_ror<8>(v));
    v = max(v, row_ror<4>(v));
    v = max(v, row_ror<2>(v));
    v = max(v, row_ror<1>(v));
    return max(max(lane_value(v, 0), lane_value(v, 16)), max(lane_value(v, 32), lane_value(v, 48)));
}

// Sum over a workgroup of 256 threads, in every thread; sm: four ints of LDS (one call per array between barriers).
__device__ __forceinline__ int block_sum(int v, int* sm) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// Order-preserving map of every float bit pattern to uint32 (negatives flipped whole, positives get the sign bit), and back: total, so
// any input -- NaN included -- has a key, and a selection or a maximum over keys always terminates.
__device__ __forceinline__ uint32_t float_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float float_key_inv(uint32_t k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

// bf16 <-> f32 on raw 16-bit storage
__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
__device__ __forceinline__ uint16_t f2bf(float f) {
    __hip_bfloat16 b = __float2bfloat16(f);   // RNE, NaN-preserving (v_cvt_pk_bf16_f32 at -O3)
    return *reinterpret_cast<uint16_t*>(&b);
}

// two floats -> two bf16 in one register (element 0 in the low half): ONE v_cvt_pk_bf16_f32, where two f2bf() and the shift / or that
// joins them cost four instructions -- same instruction, same rounding
__device__ __forceinline__ uint32_t pack2bf(float lo, float hi) {
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_{lo, hi}, bf16x2_));
}

}  // namespace colvo
