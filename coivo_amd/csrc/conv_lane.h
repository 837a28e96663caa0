// conv_lane.h -- the lane-level vocabulary of the bf16 conv kernels: what a lane does with its accumulator quad after
// mfma_result_guard, and which tap a slot of the flipped stride-2 slab holds.  conv.hip and conv_rt.hip mask with it; the resident
// kernels (pose_front.hip, pose_tail.hip), which promise the bits of a plain launch, build their close and their tap order from it
// (DESIGN.md section 3.3).  Everything here is inlined: profiles/conv_lane_ab.md records, kernel by kernel, that the emitted code
// is what it was with the arithmetic written out at each site, and names the sites that stay written out because it would not be.
#pragma once
#include "conv_common.h"

namespace colvo {
namespace {

// The producer's ReLU mask, two packed bf16 words = four channels: v[0..3] survive where the producer's value is > 0.
// bf16 > 0  <=>  sign clear and magnitude non-zero (+0, -0 and everything with the sign set mask; a NaN with the sign clear keeps)
__device__ __forceinline__ void relu_mask_keep(uint32_t m0, uint32_t m1, float* v) {
    const uint32_t m[2] = {m0, m1};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint32_t lo = m[k] & 0xFFFFu, hi = m[k] >> 16;
        if (!(lo != 0 && lo < 0x8000u)) v[2 * k] = 0.0f;
        if (!(hi != 0 && hi < 0x8000u)) v[2 * k + 1] = 0.0f;
    }
}

// A lane's close, in two halves around the mask and the accumulate add (Epi::finish, conv.hip; k_conv_rt).  First half, either
// element type: + bias (its bits, as the epilogues hold it; zeros for none, so that -0 becomes +0), then ReLU.
__device__ __forceinline__ void lane_bias_relu(const f32x4& acc, const u32x4& bias, int relu, float* v) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = acc[r] + __uint_as_float(bias[r]);
    if (relu) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.0f);
    }
}
// Second half, bf16: one v_cvt_pk_bf16_f32 per channel pair
__device__ __forceinline__ u32x2 lane_pack_bf16(const float* v) { return u32x2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])}; }

// The whole close of a bf16 launch that does not accumulate: bias, ReLU, the producer's mask (if masked), pack
__device__ __forceinline__ u32x2 lane_close_bf16(const f32x4& acc, const u32x4& bias, int relu, bool masked, const u32x2& pm) {
    float v[4];
    lane_bias_relu(acc, bias, relu, v);
    if (masked) relu_mask_keep(pm[0], pm[1], v);
    return lane_pack_bf16(v);
}

// The input gradient of a stride-2 conv, parity-decomposed (k_dgrad_s2, conv.hip): the weight operand is the flipped layout
// w_bwd [Cin][8 - tap][Cout], so slot m of a slab row holds tap t = 8 - m = (ky, kx).  With 32-channel chunks a k-group is a tap, and
// the slots run in ascending m.  Tap (ky, kx) feeds the parity class cls = 2 (iy & 1) + (ix & 1) of the input gradient -- an even
// row sees only ky = 1, an odd one ky = 0 and ky = 2 -- and reads dy at (+dy rows, +dx columns) from the lane's position: +1 row
// if ky == 0, +1 column if kx == 0.  The sum order of every kernel that forms these sums is this table.
struct S2Tap { int cls, dy, dx; };
constexpr S2Tap s2_tap(int m) {
    const int t = 8 - m, ky = t / 3, kx = t - 3 * ky;
    return S2Tap{(ky != 1 ? 2 : 0) | (kx != 1 ? 1 : 0), ky == 0 ? 1 : 0, kx == 0 ? 1 : 0};
}

}  // namespace
}  // namespace colvo
