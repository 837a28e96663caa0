// layout.hip -- layout passes around the conv stack: NCHW fp32 planes <-> NHWC feature maps (the stems' inputs, PoseNet's
// input, gradients back to planes), ReLU backward in place, and the fp32 <-> bf16 casts of the gradient transport.
#include "elem.h"

namespace colvo {
namespace {

struct Planes {
    const float* p[4];
    int c[4];
    int n;
};

template <int ES>
__global__ __launch_bounds__(NT) void k_pack_nchw(Planes src, int HW, int Cpad, void* __restrict__ dst) {
    const int b = blockIdx.y;
    const size_t pix = (size_t)blockIdx.x * NT + threadIdx.x;
    if (pix >= (size_t)HW) return;
    int ch = 0;
    const size_t o = ((size_t)b * HW + pix) * Cpad;
    for (int s = 0; s < src.n; ++s)
        for (int c = 0; c < src.c[s]; ++c, ++ch)
            Elem<ES>::st(dst, o + ch, src.p[s][((size_t)b * src.c[s] + c) * HW + pix]);
    for (; ch < Cpad; ++ch) Elem<ES>::st(dst, o + ch, 0.0f);
}

// The stems (Cpad = 8): the pixel's 8 channels are gathered in registers and leave as ONE 16-byte (bf16) / two 16-byte (f32)
// stores; the element-wise version above issued eight 2-byte stores per pixel (15.6 us for DepthNet's 16 frames, 2.4 TB/s).
template <int ES>
__global__ __launch_bounds__(NT) void k_pack_nchw8(Planes src, int HW, void* __restrict__ dst) {
    typedef __attribute__((ext_vector_type(4))) unsigned int u4;
    const int b = blockIdx.y;
    const size_t pix = (size_t)blockIdx.x * NT + threadIdx.x;
    if (pix >= (size_t)HW) return;
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = 0.0f;
    int ch = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (s >= src.n) break;
        const int cs = src.c[s];
        const float* base = src.p[s] + (size_t)b * cs * HW + pix;
#pragma unroll
        for (int c = 0; c < 4; ++c) {            // a stem source has at most 3 (image) or 1 (depth) channels
            if (c < cs) {
                const float x = base[(size_t)c * HW];
#pragma unroll
                for (int k = 0; k < 8; ++k) if (k == ch + c) v[k] = x;
            }
        }
        ch += cs;
    }
    const size_t o = ((size_t)b * HW + pix) * 8;
    if constexpr (ES == 2) {
        u4 w;
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = pack2bf(v[2 * k], v[2 * k + 1]);
        *reinterpret_cast<u4*>(reinterpret_cast<uint16_t*>(dst) + o) = w;
    } else {
        u4 w0, w1;
#pragma unroll
        for (int k = 0; k < 4; ++k) { w0[k] = __float_as_uint(v[k]); w1[k] = __float_as_uint(v[4 + k]); }
        u4* d = reinterpret_cast<u4*>(reinterpret_cast<float*>(dst) + o);
        d[0] = w0; d[1] = w1;
    }
}

// DepthNet's stem pack for the DCDP pair batch [target frames | reference frames] (bf16), which ALSO writes the six rgb channels of
// PoseNet's 8-channel input [tgt rgb | ref rgb | depth_t | depth_r]: image i fills channels 0..2 (i < Bh) or 3..5 of pair i mod Bh.
// The two depth channels are written by the depth head's kernel (csrc/fwd16.hip): PoseNet's own packing pass -- a read of the same
// frames plus both depth maps, 13 us at 8 pairs on the forward chain -- disappears.
// A thread takes one pixel of one PAIR (six plane reads in flight), so PoseNet's pixel is one full 16-byte store: its depth channels are
// zero until the head's kernel -- later in the same pass -- writes them.
__global__ __launch_bounds__(NT) void k_pack_stem_pose(const float* __restrict__ frames, int HW, int Bh, void* __restrict__ stem,
                                                        void* __restrict__ pose_in) {
    typedef __attribute__((ext_vector_type(4))) unsigned int u4;
    const int p = blockIdx.y;
    const size_t pix = (size_t)blockIdx.x * NT + threadIdx.x;
    if (pix >= (size_t)HW) return;
    const float* t = frames + (size_t)p * 3 * HW + pix;
    const float* r = frames + (size_t)(p + Bh) * 3 * HW + pix;
    const float t0 = t[0], t1 = t[(size_t)HW], t2 = t[2 * (size_t)HW], r0 = r[0], r1 = r[(size_t)HW], r2 = r[2 * (size_t)HW];
    const unsigned a0 = f2bf(t0), a1 = f2bf(t1), a2 = f2bf(t2), b0 = f2bf(r0), b1 = f2bf(r1), b2 = f2bf(r2);
    u4 w;
    w[0] = a0 | (a1 << 16); w[1] = a2; w[2] = 0u; w[3] = 0u;
    *reinterpret_cast<u4*>(reinterpret_cast<uint16_t*>(stem) + ((size_t)p * HW + pix) * 8) = w;
    w[0] = b0 | (b1 << 16); w[1] = b2;
    *reinterpret_cast<u4*>(reinterpret_cast<uint16_t*>(stem) + ((size_t)(p + Bh) * HW + pix) * 8) = w;
    w[0] = a0 | (a1 << 16); w[1] = a2 | (b0 << 16); w[2] = b1 | (b2 << 16); w[3] = 0u;
    *reinterpret_cast<u4*>(reinterpret_cast<uint16_t*>(pose_in) + ((size_t)p * HW + pix) * 8) = w;
}

// PX pixels per thread: the reads are 2 / 4 useful bytes per 16 / 32-byte pixel, so a thread needs several in flight
template <int ES, int PX = 4>
__global__ __launch_bounds__(NT) void k_unpack_nhwc(const void* __restrict__ src, int HW, int Cpad, int c_begin,
                                                    int c_count, float* __restrict__ dst, int flags) {
    const int b = blockIdx.y;
    const bool accumulate = flags & 1, by_channel = flags & 2;      // by_channel: dst is [c_count][B][H][W]
    const size_t pix0 = (size_t)blockIdx.x * NT * PX + threadIdx.x;
    for (int c = 0; c < c_count; ++c) {
        float v[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const size_t pix = pix0 + (size_t)j * NT;
            v[j] = (pix < (size_t)HW) ? Elem<ES>::ld(src, ((size_t)b * HW + pix) * Cpad + c_begin + c) : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const size_t pix = pix0 + (size_t)j * NT;
            if (pix >= (size_t)HW) continue;
            float* d = dst + (by_channel ? (size_t)c * gridDim.y + b : (size_t)b * c_count + c) * HW + pix;
            *d = accumulate ? (*d + v[j]) : v[j];
        }
    }
}

template <int ES>
__global__ __launch_bounds__(NT) void k_relu_bwd(const void* __restrict__ y, void* __restrict__ dy, size_t n) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    if (!(Elem<ES>::ld(y, i) > 0.0f)) Elem<ES>::st(dy, i, 0.0f);
}

// ---- gradient transport in bf16 (ddp.GradBuckets(transport_dtype=bfloat16)): fp32 slice <-> bf16 staging slice ----
// (round 4 staged through Tensor.copy_, i.e. at::native kernels inside the data-parallel step; same RNE rounding here)
__global__ __launch_bounds__(NT) void k_cast_f32_bf16(const float* __restrict__ src, uint16_t* __restrict__ dst, size_t n) {
    const size_t stride = (size_t)gridDim.x * NT * 4;
    for (size_t i = ((size_t)blockIdx.x * NT + threadIdx.x) * 4; i < n; i += stride) {
        if (i + 4 <= n) {
            const float4 v = *reinterpret_cast<const float4*>(src + i);
            uint2 o;
            o.x = pack2bf(v.x, v.y);
            o.y = pack2bf(v.z, v.w);
            *reinterpret_cast<uint2*>(dst + i) = o;
        } else {
            for (size_t j = i; j < n; ++j) dst[j] = f2bf(src[j]);
        }
    }
}
__global__ __launch_bounds__(NT) void k_cast_bf16_f32(const uint16_t* __restrict__ src, float* __restrict__ dst, size_t n) {
    const size_t stride = (size_t)gridDim.x * NT * 4;
    for (size_t i = ((size_t)blockIdx.x * NT + threadIdx.x) * 4; i < n; i += stride) {
        if (i + 4 <= n) {
            const uint2 v = *reinterpret_cast<const uint2*>(src + i);
            *reinterpret_cast<float4*>(dst + i) = make_float4(bf2f((uint16_t)(v.x & 0xFFFFu)), bf2f((uint16_t)(v.x >> 16)),
                                                              bf2f((uint16_t)(v.y & 0xFFFFu)), bf2f((uint16_t)(v.y >> 16)));
        } else {
            for (size_t j = i; j < n; ++j) dst[j] = bf2f(src[j]);
        }
    }
}

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" int colvo_pack_nchw(int dtype, const float* const* src, const int32_t* src_channels, int nsrc, int B, int H,
                               int W, int Cpad, void* dst, colvo_stream_t stream) {
    COLVO_CHECK_ARG(src && src_channels && dst && nsrc >= 1 && nsrc <= 4, "colvo_pack_nchw: bad arguments");
    COLVO_CHECK_DTYPE(dtype, "colvo_pack_nchw");
    Planes pl{};
    int tot = 0;
    for (int i = 0; i < nsrc; ++i) {
        COLVO_CHECK_ARG(src[i] && src_channels[i] > 0, "colvo_pack_nchw: null source %d", i);
        pl.p[i] = src[i]; pl.c[i] = src_channels[i]; tot += src_channels[i];
    }
    pl.n = nsrc;
    COLVO_CHECK_ARG(tot <= Cpad && Cpad % 8 == 0 && B >= 1 && B <= 65535, "colvo_pack_nchw: bad channel padding %d for %d", Cpad, tot);
    const size_t HW = (size_t)H * W;
    bool narrow = Cpad == 8;
    for (int i = 0; i < nsrc; ++i) narrow = narrow && src_channels[i] <= 4;
    if (narrow)
        DISPATCH_ES(dtype, colvo::launch((k_pack_nchw8<ES>), dim3(nblk(HW), B), dim3(NT), 0, (hipStream_t)stream, pl, (int)HW, dst));
    else
        DISPATCH_ES(dtype, colvo::launch((k_pack_nchw<ES>), dim3(nblk(HW), B), dim3(NT), 0, (hipStream_t)stream, pl, (int)HW, Cpad, dst));
    COLVO_CHECK_LAUNCH("k_pack_nchw");
    return 0;
}

extern "C" int colvo_pack_stem_pose(const float* frames, int B2, int H, int W, void* stem, void* pose_in, colvo_stream_t stream) {
    COLVO_CHECK_ARG(frames && stem && pose_in && B2 >= 2 && B2 % 2 == 0 && B2 <= 65534 && H >= 1 && W >= 1,
                    "colvo_pack_stem_pose: bad arguments (B2 = 2 * pairs images)");
    const size_t HW = (size_t)H * W;
    colvo::launch(k_pack_stem_pose, dim3(nblk(HW), B2 / 2), dim3(NT), 0, (hipStream_t)stream, frames, (int)HW, B2 / 2, stem, pose_in);
    COLVO_CHECK_LAUNCH("k_pack_stem_pose");
    return 0;
}

extern "C" int colvo_unpack_nhwc_grad(int dtype, const void* dsrc, int B, int H, int W, int Cpad, int c_begin,
                                      int c_count, float* dst_nchw, int accumulate, colvo_stream_t stream) {
    COLVO_CHECK_ARG(dsrc && dst_nchw && c_begin >= 0 && c_count >= 1 && c_begin + c_count <= Cpad && B >= 1 && B <= 65535,
                    "colvo_unpack_nhwc_grad: bad arguments");
    const size_t HW = (size_t)H * W;
    COLVO_DISPATCH_ES(dtype, "colvo_unpack_nhwc_grad",
                      colvo::launch((k_unpack_nhwc<ES, 4>), dim3(nblk((HW + 3) / 4), B), dim3(NT), 0, (hipStream_t)stream, dsrc,
                                    (int)HW, Cpad, c_begin, c_count, dst_nchw, accumulate));
    COLVO_CHECK_LAUNCH("k_unpack_nhwc");
    return 0;
}

extern "C" int colvo_relu_bwd_inplace(int dtype, const void* y, void* dy, size_t n, colvo_stream_t stream) {
    COLVO_CHECK_ARG(y && dy, "colvo_relu_bwd_inplace: null pointer argument");
    COLVO_CHECK_DTYPE(dtype, "colvo_relu_bwd_inplace");
    if (n == 0) return 0;
    DISPATCH_ES(dtype, colvo::launch((k_relu_bwd<ES>), dim3(nblk(n)), dim3(NT), 0, (hipStream_t)stream, y, dy, n));
    COLVO_CHECK_LAUNCH("k_relu_bwd");
    return 0;
}

extern "C" int colvo_cast_f32_bf16(const float* src, void* dst, size_t n, int to_bf16, colvo_stream_t stream) {
    COLVO_CHECK_ARG(src && dst, "colvo_cast_f32_bf16: null pointer argument");
    // (to_bf16 = 0: `src` is the bf16 buffer and `dst` the fp32 one -- the argument order stays source, destination)
    COLVO_CHECK_ARG((uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0, "colvo_cast_f32_bf16: buffers must be 16-byte aligned");
    if (n == 0) return 0;
    unsigned blocks = nblk((n + 3) / 4);
    if (blocks > 2048) blocks = 2048;
    if (to_bf16) colvo::launch(k_cast_f32_bf16, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, src, (uint16_t*)dst, n);
    else colvo::launch(k_cast_bf16_f32, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, (const uint16_t*)src, (float*)dst, n);
    COLVO_CHECK_LAUNCH("k_cast_f32_bf16");
    return 0;
}
