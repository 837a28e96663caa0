// dgrad_planes.hip -- input gradient of a 3x3 conv w.r.t. a FEW input channels, as fp32 planes (colvo_conv_dgrad_planes).
// PoseNet's first layer takes [tgt rgb | ref rgb | depth_t | depth_r]; of its input gradient only the two depth channels are wanted,
// as fp32 NCHW planes for DepthNet's backward pass.  The general path computed all 8 channels of the 256x320 gradient with the MFMA
// kernel (24 us at 8 pairs: it is a write of 10.5 MB NHWC for 0.4 GFLOP) and then unpacked two of them (+5 us), on the critical path
// between the two networks' backward passes.  Here: dx[c] = sum over the output pixels that see the input pixel and over Cout of
// w[co][tap][c] dy[co], weights of the wanted channels in LDS as [tap][co][c], dy rows through L2, planes written coalesced.
// Stride 2: a thread takes a PAIR of horizontally adjacent input pixels (2m, 2m + 1) -- the even one sees the middle tap column of
// output column m, the odd one the right column of m and the left column of m + 1 -- so every lane of a wave runs the same taps (with a
// thread per pixel the lanes alternated between the two parity classes: every tap body ran under half an EXEC mask, 21 us in the step).
#include "elem.h"
#include "tuning.h"

namespace colvo {
namespace {

template <int ES, int NC>
__global__ __launch_bounds__(NT) void k_conv_dgrad_planes(const void* __restrict__ dy, const float* __restrict__ w, int Cout, int Cin,
                                                          int c_begin, int B, int Hi, int Wi, int Ho, int Wo, int S,
                                                          float* __restrict__ dst, int accumulate) {
    extern __shared__ float sw[];                       // [9][Cout][NC]
    for (int i = threadIdx.x; i < 9 * Cout * NC; i += NT) {
        const int c = i % NC, co = (i / NC) % Cout, tap = i / (NC * Cout);
        sw[i] = w[((size_t)co * 9 + tap) * Cin + c_begin + c];
    }
    __syncthreads();
    const size_t HW = (size_t)Hi * Wi;
    if (S == 2) {
        const int Wp = (Wi + 1) >> 1;                   // pixel pairs per row
        const size_t p = (size_t)blockIdx.x * NT + threadIdx.x;
        if (p >= (size_t)B * Hi * Wp) return;
        const int b = (int)(p / ((size_t)Hi * Wp));
        const int r = (int)(p - (size_t)b * Hi * Wp);
        const int iy = r / Wp, m = r - iy * Wp;
        float a0[NC], a1[NC];                           // pixel 2m, pixel 2m + 1
#pragma unroll
        for (int c = 0; c < NC; ++c) { a0[c] = 0.0f; a1[c] = 0.0f; }
        const char* dyb = (const char*)dy + (size_t)b * Ho * Wo * Cout * ES;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int ty = iy + 1 - ky;                 // 2 oy
            if (ty < 0 || (ty & 1)) continue;           // (wave-uniform: a wave holds pixels of one row or two)
            const int oy = ty >> 1;
            if (oy >= Ho) continue;
            const char* r0 = dyb + ((size_t)oy * Wo + m) * Cout * ES;            // output column m
            const bool has1 = m + 1 < Wo;                                        // output column m + 1 (left tap of the odd pixel)
            const float* w0 = sw + (ky * 3 + 0) * Cout * NC, *w1 = sw + (ky * 3 + 1) * Cout * NC, *w2 = sw + (ky * 3 + 2) * Cout * NC;
            for (int co = 0; co < Cout; co += 8) {
                float v[8], u[8];
                load8<ES>(r0 + co * ES, v);
                if (has1) load8<ES>(r0 + Cout * ES + co * ES, u);
                else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) u[j] = 0.0f;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        a0[c] = fmaf(w1[(co + j) * NC + c], v[j], a0[c]);                       // 2m     + 1 - 1 = 2 m
                        a1[c] = fmaf(w2[(co + j) * NC + c], v[j], a1[c]);                       // 2m + 1 + 1 - 2 = 2 m
                        a1[c] = fmaf(w0[(co + j) * NC + c], u[j], a1[c]);                       // 2m + 1 + 1 - 0 = 2 (m + 1)
                    }
            }
        }
        const int ix = 2 * m;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float* d = dst + ((size_t)c * B + b) * HW + (size_t)iy * Wi + ix;   // [c][B][1][Hi][Wi]
            d[0] = accumulate ? d[0] + a0[c] : a0[c];
            if (ix + 1 < Wi) d[1] = accumulate ? d[1] + a1[c] : a1[c];
        }
        return;
    }
    const size_t p = (size_t)blockIdx.x * NT + threadIdx.x;
    if (p >= (size_t)B * HW) return;
    const int b = (int)(p / HW);
    const int r = (int)(p - (size_t)b * HW);
    const int iy = r / Wi, ix = r - iy * Wi;
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0f;
    const char* dyb = (const char*)dy + (size_t)b * Ho * Wo * Cout * ES;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int oy = iy + 1 - ky;
        if (oy < 0 || oy >= Ho) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ox = ix + 1 - kx;
            if (ox < 0 || ox >= Wo) continue;
            const char* row = dyb + ((size_t)oy * Wo + ox) * Cout * ES;
            const float* wt = sw + (ky * 3 + kx) * Cout * NC;
            for (int co = 0; co < Cout; co += 8) {
                float v[8];
                load8<ES>(row + co * ES, v);
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int c = 0; c < NC; ++c) acc[c] = fmaf(wt[(co + j) * NC + c], v[j], acc[c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        float* d = dst + ((size_t)c * B + b) * HW + r;   // [c][B][1][Hi][Wi]: every channel a contiguous [B,1,H,W] tensor of its own
        *d = accumulate ? *d + acc[c] : acc[c];
    }
}

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" int colvo_conv_dgrad_planes(const ColvoConvDesc* d, const void* dy, const float* w_master, int c_begin, int c_count,
                                       float* dst, int accumulate, colvo_stream_t stream) {
    COLVO_CHECK_ARG(d && dy && w_master && dst, "colvo_conv_dgrad_planes: null pointer argument");
    COLVO_CHECK_ARG(d->dtype == COLVO_F32 || d->dtype == COLVO_BF16, "colvo_conv_dgrad_planes: bad dtype %d", d->dtype);
    COLVO_CHECK_ARG(d->ksize == 3 && (d->stride == 1 || d->stride == 2) && d->C1 == 0 && !d->up0,
                    "colvo_conv_dgrad_planes: a 3x3 conv over one directly stored source, stride 1 or 2");
    COLVO_CHECK_ARG(d->Ho == (d->Hi - 1) / d->stride + 1 && d->Wo == (d->Wi - 1) / d->stride + 1 && d->B >= 1,
                    "colvo_conv_dgrad_planes: output %dx%d does not match input %dx%d / stride %d", d->Ho, d->Wo, d->Hi, d->Wi, d->stride);
    COLVO_CHECK_ARG(d->Cout >= 8 && d->Cout % 8 == 0 && d->Cout <= 128 && (c_count == 1 || c_count == 2 || c_count == 4) && c_begin >= 0 &&
                    c_begin + c_count <= d->C0,
                    "colvo_conv_dgrad_planes: Cout a multiple of 8 up to 128, 1 / 2 / 4 channels inside [0, C0) (Cout=%d, channels %d..%d of %d)",
                    d->Cout, c_begin, c_begin + c_count - 1, d->C0);
    if (d->dtype == COLVO_BF16 && d->stride == 2 && d->Cout == 16 && c_count == 2 && d->Hi % 2 == 0 && d->Wi % 2 == 0 &&
        (long long)d->B * d->Ho * d->Wo * 32 < 0x7fffffffLL && TUNE(planes_mfma) != 0) {
        // PoseNet's first layer in the training step: one small MFMA product per 2 x 2 block of input pixels (csrc/bwd16.hip)
        const int rc = colvo::launch_dgrad_planes_s2_mfma(dy, w_master, d->C0, c_begin, d->B, d->Hi, d->Wi, d->Ho, d->Wo, dst, accumulate,
                                                          (hipStream_t)stream);
        if (rc != 0) return rc;
        COLVO_CHECK_LAUNCH("k_dgrad_planes_s2_mfma");
        return 0;
    }
    const size_t npix = d->stride == 2 ? (size_t)d->B * d->Hi * ((d->Wi + 1) / 2) : (size_t)d->B * d->Hi * d->Wi;   // threads
    const size_t lds = (size_t)9 * d->Cout * c_count * 4;
    hipStream_t s = (hipStream_t)stream;
#define COLVO_DGP(NC_)                                                                                                            \
    colvo::launch((k_conv_dgrad_planes<ES, NC_>), dim3(nblk(npix)), dim3(NT), lds, s, dy, w_master, d->Cout, d->C0, c_begin, d->B, \
                       d->Hi, d->Wi, d->Ho, d->Wo, d->stride, dst, accumulate)
    DISPATCH_ES(d->dtype, if (c_count == 1) COLVO_DGP(1); else if (c_count == 2) COLVO_DGP(2); else COLVO_DGP(4));
#undef COLVO_DGP
    COLVO_CHECK_LAUNCH("k_conv_dgrad_planes");
    return 0;
}
