// augment.hip -- the input conversion of frames.hip with a per-frame augmentation folded into the same pass:
// u8 interleaved -> crop / mirror / bilinear resize -> 3x4 colour map -> clamp -> gamma -> planar fp32, one launch, the source read
// once.  HBM / L2-bound like its sibling: 4 taps of 3 bytes in (neighbours share them), 12 B out per output pixel; the frame's row of
// the parameter table (80 B) is wave-uniform and arrives through scalar loads, once per wave.
//
// The coordinate and blend arithmetic is k_frames_u8_to_f32's, term for term, with every rounding pinned (fmaf / __fmul_rn) to what
// the compiler makes of that kernel: with an identity row the two agree bit for bit (tests/test_augment_gpu.py).
#include "common.h"

namespace colvo {
namespace {

constexpr int NT = 256;
static_assert(sizeof(ColvoAugRow) == 80 && sizeof(ColvoAugRow) % 16 == 0, "table rows are 80 bytes (coivo_amd/_lib.py AUG_ROW_FLOATS)");

// 0 <= result <= n-1 for any t (NaN -> 0): the tap index of a source coordinate already clamped into [0, n]
__device__ __forceinline__ int tap(float t, int n) { return min((int)t, n - 1); }

// grid (ceil(W/64), ceil(H/4), n): a 64x4 output tile per workgroup, one output pixel (3 channels) per thread
__global__ __launch_bounds__(NT) void k_frames_u8_augment(const uint8_t* __restrict__ src, int h, int w, int H, int W,
                                                          const ColvoAugRow* __restrict__ params, float* __restrict__ dst) {
    const int b = blockIdx.z;
    const ColvoAugRow& p = params[b];             // uniform address: scalar loads
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    // a mirrored frame reverses the READS: lane x still stores column x
    const int xs = p.flip != 0 ? W - 1 - x : x;
    // source index = origin + step * (dst + 0.5) - 0.5, one rounding; fmaxf sends a NaN to 0, and the upper clamp (never active for a
    // crop inside the frame: the index then stays below h - 0.5) keeps the conversion to int defined for any table
    const float fy = fminf(fmaxf(fmaf(p.sy, (float)y + 0.5f, p.oy - 0.5f), 0.0f), (float)h);
    const float fx = fminf(fmaxf(fmaf(p.sx, (float)xs + 0.5f, p.ox - 0.5f), 0.0f), (float)w);
    const int y0 = tap(fy, h), x0 = tap(fx, w);
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    const uint8_t* img = src + (size_t)b * h * w * 3;
    const uint8_t* p00 = img + ((size_t)y0 * w + x0) * 3;
    const uint8_t* p01 = img + ((size_t)y0 * w + x1) * 3;
    const uint8_t* p10 = img + ((size_t)y1 * w + x0) * 3;
    const uint8_t* p11 = img + ((size_t)y1 * w + x1) * 3;
    float rgb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = fmaf(hx, (float)p00[c], __fmul_rn(lx, (float)p01[c]));
        const float bot = fmaf(hx, (float)p10[c], __fmul_rn(lx, (float)p11[c]));
        rgb[c] = __fdiv_rn(fmaf(hy, top, __fmul_rn(ly, bot)), 255.0f);
    }
    const size_t plane = (size_t)H * W;
    float* o = dst + (size_t)b * 3 * plane + (size_t)y * W + x;
    const float gamma = p.gamma;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* a = p.A + 4 * c;
        float v = fmaf(a[0], rgb[0], fmaf(a[1], rgb[1], fmaf(a[2], rgb[2], a[3])));
        v = fminf(fmaxf(v, 0.0f), 1.0f);          // (a NaN becomes 0)
        if (gamma != 1.0f) v = fminf(fmaxf(powf(v, gamma), 0.0f), 1.0f);      // uniform branch; the clamp only matters for a senseless gamma
        o[c * plane] = v;
    }
}

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" int colvo_frames_u8_augment(const uint8_t* frames, int n, int h, int w, int H, int W, const ColvoAugRow* params,
                                       float* out, colvo_stream_t stream) {
    COLVO_CHECK_ARG(frames && params && out, "colvo_frames_u8_augment: null pointer argument");
    COLVO_CHECK_ARG(((uintptr_t)params & 15) == 0, "colvo_frames_u8_augment: the parameter table must be 16-byte aligned");
    COLVO_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0 && H > 0 && W > 0 && (long long)h * w < (1ll << 28) &&
                        (long long)H * W < (1ll << 28) && (H + 3) / 4 <= 65535,
                    "colvo_frames_u8_augment: bad shape n=%d %dx%d -> %dx%d", n, h, w, H, W);
    colvo::launch(k_frames_u8_augment, dim3((W + 63) / 64, (H + 3) / 4, n), dim3(NT), 0, (hipStream_t)stream, frames, h, w, H, W,
                  params, out);
    COLVO_CHECK_LAUNCH("k_frames_u8_augment");
    return 0;
}
