// pose_front.hip -- PoseNet's three front layers (8 -> 16 -> 32 -> 64, all stride 2, bias + ReLU, bf16) in ONE launch.
//
// Why: at 8 pairs every one of these layers is a launch at the floor (6-7 us each whatever its flops), and
// they sit in the serial island between DepthNet's forward and backward pass, where one kernel is in flight at a time.  A stride-2
// pyramid shrinks, so a workgroup can carry ONE conv3 tile through all three levels with a small halo recompute and no grid-wide
// hand-over: a toh x tow tile of conv3 needs (2 toh + 1) x (2 tow + 1) of conv2, (4 toh + 3) x (4 tow + 3) of conv1 and
// (8 toh + 7) x (8 tow + 7) input pixels.  The weights of all three layers (24 192 parameters) stay in LDS.
//
// Bits: every output element is the sum the one-tile kernel k_conv3x3 (conv.hip) forms for it -- one channel chunk per layer, the
// same v_mfma_f32_16x16x32_bf16 per k-group of four 16-byte granules (granule = tap * NG + channel granule, padded k-groups read
// tap 8's pixels against zero weights), k-groups in ascending order from a zero accumulator, the in-place terminator of
// mfma_result_guard, then the close the plain kernels use (conv_lane.h lane_close_bf16; DESIGN.md section 3.3 has the rule).  Which
// pixels share a fragment does not enter a column's sum, so the three maps are byte-identical to three colvo_conv_fwd calls in their
// one-tile form (tests/test_pose_front_gpu.py); the planner selects the chain only where conv_plain_form says that is the form
// they would take.
//
// The padding trap: each level's zero padding is the border of that level's MAP.  A halo position outside conv1's (conv2's) map is
// stored as zero in the LDS tile, never as the layer evaluated outside the image.
#define COLVO_ACC_CONSTRAINT "+v"     // built with -mllvm -amdgpu-mfma-vgpr-form (coivo_amd/build.py)
#include "conv_lane.h"

namespace colvo {
namespace {

constexpr int PF_NT = 512;                         // 8 waves: two per SIMD, the (fragment, channel tile) items are dealt over them
constexpr int PF_TOH = 4;                          // conv3 tile rows; the planner picks the width from {8, 10}
constexpr int PF_IN_PPT = 7;                       // input-patch granules per thread held in registers: 39 x 87 <= 7 x 512
constexpr int PF_W3_GR = 64 * 36;                  // conv3's weight granules: [64][9][32] bf16, rows contiguous
constexpr int PF_W3_PPT = (PF_W3_GR + PF_NT - 1) / PF_NT;

// LDS pitches (bytes): input pixels 16 (one granule), conv1 / conv2 tiles at the stride-2 pitches of conv_common.h
constexpr int PF_PIX0 = pitch_bytes_s2(16), PF_PIX1 = pitch_bytes_s2(32), PF_PIX2 = pitch_bytes_s2(64);
constexpr int PF_WROW1 = wrow_bytes(12), PF_WROW2 = wrow_bytes(20), PF_WROW3 = wrow_bytes(36);

struct PoseFrontK {
    const char* x;                                 // [B][H][W][8]
    const char *w1, *w2, *w3;                      // w_fwd [N][9][C]
    const float *b1, *b2, *b3;
    char *a1, *a2, *a3;                            // [B][H/2][W/2][16], [B][H/4][W/4][32], [B][H/8][W/8][64]
    int H, W;
    int tow, tiles_x, tiles_y;
    uint32_t m_pw0, m_w1, m_w2, m_w3;              // magic divisors: input patch width, conv1 / conv2 / conv3 tile widths
    int relu;
};

struct PoseFrontLds { int in, a1, a2, w1, w2, bias, total; };
inline PoseFrontLds pose_front_lds(int tow) {
    const int ph0 = 8 * PF_TOH + 7, pw0 = 8 * tow + 7, ph1 = 4 * PF_TOH + 3, pw1 = 4 * tow + 3, ph2 = 2 * PF_TOH + 1, pw2 = 2 * tow + 1;
    PoseFrontLds l;
    l.in = 0;                                       // the input patch; conv3's weights move in once conv1 has read it
    l.a1 = std::max(ph0 * pw0 * PF_PIX0, 64 * PF_WROW3);
    l.a2 = l.a1 + ph1 * pw1 * PF_PIX1;
    l.w1 = l.a2 + ph2 * pw2 * PF_PIX2;
    l.w2 = l.w1 + 16 * PF_WROW1;
    l.bias = l.w2 + 32 * PF_WROW2;
    l.total = l.bias + (16 + 32 + 64) * 4;
    return l;
}

// One level of the pyramid over the workgroup's tile: input tile in LDS (sIn, rows of inW pixels at PIXP_IN bytes, NG granules per
// pixel), weights in LDS (rows of WROW bytes), OH x OW outputs of 16 * NFT channels whose position (0, 0) is map position
// (gy0, gx0).  Items = (16-pixel fragment, 16-channel tile), dealt over the waves.  Written: the LDS tile of the next level (zero
// outside the map) and, for the owned rectangle inside the map, global memory.
template <int NG, int NFT, int PIXP_IN, int PIXP_OUT>
__device__ __forceinline__ void pose_front_level(const char* sIn, int inW, const char* sW, const float* sBias, int OH, int OW,
                                                 uint32_t m_ow, int gy0, int gx0, int Hm, int Wm, int own_y0, int own_x0, int own_h,
                                                 int own_w, char* sOut, char* gout, int relu, int wave, int l15, int kg) {
    constexpr int STEPS = (9 * NG + 3) / 4;
    constexpr int WROW = wrow_bytes(STEPS * 4);
    constexpr int N = 16 * NFT;
    const int npix = OH * OW;
    const int nitems = ((npix + 15) >> 4) * NFT;
    const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc((void*)gout, 0, Hm * Wm * N * 2, 0x00020000);
    for (int item = wave; item < nitems; item += PF_NT / 64) {
        const int f = item / NFT, nf = item - f * NFT;
        const int p = f * 16 + l15;
        const bool valid = p < npix;
        const int pc = valid ? p : 0;
        const int oy = mdiv(pc, m_ow), ox = pc - oy * OW;
        const char* pin = sIn + ((oy * 2) * inW + ox * 2) * PIXP_IN;
        const char* pw = sW + (nf * 16 + l15) * WROW;
        u32x4 av[STEPS], bv[STEPS];
#pragma unroll
        for (int m = 0; m < STEPS; ++m) {
            const int gi = 4 * m + kg;
            int tap = gi / NG;
            const int cg = gi - tap * NG;
            tap = min(tap, 8);                      // padded k-groups multiply real pixels by zero weights (as k_conv3x3 does)
            const int ky = tap / 3, kx = tap - 3 * ky;
            av[m] = ld16(pin + (ky * inW + kx) * PIXP_IN + cg * 16);
            bv[m] = ld16(pw + gi * 16);
        }
        f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int m = 0; m < STEPS; ++m)
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bv[m]), __builtin_bit_cast(bf16x8, av[m]), acc[0],
                                                             0, 0, 0);
        const u32x4 bs = *reinterpret_cast<const u32x4*>(sBias + nf * 16 + kg * 4);
        mfma_result_guard<bf16_t>(acc);
        u32x2 o = lane_close_bf16(acc[0], bs, relu, false, u32x2{0u, 0u});
        const int gy = gy0 + oy, gx = gx0 + ox;
        const bool inmap = valid && (unsigned)gy < (unsigned)Hm && (unsigned)gx < (unsigned)Wm;
        if (sOut != nullptr && valid) {
            if (!inmap) o = u32x2{0u, 0u};          // the next level's zero padding is THIS map's border
            *reinterpret_cast<u32x2*>(sOut + p * PIXP_OUT + (nf * 16 + kg * 4) * 2) = o;
        }
        const bool own = inmap && (unsigned)(oy - own_y0) < (unsigned)own_h && (unsigned)(ox - own_x0) < (unsigned)own_w;
        const int goff = own ? ((gy * Wm + gx) * N + nf * 16 + kg * 4) * 2 : OOB_OFF;      // out of range: store dropped
        __builtin_amdgcn_raw_buffer_store_b64(o, rout, goff, 0, 0);
    }
}

__global__ __launch_bounds__(PF_NT, 1) void k_pose_front_fwd(const PoseFrontK a, const PoseFrontLds L) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sIn = smem + L.in;
    char* sA1 = smem + L.a1;
    char* sA2 = smem + L.a2;
    char* sW1 = smem + L.w1;
    char* sW2 = smem + L.w2;
    char* sW3 = smem + L.in;                        // after conv1
    float* sBias = reinterpret_cast<float*>(smem + L.bias);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kg = lane >> 4;
    const int lid = __builtin_amdgcn_readfirstlane(blockIdx.x);
    const int tpi = a.tiles_x * a.tiles_y;
    const int b = lid / tpi, trem = lid - b * tpi;
    const int ty = trem / a.tiles_x, tx = trem - ty * a.tiles_x;
    const int oy3 = ty * PF_TOH, ox3 = tx * a.tow;               // tile origin in conv3's map
    const int H1 = a.H >> 1, W1 = a.W >> 1, H2 = a.H >> 2, W2 = a.W >> 2, H3 = a.H >> 3, W3 = a.W >> 3;
    const int PH0 = 8 * PF_TOH + 7, PW0 = 8 * a.tow + 7;
    const int PH1 = 4 * PF_TOH + 3, PW1 = 4 * a.tow + 3;
    const int PH2 = 2 * PF_TOH + 1, PW2 = 2 * a.tow + 1;
    const int iy0 = 8 * oy3 - 7, ix0 = 8 * ox3 - 7;              // input patch origin; conv1's at 4 o - 3, conv2's at 2 o - 1

    // ---- all global loads of the staging phase, back to back ----
    const __amdgpu_buffer_rsrc_t rw3 = __builtin_amdgcn_make_buffer_rsrc((void*)a.w3, 0, PF_W3_GR * 16, 0x00020000);
    u32x4 w3v[PF_W3_PPT];
#pragma unroll
    for (int it = 0; it < PF_W3_PPT; ++it) {
        const int i = it * PF_NT + tid;
        w3v[it] = bld16(rw3, i < PF_W3_GR ? i * 16 : OOB_OFF, 0);
    }
    const __amdgpu_buffer_rsrc_t rw1 = __builtin_amdgcn_make_buffer_rsrc((void*)a.w1, 0, 16 * 9 * 16, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.w2, 0, 32 * 18 * 16, 0x00020000);
    const u32x4 w1v = bld16(rw1, tid < 16 * 9 ? tid * 16 : OOB_OFF, 0);
    u32x4 w2v[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int i = it * PF_NT + tid;
        w2v[it] = bld16(rw2, i < 32 * 18 ? i * 16 : OOB_OFF, 0);
    }
    float biasv = 0.0f;
    if (tid < 16) biasv = a.b1[tid];
    else if (tid < 48) biasv = a.b2[tid - 16];
    else if (tid < 112) biasv = a.b3[tid - 48];
    const int in_bytes = a.H * a.W * 16;
    const __amdgpu_buffer_rsrc_t rin =
        __builtin_amdgcn_make_buffer_rsrc((void*)(a.x + (size_t)b * in_bytes), 0, in_bytes, 0x00020000);
    const int ptotal = PH0 * PW0;
    u32x4 pv[PF_IN_PPT];
#pragma unroll
    for (int it = 0; it < PF_IN_PPT; ++it) {
        const int i = it * PF_NT + tid;
        const int py = mdiv(i, a.m_pw0), px = i - py * PW0;
        const int vy = iy0 + py, vx = ix0 + px;
        const bool inb = i < ptotal && (unsigned)vy < (unsigned)a.H && (unsigned)vx < (unsigned)a.W;
        pv[it] = bld16(rin, inb ? (vy * a.W + vx) * 16 : OOB_OFF, 0);
    }

    // ---- LDS: conv1 / conv2 weight rows (padding granules zero), biases, the input patch ----
    if (tid < 16 * 3) {                             // conv1: rows of 9 granules padded to 12
        const int n = tid / 3, q = tid - n * 3;
        st16(sW1 + n * PF_WROW1 + (9 + q) * 16, u32x4{0u, 0u, 0u, 0u});
    } else if (tid >= 64 && tid < 64 + 32 * 2) {    // conv2: 18 padded to 20
        const int i = tid - 64, n = i >> 1, q = i & 1;
        st16(sW2 + n * PF_WROW2 + (18 + q) * 16, u32x4{0u, 0u, 0u, 0u});
    }
    if (tid < 16 * 9) {
        const int n = tid / 9;
        st16(sW1 + tid * 16 + n * (PF_WROW1 - 9 * 16), w1v);
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int i = it * PF_NT + tid;
        if (i < 32 * 18) {
            const int n = i / 18;
            st16(sW2 + i * 16 + n * (PF_WROW2 - 18 * 16), w2v[it]);
        }
    }
    if (tid < 112) sBias[tid] = biasv;
#pragma unroll
    for (int it = 0; it < PF_IN_PPT; ++it) {
        const int i = it * PF_NT + tid;
        if (i < ptotal) st16(sIn + i * PF_PIX0, pv[it]);
    }
    __syncthreads();

    // ---- conv1: 8 -> 16 over (4 toh + 3) x (4 tow + 3); owned: the 4 toh x 4 tow behind the three halo rows / columns ----
    pose_front_level<1, 1, PF_PIX0, PF_PIX1>(sIn, PW0, sW1, sBias, PH1, PW1, a.m_w1, 4 * oy3 - 3, 4 * ox3 - 3, H1, W1, 3, 3, 4 * PF_TOH,
                                             4 * a.tow, sA1, a.a1 + (size_t)b * H1 * W1 * 32, a.relu, wave, l15, kg);
    __syncthreads();                                // conv1's tile is complete and the input patch is dead
#pragma unroll
    for (int it = 0; it < PF_W3_PPT; ++it) {
        const int i = it * PF_NT + tid;
        if (i < PF_W3_GR) {
            const int n = i / 36;
            st16(sW3 + i * 16 + n * (PF_WROW3 - 36 * 16), w3v[it]);
        }
    }
    // ---- conv2: 16 -> 32 over (2 toh + 1) x (2 tow + 1); owned: behind one halo row / column ----
    pose_front_level<2, 2, PF_PIX1, PF_PIX2>(sA1, PW1, sW2, sBias + 16, PH2, PW2, a.m_w2, 2 * oy3 - 1, 2 * ox3 - 1, H2, W2, 1, 1,
                                             2 * PF_TOH, 2 * a.tow, sA2, a.a2 + (size_t)b * H2 * W2 * 64, a.relu, wave, l15, kg);
    __syncthreads();
    // ---- conv3: 32 -> 64 over the tile ----
    pose_front_level<4, 4, PF_PIX2, 0>(sA2, PW2, sW3, sBias + 48, PF_TOH, a.tow, a.m_w3, oy3, ox3, H3, W3, 0, 0, PF_TOH, a.tow, nullptr,
                                       a.a3 + (size_t)b * H3 * W3 * 128, a.relu, wave, l15, kg);
}

// --------------------------------------------------------------------------------------------- //
// the input-gradient chain: g3 -> g2 -> g1 -> the two depth planes of conv1's input gradient      //
// --------------------------------------------------------------------------------------------- //
// Replaces conv3's and conv2's k_dgrad_s2 launches (conv.hip) and k_dgrad_planes_s2_mfma (bwd16.hip).  Going down, a level needs only
// a slightly larger patch of the level above: the parity classes of a stride-2 input gradient at position (gy, gx) read
// dy[gy .. gy + 1][gx .. gx + 1], so the workgroup that owns a toh x tow tile of g3 positions writes 2 toh x 2 tow of g2, 4 toh x 4 tow
// of g1 and 8 toh x 8 tow of each plane, and recomputes ONE extra row and column of g2 and of g1 (even parity: they need no further
// g3).  Bits: per dy position the nine taps run once in k_dgrad_s2's order (conv_lane.h s2_tap, chunk by chunk) into the four class
// accumulators, closed by mfma_result_guard and lane_close_bf16 with no bias and the producer's ReLU mask; the planes are
// k_dgrad_planes_s2_mfma's six MFMAs per 16 blocks with its three-term bf16 split of the fp32 master weights.
constexpr int PB_PIX3 = pitch_bytes(128), PB_PIX2 = pitch_bytes(64), PB_PIX1 = pitch_bytes(32);
constexpr int PB_WROW3 = wrow_bytes(72), PB_WROW2 = wrow_bytes(36);     // conv3: two 36-granule chunks per row; conv2: one

struct PoseBackK {
    const char* g3;                                // [B][H/8][W/8][64]
    const char *wb3, *wb2;                         // w_bwd [Cin][9 (flipped)][Cout]: [32][9][64], [16][9][32]
    const float* w1;                               // conv1's fp32 master [16][9][8]
    const char *act2, *act1;                       // ReLU masks
    char *g2, *g1;
    float* dtr;                                    // [2][B][1][H][W]
    int B, H, W, c_begin;
    int tow, tiles_x, tiles_y;
    uint32_t m_p3, m_n3, m_n2;                     // magic divisors: g3 patch width, position-tile widths of the two dgrad levels
};

struct PoseBackLds { int g3, w3, g2, w2, g1, total; };
inline PoseBackLds pose_back_lds(int tow) {
    PoseBackLds l;
    l.g3 = 0;
    l.w3 = (PF_TOH + 2) * (tow + 2) * PB_PIX3;
    l.g2 = l.w3 + 32 * PB_WROW3;
    l.w2 = l.g2 + (2 * PF_TOH + 2) * (2 * tow + 2) * PB_PIX2;
    l.g1 = l.w2 + 16 * PB_WROW2;
    l.total = l.g1 + (4 * PF_TOH + 1) * (4 * tow + 1) * PB_PIX1;
    return l;
}

// One stride-2 input-gradient level: dy tile in LDS (rows of inW pixels at IN_PIX bytes, NCH chunks of 64 bytes per pixel), flipped
// weight rows in LDS, nH x nW dy positions -> their four parity classes, 16 * NFT channels.  Position (0, 0)'s class (0, 0) is map
// pixel (gy0, gx0) of the output, which is kept where it lies inside the outH x outW tile (LDS, rows of outW pixels) and written to
// memory inside the owned own_h x own_w rectangle of the Hm x Wm map.
template <int NCH, int NFT, int IN_PIX, int WROW, int OUT_PIX>
__device__ __forceinline__ void pose_back_level(const char* sIn, int inW, const char* sW, int nH, int nW, uint32_t m_nw, int gy0, int gx0,
                                                int Hm, int Wm, int outH, int outW, int own_h, int own_w, const char* gmask, char* gout,
                                                char* sOut, int wave, int l15, int kg) {
    constexpr int N = 16 * NFT;
    const int npos = nH * nW;
    const int nitems = ((npos + 15) >> 4) * NFT;
    const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc((void*)gout, 0, Hm * Wm * N * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rmask = __builtin_amdgcn_make_buffer_rsrc((void*)gmask, 0, Hm * Wm * N * 2, 0x00020000);
    for (int item = wave; item < nitems; item += PF_NT / 64) {
        const int f = item / NFT, nf = item - f * NFT;
        const int p = f * 16 + l15;
        const bool valid = p < npos;
        const int pc = valid ? p : 0;
        const int oy = mdiv(pc, m_nw), ox = pc - oy * nW;
        // the four classes' mask granules first: their latency hides under the MFMAs
        int goff[4], loff[4];
        u32x2 pm[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int ty = 2 * oy + (c >> 1), tx = 2 * ox + (c & 1);
            const int gy = gy0 + ty, gx = gx0 + tx;
            const bool intile = valid && ty < outH && tx < outW;
            const bool inmap = intile && gy < Hm && gx < Wm;
            const int off = ((gy * Wm + gx) * N + nf * 16 + kg * 4) * 2;
            pm[c] = __builtin_amdgcn_raw_buffer_load_b64(rmask, inmap ? off : OOB_OFF, 0, 0);       // outside the map: 0 -> masked
            goff[c] = (inmap && ty < own_h && tx < own_w) ? off : OOB_OFF;
            loff[c] = intile ? (ty * outW + tx) * OUT_PIX + (nf * 16 + kg * 4) * 2 : -1;
        }
        const char* pin = sIn + (oy * inW + ox) * IN_PIX + kg * 16;
        const char* pw = sW + (nf * 16 + l15) * WROW + kg * 16;
        f32x4 acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            u32x4 av[9], bv[9];
#pragma unroll
            for (int m = 0; m < 9; ++m) {
                const S2Tap tp = s2_tap(m);
                av[m] = ld16(pin + ((tp.dy ? inW : 0) + tp.dx) * IN_PIX + k * 64);
                bv[m] = ld16(pw + (k * 36 + 4 * m) * 16);
            }
#pragma unroll
            for (int m = 0; m < 9; ++m) {
                const int cls = s2_tap(m).cls;
                acc[cls] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bv[m]), __builtin_bit_cast(bf16x8, av[m]),
                                                                   acc[cls], 0, 0, 0);
            }
        }
        mfma_result_guard<bf16_t>(acc);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            // (k_dgrad_s2's epilogue adds its zero bias)
            const u32x2 o = lane_close_bf16(acc[c], u32x4{0u, 0u, 0u, 0u}, 0, true, pm[c]);
            if (loff[c] >= 0) *reinterpret_cast<u32x2*>(sOut + loff[c]) = o;
            __builtin_amdgcn_raw_buffer_store_b64(o, rout, goff[c], 0, 0);                         // out of range: dropped
        }
    }
}

__global__ __launch_bounds__(PF_NT, 1) void k_pose_front_bwd(const PoseBackK a, const PoseBackLds L) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sG3 = smem + L.g3;
    char* sW3 = smem + L.w3;
    char* sG2 = smem + L.g2;
    char* sW2 = smem + L.w2;
    char* sG1 = smem + L.g1;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kg = lane >> 4;
    const int lid = __builtin_amdgcn_readfirstlane(blockIdx.x);
    const int tpi = a.tiles_x * a.tiles_y;
    const int b = lid / tpi, trem = lid - b * tpi;
    const int ty = trem / a.tiles_x, tx = trem - ty * a.tiles_x;
    const int y3 = ty * PF_TOH, x3 = tx * a.tow;
    const int H1 = a.H >> 1, W1 = a.W >> 1, H2 = a.H >> 2, W2 = a.W >> 2, H3 = a.H >> 3, W3 = a.W >> 3;
    const int P3H = PF_TOH + 2, P3W = a.tow + 2;                 // g3 patch: the tile, its halo row / column, one more the unused classes read
    const int T2H = 2 * PF_TOH + 1, T2W = 2 * a.tow + 1;         // g2 / g1 tiles kept: the owned part and one halo row / column
    const int T1H = 4 * PF_TOH + 1, T1W = 4 * a.tow + 1;

    // ---- global loads of the staging phase, back to back: g3 patch, both flipped weight tensors ----
    const int g3_bytes = H3 * W3 * 128;
    const __amdgpu_buffer_rsrc_t rg3 =
        __builtin_amdgcn_make_buffer_rsrc((void*)(a.g3 + (size_t)b * g3_bytes), 0, g3_bytes, 0x00020000);
    constexpr int G3_PPT = ((PF_TOH + 2) * 12 * 8 + PF_NT - 1) / PF_NT;      // tow <= 10
    const int g3_total = P3H * P3W * 8;
    u32x4 g3v[G3_PPT];
    int g3lds[G3_PPT];
#pragma unroll
    for (int it = 0; it < G3_PPT; ++it) {
        const int i = it * PF_NT + tid;
        const int pix = i >> 3, cg = i & 7;
        const int py = mdiv(pix, a.m_p3), px = pix - py * P3W;
        const int vy = y3 + py, vx = x3 + px;
        const bool inb = i < g3_total && vy < H3 && vx < W3;
        g3v[it] = bld16(rg3, inb ? ((vy * W3 + vx) * 8 + cg) * 16 : OOB_OFF, 0);
        g3lds[it] = i < g3_total ? pix * PB_PIX3 + cg * 16 : -1;
    }
    constexpr int W3_GR = 32 * 72, W3_PPT = (W3_GR + PF_NT - 1) / PF_NT, W2_GR = 16 * 36, W2_PPT = (W2_GR + PF_NT - 1) / PF_NT;
    const __amdgpu_buffer_rsrc_t rw3 = __builtin_amdgcn_make_buffer_rsrc((void*)a.wb3, 0, W3_GR * 16, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.wb2, 0, W2_GR * 16, 0x00020000);
    u32x4 w3v[W3_PPT], w2v[W2_PPT];
#pragma unroll
    for (int it = 0; it < W3_PPT; ++it) {
        const int i = it * PF_NT + tid;
        w3v[it] = bld16(rw3, i < W3_GR ? i * 16 : OOB_OFF, 0);
    }
#pragma unroll
    for (int it = 0; it < W2_PPT; ++it) {
        const int i = it * PF_NT + tid;
        w2v[it] = bld16(rw2, i < W2_GR ? i * 16 : OOB_OFF, 0);
    }
    // the planes' A operand, exactly as k_dgrad_planes_s2_mfma builds it: row n = l15 = (py, px, c),
    // k = 32 q + 8 kg + j = (gy = q, gx = kg >> 1, co = 8 (kg & 1) + j); fp32 masters split into three bf16 terms
    bf16x8 wa[2][3];
    {
        const int n = l15, c = n & 1, px = (n >> 1) & 1, py = (n >> 2) & 1, gx = kg >> 1;
        const int kx = px == 0 ? (gx == 0 ? 1 : -1) : (gx == 0 ? 2 : 0);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int ky = py == 0 ? (q == 0 ? 1 : -1) : (q == 0 ? 2 : 0);
            const bool on = n < 8 && kx >= 0 && ky >= 0;
            uint16_t t0[8], t1[8], t2[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int co = 8 * (kg & 1) + j;
                const float wv = on ? a.w1[((size_t)co * 9 + ky * 3 + kx) * 8 + a.c_begin + c] : 0.0f;
                t0[j] = f2bf(wv);
                const float r1 = wv - bf2f(t0[j]);
                t1[j] = f2bf(r1);
                t2[j] = f2bf(r1 - bf2f(t1[j]));
            }
            auto pack = [](const uint16_t (&t)[8]) {
                const u32x4 v = u32x4{(unsigned)t[0] | ((unsigned)t[1] << 16), (unsigned)t[2] | ((unsigned)t[3] << 16),
                                      (unsigned)t[4] | ((unsigned)t[5] << 16), (unsigned)t[6] | ((unsigned)t[7] << 16)};
                return __builtin_bit_cast(bf16x8, v);
            };
            wa[q][0] = pack(t0); wa[q][1] = pack(t1); wa[q][2] = pack(t2);
        }
    }
    // ---- LDS ----
#pragma unroll
    for (int it = 0; it < G3_PPT; ++it)
        if (g3lds[it] >= 0) st16(sG3 + g3lds[it], g3v[it]);
#pragma unroll
    for (int it = 0; it < W3_PPT; ++it) {
        const int i = it * PF_NT + tid;
        if (i < W3_GR) {                            // row n: 9 slots x 8 granules in memory -> two chunks of 9 slots x 4 granules
            const int n = i / 72, j = i - n * 72, m = j >> 3, c8 = j & 7;
            st16(sW3 + n * PB_WROW3 + ((c8 >> 2) * 36 + m * 4 + (c8 & 3)) * 16, w3v[it]);
        }
    }
#pragma unroll
    for (int it = 0; it < W2_PPT; ++it) {
        const int i = it * PF_NT + tid;
        if (i < W2_GR) {
            const int n = i / 36;
            st16(sW2 + i * 16 + n * (PB_WROW2 - 36 * 16), w2v[it]);
        }
    }
    // the row behind the g2 tile (rows of T2W pixels) is read by classes whose results are dropped: keep it defined
    for (int i = tid; i < (T2W + 2) * 4; i += PF_NT) st16(sG2 + (T2H * T2W + (i >> 2)) * PB_PIX2 + (i & 3) * 16, u32x4{0u, 0u, 0u, 0u});
    __syncthreads();

    // ---- g2 = dgrad(conv3) masked by act2 > 0: (toh + 1) x (tow + 1) positions, 32 channels, two 32-channel chunks of g3 ----
    pose_back_level<2, 2, PB_PIX3, PB_WROW3, PB_PIX2>(sG3, P3W, sW3, PF_TOH + 1, a.tow + 1, a.m_n3, 2 * y3, 2 * x3, H2, W2, T2H, T2W,
                                                      2 * PF_TOH, 2 * a.tow, a.act2 + (size_t)b * H2 * W2 * 64,
                                                      a.g2 + (size_t)b * H2 * W2 * 64, sG2, wave, l15, kg);
    __syncthreads();
    // ---- g1 = dgrad(conv2) masked by act1 > 0: (2 toh + 1) x (2 tow + 1) positions, 16 channels ----
    pose_back_level<1, 1, PB_PIX2, PB_WROW2, PB_PIX1>(sG2, T2W, sW2, T2H, T2W, a.m_n2, 4 * y3, 4 * x3, H1, W1, T1H, T1W, 4 * PF_TOH,
                                                      4 * a.tow, a.act1 + (size_t)b * H1 * W1 * 32, a.g1 + (size_t)b * H1 * W1 * 32, sG1,
                                                      wave, l15, kg);
    __syncthreads();
    // ---- planes: a 2 x 2 block of input pixels (2Y + py, 2X + px) from g1[Y .. Y + 1][X .. X + 1]; 16 blocks of a row per step ----
    const int ngx = (4 * a.tow + 15) >> 4;
    const size_t plane = (size_t)a.B * a.H * a.W;
    for (int gid = wave; gid < 4 * PF_TOH * ngx; gid += PF_NT / 64) {
        const int Y = gid / ngx, X = (gid - Y * ngx) * 16 + l15;
        const int gY = 4 * y3 + Y, gX = 4 * x3 + X;
        const int xx = min(X + (kg >> 1), T1W - 1);                // lanes beyond the tile's blocks: any defined pixel, nothing stored
        u32x4 gv[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) gv[q] = ld16(sG1 + ((Y + q) * T1W + xx) * PB_PIX1 + (kg & 1) * 16);
        f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int sp = 0; sp < 3; ++sp)
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[q][sp], __builtin_bit_cast(bf16x8, gv[q]), acc[0], 0, 0, 0);
        mfma_result_guard<bf16_t>(acc);
        // lane (block l15, kg < 2): rows n = 4 kg + r = (py = kg, px = r >> 1, c = r & 1) -> input row 2Y + kg, columns 2X, 2X + 1
        if (kg < 2 && X < 4 * a.tow && gY < H1 && gX < W1) {
            const size_t o = ((size_t)b * a.H + 2 * gY + kg) * a.W + 2 * gX;
            *reinterpret_cast<float2*>(a.dtr + o) = make_float2(acc[0][0], acc[0][2]);
            *reinterpret_cast<float2*>(a.dtr + plane + o) = make_float2(acc[0][1], acc[0][3]);
        }
    }
}

struct PoseFrontPlan { int tow, tiles_x, tiles_y, nwg, lds; };

// The layers behind layer 1's descriptor: the chain's fixed channel counts at halved extents
ColvoConvDesc pose_front_layer(const ColvoConvDesc& d1, int i) {
    static const int ch[4] = {8, 16, 32, 64};
    ColvoConvDesc d = d1;
    d.Hi = d1.Hi >> i; d.Wi = d1.Wi >> i;
    d.Ho = d.Hi >> 1; d.Wo = d.Wi >> 1;
    d.C0 = ch[i]; d.Cout = ch[i + 1];
    return d;
}

// Reads the descriptor and the tuning table only.  true: layers 1-3 behind d1 go as one k_pose_front_fwd launch (direction 0), or their
// input-gradient chain down to the two depth planes as one k_pose_front_bwd launch (direction 1).
bool pose_front_plan(const ColvoConvDesc* d1, int direction, PoseFrontPlan& p) {
    if (!d1 || !TUNE(pose_front) || (direction != 0 && direction != 1)) return false;
    if (direction == 1 && !TUNE(pose_front_bwd)) return false;
    if (d1->dtype != COLVO_BF16 || d1->ksize != 3 || d1->stride != 2 || !d1->relu || d1->C0 != 8 || d1->C1 != 0 || d1->up0 || d1->up1 ||
        d1->Cout != 16)
        return false;
    if (d1->B < 1 || d1->Hi < 8 || d1->Wi < 8 || (d1->Hi & 7) || (d1->Wi & 7) || d1->Ho != d1->Hi / 2 || d1->Wo != d1->Wi / 2) return false;
    if ((long long)d1->Hi * d1->Wi * 16 >= 0x40000000LL) return false;             // per-image byte offsets are 32-bit
    // the bit guarantee is against ONE reference: every layer would otherwise take the one-tile form of k_conv3x3 -- in both
    // directions, so that one batch size (13 pairs of 256x320, where conv2 goes to the stride-2 resident kernel) ends both chains --
    for (int i = 0; i < 3; ++i) {
        const ColvoConvDesc d = pose_front_layer(*d1, i);
        const PlainForm f = conv_plain_form(&d, PASS_FWD, "colvo_pose_front_plan");
        // k_conv3x3, 256 threads, one chunk in flight: k-groups in ascending order into one accumulator
        if (!(f.form == CONV_TILE && f.nth == NT && f.depth == 1)) return false;
    }
    if (direction == 1) {
        // ... and the three replaced launches theirs: k_dgrad_s2 with one chunk in flight for conv3 and conv2, k_dgrad_planes_s2_mfma
        // (the condition of colvo_conv_dgrad_planes, csrc/dgrad_planes.hip)
        for (int i = 1; i < 3; ++i) {
            const ColvoConvDesc d = pose_front_layer(*d1, i);
            const PlainForm f = conv_plain_form(&d, PASS_DGRAD, "colvo_pose_front_plan");
            // k_dgrad_s2, K loop not unrolled: s2_tap's order, chunk by chunk
            if (!(f.form == DGRAD_S2 && f.nch == 0)) return false;
        }
        if ((long long)d1->B * d1->Ho * d1->Wo * 32 >= 0x7fffffffLL || TUNE(planes_mfma) == 0) return false;
    }
    // conv3 tiles of 4 x 8 or 4 x 10: one workgroup per CU at a time (LDS), so fewer rounds of 256 first, then the narrower tile
    const int H3 = d1->Hi >> 3, W3 = d1->Wi >> 3;
    long best = -1;
    for (int tow : {8, 10}) {
        const int tx = (W3 + tow - 1) / tow, ty = (H3 + PF_TOH - 1) / PF_TOH;
        const long long nwg = (long long)tx * ty * d1->B;
        if (nwg >= (1ll << 30)) return false;
        const long cost = (long)((nwg + 255) / 256) * tow;
        if (best < 0 || cost < best) {
            best = cost;
            p.tow = tow; p.tiles_x = tx; p.tiles_y = ty; p.nwg = (int)nwg;
        }
    }
    p.lds = direction == 0 ? pose_front_lds(p.tow).total : pose_back_lds(p.tow).total;
    return p.lds <= 160 * 1024 && (8 * PF_TOH + 7) * (8 * p.tow + 7) <= PF_IN_PPT * PF_NT;
}

}  // namespace

// CMD_CONV_FWD with a chain length in i[0] (program.hip): p = x, -, w1, b1, a1, w2, b2, a2, w3, b3, a3; i = 3, 16, 32, 64.
// A chain the planner does not select is an error: the caller asks colvo_pose_front_plan first.
int pose_front_fwd(const ColvoCmd& c, hipStream_t s) {
    const ColvoConvDesc* d = &c.desc;
    COLVO_CHECK_ARG(c.i[0] == 3 && c.i[1] == 16 && c.i[2] == 32 && c.i[3] == 64,
                    "colvo_conv_fwd: chain of %d layers (%d, %d, %d channels): only PoseNet's 8 -> 16 -> 32 -> 64 front", c.i[0], c.i[1],
                    c.i[2], c.i[3]);
    for (int k : {0, 2, 3, 4, 5, 6, 7, 8, 9, 10}) COLVO_CHECK_ARG(c.p[k], "colvo_conv_fwd: null pointer argument (chain slot %d)", k);
    PoseFrontPlan p{};
    COLVO_CHECK_ARG(pose_front_plan(d, 0, p), "colvo_conv_fwd: the three-layer chain is not selected for this descriptor "
                                              "(colvo_pose_front_plan answers 0): issue the layers one by one");
    PoseFrontK k{};
    k.x = (const char*)c.p[0];
    k.w1 = (const char*)c.p[2]; k.b1 = (const float*)c.p[3]; k.a1 = (char*)c.p[4];
    k.w2 = (const char*)c.p[5]; k.b2 = (const float*)c.p[6]; k.a2 = (char*)c.p[7];
    k.w3 = (const char*)c.p[8]; k.b3 = (const float*)c.p[9]; k.a3 = (char*)c.p[10];
    k.H = d->Hi; k.W = d->Wi;
    k.tow = p.tow; k.tiles_x = p.tiles_x; k.tiles_y = p.tiles_y;
    k.m_pw0 = mdiv_magic(8 * p.tow + 7); k.m_w1 = mdiv_magic(4 * p.tow + 3); k.m_w2 = mdiv_magic(2 * p.tow + 1); k.m_w3 = mdiv_magic(p.tow);
    k.relu = d->relu;
    return launch_resident<k_pose_front_fwd>((unsigned)p.nwg, PF_NT, p.lds, s, "colvo_conv_fwd (chain)", "k_pose_front_fwd", k,
                                             pose_front_lds(p.tow));
}

// CMD_CONV_DGRAD_PLANES with g3 in p[3] (program.hip): p = g1, w_master (conv1), d_tr, g3, w_bwd3, w_bwd2, act2, act1, g2, g1;
// i = c_begin, c_count, accumulate; desc: conv1's.  Writes g2, g1 (the weight gradients of conv2 and conv1 read them) and d_tr.
int pose_front_bwd(const ColvoCmd& c, hipStream_t s) {
    const ColvoConvDesc* d = &c.desc;
    for (int k = 0; k < 10; ++k) COLVO_CHECK_ARG(c.p[k], "colvo_conv_dgrad_planes: null pointer argument (chain slot %d)", k);
    COLVO_CHECK_ARG(c.p[0] == c.p[9], "colvo_conv_dgrad_planes: chain form: p[0] (the planes' dy) and p[9] (g1) are the same tensor");
    COLVO_CHECK_ARG(c.i[0] >= 0 && c.i[0] + 2 <= d->C0 && c.i[1] == 2 && c.i[2] == 0,
                    "colvo_conv_dgrad_planes: chain form: two channels inside [0, C0), no accumulate (c_begin=%d c_count=%d accumulate=%d)",
                    c.i[0], c.i[1], c.i[2]);
    PoseFrontPlan p{};
    COLVO_CHECK_ARG(pose_front_plan(d, 1, p), "colvo_conv_dgrad_planes: the input-gradient chain is not selected for this descriptor "
                                              "(colvo_pose_front_plan answers 0): issue the launches one by one");
    PoseBackK k{};
    k.w1 = (const float*)c.p[1]; k.dtr = (float*)c.p[2]; k.g3 = (const char*)c.p[3];
    k.wb3 = (const char*)c.p[4]; k.wb2 = (const char*)c.p[5]; k.act2 = (const char*)c.p[6]; k.act1 = (const char*)c.p[7];
    k.g2 = (char*)c.p[8]; k.g1 = (char*)c.p[9];
    k.B = d->B; k.H = d->Hi; k.W = d->Wi; k.c_begin = c.i[0];
    k.tow = p.tow; k.tiles_x = p.tiles_x; k.tiles_y = p.tiles_y;
    k.m_p3 = mdiv_magic(p.tow + 2); k.m_n3 = mdiv_magic(p.tow + 1); k.m_n2 = mdiv_magic(2 * p.tow + 1);
    return launch_resident<k_pose_front_bwd>((unsigned)p.nwg, PF_NT, p.lds, s, "colvo_conv_dgrad_planes (chain)", "k_pose_front_bwd", k,
                                             pose_back_lds(p.tow));
}

}  // namespace colvo

using namespace colvo;

extern "C" int colvo_pose_front_plan(const ColvoConvDesc* d1, int direction, int32_t* out) {
    PoseFrontPlan p{};
    if (!pose_front_plan(d1, direction, p)) return 0;
    if (out) { out[0] = p.nwg; out[1] = PF_TOH; out[2] = p.tow; out[3] = p.lds; }
    return 1;
}
