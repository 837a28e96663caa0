// pose_tail.hip -- PoseNet's deep layers conv5-conv7 (128 -> 256 -> 256 -> 256, stride 2, bf16) and their input gradients at small
// batches as WHOLE-K RESIDENT launches.
//
// Why: at 8 pairs these maps are 8 x 10, 4 x 5 and 2 x 3 pixels.  k_conv3x3 / k_dgrad_s2 (conv.hip) tile by (image, pixel tile, 32
// output channels) and walk the 4 or 8 channel chunks of K one after another -- stage, barrier, nine k-groups, next chunk -- so a
// launch is a chain of 4-8 dependent round trips for 0.03-0.4 GFLOP (about 0.9 us per chunk + 3 us, profiles/r6_fwd_vs_frames.md),
// in the serial island between DepthNet's forward and backward pass.  Splitting K (across workgroups, or across teams of a
// workgroup) pays a seam larger than what it saves (profiles/r3_splitk_negative.md).  Here the chain is removed
// instead: for these layers the WHOLE K extent of a workgroup's operands fits in LDS, so a workgroup
//   * owns 16 output channels x all pixels of P whole images (no halo: the zero padding is one zero pixel in LDS that out-of-range
//     and zero-inserted taps read),
//   * requests its whole [16][9][K] weight slab, its P source maps and its bias with every global load issued before the first wait,
//   * and after ONE barrier each wave runs complete K chains for the 16-pixel fragments it owns (fragments are filled across images)
//     and stores from the accumulators.
// No grid barrier, no flag, no atomic: a workgroup depends on nothing but its own loads.
//
// Bits: every output element is the sum the replaced launch forms for it.
//   * WK_CONV (forward; conv7's input gradient = stride-1 conv over the zero-dilated dy): k_conv3x3's order -- one accumulator per
//     element, the 32-channel chunks in ascending order, within a chunk k-group m = tap m (granule 4 m + kg: tap m, channel granule
//     kg), one v_mfma_f32_16x16x32_bf16 per (chunk, tap) with A = weights, B = pixels; a tap outside the map or on an inserted zero
//     multiplies the weights by zeros and IS issued (the accumulator may hold -0).  Then mfma_result_guard's in-place terminator
//     and the plain kernels' close (conv_lane.h lane_close_bf16; DESIGN.md section 3.3 has the rule).
//   * WK_DGRAD_S2 (conv6's and conv5's input gradient): k_dgrad_s2's order -- per chunk, slot m of the flipped slab goes to the
//     accumulator of its tap's parity class, reading dy at the tap's offset (conv_lane.h s2_tap); closed the same way.
// Which pixels share a fragment does not enter a column's sum, so fragments may span images and channel tiles may be 16 wide.
// The planner selects a layer only where conv_plain_form says the plain call would run one of exactly these forms
// (tests/test_pose_tail_gpu.py).
#define COLVO_ACC_CONSTRAINT "+v"     // built with -mllvm -amdgpu-mfma-vgpr-form (coivo_amd/build.py)
#include "conv_lane.h"

namespace colvo {
namespace {

constexpr int WK_NT = 512;                         // 8 waves: the staging loads of up to 160 KB are held in registers (<= 21 per thread)
constexpr int WK_IN_PPT = 12;                      // source granules per thread held in registers
enum { WK_CONV = 0, WK_DGRAD_S2 = 1 };

struct WholeK {
    const char* src;                               // [B][Hs][Ws][K]
    const char* w;                                 // [N][9][K]
    const float* bias;                             // [N] or null
    const char* mask;                              // shape of out, or null
    char* out;
    int B, P;                                      // images; images per workgroup
    int Hs, Ws;                                    // stored source extent
    int Ho, Wo;                                    // positions per image the fragments run over
    int N, ntn;                                    // output channels, N / 16
    int S, dil;                                    // WK_CONV: stride over the virtual input; dil 1: the virtual input is the source zero-dilated
    int relu;
    int pixp, wrow;                                // LDS pitches (bytes) of a source pixel and of a weight row
    int in_gran;                                   // 16-byte granules of ONE source image
};

// LDS: [16 weight rows][one zero pixel][P source maps, pixel-major]
template <int NCH, int KIND>
__global__ __launch_bounds__(WK_NT, 1) void k_conv_wholek(const WholeK a) {
    constexpr int CG = NCH * 4;                    // granules per pixel (K / 8)
    constexpr int RG = 9 * CG;                     // ... per weight row
    constexpr int W_GR = 16 * RG, W_PPT = (W_GR + WK_NT - 1) / WK_NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sW = smem;
    char* sZ = smem + 16 * a.wrow;
    char* sIn = sZ + a.pixp;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kg = lane >> 4;
    // logical id = (image group, channel tile), channel tile fastest: an XCD's workgroups share few weight slabs
    const int lid = __builtin_amdgcn_readfirstlane(blockIdx.x);
    const int grp = lid / a.ntn, n0 = (lid - grp * a.ntn) * 16;
    const int b0 = grp * a.P, pe = min(a.P, a.B - b0);

    // ---- every global load of the staging phase, back to back ----
    const __amdgpu_buffer_rsrc_t rw =
        __builtin_amdgcn_make_buffer_rsrc((void*)(a.w + (size_t)n0 * RG * 16), 0, W_GR * 16, 0x00020000);
    u32x4 wv[W_PPT];
#pragma unroll
    for (int it = 0; it < W_PPT; ++it) {
        const int i = it * WK_NT + tid;
        wv[it] = bld16(rw, i < W_GR ? i * 16 : OOB_OFF, 0);
    }
    const int in_total = pe * a.in_gran;
    const __amdgpu_buffer_rsrc_t rin =
        __builtin_amdgcn_make_buffer_rsrc((void*)(a.src + (size_t)b0 * a.in_gran * 16), 0, in_total * 16, 0x00020000);
    u32x4 pv[WK_IN_PPT];
#pragma unroll
    for (int it = 0; it < WK_IN_PPT; ++it) {
        const int i = it * WK_NT + tid;
        pv[it] = bld16(rin, i < in_total ? i * 16 : OOB_OFF, 0);
    }
    const __amdgpu_buffer_rsrc_t rbias = __builtin_amdgcn_make_buffer_rsrc((void*)a.bias, 0, a.bias ? a.N * 4 : 0, 0x00020000);
    const u32x4 biasv = bld16(rbias, (n0 + kg * 4) * 4, 0);                      // zeros without a bias

    __builtin_amdgcn_sched_barrier(0);             // (hipcc otherwise sinks a third of the loads behind the first LDS stores)

    // ---- LDS ----
#pragma unroll
    for (int it = 0; it < W_PPT; ++it) {
        const int i = it * WK_NT + tid;
        if (W_GR % WK_NT == 0 || i < W_GR) {
            const int n = i / RG;
            st16(sW + i * 16 + n * (a.wrow - RG * 16), wv[it]);
        }
    }
#pragma unroll
    for (int it = 0; it < WK_IN_PPT; ++it) {
        const int i = it * WK_NT + tid;
        if (i < in_total) st16(sIn + (i / CG) * a.pixp + (i % CG) * 16, pv[it]);
    }
    if (tid < CG) st16(sZ + tid * 16, u32x4{0u, 0u, 0u, 0u});
    __syncthreads();

    // ---- complete K chains: items = 16-pixel fragments over the workgroup's images, dealt over the waves ----
    const int hw = a.Ho * a.Wo;
    const int npix = pe * hw;
    const int nfrag = (npix + 15) >> 4;
    const int opi = KIND == WK_DGRAD_S2 ? 4 * hw : hw;                            // output pixels per image
    const int out_bytes = pe * opi * a.N * 2;
    const __amdgpu_buffer_rsrc_t rout =
        __builtin_amdgcn_make_buffer_rsrc((void*)(a.out + (size_t)b0 * opi * a.N * 2), 0, out_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rmask = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.mask ? a.mask + (size_t)b0 * opi * a.N * 2 : a.out), 0, a.mask ? out_bytes : 0, 0x00020000);
    const char* pin = sZ + kg * 16;
    const char* pw = sW + l15 * a.wrow + kg * 16;

    for (int item = wave; item < nfrag; item += WK_NT / 64) {
        const int p = item * 16 + l15;
        const bool valid = p < npix;
        const int pc = valid ? p : 0;                                             // padding columns: any valid LDS address, not stored
        const int bi = pc / hw, rem = pc - bi * hw;
        const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
        if constexpr (KIND == WK_CONV) {
            const int goff = valid ? (p * a.N + n0 + kg * 4) * 2 : OOB_OFF;
            u32x2 pm = {0u, 0u};
            if (a.mask) pm = __builtin_amdgcn_raw_buffer_load_b64(rmask, goff, 0, 0);
            const int Hv = a.Hs << a.dil, Wv = a.Ws << a.dil;
            int aoff[9];                                                          // byte offsets from the zero pixel
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ky = t / 3, kx = t - 3 * ky;
                const int vy = oy * a.S + ky - 1, vx = ox * a.S + kx - 1;
                const bool inb = (unsigned)vy < (unsigned)Hv && (unsigned)vx < (unsigned)Wv && ((vy | vx) & a.dil) == 0;
                aoff[t] = inb ? (1 + (bi * a.Hs + (vy >> a.dil)) * a.Ws + (vx >> a.dil)) * a.pixp : 0;
            }
            f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                u32x4 av[9], bv[9];
#pragma unroll
                for (int m = 0; m < 9; ++m) {
                    av[m] = ld16(pin + aoff[m] + k * 64);
                    bv[m] = ld16(pw + (m * CG + k * 4) * 16);
                }
#pragma unroll
                for (int m = 0; m < 9; ++m)
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bv[m]), __builtin_bit_cast(bf16x8, av[m]),
                                                                     acc[0], 0, 0, 0);
            }
            mfma_result_guard<bf16_t>(acc);
            // lane_close_bf16 with its first half (lane_bias_relu) written out: through the helper hipcc swaps the source operands of
            // the four bias adds, the only change in the listing (profiles/conv_lane_ab.md)
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[0][r] + __uint_as_float(biasv[r]);
            if (a.relu) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.0f);
            }
            if (a.mask) relu_mask_keep(pm[0], pm[1], v);
            const u32x2 o = lane_pack_bf16(v);
            __builtin_amdgcn_raw_buffer_store_b64(o, rout, goff, 0, 0);            // out of range: dropped
        } else {
            // position (oy, ox) of dy: parity class (py, px) of the input gradient is pixel (2 oy + py, 2 ox + px)
            int goff[4];
            u32x2 pm[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int gy = 2 * oy + (c >> 1), gx = 2 * ox + (c & 1);
                goff[c] = valid ? (((bi * 2 * a.Ho + gy) * 2 * a.Wo + gx) * a.N + n0 + kg * 4) * 2 : OOB_OFF;
                pm[c] = u32x2{0u, 0u};
                if (a.mask) pm[c] = __builtin_amdgcn_raw_buffer_load_b64(rmask, goff[c], 0, 0);
            }
            int aoff[4];                                                          // dy at (+ row, + column); beyond the map: zero
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int y = oy + (q >> 1), x = ox + (q & 1);
                aoff[q] = (y < a.Ho && x < a.Wo) ? (1 + (bi * a.Ho + y) * a.Wo + x) * a.pixp : 0;
            }
            f32x4 acc[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                u32x4 av[4], bv[9];
#pragma unroll
                for (int q = 0; q < 4; ++q) av[q] = ld16(pin + aoff[q] + k * 64);
#pragma unroll
                for (int m = 0; m < 9; ++m) bv[m] = ld16(pw + (m * CG + k * 4) * 16);
#pragma unroll
                for (int m = 0; m < 9; ++m) {
                    const S2Tap tp = s2_tap(m);
                    acc[tp.cls] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        __builtin_bit_cast(bf16x8, bv[m]), __builtin_bit_cast(bf16x8, av[2 * tp.dy + tp.dx]), acc[tp.cls], 0, 0, 0);
                }
            }
            mfma_result_guard<bf16_t>(acc);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                // (k_dgrad_s2's epilogue adds its zero bias)
                const u32x2 o = lane_close_bf16(acc[c], u32x4{0u, 0u, 0u, 0u}, 0, a.mask != nullptr, pm[c]);
                __builtin_amdgcn_raw_buffer_store_b64(o, rout, goff[c], 0, 0);
            }
        }
    }
}

struct PoseTailPlan { int kind, nch, nwg, lds; WholeK k; };

// Reads the descriptor and the tuning table only.  true: layer d goes as one k_conv_wholek launch -- its forward pass (direction 0)
// or its input gradient (direction 1); p.k then holds everything of the kernel argument but the pointers and the ReLU flag.
bool pose_tail_plan(const ColvoConvDesc* d, int direction, PoseTailPlan& p) {
    if (!d || !TUNE(pose_tail) || (direction != 0 && direction != 1)) return false;
    if (direction == 1 && !TUNE(pose_tail_bwd)) return false;
    if (d->dtype != COLVO_BF16 || d->ksize != 3 || d->stride != 2 || d->C1 != 0 || d->up0 || d->up1) return false;
    if (d->B < 1 || d->B > TUNE(pose_tail_max_pairs) || d->Hi < 1 || d->Wi < 1) return false;
    const int K = direction == 0 ? d->C0 : d->Cout, N = direction == 0 ? d->Cout : d->C0;
    if ((K != 128 && K != 256) || N < 16 || N % 16) return false;
    WholeK& k = p.k;
    k = WholeK{};
    // the bit guarantee is against ONE reference per layer and direction: the form the plain call would take
    const PlainForm f = conv_plain_form(d, direction == 0 ? PASS_FWD : PASS_DGRAD, "colvo_pose_tail_plan");
    // k_conv3x3 over 32-channel chunks, in any of its one-tile forms (one chunk in flight, the two-chunk ring, 512 threads): the chunks
    // in ascending order, tap by tap
    const bool tile32 = f.form == CONV_TILE && f.ng == 4;
    if (direction == 0) {
        if (!tile32) return false;
        p.kind = WK_CONV;
        k.Hs = d->Hi; k.Ws = d->Wi; k.Ho = d->Ho; k.Wo = d->Wo; k.S = 2; k.dil = 0;
        k.pixp = pitch_bytes_s2(K * 2);            // consecutive fragment rows are two source pixels apart
    } else {
        if (f.form == DGRAD_S2) {                  // k_dgrad_s2: s2_tap's order, chunk by chunk
            p.kind = WK_DGRAD_S2;
            k.Hs = d->Ho; k.Ws = d->Wo; k.Ho = d->Ho; k.Wo = d->Wo; k.S = 1; k.dil = 0;
        } else if (tile32 && f.dilated) {          // the same k_conv3x3 order over the zero-dilated dy
            p.kind = WK_CONV;
            k.Hs = d->Ho; k.Ws = d->Wo; k.Ho = d->Hi; k.Wo = d->Wi; k.S = 1; k.dil = 1;
        } else {
            return false;
        }
        k.pixp = pitch_bytes(K * 2);
    }
    p.nch = K / 32;
    k.B = d->B; k.N = N; k.ntn = N / 16;
    k.wrow = wrow_bytes(9 * K / 8);
    const long long in_gran = (long long)k.Hs * k.Ws * (K / 8);
    if (in_gran > WK_IN_PPT * WK_NT) return false;
    k.in_gran = (int)in_gran;
    // images per workgroup: the fewest at which the grid is a single round (more workgroups with fewer images each cost only L2
    // re-reads of the weight slabs); beyond that, as many as LDS and the staging registers hold
    const int forced = (int)TUNE(pose_tail_images);
    auto lds_of = [&](int P) { return (long long)16 * k.wrow + k.pixp + (long long)P * k.Hs * k.Ws * k.pixp; };
    auto fits = [&](int P) { return lds_of(P) <= 160 * 1024 && (long long)P * in_gran <= WK_IN_PPT * WK_NT; };
    int P = 0;
    if (forced > 0) {
        P = std::min(forced, d->B);
        if (!fits(P)) return false;
    } else {
        for (int q = 1; q <= d->B && fits(q); ++q) {
            P = q;
            if ((long long)((d->B + q - 1) / q) * k.ntn <= 256) break;
        }
        if (P == 0) return false;
    }
    k.P = P;
    p.nwg = (d->B + P - 1) / P * k.ntn;
    p.lds = (int)lds_of(P);
    return true;
}

template <int NCH, int KIND>
int launch_wholek(const PoseTailPlan& p, hipStream_t s, const char* who) {
    return launch_resident<k_conv_wholek<NCH, KIND>>((unsigned)p.nwg, WK_NT, p.lds, s, who, "k_conv_wholek", p.k);
}

int launch_pose_tail(const PoseTailPlan& p, hipStream_t s, const char* who) {
    if (p.kind == WK_CONV) return p.nch == 4 ? launch_wholek<4, WK_CONV>(p, s, who) : launch_wholek<8, WK_CONV>(p, s, who);
    return p.nch == 4 ? launch_wholek<4, WK_DGRAD_S2>(p, s, who) : launch_wholek<8, WK_DGRAD_S2>(p, s, who);
}

}  // namespace

// CMD_CONV_FWD with i[0] = -1 (program.hip): p = x, -, w_fwd, bias, y as in the plain form.  A layer the planner does not select is
// an error: the caller asks colvo_pose_tail_plan first.  Counts no form.
int pose_tail_fwd(const ColvoCmd& c, hipStream_t s) {
    const ColvoConvDesc* d = &c.desc;
    COLVO_CHECK_ARG(c.p[0] && !c.p[1] && c.p[2] && c.p[4], "colvo_conv_fwd (whole-K form): needs x0, w_fwd and y, and takes no second source");
    PoseTailPlan p{};
    COLVO_CHECK_ARG(pose_tail_plan(d, 0, p), "colvo_conv_fwd: the whole-K form is not selected for this descriptor "
                                             "(colvo_pose_tail_plan answers 0): issue the plain form");
    p.k.src = (const char*)c.p[0]; p.k.w = (const char*)c.p[2]; p.k.bias = (const float*)c.p[3]; p.k.out = (char*)c.p[4];
    p.k.mask = nullptr; p.k.relu = d->relu;
    return launch_pose_tail(p, s, "colvo_conv_fwd (whole-K form)");
}

// CMD_CONV_DGRAD with i[2] = 1 (program.hip): p = dy, w_bwd, relu_mask, dx; i = src (0), accumulate (0), 1.
int pose_tail_dgrad(const ColvoCmd& c, hipStream_t s) {
    const ColvoConvDesc* d = &c.desc;
    COLVO_CHECK_ARG(c.p[0] && c.p[1] && c.p[3], "colvo_conv_dgrad (whole-K form): null pointer argument");
    COLVO_CHECK_ARG(c.i[0] == 0 && c.i[1] == 0 && c.i[2] == 1,
                    "colvo_conv_dgrad (whole-K form): source 0, no accumulate, i[2] = 1 (src=%d accumulate=%d i[2]=%d)", c.i[0], c.i[1], c.i[2]);
    PoseTailPlan p{};
    COLVO_CHECK_ARG(pose_tail_plan(d, 1, p), "colvo_conv_dgrad: the whole-K form is not selected for this descriptor "
                                             "(colvo_pose_tail_plan answers 0): issue the plain form");
    p.k.src = (const char*)c.p[0]; p.k.w = (const char*)c.p[1]; p.k.bias = nullptr; p.k.mask = (const char*)c.p[2];
    p.k.out = (char*)c.p[3]; p.k.relu = 0;
    return launch_pose_tail(p, s, "colvo_conv_dgrad (whole-K form)");
}

}  // namespace colvo

using namespace colvo;

extern "C" int colvo_pose_tail_plan(const ColvoConvDesc* d, int direction, int32_t* out) {
    PoseTailPlan p{};
    if (!pose_tail_plan(d, direction, p)) return 0;
    if (out) { out[0] = p.nwg; out[1] = p.k.P; out[2] = p.lds; out[3] = p.kind; }
    return 1;
}
