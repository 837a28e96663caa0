// stem.hip -- DepthNet's stem in ONE launch at small batches: the packing pass of the pair batch (colvo_pack_stem_pose), enc1a
// (8 -> 32, stride 2) and enc1b (32 -> 32, stride 1), bf16.
//
// Why: the three launches are bound by their bytes (profiles/r6_fwd_vs_frames.md) and two thirds of what the second and third read
// is what the launch before has just written: the packed stem input (21 MB at 16 frames of 256 x 320) and enc1a's output (21 MB).
// Here a persistent workgroup walks output tiles of enc1b with both layers' weight slabs resident in LDS; per tile it
//   1. takes the fp32 planar frame patch the tile needs through both layers -- (2 toh + 5) x (2 tow + 5) pixels, requested during the
//      previous tile's MFMA phases, three planes of up to ST_PPT pixels per thread in registers --, rounds it to bf16 as
//      k_pack_stem_pose does (layout.hip), puts it into LDS and stores the pixels the tile OWNS (its 2 toh x 2 tow inputs, not
//      the halo) to the stem input, one whole 16-byte pixel per store.  A workgroup's item is a PAIR tile: the same tile of frame p
//      and of frame Bh + p, one after the other, and a thread holds the same patch pixels in both -- so it keeps the target frame's
//      three channels in two registers and stores PoseNet's pixel [tgt rgb | ref rgb | 0 0] whole, once, with the second;
//   2. computes enc1a on the tile plus a one-pixel halo, (toh + 2) x (tow + 2) positions in 16-pixel fragments dealt over the waves,
//      into LDS -- positions outside the map are ZERO there: they are enc1b's padding -- and stores the tile's own pixels;
//   3. computes enc1b from that LDS image as k_conv3x3_res does from its patch, and stores it.
// Two barriers a tile; nothing crosses workgroups.
//
// Bits: every output element is the sum the replaced launch forms for it.
//   * enc1a: k_conv3x3 / k_conv3x3_res<.., S2> with ONE-granule chunks (NG = 1): one accumulator per element, k-groups m = 0, 1, 2 in
//     ascending order, lane group kg of k-group m holds tap 4 m + kg; the three padded granules 9..11 multiply tap 8's pixel by zero
//     weights and ARE issued.  One v_mfma_f32_16x16x32_bf16 per k-group with A = weights, B = pixels.
//   * enc1b: the same kernels with 32-channel chunks (NG = 4), one chunk: k-group m = tap m, lane group kg = channel granule kg.
//   Then mfma_result_guard's in-place terminator and lane_close_bf16 (conv_lane.h).  Which pixels share a fragment or a tile does not
//   enter a column's sum.  The planner selects the launch only where conv_plain_form says both plain calls would run these forms.
#define COLVO_ACC_CONSTRAINT "+v"     // built with -mllvm -amdgpu-mfma-vgpr-form (coivo_amd/build.py)
#include "conv_lane.h"

namespace colvo {
namespace {

constexpr int ST_NT = 256;
constexpr int ST_PPT = 4;                          // patch pixels per thread held in registers (three planes each)
constexpr int ST_N = 32;                           // output channels of both layers
constexpr int ST_W1ROW = wrow_bytes(12);           // enc1a's weight row in LDS: 9 real + 3 zero granules
constexpr int ST_W2ROW = wrow_bytes(36);           // enc1b's: 9 taps x 4 granules
constexpr int ST_PIXI = 8;                         // a frame pixel in LDS: its three bf16 channels and one zero (the other four are not stored)
constexpr int ST_PIXA = pitch_bytes(64);           // an enc1a pixel in LDS

struct StemK {
    const float* frames;                           // [2 Bh][3][H][W]
    char* stem;                                    // [2 Bh][H][W][8]
    char* pose_in;                                 // [Bh][H][W][8]
    const char* w1; const float* b1; char* y1;     // enc1a: [32][9][8], [32], [2 Bh][H1][W1][32]
    const char* w2; const float* b2; char* y2;     // enc1b: [32][9][32], [32], [2 Bh][H1][W1][32]
    int Bh, H, W, H1, W1;
    int relu1, relu2;
    int toh, tow, tiles_x, tiles_y;                // tiles of enc1b's output
    int ewp;                                       // LDS row pitch of the enc1a image, in pixels (>= tow + 2: pick_tile's padding)
    uint32_t m_pw, m_ew, m_tow;                    // magic divisors: patch width, enc1a region width, tile width
    int nitems;                                    // pair tiles: Bh x tiles per image
};

// LDS: [enc1a weights][enc1b weights][frame patch, 8 bytes a pixel][enc1a image: tile + halo]
__global__ __launch_bounds__(ST_NT, 2) void k_stem(const StemK a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int PH = 2 * a.toh + 5, PW = 2 * a.tow + 5;              // frame patch
    const int EH = a.toh + 2, EW = a.tow + 2;                      // enc1a region
    char* sW1 = smem;
    char* sW2 = sW1 + ST_N * ST_W1ROW;
    char* sIn = sW2 + ST_N * ST_W2ROW;
    char* sA = sIn + ((PH * PW * ST_PIXI + 15) & ~15);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kg = lane >> 4;
    const int HW = a.H * a.W, HW1 = a.H1 * a.W1;
    const int tpi = a.tiles_x * a.tiles_y;

    // ---- both weight slabs and biases, once ----
    {
        const __amdgpu_buffer_rsrc_t rw1 = __builtin_amdgcn_make_buffer_rsrc((void*)a.w1, 0, ST_N * 9 * 16, 0x00020000);
        const __amdgpu_buffer_rsrc_t rw2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.w2, 0, ST_N * 36 * 16, 0x00020000);
        constexpr int W1_GR = ST_N * 12, W1_IT = (W1_GR + ST_NT - 1) / ST_NT;
        constexpr int W2_GR = ST_N * 36, W2_IT = (W2_GR + ST_NT - 1) / ST_NT;
        u32x4 v1[W1_IT], v2[W2_IT];
#pragma unroll
        for (int it = 0; it < W1_IT; ++it) {
            const int i = it * ST_NT + tid, n = i / 12, gi = i - n * 12;
            v1[it] = bld16(rw1, (i < W1_GR && gi < 9) ? (n * 9 + gi) * 16 : OOB_OFF, 0);      // granules 9..11 of a row: zeros
        }
#pragma unroll
        for (int it = 0; it < W2_IT; ++it) {
            const int i = it * ST_NT + tid;
            v2[it] = bld16(rw2, i < W2_GR ? i * 16 : OOB_OFF, 0);
        }
#pragma unroll
        for (int it = 0; it < W1_IT; ++it) {
            const int i = it * ST_NT + tid, n = i / 12, gi = i - n * 12;
            if (W1_GR % ST_NT == 0 || i < W1_GR) st16(sW1 + n * ST_W1ROW + gi * 16, v1[it]);
        }
#pragma unroll
        for (int it = 0; it < W2_IT; ++it) {
            const int i = it * ST_NT + tid, n = i / 36, gi = i - n * 36;
            if (W2_GR % ST_NT == 0 || i < W2_GR) st16(sW2 + n * ST_W2ROW + gi * 16, v2[it]);
        }
    }
    u32x4 b1v[2], b2v[2];
    {
        const __amdgpu_buffer_rsrc_t rb1 = __builtin_amdgcn_make_buffer_rsrc((void*)a.b1, 0, a.b1 ? ST_N * 4 : 0, 0x00020000);
        const __amdgpu_buffer_rsrc_t rb2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.b2, 0, a.b2 ? ST_N * 4 : 0, 0x00020000);
#pragma unroll
        for (int nf = 0; nf < 2; ++nf) {
            b1v[nf] = bld16(rb1, (nf * 16 + kg * 4) * 4, 0);      // zeros without a bias
            b2v[nf] = bld16(rb2, (nf * 16 + kg * 4) * 4, 0);
        }
    }

    // descriptors over the WHOLE tensors (host guarantees < 1 GiB each): an offset of OOB_OFF reads zeros / drops the store
    const int nimg = 2 * a.Bh;
    const __amdgpu_buffer_rsrc_t rfr = __builtin_amdgcn_make_buffer_rsrc((void*)a.frames, 0, nimg * 3 * HW * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rstem = __builtin_amdgcn_make_buffer_rsrc((void*)a.stem, 0, nimg * HW * 16, 0x00020000);
    const __amdgpu_buffer_rsrc_t rpose = __builtin_amdgcn_make_buffer_rsrc((void*)a.pose_in, 0, a.Bh * HW * 16, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry1 = __builtin_amdgcn_make_buffer_rsrc((void*)a.y1, 0, nimg * HW1 * ST_N * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.y2, 0, nimg * HW1 * ST_N * 2, 0x00020000);

    // this thread's patch pixels: their place in the patch is tile-invariant.  ppy = 0x4000: beyond the patch, never in range
    int ppy[ST_PPT], ppx[ST_PPT];
    bool own[ST_PPT];
#pragma unroll
    for (int it = 0; it < ST_PPT; ++it) {
        const int i = it * ST_NT + tid;
        const int py = mdiv(i, a.m_pw);
        ppx[it] = i - py * PW;
        ppy[it] = i < PH * PW ? py : 0x4000;
        own[it] = ppy[it] >= 3 && ppy[it] < 3 + 2 * a.toh && ppx[it] >= 3 && ppx[it] < 3 + 2 * a.tow;
    }
    // enc1b: the two fragment columns (tile pixels) of this lane
    const int npix = a.toh * a.tow;
    int pbase[2], poy[2], pox[2];
#pragma unroll
    for (int mf = 0; mf < 2; ++mf) {
        const int p = wave * 32 + mf * 16 + l15;
        const int pc = p < npix ? p : 0;
        const int oy = mdiv(pc, a.m_tow), ox = pc - oy * a.tow;
        pbase[mf] = (oy * a.ewp + ox) * ST_PIXA;
        poy[mf] = p < npix ? oy : 0x4000;
        pox[mf] = ox;
    }

    struct Item { int frame, pair, oy0, ox0; };
    auto item_of = [&](int j) -> Item {               // wave-uniform: step j of this workgroup's walk = (pair tile, half)
        const int t = __builtin_amdgcn_readfirstlane((int)blockIdx.x + (j >> 1) * (int)gridDim.x);
        const int tt = t < a.nitems ? t : 0;
        const int p = tt / tpi, tr_ = tt - p * tpi;   // (scalar divisions, twice a tile: a one-tile image divides by 1)
        const int ty = tr_ / a.tiles_x, tx = tr_ - ty * a.tiles_x;
        return Item{t < a.nitems ? p + (j & 1) * a.Bh : -1, p, ty * a.toh, tx * a.tow};
    };
    float pv[ST_PPT][3];
    auto load_p = [&](const Item& o) {
        const int iy0 = 2 * o.oy0 - 3, ix0 = 2 * o.ox0 - 3;
        const int soff = o.frame * 3 * HW * 4;
#pragma unroll
        for (int it = 0; it < ST_PPT; ++it) {
            const int vy = iy0 + ppy[it], vx = ix0 + ppx[it];
            const bool inb = (unsigned)vy < (unsigned)a.H && (unsigned)vx < (unsigned)a.W;
            const int off = inb ? (vy * a.W + vx) * 4 : OOB_OFF;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                pv[it][c] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rfr, off, soff + c * HW * 4, 0));
        }
    };

    Item cur = item_of(0);
    if (cur.frame >= 0) load_p(cur);
    uint32_t tw[ST_PPT][2];                           // the target frame's three channels of this thread's pixels, kept for the pair's second half
#pragma unroll
    for (int it = 0; it < ST_PPT; ++it) tw[it][0] = tw[it][1] = 0u;

    for (int j = 0; cur.frame >= 0; ++j) {
        // ---- 1. pack: patch -> LDS, owned pixels -> the stem input and (second half) PoseNet's input ----
        {
            const int iy0 = 2 * cur.oy0 - 3, ix0 = 2 * cur.ox0 - 3;
            const int second = j & 1;
#pragma unroll
            for (int it = 0; it < ST_PPT; ++it) {
                const int i = it * ST_NT + tid;
                const unsigned c0 = f2bf(pv[it][0]), c1 = f2bf(pv[it][1]), c2 = f2bf(pv[it][2]);
                const uint32_t w0 = c0 | (c1 << 16), w1 = c2;
                if (ppy[it] != 0x4000) *reinterpret_cast<u32x2*>(sIn + i * ST_PIXI) = u32x2{w0, w1};
                const int vy = iy0 + ppy[it], vx = ix0 + ppx[it];
                const bool st = own[it] && vy < a.H && vx < a.W;           // (an owned pixel has vy, vx >= 0)
                const int off = st ? (vy * a.W + vx) * 16 : OOB_OFF;
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{w0, w1, 0u, 0u}, rstem, off, cur.frame * HW * 16, 0);
                if (second) {
                    const u32x4 pw = {tw[it][0], (tw[it][1] & 0xFFFFu) | (w0 << 16), (w0 >> 16) | (w1 << 16), 0u};
                    __builtin_amdgcn_raw_buffer_store_b128(pw, rpose, off, cur.pair * HW * 16, 0);
                } else {
                    tw[it][0] = w0; tw[it][1] = w1;
                }
            }
        }
        __syncthreads();                              // the patch is in LDS; the previous tile's enc1b has finished reading sA
        const Item nxt = item_of(j + 1);
        if (nxt.frame >= 0) load_p(nxt);              // in flight during both MFMA phases below

        // ---- 2. enc1a on the tile plus halo -> sA (zero outside the map), own pixels -> y1 ----
        {
            const int npos = EH * EW, nfrag = (npos + 15) >> 4;
            const int soff = cur.frame * HW1 * ST_N * 2;
            for (int f = wave; f < nfrag; f += ST_NT / 64) {
                const int p = f * 16 + l15;
                const bool pvalid = p < npos;
                const int pc = pvalid ? p : 0;        // padding columns: any valid LDS address, nothing stored
                const int ey = mdiv(pc, a.m_ew), ex = pc - ey * EW;
                const int gy = cur.oy0 - 1 + ey, gx = cur.ox0 - 1 + ex;
                const bool inimg = pvalid && (unsigned)gy < (unsigned)a.H1 && (unsigned)gx < (unsigned)a.W1;
                const bool mine = inimg && ey >= 1 && ey <= a.toh && ex >= 1 && ex <= a.tow;
                const char* pin = sIn + ((2 * ey) * PW + 2 * ex) * ST_PIXI;
                f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const int gi = 4 * m + kg;
                    const int tap = min(gi, 8);       // padded granules multiply real pixels by zero weights
                    const int ky = tap / 3, kx = tap - 3 * ky;
                    const u32x2 lo = *reinterpret_cast<const u32x2*>(pin + (ky * PW + kx) * ST_PIXI);
                    const u32x4 av = {lo[0], lo[1], 0u, 0u};      // channels 4..7 of the packed pixel are zero
                    u32x4 bv[2];
#pragma unroll
                    for (int nf = 0; nf < 2; ++nf) bv[nf] = ld16(sW1 + (nf * 16 + l15) * ST_W1ROW + gi * 16);
#pragma unroll
                    for (int nf = 0; nf < 2; ++nf)
                        acc[nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bv[nf]), __builtin_bit_cast(bf16x8, av),
                                                                         acc[nf], 0, 0, 0);
                }
                mfma_result_guard<bf16_t>(acc);
                const int goff = mine ? (gy * a.W1 + gx) * ST_N * 2 + kg * 8 : OOB_OFF;
                char* pa = sA + (ey * a.ewp + ex) * ST_PIXA + kg * 8;
#pragma unroll
                for (int nf = 0; nf < 2; ++nf) {
                    u32x2 o = lane_close_bf16(acc[nf], b1v[nf], a.relu1, false, u32x2{0u, 0u});
                    __builtin_amdgcn_raw_buffer_store_b64(o, ry1, goff + (mine ? nf * 32 : 0), soff, 0);
                    if (!inimg) o = u32x2{0u, 0u};    // enc1b's zero padding, not enc1a evaluated off the map
                    if (pvalid) *reinterpret_cast<u32x2*>(pa + nf * 32) = o;
                }
            }
        }
        __syncthreads();                              // sA is complete; every wave is done reading the patch

        // ---- 3. enc1b from sA -> y2 ----
        {
            f32x4 acc[2][2];
#pragma unroll
            for (int mf = 0; mf < 2; ++mf)
#pragma unroll
                for (int nf = 0; nf < 2; ++nf) acc[mf][nf] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int m = 0; m < 9; ++m) {
                const int ky = m / 3, kx = m - 3 * ky;
                const int aoff = (ky * a.ewp + kx) * ST_PIXA + kg * 16;
                u32x4 av[2], bv[2];
#pragma unroll
                for (int mf = 0; mf < 2; ++mf) av[mf] = ld16(sA + pbase[mf] + aoff);
#pragma unroll
                for (int nf = 0; nf < 2; ++nf) bv[nf] = ld16(sW2 + (nf * 16 + l15) * ST_W2ROW + (4 * m + kg) * 16);
#pragma unroll
                for (int mf = 0; mf < 2; ++mf)
#pragma unroll
                    for (int nf = 0; nf < 2; ++nf)
                        acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bv[nf]),
                                                                             __builtin_bit_cast(bf16x8, av[mf]), acc[mf][nf], 0, 0, 0);
            }
            mfma_result_guard<bf16_t>(reinterpret_cast<f32x4 (&)[4]>(acc));
            const int soff = cur.frame * HW1 * ST_N * 2;
#pragma unroll
            for (int mf = 0; mf < 2; ++mf) {
                const int gy = cur.oy0 + poy[mf], gx = cur.ox0 + pox[mf];
                const bool ok = gy < a.H1 && gx < a.W1;                     // (poy = 0x4000 beyond the tile)
                const int goff = ok ? (gy * a.W1 + gx) * ST_N * 2 + kg * 8 : OOB_OFF;
#pragma unroll
                for (int nf = 0; nf < 2; ++nf) {
                    const u32x2 o = lane_close_bf16(acc[mf][nf], b2v[nf], a.relu2, false, u32x2{0u, 0u});
                    __builtin_amdgcn_raw_buffer_store_b64(o, ry2, goff + (ok ? nf * 32 : 0), soff, 0);
                }
            }
        }
        cur = nxt;
    }
}

struct StemPlan { int nwg, lds; StemK k; };

// enc1b's descriptor behind enc1a's: the same images at enc1a's output extent, 32 -> 32 at stride 1
ColvoConvDesc stem_second(const ColvoConvDesc& d) {
    ColvoConvDesc e = d;
    e.Hi = d.Ho; e.Wi = d.Wo; e.Ho = d.Ho; e.Wo = d.Wo;
    e.C0 = ST_N; e.Cout = ST_N; e.stride = 1;
    return e;
}

// Reads the descriptor and the tuning table only.  true: the packing pass, enc1a (d) and enc1b (stem_second(d)) go as one k_stem launch;
// p.k then holds everything of the kernel argument but the pointers.
bool stem_plan(const ColvoConvDesc* d, StemPlan& p) {
    if (!d || !TUNE(stem_fused)) return false;
    if (d->dtype != COLVO_BF16 || d->ksize != 3 || d->stride != 2 || d->C0 != 8 || d->C1 != 0 || d->up0 || d->up1 || d->Cout != ST_N)
        return false;
    // the pair batch: image i and image B / 2 + i share PoseNet's pixel
    if (d->B < 2 || (d->B & 1) || d->B / 2 > TUNE(stem_max_pairs)) return false;
    if (d->Hi < 16 || d->Wi < 16 || (d->Hi & 1) || (d->Wi & 1) || d->Ho != d->Hi / 2 || d->Wo != d->Wi / 2) return false;
    // one buffer descriptor per tensor: every one of them below 1 GiB (the largest: the fp32 frames or a 32-channel map)
    if ((long long)d->B * d->Hi * d->Wi * 16 >= 0x40000000LL) return false;
    // the bit guarantee is against ONE reference per layer: the form the plain call would take
    const ColvoConvDesc e = stem_second(*d);
    const PlainForm fa = conv_plain_form(d, PASS_FWD, "colvo_stem_plan"), fb = conv_plain_form(&e, PASS_FWD, "colvo_stem_plan");
    // enc1a: k_conv3x3 with one chunk in flight or k_conv3x3_res<S2> over ONE-granule chunks -- k-groups 0, 1, 2 in ascending order,
    // granule 4 m + kg = tap 4 m + kg, granules 9..11 zero weights on tap 8's pixel
    if (!((fa.form == CONV_TILE && fa.nth == NT && fa.depth == 1) || fa.form == CONV_RES_S2) || fa.ng != 1) return false;
    // enc1b: k_conv3x3_res or k_conv3x3 (one chunk in flight) over its single 32-channel chunk -- k-group m = tap m, ascending
    if (!(fb.form == CONV_RES || (fb.form == CONV_TILE && fb.nth == NT && fb.depth == 1)) || fb.ng != 4) return false;
    StemK& k = p.k;
    k = StemK{};
    k.Bh = d->B / 2; k.H = d->Hi; k.W = d->Wi; k.H1 = d->Ho; k.W1 = d->Wo;
    k.relu1 = d->relu; k.relu2 = e.relu;
    // enc1b's own tile: at most 128 pixels, LDS rows padded against the bank conflicts of its fragment reads (pick_tile)
    const Tile t = pick_tile(k.H1, k.W1, 1, false, 128, true, 3);
    if (t.toh < 1 || t.tow < 2) return false;
    k.toh = t.toh; k.tow = t.tow;
    k.ewp = std::max(t.pwp, t.tow + 2);
    const int PH = 2 * t.toh + 5, PW = 2 * t.tow + 5;
    if (PH * PW > ST_PPT * ST_NT) return false;                                   // (what the register prefetch holds)
    k.tiles_x = (k.W1 + t.tow - 1) / t.tow; k.tiles_y = (k.H1 + t.toh - 1) / t.toh;
    const long long tpi = (long long)k.tiles_x * k.tiles_y, nitems = tpi * k.Bh;
    if (nitems >= 0x40000000LL) return false;
    k.nitems = (int)nitems;
    k.m_pw = mdiv_magic(PW); k.m_ew = mdiv_magic(t.tow + 2); k.m_tow = mdiv_magic(t.tow);
    p.lds = ST_N * (ST_W1ROW + ST_W2ROW) + ((PH * PW * ST_PIXI + 15) & ~15) + (t.toh + 2) * k.ewp * ST_PIXA;
    if (p.lds > 160 * 1024) return false;
    // every resident slot takes a workgroup: workgroups are dealt round-robin over the CUs and so are their pair tiles, which keeps the
    // CUs' shares within one pair tile of each other (fewer workgroups with whole rounds each leave some CUs one workgroup, others two)
    p.nwg = (int)std::min(nitems, std::max(1LL, (long long)TUNE(stem_max_wgs)));
    return true;
}

}  // namespace

// CMD_PACK_STEM_POSE with enc1a's weights in p[3] (program.hip): p = frames, stem, pose_in, w1, b1, y1, w2, b2, y2; i = B2, H, W; desc:
// enc1a's.  A shape the planner does not select is an error: the caller asks colvo_stem_plan first.  Counts no form.
int stem_fused(const ColvoCmd& c, hipStream_t s) {
    const ColvoConvDesc* d = &c.desc;
    for (int k : {0, 1, 2, 3, 5, 6, 8}) COLVO_CHECK_ARG(c.p[k], "colvo_pack_stem_pose (stem form): null pointer argument (slot %d)", k);
    StemPlan p{};
    COLVO_CHECK_ARG(stem_plan(d, p), "colvo_pack_stem_pose: the fused stem is not selected for this descriptor "
                                     "(colvo_stem_plan answers 0): issue the packing pass and the two layers one by one");
    COLVO_CHECK_ARG(c.i[0] == d->B && c.i[1] == d->Hi && c.i[2] == d->Wi,
                    "colvo_pack_stem_pose (stem form): %d frames of %d x %d against a descriptor of %d images of %d x %d", c.i[0], c.i[1],
                    c.i[2], d->B, d->Hi, d->Wi);
    for (int k : {0, 1, 2, 3, 5, 6, 8})
        COLVO_CHECK_ARG(aligned16(c.p[k]), "colvo_pack_stem_pose (stem form): slot %d is not 16-byte aligned", k);
    p.k.frames = (const float*)c.p[0]; p.k.stem = (char*)c.p[1]; p.k.pose_in = (char*)c.p[2];
    p.k.w1 = (const char*)c.p[3]; p.k.b1 = (const float*)c.p[4]; p.k.y1 = (char*)c.p[5];
    p.k.w2 = (const char*)c.p[6]; p.k.b2 = (const float*)c.p[7]; p.k.y2 = (char*)c.p[8];
    return launch_resident<k_stem>((unsigned)p.nwg, ST_NT, p.lds, s, "colvo_pack_stem_pose (stem form)", "k_stem", p.k);
}

}  // namespace colvo

using namespace colvo;

extern "C" int colvo_stem_plan(const ColvoConvDesc* d, int32_t* out) {
    StemPlan p{};
    if (!stem_plan(d, p)) return 0;
    if (out) { out[0] = p.nwg; out[1] = p.k.toh; out[2] = p.k.tow; out[3] = p.lds; }
    return 1;
}
