// wgrad_rt.hip -- a1/a2 of SURVEY.md §8: a second decomposition of the weight / bias gradient of the 3x3 conv blocks (round 6,
// VERDICT r5 item 1).  Parity-green, level with k_wgrad3x3 alone, a LOSS in the training step: OFF by default (tuning.h wgrad_rt),
// kept with its tests and measurements (profiles/r6_wgrad_rt.md) -- the numbers say where the weight gradient's time really goes.
//
// Concept: /root/reference/README.md:5,7 (the DCDP depth and pose networks); results specified by oracle/colvo_spec.py (autograd of
// F.conv2d k=3 pad=1).  Same operands, same output layout ([Cout][9][Ctot] fp32, added to dw / db) and same ways out (fp32 atomics,
// per-split slabs, sole-writer read-modify-write, plain stores into a clean arena) as k_wgrad3x3 (wgrad.hip); bf16, stride 1.
//
// What it changes against k_wgrad3x3 (whose four waves share the 9 x 32 (tap, ci) columns of one chunk: 2 x 5 accumulators of 16 x 16
// per wave, 14 transposed LDS reads per 10 short MFMAs, every wave re-reading the dY fragments, staging through ~40 registers and
// two barriers per 128-pixel tile at one wave per SIMD -- MFMA pipe 7-14 % busy, profiles/r5_conv_pmc_b64_final.json):
//   * a CONSUMER wave (waves 0-3, one per SIMD) owns a whole 32 (co) x 32 (ci) x 9 (taps) block of dw: nine v_mfma_f32_32x32x16_bf16
//     accumulators (144 registers), A = dY (rows = co), B = x (columns = ci), K = 16 pixels.  Per K-step it reads ONE dY fragment and
//     the nine shifted x fragments (20 ds_read_b64_tr_b16) for nine 32-cycle MFMAs -- 2.2 reads per MFMA gap, no fragment read
//     twice -- as one software pipeline over (step, tap) with the fragment four MFMAs ahead in flight; the four consumers split K
//     (K-steps w, w + 4, ... of every tile, rotated from tile to tile) and meet in LDS at the very end (36 chunks x 4 waves x 1 KiB;
//     all eight waves then sum and flush), so a CU ends with ONE 36 KB slab of atomics;
//   * the LOADER waves (4-7, the consumers' SIMD partners) do nothing but stage: per tile each loads its share of the 1 KiB pieces
//     (16 pixels x 32 channels) into registers -- where a consumer holds accumulators -- one tile ahead, and stores them into the other
//     of two LDS buffers while the consumers run MFMAs: one barrier per tile, no staging instruction in a consumer;
//   * the LDS images are plain [pixel][32 channels] rows of 64 bytes: four consecutive pixels of a transposed read cover all 64
//     banks once (the patch row pitch is congruent to the tile width modulo 4: zero conflict cycles in the counters);
//   * a K-step is ANY 16 consecutive tile pixels (row-major inside the tile, image after image for maps smaller than a tile), so
//     8x10 ... 256x320 maps all run at full K efficiency; the bias gradient rides on the dY fragments (v_dot2c_f32_bf16).
// Up-sampled sources are read through (y >> 1, x >> 1) by the loaders' address arithmetic.
//
// What the measurements say (MI355X, 64 frames of 256x320, gpurun_out/r6a ... r6j; profiles/r6_wgrad_rt.md):
//   * first build -- all eight waves both staging (LDS-DMA, `buffer_load ... lds`) and computing: 5600 cycles per 320-pixel tile for
//     1440 of MFMA.  A wave's LDS-DMA instructions go ONE AT A TIME on this hardware: ~250 cycles each even from a cache-hot line,
//     300-380 under load, whatever the access pattern and with or without the M0 save / restore -- four loader waves feed a CU
//     13 B/clk.  (Inline asm; hipcc's builtin drains vmcnt in front of every later ds_read.)
//   * second build -- loader / consumer roles, LDS-DMA ring of three buffers: consumers 2350 cycles per tile (470 per K-step; 790
//     before the K-step address table), loaders 3600: the consumers wait for the loaders.
//   * this build -- plain loads into the loaders' registers: the loads issue back to back (after three listings of hipcc draining
//     vmcnt between them) and a tile's pieces still take 3000-4000 cycles to arrive: with every CU streaming, a CU gets ~12 B/clk
//     out of L2 (75 % hit rate) -- about 8-9 KB in flight per CU at the loaded latency, ~7 TB/s over the chip.  THAT bounds the
//     weight gradient of the mid layers, not LDS reads, MFMA issue or occupancy: bytes per CU go as (a + b) / (a b) for an a x b
//     (co, ci) block per CU and the atomics (1.3 TB/s chip-wide) as a b, and k_wgrad3x3's 64 x 32 block with 256-1024 workgroups
//     already sits where the two meet.  A 32 x 32 block moves 1.33 x its bytes for half its atomics.
//   * alone, over the DepthNet stack: 1287 us against 1290 (64 frames), 533 against 502 (16 frames); enc4b / enc5b / iconv5 / iconv2
//     -10...17 %, enc2b / enc3b / iconv3 / iconv4 +5...14 %.  In the step, enabled only where it wins alone: +2.6 % / +0.5 % / +0.2 % at
//     8 / 32 / 64 pairs -- one 512-thread workgroup with ~150 KB of LDS per CU leaves no room for the input-gradient chain's
//     workgroups that k_wgrad3x3 shares its CUs with.
#define COLVO_ACC_CONSTRAINT "+v"
#include "conv_common.h"

namespace colvo {
namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int WR_NT = 512, WR_WAVES = 8;
constexpr int WR_CONS = 4, WR_LOAD = 4;                       // consumer waves (0..3: accumulators, MFMAs) / loader waves (4..7: LDS-DMA)
constexpr int WR_MAXY = 10, WR_MAXX = 13;                     // dY / patch pieces per loader and tile (compile-time bounds): 40 + 52 KiB
constexpr int WR_AHEAD = 4;                                   // x fragments requested this many MFMAs ahead of their use
constexpr int WR_EX_CHUNKS = 36;                              // accumulator chunks (4 registers x 64 lanes = 1 KiB) of a consumer
constexpr int WR_EX_BYTES = WR_EX_CHUNKS * WR_CONS * 1024;    // 147456
constexpr int WR_DB_BYTES = WR_NT * 8;                        // bias-gradient fold
constexpr int WR_LDS_MAX = 160 * 1024;
constexpr int WR_TAB_BYTES = 4096;                            // K-step address table: 4 bytes per tile pixel (<= 1024)

struct WgradRtK {
    const char* dy;           // [B][Ho][Wo][Cout] bf16
    const char* src[2];       // stored sources, bf16 NHWC
    WgradSink out;            // dw [Cout][9][Ctot] / db, as for k_wgrad3x3
    int B, Ho, Wo, Cout;
    int C[2], Hs[2], Ws[2], sh[2];     // per source: channels, stored extent, 1 = stored at half size (nearest-2x up-sampled)
    int nci0, nci, nco;                // 32-channel ci tiles of source 0 / of both sources, co tiles
    int ni, toh, tow;                  // tile = ni whole images (ni > 1: toh x tow is the image) or toh x tow pixels of one image
    int npix1, npix, ksteps;           // toh * tow, ni * npix1, ceil(npix / 16)
    int pwl, pimg, xinstr;             // LDS patch row pitch / image pitch in pixels, DMA instructions of the patch
    int tiles_x, tiles_y, ntiles, tiles_per_split, nsplit;
    uint32_t m_tow, m_npix1, m_pwl, m_pimg;
    int xcd;
    int buf_bytes;                     // one staging buffer: (ksteps + xinstr) KiB
    int tab_off;                       // LDS offset of the K-step address table (behind the two staging buffers)
#ifdef COLVO_WTRACE
    long long* trace;                  // developer build (tools/wtrace_wgrad.sh): [workgroup][wave][16] shader-clock sums per phase
#endif
};

#ifndef COLVO_RT_VARIANT
#define COLVO_RT_VARIANT 0          // developer ablations (tools/wtrace_wgrad.sh): 2 = no staging in the tile loop, 4 = no MFMA phase,
#endif                              // 8 = no bias sums
__device__ __forceinline__ i32x4 make_rsrc(const void* p, long long bytes) {
    const unsigned long long a = (unsigned long long)p;
    i32x4 rs;
    rs.x = __builtin_amdgcn_readfirstlane((int)(a & 0xffffffffu));
    rs.y = __builtin_amdgcn_readfirstlane((int)((a >> 32) & 0xffff));
    rs.z = __builtin_amdgcn_readfirstlane((int)(bytes < 0x7fffffffLL ? bytes : 0x7fffffffLL));
    rs.w = __builtin_amdgcn_readfirstlane(0x00020000);
    return rs;
}
// a * b + c for 0 <= a, b < 2^24 (v_mad_u32_u24: full rate, where the 32-bit multiply takes four passes)
// (asm: given __umul24 of a value it knows to be small and a kernel argument it knows nothing about, hipcc falls back to v_mul_lo_u32)
__device__ __forceinline__ int mad24(int a, int b, int c) {
    int d;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
// i / d for 0 <= i < 1024, 2 <= d < 1024 with m = ceil(2^20 / d): one full-rate 24-bit multiply and a shift (every index divided in this
// kernel counts pixels of ONE tile or patch; the 32-bit mul_hi of conv_common.h mdiv takes four passes)
__device__ __forceinline__ int mdiv20(int i, uint32_t m) { return (int)(__umul24((unsigned)i, m) >> 20); }
inline uint32_t mdiv20_magic(int d) { return (uint32_t)(((1u << 20) + (uint32_t)d - 1) / (uint32_t)d); }
__device__ __forceinline__ s16x4 trd(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}

// hand-over of the nine 32x32 accumulators to the VALU (see conv_common.h mfma_result_guard): one in-place terminator each
__device__ __forceinline__ void guard9(f32x16 (&acc)[9]) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    asm volatile("s_nop 1\n\t"
                 "v_mfma_f32_32x32x16_bf16 %0, %9, %9, %0\n\t"
                 "v_mfma_f32_32x32x16_bf16 %1, %9, %9, %1\n\t"
                 "v_mfma_f32_32x32x16_bf16 %2, %9, %9, %2\n\t"
                 "v_mfma_f32_32x32x16_bf16 %3, %9, %9, %3\n\t"
                 "v_mfma_f32_32x32x16_bf16 %4, %9, %9, %4\n\t"
                 "v_mfma_f32_32x32x16_bf16 %5, %9, %9, %5\n\t"
                 "v_mfma_f32_32x32x16_bf16 %6, %9, %9, %6\n\t"
                 "v_mfma_f32_32x32x16_bf16 %7, %9, %9, %7\n\t"
                 "v_mfma_f32_32x32x16_bf16 %8, %9, %9, %8\n\t"
                 "s_nop 15\n\ts_nop 7"
                 : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]), "+v"(acc[7]),
                   "+v"(acc[8])
                 : "v"(z));
}

#ifdef COLVO_WTRACE
#define WT(x) x = (long long)clock64()
#else
#define WT(x) do {} while (0)
#endif

__global__ __launch_bounds__(WR_NT) void k_wgrad_rt(const WgradRtK a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef COLVO_WTRACE
    long long wt0, wt1, wt2, wt3, wt4, wt_start, wt_loop0, wt_loop1, wt_ex, wt_end;
    long long ws_vm = 0, ws_bar = 0, ws_issue = 0, ws_comp = 0;
    WT(wt_start);
#endif
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Roles: waves 0-3 (one per SIMD) are the CONSUMERS -- they own the accumulators and split K four ways --, waves 4-7 their SIMD
    // partners the LOADERS: all they do in the tile loop is issue LDS-DMA.  (First build, every wave both: a DMA instruction with its
    // address arithmetic cost the issuing wave ~350 cycles, six of them per wave and tile more than the wave's MFMA work, and with
    // all eight waves in that code at the same time the matrix pipes idled: 5600 cycles per tile for 1440 of MFMA, gpurun_out/r6c.)
    const bool loader = wave >= WR_CONS;
    const int lw = wave - WR_CONS;                         // loader index 0..3
    const int h = lane >> 5, c16 = (lane >> 4) & 1, q = (lane & 15) >> 2, pp = lane & 3;
    // 1-D grid, XCD-contiguous: logical id = (pixel-range split, ci tile, co tile), co tile fastest
    const int lid = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x, a.xcd));
    const int per_split = a.nco * a.nci;
    const int bsplit = lid / per_split, brem = lid - bsplit * per_split;
    const int bci = brem / a.nco, bco = brem - bci * a.nco;
    const int co0 = bco * 32;
    const int s = bci < a.nci0 ? 0 : 1;
    const int c0 = (s ? bci - a.nci0 : bci) * 32;
    const int wc0 = (s ? a.C[0] : 0) + c0;
    const int Cs = s ? a.C[1] : a.C[0], Hs = s ? a.Hs[1] : a.Hs[0], Ws = s ? a.Ws[1] : a.Ws[0], sh = s ? a.sh[1] : a.sh[0];
    const int Hi = a.Ho, Wi = a.Wo;                        // stride 1: the virtual input has the output's extent

    const i32x4 rdy = make_rsrc(a.dy, (long long)a.B * a.Ho * a.Wo * a.Cout * 2);
    const i32x4 rx = make_rsrc(s ? a.src[1] : a.src[0], (long long)a.B * Hs * Ws * Cs * 2);

    const int t_begin = bsplit * a.tiles_per_split;
    const int t_end = min(a.ntiles, t_begin + a.tiles_per_split);
    f32x16 acc[9];
    float dbacc = 0.0f;                                    // consumer lane (co = lane & 31, K half h): sum of its dY fragment elements
    // bias gradient: by the consumers of the workgroups of ci tile 0, from the dY fragments they hold anyway (v_dot2c_f32_bf16 with
    // a pair of ones: four instructions per K-step)
    const bool db_on = a.out.bias && bci == 0 && !(COLVO_RT_VARIANT & 8);

    // ---- ring of a.nbuf staging buffers: tile t is computed from buffer (t - t_begin) mod nbuf while the DMA of the next nbuf - 1 tiles
    // is in flight.  Every loader issues the same number of DMA instructions per tile, in tile order, so "my share of tile t has
    // landed" is a counted vmcnt; the workgroup barrier behind it makes that everyone's share, and says that tile t - 1's buffer is
    // free.  The two roles are two code paths with the same barrier sequence (their registers overlap: the loaders' instruction
    // table against the consumers' accumulators and fragments).
    {
        uint32_t* tabw = reinterpret_cast<uint32_t*>(smem + a.tab_off);
        for (int k = tid; k < a.ksteps * 16; k += WR_NT) {
            int kk = k < a.npix ? k : 0;                   // beyond the tile: dY is zero there, any finite x will do
            int img = 0, r = kk;
            if (a.ni > 1) { img = mdiv20(kk, a.m_npix1); r = kk - (int)__umul24(img, a.npix1); }
            const int oy = mdiv20(r, a.m_tow), ox = r - (int)__umul24(oy, a.tow);
            tabw[k] = (uint32_t)(img * a.pimg + oy * a.pwl + ox) * 64u;     // LDS patch pixel of tile pixel k at tap (0, 0), in bytes
        }
    }
    WT(wt_loop0);
    if (loader) {
        // ---- a loader's pieces (1 KiB = 16 pixels x 32 channels each): the dY pieces lw, lw + 4, ... < ksteps (piece id = K-step id:
        // tile pixels 16 id .. 16 id + 15) and the patch pieces lw, lw + 4, ... < xinstr (patch pixels 16 j .. 16 j + 15).
        // Lane = (pixel id >> 2, granule id & 3); LDS image: dY piece id at buffer + id KiB, patch piece j at buffer + (ksteps + j) KiB.
        // Two separate unrolled sequences: with the kind decided per piece inside one sequence hipcc either drained vmcnt in front
        // of every load (two branches, "the other one might have a load pending on these registers") or spent ~30 scalar selects
        // per load (third and fourth listing).
        const int gl = lane & 3, pl = lane >> 2;
        int pky[WR_MAXY], pkx[WR_MAXX];                    // (image << 24 | y << 12 | x) inside the tile / the patch; -1: never valid
#pragma unroll
        for (int n = 0; n < WR_MAXY; ++n) {
            const int id = lw + WR_LOAD * n, k = 16 * id + pl;
            int img = 0, r = k < 1024 ? k : 0;
            if (a.ni > 1) { img = mdiv20(r, a.m_npix1); r = r - (int)__umul24(img, a.npix1); }
            const int oy = mdiv20(r, a.m_tow), ox = r - (int)__umul24(oy, a.tow);
            pky[n] = (id < a.ksteps && k < a.npix && co0 + 8 * gl < a.Cout) ? (img << 24) | (oy << 12) | ox : -1;
        }
#pragma unroll
        for (int n = 0; n < WR_MAXX; ++n) {
            const int j = lw + WR_LOAD * n, p0 = 16 * j + pl, pc = p0 < 1024 ? p0 : 0;
            const int img = mdiv20(pc, a.m_pimg), r = pc - (int)__umul24(img, a.pimg);
            const int py = mdiv20(r, a.m_pwl), px = r - (int)__umul24(py, a.pwl);
            pkx[n] = (j < a.xinstr && img < a.ni && py < a.toh + 2 && px < a.tow + 2 && c0 + 8 * gl < Cs) ? (img << 24) | (py << 12) | px : -1;
        }
        const int ndy = lw < a.ksteps ? (a.ksteps - lw + WR_LOAD - 1) / WR_LOAD : 0;      // this loader's piece counts
        const int nxp = lw < a.xinstr ? (a.xinstr - lw + WR_LOAD - 1) / WR_LOAD : 0;
        struct TileC { int bg, ty, tx; };                  // image group, tile row, tile column (wave-uniform)
        auto tile_next = [&](TileC& c) {
            if (++c.tx == a.tiles_x) { c.tx = 0; if (++c.ty == a.tiles_y) { c.ty = 0; ++c.bg; } }
        };
        // One tile's loads into this loader's staging registers (consumers hold accumulators where a loader holds these).  Per load:
        // unpack (image, y, x), test them against what is left of the image / batch, and three 24-bit multiply-adds for the byte
        // offset; the tile's origin rides in the scalar offset.  (Round 6's first two builds staged by LDS-DMA: on this hardware a
        // wave's `buffer_load ... lds` instructions go one at a time -- ~250 cycles each even from a cache-hot line, gpurun_out/r6g --
        // so four loader waves fed a CU 13 B/clk and the consumers waited; plain loads queue up.)
        const int gch_dy = (co0 + 8 * gl) * 2, gch_x = (c0 + 8 * gl) * 2;
        const __amdgpu_buffer_rsrc_t bdy = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, rdy.z, 0x00020000);
        const __amdgpu_buffer_rsrc_t bx = __builtin_amdgcn_make_buffer_rsrc((void*)(s ? a.src[1] : a.src[0]), 0, rx.z, 0x00020000);
        u32x4 sty[WR_MAXY], stx[WR_MAXX];
        auto load_tile = [&](const TileC& c) {
            // (readfirstlane: the tile coordinates are wave-uniform but hipcc keeps them in VGPRs, and a scalar offset it cannot prove
            //  uniform gets a waterfall loop around every load: cdna_hip_programming.md T20)
            const int b0 = __builtin_amdgcn_readfirstlane(c.bg * a.ni), oy0 = __builtin_amdgcn_readfirstlane(c.ty * a.toh),
                      ox0 = __builtin_amdgcn_readfirstlane(c.tx * a.tow);
            const int soff_dy = ((b0 * a.Ho + oy0) * a.Wo + ox0) * a.Cout * 2;
            const int soff_x = b0 * Hs * Ws * Cs * 2;
            const int ry = a.Ho - oy0, rx_ = a.Wo - ox0, rb = a.B - b0;  // rows / columns / images left from the tile's origin on
            const int C2y = a.Cout * 2, C2x = Cs * 2;
            // every offset first, then the loads back to back: with address arithmetic between the loads hipcc put it into the registers
            // the NEXT load returns to and drained vmcnt in front of it ("a load might still be pending there"): fifth listing
            int vy_[WR_MAXY], vx_[WR_MAXX];
#pragma unroll
            for (int n = 0; n < WR_MAXY; ++n) {
                if (n >= ndy) break;
                const int pk = pky[n];
                const int i2 = pk >> 24, y12 = (pk >> 12) & 0xfff, x12 = pk & 0xfff;
                const bool ok = pk >= 0 && y12 < ry && x12 < rx_ && i2 < rb;
                const int off = mad24(mad24(mad24(i2, a.Ho, y12), a.Wo, x12), C2y, gch_dy);      // relative to the origin
                vy_[n] = ok ? off : OOB_OFF;
            }
#pragma unroll
            for (int n = 0; n < WR_MAXX; ++n) {
                if (n >= nxp) break;
                const int pk = pkx[n];
                const int i2 = pk >> 24, y12 = (pk >> 12) & 0xfff, x12 = pk & 0xfff;
                const int vy = oy0 - 1 + y12, vx = ox0 - 1 + x12;
                const bool ok = pk >= 0 && (unsigned)vy < (unsigned)Hi && (unsigned)vx < (unsigned)Wi && i2 < rb;
                const int off = mad24(mad24(mad24(i2, Hs, vy >> sh), Ws, vx >> sh), C2x, gch_x);
                vx_[n] = ok ? off : OOB_OFF;
            }
#pragma unroll
            for (int n = 0; n < WR_MAXY; ++n) {
                if (n >= ndy) break;
                sty[n] = bld16(bdy, vy_[n], soff_dy);
            }
#pragma unroll
            for (int n = 0; n < WR_MAXX; ++n) {
                if (n >= nxp) break;
                stx[n] = bld16(bx, vx_[n], soff_x);
            }
        };
        auto store_tile = [&](int buf) {                   // registers -> LDS image, lane-linear 16-byte stores
            char* dst = smem + buf * a.buf_bytes + lw * 1024 + lane * 16;
#pragma unroll
            for (int n = 0; n < WR_MAXY; ++n) {
                if (n >= ndy) break;
                st16(dst + n * (WR_LOAD * 1024), sty[n]);
            }
            dst += a.ksteps * 1024;
#pragma unroll
            for (int n = 0; n < WR_MAXX; ++n) {
                if (n >= nxp) break;
                st16(dst + n * (WR_LOAD * 1024), stx[n]);
            }
        };
        TileC nxt;                                         // the next tile to request
        {
            const int tpi = a.tiles_x * a.tiles_y;
            nxt.bg = t_begin / tpi;
            const int rem = t_begin - nxt.bg * tpi;
            nxt.ty = rem / a.tiles_x; nxt.tx = rem - nxt.ty * a.tiles_x;
        }
        // tile t_begin goes into buffer 0 before the loop; inside iteration t the loaders store tile t + 1 (requested one iteration
        // earlier, in flight under a whole tile of MFMAs) into the other buffer and request tile t + 2
        int t_issue = t_begin;
        if (t_issue < t_end) {
            load_tile(nxt); tile_next(nxt); ++t_issue;
            store_tile(0);
            if (t_issue < t_end) { load_tile(nxt); tile_next(nxt); ++t_issue; }
        }
        int obuf = 1;                                      // buffer the next store goes to
        for (int t = t_begin; t < t_end; ++t) {
            WT(wt1);
            __syncthreads();                               // tile t is complete in its buffer; the consumers are done with the other one
            WT(wt2);
            if (t + 1 < t_end && !(COLVO_RT_VARIANT & 2)) {
                store_tile(obuf);                          // (waits for tile t + 1's loads)
                WT(wt0);
                if (t_issue < t_end) { load_tile(nxt); tile_next(nxt); ++t_issue; }
            } else WT(wt0);
            obuf ^= 1;
#ifdef COLVO_WTRACE
            WT(wt3);
            ws_bar += wt2 - wt1; ws_vm += wt0 - wt2; ws_issue += wt3 - wt0;
#endif
        }
    } else {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        // transposed-read lane constants: lane (h, c16, q, pp) of read j supplies the address of pixel 16 ks + 8 h + 4 j + q, channels
        // 16 c16 + 4 pp .. + 3, and receives channel (lane & 31) of the four pixels q = 0..3 (cdna_hip_programming.md T10)
        const int lane_dy = (8 * h + q) * 64 + 32 * c16 + 8 * pp;
        const int lane_x = 32 * c16 + 8 * pp;
        const int kl0 = 8 * h + q;
        const int rowb = a.pwl * 64;
        // Table of xidx * 64 for every tile pixel, behind the ring (loaders and consumers fill it; the tile loop's first barrier
        // publishes it): a K-step then costs two 4-byte LDS reads instead of ~25 VALU instructions of index arithmetic, which one
        // wave per SIMD cannot hide (second listing: 790 cycles per K-step for 288 of MFMA).
        const char* tab = smem + a.tab_off;
        const char* tabl = tab + kl0 * 4;                  // this lane's column of the table: entries 16 ks + kl0 and + 4
        int buf = 0, rot = 0;                              // buffer of tile t, (tiles walked * ksteps) mod 4
        for (int t = t_begin; t < t_end; ++t) {
            WT(wt1);
            __syncthreads();
            WT(wt2);
            const char* bufc = smem + buf * a.buf_bytes;
            const char* bufx = bufc + a.ksteps * 1024 + lane_x;
            // This consumer's K-steps ks, ks + 4, ... as ONE software pipeline over (step, tap): nine x-fragment registers, one per
            // tap; the fragment of the tap WR_AHEAD MFMAs ahead -- of this step or of the next one -- is requested before each MFMA,
            // the next step's dY fragment with its first tap, the next step's table entries at this step's first tap.  No branch
            // inside a step: behind the last step the "next" one is the step itself (reads nobody uses).  Pinned with sched_barrier:
            // left alone hipcc sinks every read to just in front of its MFMA (the first listing of this kernel).
            int ks = (wave - rot) & (WR_CONS - 1);
            bool have = ks < a.ksteps && !(COLVO_RT_VARIANT & 4);
            const char *pdy = bufc, *px0 = bufx, *px1 = bufx;
            s16x4 a_lo, a_hi, n_lo, n_hi, b_lo[9], b_hi[9];
            auto read_b = [&](const char* x0_, const char* x1_, int tap) {
                const int off = (tap / 3) * rowb + (tap % 3) * 64;
                b_lo[tap] = trd(x0_ + off); b_hi[tap] = trd(x1_ + off);
            };
            if (have) {
                const uint32_t t0 = *reinterpret_cast<const uint32_t*>(tabl + ks * 64), t1 = *reinterpret_cast<const uint32_t*>(tabl + ks * 64 + 16);
                pdy = bufc + ks * 1024 + lane_dy;
                px0 = bufx + t0; px1 = bufx + t1;
                a_lo = trd(pdy); a_hi = trd(pdy + 256);
#pragma unroll
                for (int tap = 0; tap < WR_AHEAD; ++tap) read_b(px0, px1, tap);
            }
            while (have) {
                const int ksn = ks + WR_CONS;
                const bool has_next = ksn < a.ksteps;
                const int kse = has_next ? ksn : ks;
                const char *ndy = pdy, *nx0 = px0, *nx1 = px1;
                uint32_t t0 = 0, t1 = 0;
                const s16x8 af = {a_lo[0], a_lo[1], a_lo[2], a_lo[3], a_hi[0], a_hi[1], a_hi[2], a_hi[3]};
                if (db_on) {
                    // (the pairs are picked out of a bf16 vector: a bit_cast of a u32 ELEMENT to a bf16 pair makes hipcc 7.2 feed the
                    //  first dword to both instructions -- seen in this kernel's first listing, reproduced in isolation)
                    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_;
                    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_;
                    const bf16x4_ l4 = __builtin_bit_cast(bf16x4_, a_lo), h4 = __builtin_bit_cast(bf16x4_, a_hi);
                    const bf16x2_ ones = {(__bf16)1.0f, (__bf16)1.0f};
                    dbacc = __builtin_amdgcn_fdot2_f32_bf16(bf16x2_{l4[0], l4[1]}, ones, dbacc, false);
                    dbacc = __builtin_amdgcn_fdot2_f32_bf16(bf16x2_{l4[2], l4[3]}, ones, dbacc, false);
                    dbacc = __builtin_amdgcn_fdot2_f32_bf16(bf16x2_{h4[0], h4[1]}, ones, dbacc, false);
                    dbacc = __builtin_amdgcn_fdot2_f32_bf16(bf16x2_{h4[2], h4[3]}, ones, dbacc, false);
                }
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int tt = tap + WR_AHEAD;
                    if (tap == 0) {
                        t0 = *reinterpret_cast<const uint32_t*>(tabl + kse * 64); t1 = *reinterpret_cast<const uint32_t*>(tabl + kse * 64 + 16);
                    }
                    if (tt == 8) { ndy = bufc + kse * 1024 + lane_dy; nx0 = bufx + t0; nx1 = bufx + t1; }
                    if (tt < 9) read_b(px0, px1, tt);
                    else {
                        if (tt == 9) { n_lo = trd(ndy); n_hi = trd(ndy + 256); }
                        read_b(nx0, nx1, tt - 9);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    const s16x8 bf = {b_lo[tap][0], b_lo[tap][1], b_lo[tap][2], b_lo[tap][3], b_hi[tap][0], b_hi[tap][1], b_hi[tap][2], b_hi[tap][3]};
                    acc[tap] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af), __builtin_bit_cast(bf16x8, bf), acc[tap], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                a_lo = n_lo; a_hi = n_hi;
                pdy = ndy; px0 = nx0; px1 = nx1;
                ks = ksn; have = has_next;
            }
            rot = (rot + a.ksteps) & (WR_CONS - 1);
            buf ^= 1;
#ifdef COLVO_WTRACE
            WT(wt4);
            ws_bar += wt2 - wt1; ws_comp += wt4 - wt2;
#endif
        }
        guard9(acc);
    }
    WT(wt_loop1);

    // ---- the four K slices meet: every consumer stores its 36 accumulator chunks (chunk c = tap c >> 2, registers 4 (c & 3) .. + 3:
    // rows co = (c & 3) * 8 + 4 h + e, column ci = lane & 31), lane-major 16-byte stores; then wave w -- loaders too -- sums the four
    // copies of the chunks w, w + 8, ... in a fixed order and flushes them: one register = two 128-byte row segments of dw
    f32x4* sEx = reinterpret_cast<f32x4*>(smem);
    const size_t wsize = (size_t)a.Cout * 9 * a.out.Ctot;
    const int ci = lane & 31;
    const bool civ = c0 + ci < Cs;
    __syncthreads();                                       // the staging buffers are free
    if (!loader) {
#pragma unroll
        for (int c = 0; c < WR_EX_CHUNKS; ++c) {
            const int tap = c >> 2, qd = c & 3;
            sEx[(c * WR_CONS + wave) * 64 + lane] = f32x4{acc[tap][4 * qd], acc[tap][4 * qd + 1], acc[tap][4 * qd + 2], acc[tap][4 * qd + 3]};
        }
    }
    __syncthreads();
    for (int c = wave; c < WR_EX_CHUNKS; c += WR_WAVES) {
        f32x4 v[WR_CONS];
#pragma unroll
        for (int w = 0; w < WR_CONS; ++w) v[w] = sEx[(c * WR_CONS + w) * 64 + lane];
        f32x4 t = v[0];
#pragma unroll
        for (int w = 1; w < WR_CONS; ++w) t += v[w];
        const int tap = c >> 2, qd = c & 3;
        const int corow = co0 + 8 * qd + 4 * h;
        const size_t e0 = ((size_t)corow * 9 + tap) * a.out.Ctot + wc0 + ci;
        const size_t erow = (size_t)9 * a.out.Ctot;
        const int nrow = civ ? min(4, a.Cout - corow) : 0;                 // rows of this lane inside the tensor (<= 0: none)
        wgrad_put_rows(a.out, bsplit, wsize, e0, erow, nrow, t);
    }
    WT(wt_ex);
    if (a.out.bias && bci == 0) {                          // (wave-uniform: bci is the workgroup's)
        __syncthreads();
        float* sdb = reinterpret_cast<float*>(smem);
        if (!loader) sdb[tid] = dbacc;                     // [consumer][K half][co]
        __syncthreads();
        if (tid < 32 && co0 + tid < a.Cout) {
            float t = 0.0f;
#pragma unroll
            for (int j = 0; j < 2 * WR_CONS; ++j) t += sdb[j * 32 + tid];
            wgrad_put_bias(a.out, bsplit, a.Cout, co0, tid, t);
        }
    }
#ifdef COLVO_WTRACE
    if (a.trace) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the flush has left the wave
        WT(wt_end);
        if (lane == 0) {
            long long* r = a.trace + ((size_t)blockIdx.x * WR_WAVES + wave) * 16;
            r[0] = wt_loop0 - wt_start; r[1] = ws_vm; r[2] = ws_bar; r[3] = ws_issue; r[4] = ws_comp; r[5] = 0;
            r[6] = wt_ex - wt_loop1; r[7] = wt_end - wt_ex; r[8] = wt_end - wt_start; r[9] = t_end - t_begin; r[10] = wt_start;
        }
    }
#endif
}
#undef WT

struct RtTile { int ni, toh, tow, pwl, pimg, ksteps, xinstr; double cost; };

// LDS pitches of the patch: row pitch = tow (mod 4) and image pitch = toh * tow (mod 4), so that the LDS pixel index of tile pixel k is
// congruent to k modulo 4 -- the four consecutive pixels of a transposed read then sit on four different 64-byte bank quarters
inline void rt_pitches(int ni, int toh, int tow, int& pwl, int& pimg) {
    pwl = tow + 2;
    while ((pwl - tow) % 4) ++pwl;
    pimg = (toh + 2) * pwl;
    if (ni > 1) while ((pimg - toh * tow) % 4) ++pimg;
}

inline bool rt_tile_fits(const RtTile& t) {
    const int instr = t.ksteps + t.xinstr;
    return t.ksteps <= WR_LOAD * WR_MAXY && t.xinstr <= WR_LOAD * WR_MAXX && 2 * instr * 1024 <= WR_LDS_MAX - WR_TAB_BYTES && t.toh + 2 < 4096 && t.tow + 2 < 4096 && t.ni < 128 &&
           t.ksteps * 16 <= 1024 && t.xinstr * 16 <= 1024 && t.tow + 2 < 1000 && t.pimg < 1024 && t.toh * t.tow < 1024;
}

// tile = the region that minimises  tiles x (MFMA cycles of its K-steps + DMA issue + per-tile fixed cost)
inline RtTile rt_pick_tile(int B, int Ho, int Wo) {
    const int max_px = std::max(16, (int)TUNE(wgrad_rt_max_px));
    struct Key { int B, Ho, Wo, max_px; };
    static std::vector<std::pair<Key, RtTile>> cache;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    for (const auto& e : cache)
        if (e.first.B == B && e.first.Ho == Ho && e.first.Wo == Wo && e.first.max_px == max_px) return e.second;
    RtTile best{}; best.cost = 1e300;
    auto consider = [&](int ni, int toh, int tow) {
        RtTile t{}; t.ni = ni; t.toh = toh; t.tow = tow;
        rt_pitches(ni, toh, tow, t.pwl, t.pimg);
        t.ksteps = (ni * toh * tow + 15) / 16;
        t.xinstr = (ni * t.pimg + 15) / 16;
        if (!rt_tile_fits(t)) return;
        const double tiles = ni > 1 ? (double)((B + ni - 1) / ni) : (double)B * ((Ho + toh - 1) / toh) * ((Wo + tow - 1) / tow);
        // per tile: the consumers' K-steps (nine 32-cycle MFMAs each, one wave per SIMD, plus the pipeline's start and a barrier) or,
        // if longer, the loaders' share (address arithmetic, load, 16-byte LDS store per piece)
        t.cost = tiles * std::max(330.0 * ((t.ksteps + 3) / 4) + 400.0, 80.0 * ((t.ksteps + t.xinstr + 3) / 4) + 300.0);
        if (t.cost < best.cost) best = t;
    };
    for (int tow = 2; tow <= std::min(Wo, 160); ++tow) {
        if (tow != Wo && (tow & 3)) continue;              // (multiples of 4, or the whole row)
        for (int toh = 1; toh <= Ho; ++toh) {
            if (toh * tow > max_px) break;
            consider(1, toh, tow);
        }
    }
    if (Ho * Wo <= max_px / 2)
        for (int ni = 2; ni <= std::min(B, 64); ++ni) {
            if (ni * Ho * Wo > max_px) break;
            consider(ni, Ho, Wo);
        }
    cache.push_back({Key{B, Ho, Wo, max_px}, best});
    return best;
}

}  // namespace

bool wgrad_rt_plan(const ColvoConvDesc* d, WgradRtPlan& p) {
    if (!TUNE(wgrad_rt) || d->dtype != COLVO_BF16 || d->stride != 1 || d->Wo < 2 || d->Ho < 1) return false;
    const int minc = (int)TUNE(wgrad_rt_min_c);
    if (d->Cout < minc || d->C0 < minc || (d->C1 > 0 && d->C1 < minc)) return false;
    if ((long long)d->B * d->Ho * d->Wo < TUNE(wgrad_rt_min_px)) return false;
    const RtTile t = rt_pick_tile(d->B, d->Ho, d->Wo);
    if (t.cost >= 1e299) return false;
    p.ni = t.ni; p.toh = t.toh; p.tow = t.tow; p.pwl = t.pwl; p.pimg = t.pimg; p.ksteps = t.ksteps; p.xinstr = t.xinstr;
    p.tiles_x = t.ni > 1 ? 1 : (d->Wo + t.tow - 1) / t.tow;
    p.tiles_y = t.ni > 1 ? 1 : (d->Ho + t.toh - 1) / t.toh;
    p.ntiles = (t.ni > 1 ? (d->B + t.ni - 1) / t.ni : d->B) * p.tiles_x * p.tiles_y;
    p.nci0 = (d->C0 + 31) / 32;
    p.nci = p.nci0 + (d->C1 + 31) / 32;
    p.nco = (d->Cout + 31) / 32;
    const int per_split = p.nci * p.nco;
    int nsplit = std::max(1, (int)TUNE(wgrad_rt_wgs) / per_split);
    if (nsplit > p.ntiles) nsplit = p.ntiles;
    p.tiles_per_split = (p.ntiles + nsplit - 1) / nsplit;
    p.nsplit = (p.ntiles + p.tiles_per_split - 1) / p.tiles_per_split;
    return true;
}

int wgrad_rt_launch(const WgradRtPlan& p, const ColvoConvDesc* d, const void* x0, const void* x1, const void* dy, const WgradSink& out,
                    hipStream_t s) {
    WgradRtK k{};
    k.dy = (const char*)dy; k.src[0] = (const char*)x0; k.src[1] = d->C1 ? (const char*)x1 : nullptr;
    k.out = out;
    k.B = d->B; k.Ho = d->Ho; k.Wo = d->Wo; k.Cout = d->Cout;
    k.C[0] = d->C0; k.C[1] = d->C1;
    k.sh[0] = d->up0 ? 1 : 0; k.sh[1] = d->up1 ? 1 : 0;
    k.Hs[0] = d->up0 ? d->Hi / 2 : d->Hi; k.Ws[0] = d->up0 ? d->Wi / 2 : d->Wi;
    k.Hs[1] = d->up1 ? d->Hi / 2 : d->Hi; k.Ws[1] = d->up1 ? d->Wi / 2 : d->Wi;
    k.nci0 = p.nci0; k.nci = p.nci; k.nco = p.nco;
    k.ni = p.ni; k.toh = p.toh; k.tow = p.tow; k.npix1 = p.toh * p.tow; k.npix = p.ni * k.npix1; k.ksteps = p.ksteps;
    k.pwl = p.pwl; k.pimg = p.pimg; k.xinstr = p.xinstr;
    k.tiles_x = p.tiles_x; k.tiles_y = p.tiles_y; k.ntiles = p.ntiles; k.tiles_per_split = p.tiles_per_split; k.nsplit = p.nsplit;
    k.m_tow = mdiv20_magic(p.tow); k.m_npix1 = mdiv20_magic(std::max(2, k.npix1)); k.m_pwl = mdiv20_magic(p.pwl); k.m_pimg = mdiv20_magic(p.pimg);
    k.xcd = (int)TUNE(xcd_remap);
    k.buf_bytes = (p.ksteps + p.xinstr) * 1024;
    k.tab_off = 2 * k.buf_bytes;
    COLVO_CHECK_ARG(p.ksteps <= WR_LOAD * WR_MAXY && p.xinstr <= WR_LOAD * WR_MAXX && p.tow >= 2, "wgrad_rt: bad tile plan");
    // always the whole exchange area: one workgroup per CU (eight waves at <= 256 registers fill its SIMDs two deep)
    const size_t lds = std::max<size_t>((size_t)2 * k.buf_bytes + WR_TAB_BYTES, (size_t)WR_EX_BYTES + WR_DB_BYTES);
    COLVO_CHECK_ARG(lds <= (size_t)WR_LDS_MAX, "wgrad_rt: %zu bytes of LDS", lds);
    if (int e = allow_dynamic_lds<k_wgrad_rt>(lds, WR_LDS_MAX, "wgrad_rt")) return e;
    const unsigned nwg = (unsigned)(p.nsplit * p.nci * p.nco);
#ifdef COLVO_WTRACE
    static long long* g_tr = nullptr;
    static int g_calls = 0;
    k.trace = nullptr;
    if (getenv("COLVO_WTRACE") && nwg <= 4096) {
        if (!g_tr) (void)hipMalloc(&g_tr, (size_t)4096 * WR_WAVES * 16 * sizeof(long long));
        (void)hipMemsetAsync(g_tr, 0, (size_t)nwg * WR_WAVES * 16 * sizeof(long long), s);
        k.trace = g_tr;
    }
#endif
    colvo::launch(k_wgrad_rt, dim3(nwg), dim3(WR_NT), (unsigned)lds, s, k);
    COLVO_CHECK_LAUNCH("k_wgrad_rt");
#ifdef COLVO_WTRACE
    if (k.trace && (++g_calls % atoi(getenv("COLVO_WTRACE"))) == 0) {
        (void)hipStreamSynchronize(s);
        std::vector<long long> h((size_t)nwg * WR_WAVES * 16);
        (void)hipMemcpy(h.data(), g_tr, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
        double m[2][16] = {{0}};                 // waves 0-3 | waves 4-7
        long long t0 = h[10], t1 = 0;
        for (unsigned i = 0; i < nwg * WR_WAVES; ++i) {
            const int half = (i % WR_WAVES) >= 4;
            for (int j = 0; j < 10; ++j) m[half][j] += (double)h[(size_t)i * 16 + j] / (nwg * 4);
            t0 = std::min(t0, h[(size_t)i * 16 + 10]); t1 = std::max(t1, h[(size_t)i * 16 + 10] + h[(size_t)i * 16 + 8]);
        }
        for (int half = 0; half < 2; ++half) {
            const double nt = std::max(1.0, m[half][9]);
            fprintf(stderr, "[wtrace rt] Cout=%d C=%d+%d %dx%d B=%d tile %dx%dx%d ks=%d xi=%d grid=%u nsplit=%d tiles/wg %.1f | waves %s (cycles): life %.0f = "
                    "setup %.0f + loop %.0f + exchange %.0f + flush %.0f | per tile: vmwait %.0f barrier %.0f issue %.0f compute %.0f db %.0f | span %lld\n",
                    k.Cout, k.C[0], k.C[1], k.Ho, k.Wo, k.B, k.ni, k.toh, k.tow, k.ksteps, k.xinstr, nwg, k.nsplit, nt, half ? "4-7" : "0-3",
                    m[half][8], m[half][0], m[half][1] + m[half][2] + m[half][3] + m[half][4] + m[half][5], m[half][6], m[half][7],
                    m[half][1] / nt, m[half][2] / nt, m[half][3] / nt, m[half][4] / nt, m[half][5] / nt, t1 - t0);
        }
    }
#endif
    return 0;
}

}  // namespace colvo
