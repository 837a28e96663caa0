// heads.hip -- the two network heads: the 1-channel DepthNet head (conv3x3 + sigmoid + disp->depth) and the PoseNet head
// (1x1 conv + spatial mean + pose/LCC scaling), forward and backward.
// Spec: oracle/colvo_spec.py (DepthNet.head / disp_to_depth, PoseNet.pred).
#include "elem.h"
#include "tuning.h"

namespace colvo {
namespace {

// ---------------------------------------------------------------- DepthNet head -------------- //
// pre = conv3x3(x; w[9][C]) + bias;  depth = 1 / (lo + (hi - lo) * sigmoid(pre))
__device__ __forceinline__ float head_depth(float pre, float lo, float hi) {
    const float sig = 1.0f / (1.0f + expf(-pre));
    return 1.0f / (lo + (hi - lo) * sig);
}
// its inverse, d(pre) from the saved depth:  sig = (1/depth - lo)/(hi-lo);  d depth/d pre = -(hi-lo) depth^2 sig (1-sig)
__device__ __forceinline__ float head_dpre(float depth, float d_depth, float lo, float hi) {
    const float k = hi - lo;
    const float sig = (1.0f / depth - lo) / k;
    return -d_depth * k * depth * depth * sig * (1.0f - sig);
}

template <int ES>
__global__ __launch_bounds__(NT) void k_depth_head_fwd(const void* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, int H, int W, int C, float lo,
                                                       float hi, float* __restrict__ depth) {
    extern __shared__ float sw[];   // 9*C
    for (int i = threadIdx.x; i < 9 * C; i += NT) sw[i] = w[i];
    __syncthreads();
    const int b = blockIdx.y;
    const size_t pix = (size_t)blockIdx.x * NT + threadIdx.x;
    if (pix >= (size_t)H * W) return;
    const int yy = (int)(pix / W), xx = (int)(pix - (size_t)yy * W);
    float acc = bias[0];
    for (int ky = 0; ky < 3; ++ky) {
        const int y2 = yy + ky - 1;
        if (y2 < 0 || y2 >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int x2 = xx + kx - 1;
            if (x2 < 0 || x2 >= W) continue;
            const size_t o = (((size_t)b * H + y2) * W + x2) * C;
            const float* wt = sw + (ky * 3 + kx) * C;
            for (int c = 0; c < C; ++c) acc += Elem<ES>::ld(x, o + c) * wt[c];
        }
    }
    depth[(size_t)b * H * W + pix] = head_depth(acc, lo, hi);
}

// C = 16 specialisation: one 16-channel pixel is 32 B (bf16) / 64 B (f32) -> 16-byte vector loads, weights in LDS
template <int ES>
__global__ __launch_bounds__(NT) void k_depth_head_fwd16(const void* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, int H, int W, float lo, float hi,
                                                         float* __restrict__ depth) {
    constexpr int C = 16;
    __shared__ float sw[9 * C];
    if (threadIdx.x < 9 * C) sw[threadIdx.x] = w[threadIdx.x];
    __syncthreads();
    const int b = blockIdx.y;
    const size_t pix = (size_t)blockIdx.x * NT + threadIdx.x;
    if (pix >= (size_t)H * W) return;
    const int yy = (int)(pix / W), xx = (int)(pix - (size_t)yy * W);
    float acc = bias[0];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int y2 = yy + ky - 1;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int x2 = xx + kx - 1;
            if (y2 < 0 || y2 >= H || x2 < 0 || x2 >= W) continue;
            const char* p = reinterpret_cast<const char*>(x) + ((((size_t)b * H + y2) * W + x2) * C) * ES;
            const float* wt = sw + (ky * 3 + kx) * C;
#pragma unroll
            for (int v = 0; v < C * ES / 16; ++v)
                granule_each<ES>(*reinterpret_cast<const uint4*>(p + 16 * v),
                                 [&](int k, float x) { acc = fmaf(x, wt[16 / ES * v + k], acc); });
        }
    }
    depth[(size_t)b * H * W + pix] = head_depth(acc, lo, hi);
}

// bf16: LDS-tiled form.  The kernel above pulls every input pixel through the L1 nine times (18 x 16 B per output: ~10 us of
// texture-path time for 16 frames of 256x320 before any latency); here a workgroup stages the (4 + 2) x (64 + 2) input pixels
// of its 4 x 64 output tile ONCE (coalesced 16-byte loads, zero outside the image) and the nine taps read LDS.  Pixel pitch
// 48 B: 16 consecutive pixels of a ds_read_b128 group start on 16 different 16-byte slots.
__global__ __launch_bounds__(NT) void k_depth_head_fwd16_lds(const void* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, int H, int W, float lo, float hi,
                                                             float* __restrict__ depth) {
    constexpr int C = 16, TH = 4, TW = 64, PH = TH + 2, PW = TW + 2, PITCH = 48;
    __shared__ float sw[9 * C];
    __shared__ __attribute__((aligned(16))) char tile[PH * PW * PITCH];
    const int tid = threadIdx.x;
    if (tid < 9 * C) sw[tid] = w[tid];
    const int b = blockIdx.z, y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
    const char* img = reinterpret_cast<const char*>(x) + (size_t)b * H * W * C * 2;
    for (int i = tid; i < PH * PW * 2; i += NT) {          // 2 granules of 16 B per pixel
        const int pix = i >> 1, h = i & 1;
        const int py = pix / PW, px = pix - py * PW;
        const int yy = y0 - 1 + py, xx = x0 - 1 + px;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = *reinterpret_cast<const uint4*>(img + ((size_t)yy * W + xx) * C * 2 + 16 * h);
        *reinterpret_cast<uint4*>(tile + pix * PITCH + 16 * h) = v;
    }
    __syncthreads();
    const int ty = tid >> 6, tx = tid & 63;
    const int yy = y0 + ty, xx = x0 + tx;
    if (yy >= H || xx >= W) return;
    float acc0 = bias[0], acc1 = 0.0f, acc2 = 0.0f;        // one chain per tap row
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        float a = 0.0f;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const char* p = tile + ((ty + ky) * PW + tx + kx) * PITCH;
            const float* wt = sw + (ky * 3 + kx) * C;
#pragma unroll
            for (int h = 0; h < 2; ++h)
                granule_each<2>(*reinterpret_cast<const uint4*>(p + 16 * h), [&](int k, float x) { a = fmaf(x, wt[8 * h + k], a); });
        }
        if (ky == 0) acc0 += a; else if (ky == 1) acc1 = a; else acc2 = a;
    }
    depth[(size_t)b * H * W + (size_t)yy * W + xx] = head_depth(acc0 + (acc1 + acc2), lo, hi);
}
// (A four-pixels-per-thread variant -- 36 instead of 72 loads per four outputs, four independent accumulators -- measured
// 35.9 us against this kernel's 24.7: a lane stride of 128 B costs more in the load path than the reuse saves.)

__global__ __launch_bounds__(NT) void k_depth_head_dpre(const float* __restrict__ depth, const float* __restrict__ d_depth,
                                                        size_t n, float lo, float hi, float* __restrict__ dpre) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i < n) dpre[i] = head_dpre(depth[i], d_depth[i], lo, hi);
}

__device__ __forceinline__ float scale_product(const float* sa, const float* sb) { return (sa ? sa[0] : 1.0f) * (sb ? sb[0] : 1.0f); }
// the same with the incoming gradient in parts: first half of the images g0 + sa*sb*graw, second half g1 + sa*sb*graw1
// (any may be null)
__global__ __launch_bounds__(NT) void k_depth_head_dpre_parts(const float* __restrict__ depth, const float* __restrict__ g0,
                                                              const float* __restrict__ g1, const float* __restrict__ graw,
                                                              const float* __restrict__ graw1,
                                                              const float* __restrict__ sa, const float* __restrict__ sb,
                                                              size_t n_half, float lo, float hi, float* __restrict__ dpre) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= 2 * n_half) return;
    float g;
    if (i < n_half) {
        g = g0 ? g0[i] : 0.0f;
        if (graw) g = fmaf(scale_product(sa, sb), graw[i], g);
    } else {
        g = g1 ? g1[i - n_half] : 0.0f;
        if (graw1) g = fmaf(scale_product(sa, sb), graw1[i - n_half], g);
    }
    dpre[i] = head_dpre(depth[i], g, lo, hi);
}

// g[ky * 3 + kx] = d(pre) of the output pixel whose tap (ky, kx) lands on (yy, xx), zero outside the image
__device__ __forceinline__ void gather_dpre9(const float* dpre, int b, int H, int W, int yy, int xx, float (&g)[9]) {
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int y2 = yy - ky + 1, x2 = xx - kx + 1;
            g[ky * 3 + kx] = (y2 >= 0 && y2 < H && x2 >= 0 && x2 < W) ? dpre[((size_t)b * H + y2) * W + x2] : 0.0f;
        }
}

// dx[y,x,c] = (x[y,x,c] > 0) * sum_taps dpre[y-ky+1, x-kx+1] * w[ky,kx,c]
template <int ES>
__global__ __launch_bounds__(NT) void k_depth_head_dgrad(const void* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ dpre, int H, int W, int C,
                                                         void* __restrict__ dx) {
    extern __shared__ float sw[];
    for (int i = threadIdx.x; i < 9 * C; i += NT) sw[i] = w[i];
    __syncthreads();
    const int b = blockIdx.y;
    const size_t pix = (size_t)blockIdx.x * NT + threadIdx.x;
    if (pix >= (size_t)H * W) return;
    const int yy = (int)(pix / W), xx = (int)(pix - (size_t)yy * W);
    float g[9];
    gather_dpre9(dpre, b, H, W, yy, xx, g);
    const size_t o = ((size_t)b * H * W + pix) * C;
    for (int c = 0; c < C; ++c) {
        float v = 0.0f;
#pragma unroll
        for (int t = 0; t < 9; ++t) v += g[t] * sw[t * C + c];
        Elem<ES>::st(dx, o + c, (Elem<ES>::ld(x, o + c) > 0.0f) ? v : 0.0f);
    }
}

// The same for C = 16 (the DepthNet head) with whole-pixel accesses: a thread reads its pixel's 16 channels as 16-byte granules,
// and writes them back the same way -- the generic kernel above issues 16 two-byte loads and stores per pixel.
template <int ES>
__global__ __launch_bounds__(NT) void k_depth_head_dgrad16(const void* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ dpre, int H, int W, void* __restrict__ dx) {
    constexpr int C = 16, NGR = C * ES / 16;       // granules per pixel: 2 (bf16) / 4 (f32)
    __shared__ float sw[9 * C];
    if (threadIdx.x < 9 * C) sw[threadIdx.x] = w[threadIdx.x];
    __syncthreads();
    const int b = blockIdx.y;
    const size_t pix = (size_t)blockIdx.x * NT + threadIdx.x;
    if (pix >= (size_t)H * W) return;
    const int yy = (int)(pix / W), xx = (int)(pix - (size_t)yy * W);
    float g[9];
    gather_dpre9(dpre, b, H, W, yy, xx, g);
    const size_t o = ((size_t)b * H * W + pix) * NGR;
    const uint4* xin = reinterpret_cast<const uint4*>(x) + o;
    uint4* out = reinterpret_cast<uint4*>(dx) + o;
    uint4 xv[NGR];
#pragma unroll
    for (int q = 0; q < NGR; ++q) xv[q] = xin[q];
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float a = 0.0f;
#pragma unroll
        for (int t = 0; t < 9; ++t) a += g[t] * sw[t * C + c];
        v[c] = a;
    }
    float xf[C];
#pragma unroll
    for (int q = 0; q < NGR; ++q) granule_floats<ES>(xv[q], xf + q * (16 / ES));
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = xf[c] > 0.0f ? v[c] : 0.0f;
    unsigned ow[4 * NGR];
#pragma unroll
    for (int j = 0; j < 4 * NGR; ++j) {
        if constexpr (ES == 2) ow[j] = pack2bf(v[2 * j], v[2 * j + 1]);
        else ow[j] = __float_as_uint(v[j]);
    }
#pragma unroll
    for (int q = 0; q < NGR; ++q) out[q] = uint4{ow[4 * q], ow[4 * q + 1], ow[4 * q + 2], ow[4 * q + 3]};
}

// dw[t][c] += sum_pix dpre[pix] * x[pix + tap][c];  db += sum dpre.
// Written from the input pixel's side: dw[t][c] = sum_q x[q][c] * dpre[q - tap].  Each thread walks a
// strided set of pixels q, keeps all 9*C products in registers, and the workgroup reduces ONCE at the
// end (wave shuffle + LDS) before one fp32 atomic per weight.
// ROWS = 3: a thread keeps all 9 x C products (145 accumulators: two waves per SIMD).  ROWS = 1: blockIdx.z selects the tap
// row ky and a thread keeps 3 x C products -- three times the threads, each re-reading its pixel's C channels from L2, at a
// third of the registers: more waves to hide the load latency this kernel is bound by.
template <int ES, int C, int ROWS>
__global__ __launch_bounds__(NT) void k_depth_head_wgrad(const void* __restrict__ x, const float* __restrict__ dpre,
                                                         int H, int W, int px_per_block, float* __restrict__ dw,
                                                         float* __restrict__ db, float* __restrict__ partials) {
    constexpr int NTAP = 3 * ROWS;
    const int ky0 = (ROWS == 3) ? 0 : (int)blockIdx.z;
    const bool with_bias = (ROWS == 3) || ky0 == 1;
    __shared__ float red[4][NTAP * C + 1];
    const int b = blockIdx.y;
    const int HW = H * W;
    const int p0 = blockIdx.x * px_per_block, p1 = min(HW, p0 + px_per_block);
    float acc[NTAP][C];
#pragma unroll
    for (int t = 0; t < NTAP; ++t)
#pragma unroll
        for (int c = 0; c < C; ++c) acc[t][c] = 0.0f;
    float sb = 0.0f;
    // The loads of pixel q + 256 are issued before the 9*C multiply-adds of pixel q (two waves per SIMD at ~180 VGPRs:
    // without it every iteration waited out a full memory round trip; 54 -> us, profiles/r2_bench_kernel_stats.csv).
    typedef __attribute__((ext_vector_type(4))) unsigned int u4;
    constexpr int NV = C * ES / 16;              // the pixel's C channels as 16-byte vectors (C * ES is a multiple of 16)
    struct Px { u4 raw[NV]; float d[NTAP]; float dc; };
    auto fetch = [&](int q, Px& o) {
        const int qy = q / W, qx = q - qy * W;
        const u4* px = reinterpret_cast<const u4*>(reinterpret_cast<const char*>(x) + ((size_t)b * HW + q) * C * ES);
#pragma unroll
        for (int v = 0; v < NV; ++v) o.raw[v] = px[v];
        o.dc = with_bias ? dpre[(size_t)b * HW + q] : 0.0f;
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ky = ky0 + r;
                const int oy = qy - ky + 1, ox = qx - kx + 1;      // output pixel whose tap (ky,kx) lands on q
                o.d[r * 3 + kx] = (oy >= 0 && oy < H && ox >= 0 && ox < W) ? dpre[((size_t)b * H + oy) * W + ox] : 0.0f;
            }
    };
    int q = p0 + (int)threadIdx.x;
    Px cur;
    if (q < p1) fetch(q, cur);
    while (q < p1) {
        const int qn = q + NT;
        Px nxt = cur;
        if (qn < p1) fetch(qn, nxt);
        float xv[C];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const u4 t = cur.raw[v];
            granule_floats<ES>(uint4{t[0], t[1], t[2], t[3]}, xv + v * (16 / ES));
        }
        sb += cur.dc;
#pragma unroll
        for (int t = 0; t < NTAP; ++t)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[t][c] = fmaf(cur.d[t], xv[c], acc[t][c]);
        cur = nxt;
        q = qn;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < NTAP; ++t)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float v = wave_sum(acc[t][c]);
            if (lane == 0) red[wave][t * C + c] = v;
        }
    sb = wave_sum(sb);
    if (lane == 0) red[wave][NTAP * C] = sb;
    __syncthreads();
    for (int k = threadIdx.x; k < NTAP * C + 1; k += NT) {
        const float v = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        if (partials) {
            // deterministic form: row (image, pixel range) of a [rows][9 C + 1] table, every entry written by exactly one workgroup
            float* row = partials + ((size_t)b * gridDim.x + blockIdx.x) * (9 * C + 1);
            if (k < NTAP * C) row[ky0 * 3 * C + k] = v;
            else if (with_bias) row[9 * C] = v;
        } else if (k < NTAP * C) atomicAdd(dw + ky0 * 3 * C + k, v);
        else if (with_bias) atomicAdd(db, v);
    }
}

// table form, second launch: dw[k] += sum over the table's rows (k < 9 C), db += column 9 C.  ONE WORKGROUP PER COLUMN: thread t adds
// rows t, t + 256, ... in order, the 256 partial sums meet in a fixed tree -- a fixed order, so the result is reproducible.  (The
// first form, one thread per column walking all rows, took 205 us for 640 rows: a chain of dependent strided loads.)
__global__ __launch_bounds__(NT) void k_head_wgrad_reduce(const float* __restrict__ partials, int rows, int ncol,
                                                          float* __restrict__ dw, float* __restrict__ db) {
    __shared__ float s[NT];
    const int k = blockIdx.x, tid = threadIdx.x;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    int r = tid;
    for (; r + 3 * NT < rows; r += 4 * NT) {            // four loads in flight
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] += partials[(size_t)(r + q * NT) * ncol + k];
    }
    for (int q = 0; r < rows; r += NT, ++q) v[q] += partials[(size_t)r * ncol + k];
    s[tid] = (v[0] + v[1]) + (v[2] + v[3]);
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (tid < o) s[tid] += s[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        if (k < ncol - 1) dw[k] += s[0];
        else db[0] += s[0];
    }
}

// generic-C fallback: one (tap, c) pair per thread over a strip of rows
template <int ES>
__global__ __launch_bounds__(NT) void k_depth_head_wgrad_generic(const void* __restrict__ x, const float* __restrict__ dpre,
                                                                 int H, int W, int C, int rows_per_block,
                                                                 float* __restrict__ dw, float* __restrict__ db) {
    const int b = blockIdx.y;
    const int y0 = blockIdx.x * rows_per_block, y1 = min(H, y0 + rows_per_block);
    const int tid = threadIdx.x;
    const int nk = 9 * C;
    for (int k = tid; k < nk + 1; k += NT) {
        float acc = 0.0f;
        if (k < nk) {
            const int t = k / C, c = k - t * C;
            const int ky = t / 3, kx = t - 3 * ky;
            for (int yy = y0; yy < y1; ++yy) {
                const int y2 = yy + ky - 1;
                if (y2 < 0 || y2 >= H) continue;
                for (int xx = 0; xx < W; ++xx) {
                    const int x2 = xx + kx - 1;
                    if (x2 < 0 || x2 >= W) continue;
                    acc += dpre[((size_t)b * H + yy) * W + xx] * Elem<ES>::ld(x, (((size_t)b * H + y2) * W + x2) * C + c);
                }
            }
            atomicAdd(dw + k, acc);
        } else {
            for (int yy = y0; yy < y1; ++yy)
                for (int xx = 0; xx < W; ++xx) acc += dpre[((size_t)b * H + yy) * W + xx];
            atomicAdd(db, acc);
        }
    }
}

// ---------------------------------------------------------------- PoseNet head --------------- //
// o_j = s_j * (bias_j + mean_p sum_c x[b][p][c] w[j][c]) (+1 for j = 6);  s = pose_scale (j<6) | lcc_scale.
// Output is PLANAR: out = [ pose B x 6 | lcc_a B | lcc_b B ], so the three results are contiguous views.
template <int ES>
__global__ __launch_bounds__(NT) void k_pose_head_fwd(const void* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, int HW, int C, float pose_scale,
                                                      float lcc_scale, float* __restrict__ out) {
    __shared__ float red[4][8];
    const int b = blockIdx.x, tid = threadIdx.x;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
    for (int c = tid; c < C; c += NT) {
        float sx = 0.0f;
        for (int p = 0; p < HW; ++p) sx += Elem<ES>::ld(x, ((size_t)b * HW + p) * C + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += sx * w[j * C + c];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = wave_sum(acc[j]);
        if ((tid & 63) == 0) red[tid >> 6][j] = v;
    }
    __syncthreads();
    if (tid < 8) {
        const float pre = bias[tid] + ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) / (float)HW;
        float o = (tid < 6 ? pose_scale : lcc_scale) * pre;
        if (tid == 6) o += 1.0f;
        const int B = gridDim.x;
        if (tid < 6) out[b * 6 + tid] = o;
        else out[6 * B + (tid - 6) * B + b] = o;
    }
}

// the gradient of image b's eight outputs, scaled
__device__ __forceinline__ void pose_go(const float* d_pose, const float* d_a, const float* d_b, int b, float pose_scale, float lcc_scale,
                                        float (&go)[8]) {
#pragma unroll
    for (int j = 0; j < 6; ++j) go[j] = d_pose ? d_pose[b * 6 + j] * pose_scale : 0.0f;
    go[6] = d_a ? d_a[b] * lcc_scale : 0.0f;
    go[7] = d_b ? d_b[b] * lcc_scale : 0.0f;
}
// channel c of image b: writes dx over the image's pixels and returns the sum of x over them (dw[j][c] takes go[j] * sum * inv)
template <int ES>
__device__ __forceinline__ float pose_channel_bwd(const void* x, const float* w, const float (&go)[8],
                                                  int b, int c, int HW, int C, float inv, void* dx) {
    float g = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) g += go[j] * w[j * C + c];
    g *= inv;
    float sx = 0.0f;
    for (int p = 0; p < HW; ++p) {
        const size_t o = ((size_t)b * HW + p) * C + c;
        const float xv = Elem<ES>::ld(x, o);
        sx += xv;
        Elem<ES>::st(dx, o, xv > 0.0f ? g : 0.0f);
    }
    return sx;
}

template <int ES>
__global__ __launch_bounds__(NT) void k_pose_head_bwd(const void* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ d_pose, const float* __restrict__ d_a,
                                                      const float* __restrict__ d_b, const float* __restrict__ sa,
                                                      const float* __restrict__ sb, int HW, int C, float pose_scale,
                                                      float lcc_scale, void* __restrict__ dx, float* __restrict__ dw,
                                                      float* __restrict__ db) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float gs = scale_product(sa, sb);
    float go[8];
    pose_go(d_pose, d_a, d_b, b, pose_scale * gs, lcc_scale * gs, go);
    const float inv = 1.0f / (float)HW;
    for (int c = tid; c < C; c += NT) {
        const float sx = pose_channel_bwd<ES>(x, w, go, b, c, HW, C, inv, dx);
#pragma unroll
        for (int j = 0; j < 8; ++j) atomicAdd(dw + j * C + c, go[j] * sx * inv);
    }
    if (tid < 8) atomicAdd(db + tid, go[tid]);
}

// Deterministic form of the PoseNet head backward: thread = channel, the images are walked IN ORDER by the one thread that owns
// dw[.][c] (no atomics); dx as above.  The head sees <= 20 pixels per image: the serial walk costs a few microseconds.
template <int ES>
__global__ __launch_bounds__(NT) void k_pose_head_bwd_det(const void* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ d_pose, const float* __restrict__ d_a,
                                                          const float* __restrict__ d_b, const float* __restrict__ sa,
                                                          const float* __restrict__ sb, int B, int HW, int C, float pose_scale,
                                                          float lcc_scale, void* __restrict__ dx, float* __restrict__ dw,
                                                          float* __restrict__ db) {
    const int c = blockIdx.x * NT + threadIdx.x;
    const float gs = scale_product(sa, sb);
    pose_scale *= gs;
    lcc_scale *= gs;
    const float inv = 1.0f / (float)HW;
    float dwacc[8], dbacc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { dwacc[j] = 0.0f; dbacc[j] = 0.0f; }
    for (int b = 0; b < B; ++b) {
        float go[8];
        pose_go(d_pose, d_a, d_b, b, pose_scale, lcc_scale, go);
#pragma unroll
        for (int j = 0; j < 8; ++j) dbacc[j] += go[j];
        if (c >= C) continue;
        const float sx = pose_channel_bwd<ES>(x, w, go, b, c, HW, C, inv, dx);
#pragma unroll
        for (int j = 0; j < 8; ++j) dwacc[j] += go[j] * sx * inv;
    }
    if (c < C) {
#pragma unroll
        for (int j = 0; j < 8; ++j) dw[j * C + c] += dwacc[j];
    }
    if (c < 8) db[c] += dbacc[c];
}

// The same sums with the loads side by side (tuning.h: pose_head_det_parallel).  The kernel above is one workgroup whose threads each
// walk B x HW pixels with ONE load in flight: 48 dependent round trips at 8 images of 6 pixels, 24 us between the loss and PoseNet's
// backward pass.  Here a workgroup owns PH_CS channels and thread (bl, cl) the pair (image b0 + bl, channel c0 + cl): the pixel
// loads of different pairs are independent and a pair's own come PH_U at a time.  A pair parks its sum of x and its image's eight
// gradients in LDS; thread (0, cl) then adds the images' terms to dw[.][c] / db with b ascending, group after group of PH_NB images
// -- the order of the serial walk.  Bits: every rounding step of the kernel above is written out (its listing fuses go[j] * w[j]
// into g and (go[j] * sx) * inv into dwacc[j], and nothing else), with contraction off so that none is added.
constexpr int PH_CS = 32;                  // channels of a workgroup
constexpr int PH_NB = NT / PH_CS;          // images of a group
constexpr int PH_U = 8;                    // pixel loads a pair has in flight
template <int ES>
__global__ __launch_bounds__(NT) void k_pose_head_bwd_det_par(const void* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ d_pose, const float* __restrict__ d_a,
                                                              const float* __restrict__ d_b, const float* __restrict__ sa,
                                                              const float* __restrict__ sb, int B, int HW, int C, float pose_scale,
                                                              float lcc_scale, void* __restrict__ dx, float* __restrict__ dw,
                                                              float* __restrict__ db) {
#pragma clang fp contract(off)
    __shared__ float s_sx[PH_NB][PH_CS];
    __shared__ float s_go[PH_NB][8];
    const int cl = threadIdx.x % PH_CS, bl = threadIdx.x / PH_CS;
    const int c = blockIdx.x * PH_CS + cl;
    const bool owner = bl == 0 && c < C;                       // adds channel c's terms; c < 8: db[c] as well
    const float gs = (sa ? sa[0] : 1.0f) * (sb ? sb[0] : 1.0f);
    pose_scale = pose_scale * gs;
    lcc_scale = lcc_scale * gs;
    const float inv = 1.0f / (float)HW;
    float wv[8], dw0[8], dwacc[8], dbacc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        wv[j] = c < C ? w[j * C + c] : 0.0f;
        dw0[j] = owner ? dw[j * C + c] : 0.0f;
        dwacc[j] = 0.0f;
        dbacc[j] = 0.0f;
    }
    const float db0 = owner && c < 8 ? db[c] : 0.0f;
    for (int b0 = 0; b0 < B; b0 += PH_NB) {
        const int b = b0 + bl;
        if (b < B) {
            float go[8];                                       // (the loads first, side by side; then the products)
#pragma unroll
            for (int j = 0; j < 8; ++j) go[j] = 0.0f;
            if (d_pose) {
#pragma unroll
                for (int j = 0; j < 6; ++j) go[j] = d_pose[(size_t)b * 6 + j];
            }
            if (d_a) go[6] = d_a[b];
            if (d_b) go[7] = d_b[b];
#pragma unroll
            for (int j = 0; j < 6; ++j) go[j] = d_pose ? go[j] * pose_scale : 0.0f;
            go[6] = d_a ? go[6] * lcc_scale : 0.0f;
            go[7] = d_b ? go[7] * lcc_scale : 0.0f;
            if (cl == 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) s_go[bl][j] = go[j];
            }
            if (c < C) {
                float g = __builtin_fmaf(go[0], wv[0], 0.0f);
#pragma unroll
                for (int j = 1; j < 8; ++j) g = __builtin_fmaf(go[j], wv[j], g);
                g = g * inv;
                float sx = 0.0f;
                for (int p0 = 0; p0 < HW; p0 += PH_U) {
                    const size_t o = ((size_t)b * HW + p0) * C + c;
                    float xv[PH_U];
#pragma unroll
                    for (int u = 0; u < PH_U; ++u) xv[u] = Elem<ES>::ld(x, o + (size_t)min(u, HW - 1 - p0) * C);   // past the end: the last pixel again, unused
#pragma unroll
                    for (int u = 0; u < PH_U; ++u) {
                        const bool in = p0 + u < HW;
                        const float gv = xv[u] > 0.0f ? g : 0.0f;
                        sx = in ? sx + xv[u] : sx;                 // (a select: a load used only under a branch sinks into it)
                        if (in) Elem<ES>::st(dx, o + (size_t)u * C, gv);
                    }
                }
                s_sx[bl][cl] = sx;
            }
        }
        __syncthreads();
        if (owner) {
            const int nb = min(PH_NB, B - b0);
            for (int i = 0; i < nb; ++i) {
                const float sx = s_sx[i][cl];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float go = s_go[i][j];
                    dbacc[j] = dbacc[j] + go;
                    dwacc[j] = __builtin_fmaf(inv, go * sx, dwacc[j]);
                }
            }
        }
        __syncthreads();
    }
    if (owner) {
#pragma unroll
        for (int j = 0; j < 8; ++j) dw[j * C + c] = dwacc[j] + dw0[j];
        if (c < 8) {
            float t = dbacc[0];
#pragma unroll
            for (int j = 1; j < 8; ++j) t = c == j ? dbacc[j] : t;
            db[c] = t + db0;
        }
    }
}

inline bool head_dgrad_generic() { return TUNE(head_dgrad_generic) != 0; }   // A/B switch

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" int colvo_depth_head_fwd(int dtype, const void* x, const float* w, const float* bias, int B, int H, int W,
                                    int C, float min_depth, float max_depth, float* depth, colvo_stream_t stream) {
    COLVO_CHECK_ARG(x && w && bias && depth, "colvo_depth_head_fwd: null pointer argument");
    COLVO_CHECK_DTYPE(dtype, "colvo_depth_head_fwd");
    COLVO_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && C >= 1 && C <= 1024 && min_depth > 0 && max_depth > min_depth,
                    "colvo_depth_head_fwd: bad shape / range");
    const size_t HW = (size_t)H * W;
    const int head_lds = (int)TUNE(head_fwd_lds);   // A/B switch
    if (C == 16 && dtype == COLVO_BF16 && head_lds && (H + 3) / 4 <= 65535)
        colvo::launch(k_depth_head_fwd16_lds, dim3((W + 63) / 64, (H + 3) / 4, B), dim3(NT), 0, (hipStream_t)stream, x, w,
                           bias, H, W, 1.0f / max_depth, 1.0f / min_depth, depth);
    else if (C == 16)
        DISPATCH_ES(dtype, colvo::launch((k_depth_head_fwd16<ES>), dim3(nblk(HW), B), dim3(NT), 0, (hipStream_t)stream, x,
                                              w, bias, H, W, 1.0f / max_depth, 1.0f / min_depth, depth));
    else
        DISPATCH_ES(dtype, colvo::launch((k_depth_head_fwd<ES>), dim3(nblk(HW), B), dim3(NT), 9 * C * sizeof(float),
                                              (hipStream_t)stream, x, w, bias, H, W, C, 1.0f / max_depth, 1.0f / min_depth, depth));
    COLVO_CHECK_LAUNCH("k_depth_head_fwd");
    return 0;
}

// pixels per workgroup of the C = 16 kernel: a multiple of 256, at least 8 per thread, and at most ~512 workgroups (two per CU
// resident)
static int head_wgrad_ppb(size_t HW, int B) {
    int ppb = 2048;
    while ((HW + ppb - 1) / ppb * B > 512 && ppb < 16384) ppb += 256;
    return ppb;
}

extern "C" size_t colvo_depth_head_wgrad_scratch_bytes(int B, int H, int W, int C) {
    if (C != 16 || B < 1 || H < 1 || W < 1) return 0;
    const size_t HW = (size_t)H * W;
    const int ppb = head_wgrad_ppb(HW, B);
    return (size_t)B * ((HW + ppb - 1) / ppb) * (9 * C + 1) * sizeof(float);
}

static int depth_head_wgrad_impl(int dtype, const void* x, const float* dpre, int B, int H, int W, int C, float* dw, float* db,
                                 float* partials, size_t partial_bytes, colvo_stream_t stream) {
    COLVO_CHECK_ARG(x && dpre && dw && db, "colvo_depth_head_wgrad: null pointer argument");
    COLVO_CHECK_DTYPE(dtype, "colvo_depth_head_wgrad");
    COLVO_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && C >= 1 && C <= 1024, "colvo_depth_head_wgrad: bad shape");
    hipStream_t s = (hipStream_t)stream;
    const size_t HW = (size_t)H * W;
    if (C == 16) {
        const int ppb = head_wgrad_ppb(HW, B);
        const int rows_tab = (int)(B * ((HW + ppb - 1) / ppb));
        COLVO_CHECK_ARG(!partials || (size_t)rows_tab * (9 * 16 + 1) * sizeof(float) <= partial_bytes,
                        "colvo_depth_head_wgrad_det: scratch too small (colvo_depth_head_wgrad_scratch_bytes)");
        // tap rows per thread: 1 (three workgroups per pixel range) measured 57 -> 45 us inside the step, step -1 %
        const int rows = (int)TUNE(head_wgrad_rows);   // A/B switch
        DISPATCH_ES(dtype, colvo::launch(rows == 3 ? (k_depth_head_wgrad<ES, 16, 3>) : (k_depth_head_wgrad<ES, 16, 1>),
                                         dim3((unsigned)((HW + ppb - 1) / ppb), B, rows == 3 ? 1 : 3), dim3(NT), 0, s, x, dpre, H, W, ppb,
                                         dw, db, partials));
        if (partials)
            colvo::launch(k_head_wgrad_reduce, dim3(9 * 16 + 1), dim3(NT), 0, s, (const float*)partials, rows_tab, 9 * 16 + 1, dw, db);
    } else {
        const int rows = 4;
        DISPATCH_ES(dtype, colvo::launch((k_depth_head_wgrad_generic<ES>), dim3((H + rows - 1) / rows, B), dim3(NT),
                                              0, s, x, dpre, H, W, C, rows, dw, db));
    }
    COLVO_CHECK_LAUNCH("k_depth_head_wgrad");
    return 0;
}

// The weight / bias gradient alone, from the d(pre) plane colvo_depth_head_bwd left in `scratch` (so that it can run on
// another stream than the input gradient).
extern "C" int colvo_depth_head_wgrad(int dtype, const void* x, const float* dpre, int B, int H, int W, int C, float* dw,
                                      float* db, colvo_stream_t stream) {
    return depth_head_wgrad_impl(dtype, x, dpre, B, H, W, C, dw, db, nullptr, 0, stream);
}

extern "C" int colvo_depth_head_wgrad_det(int dtype, const void* x, const float* dpre, int B, int H, int W, int C, float* dw,
                                          float* db, void* scratch, size_t scratch_bytes, colvo_stream_t stream) {
    COLVO_CHECK_ARG(scratch && C == 16, "colvo_depth_head_wgrad_det: needs scratch and the 16-channel head");
    return depth_head_wgrad_impl(dtype, x, dpre, B, H, W, C, dw, db, (float*)scratch, scratch_bytes, stream);
}

extern "C" int colvo_depth_head_wgrad_reduce(const float* partials, int rows, float* dw, float* db, colvo_stream_t stream) {
    COLVO_CHECK_ARG(partials && dw && db && rows >= 1, "colvo_depth_head_wgrad_reduce: bad arguments");
    colvo::launch(k_head_wgrad_reduce, dim3(9 * 16 + 1), dim3(NT), 0, (hipStream_t)stream, partials, rows, 9 * 16 + 1, dw, db);
    COLVO_CHECK_LAUNCH("k_head_wgrad_reduce");
    return 0;
}

// the input gradient from the d(pre) plane, for both entry points below: the granule form needs C = 16 and 16-byte aligned x and dx
static int depth_head_dgrad(int dtype, const void* x, const float* w, const float* dpre, int B, int H, int W, int C, void* dx,
                            hipStream_t s) {
    const size_t HW = (size_t)H * W;
    if (C == 16 && ((uintptr_t)x | (uintptr_t)dx) % 16 == 0 && !head_dgrad_generic())
        DISPATCH_ES(dtype, colvo::launch((k_depth_head_dgrad16<ES>), dim3(nblk(HW), B), dim3(NT), 0, s, x, w, dpre, H, W, dx));
    else
        DISPATCH_ES(dtype, colvo::launch((k_depth_head_dgrad<ES>), dim3(nblk(HW), B), dim3(NT), 9 * C * sizeof(float), s, x, w, dpre,
                                         H, W, C, dx));
    COLVO_CHECK_LAUNCH("k_depth_head_dgrad");
    return 0;
}

// scratch: B*H*W floats (the d(pre) plane), caller-provided.
extern "C" int colvo_depth_head_bwd(int dtype, const void* x, const float* w, const float* depth, const float* d_depth,
                                    int B, int H, int W, int C, float min_depth, float max_depth, float* scratch,
                                    void* dx, float* dw, float* db, colvo_stream_t stream) {
    COLVO_CHECK_ARG(x && w && depth && d_depth && scratch && dx && ((dw == nullptr) == (db == nullptr)),
                    "colvo_depth_head_bwd: null pointer argument");
    COLVO_CHECK_DTYPE(dtype, "colvo_depth_head_bwd");
    COLVO_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && C >= 1 && C <= 1024 && min_depth > 0 && max_depth > min_depth,
                    "colvo_depth_head_bwd: bad shape / range");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)B * H * W;
    const float lo = 1.0f / max_depth, hi = 1.0f / min_depth;
    colvo::launch(k_depth_head_dpre, dim3(nblk(n)), dim3(NT), 0, s, depth, d_depth, n, lo, hi, scratch);
    COLVO_CHECK_LAUNCH("k_depth_head_dpre");
    if (int e = dw ? colvo_depth_head_wgrad(dtype, x, scratch, B, H, W, C, dw, db, stream) : 0) return e;
    return depth_head_dgrad(dtype, x, w, scratch, B, H, W, C, dx, s);
}

extern "C" int colvo_depth_head_bwd_parts(int dtype, const void* x, const float* w, const float* depth, const float* g_first,
                                          const float* g_second, const float* g_raw, const float* g_raw_second,
                                          const float* scale_a, const float* scale_b, int B, int H, int W, int C,
                                          float min_depth, float max_depth, float* scratch, void* dx, float* dw, float* db,
                                          colvo_stream_t stream) {
    COLVO_CHECK_ARG(x && w && depth && scratch && ((dw == nullptr) == (db == nullptr)),
                    "colvo_depth_head_bwd_parts: null pointer argument");
    COLVO_CHECK_DTYPE(dtype, "colvo_depth_head_bwd_parts");
    COLVO_CHECK_ARG(B >= 2 && B % 2 == 0 && B <= 65534 && H >= 1 && W >= 1 && C >= 1 && C <= 1024 && min_depth > 0 &&
                        max_depth > min_depth,
                    "colvo_depth_head_bwd_parts: bad shape / range (B = 2*Bh images)");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)B * H * W;
    const float lo = 1.0f / max_depth, hi = 1.0f / min_depth;
    colvo::launch(k_depth_head_dpre_parts, dim3(nblk(n)), dim3(NT), 0, s, depth, g_first, g_second, g_raw, g_raw_second,
                       scale_a, scale_b, n / 2, lo, hi, scratch);
    COLVO_CHECK_LAUNCH("k_depth_head_dpre_parts");
    if (int e = dw ? colvo_depth_head_wgrad(dtype, x, scratch, B, H, W, C, dw, db, stream) : 0) return e;
    if (!dx) return 0;          // d(pre) only: the input gradient is made by colvo_conv_bwd_fused's HEAD form from `scratch`
    return depth_head_dgrad(dtype, x, w, scratch, B, H, W, C, dx, s);
}

extern "C" int colvo_pose_head_fwd(int dtype, const void* x, const float* w, const float* bias, int B, int HW, int C,
                                   float pose_scale, float lcc_scale, float* out, colvo_stream_t stream) {
    COLVO_CHECK_ARG(x && w && bias && out && B >= 1 && HW >= 1 && C >= 1, "colvo_pose_head_fwd: bad arguments");
    COLVO_DISPATCH_ES(dtype, "colvo_pose_head_fwd",
                      colvo::launch((k_pose_head_fwd<ES>), dim3(B), dim3(NT), 0, (hipStream_t)stream, x, w, bias, HW, C, pose_scale,
                                    lcc_scale, out));
    COLVO_CHECK_LAUNCH("k_pose_head_fwd");
    return 0;
}

extern "C" int colvo_pose_head_bwd(int dtype, const void* x, const float* w, const float* d_pose, const float* d_a,
                                   const float* d_b, const float* scale_a, const float* scale_b, int B, int HW, int C,
                                   float pose_scale, float lcc_scale, void* dx, float* dw, float* db, colvo_stream_t stream) {
    COLVO_CHECK_ARG(x && w && dx && dw && db && B >= 1 && HW >= 1 && C >= 1, "colvo_pose_head_bwd: bad arguments");
    COLVO_DISPATCH_ES(dtype, "colvo_pose_head_bwd",
                      colvo::launch((k_pose_head_bwd<ES>), dim3(B), dim3(NT), 0, (hipStream_t)stream, x, w, d_pose, d_a, d_b,
                                    scale_a, scale_b, HW, C, pose_scale, lcc_scale, dx, dw, db));
    COLVO_CHECK_LAUNCH("k_pose_head_bwd");
    return 0;
}

extern "C" int colvo_pose_head_bwd_det(int dtype, const void* x, const float* w, const float* d_pose, const float* d_a,
                                       const float* d_b, const float* scale_a, const float* scale_b, int B, int HW, int C,
                                       float pose_scale, float lcc_scale, void* dx, float* dw, float* db, colvo_stream_t stream) {
    COLVO_CHECK_ARG(x && w && dx && dw && db && B >= 1 && HW >= 1 && C >= 8, "colvo_pose_head_bwd_det: bad arguments");
    const bool par = TUNE(pose_head_det_parallel) != 0;
    COLVO_DISPATCH_ES(dtype, "colvo_pose_head_bwd_det",
                      if (par) colvo::launch((k_pose_head_bwd_det_par<ES>), dim3((C + PH_CS - 1) / PH_CS), dim3(NT), 0, (hipStream_t)stream,
                                             x, w, d_pose, d_a, d_b, scale_a, scale_b, B, HW, C, pose_scale, lcc_scale, dx, dw, db);
                      else colvo::launch((k_pose_head_bwd_det<ES>), dim3((C + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, x, w,
                                         d_pose, d_a, d_b, scale_a, scale_b, B, HW, C, pose_scale, lcc_scale, dx, dw, db));
    COLVO_CHECK_LAUNCH("k_pose_head_bwd_det");
    return 0;
}
