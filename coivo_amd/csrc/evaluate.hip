// evaluate.hip -- depth evaluation with per-image median scaling: the Eigen et al. / Monodepth2
// compute_errors measures (abs_rel, sq_rel, rmse, rmse_log, a1..a3) over the valid pixels of each image.
//
//   valid     gt > min_depth && gt < max_depth && (mask == NULL || mask != 0)      (NaN / inf in gt fall out)
//   median    exact lower median (rank (n-1)/2) of pred and of gt over the valid pixels: radix select on an order-preserving
//             uint32 image of the float bits, three digit passes of 11 + 11 + 10 bits
//   scale     s = med(gt) / med(pred) (IEEE division; 1 without median scaling), p = clamp(s * pred, min_depth, max_depth)
//
// Every hand-off between phases is a kernel boundary.  Histograms are counted with integer atomics (exact, order-free); float
// sums are reduced in a fixed order (per-thread f32 over at most PPT pixels, then f64 in a fixed tree), so a call's bits do
// not depend on scheduling.  Limits as csrc/reconstruct.hip: N <= 65535 (grid .y = image), H*W < 2^30.
#include "common.h"

namespace colvo {
namespace {

constexpr int NT = 256;                    // threads per workgroup of the per-pixel kernels
constexpr int PPT = 32;                    // pixels per thread (f32 partial sums span at most this many pixels)
constexpr int PIX_PER_WG = NT * PPT;
constexpr int BINS = 2048;                 // 11-bit digit; pass 3 uses the low 1024
constexpr int NSUM = 8;                    // partial row: 7 sums + pad (one 64-B line)

// per image, between passes: the prefix of the selected key and the rank still to find inside it, for pred [0] and gt [1]
struct EvalState {
    uint32_t prefix[2];
    uint32_t rank[2];
    int32_t n;                             // valid pixels (from pass 1)
    uint32_t pad_[3];
};
static_assert(sizeof(EvalState) == 32, "EvalState is 32 B");

struct EvalWs {
    uint32_t* hist;                        // [N][2][BINS]
    EvalState* state;                      // [N]
    double* partials;                      // [N][chunks][NSUM]
    size_t bytes;
};

int eval_chunks(int H, int W) { return blocks_of((long long)H * W, PIX_PER_WG); }

EvalWs eval_ws(void* base, int N, int chunks) {
    Carver c(base);
    EvalWs w;
    w.hist = c.take<uint32_t>((size_t)N * 2 * BINS);
    w.state = c.take<EvalState>(N);
    w.partials = c.take<double>((size_t)N * chunks * NSUM);
    w.bytes = c.bytes();
    return w;
}

// One LDS histogram increment per active lane, called by the whole (converged) wave.  Depth maps are smooth, so the 64
// consecutive pixels of a wave mostly share a bin: the lanes that agree with the first active lane add once, through it; the
// rest add one by one.
__device__ __forceinline__ void wave_hist_add(uint32_t* h, bool active, uint32_t bin) {
    const unsigned long long act = __ballot(active);
    if (act == 0) return;
    const int leader = __builtin_ctzll(act);
    const uint32_t lead_bin = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
    const bool same = active && bin == lead_bin;
    const unsigned long long m = __ballot(same);
    const int lane = threadIdx.x & 63;
    if (lane == leader) atomicAdd(&h[lead_bin], (uint32_t)__popcll(m));
    else if (active && !same) atomicAdd(&h[bin], 1u);
}

// U pixels of one thread (p, p + NT, ...): every load issued before any is used (the loads are what bounds both per-pixel kernels;
// one at a time, a thread's latency chain left HBM idle).  Out-of-range pixels read pixel 0 of the image and come back in = false.
constexpr int U = 8;
static_assert(PPT % U == 0, "PPT is a multiple of U");
template <int UU>
__device__ __forceinline__ void load_px(const float* __restrict__ pred, const float* __restrict__ gt,
                                        const uint8_t* __restrict__ mask, size_t base, int p, int HW, float* gv, float* pv,
                                        bool* in) {
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        const int q = p + u * NT;
        in[u] = q < HW;
        const size_t i = base + (in[u] ? q : 0);
        gv[u] = gt[i];
        pv[u] = pred[i];
    }
    if (mask != nullptr) {
        uint8_t mv[UU];
#pragma unroll
        for (int u = 0; u < UU; ++u) mv[u] = mask[base + (in[u] ? p + u * NT : 0)];
#pragma unroll
        for (int u = 0; u < UU; ++u) in[u] = in[u] && mv[u] != 0;
    }
}

// grid (chunks, N): histogram of the current digit of pred's and gt's keys over the valid pixels whose higher digits equal the
// prefix selected so far, into the image's global histograms.  pass 0: bits 31..21; pass 1: 20..10; pass 2: 9..0.
__global__ __launch_bounds__(NT) void k_eval_hist(const float* __restrict__ pred, const float* __restrict__ gt,
                                                  const uint8_t* __restrict__ mask, int HW, float lo, float hi, int pass,
                                                  uint32_t* __restrict__ hist, const EvalState* __restrict__ state) {
    __shared__ uint32_t h[2 * BINS];
    const int img = blockIdx.y;
    uint32_t pre_p = 0, pre_g = 0;
    if (pass > 0) {
        const EvalState& st = state[img];
        if (st.n == 0) return;                         // empty image: nothing to select (uniform over the workgroup)
        pre_p = st.prefix[0];
        pre_g = st.prefix[1];
    }
    for (int b = threadIdx.x; b < 2 * BINS; b += NT) h[b] = 0;
    __syncthreads();
    const int hi_shift = pass == 1 ? 21 : 10;          // pass > 0: a key matches iff key >> hi_shift == prefix
    const int lo_shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
    const uint32_t dmask = pass == 2 ? 0x3ffu : 0x7ffu;
    const size_t base = (size_t)img * HW;
    const int p0 = blockIdx.x * PIX_PER_WG + threadIdx.x;
    for (int j0 = 0; j0 < PPT; j0 += U) {
        float gv[U], pv[U];
        bool in[U];
        load_px<U>(pred, gt, mask, base, p0 + j0 * NT, HW, gv, pv, in);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool v = in[u] && gv[u] > lo && gv[u] < hi;
            const uint32_t kp = float_key(pv[u]), kg = float_key(gv[u]);
            const bool vp = v && (pass == 0 || (kp >> hi_shift) == pre_p);
            const bool vg = v && (pass == 0 || (kg >> hi_shift) == pre_g);
            wave_hist_add(h, vp, (kp >> lo_shift) & dmask);
            wave_hist_add(h + BINS, vg, (kg >> lo_shift) & dmask);
        }
    }
    __syncthreads();
    uint32_t* gh = hist + (size_t)img * 2 * BINS;
    for (int b = threadIdx.x; b < 2 * BINS; b += NT) {
        const uint32_t v = h[b];
        if (v) atomicAdd(&gh[b], v);
    }
}

// grid N: clear the image's histograms and state (the workspace is the caller's and may hold anything)
__global__ __launch_bounds__(NT) void k_eval_init(uint32_t* __restrict__ hist, EvalState* __restrict__ state) {
    uint32_t* gh = hist + (size_t)blockIdx.x * 2 * BINS;
    for (int b = threadIdx.x; b < 2 * BINS; b += NT) gh[b] = 0;
    if (threadIdx.x == 0) state[blockIdx.x] = EvalState{};
}

// grid N: find the bucket that holds the wanted rank in each histogram, narrow prefix and rank, clear the histogram for the next
// pass.  Pass 0 also counts the valid pixels and sets the rank (n-1)/2.  On the last pass: the medians, the scale, n_valid.
__global__ __launch_bounds__(NT) void k_eval_select(uint32_t* __restrict__ hist, EvalState* __restrict__ state, int pass,
                                                    int last, int median_scaling, float* __restrict__ scale_out,
                                                    int32_t* __restrict__ n_out) {
    constexpr int PER = BINS / NT;                     // 8 bins per thread
    __shared__ uint32_t scan[NT];
    __shared__ uint32_t found[2][2];                   // bucket, count below it
    const int img = blockIdx.x;
    const int t = threadIdx.x;
    uint32_t* gh = hist + (size_t)img * 2 * BINS;
    EvalState& st = state[img];
    const int n = pass == 0 ? -1 : st.n;               // pass 0: counted below
    if (n == 0) {                                      // empty image (pass > 0): nothing was counted
        if (last && t == 0) { scale_out[img] = __builtin_nanf(""); n_out[img] = 0; }
        return;
    }
    uint32_t rank[2] = {pass == 0 ? 0u : st.rank[0], pass == 0 ? 0u : st.rank[1]};
    int total = n;
    for (int w = 0; w < 2; ++w) {
        uint32_t c[PER];
        uint32_t s = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) { c[j] = gh[w * BINS + t * PER + j]; s += c[j]; }
        scan[t] = s;
        __syncthreads();
        for (int off = 1; off < NT; off <<= 1) {       // inclusive Hillis-Steele scan over the 256 thread sums
            const uint32_t v = t >= off ? scan[t - off] : 0u;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        if (pass == 0) {
            total = (int)scan[NT - 1];                 // every valid pixel lands in exactly one bucket of each histogram
            rank[w] = total > 0 ? (uint32_t)(total - 1) / 2 : 0u;
        }
        uint32_t below = scan[t] - s;                  // exclusive prefix of this thread's first bin
        if (total > 0 && rank[w] >= below && rank[w] < below + s) {
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                if (rank[w] < below + c[j]) { found[w][0] = t * PER + j; found[w][1] = below; break; }
                below += c[j];
            }
        }
        __syncthreads();                               // scan[] is reused by the next histogram
    }
    for (int b = t; b < 2 * BINS; b += NT) gh[b] = 0;
    if (t != 0) return;
    if (total == 0) {                                  // pass 0 found no valid pixel
        st.n = 0;
        if (last) { scale_out[img] = __builtin_nanf(""); n_out[img] = 0; }
        return;
    }
    const int bits = pass == 2 ? 10 : 11;
    uint32_t pre[2];
    for (int w = 0; w < 2; ++w) {
        pre[w] = (pass == 0 ? 0u : (st.prefix[w] << bits)) | found[w][0];
        st.prefix[w] = pre[w];
        st.rank[w] = rank[w] - found[w][1];
    }
    if (pass == 0) st.n = total;
    if (last) {
        float s = 1.0f;
        if (median_scaling) s = __fdiv_rn(float_key_inv(pre[1]), float_key_inv(pre[0]));   // med(gt) / med(pred)
        scale_out[img] = s;
        n_out[img] = total;
    }
}

// grid (chunks, N): scaled and clamped prediction against gt; one f64 row of the seven sums per workgroup
__global__ __launch_bounds__(NT) void k_eval_metrics(const float* __restrict__ pred, const float* __restrict__ gt,
                                                     const uint8_t* __restrict__ mask, int HW, float lo, float hi,
                                                     const float* __restrict__ scale, const int32_t* __restrict__ n_valid,
                                                     double* __restrict__ partials) {
    __shared__ double red[NT / 64][NSUM];
    const int img = blockIdx.y;
    if (n_valid[img] == 0) return;                     // k_eval_reduce does not read the rows of an empty image
    const float s = scale[img];
    const size_t base = (size_t)img * HW;
    const int p0 = blockIdx.x * PIX_PER_WG + threadIdx.x;
    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < PPT; j0 += U) {
        float gv[U], pr[U];
        bool in[U];
        load_px<U>(pred, gt, mask, base, p0 + j0 * NT, HW, gv, pr, in);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float g = gv[u];
            if (!(in[u] && g > lo && g < hi)) continue;
            const float pv = fminf(fmaxf(s * pr[u], lo), hi);
            const float d = g - pv;
            const float d2 = d * d;
            const float dl = logf(g) - logf(pv);
            acc[0] += __fdiv_rn(fabsf(d), g);
            acc[1] += __fdiv_rn(d2, g);
            acc[2] += d2;
            acc[3] += dl * dl;
            const float th = fmaxf(__fdiv_rn(g, pv), __fdiv_rn(pv, g));
            acc[4] += th < 1.25f ? 1.f : 0.f;
            acc[5] += th < 1.5625f ? 1.f : 0.f;
            acc[6] += th < 1.953125f ? 1.f : 0.f;
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int m = 0; m < 7; ++m) {
        double v = (double)acc[m];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) red[wv][m] = v;
    }
    __syncthreads();
    if (threadIdx.x < NSUM) {
        const int m = threadIdx.x;
        const double v = m < 7 ? (red[0][m] + red[1][m]) + (red[2][m] + red[3][m]) : 0.0;
        partials[((size_t)img * gridDim.x + blockIdx.x) * NSUM + m] = v;
    }
}

// grid N, 64 threads: lane m*8+g sums the rows g, g+8, ... of metric m in order; lane m*8 adds the eight in order
__global__ __launch_bounds__(64) void k_eval_reduce(const double* __restrict__ partials, int chunks,
                                                    const int32_t* __restrict__ n_valid, double* __restrict__ per_image) {
    const int img = blockIdx.x;
    const int m = threadIdx.x >> 3, g = threadIdx.x & 7;
    const int n = n_valid[img];
    const double* rows = partials + (size_t)img * chunks * NSUM;
    double v = 0.0;
    if (n > 0 && m < 7)
        for (int c = g; c < chunks; c += 8) v += rows[(size_t)c * NSUM + m];
    double tot = v;
#pragma unroll
    for (int k = 1; k < 8; ++k) tot += __shfl(v, (threadIdx.x & ~7) + k);
    if (g != 0 || m >= 7) return;
    double r = __builtin_nan("");
    if (n > 0) {
        r = tot / (double)n;
        if (m == 2 || m == 3) r = sqrt(r);             // rmse, rmse_log
    }
    per_image[(size_t)img * 7 + m] = r;
}

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" size_t colvo_depth_metrics_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || N > 65535 || H <= 0 || W <= 0 || (long long)H * W >= (1ll << 30)) return 0;
    return eval_ws(nullptr, N, eval_chunks(H, W)).bytes;
}

extern "C" int colvo_depth_metrics(const float* pred, const float* gt, const uint8_t* mask, int N, int H, int W, float min_depth,
                                   float max_depth, int median_scaling, void* workspace, double* per_image, float* scale,
                                   int32_t* n_valid, colvo_stream_t stream) {
    COLVO_CHECK_ARG(pred && gt && workspace && per_image && scale && n_valid, "colvo_depth_metrics: null pointer argument");
    COLVO_CHECK_ARG(N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 30),
                    "colvo_depth_metrics: bad shape N=%d H=%d W=%d", N, H, W);
    COLVO_CHECK_ARG(min_depth < max_depth, "colvo_depth_metrics: bad depth range (min_depth %g, max_depth %g)", (double)min_depth,
                    (double)max_depth);
    COLVO_CHECK_ARG(aligned16(workspace), "colvo_depth_metrics: workspace must be 16-byte aligned");
    const int HW = H * W, chunks = eval_chunks(H, W);
    const EvalWs ws = eval_ws(workspace, N, chunks);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(chunks, N);
    colvo::launch(k_eval_init, dim3(N), dim3(NT), 0, s, ws.hist, ws.state);
    COLVO_CHECK_LAUNCH("k_eval_init");
    const int passes = median_scaling ? 3 : 1;         // without scaling, pass 0 still counts the valid pixels
    for (int pass = 0; pass < passes; ++pass) {
        colvo::launch(k_eval_hist, grid, dim3(NT), 0, s, pred, gt, mask, HW, min_depth, max_depth, pass, ws.hist, ws.state);
        COLVO_CHECK_LAUNCH("k_eval_hist");
        colvo::launch(k_eval_select, dim3(N), dim3(NT), 0, s, ws.hist, ws.state, pass, (int)(pass == passes - 1), median_scaling,
                      scale, n_valid);
        COLVO_CHECK_LAUNCH("k_eval_select");
    }
    colvo::launch(k_eval_metrics, grid, dim3(NT), 0, s, pred, gt, mask, HW, min_depth, max_depth, scale, n_valid, ws.partials);
    COLVO_CHECK_LAUNCH("k_eval_metrics");
    colvo::launch(k_eval_reduce, dim3(N), dim3(64), 0, s, ws.partials, chunks, n_valid, per_image);
    COLVO_CHECK_LAUNCH("k_eval_reduce");
    return 0;
}
