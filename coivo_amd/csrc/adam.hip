// adam.hip -- Adam over the flat arena (a8) and what shares its machinery: the weight-operand copies (k_pack_weights*, whose
// transpose tile k_adam_pack writes from the updated weights) and the several-buffers-in-one-launch zeroing (whose arena
// table k_adam_multi shares).
// Spec: oracle/colvo_spec.py (ADAM_KW).
#include "elem.h"
#include "tuning.h"

namespace colvo {
namespace {

// ---------------------------------------------------------------- weights -------------------- //
template <int ES>
__global__ __launch_bounds__(NT) void k_pack_weights(const float* __restrict__ w, int Cout, int kk, int Cin,
                                                     void* __restrict__ w_fwd, void* __restrict__ w_bwd) {
    const size_t n = (size_t)Cout * kk * Cin;
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % Cin);
    const int t = (int)((i / Cin) % kk);
    const int co = (int)(i / ((size_t)Cin * kk));
    const float v = w[i];
    if (w_fwd) Elem<ES>::st(w_fwd, i, v);
    if (w_bwd) Elem<ES>::st(w_bwd, ((size_t)c * kk + (kk - 1 - t)) * Cout + co, v);   // taps flipped
}

// One launch for all layers of a network: `tab` (device) holds, per layer, the element offsets of the master
// weights in the fp32 arena and of the two operand copies in their flat buffers, plus the first workgroup
// of the layer; every workgroup finds its layer by a scan of that small table.
struct PackEntry {
    long long w_off, fwd_off, bwd_off;
    int Cout, kk, Cin, blk_begin;
};
constexpr int PK_CO = 32, PK_C = 64;       // transpose tile: 32 output channels x 64 input channels of one tap
constexpr int ADAM_PLAIN_PER_WG = COLVO_ADAM_PLAIN_PER_WG;
typedef float PackTileLds[PK_CO][PK_C + 1];

// workgroup lb of a layer: tap t, first output channel co0 and first input channel c0 of its tile
struct PackTile { int t, co0, c0; };
__device__ __forceinline__ PackTile pack_tile(int lb, int Cout, int Cin) {
    const int nct = (Cin + PK_C - 1) / PK_C, ncot = (Cout + PK_CO - 1) / PK_CO;
    const int t = lb / (ncot * nct), r = lb - t * (ncot * nct);
    const int cot = r / nct, ct = r - cot * nct;
    return PackTile{t, cot * PK_CO, ct * PK_C};
}
// the tile, transposed, into the backward operand copy [Cin][kk][Cout]: stores run along Cout
template <int ES>
__device__ __forceinline__ void pack_tile_store_bwd(const PackTileLds& tile, const PackTile p, int Cout, int kk, int Cin,
                                                    void* bwd, long long bwd_off) {
    const int tid = threadIdx.x, co = p.co0 + (tid & 31);
#pragma unroll
    for (int i = 0; i < PK_C / 8; ++i) {
        const int col = (tid >> 5) + 8 * i, cc = p.c0 + col;
        if (co < Cout && cc < Cin)
            Elem<ES>::st(bwd, bwd_off + ((size_t)cc * kk + (kk - 1 - p.t)) * Cout + co, tile[tid & 31][col]);   // taps flipped
    }
}

template <int ES>
__global__ __launch_bounds__(NT) void k_pack_weights_multi(const float* __restrict__ master, const PackEntry* __restrict__ tab,
                                                           int nlayers, void* __restrict__ fwd, void* __restrict__ bwd) {
    // LDS-tiled transpose: reads (and the forward copy) run along Cin, the transposed copy is written along Cout --
    // the element-per-thread version scattered 2-byte stores at a stride of Cout and ran at ~1 TB/s
    __shared__ PackTileLds tile;
    int l = 0;
    for (int i = 1; i < nlayers; ++i)
        if ((int)blockIdx.x >= tab[i].blk_begin) l = i;
    const PackEntry e = tab[l];
    const PackTile p = pack_tile(blockIdx.x - e.blk_begin, e.Cout, e.Cin);
    const int t = p.t, co0 = p.co0, c0 = p.c0, tid = threadIdx.x;
    {
        const int cc = c0 + (tid & 63);
#pragma unroll
        for (int i = 0; i < PK_CO / 4; ++i) {
            const int row = (tid >> 6) + 4 * i, co = co0 + row;
            if (co < e.Cout && cc < e.Cin) {
                const size_t idx = ((size_t)co * e.kk + t) * e.Cin + cc;
                const float v = master[e.w_off + idx];
                tile[row][tid & 63] = v;
                if (fwd && e.fwd_off >= 0) Elem<ES>::st(fwd, e.fwd_off + idx, v);
            }
        }
    }
    __syncthreads();
    pack_tile_store_bwd<ES>(tile, p, e.Cout, e.kk, e.Cin, bwd, e.bwd_off);
}

// ---------------------------------------------------------------- arenas --------------------- //
// Several arenas in ONE launch (a dependent launch costs ~2.7 us before it does anything, tools/ubench/launch_floor.hip, and the
// small arena alone does not fill the memory system): workgroups [first[i], first[i + 1]) walk arena i.
struct ArenaGrid { int count; unsigned first[COLVO_MAX_ARENAS + 1]; };
struct ArenaBlocks { int i; unsigned b0, b1; };       // this workgroup's arena and that arena's workgroups [b0, b1)
__device__ __forceinline__ ArenaBlocks arena_of_block(const ArenaGrid& g) {
    int i = 0;
#pragma unroll
    for (int q = 1; q < COLVO_MAX_ARENAS; ++q)
        if (q < g.count && blockIdx.x >= g.first[q]) i = q;
    unsigned b0 = g.first[0], b1 = g.first[1];
#pragma unroll
    for (int q = 1; q < COLVO_MAX_ARENAS; ++q)
        if (i == q) { b0 = g.first[q]; b1 = g.first[q + 1]; }
    return ArenaBlocks{i, b0, b1};
}
// host: arena i gets blocks[i] workgroups, at least one; returns the grid
inline unsigned arena_layout(ArenaGrid& g, int count, const unsigned* blocks) {
    g.count = count;
    unsigned total = 0;
    for (int i = 0; i <= COLVO_MAX_ARENAS; ++i) {       // (the entries past `count` hold the grid's end)
        g.first[i] = total;
        if (i < count) total += blocks[i] ? blocks[i] : 1;
    }
    return total;
}

// ---------------------------------------------------------------- Adam ----------------------- //
// One thread updates 4 consecutive parameters (16-byte loads / stores: 48.1 -> 46.6 us per step for the two arenas; the entry
// points check the alignment).  (Measured and dropped: writing a bf16 mirror of the arena here as the forward operand copy and
// producing only the transposed copy in k_pack_weights_multi, on the side stream beside the forward pass -- Adam +3 us, the
// repacking pass -1 us, and the side-stream launch slowed the step by 0.6 %: DESIGN.md section 3.3.)
struct AdamCoef { float step_size, rs_bc2; };
__device__ __forceinline__ AdamCoef adam_coef(float lr, float b1, float b2, const int32_t* step_count, int t_host) {
    const int t = step_count ? step_count[0] + 1 : t_host;
    const float bc1 = 1.0f - powf(b1, (float)t);
    const float bc2 = 1.0f - powf(b2, (float)t);
    return AdamCoef{lr / bc1, 1.0f / sqrtf(bc2)};
}
__device__ __forceinline__ float adam_one(float& p, float g, float& m, float& v, float b1, float b2, float eps, float gscale,
                                          const AdamCoef c) {
    const float gi = g * gscale;
    m = b1 * m + (1.0f - b1) * gi;
    v = b2 * v + (1.0f - b2) * gi * gi;
    p -= c.step_size * (m / (sqrtf(v) * c.rs_bc2 + eps));
    return p;
}
// thread `start` of `stride`: the float4 body, then the tail (arenas of this library are multiples of 64 floats; other
// callers may pass any n)
__device__ __forceinline__ void adam_walk(float* p, const float* g, float* m, float* v, size_t n, size_t start, size_t stride, float b1,
                                          float b2, float eps, float gscale, const AdamCoef c) {
    const size_t n4 = n / 4;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    for (size_t i = start; i < n4; i += stride) {
        float4 pi = p4[i], mi = m4[i], vi = v4[i];
        const float4 gi = g4[i];
        adam_one(pi.x, gi.x, mi.x, vi.x, b1, b2, eps, gscale, c);
        adam_one(pi.y, gi.y, mi.y, vi.y, b1, b2, eps, gscale, c);
        adam_one(pi.z, gi.z, mi.z, vi.z, b1, b2, eps, gscale, c);
        adam_one(pi.w, gi.w, mi.w, vi.w, b1, b2, eps, gscale, c);
        m4[i] = mi;
        v4[i] = vi;
        p4[i] = pi;
    }
    for (size_t i = n4 * 4 + start; i < n; i += stride) {
        float pi = p[i], mi = m[i], vi = v[i];
        adam_one(pi, g[i], mi, vi, b1, b2, eps, gscale, c);
        m[i] = mi; v[i] = vi; p[i] = pi;
    }
}
__global__ __launch_bounds__(NT) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, size_t n, float lr, float b1, float b2, float eps,
                                             float gscale, const int32_t* __restrict__ step_count, int t_host) {
    const AdamCoef c = adam_coef(lr, b1, b2, step_count, t_host);
    adam_walk(p, g, m, v, n, (size_t)blockIdx.x * NT + threadIdx.x, (size_t)gridDim.x * NT, b1, b2, eps, gscale, c);
}

__global__ void k_inc_step(int32_t* step_count) { step_count[0] += 1; }

struct AdamArenas { ArenaGrid grid; ColvoAdamArena a[COLVO_MAX_ARENAS]; };
__global__ __launch_bounds__(NT) void k_adam_multi(AdamArenas as, float lr, float b1, float b2, float eps, float gscale, int t_host) {
    const AdamCoef c = adam_coef(lr, b1, b2, nullptr, t_host);
    const ArenaBlocks ab = arena_of_block(as.grid);
    ColvoAdamArena A = as.a[0];
#pragma unroll
    for (int q = 1; q < COLVO_MAX_ARENAS; ++q)
        if (ab.i == q) A = as.a[q];
    adam_walk(A.param, A.grad, A.exp_avg, A.exp_avg_sq, A.n, (size_t)(blockIdx.x - ab.b0) * NT + threadIdx.x,
              (size_t)(ab.b1 - ab.b0) * NT, b1, b2, eps, gscale, c);
}

// Adam AND the operand copies of the updated weights in one pass (both networks, one launch): the update has every new weight in
// a register, so the bf16 / transposed copies the next forward and backward pass read cost 4 more bytes per parameter here
// instead of a 12-byte-per-parameter repacking pass of their own (k_pack_weights_multi) plus its launches.  Table-driven like
// that kernel: an entry of kind 0 is one 3x3 layer's weights, walked in 32 x 64 transpose tiles of one tap; an entry of kind 1
// a plain range of the arena (biases, heads, padding) that only takes the update.  Same arithmetic as k_adam, element for element.
template <int ES>
__global__ __launch_bounds__(NT) void k_adam_pack(const ColvoAdamPackEntry* __restrict__ tab, int nentries, float lr, float b1,
                                                  float b2, float eps, float gscale_host, const float* __restrict__ gscale_dev,
                                                  const int32_t* __restrict__ step_count, int t_host) {
    __shared__ float tile[PK_CO][PK_C + 1];
    // gscale_dev: a second factor that is only known on the device (data parallel: world / max(3 n_valid of the WHOLE batch, 1), the
    // normaliser of raw loss gradients whose all-reduce overlapped the backward pass -- colvo_warp_loss_rescale_to)
    const float gscale = gscale_dev ? gscale_host * *gscale_dev : gscale_host;
    const AdamCoef c = adam_coef(lr, b1, b2, step_count, t_host);
    int l = 0;
    for (int i = 1; i < nentries; ++i)
        if ((int)blockIdx.x >= tab[i].blk_begin) l = i;
    const ColvoAdamPackEntry e = tab[l];
    const int lb = blockIdx.x - e.blk_begin, tid = threadIdx.x;
    float* __restrict__ P = e.param + e.w_off;
    float* __restrict__ G = const_cast<float*>(e.grad) + e.w_off;      // (written only where the entry asks for zeroed gradients)
    float* __restrict__ M = e.exp_avg + e.w_off;
    float* __restrict__ V = e.exp_avg_sq + e.w_off;
    const bool zg = e.zero_grad != 0;
    if (e.kind != 0) {                     // plain range: ADAM_PLAIN_PER_WG elements per workgroup
        const long long k0 = (long long)lb * ADAM_PLAIN_PER_WG;
        for (long long k = k0 + tid; k < e.n && k < k0 + ADAM_PLAIN_PER_WG; k += NT) {
            float pi = P[k], mi = M[k], vi = V[k];
            adam_one(pi, G[k], mi, vi, b1, b2, eps, gscale, c);
            M[k] = mi; V[k] = vi; P[k] = pi;
            if (zg) G[k] = 0.0f;
        }
        return;
    }
    const PackTile pt = pack_tile(lb, e.Cout, e.Cin);
    const int t = pt.t, co0 = pt.co0, c0 = pt.c0;
    {
        const int cc = c0 + (tid & 63);
        float pv[PK_CO / 4], gv[PK_CO / 4], mv[PK_CO / 4], vv[PK_CO / 4];
#pragma unroll
        for (int i = 0; i < PK_CO / 4; ++i) {           // all loads first: 32 in flight per thread
            const int co = co0 + (tid >> 6) + 4 * i;
            const bool ok = co < e.Cout && cc < e.Cin;
            const size_t idx = ok ? ((size_t)co * e.kk + t) * e.Cin + cc : 0;
            pv[i] = P[idx]; gv[i] = G[idx]; mv[i] = M[idx]; vv[i] = V[idx];
        }
#pragma unroll
        for (int i = 0; i < PK_CO / 4; ++i) {
            const int row = (tid >> 6) + 4 * i, co = co0 + row;
            if (co < e.Cout && cc < e.Cin) {
                const size_t idx = ((size_t)co * e.kk + t) * e.Cin + cc;
                adam_one(pv[i], gv[i], mv[i], vv[i], b1, b2, eps, gscale, c);
                M[idx] = mv[i]; V[idx] = vv[i]; P[idx] = pv[i];
                if (zg) G[idx] = 0.0f;
                tile[row][tid & 63] = pv[i];
                if (e.fwd && e.fwd_off >= 0) Elem<ES>::st(e.fwd, e.fwd_off + idx, pv[i]);
            }
        }
    }
    __syncthreads();
    pack_tile_store_bwd<ES>(tile, pt, e.Cout, e.kk, e.Cin, e.bwd, e.bwd_off);
}

// zero several buffers in one launch (16-byte stores; sizes are multiples of 16 bytes)
struct ZeroArenas { ArenaGrid grid; void* p[COLVO_MAX_ARENAS]; size_t n16[COLVO_MAX_ARENAS]; };
__global__ __launch_bounds__(NT) void k_zero_multi(ZeroArenas zs) {
    const ArenaBlocks ab = arena_of_block(zs.grid);
    void* p = zs.p[0]; size_t n16 = zs.n16[0];
#pragma unroll
    for (int q = 1; q < COLVO_MAX_ARENAS; ++q)
        if (ab.i == q) { p = zs.p[q]; n16 = zs.n16[q]; }
    float4* d = reinterpret_cast<float4*>(p);
    const size_t stride = (size_t)(ab.b1 - ab.b0) * NT;
    for (size_t k = (size_t)(blockIdx.x - ab.b0) * NT + threadIdx.x; k < n16; k += stride) d[k] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// one thread per four parameters, at most 4096 workgroups
inline unsigned adam_blocks(size_t n) {
    const unsigned blocks = nblk((n + 3) / 4);
    return blocks > 4096 ? 4096 : blocks;
}

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" int colvo_pack_weights(int dtype, const float* w_master, int Cout, int kk, int Cin, void* w_fwd,
                                  void* w_bwd, colvo_stream_t stream) {
    COLVO_CHECK_ARG(w_master && (w_fwd || w_bwd), "colvo_pack_weights: null pointer argument");
    COLVO_CHECK_DTYPE(dtype, "colvo_pack_weights");
    COLVO_CHECK_ARG(Cout > 0 && kk > 0 && Cin > 0, "colvo_pack_weights: bad shape");
    const size_t n = (size_t)Cout * kk * Cin;
    DISPATCH_ES(dtype, colvo::launch((k_pack_weights<ES>), dim3(nblk(n)), dim3(NT), 0, (hipStream_t)stream,
                                          w_master, Cout, kk, Cin, w_fwd, w_bwd));
    COLVO_CHECK_LAUNCH("k_pack_weights");
    return 0;
}

extern "C" int colvo_pack_weights_multi(int dtype, const float* master, const void* table, int nlayers, int nblocks,
                                        void* fwd, void* bwd, colvo_stream_t stream) {
    COLVO_CHECK_ARG(master && table && bwd && nlayers >= 1 && nblocks >= 1, "colvo_pack_weights_multi: bad arguments");
    COLVO_DISPATCH_ES(dtype, "colvo_pack_weights_multi",
                      colvo::launch((k_pack_weights_multi<ES>), dim3(nblocks), dim3(NT), 0, (hipStream_t)stream, master,
                                    (const PackEntry*)table, nlayers, fwd, bwd));
    COLVO_CHECK_LAUNCH("k_pack_weights_multi");
    return 0;
}

extern "C" int colvo_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                               float beta1, float beta2, float eps, float grad_scale, int32_t* step_count,
                               colvo_stream_t stream) {
    COLVO_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && step_count, "colvo_adam_step: null pointer argument");
    COLVO_CHECK_ARG(((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0,
                    "colvo_adam_step: arenas must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (n) {
        colvo::launch(k_adam, dim3(adam_blocks(n)), dim3(NT), 0, s, param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2,
                           eps, grad_scale, step_count, 0);
        COLVO_CHECK_LAUNCH("k_adam");
    }
    colvo::launch(k_inc_step, dim3(1), dim3(1), 0, s, step_count);
    COLVO_CHECK_LAUNCH("k_inc_step");
    return 0;
}

// The same with the step number t (1-based) supplied by the host: no device counter, no second launch.  For callers that count
// steps themselves; a step captured into a hipGraph needs the device counter of colvo_adam_step (a baked-in t would repeat).
extern "C" int colvo_adam_step_t(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                                 float beta1, float beta2, float eps, float grad_scale, int t, colvo_stream_t stream) {
    COLVO_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && t >= 1, "colvo_adam_step_t: bad arguments");
    COLVO_CHECK_ARG(((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0,
                    "colvo_adam_step_t: arenas must be 16-byte aligned");
    if (n == 0) return 0;
    colvo::launch(k_adam, dim3(adam_blocks(n)), dim3(NT), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n, lr, beta1,
                       beta2, eps, grad_scale, (const int32_t*)nullptr, t);
    COLVO_CHECK_LAUNCH("k_adam");
    return 0;
}

extern "C" int colvo_adam_step_multi(const ColvoAdamArena* arenas, int count, float lr, float beta1, float beta2, float eps,
                                     float grad_scale, int t, colvo_stream_t stream) {
    COLVO_CHECK_ARG(arenas && count >= 1 && count <= COLVO_MAX_ARENAS && t >= 1, "colvo_adam_step_multi: bad arguments");
    AdamArenas as{};
    unsigned blocks[COLVO_MAX_ARENAS];
    for (int i = 0; i < count; ++i) {
        const ColvoAdamArena& a = arenas[i];
        COLVO_CHECK_ARG(a.param && a.grad && a.exp_avg && a.exp_avg_sq, "colvo_adam_step_multi: null pointer in arena %d", i);
        COLVO_CHECK_ARG(((uintptr_t)a.param | (uintptr_t)a.grad | (uintptr_t)a.exp_avg | (uintptr_t)a.exp_avg_sq) % 16 == 0,
                        "colvo_adam_step_multi: arenas must be 16-byte aligned");
        as.a[i] = a;
        blocks[i] = adam_blocks(a.n);
    }
    const unsigned total = arena_layout(as.grid, count, blocks);
    colvo::launch(k_adam_multi, dim3(total), dim3(NT), 0, (hipStream_t)stream, as, lr, beta1, beta2, eps, grad_scale, t);
    COLVO_CHECK_LAUNCH("k_adam_multi");
    return 0;
}

extern "C" int colvo_adam_pack_step(int dtype, const void* table, int nentries, int nblocks, float lr, float beta1, float beta2,
                                    float eps, float grad_scale, int32_t* step_count, int t, colvo_stream_t stream) {
    return colvo_adam_pack_step_scaled(dtype, table, nentries, nblocks, lr, beta1, beta2, eps, grad_scale, nullptr, step_count, t, stream);
}

extern "C" int colvo_adam_pack_step_scaled(int dtype, const void* table, int nentries, int nblocks, float lr, float beta1, float beta2,
                                           float eps, float grad_scale, const float* grad_scale_dev, int32_t* step_count, int t,
                                           colvo_stream_t stream) {
    COLVO_CHECK_ARG(table && nentries >= 1 && nblocks >= 1 && (step_count || t >= 1), "colvo_adam_pack_step: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    COLVO_DISPATCH_ES(dtype, "colvo_adam_pack_step",
                      colvo::launch((k_adam_pack<ES>), dim3(nblocks), dim3(NT), 0, s, (const ColvoAdamPackEntry*)table, nentries,
                                    lr, beta1, beta2, eps, grad_scale, grad_scale_dev, (const int32_t*)step_count, t));
    COLVO_CHECK_LAUNCH("k_adam_pack");
    if (step_count) {
        colvo::launch(k_inc_step, dim3(1), dim3(1), 0, s, step_count);
        COLVO_CHECK_LAUNCH("k_inc_step");
    }
    return 0;
}

extern "C" int colvo_zero_multi(void* const* ptrs, const size_t* bytes, int count, colvo_stream_t stream) {
    COLVO_CHECK_ARG(ptrs && bytes && count >= 1 && count <= COLVO_MAX_ARENAS, "colvo_zero_multi: bad arguments");
    ZeroArenas zs{};
    unsigned blocks[COLVO_MAX_ARENAS];
    for (int i = 0; i < count; ++i) {
        COLVO_CHECK_ARG(ptrs[i] && (uintptr_t)ptrs[i] % 16 == 0 && bytes[i] % 16 == 0,
                        "colvo_zero_multi: buffer %d must be 16-byte aligned and a multiple of 16 bytes long", i);
        zs.p[i] = ptrs[i];
        zs.n16[i] = bytes[i] / 16;
        blocks[i] = nblk((zs.n16[i] + 3) / 4);          // four 16-byte stores per thread
        if (blocks[i] > 2048) blocks[i] = 2048;
    }
    const unsigned total = arena_layout(zs.grid, count, blocks);
    colvo::launch(k_zero_multi, dim3(total), dim3(NT), 0, (hipStream_t)stream, zs);
    COLVO_CHECK_LAUNCH("k_zero_multi");
    return 0;
}

extern "C" int colvo_zero(void* ptr, size_t bytes, colvo_stream_t stream) {
    COLVO_CHECK_ARG(ptr || bytes == 0, "colvo_zero: null pointer argument");
    if (bytes == 0) return 0;
    hipError_t e = hipMemsetAsync(ptr, 0, bytes, (hipStream_t)stream);
    if (e != hipSuccess) { set_error("colvo_zero: hipMemsetAsync failed: %s", hipGetErrorString(e)); return (int)e; }
    return 0;
}
