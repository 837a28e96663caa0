// scan.hip -- the library's ordered exclusive scan over int32 entries (contract: scene.h, struct Scan): chunk sums, one workgroup over
// the sums, in-chunk write-out.  No hash and no atomics, so whatever is numbered by it (the fusion's bricks and rows, the cloud index's
// cells, the stitched cloud's blocks) comes out in a fixed order.  Users: fuse.hip, cloud.hip, reconstruct.hip.
#include "scene.h"

namespace colvo {
namespace {

constexpr int NT = 256;
constexpr int PER_THREAD = SCAN_CHUNK / NT;
static_assert(PER_THREAD * NT == SCAN_CHUNK, "a chunk is 256 threads x 16 entries");

// the entries to scan (wave-uniform): the host's count, or the device word's, clamped to the bound the launch was sized for
__device__ __forceinline__ int scan_count(int n, const int32_t* __restrict__ n_dev) {
    if (n_dev == nullptr) return n;
    return min(max(__builtin_amdgcn_readfirstlane(*n_dev), 0), n - 1) + 1;
}

// grid scan_chunks(n): sums[chunk] = sum of the chunk's entries
__global__ __launch_bounds__(NT) void k_scan_chunk_sum(const int32_t* __restrict__ in, int n, const int32_t* __restrict__ n_dev,
                                                       int32_t* __restrict__ sums) {
    __shared__ int sm[NT / 64];
    n = scan_count(n, n_dev);
    const int base = blockIdx.x * SCAN_CHUNK;
    if (base >= n) return;
    int s = 0;
#pragma unroll
    for (int r = 0; r < PER_THREAD; ++r) {
        const int i = base + r * NT + threadIdx.x;
        if (i < n) s += in[i];
    }
    s = block_sum(s, sm);
    if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

// one workgroup: exclusive scan, in place, of n sums (with n_dev: of the chunks of the device count, whose bound is n_entries); their
// total -> *total (if given).  A thread takes `per` consecutive sums: more than one beyond 256 sums.
__global__ __launch_bounds__(NT) void k_scan_top(int32_t* __restrict__ sums, int n, const int32_t* __restrict__ n_dev, int n_entries,
                                                 int32_t* __restrict__ total) {
    __shared__ int part[NT];
    if (n_dev != nullptr) n = scan_chunks(scan_count(n_entries, n_dev));
    const int per = (n + NT - 1) / NT;
    const int lo = min((int)threadIdx.x * per, n), hi = min(lo + per, n);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += sums[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < NT; ++i) { const int t = part[i]; part[i] = run; run += t; }
        if (total != nullptr) *total = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int i = lo; i < hi; ++i) { const int t = sums[i]; sums[i] = run; run += t; }
}

// grid scan_chunks(n): entry i becomes the sum of the entries before it.  LIST: an entry is a mark; a marked entry becomes its slot
// and list[slot] = i, an unmarked one -1.
template <bool LIST>
__global__ __launch_bounds__(NT) void k_scan_chunk_write(int32_t* __restrict__ data, int n, const int32_t* __restrict__ n_dev,
                                                         const int32_t* __restrict__ offsets, int32_t* __restrict__ list, int list_cap) {
    __shared__ int wsum[NT / 64];
    n = scan_count(n, n_dev);
    if (blockIdx.x * SCAN_CHUNK >= n) return;
    const int base = blockIdx.x * SCAN_CHUNK + threadIdx.x * PER_THREAD;       // 16 consecutive entries per thread
    int v[PER_THREAD];
    int s = 0;
#pragma unroll
    for (int r = 0; r < PER_THREAD; ++r) {
        v[r] = base + r < n ? data[base + r] : 0;
        s += v[r];
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = s;                                                                // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int run = offsets[blockIdx.x] + inc - s;
    for (int i = 0; i < wv; ++i) run += wsum[i];
#pragma unroll
    for (int r = 0; r < PER_THREAD; ++r) {
        if (base + r >= n) break;
        if (LIST) {
            data[base + r] = v[r] ? run : -1;
            if (v[r] && run < list_cap) list[run] = base + r;
        } else {
            data[base + r] = run;
        }
        run += v[r];
    }
}

}  // namespace

int scan_exclusive(const Scan& a, hipStream_t stream) {
    const dim3 chunks(scan_chunks(a.n));
    launch(k_scan_chunk_sum, chunks, dim3(NT), 0, stream, a.data, a.n, a.n_dev, a.sums);
    COLVO_CHECK_LAUNCH("k_scan_chunk_sum");
    launch(k_scan_top, dim3(1), dim3(NT), 0, stream, a.sums, scan_chunks(a.n), a.n_dev, a.n, a.total);
    COLVO_CHECK_LAUNCH("k_scan_top");
    if (a.list != nullptr) launch(k_scan_chunk_write<true>, chunks, dim3(NT), 0, stream, a.data, a.n, a.n_dev, a.sums, a.list, a.list_cap);
    else launch(k_scan_chunk_write<false>, chunks, dim3(NT), 0, stream, a.data, a.n, a.n_dev, a.sums, (int32_t*)nullptr, 0);
    COLVO_CHECK_LAUNCH("k_scan_chunk_write");
    return 0;
}

int scan_sums(int32_t* sums, int n, int32_t* total, hipStream_t stream) {
    launch(k_scan_top, dim3(1), dim3(NT), 0, stream, sums, n, (const int32_t*)nullptr, 0, total);
    COLVO_CHECK_LAUNCH("k_scan_top");
    return 0;
}

}  // namespace colvo
