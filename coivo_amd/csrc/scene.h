// scene.h -- what the post-training kernels share about depth maps, cameras and frames, and the library's one
// ordered scan (csrc/scan.hip).  The world-point arithmetic is NOT here: the fusion (voxel_grid.h, shared by fuse.hip and normals.hip)
// and consistency.hip each pin their own operation order (no FMA contraction) against their own bit-exact replica under tests/; the
// renderers' camera point and footprint are in render_common.h.  reconstruct.hip's order is NOT pinned -- the compiler
// may contract its products and sums --: its world point is held to the float64 replica tests/reconstruct_ref.py within a bound
// derived from its operation count, 7 u (|r0 px| + |r1 py| + |r2 d| + |t|) with u = 2^-24.
#pragma once
#include "common.h"

namespace colvo {

// per frame: intrinsics and the camera-to-world transform, wave-uniform
struct Cam {
    float fx, fy, cx, cy;
    float r[9];
    float t[3];
};

__device__ __forceinline__ Cam load_cam(const float* __restrict__ K, const float* __restrict__ M, int b) {
    Cam c;
    const float* k = K + (size_t)b * 9;
    const float* m = M + (size_t)b * 16;
    c.fx = uniform_f(k[0]);
    c.fy = uniform_f(k[4]);
    c.cx = uniform_f(k[2]);
    c.cy = uniform_f(k[5]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c.r[i * 3 + j] = uniform_f(m[i * 4 + j]);
        c.t[i] = uniform_f(m[i * 4 + 3]);
    }
    return c;
}

// a depth that counts as a sample: 0 < d < max_depth; NaN falls out.  No short circuit: no branch.
__device__ __forceinline__ bool valid_depth(float d, float max_depth) { return (int)(d > 0.0f) & (int)(d < max_depth); }

// Every `stride`-th row and column of N frames of H x W pixels.  The shared limits: N <= 65535 (a grid's .y is the frame), H * W < 2^30
// (a pixel index, and a small multiple of it, stays in int32).  What else a walk needs (its tiling, a bound on its sample count) is
// the caller's, on top.
struct StridedFrame {
    int H, W, stride, Hs, Ws;
};

inline StridedFrame strided(int H, int W, int stride) {         // positive arguments, not checked
    return StridedFrame{H, W, stride, blocks_of(H, stride), blocks_of(W, stride)};
}

inline bool strided_frame(int N, int H, int W, int stride, StridedFrame& f) {
    if (N <= 0 || N > 65535 || H <= 0 || W <= 0 || stride <= 0 || (long long)H * W >= (1ll << 30)) return false;
    f = strided(H, W, stride);
    return true;
}

// A workgroup's share of K statistic counters that are striped over many lines, because every wave adding to ONE address queues the
// adds up behind each other (42 M samples into one pair: 7 ms, csrc/fuse.hip; the pitch and the number of lines are the caller's, with
// their own measurements).  Called by all 256 threads with the wave's K values (wave-uniform: ballot counts or wave sums): they go
// to LDS, the first K threads add the four waves' rows, and a total that is not zero is added to line[k].
template <typename T, int K>
__device__ __forceinline__ void striped_counter_add(const T (&v)[K], T (&sm)[4][K], T* __restrict__ line) {
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) sm[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const T t = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
        if (t) atomicAdd(&line[threadIdx.x], t);
    }
}

// ---- csrc/scan.hip: ordered exclusive scan over int32 entries, in place ------------------------------------------------------- //
constexpr int SCAN_CHUNK = 4096;           // entries one workgroup sums and writes
__host__ __device__ constexpr int scan_chunks(int n) { return (n + SCAN_CHUNK - 1) / SCAN_CHUNK; }

struct Scan {
    int32_t* data;                         // n entries; entry i becomes the sum of the entries before it
    int n;                                 // the count; with n_dev, the bound the launches are sized for (>= 1)
    const int32_t* n_dev;                  // NULL, or a device word c: the scan covers c entries and the one behind them (its prefix is
                                           // their total), min(max(c, 0), n - 1) + 1 in all -- whatever c holds, no index leaves
                                           // data[0..n) -- and the workgroups beyond that count leave at once
    int32_t* sums;                         // scan_chunks(n) words, written
    int32_t* total;                        // NULL, or where the sum of all entries goes
    int32_t* list;                         // NULL: plain write-out.  Else the entries are marks (0 / 1): a marked entry i becomes its
    int list_cap;                          // slot and list[slot] = i for slot < list_cap; an unmarked entry becomes -1
};

// k_scan_chunk_sum, k_scan_top, k_scan_chunk_write on `stream`; 0 or the launch's error code
int scan_exclusive(const Scan& a, hipStream_t stream);
// k_scan_top alone: n sums that the caller's own kernel counted (one per workgroup) become their exclusive prefixes; *total their sum
int scan_sums(int32_t* sums, int n, int32_t* total, hipStream_t stream);

}  // namespace colvo
