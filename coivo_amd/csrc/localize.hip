// localize.hip -- labelled pixels + depth maps + trajectory -> where each polyp lies and how large it is.
// Contract: include/colvo.h (colvo_localize_*).  Which pixels are polyp is the caller's (a detector's) answer; this file turns
// that answer into positions.
//
//   accumulate  k_localize_accumulate: a workgroup walks 8192 pixels of ONE frame.  Labels are read for every pixel, depths only
//               where a wave holds a label.  The labelled lanes of a wave are grouped by label with a leader loop, every field is
//               reduced across the group and added to the workgroup's LDS table (one record per label) by adjacent lanes, one
//               word each.  At the end the workgroup adds its non-empty records to the frame's global records, again adjacent
//               lanes on adjacent words.
//   bounds      k_localize_bounds: records -> the clip interval of every (frame, label); a second accumulate applies it.
//   finish      k_localize_observations: one thread per (frame, label), records -> means and covariances in float64;
//               k_localize_polyps: one wave per label, the frames in ascending order.
//
// Every hand-off between passes is a kernel boundary.  A record holds integers only (counts, pixel sums, sums of 1/4096 quanta
// and of their products, a bounding box), added with native 64-bit adds and 32-bit max: a call's bits depend on nothing but its
// inputs.  The point arithmetic is pinned: float32, every operation individually rounded -- contraction is off for this whole
// file, which also pins the float64 expressions of the finish kernels.
#include "scene.h"

#pragma clang fp contract(off)

namespace colvo {
namespace {

constexpr int NT = 256;
constexpr int PPT = 32;                    // pixels per thread
constexpr int PIX_PER_WG = NT * PPT;       // 8192, as evaluate.hip
constexpr int U = 8;                       // label loads in flight per thread
static_assert(PPT % U == 0, "PPT is a multiple of U");
constexpr int MAX_LABELS = 255;
constexpr int REC_WORDS = 16;              // 64-bit words per record (128 B)
constexpr int N_SUMS = 13;                 // words 0..12 are sums; 13, 14 the bounding box; 15 unused
constexpr int BOX_WORD = 13;
constexpr int BOX_TOP = 0x7fffffff;        // the lower corner is kept as max(BOX_TOP - coordinate): a cleared record is all zeros
constexpr float QUANTUM = 4096.0f;

// one (frame, label):
//   w[0] labelled pixels   w[1] samples   w[2] sum u   w[3] sum v   (the sums over the samples)
//   w[4..6] sum q_x, q_y, q_z (two's complement)   w[7..12] sum q_x q_x, q_x q_y, q_x q_z, q_y q_y, q_y q_z, q_z q_z
//   w[13], w[14] as four int32: max(BOX_TOP - u), max(BOX_TOP - v), max(u), max(v) over the labelled pixels
struct Record {
    unsigned long long w[REC_WORDS];
};
static_assert(sizeof(Record) == 128, "Record is 128 B");

struct Walk : StridedFrame {
    int chunks;
};

bool walk_geom(int N, int H, int W, int stride, Walk& g) {
    if (!strided_frame(N, H, W, stride, g)) return false;
    g.chunks = blocks_of(g.Hs * g.Ws, PIX_PER_WG);
    return true;
}

bool labels_ok(int L) { return L >= 1 && L <= MAX_LABELS; }
bool depth_ok(float m) { return m > 0.0f && m < __builtin_inff(); }          // NaN fails

// workspace: records [N][L], then one 64-bit count of ignored pixels per frame
struct Ws {
    Record* records;
    unsigned long long* ignored;
    size_t bytes;
};

Ws layout(void* base, int N, int L) {
    Carver c(base);
    Ws w;
    w.records = c.take<Record>((size_t)N * L);
    w.ignored = c.take<unsigned long long>(N);
    w.bytes = c.bytes();
    return w;
}

// grid (chunks, N).  bounds: NULL, or per (frame, label) the pair (mean_z, limit) of k_localize_bounds.
__global__ __launch_bounds__(NT) void k_localize_accumulate(const float* __restrict__ depth, const uint8_t* __restrict__ labels,
                                                            const float* __restrict__ K, Walk g, float max_depth, int L,
                                                            const double* __restrict__ bounds, Record* __restrict__ records,
                                                            unsigned long long* __restrict__ ignored) {
    __shared__ unsigned long long tab[MAX_LABELS * REC_WORDS];
    __shared__ int n_ignored;
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < L * REC_WORDS; i += NT) tab[i] = 0ull;
    if (threadIdx.x == 0) n_ignored = 0;
    __syncthreads();
    const float* k = K + (size_t)b * 9;
    const float fx = uniform_f(k[0]), fy = uniform_f(k[4]), cx = uniform_f(k[2]), cy = uniform_f(k[5]);
    const size_t frame = (size_t)b * g.H * g.W;
    const int n_walked = g.Hs * g.Ws;
    const int p0 = blockIdx.x * PIX_PER_WG + threadIdx.x;
    int ignored_here = 0;                                        // wave-uniform
    for (int j0 = 0; j0 < PPT; j0 += U) {
        int off[U];
        uint8_t lv[U];
#pragma unroll
        for (int r = 0; r < U; ++r) {
            const int p = p0 + (j0 + r) * NT;
            off[r] = -1;
            if (p < n_walked) {
                if (g.stride == 1) {
                    off[r] = p;
                } else {
                    const int j = p / g.Ws;
                    off[r] = (j * g.W + (p - j * g.Ws)) * g.stride;
                }
            }
            lv[r] = labels[frame + (off[r] < 0 ? 0 : off[r])];  // beyond the walk: pixel 0, not used
        }
        float dv[U];
#pragma unroll
        for (int r = 0; r < U; ++r) {                            // the depths under the labels of this batch, all in flight together
            const int lab = off[r] < 0 ? 0 : (int)lv[r];
            dv[r] = lab >= 1 && lab <= L ? depth[frame + off[r]] : 0.0f;
        }
#pragma unroll
        for (int r = 0; r < U; ++r) {
            const int lab = off[r] < 0 ? 0 : (int)lv[r];
            const bool labelled = lab >= 1 && lab <= L;
            ignored_here += __popcll(__ballot(lab > L));
            unsigned long long remaining = __ballot(labelled);
            if (remaining == 0ull) continue;                     // most waves: background only
            const int v = labelled ? off[r] / g.W : 0, u = labelled ? off[r] - v * g.W : 0;
            const float d = dv[r];
            bool sample = labelled && d > 0.0f && d < max_depth;                 // NaN falls out
            int q[3] = {0, 0, 0};
            if (sample) {
                const float px = __fdiv_rn((float)u - cx, fx) * d;
                const float py = __fdiv_rn((float)v - cy, fy) * d;
                q[0] = (int)rintf(px * QUANTUM);
                q[1] = (int)rintf(py * QUANTUM);
                q[2] = (int)rintf(d * QUANTUM);
                if (bounds != nullptr) {
                    const double* bd = bounds + ((size_t)b * L + (lab - 1)) * 2;
                    const double dz = (double)q[2] / 4096.0 - bd[0];
                    sample = dz * dz <= bd[1];
                }
            }
            while (remaining != 0ull) {                          // one round per distinct label of the wave
                const int leader = __builtin_ctzll(remaining);
                const int lead_lab = __builtin_amdgcn_readlane(lab, leader);
                const bool same = labelled && lab == lead_lab;
                const bool mine = same && sample;
                remaining &= ~__ballot(same);
                const int n_samples = __popcll(__ballot(mine));
                unsigned long long w[N_SUMS];
                w[0] = (unsigned long long)__popcll(__ballot(same));
                w[1] = (unsigned long long)n_samples;
#pragma unroll
                for (int i = 2; i < N_SUMS; ++i) w[i] = 0ull;
                if (n_samples > 0) {
                    const long long qx = mine ? q[0] : 0, qy = mine ? q[1] : 0, qz = mine ? q[2] : 0;
                    w[2] = (unsigned long long)wave_sum(mine ? (long long)u : 0ll);
                    w[3] = (unsigned long long)wave_sum(mine ? (long long)v : 0ll);
                    w[4] = (unsigned long long)wave_sum(qx);
                    w[5] = (unsigned long long)wave_sum(qy);
                    w[6] = (unsigned long long)wave_sum(qz);
                    w[7] = (unsigned long long)wave_sum(qx * qx);
                    w[8] = (unsigned long long)wave_sum(qx * qy);
                    w[9] = (unsigned long long)wave_sum(qx * qz);
                    w[10] = (unsigned long long)wave_sum(qy * qy);
                    w[11] = (unsigned long long)wave_sum(qy * qz);
                    w[12] = (unsigned long long)wave_sum(qz * qz);
                }
                const int box[4] = {wave_max(same ? BOX_TOP - u : 0), wave_max(same ? BOX_TOP - v : 0), wave_max(same ? u : 0),
                                    wave_max(same ? v : 0)};
                // every lane holds the group's totals: lane i adds word i, lanes 16..19 the box
                unsigned long long mine_w = 0ull;
                int mine_box = 0;
#pragma unroll
                for (int i = 0; i < N_SUMS; ++i) mine_w = lane == i ? w[i] : mine_w;
#pragma unroll
                for (int i = 0; i < 4; ++i) mine_box = lane == 16 + i ? box[i] : mine_box;
                unsigned long long* rec = tab + (lead_lab - 1) * REC_WORDS;
                if (lane < N_SUMS && mine_w != 0ull) atomicAdd(&rec[lane], mine_w);
                if (lane >= 16 && lane < 20) atomicMax(reinterpret_cast<int*>(rec + BOX_WORD) + (lane - 16), mine_box);
            }
        }
    }
    if (lane == 0 && ignored_here != 0) atomicAdd(&n_ignored, ignored_here);
    __syncthreads();
    // the non-empty records: word i of a record by lane i of a group of 16
    Record* out = records + (size_t)b * L;
    for (int i = threadIdx.x; i < L * REC_WORDS; i += NT) {
        const int rec = i / REC_WORDS, word = i % REC_WORDS;
        if (tab[rec * REC_WORDS] == 0ull) continue;              // no labelled pixel in this workgroup
        const unsigned long long val = tab[i];
        if (word < N_SUMS) {
            if (val != 0ull) atomicAdd(&out[rec].w[word], val);
        } else if (word < BOX_WORD + 2) {
            int* dst = reinterpret_cast<int*>(&out[rec].w[word]);
            atomicMax(dst, (int)(uint32_t)val);
            atomicMax(dst + 1, (int)(uint32_t)(val >> 32));
        }
    }
    if (threadIdx.x == 0 && n_ignored != 0) atomicAdd(&ignored[b], (unsigned long long)n_ignored);
}

// one thread per (frame, label): mean_z and limit = double(float(k))^2 * var_z; with fewer than two samples nothing is clipped
__global__ __launch_bounds__(NT) void k_localize_bounds(const Record* __restrict__ records, int n_records, float clip_sigma,
                                                        double* __restrict__ bounds) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n_records) return;
    const long long n = (long long)records[i].w[1];
    double mean = 0.0, limit = __builtin_inf();
    if (n >= 2) {
        const double dn = (double)n;
        mean = (double)(long long)records[i].w[6] / (4096.0 * dn);
        const double var = fmax(0.0, (double)(long long)records[i].w[12] / (16777216.0 * dn) - mean * mean);
        const double k = (double)clip_sigma;
        limit = (k * k) * var;
    }
    bounds[(size_t)i * 2] = mean;
    bounds[(size_t)i * 2 + 1] = limit;
}

struct ObsOut {                            // per (frame, label)
    int32_t* n_pixels;                     // [N,L]
    int32_t* n_samples;                    // [N,L]
    int32_t* bbox;                         // [N,L,4]
    double* pixel;                         // [N,L,2]
    double* center_cam;                    // [N,L,3]
    double* cov_cam;                       // [N,L,6]
    double* center_world;                  // [N,L,3]
};

struct PolypOut {                          // per label
    int32_t* n_frames;                     // [L]
    long long* n_samples_total;            // [L]
    int32_t* first_frame;                  // [L]
    int32_t* last_frame;                   // [L]
    double* position;                      // [L,3]
    double* cov_world;                     // [L,6]
};

// the six entries xx, xy, xz, yy, yz, zz as rows and columns
__device__ __forceinline__ int sym(int a, int b) {
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return lo == 0 ? hi : lo + hi + 1;     // (0,0) 0 (0,1) 1 (0,2) 2 (1,1) 3 (1,2) 4 (2,2) 5
}

__global__ __launch_bounds__(NT) void k_localize_observations(const Record* __restrict__ records, const float* __restrict__ M,
                                                              int n_records, int L, ObsOut o, long long* __restrict__ stats) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i == 0) { stats[0] = 0; stats[1] = 0; }                  // k_localize_polyps adds into them
    if (i >= n_records) return;
    const Record& r = records[i];
    const long long n_pix = (long long)r.w[0], n = (long long)r.w[1];
    o.n_pixels[i] = (int32_t)n_pix;
    o.n_samples[i] = (int32_t)n;
    const int* box = reinterpret_cast<const int*>(&r.w[BOX_WORD]);
    o.bbox[(size_t)i * 4 + 0] = n_pix > 0 ? BOX_TOP - box[0] : -1;
    o.bbox[(size_t)i * 4 + 1] = n_pix > 0 ? BOX_TOP - box[1] : -1;
    o.bbox[(size_t)i * 4 + 2] = n_pix > 0 ? box[2] : -1;
    o.bbox[(size_t)i * 4 + 3] = n_pix > 0 ? box[3] : -1;
    const double nan = __builtin_nan("");
    double pixel[2] = {nan, nan}, m[3] = {nan, nan, nan}, cov[6] = {nan, nan, nan, nan, nan, nan}, cw[3] = {nan, nan, nan};
    if (n > 0) {
        const double dn = (double)n;
        pixel[0] = (double)(long long)r.w[2] / dn;
        pixel[1] = (double)(long long)r.w[3] / dn;
#pragma unroll
        for (int a = 0; a < 3; ++a) m[a] = (double)(long long)r.w[4 + a] / (4096.0 * dn);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = a; b < 3; ++b) cov[sym(a, b)] = (double)(long long)r.w[7 + sym(a, b)] / (16777216.0 * dn) - m[a] * m[b];
        const float* mat = M + (size_t)(i / L) * 16;
#pragma unroll
        for (int a = 0; a < 3; ++a)
            cw[a] = (((double)mat[a * 4 + 0] * m[0] + (double)mat[a * 4 + 1] * m[1]) + (double)mat[a * 4 + 2] * m[2]) + (double)mat[a * 4 + 3];
    }
    o.pixel[(size_t)i * 2 + 0] = pixel[0];
    o.pixel[(size_t)i * 2 + 1] = pixel[1];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o.center_cam[(size_t)i * 3 + a] = m[a];
        o.center_world[(size_t)i * 3 + a] = cw[a];
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) o.cov_cam[(size_t)i * 6 + e] = cov[e];
}

// grid L, one wave.  64 frames at a time: lane f evaluates frame f's terms, then lanes 0..8 add their component of the 64 frames
// in ascending frame order; lane 9 keeps the integer sums.  A frame below min_samples is skipped.  Its term is stored as +0.0 and
// added like the others, which leaves the same bits: the sum starts at +0.0 and can never become -0.0 (x + (-x) and
// (+0.0) + (-0.0) are +0.0 under round-to-nearest), and y + (+0.0) == y for every other y.  So the loop has no branch and its LDS
// reads run ahead of the additions.
__global__ __launch_bounds__(64) void k_localize_polyps(const float* __restrict__ M, int N, int L, int min_samples, ObsOut o,
                                                        PolypOut out, const unsigned long long* __restrict__ ignored,
                                                        long long* __restrict__ stats) {
    __shared__ double term[64][9];
    __shared__ long long count[64];
    __shared__ long long pixels[64];
    __shared__ double pos[3];
    __shared__ long long total_s;
    const int l = blockIdx.x, lane = threadIdx.x;
    double acc = 0.0;
    long long total = 0, n_pix = 0, n_ign = 0;
    int n_frames = 0, first = -1, last = -1;
    for (int f0 = 0; f0 < N; f0 += 64) {
        const int f = f0 + lane;
        long long n = 0, np = 0;
        double t[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (f < N) {
            const size_t i = (size_t)f * L + l;
            np = o.n_pixels[i];
            n = o.n_samples[i];
            if (l == 0) n_ign += (long long)ignored[f];
            if (n >= min_samples) {
                const double dn = (double)n;
                const float* mat = M + (size_t)f * 16;
                double R[3][3], C[3][3], T[3][3], c[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    c[a] = o.center_world[i * 3 + a];
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        R[a][b] = (double)mat[a * 4 + b];
                        C[a][b] = o.cov_cam[i * 6 + sym(a, b)];
                    }
                }
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) T[a][b] = (R[a][0] * C[0][b] + R[a][1] * C[1][b]) + R[a][2] * C[2][b];
#pragma unroll
                for (int a = 0; a < 3; ++a) t[a] = dn * c[a];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = a; b < 3; ++b) {
                        const double rcr = (T[a][0] * R[b][0] + T[a][1] * R[b][1]) + T[a][2] * R[b][2];
                        t[3 + sym(a, b)] = dn * (rcr + c[a] * c[b]);
                    }
            } else {
                n = 0;
            }
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) term[lane][e] = t[e];
        count[lane] = n;
        pixels[lane] = np;
        __syncthreads();
        const int here = min(64, N - f0);
        if (lane < 9) {
#pragma unroll 16
            for (int i = 0; i < 64; ++i) acc = acc + term[i][lane];          // (frames beyond N: +0.0 as well)
        } else if (lane == 9) {
            for (int i = 0; i < here; ++i) {
                n_pix += pixels[i];
                if (count[i] > 0) {
                    total += count[i];
                    ++n_frames;
                    if (first < 0) first = f0 + i;
                    last = f0 + i;
                }
            }
        }
        __syncthreads();
    }
    if (l == 0) {                                                // the ignored pixels of all frames: an integer sum
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) n_ign += __shfl_xor(n_ign, off);
        if (lane == 0 && n_ign != 0) atomicAdd(reinterpret_cast<unsigned long long*>(stats + 1), (unsigned long long)n_ign);
    }
    if (lane == 9) {
        total_s = total;
        out.n_frames[l] = n_frames;
        out.n_samples_total[l] = total;
        out.first_frame[l] = first;
        out.last_frame[l] = last;
        if (n_pix != 0) atomicAdd(reinterpret_cast<unsigned long long*>(stats), (unsigned long long)n_pix);
    }
    __syncthreads();
    const double dt = (double)total_s;
    const bool seen = total_s > 0;
    const double mean = seen ? acc / dt : __builtin_nan("");
    if (lane < 3) {
        pos[lane] = mean;
        out.position[(size_t)l * 3 + lane] = mean;
    }
    __syncthreads();
    if (lane >= 3 && lane < 9) {
        const int e = lane - 3;
        const int a = e < 3 ? 0 : e < 5 ? 1 : 2, b = e < 3 ? e : e < 5 ? e - 2 : 2;
        out.cov_world[(size_t)l * 6 + e] = seen ? mean - pos[a] * pos[b] : __builtin_nan("");
    }
}

}  // namespace
}  // namespace colvo

using namespace colvo;

extern "C" size_t colvo_localize_workspace_bytes(int N, int num_labels) {
    if (N <= 0 || N > 65535 || !labels_ok(num_labels)) return 0;
    return layout(nullptr, N, num_labels).bytes;
}

extern "C" int colvo_localize_accumulate(const float* depths, const uint8_t* labels, const float* K, int N, int H, int W, int stride,
                                         float max_depth, int num_labels, const double* clip_bounds, void* records,
                                         colvo_stream_t stream) {
    COLVO_CHECK_ARG(depths && labels && K && records, "colvo_localize_accumulate: null pointer argument");
    Walk g;
    COLVO_CHECK_ARG(walk_geom(N, H, W, stride, g), "colvo_localize_accumulate: bad shape N=%d H=%d W=%d stride=%d", N, H, W, stride);
    COLVO_CHECK_ARG(labels_ok(num_labels), "colvo_localize_accumulate: bad num_labels %d (1 .. 255)", num_labels);
    COLVO_CHECK_ARG(depth_ok(max_depth), "colvo_localize_accumulate: bad max_depth %g (finite, positive)", (double)max_depth);
    COLVO_CHECK_ARG(aligned16(records) && aligned16(clip_bounds), "colvo_localize_accumulate: records and clip_bounds must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const Ws w = layout(records, N, num_labels);
    COLVO_CHECK_HIP(hipMemsetAsync(records, 0, w.bytes, s), "colvo_localize_accumulate");
    colvo::launch(k_localize_accumulate, dim3(g.chunks, N), dim3(NT), 0, s, depths, labels, K, g, max_depth, num_labels, clip_bounds,
                  w.records, w.ignored);
    COLVO_CHECK_LAUNCH("k_localize_accumulate");
    return 0;
}

extern "C" int colvo_localize_bounds(const void* records, int N, int num_labels, float clip_sigma, double* clip_bounds,
                                     colvo_stream_t stream) {
    COLVO_CHECK_ARG(records && clip_bounds, "colvo_localize_bounds: null pointer argument");
    COLVO_CHECK_ARG(N > 0 && N <= 65535, "colvo_localize_bounds: bad shape N=%d", N);
    COLVO_CHECK_ARG(labels_ok(num_labels), "colvo_localize_bounds: bad num_labels %d (1 .. 255)", num_labels);
    COLVO_CHECK_ARG(clip_sigma >= 0.0f && clip_sigma < __builtin_inff(), "colvo_localize_bounds: bad clip_sigma %g (finite, not negative)",
                    (double)clip_sigma);
    COLVO_CHECK_ARG(aligned16(records) && aligned16(clip_bounds), "colvo_localize_bounds: records and clip_bounds must be 16-byte aligned");
    const int n = N * num_labels;
    colvo::launch(k_localize_bounds, dim3(blocks_of(n, NT)), dim3(NT), 0, (hipStream_t)stream, static_cast<const Record*>(records), n,
                  clip_sigma, clip_bounds);
    COLVO_CHECK_LAUNCH("k_localize_bounds");
    return 0;
}

extern "C" int colvo_localize_finish(const void* records, const float* cam2world, int N, int num_labels, int min_samples,
                                     int32_t* n_pixels, int32_t* n_samples, int32_t* bbox, double* pixel, double* center_cam,
                                     double* cov_cam, double* center_world, int32_t* n_frames, int64_t* n_samples_total,
                                     int32_t* first_frame, int32_t* last_frame, double* position, double* cov_world, int64_t* stats,
                                     colvo_stream_t stream) {
    COLVO_CHECK_ARG(records && cam2world && n_pixels && n_samples && bbox && pixel && center_cam && cov_cam && center_world && n_frames &&
                        n_samples_total && first_frame && last_frame && position && cov_world && stats,
                    "colvo_localize_finish: null pointer argument");
    COLVO_CHECK_ARG(N > 0 && N <= 65535, "colvo_localize_finish: bad shape N=%d", N);
    COLVO_CHECK_ARG(labels_ok(num_labels), "colvo_localize_finish: bad num_labels %d (1 .. 255)", num_labels);
    COLVO_CHECK_ARG(min_samples >= 1, "colvo_localize_finish: bad min_samples %d (>= 1)", min_samples);
    COLVO_CHECK_ARG(aligned16(records), "colvo_localize_finish: records must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int n = N * num_labels;
    const ObsOut o{n_pixels, n_samples, bbox, pixel, center_cam, cov_cam, center_world};
    const PolypOut p{n_frames, reinterpret_cast<long long*>(n_samples_total), first_frame, last_frame, position, cov_world};
    const Ws w = layout(const_cast<void*>(records), N, num_labels);
    colvo::launch(k_localize_observations, dim3(blocks_of(n, NT)), dim3(NT), 0, s, (const Record*)w.records, cam2world, n, num_labels, o,
                  reinterpret_cast<long long*>(stats));
    COLVO_CHECK_LAUNCH("k_localize_observations");
    colvo::launch(k_localize_polyps, dim3(num_labels), dim3(64), 0, s, cam2world, N, num_labels, min_samples, o, p,
                  (const unsigned long long*)w.ignored, reinterpret_cast<long long*>(stats));
    COLVO_CHECK_LAUNCH("k_localize_polyps");
    return 0;
}
