// voxel_grid.h -- the voxel grid of the fusion and the walk over the samples of a set of depth maps, shared by
// fuse.hip, normals.hip and tsdf.hip so that all place a sample in its voxel with the very same routine: `locate` below is PINNED -- float32,
// every operation individually rounded, in the order written -- against tests/fuse_ref.py.  A file that includes this header must
// have contraction off (`#pragma clang fp contract(off)` in front of the include); the pragma below repeats it, and since a file-scope
// pragma holds to the end of the translation unit, everything behind the include is compiled without contraction as well.
#pragma once
#include "scene.h"

#pragma clang fp contract(off)

namespace colvo {
namespace voxel_grid {

constexpr int NT = 256;
constexpr int BRICK = 8;                   // voxels per brick edge
constexpr int BRICK_VOX = 512;
constexpr int TILE = 8;                    // a wave owns TILE x TILE samples: neighbouring pixels share voxels

struct Grid {
    float o[3];
    float inv;                             // float32(1) / float32(voxel_size), computed on the host
    int n[3];                              // voxels
    int nb[3];                             // bricks
};

struct Walk : StridedFrame {                // the samples of one frame as 8x8 tiles, one per wave
    int tiles_x, tiles, blocks_per_frame;
};

// sample (frame-local) of this thread; false beyond the image
__device__ __forceinline__ bool walk_pixel(const Walk& g, int& u, int& v) {
    const int tile = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    const int j = ty * TILE + (lane >> 3), i = tx * TILE + (lane & 7);
    u = i * g.stride;
    v = j * g.stride;
    return tile < g.tiles && i < g.Ws && j < g.Hs;
}

struct Voxel {
    int brick, local;                      // brick index in the grid, voxel index in the brick
    uint32_t q[3];                         // sub-voxel quanta, 0..255
};

// The pinned routine: world point, grid coordinate, voxel.  Returns whether the (kept) sample lies inside the grid.
__device__ __forceinline__ bool locate(const Cam& c, const Grid& G, float u, float v, float d, Voxel& vx) {
    const float px = __fdiv_rn(u - c.cx, c.fx) * d;
    const float py = __fdiv_rn(v - c.cy, c.fy) * d;
    bool inside = true;
    int idx[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float X = ((c.r[a * 3 + 0] * px + c.r[a * 3 + 1] * py) + c.r[a * 3 + 2] * d) + c.t[a];
        const float g = (X - G.o[a]) * G.inv;
        inside = inside && g >= 0.0f && g < (float)G.n[a];
        const float fl = floorf(g);
        idx[a] = inside ? (int)fl : 0;
        vx.q[a] = inside ? (uint32_t)(int)floorf((g - fl) * 256.0f) : 0u;
    }
    const int bx = idx[0] >> 3, by = idx[1] >> 3, bz = idx[2] >> 3;
    vx.brick = (bz * G.nb[1] + by) * G.nb[0] + bx;
    vx.local = ((idx[2] & 7) * BRICK + (idx[1] & 7)) * BRICK + (idx[0] & 7);
    return inside;
}

// a colour in [0, 1] as one of 256 quanta, summed as an integer by fuse.hip and tsdf.hip
__device__ __forceinline__ uint32_t colour_quantum(float c) {
    return (uint32_t)fminf(fmaxf(rintf(c * 255.0f), 0.0f), 255.0f);       // fmaxf(NaN, 0) = 0
}

// ---- host side: geometry ---------------------------------------------------------------------------------------------------- //
inline bool walk_geom(int N, int H, int W, int stride, Walk& g) {
    if (!strided_frame(N, H, W, stride, g)) return false;
    if ((long long)N * g.Hs * g.Ws >= (1ll << 31)) return false;             // the sample counters are int32
    g.tiles_x = blocks_of(g.Ws, TILE);
    g.tiles = g.tiles_x * blocks_of(g.Hs, TILE);
    g.blocks_per_frame = blocks_of(g.tiles, NT / 64);
    return true;
}

inline bool grid_dims(int nx, int ny, int nz, Grid& G) {
    const int n[3] = {nx, ny, nz};
    long long bricks = 1;
    for (int a = 0; a < 3; ++a) {
        if (n[a] <= 0 || n[a] % BRICK) return false;
        G.n[a] = n[a];
        G.nb[a] = n[a] / BRICK;
        bricks *= G.nb[a];
        if (bricks >= (1ll << 28)) return false;
    }
    return true;
}

inline bool grid_geom(float ox, float oy, float oz, float voxel_size, int nx, int ny, int nz, Grid& G) {
    if (!grid_dims(nx, ny, nz, G)) return false;
    if (!(voxel_size > 0.0f) || !(voxel_size < __builtin_inff()) || !(ox - ox == 0.0f) || !(oy - oy == 0.0f) || !(oz - oz == 0.0f))
        return false;
    G.o[0] = ox; G.o[1] = oy; G.o[2] = oz;
    G.inv = 1.0f / voxel_size;
    return G.inv > 0.0f && G.inv < __builtin_inff();
}

inline int total_bricks(const Grid& G) { return G.nb[0] * G.nb[1] * G.nb[2]; }

}  // namespace voxel_grid
}  // namespace colvo
