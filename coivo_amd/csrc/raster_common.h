// raster_common.h -- the triangle arithmetic of the mesh renderer (contract: include/colvo.h colvo_render_mesh): one
// set-up routine (camera points, classification, projection, snapping to the 1/256-pixel grid, area, orientation, bounding box), one
// fragment routine (the three edge functions at a pixel centre and the top-left rule) and the float64 interpolation weights.  The
// draw kernel and the resolve kernel of raster.hip both call THESE, so a winner's weights are recomputed with the bits it was drawn
// with.  Device functions only.  A file that includes this header must have contraction off in front of the include.
#pragma once
#include "render_common.h"                 // cam_point, Geom, the key buffer: shared with the point renderers, not copied

#pragma clang fp contract(off)

namespace colvo {
namespace raster {

using namespace render_common;

constexpr float GUARD = 16384.0f;          // |x|, |y| of every projected vertex: (int)rintf(x * 256) stays within 2^22
constexpr float SUBPIXELS = 256.0f;
constexpr int SUB_SHIFT = 8;

enum : int { TRI_FRONT = 1, TRI_STRADDLE = 2, TRI_OUTSIDE = 4, TRI_BACK = 8, TRI_DEGENERATE = 16, TRI_DRAWN = 32 };

// a face in one frame.  X, Y, Pz are in ORIENTED numbering (vertices 1 and 2 exchanged iff `swapped`), so that A > 0.
struct Tri {
    int X[3], Y[3];
    float Pz[3];
    long long A;
    int u_lo, u_hi, v_lo, v_hi;            // drawn: 0 <= u_lo <= u_hi < W and 0 <= v_lo <= v_hi < H; else empty (u_hi < u_lo)
    int flags;
    bool swapped;
};

// steps 1 to 4 of the contract up to the bounding box.  w: the nine world coordinates; P: the three camera points in the face's OWN
// numbering.  When no active lane has a front face the routine returns after the classification (flags is complete: a face that is
// not front has no other flag than TRI_STRADDLE).
__device__ __forceinline__ Tri setup(const Cam& c, const Geom& g, bool live, const float (&w)[9], int cull_back, CamPoint (&P)[3]) {
    Tri t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        P[k] = cam_point(c, g, live, w[3 * k], w[3 * k + 1], w[3 * k + 2]);
        t.X[k] = t.Y[k] = 0;
        t.Pz[k] = P[k].Pz;
    }
    const int nf = (int)P[0].front + (int)P[1].front + (int)P[2].front;
    const bool front = nf == 3;
    t.flags = front ? TRI_FRONT : nf > 0 ? TRI_STRADDLE : 0;
    t.A = 0;
    t.u_lo = t.v_lo = 0;
    t.u_hi = t.v_hi = -1;
    t.swapped = false;
    if (!__any((int)front)) return t;      // wave-uniform
    float x[3], y[3];
    bool in = front;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x[k] = (c.fx * P[k].Px) / P[k].Pz + c.cx;
        y[k] = (c.fy * P[k].Py) / P[k].Pz + c.cy;
        in = (int)in & (int)(fabsf(x[k]) <= GUARD) & (int)(fabsf(y[k]) <= GUARD);                  // NaN, inf fail
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {          // a face outside the band snaps zeros: every conversion sees a value within +-2^22
        t.X[k] = (int)rintf((in ? x[k] : 0.0f) * SUBPIXELS);
        t.Y[k] = (int)rintf((in ? y[k] : 0.0f) * SUBPIXELS);
    }
    const long long A = (long long)(t.X[1] - t.X[0]) * (t.Y[2] - t.Y[0]) - (long long)(t.X[2] - t.X[0]) * (t.Y[1] - t.Y[0]);
    const bool back = (int)in & (int)(A > 0), degenerate = (int)in & (int)(A == 0);
    t.flags |= ((int)front & (int)!in ? TRI_OUTSIDE : 0) | (back ? TRI_BACK : 0) | (degenerate ? TRI_DEGENERATE : 0);
    t.swapped = A < 0;
    t.A = A < 0 ? -A : A;
    if (t.swapped) {
        int i = t.X[1]; t.X[1] = t.X[2]; t.X[2] = i;
        i = t.Y[1]; t.Y[1] = t.Y[2]; t.Y[2] = i;
        const float z = t.Pz[1]; t.Pz[1] = t.Pz[2]; t.Pz[2] = z;
    }
    const int u_lo = max((min(min(t.X[0], t.X[1]), t.X[2]) + 255) >> SUB_SHIFT, 0);
    const int u_hi = min(max(max(t.X[0], t.X[1]), t.X[2]) >> SUB_SHIFT, g.W - 1);
    const int v_lo = max((min(min(t.Y[0], t.Y[1]), t.Y[2]) + 255) >> SUB_SHIFT, 0);
    const int v_hi = min(max(max(t.Y[0], t.Y[1]), t.Y[2]) >> SUB_SHIFT, g.H - 1);
    const bool drawn = (int)in & (int)(A != 0) & (int)!((int)back & (int)(cull_back != 0)) & (int)(u_lo <= u_hi) & (int)(v_lo <= v_hi);
    if (drawn) {
        t.flags |= TRI_DRAWN;
        t.u_lo = u_lo; t.u_hi = u_hi; t.v_lo = v_lo; t.v_hi = v_hi;
    }
    return t;
}

// the edge function of a -> b at p and whether p is owned: E > 0, or E == 0 on a top-left edge.  |d|, |p - a| <= 2^23: 32-bit
// differences, one 32 x 32 -> 64 product each
__device__ __forceinline__ bool edge(int ax, int ay, int bx, int by, int px, int py, long long& E) {
    const int dx = bx - ax, dy = by - ay;
    E = (long long)dx * (py - ay) - (long long)dy * (px - ax);
    const bool top_left = (int)(dy < 0) | ((int)(dy == 0) & (int)(dx > 0));
    return (int)(E > 0) | ((int)(E == 0) & (int)top_left);
}

// step 4 at the centre of pixel (u, v): e[k] is the edge function of the edge opposite (oriented) vertex k; -> covered
__device__ __forceinline__ bool fragment(const Tri& t, int u, int v, long long (&e)[3]) {
    const int px = u << SUB_SHIFT, py = v << SUB_SHIFT;
    const bool c0 = edge(t.X[1], t.Y[1], t.X[2], t.Y[2], px, py, e[0]);
    const bool c1 = edge(t.X[2], t.Y[2], t.X[0], t.Y[0], px, py, e[1]);
    const bool c2 = edge(t.X[0], t.Y[0], t.X[1], t.Y[1], px, py, e[2]);
    return (int)c0 & (int)c1 & (int)c2;
}

// step 5: the weights w_k = e_k * iz_k and their sum in the written association
struct Weights {
    double w[3], s;
};

__device__ __forceinline__ void inverse_depths(const Tri& t, double (&iz)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) iz[k] = 1.0 / (double)t.Pz[k];
}

__device__ __forceinline__ Weights weights(const long long (&e)[3], const double (&iz)[3]) {
    Weights q;
#pragma unroll
    for (int k = 0; k < 3; ++k) q.w[k] = (double)e[k] * iz[k];
    q.s = (q.w[0] + q.w[1]) + q.w[2];
    return q;
}

__device__ __forceinline__ float depth(const Tri& t, const Weights& q) { return (float)((double)t.A / q.s); }

}  // namespace raster
}  // namespace colvo
