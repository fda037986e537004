// Section 21's sampling rule S (include/mgps_fields.h, "advection"), stated once for the units that sample a grid at a point: advection
// (mgps_advect.hip) and the particle update (mgps_particles.hip).  latticeOf says where a grid's nodes are and which planes are held,
// stencilAt gives S's indices and weights, combine the eight values and their least and greatest, sampleHeld reads them from the
// planes a call holds.
// mgps_tile_pass.h holds no floating-point code by rule; this header does, and pins its contraction itself: every function body
// below is compiled under `fp contract(off)`, whatever the including unit sets, and a product that feeds a sum is fused where, and only
// where, an fma is written out.  A point has the same bits wherever it is sampled.
#pragma once
#include <cmath>

#include "mgps_tile_pass.h"

#ifdef __HIPCC__
namespace mgps {

// Grid kinds: 0 = cells, 1 + a = faces of axis a.  n: the nodes of the WHOLE grid, o: the position of node (0, 0, 0); [w0, w1) the planes
// of the window and [h0, h1) the planes held, both in the whole grid's plane index
struct Lattice {
    int n[3];
    double o[3];
    int w0, w1, h0, h1;
};

// the lattice of a grid of `kind` on the window [c0, c0 + planes) of a grid of gx x gy x gz cells with `below` and `above` halo planes
// held; the whole grid: c0 = 0, planes = gz, no halo
__device__ __forceinline__ Lattice latticeOf(int gx, int gy, int gz, int c0, int planes, int below, int above, int kind)
{
    Lattice L;
    L.n[0] = gx + (kind == 1), L.n[1] = gy + (kind == 2), L.n[2] = gz + (kind == 3);
    L.o[0] = kind == 1 ? 0.0 : 0.5, L.o[1] = kind == 2 ? 0.0 : 0.5, L.o[2] = kind == 3 ? 0.0 : 0.5;
    L.w0 = c0, L.w1 = c0 + planes + (kind == 3);
    L.h0 = L.w0 - below, L.h1 = L.w1 + above;
    return L;
}

// the plane z (held) of a grid
__device__ __forceinline__ const float *planeOf(const HeldPlanes &h, const Lattice &L, int z)
{
    return heldPlane(h, size_t(L.n[0]) * size_t(L.n[1]), L.w0, L.w1, L.h0, z);
}

// S's indices and weights at the point p.  missed: a plane inside the grid that is not held was asked for; the nearest held one is read
struct Stencil {
    int i0[3], i1[3];
    double t[3];
    bool missed;
};

__device__ __forceinline__ Stencil stencilAt(const Lattice &L, double px, double py, double pz)
{
#pragma clang fp contract(off)
    Stencil s;
    const double p[3] = {px, py, pz};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double g = fmin(fmax(p[c] - L.o[c], 0.0), double(L.n[c] - 1));
        s.i0[c] = min(int(floor(g)), L.n[c] - 1);
        s.i1[c] = min(s.i0[c] + 1, L.n[c] - 1);
        s.t[c] = g - double(s.i0[c]);
    }
    s.missed = s.i0[2] < L.h0 || s.i1[2] >= L.h1;
    s.i0[2] = min(max(s.i0[2], L.h0), L.h1 - 1);
    s.i1[2] = min(max(s.i1[2], L.h0), L.h1 - 1);
    return s;
}

__device__ __forceinline__ double lerp(double t, double u, double v)
{
#pragma clang fp contract(off)
    return fma(t, v, (1.0 - t) * u);
}

// the eight values along x, then y, then z; lo and hi: the least and the greatest of them
__device__ __forceinline__ double combine(const Stencil &s, const float v[8], double &lo, double &hi)
{
#pragma clang fp contract(off)
    lo = hi = double(v[0]);
#pragma unroll
    for (int q = 1; q < 8; ++q) lo = fmin(lo, double(v[q])), hi = fmax(hi, double(v[q]));
    const double x00 = lerp(s.t[0], double(v[0]), double(v[1])), x10 = lerp(s.t[0], double(v[2]), double(v[3]));
    const double x01 = lerp(s.t[0], double(v[4]), double(v[5])), x11 = lerp(s.t[0], double(v[6]), double(v[7]));
    return lerp(s.t[2], lerp(s.t[1], x00, x10), lerp(s.t[1], x01, x11));
}

__device__ __forceinline__ double sampleHeld(const HeldPlanes &h, const Lattice &L, const Stencil &s, double &lo, double &hi)
{
    const float *p0 = planeOf(h, L, s.i0[2]), *p1 = planeOf(h, L, s.i1[2]);
    const size_t r0 = size_t(s.i0[1]) * size_t(L.n[0]), r1 = size_t(s.i1[1]) * size_t(L.n[0]);
    const float v[8] = {p0[r0 + s.i0[0]], p0[r0 + s.i1[0]], p0[r1 + s.i0[0]], p0[r1 + s.i1[0]],
                        p1[r0 + s.i0[0]], p1[r0 + s.i1[0]], p1[r1 + s.i0[0]], p1[r1 + s.i1[0]]};
    return combine(s, v, lo, hi);
}

}  // namespace mgps
#endif
