// Plugin-side field pre/post-processing on the device (include/mgps_fields.h).
// Every pass is one thread per cell or face over a dense x-fastest grid: consecutive lanes read consecutive
// addresses of every input, HBM-bound streaming kernels with a handful of bytes per cell.  No reference
// counterpart of the layout: the reference walks 16^3 tiles of UT_VoxelArray on the host (Plug.cpp:716-1207).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "mgps_fields.h"
#include "mgps_internal.h"
#include "mgps_slab_call.h"

using namespace mgps;

namespace {

enum : int { kSolid = 0, kLiquid = 1, kAir = 2 };  // Util.h:17

struct Box {
    int gx, gy, gz;
    __host__ __device__ size_t cells() const { return size_t(gx) * gy * gz; }
};

__device__ __forceinline__ size_t cellAt(const Box &g, int i, int j, int k) { return (size_t(k) * g.gy + j) * g.gx + i; }
__device__ __forceinline__ size_t faceAt(const Box &g, int axis, int i, int j, int k)
{
    return (size_t(k) * (g.gy + (axis == 1)) + j) * (g.gx + (axis == 0)) + i;
}
// cellToFaceMap(cell, axis, dir)
__device__ __forceinline__ size_t cellFace(const Box &g, int axis, int dir, int i, int j, int k)
{
    return faceAt(g, axis, i + (axis == 0 && dir), j + (axis == 1 && dir), k + (axis == 2 && dir));
}
__device__ __forceinline__ float ghostFluidTheta(float phi0, float phi1)  // Util.h:25-42 + the clamp of Plug.cpp:850-851
{
    float theta = 0.f;
    if (phi0 < 0.f) theta = phi1 < 0.f ? 1.f : phi0 / (phi0 - phi1);
    else if (phi1 < 0.f) theta = phi1 / (phi1 - phi0);
    return fminf(fmaxf(theta, 0.01f), 1.f);
}
// thread -> (i, j, k) of a grid of extents (nx, ny, nz); false past the end
__device__ __forceinline__ bool unflatten(int nx, int ny, int nz, int &i, int &j, int &k)
{
    const size_t t = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= size_t(nx) * ny * nz) return false;
    i = int(t % nx);
    j = int((t / nx) % ny);
    k = int(t / (size_t(nx) * ny));
    return true;
}
// (i, j, k) of this thread in a rowGrid(nx, ny, nz) launch: no 64-bit division for the index; i may lie past the row's end
__device__ __forceinline__ void threadCell(int &i, int &j, int &k)
{
    i = int(blockIdx.x * blockDim.x + threadIdx.x);
    j = int(blockIdx.y);
    k = int(blockIdx.z);
}
inline dim3 rowGrid(int nx, int ny, int nz) { return dim3(unsigned((nx + 255) / 256), unsigned(ny), unsigned(nz)); }

// ---- the per-cell rules, each stated once for the whole-grid kernels and the slab kernels ----------
// A rule is templated on how the value of a cell other than the thread's own is reached: `at(i, j, k)`, (i, j, k) a cell of the
// WHOLE grid G.  The whole-grid kernels pass GridAt, which indexes the array; the slab kernels pass SlabAt (below), which goes
// through the window and its halo planes.  A rule asks only for cells inside G, and only on the branch where it needs the value:
// nothing is fetched that the kernel would not have fetched with the rule written out in it.
template <class T>
struct GridAt {
    const Box &g;
    const T *a;
    __device__ __forceinline__ T operator()(int i, int j, int k) const { return a[cellAt(g, i, j, k)]; }
};
// the same for cells next to the thread's own cell (ci, cj, ck) = c: the index is c plus strides, no product per cell asked for
template <class T>
struct GridNear {
    const Box &g;
    const T *a;
    size_t c;
    int ci, cj, ck;
    __device__ __forceinline__ T operator()(int i, int j, int k) const
    {
        return a[ptrdiff_t(c) + (i - ci) + ptrdiff_t(j - cj) * g.gx + ptrdiff_t(k - ck) * (ptrdiff_t(g.gx) * g.gy)];
    }
};

// Material label of cell (i, j, k) of the box g its own arrays (phi, solidPhi, the cut weights) are indexed in -- the grid G or a
// window of its planes -- which is cell (i, j, kg) of G.  phiAt reaches the 6-neighbours' liquid phi.  (The own arrays as pointers
// and the face loop in here: with the cut weights and the own values handed in through a functor and references the slab kernel
// measured 7 % slower, LABNOTES R10.)
template <class PhiAt>
__device__ __forceinline__ int materialLabel(const Box &G, const Box &g, int i, int j, int k, int kg, const float *phi,
                                             const float *solidPhi, const float *const cw[3], PhiAt phiAt)
{
    const int ext[3] = {G.gx, G.gy, G.gz};
    const size_t c = cellAt(g, i, j, k);
    bool open[3][2], inFluid = false;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            open[a][d] = cw[a][cellFace(g, a, d, i, j, k)] > 0.f;
            inFluid = inFluid || open[a][d];
        }
    if (!inFluid) return kSolid;
    bool liquid = phi[c] <= 0.f;
    if (!liquid && solidPhi[c] >= 0.f) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                int n[3] = {i, j, kg};
                n[a] += d ? 1 : -1;
                if (open[a][d] && n[a] >= 0 && n[a] < ext[a] && phiAt(n[0], n[1], n[2]) <= 0.f) liquid = true;
            }
    }
    return liquid ? kLiquid : kAir;
}

// The face of `axis` in front of cell (i, j, k) of G, cut weight cwf, is valid when it is open, has both cells in G and one is
// LIQUID.  mb / mf: the labels of the cell behind and in front, loaded when the face is open and both cells are in G.
template <class MatAt>
__device__ __forceinline__ bool isValidFace(const Box &G, int axis, int i, int j, int k, float cwf, MatAt mat, int &mb, int &mf)
{
    const int ext[3] = {G.gx, G.gy, G.gz};
    int b[3] = {i, j, k}, fw[3] = {i, j, k};
    b[axis] -= 1;
    if (!(cwf > 0.f && b[axis] >= 0 && fw[axis] < ext[axis])) return false;
    mb = mat(b[0], b[1], b[2]), mf = mat(fw[0], fw[1], fw[2]);
    return mb == kLiquid || mf == kLiquid;
}
// Expanded weight of that face, known to be valid: the cut weight, over theta on a liquid/air face.
template <class PhiAt>
__device__ __forceinline__ float expandedWeight(int axis, int i, int j, int k, float cwf, int mb, int mf, PhiAt phi)
{
    int b[3] = {i, j, k};
    b[axis] -= 1;
    float w = cwf;
    if ((mb == kLiquid && mf == kAir) || (mb == kAir && mf == kLiquid)) w /= ghostFluidTheta(phi(b[0], b[1], b[2]), phi(i, j, k));
    return w;
}

// material label -> domain label
__device__ __forceinline__ int domainLabel(int m)
{
    return m == kLiquid ? MGPS_INTERIOR_CELL : m == kAir ? MGPS_DIRICHLET_CELL : MGPS_EXTERIOR_CELL;
}
// An INTERIOR cell, (i, j, k) of the expanded box e, becomes BOUNDARY next to a DIRICHLET or EXTERIOR cell or at a face whose
// expanded weight is not 1.  labelAcross(a, d) is the domain label of the 6-neighbour across face (a, d).
template <class LabelAcross>
__device__ __forceinline__ bool isBoundaryCell(const Box &e, int i, int j, int k, const float *const w[3], LabelAcross labelAcross)
{
    bool bnd = false;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const int nl = labelAcross(a, d);
            bnd = bnd || nl == MGPS_DIRICHLET_CELL || nl == MGPS_EXTERIOR_CELL || w[a][cellFace(e, a, d, i, j, k)] != 1.f;
        }
    return bnd;
}

// Cell (i, j, k) of G with label m is an interface cell: LIQUID or AIR with a 6-neighbour of the other kind (the six labels are
// loaded together, not one after the other; an out-of-grid neighbour reads the cell itself: never `other`)
template <class MatAt>
__device__ __forceinline__ bool isInterfaceCell(const Box &G, int i, int j, int k, int m, MatAt mat)
{
    const int n[6] = {mat(i > 0 ? i - 1 : i, j, k), mat(i + 1 < G.gx ? i + 1 : i, j, k), mat(i, j > 0 ? j - 1 : j, k),
                      mat(i, j + 1 < G.gy ? j + 1 : j, k), mat(i, j, k > 0 ? k - 1 : k), mat(i, j, k + 1 < G.gz ? k + 1 : k)};
    const int other = m == kLiquid ? kAir : kLiquid;
    bool any = false;
#pragma unroll
    for (int q = 0; q < 6; ++q) any |= n[q] == other;
    return (m == kLiquid || m == kAir) && any;
}

// ---- surface tension: a non-zero interface pressure p_G on liquid/air faces ------------------------
// p_G of the liquid/air face between cells b (behind) and c (front): sp interpolated to the interface, theta measured from
// the liquid cell.  liquidBehind tells which of the two cells is the liquid one.
__device__ __forceinline__ float interfacePressure(float theta, bool liquidBehind, float spb, float spc)
{
    const float spL = liquidBehind ? spb : spc, spA = liquidBehind ? spc : spb;
    return (1.f - theta) * spL + theta * spA;
}

// rhsC += w_f * p_G over the liquid/air faces of the LIQUID cell (i, j, k) of G, in face order a = 0..2, d = 0..1.  rhsC is the
// cell's entry of the expanded rhs, phiC and spC its own phi and sp (references: touched only at a liquid/air face), wAcross(a, d)
// the expanded weight of its face (a, d) (cw / theta; 0 on an invalid face).  Returns the largest |p_G| met.
template <class WAcross, class MatAt, class RealAt>
__device__ __forceinline__ float addSurfaceRhs(const Box &G, int i, int j, int k, const float &phiC, const float &spC, float &rhsC,
                                               WAcross wAcross, MatAt matAt, RealAt phiAt, RealAt spAt)
{
    const int ext[3] = {G.gx, G.gy, G.gz};
    float acc = rhsC, amax = 0.f;
    bool touched = false;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            int n[3] = {i, j, k};
            n[a] += d ? 1 : -1;
            if (n[a] < 0 || n[a] >= ext[a]) continue;
            if (matAt(n[0], n[1], n[2]) != kAir) continue;
            const float wf = wAcross(a, d);
            if (wf == 0.f) continue;  // not a valid face
            const float phc = phiC, phn = phiAt(n[0], n[1], n[2]);
            const float spc = spC, spn = spAt(n[0], n[1], n[2]);
            // b / c of the face: the neighbour is behind for d = 0
            const float theta = d ? ghostFluidTheta(phc, phn) : ghostFluidTheta(phn, phc);
            const float pg = interfacePressure(theta, d == 1, d ? spc : spn, d ? spn : spc);
            acc += wf * pg;
            amax = fmaxf(amax, fabsf(pg));
            touched = true;
        }
    if (touched) rhsC = acc;
    return amax;
}
// pGammaMax (may be NULL) is raised to the largest amax of the wave, as float bits: non-negative floats order like their bits.
// Every lane of the wave calls it.
__device__ __forceinline__ void raisePGammaMax(unsigned *pGammaMax, float amax)
{
    if (!pGammaMax) return;
    for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
    if ((threadIdx.x & 63) == 0 && amax > 0.f) atomicMax(pGammaMax, __float_as_uint(amax));
}

// Pressure gradient across the valid face of `axis` in front of cell (i, j, k) of G (a valid face has both cells in G): the
// difference, over theta unless the face is liquid/liquid (Plug.cpp:1086-1087).  With `surface` the air cell's value on a
// liquid/air face is p_G first.  phi and sp are fetched only on a face that is not liquid/liquid.
template <class MatAt, class RealAt>
__device__ __forceinline__ float faceGradient(int axis, int i, int j, int k, bool surface, MatAt mat, RealAt pr, RealAt phi, RealAt sp)
{
    int b[3] = {i, j, k};
    b[axis] -= 1;
    const bool lb = mat(b[0], b[1], b[2]) == kLiquid, lf = mat(i, j, k) == kLiquid;
    float pb = pr(b[0], b[1], b[2]), pf = pr(i, j, k);
    float grad;
    if (lb && lf) grad = pf - pb;
    else {  // a valid face that is not liquid/liquid is liquid/air
        const float theta = ghostFluidTheta(phi(b[0], b[1], b[2]), phi(i, j, k));
        if (surface) {
            const float pg = interfacePressure(theta, lb, sp(b[0], b[1], b[2]), sp(i, j, k));
            if (lb) pf = pg;
            else pb = pg;
        }
        grad = (pf - pb) / theta;
    }
    return grad;
}

// scale * clamp(kappa, -1, 1) of the cell (i, j, k): the 19-point curvature from `at(x, y, z)`, the neighbour indices already
// clamped into the grid.
template <class At>
__device__ __forceinline__ float surfacePressureAt(At at, double scale, int i, int im, int ip, int j, int jm, int jp, int k, int km, int kp)
{
    const double p0 = at(i, j, k);
    const double pxm = at(im, j, k), pxp = at(ip, j, k), pym = at(i, jm, k), pyp = at(i, jp, k), pzm = at(i, j, km), pzp = at(i, j, kp);
    const double fx = 0.5 * (pxp - pxm), fy = 0.5 * (pyp - pym), fz = 0.5 * (pzp - pzm);
    const double fxx = pxp - 2.0 * p0 + pxm, fyy = pyp - 2.0 * p0 + pym, fzz = pzp - 2.0 * p0 + pzm;
    const double fxy = 0.25 * (at(ip, jp, k) - at(ip, jm, k) - at(im, jp, k) + at(im, jm, k));
    const double fxz = 0.25 * (at(ip, j, kp) - at(ip, j, km) - at(im, j, kp) + at(im, j, km));
    const double fyz = 0.25 * (at(i, jp, kp) - at(i, jp, km) - at(i, jm, kp) + at(i, jm, km));
    const double gx2 = fx * fx, gy2 = fy * fy, gz2 = fz * fz, g2 = gx2 + gy2 + gz2;
    double kappa = 0.0;
    if (g2 >= 1e-30) {
        const double num = fxx * (gy2 + gz2) + fyy * (gx2 + gz2) + fzz * (gx2 + gy2) - 2.0 * fx * fy * fxy - 2.0 * fx * fz * fxz -
                           2.0 * fy * fz * fyz;
        kappa = num / (g2 * sqrt(g2));
    }
    kappa = fmin(fmax(kappa, -1.0), 1.0);
    return float(scale * kappa);
}
// sp of cell (i, j, k) of G with label m: scale * clamp(kappa, -1, 1) at an interface cell, 0 elsewhere.  kappa is the mean
// curvature div(grad phi / |grad phi|) from unit-spacing central differences (19 points, indices clamped into the grid),
// evaluated in double: only interface cells do it, and they are a thin shell.
template <class MatAt, class PhiAt>
__device__ __forceinline__ float surfacePressure(const Box &G, int i, int j, int k, int m, double scale, MatAt mat, PhiAt phi)
{
    if (!isInterfaceCell(G, i, j, k, m, mat)) return 0.f;
    const int im = max(i - 1, 0), ip = min(i + 1, G.gx - 1), jm = max(j - 1, 0), jp = min(j + 1, G.gy - 1), km = max(k - 1, 0),
              kp = min(k + 1, G.gz - 1);
    return surfacePressureAt([&](int x, int y, int z) { return double(phi(x, y, z)); }, scale, i, im, ip, j, jm, jp, k, km, kp);
}

// weighted divergence of a LIQUID cell; signBackward = +1 gives the right-hand side (Plug.cpp:912), -1 the
// divergence report (Plug.cpp:1180).  It reads the cell's own faces only, so a window is a box of its own here.
__device__ __forceinline__ float cellDivergence(const Box &g, int i, int j, int k, float signBackward, const float *const v[3],
                                                const float *const sv[3], const float *const cw[3])
{
    float div = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const size_t f = cellFace(g, a, d, i, j, k);
            const float sign = d == 0 ? signBackward : -signBackward, w = cw[a][f];
            if (w > 0.f) div += sign * w * v[a][f];
            if (sv[a] && w < 1.f) div += sign * (1.f - w) * sv[a][f];
        }
    return div;
}

// ---- the whole-grid passes --------------------------------------------------------------------------------------------
__global__ void materialLabelsKernel(Box g, int32_t *__restrict__ material, const float *__restrict__ phi,
                                     const float *__restrict__ solidPhi, const float *__restrict__ cwx,
                                     const float *__restrict__ cwy, const float *__restrict__ cwz)
{
    int i, j, k;
    if (!unflatten(g.gx, g.gy, g.gz, i, j, k)) return;
    const float *cw[3] = {cwx, cwy, cwz};
    material[cellAt(g, i, j, k)] = materialLabel(g, g, i, j, k, k, phi, solidPhi, cw, GridAt<float>{g, phi});
}

__global__ void validFacesKernel(Box g, int axis, uint8_t *__restrict__ valid, const int32_t *__restrict__ material,
                                 const float *__restrict__ cw)
{
    int i, j, k;
    if (!unflatten(g.gx + (axis == 0), g.gy + (axis == 1), g.gz + (axis == 2), i, j, k)) return;
    const size_t f = faceAt(g, axis, i, j, k);
    int mb, mf;
    valid[f] = isValidFace(g, axis, i, j, k, cw[f], GridAt<int32_t>{g, material}, mb, mf);
}

__global__ void domainLabelsKernel(Box g, Box e, int offset, uint8_t *__restrict__ expanded, const int32_t *__restrict__ material)
{
    int bi, bj, bk;  // (the base box only: the launcher has filled the expanded grid with EXTERIOR)
    if (!unflatten(g.gx, g.gy, g.gz, bi, bj, bk)) return;
    expanded[cellAt(e, bi + offset, bj + offset, bk + offset)] = domainLabel(material[cellAt(g, bi, bj, bk)]);
}

__global__ void boundaryWeightsKernel(Box g, Box e, int offset, int axis, float *__restrict__ expanded, const float *__restrict__ cw,
                                      const float *__restrict__ phi, const uint8_t *__restrict__ valid,
                                      const int32_t *__restrict__ material)
{
    int bi, bj, bk;  // (the faces of the base box only: the launcher has zeroed the expanded face grid)
    if (!unflatten(g.gx + (axis == 0), g.gy + (axis == 1), g.gz + (axis == 2), bi, bj, bk)) return;
    const size_t f = faceAt(g, axis, bi, bj, bk);
    float w = 0.f;
    if (valid[f]) {  // a valid face has both cells inside the grid
        const GridAt<int32_t> mat{g, material};
        int b[3] = {bi, bj, bk};
        b[axis] -= 1;
        w = expandedWeight(axis, bi, bj, bk, cw[f], mat(b[0], b[1], b[2]), mat(bi, bj, bk), GridAt<float>{g, phi});
    }
    expanded[faceAt(e, axis, bi + offset, bj + offset, bk + offset)] = w;
}

__global__ void setBoundaryLabelsKernel(Box e, uint8_t *__restrict__ lab, const float *__restrict__ wx,
                                        const float *__restrict__ wy, const float *__restrict__ wz)
{
    int i, j, k;
    if (!unflatten(e.gx, e.gy, e.gz, i, j, k)) return;
    const size_t c = cellAt(e, i, j, k);
    // INTERIOR cells have all six neighbours inside the grid (the EXTERIOR shell); BOUNDARY written by another
    // thread reads as "not DIRICHLET / EXTERIOR" just like INTERIOR, so the in-place update is race-free
    if (lab[c] != MGPS_INTERIOR_CELL) return;
    const float *w[3] = {wx, wy, wz};
    const ptrdiff_t stride[3] = {1, e.gx, ptrdiff_t(e.gx) * e.gy};
    if (isBoundaryCell(e, i, j, k, w, [&](int a, int d) { return int(lab[ptrdiff_t(c) + (d ? stride[a] : -stride[a])]); }))
        lab[c] = MGPS_BOUNDARY_CELL;
}

__global__ void rhsKernel(Box g, Box e, int offset, float *__restrict__ rhs, const int32_t *__restrict__ material, const float *vx,
                          const float *vy, const float *vz, const float *svx, const float *svy, const float *svz, const float *cwx,
                          const float *cwy, const float *cwz)
{
    int bi, bj, bk;  // (the base box only: the launcher has zeroed the expanded grid)
    if (!unflatten(g.gx, g.gy, g.gz, bi, bj, bk)) return;
    if (material[cellAt(g, bi, bj, bk)] != kLiquid) return;
    const float *v[3] = {vx, vy, vz}, *sv[3] = {svx, svy, svz}, *cw[3] = {cwx, cwy, cwz};
    rhs[cellAt(e, bi + offset, bj + offset, bk + offset)] = cellDivergence(g, bi, bj, bk, 1.f, v, sv, cw);
}

__global__ void pressureToSolutionKernel(Box g, Box e, int offset, float *__restrict__ x, const float *__restrict__ pressure,
                                         const int32_t *__restrict__ material)
{
    int bi, bj, bk;  // (the base box only: the launcher has zeroed the expanded grid)
    if (!unflatten(g.gx, g.gy, g.gz, bi, bj, bk)) return;
    const size_t c = cellAt(g, bi, bj, bk);
    if (material[c] == kLiquid) x[cellAt(e, bi + offset, bj + offset, bk + offset)] = pressure[c];
}

__global__ void solutionToPressureKernel(Box g, Box e, int offset, float *__restrict__ pressure, const float *__restrict__ x,
                                         const int32_t *__restrict__ material)
{
    int i, j, k;
    if (!unflatten(g.gx, g.gy, g.gz, i, j, k)) return;
    const size_t c = cellAt(g, i, j, k);
    if (material[c] == kLiquid) pressure[c] = x[cellAt(e, i + offset, j + offset, k + offset)];
}

// velocity -= the pressure gradient on the valid faces of `axis`
__global__ void pressureGradientKernel(Box g, int axis, float *__restrict__ velocity, const float *__restrict__ phi,
                                       const float *__restrict__ pressure, const uint8_t *__restrict__ valid,
                                       const int32_t *__restrict__ material)
{
    int i, j, k;
    if (!unflatten(g.gx + (axis == 0), g.gy + (axis == 1), g.gz + (axis == 2), i, j, k)) return;
    const size_t f = faceAt(g, axis, i, j, k);
    if (!valid[f]) return;
    velocity[f] -= faceGradient(axis, i, j, k, false, GridAt<int32_t>{g, material}, GridAt<float>{g, pressure}, GridAt<float>{g, phi},
                                GridAt<float>{g, nullptr});
}
// ... with the air cell's value on a liquid/air face replaced by p_G.  faceGradient's rule written out: through the shared
// function this pass measured 0.4-0.5 % slower than before at 480^3, twice, beyond the run's noise (LABNOTES R10)
__global__ __launch_bounds__(256) void pressureGradientSurfaceKernel(Box g, int axis, float *__restrict__ velocity,
                                                                     const float *__restrict__ phi, const float *__restrict__ pressure,
                                                                     const float *__restrict__ sp, const uint8_t *__restrict__ valid,
                                                                     const int32_t *__restrict__ material)
{
    int i, j, k;
    if (!unflatten(g.gx + (axis == 0), g.gy + (axis == 1), g.gz + (axis == 2), i, j, k)) return;
    const size_t f = faceAt(g, axis, i, j, k);
    if (!valid[f]) return;  // valid faces have both cells inside the grid
    int b[3] = {i, j, k};
    b[axis] -= 1;
    const size_t cb = cellAt(g, b[0], b[1], b[2]), cf = cellAt(g, i, j, k);
    const bool lb = material[cb] == kLiquid, lf = material[cf] == kLiquid;
    float pb = pressure[cb], pf = pressure[cf], grad;
    if (lb && lf) grad = pf - pb;
    else {  // a valid face that is not liquid/liquid is liquid/air
        const float theta = ghostFluidTheta(phi[cb], phi[cf]);
        const float pg = interfacePressure(theta, lb, sp[cb], sp[cf]);
        if (lb) pf = pg;
        else pb = pg;
        grad = (pf - pb) / theta;
    }
    velocity[f] -= grad;
}

__global__ __launch_bounds__(256) void surfacePressureKernel(Box g, float *__restrict__ sp, const float *__restrict__ phi,
                                                             const int32_t *__restrict__ material, double scale)
{
    int i, j, k;
    threadCell(i, j, k);
    if (i >= g.gx) return;
    const size_t c = cellAt(g, i, j, k);
    sp[c] = surfacePressure(g, i, j, k, material[c], scale, GridNear<int32_t>{g, material, c, i, j, k}, GridAt<float>{g, phi});
}

// the surface term on top of the rhs already in the expanded grid (addSurfaceRhs), with the weights boundaryWeightsKernel wrote
__global__ __launch_bounds__(256) void rhsSurfaceKernel(Box g, Box e, int offset, float *__restrict__ rhs, const float *wx,
                                                        const float *wy, const float *wz, const float *__restrict__ phi,
                                                        const int32_t *__restrict__ material, const float *__restrict__ sp,
                                                        unsigned *__restrict__ pGammaMax)
{
    int bi, bj, bk;
    threadCell(bi, bj, bk);
    float amax = 0.f;
    // (no early return: every lane reaches the wave reduction below)
    const bool inside = bi < g.gx;
    const size_t c = inside ? cellAt(g, bi, bj, bk) : 0;
    const int m = inside ? material[c] : kSolid;
    if (inside && isInterfaceCell(g, bi, bj, bk, m, GridNear<int32_t>{g, material, c, bi, bj, bk}) && m == kLiquid) {  // (the seven labels load together)
        const float *w[3] = {wx, wy, wz};
        const int ei = bi + offset, ej = bj + offset, ek = bk + offset;
        auto wAcross = [&](int a, int d) { return w[a][cellFace(e, a, d, ei, ej, ek)]; };
        amax = addSurfaceRhs(g, bi, bj, bk, phi[c], sp[c], rhs[cellAt(e, ei, ej, ek)], wAcross, GridAt<int32_t>{g, material}, GridAt<float>{g, phi},
                             GridAt<float>{g, sp});
    }
    raisePGammaMax(pGammaMax, amax);
}

constexpr int kDivBlocks = 1024;
__global__ __launch_bounds__(256) void divergenceKernel(Box g, double *__restrict__ partials, const int32_t *__restrict__ material,
                                                        const float *vx, const float *vy, const float *vz, const float *svx,
                                                        const float *svy, const float *svz, const float *cwx, const float *cwy,
                                                        const float *cwz)
{
    const float *v[3] = {vx, vy, vz}, *sv[3] = {svx, svy, svz}, *cw[3] = {cwx, cwy, cwz};
    double sum = 0.0, mx = 0.0, count = 0.0;
    const size_t n = g.cells();
    for (size_t t = size_t(blockIdx.x) * blockDim.x + threadIdx.x; t < n; t += size_t(gridDim.x) * blockDim.x) {
        if (material[t] != kLiquid) continue;
        const int i = int(t % g.gx), j = int((t / g.gx) % g.gy), k = int(t / (size_t(g.gx) * g.gy));
        const double d = double(cellDivergence(g, i, j, k, -1.f, v, sv, cw));
        sum += d;
        mx = d > mx ? d : mx;
        count += 1.0;
    }
    __shared__ double s[3][256];
    s[0][threadIdx.x] = sum;
    s[1][threadIdx.x] = mx;
    s[2][threadIdx.x] = count;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (int(threadIdx.x) < off) {
            s[0][threadIdx.x] += s[0][threadIdx.x + off];
            s[1][threadIdx.x] = s[1][threadIdx.x] > s[1][threadIdx.x + off] ? s[1][threadIdx.x] : s[1][threadIdx.x + off];
            s[2][threadIdx.x] += s[2][threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = s[0][0];
        partials[kDivBlocks + blockIdx.x] = s[1][0];
        partials[2 * kDivBlocks + blockIdx.x] = s[2][0];
    }
}

int bad(const char *what)
{
    setLastGlobalError(std::string(what) + ": NULL pointer, axis outside 0..2 or non-positive extent");
    return MGPS_ERR_INVALID_ARGUMENT;
}
int done(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return MGPS_OK;
    setLastGlobalError(std::string(what) + ": " + hipGetErrorString(e));
    return MGPS_ERR_HIP;
}
inline unsigned blocks(size_t n) { return unsigned((n + 255) / 256); }
inline bool okBox(int x, int y, int z) { return x > 0 && y > 0 && z > 0; }
inline bool okCellGrid(int y, int z) { return y <= 65535 && z <= 65535; }  // rowGrid: y and z extents are launch-grid dimensions
inline bool okExpanded(int gx, int gy, int gz, int ex, int ey, int ez, int off)
{
    return okBox(ex, ey, ez) && off >= 0 && gx + off <= ex && gy + off <= ey && gz + off <= ez;
}

}  // namespace

extern "C" {

int mgps_fields_material_labels(int32_t *material, const float *liquid_phi, const float *solid_phi, const float *cwx,
                                const float *cwy, const float *cwz, int gx, int gy, int gz, void *stream)
try {
    if (!material || !liquid_phi || !solid_phi || !cwx || !cwy || !cwz || !okBox(gx, gy, gz)) return bad("mgps_fields_material_labels");
    const Box g{gx, gy, gz};
    materialLabelsKernel<<<blocks(g.cells()), 256, 0, static_cast<hipStream_t>(stream)>>>(g, material, liquid_phi, solid_phi, cwx, cwy, cwz);
    return done("mgps_fields_material_labels");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_valid_faces(int axis, uint8_t *valid, const int32_t *material, const float *cut_weights, int gx, int gy,
                            int gz, void *stream)
try {
    if (axis < 0 || axis > 2 || !valid || !material || !cut_weights || !okBox(gx, gy, gz)) return bad("mgps_fields_valid_faces");
    const Box g{gx, gy, gz};
    const size_t n = size_t(gx + (axis == 0)) * (gy + (axis == 1)) * (gz + (axis == 2));
    validFacesKernel<<<blocks(n), 256, 0, static_cast<hipStream_t>(stream)>>>(g, axis, valid, material, cut_weights);
    return done("mgps_fields_valid_faces");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_domain_labels(uint8_t *expanded_labels, const int32_t *material, int gx, int gy, int gz, int ex, int ey,
                              int ez, int offset, void *stream)
try {
    if (!expanded_labels || !material || !okBox(gx, gy, gz) || !okExpanded(gx, gy, gz, ex, ey, ez, offset))
        return bad("mgps_fields_domain_labels");
    const Box g{gx, gy, gz}, e{ex, ey, ez};
    // fill + a kernel over the base box: the reference's power-of-two expansion makes the solver grid up to ten times the
    // simulation grid (480^3 -> 1024^3), and one thread per expanded cell spent 2.5-4 ms per pass there
    if (hipMemsetAsync(expanded_labels, MGPS_EXTERIOR_CELL, e.cells(), static_cast<hipStream_t>(stream)) != hipSuccess) return bad("mgps_fields_domain_labels");
    domainLabelsKernel<<<blocks(g.cells()), 256, 0, static_cast<hipStream_t>(stream)>>>(g, e, offset, expanded_labels, material);
    return done("mgps_fields_domain_labels");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_boundary_weights(int axis, float *expanded_weights, const float *cut_weights, const float *liquid_phi,
                                 const uint8_t *valid, const int32_t *material, int gx, int gy, int gz, int ex, int ey,
                                 int ez, int offset, void *stream)
try {
    if (axis < 0 || axis > 2 || !expanded_weights || !cut_weights || !liquid_phi || !valid || !material || !okBox(gx, gy, gz) ||
        !okExpanded(gx, gy, gz, ex, ey, ez, offset))
        return bad("mgps_fields_boundary_weights");
    const Box g{gx, gy, gz}, e{ex, ey, ez};
    const size_t n = size_t(ex + (axis == 0)) * (ey + (axis == 1)) * (ez + (axis == 2));
    const size_t nb = size_t(gx + (axis == 0)) * (gy + (axis == 1)) * (gz + (axis == 2));
    if (hipMemsetAsync(expanded_weights, 0, n * sizeof(float), static_cast<hipStream_t>(stream)) != hipSuccess) return bad("mgps_fields_boundary_weights");
    boundaryWeightsKernel<<<blocks(nb), 256, 0, static_cast<hipStream_t>(stream)>>>(g, e, offset, axis, expanded_weights, cut_weights,
                                                                                    liquid_phi, valid, material);
    return done("mgps_fields_boundary_weights");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_set_boundary_labels(uint8_t *expanded_labels, const float *wx, const float *wy, const float *wz, int ex,
                                    int ey, int ez, void *stream)
try {
    if (!expanded_labels || !wx || !wy || !wz || !okBox(ex, ey, ez)) return bad("mgps_fields_set_boundary_labels");
    const Box e{ex, ey, ez};
    setBoundaryLabelsKernel<<<blocks(e.cells()), 256, 0, static_cast<hipStream_t>(stream)>>>(e, expanded_labels, wx, wy, wz);
    return done("mgps_fields_set_boundary_labels");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_rhs(float *expanded_rhs, const int32_t *material, const float *vx, const float *vy, const float *vz,
                    const float *svx, const float *svy, const float *svz, const float *cwx, const float *cwy,
                    const float *cwz, int gx, int gy, int gz, int ex, int ey, int ez, int offset, void *stream)
try {
    if (!expanded_rhs || !material || !vx || !vy || !vz || !cwx || !cwy || !cwz || !okBox(gx, gy, gz) ||
        !okExpanded(gx, gy, gz, ex, ey, ez, offset) || ((svx || svy || svz) && !(svx && svy && svz)))
        return bad("mgps_fields_rhs");
    const Box g{gx, gy, gz}, e{ex, ey, ez};
    if (hipMemsetAsync(expanded_rhs, 0, e.cells() * sizeof(float), static_cast<hipStream_t>(stream)) != hipSuccess) return bad("mgps_fields_rhs");
    rhsKernel<<<blocks(g.cells()), 256, 0, static_cast<hipStream_t>(stream)>>>(g, e, offset, expanded_rhs, material, vx, vy, vz, svx, svy,
                                                                             svz, cwx, cwy, cwz);
    return done("mgps_fields_rhs");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_pressure_to_solution(float *expanded_x, const float *pressure, const int32_t *material, int gx, int gy,
                                     int gz, int ex, int ey, int ez, int offset, void *stream)
try {
    if (!expanded_x || !pressure || !material || !okBox(gx, gy, gz) || !okExpanded(gx, gy, gz, ex, ey, ez, offset))
        return bad("mgps_fields_pressure_to_solution");
    const Box g{gx, gy, gz}, e{ex, ey, ez};
    if (hipMemsetAsync(expanded_x, 0, e.cells() * sizeof(float), static_cast<hipStream_t>(stream)) != hipSuccess) return bad("mgps_fields_pressure_to_solution");
    pressureToSolutionKernel<<<blocks(g.cells()), 256, 0, static_cast<hipStream_t>(stream)>>>(g, e, offset, expanded_x, pressure, material);
    return done("mgps_fields_pressure_to_solution");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_solution_to_pressure(float *pressure, const float *expanded_x, const int32_t *material, int gx, int gy,
                                     int gz, int ex, int ey, int ez, int offset, void *stream)
try {
    if (!pressure || !expanded_x || !material || !okBox(gx, gy, gz) || !okExpanded(gx, gy, gz, ex, ey, ez, offset))
        return bad("mgps_fields_solution_to_pressure");
    const Box g{gx, gy, gz}, e{ex, ey, ez};
    solutionToPressureKernel<<<blocks(g.cells()), 256, 0, static_cast<hipStream_t>(stream)>>>(g, e, offset, pressure, expanded_x, material);
    return done("mgps_fields_solution_to_pressure");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_pressure_gradient(int axis, float *velocity, const float *liquid_phi, const float *pressure,
                                  const uint8_t *valid, const int32_t *material, int gx, int gy, int gz, void *stream)
try {
    if (axis < 0 || axis > 2 || !velocity || !liquid_phi || !pressure || !valid || !material || !okBox(gx, gy, gz))
        return bad("mgps_fields_pressure_gradient");
    const Box g{gx, gy, gz};
    const size_t n = size_t(gx + (axis == 0)) * (gy + (axis == 1)) * (gz + (axis == 2));
    pressureGradientKernel<<<blocks(n), 256, 0, static_cast<hipStream_t>(stream)>>>(g, axis, velocity, liquid_phi, pressure, valid, material);
    return done("mgps_fields_pressure_gradient");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_surface_pressure(float *sp, const float *liquid_phi, const int32_t *material, double scale, int gx, int gy, int gz,
                                 void *stream)
try {
    if (!sp || !liquid_phi || !material || !okBox(gx, gy, gz) || !okCellGrid(gy, gz)) return bad("mgps_fields_surface_pressure");
    const Box g{gx, gy, gz};
    surfacePressureKernel<<<rowGrid(gx, gy, gz), 256, 0, static_cast<hipStream_t>(stream)>>>(g, sp, liquid_phi, material, scale);
    return done("mgps_fields_surface_pressure");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_rhs_surface(float *expanded_rhs, const float *wx, const float *wy, const float *wz, const float *liquid_phi,
                            const int32_t *material, const float *sp, float *p_gamma_max, int gx, int gy, int gz, int ex, int ey,
                            int ez, int offset, void *stream)
try {
    if (!expanded_rhs || !wx || !wy || !wz || !liquid_phi || !material || !sp || !okBox(gx, gy, gz) || !okCellGrid(gy, gz) ||
        !okExpanded(gx, gy, gz, ex, ey, ez, offset))
        return bad("mgps_fields_rhs_surface");
    const Box g{gx, gy, gz}, e{ex, ey, ez};
    rhsSurfaceKernel<<<rowGrid(gx, gy, gz), 256, 0, static_cast<hipStream_t>(stream)>>>(g, e, offset, expanded_rhs, wx, wy, wz, liquid_phi,
                                                                                       material, sp, reinterpret_cast<unsigned *>(p_gamma_max));
    return done("mgps_fields_rhs_surface");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_pressure_gradient_surface(int axis, float *velocity, const float *liquid_phi, const float *pressure, const float *sp,
                                          const uint8_t *valid, const int32_t *material, int gx, int gy, int gz, void *stream)
try {
    if (axis < 0 || axis > 2 || !velocity || !liquid_phi || !pressure || !sp || !valid || !material || !okBox(gx, gy, gz))
        return bad("mgps_fields_pressure_gradient_surface");
    const Box g{gx, gy, gz};
    const size_t n = size_t(gx + (axis == 0)) * (gy + (axis == 1)) * (gz + (axis == 2));
    pressureGradientSurfaceKernel<<<blocks(n), 256, 0, static_cast<hipStream_t>(stream)>>>(g, axis, velocity, liquid_phi, pressure, sp,
                                                                                         valid, material);
    return done("mgps_fields_pressure_gradient_surface");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_divergence(double out_host[3], const int32_t *material, const float *vx, const float *vy, const float *vz,
                           const float *svx, const float *svy, const float *svz, const float *cwx, const float *cwy,
                           const float *cwz, int gx, int gy, int gz, void *stream)
try {
    if (!out_host || !material || !vx || !vy || !vz || !cwx || !cwy || !cwz || !okBox(gx, gy, gz) ||
        ((svx || svy || svz) && !(svx && svy && svz)))
        return bad("mgps_fields_divergence");
    const Box g{gx, gy, gz};
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *partials = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&partials), 3 * kDivBlocks * sizeof(double)) != hipSuccess) {
        setLastGlobalError("mgps_fields_divergence: hipMalloc failed");
        return MGPS_ERR_ALLOC;
    }
    divergenceKernel<<<kDivBlocks, 256, 0, s>>>(g, partials, material, vx, vy, vz, svx, svy, svz, cwx, cwy, cwz);
    std::vector<double> host(3 * kDivBlocks);
    hipError_t e = hipMemcpyAsync(host.data(), partials, host.size() * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(partials);
    if (e != hipSuccess) {
        setLastGlobalError(std::string("mgps_fields_divergence: ") + hipGetErrorString(e));
        return MGPS_ERR_HIP;
    }
    double sum = 0.0, mx = 0.0, count = 0.0;  // fixed order: reproducible
    for (int b = 0; b < kDivBlocks; ++b) {
        sum += host[size_t(b)];
        mx = host[size_t(kDivBlocks + b)] > mx ? host[size_t(kDivBlocks + b)] : mx;
        count += host[size_t(2 * kDivBlocks + b)];
    }
    out_host[0] = sum;
    out_host[1] = mx;
    out_host[2] = count;
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

}  // extern "C"

// ---- one-call projection (mgps_project_free_surface) --------------------------------------------------------------
namespace {
__global__ void narrowRealKernel(float *__restrict__ dst, const double *__restrict__ src, size_t n)
{
    const size_t c = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c < n) dst[c] = float(src[c]);
}
__global__ void widenRealKernel(double *__restrict__ dst, const float *__restrict__ src, size_t n)
{
    const size_t c = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c < n) dst[c] = double(src[c]);
}

// number of LIQUID cells (material label 1, Util.h:17)
__global__ void countLiquidKernel(const int32_t *__restrict__ material, size_t n, unsigned long long *__restrict__ count)
{
    unsigned long long mine = 0;
    for (size_t c = size_t(blockIdx.x) * blockDim.x + threadIdx.x; c < n; c += size_t(gridDim.x) * blockDim.x) mine += material[c] == 1;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);
}

// device buffers of one call; everything is released when the object goes out of scope
struct DevPool {
    std::vector<void *> blocks;
    ~DevPool()
    {
        (void)hipDeviceSynchronize();  // (deviceFree keeps the blocks for the next call and does not wait for queued kernels)
        for (void *b : blocks) (void)mgps::deviceFree(b);
    }
    template <class T>
    T *get(size_t count)
    {
        void *p = nullptr;
        if (mgps::deviceAlloc(&p, std::max<size_t>(count, 1) * sizeof(T)) != 0) throw std::bad_alloc();
        blocks.push_back(p);
        return static_cast<T *>(p);
    }
};
size_t faceCount(int gx, int gy, int gz, int axis) { return size_t(gx + (axis == 0)) * (gy + (axis == 1)) * (gz + (axis == 2)); }

// ---- what mgps_project_free_surface and mgps_project_free_surface_slab check and prepare alike (P: their structs) ------------
// The caller's fields and the surface-tension block, before any device is touched.  `fn` is the entry point's name, the prefix of its
// messages; `shapeOk` and `missing` carry what only one of the two has to check about extents.
template <class P>
int checkProjectionFields(const P *p, const char *fn, bool shapeOk, const char *missing)
{
    bool ok = shapeOk && p->liquid_phi && p->solid_phi && p->pressure;
    for (int a = 0; a < 3; ++a) ok = ok && p->cut_weights[a] && p->velocity[a];
    const bool haveSolidVel = p->solid_velocity[0] && p->solid_velocity[1] && p->solid_velocity[2];
    if (!ok || (!haveSolidVel && (p->solid_velocity[0] || p->solid_velocity[1] || p->solid_velocity[2])))
        return refuse(fn, std::string(missing) + " (solid velocities: all three or none)");
    // surface tension: dt, dx and density are read only with surface_tension > 0
    const double sigma = p->surface_tension;
    if (!std::isfinite(sigma) || sigma < 0) return refuse(fn, "surface_tension must be finite and >= 0");
    if (sigma > 0) {
        const char *what = !(std::isfinite(p->dt) && p->dt > 0) ? "dt" : !(std::isfinite(p->dx) && p->dx > 0) ? "dx"
                         : !(std::isfinite(p->density) && p->density > 0) ? "density" : nullptr;
        if (what) return refuse(fn, std::string("surface_tension > 0 needs a finite ") + what + " > 0");
        if (p->surface_pressure) return refuse(fn, "surface_tension and surface_pressure are both set (pass one of them)");
    }
    return MGPS_OK;
}
// o = the caller's options, or the defaults; `prefix` goes in front of the refusal
int readOptions(const mgps_options *opt, mgps_options &o, const char *prefix)
{
    mgps_default_options(&o);
    if (!opt) return MGPS_OK;
    if (opt->struct_size != int(sizeof(mgps_options))) {
        setLastGlobalError(std::string(prefix) + "mgps_options.struct_size mismatch: call mgps_default_options first");
        return MGPS_ERR_INVALID_ARGUMENT;
    }
    o = *opt;
    return MGPS_OK;
}
int selectDevice(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        setLastGlobalError("no HIP device is visible (this library has no CPU path)");
        return MGPS_ERR_NO_DEVICE;
    }
    if (device >= 0 && hipSetDevice(device) != hipSuccess) {
        setLastGlobalError("hipSetDevice failed");
        return MGPS_ERR_NO_DEVICE;
    }
    return MGPS_OK;
}
// what a call reports about its solve, before there is one
template <class P>
void clearReport(P *p)
{
    std::memset(&p->stats, 0, sizeof(p->stats));
    p->residual_inf = p->residual_l2 = p->divergence_sum = p->divergence_max = 0;
    p->enclosed_components = 0;
    p->rhs_mean_removed_max = p->surface_pressure_max = 0;
}
}  // namespace

extern "C" {

int mgps_project_free_surface(mgps_projection *p, const mgps_options *opt)
try {
    using clock = SlabCall::Clock;
    const auto t0 = clock::now();
    if (!p || p->struct_size != int(sizeof(mgps_projection))) {
        setLastGlobalError("mgps_project_free_surface: NULL or struct_size mismatch");
        return MGPS_ERR_INVALID_ARGUMENT;
    }
    const int gx = p->gx, gy = p->gy, gz = p->gz;
    if (int rc = checkProjectionFields(p, "mgps_project_free_surface", gx > 0 && gy > 0 && gz > 0 && (p->real_bytes == 4 || p->real_bytes == 8),
                                       "missing field or bad extents");
        rc != MGPS_OK)
        return rc;
    const bool haveSolidVel = p->solid_velocity[0] != nullptr;  // (all three or none)
    const double sigma = p->surface_tension;
    const bool surface = sigma > 0 || p->surface_pressure;
    mgps_options o;
    if (int rc = readOptions(opt, o, ""); rc != MGPS_OK) return rc;
    if (int rc = selectDevice(o.device); rc != MGPS_OK) return rc;
    hipStream_t s = nullptr;
    DevPool pool;
    const size_t cells = size_t(gx) * gy * gz;
    const bool dbl = p->real_bytes == 8;
    double *stage = nullptr;  // device staging for double host arrays
    if (dbl) stage = pool.get<double>(faceCount(gx + 1, gy + 1, gz + 1, 3));
    auto failHip = [&](const char *what, hipError_t e) {
        setLastGlobalError(std::string("mgps_project_free_surface: ") + what + ": " + hipGetErrorString(e));
        return int(MGPS_ERR_HIP);
    };
    hipError_t he = hipSuccess;
    auto upload = [&](const void *host, size_t n) -> float * {  // float copy of a host real array on the device
        float *d = pool.get<float>(n);
        if (he != hipSuccess) return d;
        if (!dbl) he = hipMemcpy(d, host, n * sizeof(float), hipMemcpyHostToDevice);
        else {
            he = hipMemcpy(stage, host, n * sizeof(double), hipMemcpyHostToDevice);
            if (he == hipSuccess) {
                narrowRealKernel<<<unsigned((n + 255) / 256), 256, 0, s>>>(d, stage, n);
                he = hipStreamSynchronize(s);
            }
        }
        return d;
    };
    auto download = [&](void *host, const float *d, size_t n) {
        if (he != hipSuccess) return;
        if (!dbl) he = hipMemcpy(host, d, n * sizeof(float), hipMemcpyDeviceToHost);
        else {
            widenRealKernel<<<unsigned((n + 255) / 256), 256, 0, s>>>(stage, d, n);
            he = hipMemcpy(host, stage, n * sizeof(double), hipMemcpyDeviceToHost);
        }
    };
    // What the labels and weights are made from goes up first; the velocities, the solid velocities and the old pressure --
    // needed from the right-hand side on -- follow on a copy stream while the passes below and the solver's set-up run
    // (float arrays in page-locked memory, mgps_host_alloc: from pageable memory the call degrades to a blocking copy).
    struct CopyStream {
        hipStream_t s = nullptr;
        ~CopyStream()
        {
            if (s) {
                (void)hipStreamSynchronize(s);
                (void)hipStreamDestroy(s);
            }
        }
    } copy;
    if (!dbl && hipStreamCreateWithFlags(&copy.s, hipStreamNonBlocking) != hipSuccess) copy.s = nullptr;
    auto uploadLater = [&](const void *host, size_t n) -> float * {
        if (!copy.s) return upload(host, n);
        float *d = pool.get<float>(n);
        if (he == hipSuccess) he = hipMemcpyAsync(d, host, n * sizeof(float), hipMemcpyHostToDevice, copy.s);
        return d;
    };
    float *phi = upload(p->liquid_phi, cells), *solidPhi = upload(p->solid_phi, cells);
    float *cw[3], *vel[3], *svel[3] = {nullptr, nullptr, nullptr};
    for (int a = 0; a < 3; ++a) cw[a] = upload(p->cut_weights[a], faceCount(gx, gy, gz, a));
    float *pressure = uploadLater(p->pressure, cells);
    for (int a = 0; a < 3; ++a) {
        vel[a] = uploadLater(p->velocity[a], faceCount(gx, gy, gz, a));
        if (haveSolidVel) svel[a] = uploadLater(p->solid_velocity[a], faceCount(gx, gy, gz, a));
    }
    // the surface pressure: one more cell grid, only with the feature on (the caller's, or computed below from the labels)
    float *sp = !surface ? nullptr : p->surface_pressure ? uploadLater(p->surface_pressure, cells) : pool.get<float>(cells);
    if (he != hipSuccess) return failHip("upload", he);
#define PROJ_TRY(call)               \
    do {                             \
        const int rc_ = (call);      \
        if (rc_ != MGPS_OK) return rc_; \
    } while (0)
    // Plug.cpp:270, 286
    int32_t *material = pool.get<int32_t>(cells);
    PROJ_TRY(mgps_fields_material_labels(material, phi, solidPhi, cw[0], cw[1], cw[2], gx, gy, gz, s));
    uint8_t *valid[3];
    for (int a = 0; a < 3; ++a) {
        valid[a] = pool.get<uint8_t>(faceCount(gx, gy, gz, a));
        PROJ_TRY(mgps_fields_valid_faces(a, valid[a], material, cw[a], gx, gy, gz, s));
    }
    // Plug.cpp:316-362: MG labels and weights at +offset of the expanded grid, then the BOUNDARY labels
    int dims[3], offset = 0, levels = 0;
    PROJ_TRY(mgps_expanded_layout(gx, gy, gz, 0, p->power_of_two, dims, &offset, &levels));
    const int ex = dims[0], ey = dims[1], ez = dims[2];
    const size_t ecells = size_t(ex) * ey * ez;
    uint8_t *labels = pool.get<uint8_t>(ecells);
    PROJ_TRY(mgps_fields_domain_labels(labels, material, gx, gy, gz, ex, ey, ez, offset, s));
    float *w[3];
    for (int a = 0; a < 3; ++a) {
        w[a] = pool.get<float>(faceCount(ex, ey, ez, a));
        PROJ_TRY(mgps_fields_boundary_weights(a, w[a], cw[a], phi, valid[a], material, gx, gy, gz, ex, ey, ez, offset, s));
    }
    PROJ_TRY(mgps_fields_set_boundary_labels(labels, w[0], w[1], w[2], ex, ey, ez, s));
    p->mg_levels = levels;
    p->offset = offset;
    p->expanded[0] = ex;
    p->expanded[1] = ey;
    p->expanded[2] = ez;
    // liquid cell count first: a domain without liquid has nothing to solve.  (The reference has no such exit: it would run
    // its solver on an empty system.  What it would publish -- the valid faces it computed and an all-zero pressure,
    // Plug.cpp:286, 641 -- is published here as well; velocities stay as they came.)
    double div[3] = {0, 0, 0};
    {
        unsigned long long *count = pool.get<unsigned long long>(1), liquid = 0;
        he = hipMemsetAsync(count, 0, sizeof(unsigned long long), s);
        if (he == hipSuccess) {
            countLiquidKernel<<<unsigned(std::min<size_t>((cells + 255) / 256, 4096)), 256, 0, s>>>(material, cells, count);
            he = hipMemcpy(&liquid, count, sizeof(liquid), hipMemcpyDeviceToHost);
        }
        if (he != hipSuccess) return failHip("liquid cell count", he);
        div[2] = double(liquid);
    }
    p->liquid_cells = div[2];
    clearReport(p);
    if (div[2] == 0) {
        if (copy.s && (he = hipStreamSynchronize(copy.s)) != hipSuccess) return failHip("upload", he);
        if ((he = hipMemsetAsync(pressure, 0, cells * sizeof(float), s)) != hipSuccess) return failHip("pressure clear", he);
        download(p->pressure, pressure, cells);
        for (int a = 0; a < 3; ++a)
            if (p->valid_faces[a] && he == hipSuccess) he = hipMemcpy(p->valid_faces[a], valid[a], faceCount(gx, gy, gz, a), hipMemcpyDeviceToHost);
        if (he != hipSuccess) return failHip("download", he);
        p->setup_ms = p->total_ms = SlabCall::ms(t0, clock::now());
        p->solve_ms = 0;
        p->stats.outcome = MGPS_PCG_RHS_ZERO;
        return MGPS_OK;
    }
    mgps_solver *mg = nullptr;  // Plug.cpp:463-466 (before the right-hand side here: the velocities may still be on their way)
    o.borrow_device_weights = 1;  // (the pool outlives the solver: `guard` below is destroyed first)
    int rc = mgps_create_device(&mg, ex, ey, ez, labels, w[0], w[1], w[2], levels, p->use_gauss_seidel, &o);
    if (rc != MGPS_OK) return rc;
    struct Guard {
        mgps_solver *h;
        ~Guard() { mgps_destroy(h); }
    } guard{mg};
    if (copy.s && (he = hipStreamSynchronize(copy.s)) != hipSuccess) return failHip("upload", he);
    // Plug.cpp:386, 413
    float *rhs = pool.get<float>(ecells), *x = nullptr;
    PROJ_TRY(mgps_fields_rhs(rhs, material, vel[0], vel[1], vel[2], svel[0], svel[1], svel[2], cw[0], cw[1], cw[2], gx, gy, gz, ex, ey, ez, offset, s));
    float *pGammaMax = nullptr;
    if (surface) {  // b_L += w_f p_G: before the enclosed-liquid projection and the solve, which then see the system actually solved
        if (sigma > 0) PROJ_TRY(mgps_fields_surface_pressure(sp, phi, material, sigma * p->dt / (p->density * p->dx * p->dx), gx, gy, gz, s));
        pGammaMax = pool.get<float>(1);
        if ((he = hipMemsetAsync(pGammaMax, 0, sizeof(float), s)) != hipSuccess) return failHip("surface pressure", he);
        PROJ_TRY(mgps_fields_rhs_surface(rhs, w[0], w[1], w[2], phi, material, sp, pGammaMax, gx, gy, gz, ex, ey, ez, offset, s));
    }
    rc = mgps_grid_alloc(mg, 0, &x);  // zero-filled
    if (rc == MGPS_OK && p->use_old_pressure) rc = mgps_fields_pressure_to_solution(x, pressure, material, gx, gy, gz, ex, ey, ez, offset, s);
    if (rc == MGPS_OK && o.enclosed_liquid) {  // the rhs as the solve sees it (P b): the residual below is then that of the solved system
        int64_t m = 0;
        rc = mgps_enclosed_components(mg, &m, nullptr);
        p->enclosed_components = int(m);
        if (rc == MGPS_OK && m > 0) rc = mgps_project_enclosed(mg, rhs, &p->rhs_mean_removed_max);
    }
    if (rc != MGPS_OK) {
        setLastGlobalError(mgps_last_error(mg));
        return rc;
    }
    (void)hipDeviceSynchronize();
    const auto t1 = clock::now();
    rc = mgps_solve_pcg(mg, x, rhs, p->tolerance, p->max_iterations, p->use_mg_preconditioner, &p->stats);  // Plug.cpp:474-483 / 609-618
    if (rc == MGPS_OK) {  // Plug.cpp:625-628
        float *r = nullptr;
        rc = mgps_grid_alloc(mg, 0, &r);
        if (rc == MGPS_OK) rc = mgps_residual(mg, 0, r, x, rhs);
        if (rc == MGPS_OK) rc = mgps_inf_norm(mg, 0, r, 1, &p->residual_inf);
        if (rc == MGPS_OK) rc = mgps_l2_norm(mg, 0, r, &p->residual_l2);
    }
    if (rc != MGPS_OK && rc != MGPS_ERR_INTERRUPTED) {
        setLastGlobalError(mgps_last_error(mg));
        return rc;
    }
    const int solveRc = rc;
    (void)hipDeviceSynchronize();
    const auto t2 = clock::now();
    // Plug.cpp:641-707: the pressure field is cleared before the solution is written into the liquid cells (`makeConstant(0)`,
    // Plug.cpp:641) -- the warm start above has consumed the caller's old values; a cell that was liquid in the last sub-step and
    // is air or solid now must not keep its old pressure (the gradient pass reads it across ghost-fluid faces)
    if ((he = hipMemsetAsync(pressure, 0, cells * sizeof(float), s)) != hipSuccess) return failHip("pressure clear", he);
    PROJ_TRY(mgps_fields_solution_to_pressure(pressure, x, material, gx, gy, gz, ex, ey, ez, offset, s));
    for (int a = 0; a < 3; ++a)
        PROJ_TRY(surface ? mgps_fields_pressure_gradient_surface(a, vel[a], phi, pressure, sp, valid[a], material, gx, gy, gz, s)
                         : mgps_fields_pressure_gradient(a, vel[a], phi, pressure, valid[a], material, gx, gy, gz, s));
    PROJ_TRY(mgps_fields_divergence(div, material, vel[0], vel[1], vel[2], svel[0], svel[1], svel[2], cw[0], cw[1], cw[2], gx, gy, gz, s));
    p->divergence_sum = div[0];
    p->divergence_max = div[1];
#undef PROJ_TRY
    download(p->pressure, pressure, cells);
    for (int a = 0; a < 3; ++a) {
        download(p->velocity[a], vel[a], faceCount(gx, gy, gz, a));
        if (p->valid_faces[a] && he == hipSuccess) he = hipMemcpy(p->valid_faces[a], valid[a], faceCount(gx, gy, gz, a), hipMemcpyDeviceToHost);
    }
    if (surface && he == hipSuccess) {
        float m = 0;
        he = hipMemcpy(&m, pGammaMax, sizeof(m), hipMemcpyDeviceToHost);
        p->surface_pressure_max = m;
    }
    if (he != hipSuccess) return failHip("download", he);
    const auto t3 = clock::now();
    p->setup_ms = SlabCall::ms(t0, t1);
    p->solve_ms = SlabCall::ms(t1, t2);
    p->total_ms = SlabCall::ms(t0, t3);
    if (solveRc != MGPS_OK) setLastGlobalError("mgps_project_free_surface: interrupted");
    return solveRc;
}
MGPS_API_CATCH(nullptr)

}  // extern "C"

// ---- the fields layer on Z-slabs (include/mgps_fields.h) ---------------------------------------------------
// Kernels for a z-window of the grid: one thread per cell (or per face triple) of a (ceil(nx / 256), ny, planes) launch, so the
// index costs no 64-bit division.  What a pass reads of a neighbour rank's planes arrives in halo planes; a neighbour outside the
// WHOLE grid is ignored, as the whole-grid kernels ignore it.  The per-cell arithmetic is that of the kernels above (ghostFluidTheta,
// cellDivergence, surfacePressureAt, interfacePressure).
namespace {
struct Slab {
    int gx, gy, gz, c0, c1, ex, ey, ez, off, e0, e1;
    __host__ __device__ Box whole() const { return Box{gx, gy, gz}; }        // the base grid
    __host__ __device__ Box base() const { return Box{gx, gy, c1 - c0}; }    // the window of the base grid
    __host__ __device__ Box window() const { return Box{ex, ey, e1 - e0}; }  // the window of the expanded grid
};
// a window of a base cell grid with the neighbours' planes next to it
template <class T>
struct Planes {
    const T *own, *lo, *hi;
};
// value at base cell (i, j, kg), kg a plane of the whole grid in [c0 - 1, c1] (callers never ask for a plane outside the grid)
template <class T>
__device__ __forceinline__ T zAt(const Slab &s, const Planes<T> &p, int i, int j, int kg)
{
    const size_t ij = size_t(j) * s.gx + i;
    if (kg < s.c0) return p.lo[ij];
    if (kg >= s.c1) return p.hi[ij];
    return p.own[size_t(kg - s.c0) * s.gy * s.gx + ij];
}
// how the slab kernels hand a grid to a rule (GridAt's counterpart)
template <class T>
struct SlabAt {
    const Slab &s;
    const Planes<T> &p;
    __device__ __forceinline__ T operator()(int i, int j, int kg) const { return zAt(s, p, i, j, kg); }
};

__global__ __launch_bounds__(256) void materialLabelsSlabKernel(Slab s, int32_t *__restrict__ material, Planes<float> phi,
                                                                const float *__restrict__ solidPhi, const float *__restrict__ cwx,
                                                                const float *__restrict__ cwy, const float *__restrict__ cwz)
{
    int i, j, k;
    threadCell(i, j, k);
    if (i >= s.gx) return;
    const Box g = s.base();
    const float *cw[3] = {cwx, cwy, cwz};
    material[cellAt(g, i, j, k)] = materialLabel(s.whole(), g, i, j, k, s.c0 + k, phi.own, solidPhi, cw, SlabAt<float>{s, phi});
}

// valid flag and expanded weight of the base face of `axis` in front of base cell (bi, bj, bkg)
__device__ __forceinline__ float faceWeight(const Slab &s, int axis, int bi, int bj, int bkg, float cwf, const Planes<int32_t> &mat,
                                            const Planes<float> &phi, uint8_t &valid)
{
    int mb, mf;
    valid = isValidFace(s.whole(), axis, bi, bj, bkg, cwf, SlabAt<int32_t>{s, mat}, mb, mf);
    return valid ? expandedWeight(axis, bi, bj, bkg, cwf, mb, mf, SlabAt<float>{s, phi}) : 0.f;
}

// One thread per (i, j, k) of the window's expanded face grids, (ex + 1) x (ey + 1) x (planes + 1): the x-, y- and z-face in front of
// expanded cell (i, j, e0 + k).  Writes the three expanded weights everywhere (0 outside the base box) and the valid flags.
__global__ __launch_bounds__(256) void facesSlabKernel(Slab s, uint8_t *__restrict__ vx, uint8_t *__restrict__ vy, uint8_t *__restrict__ vz,
                                                       float *__restrict__ wx, float *__restrict__ wy, float *__restrict__ wz,
                                                       Planes<int32_t> mat, Planes<float> phi, const float *__restrict__ cwx,
                                                       const float *__restrict__ cwy, const float *__restrict__ cwz)
{
    int i, j, k;
    threadCell(i, j, k);
    if (i > s.ex) return;
    const Box g = s.base(), e = s.window();
    const int bi = i - s.off, bj = j - s.off, bkg = s.e0 + k - s.off, bk = bkg - s.c0;
    const bool inX = bi >= 0 && bi < s.gx, inY = bj >= 0 && bj < s.gy, inZ = bkg >= s.c0 && bkg < s.c1;
    uint8_t v;
    if (j < s.ey && k < e.gz) {  // x-face
        float w = 0.f;
        if (bi >= 0 && bi <= s.gx && inY && inZ) {
            const size_t f = faceAt(g, 0, bi, bj, bk);
            w = faceWeight(s, 0, bi, bj, bkg, cwx[f], mat, phi, v);
            vx[f] = v;
        }
        wx[faceAt(e, 0, i, j, k)] = w;
    }
    if (i < s.ex && k < e.gz) {  // y-face
        float w = 0.f;
        if (inX && bj >= 0 && bj <= s.gy && inZ) {
            const size_t f = faceAt(g, 1, bi, bj, bk);
            w = faceWeight(s, 1, bi, bj, bkg, cwy[f], mat, phi, v);
            vy[f] = v;
        }
        wy[faceAt(e, 1, i, j, k)] = w;
    }
    if (i < s.ex && j < s.ey) {  // z-face (the window holds the faces c0 .. c1)
        float w = 0.f;
        if (inX && inY && bkg >= s.c0 && bkg <= s.c1) {
            const size_t f = faceAt(g, 2, bi, bj, bk);
            w = faceWeight(s, 2, bi, bj, bkg, cwz[f], mat, phi, v);
            vz[f] = v;
        }
        wz[faceAt(e, 2, i, j, k)] = w;
    }
}

// domain label of base cell (bi, bj, bkg): EXTERIOR outside the base box (domainLabelsKernel + its fill)
__device__ __forceinline__ int domainLabelAt(const Slab &s, const Planes<int32_t> &mat, int bi, int bj, int bkg)
{
    if (bi < 0 || bi >= s.gx || bj < 0 || bj >= s.gy || bkg < 0 || bkg >= s.gz) return MGPS_EXTERIOR_CELL;
    return domainLabel(zAt(s, mat, bi, bj, bkg));
}

// domainLabelsKernel + setBoundaryLabelsKernel on the window: the neighbours' labels come from the material labels, so nothing
// is updated in place
__global__ __launch_bounds__(256) void labelsSlabKernel(Slab s, uint8_t *__restrict__ lab, Planes<int32_t> mat, const float *__restrict__ wx,
                                                        const float *__restrict__ wy, const float *__restrict__ wz)
{
    int i, j, k;
    threadCell(i, j, k);
    if (i >= s.ex) return;
    const Box e = s.window();
    const int bi = i - s.off, bj = j - s.off, bkg = s.e0 + k - s.off;
    int label = domainLabelAt(s, mat, bi, bj, bkg);
    if (label == MGPS_INTERIOR_CELL) {
        const float *w[3] = {wx, wy, wz};
        auto labelAcross = [&](int a, int d) {
            int n[3] = {bi, bj, bkg};
            n[a] += d ? 1 : -1;
            return domainLabelAt(s, mat, n[0], n[1], n[2]);
        };
        if (isBoundaryCell(e, i, j, k, w, labelAcross)) label = MGPS_BOUNDARY_CELL;
    }
    lab[cellAt(e, i, j, k)] = uint8_t(label);
}

// rhsKernel / pressureToSolutionKernel on the window's expanded planes, written everywhere
__global__ __launch_bounds__(256) void rhsSlabKernel(Slab s, float *__restrict__ rhs, const int32_t *__restrict__ material, const float *vx,
                                                     const float *vy, const float *vz, const float *svx, const float *svy, const float *svz,
                                                     const float *cwx, const float *cwy, const float *cwz)
{
    int i, j, k;
    threadCell(i, j, k);
    if (i >= s.ex) return;
    const Box g = s.base(), e = s.window();
    const int bi = i - s.off, bj = j - s.off, bk = s.e0 + k - s.off - s.c0;
    float out = 0.f;
    if (bi >= 0 && bi < g.gx && bj >= 0 && bj < g.gy && bk >= 0 && bk < g.gz && material[cellAt(g, bi, bj, bk)] == kLiquid) {
        const float *v[3] = {vx, vy, vz}, *sv[3] = {svx, svy, svz}, *cw[3] = {cwx, cwy, cwz};
        out = cellDivergence(g, bi, bj, bk, 1.f, v, sv, cw);
    }
    rhs[cellAt(e, i, j, k)] = out;
}

__global__ __launch_bounds__(256) void pressureToSolutionSlabKernel(Slab s, float *__restrict__ x, const float *__restrict__ pressure,
                                                                    const int32_t *__restrict__ material)
{
    int i, j, k;
    threadCell(i, j, k);
    if (i >= s.ex) return;
    const Box g = s.base(), e = s.window();
    const int bi = i - s.off, bj = j - s.off, bk = s.e0 + k - s.off - s.c0;
    float out = 0.f;
    if (bi >= 0 && bi < g.gx && bj >= 0 && bj < g.gy && bk >= 0 && bk < g.gz) {
        const size_t c = cellAt(g, bi, bj, bk);
        if (material[c] == kLiquid) out = pressure[c];
    }
    x[cellAt(e, i, j, k)] = out;
}

__global__ __launch_bounds__(256) void solutionToPressureSlabKernel(Slab s, float *__restrict__ pressure, const float *__restrict__ x,
                                                                    const int32_t *__restrict__ material, int clearOthers)
{
    int i, j, k;
    threadCell(i, j, k);
    if (i >= s.gx) return;
    const Box g = s.base(), e = s.window();
    const size_t c = cellAt(g, i, j, k);
    if (material[c] == kLiquid) pressure[c] = x[cellAt(e, i + s.off, j + s.off, s.c0 + k + s.off - s.e0)];
    else if (clearOthers) pressure[c] = 0.f;
}

// One thread per (i, j, k) of the window's base face grids, (gx + 1) x (gy + 1) x (planes + 1): the three faces in front of base
// cell (i, j, c0 + k).  A valid face has both cells inside the whole grid, so no halo is read past it.  sp.own == NULL gives the
// plain gradient.
__global__ __launch_bounds__(256) void pressureGradientSlabKernel(Slab s, float *__restrict__ velx, float *__restrict__ vely,
                                                                  float *__restrict__ velz, Planes<float> phi, Planes<float> pr,
                                                                  Planes<float> sp, const uint8_t *__restrict__ vx,
                                                                  const uint8_t *__restrict__ vy, const uint8_t *__restrict__ vz,
                                                                  Planes<int32_t> mat)
{
    int i, j, k;
    threadCell(i, j, k);
    if (i > s.gx) return;
    const Box g = s.base();
    const int kg = s.c0 + k;
    const bool surface = sp.own != nullptr;
    const SlabAt<int32_t> matAt{s, mat};
    const SlabAt<float> prAt{s, pr}, phiAt{s, phi}, spAt{s, sp};
    if (j < s.gy && k < g.gz) {
        const size_t f = faceAt(g, 0, i, j, k);
        if (vx[f]) velx[f] -= faceGradient(0, i, j, kg, surface, matAt, prAt, phiAt, spAt);
    }
    if (i < s.gx && k < g.gz) {
        const size_t f = faceAt(g, 1, i, j, k);
        if (vy[f]) vely[f] -= faceGradient(1, i, j, kg, surface, matAt, prAt, phiAt, spAt);
    }
    if (i < s.gx && j < s.gy) {
        const size_t f = faceAt(g, 2, i, j, k);
        if (vz[f]) velz[f] -= faceGradient(2, i, j, kg, surface, matAt, prAt, phiAt, spAt);
    }
}

__global__ __launch_bounds__(256) void surfacePressureSlabKernel(Slab s, float *__restrict__ sp, Planes<float> phi, Planes<int32_t> mat,
                                                                 double scale)
{
    int i, j, k;
    threadCell(i, j, k);
    if (i >= s.gx) return;
    const size_t c = cellAt(s.base(), i, j, k);
    sp[c] = surfacePressure(s.whole(), i, j, s.c0 + k, mat.own[c], scale, SlabAt<int32_t>{s, mat}, SlabAt<float>{s, phi});
}

// rhsSurfaceKernel on the window: the expanded weights are the window's (what facesSlabKernel wrote)
__global__ __launch_bounds__(256) void rhsSurfaceSlabKernel(Slab s, float *__restrict__ rhs, const float *wx, const float *wy, const float *wz,
                                                            Planes<float> phi, Planes<int32_t> mat, Planes<float> sp,
                                                            unsigned *__restrict__ pGammaMax)
{
    int bi, bj, bk;
    threadCell(bi, bj, bk);
    float amax = 0.f;
    // (no early return: every lane reaches the wave reduction below)
    const bool inside = bi < s.gx;
    const Box G = s.whole();
    const int kg = s.c0 + bk;
    const size_t c = inside ? cellAt(s.base(), bi, bj, bk) : 0;
    const int m = inside ? mat.own[c] : kSolid;
    const SlabAt<int32_t> matAt{s, mat};
    if (inside && isInterfaceCell(G, bi, bj, kg, m, matAt) && m == kLiquid) {
        const float *w[3] = {wx, wy, wz};
        const Box e = s.window();
        const int ei = bi + s.off, ej = bj + s.off, ek = kg + s.off - s.e0;
        auto wAcross = [&](int a, int d) { return w[a][cellFace(e, a, d, ei, ej, ek)]; };
        amax = addSurfaceRhs(G, bi, bj, kg, phi.own[c], sp.own[c], rhs[cellAt(e, ei, ej, ek)], wAcross, matAt, SlabAt<float>{s, phi},
                             SlabAt<float>{s, sp});
    }
    raisePGammaMax(pGammaMax, amax);
}

inline int clampInt(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
// the descriptor as the kernels take it; false with a message when it is not a window of a layout
bool readSlab(const mgps_fields_slab *d, Slab &s, const char *what)
{
    bool ok = d && d->struct_size == int(sizeof(mgps_fields_slab));
    if (ok) {
        s = Slab{d->gx, d->gy, d->gz, d->c0, d->c1, d->ex, d->ey, d->ez, d->offset, d->e0, d->e1};
        ok = okBox(s.gx, s.gy, s.gz) && okExpanded(s.gx, s.gy, s.gz, s.ex, s.ey, s.ez, s.off) && s.e0 >= 0 && s.e0 < s.e1 && s.e1 <= s.ez &&
             s.c0 == clampInt(s.e0 - s.off, 0, s.gz) && s.c1 == clampInt(s.e1 - s.off, 0, s.gz) && s.c0 < s.c1 &&
             s.ey + 1 <= 65535 && s.e1 - s.e0 + 1 <= 65535;  // (y and z extents are launch-grid dimensions)
    }
    if (!ok) setLastGlobalError(std::string(what) + ": not a slab window (struct_size, extents, c0 < c1 = the base planes of [e0, e1))");
    return ok;
}
// halo planes: present exactly where the whole grid goes on
template <class T>
bool okHalo(const Slab &s, const T *own, const T *lo, const T *hi)
{
    return own && (s.c0 == 0 || lo) && (s.c1 == s.gz || hi);
}
}  // namespace

namespace mgps {
bool fieldsSlabWindow(const mgps_fields_slab *d, const char *fn)
{
    Slab s;
    return readSlab(d, s, fn);
}
}  // namespace mgps

extern "C" {

int mgps_fields_slab_describe(mgps_fields_slab *out, int gx, int gy, int gz, int power_of_two, const int *splits, int size, int rank)
try {
    if (!out || !splits || size < 1 || rank < 0 || rank >= size) return bad("mgps_fields_slab_describe");
    int dims[3], offset = 0, levels = 0;
    if (int rc = mgps_expanded_layout(gx, gy, gz, 0, power_of_two, dims, &offset, &levels); rc != MGPS_OK) return rc;
    bool ok = splits[0] == 0 && splits[size] == dims[2];
    for (int r = 0; r < size && ok; ++r) ok = splits[r + 1] > splits[r];
    if (!ok) {
        setLastGlobalError("mgps_fields_slab_describe: the cuts must run from 0 to the expanded nz (" + std::to_string(dims[2]) + "), increasing");
        return MGPS_ERR_INVALID_ARGUMENT;
    }
    for (int r = 0; r < size; ++r)
        if (clampInt(splits[r] - offset, 0, gz) >= clampInt(splits[r + 1] - offset, 0, gz)) {
            setLastGlobalError("mgps_fields_slab_describe: rank " + std::to_string(r) + " owns no plane of the base grid (expanded planes " +
                               std::to_string(splits[r]) + " .. " + std::to_string(splits[r + 1]) + ", base planes at " + std::to_string(offset) +
                               " .. " + std::to_string(offset + gz) + "): see mgps_projection_slab_layout");
            return MGPS_ERR_INVALID_ARGUMENT;
        }
    *out = mgps_fields_slab{int(sizeof(mgps_fields_slab)), gx, gy, gz, clampInt(splits[rank] - offset, 0, gz), clampInt(splits[rank + 1] - offset, 0, gz),
                            dims[0], dims[1], dims[2], offset, splits[rank], splits[rank + 1]};
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

int mgps_projection_slab_layout(int gx, int gy, int gz, int power_of_two, int size, int use_gauss_seidel, int out_expanded[3],
                                int *out_offset, int *out_levels, int *out_splits)
try {
    if (!out_expanded || !out_offset || !out_levels || !out_splits || size < 1) return bad("mgps_projection_slab_layout");
    if (int rc = mgps_expanded_layout(gx, gy, gz, 0, power_of_two, out_expanded, out_offset, out_levels); rc != MGPS_OK) return rc;
    const int ez = out_expanded[2], off = *out_offset, unit = use_gauss_seidel ? 16 : 2, minPlanes = 16;
    auto refuse = [&](const std::string &why) {
        setLastGlobalError("mgps_projection_slab_layout: " + std::to_string(gz) + " base planes in " + std::to_string(ez) + " expanded planes cannot be cut for " +
                           std::to_string(size) + " ranks: " + why);
        return int(MGPS_ERR_INVALID_ARGUMENT);
    };
    if (ez % unit != 0) return refuse("the expanded grid is not a multiple of the cut granule " + std::to_string(unit));
    // Cuts on multiples of `unit`, every rank >= 16 planes and >= 1 base plane, minimising the sum of the squared base-plane counts
    // (the most even division the granule allows): a dynamic programme over the n = ez / unit cut positions.
    const int n = ez / unit;
    auto basePlanes = [&](int a, int b) { return clampInt(b * unit - off, 0, gz) - clampInt(a * unit - off, 0, gz); };
    const double kInf = 1e300;
    std::vector<std::vector<double>> best(size_t(size) + 1, std::vector<double>(size_t(n) + 1, kInf));
    std::vector<std::vector<int>> from(size_t(size) + 1, std::vector<int>(size_t(n) + 1, -1));
    best[0][0] = 0.0;
    for (int r = 1; r <= size; ++r)
        for (int b = 1; b <= n; ++b) {
            if (r == size && b != n) continue;
            for (int a = 0; a < b; ++a) {
                if (best[size_t(r) - 1][size_t(a)] >= kInf || (b - a) * unit < minPlanes) continue;
                const int planes = basePlanes(a, b);
                if (planes < 1) continue;
                const double cost = best[size_t(r) - 1][size_t(a)] + double(planes) * planes;
                if (cost < best[size_t(r)][size_t(b)]) {
                    best[size_t(r)][size_t(b)] = cost;
                    from[size_t(r)][size_t(b)] = a;
                }
            }
        }
    if (best[size_t(size)][size_t(n)] >= kInf)
        return refuse("every rank needs at least 16 expanded planes and one base plane, on cuts that are multiples of " + std::to_string(unit));
    for (int r = size, b = n; r > 0; --r) {
        out_splits[r] = b * unit;
        b = from[size_t(r)][size_t(b)];
    }
    out_splits[0] = 0;
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_material_labels(const mgps_fields_slab *d, int32_t *material, const float *liquid_phi, const float *phi_lo,
                                     const float *phi_hi, const float *solid_phi, const float *cwx, const float *cwy, const float *cwz,
                                     void *stream)
try {
    Slab s;
    if (!readSlab(d, s, "mgps_fields_slab_material_labels")) return MGPS_ERR_INVALID_ARGUMENT;
    if (!material || !okHalo(s, liquid_phi, phi_lo, phi_hi) || !solid_phi || !cwx || !cwy || !cwz) return bad("mgps_fields_slab_material_labels");
    materialLabelsSlabKernel<<<rowGrid(s.gx, s.gy, s.c1 - s.c0), 256, 0, static_cast<hipStream_t>(stream)>>>(
        s, material, Planes<float>{liquid_phi, phi_lo, phi_hi}, solid_phi, cwx, cwy, cwz);
    return done("mgps_fields_slab_material_labels");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_faces(const mgps_fields_slab *d, uint8_t *const valid[3], float *const expanded_weights[3], const int32_t *material,
                           const int32_t *material_lo, const int32_t *material_hi, const float *liquid_phi, const float *phi_lo,
                           const float *phi_hi, const float *const cut_weights[3], void *stream)
try {
    Slab s;
    if (!readSlab(d, s, "mgps_fields_slab_faces")) return MGPS_ERR_INVALID_ARGUMENT;
    bool ok = valid && expanded_weights && cut_weights && okHalo(s, material, material_lo, material_hi) && okHalo(s, liquid_phi, phi_lo, phi_hi);
    for (int a = 0; a < 3 && ok; ++a) ok = valid[a] && expanded_weights[a] && cut_weights[a];
    if (!ok) return bad("mgps_fields_slab_faces");
    facesSlabKernel<<<rowGrid(s.ex + 1, s.ey + 1, s.e1 - s.e0 + 1), 256, 0, static_cast<hipStream_t>(stream)>>>(
        s, valid[0], valid[1], valid[2], expanded_weights[0], expanded_weights[1], expanded_weights[2],
        Planes<int32_t>{material, material_lo, material_hi}, Planes<float>{liquid_phi, phi_lo, phi_hi}, cut_weights[0], cut_weights[1], cut_weights[2]);
    return done("mgps_fields_slab_faces");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_labels(const mgps_fields_slab *d, uint8_t *expanded_labels, const int32_t *material, const int32_t *material_lo,
                            const int32_t *material_hi, const float *const expanded_weights[3], void *stream)
try {
    Slab s;
    if (!readSlab(d, s, "mgps_fields_slab_labels")) return MGPS_ERR_INVALID_ARGUMENT;
    if (!expanded_labels || !okHalo(s, material, material_lo, material_hi) || !expanded_weights || !expanded_weights[0] || !expanded_weights[1] ||
        !expanded_weights[2])
        return bad("mgps_fields_slab_labels");
    labelsSlabKernel<<<rowGrid(s.ex, s.ey, s.e1 - s.e0), 256, 0, static_cast<hipStream_t>(stream)>>>(
        s, expanded_labels, Planes<int32_t>{material, material_lo, material_hi}, expanded_weights[0], expanded_weights[1], expanded_weights[2]);
    return done("mgps_fields_slab_labels");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_rhs(const mgps_fields_slab *d, float *expanded_rhs, const int32_t *material, const float *const velocity[3],
                         const float *const solid_velocity[3], const float *const cut_weights[3], void *stream)
try {
    Slab s;
    if (!readSlab(d, s, "mgps_fields_slab_rhs")) return MGPS_ERR_INVALID_ARGUMENT;
    const float *sv[3] = {solid_velocity ? solid_velocity[0] : nullptr, solid_velocity ? solid_velocity[1] : nullptr, solid_velocity ? solid_velocity[2] : nullptr};
    bool ok = expanded_rhs && material && velocity && cut_weights && (!(sv[0] || sv[1] || sv[2]) || (sv[0] && sv[1] && sv[2]));
    for (int a = 0; a < 3 && ok; ++a) ok = velocity[a] && cut_weights[a];
    if (!ok) return bad("mgps_fields_slab_rhs");
    rhsSlabKernel<<<rowGrid(s.ex, s.ey, s.e1 - s.e0), 256, 0, static_cast<hipStream_t>(stream)>>>(
        s, expanded_rhs, material, velocity[0], velocity[1], velocity[2], sv[0], sv[1], sv[2], cut_weights[0], cut_weights[1], cut_weights[2]);
    return done("mgps_fields_slab_rhs");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_pressure_to_solution(const mgps_fields_slab *d, float *expanded_x, const float *pressure, const int32_t *material,
                                          void *stream)
try {
    Slab s;
    if (!readSlab(d, s, "mgps_fields_slab_pressure_to_solution")) return MGPS_ERR_INVALID_ARGUMENT;
    if (!expanded_x || !pressure || !material) return bad("mgps_fields_slab_pressure_to_solution");
    pressureToSolutionSlabKernel<<<rowGrid(s.ex, s.ey, s.e1 - s.e0), 256, 0, static_cast<hipStream_t>(stream)>>>(s, expanded_x, pressure, material);
    return done("mgps_fields_slab_pressure_to_solution");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_solution_to_pressure(const mgps_fields_slab *d, float *pressure, const float *expanded_x, const int32_t *material,
                                          int clear_others, void *stream)
try {
    Slab s;
    if (!readSlab(d, s, "mgps_fields_slab_solution_to_pressure")) return MGPS_ERR_INVALID_ARGUMENT;
    if (!pressure || !expanded_x || !material) return bad("mgps_fields_slab_solution_to_pressure");
    solutionToPressureSlabKernel<<<rowGrid(s.gx, s.gy, s.c1 - s.c0), 256, 0, static_cast<hipStream_t>(stream)>>>(s, pressure, expanded_x, material,
                                                                                                                 clear_others);
    return done("mgps_fields_slab_solution_to_pressure");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_pressure_gradient(const mgps_fields_slab *d, float *const velocity[3], const float *liquid_phi, const float *phi_lo,
                                       const float *phi_hi, const float *pressure, const float *pressure_lo, const float *pressure_hi,
                                       const float *sp, const float *sp_lo, const float *sp_hi, const uint8_t *const valid[3],
                                       const int32_t *material, const int32_t *material_lo, const int32_t *material_hi, void *stream)
try {
    Slab s;
    if (!readSlab(d, s, "mgps_fields_slab_pressure_gradient")) return MGPS_ERR_INVALID_ARGUMENT;
    bool ok = velocity && valid && okHalo(s, liquid_phi, phi_lo, phi_hi) && okHalo(s, pressure, pressure_lo, pressure_hi) &&
              okHalo(s, material, material_lo, material_hi) && (!sp || okHalo(s, sp, sp_lo, sp_hi));
    for (int a = 0; a < 3 && ok; ++a) ok = velocity[a] && valid[a];
    if (!ok) return bad("mgps_fields_slab_pressure_gradient");
    pressureGradientSlabKernel<<<rowGrid(s.gx + 1, s.gy + 1, s.c1 - s.c0 + 1), 256, 0, static_cast<hipStream_t>(stream)>>>(
        s, velocity[0], velocity[1], velocity[2], Planes<float>{liquid_phi, phi_lo, phi_hi}, Planes<float>{pressure, pressure_lo, pressure_hi},
        Planes<float>{sp, sp_lo, sp_hi}, valid[0], valid[1], valid[2], Planes<int32_t>{material, material_lo, material_hi});
    return done("mgps_fields_slab_pressure_gradient");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_surface_pressure(const mgps_fields_slab *d, float *sp, const float *liquid_phi, const float *phi_lo,
                                      const float *phi_hi, const int32_t *material, const int32_t *material_lo, const int32_t *material_hi,
                                      double scale, void *stream)
try {
    Slab s;
    if (!readSlab(d, s, "mgps_fields_slab_surface_pressure")) return MGPS_ERR_INVALID_ARGUMENT;
    if (!sp || !okHalo(s, liquid_phi, phi_lo, phi_hi) || !okHalo(s, material, material_lo, material_hi)) return bad("mgps_fields_slab_surface_pressure");
    surfacePressureSlabKernel<<<rowGrid(s.gx, s.gy, s.c1 - s.c0), 256, 0, static_cast<hipStream_t>(stream)>>>(
        s, sp, Planes<float>{liquid_phi, phi_lo, phi_hi}, Planes<int32_t>{material, material_lo, material_hi}, scale);
    return done("mgps_fields_slab_surface_pressure");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_rhs_surface(const mgps_fields_slab *d, float *expanded_rhs, const float *const expanded_weights[3],
                                 const float *liquid_phi, const float *phi_lo, const float *phi_hi, const int32_t *material,
                                 const int32_t *material_lo, const int32_t *material_hi, const float *sp, const float *sp_lo,
                                 const float *sp_hi, float *p_gamma_max, void *stream)
try {
    Slab s;
    if (!readSlab(d, s, "mgps_fields_slab_rhs_surface")) return MGPS_ERR_INVALID_ARGUMENT;
    if (!expanded_rhs || !expanded_weights || !expanded_weights[0] || !expanded_weights[1] || !expanded_weights[2] ||
        !okHalo(s, liquid_phi, phi_lo, phi_hi) || !okHalo(s, material, material_lo, material_hi) || !okHalo(s, sp, sp_lo, sp_hi))
        return bad("mgps_fields_slab_rhs_surface");
    rhsSurfaceSlabKernel<<<rowGrid(s.gx, s.gy, s.c1 - s.c0), 256, 0, static_cast<hipStream_t>(stream)>>>(
        s, expanded_rhs, expanded_weights[0], expanded_weights[1], expanded_weights[2], Planes<float>{liquid_phi, phi_lo, phi_hi},
        Planes<int32_t>{material, material_lo, material_hi}, Planes<float>{sp, sp_lo, sp_hi}, reinterpret_cast<unsigned *>(p_gamma_max));
    return done("mgps_fields_slab_rhs_surface");
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_divergence(const mgps_fields_slab *d, double out_host[3], const int32_t *material, const float *const velocity[3],
                                const float *const solid_velocity[3], const float *const cut_weights[3], void *stream)
try {
    Slab s;
    if (!readSlab(d, s, "mgps_fields_slab_divergence")) return MGPS_ERR_INVALID_ARGUMENT;
    if (!velocity || !cut_weights) return bad("mgps_fields_slab_divergence");
    // every face of an owned cell is in the window (the z-face grid closes with plane c1): the window is a box of its own here
    return mgps_fields_divergence(out_host, material, velocity[0], velocity[1], velocity[2], solid_velocity ? solid_velocity[0] : nullptr,
                                  solid_velocity ? solid_velocity[1] : nullptr, solid_velocity ? solid_velocity[2] : nullptr, cut_weights[0],
                                  cut_weights[1], cut_weights[2], s.gx, s.gy, s.c1 - s.c0, stream);
}
MGPS_API_CATCH(nullptr)

}  // extern "C"

// ---- one-call projection on slab ranks (mgps_project_free_surface_slab) -----------------------------------------------------------
namespace {
// a HIP call of a slab one-call (mgps_slab_call.h): its failure is the rank's own and travels in the next agreement
void hipStep(SlabCall &c, hipError_t e, const char *what)
{
    if (e != hipSuccess) c.fail(MGPS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
// The transport the slab solver of a world of one gets instead of the caller's, so that the one-call keeps its word -- with
// comm->size = 1 no entry of the caller's transport is called -- through the constructor and the solve as well: nobody to trade
// with, reductions over one rank are the identity, a gather or scatter is a device copy that synchronises the stream and blocks.
int soloCopy(void *dst, const void *src, size_t bytes, void *stream)
{
    if (!bytes || dst == src) return 0;
    if (hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess) return 1;
    return hipMemcpy(dst, src, bytes, hipMemcpyDefault) == hipSuccess ? 0 : 1;
}
mgps_comm soloComm()
{
    mgps_comm cm{};
    cm.struct_size = int(sizeof(mgps_comm));
    cm.rank = 0, cm.size = 1;
    cm.exchange = [](void *, const void *, size_t, void *, size_t, const void *, size_t, void *, size_t, void *) { return 0; };
    cm.allreduce = [](void *, double *, int, int) { return 0; };
    cm.gather = [](void *, const void *send, void *recv, size_t bytes, int, void *stream) { return soloCopy(recv, send, bytes, stream); };
    cm.scatter = [](void *, const void *send, void *recv, size_t bytes, int, void *stream) { return soloCopy(recv, send, bytes, stream); };
    cm.gatherv = [](void *, const void *send, size_t bytes, void *recv, const size_t *, const size_t *displs, int, void *stream) {
        return soloCopy(static_cast<char *>(recv) + (bytes ? displs[0] : 0), send, bytes, stream);
    };
    cm.scatterv = [](void *, const void *send, const size_t *, const size_t *displs, void *recv, size_t bytes, int, void *stream) {
        return soloCopy(recv, static_cast<const char *>(send) + (bytes ? displs[0] : 0), bytes, stream);
    };
    cm.allreduce_device = [](void *, double *, int, int, void *) { return 0; };
    cm.exchange2 = [](void *, const mgps_xfer2 *, const mgps_xfer2 *, const mgps_xfer2 *, const mgps_xfer2 *, void *) { return 0; };
    return cm;
}
// (the checks of the bodies' count and host tables, stated with the pressure feedback and the coupling further down)
int forceCheckBodies(const char *fn, int bodies);
int coupleCheckBodies(const char *fn, int bodies, const double *centres, const double *invMass, const double *invInertia);

// The sequence of mgps_project_free_surface_slab and mgps_project_free_surface_rigid_slab, stated once.  r: the rigid block, or NULL
// for the plain call -- then no launch, transport call, message or result differs from what the sequence was without it.  With r
// (DESIGN.md section 17.2): the bodies' count travels in the first agreement; after the solver, the rank's coupling object and one
// more agreement (it carries the coupled cells' count), then what the coupled solve refuses, asked before any output but the valid
// faces is touched; sv = the base solid velocity with V* on the bodies' faces feeds the right-hand side; the solve is
// mgps_solve_pcg_coupled and its residual loses G K G^T x; V_out and the impulses come from one more collective and V_out goes over
// sv in front of the divergence report.
int projectFreeSurfaceSlab(const char *fn, mgps_projection_slab *p, mgps_projection_rigid_slab *r, const mgps_options *opt, const mgps_comm *comm,
                           const int *splits, void *stream)
{
    using clock = SlabCall::Clock;
    SlabCall c;
    const auto t0 = c.t0;
    // ---- what every rank shares: a refusal here is every rank's, before any collective
    if (!p || p->struct_size != int(sizeof(mgps_projection_slab))) return refuse(fn, "NULL or struct_size mismatch");
    if (int rc = c.open(fn, comm, splits, offsetof(mgps_comm, gatherv)); rc != MGPS_OK) return rc;
    const mgps_comm &cm = c.cm;
    const int P = c.P, rank = c.rank;
    if (P > 1 && (!cm.gatherv || !cm.scatterv))
        return refuse(fn, "the collapse of uneven cuts and the enclosed-liquid merge go through gatherv and scatterv (and, with host_setup, the whole grid's labels): the transport has none");
    const size_t tableDoubles = r ? size_t(r->bodies + 1) * 6 : 0;
    if (r) {
        if (int rc = forceCheckBodies(fn, r->bodies); rc != MGPS_OK) return rc;
        if (int rc = coupleCheckBodies(fn, r->bodies, r->centres, r->inv_mass, r->inv_inertia); rc != MGPS_OK) return rc;
        if (!r->motions) return refuse(fn, "motions is NULL");
        if (!r->motions_out) return refuse(fn, "motions_out is NULL");
        const int given = (r->solid_velocity_out[0] != nullptr) + (r->solid_velocity_out[1] != nullptr) + (r->solid_velocity_out[2] != nullptr);
        if (given != 0 && given != 3) return refuse(fn, "solid_velocity_out: all three or none");
        r->coupled_cells = r->coupled_cells_rank = 0;
    }
    mgps_options o;
    if (int rc = readOptions(opt, o, (std::string(fn) + ": ").c_str()); rc != MGPS_OK) return rc;
    mgps_fields_slab desc;
    if (int rc = mgps_fields_slab_describe(&desc, p->gx, p->gy, p->gz, p->power_of_two, splits, P, rank); rc != MGPS_OK) return rc;
    Slab s;
    if (!readSlab(&desc, s, fn)) return MGPS_ERR_INVALID_ARGUMENT;
    int levels = 0;
    {
        int dims[3], off;
        (void)mgps_expanded_layout(p->gx, p->gy, p->gz, 0, p->power_of_two, dims, &off, &levels);
    }
    const int gx = s.gx, gy = s.gy, nzl = s.c1 - s.c0, ex = s.ex, ey = s.ey, ez = s.ez, nze = s.e1 - s.e0;
    const bool lo = s.c0 > 0, hi = s.c1 < s.gz;  // a neighbour with base planes on that side (every rank has some)
    const size_t plane = size_t(gx) * gy, cells = plane * size_t(nzl), eplane = size_t(ex) * ey, ecells = eplane * size_t(ez);
    // the solver is built from the rank's own label planes (mgps_create_slab_device_labels).  The host builder needs the whole
    // grid's labels on every rank's host: with it they are gathered and broadcast as before (options and environment are everybody's)
    const bool labelsToHosts = hostSetupRequested(o);
    hipStream_t st = static_cast<hipStream_t>(stream);
    p->mg_levels = levels;
    p->offset = s.off;
    p->expanded[0] = ex;
    p->expanded[1] = ey;
    p->expanded[2] = ez;
    p->liquid_cells = 0;
    clearReport(p);
    p->setup_ms = p->solve_ms = p->total_ms = 0;
    std::fill(p->stage_ms, p->stage_ms + 8, 0.0);

    // ---- this rank's own arguments and buffers: a failure is carried by the first all-reduce
    const double sigma = p->surface_tension;
    const bool surface = sigma > 0 || p->surface_pressure;
    const bool haveSolidVel = p->solid_velocity[0] && p->solid_velocity[1] && p->solid_velocity[2];
    DevPool pool;
    int32_t *material = nullptr;  // [lo plane | owned planes | hi plane]
    float *phiHalo = nullptr, *prHalo = nullptr, *spHalo = nullptr, *spOwn = nullptr, *w[3] = {nullptr, nullptr, nullptr}, *pGammaMax = nullptr;
    float *sv[3] = {nullptr, nullptr, nullptr};  // rigid: the solid velocity the right-hand side and the report see
    uint8_t *valid[3] = {nullptr, nullptr, nullptr}, *labelsAll = nullptr;
    unsigned long long *count = nullptr;
    void *labelsHost = nullptr;
    struct HostBlock {
        void *&p;
        ~HostBlock() { mgps_host_free(p); }
    } hostBlock{labelsHost};
    c.step([&]() -> int {
        if (int rc = checkProjectionFields(p, fn, true, "missing field"); rc != MGPS_OK) return rc;
        if (r && !(r->body[0] && r->body[1] && r->body[2])) return refuse(fn, "body: three grids are required");
        if (int rc = selectDevice(o.device); rc != MGPS_OK) return rc;
        try {
            material = pool.get<int32_t>(cells + 2 * plane);
            phiHalo = pool.get<float>(2 * plane);
            prHalo = pool.get<float>(2 * plane);
            if (surface) spHalo = pool.get<float>(2 * plane);
            if (sigma > 0) spOwn = pool.get<float>(cells);
            if (surface) pGammaMax = pool.get<float>(1);
            for (int a = 0; a < 3; ++a) {
                valid[a] = p->valid_faces[a] ? p->valid_faces[a] : pool.get<uint8_t>(faceCount(gx, gy, nzl, a));
                w[a] = pool.get<float>(faceCount(ex, ey, nze, a));
                if (r) sv[a] = r->solid_velocity_out[a] ? r->solid_velocity_out[a] : pool.get<float>(faceCount(gx, gy, nzl, a));
            }
            // the labels pass writes the rank's window: a buffer of its own, or (host set-up) in place in the whole grid's labels
            labelsAll = pool.get<uint8_t>(labelsToHosts ? ecells : size_t(nze) * eplane);
            count = pool.get<unsigned long long>(1);
        } catch (const std::bad_alloc &) {
            return c.fail(MGPS_ERR_ALLOC, "device allocation failed");
        }
        if (labelsToHosts) labelsHost = mgps_host_alloc(ecells);
        if (labelsToHosts && !labelsHost) return c.fail(MGPS_ERR_ALLOC, "host allocation of the whole grid's labels failed");
        return MGPS_OK;
    }());
    {
        // (both flags set on some rank: the ranks disagree; rigid: the largest and the smallest count of bodies)
        double flags[4] = {surface ? 1.0 : 0.0, surface ? 0.0 : 1.0, r ? double(r->bodies) : 0.0, r ? -double(r->bodies) : 0.0};
        if (int rc = c.agree("arguments", nullptr, 0, flags, r ? 4 : 2); rc != MGPS_OK) return rc;
        if (flags[0] != 0 && flags[1] != 0) return refuse(fn, "surface tension / surface_pressure is set on some ranks only");
        if (flags[2] != -flags[3])
            return refuse(fn, "bodies differs between the ranks (" + std::to_string(int(-flags[3])) + " .. " + std::to_string(int(flags[2])) + ")");
    }
    // (from here on the buffers exist on every rank: a failing rank still takes part in every exchange, with whatever its buffers
    //  hold, and the next agreement carries its status)
    // trade one plane with each neighbour: own first plane down, own last plane up; what arrives lands in halo[0] / halo[1]
    auto tradePlane = [&](const void *own, void *haloLo, void *haloHi, size_t elem, const char *what) -> int {
        const size_t bytes = plane * elem;
        const char *first = static_cast<const char *>(own), *last = first + size_t(nzl - 1) * bytes;
        return c.trade(lo ? first : nullptr, lo ? bytes : 0, lo ? haloLo : nullptr, lo ? bytes : 0, hi ? last : nullptr, hi ? bytes : 0,
                       hi ? haloHi : nullptr, hi ? bytes : 0, st, what);
    };
#define SLAB_COMM(call)                 \
    do {                                \
        const int rc_ = (call);         \
        if (rc_ != MGPS_OK) return rc_; \
    } while (0)
    const float *cw[3] = {p->cut_weights[0], p->cut_weights[1], p->cut_weights[2]};
    const float *svel[3];
    for (int a = 0; a < 3; ++a) svel[a] = r ? sv[a] : haveSolidVel ? p->solid_velocity[a] : nullptr;
    // rigid: sv = the caller's solid velocity (or zeros) with `motions` on the faces the bodies own; again: those faces only
    auto rigidSolidVelocity = [&](const double *motions, bool again) {
        for (int a = 0; a < 3 && !again && c.status == MGPS_OK; ++a) {
            const size_t bytes = faceCount(gx, gy, nzl, a) * sizeof(float);
            if (!haveSolidVel) hipStep(c, hipMemsetAsync(sv[a], 0, bytes, st), "solid velocity");
            else if (sv[a] != p->solid_velocity[a]) hipStep(c, hipMemcpyAsync(sv[a], p->solid_velocity[a], bytes, hipMemcpyDeviceToDevice, st), "solid velocity");
        }
        if (c.status == MGPS_OK) c.step(mgps_fields_slab_rigid_velocity(&desc, sv, r->body, r->centres, motions, r->bodies, st));
    };
    int32_t *matOwn = material + plane, *matLo = lo ? material : nullptr, *matHi = hi ? matOwn + cells : nullptr;
    float *phiLo = lo ? phiHalo : nullptr, *phiHi = hi ? phiHalo + plane : nullptr;
    // ---- 1. phi plane, material labels, material plane, the faces pass and the labels pass (Plug.cpp:270-362)
    SLAB_COMM(tradePlane(p->liquid_phi, phiHalo, phiHalo + plane, sizeof(float), "liquid_phi"));
    if (c.status == MGPS_OK) c.step(mgps_fields_slab_material_labels(&desc, matOwn, p->liquid_phi, phiLo, phiHi, p->solid_phi, cw[0], cw[1], cw[2], st));
    SLAB_COMM(tradePlane(matOwn, material, matOwn + cells, sizeof(int32_t), "material labels"));
    uint8_t *labelsWin = labelsToHosts ? labelsAll + size_t(s.e0) * eplane : labelsAll;
    if (c.status == MGPS_OK) c.step(mgps_fields_slab_faces(&desc, valid, w, matOwn, matLo, matHi, p->liquid_phi, phiLo, phiHi, cw, st));
    if (c.status == MGPS_OK) c.step(mgps_fields_slab_labels(&desc, labelsWin, matOwn, matLo, matHi, w, st));
    // ---- 2. liquid cells over all ranks; a domain without liquid has nothing to solve (the single-device rule)
    double liquid = 0;
    if (c.status == MGPS_OK) {
        unsigned long long mine = 0;
        hipStep(c, hipMemsetAsync(count, 0, sizeof(unsigned long long), st), "liquid cell count");
        if (c.status == MGPS_OK) {
            countLiquidKernel<<<unsigned(std::min<size_t>((cells + 255) / 256, 4096)), 256, 0, st>>>(matOwn, cells, count);
            hipStep(c, hipMemcpyAsync(&mine, count, sizeof(mine), hipMemcpyDeviceToHost, st), "liquid cell count");
            hipStep(c, hipStreamSynchronize(st), "field passes");
        }
        liquid = double(mine);
    }
    SLAB_COMM(c.agree("field passes", &liquid, 1));
    p->liquid_cells = liquid;
    const auto t1 = clock::now();
    p->stage_ms[0] = SlabCall::ms(t0, t1);
    if (liquid == 0) {
        hipStep(c, hipMemsetAsync(p->pressure, 0, cells * sizeof(float), st), "pressure clear");
        if (r && r->solid_velocity_out[0]) rigidSolidVelocity(r->motions, false);
        hipStep(c, hipStreamSynchronize(st), "pressure clear");
        SLAB_COMM(c.agree("pressure clear"));
        if (r) {  // nothing pushes back: V_out = V*
            std::copy(r->motions, r->motions + tableDoubles, r->motions_out);
            if (r->impulses) std::fill(r->impulses, r->impulses + tableDoubles, 0.0);
        }
        p->stage_ms[6] = c.exchangeMs;
        p->setup_ms = p->total_ms = SlabCall::ms(t0, clock::now());
        p->stats.outcome = MGPS_PCG_RHS_ZERO;
        return MGPS_OK;
    }
    // ---- 3. the ranks agree that the passes went through (the constructor is a collective).  Host set-up only: the whole grid's
    //         labels on every rank's host -- gatherv to rank 0 (every window already sits at its place of the rank's whole-grid
    //         buffer), then scatterv with every other rank's range set to the whole buffer, a broadcast
    if (labelsToHosts && P > 1) {
        std::vector<size_t> counts(static_cast<size_t>(P), 0), displs(static_cast<size_t>(P), 0);
        for (int r = 0; r < P; ++r) {
            counts[size_t(r)] = r == 0 ? 0 : size_t(splits[r + 1] - splits[r]) * eplane;  // (rank 0's window is in place)
            displs[size_t(r)] = size_t(splits[r]) * eplane;
        }
        if (cm.gatherv(cm.user, labelsWin, rank == 0 ? 0 : size_t(nze) * eplane, rank == 0 ? labelsAll : nullptr, counts.data(), displs.data(), 0, st) != 0)
            return c.leave(MGPS_ERR_COMM, "gatherv of the labels failed");
        for (int r = 0; r < P; ++r) {
            counts[size_t(r)] = r == 0 ? 0 : ecells;
            displs[size_t(r)] = 0;
        }
        if (cm.scatterv(cm.user, rank == 0 ? labelsAll : nullptr, counts.data(), displs.data(), labelsAll, rank == 0 ? 0 : ecells, 0, st) != 0)
            return c.leave(MGPS_ERR_COMM, "scatterv of the labels failed");
    }
    if (labelsToHosts) {
        hipStep(c, hipMemcpyAsync(labelsHost, labelsAll, ecells, hipMemcpyDeviceToHost, st), "labels to the host");
        hipStep(c, hipStreamSynchronize(st), "labels to the host");
    }
    SLAB_COMM(c.agree(labelsToHosts ? "labels to the host" : "labels"));
    const auto t2 = clock::now();
    p->stage_ms[1] = SlabCall::ms(t1, t2);
    // ---- 4. the slab solver on the rank's expanded weights (borrowed: the pool outlives the solver), rhs, warm start, surface
    //         term, enclosed-liquid projection, MG-PCG (Plug.cpp:386-629)
    mgps_solver *mg = nullptr;
    o.borrow_device_weights = 1;
    const mgps_comm solo = soloComm(), *solverComm = P == 1 ? &solo : &cm;  // (the solver copies it)
    if (int rc = labelsToHosts ? mgps_create_slab_device_weights(&mg, ex, ey, ez, static_cast<const uint8_t *>(labelsHost), w[0], w[1], w[2], levels,
                                                                 p->use_gauss_seidel, &o, solverComm, splits)
                               : mgps_create_slab_device_labels(&mg, ex, ey, ez, labelsWin, w[0], w[1], w[2], levels, p->use_gauss_seidel, &o, solverComm, splits);
        rc != MGPS_OK)
        return rc;  // (a collective with one verdict)
    struct Guard {
        mgps_solver *h;
        ~Guard() { mgps_destroy(h); }
    } guard{mg};
    // rigid: the rank's coupling object (its failure is the rank's own), the whole grid's count, and what the coupled solve refuses
    // -- every rank alike -- while pressure, velocity and solid_velocity_out still hold what they held
    mgps_coupling *cpl = nullptr;
    struct CouplingGuard {
        mgps_coupling *&h;
        ~CouplingGuard() { mgps_coupling_destroy(h); }
    } couplingGuard{cpl};
    if (r) {
        int64_t mine = 0;
        if (c.status == MGPS_OK) {
            mgps_coupling_desc cd{};
            cd.struct_size = int(sizeof(cd));
            cd.gx = s.gx, cd.gy = s.gy, cd.gz = s.gz, cd.ex = ex, cd.ey = ey, cd.ez = ez, cd.offset = s.off, cd.bodies = r->bodies;
            cd.material = matOwn;
            for (int a = 0; a < 3; ++a) cd.cut_weights[a] = cw[a], cd.body[a] = r->body[a];
            cd.centres = r->centres, cd.inv_mass = r->inv_mass, cd.inv_inertia = r->inv_inertia;
            c.step(mgps_coupling_create_slab(&cpl, &cd, &desc, &cm, st));
            if (c.status == MGPS_OK) c.step(mgps_coupling_cells(cpl, &mine));
        }
        double all = double(mine);
        SLAB_COMM(c.agree("coupling", &all, 1));
        r->coupled_cells = int64_t(all);
        r->coupled_cells_rank = mine;
        if (int rc = coupledSolveRefusal(mg, cpl, "mgps_solve_pcg_coupled"); rc != MGPS_OK) {
            setLastGlobalError(mgps_last_error(mg));
            return rc;
        }
    }
    const auto t3 = clock::now();
    p->stage_ms[2] = SlabCall::ms(t2, t3);
    float *rhs = nullptr, *x = nullptr, *res = nullptr, *gkg = nullptr;
    const float *sp = p->surface_pressure ? p->surface_pressure : spOwn;
    float *spLo = surface && lo ? spHalo : nullptr, *spHi = surface && hi ? spHalo + plane : nullptr;
    const float *velIn[3] = {p->velocity[0], p->velocity[1], p->velocity[2]};
    auto solverStep = [&](int rc) {
        if (rc != MGPS_OK && c.status == MGPS_OK) {
            setLastGlobalError(mgps_last_error(mg));
            c.status = rc;
        }
    };
    solverStep(mgps_set_stream(mg, stream));
    if (c.status == MGPS_OK) solverStep(mgps_grid_alloc(mg, 0, &rhs));
    if (c.status == MGPS_OK) solverStep(mgps_grid_alloc(mg, 0, &x));  // zero-filled
    if (c.status == MGPS_OK) solverStep(mgps_grid_alloc(mg, 0, &res));
    if (c.status == MGPS_OK && r) solverStep(mgps_grid_alloc(mg, 0, &gkg));
    if (r) rigidSolidVelocity(r->motions, false);
    if (c.status == MGPS_OK) c.step(mgps_fields_slab_rhs(&desc, rhs, matOwn, velIn, svel, cw, st));
    if (c.status == MGPS_OK && p->use_old_pressure) c.step(mgps_fields_slab_pressure_to_solution(&desc, x, p->pressure, matOwn, st));
    if (surface) {  // b_L += w_f p_G: before the enclosed-liquid projection and the solve, which then see the system actually solved
        if (c.status == MGPS_OK && sigma > 0)
            c.step(mgps_fields_slab_surface_pressure(&desc, spOwn, p->liquid_phi, phiLo, phiHi, matOwn, matLo, matHi, sigma * p->dt / (p->density * p->dx * p->dx), st));
        SLAB_COMM(tradePlane(sp, spHalo, spHalo + plane, sizeof(float), "surface pressure"));
        if (c.status == MGPS_OK) hipStep(c, hipMemsetAsync(pGammaMax, 0, sizeof(float), st), "surface pressure");
        if (c.status == MGPS_OK) c.step(mgps_fields_slab_rhs_surface(&desc, rhs, w, p->liquid_phi, phiLo, phiHi, matOwn, matLo, matHi, sp, spLo, spHi, pGammaMax, st));
    }
    SLAB_COMM(c.agree("right-hand side"));
    if (o.enclosed_liquid) {  // the rhs as the solve sees it (P b); both calls return one verdict on every rank
        int64_t m = 0;
        int rc = mgps_enclosed_components(mg, &m, nullptr);
        p->enclosed_components = int(m);
        if (rc == MGPS_OK && m > 0) rc = mgps_project_enclosed(mg, rhs, &p->rhs_mean_removed_max);
        if (rc != MGPS_OK) {
            setLastGlobalError(mgps_last_error(mg));
            return rc;
        }
    }
    (void)hipStreamSynchronize(st);
    const auto t4 = clock::now();
    p->stage_ms[3] = SlabCall::ms(t3, t4);
    int rc = r ? mgps_solve_pcg_coupled(mg, cpl, x, rhs, p->tolerance, p->max_iterations, p->use_mg_preconditioner, &p->stats)
               : mgps_solve_pcg(mg, x, rhs, p->tolerance, p->max_iterations, p->use_mg_preconditioner, &p->stats);
    if (rc == MGPS_OK) rc = mgps_residual(mg, 0, res, x, rhs);  // Plug.cpp:625-628
    if (rc == MGPS_OK && r) {  // the coupled system's: b - (A + G K G^T) x (a collective; its message is the library's already)
        if (int arc = mgps_coupling_apply(cpl, gkg, x, st); arc != MGPS_OK) return arc;
        rc = mgps_add_to_vector(mg, 0, res, gkg, -1.0);
    }
    if (rc == MGPS_OK) rc = mgps_inf_norm(mg, 0, res, 1, &p->residual_inf);
    if (rc == MGPS_OK) rc = mgps_l2_norm(mg, 0, res, &p->residual_l2);
    if (rc != MGPS_OK && rc != MGPS_ERR_INTERRUPTED) {
        setLastGlobalError(mgps_last_error(mg));
        return rc;
    }
    const int solveRc = rc;
    (void)hipStreamSynchronize(st);
    const auto t5 = clock::now();
    p->stage_ms[4] = SlabCall::ms(t4, t5);
    // ---- 5. pressure (0 outside LIQUID cells, Plug.cpp:641), its plane to the neighbours, the gradient on the owned faces -- the
    //         rank's copy of a cut's z-face plane included -- and the divergence report (Plug.cpp:637-707)
    if (r) {  // V_out and the impulses of the iterate handed back (a collective: every rank, whatever its status), V_out over sv
        const int vrc = mgps_coupling_velocities(cpl, x, r->motions, r->motions_out, r->impulses, st);
        if (vrc == MGPS_ERR_COMM) return vrc;
        c.step(vrc);
        rigidSolidVelocity(r->motions_out, true);
    }
    c.step(mgps_fields_slab_solution_to_pressure(&desc, p->pressure, x, matOwn, 1, st));
    SLAB_COMM(tradePlane(p->pressure, prHalo, prHalo + plane, sizeof(float), "pressure"));
    if (c.status == MGPS_OK)
        c.step(mgps_fields_slab_pressure_gradient(&desc, p->velocity, p->liquid_phi, phiLo, phiHi, p->pressure, lo ? prHalo : nullptr, hi ? prHalo + plane : nullptr,
                                                  surface ? sp : nullptr, spLo, spHi, valid, matOwn, matLo, matHi, st));
    double div[3] = {0, 0, 0}, maxes[2] = {0, 0};
    if (c.status == MGPS_OK) c.step(mgps_fields_slab_divergence(&desc, div, matOwn, velIn, svel, cw, st));
    if (c.status == MGPS_OK && surface) {
        float m = 0;
        hipStep(c, hipMemcpy(&m, pGammaMax, sizeof(m), hipMemcpyDeviceToHost), "surface pressure");
        maxes[1] = m;
    }
    maxes[0] = div[1];
    double sums[2] = {div[0], div[2]};
    SLAB_COMM(c.agree("write-back", sums, 2, maxes, 2));
#undef SLAB_COMM
    p->divergence_sum = sums[0];
    p->divergence_max = maxes[0];
    p->surface_pressure_max = maxes[1];
    const auto t6 = clock::now();
    p->stage_ms[5] = SlabCall::ms(t5, t6);
    p->stage_ms[6] = c.exchangeMs;
    p->setup_ms = SlabCall::ms(t0, t4);
    p->solve_ms = SlabCall::ms(t4, t5);
    p->total_ms = SlabCall::ms(t0, t6);
    if (setupTimingOn())
        std::printf("projection slab rank %d: passes %.2f ms, agreement (host set-up: labels to hosts) %.2f ms, solver set-up %.2f ms, rhs %.2f ms, solve %.2f ms, write-back %.2f ms "
                    "(plane exchanges %.2f ms)\n",
                    rank, p->stage_ms[0], p->stage_ms[1], p->stage_ms[2], p->stage_ms[3], p->stage_ms[4], p->stage_ms[5], c.exchangeMs);
    return solveRc != MGPS_OK ? c.leave(solveRc, "interrupted") : MGPS_OK;
}
}  // namespace

extern "C" {

int mgps_project_free_surface_slab(mgps_projection_slab *p, const mgps_options *opt, const mgps_comm *comm, const int *splits, void *stream)
try {
    return projectFreeSurfaceSlab("mgps_project_free_surface_slab", p, nullptr, opt, comm, splits, stream);
}
MGPS_API_CATCH(nullptr)

int mgps_project_free_surface_rigid_slab(mgps_projection_rigid_slab *r, const mgps_options *opt, const mgps_comm *comm, const int *splits, void *stream)
try {
    const char *fn = "mgps_project_free_surface_rigid_slab";
    if (!r || r->struct_size != int(sizeof(mgps_projection_rigid_slab))) return refuse(fn, "NULL or struct_size mismatch (mgps_projection_rigid_slab)");
    return projectFreeSurfaceSlab(fn, r->projection, r, opt, comm, splits, stream);
}
MGPS_API_CATCH(nullptr)

}  // extern "C"

// ---- velocity extrapolation into the air band (include/mgps_fields.h) ---------------------------------------
// One launch per layer over the three face grids (blockIdx.y = axis).  A layer touches a thin shell of faces, so the pass is a sweep
// of the `layer` bytes: a thread reads one aligned dword -- 4 faces that follow each other in the flat x-fastest grid, whatever the
// row length -- and a wave none of whose 256 faces is still open (255) leaves at once.  Only an open face looks at its 6 neighbours'
// bytes, and only a known neighbour's velocity is fetched.  In place: a layer reads values of layers < l and writes faces of layer
// 255, so a neighbour byte that another thread turns from 255 to l meanwhile reads as "not known" either way.
namespace {
struct ExAxis {
    float *vel;
    uint8_t *layer;
    const uint8_t *valid;               // read by the l == 0 pass only
    const float *cw;                    // or NULL
    const float *velLo, *velHi;         // the face planes in front of / behind the window, or NULL
    const uint8_t *layLo, *layHi;
    int nx, ny, nz;                     // the face grid of the window
};
struct ExArgs {
    ExAxis a[3];
    int l;
};

// flat face index -> (i, j, k)
__device__ __forceinline__ void exUnflatten(const ExAxis &A, long long n, long long idx, int &i, int &j, int &k)
{
    if (n <= 0xffffffffll) {
        const unsigned u = unsigned(idx), row = u / unsigned(A.nx);
        i = int(u - row * unsigned(A.nx));
        k = int(row / unsigned(A.ny));
        j = int(row - unsigned(k) * unsigned(A.ny));
    } else {
        const long long row = idx / A.nx;
        i = int(idx - row * A.nx);
        k = int(row / A.ny);
        j = int(row - (long long)k * A.ny);
    }
}

// the 4 faces [first, first + 4) of the grid that share the aligned dword at layer + first (first may be < 0 and first + 4 > n when
// the grid does not start or end on a dword: those bytes are fetched one by one and the missing ones read as 0, "not open")
__device__ __forceinline__ unsigned exLoad4(const uint8_t *p, long long first, long long n)
{
    if (first >= 0 && first + 4 <= n) return *reinterpret_cast<const unsigned *>(p + first);
    unsigned w = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (first + q >= 0 && first + q < n) w |= unsigned(p[first + q]) << (8 * q);
    return w;
}
// does a byte of w equal 255?  (exact: ~w has a zero byte)
__device__ __forceinline__ bool exAnyOpen(unsigned w) { return ((~w - 0x01010101u) & w & 0x80808080u) != 0; }

__device__ __forceinline__ void extrapolateAxis(const ExAxis &A, unsigned l)
{
    const long long n = (long long)A.nx * A.ny * A.nz;
    const long long first = 4 * ((long long)blockIdx.x * blockDim.x + threadIdx.x) - (long long)(reinterpret_cast<uintptr_t>(A.layer) & 3u);
    const unsigned w = first < n ? exLoad4(A.layer, first, n) : 0u;
    if (!__any(exAnyOpen(w))) return;  // (wave-uniform: the common case)
    if (exAnyOpen(w)) {
        const long long plane = (long long)A.nx * A.ny;
        const long long base = first < 0 ? 0 : first;
        int i0, j0, k0;
        exUnflatten(A, n, base, i0, j0, k0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (((w >> (8 * q)) & 0xffu) != 255u) continue;
            const long long idx = first + q;
            int i = i0 + int(idx - base), j = j0, k = k0;
            while (i >= A.nx) {
                i -= A.nx;
                if (++j == A.ny) j = 0, ++k;
            }
            float sum = 0.f;
            int known = 0;
            // -x, +x: inside the dword where they are
            if (i > 0 && (q > 0 ? (w >> (8 * (q - 1))) & 0xffu : unsigned(A.layer[idx - 1])) < l) sum += A.vel[idx - 1], ++known;
            if (i + 1 < A.nx && (q < 3 ? (w >> (8 * (q + 1))) & 0xffu : unsigned(A.layer[idx + 1])) < l) sum += A.vel[idx + 1], ++known;
            if (j > 0 && A.layer[idx - A.nx] < l) sum += A.vel[idx - A.nx], ++known;
            if (j + 1 < A.ny && A.layer[idx + A.nx] < l) sum += A.vel[idx + A.nx], ++known;
            const long long ij = (long long)j * A.nx + i;
            if (k > 0) {
                if (A.layer[idx - plane] < l) sum += A.vel[idx - plane], ++known;
            } else if (A.layLo) {
                if (A.layLo[ij] < l) sum += A.velLo[ij], ++known;
            }
            if (k + 1 < A.nz) {
                if (A.layer[idx + plane] < l) sum += A.vel[idx + plane], ++known;
            } else if (A.layHi) {
                if (A.layHi[ij] < l) sum += A.velHi[ij], ++known;
            }
            if (known == 0 || (A.cw && !(A.cw[idx] > 0.f))) continue;
            A.vel[idx] = sum / float(known);
            A.layer[idx] = uint8_t(l);
        }
    }
}

// layer l of up to three face grids; blocks past the end of a shorter grid leave at once
__global__ __launch_bounds__(256) void extrapolateLayerKernel(ExArgs p)
{
    // (constant indices: a dynamically indexed by-value argument would be copied to scratch)
    if (blockIdx.y == 0) extrapolateAxis(p.a[0], unsigned(p.l));
    else if (blockIdx.y == 1) extrapolateAxis(p.a[1], unsigned(p.l));
    else extrapolateAxis(p.a[2], unsigned(p.l));
}

// filled[axis] += the faces [0, n[axis]) whose layer lies in [lo, hi].  A pass of its own over the layer bytes, behind the layers:
// counting where the faces are filled costs one atomic per wave of the shell on three addresses, which took longer than the layer
// itself.  Here a block sums its share in registers and LDS and adds once: kCountBlocks adds per axis
constexpr int kCountBlocks = 1024;
struct ExCount {
    const uint8_t *layer[3];
    long long n[3];
    unsigned lo, hi;
    unsigned long long *filled;
};
__global__ __launch_bounds__(256) void extrapolateCountKernel(ExCount p)
{
    const int axis = int(blockIdx.y);
    const uint8_t *layer = axis == 0 ? p.layer[0] : axis == 1 ? p.layer[1] : p.layer[2];
    const long long n = axis == 0 ? p.n[0] : axis == 1 ? p.n[1] : p.n[2];
    const long long mis = (long long)(reinterpret_cast<uintptr_t>(layer) & 3u);
    unsigned mine = 0;  // (at most 4 faces per step of 2^20 faces: no overflow below 2^50 faces)
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; 4 * c - mis < n; c += (long long)gridDim.x * blockDim.x) {
        const unsigned w = exLoad4(layer, 4 * c - mis, n);  // (a missing byte reads 0: lo >= 1)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned b = (w >> (8 * q)) & 0xffu;
            mine += b >= p.lo && b <= p.hi;
        }
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    __shared__ unsigned part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = part[0] + part[1] + part[2] + part[3];
        if (total) atomicAdd(p.filled + axis, (unsigned long long)total);
    }
}

// layer = valid ? 0 : 255, 4 faces per thread (dword-wide where both grids allow it)
__device__ __forceinline__ void extrapolateInitAxis(const ExAxis &A)
{
    const long long n = (long long)A.nx * A.ny * A.nz;
    const long long first = 4 * ((long long)blockIdx.x * blockDim.x + threadIdx.x) - (long long)(reinterpret_cast<uintptr_t>(A.layer) & 3u);
    if (first >= n) return;
    if (first >= 0 && first + 4 <= n && ((reinterpret_cast<uintptr_t>(A.valid) ^ reinterpret_cast<uintptr_t>(A.layer)) & 3u) == 0) {
        const unsigned v = *reinterpret_cast<const unsigned *>(A.valid + first);
        unsigned out = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) out |= (((v >> (8 * q)) & 0xffu) == 1u ? 0u : 255u) << (8 * q);
        *reinterpret_cast<unsigned *>(A.layer + first) = out;
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (first + q >= 0 && first + q < n) A.layer[first + q] = A.valid[first + q] == 1 ? 0 : 255;
}
__global__ __launch_bounds__(256) void extrapolateInitKernel(ExArgs p)
{
    if (blockIdx.y == 0) extrapolateInitAxis(p.a[0]);
    else if (blockIdx.y == 1) extrapolateInitAxis(p.a[1]);
    else extrapolateInitAxis(p.a[2]);
}

// the planes a slab rank sends to its neighbours before a layer, packed: [x-face | y-face | z-face velocity planes (float) | the same
// three layer planes (uint8)].  To the rank below: plane 0 of every window (of the z-faces plane 1: plane 0 is the cut's, the
// neighbour has its own copy); to the rank above: the last plane (of the z-faces the last but one)
struct ExPack {
    const float *vel[3];
    const uint8_t *lay[3];
    int count[3];  // entries of one plane per axis
    long long lo[3], hi[3];  // first entry of the plane sent down / up (-1: no neighbour)
    float *outLo, *outHi;
};
__global__ __launch_bounds__(256) void extrapolatePackKernel(ExPack p)
{
    const int total = p.count[0] + p.count[1] + p.count[2];
    int t = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= total) return;
    const int slot = t;
    const int a = t < p.count[0] ? 0 : t < p.count[0] + p.count[1] ? 1 : 2;
    t -= a == 0 ? 0 : a == 1 ? p.count[0] : p.count[0] + p.count[1];
    const float *vel = a == 0 ? p.vel[0] : a == 1 ? p.vel[1] : p.vel[2];
    const uint8_t *lay = a == 0 ? p.lay[0] : a == 1 ? p.lay[1] : p.lay[2];
    const long long lo = a == 0 ? p.lo[0] : a == 1 ? p.lo[1] : p.lo[2], hi = a == 0 ? p.hi[0] : a == 1 ? p.hi[1] : p.hi[2];
    if (lo >= 0) {
        p.outLo[slot] = vel[lo + t];
        reinterpret_cast<uint8_t *>(p.outLo + total)[slot] = lay[lo + t];
    }
    if (hi >= 0) {
        p.outHi[slot] = vel[hi + t];
        reinterpret_cast<uint8_t *>(p.outHi + total)[slot] = lay[hi + t];
    }
}

// the checks every extrapolation entry shares, on the host, before any HIP call
int exCheckLayers(const char *fn, int layers)
{
    if (layers < 1 || layers > 254) return refuse(fn, "layers = " + std::to_string(layers) + " is outside 1 .. 254 (layer is a uint8 grid, 255 = not reached)");
    return MGPS_OK;
}
int exCheckExtents(const char *fn, int gx, int gy, int gz)
{
    if (!okBox(gx, gy, gz)) return refuse(fn, "non-positive extent (gx, gy, gz = " + std::to_string(gx) + ", " + std::to_string(gy) + ", " + std::to_string(gz) + ")");
    return MGPS_OK;
}
// cut_weights: NULL, or all three
int exCheckCutWeights(const char *fn, const float *const cw[3])
{
    if (cw && !(cw[0] && cw[1] && cw[2]) && (cw[0] || cw[1] || cw[2])) return refuse(fn, "cut_weights: all three grids, or none");
    return MGPS_OK;
}
inline dim3 exGrid(const ExArgs &p, int naxes)
{
    long long n = 0;
    for (int a = 0; a < naxes; ++a) n = std::max(n, (long long)p.a[a].nx * p.a[a].ny * p.a[a].nz);
    return dim3(unsigned((n + 3 + 4 * 256 - 1) / (4 * 256)), unsigned(naxes));  // (+3: a grid that starts inside a dword)
}
int exLaunchLayer(const ExArgs &p, int naxes, hipStream_t st, const char *fn)
{
    if (p.l == 0) extrapolateInitKernel<<<exGrid(p, naxes), 256, 0, st>>>(p);
    else extrapolateLayerKernel<<<exGrid(p, naxes), 256, 0, st>>>(p);
    return done(fn);
}
// filled[a] += the faces of the planes [0, countNz[a]) of the three grids of p whose layer lies in [lo, hi]
int exLaunchCount(const ExArgs &p, const int countNz[3], unsigned lo, unsigned hi, unsigned long long *filled, hipStream_t st, const char *fn)
{
    ExCount c{};
    long long most = 0;
    for (int a = 0; a < 3; ++a) {
        c.layer[a] = p.a[a].layer;
        c.n[a] = (long long)p.a[a].nx * p.a[a].ny * countNz[a];
        most = std::max(most, c.n[a]);
    }
    c.lo = lo;
    c.hi = hi;
    c.filled = filled;
    const long long want = (most + 3 + 4 * 256 - 1) / (4 * 256);
    extrapolateCountKernel<<<dim3(unsigned(std::min<long long>(std::max<long long>(want, 1), kCountBlocks)), 3), 256, 0, st>>>(c);
    return done(fn);
}
}  // namespace

extern "C" {

int mgps_fields_extrapolate(int axis, float *velocity, uint8_t *layer, const uint8_t *valid, const float *cut_weights, int layers, int gx,
                            int gy, int gz, void *stream)
try {
    const char *fn = "mgps_fields_extrapolate";
    if (axis < 0 || axis > 2) return refuse(fn, "axis = " + std::to_string(axis) + " is outside 0 .. 2");
    if (int rc = exCheckLayers(fn, layers); rc != MGPS_OK) return rc;
    if (int rc = exCheckExtents(fn, gx, gy, gz); rc != MGPS_OK) return rc;
    if (!velocity) return refuse(fn, "velocity is NULL");
    if (!layer) return refuse(fn, "layer is NULL");
    if (!valid) return refuse(fn, "valid is NULL");
    ExArgs p{};
    p.a[0] = ExAxis{velocity, layer, valid, cut_weights, nullptr, nullptr, nullptr, nullptr, gx + (axis == 0), gy + (axis == 1), gz + (axis == 2)};
    for (p.l = 0; p.l <= layers; ++p.l)
        if (int rc = exLaunchLayer(p, 1, static_cast<hipStream_t>(stream), fn); rc != MGPS_OK) return rc;
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

int mgps_fields_extrapolate3(float *const velocity[3], uint8_t *const layer[3], const uint8_t *const valid[3], const float *const cut_weights[3],
                             int layers, int gx, int gy, int gz, unsigned long long *filled_dev, void *stream)
try {
    const char *fn = "mgps_fields_extrapolate3";
    if (int rc = exCheckLayers(fn, layers); rc != MGPS_OK) return rc;
    if (int rc = exCheckExtents(fn, gx, gy, gz); rc != MGPS_OK) return rc;
    if (!velocity || !velocity[0] || !velocity[1] || !velocity[2]) return refuse(fn, "velocity: three grids are required");
    if (!layer || !layer[0] || !layer[1] || !layer[2]) return refuse(fn, "layer: three grids are required");
    if (!valid || !valid[0] || !valid[1] || !valid[2]) return refuse(fn, "valid: three grids are required");
    if (int rc = exCheckCutWeights(fn, cut_weights); rc != MGPS_OK) return rc;
    const bool closed = cut_weights && cut_weights[0];
    ExArgs p{};
    for (int a = 0; a < 3; ++a)
        p.a[a] = ExAxis{velocity[a], layer[a], valid[a], closed ? cut_weights[a] : nullptr, nullptr, nullptr, nullptr, nullptr, gx + (a == 0), gy + (a == 1),
                        gz + (a == 2)};
    for (p.l = 0; p.l <= layers; ++p.l)
        if (int rc = exLaunchLayer(p, 3, static_cast<hipStream_t>(stream), fn); rc != MGPS_OK) return rc;
    if (!filled_dev) return MGPS_OK;
    const int countNz[3] = {gz, gz, gz + 1};
    return exLaunchCount(p, countNz, 1, 254, filled_dev, static_cast<hipStream_t>(stream), fn);
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_extrapolate_layer(const mgps_fields_slab *d, int l, float *const velocity[3], uint8_t *const layer[3],
                                       const uint8_t *const valid[3], const float *const velocity_lo[3], const float *const velocity_hi[3],
                                       const uint8_t *const layer_lo[3], const uint8_t *const layer_hi[3], const float *const cut_weights[3],
                                       unsigned long long *filled_dev, void *stream)
try {
    const char *fn = "mgps_fields_slab_extrapolate_layer";
    Slab s;
    if (!readSlab(d, s, fn)) return MGPS_ERR_INVALID_ARGUMENT;
    if (l < 0 || l > 254) return refuse(fn, "l = " + std::to_string(l) + " is outside 0 .. 254 (0 initialises layer from valid)");
    if (!velocity || !velocity[0] || !velocity[1] || !velocity[2]) return refuse(fn, "velocity: three grids are required");
    if (!layer || !layer[0] || !layer[1] || !layer[2]) return refuse(fn, "layer: three grids are required");
    if (l == 0 && (!valid || !valid[0] || !valid[1] || !valid[2])) return refuse(fn, "valid: three grids are required with l = 0");
    if (int rc = exCheckCutWeights(fn, cut_weights); rc != MGPS_OK) return rc;
    const bool lo = l > 0 && s.c0 > 0, hi = l > 0 && s.c1 < s.gz;
    for (int a = 0; a < 3; ++a) {
        if (lo && !(velocity_lo && layer_lo && velocity_lo[a] && layer_lo[a])) return refuse(fn, "velocity_lo / layer_lo: the planes below the window are required (c0 > 0)");
        if (hi && !(velocity_hi && layer_hi && velocity_hi[a] && layer_hi[a])) return refuse(fn, "velocity_hi / layer_hi: the planes above the window are required (c1 < gz)");
    }
    const bool closed = cut_weights && cut_weights[0];
    const int nzl = s.c1 - s.c0;
    ExArgs p{};
    for (int a = 0; a < 3; ++a)
        p.a[a] = ExAxis{velocity[a], layer[a], l == 0 ? valid[a] : nullptr, closed ? cut_weights[a] : nullptr, lo ? velocity_lo[a] : nullptr,
                        hi ? velocity_hi[a] : nullptr, lo ? layer_lo[a] : nullptr, hi ? layer_hi[a] : nullptr, s.gx + (a == 0), s.gy + (a == 1), nzl + (a == 2)};
    p.l = l;
    if (int rc = exLaunchLayer(p, 3, static_cast<hipStream_t>(stream), fn); rc != MGPS_OK || !filled_dev || l == 0) return rc;
    const int countNz[3] = {nzl, nzl, s.c1 < s.gz ? nzl : nzl + 1};  // (the cut's z-face plane is counted by the rank above it)
    return exLaunchCount(p, countNz, unsigned(l), unsigned(l), filled_dev, static_cast<hipStream_t>(stream), fn);
}
MGPS_API_CATCH(nullptr)

int mgps_extrapolate_velocity_slab(mgps_extrapolation_slab *e, const mgps_comm *comm, const int *splits, void *stream)
try {
    SlabCall c;
    const char *fn = "mgps_extrapolate_velocity_slab";
    // ---- what every rank shares: a refusal here is every rank's, before any collective and any HIP call
    if (!e || e->struct_size != int(sizeof(mgps_extrapolation_slab))) return refuse(fn, "NULL or struct_size mismatch (mgps_extrapolation_slab)");
    if (int rc = c.open(fn, comm, splits, offsetof(mgps_comm, gather)); rc != MGPS_OK) return rc;
    if (int rc = exCheckLayers(fn, e->layers); rc != MGPS_OK) return rc;
    if (int rc = exCheckExtents(fn, e->gx, e->gy, e->gz); rc != MGPS_OK) return rc;
    const int P = c.P, rank = c.rank, L = e->layers;
    mgps_fields_slab desc;
    if (int rc = mgps_fields_slab_describe(&desc, e->gx, e->gy, e->gz, e->power_of_two, splits, P, rank); rc != MGPS_OK) return rc;
    Slab s;
    if (!readSlab(&desc, s, fn)) return MGPS_ERR_INVALID_ARGUMENT;
    e->filled[0] = e->filled[1] = e->filled[2] = 0;
    e->total_ms = e->exchange_ms = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int gx = s.gx, gy = s.gy, nzl = s.c1 - s.c0;
    const bool lo = s.c0 > 0, hi = s.c1 < s.gz;
    const int count[3] = {(gx + 1) * gy, gx * (gy + 1), gx * gy};
    const size_t entries = size_t(count[0]) + size_t(count[1]) + size_t(count[2]), message = entries * (sizeof(float) + 1);
    // ---- this rank's own arguments and buffers: a failure is carried by the all-reduce in front of the first exchange
    std::unique_ptr<DevPool> pool;  // (made after the argument checks: a refusal makes no HIP call)
    uint8_t *layer[3] = {nullptr, nullptr, nullptr};
    float *sendLo = nullptr, *sendHi = nullptr, *recvLo = nullptr, *recvHi = nullptr;
    unsigned long long *filled = nullptr;
    c.step([&]() -> int {
        for (int a = 0; a < 3; ++a) {
            if (!e->velocity[a]) return refuse(fn, "velocity: three grids are required");
            if (!e->valid_faces[a]) return refuse(fn, "valid_faces: three grids are required");
        }
        if (int rc = exCheckCutWeights(fn, e->cut_weights); rc != MGPS_OK) return rc;
        if (int rc = selectDevice(-1); rc != MGPS_OK) return rc;
        try {
            pool.reset(new DevPool);
            for (int a = 0; a < 3; ++a) layer[a] = e->layer[a] ? e->layer[a] : pool->get<uint8_t>(faceCount(gx, gy, nzl, a));
            // (a message is floats first: every block of the cache is aligned for them)
            if (lo) sendLo = pool->get<float>((message + 3) / 4), recvLo = pool->get<float>((message + 3) / 4);
            if (hi) sendHi = pool->get<float>((message + 3) / 4), recvHi = pool->get<float>((message + 3) / 4);
            filled = pool->get<unsigned long long>(3);
        } catch (const std::bad_alloc &) {
            return c.fail(MGPS_ERR_ALLOC, "device allocation failed");
        }
        hipStep(c, hipMemsetAsync(filled, 0, 3 * sizeof(unsigned long long), st), "clearing the counts");
        return c.status;
    }());
    if (int rc = c.agree("arguments"); rc != MGPS_OK) return rc;
    // (from here on the buffers exist on every rank: a failing rank still takes part in every exchange and the last agreement
    //  carries its status)
    const float *cw[3] = {e->cut_weights[0], e->cut_weights[1], e->cut_weights[2]};
    const float *velLo[3], *velHi[3];
    const uint8_t *layLo[3], *layHi[3];
    ExPack pack{};
    {
        size_t at = 0;
        for (int a = 0; a < 3; ++a) {
            velLo[a] = lo ? recvLo + at : nullptr;
            velHi[a] = hi ? recvHi + at : nullptr;
            layLo[a] = lo ? reinterpret_cast<const uint8_t *>(recvLo + entries) + at : nullptr;
            layHi[a] = hi ? reinterpret_cast<const uint8_t *>(recvHi + entries) + at : nullptr;
            at += size_t(count[a]);
            pack.vel[a] = e->velocity[a];
            pack.lay[a] = layer[a];
            pack.count[a] = count[a];
            // the z-face window holds the faces c0 .. c1: the neighbours have the end planes themselves
            pack.lo[a] = lo ? (long long)(a == 2 ? 1 : 0) * count[a] : -1;
            pack.hi[a] = hi ? (long long)(a == 2 ? nzl - 1 : nzl - 1) * count[a] : -1;
        }
        pack.outLo = sendLo;
        pack.outHi = sendHi;
    }
    c.step(mgps_fields_slab_extrapolate_layer(&desc, 0, e->velocity, layer, e->valid_faces, nullptr, nullptr, nullptr, nullptr, cw[0] ? cw : nullptr, nullptr, st));
    for (int l = 1; l <= L; ++l) {
        if (P > 1) {
            extrapolatePackKernel<<<blocks(entries), 256, 0, st>>>(pack);
            c.step(done(fn));
            if (int rc = c.trade(sendLo, lo ? message : 0, recvLo, lo ? message : 0, sendHi, hi ? message : 0, recvHi, hi ? message : 0, st, "layer " + std::to_string(l));
                rc != MGPS_OK)
                return rc;
        }
        if (c.status == MGPS_OK)
            c.step(mgps_fields_slab_extrapolate_layer(&desc, l, e->velocity, layer, nullptr, velLo, velHi, layLo, layHi, cw[0] ? cw : nullptr, nullptr, st));
    }
    if (c.status == MGPS_OK) {  // the faces filled, counted once behind the layers (the cut's z-face plane by the rank above it)
        ExArgs grids{};
        for (int a = 0; a < 3; ++a) grids.a[a] = ExAxis{nullptr, layer[a], nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, gx + (a == 0), gy + (a == 1), nzl + (a == 2)};
        const int countNz[3] = {nzl, nzl, hi ? nzl : nzl + 1};
        c.step(exLaunchCount(grids, countNz, 1, 254, filled, st, fn));
    }
    unsigned long long mine[3] = {0, 0, 0};
    if (c.status == MGPS_OK) hipStep(c, hipMemcpyAsync(mine, filled, sizeof(mine), hipMemcpyDeviceToHost, st), "the counts to the host");
    if (c.status == MGPS_OK) hipStep(c, hipStreamSynchronize(st), "the counts to the host");
    double sums[3] = {double(mine[0]), double(mine[1]), double(mine[2])};
    const int rc = c.agree("layers", sums, 3);
    for (int a = 0; a < 3; ++a) e->filled[a] = (unsigned long long)(sums[a]);
    e->exchange_ms = c.exchangeMs;
    e->total_ms = SlabCall::ms(c.t0, SlabCall::Clock::now());
    return rc;
}
MGPS_API_CATCH(nullptr)

}  // extern "C"

// ---- pressure feedback: force and torque of the pressure on solid bodies (include/mgps_fields.h) ------------
// One launch over the cells of the grid (or of a window): a thread handles the three backward faces of its cell and, at the far end
// of an axis, the end face.  Almost every face is open: the cut weight is loaded first and body, material and pressure only where
// w < 1, so far from solids the pass streams the three weight grids (12 bytes per cell).  Contributions are summed per row (body) in
// fp64 without atomics: lanes of a wave that hold the same row are reduced by shuffles, lane 0 adds the sum into the wave's own
// table in LDS, the waves' tables are added in wave order into one table per workgroup, and a second kernel adds the workgroups'
// tables in index order.  The launch is a fixed number of workgroups walking the cells with a fixed stride: every sum has one order.
namespace {
constexpr int kForceBlocks = 1024, kForceThreads = 256, kForceWaves = kForceThreads / 64, kForceCols = 8;
constexpr int kForceSlices = 16;  // the second kernel: 16 threads share the workgroups of one table entry
static_assert(kForceBlocks % kForceSlices == 0, "the slices divide the workgroups evenly");

// The rule of one face: the face of `axis` behind cell (i, j, k) of G (its forward cell; k a plane of the whole grid) with cut weight
// w.  False unless the face is wet; then, and only then, s is set to its closed fraction, phi to the push along +axis and row to the
// table row.  mat / pr reach
// material and pressure of a cell of G, bodyOf() loads the face's body id; all three are touched on a closed or cut face only.
template <class MatAt, class PrAt, class BodyOf>
__device__ __forceinline__ bool solidFaceTerm(const Box &G, int axis, int i, int j, int k, float w, int bodies, MatAt mat, PrAt pr,
                                              BodyOf bodyOf, int &row, float &s, double &phi)
{
    if (!(w < 1.f)) return false;
    const int ext[3] = {G.gx, G.gy, G.gz};
    int b[3] = {i, j, k}, f[3] = {i, j, k};
    b[axis] -= 1;
    const bool lb = b[axis] >= 0 && mat(b[0], b[1], b[2]) == kLiquid, lf = f[axis] < ext[axis] && mat(i, j, k) == kLiquid;
    if (!(lb || lf)) return false;
    const float pb = lb ? pr(b[0], b[1], b[2]) : 0.f, pf = lf ? pr(i, j, k) : 0.f;
    s = 1.f - w;  // (w < 1: s > 0)
    phi = double(s) * (double(pb) - double(pf));
    const int id = bodyOf();
    row = id >= 1 && id <= bodies ? id : 0;
    return true;
}

__device__ __forceinline__ double waveSum(double v)  // every lane gets the sum, in one fixed order
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Adds the wave's terms of one face slot of axis A into the wave's table: while terms are pending, the row of the first pending lane
// is taken, the lanes of that row are reduced and lane 0 adds once.  (x, y, z): the face centre.  Every lane of the wave calls it.
template <int A>
__device__ __forceinline__ void addFaceTerms(double *table, const double *__restrict__ centres, bool has, int row, float s, double phi,
                                             double x, double y, double z)
{
    unsigned long long todo = __ballot(has);
    if (!todo) return;
    constexpr int U = (A + 1) % 3, V = (A + 2) % 3;
    double tu = 0.0, tv = 0.0;  // (d x phi e_A)_U = d_V phi, (d x phi e_A)_V = -d_U phi, d = the arm from the row's centre
    if (has) {
        const double pos[3] = {x, y, z};
        tu = (pos[V] - centres[3 * row + V]) * phi;
        tv = -(pos[U] - centres[3 * row + U]) * phi;
    }
    while (todo) {
        const int r0 = __builtin_amdgcn_readlane(row, __ffsll(todo) - 1);
        const bool mine = has && row == r0;
        const unsigned long long m = __ballot(mine);
        const double f = waveSum(mine ? phi : 0.0), su = waveSum(mine ? tu : 0.0), sv = waveSum(mine ? tv : 0.0),
                     area = waveSum(mine ? double(s) : 0.0);
        if ((threadIdx.x & 63) == 0) {
            double *t = table + size_t(r0) * kForceCols;
            t[A] += f;
            t[3 + U] += su;
            t[3 + V] += sv;
            t[6] += area;
            t[7] += double(__popcll(m));
        }
        todo &= ~m;
    }
}

struct ForceArgs {
    Box G;                 // the whole grid
    Box g;                 // the box the face grids are indexed in: G, or the window's planes
    int k0;                // the whole grid's plane of the box's plane 0
    int topCounts;         // the z end face of the box's last plane counts (the whole grid's plane gz)
    int bodies;
    int di, dj, dk;        // the stride of the walk, kForceBlocks * kForceThreads cells, as steps of (i, j, k)
    const float *cw[3];
    const int32_t *body[3];
    const double *centres; // device, (bodies + 1) * 3
    double *partials;      // device, kForceBlocks tables of (bodies + 1) * 8
};

// the walk and the sums; mat / pr: GridAt of the whole grid, or SlabAt of the window with its lower halo
template <class MatAt, class PrAt>
__device__ __forceinline__ void solidForcesWalk(const ForceArgs &p, MatAt mat, PrAt pr, double *lds)
{
    const int entries = (p.bodies + 1) * kForceCols;
    for (int e = int(threadIdx.x); e < kForceWaves * entries; e += kForceThreads) lds[e] = 0.0;
    __syncthreads();
    double *table = lds + size_t(threadIdx.x >> 6) * entries;
    const Box g = p.g;
    const size_t n = g.cells(), plane = size_t(g.gx) * g.gy, stride = size_t(kForceBlocks) * kForceThreads;
    size_t base = size_t(blockIdx.x) * kForceThreads, t = base + threadIdx.x;
    int i = int(t % g.gx), j = int((t / g.gx) % g.gy), k = int(min(t / plane, size_t(g.gz)));  // (past the end: k = gz and stays there)
    bool active = t < n;
    // the cut weights of the cell's backward faces: x-face c + (k gy + j), y-face c + k gx, z-face c (c = the cell's index)
    auto loadW = [&](float w[3]) {
        w[0] = w[1] = w[2] = 1.f;
        if (active) {
            w[0] = p.cw[0][t + size_t(k) * g.gy + j];
            w[1] = p.cw[1][t + size_t(k) * g.gx];
            w[2] = p.cw[2][t];
        }
    };
    float w[3];
    loadW(w);
    for (; base < n; base += stride) {  // (a wave-uniform bound: every lane stays for the ballots and shuffles)
        const size_t tc = t;
        const int ci = i, cj = j, ck = k;
        const bool cur = active;
        const float wc[3] = {w[0], w[1], w[2]};
        // the next cell of the walk, and its weights on their way while this one is worked on
        t += stride;
        i += p.di;
        if (i >= g.gx) i -= g.gx, ++j;
        j += p.dj;
        if (j >= g.gy) j -= g.gy, ++k;
        k = min(k + p.dk, g.gz);
        active = t < n;
        loadW(w);
        const int kg = p.k0 + ck;
        const size_t fx = tc + size_t(ck) * g.gy + cj, fy = tc + size_t(ck) * g.gx, fz = tc;
        int row = 0;
        float s = 0.f;
        double phi = 0.0;
        bool has;
        has = cur && solidFaceTerm(p.G, 0, ci, cj, kg, wc[0], p.bodies, mat, pr, [&] { return p.body[0][fx]; }, row, s, phi);
        addFaceTerms<0>(table, p.centres, has, row, s, phi, double(ci), cj + 0.5, kg + 0.5);
        has = cur && solidFaceTerm(p.G, 1, ci, cj, kg, wc[1], p.bodies, mat, pr, [&] { return p.body[1][fy]; }, row, s, phi);
        addFaceTerms<1>(table, p.centres, has, row, s, phi, ci + 0.5, double(cj), kg + 0.5);
        has = cur && solidFaceTerm(p.G, 2, ci, cj, kg, wc[2], p.bodies, mat, pr, [&] { return p.body[2][fz]; }, row, s, phi);
        addFaceTerms<2>(table, p.centres, has, row, s, phi, ci + 0.5, cj + 0.5, double(kg));
        // the end faces: in front of the last cell of an axis
        const bool endX = cur && ci == g.gx - 1, endY = cur && cj == g.gy - 1, endZ = cur && ck == g.gz - 1 && p.topCounts;
        if (__ballot(endX)) {
            has = endX && solidFaceTerm(p.G, 0, ci + 1, cj, kg, endX ? p.cw[0][fx + 1] : 1.f, p.bodies, mat, pr, [&] { return p.body[0][fx + 1]; }, row, s, phi);
            addFaceTerms<0>(table, p.centres, has, row, s, phi, double(ci + 1), cj + 0.5, kg + 0.5);
        }
        if (__ballot(endY)) {
            has = endY && solidFaceTerm(p.G, 1, ci, cj + 1, kg, endY ? p.cw[1][fy + g.gx] : 1.f, p.bodies, mat, pr, [&] { return p.body[1][fy + g.gx]; }, row, s, phi);
            addFaceTerms<1>(table, p.centres, has, row, s, phi, ci + 0.5, double(cj + 1), kg + 0.5);
        }
        if (__ballot(endZ)) {
            has = endZ && solidFaceTerm(p.G, 2, ci, cj, kg + 1, endZ ? p.cw[2][fz + plane] : 1.f, p.bodies, mat, pr, [&] { return p.body[2][fz + plane]; }, row, s, phi);
            addFaceTerms<2>(table, p.centres, has, row, s, phi, ci + 0.5, cj + 0.5, double(kg + 1));
        }
    }
    __syncthreads();
    double *out = p.partials + size_t(blockIdx.x) * entries;
    for (int e = int(threadIdx.x); e < entries; e += kForceThreads) {
        double sum = lds[e];
#pragma unroll
        for (int wv = 1; wv < kForceWaves; ++wv) sum += lds[size_t(wv) * entries + e];  // wave order
        out[e] = sum;
    }
}

__global__ __launch_bounds__(kForceThreads) void solidForcesKernel(ForceArgs p, const int32_t *__restrict__ material,
                                                                   const float *__restrict__ pressure)
{
    extern __shared__ double forceTables[];
    solidForcesWalk(p, GridAt<int32_t>{p.G, material}, GridAt<float>{p.G, pressure}, forceTables);
}
__global__ __launch_bounds__(kForceThreads) void solidForcesSlabKernel(ForceArgs p, Slab s, Planes<int32_t> mat, Planes<float> pr)
{
    extern __shared__ double forceTables[];
    solidForcesWalk(p, SlabAt<int32_t>{s, mat}, SlabAt<float>{s, pr}, forceTables);
}

// out[e] = the workgroups' tables added in index order, force and torque columns times scale.  16 entries x 16 slices per block: a
// slice adds its 64 workgroups in order, thread 0 of the entry adds the slices in order.
__global__ __launch_bounds__(kForceSlices * 16) void solidForcesSumKernel(double *__restrict__ out, const double *__restrict__ partials,
                                                                          int entries, double scale)
{
    __shared__ double part[kForceSlices][16];
    const int lane = int(threadIdx.x) & 15, slice = int(threadIdx.x) >> 4, e = int(blockIdx.x) * 16 + lane;
    constexpr int per = kForceBlocks / kForceSlices;
    double sum = 0.0;
    if (e < entries)
        for (int b = slice * per; b < (slice + 1) * per; ++b) sum += partials[size_t(b) * entries + e];
    part[slice][lane] = sum;
    __syncthreads();
    if (slice == 0 && e < entries) {
        double total = part[0][lane];
        for (int q = 1; q < kForceSlices; ++q) total += part[q][lane];
        out[e] = e % kForceCols < 6 ? scale * total : total;
    }
}

int forceCheckBodies(const char *fn, int bodies)
{
    if (bodies < 1 || bodies > 255) return refuse(fn, "bodies = " + std::to_string(bodies) + " is outside 1 .. 255");
    return MGPS_OK;
}

// The launches of one call and the rows' way to the host.  `slab`: the window and its lower halo, or NULL for the whole grid G.
// Synchronises the stream.
int runSolidForces(const char *fn, double *outHost, const Box &G, const Slab *slab, const float *pressure, const float *pressureLo,
                   const int32_t *material, const int32_t *materialLo, const float *const cw[3], const int32_t *const body[3],
                   const double *centresHost, int bodies, double scale, hipStream_t st)
{
    ForceArgs p{};
    p.G = G;
    p.g = slab ? slab->base() : G;
    p.k0 = slab ? slab->c0 : 0;
    p.topCounts = slab ? slab->c1 == slab->gz : 1;
    p.bodies = bodies;
    {
        const size_t stride = size_t(kForceBlocks) * kForceThreads, plane = size_t(p.g.gx) * p.g.gy;
        p.di = int(stride % size_t(p.g.gx));
        p.dj = int((stride / size_t(p.g.gx)) % size_t(p.g.gy));
        p.dk = int(std::min<size_t>(stride / plane, size_t(p.g.gz)));
    }
    const size_t entries = size_t(bodies + 1) * kForceCols, centreCount = size_t(bodies + 1) * 3;
    DevPool pool;
    double *dev = nullptr;  // [partials | rows | centres]
    try {
        dev = pool.get<double>(size_t(kForceBlocks) * entries + entries + centreCount);
    } catch (const std::bad_alloc &) {
        setLastGlobalError(std::string(fn) + ": device allocation failed");
        return MGPS_ERR_ALLOC;
    }
    double *rows = dev + size_t(kForceBlocks) * entries, *centres = rows + entries;
    for (int a = 0; a < 3; ++a) p.cw[a] = cw[a], p.body[a] = body[a];
    p.centres = centres;
    p.partials = dev;
    hipError_t e = hipMemcpyAsync(centres, centresHost, centreCount * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const size_t lds = size_t(kForceWaves) * entries * sizeof(double);  // 64 KiB at 255 bodies
        if (slab)
            solidForcesSlabKernel<<<kForceBlocks, kForceThreads, lds, st>>>(p, *slab, Planes<int32_t>{material, materialLo, nullptr},
                                                                            Planes<float>{pressure, pressureLo, nullptr});
        else solidForcesKernel<<<kForceBlocks, kForceThreads, lds, st>>>(p, material, pressure);
        solidForcesSumKernel<<<unsigned((entries + 15) / 16), kForceSlices * 16, 0, st>>>(rows, dev, int(entries), scale);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(outHost, rows, entries * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        setLastGlobalError(std::string(fn) + ": " + hipGetErrorString(e));
        return MGPS_ERR_HIP;
    }
    return MGPS_OK;
}
}  // namespace

extern "C" {

int mgps_fields_solid_forces(double *out_host, const float *pressure, const int32_t *material, const float *cwx, const float *cwy,
                             const float *cwz, const int32_t *bx, const int32_t *by, const int32_t *bz, const double *centres_host,
                             int bodies, double scale, int gx, int gy, int gz, void *stream)
try {
    const char *fn = "mgps_fields_solid_forces";
    if (int rc = forceCheckBodies(fn, bodies); rc != MGPS_OK) return rc;
    if (int rc = exCheckExtents(fn, gx, gy, gz); rc != MGPS_OK) return rc;
    if (!out_host) return refuse(fn, "out_host is NULL");
    if (!pressure) return refuse(fn, "pressure is NULL");
    if (!material) return refuse(fn, "material is NULL");
    if (!cwx || !cwy || !cwz) return refuse(fn, "cut weights: three grids are required");
    if (!bx || !by || !bz) return refuse(fn, "body: three grids are required");
    if (!centres_host) return refuse(fn, "centres_host is NULL");
    const float *cw[3] = {cwx, cwy, cwz};
    const int32_t *body[3] = {bx, by, bz};
    return runSolidForces(fn, out_host, Box{gx, gy, gz}, nullptr, pressure, nullptr, material, nullptr, cw, body, centres_host, bodies, scale,
                          static_cast<hipStream_t>(stream));
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_solid_forces(const mgps_fields_slab *d, double *out_host, const float *pressure, const float *pressure_lo,
                                  const int32_t *material, const int32_t *material_lo, const float *const cut_weights[3],
                                  const int32_t *const body[3], const double *centres_host, int bodies, double scale, void *stream)
try {
    const char *fn = "mgps_fields_slab_solid_forces";
    Slab s;
    if (!readSlab(d, s, fn)) return MGPS_ERR_INVALID_ARGUMENT;
    if (int rc = forceCheckBodies(fn, bodies); rc != MGPS_OK) return rc;
    if (!out_host) return refuse(fn, "out_host is NULL");
    if (!pressure) return refuse(fn, "pressure is NULL");
    if (!material) return refuse(fn, "material is NULL");
    if (!cut_weights || !cut_weights[0] || !cut_weights[1] || !cut_weights[2]) return refuse(fn, "cut_weights: three grids are required");
    if (!body || !body[0] || !body[1] || !body[2]) return refuse(fn, "body: three grids are required");
    if (!centres_host) return refuse(fn, "centres_host is NULL");
    if (s.c0 > 0 && !pressure_lo) return refuse(fn, "pressure_lo: the plane below the window is required (c0 > 0)");
    if (s.c0 > 0 && !material_lo) return refuse(fn, "material_lo: the plane below the window is required (c0 > 0)");
    return runSolidForces(fn, out_host, s.whole(), &s, pressure, s.c0 > 0 ? pressure_lo : nullptr, material, s.c0 > 0 ? material_lo : nullptr,
                          cut_weights, body, centres_host, bodies, scale, static_cast<hipStream_t>(stream));
}
MGPS_API_CATCH(nullptr)

int mgps_solid_forces_slab(struct mgps_solid_forces_slab *f, const mgps_comm *comm, const int *splits, void *stream)
try {
    SlabCall c;
    const char *fn = "mgps_solid_forces_slab";
    // ---- what every rank shares: a refusal here is every rank's, before any collective and any HIP call
    if (!f || f->struct_size != int(sizeof(struct mgps_solid_forces_slab))) return refuse(fn, "NULL or struct_size mismatch (mgps_solid_forces_slab)");
    if (int rc = c.open(fn, comm, splits, offsetof(mgps_comm, gather)); rc != MGPS_OK) return rc;
    if (int rc = forceCheckBodies(fn, f->bodies); rc != MGPS_OK) return rc;
    if (int rc = exCheckExtents(fn, f->gx, f->gy, f->gz); rc != MGPS_OK) return rc;
    const int P = c.P, rank = c.rank;
    mgps_fields_slab desc;
    if (int rc = mgps_fields_slab_describe(&desc, f->gx, f->gy, f->gz, f->power_of_two, splits, P, rank); rc != MGPS_OK) return rc;
    Slab s;
    if (!readSlab(&desc, s, fn)) return MGPS_ERR_INVALID_ARGUMENT;
    f->total_ms = f->exchange_ms = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nzl = s.c1 - s.c0;
    const bool lo = s.c0 > 0, hi = s.c1 < s.gz;
    const size_t plane = size_t(s.gx) * s.gy, cells = plane * size_t(nzl), entries = size_t(f->bodies + 1) * kForceCols;
    // ---- this rank's own arguments: a failure is carried by the agreement at the end, the rank takes part in both exchanges
    c.step([&]() -> int {
        if (!f->pressure) return refuse(fn, "pressure is NULL");
        if (!f->liquid_phi || !f->solid_phi) return refuse(fn, "liquid_phi / solid_phi: both are required");
        if (!f->cut_weights[0] || !f->cut_weights[1] || !f->cut_weights[2]) return refuse(fn, "cut_weights: three grids are required");
        if (!f->body[0] || !f->body[1] || !f->body[2]) return refuse(fn, "body: three grids are required");
        if (!f->centres) return refuse(fn, "centres is NULL");
        if (!f->out) return refuse(fn, "out is NULL");
        return MGPS_OK;
    }());
    if (P == 1 && c.status != MGPS_OK) return c.status;
    // the buffers the exchanges need: without them the rank cannot take part, and returns at once and alone
    if (int rc = selectDevice(-1); rc != MGPS_OK) return rc;
    DevPool pool;
    int32_t *material = nullptr;
    float *phiHalo = nullptr, *up = nullptr, *below = nullptr;  // messages: [pressure plane | material plane]
    try {
        material = pool.get<int32_t>(cells);
        phiHalo = pool.get<float>(2 * plane);
        if (hi) up = pool.get<float>(2 * plane);
        if (lo) below = pool.get<float>(2 * plane);
    } catch (const std::bad_alloc &) {
        return c.leave(MGPS_ERR_ALLOC, "device allocation failed");
    }
    const size_t planeBytes = plane * sizeof(float);
    float *phiLo = lo ? phiHalo : nullptr, *phiHi = hi ? phiHalo + plane : nullptr;
    {  // 1. the liquid_phi plane, both ways (a rank without the array sends what its halo buffer holds)
        const float *first = c.status == MGPS_OK ? f->liquid_phi : phiHalo, *last = c.status == MGPS_OK ? f->liquid_phi + size_t(nzl - 1) * plane : phiHalo;
        if (int rc = c.trade(lo ? first : nullptr, lo ? planeBytes : 0, phiLo, lo ? planeBytes : 0, hi ? last : nullptr, hi ? planeBytes : 0, phiHi,
                             hi ? planeBytes : 0, st, "liquid_phi");
            rc != MGPS_OK)
            return rc;
    }
    // 2. the projection's labels, made again
    if (c.status == MGPS_OK)
        c.step(mgps_fields_slab_material_labels(&desc, material, f->liquid_phi, phiLo, phiHi, f->solid_phi, f->cut_weights[0], f->cut_weights[1],
                                                f->cut_weights[2], st));
    if (P > 1) {  // 3. the last pressure plane and the last material plane go up in one message; the lower halo arrives from below
        if (hi && c.status == MGPS_OK) {
            hipStep(c, hipMemcpyAsync(up, f->pressure + size_t(nzl - 1) * plane, planeBytes, hipMemcpyDeviceToDevice, st), "packing the pressure plane");
            hipStep(c, hipMemcpyAsync(up + plane, material + size_t(nzl - 1) * plane, planeBytes, hipMemcpyDeviceToDevice, st), "packing the material plane");
        }
        if (int rc = c.trade(nullptr, 0, below, lo ? 2 * planeBytes : 0, up, hi ? 2 * planeBytes : 0, nullptr, 0, st, "pressure and material planes"); rc != MGPS_OK)
            return rc;
    }
    // 4. the window pass
    std::vector<double> rows(entries, 0.0);
    if (c.status == MGPS_OK)
        c.step(runSolidForces(fn, rows.data(), s.whole(), &s, f->pressure, lo ? below : nullptr, material,
                              lo ? reinterpret_cast<const int32_t *>(below + plane) : nullptr, f->cut_weights, f->body, f->centres, f->bodies, f->scale, st));
    // 5. the rows of all ranks travel as sums with the statuses: the one all-reduce of the call
    if (c.status != MGPS_OK) std::fill(rows.begin(), rows.end(), 0.0);
    const int rc = c.agree("rows", rows.data(), int(entries));
    if (rc == MGPS_OK) std::copy(rows.begin(), rows.end(), f->out);
    f->exchange_ms = c.exchangeMs;
    f->total_ms = SlabCall::ms(c.t0, SlabCall::Clock::now());
    return rc;
}
MGPS_API_CATCH(nullptr)

}  // extern "C"

// ---- two-way rigid-body coupling: body velocities solved with the pressure (include/mgps_fields.h) -----------
// Set-up compacts the COUPLED cells -- LIQUID cells with a wet face some body owns -- into a list in base-cell order: a count per
// workgroup of 256 consecutive cells, an exclusive scan of the counts, and a fill pass that ranks the cells of a workgroup by
// ballots.  Both passes take the faces from solidFaceTerm, the rule of the forces pass.  An application of G K G^T is three launches
// over the list: the gather g = - G^T x sums per row with addFaceTerms (the forces pass's tables: lanes of one row by shuffles, a
// table per wave, the waves' tables in wave order), one workgroup adds the workgroups' tables in index order and forms W = K g per
// row (and g^T K g for the loop's <p, A p>), and the scatter gives each coupled cell - (G W)_c: a cell is written by its own thread.
// On slab ranks (mgps_coupling_create_slab) a rank lists its own cells from its window of the grids, and g is summed over the ranks
// between the two halves of the sum stage: one all-reduce of (bodies + 1) * 6 doubles per application.
namespace {
constexpr int kCoupleThreads = 256, kCoupleWaves = kCoupleThreads / 64, kCoupleBlocksMax = 128, kCoupleSumThreads = 1024;
constexpr int kCoupleK = 7;  // K of one row: inv_mass, then inv_inertia xx, yy, zz, xy, xz, yz

struct CoupleGrids {
    Box g, e;  // the base cell grid the arrays are indexed in and the expanded grid of the list's indices: whole grids, or a rank's windows
    int offset, zoff, bodies;  // base cell (i, j, k) of g lives at (i + offset, j + offset, k + zoff) of e; zoff = offset on whole grids
    const int32_t *material;
    const float *cw[3];
    const int32_t *body[3];
};

// The six faces of cell t of the base grid, slot 2 a + d: the backward (d = 0) and forward (d = 1) face of axis a.  False unless t is
// a LIQUID cell with a wet face of row >= 1; then row[slot] is the face's row (0: not part of G) and sg[slot] its signed closed
// fraction, + s on a backward and - s on a forward face ((G V)_c = sum of sg * sv over the slots).
// Window: g is a rank's window and the cell across a face may lie on another rank.  The cell itself is LIQUID, so solidFaceTerm
// finds every face of w < 1 wet whatever lies across it: it is handed `LIQUID` for every cell and no label but the cell's own is read.
template <bool Window>
__device__ __forceinline__ bool coupledCell(const CoupleGrids &p, size_t t, int &i, int &j, int &k, int row[6], float sg[6])
{
    if (t >= p.g.cells()) return false;
    if (p.material[t] != kLiquid) return false;
    i = int(t % p.g.gx), j = int((t / p.g.gx) % p.g.gy), k = int(t / (size_t(p.g.gx) * p.g.gy));
    const GridAt<int32_t> mat{p.g, p.material};
    const auto noPressure = [](int, int, int) { return 0.f; };  // (phi is not wanted here)
    bool any = false;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            int fc[3] = {i, j, k};  // the face lies behind cell fc
            fc[a] += d;
            const size_t f = faceAt(p.g, a, fc[0], fc[1], fc[2]);
            int r = 0;
            float s = 0.f;
            double phi = 0.0;
            const auto bodyOf = [&] { return p.body[a][f]; };
            bool wet;
            if constexpr (Window) wet = solidFaceTerm(p.g, a, fc[0], fc[1], fc[2], p.cw[a][f], p.bodies, [](int, int, int) { return kLiquid; }, noPressure, bodyOf, r, s, phi);
            else wet = solidFaceTerm(p.g, a, fc[0], fc[1], fc[2], p.cw[a][f], p.bodies, mat, noPressure, bodyOf, r, s, phi);
            const bool on = wet && r >= 1;
            row[2 * a + d] = on ? r : 0;
            sg[2 * a + d] = on ? (d ? -s : s) : 0.f;
            any = any || on;
        }
    return any;
}

template <bool Window>
__device__ __forceinline__ void coupleCount(const CoupleGrids &p, int32_t *__restrict__ blockCount)
{
    int i, j, k, row[6];
    float sg[6];
    const int n = __syncthreads_count(coupledCell<Window>(p, size_t(blockIdx.x) * kCoupleThreads + threadIdx.x, i, j, k, row, sg));
    if (threadIdx.x == 0) blockCount[blockIdx.x] = n;
}
__global__ __launch_bounds__(kCoupleThreads) void coupleCountKernel(CoupleGrids p, int32_t *__restrict__ blockCount) { coupleCount<false>(p, blockCount); }
__global__ __launch_bounds__(kCoupleThreads) void coupleCountWindowKernel(CoupleGrids p, int32_t *__restrict__ blockCount) { coupleCount<true>(p, blockCount); }

// cell[e] = the expanded index, rows[slot * count + e], sg[slot * count + e]: the list, entry e = blockStart + the cell's rank in its workgroup
template <bool Window>
__device__ __forceinline__ void coupleFill(const CoupleGrids &p, const int32_t *__restrict__ blockStart, int count, int32_t *__restrict__ cell,
                                           uint8_t *__restrict__ rows, float *__restrict__ sgs)
{
    __shared__ int waveCount[kCoupleWaves];
    int i = 0, j = 0, k = 0, row[6];
    float sg[6];
    const bool on = coupledCell<Window>(p, size_t(blockIdx.x) * kCoupleThreads + threadIdx.x, i, j, k, row, sg);
    const unsigned long long mask = __ballot(on);
    const int lane = int(threadIdx.x) & 63, wave = int(threadIdx.x) >> 6;
    if (lane == 0) waveCount[wave] = __popcll(mask);
    __syncthreads();
    if (!on) return;
    int e = blockStart[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) e += waveCount[w];
    if (e >= count) return;  // (cannot happen: the count pass applied the same rule)
    cell[e] = int32_t(cellAt(p.e, i + p.offset, j + p.offset, k + p.zoff));
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        rows[size_t(s) * count + e] = uint8_t(row[s]);
        sgs[size_t(s) * count + e] = sg[s];
    }
}
__global__ __launch_bounds__(kCoupleThreads) void coupleFillKernel(CoupleGrids p, const int32_t *__restrict__ blockStart, int count,
                                                                   int32_t *__restrict__ cell, uint8_t *__restrict__ rows, float *__restrict__ sgs)
{
    coupleFill<false>(p, blockStart, count, cell, rows, sgs);
}
__global__ __launch_bounds__(kCoupleThreads) void coupleFillWindowKernel(CoupleGrids p, const int32_t *__restrict__ blockStart, int count,
                                                                         int32_t *__restrict__ cell, uint8_t *__restrict__ rows, float *__restrict__ sgs)
{
    coupleFill<true>(p, blockStart, count, cell, rows, sgs);
}

struct CoupleList {
    int count, bodies;
    int ex, ey, offset;
    int z0;  // the expanded plane of the whole grid that plane 0 of the list's indices is: 0 on whole grids, e0 on a rank's window
    const int32_t *cell;
    const uint8_t *rows;
    const float *sg;
    const double *centres;  // device, (bodies + 1) * 3
};
// base coordinates, in the whole grid, of the list's cell c (an expanded index)
__device__ __forceinline__ void coupleCoords(const CoupleList &L, int c, int &i, int &j, int &k)
{
    i = c % L.ex - L.offset;
    j = (c / L.ex) % L.ey - L.offset;
    k = c / (L.ex * L.ey) - L.offset + L.z0;
}

// partials[workgroup][(bodies + 1) * kForceCols]: columns 0 .. 5 hold the workgroup's share of g = - G^T x (the layout of the forces
// pass's tables; columns 6 and 7 are addFaceTerms' area and count, not used here)
template <class X>
__global__ __launch_bounds__(kCoupleThreads) void coupleGatherKernel(CoupleList L, const X *__restrict__ x, double *__restrict__ partials)
{
    extern __shared__ double coupleTables[];
    const int entries = (L.bodies + 1) * kForceCols;
    for (int e = int(threadIdx.x); e < kCoupleWaves * entries; e += kCoupleThreads) coupleTables[e] = 0.0;
    __syncthreads();
    double *table = coupleTables + size_t(threadIdx.x >> 6) * entries;
    const int stride = int(gridDim.x) * kCoupleThreads;
    for (int base = int(blockIdx.x) * kCoupleThreads; base < L.count; base += stride) {  // (a wave-uniform bound: every lane stays for the ballots)
        const int e = base + int(threadIdx.x);
        const bool on = e < L.count;
        const int c = on ? L.cell[e] : 0;
        const double xv = on ? double(x[c]) : 0.0;
        int i, j, k;
        coupleCoords(L, c, i, j, k);
        int row[6];
        float sg[6];
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            row[s] = on ? int(L.rows[size_t(s) * L.count + e]) : 0;
            sg[s] = row[s] ? L.sg[size_t(s) * L.count + e] : 0.f;
        }
        // - sg x: the cell's share of the push on the body along +a (phi of the forces pass, cell by cell)
        addFaceTerms<0>(table, L.centres, row[0] != 0, row[0], fabsf(sg[0]), -double(sg[0]) * xv, double(i), j + 0.5, k + 0.5);
        addFaceTerms<0>(table, L.centres, row[1] != 0, row[1], fabsf(sg[1]), -double(sg[1]) * xv, double(i + 1), j + 0.5, k + 0.5);
        addFaceTerms<1>(table, L.centres, row[2] != 0, row[2], fabsf(sg[2]), -double(sg[2]) * xv, i + 0.5, double(j), k + 0.5);
        addFaceTerms<1>(table, L.centres, row[3] != 0, row[3], fabsf(sg[3]), -double(sg[3]) * xv, i + 0.5, double(j + 1), k + 0.5);
        addFaceTerms<2>(table, L.centres, row[4] != 0, row[4], fabsf(sg[4]), -double(sg[4]) * xv, i + 0.5, j + 0.5, double(k));
        addFaceTerms<2>(table, L.centres, row[5] != 0, row[5], fabsf(sg[5]), -double(sg[5]) * xv, i + 0.5, j + 0.5, double(k + 1));
    }
    __syncthreads();
    double *out = partials + size_t(blockIdx.x) * entries;
    for (int e = int(threadIdx.x); e < entries; e += kCoupleThreads) {
        double sum = coupleTables[e];
#pragma unroll
        for (int wv = 1; wv < kCoupleWaves; ++wv) sum += coupleTables[size_t(wv) * entries + e];  // wave order
        out[e] = sum;
    }
}

// The three steps of the sum stage, each stated once: on one device coupleSumKernel takes them in one launch; on slab ranks
// coupleRankSumKernel and coupleRowsKernel take them on either side of the all-reduce of g.
// Entry e of g: the workgroups' tables added in index order (sixteen loads in flight per thread: a sum that waits for each load in
// turn took 32 us at one body and 194 us at 255); 0 without a workgroup
__device__ __forceinline__ double coupleTableSum(const double *__restrict__ partials, int e, int nblocks, int entries)
{
    const double *at = partials + (e / 6) * kForceCols + e % 6;
    double sum = 0.0;
    for (int b = 0; b < nblocks; b += 16) {
        double v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = b + q < nblocks ? at[size_t(b + q) * entries] : 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) sum += v[q];
    }
    return sum;
}
// W[r] = K[r] g[r] (inv_mass on the force, inv_inertia on the torque); returns g[r] . W[r]
__device__ __forceinline__ double coupleRowProduct(const double *gr, const double *__restrict__ k, double *__restrict__ Wr)
{
    const double w[6] = {k[0] * gr[0], k[0] * gr[1], k[0] * gr[2],
                         k[1] * gr[3] + k[4] * gr[4] + k[5] * gr[5],
                         k[4] * gr[3] + k[2] * gr[4] + k[6] * gr[5],
                         k[5] * gr[3] + k[6] * gr[4] + k[3] * gr[5]};
    double qr = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        Wr[c] = w[c];
        qr += gr[c] * w[c];
    }
    return qr;
}
// *quad += the sum of the 256 slots of q in one fixed order (one wave: four rows per lane in order, then the butterfly)
__device__ __forceinline__ void coupleQuadSum(const double *q, double *quad)
{
    if (threadIdx.x < 64 && quad) {
        const int l = int(threadIdx.x);
        const double total = waveSum(((q[l] + q[l + 64]) + q[l + 128]) + q[l + 192]);
        if (l == 0) *quad += total;
    }
}

// One workgroup: g = the workgroups' tables added; W = K g per row; *quad += the sum over the rows of g[r] . W[r] (quad may be NULL)
__global__ __launch_bounds__(kCoupleSumThreads) void coupleSumKernel(int bodies, int nblocks, const double *__restrict__ partials,
                                                                     const double *__restrict__ K, double *__restrict__ g, double *__restrict__ W,
                                                                     double *quad)
{
    extern __shared__ double coupleRows[];  // (bodies + 1) * 6, then 256 slots of q
    const int n6 = (bodies + 1) * 6, entries = (bodies + 1) * kForceCols;
    for (int e = int(threadIdx.x); e < n6; e += kCoupleSumThreads) {
        const double sum = coupleTableSum(partials, e, nblocks, entries);
        coupleRows[e] = sum;
        g[e] = sum;
    }
    double *q = coupleRows + n6;
    if (threadIdx.x < 256) q[threadIdx.x] = 0.0;
    __syncthreads();
    const int r = int(threadIdx.x);  // (bodies <= 255: a thread per row; row 0 has K = 0)
    if (r <= bodies) q[r] = coupleRowProduct(coupleRows + 6 * r, K + size_t(kCoupleK) * r, W + 6 * r);
    __syncthreads();
    coupleQuadSum(q, quad);
}
// Slab ranks, in front of the all-reduce: g = this rank's share, the workgroups' tables added (nblocks = 0, an empty list: zeros)
__global__ __launch_bounds__(kCoupleSumThreads) void coupleRankSumKernel(int bodies, int nblocks, const double *__restrict__ partials,
                                                                         double *__restrict__ g)
{
    const int n6 = (bodies + 1) * 6, entries = (bodies + 1) * kForceCols;
    for (int e = int(threadIdx.x); e < n6; e += kCoupleSumThreads) g[e] = coupleTableSum(partials, e, nblocks, entries);
}
// Slab ranks, behind it: g is the whole grid's; W = K g per row; *quad += g^T K g (quad: NULL on every rank but one, the solver
// sums its scalar over the ranks)
__global__ __launch_bounds__(256) void coupleRowsKernel(int bodies, const double *__restrict__ K, const double *__restrict__ g,
                                                        double *__restrict__ W, double *quad)
{
    __shared__ double q[256];
    const int r = int(threadIdx.x);
    q[r] = r <= bodies ? coupleRowProduct(g + 6 * r, K + size_t(kCoupleK) * r, W + 6 * r) : 0.0;
    __syncthreads();
    coupleQuadSum(q, quad);
}

// target[c] = T(double(target[c]) + sign * (G W)_c) on the list's cells.  (G K G^T x = - G W with W = K g, g = - G^T x: sign = -1 adds
// the operator, sign = +1 takes it off a residual.)  r32 (may be NULL): the float32 copy of the new value; corr (may be NULL): per
// workgroup the sum of new^2 - old^2, lanes by the butterfly, waves in wave order
template <class T>
__global__ __launch_bounds__(kCoupleThreads) void coupleScatterKernel(CoupleList L, const double *__restrict__ W, double sign, T *__restrict__ target,
                                                                      float *__restrict__ r32, double *__restrict__ corr)
{
    __shared__ double waveDelta[kCoupleWaves];
    const int e = int(blockIdx.x) * kCoupleThreads + int(threadIdx.x);
    double delta = 0.0;
    if (e < L.count) {
        const int c = L.cell[e];
        int ijk[3];
        coupleCoords(L, c, ijk[0], ijk[1], ijk[2]);
        double v = 0.0;
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const int r = int(L.rows[size_t(s) * L.count + e]);
            if (!r) continue;
            const int a = s >> 1, u = (a + 1) % 3, vv = (a + 2) % 3;
            double pos[3] = {ijk[0] + 0.5, ijk[1] + 0.5, ijk[2] + 0.5};
            pos[a] = double(ijk[a] + (s & 1));
            const double *w = W + 6 * r, *cen = L.centres + 3 * r;
            // (U + omega x d)_a = U_a + omega_u d_v - omega_v d_u
            v += double(L.sg[size_t(s) * L.count + e]) * (w[a] + w[3 + u] * (pos[vv] - cen[vv]) - w[3 + vv] * (pos[u] - cen[u]));
        }
        const double old = double(target[c]), now = old + sign * v;
        target[c] = T(now);
        if (r32) r32[c] = float(now);
        delta = now * now - old * old;
    }
    if (!corr) return;
    delta = waveSum(delta);
    if ((threadIdx.x & 63) == 0) waveDelta[threadIdx.x >> 6] = delta;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = waveDelta[0];
#pragma unroll
        for (int wv = 1; wv < kCoupleWaves; ++wv) sum += waveDelta[wv];
        corr[blockIdx.x] = sum;
    }
}
// *out += corr[0 .. n) added in a fixed order: each thread its strided share, then the threads in index order
__global__ __launch_bounds__(kCoupleThreads) void coupleCorrKernel(int n, const double *__restrict__ corr, double *out)
{
    __shared__ double part[kCoupleThreads];
    double sum = 0.0;
    for (int b = int(threadIdx.x); b < n; b += kCoupleThreads) sum += corr[b];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int t = 0; t < kCoupleThreads; ++t) total += part[t];
        *out += total;
    }
}

// sv[f] = float((U_r + omega_r x (x_f - centres[r]))_axis) on the faces of row r >= 1 of one axis; g: the box the face grids are
// indexed in, plane 0 of which is plane k0 of the whole grid
__device__ __forceinline__ void rigidVelocityFace(const Box &g, int k0, int axis, float *__restrict__ sv, const int32_t *__restrict__ body,
                                                  const double *__restrict__ centres, const double *__restrict__ motions, int bodies)
{
    int i, j, k;
    if (!unflatten(g.gx + (axis == 0), g.gy + (axis == 1), g.gz + (axis == 2), i, j, k)) return;
    const size_t f = faceAt(g, axis, i, j, k);
    const int r = body[f];
    if (r < 1 || r > bodies) return;
    k += k0;
    double pos[3] = {i + 0.5, j + 0.5, k + 0.5};
    const int ijk[3] = {i, j, k};
    pos[axis] = double(ijk[axis]);
    const int u = (axis + 1) % 3, v = (axis + 2) % 3;
    const double *m = motions + 6 * r, *c = centres + 3 * r;
    sv[f] = float(m[axis] + m[3 + u] * (pos[v] - c[v]) - m[3 + v] * (pos[u] - c[u]));
}
__global__ void rigidVelocityKernel(Box g, int axis, float *__restrict__ sv, const int32_t *__restrict__ body, const double *__restrict__ centres,
                                    const double *__restrict__ motions, int bodies)
{
    rigidVelocityFace(g, 0, axis, sv, body, centres, motions, bodies);
}
__global__ void rigidVelocityWindowKernel(Box g, int k0, int axis, float *__restrict__ sv, const int32_t *__restrict__ body,
                                          const double *__restrict__ centres, const double *__restrict__ motions, int bodies)
{
    rigidVelocityFace(g, k0, axis, sv, body, centres, motions, bodies);
}

template <class T>
struct CoupleBuf {  // a device block of the library's allocator
    T *p = nullptr;
    int get(size_t count) { return mgps::deviceAlloc(reinterpret_cast<void **>(&p), std::max<size_t>(count, 1) * sizeof(T)); }
    ~CoupleBuf()
    {
        if (p) (void)mgps::deviceFree(p);
    }
};

// the host tables of the bodies: finite, inv_mass >= 0, the diagonal of inv_inertia >= 0 (rows 1 .. bodies; row 0 is not read)
int coupleCheckBodies(const char *fn, int bodies, const double *centres, const double *invMass, const double *invInertia)
{
    if (!centres) return refuse(fn, "centres is NULL");
    if (!invMass) return refuse(fn, "inv_mass is NULL");
    if (!invInertia) return refuse(fn, "inv_inertia is NULL");
    for (int r = 1; r <= bodies; ++r) {
        if (!(std::isfinite(invMass[r]) && invMass[r] >= 0)) return refuse(fn, "inv_mass of body " + std::to_string(r) + " is negative or not finite");
        for (int c = 0; c < 6; ++c)
            if (!std::isfinite(invInertia[6 * r + c]) || (c < 3 && invInertia[6 * r + c] < 0))
                return refuse(fn, "inv_inertia of body " + std::to_string(r) + " is not finite or has a negative diagonal entry");
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(centres[3 * r + c])) return refuse(fn, "centre of body " + std::to_string(r) + " is not finite");
    }
    return MGPS_OK;
}
int coupleHip(const char *fn, hipError_t e)
{
    if (e == hipSuccess) return MGPS_OK;
    setLastGlobalError(std::string(fn) + ": " + hipGetErrorString(e));
    return MGPS_ERR_HIP;
}
}  // namespace

struct mgps_coupling {
    int bodies = 0, count = 0;
    int ex = 0, ey = 0, ez = 0, offset = 0;
    CoupleBuf<int32_t> cell;
    CoupleBuf<uint8_t> rows;
    CoupleBuf<float> sg;
    CoupleBuf<double> tables;    // [centres (b + 1) * 3 | K (b + 1) * 7 | g (b + 1) * 6 | W (b + 1) * 6]
    CoupleBuf<double> partials;  // gather: kCoupleBlocksMax tables; behind them the scatter's per-workgroup corrections
    std::vector<double> K;       // host: what the device holds (mgps_coupling_velocities forms K g on the host)
    // a slab coupling (mgps_coupling_create_slab): the list holds the rank's own cells as indices of its e1 - e0 expanded planes, and
    // g is summed over the ranks of `cm` in every application
    bool slab = false;
    int e0 = 0, e1 = 0;          // the owned expanded planes (ez: the whole grid's)
    mgps_comm cm{};              // the caller's transport at full size, as SlabCall::open keeps it
    std::vector<double> gHost;   // (a transport without allreduce_device: g goes through the host)
    bool collective() const { return slab && cm.size > 1; }
    int gatherBlocks() const { return std::min(kCoupleBlocksMax, (count + kCoupleThreads - 1) / kCoupleThreads); }
    int scatterBlocks() const { return (count + kCoupleThreads - 1) / kCoupleThreads; }
    size_t rows3() const { return size_t(bodies + 1) * 3; }
    double *centres() const { return tables.p; }
    double *Kdev() const { return tables.p + rows3(); }
    double *g() const { return Kdev() + size_t(bodies + 1) * kCoupleK; }
    double *W() const { return g() + size_t(bodies + 1) * 6; }
    double *corr() const { return partials.p + size_t(kCoupleBlocksMax) * (bodies + 1) * kForceCols; }
    CoupleList list() const { return CoupleList{count, bodies, ex, ey, offset, e0, cell.p, rows.p, sg.p, centres()}; }
};

namespace {
int coupleUpload(const char *fn, mgps_coupling *c, const double *centres, const double *invMass, const double *invInertia, hipStream_t st)
{
    const int n = c->bodies + 1;
    std::vector<double> host(c->rows3() + size_t(n) * kCoupleK, 0.0);  // (row 0: zeros, never read through a face)
    for (int r = 1; r < n; ++r) {
        for (int q = 0; q < 3; ++q) host[size_t(3) * r + q] = centres[3 * r + q];
        double *k = host.data() + c->rows3() + size_t(kCoupleK) * r;
        k[0] = invMass[r];
        for (int q = 0; q < 6; ++q) k[1 + q] = invInertia[6 * r + q];
    }
    c->K.assign(host.begin() + ptrdiff_t(c->rows3()), host.end());
    if (int rc = coupleHip(fn, hipMemcpyAsync(c->tables.p, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, st)); rc != MGPS_OK) return rc;
    return coupleHip(fn, hipStreamSynchronize(st));  // (`host` leaves scope)
}

// What a step of an application returns: 0, a hipError_t, or this when a call of the transport failed (MGPS_ERR_COMM to the caller)
constexpr int kCoupleCommFailed = mgps::kCouplingCommFailed;

// g on the device summed over the ranks, in place: on the stream where the transport can, through the host otherwise (as the
// solver's encSumOverRanks).  Every rank of a slab coupling comes here once per application, whatever its list holds
int coupleSumOverRanks(mgps_coupling *c, hipStream_t st)
{
    const int n = (c->bodies + 1) * 6;
    if (c->cm.allreduce_device) return c->cm.allreduce_device(c->cm.user, c->g(), n, 0, st) == 0 ? 0 : kCoupleCommFailed;
    c->gHost.resize(size_t(n));
    if (hipError_t e = hipMemcpyAsync(c->gHost.data(), c->g(), size_t(n) * sizeof(double), hipMemcpyDeviceToHost, st); e != hipSuccess) return int(e);
    if (hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return int(e);
    if (c->cm.allreduce(c->cm.user, c->gHost.data(), n, 0) != 0) return kCoupleCommFailed;
    if (hipError_t e = hipMemcpyAsync(c->g(), c->gHost.data(), size_t(n) * sizeof(double), hipMemcpyHostToDevice, st); e != hipSuccess) return int(e);
    return int(hipStreamSynchronize(st));
}

// gather + sum: g and W = K g on the device; *quad += g^T K g (quad may be NULL).  One device, or a world of one: nothing to do on
// an empty list (g, W stay 0).  Slab ranks: the sum stage in two halves around the all-reduce of g, and an empty list still takes
// part in it; g^T K g, a number of the whole grid, is added on rank 0 only (the solver sums its scalar over the ranks)
template <class X>
int coupleGather(mgps_coupling *c, hipStream_t st, const X *x, double *quad)
{
    const int nb = c->gatherBlocks(), entries = (c->bodies + 1) * kForceCols;
    if (!c->collective()) {
        if (c->count == 0) return 0;
        coupleGatherKernel<X><<<nb, kCoupleThreads, size_t(kCoupleWaves) * entries * sizeof(double), st>>>(c->list(), x, c->partials.p);
        coupleSumKernel<<<1, kCoupleSumThreads, (size_t(c->bodies + 1) * 6 + 256) * sizeof(double), st>>>(c->bodies, nb, c->partials.p, c->Kdev(), c->g(), c->W(), quad);
        return int(hipGetLastError());
    }
    if (c->count > 0) coupleGatherKernel<X><<<nb, kCoupleThreads, size_t(kCoupleWaves) * entries * sizeof(double), st>>>(c->list(), x, c->partials.p);
    coupleRankSumKernel<<<1, kCoupleSumThreads, 0, st>>>(c->bodies, nb, c->partials.p, c->g());
    if (int e = int(hipGetLastError())) return e;
    if (int e = coupleSumOverRanks(c, st)) return e;
    coupleRowsKernel<<<1, 256, 0, st>>>(c->bodies, c->Kdev(), c->g(), c->W(), c->cm.rank == 0 ? quad : nullptr);
    return int(hipGetLastError());
}
template <class T>
int coupleScatter(mgps_coupling *c, hipStream_t st, double sign, T *target, float *r32, double *norm2)
{
    if (c->count == 0) return 0;
    const int nb = c->scatterBlocks();
    coupleScatterKernel<T><<<nb, kCoupleThreads, 0, st>>>(c->list(), c->W(), sign, target, r32, norm2 ? c->corr() : nullptr);
    if (norm2) coupleCorrKernel<<<1, kCoupleThreads, 0, st>>>(nb, c->corr(), norm2);
    return int(hipGetLastError());
}
// the rigid velocity on the face grids of box g: the whole grid (win NULL), or a rank's window of it
int runRigidVelocity(const char *fn, const Box &g, const Slab *win, float *const sv[3], const int32_t *const body[3], const double *centresHost,
                     const double *motionsHost, int bodies, hipStream_t st)
{
    if (!sv[0] || !sv[1] || !sv[2]) return refuse(fn, "solid velocity: three grids are required");
    if (!body[0] || !body[1] || !body[2]) return refuse(fn, "body: three grids are required");
    if (!centresHost) return refuse(fn, "centres_host is NULL");
    if (!motionsHost) return refuse(fn, "motions_host is NULL");
    const size_t nc = size_t(bodies + 1) * 3, nm = size_t(bodies + 1) * 6;
    DevPool pool;
    double *dev = nullptr;  // [centres | motions]
    try {
        dev = pool.get<double>(nc + nm);
    } catch (const std::bad_alloc &) {
        setLastGlobalError(std::string(fn) + ": device allocation failed");
        return MGPS_ERR_ALLOC;
    }
    if (int rc = coupleHip(fn, hipMemcpyAsync(dev, centresHost, nc * sizeof(double), hipMemcpyHostToDevice, st)); rc != MGPS_OK) return rc;
    if (int rc = coupleHip(fn, hipMemcpyAsync(dev + nc, motionsHost, nm * sizeof(double), hipMemcpyHostToDevice, st)); rc != MGPS_OK) return rc;
    for (int a = 0; a < 3; ++a) {
        const unsigned nb = blocks(faceCount(g.gx, g.gy, g.gz, a));
        if (win) rigidVelocityWindowKernel<<<nb, 256, 0, st>>>(g, win->c0, a, sv[a], body[a], dev, dev + nc, bodies);
        else rigidVelocityKernel<<<nb, 256, 0, st>>>(g, a, sv[a], body[a], dev, dev + nc, bodies);
    }
    return coupleHip(fn, hipGetLastError());
}

// what both constructors refuse of a desc, before any device work
int coupleCheckDesc(const char *fn, const mgps_coupling_desc *d, bool wholeGrid)
{
    if (!d || d->struct_size != int(sizeof(mgps_coupling_desc))) return refuse(fn, "NULL or struct_size mismatch (mgps_coupling_desc)");
    if (int rc = forceCheckBodies(fn, d->bodies); rc != MGPS_OK) return rc;
    if (int rc = exCheckExtents(fn, d->gx, d->gy, d->gz); rc != MGPS_OK) return rc;
    if (int rc = exCheckExtents(fn, d->ex, d->ey, d->ez); rc != MGPS_OK) return rc;
    if (d->offset < 0 || d->gx + d->offset > d->ex || d->gy + d->offset > d->ey || d->gz + d->offset > d->ez)
        return refuse(fn, "the expanded box does not hold the base grid at this offset");
    // (the list's indices are int32: of the whole expanded grid here, of the rank's planes on a slab, checked with the window)
    if (wholeGrid && size_t(d->ex) * d->ey * d->ez > size_t(0x7fffffff)) return refuse(fn, "more than 2^31 - 1 expanded cells");
    if (!d->material) return refuse(fn, "material is NULL");
    if (!d->cut_weights[0] || !d->cut_weights[1] || !d->cut_weights[2]) return refuse(fn, "cut weights: three grids are required");
    if (!d->body[0] || !d->body[1] || !d->body[2]) return refuse(fn, "body: three grids are required");
    return coupleCheckBodies(fn, d->bodies, d->centres, d->inv_mass, d->inv_inertia);
}

// The object from a checked desc: count, scan, fill, tables.  win: NULL for whole grids; else the rank's window -- the desc's grids
// hold its planes, the list its own cells as indices of its e1 - e0 expanded planes
int coupleBuild(const char *fn, mgps_coupling **out, const mgps_coupling_desc *d, const Slab *win, hipStream_t st)
{
    std::unique_ptr<mgps_coupling> c(new mgps_coupling);
    c->bodies = d->bodies;
    c->ex = d->ex, c->ey = d->ey, c->ez = d->ez, c->offset = d->offset;
    c->e1 = d->ez;
    CoupleGrids p{Box{d->gx, d->gy, d->gz}, Box{d->ex, d->ey, d->ez}, d->offset, d->offset, d->bodies, d->material, {d->cut_weights[0], d->cut_weights[1], d->cut_weights[2]},
                  {d->body[0], d->body[1], d->body[2]}};
    if (win) {
        c->slab = true;
        c->e0 = win->e0, c->e1 = win->e1;
        p.g = win->base(), p.e = win->window();
        p.zoff = win->c0 + win->off - win->e0;  // (base plane c0 is expanded plane c0 + offset of the whole grid)
    }
    const size_t nblocks = (p.g.cells() + kCoupleThreads - 1) / kCoupleThreads;
    if (nblocks > size_t(0x7fffffff)) return refuse(fn, "the base grid is too large");
    const auto noMemory = [&] {
        setLastGlobalError(std::string(fn) + ": device allocation failed");
        return MGPS_ERR_ALLOC;
    };
    {
        CoupleBuf<int32_t> blockCount, blockStart, scratch;
        if (blockCount.get(nblocks) || blockStart.get(nblocks + 1) || scratch.get(scanScratchInts(nblocks))) return noMemory();
        if (win) coupleCountWindowKernel<<<unsigned(nblocks), kCoupleThreads, 0, st>>>(p, blockCount.p);
        else coupleCountKernel<<<unsigned(nblocks), kCoupleThreads, 0, st>>>(p, blockCount.p);
        if (int rc = coupleHip(fn, hipGetLastError()); rc != MGPS_OK) return rc;
        if (int e = launchExclusiveScan(st, blockCount.p, blockStart.p, nblocks, scratch.p)) return coupleHip(fn, hipError_t(e));
        int32_t total = 0;
        if (int rc = coupleHip(fn, hipMemcpyAsync(&total, blockStart.p + nblocks, sizeof(total), hipMemcpyDeviceToHost, st)); rc != MGPS_OK) return rc;
        if (int rc = coupleHip(fn, hipStreamSynchronize(st)); rc != MGPS_OK) return rc;
        c->count = total;
        const size_t n = size_t(std::max(total, 1)), tab = size_t(d->bodies + 1);
        if (c->cell.get(n) || c->rows.get(6 * n) || c->sg.get(6 * n) || c->tables.get(tab * (3 + kCoupleK + 6 + 6)) ||
            c->partials.get(size_t(kCoupleBlocksMax) * tab * kForceCols + size_t(c->scatterBlocks()) + 1))
            return noMemory();
        if (total > 0) {
            if (win) coupleFillWindowKernel<<<unsigned(nblocks), kCoupleThreads, 0, st>>>(p, blockStart.p, total, c->cell.p, c->rows.p, c->sg.p);
            else coupleFillKernel<<<unsigned(nblocks), kCoupleThreads, 0, st>>>(p, blockStart.p, total, c->cell.p, c->rows.p, c->sg.p);
        }
        if (int rc = coupleHip(fn, hipGetLastError()); rc != MGPS_OK) return rc;
        if (int rc = coupleHip(fn, hipMemsetAsync(c->tables.p, 0, tab * (3 + kCoupleK + 6 + 6) * sizeof(double), st)); rc != MGPS_OK) return rc;
        if (int rc = coupleHip(fn, hipStreamSynchronize(st)); rc != MGPS_OK) return rc;  // (the scan's buffers leave scope)
    }
    if (int rc = coupleUpload(fn, c.get(), d->centres, d->inv_mass, d->inv_inertia, st); rc != MGPS_OK) return rc;
    *out = c.release();
    return MGPS_OK;
}

// the status of a public entry from what a step returned
int coupleStatus(const char *fn, int e)
{
    if (e != kCoupleCommFailed) return coupleHip(fn, hipError_t(e));
    setLastGlobalError(std::string(fn) + ": all-reduce failed (the impulses g)");
    return MGPS_ERR_COMM;
}
}  // namespace

namespace mgps {
void couplingExtents(const mgps_coupling *c, int e[3]) { e[0] = c->ex, e[1] = c->ey, e[2] = c->ez; }
bool couplingOnSlab(const mgps_coupling *c, int planes[2], int *rank, int *size)
{
    planes[0] = c->e0, planes[1] = c->e1;
    *rank = c->cm.rank, *size = c->cm.size;
    return c->slab;
}
int couplingApply64(mgps_coupling *c, void *stream, double *t, const double *p, double *dotDev)
{
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int e = coupleGather(c, st, p, dotDev)) return e;
    return coupleScatter<double>(c, st, -1.0, t, nullptr, nullptr);
}
int couplingResidual64(mgps_coupling *c, void *stream, double *r, const double *x, float *r32, double *norm2Dev)
{
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int e = coupleGather(c, st, x, static_cast<double *>(nullptr))) return e;
    return coupleScatter<double>(c, st, 1.0, r, r32, norm2Dev);
}
}  // namespace mgps

extern "C" {

int mgps_fields_rigid_velocity(float *svx, float *svy, float *svz, const int32_t *bx, const int32_t *by, const int32_t *bz,
                               const double *centres_host, const double *motions_host, int bodies, int gx, int gy, int gz, void *stream)
try {
    const char *fn = "mgps_fields_rigid_velocity";
    if (int rc = forceCheckBodies(fn, bodies); rc != MGPS_OK) return rc;
    if (int rc = exCheckExtents(fn, gx, gy, gz); rc != MGPS_OK) return rc;
    float *sv[3] = {svx, svy, svz};
    const int32_t *body[3] = {bx, by, bz};
    return runRigidVelocity(fn, Box{gx, gy, gz}, nullptr, sv, body, centres_host, motions_host, bodies, static_cast<hipStream_t>(stream));
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_rigid_velocity(const mgps_fields_slab *d, float *const sv[3], const int32_t *const body[3], const double *centres_host,
                                    const double *motions_host, int bodies, void *stream)
try {
    const char *fn = "mgps_fields_slab_rigid_velocity";
    Slab s;
    if (!readSlab(d, s, fn)) return MGPS_ERR_INVALID_ARGUMENT;
    if (int rc = forceCheckBodies(fn, bodies); rc != MGPS_OK) return rc;
    if (!sv) return refuse(fn, "solid velocity: three grids are required");
    if (!body) return refuse(fn, "body: three grids are required");
    return runRigidVelocity(fn, s.base(), &s, sv, body, centres_host, motions_host, bodies, static_cast<hipStream_t>(stream));
}
MGPS_API_CATCH(nullptr)

int mgps_coupling_create(mgps_coupling **out, const mgps_coupling_desc *d, void *stream)
try {
    const char *fn = "mgps_coupling_create";
    if (!out) return refuse(fn, "out is NULL");
    *out = nullptr;
    if (int rc = coupleCheckDesc(fn, d, true); rc != MGPS_OK) return rc;
    return coupleBuild(fn, out, d, nullptr, static_cast<hipStream_t>(stream));
}
MGPS_API_CATCH(nullptr)

int mgps_coupling_create_slab(mgps_coupling **out, const mgps_coupling_desc *d, const mgps_fields_slab *window, const mgps_comm *comm, void *stream)
try {
    const char *fn = "mgps_coupling_create_slab";
    if (!out) return refuse(fn, "out is NULL");
    *out = nullptr;
    if (int rc = coupleCheckDesc(fn, d, false); rc != MGPS_OK) return rc;
    Slab s;
    if (!readSlab(window, s, fn)) return MGPS_ERR_INVALID_ARGUMENT;
    if (s.gx != d->gx || s.gy != d->gy || s.gz != d->gz || s.ex != d->ex || s.ey != d->ey || s.ez != d->ez || s.off != d->offset)
        return refuse(fn, "the window does not match the desc (gx .. ez and offset are the whole grid's in both)");
    if (size_t(s.ex) * s.ey * size_t(s.e1 - s.e0) > size_t(0x7fffffff)) return refuse(fn, "more than 2^31 - 1 expanded cells in the window");
    if (!comm || comm->struct_size < int(offsetof(mgps_comm, gather)) || comm->struct_size > int(sizeof(mgps_comm)) || !comm->exchange || !comm->allreduce ||
        comm->size < 1 || comm->rank < 0 || comm->rank >= comm->size)
        return refuse(fn, "comm: a mgps_comm with exchange and allreduce is required");
    mgps_comm cm{};
    std::memcpy(&cm, comm, size_t(comm->struct_size));  // (members behind the caller's struct_size read as NULL)
    cm.struct_size = int(sizeof(mgps_comm));
    const int rc = coupleBuild(fn, out, d, &s, static_cast<hipStream_t>(stream));
    if (rc == MGPS_OK) (*out)->cm = cm;
    return rc;
}
MGPS_API_CATCH(nullptr)

void mgps_coupling_destroy(mgps_coupling *c)
{
    if (!c) return;
    (void)hipDeviceSynchronize();  // (deviceFree does not wait for queued kernels)
    delete c;
}

int mgps_coupling_set_bodies(mgps_coupling *c, const double *centres_host, const double *inv_mass_host, const double *inv_inertia_host, void *stream)
try {
    const char *fn = "mgps_coupling_set_bodies";
    if (!c) return refuse(fn, "NULL coupling");
    if (int rc = coupleCheckBodies(fn, c->bodies, centres_host, inv_mass_host, inv_inertia_host); rc != MGPS_OK) return rc;
    return coupleUpload(fn, c, centres_host, inv_mass_host, inv_inertia_host, static_cast<hipStream_t>(stream));
}
MGPS_API_CATCH(nullptr)

int mgps_coupling_cells(const mgps_coupling *c, int64_t *count)
{
    if (!c || !count) return refuse("mgps_coupling_cells", "NULL argument");
    *count = c->count;
    return MGPS_OK;
}

int mgps_coupling_apply(mgps_coupling *c, float *y_dev, const float *x_dev, void *stream)
try {
    const char *fn = "mgps_coupling_apply";
    if (!c) return refuse(fn, "NULL coupling");
    if (!y_dev || !x_dev) return refuse(fn, "NULL grid");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int e = coupleGather(c, st, x_dev, static_cast<double *>(nullptr))) return coupleStatus(fn, e);
    return coupleHip(fn, hipError_t(coupleScatter<float>(c, st, -1.0, y_dev, nullptr, nullptr)));
}
MGPS_API_CATCH(nullptr)

int mgps_coupling_impulses(mgps_coupling *c, const float *x_dev, double *out_host, void *stream)
try {
    const char *fn = "mgps_coupling_impulses";
    if (!c) return refuse(fn, "NULL coupling");
    if (!x_dev) return refuse(fn, "x is NULL");
    if (!out_host) return refuse(fn, "out_host is NULL");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = size_t(c->bodies + 1) * 6;
    std::fill(out_host, out_host + n, 0.0);
    if (c->count == 0 && !c->collective()) return coupleHip(fn, hipStreamSynchronize(st));  // (an empty rank still joins the all-reduce)
    if (int e = coupleGather(c, st, x_dev, static_cast<double *>(nullptr))) return coupleStatus(fn, e);
    if (int rc = coupleHip(fn, hipMemcpyAsync(out_host, c->g(), n * sizeof(double), hipMemcpyDeviceToHost, st)); rc != MGPS_OK) return rc;
    return coupleHip(fn, hipStreamSynchronize(st));
}
MGPS_API_CATCH(nullptr)

int mgps_coupling_velocities(mgps_coupling *c, const float *x_dev, const double *v_in_host, double *v_out_host, double *impulses_host, void *stream)
try {
    const char *fn = "mgps_coupling_velocities";
    if (!c) return refuse(fn, "NULL coupling");
    if (!v_in_host || !v_out_host) return refuse(fn, "NULL velocity table");
    std::vector<double> g(size_t(c->bodies + 1) * 6);
    if (int rc = mgps_coupling_impulses(c, x_dev, g.data(), stream); rc != MGPS_OK) return rc;
    for (int r = 0; r <= c->bodies; ++r) {
        const double *gr = g.data() + 6 * r, *k = c->K.data() + size_t(kCoupleK) * r, *in = v_in_host + 6 * r;
        double *o = v_out_host + 6 * r;
        for (int q = 0; q < 3; ++q) o[q] = in[q] + k[0] * gr[q];
        o[3] = in[3] + (k[1] * gr[3] + k[4] * gr[4] + k[5] * gr[5]);
        o[4] = in[4] + (k[4] * gr[3] + k[2] * gr[4] + k[6] * gr[5]);
        o[5] = in[5] + (k[5] * gr[3] + k[6] * gr[4] + k[3] * gr[5]);
    }
    if (impulses_host) std::copy(g.begin(), g.end(), impulses_host);
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

}  // extern "C"
