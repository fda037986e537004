// FLIP particles on the device (include/mgps_fields.h, "FLIP particles"): particles in cell order, particles ->
// grid, grid -> particles and move.
// bin: a key kernel, rocprim's stable radix sort over the bits that cells + 1 needs, a lower bound per cell and one gather, in stream
// order with temporary storage from the stream's pool.
// to grid: one launch over the tiles of mgps_tile_pass.h.  A thread owns its cell's phi and the backward face of its cell per axis, and
// the forward face where the grid ends (CellFaces' ownership), and adds every particle of the cells a target's definition names into
// that target's fp64 accumulators, in ascending k, j, i and slot.  Two kernels do that walk: the staged march (the default: source
// planes upward, each row's run of slots through LDS) and the plain gather (every target's 27 cells from global memory).  No target is
// written by two threads and no sum depends on a schedule: the same inputs give the same bits, in both.  All arithmetic of the
// transfer is fp64 and rounded operation by operation -- no contraction in this unit -- so that tests/particles_reference.py, which
// states the same operations in numpy, has the same bits.
// update: one thread per particle; the grids are sampled with mgps_sample.h's rule, which advection shares and which pins its own
// contraction; the trace's fused multiply-adds are written out.
// collide: the push-out rule of the header, one device function that the standalone kernel applies to the
// arrays and the update applies to its own float32 results in registers -- updateKernel is written once, over its argument type.
// resample: a count per cell, rocprim's exclusive scan into cell_start_out, a copy per input slot (its cell from its position, its
// rank from the stride rule in closed form) and a seeding kernel over (cell, q); stream order, temporary storage from the pool.
#include <cmath>
#include <cstdint>
#include <type_traits>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "mgps_sample.h"
#include "mgps_tile_pass.h"

#pragma clang fp contract(off)

using namespace mgps;

namespace {

constexpr int kFlat = 256;  // threads of the per-particle and per-cell launches

inline unsigned flatBlocks(size_t n) { return unsigned((n + kFlat - 1) / kFlat); }

// inside: 0 <= x_c <= g_c for all three components (false for NaN); the cell: min(int(floor(x_c)), g_c - 1) per component
__device__ __forceinline__ bool insideBox(float x, float y, float z, int gx, int gy, int gz)
{
    return x >= 0.0f && double(x) <= double(gx) && y >= 0.0f && double(y) <= double(gy) && z >= 0.0f && double(z) <= double(gz);
}

// ---- bin ---------------------------------------------------------------------------------------------------------------------------
struct BinArgs {
    int gx, gy, gz, n, cells;
    const float *pin[3], *vin[3];
    float *pout[3], *vout[3];
    int32_t *order, *cellStart;
    unsigned long long *counts;
};

__global__ __launch_bounds__(kFlat) void binKeyKernel(BinArgs a, int32_t *key, int32_t *index)
{
    const int p = int(blockIdx.x) * kFlat + int(threadIdx.x);
    if (p >= a.n) return;
    const float x = a.pin[0][p], y = a.pin[1][p], z = a.pin[2][p];
    int c = a.cells;  // the outside bin
    if (insideBox(x, y, z, a.gx, a.gy, a.gz)) {
        const int i = min(int(floorf(x)), a.gx - 1), j = min(int(floorf(y)), a.gy - 1), k = min(int(floorf(z)), a.gz - 1);
        c = (k * a.gy + j) * a.gx + i;
    }
    key[p] = c, index[p] = p;
}

// the first slot whose key is >= c, for c = 0 .. cells + 1 (cells + 1: n)
__device__ __forceinline__ int lowerBound(const int32_t *sorted, int n, int c)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (sorted[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kFlat) void binStartKernel(BinArgs a, const int32_t *sorted)
{
    __shared__ unsigned int tally[2];
    zeroTally(tally);
    __syncthreads();
    const long long c = (long long)blockIdx.x * kFlat + int(threadIdx.x);
    unsigned int found[2] = {0, 0};
    if (c <= (long long)a.cells + 1) {
        const int first = lowerBound(sorted, a.n, int(c));
        a.cellStart[c] = first;
        if (c == a.cells) found[0] = unsigned(a.n - first);
        if (c < a.cells && first < a.n && sorted[first] == int(c)) found[1] = 1;
    }
    if (a.counts) addTally(tally, found, a.counts);
}

__global__ __launch_bounds__(kFlat) void binGatherKernel(BinArgs a)
{
    const int s = int(blockIdx.x) * kFlat + int(threadIdx.x);
    if (s >= a.n) return;
    const int p = a.order[s];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a.pout[c][s] = a.pin[c][p];
        if (a.vout[0]) a.vout[c][s] = a.vin[c][p];
    }
}

// what every entry refuses of its grid and its count
int checkParticleGrid(const char *fn, int gx, int gy, int gz, int n)
{
    if (gx < 1 || gy < 1 || gz < 1)
        return refuse(fn, "non-positive extent (gx, gy, gz = " + std::to_string(gx) + ", " + std::to_string(gy) + ", " + std::to_string(gz) + ")");
    if ((long long)gx * gy * gz + 1 >= (1LL << 31))
        return refuse(fn, "too many cells for the int32 keys: gx gy gz + 1 must be < 2^31");
    if (n < 0) return refuse(fn, "n = " + std::to_string(n) + " is negative");
    return MGPS_OK;
}

int allOrNone(const char *fn, const void *const p[3], const std::string &name, int &set)
{
    set = (p[0] != nullptr) + (p[1] != nullptr) + (p[2] != nullptr);
    if (set != 0 && set != 3) return refuse(fn, name + ": all three arrays, or none");
    return MGPS_OK;
}

std::string indexed(const char *base, int c) { return std::string(base) + "[" + std::to_string(c) + "]"; }

size_t faceElems(int gx, int gy, int gz, int axis)
{
    return size_t(gx + (axis == 0)) * size_t(gy + (axis == 1)) * size_t(gz + (axis == 2));
}

int streamAlloc(const char *fn, hipStream_t st, size_t bytes, void **dev)
{
    if (const hipError_t e = hipMallocAsync(dev, bytes, st); e != hipSuccess) {
        (void)hipGetLastError();
        *dev = nullptr;
        setLastGlobalError(std::string(fn) + ": device allocation failed (" + hipGetErrorString(e) + ")");
        return e == hipErrorNoDevice || e == hipErrorInvalidDevice ? MGPS_ERR_NO_DEVICE : MGPS_ERR_ALLOC;
    }
    return MGPS_OK;
}

// ---- particles -> grid ---------------------------------------------------------------------------------------------------------------
struct ToGridArgs {
    int gx, gy, planes;  // (planes = gz: the box in CellFaces' terms)
    int n;
    double radius, dx;
    const float *pos[3], *vel[3];
    const int32_t *cellStart;
    float *vout[3], *wout[3];
    uint8_t *known[3];
    float *phi;
    unsigned long long *counts;
};

__device__ __forceinline__ double hat(double d) { return fmax(0.0, 1.0 - fabs(d)); }

// the slots [s0, s1) of the cells [c0, c1) of one row, clamped into [0, n]: device data cannot be refused
__device__ __forceinline__ void slotsOf(const ToGridArgs &a, int c0, int c1, int &s0, int &s1)
{
    s0 = min(max(a.cellStart[c0], 0), a.n), s1 = min(max(a.cellStart[c1], 0), a.n);
}

// a face's three stores from its sums; counts it where it is known
__device__ __forceinline__ void putFace(const ToGridArgs &a, int c, size_t f, double num, double den, unsigned int &knownFaces)
{
    const bool known = den > 0.0;
    put(a.vout[c] + f, known ? float(num / den) : 0.0f);
    if (a.wout[0]) put(a.wout[c] + f, float(den));
    put(a.known[c] + f, uint8_t(known));
    knownFaces += known;
}

// a cell's phi from the least squared distance; counts it where phi <= 0
__device__ __forceinline__ void putPhi(const ToGridArgs &a, size_t cell, double least, unsigned int &inside)
{
    const double phi = a.dx * (fmin(sqrt(least), 1.5) - a.radius);
    if (a.phi) put(a.phi + cell, float(phi));
    inside += phi <= 0.0;
}

// does any of the (kTZ + 2) x (kTY + 2) rows of kTX + 2 cells around the tile hold a particle?  (two barriers)
__device__ __forceinline__ bool tileOccupied(const ToGridArgs &a, const TileThread &th, int &occupied)
{
    if (th.t == 0) occupied = 0;
    __syncthreads();
    if (th.t < (kTY + 2) * (kTZ + 2)) {
        const int jy = th.j0 - 1 + th.t % (kTY + 2), kz = th.k0 - 1 + th.t / (kTY + 2);
        if (jy >= 0 && jy < a.gy && kz >= 0 && kz < a.planes) {
            const int row = (kz * a.gy + jy) * a.gx;
            int s0, s1;
            slotsOf(a, row + max(th.i0 - 1, 0), row + min(th.i0 + kTX + 1, a.gx), s0, s1);
            if (s1 > s0) occupied = 1;
        }
    }
    __syncthreads();
    return occupied != 0;
}

// FORM 1, the plain gather: every thread reads its particles from global memory (L2 and the vector cache serve the neighbours' reuse)
__global__ __launch_bounds__(kThreads) void toGridKernel(ToGridArgs a)
{
    __shared__ unsigned int tally[2];
    __shared__ int occupied;
    const TileThread th;
    zeroTally(tally);
    const bool any = tileOccupied(a, th, occupied);

    unsigned int found[2] = {0, 0};
    const int i = th.i, j = th.j;
    if (i < a.gx && j < a.gy) {
        for (int kk = 0; kk < kTZ; ++kk) {
            const int k = th.k0 + kk;
            if (k >= a.planes) break;
            const CellFaces at(a, i, j, k);
            // [0 .. 2]: the backward faces, [3 .. 5]: the forward ones (where the grid ends)
            double num[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, den[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, least = INFINITY;
            const double node[3] = {double(i), double(j), double(k)}, centre[3] = {node[0] + 0.5, node[1] + 0.5, node[2] + 0.5};
            if (any) {
                for (int dz = -1; dz <= 1; ++dz) {
                    const int kz = k + dz;
                    if (kz < 0 || kz >= a.planes) continue;
                    for (int dy = -1; dy <= 1; ++dy) {
                        const int jy = j + dy;
                        if (jy < 0 || jy >= a.gy) continue;
                        const int row = (kz * a.gy + jy) * a.gx;
                        for (int dxc = -1; dxc <= 1; ++dxc) {
                            const int ix = i + dxc;
                            if (ix < 0 || ix >= a.gx) continue;
                            int s0, s1;
                            slotsOf(a, row + ix, row + ix + 1, s0, s1);
                            const int off[3] = {dxc, dy, dz};
                            for (int s = s0; s < s1; ++s) {
                                double hc[3], hb[3], hf[3], d[3], v[3];
#pragma unroll
                                for (int c = 0; c < 3; ++c) {
                                    const double x = double(a.pos[c][s]);
                                    d[c] = x - centre[c];
                                    v[c] = double(a.vel[c][s]);
                                    hc[c] = hat(d[c]), hb[c] = hat(x - node[c]), hf[c] = hat(x - (node[c] + 1.0));
                                }
                                least = fmin(least, (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
                                for (int c = 0; c < 3; ++c) {
                                    if (off[c] <= 0) {
                                        const double w = ((c == 0 ? hb[0] : hc[0]) * (c == 1 ? hb[1] : hc[1])) * (c == 2 ? hb[2] : hc[2]);
                                        num[c] = num[c] + w * v[c];
                                        den[c] = den[c] + w;
                                    }
                                    if (at.more[c] && off[c] >= 0) {
                                        const double w = ((c == 0 ? hf[0] : hc[0]) * (c == 1 ? hf[1] : hc[1])) * (c == 2 ? hf[2] : hc[2]);
                                        num[3 + c] = num[3 + c] + w * v[c];
                                        den[3 + c] = den[3 + c] + w;
                                    }
                                }
                            }
                        }
                    }
                }
            }
            putPhi(a, at.c, least, found[1]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                putFace(a, c, at.f[c], num[c], den[c], found[0]);
                if (at.more[c]) putFace(a, c, at.f[c] + at.step[c], num[3 + c], den[3 + c], found[0]);
            }
        }
    }
    if (a.counts) addTally(tally, found, a.counts);
}

// FORM 2, the staged march.  The tile marches the source planes k0 - 1 .. k0 + kTZ upward; per plane it stages the particles of the
// rows j0 - 1 .. j0 + kTY, cells i0 - 1 .. i0 + kTX -- binned, so each row is ONE run of slots -- in LDS, kChunk particles at a time, and
// every thread adds the particles of its three cells of the row into the accumulators of its column's targets on the planes kz - 1,
// kz, kz + 1.  Marching upward, rows and slots ascending, visits every target's sources in the order the definition states, so the
// bits are FORM 1's.  A particle's hats along x and y are formed once for the three planes.  The forward faces where the grid ends
// are few: their threads gather them from global memory afterwards.
constexpr int kChunk = 768;  // particles per staged chunk: 6 floats each, 18 KiB of LDS; a row of 66 cells at 8 per cell is 528

struct Sums {
    double num[3], den[3], least;
};
__device__ __forceinline__ Sums noSums() { return Sums{{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, INFINITY}; }

// the forward face of axis c of cell (i, j, k), whose far cells lie outside the grid: the cells with offset 0 along c, as FORM 1 walks them
__device__ __forceinline__ void forwardFace(const ToGridArgs &a, int c, int i, int j, int k, double &num, double &den)
{
    const double node[3] = {double(i) + (c == 0 ? 1.0 : 0.5), double(j) + (c == 1 ? 1.0 : 0.5), double(k) + (c == 2 ? 1.0 : 0.5)};
    num = den = 0.0;
    for (int dz = (c == 2 ? 0 : -1); dz <= (c == 2 ? 0 : 1); ++dz) {
        const int kz = k + dz;
        if (kz < 0 || kz >= a.planes) continue;
        for (int dy = (c == 1 ? 0 : -1); dy <= (c == 1 ? 0 : 1); ++dy) {
            const int jy = j + dy;
            if (jy < 0 || jy >= a.gy) continue;
            const int row = (kz * a.gy + jy) * a.gx;
            for (int dxc = (c == 0 ? 0 : -1); dxc <= (c == 0 ? 0 : 1); ++dxc) {
                const int ix = i + dxc;
                if (ix < 0 || ix >= a.gx) continue;
                int s0, s1;
                slotsOf(a, row + ix, row + ix + 1, s0, s1);
                for (int s = s0; s < s1; ++s) {
                    const double w = (hat(double(a.pos[0][s]) - node[0]) * hat(double(a.pos[1][s]) - node[1])) * hat(double(a.pos[2][s]) - node[2]);
                    num = num + w * double(a.vel[c][s]);
                    den = den + w;
                }
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void toGridStagedKernel(ToGridArgs a)
{
    __shared__ unsigned int tally[2];
    __shared__ int occupied;
    __shared__ int rowStart[kTX + 3];  // the first slots of the cells i0 - 1 .. i0 + kTX of the row, and the row's end
    __shared__ float staged[6][kChunk];
    const TileThread th;
    zeroTally(tally);
    const bool any = tileOccupied(a, th, occupied);

    unsigned int found[2] = {0, 0};
    const int i = th.i, j = th.j;
    const bool column = i < a.gx && j < a.gy;
    const int top = min(th.k0 + kTZ, a.planes);  // the tile's planes: [k0, top)
    const double nodeX = double(i), centreX = nodeX + 0.5, nodeY = double(j), centreY = nodeY + 0.5;
    Sums below = noSums(), level = noSums(), above = noSums();  // the targets on the planes kz - 1, kz, kz + 1
    for (int kz = th.k0 - 1; kz <= top; ++kz) {
        if (any && kz >= 0 && kz < a.planes) {
            // (uniform) which of the three planes are the tile's
            const bool onBelow = kz - 1 >= th.k0, onLevel = kz >= th.k0 && kz < top, onAbove = kz + 1 < top;
            const double nodeZ[3] = {double(kz - 1), double(kz), double(kz + 1)};
            for (int jy = max(th.j0 - 1, 0); jy <= min(th.j0 + kTY, a.gy - 1); ++jy) {
                const int row = (kz * a.gy + jy) * a.gx;
                __syncthreads();  // (the previous row's readers are done)
                if (th.t < kTX + 3) {
                    int s0, s1;
                    slotsOf(a, row + min(max(th.i0 - 1 + th.t, 0), a.gx), row, s0, s1);
                    rowStart[th.t] = s0;
                }
                __syncthreads();
                const int rs0 = rowStart[0], rs1 = rowStart[kTX + 2];
                // this thread's cells i - 1 .. i + 1 of the row: [mine0, mine1); the slots below `ahead` lie in the cells i - 1 and i
                const bool reads = column && jy >= j - 1 && jy <= j + 1;
                const int mine0 = rowStart[th.lane], ahead = rowStart[th.lane + 2], mine1 = rowStart[th.lane + 3];
                const bool yBack = jy <= j;
                for (long long base = rs0; base < rs1; base += kChunk) {
                    const int len = int(min((long long)kChunk, rs1 - base));
                    if (base != rs0) __syncthreads();  // (the previous chunk's readers are done)
                    for (int q = th.t; q < len; q += kThreads) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) staged[c][q] = a.pos[c][base + q], staged[3 + c][q] = a.vel[c][base + q];
                    }
                    __syncthreads();
                    if (!reads) continue;
                    const int q0 = int(max((long long)mine0, base) - base), q1 = int(min((long long)mine1, base + len) - base);
                    for (int q = q0; q < q1; ++q) {
                        const double x = double(staged[0][q]), y = double(staged[1][q]), z = double(staged[2][q]);
                        const double v[3] = {double(staged[3][q]), double(staged[4][q]), double(staged[5][q])};
                        const double dx = x - centreX, dy = y - centreY;
                        const double hxc = hat(dx), hyc = hat(dy), hxb = hat(x - nodeX), hyb = hat(y - nodeY);
                        const double flat = dx * dx + dy * dy;
                        const bool xBack = base + q < ahead;
                        Sums *const on[3] = {&below, &level, &above};
                        const bool use[3] = {onBelow, onLevel, onAbove};
#pragma unroll
                        for (int t = 0; t < 3; ++t) {
                            if (!use[t]) continue;
                            Sums &g = *on[t];
                            const double dz = z - (nodeZ[t] + 0.5);
                            const double hzc = hat(dz);
                            g.least = fmin(g.least, flat + dz * dz);
                            if (xBack) {
                                const double w = (hxb * hyc) * hzc;
                                g.num[0] = g.num[0] + w * v[0], g.den[0] = g.den[0] + w;
                            }
                            if (yBack) {
                                const double w = (hxc * hyb) * hzc;
                                g.num[1] = g.num[1] + w * v[1], g.den[1] = g.den[1] + w;
                            }
                            if (t >= 1) {  // the z-face of plane k takes the cells k - 1 and k: the source plane is not above it
                                const double w = (hxc * hyc) * hat(z - nodeZ[t]);
                                g.num[2] = g.num[2] + w * v[2], g.den[2] = g.den[2] + w;
                            }
                        }
                    }
                }
            }
        }
        // the plane kz - 1 has seen its three source planes
        if (column && kz - 1 >= th.k0) {
            const CellFaces at(a, i, j, kz - 1);
            putPhi(a, at.c, below.least, found[1]);
#pragma unroll
            for (int c = 0; c < 3; ++c) putFace(a, c, at.f[c], below.num[c], below.den[c], found[0]);
        }
        below = level, level = above, above = noSums();
    }
    if (column) {
        for (int k = th.k0; k < top; ++k) {
            const CellFaces at(a, i, j, k);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (!at.more[c]) continue;
                double num, den;
                forwardFace(a, c, i, j, k, num, den);
                putFace(a, c, at.f[c] + at.step[c], num, den, found[0]);
            }
        }
    }
    if (a.counts) addTally(tally, found, a.counts);
}

// ---- grid -> particles, and move ---------------------------------------------------------------------------------------------------
struct UpdateArgs {
    int gx, gy, gz, n, order;
    double dt, flip;
    const float *pin[3], *vin[3];
    float *pout[3], *vout[3];
    const float *gnew[3], *gold[3];  // gold[0] == nullptr: old = pic
    unsigned long long *counts;
};

// S(p) of a whole grid of `kind` (0 cells, 1 + a the faces of axis a)
__device__ __forceinline__ double sampleAt(int gx, int gy, int gz, int kind, const float *grid, double px, double py, double pz)
{
    const Lattice L = latticeOf(gx, gy, gz, 0, gz, 0, 0, kind);
    const Stencil s = stencilAt(L, px, py, pz);
    double lo, hi;
    return sampleHeld(HeldPlanes{grid, nullptr, nullptr}, L, s, lo, hi);
}

// U(p) of three face grids of the whole grid
template <class Box>
__device__ __forceinline__ void velocityAt(const Box &a, const float *const grid[3], const double p[3], double u[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = sampleAt(a.gx, a.gy, a.gz, c + 1, grid[c], p[0], p[1], p[2]);
}

// ---- collision with solids: the rule (include/mgps_fields.h, "4. mgps_particles_collide") ----------------------------------------
struct SolidArgs {
    int gx, gy, gz, iterations;
    double margin, friction;
    const float *phi;
    const float *sv[3];  // sv[0] == nullptr: the solid is at rest
    unsigned long long *counts;
};

// the rule on one particle's float32 position and velocity, in place; found: [0] pushed, [1] still inside the solid, [2] stuck
__device__ __forceinline__ void collideRule(const SolidArgs &s, float (&xf)[3], float (&vf)[3], unsigned int (&found)[3])
{
    if (!insideBox(xf[0], xf[1], xf[2], s.gx, s.gy, s.gz)) return;
    const double box[3] = {double(s.gx), double(s.gy), double(s.gz)};
    double x[3] = {double(xf[0]), double(xf[1]), double(xf[2])}, n[3] = {0.0, 0.0, 0.0};
    bool pushed = false;
    for (int it = 0; it < s.iterations; ++it) {
        const double phi = sampleAt(s.gx, s.gy, s.gz, 0, s.phi, x[0], x[1], x[2]);
        if (phi >= s.margin) break;
        const double g[3] = {sampleAt(s.gx, s.gy, s.gz, 0, s.phi, x[0] + 0.5, x[1], x[2]) - sampleAt(s.gx, s.gy, s.gz, 0, s.phi, x[0] - 0.5, x[1], x[2]),
                             sampleAt(s.gx, s.gy, s.gz, 0, s.phi, x[0], x[1] + 0.5, x[2]) - sampleAt(s.gx, s.gy, s.gz, 0, s.phi, x[0], x[1] - 0.5, x[2]),
                             sampleAt(s.gx, s.gy, s.gz, 0, s.phi, x[0], x[1], x[2] + 0.5) - sampleAt(s.gx, s.gy, s.gz, 0, s.phi, x[0], x[1], x[2] - 0.5)};
        const double m = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
        if (!(m > 1e-12)) {  // (NaN as well)
            found[2] = 1;
            break;
        }
        const double length = sqrt(m), push = s.margin - phi;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            n[c] = g[c] / length;
            x[c] = fmin(fmax(fma(push, n[c], x[c]), 0.0), box[c]);
        }
        pushed = true;
    }
    if (!pushed) return;
    found[0] = 1;
    double us[3] = {0.0, 0.0, 0.0}, r[3];
    if (s.sv[0]) velocityAt(s, s.sv, x, us);
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = double(vf[c]) - us[c];
    const double vn = (r[0] * n[0] + r[1] * n[1]) + r[2] * n[2];
    if (vn < 0.0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            r[c] = r[c] - vn * n[c];
            r[c] = (1.0 - s.friction) * r[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) vf[c] = float(r[c] + us[c]), xf[c] = float(x[c]);
    if (sampleAt(s.gx, s.gy, s.gz, 0, s.phi, double(xf[0]), double(xf[1]), double(xf[2])) < 0.0) found[1] = 1;
}

// the update's arguments with a solid: the fused form
struct UpdateSolidArgs : UpdateArgs {
    SolidArgs solid;
};

// Args: UpdateArgs, or UpdateSolidArgs -- the collision rule then runs on the float32 results before they are stored
template <class Args>
__global__ __launch_bounds__(kFlat) void updateKernel(Args a)
{
    constexpr bool kSolids = std::is_same_v<Args, UpdateSolidArgs>;
    __shared__ unsigned int tally[2];
    __shared__ unsigned int hits[3];
    zeroTally(tally);
    if constexpr (kSolids) zeroTally(hits);
    __syncthreads();
    const long long p = (long long)blockIdx.x * kFlat + int(threadIdx.x);
    unsigned int found[2] = {0, 0};
    [[maybe_unused]] unsigned int hit[3] = {0, 0, 0};
    if (p < a.n) {
        const float xf[3] = {a.pin[0][p], a.pin[1][p], a.pin[2][p]}, vf[3] = {a.vin[0][p], a.vin[1][p], a.vin[2][p]};
        float xo[3] = {xf[0], xf[1], xf[2]}, vo[3] = {vf[0], vf[1], vf[2]};
        if (insideBox(xf[0], xf[1], xf[2], a.gx, a.gy, a.gz)) {
            const double x[3] = {double(xf[0]), double(xf[1]), double(xf[2])}, box[3] = {double(a.gx), double(a.gy), double(a.gz)};
            double pic[3], old[3];
            velocityAt(a, a.gnew, x, pic);
            if (a.gold[0]) velocityAt(a, a.gold, x, old);
            else old[0] = pic[0], old[1] = pic[1], old[2] = pic[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) vo[c] = float((1.0 - a.flip) * pic[c] + a.flip * (double(vf[c]) + (pic[c] - old[c])));
            // section 21's trace under -dt: the product and the sum are one fused multiply-add, as in mgps_advect.hip's departure
            bool clamped = false;
            double u[3] = {pic[0], pic[1], pic[2]};
            if (a.order == 2) {
                double p1[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double q = fma(0.5 * a.dt, pic[c], x[c]);
                    p1[c] = fmin(fmax(q, 0.0), box[c]);
                    clamped |= p1[c] != q;
                }
                velocityAt(a, a.gnew, p1, u);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double q = fma(a.dt, u[c], x[c]);
                const double e = fmin(fmax(q, 0.0), box[c]);
                clamped |= e != q;
                xo[c] = float(e);
            }
            found[0] = clamped;
        } else {
            found[1] = 1;
        }
        if constexpr (kSolids) collideRule(a.solid, xo, vo, hit);
#pragma unroll
        for (int c = 0; c < 3; ++c) a.pout[c][p] = xo[c], a.vout[c][p] = vo[c];
    }
    if (a.counts) addTally(tally, found, a.counts);
    if constexpr (kSolids) {
        if (a.solid.counts) addTally(hits, hit, a.solid.counts);
    }
}

// ---- collision with solids: the standalone pass ------------------------------------------------------------------------------------
struct CollideArgs {
    int n;
    const float *pin[3], *vin[3];
    float *pout[3], *vout[3];
    SolidArgs solid;
};

__global__ __launch_bounds__(kFlat) void collideKernel(CollideArgs a)
{
    __shared__ unsigned int hits[3];
    zeroTally(hits);
    __syncthreads();
    const long long p = (long long)blockIdx.x * kFlat + int(threadIdx.x);
    unsigned int hit[3] = {0, 0, 0};
    if (p < a.n) {
        float x[3] = {a.pin[0][p], a.pin[1][p], a.pin[2][p]}, v[3] = {a.vin[0][p], a.vin[1][p], a.vin[2][p]};
        collideRule(a.solid, x, v, hit);
#pragma unroll
        for (int c = 0; c < 3; ++c) a.pout[c][p] = x[c], a.vout[c][p] = v[c];
    }
    if (a.solid.counts) addTally(hits, hit, a.solid.counts);
}

// ---- resample: thin crowded cells, seed deep ones -----------------------------------------------------------------------------------
struct ResampleArgs {
    int gx, gy, gz, n, cells, capacity, minPer, maxPer, keepOutside;
    uint32_t seed;
    float deepBelow;  // -float(seed_depth dx)
    const float *pos[3], *vel[3];
    const int32_t *cellStart;
    const float *liquidPhi, *solidPhi, *grid[3];
    float *pout[3], *vout[3];
    int32_t *cellStartOut, *nOut;
    unsigned long long *counts;
};

// bin c (a cell, or `cells`: the outside bin): its first slot and its slots m, as slotsOf clamps them, the slots it keeps and the
// particles it is given
struct CellPlan {
    int first, m, kept, seeds;
    bool deep;
};
__device__ __forceinline__ CellPlan planOf(const ResampleArgs &a, int c)
{
    CellPlan p;
    p.first = min(max(a.cellStart[c], 0), a.n);
    p.m = max(min(max(a.cellStart[c + 1], 0), a.n) - p.first, 0);
    p.deep = false, p.seeds = 0;
    if (c == a.cells) {
        p.kept = a.keepOutside ? p.m : 0;
        return p;
    }
    p.kept = min(p.m, a.maxPer);
    p.deep = a.liquidPhi && a.liquidPhi[c] <= a.deepBelow && (!a.solidPhi || a.solidPhi[c] > 0.0f);
    if (p.deep && p.kept < a.minPer) p.seeds = a.minPer - p.kept;
    return p;
}

__global__ __launch_bounds__(kFlat) void resampleCountKernel(ResampleArgs a, int32_t *count)
{
    __shared__ unsigned int tally[3];
    zeroTally(tally);
    __syncthreads();
    const long long c = (long long)blockIdx.x * kFlat + int(threadIdx.x);
    unsigned int found[3] = {0, 0, 0};
    if (c <= a.cells) {
        const CellPlan p = planOf(a, int(c));
        count[c] = p.kept + p.seeds;
        if (c < a.cells) found[0] = unsigned(p.m - p.kept), found[1] = unsigned(p.seeds), found[2] = p.deep;
    } else if (c == (long long)a.cells + 1) {
        count[c] = 0;
    }
    if (a.counts) addTally(tally, found, a.counts);
}

// one thread per input slot (and at least one: thread 0 publishes the total)
__global__ __launch_bounds__(kFlat) void resampleCopyKernel(ResampleArgs a)
{
    const long long s = (long long)blockIdx.x * kFlat + int(threadIdx.x);
    if (s == 0) {
        const int total = a.cellStartOut[a.cells + 1];
        *a.nOut = total;
        if (total > a.capacity && a.counts) atomicAdd(a.counts + 3, 1ull);
    }
    if (s >= a.n) return;
    const float x = a.pos[0][s], y = a.pos[1][s], z = a.pos[2][s];
    int c = a.cells;
    if (insideBox(x, y, z, a.gx, a.gy, a.gz)) {
        const int i = min(int(floorf(x)), a.gx - 1), j = min(int(floorf(y)), a.gy - 1), k = min(int(floorf(z)), a.gz - 1);
        c = (k * a.gy + j) * a.gx + i;
    }
    const CellPlan p = planOf(a, c);
    const long long t = s - p.first;
    if (t < 0 || t >= p.m) return;  // (a wrong cell_start: the slot is not one of its cell's)
    long long rank = t;
    if (c == a.cells) {
        if (!a.keepOutside) return;
    } else if (p.m > a.maxPer) {
        rank = t * a.maxPer / p.m;
        if ((t + 1) * a.maxPer / p.m == rank) return;
    }
    const long long to = (long long)a.cellStartOut[c] + rank;
    if (to < 0 || to >= a.capacity) return;
    a.pout[0][to] = x, a.pout[1][to] = y, a.pout[2][to] = z;
#pragma unroll
    for (int q = 0; q < 3; ++q) a.vout[q][to] = a.vel[q][s];
}

__device__ __forceinline__ uint32_t mix(uint32_t x)
{
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return x;
}

// one thread per (cell, q), q = 0 .. min_per_cell - 1
__global__ __launch_bounds__(kFlat) void resampleSeedKernel(ResampleArgs a)
{
    const long long at = (long long)blockIdx.x * kFlat + int(threadIdx.x);
    if (at >= (long long)a.cells * a.minPer) return;
    const int c = int(at / a.minPer), q = int(at % a.minPer);
    const CellPlan p = planOf(a, c);
    if (q >= p.seeds) return;
    const long long to = (long long)a.cellStartOut[c] + p.kept + q;
    if (to < 0 || to >= a.capacity) return;
    const int cell[3] = {c % a.gx, c / a.gx % a.gy, c / a.gx / a.gy};
    const uint32_t base = mix(mix(a.seed ^ 0x9e3779b9u) + uint32_t(c));
    float xf[3];
    double x[3], u[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const uint32_t h = mix(base + uint32_t(3 * (p.kept + q) + ax));
        const double r = double(h >> 8) * 0x1p-24;
        const float top = __uint_as_float(__float_as_uint(float(cell[ax] + 1)) - 1u);  // the float32 just below i + 1
        xf[ax] = fminf(float(double(cell[ax]) + r), top);
        x[ax] = double(xf[ax]);
    }
    velocityAt(a, a.grid, x, u);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) a.pout[ax][to] = xf[ax], a.vout[ax][to] = float(u[ax]);
}

// ---- what the per-particle entries refuse, stated once ------------------------------------------------------------------------------
// the arrays of component c of a per-particle pass: an output that is exactly its input is one array, written in place; any other
// output overlaps nothing
int particleArrays(const char *fn, ArrayRanges &arrays, int c, int n, const float *pin, const float *vin, float *pout, float *vout)
{
    const size_t bytes = size_t(n) * sizeof(float);
    const float *in[2] = {pin, vin};
    float *out[2] = {pout, vout};
    const char *names[2][2] = {{"position_in", "position_out"}, {"velocity_in", "velocity_out"}};
    for (int q = 0; q < 2; ++q) {
        if (!in[q]) return refuse(fn, indexed(names[q][0], c) + " is NULL");
        if (!out[q]) return refuse(fn, indexed(names[q][1], c) + " is NULL");
        arrays.add(indexed(names[q][0], c), in[q], bytes, in[q] == out[q]);
        if (in[q] != out[q]) arrays.add(indexed(names[q][1], c), out[q], bytes, true);
    }
    return MGPS_OK;
}

// the update desc: refusals, the arrays' ranges, the kernel's arguments
int updateArgs(const char *fn, const mgps_particles_update_desc *d, ArrayRanges &arrays, UpdateArgs &a)
{
    if (!d || d->struct_size != int(sizeof(mgps_particles_update_desc))) return refuse(fn, "NULL or struct_size mismatch (mgps_particles_update_desc)");
    if (int rc = checkParticleGrid(fn, d->gx, d->gy, d->gz, d->n); rc != MGPS_OK) return rc;
    if (d->trace_order != 1 && d->trace_order != 2) return refuse(fn, "trace_order = " + std::to_string(d->trace_order) + " is neither 1 nor 2");
    if (!std::isfinite(d->dt)) return refuse(fn, "dt is not finite");
    if (!(d->flip >= 0.0 && d->flip <= 1.0)) return refuse(fn, "flip is outside [0, 1]");
    int olds = 0;
    if (int rc = allOrNone(fn, reinterpret_cast<const void *const *>(d->grid_old), "grid_old", olds); rc != MGPS_OK) return rc;
    if (olds == 0 && d->flip > 0.0) return refuse(fn, "grid_old is NULL with flip > 0: the FLIP part needs the velocity before forces and projection");
    a.gx = d->gx, a.gy = d->gy, a.gz = d->gz, a.n = d->n, a.order = d->trace_order, a.dt = d->dt, a.flip = d->flip, a.counts = d->counts_dev;
    for (int c = 0; c < 3; ++c) {
        if (!d->grid_new[c]) return refuse(fn, indexed("grid_new", c) + " is NULL");
        const size_t faces = faceElems(d->gx, d->gy, d->gz, c) * sizeof(float);
        arrays.add(indexed("grid_new", c), d->grid_new[c], faces, false);
        if (olds) arrays.add(indexed("grid_old", c), d->grid_old[c], faces, false);
        a.gnew[c] = d->grid_new[c], a.gold[c] = d->grid_old[c];
        if (d->n == 0) continue;
        if (int rc = particleArrays(fn, arrays, c, d->n, d->position_in[c], d->velocity_in[c], d->position_out[c], d->velocity_out[c]); rc != MGPS_OK) return rc;
        a.pin[c] = d->position_in[c], a.vin[c] = d->velocity_in[c], a.pout[c] = d->position_out[c], a.vout[c] = d->velocity_out[c];
    }
    return MGPS_OK;
}

// the collide desc without its particle arrays: refusals, the grids' ranges, the rule's arguments
int solidArgs(const char *fn, const mgps_particles_collide_desc *d, ArrayRanges &arrays, SolidArgs &s)
{
    if (!d || d->struct_size != int(sizeof(mgps_particles_collide_desc))) return refuse(fn, "NULL or struct_size mismatch (mgps_particles_collide_desc)");
    if (int rc = checkParticleGrid(fn, d->gx, d->gy, d->gz, 0); rc != MGPS_OK) return rc;
    if (!(std::isfinite(d->margin) && d->margin >= 0.0)) return refuse(fn, "margin is not finite and >= 0");
    if (d->iterations < 1 || d->iterations > 4) return refuse(fn, "iterations = " + std::to_string(d->iterations) + " is outside 1 .. 4");
    if (!(d->friction >= 0.0 && d->friction <= 1.0)) return refuse(fn, "friction is outside [0, 1]");
    if (!d->solid_phi) return refuse(fn, "solid_phi is NULL");
    int moving = 0;
    if (int rc = allOrNone(fn, reinterpret_cast<const void *const *>(d->solid_velocity), "solid_velocity", moving); rc != MGPS_OK) return rc;
    arrays.add("solid_phi", d->solid_phi, size_t(d->gx) * size_t(d->gy) * size_t(d->gz) * sizeof(float), false);
    for (int c = 0; c < 3 && moving; ++c) arrays.add(indexed("solid_velocity", c), d->solid_velocity[c], faceElems(d->gx, d->gy, d->gz, c) * sizeof(float), false);
    if (d->counts_dev) arrays.add("counts_dev (collide)", d->counts_dev, 3 * sizeof(unsigned long long), true);
    s.gx = d->gx, s.gy = d->gy, s.gz = d->gz, s.iterations = d->iterations, s.margin = d->margin, s.friction = d->friction;
    s.phi = d->solid_phi, s.counts = d->counts_dev;
    for (int c = 0; c < 3; ++c) s.sv[c] = d->solid_velocity[c];
    return MGPS_OK;
}

}  // namespace

extern "C" {

int mgps_particles_bin(const mgps_particles_bin_desc *d, void *stream)
try {
    const char *fn = "mgps_particles_bin";
    if (!d || d->struct_size != int(sizeof(mgps_particles_bin_desc))) return refuse(fn, "NULL or struct_size mismatch (mgps_particles_bin_desc)");
    if (int rc = checkParticleGrid(fn, d->gx, d->gy, d->gz, d->n); rc != MGPS_OK) return rc;
    int vouts = 0;
    if (int rc = allOrNone(fn, reinterpret_cast<const void *const *>(d->velocity_out), "velocity_out", vouts); rc != MGPS_OK) return rc;
    const int cells = d->gx * d->gy * d->gz;
    const size_t bytes = size_t(d->n) * sizeof(float);
    ArrayRanges arrays;
    BinArgs a{};
    a.gx = d->gx, a.gy = d->gy, a.gz = d->gz, a.n = d->n, a.cells = cells, a.counts = d->counts_dev;
    for (int c = 0; c < 3 && d->n > 0; ++c) {
        if (!d->position_in[c]) return refuse(fn, indexed("position_in", c) + " is NULL");
        if (!d->position_out[c]) return refuse(fn, indexed("position_out", c) + " is NULL");
        arrays.add(indexed("position_in", c), d->position_in[c], bytes, false);
        arrays.add(indexed("position_out", c), d->position_out[c], bytes, true);
        a.pin[c] = d->position_in[c], a.pout[c] = d->position_out[c];
        if (vouts == 0) continue;
        if (!d->velocity_in[c]) return refuse(fn, indexed("velocity_in", c) + " is NULL");
        arrays.add(indexed("velocity_in", c), d->velocity_in[c], bytes, false);
        arrays.add(indexed("velocity_out", c), d->velocity_out[c], bytes, true);
        a.vin[c] = d->velocity_in[c], a.vout[c] = d->velocity_out[c];
    }
    if (d->n > 0 && !d->order) return refuse(fn, "order is NULL");
    if (!d->cell_start) return refuse(fn, "cell_start is NULL");
    if (d->n > 0) arrays.add("order", d->order, size_t(d->n) * sizeof(int32_t), true);
    arrays.add("cell_start", d->cell_start, (size_t(cells) + 2) * sizeof(int32_t), true);
    if (int rc = arrays.refuseOverlap(fn); rc != MGPS_OK) return rc;
    a.order = d->order, a.cellStart = d->cell_start;

    const hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = size_t(d->n);
    unsigned endBit = 1;  // exactly the bits that the keys 0 .. cells need
    while (endBit < 31 && (int64_t(1) << endBit) < int64_t(cells) + 1) ++endBit;
    size_t sortBytes = 0;
    if (n > 0) {
        int32_t *none = nullptr;
        if (int rc = hipStatus(fn, rocprim::radix_sort_pairs(nullptr, sortBytes, none, none, none, none, n, 0u, endBit, st)); rc != MGPS_OK) return rc;
    }
    // one block of the stream's pool: the keys, the sorted keys, the input indices, the sort's own storage
    const size_t ints = (n * sizeof(int32_t) + 255) / 256 * 256;
    void *block = nullptr;
    if (int rc = streamAlloc(fn, st, 3 * ints + std::max<size_t>(sortBytes, 256), &block); rc != MGPS_OK) return rc;
    int32_t *key = static_cast<int32_t *>(block), *sorted = key + ints / sizeof(int32_t), *index = sorted + ints / sizeof(int32_t);
    void *sortTemp = index + ints / sizeof(int32_t);
    int rc = MGPS_OK;
    if (n > 0) {
        binKeyKernel<<<flatBlocks(n), kFlat, 0, st>>>(a, key, index);
        rc = hipStatus(fn, hipGetLastError());
        if (rc == MGPS_OK) rc = hipStatus(fn, rocprim::radix_sort_pairs(sortTemp, sortBytes, key, sorted, index, a.order, n, 0u, endBit, st));
    }
    if (rc == MGPS_OK) {
        binStartKernel<<<flatBlocks(size_t(cells) + 2), kFlat, 0, st>>>(a, sorted);
        rc = hipStatus(fn, hipGetLastError());
    }
    if (rc == MGPS_OK && n > 0) {
        binGatherKernel<<<flatBlocks(n), kFlat, 0, st>>>(a);
        rc = hipStatus(fn, hipGetLastError());
    }
    const int freed = hipStatus(fn, hipFreeAsync(block, st));
    return rc != MGPS_OK ? rc : freed;
}
MGPS_API_CATCH(nullptr)

int mgps_particles_to_grid(const mgps_particles_to_grid_desc *d, void *stream)
try {
    const char *fn = "mgps_particles_to_grid";
    if (!d || d->struct_size != int(sizeof(mgps_particles_to_grid_desc))) return refuse(fn, "NULL or struct_size mismatch (mgps_particles_to_grid_desc)");
    if (int rc = checkTileExtents(fn, d->gx, d->gy, d->gz, false); rc != MGPS_OK) return rc;
    if (int rc = checkParticleGrid(fn, d->gx, d->gy, d->gz, d->n); rc != MGPS_OK) return rc;
    if (d->form < 0 || d->form > 2) return refuse(fn, "form = " + std::to_string(d->form) + " is outside 0 .. 2");
    if (!(d->radius > 0.0 && d->radius <= 1.5)) return refuse(fn, "radius is outside (0, 1.5] cells");
    if (!(std::isfinite(d->dx) && d->dx > 0.0)) return refuse(fn, "dx is not finite and > 0");
    int wouts = 0;
    if (int rc = allOrNone(fn, reinterpret_cast<const void *const *>(d->weight_out), "weight_out", wouts); rc != MGPS_OK) return rc;
    const size_t cells = size_t(d->gx) * size_t(d->gy) * size_t(d->gz), bytes = size_t(d->n) * sizeof(float);
    ArrayRanges arrays;
    ToGridArgs a{};
    a.gx = d->gx, a.gy = d->gy, a.planes = d->gz, a.n = d->n, a.radius = d->radius, a.dx = d->dx, a.counts = d->counts_dev;
    for (int c = 0; c < 3; ++c) {
        if (d->n > 0) {
            if (!d->position[c]) return refuse(fn, indexed("position", c) + " is NULL");
            if (!d->velocity[c]) return refuse(fn, indexed("velocity", c) + " is NULL");
            arrays.add(indexed("position", c), d->position[c], bytes, false);
            arrays.add(indexed("velocity", c), d->velocity[c], bytes, false);
        }
        if (!d->velocity_out[c]) return refuse(fn, indexed("velocity_out", c) + " is NULL");
        if (!d->known_out[c]) return refuse(fn, indexed("known_out", c) + " is NULL");
        const size_t faces = faceElems(d->gx, d->gy, d->gz, c);
        arrays.add(indexed("velocity_out", c), d->velocity_out[c], faces * sizeof(float), true);
        arrays.add(indexed("known_out", c), d->known_out[c], faces, true);
        if (wouts) arrays.add(indexed("weight_out", c), d->weight_out[c], faces * sizeof(float), true);
        a.pos[c] = d->position[c], a.vel[c] = d->velocity[c], a.vout[c] = d->velocity_out[c], a.wout[c] = d->weight_out[c], a.known[c] = d->known_out[c];
    }
    if (!d->cell_start) return refuse(fn, "cell_start is NULL");
    arrays.add("cell_start", d->cell_start, (cells + 2) * sizeof(int32_t), false);
    if (d->liquid_phi_out) arrays.add("liquid_phi_out", d->liquid_phi_out, cells * sizeof(float), true);
    if (int rc = arrays.refuseOverlap(fn); rc != MGPS_OK) return rc;
    a.cellStart = d->cell_start, a.phi = d->liquid_phi_out;
    if (d->form == 1) toGridKernel<<<tileGrid(d->gx, d->gy, d->gz), kThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    else toGridStagedKernel<<<tileGrid(d->gx, d->gy, d->gz), kThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    return hipStatus(fn, hipGetLastError());
}
MGPS_API_CATCH(nullptr)

int mgps_particles_update(const mgps_particles_update_desc *d, void *stream)
try {
    const char *fn = "mgps_particles_update";
    ArrayRanges arrays;
    UpdateArgs a{};
    if (int rc = updateArgs(fn, d, arrays, a); rc != MGPS_OK) return rc;
    if (int rc = arrays.refuseOverlap(fn); rc != MGPS_OK) return rc;
    if (d->n == 0) return MGPS_OK;
    updateKernel<<<flatBlocks(size_t(d->n)), kFlat, 0, static_cast<hipStream_t>(stream)>>>(a);
    return hipStatus(fn, hipGetLastError());
}
MGPS_API_CATCH(nullptr)

int mgps_particles_collide(const mgps_particles_collide_desc *d, void *stream)
try {
    const char *fn = "mgps_particles_collide";
    ArrayRanges arrays;
    CollideArgs a{};
    if (int rc = solidArgs(fn, d, arrays, a.solid); rc != MGPS_OK) return rc;
    if (d->n < 0) return refuse(fn, "n = " + std::to_string(d->n) + " is negative");
    a.n = d->n;
    for (int c = 0; c < 3 && d->n > 0; ++c) {
        if (int rc = particleArrays(fn, arrays, c, d->n, d->position_in[c], d->velocity_in[c], d->position_out[c], d->velocity_out[c]); rc != MGPS_OK) return rc;
        a.pin[c] = d->position_in[c], a.vin[c] = d->velocity_in[c], a.pout[c] = d->position_out[c], a.vout[c] = d->velocity_out[c];
    }
    if (int rc = arrays.refuseOverlap(fn); rc != MGPS_OK) return rc;
    if (d->n == 0) return MGPS_OK;
    collideKernel<<<flatBlocks(size_t(d->n)), kFlat, 0, static_cast<hipStream_t>(stream)>>>(a);
    return hipStatus(fn, hipGetLastError());
}
MGPS_API_CATCH(nullptr)

int mgps_particles_update_solid(const mgps_particles_update_desc *d, const mgps_particles_collide_desc *solid, void *stream)
try {
    const char *fn = "mgps_particles_update_solid";
    ArrayRanges arrays;
    UpdateSolidArgs a{};
    if (int rc = updateArgs(fn, d, arrays, a); rc != MGPS_OK) return rc;
    if (int rc = solidArgs(fn, solid, arrays, a.solid); rc != MGPS_OK) return rc;
    if (solid->gx != d->gx || solid->gy != d->gy || solid->gz != d->gz) return refuse(fn, "the two descs are not of one grid (gx, gy, gz differ)");
    if (int rc = arrays.refuseOverlap(fn); rc != MGPS_OK) return rc;
    if (d->n == 0) return MGPS_OK;
    updateKernel<<<flatBlocks(size_t(d->n)), kFlat, 0, static_cast<hipStream_t>(stream)>>>(a);
    return hipStatus(fn, hipGetLastError());
}
MGPS_API_CATCH(nullptr)

int mgps_particles_resample(const mgps_particles_resample_desc *d, void *stream)
try {
    const char *fn = "mgps_particles_resample";
    if (!d || d->struct_size != int(sizeof(mgps_particles_resample_desc))) return refuse(fn, "NULL or struct_size mismatch (mgps_particles_resample_desc)");
    if (int rc = checkParticleGrid(fn, d->gx, d->gy, d->gz, d->n); rc != MGPS_OK) return rc;
    if (d->capacity < 0) return refuse(fn, "capacity = " + std::to_string(d->capacity) + " is negative");
    if (d->max_per_cell < 1 || d->max_per_cell > 64) return refuse(fn, "max_per_cell = " + std::to_string(d->max_per_cell) + " is outside 1 .. 64");
    if (d->min_per_cell < 0 || d->min_per_cell > d->max_per_cell)
        return refuse(fn, "min_per_cell = " + std::to_string(d->min_per_cell) + " is outside 0 .. max_per_cell");
    if (d->keep_outside != 0 && d->keep_outside != 1) return refuse(fn, "keep_outside = " + std::to_string(d->keep_outside) + " is neither 0 nor 1");
    if (!(std::isfinite(d->dx) && d->dx > 0.0)) return refuse(fn, "dx is not finite and > 0");
    if (!(std::isfinite(d->seed_depth) && d->seed_depth >= 0.0)) return refuse(fn, "seed_depth is not finite and >= 0");
    const long long cells = (long long)d->gx * d->gy * d->gz;
    if (d->n + cells * d->min_per_cell >= (1LL << 31)) return refuse(fn, "the total can pass int32: n + gx gy gz min_per_cell must be < 2^31");
    int grids = 0;
    if (int rc = allOrNone(fn, reinterpret_cast<const void *const *>(d->grid), "grid", grids); rc != MGPS_OK) return rc;
    if (d->min_per_cell > 0 && !d->liquid_phi) return refuse(fn, "liquid_phi is NULL with min_per_cell > 0: seeding needs the deep cells");
    if (d->min_per_cell > 0 && grids == 0) return refuse(fn, "grid is NULL with min_per_cell > 0: seeded particles take their velocity from it");
    const size_t bytes = size_t(d->n) * sizeof(float), outBytes = size_t(d->capacity) * sizeof(float);
    ArrayRanges arrays;
    ResampleArgs a{};
    a.gx = d->gx, a.gy = d->gy, a.gz = d->gz, a.n = d->n, a.cells = int(cells), a.capacity = d->capacity, a.minPer = d->min_per_cell;
    a.maxPer = d->max_per_cell, a.keepOutside = d->keep_outside, a.seed = d->seed, a.deepBelow = -float(d->seed_depth * d->dx), a.counts = d->counts_dev;
    for (int c = 0; c < 3; ++c) {
        if (d->n > 0) {
            if (!d->position[c]) return refuse(fn, indexed("position", c) + " is NULL");
            if (!d->velocity[c]) return refuse(fn, indexed("velocity", c) + " is NULL");
            arrays.add(indexed("position", c), d->position[c], bytes, false);
            arrays.add(indexed("velocity", c), d->velocity[c], bytes, false);
        }
        if (d->capacity > 0) {
            if (!d->position_out[c]) return refuse(fn, indexed("position_out", c) + " is NULL");
            if (!d->velocity_out[c]) return refuse(fn, indexed("velocity_out", c) + " is NULL");
            arrays.add(indexed("position_out", c), d->position_out[c], outBytes, true);
            arrays.add(indexed("velocity_out", c), d->velocity_out[c], outBytes, true);
        }
        if (grids) arrays.add(indexed("grid", c), d->grid[c], faceElems(d->gx, d->gy, d->gz, c) * sizeof(float), false);
        a.pos[c] = d->position[c], a.vel[c] = d->velocity[c], a.pout[c] = d->position_out[c], a.vout[c] = d->velocity_out[c], a.grid[c] = d->grid[c];
    }
    if (!d->cell_start) return refuse(fn, "cell_start is NULL");
    if (!d->cell_start_out) return refuse(fn, "cell_start_out is NULL");
    if (!d->n_out_dev) return refuse(fn, "n_out_dev is NULL");
    arrays.add("cell_start", d->cell_start, (size_t(cells) + 2) * sizeof(int32_t), false);
    arrays.add("cell_start_out", d->cell_start_out, (size_t(cells) + 2) * sizeof(int32_t), true);
    arrays.add("n_out_dev", d->n_out_dev, sizeof(int32_t), true);
    if (d->liquid_phi) arrays.add("liquid_phi", d->liquid_phi, size_t(cells) * sizeof(float), false);
    if (d->solid_phi) arrays.add("solid_phi", d->solid_phi, size_t(cells) * sizeof(float), false);
    if (d->counts_dev) arrays.add("counts_dev", d->counts_dev, 4 * sizeof(unsigned long long), true);
    if (int rc = arrays.refuseOverlap(fn); rc != MGPS_OK) return rc;
    a.cellStart = d->cell_start, a.cellStartOut = d->cell_start_out, a.nOut = d->n_out_dev, a.liquidPhi = d->liquid_phi, a.solidPhi = d->solid_phi;

    const hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t bins = size_t(cells) + 2;
    size_t scanBytes = 0;
    int32_t *none = nullptr;
    if (int rc = hipStatus(fn, rocprim::exclusive_scan(nullptr, scanBytes, none, none, int32_t(0), bins, rocprim::plus<int32_t>(), st)); rc != MGPS_OK) return rc;
    // one block of the stream's pool: the bins' counts and the scan's own storage
    const size_t ints = (bins * sizeof(int32_t) + 255) / 256 * 256;
    void *block = nullptr;
    if (int rc = streamAlloc(fn, st, ints + std::max<size_t>(scanBytes, 256), &block); rc != MGPS_OK) return rc;
    int32_t *count = static_cast<int32_t *>(block);
    void *scanTemp = count + ints / sizeof(int32_t);
    resampleCountKernel<<<flatBlocks(bins), kFlat, 0, st>>>(a, count);
    int rc = hipStatus(fn, hipGetLastError());
    if (rc == MGPS_OK) rc = hipStatus(fn, rocprim::exclusive_scan(scanTemp, scanBytes, count, a.cellStartOut, int32_t(0), bins, rocprim::plus<int32_t>(), st));
    if (rc == MGPS_OK) {
        resampleCopyKernel<<<flatBlocks(std::max<size_t>(size_t(d->n), 1)), kFlat, 0, st>>>(a);
        rc = hipStatus(fn, hipGetLastError());
    }
    if (rc == MGPS_OK && d->min_per_cell > 0) {
        resampleSeedKernel<<<flatBlocks(size_t(cells) * size_t(d->min_per_cell)), kFlat, 0, st>>>(a);
        rc = hipStatus(fn, hipGetLastError());
    }
    const int freed = hipStatus(fn, hipFreeAsync(block, st));
    return rc != MGPS_OK ? rc : freed;
}
MGPS_API_CATCH(nullptr)
}
