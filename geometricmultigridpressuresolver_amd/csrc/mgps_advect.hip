// Advection on the device (include/mgps_fields.h, "advection"): semi-Lagrangian and MacCormack passes over the three
// face grids of the velocity and up to four cell grids, on a whole grid or a slab window.
// One launch over the tiles of mgps_tile_pass.h, two under MacCormack.  A thread owns its cell's scalars and the
// backward face of its cell per axis, and the forward face where the box ends (CellFaces' ownership).  The first velocity sample of a
// trace, U(x), sits at a fixed offset from the thread's cell: the workgroup stages its tile of the three components with a rim in LDS and
// every U(x) is read from there.  The midpoint and departure samples depend on the data and go to global memory.
// Every rule is stated once: latticeOf (where a grid's nodes are and which planes are held), stencilAt (section 20's interpolant: indices
// and weights), combine (the eight values, their least and greatest) -- these in mgps_sample.h, which the particle update shares --,
// departure (the trace).  Both launches and both forms inline the
// same functions, with explicit fused multiply-adds where a product feeds a sum, so a departure point has the same bits wherever it is
// formed again.
#include <cmath>

#include "mgps_sample.h"
#include "mgps_tile_pass.h"

using namespace mgps;

namespace {

// the staged box: the tile's nodes and one node below and above per axis; along z one more above, which the z-face lattice asks for
// (with weight 0) at the forward face of a window that ends inside the grid
constexpr int kSX = kTX + 2, kSY = kTY + 2, kSZ = kTZ + 3, kStage = kSX * kSY * kSZ;
constexpr int kGrids = 7;  // vx, vy, vz, then four scalars

struct AdvectArgs {
    int gx, gy, gz;    // the whole grid
    int c0, planes;    // the window's base planes [c0, c0 + planes); the whole grid: 0, gz
    int below, above;  // halo planes held on either side
    int order, scalars, faces;  // trace order; scalar grids; 1 = the velocity is advected too
    double dt;
    HeldPlanes in[kGrids];
    const float *hat[kGrids];  // second launch: the semi-Lagrangian result of the first
    float *out[kGrids];
    unsigned long long *counts;
};

__device__ __forceinline__ Lattice latticeOf(const AdvectArgs &a, int kind)
{
    return mgps::latticeOf(a.gx, a.gy, a.gz, a.c0, a.planes, a.below, a.above, kind);
}

// the staged box of one component: node (x, y, z) of the whole grid's index lives at (x - xb, y - yb, z - zb)
struct Staged {
    const float *at;
    int xb, yb, zb;
};

__device__ __forceinline__ double sampleStaged(const Staged &g, const Stencil &s)
{
    const int z0 = (s.i0[2] - g.zb) * kSY, z1 = (s.i1[2] - g.zb) * kSY;
    const int r00 = (z0 + s.i0[1] - g.yb) * kSX - g.xb, r10 = (z0 + s.i1[1] - g.yb) * kSX - g.xb;
    const int r01 = (z1 + s.i0[1] - g.yb) * kSX - g.xb, r11 = (z1 + s.i1[1] - g.yb) * kSX - g.xb;
    const float v[8] = {g.at[r00 + s.i0[0]], g.at[r00 + s.i1[0]], g.at[r10 + s.i0[0]], g.at[r10 + s.i1[0]],
                        g.at[r01 + s.i0[0]], g.at[r01 + s.i1[0]], g.at[r11 + s.i0[0]], g.at[r11 + s.i1[0]]};
    double lo, hi;
    return combine(s, v, lo, hi);
}

// U(p) from global memory
__device__ __forceinline__ void velocityAt(const AdvectArgs &a, const double p[3], double u[3], bool &missed)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const Lattice L = latticeOf(a, c + 1);
        const Stencil s = stencilAt(L, p[0], p[1], p[2]);
        missed |= s.missed;
        double lo, hi;
        u[c] = sampleHeld(a.in[c], L, s, lo, hi);
    }
}

// The departure point of x under the step dt (the forward point: -dt), given u0 = U(x).  clamped: a clamp into the box moved a coordinate
__device__ __forceinline__ void departure(const AdvectArgs &a, const double x[3], const double u0[3], double dt, double p[3], bool &clamped,
                                          bool &missed)
{
    const double box[3] = {double(a.gx), double(a.gy), double(a.gz)};
    double u[3] = {u0[0], u0[1], u0[2]};
    if (a.order == 2) {
        double p1[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double q = fma(-(0.5 * dt), u0[c], x[c]);
            p1[c] = fmin(fmax(q, 0.0), box[c]);
            clamped |= p1[c] != q;
        }
        velocityAt(a, p1, u, missed);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double q = fma(-dt, u[c], x[c]);
        p[c] = fmin(fmax(q, 0.0), box[c]);
        clamped |= p[c] != q;
    }
}

// PASS 0: out = the semi-Lagrangian value (under MacCormack `out` is the scratch).  PASS 1: the MacCormack correction from in and hat
template <int PASS>
__global__ __launch_bounds__(kThreads) void advectKernel(AdvectArgs a)
{
    __shared__ float stage[3][kStage];
    __shared__ unsigned int tally[2];

    // TileThread's mapping (mgps_tile_pass.h), restated: through the struct the staging loops cost 20 instructions more (LABNOTES R14)
    const int t = int(threadIdx.x), lane = t & 63, wave = t >> 6;
    const int ti0 = int(blockIdx.x) * kTX, tj0 = int(blockIdx.y) * kTY, k0 = int(blockIdx.z) * kTZ;
    const int kg0 = k0 + a.c0;
    zeroTally(tally);

    // the three components' nodes around the tile; a node outside the grid or outside the held planes is the nearest one inside
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const Lattice L = latticeOf(a, c + 1);
        for (int n = t; n < kStage; n += kThreads) {
            const int lx = n % kSX, ly = (n / kSX) % kSY, lz = n / (kSX * kSY);
            const int x = min(max(ti0 - 1 + lx, 0), L.n[0] - 1), y = min(max(tj0 - 1 + ly, 0), L.n[1] - 1);
            const int z = min(max(min(max(kg0 - 1 + lz, 0), L.n[2] - 1), L.h0), L.h1 - 1);
            stage[c][n] = planeOf(a.in[c], L, z)[size_t(y) * size_t(L.n[0]) + x];
        }
    }
    __syncthreads();

    const int i = ti0 + lane, j = tj0 + wave;
    unsigned int nClamped = 0, nMissed = 0;
    if (i < a.gx && j < a.gy) {
        for (int kk = 0; kk < kTZ; ++kk) {
            const int k = k0 + kk;
            if (k >= a.planes) break;
            for (int kind = 0; kind <= (a.faces ? 3 : 0); ++kind) {
                const int first = kind == 0 ? 3 : kind - 1, grids = kind == 0 ? a.scalars : 1;
                if (grids == 0) continue;
                const Lattice L = latticeOf(a, kind);
                // CellFaces' rule, restated: indexing its arrays by a run-time `kind` cost 7 and 11 VGPRs and 72 B of scratch (R14)
                const int more = kind == 1 ? i == a.gx - 1 : kind == 2 ? j == a.gy - 1 : kind == 3 ? k == a.planes - 1 : 0;
                for (int side = 0; side <= more; ++side) {
                    const int fi = i + (kind == 1 ? side : 0), fj = j + (kind == 2 ? side : 0), fk = k + (kind == 3 ? side : 0);
                    const size_t at = (size_t(fk) * size_t(L.n[1]) + size_t(fj)) * size_t(L.n[0]) + size_t(fi);
                    const double x[3] = {kind == 1 ? double(fi) : double(fi) + 0.5, kind == 2 ? double(fj) : double(fj) + 0.5,
                                         kind == 3 ? double(fk + a.c0) : double(fk + a.c0) + 0.5};
                    bool clamped = false, missed = false;
                    double u0[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const Stencil s = stencilAt(latticeOf(a, c + 1), x[0], x[1], x[2]);
                        missed |= s.missed;
                        u0[c] = sampleStaged(Staged{stage[c], ti0 - 1, tj0 - 1, kg0 - 1}, s);
                    }
                    double p[3];
                    departure(a, x, u0, a.dt, p, clamped, missed);
                    const Stencil s = stencilAt(L, p[0], p[1], p[2]);
                    missed |= s.missed;
                    if (PASS == 0) {
                        for (int g = 0; g < grids; ++g) {
                            double lo, hi;
                            put(a.out[first + g] + at, float(sampleHeld(a.in[first + g], L, s, lo, hi)));
                        }
                        // of the z-faces the planes c0 .. c1 - 1 count, and plane gz: a sum over the ranks counts every target once
                        if (kind != 3 || side == 0 || a.c0 + a.planes == a.gz) {
                            nClamped += clamped ? grids : 0;
                            nMissed += missed ? grids : 0;
                        }
                    } else {
                        double pf[3];
                        bool unused = false;
                        departure(a, x, u0, -a.dt, pf, unused, unused);
                        const Stencil sf = stencilAt(L, pf[0], pf[1], pf[2]);
                        for (int g = 0; g < grids; ++g) {
                            double lo, hi, lo2, hi2;
                            (void)sampleHeld(a.in[first + g], L, s, lo, hi);
                            const double back = sampleHeld(HeldPlanes{a.hat[first + g], nullptr, nullptr}, L, sf, lo2, hi2);
                            const double m = fma(0.5, double(a.in[first + g].win[at]) - back, double(a.hat[first + g][at]));
                            put(a.out[first + g] + at, float(fmin(fmax(m, lo), hi)));
                        }
                    }
                }
            }
        }
    }
    if (PASS == 0 && a.counts) {
        const unsigned int found[2] = {nClamped, nMissed};
        addTally(tally, found, a.counts);
    }
}

// What both entries refuse of a desc, before any device work; [c0, c0 + planes) with the halo planes held is the box of the arrays.
// Fills the kernel's arguments
int checkDesc(const char *fn, const mgps_advect_desc *d, int c0, int planes, int below, int above, const float *const vlo[3],
              const float *const vhi[3], const float *const slo[4], const float *const shi[4], AdvectArgs &a)
{
    if (!d || d->struct_size != int(sizeof(mgps_advect_desc))) return refuse(fn, "NULL or struct_size mismatch (mgps_advect_desc)");
    if (int rc = checkTileExtents(fn, d->gx, d->gy, d->gz, false); rc != MGPS_OK) return rc;
    if (d->scheme != 0 && d->scheme != 1) return refuse(fn, "scheme = " + std::to_string(d->scheme) + " is neither 0 (semi-Lagrangian) nor 1 (MacCormack)");
    if (d->trace_order != 1 && d->trace_order != 2) return refuse(fn, "trace_order = " + std::to_string(d->trace_order) + " is neither 1 nor 2");
    if (!std::isfinite(d->dt)) return refuse(fn, "dt is not finite");
    if (d->scalars < 0 || d->scalars > 4) return refuse(fn, "scalars = " + std::to_string(d->scalars) + " is outside 0 .. 4");
    const int outs = (d->velocity_out[0] != nullptr) + (d->velocity_out[1] != nullptr) + (d->velocity_out[2] != nullptr);
    if (outs != 0 && outs != 3) return refuse(fn, "velocity_out: all three grids, or none (scalars only)");
    if (outs == 0 && d->scalars == 0) return refuse(fn, "nothing to advect: velocity_out is NULL and scalars = 0");

    const size_t gx = size_t(d->gx), gy = size_t(d->gy), pl = size_t(planes);
    const size_t plane[4] = {gx * gy, (gx + 1) * gy, gx * (gy + 1), gx * gy};  // by grid kind
    const size_t held[4] = {pl, pl, pl, pl + 1};
    ArrayRanges arrays;
    const auto add = [&](const void *p, int kind, bool written, const std::string &name) {
        arrays.add(name, p, plane[kind] * held[kind] * sizeof(float), written);
    };
    const auto addHalo = [&](const void *p, int kind, int count, const std::string &name) {
        arrays.add(name, p, plane[kind] * size_t(count) * sizeof(float), false);
    };
    a = AdvectArgs{};
    a.gx = d->gx, a.gy = d->gy, a.gz = d->gz, a.c0 = c0, a.planes = planes, a.below = below, a.above = above;
    a.order = d->trace_order, a.scalars = d->scalars, a.faces = outs == 3, a.dt = d->dt, a.counts = d->counts_dev;
    for (int g = 0; g < 3 + d->scalars; ++g) {
        const bool face = g < 3;
        const int q = face ? g : g - 3, kind = face ? g + 1 : 0;
        const std::string idx = "[" + std::to_string(q) + "]", base = face ? "velocity" : "scalar";
        const float *in = face ? d->velocity_in[q] : d->scalar_in[q];
        float *out = face ? d->velocity_out[q] : d->scalar_out[q];
        float *scratch = face ? d->velocity_scratch[q] : d->scalar_scratch[q];
        const float *lo = face ? (vlo ? vlo[q] : nullptr) : (slo ? slo[q] : nullptr);
        const float *hi = face ? (vhi ? vhi[q] : nullptr) : (shi ? shi[q] : nullptr);
        if (!in) return refuse(fn, base + "_in" + idx + " is NULL");
        add(in, kind, false, base + "_in" + idx);
        if (int rc = checkHaloArrays(fn, base + "_lo" + idx, lo, below, base + "_hi" + idx, hi, above); rc != MGPS_OK) return rc;
        if (below > 0) addHalo(lo, kind, below, base + "_lo" + idx);
        if (above > 0) addHalo(hi, kind, above, base + "_hi" + idx);
        a.in[g] = HeldPlanes{in, below > 0 ? lo : nullptr, above > 0 ? hi : nullptr};
        if (face && outs == 0) continue;
        if (!out) return refuse(fn, base + "_out" + idx + " is NULL");
        add(out, kind, true, base + "_out" + idx);
        if (d->scheme == 1) {
            if (!scratch) return refuse(fn, base + "_scratch" + idx + " is NULL: MacCormack needs scratch grids of the outputs' shapes");
            add(scratch, kind, true, base + "_scratch" + idx);
        }
        a.out[g] = out, a.hat[g] = scratch;
    }
    return arrays.refuseOverlap(fn);  // (out and scratch are written)
}

// one launch for the semi-Lagrangian scheme, two under MacCormack: the first fills the scratch grids, the second corrects and limits
int runAdvect(const char *fn, const AdvectArgs &args, int scheme, hipStream_t st)
{
    const dim3 grid = tileGrid(args.gx, args.gy, args.planes);
    AdvectArgs first = args;
    if (scheme == 1)
        for (int g = 0; g < kGrids; ++g) first.out[g] = const_cast<float *>(args.hat[g]);
    advectKernel<0><<<grid, kThreads, 0, st>>>(first);
    if (int rc = hipStatus(fn, hipGetLastError()); rc != MGPS_OK || scheme == 0) return rc;
    advectKernel<1><<<grid, kThreads, 0, st>>>(args);
    return hipStatus(fn, hipGetLastError());
}
}  // namespace

extern "C" {

int mgps_fields_advect(const mgps_advect_desc *d, void *stream)
try {
    const char *fn = "mgps_fields_advect";
    AdvectArgs a;
    if (int rc = checkDesc(fn, d, 0, d ? d->gz : 0, 0, 0, nullptr, nullptr, nullptr, nullptr, a); rc != MGPS_OK) return rc;
    return runAdvect(fn, a, d->scheme, static_cast<hipStream_t>(stream));
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_advect(const mgps_fields_slab *w, const mgps_advect_desc *d, int halo, const float *const velocity_lo[3],
                            const float *const velocity_hi[3], const float *const scalar_lo[4], const float *const scalar_hi[4], void *stream)
try {
    const char *fn = "mgps_fields_slab_advect";
    int below = 0, above = 0;
    if (int rc = checkWindowOf(fn, w, d, halo, below, above); rc != MGPS_OK) return rc;
    if (d && d->struct_size == int(sizeof(mgps_advect_desc)) && d->scheme == 1)
        return refuse(fn, "scheme = 1 (MacCormack) on a window needs the semi-Lagrangian result on the halo planes too: the window form takes "
                          "scheme = 0 only");
    AdvectArgs a;
    if (int rc = checkDesc(fn, d, w->c0, w->c1 - w->c0, below, above, velocity_lo, velocity_hi, scalar_lo, scalar_hi, a); rc != MGPS_OK) return rc;
    return runAdvect(fn, a, 0, static_cast<hipStream_t>(stream));
}
MGPS_API_CATCH(nullptr)
}
