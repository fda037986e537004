// Redistancing on the device (include/mgps_fields.h, "redistancing"): a fast iterative Eikonal pass that turns
// liquid_phi back into a signed distance within a band, on a whole grid or a slab window.
// The state of a cell is the float32 value s T: T >= 0 the distance in cells, s = - where phi <= 0.  One streaming launch fixes the
// interface cells (initKernel); every round is one launch of block Jacobi over the tiles of mgps_tile_pass.h, anchored
// at cell (0, 0, 0) of the whole grid (roundKernel): the tile and a one-cell rim are staged in LDS once, a thread owns a z-column of
// four cells in registers and reads its x/y neighbours from LDS, the rim is held, and `inner` Jacobi iterations of the first-order
// Godunov update run before the tile's cells are stored.  Whether a cell is an interface cell is the sign test on the staged box.
// All arithmetic is fp64 on float32 data and every operation is rounded on its own -- no contraction in this unit -- so that
// tests/redistance_reference.py, which states the same operations in numpy, has the same bits.
#include <cmath>

#include "mgps_tile_pass.h"

#pragma clang fp contract(off)

using namespace mgps;

namespace {

constexpr int kSX = kTX + 2, kSY = kTY + 2, kSZ = kTZ + 2, kBox = kSX * kSY * kSZ;  // the tile and a one-cell rim

struct RedistanceArgs {
    int gx, gy, gz;    // the whole grid
    int c0, planes;    // the window's planes [c0, c0 + planes); the whole grid: 0, gz
    int below, above;  // halo planes held on either side
    int inner;
    int scale;  // 1: the stores are float(dx state)
    int count;  // 1: the round adds the own cells it changed to counts[1]
    double B, dx;
    HeldPlanes in;
    float *out;
    unsigned long long *counts;
};

// the plane z (held) of the input, z in the whole grid's plane index
__device__ __forceinline__ const float *planeOf(const RedistanceArgs &a, int z)
{
    return heldPlane(a.in, size_t(a.gx) * size_t(a.gy), a.c0, a.c0 + a.planes, a.c0 - a.below, z);
}

__device__ __forceinline__ float stored(const RedistanceArgs &a, float state)
{
    return a.scale ? float(a.dx * double(state)) : state;
}

// The initial pass: T0 of every own cell from phi's seven-point neighbourhood.  A streaming kernel over tiles of the window's planes
__global__ __launch_bounds__(kThreads) void initKernel(RedistanceArgs a)
{
    __shared__ unsigned int tally[1];
    const TileThread th;
    const int i = th.i, j = th.j, k0 = th.k0;
    zeroTally(tally);
    __syncthreads();
    unsigned int interfaces = 0;
    if (i < a.gx && j < a.gy) {
        const size_t row = size_t(j) * size_t(a.gx) + size_t(i);
        for (int kk = 0; kk < kTZ; ++kk) {
            const int k = k0 + kk;
            if (k >= a.planes) break;
            const int z = a.c0 + k;
            const float *here = planeOf(a, z);
            const float phi = here[row];
            const double p = double(phi);
            const bool inside = phi <= 0.0f;
            // per axis: is there a neighbour below / above, and its value
            const bool has[3][2] = {{i > 0, i + 1 < a.gx}, {j > 0, j + 1 < a.gy}, {z > 0, z + 1 < a.gz}};
            double n[3][2];
            n[0][0] = has[0][0] ? double(here[row - 1]) : 0.0;
            n[0][1] = has[0][1] ? double(here[row + 1]) : 0.0;
            n[1][0] = has[1][0] ? double(here[row - size_t(a.gx)]) : 0.0;
            n[1][1] = has[1][1] ? double(here[row + size_t(a.gx)]) : 0.0;
            n[2][0] = has[2][0] ? double(planeOf(a, z - 1)[row]) : 0.0;
            n[2][1] = has[2][1] ? double(planeOf(a, z + 1)[row]) : 0.0;
            bool iface = false;
            double cross = INFINITY, g[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    if (has[c][s] && (n[c][s] <= 0.0) != inside) {
                        iface = true;
                        cross = fmin(cross, p / (p - n[c][s]));
                    }
                g[c] = has[c][0] && has[c][1] ? 0.5 * (n[c][1] - n[c][0]) : has[c][1] ? n[c][1] - p : has[c][0] ? p - n[c][0] : 0.0;
            }
            double T = a.B;
            if (iface) {
                const double g2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
                const double grad = g2 > 0.0 ? fabs(p) / sqrt(g2) : INFINITY;
                T = fmin(fmin(grad, cross), a.B);
                ++interfaces;
            }
            const float state = copysignf(float(fabs(T)), inside ? -1.0f : 1.0f);
            a.out[size_t(k) * size_t(a.gx) * size_t(a.gy) + row] = stored(a, state);
        }
    }
    const unsigned int found[1] = {interfaces};
    if (a.counts) addTally(tally, found, a.counts);
}

// G: the first-order Godunov update of a cell from the least T of its two neighbours per axis (+inf outside the whole grid)
__device__ __forceinline__ double godunov(float fx, float fy, float fz)
{
    const double x = double(fx), y = double(fy), z = double(fz);
    const double lo = fmin(x, y), hi = fmax(x, y);
    const double a1 = fmin(lo, z), a2 = fmax(lo, fmin(hi, z)), a3 = fmax(hi, z);
    double t = a1 + 1.0;
    if (t > a2) {
        const double d = a1 - a2;
        t = 0.5 * ((a1 + a2) + sqrt(2.0 - d * d));
    }
    if (t > a3) {
        const double s = (a1 + a2) + a3, q = (a1 * a1 + a2 * a2) + a3 * a3;
        const double disc = fmax(s * s - 3.0 * (q - 1.0), 0.0);
        t = (s + sqrt(disc)) / 3.0;
    }
    return t;
}

__device__ __forceinline__ int boxAt(int lx, int ly, int lz)
{
    return (lz * kSY + ly) * kSX + lx;
}

// One round.  blockIdx.z counts the whole grid's tile layers from the one that holds plane c0
__global__ __launch_bounds__(kThreads) void roundKernel(RedistanceArgs a)
{
    __shared__ float box[kBox];
    __shared__ unsigned int tally[1];

    const TileThread th;
    const int t = th.t, lane = th.lane, wave = th.wave;
    const int ti0 = th.i0, tj0 = th.j0, k0 = (a.c0 / kTZ + int(blockIdx.z)) * kTZ;
    const int h0 = a.c0 - a.below, h1 = a.c0 + a.planes + a.above;
    const float Bf = float(a.B);
    zeroTally(tally);

    // the tile's cells and the rim; a plane inside the grid that is not held is the nearest one held (no own cell depends on it),
    // a cell outside the whole grid holds +inf
    // Every load is made at an address clamped into the grid and its value dropped where the cell lies outside: no load hangs on a
    // branch, so the ten of a thread are in flight together
    int live = 0;
#pragma unroll
    for (int u = 0; u < (kBox + kThreads - 1) / kThreads; ++u) {
        const int n = t + u * kThreads, m = min(n, kBox - 1);
        const int x = ti0 - 1 + m % kSX, y = tj0 - 1 + (m / kSX) % kSY, z = k0 - 1 + m / (kSX * kSY);
        const int xc = min(max(x, 0), a.gx - 1), yc = min(max(y, 0), a.gy - 1), zc = min(max(z, 0), a.gz - 1);
        const float got = planeOf(a, min(max(zc, h0), h1 - 1))[size_t(yc) * size_t(a.gx) + size_t(xc)];
        const float v = x == xc && y == yc && z == zc ? got : INFINITY;
        live |= fabsf(v) < Bf;
        if (n < kBox) box[n] = v;
    }
    const int any = __syncthreads_or(live);

    const int i = th.i, j = th.j;
    const bool column = i < a.gx && j < a.gy;
    const size_t row = size_t(j) * size_t(a.gx) + size_t(i), plane = size_t(a.gx) * size_t(a.gy);
    const int lx = lane + 1, ly = wave + 1;
    if (!any) {  // no T < B in the box: nothing can change
        if (column)
            for (int kk = 0; kk < kTZ; ++kk) {
                const int k = k0 + kk - a.c0;
                if (k >= 0 && k < a.planes) a.out[size_t(k) * plane + row] = stored(a, box[boxAt(lx, ly, kk + 1)]);
            }
        return;
    }

    float cur[kTZ], first[kTZ];
    bool fixed[kTZ];
#pragma unroll
    for (int kk = 0; kk < kTZ; ++kk) {
        const int z = k0 + kk;
        const float c = box[boxAt(lx, ly, kk + 1)];
        cur[kk] = first[kk] = c;
        // interface cells (an in-grid neighbour of the other sign) and cells outside the grid are never updated
        const bool neg = signbit(c);
        bool hold = !column || z >= a.gz;
        hold |= i > 0 && signbit(box[boxAt(lx - 1, ly, kk + 1)]) != neg;
        hold |= i + 1 < a.gx && signbit(box[boxAt(lx + 1, ly, kk + 1)]) != neg;
        hold |= j > 0 && signbit(box[boxAt(lx, ly - 1, kk + 1)]) != neg;
        hold |= j + 1 < a.gy && signbit(box[boxAt(lx, ly + 1, kk + 1)]) != neg;
        hold |= z > 0 && signbit(box[boxAt(lx, ly, kk)]) != neg;
        hold |= z + 1 < a.gz && signbit(box[boxAt(lx, ly, kk + 2)]) != neg;
        fixed[kk] = hold;
    }
    const float below = fabsf(box[boxAt(lx, ly, 0)]), above = fabsf(box[boxAt(lx, ly, kTZ + 1)]);  // the rim along z: held

    for (int it = 0; it < a.inner; ++it) {
        float next[kTZ];
#pragma unroll
        for (int kk = 0; kk < kTZ; ++kk) {
            next[kk] = cur[kk];
            if (fixed[kk]) continue;
            const float ax = fminf(fabsf(box[boxAt(lx - 1, ly, kk + 1)]), fabsf(box[boxAt(lx + 1, ly, kk + 1)]));
            const float ay = fminf(fabsf(box[boxAt(lx, ly - 1, kk + 1)]), fabsf(box[boxAt(lx, ly + 1, kk + 1)]));
            const float zm = kk == 0 ? below : fabsf(cur[kk - 1]), zp = kk == kTZ - 1 ? above : fabsf(cur[kk + 1]);
            const float tn = float(fmin(godunov(ax, ay, fminf(zm, zp)), a.B));
            next[kk] = copysignf(fminf(fabsf(cur[kk]), tn), cur[kk]);
        }
#pragma unroll
        for (int kk = 0; kk < kTZ; ++kk) cur[kk] = next[kk];
        if (it + 1 < a.inner) {  // (uniform) the tile's cells of the box become the new iterate; the rim stays
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < kTZ; ++kk) box[boxAt(lx, ly, kk + 1)] = cur[kk];
            __syncthreads();
        }
    }

    unsigned int changed = 0;
    if (column) {
#pragma unroll
        for (int kk = 0; kk < kTZ; ++kk) {
            const int k = k0 + kk - a.c0;
            if (k < 0 || k >= a.planes) continue;
            changed += cur[kk] != first[kk];
            a.out[size_t(k) * plane + row] = stored(a, cur[kk]);
        }
    }
    const unsigned int found[1] = {changed};
    if (a.count && a.counts) addTally(tally, found, a.counts + 1);
}

// What the three entries refuse of a desc, before any device work.  [c0, c0 + planes) with the halo planes held is the box of the
// arrays; `scratch`: the call ping-pongs through d->scratch; in_name: what phi_in holds for this entry.  Fills the kernels' arguments
int checkDesc(const char *fn, const mgps_redistance_desc *d, int c0, int planes, int below, int above, const float *lo, const float *hi,
              bool scratch, const char *lo_name, const char *hi_name, RedistanceArgs &a)
{
    if (!d || d->struct_size != int(sizeof(mgps_redistance_desc))) return refuse(fn, "NULL or struct_size mismatch (mgps_redistance_desc)");
    if (int rc = checkTileExtents(fn, d->gx, d->gy, d->gz, true); rc != MGPS_OK) return rc;
    if (!std::isfinite(d->band) || !(float(d->band) > 0.0f) || !std::isfinite(float(d->band)))
        return refuse(fn, "band is not finite and > 0 (as a float32 number of cells)");
    if (!std::isfinite(d->dx) || !(d->dx > 0.0)) return refuse(fn, "dx is not finite and > 0");
    if (d->rounds < 0) return refuse(fn, "rounds = " + std::to_string(d->rounds) + " is negative");
    if (d->inner < 1 || d->inner > 8) return refuse(fn, "inner = " + std::to_string(d->inner) + " is outside 1 .. 8");
    if (!d->phi_in) return refuse(fn, "phi_in is NULL");
    if (!d->phi_out) return refuse(fn, "phi_out is NULL");
    if (scratch && !d->scratch) return refuse(fn, "scratch is NULL: rounds > 0 ping-pong between phi_out and a scratch grid of its shape");
    if (int rc = checkHaloArrays(fn, lo_name, lo, below, hi_name, hi, above); rc != MGPS_OK) return rc;

    const size_t plane = size_t(d->gx) * size_t(d->gy) * sizeof(float);
    ArrayRanges arrays;
    arrays.add("phi_in", d->phi_in, plane * size_t(planes), false);
    arrays.add("phi_out", d->phi_out, plane * size_t(planes), true);
    if (scratch) arrays.add("scratch", d->scratch, plane * size_t(planes), true);
    if (below > 0) arrays.add(lo_name, lo, plane * size_t(below), false);
    if (above > 0) arrays.add(hi_name, hi, plane * size_t(above), false);
    if (int rc = arrays.refuseOverlap(fn); rc != MGPS_OK) return rc;
    a = RedistanceArgs{};
    a.gx = d->gx, a.gy = d->gy, a.gz = d->gz, a.c0 = c0, a.planes = planes, a.below = below, a.above = above;
    a.inner = d->inner, a.B = double(float(d->band)), a.dx = d->dx;
    a.in = HeldPlanes{d->phi_in, below > 0 ? lo : nullptr, above > 0 ? hi : nullptr};
    a.out = d->phi_out, a.counts = d->counts_dev;
    return MGPS_OK;
}

int launchInit(const char *fn, const RedistanceArgs &a, hipStream_t st)
{
    initKernel<<<tileGrid(a.gx, a.gy, a.planes), kThreads, 0, st>>>(a);
    return hipStatus(fn, hipGetLastError());
}

// every whole-grid tile layer that meets the window
int launchRound(const char *fn, const RedistanceArgs &a, hipStream_t st)
{
    const int layers = (a.c0 + a.planes + kTZ - 1) / kTZ - a.c0 / kTZ;
    roundKernel<<<tileGrid(a.gx, a.gy, layers * kTZ), kThreads, 0, st>>>(a);
    return hipStatus(fn, hipGetLastError());
}
}  // namespace

extern "C" {

int mgps_fields_redistance(const mgps_redistance_desc *d, void *stream)
try {
    const char *fn = "mgps_fields_redistance";
    RedistanceArgs a;
    if (int rc = checkDesc(fn, d, 0, d ? d->gz : 0, 0, 0, nullptr, nullptr, d && d->rounds > 0, "", "", a); rc != MGPS_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    // launch l of 0 .. rounds writes phi_out where rounds - l is even: the last one does
    const auto target = [&](int l) { return (d->rounds - l) % 2 == 0 ? d->phi_out : d->scratch; };
    RedistanceArgs first = a;
    first.out = target(0), first.scale = d->rounds == 0;
    if (int rc = launchInit(fn, first, st); rc != MGPS_OK) return rc;
    for (int l = 1; l <= d->rounds; ++l) {
        RedistanceArgs r = a;
        r.in.win = target(l - 1), r.out = target(l);
        r.scale = r.count = l == d->rounds;
        if (int rc = launchRound(fn, r, st); rc != MGPS_OK) return rc;
    }
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_redistance_init(const mgps_fields_slab *w, const mgps_redistance_desc *d, int halo, const float *phi_lo,
                                     const float *phi_hi, void *stream)
try {
    const char *fn = "mgps_fields_slab_redistance_init";
    int below = 0, above = 0;
    if (int rc = checkWindowOf(fn, w, d, halo, below, above); rc != MGPS_OK) return rc;
    RedistanceArgs a;
    if (int rc = checkDesc(fn, d, w->c0, w->c1 - w->c0, below, above, phi_lo, phi_hi, false, "phi_lo", "phi_hi", a); rc != MGPS_OK) return rc;
    int n0, n1;
    planesRead(w->c0, w->c1, false, n0, n1);
    if (int rc = checkHalo(fn, w->c0, w->c1, w->gz, halo, below, above, n0, n1, "the initial pass"); rc != MGPS_OK) return rc;
    return launchInit(fn, a, static_cast<hipStream_t>(stream));
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_redistance_round(const mgps_fields_slab *w, const mgps_redistance_desc *d, int halo, const float *state_lo,
                                      const float *state_hi, int last, void *stream)
try {
    const char *fn = "mgps_fields_slab_redistance_round";
    int below = 0, above = 0;
    if (int rc = checkWindowOf(fn, w, d, halo, below, above); rc != MGPS_OK) return rc;
    RedistanceArgs a;
    if (int rc = checkDesc(fn, d, w->c0, w->c1 - w->c0, below, above, state_lo, state_hi, false, "state_lo", "state_hi", a); rc != MGPS_OK) return rc;
    // inner = 1 reads the own cells' neighbours only; more iterations read every tile that meets the window, and its rim
    int n0, n1;
    planesRead(w->c0, w->c1, d->inner > 1, n0, n1);
    if (int rc = checkHalo(fn, w->c0, w->c1, w->gz, halo, below, above, n0, n1, "a round of inner = " + std::to_string(d->inner)); rc != MGPS_OK) return rc;
    a.scale = a.count = last != 0;
    return launchRound(fn, a, static_cast<hipStream_t>(stream));
}
MGPS_API_CATCH(nullptr)
}
