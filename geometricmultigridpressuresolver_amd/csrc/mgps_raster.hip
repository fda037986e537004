// Rigid bodies rasterised on the device (include/mgps_fields.h, "rigid bodies rasterised"): solid_phi, the three
// cut-weight face grids and the three body-id face grids from a host table of shapes and poses, on a whole grid or a slab window.
// One launch over the tiles of mgps_tile_pass.h.  A workgroup tests the bodies' reach boxes against its tile and compacts the hits
// into an LDS list in ascending id; with an empty list it streams the static values through.  Otherwise it evaluates the tile's
// (kTX + 1)(kTY + 1)(kTZ + 1) nodes over the list into LDS (fp64 phi, uint8 owner) and writes its cells and the faces it owns from
// them: a tile owns the backward face of each of its cells per axis, and the forward face where the grid ends.  A node on a tile's
// rim is evaluated by every tile that holds it, each over its own list -- the same value, since a body off a tile's list does not
// reach any of its nodes and contributes `band` there either way.
#include <cmath>
#include <new>

#include "mgps_tile_pass.h"

using namespace mgps;

namespace {

constexpr int kNX = kTX + 1, kNY = kTY + 1, kNZ = kTZ + 1, kNodes = kNX * kNY * kNZ;

// one row of the device table: the shape, and its reach box
struct RasterBody {
    double centre[3], rot[9], half[3], origin[3], spacing;
    double lo[3], hi[3];  // the reach box, bounds included
    const float *sdf;
    int kind, nx, ny, nz;
};

struct RasterArgs {
    int gx, gy, planes;  // the box the arrays are indexed in: the whole grid, or a window of its planes
    int c0;              // the whole grid's plane of the box's plane 0
    int bodies;
    double band, minOpen;
    const RasterBody *table;  // bodies + 1 rows
    const float *staticPhi, *staticCw[3];
    float *phi, *cw[3];
    int32_t *body[3];
};

// contribution of body b at the point x
__device__ __forceinline__ double contribution(const RasterBody &b, double band, double x, double y, double z)
{
    if (x < b.lo[0] || x > b.hi[0] || y < b.lo[1] || y > b.hi[1] || z < b.lo[2] || z > b.hi[2]) return band;
    const double dx = x - b.centre[0], dy = y - b.centre[1], dz = z - b.centre[2];
    const double p[3] = {b.rot[0] * dx + b.rot[3] * dy + b.rot[6] * dz, b.rot[1] * dx + b.rot[4] * dy + b.rot[7] * dz,
                         b.rot[2] * dx + b.rot[5] * dy + b.rot[8] * dz};  // R^T (x - centre)
    double sdf;
    if (b.kind == MGPS_BODY_SPHERE) {
        sdf = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) - b.half[0];
    } else if (b.kind == MGPS_BODY_BOX) {
        const double q0 = fabs(p[0]) - b.half[0], q1 = fabs(p[1]) - b.half[1], q2 = fabs(p[2]) - b.half[2];
        const double o0 = fmax(q0, 0.0), o1 = fmax(q1, 0.0), o2 = fmax(q2, 0.0);
        sdf = sqrt(o0 * o0 + o1 * o1 + o2 * o2) + fmin(fmax(q0, fmax(q1, q2)), 0.0);
    } else {
        const int n[3] = {b.nx, b.ny, b.nz};
        int i0[3];
        double f[3], out2 = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double top = double(n[a] - 1);
            const double g = fmin(fmax((p[a] - b.origin[a]) / b.spacing, 0.0), top);
            i0[a] = min(int(floor(g)), n[a] - 2);
            f[a] = g - double(i0[a]);
            const double lo = b.origin[a], hi = b.origin[a] + top * b.spacing;
            const double e = fmax(fmax(lo - p[a], p[a] - hi), 0.0);
            out2 += e * e;
        }
        const float *s = b.sdf + (size_t(i0[2]) * b.ny + i0[1]) * b.nx + i0[0];
        const size_t sy = size_t(b.nx), sz = size_t(b.nx) * b.ny;
        const auto lerp = [](double t, double u, double v) { return (1.0 - t) * u + t * v; };
        const double x00 = lerp(f[0], double(s[0]), double(s[1])), x10 = lerp(f[0], double(s[sy]), double(s[sy + 1]));
        const double x01 = lerp(f[0], double(s[sz]), double(s[sz + 1])), x11 = lerp(f[0], double(s[sz + sy]), double(s[sz + sy + 1]));
        sdf = lerp(f[2], lerp(f[1], x00, x10), lerp(f[1], x01, x11)) + sqrt(out2);
    }
    return fmin(sdf, band);
}

// min(band, min over the list) at a point, and the lowest id that attains it below band (0: none)
__device__ __forceinline__ double fieldAt(const RasterArgs &a, const uint8_t *list, int count, double x, double y, double z, int &owner)
{
    double phi = a.band;
    owner = 0;
    for (int q = 0; q < count; ++q) {
        const int r = __builtin_amdgcn_readfirstlane(int(list[q]));  // (the list is the workgroup's: the row is a scalar load)
        const double v = contribution(a.table[r], a.band, x, y, z);
        if (v < phi) phi = v, owner = r;  // ascending ids and a strict <: ties go to the lowest id
    }
    return phi;
}

// the open fraction of a face and the owner of its closed part from its corners in cyclic order (0,0), (1,0), (1,1), (0,1)
__device__ __forceinline__ void faceFromCorners(const double p[4], const uint8_t o[4], double minOpen, float &w, int32_t &owner)
{
    // a running shoelace sum over the polygon's vertices: no vertex array
    double fx = 0, fy = 0, px = 0, py = 0, twice = 0;
    int nv = 0;
    const auto vertex = [&](double x, double y) {
        if (nv == 0) fx = x, fy = y;
        else twice += px * y - x * py;
        px = x, py = y, ++nv;
    };
    const double cx[4] = {0, 1, 1, 0}, cy[4] = {0, 0, 1, 1};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int n = (e + 1) & 3;
        const bool ina = p[e] >= 0.0, inb = p[n] >= 0.0;
        if (ina) vertex(cx[e], cy[e]);
        if (ina != inb) {
            const double t = p[e] / (p[e] - p[n]);
            vertex(cx[e] + t * (cx[n] - cx[e]), cy[e] + t * (cy[n] - cy[e]));
        }
    }
    if (nv > 0) twice += px * fy - fx * py;
    double wb = fmin(fmax(0.5 * twice, 0.0), 1.0);
    if (wb < minOpen) wb = 0.0;
    if (wb > 1.0 - minOpen) wb = 1.0;
    w = float(wb);
    double least = p[0];
    int32_t leastOwner = o[0];
#pragma unroll
    for (int e = 1; e < 4; ++e)
        if (p[e] < least) least = p[e], leastOwner = o[e];  // (a strict <: ties go to the first corner)
    owner = w < 1.f ? leastOwner : 0;
}

// A tile no body reaches: the static values go through (phi against band, the weights against 1), with ids 0.  The loads of the
// thread's kTZ cells are all issued before the first store
__device__ __forceinline__ void streamCells(const RasterArgs &a, int i, int j, int k0)
{
    const float bandF = float(a.band);
    float sp[kTZ], sw[3][kTZ];
#pragma unroll
    for (int kk = 0; kk < kTZ; ++kk) {
        const CellFaces at(a, i, j, min(k0 + kk, a.planes - 1));
        sp[kk] = a.staticPhi ? a.staticPhi[at.c] : 1e30f;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) sw[ax][kk] = a.staticCw[ax] ? a.staticCw[ax][at.f[ax]] : 1.f;
    }
#pragma unroll
    for (int kk = 0; kk < kTZ; ++kk) {
        if (k0 + kk >= a.planes) break;
        const CellFaces at(a, i, j, k0 + kk);
        put(a.phi + at.c, fminf(sp[kk], bandF));
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            put(a.cw[ax] + at.f[ax], fminf(sw[ax][kk], 1.f));
            put(a.body[ax] + at.f[ax], int32_t(0));
            if (at.more[ax]) {
                const size_t f = at.f[ax] + at.step[ax];
                a.cw[ax][f] = fminf(a.staticCw[ax] ? a.staticCw[ax][f] : 1.f, 1.f);
                a.body[ax][f] = 0;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void rasterKernel(RasterArgs a)
{
    __shared__ double nodePhi[kNodes];
    __shared__ uint8_t nodeOwner[kNodes];
    __shared__ uint8_t list[256];
    __shared__ unsigned long long hitMask[kThreads / 64];

    // (TileThread's mapping, restated: through the struct the node loop below compiles to other code, LABNOTES R14)
    const int t = int(threadIdx.x), lane = t & 63, wave = t >> 6;
    const int i0 = int(blockIdx.x) * kTX, j0 = int(blockIdx.y) * kTY, k0 = int(blockIdx.z) * kTZ;
    const int kg0 = k0 + a.c0;

    // the bodies whose reach box meets the tile's node box: thread t tests body t, the hits go to the list in ascending id
    bool hit = false;
    if (t >= 1 && t <= a.bodies) {
        const RasterBody &b = a.table[t];
        hit = b.lo[0] <= double(i0 + kTX) && b.hi[0] >= double(i0) && b.lo[1] <= double(j0 + kTY) && b.hi[1] >= double(j0) &&
              b.lo[2] <= double(kg0 + kTZ) && b.hi[2] >= double(kg0);
    }
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) hitMask[wave] = mask;
    __syncthreads();
    int before = 0, count = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const int n = __popcll(hitMask[w]);
        if (w < wave) before += n;
        count += n;
    }
    if (hit) list[before + __popcll(mask & ((1ull << lane) - 1ull))] = uint8_t(t);
    __syncthreads();

    // thread (lane, wave) owns the cells (i0 + lane, j0 + wave, k0 + kk), kk = 0 .. kTZ - 1
    const int i = i0 + lane, j = j0 + wave;
    if (count == 0) {
        if (i < a.gx && j < a.gy) streamCells(a, i, j, k0);
        return;
    }
    for (int n = t; n < kNodes; n += kThreads) {
        const int ni = n % kNX, nj = (n / kNX) % kNY, nk = n / (kNX * kNY);
        int owner;
        nodePhi[n] = fieldAt(a, list, count, double(i0 + ni), double(j0 + nj), double(kg0 + nk), owner);
        nodeOwner[n] = uint8_t(owner);
    }
    __syncthreads();
    if (i >= a.gx || j >= a.gy) return;
    for (int kk = 0; kk < kTZ; ++kk) {
        const int k = k0 + kk;
        if (k >= a.planes) break;
        const CellFaces at(a, i, j, k);
        int owner;
        const float cellPhi = float(fieldAt(a, list, count, double(i) + 0.5, double(j) + 0.5, double(k + a.c0) + 0.5, owner));
        a.phi[at.c] = fminf(a.staticPhi ? a.staticPhi[at.c] : 1e30f, cellPhi);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            // in-plane axes u < v of the face; its corners in (u, v): (0,0), (1,0), (1,1), (0,1)
            const int u = ax == 0 ? 1 : 0, v = ax == 2 ? 1 : 2;
            const int stride[3] = {1, kNX, kNX * kNY};
            for (int side = 0; side <= int(at.more[ax]); ++side) {
                const size_t f = at.f[ax] + size_t(side) * at.step[ax];
                const int n00 = (kk * kNY + wave) * kNX + lane + side * stride[ax];
                const int n[4] = {n00, n00 + stride[u], n00 + stride[u] + stride[v], n00 + stride[v]};
                const double p[4] = {nodePhi[n[0]], nodePhi[n[1]], nodePhi[n[2]], nodePhi[n[3]]};
                const uint8_t o[4] = {nodeOwner[n[0]], nodeOwner[n[1]], nodeOwner[n[2]], nodeOwner[n[3]]};
                float w;
                faceFromCorners(p, o, a.minOpen, w, owner);
                a.cw[ax][f] = fminf(a.staticCw[ax] ? a.staticCw[ax][f] : 1.f, w);
                a.body[ax][f] = owner;
            }
        }
    }
}

bool finite3(const double *v, int n)
{
    for (int q = 0; q < n; ++q)
        if (!std::isfinite(v[q])) return false;
    return true;
}

// the table row of a checked shape: its reach box is the world AABB of the frame box, grown by band
RasterBody tableRow(const mgps_body_shape &s, double band)
{
    RasterBody b{};
    b.kind = s.kind, b.nx = s.nx, b.ny = s.ny, b.nz = s.nz, b.sdf = s.sdf, b.spacing = s.spacing;
    double mid[3] = {0, 0, 0}, h[3];
    for (int q = 0; q < 3; ++q) {
        b.centre[q] = s.centre[q], b.half[q] = s.half[q], b.origin[q] = s.origin[q];
        h[q] = s.kind == MGPS_BODY_SPHERE ? s.half[0] : s.half[q];
    }
    for (int q = 0; q < 9; ++q) b.rot[q] = s.rotation[q];
    if (s.kind == MGPS_BODY_GRID) {
        const int n[3] = {s.nx, s.ny, s.nz};
        for (int q = 0; q < 3; ++q) {
            h[q] = 0.5 * double(n[q] - 1) * s.spacing;
            mid[q] = s.origin[q] + h[q];
        }
    }
    for (int q = 0; q < 3; ++q) {
        const double *R = s.rotation + 3 * q;
        const double c = s.centre[q] + (R[0] * mid[0] + R[1] * mid[1] + R[2] * mid[2]);
        const double e = (std::fabs(R[0]) * h[0] + std::fabs(R[1]) * h[1] + std::fabs(R[2]) * h[2]) + band;
        b.lo[q] = c - e, b.hi[q] = c + e;
    }
    return b;
}

int checkShape(const char *fn, int r, const mgps_body_shape &s)
{
    const std::string who = "body " + std::to_string(r) + ": ";
    if (s.kind != MGPS_BODY_SPHERE && s.kind != MGPS_BODY_BOX && s.kind != MGPS_BODY_GRID) return refuse(fn, who + "unknown kind " + std::to_string(s.kind));
    if (!finite3(s.centre, 3)) return refuse(fn, who + "non-finite centre");
    if (!finite3(s.rotation, 9)) return refuse(fn, who + "non-finite rotation");
    double worst = 0;
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) {
            double dot = 0;
            for (int m = 0; m < 3; ++m) dot += s.rotation[3 * m + p] * s.rotation[3 * m + q];
            worst = std::max(worst, std::fabs(dot - (p == q ? 1.0 : 0.0)));
        }
    if (!(worst <= 1e-6)) return refuse(fn, who + "rotation is not orthonormal (|R^T R - I| = " + std::to_string(worst) + " > 1e-6)");
    if (s.kind == MGPS_BODY_SPHERE && !(s.half[0] > 0 && std::isfinite(s.half[0]))) return refuse(fn, who + "the radius must be positive and finite");
    if (s.kind == MGPS_BODY_BOX)
        for (int q = 0; q < 3; ++q)
            if (!(s.half[q] > 0 && std::isfinite(s.half[q]))) return refuse(fn, who + "every half extent must be positive and finite");
    if (s.kind == MGPS_BODY_GRID) {
        if (!s.sdf) return refuse(fn, who + "sdf is NULL");
        if (s.nx < 2 || s.ny < 2 || s.nz < 2) return refuse(fn, who + "every sample dimension must be at least 2");
        if (!(s.spacing > 0 && std::isfinite(s.spacing))) return refuse(fn, who + "the spacing must be positive and finite");
        if (!finite3(s.origin, 3)) return refuse(fn, who + "non-finite origin");
    }
    return MGPS_OK;
}

// what both entries refuse of a desc
int checkDesc(const char *fn, const mgps_raster_desc *d)
{
    if (!d || d->struct_size != int(sizeof(mgps_raster_desc))) return refuse(fn, "NULL or struct_size mismatch (mgps_raster_desc)");
    if (int rc = checkTileExtents(fn, d->gx, d->gy, d->gz, false); rc != MGPS_OK) return rc;
    if (d->bodies < 1 || d->bodies > 255) return refuse(fn, "bodies = " + std::to_string(d->bodies) + " is outside 1 .. 255");
    if (!d->shapes) return refuse(fn, "shapes is NULL");
    if (!(d->band >= 2.0 && d->band <= 16.0)) return refuse(fn, "band must lie in 2 .. 16 cells");
    if (!(d->min_open >= 0.0 && d->min_open < 0.5)) return refuse(fn, "min_open must lie in [0, 0.5)");
    for (int r = 1; r <= d->bodies; ++r)
        if (int rc = checkShape(fn, r, d->shapes[r]); rc != MGPS_OK) return rc;
    if (!d->solid_phi) return refuse(fn, "solid_phi (output) is NULL");
    for (int a = 0; a < 3; ++a) {
        if (!d->cut_weights[a]) return refuse(fn, "cut_weights (output): three grids are required");
        if (!d->body[a]) return refuse(fn, "body (output): three grids are required");
    }
    const int given = (d->static_cut_weights[0] != nullptr) + (d->static_cut_weights[1] != nullptr) + (d->static_cut_weights[2] != nullptr);
    if (given != 0 && given != 3) return refuse(fn, "static_cut_weights: all three grids, or none");
    return MGPS_OK;
}

// the launch on the planes [c0, c0 + planes) of a checked desc; the table goes up from a host copy into a block in stream order
int runRaster(const char *fn, const mgps_raster_desc *d, int c0, int planes, hipStream_t st)
{
    std::vector<RasterBody> rows(size_t(d->bodies) + 1);
    for (int r = 1; r <= d->bodies; ++r) rows[size_t(r)] = tableRow(d->shapes[r], d->band);
    const size_t bytes = rows.size() * sizeof(RasterBody);
    return withStreamBlock(fn, st, bytes, rows.data(), bytes, [&](void *dev) {
        RasterArgs a{};
        a.gx = d->gx, a.gy = d->gy, a.planes = planes, a.c0 = c0, a.bodies = d->bodies, a.band = d->band, a.minOpen = d->min_open;
        a.table = static_cast<const RasterBody *>(dev);
        a.staticPhi = d->static_solid_phi, a.phi = d->solid_phi;
        for (int q = 0; q < 3; ++q) a.staticCw[q] = d->static_cut_weights[q], a.cw[q] = d->cut_weights[q], a.body[q] = d->body[q];
        rasterKernel<<<tileGrid(d->gx, d->gy, planes), kThreads, 0, st>>>(a);
        return hipStatus(fn, hipGetLastError());
    });
}

// ---- velocity samples of deforming colliders on the face grids (include/mgps_fields.h, "deforming mesh colliders"; DESIGN.md
// section 20) -----------------------------------------------------------------------------------------------------------------------
// one row of the device table: the pose and sample box of a GRID body, its three sample arrays and the motion of its frame
struct SampledBody {
    double centre[3], rot[9], origin[3], spacing, motion[6];
    const float *vel[3];  // all NULL: the body's faces are not written
    int nx, ny, nz, pad;
};

struct SampledArgs {
    int gx, gy, planes, c0;  // as RasterArgs
    int bodies;
    const SampledBody *table;  // bodies + 1 rows
    float *sv[3];
    const int32_t *body[3];
};

// the value of face f of `axis` at (i, j, k) of the box, owned by body b
__device__ __forceinline__ float sampledFace(const SampledBody &b, int axis, int i, int j, int kg)
{
    double pos[3] = {i + 0.5, j + 0.5, kg + 0.5};
    const int ijk[3] = {i, j, kg};
    pos[axis] = double(ijk[axis]);
    const double dx = pos[0] - b.centre[0], dy = pos[1] - b.centre[1], dz = pos[2] - b.centre[2];
    const double p[3] = {b.rot[0] * dx + b.rot[3] * dy + b.rot[6] * dz, b.rot[1] * dx + b.rot[4] * dy + b.rot[7] * dz,
                         b.rot[2] * dx + b.rot[5] * dy + b.rot[8] * dz};  // R^T (x - centre)
    const int n[3] = {b.nx, b.ny, b.nz};
    int i0[3];
    double f[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double g = fmin(fmax((p[a] - b.origin[a]) / b.spacing, 0.0), double(n[a] - 1));
        i0[a] = min(int(floor(g)), n[a] - 2);
        f[a] = g - double(i0[a]);
    }
    const size_t at = (size_t(i0[2]) * b.ny + i0[1]) * b.nx + i0[0], sy = size_t(b.nx), sz = size_t(b.nx) * b.ny;
    const auto lerp = [](double t, double u, double v) { return (1.0 - t) * u + t * v; };
    double u[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *s = b.vel[c] + at;
        const double x00 = lerp(f[0], double(s[0]), double(s[1])), x10 = lerp(f[0], double(s[sy]), double(s[sy + 1]));
        const double x01 = lerp(f[0], double(s[sz]), double(s[sz + 1])), x11 = lerp(f[0], double(s[sz + sy]), double(s[sz + sy + 1]));
        u[c] = lerp(f[2], lerp(f[1], x00, x10), lerp(f[1], x01, x11));
    }
    const double d[3] = {dx, dy, dz};
    const int uu = (axis + 1) % 3, vv = (axis + 2) % 3;
    const double *m = b.motion;
    const double frame = m[axis] + m[3 + uu] * d[vv] - m[3 + vv] * d[uu];  // (U + omega x (x_f - centre))_axis, as the rigid pass forms it
    const double *R = b.rot + 3 * axis;
    return float(((R[0] * u[0] + R[1] * u[1]) + R[2] * u[2]) + frame);
}

// A thread per cell and kTZ planes: the faces a cell owns (CellFaces).  Three id loads per cell; the table row and the samples are
// read only where a sampled body owns the face
__global__ __launch_bounds__(kThreads) void sampledVelocityKernel(SampledArgs s)
{
    const TileThread th;
    const int i = th.i, j = th.j, k0 = th.k0;
    if (i >= s.gx || j >= s.gy) return;
    const TileBox box{s.gx, s.gy, s.planes};
#pragma unroll
    for (int kk = 0; kk < kTZ; ++kk) {
        const int k = k0 + kk;
        if (k >= s.planes) break;
        const CellFaces at(box, i, j, k);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax)
            for (int side = 0; side <= int(at.more[ax]); ++side) {
                const size_t f = at.f[ax] + size_t(side) * at.step[ax];
                const int r = s.body[ax][f];
                if (r < 1 || r > s.bodies) continue;
                const SampledBody &b = s.table[r];
                if (!b.vel[0]) continue;
                s.sv[ax][f] = sampledFace(b, ax, i + (ax == 0 ? side : 0), j + (ax == 1 ? side : 0), k + s.c0 + (ax == 2 ? side : 0));
            }
    }
}

// what both entries refuse, before any device work
int checkSampled(const char *fn, float *const sv[3], const int32_t *const body[3], int bodies, const mgps_body_shape *shapes,
                 const mgps_body_velocity *velocities, int gx, int gy, int gz)
{
    if (bodies < 1 || bodies > 255) return refuse(fn, "bodies = " + std::to_string(bodies) + " is outside 1 .. 255");
    if (int rc = checkTileExtents(fn, gx, gy, gz, false); rc != MGPS_OK) return rc;
    if (!sv || !sv[0] || !sv[1] || !sv[2]) return refuse(fn, "solid velocity: three grids are required");
    if (!body || !body[0] || !body[1] || !body[2]) return refuse(fn, "body: three grids are required");
    if (!shapes) return refuse(fn, "shapes is NULL");
    if (!velocities) return refuse(fn, "velocities is NULL");
    for (int r = 1; r <= bodies; ++r) {
        if (int rc = checkShape(fn, r, shapes[r]); rc != MGPS_OK) return rc;
        const mgps_body_velocity &v = velocities[r];
        const std::string who = "body " + std::to_string(r) + ": ";
        const int given = (v.vel[0] != nullptr) + (v.vel[1] != nullptr) + (v.vel[2] != nullptr);
        if (given != 0 && given != 3) return refuse(fn, who + "vel: all three sample arrays, or none");
        if (given == 0) continue;
        if (shapes[r].kind != MGPS_BODY_GRID) return refuse(fn, who + "velocity samples need a GRID body (kind = " + std::to_string(shapes[r].kind) + ")");
        if (!finite3(v.motion, 6)) return refuse(fn, who + "non-finite motion");
    }
    return MGPS_OK;
}

// the launch on the planes [c0, c0 + planes) of checked arguments; the table goes up into a block in stream order
int runSampled(const char *fn, float *const sv[3], const int32_t *const body[3], int bodies, const mgps_body_shape *shapes,
               const mgps_body_velocity *velocities, int gx, int gy, int c0, int planes, hipStream_t st)
{
    std::vector<SampledBody> rows(size_t(bodies) + 1);
    for (int r = 1; r <= bodies; ++r) {
        const mgps_body_shape &s = shapes[r];
        SampledBody &b = rows[size_t(r)];
        b = SampledBody{};
        for (int q = 0; q < 3; ++q) b.centre[q] = s.centre[q], b.origin[q] = s.origin[q], b.vel[q] = velocities[r].vel[q];
        for (int q = 0; q < 9; ++q) b.rot[q] = s.rotation[q];
        for (int q = 0; q < 6; ++q) b.motion[q] = velocities[r].motion[q];
        b.spacing = s.spacing, b.nx = s.nx, b.ny = s.ny, b.nz = s.nz;
    }
    const size_t bytes = rows.size() * sizeof(SampledBody);
    return withStreamBlock(fn, st, bytes, rows.data(), bytes, [&](void *dev) {
        SampledArgs a{};
        a.gx = gx, a.gy = gy, a.planes = planes, a.c0 = c0, a.bodies = bodies, a.table = static_cast<const SampledBody *>(dev);
        for (int q = 0; q < 3; ++q) a.sv[q] = sv[q], a.body[q] = body[q];
        sampledVelocityKernel<<<tileGrid(gx, gy, planes), kThreads, 0, st>>>(a);
        return hipStatus(fn, hipGetLastError());
    });
}
}  // namespace

extern "C" {

int mgps_fields_rasterize_bodies(const mgps_raster_desc *d, void *stream)
try {
    const char *fn = "mgps_fields_rasterize_bodies";
    if (int rc = checkDesc(fn, d); rc != MGPS_OK) return rc;
    return runRaster(fn, d, 0, d->gz, static_cast<hipStream_t>(stream));
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_rasterize_bodies(const mgps_fields_slab *w, const mgps_raster_desc *d, void *stream)
try {
    const char *fn = "mgps_fields_slab_rasterize_bodies";
    if (int rc = checkDesc(fn, d); rc != MGPS_OK) return rc;
    int below, above;  // (no halo: a cell's values depend on the bodies alone)
    if (int rc = checkWindowOf(fn, w, d, 0, below, above); rc != MGPS_OK) return rc;
    return runRaster(fn, d, w->c0, w->c1 - w->c0, static_cast<hipStream_t>(stream));
}
MGPS_API_CATCH(nullptr)

int mgps_fields_sampled_velocity(float *const sv[3], const int32_t *const body[3], int bodies, const mgps_body_shape *shapes,
                                 const mgps_body_velocity *velocities, int gx, int gy, int gz, void *stream)
try {
    const char *fn = "mgps_fields_sampled_velocity";
    if (int rc = checkSampled(fn, sv, body, bodies, shapes, velocities, gx, gy, gz); rc != MGPS_OK) return rc;
    return runSampled(fn, sv, body, bodies, shapes, velocities, gx, gy, 0, gz, static_cast<hipStream_t>(stream));
}
MGPS_API_CATCH(nullptr)

int mgps_fields_slab_sampled_velocity(const mgps_fields_slab *w, float *const sv[3], const int32_t *const body[3], int bodies,
                                      const mgps_body_shape *shapes, const mgps_body_velocity *velocities, void *stream)
try {
    const char *fn = "mgps_fields_slab_sampled_velocity";
    if (!fieldsSlabWindow(w, fn)) return MGPS_ERR_INVALID_ARGUMENT;
    if (int rc = checkSampled(fn, sv, body, bodies, shapes, velocities, w->gx, w->gy, w->gz); rc != MGPS_OK) return rc;
    return runSampled(fn, sv, body, bodies, shapes, velocities, w->gx, w->gy, w->c0, w->c1 - w->c0, static_cast<hipStream_t>(stream));
}
MGPS_API_CATCH(nullptr)
}
