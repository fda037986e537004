// Triangle-mesh rigid bodies (include/mgps_fields.h, "triangle-mesh rigid bodies"): the float32 body-frame SDF
// samples of a closed mesh that a MGPS_BODY_GRID body reads, and the mesh's volume, centre of mass and inertia tensor on the host.
// The host checks the mesh, turns every triangle so that its lowest vertex index comes first (a cyclic turn: the same triangle, and
// from here on the same numbers whichever turn the caller gave), and works out per triangle the range of bins it is listed in: the
// tiles of kTX x kTY x kTZ samples its box grown by band touches, and the tiles of kCY x kCZ columns its y-z projection touches.  From
// the ranges it makes the bins' list offsets, so the device never sizes anything.  Three launches:
//   meshFillKernel      a thread per triangle gathers its nine coordinates into a table row and claims a slot in each of its bins'
//                       lists (integer atomics: the order of a list changes neither a minimum nor a parity);
//   meshSignKernel      a thread per column and word of 64 samples along x walks its column tile's list and XORs in, for every
//                       triangle the column crosses, the mask of the samples below the crossing: one bit per sample, set inside;
//   meshDistanceKernel  a workgroup per tile walks its list, each thread keeps the least squared distance of its kTZ samples in
//                       registers, then applies sign and clamp and stores once.  An empty list stores +-band.
// Deforming colliders: mgps_fields_mesh_sdf_velocity runs the same host pass and the first two launches, and
// as its third
//   meshVelocityKernel  the distance kernel's walk, which also keeps the table row of the triangle that attains the minimum (ties by
//                       the turned index triple, read from the table only on an equal d^2); after the walk a thread classifies the
//                       closest point on its winner once more for the weights, gathers the three vertex velocities and stores.
#include <cmath>
#include <limits>

#include "mgps_tile_pass.h"

using namespace mgps;

namespace {

// (the tiles of mgps_tile_pass.h: a wave per x-row of 64 samples is also one word of inside bits per row)
constexpr int kCY = 16, kCZ = 16;  // columns (y, z) per workgroup of the sign pass
constexpr int kMaxSamples = 1024;
static_assert(kCY * kCZ == kThreads, "one thread per column");

// one row of the device table: the turned triangle's coordinates (a, b, c) and vertex indices
struct MeshTri {
    double p[9];
    int32_t v[3], pad;
};

// the bins of one triangle, bounds included; `some` says which of the two ranges is not empty
struct TriBins {
    uint8_t lo[3], hi[3];  // tiles of the distance pass, (x, y, z)
    uint8_t clo[2], chi[2];  // column tiles of the sign pass, (y, z)
    uint8_t some[2];
};

struct MeshArgs {
    int nx, ny, nz, triangles;
    int tilesX, tilesY, tilesZ, colsY, colsZ, words;  // words = tilesX: 64 samples of a row per word
    double origin[3], spacing, band;
    const double *xyz;
    const int32_t *tri;  // turned
    const TriBins *bins;
    MeshTri *table;
    const int *offsets;  // tiles + column tiles + 1 entries: the bins' lists, the tiles first
    int *cursor;         // one per bin, zeroed
    int *list;
    unsigned long long *inside;  // (nz, ny, words)
    float *sdf;
};

// the sample position of the definition: one product and one sum, each rounded
__device__ __forceinline__ double samplePos(double origin, double spacing, int i)
{
#pragma clang fp contract(off)
    const double step = spacing * double(i);
    return origin + step;
}

__global__ __launch_bounds__(kThreads) void meshFillKernel(MeshArgs a)
{
    const int t = int(blockIdx.x) * kThreads + int(threadIdx.x);
    if (t >= a.triangles) return;
    MeshTri row;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        row.v[q] = a.tri[3 * t + q];
#pragma unroll
        for (int c = 0; c < 3; ++c) row.p[3 * q + c] = a.xyz[3 * size_t(row.v[q]) + c];
    }
    row.pad = 0;
    a.table[t] = row;
    const TriBins b = a.bins[t];
    const auto claim = [&](int bin) {
        const int slot = a.offsets[bin] + atomicAdd(a.cursor + bin, 1);
        if (slot < a.offsets[bin + 1]) a.list[slot] = t;  // (always: the offsets were counted from the same ranges)
    };
    if (b.some[0])
        for (int z = b.lo[2]; z <= b.hi[2]; ++z)
            for (int y = b.lo[1]; y <= b.hi[1]; ++y)
                for (int x = b.lo[0]; x <= b.hi[0]; ++x) claim((z * a.tilesY + y) * a.tilesX + x);
    if (b.some[1]) {
        const int base = a.tilesX * a.tilesY * a.tilesZ;
        for (int z = b.clo[1]; z <= b.chi[1]; ++z)
            for (int y = b.clo[0]; y <= b.chi[0]; ++y) claim(base + z * a.colsY + y);
    }
}

// The edge function of the projected edge p -> q (p the end with the lower vertex index) at the column (sy, sz), and its sign under the
// shift (sy + eps, sz + eps^2): the sign of the first non-zero term of (e, -(q.z - p.z), q.y - p.y)
__device__ __forceinline__ double edgeFunction(double py, double pz, double qy, double qz, double sy, double sz, int &sign)
{
#pragma clang fp contract(off)
    const double dy = qy - py, dz = qz - pz;
    const double left = dy * (sz - pz), right = dz * (sy - py);
    const double e = left - right;
    sign = e > 0.0 ? 1 : e < 0.0 ? -1 : dz < 0.0 ? 1 : dz > 0.0 ? -1 : dy > 0.0 ? 1 : dy < 0.0 ? -1 : 0;
    return e;
}

// the same for the directed edge u -> w of a triangle: evaluated from the lower index, negated when that swaps the ends, so that the
// two triangles on an edge see the same number
__device__ __forceinline__ double directedEdge(const MeshTri &T, int u, int w, double sy, double sz, int &sign)
{
    const bool swap = T.v[u] > T.v[w];
    const int p = swap ? w : u, q = swap ? u : w;
    const double e = edgeFunction(T.p[3 * p + 1], T.p[3 * p + 2], T.p[3 * q + 1], T.p[3 * q + 2], sy, sz, sign);
    if (swap) sign = -sign;
    return swap ? -e : e;
}

__global__ __launch_bounds__(kThreads) void meshSignKernel(MeshArgs a)
{
    const int t = int(threadIdx.x);
    const int word = int(blockIdx.x), j = int(blockIdx.y) * kCY + (t & (kCY - 1)), k = int(blockIdx.z) * kCZ + t / kCY;
    if (j >= a.ny || k >= a.nz) return;
    const double sy = samplePos(a.origin[1], a.spacing, j), sz = samplePos(a.origin[2], a.spacing, k);
    const int bin = a.tilesX * a.tilesY * a.tilesZ + int(blockIdx.z) * a.colsY + int(blockIdx.y);
    const int begin = a.offsets[bin], end = a.offsets[bin + 1];
    unsigned long long bits = 0;
    for (int q = begin; q < end; ++q) {
        const int r = __builtin_amdgcn_readfirstlane(a.list[q]);  // (the list is the workgroup's: the row is a scalar load)
        const MeshTri &T = a.table[r];
        double area;
        {
#pragma clang fp contract(off)
            const double l = (T.p[4] - T.p[1]) * (T.p[8] - T.p[2]), m = (T.p[5] - T.p[2]) * (T.p[7] - T.p[1]);
            area = l - m;
        }
        if (area == 0.0) continue;  // zero projected area: never crossed
        int sa, sb, sc;
        const double ea = directedEdge(T, 1, 2, sy, sz, sa), eb = directedEdge(T, 2, 0, sy, sz, sb), ec = directedEdge(T, 0, 1, sy, sz, sc);
        if (sa == 0 || sa != sb || sb != sc) continue;
        double sum, depth;
        {
#pragma clang fp contract(off)
            sum = (ea + eb) + ec;
            const double ta = ea * T.p[0], tb = eb * T.p[3], tc = ec * T.p[6];
            depth = ((ta + tb) + tc) / sum;
        }
        if (sum == 0.0) continue;
        // below = the number of samples of the row with s.x < depth (s.x ascends with i)
        const double guess = (depth - a.origin[0]) / a.spacing;
        int below = !(guess > 0.0) ? 0 : guess >= double(a.nx) ? a.nx : int(ceil(guess));
        while (below > 0 && !(samplePos(a.origin[0], a.spacing, below - 1) < depth)) --below;
        while (below < a.nx && samplePos(a.origin[0], a.spacing, below) < depth) ++below;
        const int mine = below - 64 * word;
        bits ^= mine >= 64 ? ~0ull : mine <= 0 ? 0ull : (1ull << mine) - 1ull;
    }
    a.inside[(size_t(k) * a.ny + j) * a.words + word] = bits;
}

// the squared distance from x to the triangle (a, b, c) with ab = b - a, ac = c - a, n = ab x ac, nn = |n|^2: the closest point's
// region by the signs of the projections onto the edges (vertex, edge or face), then the distance to that feature
__device__ __forceinline__ double pointTriangle2(const double *p, const double ab[3], const double ac[3], const double n[3], double nn, double x,
                                                 double y, double z)
{
    const auto dot = [](const double u[3], const double w[3]) { return u[0] * w[0] + u[1] * w[1] + u[2] * w[2]; };
    const double ap[3] = {x - p[0], y - p[1], z - p[2]};
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) return dot(ap, ap);
    const double bp[3] = {x - p[3], y - p[4], z - p[5]};
    const double d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) return dot(bp, bp);
    if (d1 * d4 - d3 * d2 <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
        const double r[3] = {ap[0] - v * ab[0], ap[1] - v * ab[1], ap[2] - v * ab[2]};
        return dot(r, r);
    }
    const double cp[3] = {x - p[6], y - p[7], z - p[8]};
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) return dot(cp, cp);
    if (d5 * d2 - d1 * d6 <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double w = d2 / (d2 - d6);
        const double r[3] = {ap[0] - w * ac[0], ap[1] - w * ac[1], ap[2] - w * ac[2]};
        return dot(r, r);
    }
    if (d3 * d6 - d5 * d4 <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        const double r[3] = {bp[0] - w * (p[6] - p[3]), bp[1] - w * (p[7] - p[4]), bp[2] - w * (p[8] - p[5])};
        return dot(r, r);
    }
    const double h = dot(n, ap);
    return h * h / nn;
}

__global__ __launch_bounds__(kThreads) void meshDistanceKernel(MeshArgs a)
{
    const TileThread th;
    const int lane = th.lane, i = th.i, j = th.j, k0 = th.k0;
    // thread (lane, wave) owns the samples (i, j, k0 + kk), kk = 0 .. kTZ - 1; a thread past the box's end works on the last sample
    const double x = samplePos(a.origin[0], a.spacing, min(i, a.nx - 1)), y = samplePos(a.origin[1], a.spacing, min(j, a.ny - 1));
    double z[kTZ], best[kTZ];
#pragma unroll
    for (int kk = 0; kk < kTZ; ++kk) {
        z[kk] = samplePos(a.origin[2], a.spacing, min(k0 + kk, a.nz - 1));
        best[kk] = std::numeric_limits<double>::infinity();
    }
    const int bin = (int(blockIdx.z) * a.tilesY + int(blockIdx.y)) * a.tilesX + int(blockIdx.x);
    const int begin = a.offsets[bin], end = a.offsets[bin + 1];
    for (int q = begin; q < end; ++q) {
        const int r = __builtin_amdgcn_readfirstlane(a.list[q]);  // (the list is the workgroup's: the row is a scalar load)
        const double *p = a.table[r].p;
        const double ab[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, ac[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
        const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
        const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
#pragma unroll
        for (int kk = 0; kk < kTZ; ++kk) best[kk] = fmin(best[kk], pointTriangle2(p, ab, ac, n, nn, x, y, z[kk]));
    }
    if (i >= a.nx || j >= a.ny) return;
#pragma unroll
    for (int kk = 0; kk < kTZ; ++kk) {
        const int k = k0 + kk;
        if (k >= a.nz) break;
        const size_t row = size_t(k) * a.ny + j;
        const bool in = (a.inside[row * a.words + blockIdx.x] >> lane) & 1ull;
        const double d = fmin(sqrt(best[kk]), a.band);
        a.sdf[row * a.nx + i] = float(in ? -d : d);
    }
}

// ---- vertex velocities at the closest point ---------------------------------------------------------------------
struct MeshVelocityArgs {
    MeshArgs m;              // m.sdf may be NULL
    const double *velocity;  // per vertex, (x, y, z)
    float *vel[3];
};

// The weights (wa, wb, wc) of the closest point of the triangle (a, b, c) to x: the region tests of pointTriangle2, in its order
__device__ __forceinline__ void closestWeights(const double *p, double x, double y, double z, double &wa, double &wb, double &wc)
{
    const auto dot = [](const double u[3], const double w[3]) { return u[0] * w[0] + u[1] * w[1] + u[2] * w[2]; };
    const double ab[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, ac[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
    const double ap[3] = {x - p[0], y - p[1], z - p[2]};
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    wa = 1.0, wb = 0.0, wc = 0.0;
    if (d1 <= 0.0 && d2 <= 0.0) return;
    const double bp[3] = {x - p[3], y - p[4], z - p[5]};
    const double d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) {
        wa = 0.0, wb = 1.0;
        return;
    }
    if (d1 * d4 - d3 * d2 <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
        wa = 1.0 - v, wb = v;
        return;
    }
    const double cp[3] = {x - p[6], y - p[7], z - p[8]};
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) {
        wa = 0.0, wc = 1.0;
        return;
    }
    if (d5 * d2 - d1 * d6 <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double w = d2 / (d2 - d6);
        wa = 1.0 - w, wc = w;
        return;
    }
    if (d3 * d6 - d5 * d4 <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        wa = 0.0, wb = 1.0 - w, wc = w;
        return;
    }
    const double va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
    const double den = (va + vb) + vc;
    wb = vb / den, wc = vc / den;
    wa = (1.0 - wb) - wc;
}

// row r comes before row w in the order of the turned index triples (two rows never hold the same triple on a checked mesh)
__device__ __forceinline__ bool keyBefore(const MeshTri *table, int r, int w)
{
    const int32_t *a = table[r].v, *b = table[w].v;
    if (a[0] != b[0]) return a[0] < b[0];
    if (a[1] != b[1]) return a[1] < b[1];
    return a[2] < b[2];
}

__global__ __launch_bounds__(kThreads) void meshVelocityKernel(MeshVelocityArgs va)
{
    const MeshArgs &a = va.m;
    const TileThread th;
    const int lane = th.lane, i = th.i, j = th.j, k0 = th.k0;
    // the samples of meshDistanceKernel's thread, and its walk: d^2 by the same expressions, so its minimum is that kernel's
    const double x = samplePos(a.origin[0], a.spacing, min(i, a.nx - 1)), y = samplePos(a.origin[1], a.spacing, min(j, a.ny - 1));
    double z[kTZ], best[kTZ];
    int winner[kTZ];
#pragma unroll
    for (int kk = 0; kk < kTZ; ++kk) {
        z[kk] = samplePos(a.origin[2], a.spacing, min(k0 + kk, a.nz - 1));
        best[kk] = std::numeric_limits<double>::infinity();
        winner[kk] = -1;
    }
    const int bin = (int(blockIdx.z) * a.tilesY + int(blockIdx.y)) * a.tilesX + int(blockIdx.x);
    const int begin = a.offsets[bin], end = a.offsets[bin + 1];
    for (int q = begin; q < end; ++q) {
        const int r = __builtin_amdgcn_readfirstlane(a.list[q]);
        const double *p = a.table[r].p;
        const double ab[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, ac[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
        const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
        const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
#pragma unroll
        for (int kk = 0; kk < kTZ; ++kk) {
            const double d2 = pointTriangle2(p, ab, ac, n, nn, x, y, z[kk]);
            // (an equal d^2 is rare -- a vertex's fan, an edge's pair: only then are the keys read)
            bool take = d2 < best[kk];
            if (d2 == best[kk] && winner[kk] >= 0) take = keyBefore(a.table, r, winner[kk]);
            best[kk] = take ? d2 : best[kk];
            winner[kk] = take ? r : winner[kk];
        }
    }
    if (i >= a.nx || j >= a.ny) return;
#pragma unroll
    for (int kk = 0; kk < kTZ; ++kk) {
        const int k = k0 + kk;
        if (k >= a.nz) break;
        const size_t row = size_t(k) * a.ny + j;
        const double root = sqrt(best[kk]);
        if (a.sdf) {
            const bool in = (a.inside[row * a.words + blockIdx.x] >> lane) & 1ull;
            const double d = fmin(root, a.band);
            a.sdf[row * a.nx + i] = float(in ? -d : d);
        }
        float out[3] = {0.f, 0.f, 0.f};
        if (root < a.band && winner[kk] >= 0) {  // (beyond band the tile's list no longer holds every triangle)
            const MeshTri &T = a.table[winner[kk]];
            double wa, wb, wc;
            closestWeights(T.p, x, y, z[kk], wa, wb, wc);
            const double *Va = va.velocity + 3 * size_t(T.v[0]), *Vb = va.velocity + 3 * size_t(T.v[1]), *Vc = va.velocity + 3 * size_t(T.v[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] = float((wa * Va[c] + wb * Vb[c]) + wc * Vc[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) va.vel[c][row * a.nx + i] = out[c];
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
bool allFinite(const double *v, size_t n)
{
    for (size_t q = 0; q < n; ++q)
        if (!std::isfinite(v[q])) return false;
    return true;
}

std::string edgeName(int32_t a, int32_t b) { return "edge (" + std::to_string(a) + ", " + std::to_string(b) + ")"; }

// What both entries refuse of a mesh.  turned (may be NULL) receives the triangles with the lowest index first
int checkMesh(const char *fn, int vertices, int triangles, const double *xyz, const int32_t *tri, std::vector<int32_t> *turned)
{
    if (vertices < 4 || triangles < 4)
        return refuse(fn, "a closed mesh has at least 4 vertices and 4 triangles (vertices, triangles = " + std::to_string(vertices) + ", " +
                              std::to_string(triangles) + ")");
    if (!xyz || !tri) return refuse(fn, "xyz or tri is NULL");
    if (!allFinite(xyz, size_t(vertices) * 3)) return refuse(fn, "non-finite coordinate");
    const size_t nt = size_t(triangles);
    for (size_t t = 0; t < nt; ++t) {
        const int32_t *v = tri + 3 * t;
        const auto who = [t] { return "triangle " + std::to_string(t) + ": "; };
        for (int q = 0; q < 3; ++q)
            if (v[q] < 0 || v[q] >= vertices) return refuse(fn, who() + "index " + std::to_string(v[q]) + " is out of range");
        if (v[0] == v[1] || v[1] == v[2] || v[2] == v[0]) return refuse(fn, who() + "repeated index");
        const double *a = xyz + 3 * size_t(v[0]), *b = xyz + 3 * size_t(v[1]), *c = xyz + 3 * size_t(v[2]);
        const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
        if (n[0] * n[0] + n[1] * n[1] + n[2] * n[2] == 0.0) return refuse(fn, who() + "zero area");
    }
    // closed and consistently oriented: every directed edge once, its reverse once.  The directed edges a -> b are bucketed by a
    // (a counting sort) and each vertex's few ends sorted, so a count is a search in one short run
    std::vector<size_t> start(size_t(vertices) + 1, 0);
    for (size_t e = 0; e < 3 * nt; ++e) ++start[size_t(tri[e]) + 1];
    for (size_t v = 0; v < size_t(vertices); ++v) start[v + 1] += start[v];
    std::vector<int32_t> ends(3 * nt);
    {
        std::vector<size_t> at(start.begin(), start.end() - 1);
        for (size_t t = 0; t < nt; ++t)
            for (int q = 0; q < 3; ++q) ends[at[size_t(tri[3 * t + size_t(q)])]++] = tri[3 * t + size_t((q + 1) % 3)];
    }
    for (size_t v = 0; v < size_t(vertices); ++v) std::sort(ends.begin() + long(start[v]), ends.begin() + long(start[v + 1]));
    const auto count = [&](int32_t a, int32_t b) {
        const auto range = std::equal_range(ends.begin() + long(start[size_t(a)]), ends.begin() + long(start[size_t(a) + 1]), b);
        return long(range.second - range.first);
    };
    for (size_t t = 0; t < nt; ++t)
        for (int q = 0; q < 3; ++q) {
            const int32_t a = tri[3 * t + size_t(q)], b = tri[3 * t + size_t((q + 1) % 3)];
            const long fwd = count(a, b), rev = count(b, a);
            if (fwd != 1 || rev != 1)
                return refuse(fn, "the mesh is not closed and consistently oriented: " + edgeName(a, b) + " of triangle " + std::to_string(t) + " occurs " +
                                      std::to_string(fwd) + " times and its reverse " + std::to_string(rev) + " times (once each is required)");
        }
    if (turned) {
        turned->resize(3 * nt);
        for (size_t t = 0; t < nt; ++t) {
            const int32_t *v = tri + 3 * t;
            const int first = v[0] < v[1] ? (v[0] < v[2] ? 0 : 2) : (v[1] < v[2] ? 1 : 2);
            for (int q = 0; q < 3; ++q) (*turned)[3 * t + size_t(q)] = v[(first + q) % 3];
        }
    }
    return MGPS_OK;
}

// Volume, centre and inertia about the centre from the signed tetrahedra (r0, a, b, c): with u = a - r0 ... and det = u . (v x w),
// V = det / 6, int x = det / 24 (u + v + w), int x_i x_j = det / 120 (sum of p_i p_j over the corners + S_i S_j), S = u + v + w.
// r0 is the middle of the bounding box, which keeps the shift to the centre of mass small against the body
void massProperties(int vertices, int triangles, const double *xyz, const int32_t *tri, mgps_mass_properties *out)
{
    double lo[3], hi[3], r0[3];
    for (int c = 0; c < 3; ++c) lo[c] = hi[c] = xyz[c];
    for (size_t v = 1; v < size_t(vertices); ++v)
        for (int c = 0; c < 3; ++c) lo[c] = std::min(lo[c], xyz[3 * v + c]), hi[c] = std::max(hi[c], xyz[3 * v + c]);
    for (int c = 0; c < 3; ++c) r0[c] = 0.5 * (lo[c] + hi[c]);
    double vol = 0, first[3] = {0, 0, 0}, second[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (size_t t = 0; t < size_t(triangles); ++t) {
        double p[3][3], s[3];
        for (int q = 0; q < 3; ++q)
            for (int c = 0; c < 3; ++c) p[q][c] = xyz[3 * size_t(tri[3 * t + size_t(q)]) + c] - r0[c];
        const double det = p[0][0] * (p[1][1] * p[2][2] - p[1][2] * p[2][1]) + p[0][1] * (p[1][2] * p[2][0] - p[1][0] * p[2][2]) +
                           p[0][2] * (p[1][0] * p[2][1] - p[1][1] * p[2][0]);
        for (int c = 0; c < 3; ++c) s[c] = p[0][c] + p[1][c] + p[2][c];
        vol += det / 6.0;
        for (int c = 0; c < 3; ++c) first[c] += det / 24.0 * s[c];
        for (int c = 0; c < 3; ++c)
            for (int e = 0; e < 3; ++e) second[c][e] += det / 120.0 * (p[0][c] * p[0][e] + p[1][c] * p[1][e] + p[2][c] * p[2][e] + s[c] * s[e]);
    }
    out->volume = vol;
    double m[3], cov[3][3];
    for (int c = 0; c < 3; ++c) m[c] = first[c] / vol, out->centre[c] = r0[c] + m[c];
    for (int c = 0; c < 3; ++c)
        for (int e = 0; e < 3; ++e) cov[c][e] = second[c][e] - vol * m[c] * m[e];
    const double trace = cov[0][0] + cov[1][1] + cov[2][2];
    for (int c = 0; c < 3; ++c)
        for (int e = 0; e < 3; ++e) out->inertia[3 * c + e] = (c == e ? trace : 0.0) - cov[c][e];
}

int checkedMass(const char *fn, int vertices, int triangles, const double *xyz, const int32_t *tri, mgps_mass_properties *out, std::vector<int32_t> *turned)
{
    if (int rc = checkMesh(fn, vertices, triangles, xyz, tri, turned); rc != MGPS_OK) return rc;
    massProperties(vertices, triangles, xyz, tri, out);
    if (!(out->volume > 0.0)) return refuse(fn, "the signed volume " + std::to_string(out->volume) + " is not positive: inward orientation");
    return MGPS_OK;
}

// the inclusive range [lo, hi] of the samples 0 .. n - 1 of one axis within [from, to], one sample wider on each side than the
// quotient says (its rounding must not lose a sample); false when empty
bool sampleRange(double from, double to, double origin, double spacing, int n, int &lo, int &hi)
{
    const double a = std::floor((from - origin) / spacing) - 1.0, b = std::ceil((to - origin) / spacing) + 1.0;
    if (!(a <= double(n - 1)) || !(b >= 0.0)) return false;
    lo = int(std::max(a, 0.0)), hi = int(std::min(b, double(n - 1)));
    return true;
}

size_t roundUp(size_t v) { return (v + 255) / 256 * 256; }

// One mesh pass: the checks both entries share, the bins, the upload and the three launches.  `velocity` NULL: the signed distance
// alone (meshDistanceKernel); else the third launch is meshVelocityKernel, which writes vel and, where d->sdf is given, the same sdf
int runMesh(const char *fn, const mgps_mesh_desc *d, const double *velocity, float *const vel[3], void *stream)
{
    for (const int n : {d->nx, d->ny, d->nz})
        if (n < 2 || n > kMaxSamples) return refuse(fn, "every sample dimension must lie in 2 .. " + std::to_string(kMaxSamples));
    if (!(d->spacing > 0 && std::isfinite(d->spacing))) return refuse(fn, "the spacing must be positive and finite");
    if (!(d->band > 0 && std::isfinite(d->band))) return refuse(fn, "band must be positive and finite");
    if (!allFinite(d->origin, 3)) return refuse(fn, "non-finite origin");
    std::vector<int32_t> turned;
    mgps_mass_properties mass;
    if (int rc = checkedMass(fn, d->vertices, d->triangles, d->xyz, d->tri, &mass, &turned); rc != MGPS_OK) return rc;
    if (velocity && !allFinite(velocity, size_t(d->vertices) * 3)) return refuse(fn, "non-finite vertex velocity");

    // the bins of every triangle, and from them the lists' offsets
    MeshArgs a{};
    a.nx = d->nx, a.ny = d->ny, a.nz = d->nz, a.triangles = d->triangles;
    a.tilesX = (d->nx + kTX - 1) / kTX, a.tilesY = (d->ny + kTY - 1) / kTY, a.tilesZ = (d->nz + kTZ - 1) / kTZ;
    a.colsY = (d->ny + kCY - 1) / kCY, a.colsZ = (d->nz + kCZ - 1) / kCZ, a.words = a.tilesX;
    for (int c = 0; c < 3; ++c) a.origin[c] = d->origin[c];
    a.spacing = d->spacing, a.band = d->band;
    const int tiles = a.tilesX * a.tilesY * a.tilesZ, binCount = tiles + a.colsY * a.colsZ;
    const int n[3] = {d->nx, d->ny, d->nz}, tile[3] = {kTX, kTY, kTZ}, cols[2] = {kCY, kCZ};
    const size_t nt = size_t(d->triangles);
    std::vector<TriBins> bins(nt);
    std::vector<int64_t> counts(size_t(binCount) + 1, 0);
    for (size_t t = 0; t < nt; ++t) {
        TriBins b{};
        double lo[3], hi[3];
        for (int c = 0; c < 3; ++c) {
            const double p0 = d->xyz[3 * size_t(turned[3 * t]) + c], p1 = d->xyz[3 * size_t(turned[3 * t + 1]) + c], p2 = d->xyz[3 * size_t(turned[3 * t + 2]) + c];
            lo[c] = std::min(p0, std::min(p1, p2)), hi[c] = std::max(p0, std::max(p1, p2));
        }
        int s0[3], s1[3];
        bool near = true, over = true;
        for (int c = 0; c < 3; ++c) near = near && sampleRange(lo[c] - d->band, hi[c] + d->band, d->origin[c], d->spacing, n[c], s0[c], s1[c]);
        if (near) {
            for (int c = 0; c < 3; ++c) b.lo[c] = uint8_t(s0[c] / tile[c]), b.hi[c] = uint8_t(s1[c] / tile[c]);
            b.some[0] = 1;
            for (int z = b.lo[2]; z <= b.hi[2]; ++z)
                for (int y = b.lo[1]; y <= b.hi[1]; ++y)
                    for (int x = b.lo[0]; x <= b.hi[0]; ++x) ++counts[size_t((z * a.tilesY + y) * a.tilesX + x)];
        }
        for (int c = 1; c < 3; ++c) over = over && sampleRange(lo[c], hi[c], d->origin[c], d->spacing, n[c], s0[c], s1[c]);
        if (over) {
            for (int c = 1; c < 3; ++c) b.clo[c - 1] = uint8_t(s0[c] / cols[c - 1]), b.chi[c - 1] = uint8_t(s1[c] / cols[c - 1]);
            b.some[1] = 1;
            for (int z = b.clo[1]; z <= b.chi[1]; ++z)
                for (int y = b.clo[0]; y <= b.chi[0]; ++y) ++counts[size_t(tiles + z * a.colsY + y)];
        }
        bins[t] = b;
    }
    std::vector<int> offsets(size_t(binCount) + 1);
    int64_t total = 0;
    for (int q = 0; q <= binCount; ++q) {
        if (total > int64_t(std::numeric_limits<int>::max())) return refuse(fn, "the tiles' triangle lists have more than 2^31 - 1 entries: sample a smaller box or use a smaller band");
        offsets[size_t(q)] = int(total);
        total += counts[size_t(q)];
    }
    const size_t entries = size_t(offsets[size_t(binCount)]);

    // one block in stream order; the host tables, its first part, go up in one copy
    const size_t xyzBytes = size_t(d->vertices) * 3 * sizeof(double), triBytes = nt * 3 * sizeof(int32_t), binBytes = nt * sizeof(TriBins);
    const size_t offBytes = offsets.size() * sizeof(int);
    const size_t atXyz = 0, atTri = atXyz + roundUp(xyzBytes), atBins = atTri + roundUp(triBytes), atOff = atBins + roundUp(binBytes);
    const size_t atVel = atOff + roundUp(offBytes);  // (the vertex velocities, where given, as the host block's last part)
    const size_t hostBytes = atVel + (velocity ? roundUp(xyzBytes) : 0);
    const size_t atTable = hostBytes, atCursor = atTable + roundUp(nt * sizeof(MeshTri)), atList = atCursor + roundUp(size_t(binCount) * sizeof(int));
    const size_t atInside = atList + roundUp(std::max(entries, size_t(1)) * sizeof(int));
    const size_t bytes = atInside + roundUp(size_t(d->nz) * d->ny * a.words * sizeof(unsigned long long));
    std::vector<unsigned char> stage(hostBytes, 0);
    std::copy_n(reinterpret_cast<const unsigned char *>(d->xyz), xyzBytes, stage.data() + atXyz);
    std::copy_n(reinterpret_cast<const unsigned char *>(turned.data()), triBytes, stage.data() + atTri);
    std::copy_n(reinterpret_cast<const unsigned char *>(bins.data()), binBytes, stage.data() + atBins);
    std::copy_n(reinterpret_cast<const unsigned char *>(offsets.data()), offBytes, stage.data() + atOff);
    if (velocity) std::copy_n(reinterpret_cast<const unsigned char *>(velocity), xyzBytes, stage.data() + atVel);

    const hipStream_t st = static_cast<hipStream_t>(stream);
    return withStreamBlock(fn, st, bytes, stage.data(), hostBytes, [&](void *dev) {
        unsigned char *base = static_cast<unsigned char *>(dev);
        a.xyz = reinterpret_cast<const double *>(base + atXyz), a.tri = reinterpret_cast<const int32_t *>(base + atTri);
        a.bins = reinterpret_cast<const TriBins *>(base + atBins), a.offsets = reinterpret_cast<const int *>(base + atOff);
        a.table = reinterpret_cast<MeshTri *>(base + atTable), a.cursor = reinterpret_cast<int *>(base + atCursor);
        a.list = reinterpret_cast<int *>(base + atList), a.inside = reinterpret_cast<unsigned long long *>(base + atInside);
        a.sdf = d->sdf;
        // (the cursors must start at zero; the lists that follow them are cleared along with them, so that every entry is a triangle)
        if (int rc = hipStatus(fn, hipMemsetAsync(a.cursor, 0, atInside - atCursor, st)); rc != MGPS_OK) return rc;
        meshFillKernel<<<unsigned((nt + kThreads - 1) / kThreads), kThreads, 0, st>>>(a);
        meshSignKernel<<<dim3(unsigned(a.words), unsigned(a.colsY), unsigned(a.colsZ)), kThreads, 0, st>>>(a);
        const dim3 tiles = tileGrid(d->nx, d->ny, d->nz);
        if (velocity) {
            MeshVelocityArgs va{};
            va.m = a, va.velocity = reinterpret_cast<const double *>(base + atVel);
            for (int c = 0; c < 3; ++c) va.vel[c] = vel[c];
            meshVelocityKernel<<<tiles, kThreads, 0, st>>>(va);
        } else {
            meshDistanceKernel<<<tiles, kThreads, 0, st>>>(a);
        }
        return hipStatus(fn, hipGetLastError());
    });
}
}  // namespace

extern "C" {

int mgps_mesh_mass_properties(int vertices, int triangles, const double *xyz, const int32_t *tri, mgps_mass_properties *out)
try {
    const char *fn = "mgps_mesh_mass_properties";
    if (!out) return refuse(fn, "out is NULL");
    return checkedMass(fn, vertices, triangles, xyz, tri, out, nullptr);
}
MGPS_API_CATCH(nullptr)

int mgps_mesh_sample_box(int vertices, const double *xyz, double spacing, double band, int out_n[3], double out_origin[3])
try {
    const char *fn = "mgps_mesh_sample_box";
    if (!xyz || !out_n || !out_origin) return refuse(fn, "xyz, out_n or out_origin is NULL");
    if (vertices < 1) return refuse(fn, "no vertices");
    if (!allFinite(xyz, size_t(vertices) * 3)) return refuse(fn, "non-finite coordinate");
    if (!(spacing > 0 && std::isfinite(spacing))) return refuse(fn, "the spacing must be positive and finite");
    if (!(band > 0 && std::isfinite(band))) return refuse(fn, "band must be positive and finite");
    const double grow = band + spacing;
    int n[3];
    double origin[3];
    for (int c = 0; c < 3; ++c) {
        double lo = xyz[c], hi = xyz[c];
        for (size_t v = 1; v < size_t(vertices); ++v) lo = std::min(lo, xyz[3 * v + c]), hi = std::max(hi, xyz[3 * v + c]);
        origin[c] = lo - grow;
        const double steps = std::ceil((hi + grow - origin[c]) / spacing);
        if (!(steps + 1.0 <= double(kMaxSamples)))
            return refuse(fn, "the box needs more than " + std::to_string(kMaxSamples) + " samples along an axis: choose a larger spacing");
        n[c] = std::max(int(steps) + 1, 2);
    }
    for (int c = 0; c < 3; ++c) out_n[c] = n[c], out_origin[c] = origin[c];
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

int mgps_fields_mesh_sdf(const mgps_mesh_desc *d, void *stream)
try {
    const char *fn = "mgps_fields_mesh_sdf";
    if (!d || d->struct_size != int(sizeof(mgps_mesh_desc))) return refuse(fn, "NULL or struct_size mismatch (mgps_mesh_desc)");
    if (!d->sdf) return refuse(fn, "sdf (output) is NULL");
    return runMesh(fn, d, nullptr, nullptr, stream);
}
MGPS_API_CATCH(nullptr)

int mgps_fields_mesh_sdf_velocity(const mgps_mesh_velocity_desc *d, void *stream)
try {
    const char *fn = "mgps_fields_mesh_sdf_velocity";
    if (!d || d->struct_size != int(sizeof(mgps_mesh_velocity_desc))) return refuse(fn, "NULL or struct_size mismatch (mgps_mesh_velocity_desc)");
    if (!d->velocity) return refuse(fn, "velocity is NULL");
    for (int c = 0; c < 3; ++c)
        if (!d->vel[c]) return refuse(fn, "vel (output): three grids are required");
    mgps_mesh_desc m{};
    m.struct_size = int(sizeof(mgps_mesh_desc));
    m.vertices = d->vertices, m.triangles = d->triangles, m.xyz = d->xyz, m.tri = d->tri;
    m.nx = d->nx, m.ny = d->ny, m.nz = d->nz, m.spacing = d->spacing, m.band = d->band, m.sdf = d->sdf;
    for (int c = 0; c < 3; ++c) m.origin[c] = d->origin[c];
    return runMesh(fn, &m, d->velocity, d->vel, stream);
}
MGPS_API_CATCH(nullptr)
}
