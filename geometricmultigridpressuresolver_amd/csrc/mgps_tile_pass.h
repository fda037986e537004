// What a tiled field pass is made of ("what a tiled field pass is made of"): the pieces that the rasteriser, the
// mesh passes, advection and redistancing share, stated once.  A pass runs over tiles of kTX x kTY x kTZ cells of a box of planes (the
// whole grid, or a slab window [c0, c1) of it, with `halo` planes held on either side), one thread per column of kTZ cells.
// Two parts, in the manner of mgps_slab_call.h: the host part (what the entries refuse before any device work) needs no HIP header
// and runs in tests/cpp/tile_pass_check.cpp; the device and launch part follows behind __HIPCC__.
// The header holds index arithmetic, pointer selection, stores, integer atomics and host code only -- NO floating-point arithmetic:
// each unit's interpolant is pinned bit for bit by its own restatement (redistance without contraction, advection with explicit
// fused multiply-adds, the sampled faces without), and a header is compiled under whatever the including unit sets afterwards.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "mgps_fields.h"
#include "mgps_internal.h"
#include "mgps_slab_call.h"

namespace mgps {

// a wave per x-row of 64 cells: 256 B per request on a cell grid, and the face grids' rows (gx + 1 or gx entries) stay unit stride
constexpr int kTX = 64, kTY = 4, kTZ = 4, kThreads = 256;
constexpr int kMaxTileLayers = 65535;  // a launch grid's y and z dimensions
static_assert(kTX == 64 && kTY * 64 == kThreads && kTY == kTZ, "one wave per row of a tile plane; checkTileExtents states one limit for y and z");

// ---- host part ---------------------------------------------------------------------------------------------------------------------
// The byte ranges of a call's arrays: an array that is written overlaps no other array of the call
struct ArrayRanges {
    struct Range { std::string name; uintptr_t at; size_t bytes; bool written; };
    std::vector<Range> ranges;

    void add(const std::string &name, const void *p, size_t bytes, bool written) { ranges.push_back(Range{name, reinterpret_cast<uintptr_t>(p), bytes, written}); }
    int refuseOverlap(const char *fn) const
    {
        for (size_t p = 0; p < ranges.size(); ++p)
            for (size_t q = p + 1; q < ranges.size(); ++q) {
                const Range &r = ranges[p], &s = ranges[q];
                if (!r.written && !s.written) continue;  // (two arrays that are only read may be one)
                if (r.at < s.at + s.bytes && s.at < r.at + r.bytes) return refuse(fn, r.name + " and " + s.name + " overlap: the pass is out of place");
            }
        return MGPS_OK;
    }
};

// the halo rule: of `halo` planes asked for, those that exist below plane c0 and above plane c1 - 1 of a grid of gz planes are held
inline void haloPlanes(int halo, int c0, int c1, int gz, int &below, int &above)
{
    below = std::min(halo, c0), above = std::min(halo, gz - c1);
}

// the planes held come in arrays of their own: lo (below the window) and hi (above it)
inline int checkHaloArrays(const char *fn, const std::string &loName, const void *lo, int below, const std::string &hiName, const void *hi, int above)
{
    if (below > 0 && !lo) return refuse(fn, loName + " is NULL: " + std::to_string(below) + " halo planes lie below the window");
    if (above > 0 && !hi) return refuse(fn, hiName + " is NULL: " + std::to_string(above) + " halo planes lie above the window");
    return MGPS_OK;
}

// the planes [n0, n1) that a pass over the window [c0, c1) reads, against the planes held: fewer is refused
inline int checkHalo(const char *fn, int c0, int c1, int gz, int halo, int below, int above, int n0, int n1, const std::string &why)
{
    n0 = std::max(n0, 0), n1 = std::min(n1, gz);
    if (c0 - below <= n0 && c1 + above >= n1) return MGPS_OK;
    return refuse(fn, "too few halo planes: halo = " + std::to_string(halo) + " holds the planes " + std::to_string(c0 - below) + " .. " +
                          std::to_string(c1 + above - 1) + ", " + why + " reads " + std::to_string(n0) + " .. " + std::to_string(n1 - 1));
}

// the planes [n0, n1) (not yet cut to the grid) that a pass over the window [c0, c1) reads which looks one plane past its cells: the
// own planes and one either way, or with wholeTiles every tile layer (anchored at plane 0 of the grid) that meets the window, and its rim
inline void planesRead(int c0, int c1, bool wholeTiles, int &n0, int &n1)
{
    n0 = (wholeTiles ? c0 / kTZ * kTZ : c0) - 1, n1 = (wholeTiles ? (c1 + kTZ - 1) / kTZ * kTZ : c1) + 1;
}

// What a window entry refuses of its window: not a window of a layout, a negative halo, a window of another grid than the desc's (a
// desc that is NULL or of another size is left to its own check).  Gives the planes held on either side
template <class Desc>
int checkWindowOf(const char *fn, const mgps_fields_slab *w, const Desc *d, int halo, int &below, int &above)
{
    if (!fieldsSlabWindow(w, fn)) return MGPS_ERR_INVALID_ARGUMENT;
    if (halo < 0) return refuse(fn, "halo = " + std::to_string(halo) + " is negative");
    if (d && d->struct_size == int(sizeof(Desc)) && (w->gx != d->gx || w->gy != d->gy || w->gz != d->gz))
        return refuse(fn, "the window is not one of the desc's extents (gx, gy, gz are the whole grid's in both)");
    haloPlanes(halo, w->c0, w->c1, w->gz, below, above);
    return MGPS_OK;
}

// What every pass refuses of its grid: an extent below 1, and more tile layers along y or z than a launch grid takes.  extraLayer: a
// window off the tile's planes meets one tile layer more than it has planes for (passes over whole-grid tiles)
inline int checkTileExtents(const char *fn, int gx, int gy, int gz, bool extraLayer)
{
    if (gx < 1 || gy < 1 || gz < 1)
        return refuse(fn, "non-positive extent (gx, gy, gz = " + std::to_string(gx) + ", " + std::to_string(gy) + ", " + std::to_string(gz) + ")");
    const int layers = kMaxTileLayers - (extraLayer ? 1 : 0);
    if ((gy - 1) / kTY + 1 > layers || (gz - 1) / kTZ + 1 > layers) return refuse(fn, "more than " + std::to_string(layers * kTZ) + " cells along y or z");
    return MGPS_OK;
}

}  // namespace mgps

// ---- device and launch part --------------------------------------------------------------------------------------------------------
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace mgps {

// the launch grid over the tiles of a box of gx x gy cells and `planes` planes
inline dim3 tileGrid(int gx, int gy, int planes)
{
    return dim3(unsigned((gx + kTX - 1) / kTX), unsigned((gy + kTY - 1) / kTY), unsigned((planes + kTZ - 1) / kTZ));
}

// thread (lane, wave) of the workgroup of tile (i0, j0, k0) owns the column (i, j) and the planes k0 .. k0 + kTZ - 1
struct TileThread {
    int t, lane, wave, i0, j0, k0, i, j;
    __device__ __forceinline__ TileThread()
    {
        t = int(threadIdx.x), lane = t & 63, wave = t >> 6;
        i0 = int(blockIdx.x) * kTX, j0 = int(blockIdx.y) * kTY, k0 = int(blockIdx.z) * kTZ;
        i = i0 + lane, j = j0 + wave;
    }
};

inline int hipStatus(const char *fn, hipError_t e)
{
    if (e == hipSuccess) return MGPS_OK;
    setLastGlobalError(std::string(fn) + ": " + hipGetErrorString(e));
    return MGPS_ERR_HIP;
}

// a store of a streamed tile: the pass does not read its outputs again (measured at 480^3: 9 % of the rasteriser)
template <class T>
__device__ __forceinline__ void put(T *p, T v)
{
    __builtin_nontemporal_store(v, p);
}

// the planes of a grid that the call holds: the window's, and the halo planes below and above it
struct HeldPlanes {
    const float *win, *lo, *hi;
};

// the plane z (held) of a grid of planeElems per plane: [w0, w1) are the window's planes and h0 is the lowest one held, all in the
// whole grid's plane index
__device__ __forceinline__ const float *heldPlane(const HeldPlanes &h, size_t planeElems, int w0, int w1, int h0, int z)
{
    if (z < w0) return h.lo + size_t(z - h0) * planeElems;
    if (z < w1) return h.win + size_t(z - w0) * planeElems;
    return h.hi + size_t(z - w1) * planeElems;
}

// A workgroup's tally of N counts (in LDS).  zeroTally, then a barrier of the kernel's own, then addTally by every thread of the
// workgroup: one LDS atomic per thread that has something, one global atomic per workgroup and count
template <int N>
__device__ __forceinline__ void zeroTally(unsigned int (&tally)[N])
{
    if (int(threadIdx.x) < N) tally[threadIdx.x] = 0;
}
template <int N>
__device__ __forceinline__ void addTally(unsigned int (&tally)[N], const unsigned int (&mine)[N], unsigned long long *counts)
{
#pragma unroll
    for (int q = 0; q < N; ++q)
        if (mine[q]) atomicAdd(&tally[q], mine[q]);
    __syncthreads();
    const int t = int(threadIdx.x);
    if (t < N && tally[t]) atomicAdd(counts + t, (unsigned long long)tally[t]);
}

struct TileBox { int gx, gy, planes; };  // a box's extents on their own
// where cell (i, j, k) of a box of gx x gy cells and `planes` planes and the faces it owns live: its backward face per axis, and the
// forward one (f + step) where the box ends.  The box is anything with gx, gy and planes, read in place: a kernel's arguments (the
// rasteriser) or a TileBox (the sampled faces) -- each the form under which that kernel keeps its code, LABNOTES R14
struct CellFaces {
    size_t c, f[3], step[3];
    bool more[3];
    template <class Box> __device__ __forceinline__ CellFaces(const Box &a, int i, int j, int k)
    {
        c = (size_t(k) * a.gy + j) * a.gx + i;
        f[0] = (size_t(k) * a.gy + j) * (size_t(a.gx) + 1) + i, f[1] = (size_t(k) * (size_t(a.gy) + 1) + j) * a.gx + i, f[2] = c;
        step[0] = 1, step[1] = size_t(a.gx), step[2] = size_t(a.gx) * a.gy;
        more[0] = i == a.gx - 1, more[1] = j == a.gy - 1, more[2] = k == a.planes - 1;
    }
};

// A device block in stream order: `bytes` are allocated, the first hostBytes of them filled from `host` (pageable memory:
// hipMemcpyAsync returns once it is staged), launch(block) runs and the block is released -- no synchronisation here.  Returns the
// launch's status first, the release's second.  Always inlined: behind a call the callable's captures are memory to the caller's host loops
// (the mesh pass: 1.4 % of a call, LABNOTES R14)
template <class Launch>
__attribute__((always_inline)) inline int withStreamBlock(const char *fn, hipStream_t st, size_t bytes, const void *host, size_t hostBytes, Launch &&launch)
{
    void *dev = nullptr;
    if (const hipError_t e = hipMallocAsync(&dev, bytes, st); e != hipSuccess) {
        (void)hipGetLastError();
        setLastGlobalError(std::string(fn) + ": device allocation failed (" + hipGetErrorString(e) + ")");
        return e == hipErrorNoDevice || e == hipErrorInvalidDevice ? MGPS_ERR_NO_DEVICE : MGPS_ERR_ALLOC;
    }
    int rc = hipStatus(fn, hipMemcpyAsync(dev, host, hostBytes, hipMemcpyHostToDevice, st));
    if (rc == MGPS_OK) rc = launch(dev);
    const int freed = hipStatus(fn, hipFreeAsync(dev, st));
    return rc != MGPS_OK ? rc : freed;
}

}  // namespace mgps
#endif
