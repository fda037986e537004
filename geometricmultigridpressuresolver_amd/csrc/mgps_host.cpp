// Host side of the solver: domain expansion, structural checks and the multigrid hierarchy
// (label coarsening, band lists, coarsest-level factorisation).  Pure C++17, no HIP calls, so the
// whole file is exercised by the CPU test-suite.  Reference citations: "Ops.h" =
// Source/HDK_GeometricMultigridOperators.h, "Ops.cpp" = Source/HDK_GeometricMultigridOperators.cpp,
// "MG.cpp" = Source/HDK_GeometricMultigridPoissonSolver.cpp.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>

#include "mgps_internal.h"

namespace mgps {

static std::mutex gErrMutex;
static std::string gLastError = "";

void setLastGlobalError(const std::string &msg)
{
    std::lock_guard<std::mutex> lock(gErrMutex);
    gLastError = msg;
}
const char *lastGlobalError()
{
    std::lock_guard<std::mutex> lock(gErrMutex);
    static thread_local std::string copy;
    copy = gLastError;
    return copy.c_str();
}

namespace {
std::atomic<void *(*)(size_t)> gBigAlloc{nullptr};
std::atomic<void (*)(void *)> gBigFree{nullptr};
constexpr size_t kBigHeader = 64;  // keeps the block 64-byte aligned; word 0 = the function that releases it
}  // namespace
void (*gSetHandleError)(const mgps_solver *h, const char *msg) noexcept = nullptr;

int apiException(const mgps_solver *h) noexcept
{
    int code = MGPS_ERR_INTERNAL;
    const char *text = "unexpected C++ exception at the C ABI";
    char buf[256];
    try {
        throw;
    } catch (const std::bad_alloc &) {
        code = MGPS_ERR_ALLOC;
        text = "out of host memory (std::bad_alloc)";
    } catch (const std::exception &e) {
        std::snprintf(buf, sizeof(buf), "internal error: %s", e.what());
        text = buf;
    } catch (...) {
    }
    if (h && gSetHandleError) gSetHandleError(h, text);
    else {
        try {
            setLastGlobalError(text);
        } catch (...) {
        }
    }
    return code;
}
void *hostBigAlloc(size_t bytes)
{
    void *(*alloc)(size_t) = gBigAlloc.load();
    void (*release)(void *) = gBigFree.load();
    void *raw = (alloc && release) ? alloc(bytes + kBigHeader) : nullptr;
    if (!raw) {
        raw = std::malloc(bytes + kBigHeader);
        release = nullptr;
    }
    if (!raw) throw std::bad_alloc();
    std::memcpy(raw, &release, sizeof(release));
    return static_cast<char *>(raw) + kBigHeader;
}
void hostBigFree(void *p)
{
    if (!p) return;
    void *raw = static_cast<char *>(p) - kBigHeader;
    void (*release)(void *) = nullptr;
    std::memcpy(&release, raw, sizeof(release));
    if (release) release(raw);
    else std::free(raw);
}
void setHostBigAllocator(void *(*alloc)(size_t), void (*release)(void *))
{
    gBigFree = release;
    gBigAlloc = alloc;
}

static int fail(int code, const std::string &msg)
{
    setLastGlobalError(msg);
    return code;
}

static inline int ilog2ceil(int v)
{
    int p = 0;
    while ((1 << p) < v) ++p;
    return p;
}

// MGPS_SETUP_TIMING=1: stage times of the host-side set-up on stderr (tuning aid)
bool setupTimingOn()
{
    static const bool v = getenv("MGPS_SETUP_TIMING") != nullptr;
    return v;
}
struct HostLap {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    static bool on() { return setupTimingOn(); }
    void lap(const char *what)
    {
        if (!on()) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "    host set-up: %-34s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = std::chrono::steady_clock::now();
    }
};

// Threads worth starting: the visible cores capped by the cgroup CPU quota (a GPU box shows every host core
// but grants a share; one thread per visible core there is slower than running serially).
static int hostThreads()
{
    static const int n = [] {
        unsigned hw = std::thread::hardware_concurrency();
        int v = int(hw ? hw : 4);
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char quota[32] = {0};
            long period = 0;
            if (fscanf(f, "%31s %ld", quota, &period) == 2 && period > 0 && quota[0] != 'm') v = std::min(v, std::max(1, int(atol(quota) / period)));
            fclose(f);
        }
        return std::max(1, std::min(v, 64));
    }();
    return n;
}

// ordered parallel collect: fn(begin, end, out) appends the items of [begin, end) to out; the pieces are
// concatenated in range order, so the result equals the serial loop's
template <class T, class F>
static void parallelCollect(int64_t n, int64_t minPerThread, std::vector<T> &result, F fn)
{
    const int nt = int(std::max<int64_t>(1, std::min<int64_t>(hostThreads(), n / std::max<int64_t>(1, minPerThread))));
    std::vector<std::vector<T>> parts{size_t(nt)};
    const int64_t chunk = (n + nt - 1) / nt;
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t) {
        const int64_t b = t * chunk, e = std::min(n, b + chunk);
        if (b >= e) break;
        if (t + 1 < nt && e < n) pool.emplace_back([&, b, e, t] { fn(b, e, parts[size_t(t)]); });
        else fn(b, e, parts[size_t(t)]);
    }
    for (auto &th : pool) th.join();
    size_t total = 0;
    for (auto &v : parts) total += v.size();
    result.clear();
    result.reserve(total);
    for (auto &v : parts) result.insert(result.end(), v.begin(), v.end());
}

// run fn(begin, end) over [0, n) on a handful of host threads
template <class F>
static void parallelFor(int64_t n, F fn, int64_t grain = 1)  // grain: smallest range worth a thread
{
    int nt = int(std::min<int64_t>(hostThreads(), std::max<int64_t>(1, n / std::max<int64_t>(1, grain))));
    if (nt <= 1) {
        fn(int64_t(0), n);
        return;
    }
    std::vector<std::thread> pool;
    const int64_t chunk = (n + nt - 1) / nt;
    for (int t = 0; t < nt; ++t) {
        const int64_t b = t * chunk, e = std::min(n, b + chunk);
        if (b >= e) break;
        pool.emplace_back([=] { fn(b, e); });
    }
    for (auto &th : pool) th.join();
}

// Coarse labels from the 8 children, then BOUNDARY marking (Ops.cpp:23-163).
// Returns false -- before the BOUNDARY marking, which looks at all six neighbours of every INTERIOR cell -- when the
// coarse level has lost its EXTERIOR shell (the reference asserts unitTestExteriorCells on every level, MG.cpp:252):
// the fine grid then carries fewer than 2^level EXTERIOR cells on some side.
static bool coarsenLabels(const HostLevel &fine, HostLevel &coarse)
{
    const Dims fd = fine.d;
    Dims cd;
    cd.nx = fd.nx / 2;
    cd.ny = fd.ny / 2;
    cd.nz = fd.nz / 2;
    coarse.d = cd;
    coarse.labels.resize(cd.cells());
    const uint8_t *fl = fine.labels.data();
    uint8_t *cl = coarse.labels.data();
    parallelFor(cd.nz, [&](int64_t k0, int64_t k1) {
        // row-wise so that the compiler vectorises: the four fine rows of a coarse row are folded first, then pairs along x
        std::vector<uint8_t> dir(size_t(fd.nx)), act(size_t(fd.nx));
        for (int k = int(k0); k < int(k1); ++k)
            for (int j = 0; j < cd.ny; ++j) {
                const uint8_t *r0 = fl + fd.idx(0, 2 * j, 2 * k), *r1 = r0 + fd.nx, *r2 = r0 + size_t(fd.nx) * fd.ny, *r3 = r2 + fd.nx;
                uint8_t *dp = dir.data(), *ap = act.data();
                for (int i = 0; i < fd.nx; ++i) {
                    dp[i] = uint8_t((r0[i] == MGPS_DIRICHLET_CELL) | (r1[i] == MGPS_DIRICHLET_CELL) | (r2[i] == MGPS_DIRICHLET_CELL) |
                                    (r3[i] == MGPS_DIRICHLET_CELL));
                    ap[i] = uint8_t((r0[i] == MGPS_INTERIOR_CELL) | (r0[i] == MGPS_BOUNDARY_CELL) | (r1[i] == MGPS_INTERIOR_CELL) |
                                    (r1[i] == MGPS_BOUNDARY_CELL) | (r2[i] == MGPS_INTERIOR_CELL) | (r2[i] == MGPS_BOUNDARY_CELL) |
                                    (r3[i] == MGPS_INTERIOR_CELL) | (r3[i] == MGPS_BOUNDARY_CELL));
                }
                uint8_t *out = cl + cd.idx(0, j, k);
                for (int i = 0; i < cd.nx; ++i) {
                    const uint8_t dirichlet = dp[2 * i] | dp[2 * i + 1], active = ap[2 * i] | ap[2 * i + 1];
                    out[i] = dirichlet ? uint8_t(MGPS_DIRICHLET_CELL) : (active ? uint8_t(MGPS_INTERIOR_CELL) : uint8_t(MGPS_EXTERIOR_CELL));
                }
            }
    });
    {
        int shell = 0;
        mgps_check_exterior_cells(cl, cd.nx, cd.ny, cd.nz, &shell);
        if (!shell) return false;
    }
    // second pass on a snapshot of "is this neighbour EXTERIOR or DIRICHLET" -- marking only turns
    // INTERIOR into BOUNDARY, neither of which the test looks for, so reading in place is safe
    const ptrdiff_t stride[3] = {1, cd.nx, ptrdiff_t(cd.nx) * cd.ny};
    parallelFor(cd.nz, [&](int64_t k0, int64_t k1) {
        for (int k = int(k0); k < int(k1); ++k)
            for (int j = 0; j < cd.ny; ++j)
                for (int i = 0; i < cd.nx; ++i) {
                    const size_t c = cd.idx(i, j, k);
                    if (cl[c] != MGPS_INTERIOR_CELL) continue;
                    bool bnd = false;
                    for (int a = 0; a < 3 && !bnd; ++a)
                        for (int s = -1; s <= 1; s += 2) {
                            const uint8_t nl = cl[c + s * stride[a]];
                            if (nl == MGPS_EXTERIOR_CELL || nl == MGPS_DIRICHLET_CELL) bnd = true;
                        }
                    if (bnd) cl[c] = MGPS_BOUNDARY_CELL;
                }
    });
    return true;
}

// Band list (Ops.cpp:165-469): BOUNDARY cells plus `width`-1 rings of INTERIOR cells grown
// through face neighbours, ordered by (tile id, k, j, i).
// tk0 / tk1 (slab runs): only the tiles of the z-rows [tk0, tk1] (the rank's window: its slab, the ghost planes and the planes
// its one-exchange band stage reaches); the other tiles get no entries
static void buildBand(HostLevel &L, int width, int tk0 = 0, int tk1 = -1)
{
    // Tile by tile, which is the order of the list: a band cell of a 16^3 tile lies within width-1 steps of a
    // BOUNDARY cell, so the tile plus a halo of width-1 cells decides its part of the list.  Every tile is an
    // independent piece of work for the host threads and the pieces concatenate into the reference order.
    const Dims d = L.d;
    const uint8_t *lab = L.labels.data();
    const int halo = std::max(0, width - 1), E = kTile + 2 * halo, F = E + 2;  // F: one more EXTERIOR layer, no bounds tests
    const int tx = (d.nx + kTile - 1) / kTile, ty = (d.ny + kTile - 1) / kTile, tz = (d.nz + kTile - 1) / kTile;
    const int64_t ntiles = int64_t(tx) * ty * tz;
    L.bandTileStart.assign(size_t(ntiles) + 1, 0);
    int32_t *tileCount = L.bandTileStart.data() + 1;
    if (tk1 < 0 || tk1 >= tz) tk1 = tz - 1;
    tk0 = std::max(0, std::min(tk0, tk1));
    const int64_t tFirst = int64_t(tk0) * tx * ty, tCount = int64_t(tk1 - tk0 + 1) * tx * ty;
    parallelCollect<int32_t>(tCount, 64, L.band, [&](int64_t b0, int64_t e0, std::vector<int32_t> &out) {
        const int64_t b = b0 + tFirst, e = e0 + tFirst;
        // (the outermost layer of blk is never written: it stays EXTERIOR)
        std::vector<uint8_t> blk(size_t(F) * F * F, uint8_t(MGPS_EXTERIOR_CELL)), dist(size_t(F) * F * F);
        std::vector<int32_t> cur, nxt;
        const int off[6] = {-1, 1, -F, F, -F * F, F * F};
        for (int64_t t = b; t < e; ++t) {
            const int ti = int(t % tx), tj = int((t / tx) % ty), tk = int(t / (int64_t(tx) * ty));
            const int oi = ti * kTile - halo - 1, oj = tj * kTile - halo - 1, ok = tk * kTile - halo - 1;  // grid cell of local (0,0,0)
            // the labels of the block; rows without a BOUNDARY cell leave no trace beyond their copy
            cur.clear();
            const int i0 = std::max(0, oi + 1), i1 = std::min(d.nx, oi + 1 + E);
            for (int lk = 1; lk <= E; ++lk)
                for (int lj = 1; lj <= E; ++lj) {
                    uint8_t *row = blk.data() + (size_t(lk) * F + lj) * F;
                    const int j = oj + lj, k = ok + lk;
                    std::memset(row, MGPS_EXTERIOR_CELL, size_t(F));
                    if (j < 0 || j >= d.ny || k < 0 || k >= d.nz) continue;
                    const uint8_t *src = lab + d.idx(i0, j, k);
                    std::memcpy(row + (i0 - oi), src, size_t(i1 - i0));
                    for (int i = i0; i < i1; ++i)
                        if (src[i - i0] == MGPS_BOUNDARY_CELL) cur.push_back(int32_t((size_t(lk) * F + lj) * F + (i - oi)));
                }
            if (cur.empty()) continue;
            std::fill(dist.begin(), dist.end(), uint8_t(255));
            for (int32_t c : cur) dist[size_t(c)] = 0;
            for (int ring = 1; ring < width; ++ring) {
                nxt.clear();
                for (int32_t c : cur)
                    for (int q = 0; q < 6; ++q) {
                        const int32_t n = c + off[q];
                        if (blk[size_t(n)] == MGPS_INTERIOR_CELL && dist[size_t(n)] == 255) {
                            dist[size_t(n)] = uint8_t(ring);
                            nxt.push_back(n);
                        }
                    }
                cur.swap(nxt);
            }
            const size_t before = out.size();
            for (int lk = halo + 1; lk <= halo + kTile; ++lk)
                for (int lj = halo + 1; lj <= halo + kTile; ++lj) {
                    const uint8_t *drow = dist.data() + (size_t(lk) * F + lj) * F;
                    for (int li = halo + 1; li <= halo + kTile; ++li)
                        if (drow[li] != 255) out.push_back(int32_t(d.idx(oi + li, oj + lj, ok + lk)));
                }
            tileCount[t] = int32_t(out.size() - before);
        }
    });
    for (int64_t t = 0; t < ntiles; ++t) L.bandTileStart[size_t(t) + 1] += L.bandTileStart[size_t(t)];
}
static void buildTileBoundaryOffsets(HostLevel &L);
static void buildTileLists(HostLevel &L, int tileZOffset);

// Run length of a level's activity list from the number of active runs of 1024, 256, 64 and 32 cells: the length whose runs
// cost least, cells visited x cost per visited cell.  The costs are measured on the 512^3 cube's fine Jacobi sweep with the
// length forced: 2.41 / 2.46 / 2.72 / 2.94 ps per visited cell -- shorter runs mean more list entries, more
// run ends that fetch their x-neighbour from memory, and waves that gather from eight places.  A shorter length has to win by
// 3 % to be taken.  (The cube keeps 1024-cell runs although 32-cell runs would skip its 33-cell padding: 540 against 528
// V-cycles/s; the reference's free-surface test domain goes to 32: MG-PCG 79.8 / 69.7 / 65.2 ms with 256 / 64 / 32.)
int chooseRunCells(const int64_t nAct[4])
{
    int cells = kRunSizes[0];
    double best = double(nAct[0]) * kRunSizes[0] * runCostFactor(kRunSizes[0]);
    for (int z = 1; z < 4; ++z) {
        const double c = double(nAct[z]) * kRunSizes[z] * runCostFactor(kRunSizes[z]);
        if (c < 0.97 * best) {
            cells = kRunSizes[z];
            best = c;
        }
    }
    return cells;
}

// The activity list of a level (HostLevel::chunks, chunkCells) from the flags of its n runs of runCells cells.
void runListFromFlags(HostLevel &L, const uint8_t *runAct, int64_t nq, int runCells)
{
    const Dims d = L.d;
    L.chunkCells = runCells;
    // Launch order = list order.  Walking the grid plane by plane puts the z+-1 rows a sweep re-reads one
    // whole x-y plane apart -- 1 MiB at 512^2, three arrays of it overflow a chiplet's 4 MiB L2 (measured:
    // 1.36x the algorithmic HBM traffic).  Strips of kStripRows rows walked through all planes keep them a
    // strip (64 KiB) apart instead: the list is ordered by (strip of the run's first cell, run index).
    // Pure locality: any order is correct.
    constexpr int kStripRows = 32;
    const bool strips = size_t(d.nx) * d.ny * sizeof(float) > (size_t(256) << 10) && d.ny > kStripRows;
    const size_t nstrips = strips ? (size_t(d.ny) + kStripRows - 1) / kStripRows : 1;
    const size_t cpr = size_t(runCells);
    // the strip of run q's first cell, for q walking upwards from q0 (no division per run: three of them cost more than
    // everything else in this function)
    struct StripWalk {
        size_t rem, j, cpr, nx, ny;
        bool strips;
        StripWalk(int64_t q0, size_t cpr_, const Dims &d, bool strips_) : cpr(cpr_), nx(size_t(d.nx)), ny(size_t(d.ny)), strips(strips_)
        {
            const size_t c = size_t(q0) * cpr;
            rem = c % nx;
            j = (c / nx) % ny;
        }
        size_t strip() const { return strips ? j / kStripRows : 0; }
        void next()
        {
            rem += cpr;
            while (rem >= nx) {
                rem -= nx;
                if (++j == ny) j = 0;
            }
        }
    };
    // contiguous parts of the run range: counts per (part, strip), offsets strip-major, then every part writes its own
    // (below a few million runs one thread is faster than starting several: measured 1.8 ms per million serially against
    // 2.8-3.2 ms on eight threads here and 25 ms on the GPU box's sixteen)
    const int64_t parts = nq < (int64_t(1) << 22) ? 1 : std::min<int64_t>(int64_t(hostThreads()), nq / (1 << 21));
    const int64_t perPart = (nq + parts - 1) / parts;
    std::vector<int64_t> count(size_t(parts) * nstrips, 0);
    parallelFor(parts, [&](int64_t p0, int64_t p1) {
        for (int64_t p = p0; p < p1; ++p) {
            int64_t *c = count.data() + size_t(p) * nstrips;
            StripWalk w(p * perPart, cpr, d, strips);
            for (int64_t q = p * perPart; q < std::min(nq, (p + 1) * perPart); ++q, w.next())
                if (runAct[size_t(q)]) ++c[w.strip()];
        }
    });
    std::vector<int64_t> at(size_t(parts) * nstrips, 0);
    int64_t run = 0;
    for (size_t sidx = 0; sidx < nstrips; ++sidx)
        for (int64_t p = 0; p < parts; ++p) {
            at[size_t(p) * nstrips + sidx] = run;
            run += count[size_t(p) * nstrips + sidx];
        }
    // The scattered writes (one stream per strip) go to an ordinary buffer that this thread keeps; the list itself is a
    // page-locked block (RawVec above 1 MB) filled by one sequential copy.  Measured at 1024^3 inside the solver process on
    // the GPU box, this function: 23 ms with a fresh std::vector as the target (fresh pages are slow in a process that holds
    // GPU mappings), 7.5 ms writing the streams straight into the page-locked block, against 1.3 ms for the same code in a
    // process without the runtime.
    static thread_local std::vector<int32_t> work;
    if (work.size() < size_t(run)) work.resize(size_t(run));
    int32_t *out = work.data();
    parallelFor(parts, [&](int64_t p0, int64_t p1) {
        for (int64_t p = p0; p < p1; ++p) {
            int64_t *a = at.data() + size_t(p) * nstrips;
            StripWalk w(p * perPart, cpr, d, strips);
            for (int64_t q = p * perPart; q < std::min(nq, (p + 1) * perPart); ++q, w.next())
                if (runAct[size_t(q)]) out[size_t(a[w.strip()]++)] = int32_t(q);
        }
    });
    L.chunks.resize(size_t(run));
    if (run) std::memcpy(L.chunks.data(), out, size_t(run) * sizeof(int32_t));
    if (work.size() > (size_t(16) << 20)) std::vector<int32_t>().swap(work);  // (64 MB and more: give it back)
    // a workgroup takes kChunkCells / chunkCells list entries (one per wavefront, or one per 16 / 8 lanes)
    while (L.chunks.size() % size_t(kChunkCells / L.chunkCells)) L.chunks.push_back(-1);
}

// The same from the flags of the runs of kSegCells cells (the host builder's path): count, choose, fold, list.
void chunkListsFromFlags(HostLevel &L, const uint8_t *segAct, int64_t nseg)
{
    constexpr int kPerChunk = kChunkCells / kSegCells;
    const int64_t ncoarse = (nseg + kPerChunk - 1) / kPerChunk;
    std::atomic<int64_t> nAct[4];
    for (auto &a : nAct) a = 0;
    parallelFor(ncoarse, [&](int64_t b, int64_t e) {
        int64_t cnt[4] = {0, 0, 0, 0};
        for (int64_t q = b; q < e; ++q) {
            const int64_t s0 = q * kPerChunk, s1 = std::min(nseg, s0 + kPerChunk);
            for (int z = 0; z < 4; ++z) {
                const int per = kRunSizes[z] / kSegCells;
                for (int64_t r0 = s0; r0 < s1; r0 += per) {
                    bool any = false;
                    for (int64_t r = r0; r < std::min(s1, r0 + per); ++r) any = any || segAct[size_t(r)];
                    cnt[z] += any;
                }
            }
        }
        for (int z = 0; z < 4; ++z) nAct[z] += cnt[z];
    }, 1 << 12);
    const int64_t counts[4] = {nAct[0].load(), nAct[1].load(), nAct[2].load(), nAct[3].load()};
    const int runCells = chooseRunCells(counts);
    const int per = runCells / kSegCells;
    if (per == 1) {
        runListFromFlags(L, segAct, nseg, runCells);
        return;
    }
    const int64_t nq = (nseg + per - 1) / per;
    std::vector<uint8_t> folded(size_t(nq), 0);
    parallelFor(nq, [&](int64_t b, int64_t e) {
        for (int64_t q = b; q < e; ++q) {
            bool any = false;
            for (int64_t r = q * per; r < std::min(nseg, (q + 1) * per); ++r) any = any || segAct[size_t(r)];
            folded[size_t(q)] = any;
        }
    }, 1 << 14);
    runListFromFlags(L, folded.data(), nq, runCells);
}

// A cut level sends the planes next to its cuts to the neighbours after every full-domain sweep.  Its lists are walked edge
// first -- the runs / plane blocks that touch the kSlabEdgePlanes planes at either end of the slab (the ghost exchange of a band
// stage reads the band closure of that many planes), then the rest, each part in its launch order -- so that a sweep can be
// launched in two parts with the exchange of the first under way while the second runs.  Order is free: same results.
void edgeFirst(HostLevel &L)
{
    const Dims d = L.d;
    const size_t plane = size_t(d.nx) * d.ny;
    const int E = std::min(kSlabEdgePlanes, std::max(1, d.nz / 2));
    {
        const size_t cpr = size_t(L.chunkCells), perGroup = size_t(kChunkCells / L.chunkCells);
        RawVec<int32_t> edge, rest;
        for (int32_t q : L.chunks) {
            if (q < 0) continue;  // padding
            const size_t c0 = size_t(q) * cpr, c1 = std::min(d.cells(), c0 + cpr) - 1;
            const int k0 = int(c0 / plane), k1 = int(c1 / plane);
            (k0 < E || k1 >= d.nz - E ? edge : rest).push_back(q);
        }
        while (edge.size() % perGroup) edge.push_back(-1);
        while (rest.size() % perGroup) rest.push_back(-1);
        L.edgeChunks = int32_t(edge.size());
        L.chunks.swap(edge);
        L.chunks.insert(L.chunks.end(), rest.begin(), rest.end());
    }
    if (L.planeZc) {
        const size_t layer = planeTiles(d.nx, d.ny, d.nz, L.planeZc).layer();
        std::vector<int32_t> edge, rest;
        for (int32_t b : L.planeBlocks) {
            const int bz = int(size_t(b) / layer), k0 = bz * L.planeZc, k1 = std::min(d.nz, k0 + L.planeZc) - 1;
            (k0 < E || k1 >= d.nz - E ? edge : rest).push_back(b);
        }
        L.edgePlaneBlocks = int32_t(edge.size());
        L.planeBlocks.swap(edge);
        L.planeBlocks.insert(L.planeBlocks.end(), rest.begin(), rest.end());
    }
}

// Everything the device needs for the planes [z0, z1) of level G (the whole level when z0 = 0,
// z1 = nz): local labels, band list, cell codes (with one ghost plane of plain labels on each side),
// the operator rows of the general BOUNDARY cells and the Gauss-Seidel tile lists.
//
// Operator rows (Ops.h:208-256, evaluated once): an INTERIOR neighbour contributes -x_n and +1 to the
// diagonal, a BOUNDARY neighbour -w x_n and +w, a DIRICHLET neighbour only +w to the diagonal, an
// EXTERIOR neighbour nothing.  w = 1 on coarse levels (wx == nullptr); otherwise wx / wy / wz are the
// face weights of the slab (wz with the closing face plane).  z0 must be a multiple of 16 so that the
// local 16^3 tiles coincide with the global ones.
void buildSlabLevel(const HostLevel &G, int z0, int z1, const float *wx, const float *wy, const float *wz,
                    HostLevel &L, const float *rowsIn)
{
    HostLap lap;
    const Dims gd = G.d;
    Dims d = gd;
    d.nz = z1 - z0;
    L = HostLevel();
    L.d = d;
    const size_t plane = size_t(gd.nx) * gd.ny;
    const uint8_t *glab = G.labels.data();
    L.ownedLabels = glab + size_t(z0) * plane;
    L.ghostLoLabels = z0 > 0 ? glab + size_t(z0 - 1) * plane : nullptr;
    L.ghostHiLabels = z1 < gd.nz ? glab + size_t(z1) * plane : nullptr;
    // the activity and tile lists only read the labels: they are built beside the band split below
    std::thread listsJob([&L, d, z0] {
        const uint8_t *labels = L.ownedLabels;
        {  // activity lists
            const size_t n = d.cells();
            // flags of the runs of kSegCells cells (eight labels per test: a byte is active iff it is 0 or 3)
            const int64_t nfine = int64_t((n + kSegCells - 1) / kSegCells);
            std::vector<uint8_t> fineAct(size_t(nfine), 0);
            parallelFor(nfine, [&](int64_t b, int64_t e) {
                constexpr uint64_t k01 = 0x0101010101010101ull, k80 = 0x8080808080808080ull;
                for (int64_t q = b; q < e; ++q) {
                    const size_t c0 = size_t(q) * kSegCells, c1 = std::min(n, c0 + kSegCells);
                    bool act = false;
                    size_t c = c0;
                    for (; c + 8 <= c1 && !act; c += 8) {
                        uint64_t v;
                        std::memcpy(&v, labels + c, 8);
                        const uint64_t u = v ^ (k01 * uint64_t(MGPS_BOUNDARY_CELL));
                        act = (((v - k01) & ~v & k80) | ((u - k01) & ~u & k80)) != 0;
                    }
                    for (; c < c1 && !act; ++c) act = isActive(labels[c]);
                    fineAct[size_t(q)] = act;
                }
            }, 1 << 12);
            chunkListsFromFlags(L, fineAct.data(), nfine);
            L.planeBlocks.clear();
            L.planeZc = planeSweepZc(d.nx, d.ny, d.nz);
            if (L.planeZc) {
                const PlaneTiles pt = planeTiles(d.nx, d.ny, d.nz, L.planeZc);
                const int nbx = int(pt.nbx), nbz = int(pt.nbz);
                std::vector<uint8_t> act(pt.count(), 0);
                const int zc = L.planeZc;
                parallelFor(nbz, [&](int64_t b0, int64_t b1) {
                    for (int k = int(b0) * zc; k < std::min(d.nz, int(b1) * zc); ++k)
                        for (int j = 0; j < d.ny; ++j) {
                            const uint8_t *row = labels + d.idx(0, j, k);
                            for (int bx = 0; bx < nbx; ++bx) {
                                uint8_t &a = act[pt.index(bx, j / kPlaneRows, k / zc)];
                                if (a) continue;
                                for (int i = bx * kPlaneCols; i < std::min(d.nx, (bx + 1) * kPlaneCols); ++i)
                                    if (isActive(row[i])) {
                                        a = 1;
                                        break;
                                    }
                            }
                        }
                });
                for (size_t q = 0; q < act.size(); ++q)
                    if (act[q]) L.planeBlocks.push_back(int32_t(q));
            }
        }
        buildTileLists(L, z0 / kTile);
    });
    const ptrdiff_t sy = gd.nx, sz = ptrdiff_t(plane);
    const ptrdiff_t off[6] = {-1, 1, -sy, sy, -sz, sz};

    struct Row {
        float w[6], diag;
        bool simple;
    };
    auto rowOf = [&](size_t gc) {  // gc: global linear index
        Row r{};
        const int i = int(gc % gd.nx), j = int((gc / gd.nx) % gd.ny), k = int(gc / plane) - z0;
        float w[6] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
        if (wx) {
            const size_t fx = (size_t(k) * d.ny + j) * (d.nx + 1) + i;
            const size_t fy = (size_t(k) * (d.ny + 1) + j) * d.nx + i;
            const size_t fz = (size_t(k) * d.ny + j) * d.nx + i;
            w[0] = wx[fx];
            w[1] = wx[fx + 1];
            w[2] = wy[fy];
            w[3] = wy[fy + d.nx];
            w[4] = wz[fz];
            w[5] = wz[fz + plane];
        }
        r.simple = true;
        for (int q = 0; q < 6; ++q) {
            const uint8_t nl = glab[ptrdiff_t(gc) + off[q]];
            if (nl == MGPS_INTERIOR_CELL) {
                r.w[q] = 1.f;
                r.diag += 1.f;
            } else if (nl == MGPS_BOUNDARY_CELL) {
                r.w[q] = w[q];
                r.diag += w[q];
                r.simple &= (w[q] == 1.f);
            } else if (nl == MGPS_DIRICHLET_CELL) {
                r.diag += w[q];
                r.simple &= (w[q] == 1.f);
            }
        }
        r.simple = r.simple && r.diag >= 1.f;  // (no open face: a general row, see evalRow in mgps_setup.hip)
        return r;
    };
    // band of the slab in reference order, then split: general BOUNDARY cells first, the rest after.  Ranges of the
    // global band list are classified by the host threads and stitched together in order.
    const size_t lo = size_t(z0) * plane, hi = size_t(z1) * plane;
    struct Part {
        std::vector<int32_t> band, general, rest;
        std::vector<uint8_t> restDiag, isGeneral;  // isGeneral: per entry of `band`
        std::vector<Row> generalRows;
        size_t boundaryBefore = 0;  // BOUNDARY cells of the slab in earlier ranges (index into rowsIn)
    };
    const int64_t nbandG = int64_t(G.band.size());
    const int nt = int(std::max<int64_t>(1, std::min<int64_t>(hostThreads(), nbandG / (1 << 15))));
    std::vector<Part> parts{size_t(nt)};
    const int64_t per = (nbandG + nt - 1) / nt;
    if (rowsIn) {  // the rows arrive in band order: every range needs the count of BOUNDARY cells before it
        parallelFor(nt, [&](int64_t t0, int64_t t1) {
            for (int64_t t = t0; t < t1; ++t) {
                size_t count = 0;
                for (int64_t q = t * per; q < std::min(nbandG, (t + 1) * per); ++q) {
                    const size_t gc = size_t(G.band[size_t(q)]);
                    count += gc >= lo && gc < hi && glab[gc] == MGPS_BOUNDARY_CELL;
                }
                parts[size_t(t)].boundaryBefore = count;
            }
        });
        size_t run = 0;
        for (auto &p : parts) {
            const size_t mine = p.boundaryBefore;
            p.boundaryBefore = run;
            run += mine;
        }
    }
    parallelFor(nt, [&](int64_t t0, int64_t t1) {
        for (int64_t t = t0; t < t1; ++t) {
            Part &P = parts[size_t(t)];
            size_t nextRowIn = P.boundaryBefore;
            for (int64_t q = t * per; q < std::min(nbandG, (t + 1) * per); ++q) {
                const size_t gc = size_t(G.band[size_t(q)]);
                if (gc < lo || gc >= hi) continue;
                const int32_t c = int32_t(gc - lo);
                P.band.push_back(c);
                bool general = false;
                if (glab[gc] == MGPS_BOUNDARY_CELL) {
                    Row r;
                    if (rowsIn) {
                        const float *src = rowsIn + 8 * nextRowIn++;
                        for (int a = 0; a < 6; ++a) r.w[a] = src[a];
                        r.diag = src[6];
                        r.simple = src[7] != 0.f;
                    } else
                        r = rowOf(gc);
                    if (r.simple) {
                        P.rest.push_back(c);
                        P.restDiag.push_back(uint8_t(int(r.diag)));
                    } else {
                        general = true;
                        P.general.push_back(c);
                        P.generalRows.push_back(r);
                    }
                } else {
                    P.rest.push_back(c);
                    P.restDiag.push_back(6);
                }
                P.isGeneral.push_back(uint8_t(general));
            }
        }
    });
    size_t nGeneral = 0, nRest = 0;
    for (auto &P : parts) {
        nGeneral += P.general.size();
        nRest += P.rest.size();
    }
    L.numBoundary = int32_t(nGeneral);
    L.band.resize(nGeneral + nRest);
    L.bandEntry.resize(nGeneral + nRest);
    L.bandDev.resize(nGeneral + nRest);
    L.bandDiag.assign(nGeneral + nRest, 0);
    std::vector<Row> generalRows(nGeneral);
    {
        std::vector<size_t> gAt(parts.size() + 1, 0), rAt(parts.size() + 1, nGeneral), bAt(parts.size() + 1, 0);
        for (size_t q = 0; q < parts.size(); ++q) {
            gAt[q + 1] = gAt[q] + parts[q].general.size();
            rAt[q + 1] = rAt[q] + parts[q].rest.size();
            bAt[q + 1] = bAt[q] + parts[q].band.size();
        }
        parallelFor(int64_t(parts.size()), [&](int64_t q0, int64_t q1) {
            for (int64_t q = q0; q < q1; ++q) {
                const Part &P = parts[size_t(q)];
                std::copy(P.band.begin(), P.band.end(), L.band.begin() + ptrdiff_t(bAt[size_t(q)]));
                size_t gi = gAt[size_t(q)], ri = rAt[size_t(q)], bi = bAt[size_t(q)];
                for (uint8_t isG : P.isGeneral) L.bandEntry[bi++] = int32_t(isG ? gi++ : ri++);
                std::copy(P.general.begin(), P.general.end(), L.bandDev.begin() + ptrdiff_t(gAt[size_t(q)]));
                std::copy(P.rest.begin(), P.rest.end(), L.bandDev.begin() + ptrdiff_t(rAt[size_t(q)]));
                std::copy(P.restDiag.begin(), P.restDiag.end(), L.bandDiag.begin() + ptrdiff_t(rAt[size_t(q)]));
                std::copy(P.generalRows.begin(), P.generalRows.end(), generalRows.begin() + ptrdiff_t(gAt[size_t(q)]));
            }
        });
    }
    parts.clear();
    if (z0 == 0 && z1 == gd.nz) L.bandTileStart = G.bandTileStart;
    else {  // the slab's own tiles (z0 is a multiple of 16)
        const int tx = (d.nx + kTile - 1) / kTile, ty = (d.ny + kTile - 1) / kTile, tz = (d.nz + kTile - 1) / kTile;
        L.bandTileStart.assign(size_t(tx) * ty * tz + 1, 0);
        for (int32_t c : L.band) {
            const int i = int(size_t(c) % d.nx), j = int((size_t(c) / d.nx) % d.ny), k = int(size_t(c) / plane);
            ++L.bandTileStart[(size_t(k / kTile) * ty + j / kTile) * tx + i / kTile + 1];
        }
        for (size_t t = 0; t + 1 < L.bandTileStart.size(); ++t) L.bandTileStart[t + 1] += L.bandTileStart[t];
    }
    lap.lap("slab level: band split + rows");
    // band cells of the planes a band-only ghost exchange moves (see HostLevel::bandPlane)
    {
        const int planes[4] = {z0, z0 - 1, z1 - 1, z1};
        for (int q = 0; q < 4; ++q) {
            L.bandPlane[q].clear();
            if (planes[q] < 0 || planes[q] >= gd.nz || (z0 == 0 && z1 == gd.nz)) continue;  // (a whole grid exchanges nothing)
            const size_t plo = size_t(planes[q]) * plane, phi = plo + plane;
            for (int32_t gcI : G.band) {
                const size_t gc = size_t(gcI);
                if (gc >= plo && gc < phi) L.bandPlane[q].push_back(int32_t(ptrdiff_t(gc) - ptrdiff_t(lo)));
            }
        }
    }
    lap.lap("slab level: band planes");
    listsJob.join();
    lap.lap("slab level: activity + tile lists (joined)");
    if (!(z0 == 0 && z1 == gd.nz)) edgeFirst(L);
    buildTileBoundaryOffsets(L);
    const size_t nb = size_t(L.numBoundary);
    L.rows.assign(7 * nb, 0.f);
    for (size_t t = 0; t < nb; ++t) {
        for (int q = 0; q < 6; ++q) L.rows[q * nb + t] = generalRows[t].w[q];
        L.rows[6 * nb + t] = generalRows[t].diag;
    }
}

#define MGPS_TRY_RC(call)            \
    do {                              \
        const int rc_ = (call);       \
        if (rc_ != MGPS_OK) return rc_; \
    } while (0)

// ---- fused band stage, box form (BandBoxes in mgps_internal.h): host builder ----------------------------------------
// Per 16^3 tile (the tiles that can hold a closure cell: a band cell in the tile or in a face neighbour), a window of the
// tile grown by depth + 2 cells holds per cell: active, band member, band entry.  A stack of sub-boxes of the tile is walked
// left half first: O = bounding box of the sub-box's closure cells (band cells and active cells next to one); every cell of
// O grown by depth + 1 is classified (see BandBoxes), R = bounding box of the classes != 0; a group whose R exceeds the
// workgroup budget is halved along O's longest axis.  The device builder (bandBoxKernel, mgps_setup.hip) walks the same
// recursion and fills the same arrays.
namespace {

struct BoxTileOut {
    std::vector<int32_t> info, general;
    std::vector<uint32_t> list;
};

}  // namespace

void buildBandBoxes(const HostLevel &L, int depth, BandBoxes &out)
{
    out = BandBoxes();
    out.depth = depth;
    if (depth < 1 || depth > kBandMaxDepth || L.band.empty()) return;
    const Dims d = L.d;
    const uint8_t *lab = L.ownedLabels ? L.ownedLabels : L.labels.data();
    const int tx = (d.nx + kTile - 1) / kTile, ty = (d.ny + kTile - 1) / kTile, tz = (d.nz + kTile - 1) / kTile;
    const int64_t nt = int64_t(tx) * ty * tz;
    const int P = depth + 2, E = kTile + 2 * P, E2 = E * E, E3 = E2 * E, D = depth;
    std::vector<BoxTileOut> tiles{size_t(nt)};
    std::atomic<bool> broken{false};
    const int32_t *tstart = L.bandTileStart.data();
    parallelFor(nt, [&](int64_t t0, int64_t t1) {
        std::vector<uint8_t> fl(static_cast<size_t>(E3), 0), cls(static_cast<size_t>(E3), 0);
        std::vector<int32_t> ent(static_cast<size_t>(E3), 0);
        for (int64_t t = t0; t < t1; ++t) {
            const int ti = int(t % tx), tj = int((t / tx) % ty), tk = int(t / (int64_t(tx) * ty));
            auto hasBand = [&](int a, int b, int c) {
                if (a < 0 || b < 0 || c < 0 || a >= tx || b >= ty || c >= tz) return false;
                const size_t q = (size_t(c) * ty + b) * tx + a;
                return tstart[q + 1] > tstart[q];
            };
            if (!(hasBand(ti, tj, tk) || hasBand(ti - 1, tj, tk) || hasBand(ti + 1, tj, tk) || hasBand(ti, tj - 1, tk) || hasBand(ti, tj + 1, tk) ||
                  hasBand(ti, tj, tk - 1) || hasBand(ti, tj, tk + 1)))
                continue;
            const int oi = ti * kTile - P, oj = tj * kTile - P, ok = tk * kTile - P;  // grid cell of window cell (0, 0, 0)
            // window flags: bit 0 active, bit 1 band; ent = band entry (device order) of a band cell
            for (int wk = 0; wk < E; ++wk)
                for (int wj = 0; wj < E; ++wj) {
                    const int gj = oj + wj, gk = ok + wk;
                    const bool rowIn = gj >= 0 && gj < d.ny && gk >= 0 && gk < d.nz;
                    for (int wi = 0; wi < E; ++wi) {
                        const int gi = oi + wi;
                        fl[size_t((wk * E + wj) * E + wi)] = (rowIn && gi >= 0 && gi < d.nx && isActive(lab[d.idx(gi, gj, gk)])) ? 1 : 0;
                    }
                }
            for (int c = tk - 1; c <= tk + 1; ++c)
                for (int b = tj - 1; b <= tj + 1; ++b)
                    for (int a = ti - 1; a <= ti + 1; ++a) {
                        if (a < 0 || b < 0 || c < 0 || a >= tx || b >= ty || c >= tz) continue;
                        const size_t q = (size_t(c) * ty + b) * tx + a;
                        for (int32_t s = tstart[q]; s < tstart[q + 1]; ++s) {
                            const int32_t cell = L.band[size_t(s)];
                            const int wi = cell % d.nx - oi, wj = (cell / d.nx) % d.ny - oj, wk = cell / (d.nx * d.ny) - ok;
                            if (wi < 0 || wj < 0 || wk < 0 || wi >= E || wj >= E || wk >= E) continue;
                            const size_t w = size_t((wk * E + wj) * E + wi);
                            fl[w] |= 2;
                            ent[w] = L.bandEntry[size_t(s)];
                        }
                    }
            const int off[6] = {-1, 1, -E, E, -E2, E2};
            auto closureCell = [&](int w) {  // band cell, or active cell with a band face neighbour (w not on the window's rim)
                if (fl[size_t(w)] & 2) return true;
                if (!(fl[size_t(w)] & 1)) return false;
                for (int q = 0; q < 6; ++q)
                    if (fl[size_t(w + off[q])] & 2) return true;
                return false;
            };
            struct Box {
                int lo[3], hi[3];
            };
            std::vector<Box> stack;
            stack.push_back(Box{{0, 0, 0}, {kTile - 1, kTile - 1, kTile - 1}});
            BoxTileOut &T = tiles[size_t(t)];
            while (!stack.empty()) {
                const Box B = stack.back();
                stack.pop_back();
                int lo[3] = {99, 99, 99}, hi[3] = {-1, -1, -1};
                for (int lk = B.lo[2]; lk <= B.hi[2]; ++lk)
                    for (int lj = B.lo[1]; lj <= B.hi[1]; ++lj)
                        for (int li = B.lo[0]; li <= B.hi[0]; ++li) {
                            if (!closureCell(((lk + P) * E + lj + P) * E + li + P)) continue;
                            const int v[3] = {li, lj, lk};
                            for (int a = 0; a < 3; ++a) {
                                lo[a] = std::min(lo[a], v[a]);
                                hi[a] = std::max(hi[a], v[a]);
                            }
                        }
                if (hi[0] < 0) continue;
                // window coordinates of O and of O grown by depth + 1
                const int olo[3] = {lo[0] + P, lo[1] + P, lo[2] + P}, ohi[3] = {hi[0] + P, hi[1] + P, hi[2] + P};
                const int mlo[3] = {olo[0] - (D + 1), olo[1] - (D + 1), olo[2] - (D + 1)}, mhi[3] = {ohi[0] + D + 1, ohi[1] + D + 1, ohi[2] + D + 1};
                auto ringOf = [&](int wi, int wj, int wk) {
                    const int v[3] = {wi, wj, wk};
                    int r = 0;
                    for (int a = 0; a < 3; ++a) r = std::max(r, std::max(olo[a] - v[a], v[a] - ohi[a]));
                    return r;
                };
                const int dI[6] = {-1, 1, 0, 0, 0, 0}, dJ[6] = {0, 0, -1, 1, 0, 0}, dK[6] = {0, 0, 0, 0, -1, 1};
                for (int wk = mlo[2]; wk <= mhi[2]; ++wk)
                    for (int wj = mlo[1]; wj <= mhi[1]; ++wj)
                        for (int wi = mlo[0]; wi <= mhi[0]; ++wi) {
                            const int w = (wk * E + wj) * E + wi;
                            const uint8_t f = fl[size_t(w)];
                            uint8_t c = kBoxSkip;
                            if (f & 2) c = kBoxGeneral;  // band cell (its code is looked up when the group is written)
                            else {
                                int best = 99;  // smallest ring among the band face neighbours
                                for (int q = 0; q < 6; ++q)
                                    if (fl[size_t(w + off[q])] & 2) best = std::min(best, ringOf(wi + dI[q], wj + dJ[q], wk + dK[q]));
                                if (f & 1) {
                                    if (best < 99 && ringOf(wi, wj, wk) == 0) c = kBoxFrozenOut;
                                    else if (best <= D - 1) c = kBoxFrozen;
                                    else if (best <= D) c = kBoxFrozenFar;
                                } else if (best <= D)
                                    c = kBoxZero;
                            }
                            cls[size_t(w)] = c;
                        }
                // active cells next to a closure-output cell: read by the closure pass
                for (int wk = mlo[2]; wk <= mhi[2]; ++wk)
                    for (int wj = mlo[1]; wj <= mhi[1]; ++wj)
                        for (int wi = mlo[0]; wi <= mhi[0]; ++wi) {
                            const int w = (wk * E + wj) * E + wi;
                            if (cls[size_t(w)] != kBoxSkip || !(fl[size_t(w)] & 1)) continue;
                            for (int q = 0; q < 6; ++q) {
                                const int ni = wi + dI[q], nj = wj + dJ[q], nk = wk + dK[q];
                                if (ni < mlo[0] || ni > mhi[0] || nj < mlo[1] || nj > mhi[1] || nk < mlo[2] || nk > mhi[2]) continue;
                                if (cls[size_t(w + off[q])] == kBoxFrozenOut) {
                                    cls[size_t(w)] = kBoxFrozenFar;  // (only class 11 seeds: no cascade inside this sweep)
                                    break;
                                }
                            }
                        }
                int rlo[3] = {99, 99, 99}, rhi[3] = {-1, -1, -1}, gen = 0, listed = 0;
                for (int wk = mlo[2]; wk <= mhi[2]; ++wk)
                    for (int wj = mlo[1]; wj <= mhi[1]; ++wj)
                        for (int wi = mlo[0]; wi <= mhi[0]; ++wi) {
                            const size_t w = size_t((wk * E + wj) * E + wi);
                            if (cls[w] == kBoxSkip) continue;
                            ++listed;
                            const int v[3] = {wi, wj, wk};
                            for (int a = 0; a < 3; ++a) {
                                rlo[a] = std::min(rlo[a], v[a]);
                                rhi[a] = std::max(rhi[a], v[a]);
                            }
                            if ((fl[w] & 2) && L.bandDiag[size_t(ent[w])] == 0 && ringOf(wi, wj, wk) <= D) ++gen;
                        }
                const int rx = rhi[0] - rlo[0] + 1, ry = rhi[1] - rlo[1] + 1, rz = rhi[2] - rlo[2] + 1, nodes = rx * ry * rz;
                if (nodes > kBoxMaxNodes || listed > kBoxMaxList || gen > kBoxMaxGeneral) {
                    int axis = 0;
                    for (int a = 1; a < 3; ++a)
                        if (hi[a] - lo[a] > hi[axis] - lo[axis]) axis = a;
                    if (hi[axis] == lo[axis]) {  // a single cell cannot exceed the budget
                        broken = true;
                        return;
                    }
                    const int mid = (lo[axis] + hi[axis] + 1) / 2;
                    Box Lh, Rh;
                    for (int a = 0; a < 3; ++a) {
                        Lh.lo[a] = Rh.lo[a] = lo[a];
                        Lh.hi[a] = Rh.hi[a] = hi[a];
                    }
                    Lh.hi[axis] = mid - 1;
                    Rh.lo[axis] = mid;
                    stack.push_back(Rh);  // the left half is walked first
                    stack.push_back(Lh);
                    continue;
                }
                if (rx > 31 || ry > 31 || rz > 31) {  // (5 bits per coordinate; O grown by depth + 1 is at most 26 wide)
                    broken = true;
                    return;
                }
                // Lists in region order (k, j, i) per category: band cells by ring 0 .. depth, closure-output cells, what the
                // plain mode reads besides, what only the closure mode reads
                enum { kCatOut = kBandMaxDepth + 1, kCatReadPlain, kCatReadFar, kCats };
                auto catOf = [&](int wi, int wj, int wk, bool &zero) {
                    const size_t w = size_t((wk * E + wj) * E + wi);
                    zero = false;
                    const uint8_t c = cls[w];
                    if (c == kBoxSkip) return -1;
                    if (fl[w] & 2) {
                        const int ring = ringOf(wi, wj, wk);
                        return ring <= D ? ring : int(kCatReadFar);
                    }
                    if (c == kBoxFrozenOut) return int(kCatOut);
                    if (c == kBoxFrozenFar) return int(kCatReadFar);
                    zero = c == kBoxZero;
                    return int(kCatReadPlain);
                };
                int count[kCats] = {0};
                for (int wk = rlo[2]; wk <= rhi[2]; ++wk)
                    for (int wj = rlo[1]; wj <= rhi[1]; ++wj)
                        for (int wi = rlo[0]; wi <= rhi[0]; ++wi) {
                            bool zero;
                            const int c = catOf(wi, wj, wk, zero);
                            if (c >= 0) ++count[c];
                        }
                const int listBase = int(T.list.size());
                int cum[kBandMaxDepth + 1], total = 0;
                {
                    int run = 0;
                    for (int r = 0; r <= kBandMaxDepth; ++r) {
                        run += count[r];
                        cum[r] = run;
                    }
                    for (int q = 0; q < kCats; ++q) total += count[q];
                }
                const int32_t origin = int32_t(d.idx(oi + rlo[0], oj + rlo[1], ok + rlo[2]));
                const int32_t inf[kBoxInfoInts] = {origin, rx | (ry << 8) | (rz << 16), listBase, 0, int32_t(T.general.size() / 2), gen, 0, total,
                                                   cum[0], cum[1], cum[2], cum[3], cum[4], count[kCatOut],
                                                   (olo[0] - rlo[0]) | ((olo[1] - rlo[1]) << 8) | ((olo[2] - rlo[2]) << 16),
                                                   (ohi[0] - olo[0] + 1) | ((ohi[1] - olo[1] + 1) << 8) | ((ohi[2] - olo[2] + 1) << 16)};
                T.info.insert(T.info.end(), inf, inf + kBoxInfoInts);
                for (int wk = rlo[2]; wk <= rhi[2]; ++wk)
                    for (int wj = rlo[1]; wj <= rhi[1]; ++wj)
                        for (int wi = rlo[0]; wi <= rhi[0]; ++wi) {
                            bool zero;
                            const int c = catOf(wi, wj, wk, zero);
                            if (c < 0) continue;
                            const size_t w = size_t((wk * E + wj) * E + wi);
                            const uint32_t coords = uint32_t(wi - rlo[0]) | (uint32_t(wj - rlo[1]) << 5) | (uint32_t(wk - rlo[2]) << 10);
                            uint32_t code = c == kCatOut ? uint32_t(kBoxFrozenOut) : c == kCatReadFar ? uint32_t(kBoxFrozenFar) : zero ? uint32_t(kBoxZero) : uint32_t(kBoxFrozen);
                            const uint32_t ring = uint32_t(std::min(ringOf(wi, wj, wk), 7));
                            if (c <= kBandMaxDepth) {
                                const int dg = L.bandDiag[size_t(ent[w])];
                                code = dg == 0 ? uint32_t(kBoxGeneral) : uint32_t(kBoxSimple + dg);
                                if (dg == 0) {
                                    T.general.push_back(int32_t(coords | (code << 16) | (ring << 20)));
                                    T.general.push_back(ent[w]);
                                }
                            }
                            T.list.push_back(coords | (code << 16) | (ring << 20));
                        }
            }
        }
    }, 8);
    if (broken) {
        out = BandBoxes();
        out.depth = depth;
        return;
    }
    // concatenate in tile order; the per-tile offsets become global ones
    std::vector<size_t> gAt(size_t(nt) + 1, 0), uAt(size_t(nt) + 1, 0), nAt(size_t(nt) + 1, 0);
    for (int64_t t = 0; t < nt; ++t) {
        gAt[size_t(t) + 1] = gAt[size_t(t)] + tiles[size_t(t)].info.size() / kBoxInfoInts;
        uAt[size_t(t) + 1] = uAt[size_t(t)] + tiles[size_t(t)].list.size();
        nAt[size_t(t) + 1] = nAt[size_t(t)] + tiles[size_t(t)].general.size() / 2;
    }
    out.info.resize(gAt.back() * kBoxInfoInts);
    out.list.resize(uAt.back());
    out.general.resize(nAt.back() * 2);
    parallelFor(nt, [&](int64_t t0, int64_t t1) {
        for (int64_t t = t0; t < t1; ++t) {
            const BoxTileOut &T = tiles[size_t(t)];
            std::copy(T.list.begin(), T.list.end(), out.list.begin() + ptrdiff_t(uAt[size_t(t)]));
            std::copy(T.general.begin(), T.general.end(), out.general.begin() + ptrdiff_t(2 * nAt[size_t(t)]));
            for (size_t g = 0; g < T.info.size() / kBoxInfoInts; ++g) {
                int32_t *dst = out.info.data() + (gAt[size_t(t)] + g) * kBoxInfoInts;
                std::copy(T.info.begin() + ptrdiff_t(g * kBoxInfoInts), T.info.begin() + ptrdiff_t((g + 1) * kBoxInfoInts), dst);
                dst[2] += int32_t(uAt[size_t(t)]);
                dst[4] += int32_t(nAt[size_t(t)]);
            }
        }
    }, 64);
}

// tileZOffset: number of 16-plane tile layers below this slab (the colour uses the global tile index)
static void buildTileLists(HostLevel &L, int tileZOffset)
{
    const Dims d = L.d;
    const int tx = (d.nx + kTile - 1) / kTile, ty = (d.ny + kTile - 1) / kTile, tz = (d.nz + kTile - 1) / kTile;
    // per tile: 0 = no active cell, else (active count << 1) | all-INTERIOR
    std::vector<int64_t> kind;
    parallelCollect<int64_t>(int64_t(tx) * ty * tz, 256, kind, [&](int64_t b, int64_t e, std::vector<int64_t> &out) {
        for (int64_t t = b; t < e; ++t) {
            const int ti = int(t % tx), tj = int((t / tx) % ty), tk = int(t / (int64_t(tx) * ty));
            int64_t active = 0, interior = 0;
            for (int k = tk * kTile; k < std::min(d.nz, (tk + 1) * kTile); ++k)
                for (int j = tj * kTile; j < std::min(d.ny, (tj + 1) * kTile); ++j) {
                    const uint8_t *row = L.ownedLabels + d.idx(0, j, k);
                    for (int i = ti * kTile; i < std::min(d.nx, (ti + 1) * kTile); ++i) {
                        active += isActive(row[i]);
                        interior += (row[i] == MGPS_INTERIOR_CELL);
                    }
                }
            out.push_back((active << 1) | int64_t(interior == int64_t(kTile) * kTile * kTile));
        }
    });
    tileListsFromKinds(L, kind.data(), tileZOffset);
}
// per tile `kind`: 0 = no active cell, else (active cells << 1) | all 4096 cells INTERIOR
template <class K>
void tileListsFromKindsT(HostLevel &L, const K *kind, int tileZOffset)
{
    const Dims d = L.d;
    const int tx = (d.nx + kTile - 1) / kTile, ty = (d.ny + kTile - 1) / kTile, tz = (d.nz + kTile - 1) / kTile;
    for (auto *v : {&L.tilesOdd, &L.tilesEven, &L.pureOdd, &L.pureEven, &L.mixedOdd, &L.mixedEven}) v->clear();
    L.activeCells = 0;
    for (int t = 0; t < tx * ty * tz; ++t) {
        const int64_t active = int64_t(kind[size_t(t)]) >> 1;
        if (!active) continue;
        const int ti = t % tx, tj = (t / tx) % ty, tk = t / (tx * ty);
        L.activeCells += active;
        const bool odd = (ti + tj + tk + tileZOffset) & 1;
        (odd ? L.tilesOdd : L.tilesEven).push_back(t);
        if (kind[size_t(t)] & 1) (odd ? L.pureOdd : L.pureEven).push_back(t);
        else (odd ? L.mixedOdd : L.mixedEven).push_back(t);
    }
}
void tileListsFromKinds(HostLevel &L, const int64_t *kind, int tileZOffset) { tileListsFromKindsT(L, kind, tileZOffset); }
void tileListsFromKinds(HostLevel &L, const int32_t *kind, int tileZOffset) { tileListsFromKindsT(L, kind, tileZOffset); }
static void buildTileBoundaryOffsets(HostLevel &L)
{
    const Dims d = L.d;
    const int tx = (d.nx + kTile - 1) / kTile, ty = (d.ny + kTile - 1) / kTile, tz = (d.nz + kTile - 1) / kTile;
    const int nt = tx * ty * tz;
    L.tileBndStart.assign(size_t(nt) + 1, 0);
    for (int32_t q = 0; q < L.numBoundary; ++q) {
        const size_t c = size_t(L.bandDev[q]);
        const int i = int(c % d.nx), j = int((c / d.nx) % d.ny), k = int(c / (size_t(d.nx) * d.ny));
        const int t = ((k / kTile) * ty + (j / kTile)) * tx + (i / kTile);
        L.tileBndStart[size_t(t) + 1]++;
    }
    for (int t = 0; t < nt; ++t) L.tileBndStart[size_t(t) + 1] += L.tileBndStart[size_t(t)];
}

}  // namespace mgps

using namespace mgps;

// Coarsest system (MG.cpp:288-411): one row per active cell, -1 per active neighbour, diagonal =
// #active + #DIRICHLET neighbours; unknowns numbered tile by tile, x fastest inside a tile.
// Factorised as a banded Cholesky (an exact SPD direct solve like Eigen::SimplicialCholesky).
static int factorCoarseOnHost(mgps_hierarchy &H);
// options.enclosed_liquid: the unknown of the minimum-index cell of every component of the coarsest level's active cells (unit
// coupling: the matrix below) that has no DIRICHLET neighbour -- the null space of the matrix, one constant per such component
static void findCoarsePins(mgps_hierarchy &H)
{
    H.coarsePinned.clear();
    H.coarseComp.clear();
    if (!H.pinEnclosed) return;
    std::vector<size_t> members;
    const HostLevel &L = H.lv[H.levels - 1];
    const Dims d = L.d;
    const ptrdiff_t stride[3] = {1, d.nx, ptrdiff_t(d.nx) * d.ny};
    std::vector<uint8_t> seen(d.cells(), 0);
    std::vector<size_t> stack;
    for (size_t c0 = 0; c0 < d.cells(); ++c0) {  // ascending: c0 is the minimum of the component it starts
        if (seen[c0] || !isActive(L.labels[c0])) continue;
        bool open = false;
        seen[c0] = 1;
        stack.assign(1, c0);
        members.clear();
        while (!stack.empty()) {
            const size_t c = stack.back();
            stack.pop_back();
            members.push_back(c);
            for (int a = 0; a < 3; ++a)
                for (int s = -1; s <= 1; s += 2) {
                    const size_t nb = size_t(ptrdiff_t(c) + s * stride[a]);  // (the EXTERIOR shell keeps nb inside the grid)
                    if (isActive(L.labels[nb])) {
                        if (!seen[nb]) {
                            seen[nb] = 1;
                            stack.push_back(nb);
                        }
                    } else if (L.labels[nb] == MGPS_DIRICHLET_CELL)
                        open = true;
                }
        }
        if (!open) {
            if (H.coarseComp.empty()) H.coarseComp.assign(H.coarseCell.size(), -1);
            for (size_t c : members) H.coarseComp[size_t(H.coarseIndex[c])] = int32_t(H.coarsePinned.size());
            H.coarsePinned.push_back(H.coarseIndex[c0]);
        }
    }
    std::sort(H.coarsePinned.begin(), H.coarsePinned.end());
}

static int buildCoarseSolver(mgps_hierarchy &H, int maxUnknowns)
{
    const HostLevel &L = H.lv[H.levels - 1];
    const Dims d = L.d;
    const size_t n = d.cells();
    H.coarseIndex.assign(n, -1);
    H.coarseCell.clear();
    const int tx = (d.nx + kTile - 1) / kTile, ty = (d.ny + kTile - 1) / kTile, tz = (d.nz + kTile - 1) / kTile;
    for (int t = 0; t < tx * ty * tz; ++t) {
        const int ti = t % tx, tj = (t / tx) % ty, tk = t / (tx * ty);
        for (int k = tk * kTile; k < std::min(d.nz, (tk + 1) * kTile); ++k)
            for (int j = tj * kTile; j < std::min(d.ny, (tj + 1) * kTile); ++j)
                for (int i = ti * kTile; i < std::min(d.nx, (ti + 1) * kTile); ++i)
                    if (isActive(L.labels[d.idx(i, j, k)])) {
                        H.coarseIndex[d.idx(i, j, k)] = int32_t(H.coarseCell.size());
                        H.coarseCell.push_back(int32_t(d.idx(i, j, k)));
                    }
    }
    const int cn = int(H.coarseCell.size());
    H.coarseN = cn;
    findCoarsePins(H);
    if (cn > maxUnknowns)
        return fail(MGPS_ERR_COARSE_TOO_LARGE,
                    "coarsest level has " + std::to_string(cn) + " unknowns (cap " + std::to_string(maxUnknowns) +
                        "): raise mg_levels or options.max_coarse_unknowns");
    const ptrdiff_t stride[3] = {1, d.nx, ptrdiff_t(d.nx) * d.ny};
    int bw = 0;
    if (cn <= kHostCoarseMax)
        for (int r = 0; r < cn; ++r)
            for (int a = 0; a < 3; ++a)
                for (int s = -1; s <= 1; s += 2) {
                    const int q = H.coarseIndex[H.coarseCell[r] + s * stride[a]];
                    if (q >= 0) bw = std::max(bw, std::abs(q - r));
                }
    // The banded factor below costs n x bw^2 on one thread, and the reference's tile numbering makes bw the better part of a tile
    // (thousands) as soon as the level is larger than one 16^3 tile: a 66 x 18 x 16 level with 10 000 unknowns took 30 s here
    // against well under a second for the dense factorisation on the device.  Past kHostCoarseMax unknowns or kHostFactorFlops
    // the solver factorises and inverts on the device (BASELINE configs 3 / 5 as SURVEY 8(d) states them: 512^3 with 5 levels,
    // coarsest 32^3).
    // (the dense inverse the device mat-vec needs is one banded solve per unknown on the host threads: 2 n^2 bw, priced at 5 x the budget)
    H.coarseBW = bw;
    H.coarseOnDevice = cn > kHostCoarseMax || double(cn) * double(bw) * double(bw) > kHostFactorFlops || 2.0 * double(cn) * double(cn) * double(bw) > 5.0 * kHostFactorFlops;
    if (H.coarseOnDevice) {
        H.coarseL.clear();
        return MGPS_OK;
    }
    return factorCoarseOnHost(H);
}

// the banded Cholesky factor of the coarsest matrix (numbering and coarseBW from buildCoarseSolver)
static int factorCoarseOnHost(mgps_hierarchy &H)
{
    const HostLevel &L = H.lv[H.levels - 1];
    const Dims d = L.d;
    const ptrdiff_t stride[3] = {1, d.nx, ptrdiff_t(d.nx) * d.ny};
    const int cn = H.coarseN, bw = H.coarseBW;
    const int W = bw + 1;
    std::vector<double> &A = H.coarseL;
    A.assign(size_t(cn) * W, 0.0);
    auto at = [&](int r, int c) -> double & { return A[size_t(r) * W + (bw - (r - c))]; };
    std::vector<uint8_t> pinned(H.coarsePinned.empty() ? 0 : size_t(cn), 0);
    for (int32_t p : H.coarsePinned) pinned[size_t(p)] = 1;
    for (int r = 0; r < cn; ++r) {
        if (!pinned.empty() && pinned[size_t(r)]) {  // (a pinned unknown: the identity's row and column)
            at(r, r) = 1.0;
            continue;
        }
        double diag = 0;
        for (int a = 0; a < 3; ++a)
            for (int s = -1; s <= 1; s += 2) {
                const size_t nb = H.coarseCell[r] + s * stride[a];
                if (isActive(L.labels[nb])) {
                    const int q = H.coarseIndex[nb];
                    if (q < r && (pinned.empty() || !pinned[size_t(q)])) at(r, q) = -1.0;
                    diag += 1.0;
                } else if (L.labels[nb] == MGPS_DIRICHLET_CELL)
                    diag += 1.0;
            }
        at(r, r) = diag;
    }
    for (int r = 0; r < cn; ++r) {
        const int c0 = std::max(0, r - bw);
        for (int c = c0; c <= r; ++c) {
            double sum = at(r, c);
            for (int m = std::max(c0, c - bw); m < c; ++m) sum -= at(r, m) * at(c, m);
            if (c == r) {
                if (!(sum > 0)) return fail(MGPS_ERR_COARSE_FACTOR, "coarsest-level matrix is not positive definite");
                at(r, r) = std::sqrt(sum);
            } else
                at(r, c) = sum / at(c, c);
        }
    }
    return MGPS_OK;
}

// A coarsest level that the cost rule sent to the device (coarseOnDevice) but that the host can still factorise -- at most
// kHostCoarseMax unknowns: slowly (the reference's tile numbering gives the band a width of thousands), for callers without
// libhipsolver and for the host-only mgps_hierarchy_coarse_solve
namespace mgps {
int hostCoarseFallback(mgps_hierarchy *H)
{
    static std::mutex guard;
    std::lock_guard<std::mutex> lock(guard);
    if (!H->coarseOnDevice) return MGPS_OK;
    if (H->coarseN > kHostCoarseMax)
        return fail(MGPS_ERR_COARSE_TOO_LARGE, "coarsest level has " + std::to_string(H->coarseN) + " unknowns: above " + std::to_string(kHostCoarseMax) +
                                                   " the direct solver needs libhipsolver.so (raise mg_levels)");
    const int rc = factorCoarseOnHost(*H);
    if (rc == MGPS_OK) H->coarseOnDevice = false;
    return rc;
}
}  // namespace mgps

void mgps_hierarchy::bandedSolve(double *v) const
{
    if (coarseOnDevice) return;  // (no host factor: callers check)
    const int n = coarseN, bw = coarseBW, W = bw + 1;
    const double *Lm = coarseL.data();
    for (int32_t p : coarsePinned) v[p] = 0.0;  // (decoupled identity rows: the pinned unknowns come out 0)
    for (int r = 0; r < n; ++r) {
        double sum = v[r];
        for (int c = std::max(0, r - bw); c < r; ++c) sum -= Lm[size_t(r) * W + (bw - (r - c))] * v[c];
        v[r] = sum / Lm[size_t(r) * W + bw];
    }
    for (int r = n - 1; r >= 0; --r) {
        double sum = v[r];
        for (int c = r + 1; c <= std::min(n - 1, r + bw); ++c) sum -= Lm[size_t(c) * W + (bw - (c - r))] * v[c];
        v[r] = sum / Lm[size_t(r) * W + bw];
    }
}

// Dense inverse of the coarsest matrix, one banded solve per unit vector.  On the GPU the direct
// solve is then a single dense mat-vec (n <= a few thousand), which beats two latency-bound banded
// triangular sweeps by orders of magnitude.
void mgps_hierarchy::buildDenseInverse()
{
    if (!coarseInverse.empty() || coarseN == 0 || coarseOnDevice) return;
    const int n = coarseN, bw = coarseBW, W = bw + 1;
    coarseInverse.assign(size_t(n) * n, 0.f);
    // kCols unit vectors per sweep over the factor: the factor (n x W doubles, megabytes) is streamed once per
    // block instead of once per column, and the inner loops vectorise over the block
    constexpr int kCols = 8;
    const int nblocks = (n + kCols - 1) / kCols;
    std::atomic<int> nextBlock{0};
    const int nt = std::min(hostThreads(), std::max(1, nblocks / 4));
    const double *Lm = coarseL.data();
    auto work = [&] {
        std::vector<double> v(size_t(n) * kCols);
        for (;;) {
            const int blk = nextBlock.fetch_add(1);
            if (blk >= nblocks) break;
            const int col0 = blk * kCols, ncol = std::min(kCols, n - col0);
            std::fill(v.begin(), v.end(), 0.0);
            for (int q = 0; q < ncol; ++q) v[size_t(col0 + q) * kCols + q] = 1.0;
            for (int r = col0; r < n; ++r) {  // rows above col0 stay 0 in the forward sweep
                double sum[kCols];
                for (int q = 0; q < kCols; ++q) sum[q] = v[size_t(r) * kCols + q];
                for (int c = std::max(col0, r - bw); c < r; ++c) {
                    const double l = Lm[size_t(r) * W + (bw - (r - c))];
                    for (int q = 0; q < kCols; ++q) sum[q] -= l * v[size_t(c) * kCols + q];
                }
                const double inv = Lm[size_t(r) * W + bw];
                for (int q = 0; q < kCols; ++q) v[size_t(r) * kCols + q] = sum[q] / inv;
            }
            for (int r = n - 1; r >= 0; --r) {
                double sum[kCols];
                for (int q = 0; q < kCols; ++q) sum[q] = v[size_t(r) * kCols + q];
                for (int c = r + 1; c <= std::min(n - 1, r + bw); ++c) {
                    const double l = Lm[size_t(c) * W + (bw - (c - r))];
                    for (int q = 0; q < kCols; ++q) sum[q] -= l * v[size_t(c) * kCols + q];
                }
                const double inv = Lm[size_t(r) * W + bw];
                for (int q = 0; q < kCols; ++q) v[size_t(r) * kCols + q] = sum[q] / inv;
            }
            for (int r = 0; r < n; ++r)
                for (int q = 0; q < ncol; ++q) coarseInverse[size_t(r) * n + col0 + q] = float(v[size_t(r) * kCols + q]);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
    for (int32_t p : coarsePinned) coarseInverse[size_t(p) * n + p] = 0.f;  // (row and column are 0 already: the identity's block)
    projectPinnedInverse(coarseInverse.data(), n, coarseComp, int(coarsePinned.size()));
}

// inv <- (I - Q) inv (I - Q), Q = the mean over each pinned component (the coarse correction of the V-cycle becomes the
// pseudo-inverse).  The pinned inverse is block-diagonal across components, so with w_j = mean over j's component of row j:
// inv_ij -= w_i + w_j - mean(w over the component) for i, j of the same component
void mgps::projectPinnedInverse(float *inv, int n, const std::vector<int32_t> &comp, int ncomp)
{
    if (ncomp == 0 || comp.empty()) return;
    std::vector<double> w(size_t(n), 0.0), T(size_t(ncomp), 0.0);
    std::vector<int64_t> count(size_t(ncomp), 0);
    for (int i = 0; i < n; ++i)
        if (comp[size_t(i)] >= 0) ++count[size_t(comp[size_t(i)])];
    parallelFor(n, [&](int64_t r0, int64_t r1) {
        for (int64_t i = r0; i < r1; ++i) {
            const int c = comp[size_t(i)];
            if (c < 0) continue;
            double s = 0.0;
            for (int k = 0; k < n; ++k)
                if (comp[size_t(k)] == c) s += double(inv[size_t(i) * n + k]);
            w[size_t(i)] = s / double(count[size_t(c)]);
        }
    }, 64);
    for (int i = 0; i < n; ++i)
        if (comp[size_t(i)] >= 0) T[size_t(comp[size_t(i)])] += w[size_t(i)];
    for (int c = 0; c < ncomp; ++c) T[size_t(c)] /= double(count[size_t(c)]);
    parallelFor(n, [&](int64_t r0, int64_t r1) {
        for (int64_t i = r0; i < r1; ++i) {
            const int c = comp[size_t(i)];
            if (c < 0) continue;
            for (int j = 0; j < n; ++j)
                if (comp[size_t(j)] == c) inv[size_t(i) * n + j] = float(double(inv[size_t(i) * n + j]) - w[size_t(i)] - w[size_t(j)] + T[size_t(c)]);
        }
    }, 64);
}

// Fine-level components for options.enclosed_liquid, serial union-find (the checker: the device labelling must match it entry for entry)
void mgps::enclosedComponentsHost(const uint8_t *labels, const float *wx, const float *wy, const float *wz, const Dims &d, std::vector<int32_t> &offsets,
                                  std::vector<int32_t> &cells)
{
    const size_t n = d.cells();
    const float *w[3] = {wx, wy, wz};
    const ptrdiff_t stride[3] = {1, d.nx, ptrdiff_t(d.nx) * d.ny};
    std::vector<int32_t> parent(n, -1);
    auto find = [&](int32_t c) {
        while (parent[size_t(c)] != c) {
            parent[size_t(c)] = parent[size_t(parent[size_t(c)])];
            c = parent[size_t(c)];
        }
        return c;
    };
    for (size_t c = 0; c < n; ++c)
        if (isActive(labels[c])) parent[c] = int32_t(c);
    std::vector<uint8_t> open(n, 0);
    for (int k = 0; k < d.nz; ++k)
        for (int j = 0; j < d.ny; ++j)
            for (int i = 0; i < d.nx; ++i) {
                const size_t c = d.idx(i, j, k);
                const uint8_t lc = labels[c];
                if (!isActive(lc)) continue;
                const int ijk[3] = {i, j, k}, ext[3] = {d.nx, d.ny, d.nz};
                for (int a = 0; a < 3; ++a)
                    for (int p = 0; p < 2; ++p) {
                        if (p ? ijk[a] + 1 >= ext[a] : ijk[a] == 0) continue;
                        const size_t nb = size_t(ptrdiff_t(c) + (p ? stride[a] : -stride[a]));
                        const uint8_t ln = labels[nb];
                        const int fi = i + (a == 0 && p), fj = j + (a == 1 && p), fk = k + (a == 2 && p);  // (face grids: one more entry along a)
                        const float wf = w[a][(size_t(fk) * (d.ny + (a == 1)) + fj) * (d.nx + (a == 0)) + fi];
                        if (lc == MGPS_BOUNDARY_CELL && ln == MGPS_DIRICHLET_CELL && wf > 0.f) open[c] = 1;
                        if (p && isActive(ln) && (lc == MGPS_INTERIOR_CELL || ln == MGPS_INTERIOR_CELL || wf > 0.f)) {
                            int32_t ra = find(int32_t(c)), rb = find(int32_t(nb));
                            if (ra != rb) parent[size_t(std::max(ra, rb))] = std::min(ra, rb);  // the root stays the minimum cell
                        }
                    }
            }
    for (size_t c = 0; c < n; ++c)
        if (parent[c] >= 0 && open[c]) open[size_t(find(int32_t(c)))] = 1;
    std::vector<int32_t> rank(n, -1);
    offsets.assign(1, 0);
    std::vector<int32_t> count;
    for (size_t c = 0; c < n; ++c)
        if (parent[c] == int32_t(c) && !open[c]) {
            rank[c] = int32_t(count.size());
            count.push_back(0);
        }
    for (size_t c = 0; c < n; ++c)
        if (parent[c] >= 0) {
            const int32_t r = rank[size_t(find(int32_t(c)))];
            if (r >= 0) ++count[size_t(r)];
        }
    for (int32_t v : count) offsets.push_back(offsets.back() + v);
    cells.resize(size_t(offsets.back()));
    std::vector<int32_t> at(offsets.begin(), offsets.end() - 1);
    for (size_t c = 0; c < n; ++c)
        if (parent[c] >= 0) {
            const int32_t r = rank[size_t(find(int32_t(c)))];
            if (r >= 0) cells[size_t(at[size_t(r)]++)] = int32_t(c);
        }
}

extern "C" {

void mgps_default_options(mgps_options *opt)
{
    if (!opt) return;
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = int(sizeof(mgps_options));
    opt->band_width = 3;               // MG.cpp:141
    opt->band_iterations = 3;          // MG.cpp:142
    opt->fuse_band_passes = 1;
    opt->deep_band_halo = 1;
    opt->min_cells_per_rank = 1 << 21;
    opt->pcg_fp64_vectors = 2;  // the iterate in fp64 + residual replacement: the reported residual is a true one (+3..9 % solve time; 0 = all fp32)
    opt->jacobi_weight = 2.0f / 3.0f;  // Ops.h:291, 554
    opt->device = -1;
    opt->print_stats = 0;
    opt->max_coarse_unknowns = 32768;  // 32^3: above 8192 the solver factorises on the device
    opt->interrupt = nullptr;
    opt->interrupt_user = nullptr;
    opt->pre_sweeps = 1;   // MG.cpp:466-486
    opt->post_sweeps = 1;  // MG.cpp:740-757
    opt->stencil_path = 0;
}

const char *mgps_status_string(int status)
{
    switch (status) {
        case MGPS_OK: return "ok";
        case MGPS_ERR_INVALID_ARGUMENT: return "invalid argument";
        case MGPS_ERR_NO_DEVICE: return "no HIP device";
        case MGPS_ERR_HIP: return "HIP runtime error";
        case MGPS_ERR_ALLOC: return "allocation failed";
        case MGPS_ERR_HIERARCHY: return "multigrid hierarchy could not be built";
        case MGPS_ERR_COARSE_TOO_LARGE: return "coarsest level too large for the direct solver";
        case MGPS_ERR_COARSE_FACTOR: return "coarsest-level factorisation failed";
        case MGPS_ERR_COMM: return "communication error";
        case MGPS_ERR_INTERNAL: return "internal error (C++ exception caught at the boundary)";
        case MGPS_ERR_INTERRUPTED: return "interrupted";
        default: return "unknown status";
    }
}

int mgps_expanded_layout(int bnx, int bny, int bnz, int levels_in, int power_of_two, int out_dims[3],
                         int *out_offset, int *out_levels)
try {
    if (bnx <= 0 || bny <= 0 || bnz <= 0 || !out_dims || !out_offset || !out_levels)
        return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_expanded_layout: bad arguments");
    int levels = levels_in;
    if (levels <= 0) levels = ilog2ceil(std::min(bnx, std::min(bny, bnz))) - 1;  // Ops.h:1341-1345
    if (levels < 1) levels = 1;
    const int pad = 1 << (levels - 1);  // Ops.h:1349
    const int base[3] = {bnx, bny, bnz};
    for (int a = 0; a < 3; ++a) {
        const int need = base[a] + 2 * pad;
        if (power_of_two)
            out_dims[a] = 1 << ilog2ceil(need);  // Ops.h:1353-1360
        else {
            const int m = 1 << levels;  // every level needs even extents (Ops.h:751-752, Ops.cpp:27-30)
            out_dims[a] = ((need + m - 1) / m) * m;
        }
    }
    *out_offset = pad;
    *out_levels = levels;
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

int mgps_expand_labels(uint8_t *expanded, const uint8_t *base, int bnx, int bny, int bnz, int enx, int eny,
                       int enz, int offset)
try {
    if (!expanded || !base || offset < 0 || enx < bnx + offset || eny < bny + offset || enz < bnz + offset)
        return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_expand_labels: bad arguments");
    const Dims bd{bnx, bny, bnz}, ed{enx, eny, enz};
    std::memset(expanded, MGPS_EXTERIOR_CELL, ed.cells());
    for (int k = 0; k < bnz; ++k)
        for (int j = 0; j < bny; ++j) {
            const uint8_t *src = base + bd.idx(0, j, k);
            uint8_t *dst = expanded + ed.idx(offset, j + offset, k + offset);
            for (int i = 0; i < bnx; ++i)
                if (src[i] != MGPS_EXTERIOR_CELL)
                    dst[i] = (src[i] == MGPS_INTERIOR_CELL) ? MGPS_INTERIOR_CELL : MGPS_DIRICHLET_CELL;
        }
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

int mgps_expand_weights(float *expanded, const float *base, int axis, int bnx, int bny, int bnz, int enx,
                        int eny, int enz, int offset)
try {
    if (!expanded || !base || axis < 0 || axis > 2)
        return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_expand_weights: bad arguments");
    const Dims bf{bnx + (axis == 0), bny + (axis == 1), bnz + (axis == 2)};
    const Dims ef{enx + (axis == 0), eny + (axis == 1), enz + (axis == 2)};
    if (ef.nx < bf.nx + offset || ef.ny < bf.ny + offset || ef.nz < bf.nz + offset)
        return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_expand_weights: expanded grid too small");
    std::memset(expanded, 0, ef.cells() * sizeof(float));
    for (int k = 0; k < bf.nz; ++k)
        for (int j = 0; j < bf.ny; ++j)
            for (int i = 0; i < bf.nx; ++i) {
                const float v = base[bf.idx(i, j, k)];
                if (v > 0) expanded[ef.idx(i + offset, j + offset, k + offset)] = v;
            }
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

static inline size_t faceIndex(const Dims &d, int axis, int i, int j, int k, int plus)
{
    const int fx = d.nx + (axis == 0), fy = d.ny + (axis == 1);
    if (axis == 0) i += plus;
    else if (axis == 1) j += plus;
    else k += plus;
    return (size_t(k) * fy + j) * fx + i;
}

int mgps_set_boundary_labels(uint8_t *labels, const float *wx, const float *wy, const float *wz, int nx, int ny,
                             int nz)
try {
    if (!labels || !wx || !wy || !wz || nx < 3 || ny < 3 || nz < 3)
        return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_set_boundary_labels: bad arguments");
    const Dims d{nx, ny, nz};
    const float *w[3] = {wx, wy, wz};
    const ptrdiff_t stride[3] = {1, nx, ptrdiff_t(nx) * ny};
    parallelFor(nz - 2, [&](int64_t k0, int64_t k1) {
        for (int k = int(k0) + 1; k < int(k1) + 1; ++k)
            for (int j = 1; j < ny - 1; ++j)
                for (int i = 1; i < nx - 1; ++i) {
                    const size_t c = d.idx(i, j, k);
                    if (labels[c] != MGPS_INTERIOR_CELL) continue;
                    bool bnd = false;
                    for (int a = 0; a < 3 && !bnd; ++a)
                        for (int p = 0; p < 2 && !bnd; ++p) {
                            const uint8_t nl = labels[c + (p ? stride[a] : -stride[a])];
                            bnd = (nl == MGPS_DIRICHLET_CELL || nl == MGPS_EXTERIOR_CELL) ||
                                  (w[a][faceIndex(d, a, i, j, k, p)] != 1.0f);
                        }
                    if (bnd) labels[c] = MGPS_BOUNDARY_CELL;
                }
    });
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

int mgps_check_exterior_cells(const uint8_t *labels, int nx, int ny, int nz, int *pass)
try {
    if (!labels || !pass) return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_check_exterior_cells: bad arguments");
    const Dims d{nx, ny, nz};
    *pass = 0;
    auto rowIsExterior = [&](int j, int k, int i0, int i1) {
        const uint8_t *row = labels + d.idx(0, j, k);
        for (int i = i0; i < i1; ++i)
            if (row[i] != MGPS_EXTERIOR_CELL) return false;
        return true;
    };
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j) {
            const bool whole = k == 0 || k == nz - 1 || j == 0 || j == ny - 1;  // a face of the box: every cell of the row
            if (whole ? !rowIsExterior(j, k, 0, nx) : (labels[d.idx(0, j, k)] != MGPS_EXTERIOR_CELL || labels[d.idx(nx - 1, j, k)] != MGPS_EXTERIOR_CELL))
                return MGPS_OK;
        }
    *pass = 1;
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

int mgps_check_boundary_cells(const uint8_t *labels, const float *wx, const float *wy, const float *wz, int nx,
                              int ny, int nz, int *pass)
try {
    if (!labels || !pass) return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_check_boundary_cells: bad arguments");
    const Dims d{nx, ny, nz};
    const float *w[3] = {wx, wy, wz};
    const bool weighted = wx && wy && wz;
    const ptrdiff_t stride[3] = {1, nx, ptrdiff_t(nx) * ny};
    std::atomic<int> ok{1};
    parallelFor(int64_t(std::max(nz - 2, 0)), [&](int64_t k0, int64_t k1) {
        for (int k = int(k0) + 1; k < int(k1) + 1 && ok.load(std::memory_order_relaxed); ++k)
            for (int j = 1; j < ny - 1; ++j)
                for (int i = 1; i < nx - 1; ++i) {
                    const size_t c = d.idx(i, j, k);
                    if (labels[c] == MGPS_INTERIOR_CELL) {
                        for (int a = 0; a < 3; ++a)
                            for (int p = 0; p < 2; ++p)
                                if (!isActive(labels[c + (p ? stride[a] : -stride[a])])) ok = 0;
                    } else if (labels[c] == MGPS_BOUNDARY_CELL) {
                        bool fine = false;
                        for (int a = 0; a < 3; ++a)
                            for (int p = 0; p < 2; ++p) {
                                const uint8_t nl = labels[c + (p ? stride[a] : -stride[a])];
                                if (!isActive(nl)) fine = true;
                                else if (weighted && nl == MGPS_BOUNDARY_CELL && w[a][faceIndex(d, a, i, j, k, p)] != 1.0f)
                                    fine = true;
                            }
                        if (!fine) ok = 0;
                    }
                }
    });
    *pass = ok.load();
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

}  // extern "C"

void mgps::checkInteriorCells(const uint8_t *labels, int nx, int ny, int nz, int *pass)
{
    const Dims d{nx, ny, nz};
    const ptrdiff_t stride[3] = {1, nx, ptrdiff_t(nx) * ny};
    std::atomic<int> ok{1};
    parallelFor(int64_t(std::max(nz - 2, 0)), [&](int64_t k0, int64_t k1) {
        for (int k = int(k0) + 1; k < int(k1) + 1 && ok.load(std::memory_order_relaxed); ++k)
            for (int j = 1; j < ny - 1; ++j)
                for (int i = 1; i < nx - 1; ++i) {
                    const size_t c = d.idx(i, j, k);
                    if (labels[c] != MGPS_INTERIOR_CELL) continue;
                    for (int a = 0; a < 3; ++a)
                        for (int p = 0; p < 2; ++p)
                            if (!isActive(labels[c + (p ? stride[a] : -stride[a])])) ok = 0;
                }
    });
    *pass = ok.load();
}

extern "C" {

int mgps_check_coarsening(const uint8_t *coarse, const uint8_t *fine, int fnx, int fny, int fnz, int *pass)
try {
    if (!coarse || !fine || !pass) return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_check_coarsening: bad arguments");
    const Dims fd{fnx, fny, fnz}, cd{fnx / 2, fny / 2, fnz / 2};
    *pass = 0;
    if ((fnx | fny | fnz | cd.nx | cd.ny | cd.nz) & 1) return MGPS_OK;
    for (int k = 0; k < cd.nz; ++k)
        for (int j = 0; j < cd.ny; ++j)
            for (int i = 0; i < cd.nx; ++i) {
                bool dch = false, ach = false, ech = false;
                for (int c = 0; c < 8; ++c) {
                    const uint8_t l = fine[fd.idx(2 * i + (c & 1), 2 * j + ((c >> 1) & 1), 2 * k + (c >> 2))];
                    dch |= l == MGPS_DIRICHLET_CELL;
                    ach |= isActive(l);
                    ech |= l == MGPS_EXTERIOR_CELL;
                }
                const uint8_t cl = coarse[cd.idx(i, j, k)];
                const bool good = (cl == MGPS_DIRICHLET_CELL) ? dch
                                  : isActive(cl)              ? (!dch && ach)
                                                              : (!dch && !ach && ech);
                if (!good) return MGPS_OK;
            }
    *pass = 1;
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

int mgps_hierarchy_create(mgps_hierarchy **out, int nx, int ny, int nz, const uint8_t *labels, int mg_levels,
                          const mgps_options *opt)
try {
    return mgps::hierarchyCreate(out, nx, ny, nz, labels, mg_levels, opt, false, true);
}
MGPS_API_CATCH(nullptr)

}  // extern "C"

// forceCoarseSolver: factorise the last level even in a one-level hierarchy (the collapsed tail of a
// slab solver can consist of the direct solve alone).  requireShell: insist on the EXTERIOR shell.
// window (slab runs; fine planes [window[0], window[1]) of the rank): band lists only for the tiles the rank's slab builders
// read -- its slab and kSlabWindowMargin planes either side on every level; no coarsest-level factor (the tail builds its own).
// Labels of all levels stay global (the collapse level needs them).  mgps_get_hierarchy completes such a hierarchy on demand.
int mgps::hierarchyCreate(mgps_hierarchy **out, int nx, int ny, int nz, const uint8_t *labels, int mg_levels,
                          const mgps_options *opt, bool forceCoarseSolver, bool requireShell, const int *window)
{
    if (!out) return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_hierarchy_create: out is NULL");
    *out = nullptr;
    mgps_options o;
    mgps_default_options(&o);
    if (opt) {
        if (opt->struct_size != int(sizeof(mgps_options)))
            return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_options.struct_size mismatch: call mgps_default_options first");
        o = *opt;
    }
    if (!labels || mg_levels < 1 || nx < 2 || ny < 2 || nz < 2 || (nx & 1) || (ny & 1) || (nz & 1))
        return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_hierarchy_create: extents must be even and >= 2, mg_levels >= 1");
    if (size_t(nx) * ny * nz > size_t(0x7fffffff))
        return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_hierarchy_create: more than 2^31-1 cells per grid");
    // MG.cpp:159-161: log2(res) + 1 >= mgLevels on every axis; every level must keep even extents
    for (int l = 1; l < mg_levels; ++l)
        if (((nx >> (l - 1)) & 1) || ((ny >> (l - 1)) & 1) || ((nz >> (l - 1)) & 1) || (nx >> l) < 1 || (ny >> l) < 1 ||
            (nz >> l) < 1)
            return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_hierarchy_create: extents are not divisible by 2^(levels-1)");
    if (o.band_width < 1 || o.band_iterations < 0)
        return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_hierarchy_create: band_width >= 1, band_iterations >= 0");
    if (o.enclosed_liquid != 0 && o.enclosed_liquid != 1)
        return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_options.enclosed_liquid must be 0 or 1");

    HostLap lap;
    auto H = new mgps_hierarchy();
    H->bandWidth = o.band_width;
    H->pinEnclosed = o.enclosed_liquid == 1;
    H->lv.resize(mg_levels);
    H->lv[0].d = Dims{nx, ny, nz};
    H->lv[0].labels.resize(H->lv[0].d.cells());
    {
        uint8_t *dst = H->lv[0].labels.data();
        parallelFor(int64_t(H->lv[0].d.cells()), [=](int64_t b, int64_t e) { std::memcpy(dst + b, labels + b, size_t(e - b)); }, 1 << 22);
    }
    {
        int pass = 0;
        mgps_check_exterior_cells(labels, nx, ny, nz, &pass);  // MG.cpp:235
        if (!pass && requireShell) {
            delete H;
            return fail(MGPS_ERR_HIERARCHY, "labels need an EXTERIOR shell on all six sides (unitTestExteriorCells)");
        }
    }
    auto solvable = [](const HostLevel &L) {  // any INTERIOR (0) or BOUNDARY (3) label; eight at a time through the padding
        const uint8_t *p = L.labels.data();
        const size_t n = L.labels.size();
        constexpr uint64_t k01 = 0x0101010101010101ull, k80 = 0x8080808080808080ull;
        size_t c = 0;
        for (; c + 8 <= n; c += 8) {
            uint64_t v;
            std::memcpy(&v, p + c, 8);
            const uint64_t u = v ^ (k01 * uint64_t(MGPS_BOUNDARY_CELL));
            if ((((v - k01) & ~v & k80) | ((u - k01) & ~u & k80)) != 0) return true;
        }
        for (; c < n; ++c)
            if (isActive(p[c])) return true;
        return false;
    };
    if (!solvable(H->lv[0])) {  // MG.cpp:233
        delete H;
        return fail(MGPS_ERR_HIERARCHY, "no INTERIOR or BOUNDARY cell in the domain");
    }
    lap.lap("hierarchy: copy + shell check");
    // the fine level's band list (the largest single piece, MG.cpp:279-281) beside the coarsening chain
    constexpr int kSlabWindowMargin = kBandMaxDepth + 3;  // ghost plane + the closure planes of the one-exchange band stage + one
    auto tileRows = [&](int l, int &tk0, int &tk1) {
        tk0 = 0;
        tk1 = -1;
        if (!window) return;
        tk0 = std::max(0, ((window[0] >> l) - kSlabWindowMargin)) / kTile;
        tk1 = ((window[1] >> l) + kSlabWindowMargin) / kTile;
    };
    H->windowed = window != nullptr;
    int ftk0, ftk1;
    tileRows(0, ftk0, ftk1);
    std::thread fineBand([H, ftk0, ftk1] { buildBand(H->lv[0], H->bandWidth, ftk0, ftk1); });
    int levels = mg_levels;
    int shellLost = 0;
    for (int l = 1; l < levels; ++l) {  // MG.cpp:238-253
        if (!coarsenLabels(H->lv[l - 1], H->lv[l])) {  // MG.cpp:252
            shellLost = l;
            break;
        }
        if (!solvable(H->lv[l])) {
            levels = l - 1;  // the reference drops the last solvable level too (MG.cpp:245)
            break;
        }
    }
    fineBand.join();
    if (shellLost) {
        delete H;
        return fail(MGPS_ERR_HIERARCHY, "level " + std::to_string(shellLost) + " has no EXTERIOR shell (unitTestExteriorCells, MG.cpp:252): " +
                                            std::to_string(mg_levels) + " levels need 2^(levels-1) = " + std::to_string(1 << (mg_levels - 1)) +
                                            " EXTERIOR cells on every side of the solver grid (mgps_expanded_layout pads that much)");
    }
    if (levels < 1) {
        delete H;
        return fail(MGPS_ERR_HIERARCHY, "level cap left no multigrid level (first coarse level has no solvable cell)");
    }
    H->levels = levels;
    H->lv.resize(levels);
    lap.lap("hierarchy: coarsen labels + fine band list");
    for (int l = 1; l < levels; ++l) {
        int tk0, tk1;
        tileRows(l, tk0, tk1);
        buildBand(H->lv[size_t(l)], H->bandWidth, tk0, tk1);  // MG.cpp:279-281
        lap.lap("hierarchy: band list");
    }
    // A one-level hierarchy never reaches the direct solve (applyVCycle returns at MG.cpp:516-517);
    // the reference still factorises the fine matrix there, which serves nothing, so it is skipped.
    const int rc = ((levels > 1 || forceCoarseSolver) && !window) ? buildCoarseSolver(*H, o.max_coarse_unknowns) : MGPS_OK;
    lap.lap("hierarchy: coarse factor");
    if (rc != MGPS_OK) {
        delete H;
        return rc;
    }
    *out = H;
    return MGPS_OK;
}

int mgps::hierarchyLight(mgps_hierarchy **out, int nx, int ny, int nz, int levels, const uint8_t *coarsestLabels, const mgps_options &o,
                         bool needCoarseSolver)
{
    auto H = new mgps_hierarchy();
    H->light = true;
    H->bandWidth = o.band_width;
    H->pinEnclosed = o.enclosed_liquid == 1;
    H->levels = levels;
    H->lv.resize(size_t(levels));
    for (int l = 0; l < levels; ++l) H->lv[size_t(l)].d = Dims{nx >> l, ny >> l, nz >> l};
    HostLevel &C = H->lv[size_t(levels - 1)];
    if (coarsestLabels) {  // (nullptr: a slab rank keeps the extents only)
        C.labels.resize(C.d.cells());
        std::memcpy(C.labels.data(), coarsestLabels, C.d.cells());
    }
    if (needCoarseSolver && coarsestLabels) {
        // A time-stepping caller builds a solver per sub-step and the coarsest labels rarely change between two of them:
        // the last few factorisations and dense inverses (10 ms of host threads at 14^3 unknowns) are kept by label pattern.
        struct Kept {
            Dims d;
            std::vector<uint8_t> labels;
            int n = 0, bw = 0;
            bool pinEnclosed = false;  // (part of the key: the same labels give another matrix with the pins)
            std::vector<int32_t> cell, index, pinned, comp;
            std::vector<double> factor;
            std::vector<float> inverse;
        };
        static std::mutex guard;
        static std::vector<std::shared_ptr<Kept>> kept;  // most recent first
        std::shared_ptr<Kept> hit;
        {
            std::lock_guard<std::mutex> lock(guard);
            for (auto &k : kept)
                if (k->d.nx == C.d.nx && k->d.ny == C.d.ny && k->d.nz == C.d.nz && k->n <= o.max_coarse_unknowns && k->n <= kHostCoarseMax &&
                    k->pinEnclosed == H->pinEnclosed &&
                    std::memcmp(k->labels.data(), coarsestLabels, C.d.cells()) == 0) {
                    hit = k;
                    break;
                }
        }
        if (hit) {
            H->coarseN = hit->n;
            H->coarseBW = hit->bw;
            H->coarseCell = hit->cell;
            H->coarseIndex = hit->index;
            H->coarsePinned = hit->pinned;
            H->coarseComp = hit->comp;
            H->coarseL = hit->factor;
            H->coarseInverse = hit->inverse;
        } else {
            const int rc = buildCoarseSolver(*H, o.max_coarse_unknowns);
            if (rc != MGPS_OK) {
                delete H;
                return rc;
            }
            H->buildDenseInverse();
            if (!H->coarseOnDevice && size_t(H->coarseN) * H->coarseN * sizeof(float) <= (size_t(64) << 20)) {
                auto k = std::make_shared<Kept>();
                k->d = C.d;
                k->labels.assign(coarsestLabels, coarsestLabels + C.d.cells());
                k->n = H->coarseN;
                k->bw = H->coarseBW;
                k->cell = H->coarseCell;
                k->index = H->coarseIndex;
                k->pinEnclosed = H->pinEnclosed;
                k->pinned = H->coarsePinned;
                k->comp = H->coarseComp;
                k->factor = H->coarseL;
                k->inverse = H->coarseInverse;
                std::lock_guard<std::mutex> lock(guard);
                kept.insert(kept.begin(), k);
                if (kept.size() > 4) kept.pop_back();
            }
        }
    }
    *out = H;
    return MGPS_OK;
}

extern "C" {

void mgps_hierarchy_destroy(mgps_hierarchy *hier) { delete hier; }
int mgps_hierarchy_levels(const mgps_hierarchy *hier) { return hier ? hier->levels : 0; }

int mgps_hierarchy_level_dims(const mgps_hierarchy *hier, int level, int out_dims[3])
try {
    if (!hier || level < 0 || level >= hier->levels || !out_dims)
        return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_hierarchy_level_dims: bad arguments");
    out_dims[0] = hier->lv[level].d.nx;
    out_dims[1] = hier->lv[level].d.ny;
    out_dims[2] = hier->lv[level].d.nz;
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

int mgps_hierarchy_level_labels(const mgps_hierarchy *hier, int level, uint8_t *out)
try {
    if (!hier || level < 0 || level >= hier->levels || !out)
        return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_hierarchy_level_labels: bad arguments");
    std::memcpy(out, hier->lv[level].labels.data(), hier->lv[level].labels.size());
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

int64_t mgps_hierarchy_band_count(const mgps_hierarchy *hier, int level)
{
    if (!hier || level < 0 || level >= hier->levels) return -1;
    return int64_t(hier->lv[level].band.size());
}

int mgps_hierarchy_band_cells(const mgps_hierarchy *hier, int level, int32_t *out_ijk)
try {
    if (!hier || level < 0 || level >= hier->levels || !out_ijk)
        return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_hierarchy_band_cells: bad arguments");
    const Dims d = hier->lv[level].d;
    size_t q = 0;
    for (int32_t c : hier->lv[level].band) {
        out_ijk[q++] = c % d.nx;
        out_ijk[q++] = (c / d.nx) % d.ny;
        out_ijk[q++] = c / (d.nx * d.ny);
    }
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

// Host check of the box form of the fused band stage (BandBoxes): builds the level's boxes, verifies their structure (every
// closure cell -- band cell or active face neighbour of one -- in exactly one owned box, regions within the workgroup
// budget, every neighbour a pass reads present in the region) and replays, on a seeded grid, what launchBandBox computes:
//   plain mode    `depth` band passes group by group            == pass by pass over the whole band,
//   closure mode  sweep(x) overwritten on the closure by the groups' depth passes + one Jacobi step
//                                                                == band passes, then the Jacobi sweep,
//   and the plain mode fed from the closure mode's snapshot (the stage after the sweep) == band passes on the sweep's result;
// all bit for bit.  wx / wy / wz (optional, level 0 only): face weights, so that general BOUNDARY cells (operator rows) take
// part; without them the operator has unit weights.
int mgps_hierarchy_check_band_boxes(const mgps_hierarchy *hier, int level, int depth, const float *wx, const float *wy, const float *wz,
                                    int64_t *out_groups, int64_t *out_region_cells, int64_t *out_general)
try {
    if (!hier || level < 0 || level >= hier->levels || depth < 1 || depth > kBandMaxDepth || ((wx || wy || wz) && (level != 0 || !wx || !wy || !wz)))
        return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_hierarchy_check_band_boxes: bad arguments");
    HostLevel L;
    buildSlabLevel(hier->lv[level], 0, hier->lv[level].d.nz, wx, wy, wz, L);
    BandBoxes bx;
    buildBandBoxes(L, depth, bx);
    const Dims d = L.d;
    const size_t n = d.cells(), nband = L.bandDev.size();
    const ptrdiff_t sy = d.nx, sz = ptrdiff_t(d.nx) * d.ny;
    const ptrdiff_t goff[6] = {-1, 1, -sy, sy, -sz, sz};
    if (out_groups) *out_groups = int64_t(bx.groups());
    if (out_region_cells) *out_region_cells = 0;
    if (out_general) *out_general = int64_t(bx.general.size() / 2);
    if (nband == 0) return bx.groups() == 0 ? MGPS_OK : fail(MGPS_ERR_HIERARCHY, "band boxes without band cells");
    if (bx.groups() == 0) return fail(MGPS_ERR_HIERARCHY, "band boxes: builder failed");
    const uint8_t *lab = L.ownedLabels;
    std::vector<int32_t> entryOfCell(n, -1);
    for (size_t t = 0; t < nband; ++t) entryOfCell[size_t(L.bandDev[t])] = int32_t(t);
    auto isBand = [&](ptrdiff_t c) { return entryOfCell[size_t(c)] >= 0; };
    auto isClosure = [&](ptrdiff_t c) {
        if (isBand(c)) return true;
        if (!isActive(lab[c])) return false;
        for (int q = 0; q < 6; ++q)
            if (isBand(c + goff[q])) return true;
        return false;
    };
    // seeded grids
    std::vector<float> x(n, 0.f), b(n, 0.f);
    uint32_t state = 777u + uint32_t(level) * 31u + uint32_t(depth);
    auto rnd = [&] {
        state = state * 1664525u + 1013904223u;
        return float(state >> 8) * (1.f / 16777216.f);
    };
    for (size_t c = 0; c < n; ++c)
        if (isActive(lab[c])) {
            x[c] = rnd();
            b[c] = rnd();
        }
    const float omega = 2.f / 3.f;
    const size_t nb = size_t(L.numBoundary);
    // one damped Jacobi update of cell c from grid v (entry t >= 0: a band cell, general when t < numBoundary; t < 0: INTERIOR)
    auto updateCell = [&](const std::vector<float> &v, ptrdiff_t c, int32_t t) {
        const float xc = v[size_t(c)];
        if (t >= 0 && size_t(t) < nb) {
            const float *r = L.rows.data() + t;
            float acc = 0.f;
            for (int q = 0; q < 6; ++q) acc -= r[size_t(q) * nb] * v[size_t(c + goff[q])];
            const float diag = r[6 * nb], lap = acc + diag * xc;
            return xc + omega * ((b[size_t(c)] - lap) / diag);
        }
        const float diag = t >= 0 ? float(L.bandDiag[size_t(t)]) : 6.f;
        const float lap = diag * xc - (v[size_t(c - 1)] + v[size_t(c + 1)] + v[size_t(c - sy)] + v[size_t(c + sy)] + v[size_t(c - sz)] + v[size_t(c + sz)]);
        return xc + omega * ((b[size_t(c)] - lap) * (1.f / diag));
    };
    auto bandPasses = [&](std::vector<float> &v) {
        std::vector<float> tmp(nband);
        for (int p = 0; p < depth; ++p) {
            for (size_t t = 0; t < nband; ++t) tmp[t] = updateCell(v, L.bandDev[t], int32_t(t));
            for (size_t t = 0; t < nband; ++t) v[size_t(L.bandDev[t])] = tmp[t];
        }
    };
    // the full-domain sweep, out of place: simple cells in line (their diagonal from the labels' neighbours), general ones by row
    auto sweep = [&](const std::vector<float> &v, std::vector<float> &o) {
        o = v;
        for (size_t c = 0; c < n; ++c) {
            if (!isActive(lab[c])) continue;
            int32_t t = entryOfCell[c];
            if (t < 0 && lab[c] != MGPS_INTERIOR_CELL) return false;  // a BOUNDARY cell outside the band cannot be
            o[c] = updateCell(v, ptrdiff_t(c), t);
        }
        return true;
    };
    // reference results
    std::vector<float> refA = x;  // band passes
    bandPasses(refA);
    std::vector<float> refB;      // ... then the sweep
    if (!sweep(refA, refB)) return fail(MGPS_ERR_HIERARCHY, "band boxes: BOUNDARY cell outside the band");
    std::vector<float> refC = refB;  // ... then band passes again
    bandPasses(refC);
    // group replay, as the kernel does it
    std::vector<uint8_t> owned(n, 0);
    int64_t regionCells = 0;
    auto runGroups = [&](bool closure, const std::vector<float> &src, std::vector<float> &dst, std::vector<float> *snap) -> int {
        const int H = depth + (closure ? 1 : 0);
        std::vector<float> v0, v1;
        std::vector<uint8_t> present;
        std::vector<int32_t> rowOf;
        for (size_t gI = 0; gI < bx.groups(); ++gI) {
            const int32_t *gi = bx.info.data() + kBoxInfoInts * gI;
            const int rx = gi[1] & 255, ry = (gi[1] >> 8) & 255, rz = gi[1] >> 16, nodes = rx * ry * rz;
            const int nList = gi[7], ngen = gi[5];
            if (nodes > kBoxMaxNodes || ngen > kBoxMaxGeneral || rx > 31 || ry > 31 || rz > 31 || nList > kBoxMaxList)
                return fail(MGPS_ERR_HIERARCHY, "band box exceeds the workgroup budget");
            const uint32_t *U = bx.list.data() + gi[2];
            auto nodeOf = [&](uint32_t e) { return int((((e >> 10) & 31u) * unsigned(ry) + ((e >> 5) & 31u)) * unsigned(rx) + (e & 31u)); };
            auto cellOf = [&](uint32_t e) { return ptrdiff_t(gi[0]) + ptrdiff_t(e & 31u) + ptrdiff_t((e >> 5) & 31u) * sy + ptrdiff_t((e >> 10) & 31u) * sz; };
            v0.assign(size_t(nodes), NAN);  // (a pass that reads a cell nobody staged propagates the NaN into the comparison)
            present.assign(size_t(nodes), 0);
            rowOf.assign(size_t(nList), -1);
            for (int q = 0; q < ngen; ++q) {
                const uint32_t ge = uint32_t(bx.general[2 * size_t(gi[4] + q)]);
                const int32_t row = bx.general[2 * size_t(gi[4] + q) + 1];
                int k = -1;
                for (int kk = 0; kk < nList && k < 0; ++kk)
                    if (U[kk] == ge) k = kk;
                if (k < 0 || ((ge >> 16) & 15u) != kBoxGeneral || row < 0 || size_t(row) >= nb || L.bandDev[size_t(row)] != cellOf(ge))
                    return fail(MGPS_ERR_HIERARCHY, "band box: general entry does not match its cell");
                rowOf[size_t(k)] = row;
            }
            int ringCount[kBandMaxDepth + 1] = {0}, nOut = 0, lastNode = -1;
            for (int k = 0; k < nList; ++k) {
                const uint32_t e = U[k], cl = (e >> 16) & 15u, ring = e >> 20;
                const int nd = nodeOf(e);
                const ptrdiff_t c = cellOf(e);
                if ((e & 31u) >= unsigned(rx) || ((e >> 5) & 31u) >= unsigned(ry) || ((e >> 10) & 31u) >= unsigned(rz) || c < 0 || size_t(c) >= n || present[size_t(nd)]++ ||
                    nd <= lastNode)
                    return fail(MGPS_ERR_HIERARCHY, "band box: bad list entry");
                lastNode = nd;
                const bool band = cl >= kBoxGeneral && cl <= kBoxSimple + 6, act = isActive(lab[c]);
                if ((cl == kBoxZero) != !act || cl == kBoxSkip || (band && (!isBand(c) || int(ring) > depth)) || (!band && cl != kBoxFrozenFar && isBand(c)) ||
                    (cl == kBoxFrozenOut && ring != 0))
                    return fail(MGPS_ERR_HIERARCHY, "band box: cell class does not match the cell");
                if (band && cl != kBoxGeneral && int(cl) - kBoxSimple != int(L.bandDiag[size_t(entryOfCell[size_t(c)])]))
                    return fail(MGPS_ERR_HIERARCHY, "band box: diagonal mismatch");
                if (band && cl == kBoxGeneral && rowOf[size_t(k)] < 0) return fail(MGPS_ERR_HIERARCHY, "band box: general cell without row");
                if (band)
                    for (int r = int(ring); r <= kBandMaxDepth; ++r) ++ringCount[r];
                nOut += cl == kBoxFrozenOut;
                const bool need = cl != kBoxZero && (closure || cl != kBoxFrozenFar);
                if (need) v0[size_t(nd)] = src[size_t(c)];
                else if (cl == kBoxZero) v0[size_t(nd)] = 0.f;
            }
            for (int r = 0; r <= kBandMaxDepth; ++r)
                if (gi[8 + r] != ringCount[r]) return fail(MGPS_ERR_HIERARCHY, "band box: ring counts");
            if (gi[13] != nOut) return fail(MGPS_ERR_HIERARCHY, "band box: closure-output count");
            v1 = v0;
            const int loff[6] = {-1, 1, -rx, rx, -rx * ry, rx * ry};
            auto nodeUpdate = [&](const std::vector<float> &v, int k) -> float {
                const uint32_t e = U[k], cl = (e >> 16) & 15u;
                const int nd = nodeOf(e);
                const unsigned li = e & 31u, lj = (e >> 5) & 31u, lk = (e >> 10) & 31u;
                if (li == 0 || lj == 0 || lk == 0 || int(li) == rx - 1 || int(lj) == ry - 1 || int(lk) == rz - 1) return NAN;  // an updated cell on the region's rim
                const float xc = v[size_t(nd)], bc = b[size_t(cellOf(e))];
                if (cl == kBoxGeneral) {
                    const float *r = L.rows.data() + rowOf[size_t(k)];
                    float acc = 0.f;
                    for (int q = 0; q < 6; ++q) acc -= r[size_t(q) * nb] * v[size_t(nd + loff[q])];
                    const float diag = r[6 * nb], lap = acc + diag * xc;
                    return xc + omega * ((bc - lap) / diag);
                }
                const float diag = cl == kBoxFrozenOut ? 6.f : float(int(cl) - kBoxSimple);
                const float lap = diag * xc - (v[size_t(nd - 1)] + v[size_t(nd + 1)] + v[size_t(nd - rx)] + v[size_t(nd + rx)] + v[size_t(nd - rx * ry)] + v[size_t(nd + rx * ry)]);
                return xc + omega * ((bc - lap) * (1.f / diag));
            };
            for (int p = 1; p <= H; ++p) {
                const std::vector<float> &s = (p & 1) ? v0 : v1;
                std::vector<float> &o = (p & 1) ? v1 : v0;
                const bool last = closure && p == H;
                for (int k = 0; k < nList; ++k) {
                    const uint32_t cl = (U[k] >> 16) & 15u, ring = U[k] >> 20;
                    const bool band = cl >= kBoxGeneral && cl <= kBoxSimple + 6;
                    if (!((band && int(ring) <= H - p) || (last && cl == kBoxFrozenOut))) continue;
                    const float r = nodeUpdate(s, k);
                    if (r != r) return fail(MGPS_ERR_HIERARCHY, "band box: a pass reads a cell outside its list");
                    o[size_t(nodeOf(U[k]))] = r;
                }
            }
            const std::vector<float> &fin = (H & 1) ? v1 : v0;
            for (int k = 0; k < nList; ++k) {
                const uint32_t cl = (U[k] >> 16) & 15u, ring = U[k] >> 20;
                const bool band = cl >= kBoxGeneral && cl <= kBoxSimple + 6;
                if (ring != 0 || !(band || (closure && cl == kBoxFrozenOut))) continue;
                const ptrdiff_t c = cellOf(U[k]);
                dst[size_t(c)] = fin[size_t(nodeOf(U[k]))];
                if (snap) (*snap)[size_t(c)] = fin[size_t(nodeOf(U[k]))];
                if (closure) ++owned[size_t(c)];
            }
            if (closure) regionCells += nList;
        }
        return MGPS_OK;
    };
    // plain mode, legacy form: out of place from x, band cells copied back
    {
        std::vector<float> scratch = x, got = x;
        MGPS_TRY_RC(runGroups(false, x, scratch, nullptr));
        for (size_t t = 0; t < nband; ++t) got[size_t(L.bandDev[t])] = scratch[size_t(L.bandDev[t])];
        if (got != refA) return fail(MGPS_ERR_HIERARCHY, "band boxes: plain stage differs from pass-by-pass replay");
    }
    // closure mode: y = sweep(x) everywhere, then overwritten on the closure; snapshot = the closure values
    std::vector<float> y, snapshot(n, NAN);
    if (!sweep(x, y)) return fail(MGPS_ERR_HIERARCHY, "band boxes: BOUNDARY cell outside the band");
    MGPS_TRY_RC(runGroups(true, x, y, &snapshot));
    for (size_t c = 0; c < n; ++c)
        if (owned[c] != (isClosure(ptrdiff_t(c)) ? 1 : 0)) return fail(MGPS_ERR_HIERARCHY, "band boxes: closure cell not owned exactly once");
    if (y != refB) return fail(MGPS_ERR_HIERARCHY, "band boxes: closure stage differs from band passes + sweep");
    // the stage after the sweep: reads the snapshot only, writes y in place
    MGPS_TRY_RC(runGroups(false, snapshot, y, nullptr));
    if (y != refC) return fail(MGPS_ERR_HIERARCHY, "band boxes: stage fed from the snapshot differs from pass-by-pass replay");
    if (out_region_cells) *out_region_cells = regionCells;
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

int mgps_hierarchy_coarse_unknowns(const mgps_hierarchy *hier) { return hier ? hier->coarseN : 0; }

int mgps_hierarchy_coarse_solve(const mgps_hierarchy *hier, float *x, const float *b)
try {
    if (!hier || !x || !b) return fail(MGPS_ERR_INVALID_ARGUMENT, "mgps_hierarchy_coarse_solve: bad arguments");
    if (hier->coarseOnDevice) {  // (the cost rule sent this level to the device: the host factorises it now, slowly, up to kHostCoarseMax unknowns)
        const int rc = hostCoarseFallback(const_cast<mgps_hierarchy *>(hier));
        if (rc != MGPS_OK) return rc;
    }
    std::vector<double> v(hier->coarseN);
    for (int r = 0; r < hier->coarseN; ++r) v[r] = b[hier->coarseCell[r]];
    if (!hier->coarseComp.empty()) {  // (options.enclosed_liquid: the rhs's mean over a pinned component is removed first -- the consistent part)
        std::vector<double> sum(hier->coarsePinned.size(), 0.0), cnt(hier->coarsePinned.size(), 0.0);
        for (int r = 0; r < hier->coarseN; ++r)
            if (hier->coarseComp[size_t(r)] >= 0) sum[size_t(hier->coarseComp[size_t(r)])] += v[r], cnt[size_t(hier->coarseComp[size_t(r)])] += 1.0;
        for (int r = 0; r < hier->coarseN; ++r)
            if (hier->coarseComp[size_t(r)] >= 0) v[r] -= sum[size_t(hier->coarseComp[size_t(r)])] / cnt[size_t(hier->coarseComp[size_t(r)])];
    }
    hier->bandedSolve(v.data());
    for (int r = 0; r < hier->coarseN; ++r) x[hier->coarseCell[r]] = float(v[r]);
    return MGPS_OK;
}
MGPS_API_CATCH(nullptr)

}  // extern "C"
