// The host part of csrc/mgps_tile_pass.h without a GPU: what the tiled field passes refuse before any device work.  The overlap rule
// on every pair of {read, written} x {disjoint, touching, one byte shared, nested, identical}, the halo rule at the grid's ends, the
// planes a redistance pass reads against the planes held (cross-checked against the rule as tests/redistance_reference.py held()
// states it) and the launch-grid limit with its number.  No pointer here is ever dereferenced.
#include <cstdio>
#include <cstring>

#include "mgps_tile_pass.h"
using namespace mgps;

static int gFailures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++gFailures;                                                     \
        }                                                                    \
    } while (0)

static const char *kFn = "tile_pass_check";

static bool said(const std::string &what)
{
    const std::string msg = lastGlobalError();
    return msg.rfind(std::string(kFn) + ": ", 0) == 0 && msg.find(what) != std::string::npos;
}

static void arrayRanges()
{
    static char block[64];
    struct Layout {
        const char *name;
        size_t a0, an, b0, bn;  // [a0, a0 + an) and [b0, b0 + bn) of the block
        bool shared;
    };
    const Layout layouts[] = {{"disjoint", 0, 8, 16, 8, false}, {"touching end to start", 0, 8, 8, 8, false}, {"one byte shared", 0, 9, 8, 8, true},
                              {"nested", 0, 32, 8, 8, true},    {"identical", 4, 12, 4, 12, true}};
    for (const Layout &l : layouts)
        for (int writes = 0; writes < 4; ++writes)
            for (int swapped = 0; swapped < 2; ++swapped) {
                const bool wa = writes & 1, wb = writes & 2;
                ArrayRanges r;
                if (!swapped) r.add("first", block + l.a0, l.an, wa), r.add("second", block + l.b0, l.bn, wb);
                else r.add("second", block + l.b0, l.bn, wb), r.add("first", block + l.a0, l.an, wa);
                r.add("far", block + 48, 8, true);  // (a written array apart from both changes nothing)
                const int rc = r.refuseOverlap(kFn);
                const bool want = l.shared && (wa || wb);
                CHECK(rc == (want ? MGPS_ERR_INVALID_ARGUMENT : MGPS_OK));
                if (rc != MGPS_OK)
                    CHECK(said(swapped ? "second and first overlap: the pass is out of place" : "first and second overlap: the pass is out of place"));
            }
    ArrayRanges same;  // two arrays that are only read may be one, whatever else the call writes
    same.add("in", block, 16, false), same.add("lo", block, 16, false), same.add("out", block + 32, 16, true);
    CHECK(same.refuseOverlap(kFn) == MGPS_OK);
    same.add("scratch", block + 40, 16, true);
    CHECK(same.refuseOverlap(kFn) == MGPS_ERR_INVALID_ARGUMENT && said("out and scratch overlap"));
    CHECK(ArrayRanges{}.refuseOverlap(kFn) == MGPS_OK);
    std::printf("array ranges ok: %d\n", gFailures == 0);
}

static void haloRule()
{
    int below = -1, above = -1;
    haloPlanes(3, 0, 5, 19, below, above);  // c0 = 0: nothing lies below
    CHECK(below == 0 && above == 3);
    haloPlanes(3, 13, 19, 19, below, above);  // c1 = gz: nothing lies above
    CHECK(below == 3 && above == 0);
    haloPlanes(0, 6, 13, 19, below, above);
    CHECK(below == 0 && above == 0);
    haloPlanes(100, 6, 13, 19, below, above);  // a halo larger than the grid: every plane there is
    CHECK(below == 6 && above == 6);
    haloPlanes(4, 0, 19, 19, below, above);  // the whole grid as a window
    CHECK(below == 0 && above == 0);

    static char plane[4];
    CHECK(checkHaloArrays(kFn, "phi_lo", nullptr, 0, "phi_hi", nullptr, 0) == MGPS_OK);
    CHECK(checkHaloArrays(kFn, "phi_lo", plane, 2, "phi_hi", plane, 3) == MGPS_OK);
    CHECK(checkHaloArrays(kFn, "phi_lo", nullptr, 2, "phi_hi", nullptr, 3) == MGPS_ERR_INVALID_ARGUMENT && said("phi_lo is NULL: 2 halo planes lie below the window"));
    CHECK(checkHaloArrays(kFn, "velocity_lo[1]", plane, 2, "velocity_hi[1]", nullptr, 3) == MGPS_ERR_INVALID_ARGUMENT &&
          said("velocity_hi[1] is NULL: 3 halo planes lie above the window"));
    std::printf("halo rule ok: %d\n", gFailures == 0);
}

// tests/redistance_reference.py held(): does a window (c0, c1, halo) of gz planes hold what a pass reads?  inner = 0: the initial pass
static bool referenceHolds(int gz, int c0, int c1, int halo, int inner)
{
    const int h0 = c0 - std::min(halo, c0), h1 = c1 + std::min(halo, gz - c1);
    int n0, n1;
    if (inner == 0 || inner == 1) n0 = std::max(c0 - 1, 0), n1 = std::min(c1 + 1, gz);
    else n0 = std::max(4 * (c0 / 4) - 1, 0), n1 = std::min(4 * ((c1 + 3) / 4) + 1, gz);
    return !(h0 > n0 || h1 < n1);
}

static void heldAgainstRead()
{
    int windows = 0, refusals = 0;
    for (int gz : {1, 8, 19, 20})
        for (int c0 = 0; c0 < gz; ++c0)
            for (int c1 = c0 + 1; c1 <= gz; ++c1)  // windows on and off the tile's four planes, at the grid's ends and inside
                for (int halo = 0; halo <= 5; ++halo)
                    for (int inner : {0, 1, 4}) {
                        int below, above, n0, n1;
                        haloPlanes(halo, c0, c1, gz, below, above);
                        planesRead(c0, c1, inner > 1, n0, n1);
                        const std::string why = inner ? "a round of inner = " + std::to_string(inner) : "the initial pass";
                        const int rc = checkHalo(kFn, c0, c1, gz, halo, below, above, n0, n1, why);
                        const bool holds = referenceHolds(gz, c0, c1, halo, inner);
                        CHECK(rc == (holds ? MGPS_OK : MGPS_ERR_INVALID_ARGUMENT));
                        if (rc != MGPS_OK) CHECK(said("too few halo planes: halo = " + std::to_string(halo) + " holds the planes ") && said(why + " reads "));
                        ++windows, refusals += rc != MGPS_OK;
                    }
    CHECK(windows > 1000 && refusals > 100 && refusals < windows);
    // the cases of tests/test_redistance.py: cuts at 9 and at 6, 13 of 19 planes
    int below, above, n0, n1;
    haloPlanes(1, 9, 19, 19, below, above);
    planesRead(9, 19, true, n0, n1);
    CHECK(n0 == 7 && n1 == 21);
    CHECK(checkHalo(kFn, 9, 19, 19, 1, below, above, n0, n1, "a round of inner = 4") == MGPS_ERR_INVALID_ARGUMENT &&
          said("too few halo planes: halo = 1 holds the planes 8 .. 18, a round of inner = 4 reads 7 .. 18"));
    haloPlanes(4, 6, 13, 19, below, above);
    planesRead(6, 13, true, n0, n1);
    CHECK(n0 == 3 && n1 == 17 && checkHalo(kFn, 6, 13, 19, 4, below, above, n0, n1, "a round of inner = 4") == MGPS_OK);
    planesRead(8, 16, true, n0, n1);  // a window on the tile's planes
    CHECK(n0 == 7 && n1 == 17);
    planesRead(8, 16, false, n0, n1);
    CHECK(n0 == 7 && n1 == 17);
    planesRead(6, 13, false, n0, n1);
    CHECK(n0 == 5 && n1 == 14);
    std::printf("held against read ok: %d\n", gFailures == 0);
}

static void tileExtents()
{
    CHECK(checkTileExtents(kFn, 1, 1, 1, false) == MGPS_OK && checkTileExtents(kFn, 1, 1, 1, true) == MGPS_OK);
    for (int axis = 0; axis < 3; ++axis)
        for (int bad : {0, -3}) {
            int g[3] = {5, 6, 7};
            g[axis] = bad;
            CHECK(checkTileExtents(kFn, g[0], g[1], g[2], false) == MGPS_ERR_INVALID_ARGUMENT);
            CHECK(said("non-positive extent (gx, gy, gz = " + std::to_string(g[0]) + ", " + std::to_string(g[1]) + ", " + std::to_string(g[2]) + ")"));
        }
    // 65535 tile layers of four cells along y and z; x is the launch grid's first dimension and has no such limit
    CHECK(checkTileExtents(kFn, 1 << 30, 262140, 262140, false) == MGPS_OK);
    CHECK(checkTileExtents(kFn, 8, 262141, 8, false) == MGPS_ERR_INVALID_ARGUMENT && said("more than 262140 cells along y or z"));
    CHECK(checkTileExtents(kFn, 8, 8, 262141, false) == MGPS_ERR_INVALID_ARGUMENT && said("more than 262140 cells along y or z"));
    // a pass over whole-grid tiles on a window off the tile's planes: one layer fewer
    CHECK(checkTileExtents(kFn, 8, 262136, 262136, true) == MGPS_OK);
    CHECK(checkTileExtents(kFn, 8, 262137, 8, true) == MGPS_ERR_INVALID_ARGUMENT && said("more than 262136 cells along y or z"));
    CHECK(checkTileExtents(kFn, 8, 8, 262137, true) == MGPS_ERR_INVALID_ARGUMENT && said("more than 262136 cells along y or z"));
    CHECK(checkTileExtents(kFn, 8, 8, 2147483647, false) == MGPS_ERR_INVALID_ARGUMENT);  // (no overflow on the way to the answer)
    std::printf("tile extents ok: %d\n", gFailures == 0);
}

int main()
{
    arrayRanges();
    haloRule();
    heldAgainstRead();
    tileExtents();
    if (gFailures) {
        std::printf("tile pass check: %d checks FAILED\n", gFailures);
        return 1;
    }
    std::printf("tile pass check ok\n");
    return 0;
}
