/*
 * Stand-in for the HDK's SYS basics, written from the HDK's documented behaviour for the one purpose of
 * compiling the reference solver core and its plugin into oracle/_ref/ (see oracle/Makefile, target `ref`).  TEST
 * INFRASTRUCTURE ONLY.  Nothing here is taken from the HDK or from the reference.
 *
 * Semantics of the whole oracle/ref_standin/ tree ("Reference parity"):
 *   - voxel arrays are dense and never compressed; tiles are 16^3, numbered x fastest, then y, then z;
 *     voxels within a tile are visited x fastest, then y, then z; partial tiles at the upper edges;
 *   - isTileConstant() / isConstant() are always false; uncompress / collapseAllTiles are no-ops;
 *   - probes are write-through and read the array directly (no cached line);
 *   - every UTparallelFor* / UT_ThreadedAlgorithm::run body runs once, serially, over the whole range
 *     (one job, one processor); UTparallelSort is std::sort; the interrupt never fires;
 *   - assert() stays armed and throws refstandin::AssertionFailed instead of aborting, so a violated
 *     reference assertion reaches the driver as an error code;
 *   - for the plugin files (SIM/SIM_RawField.h has the detail): raw fields store fpreal32 and
 *     SIM::FieldUtils::getFieldValue hands a sample out as fpreal32; tiles are never constant and
 *     makeConstant fills, while the ARRAY's isConstant(&v) answers by value; indexToPos uses the sample's
 *     offset for centre and face sampling; getValue(pos) is the trilinear interpolant in the form
 *     (1 - t) a + t b, clamped at the border, and returns a sample bit for bit at a sample's position;
 *     SIM_Object is a table of named fields, GAS_SubSolver a table of options.
 */
#ifndef REFSTANDIN_SYS_TYPES_H
#define REFSTANDIN_SYS_TYPES_H

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

using exint = std::int64_t;
using int32 = std::int32_t;
using int64 = std::int64_t;
using fpreal = double;
using fpreal32 = float;
using fpreal64 = double;

#define SYS_FORCE_INLINE inline

namespace refstandin
{
struct AssertionFailed : std::runtime_error
{
    using std::runtime_error::runtime_error;
};

[[noreturn]] inline void assertFailed(const char *expr, const char *file, int line)
{
    throw AssertionFailed(std::string(file) + ":" + std::to_string(line) + ": assertion failed: " + expr);
}
} // namespace refstandin

#ifdef assert
#undef assert
#endif
#ifdef NDEBUG
#define assert(...) ((void)0)
#else
#define assert(...) ((__VA_ARGS__) ? (void)0 : ::refstandin::assertFailed(#__VA_ARGS__, __FILE__, __LINE__))
#endif

#endif
