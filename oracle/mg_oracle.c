/*
 * mg_oracle.c -- CPU restatement (fp64, flat arrays) of the reference's geometric multigrid
 * hot path.  TEST INFRASTRUCTURE ONLY: nothing in the product path
 * (geometricmultigridpressuresolver_amd/) may include, link, import or call this file.  Only
 * tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg use it, and only as the
 * checker / the timed CPU baseline.
 *
 * PARITY: pinned to the reference (rgoldade/GeometricMultigridPressureSolver) itself.  The reference
 * ships no golden vectors, but its solver core compiles, unchanged, against the stand-in headers of
 * oracle/ref_standin/ (`make ref`, see the Makefile and ref_driver.cpp); tests/golden/ref_*.npz hold
 * what that binary computes and tests/test_reference_parity.py holds every entry of this file to it:
 * per-cell results bit for bit on every level (visiting and accumulation order included), reductions
 * within the bound of a different summation order, V-cycles and PCG within the measured sensitivity
 * to the coarse direct solve.  The reference's own *property* checks,
 * re-expressed in tests/test_oracle_*.py, stay as a second, independent pin: the operator symmetry
 * identities (Test.cpp:1197-1875), the structural label invariants (Ops.cpp:471-632,
 * Ops.h:1771-1870), the 50-V-cycle convergence trace (Test.cpp:1877-1960), the CG test
 * (Test.cpp:675-1009) and an independent SciPy assembly of the same matrix (row rules
 * Test.cpp:1350-1433).
 *
 * Every function cites the reference file:line it follows ("Ops.h" =
 * Source/HDK_GeometricMultigridOperators.h, "Ops.cpp" = ...Operators.cpp, "MG.cpp" =
 * Source/HDK_GeometricMultigridPoissonSolver.cpp, "CG.h" = Source/HDK_GeometricCGPoissonSolver.h,
 * "Test.cpp" = Source/HDK_TestGeometricMultigrid.cpp, "Util.h" = Source/HDK_Utilities.h).
 *
 * Conventions: grids are dense, x fastest: idx = (k*ny + j)*nx + i.  The face grid of axis a has
 * one more entry along a; face f of axis a lies between cells f-e_a and f (SIM::FieldUtils maps,
 * inferred from use at Ops.h:196,342 and Plug.cpp:838-839).  Tiles are 16^3, linear tile id x
 * fastest (HDK UT_VoxelArray).  The reference's structural costs are kept on purpose (4-byte
 * labels, whole-grid copy per Jacobi sweep, clear + A.x + add residual) so that timing this file
 * is timing a faithful port.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#ifndef MGO_REAL
#define MGO_REAL double
#endif
typedef MGO_REAL real;

enum { MGO_INTERIOR = 0, MGO_EXTERIOR = 1, MGO_DIRICHLET = 2, MGO_BOUNDARY = 3 }; /* Ops.h:11 */
#define TILE 16

typedef struct {
    int nx, ny, nz;
} dims_t;

static inline size_t cidx(const dims_t *d, int i, int j, int k)
{
    return ((size_t)k * d->ny + j) * d->nx + i;
}
static inline int is_active(int l) { return l == MGO_INTERIOR || l == MGO_BOUNDARY; }

/* face index of the face on side `dir` (0 = minus, 1 = plus) of cell (i,j,k) along `axis`
 * (cellToFaceMap: c / c + e_a), inside the axis face grid. */
static inline size_t fidx(const dims_t *d, int axis, int i, int j, int k, int dir)
{
    int fx = d->nx + (axis == 0), fy = d->ny + (axis == 1);
    if (axis == 0) i += dir;
    else if (axis == 1) j += dir;
    else k += dir;
    return ((size_t)k * fy + j) * fx + i;
}

int mgo_real_bytes(void) { return (int)sizeof(real); }

void mgo_set_threads(int n)
{
#ifdef _OPENMP
    if (n > 0) omp_set_num_threads(n);
#else
    (void)n;
#endif
}
int mgo_get_threads(void)
{
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

/* ------------------------------------------------------------------------------------------
 * computeLaplacian  (Ops.h:177-260).  w[3] may be NULL (unit weights, coarse levels).
 * Neighbour visiting order and the accumulation order are the reference's.
 * ---------------------------------------------------------------------------------------- */
static inline void laplacian(const dims_t *d, const real *x, const int32_t *lab,
                             const real *const w[3], int i, int j, int k, real *lap_out,
                             real *diag_out)
{
    const size_t c = cidx(d, i, j, k);
    const ptrdiff_t stride[3] = {1, d->nx, (ptrdiff_t)d->nx * d->ny};
    real lap = 0, diag = 0;
    if (lab[c] == MGO_INTERIOR) { /* Ops.h:191-207 */
        for (int axis = 0; axis < 3; ++axis)
            for (int dir = 0; dir < 2; ++dir)
                lap -= x[c + (dir ? stride[axis] : -stride[axis])];
        diag = 6;
    } else { /* BOUNDARY centre, Ops.h:208-256 */
        for (int axis = 0; axis < 3; ++axis)
            for (int dir = 0; dir < 2; ++dir) {
                const size_t n = c + (dir ? stride[axis] : -stride[axis]);
                const int nl = lab[n];
                if (nl == MGO_INTERIOR) {
                    lap -= x[n];
                    diag += 1;
                } else if (nl == MGO_BOUNDARY) {
                    if (w) {
                        const real wt = w[axis][fidx(d, axis, i, j, k, dir)];
                        lap -= wt * x[n];
                        diag += wt;
                    } else {
                        lap -= x[n];
                        diag += 1;
                    }
                } else if (nl == MGO_DIRICHLET) {
                    if (w) diag += w[axis][fidx(d, axis, i, j, k, dir)];
                    else diag += 1;
                }
            }
    }
    lap += diag * x[c]; /* Ops.h:258 */
    *lap_out = lap;
    *diag_out = diag;
}

static inline void pack_w(const real *wx, const real *wy, const real *wz, const real *w[3])
{
    w[0] = wx;
    w[1] = wy;
    w[2] = wz;
}

/* jacobiPoissonSmoother (Ops.h:262-367): x <- x + 2/3 (b - A xcopy)/diag on active cells.
 * `scratch` (n cells) holds the whole-grid copy the reference takes at Ops.h:289. */
void mgo_jacobi_weighted(real *x, const real *b, const int32_t *lab, const real *wx, const real *wy,
                         const real *wz, int nx, int ny, int nz, real *scratch, double weight)
{
    const dims_t d = {nx, ny, nz};
    const real *w[3];
    pack_w(wx, wy, wz, w);
    const real *const *wp = wx ? w : NULL;
    const size_t n = (size_t)nx * ny * nz;
    int own = 0;
    if (!scratch) {
        scratch = (real *)malloc(n * sizeof(real));
        own = 1;
    }
#pragma omp parallel for schedule(static)
    for (int k = 0; k < nz; ++k)
        memcpy(scratch + (size_t)k * nx * ny, x + (size_t)k * nx * ny, (size_t)nx * ny * sizeof(real));
    const real damped = weight; /* Ops.h:291 hard-wires 2. / 3. */
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) {
                const size_t c = cidx(&d, i, j, k);
                if (!is_active(lab[c])) continue;
                real lap, diag;
                laplacian(&d, scratch, lab, wp, i, j, k, &lap, &diag);
                real res = b[c] - lap;
                res /= diag;
                x[c] = x[c] + damped * res; /* Ops.h:356-361 */
            }
    if (own) free(scratch);
}
void mgo_jacobi(real *x, const real *b, const int32_t *lab, const real *wx, const real *wy,
                const real *wz, int nx, int ny, int nz, real *scratch)
{
    mgo_jacobi_weighted(x, b, lab, wx, wy, wz, nx, ny, nz, scratch, 2. / 3.);
}

/* tiledGaussSeidelPoissonSmoother (Ops.h:369-520): undamped in-place GS over the 16^3 tiles whose
 * (tx+ty+tz) parity matches `odd`; lexicographic i->j->k inside a tile, forward or reversed. */
void mgo_tiled_gs(real *x, const real *b, const int32_t *lab, const real *wx, const real *wy,
                  const real *wz, int nx, int ny, int nz, int odd, int forward)
{
    const dims_t d = {nx, ny, nz};
    const real *w[3];
    pack_w(wx, wy, wz, w);
    const real *const *wp = wx ? w : NULL;
    const int tx = (nx + TILE - 1) / TILE, ty = (ny + TILE - 1) / TILE, tz = (nz + TILE - 1) / TILE;
    const int ntiles = tx * ty * tz;
#pragma omp parallel for schedule(dynamic, 4)
    for (int t = 0; t < ntiles; ++t) {
        const int ti = t % tx, tj = (t / tx) % ty, tk = t / (tx * ty);
        const int is_odd = ((ti + tj + tk) % 2) != 0; /* Ops.h:441-448 */
        if ((odd && !is_odd) || (!odd && is_odd)) continue;
        const int i0 = ti * TILE, j0 = tj * TILE, k0 = tk * TILE;
        const int i1 = i0 + TILE < nx ? i0 + TILE : nx;
        const int j1 = j0 + TILE < ny ? j0 + TILE : ny;
        const int k1 = k0 + TILE < nz ? k0 + TILE : nz;
#define GS_CELL(i, j, k)                                                                           \
    do {                                                                                           \
        const size_t c = cidx(&d, i, j, k);                                                        \
        if (is_active(lab[c])) {                                                                   \
            real lap, diag;                                                                        \
            laplacian(&d, x, lab, wp, i, j, k, &lap, &diag);                                       \
            real res = b[c] - lap;                                                                 \
            res /= diag;                                                                           \
            x[c] = x[c] + res; /* Ops.h:493 */                                                     \
        }                                                                                          \
    } while (0)
        if (forward) { /* Ops.h:497-506 */
            for (int k = k0; k < k1; ++k)
                for (int j = j0; j < j1; ++j)
                    for (int i = i0; i < i1; ++i) GS_CELL(i, j, k);
        } else { /* Ops.h:507-516 */
            for (int k = k1 - 1; k >= k0; --k)
                for (int j = j1 - 1; j >= j0; --j)
                    for (int i = i1 - 1; i >= i0; --i) GS_CELL(i, j, k);
        }
#undef GS_CELL
    }
}

/* boundaryJacobiPoissonSmoother (Ops.h:524-619): damped Jacobi on the band list; compute into a
 * temp list, then scatter.  cells = ncells x (i,j,k) int32 triples. */
void mgo_boundary_jacobi_weighted(real *x, const real *b, const int32_t *lab, const int32_t *cells,
                                  int64_t ncells, const real *wx, const real *wy, const real *wz, int nx,
                                  int ny, int nz, double weight)
{
    const dims_t d = {nx, ny, nz};
    const real *w[3];
    pack_w(wx, wy, wz, w);
    const real *const *wp = wx ? w : NULL;
    const real damped = weight; /* Ops.h:554 hard-wires 2. / 3. */
    real *tmp = (real *)malloc((size_t)(ncells > 0 ? ncells : 1) * sizeof(real));
#pragma omp parallel for schedule(static)
    for (int64_t n = 0; n < ncells; ++n) {
        const int i = cells[3 * n], j = cells[3 * n + 1], k = cells[3 * n + 2];
        const size_t c = cidx(&d, i, j, k);
        real lap, diag;
        laplacian(&d, x, lab, wp, i, j, k, &lap, &diag);
        real res = b[c] - lap;
        res /= diag;
        tmp[n] = x[c] + damped * res; /* Ops.h:596-599 */
    }
#pragma omp parallel for schedule(static)
    for (int64_t n = 0; n < ncells; ++n) /* Ops.h:604-618 */
        x[cidx(&d, cells[3 * n], cells[3 * n + 1], cells[3 * n + 2])] = tmp[n];
    free(tmp);
}
void mgo_boundary_jacobi(real *x, const real *b, const int32_t *lab, const int32_t *cells,
                         int64_t ncells, const real *wx, const real *wy, const real *wz, int nx,
                         int ny, int nz)
{
    mgo_boundary_jacobi_weighted(x, b, lab, cells, ncells, wx, wy, wz, nx, ny, nz, 2. / 3.);
}

/* applyPoissonMatrix (Ops.h:621-714): y = A x on active cells, other cells untouched. */
void mgo_apply_poisson(real *y, const real *x, const int32_t *lab, const real *wx, const real *wy,
                       const real *wz, int nx, int ny, int nz)
{
    const dims_t d = {nx, ny, nz};
    const real *w[3];
    pack_w(wx, wy, wz, w);
    const real *const *wp = wx ? w : NULL;
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) {
                const size_t c = cidx(&d, i, j, k);
                if (!is_active(lab[c])) continue;
                real lap, diag;
                laplacian(&d, x, lab, wp, i, j, k, &lap, &diag);
                y[c] = lap;
            }
}

/* addVectors (Ops.h:1139-1195): d = a + s*bs on active cells; d may alias bs. */
void mgo_add_vectors(real *dst, const real *a, const real *bs, real s, const int32_t *lab,
                     int64_t n)
{
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < n; ++c)
        if (is_active(lab[c])) dst[c] = a[c] + s * bs[c];
}

/* addToVector (Ops.h:1087-1137): d += s*a on active cells. */
void mgo_add_to_vector(real *dst, const real *a, real s, const int32_t *lab, int64_t n)
{
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < n; ++c)
        if (is_active(lab[c])) dst[c] = dst[c] + s * a[c];
}

/* scaleVector (Ops.h:974-1018). */
void mgo_scale_vector(real *v, real s, const int32_t *lab, int64_t n)
{
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < n; ++c)
        if (is_active(lab[c])) v[c] = s * v[c];
}

/* computePoissonResidual (Ops.h:716-732): r = 0; r = A x; r = b - r (three passes, as there). */
void mgo_residual(real *r, const real *x, const real *b, const int32_t *lab, const real *wx,
                  const real *wy, const real *wz, int nx, int ny, int nz)
{
    const size_t n = (size_t)nx * ny * nz;
#pragma omp parallel for schedule(static)
    for (int k = 0; k < nz; ++k) memset(r + (size_t)k * nx * ny, 0, (size_t)nx * ny * sizeof(real));
    mgo_apply_poisson(r, x, lab, wx, wy, wz, nx, ny, nz);
    mgo_add_vectors(r, b, r, -1, lab, (int64_t)n);
}

/* Tile-ordered reductions: per-tile partial in tile-local (x fastest) order, then a serial sum
 * over tiles in linear tile order (Ops.h:1020-1085, 1205-1265, 1267-1326). */
typedef enum { RED_DOT, RED_SQR, RED_MAX } red_kind;
static double tile_reduce(red_kind kind, const real *a, const real *b, const int32_t *lab, int nx,
                          int ny, int nz)
{
    const dims_t d = {nx, ny, nz};
    const int tx = (nx + TILE - 1) / TILE, ty = (ny + TILE - 1) / TILE, tz = (nz + TILE - 1) / TILE;
    const int ntiles = tx * ty * tz;
    double *part = (double *)calloc((size_t)ntiles, sizeof(double));
#pragma omp parallel for schedule(static)
    for (int t = 0; t < ntiles; ++t) {
        const int ti = t % tx, tj = (t / tx) % ty, tk = t / (tx * ty);
        const int i0 = ti * TILE, j0 = tj * TILE, k0 = tk * TILE;
        const int i1 = i0 + TILE < nx ? i0 + TILE : nx;
        const int j1 = j0 + TILE < ny ? j0 + TILE : ny;
        const int k1 = k0 + TILE < nz ? k0 + TILE : nz;
        double acc = 0;
        for (int k = k0; k < k1; ++k)
            for (int j = j0; j < j1; ++j)
                for (int i = i0; i < i1; ++i) {
                    const size_t c = cidx(&d, i, j, k);
                    if (!is_active(lab[c])) continue;
                    if (kind == RED_DOT) acc += (double)a[c] * (double)b[c];
                    else if (kind == RED_SQR) acc += (double)a[c] * (double)a[c];
                    else acc = acc > (double)a[c] ? acc : (double)a[c];
                }
        part[t] = acc;
    }
    double total = 0;
    for (int t = 0; t < ntiles; ++t) {
        if (kind == RED_MAX) total = total > part[t] ? total : part[t];
        else total += part[t];
    }
    free(part);
    return total;
}
double mgo_dot(const real *a, const real *b, const int32_t *lab, int nx, int ny, int nz)
{
    return tile_reduce(RED_DOT, a, b, lab, nx, ny, nz);
}
double mgo_squared_l2(const real *a, const int32_t *lab, int nx, int ny, int nz)
{
    return tile_reduce(RED_SQR, a, NULL, lab, nx, ny, nz);
}
double mgo_l2(const real *a, const int32_t *lab, int nx, int ny, int nz)
{
    return sqrt(mgo_squared_l2(a, lab, nx, ny, nz));
}
/* infNorm (Ops.h:1267-1326): max(0, max_active v) -- NO absolute value, as in the reference. */
double mgo_inf_norm(const real *a, const int32_t *lab, int nx, int ny, int nz)
{
    return tile_reduce(RED_MAX, a, NULL, lab, nx, ny, nz);
}

/* downsample (Ops.h:734-835): full weighting, 4x4x4 fine samples starting at 2C-1, weights
 * {1/8,3/8,3/8,1/8}^3, accumulation order z,y,x as there; destination cleared first. */
void mgo_downsample(real *coarse, const real *fine, const int32_t *coarse_lab, int cnx, int cny,
                    int cnz)
{
    static const real rw[4] = {1. / 8., 3. / 8., 3. / 8., 1. / 8.};
    const dims_t cd = {cnx, cny, cnz}, fd = {2 * cnx, 2 * cny, 2 * cnz};
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = 0; k < cnz; ++k)
        for (int j = 0; j < cny; ++j)
            for (int i = 0; i < cnx; ++i) {
                const size_t c = cidx(&cd, i, j, k);
                if (!is_active(coarse_lab[c])) {
                    coarse[c] = 0; /* Ops.h:756 */
                    continue;
                }
                real s = 0;
                const int si = 2 * i - 1, sj = 2 * j - 1, sk = 2 * k - 1; /* Ops.h:799 */
                for (int zo = 0; zo < 4; ++zo)
                    for (int yo = 0; yo < 4; ++yo)
                        for (int xo = 0; xo < 4; ++xo)
                            s += rw[xo] * rw[yo] * rw[zo] * fine[cidx(&fd, si + xo, sj + yo, sk + zo)];
                coarse[c] = s;
            }
}

static inline real lerp(real a, real b, real f) { return (1. - f) * a + f * b; } /* Ops.h:841-847 */

/* upsampleAndAdd (Ops.h:873-972): fine += 4 * trilerp(coarse) at sample point c/2 - 1/4. */
void mgo_upsample_add(real *fine, const real *coarse, const int32_t *fine_lab, int fnx, int fny,
                      int fnz)
{
    const dims_t fd = {fnx, fny, fnz}, cd = {fnx / 2, fny / 2, fnz / 2};
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = 0; k < fnz; ++k)
        for (int j = 0; j < fny; ++j)
            for (int i = 0; i < fnx; ++i) {
                const size_t c = cidx(&fd, i, j, k);
                if (!is_active(fine_lab[c])) continue;
                const real px = .5 * ((real)i + .5) - .5, py = .5 * ((real)j + .5) - .5,
                           pz = .5 * ((real)k + .5) - .5; /* Ops.h:931 */
                const int bi = (int)px, bj = (int)py, bk = (int)pz; /* Ops.h:933 (truncation) */
                const real fx = px - bi, fy = py - bj, fz = pz - bk;
                real v[2][2][2];
                for (int zo = 0; zo < 2; ++zo)
                    for (int yo = 0; yo < 2; ++yo)
                        for (int xo = 0; xo < 2; ++xo)
                            v[xo][yo][zo] = coarse[cidx(&cd, bi + xo, bj + yo, bk + zo)];
                const real t = lerp(lerp(lerp(v[0][0][0], v[1][0][0], fx), lerp(v[0][1][0], v[1][1][0], fx), fy),
                                    lerp(lerp(v[0][0][1], v[1][0][1], fx), lerp(v[0][1][1], v[1][1][1], fx), fy),
                                    fz); /* Ops.h:863-871 */
                fine[c] = fine[c] + 4. * t; /* Ops.h:964 */
            }
}

/* ------------------------------------------------------------------------------------------
 * Domain / hierarchy construction
 * ---------------------------------------------------------------------------------------- */

/* buildExpandedCellLabels sizing rule (Ops.h:1340-1362): levels = ceil(log2(min res)) - 1,
 * padding 2^(levels-1) per side, every extent rounded up to a power of two. */
void mgo_expanded_layout(int bnx, int bny, int bnz, int *out_dims, int *out_offset, int *out_levels)
{
    double minlog = fmin(log2((double)bnx), log2((double)bny));
    minlog = fmin(minlog, log2((double)bnz));
    const int levels = (int)(ceil(minlog) - log2(2.0));
    const int pad = (int)pow(2, levels - 1);
    const int base[3] = {bnx, bny, bnz};
    for (int a = 0; a < 3; ++a) {
        double ls = ceil(log2((double)(base[a] + 2 * pad)));
        out_dims[a] = (int)exp2(ls);
        out_offset[a] = pad;
    }
    *out_levels = levels;
}

/* buildExpandedCellLabels copy (Ops.h:1364-1453): EXTERIOR everywhere, base labels at +offset. */
void mgo_build_expanded_labels(int32_t *exp_lab, const int32_t *base_lab, int bnx, int bny, int bnz,
                               int enx, int eny, int enz, int off)
{
    const dims_t bd = {bnx, bny, bnz}, ed = {enx, eny, enz};
    const size_t n = (size_t)enx * eny * enz;
    for (size_t c = 0; c < n; ++c) exp_lab[c] = MGO_EXTERIOR;
    for (int k = 0; k < bnz; ++k)
        for (int j = 0; j < bny; ++j)
            for (int i = 0; i < bnx; ++i) {
                const int l = base_lab[cidx(&bd, i, j, k)];
                if (l == MGO_EXTERIOR) continue;
                exp_lab[cidx(&ed, i + off, j + off, k + off)] =
                    (l == MGO_INTERIOR) ? MGO_INTERIOR : MGO_DIRICHLET;
            }
}

/* buildExpandedBoundaryWeights (Ops.h:1458-1572): zero, then positive base weights at +offset. */
void mgo_build_expanded_weights(real *exp_w, const real *base_w, int axis, int bnx, int bny,
                                int bnz, int enx, int eny, int enz, int off)
{
    const int bfx = bnx + (axis == 0), bfy = bny + (axis == 1), bfz = bnz + (axis == 2);
    const int efx = enx + (axis == 0), efy = eny + (axis == 1), efz = enz + (axis == 2);
    memset(exp_w, 0, (size_t)efx * efy * efz * sizeof(real));
    for (int k = 0; k < bfz; ++k)
        for (int j = 0; j < bfy; ++j)
            for (int i = 0; i < bfx; ++i) {
                const real v = base_w[((size_t)k * bfy + j) * bfx + i];
                if (v > 0) exp_w[((size_t)(k + off) * efy + (j + off)) * efx + (i + off)] = v;
            }
}

/* setBoundaryCellLabels (Ops.h:1574-1644): INTERIOR -> BOUNDARY if a neighbour is DIRICHLET or
 * EXTERIOR, or any of the 6 face weights != 1.  Reads labels while other cells are rewritten in
 * the reference too; only INTERIOR->BOUNDARY transitions happen and the test is on
 * DIRICHLET/EXTERIOR, so the result does not depend on the visiting order. */
void mgo_set_boundary_labels(int32_t *lab, const real *wx, const real *wy, const real *wz, int nx,
                             int ny, int nz)
{
    const dims_t d = {nx, ny, nz};
    const real *w[3] = {wx, wy, wz};
    const ptrdiff_t stride[3] = {1, nx, (ptrdiff_t)nx * ny};
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) {
                const size_t c = cidx(&d, i, j, k);
                if (lab[c] != MGO_INTERIOR) continue;
                int bnd = 0;
                for (int axis = 0; axis < 3 && !bnd; ++axis)
                    for (int dir = 0; dir < 2; ++dir) {
                        const int nl = lab[c + (dir ? stride[axis] : -stride[axis])];
                        if (nl == MGO_DIRICHLET || nl == MGO_EXTERIOR) {
                            bnd = 1;
                            break;
                        }
                        if (w[axis][fidx(&d, axis, i, j, k, dir)] != 1) {
                            bnd = 1;
                            break;
                        }
                    }
                if (bnd) lab[c] = MGO_BOUNDARY;
            }
}

/* buildCoarseCellLabels (Ops.cpp:23-163). */
void mgo_build_coarse_labels(int32_t *coarse, const int32_t *fine, int fnx, int fny, int fnz)
{
    const dims_t fd = {fnx, fny, fnz}, cd = {fnx / 2, fny / 2, fnz / 2};
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = 0; k < cd.nz; ++k)
        for (int j = 0; j < cd.ny; ++j)
            for (int i = 0; i < cd.nx; ++i) {
                int has_d = 0, has_i = 0;
                for (int zo = 0; zo < 2; ++zo)
                    for (int yo = 0; yo < 2; ++yo)
                        for (int xo = 0; xo < 2; ++xo) {
                            const int l = fine[cidx(&fd, 2 * i + xo, 2 * j + yo, 2 * k + zo)];
                            if (l == MGO_DIRICHLET) has_d = 1;
                            else if (is_active(l)) has_i = 1;
                        }
                coarse[cidx(&cd, i, j, k)] = has_d ? MGO_DIRICHLET : (has_i ? MGO_INTERIOR : MGO_EXTERIOR);
            }
    /* second pass (Ops.cpp:104-158): INTERIOR with an EXTERIOR/DIRICHLET face neighbour -> BOUNDARY.
     * Writes only turn INTERIOR into BOUNDARY and the test ignores both, so in-place is safe. */
    const ptrdiff_t stride[3] = {1, cd.nx, (ptrdiff_t)cd.nx * cd.ny};
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = 0; k < cd.nz; ++k)
        for (int j = 0; j < cd.ny; ++j)
            for (int i = 0; i < cd.nx; ++i) {
                const size_t c = cidx(&cd, i, j, k);
                if (coarse[c] != MGO_INTERIOR) continue;
                int bnd = 0;
                for (int axis = 0; axis < 3 && !bnd; ++axis)
                    for (int dir = 0; dir < 2; ++dir) {
                        const int nl = coarse[c + (dir ? stride[axis] : -stride[axis])];
                        if (nl == MGO_EXTERIOR || nl == MGO_DIRICHLET) {
                            bnd = 1;
                            break;
                        }
                    }
                if (bnd) coarse[c] = MGO_BOUNDARY;
            }
}

static int has_solvable(const int32_t *lab, size_t n) /* MG.cpp:187-231 */
{
    for (size_t c = 0; c < n; ++c)
        if (is_active(lab[c])) return 1;
    return 0;
}

typedef struct {
    int tile, k, j, i;
} bcell_t;
static int bcell_cmp(const void *pa, const void *pb) /* Ops.cpp:441-464 */
{
    const bcell_t *a = (const bcell_t *)pa, *b = (const bcell_t *)pb;
    if (a->tile != b->tile) return a->tile < b->tile ? -1 : 1;
    if (a->k != b->k) return a->k < b->k ? -1 : 1;
    if (a->j != b->j) return a->j < b->j ? -1 : 1;
    if (a->i != b->i) return a->i < b->i ? -1 : 1;
    return 0;
}

/* buildBoundaryCells (Ops.cpp:165-469): layer 0 = BOUNDARY cells, each further layer = unvisited
 * INTERIOR face neighbours of the previous one; final list re-read from the visited grid and
 * sorted by (tile, k, j, i).  Returns the count; *out is malloc'ed (3 int32 per cell). */
int64_t mgo_build_boundary_cells(const int32_t *lab, int nx, int ny, int nz, int width, int32_t **out)
{
    const dims_t d = {nx, ny, nz};
    const size_t n = (size_t)nx * ny * nz;
    const ptrdiff_t stride[3] = {1, nx, (ptrdiff_t)nx * ny};
    /* 0 = unvisited, 1 = visited, 2 = queued for the next layer (the reference lets duplicates
     * into a layer and removes them by re-reading the visited grid, Ops.cpp:382-427; queue
     * marking gives the same set) */
    uint8_t *visited = (uint8_t *)calloc(n, 1);
    size_t cur_cap = 1024, cur_n = 0, next_cap = 1024, next_n = 0;
    size_t *cur = (size_t *)malloc(cur_cap * sizeof(size_t));
    size_t *next = (size_t *)malloc(next_cap * sizeof(size_t));
    for (size_t c = 0; c < n; ++c) /* layer 0: all BOUNDARY cells, Ops.cpp:192-224 */
        if (lab[c] == MGO_BOUNDARY) {
            if (cur_n == cur_cap) cur = (size_t *)realloc(cur, (cur_cap *= 2) * sizeof(size_t));
            cur[cur_n++] = c;
        }
    for (int layer = 0; layer < width; ++layer) {
        for (size_t q = 0; q < cur_n; ++q) visited[cur[q]] = 1; /* Ops.cpp:308-330 */
        if (layer < width - 1) {                                /* Ops.cpp:333-378 */
            next_n = 0;
            for (size_t q = 0; q < cur_n; ++q)
                for (int axis = 0; axis < 3; ++axis)
                    for (int dir = 0; dir < 2; ++dir) {
                        const size_t nb = cur[q] + (dir ? stride[axis] : -stride[axis]);
                        if (lab[nb] == MGO_INTERIOR && visited[nb] == 0) {
                            visited[nb] = 2;
                            if (next_n == next_cap)
                                next = (size_t *)realloc(next, (next_cap *= 2) * sizeof(size_t));
                            next[next_n++] = nb;
                        }
                    }
            size_t *tp = cur;
            cur = next;
            next = tp;
            size_t tc = cur_cap;
            cur_cap = next_cap;
            next_cap = tc;
            cur_n = next_n;
        }
    }
    int64_t count = 0;
    for (size_t c = 0; c < n; ++c) count += visited[c] != 0;
    bcell_t *list = (bcell_t *)malloc((size_t)(count > 0 ? count : 1) * sizeof(bcell_t));
    const int tx = (nx + TILE - 1) / TILE, ty = (ny + TILE - 1) / TILE;
    int64_t m = 0;
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i)
                if (visited[cidx(&d, i, j, k)]) {
                    bcell_t bc = {((k / TILE) * ty + (j / TILE)) * tx + (i / TILE), k, j, i};
                    list[m++] = bc;
                }
    qsort(list, (size_t)count, sizeof(bcell_t), bcell_cmp); /* Ops.cpp:440-466 */
    int32_t *res = (int32_t *)malloc((size_t)(count > 0 ? count : 1) * 3 * sizeof(int32_t));
    for (int64_t q = 0; q < count; ++q) {
        res[3 * q] = list[q].i;
        res[3 * q + 1] = list[q].j;
        res[3 * q + 2] = list[q].k;
    }
    free(list);
    free(visited);
    free(cur);
    free(next);
    *out = res;
    return count;
}
void mgo_free(void *p) { free(p); }

/* Structural checkers, return 1 = pass. */
int mgo_unit_test_exterior(const int32_t *lab, int nx, int ny, int nz) /* Ops.cpp:602-632 */
{
    const dims_t d = {nx, ny, nz};
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i)
                if ((i == 0 || j == 0 || k == 0 || i == nx - 1 || j == ny - 1 || k == nz - 1) &&
                    lab[cidx(&d, i, j, k)] != MGO_EXTERIOR)
                    return 0;
    return 1;
}
int mgo_unit_test_boundary(const int32_t *lab, const real *wx, const real *wy, const real *wz,
                           int nx, int ny, int nz) /* Ops.h:1771-1870 */
{
    const dims_t d = {nx, ny, nz};
    const real *w[3] = {wx, wy, wz};
    const ptrdiff_t stride[3] = {1, nx, (ptrdiff_t)nx * ny};
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) {
                const size_t c = cidx(&d, i, j, k);
                if (lab[c] == MGO_INTERIOR) {
                    for (int axis = 0; axis < 3; ++axis)
                        for (int dir = 0; dir < 2; ++dir)
                            if (!is_active(lab[c + (dir ? stride[axis] : -stride[axis])])) return 0;
                } else if (lab[c] == MGO_BOUNDARY) {
                    int ok = 0;
                    for (int axis = 0; axis < 3; ++axis)
                        for (int dir = 0; dir < 2; ++dir) {
                            const int nl = lab[c + (dir ? stride[axis] : -stride[axis])];
                            if (!is_active(nl)) ok = 1;
                            else if (wx && w[axis][fidx(&d, axis, i, j, k, dir)] != 1 && nl == MGO_BOUNDARY)
                                ok = 1;
                        }
                    if (!ok) return 0;
                }
            }
    return 1;
}
int mgo_unit_test_coarsening(const int32_t *coarse, const int32_t *fine, int fnx, int fny, int fnz)
{ /* Ops.cpp:471-600 */
    const dims_t fd = {fnx, fny, fnz}, cd = {fnx / 2, fny / 2, fnz / 2};
    if (fnx % 2 || fny % 2 || fnz % 2 || cd.nx % 2 || cd.ny % 2 || cd.nz % 2) return 0;
    for (int k = 0; k < fnz; ++k)
        for (int j = 0; j < fny; ++j)
            for (int i = 0; i < fnx; ++i) {
                const int fl = fine[cidx(&fd, i, j, k)], cl = coarse[cidx(&cd, i / 2, j / 2, k / 2)];
                if (fl == MGO_DIRICHLET && cl != MGO_DIRICHLET) return 0;
                if (is_active(fl) && cl == MGO_EXTERIOR) return 0;
            }
    for (int k = 0; k < cd.nz; ++k)
        for (int j = 0; j < cd.ny; ++j)
            for (int i = 0; i < cd.nx; ++i) {
                int fd_ = 0, fi = 0, fe = 0;
                for (int ch = 0; ch < 8; ++ch) {
                    const int l = fine[cidx(&fd, 2 * i + (ch & 1), 2 * j + ((ch >> 1) & 1), 2 * k + ((ch >> 2) & 1))];
                    if (l == MGO_DIRICHLET) fd_ = 1;
                    else if (is_active(l)) fi = 1;
                    else fe = 1;
                }
                const int cl = coarse[cidx(&cd, i, j, k)];
                if (cl == MGO_DIRICHLET && !fd_) return 0;
                if (is_active(cl) && (fd_ || !fi)) return 0;
                if (cl == MGO_EXTERIOR && (fd_ || fi || !fe)) return 0;
            }
    return 1;
}

/* computeGhostFluidWeight (Util.h:25-42). */
double mgo_ghost_fluid_weight(double phi0, double phi1)
{
    double theta = 0;
    if (phi0 < 0) {
        if (phi1 < 0) theta = 1;
        else if (phi1 >= 0) theta = phi0 / (phi0 - phi1);
    } else if (phi1 < 0)
        theta = phi1 / (phi1 - phi0);
    return theta;
}

/* ------------------------------------------------------------------------------------------
 * GeometricMultigridPoissonSolver  (MG.cpp:135-418 ctor, 420-881 applyVCycle)
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int levels, alloc_levels, use_gs, band_width, band_iters;
    double omega; /* damping of the Jacobi and band sweeps; the reference hard-wires 2. / 3. (Ops.h:291, 554) */
    int pre_sweeps, post_sweeps; /* full-domain smoother sweeps per stroke; the reference hard-wires 1 (MG.cpp:466-486, 740-757) */
    dims_t *dims;
    int32_t **lab;
    real **x, **b, **r; /* x[0], b[0] unused (caller's grids) */
    int32_t **band;
    int64_t *band_n;
    real *w[3]; /* copies of the fine weights */
    real *scratch;
    /* coarsest level: banded Cholesky of the unit-weight matrix */
    int cn, cbw;
    int32_t *cindex; /* coarsest grid -> unknown id, -1 inactive */
    double *cL;      /* cn x (cbw+1), row-major, cL[r*(cbw+1)+ (cbw-(r-c))] = L(r,c) */
    void *fast;      /* state of the optimised comparator (mgo_solver_apply_vcycle_fast), made on first use */
} mgo_solver;
static void fast_free(mgo_solver *s);

static int build_coarse_direct(mgo_solver *s)
{
    const int L = s->levels - 1;
    const dims_t d = s->dims[L];
    const int32_t *lab = s->lab[L];
    const size_t n = (size_t)d.nx * d.ny * d.nz;
    s->cindex = (int32_t *)malloc(n * sizeof(int32_t));
    int cnt = 0;
    /* numbering: tile order, then in-tile x-fastest order (MG.cpp:296-324) -- while the coarsest grid is a single tile,
     * which is every hierarchy the reference's own level rule produces.  A larger coarsest level (BASELINE configs 3 / 5:
     * 512^3 with 5 levels, 32^3 = 2 x 2 x 2 tiles) is numbered cell by cell instead: the numbering only decides the band
     * width of this file's Cholesky factor (tile order: ~12 000, cell order: nx * ny <= 1024), not the solution of the
     * system -- Eigen's SimplicialCholesky reorders by AMD anyway (MG.cpp:405-411). */
    const int tx = (d.nx + TILE - 1) / TILE, ty = (d.ny + TILE - 1) / TILE, tz = (d.nz + TILE - 1) / TILE;
    for (size_t c = 0; c < n; ++c) s->cindex[c] = -1;
    if (tx * ty * tz == 1) {
        for (int k = 0; k < d.nz; ++k)
            for (int j = 0; j < d.ny; ++j)
                for (int i = 0; i < d.nx; ++i) {
                    const size_t c = cidx(&d, i, j, k);
                    if (is_active(lab[c])) s->cindex[c] = cnt++;
                }
    } else {
        for (size_t c = 0; c < n; ++c)
            if (is_active(lab[c])) s->cindex[c] = cnt++;
    }
    s->cn = cnt;
    const ptrdiff_t stride[3] = {1, d.nx, (ptrdiff_t)d.nx * d.ny};
    int bw = 0;
    for (size_t c = 0; c < n; ++c) {
        if (s->cindex[c] < 0) continue;
        for (int axis = 0; axis < 3; ++axis)
            for (int dir = 0; dir < 2; ++dir) {
                const size_t nb = c + (dir ? stride[axis] : -stride[axis]);
                if (s->cindex[nb] >= 0) {
                    int dd = abs(s->cindex[nb] - s->cindex[c]);
                    if (dd > bw) bw = dd;
                }
            }
    }
    s->cbw = bw;
    const int W = bw + 1;
    double *A = (double *)calloc((size_t)cnt * W, sizeof(double));
    /* rows (MG.cpp:359-382): -1 per active neighbour, diagonal = #active + #DIRICHLET neighbours */
    for (size_t c = 0; c < n; ++c) {
        const int r = s->cindex[c];
        if (r < 0) continue;
        double diag = 0;
        for (int axis = 0; axis < 3; ++axis)
            for (int dir = 0; dir < 2; ++dir) {
                const size_t nb = c + (dir ? stride[axis] : -stride[axis]);
                if (is_active(lab[nb])) {
                    const int q = s->cindex[nb];
                    if (q < r) A[(size_t)r * W + (bw - (r - q))] = -1;
                    diag += 1;
                } else if (lab[nb] == MGO_DIRICHLET)
                    diag += 1;
            }
        A[(size_t)r * W + bw] = diag;
    }
    /* banded Cholesky A = L L^T (stands in for Eigen::SimplicialCholesky, MG.cpp:405-411; an exact
     * SPD direct solve, so it agrees with any other to round-off) */
    for (int r = 0; r < cnt; ++r) {
        const int c0 = r - bw > 0 ? r - bw : 0;
        for (int c = c0; c <= r; ++c) {
            double sum = A[(size_t)r * W + (bw - (r - c))];
            const int m0 = c - bw > c0 ? c - bw : c0;
            for (int m = m0; m < c; ++m)
                sum -= A[(size_t)r * W + (bw - (r - m))] * A[(size_t)c * W + (bw - (c - m))];
            if (c == r) {
                if (sum <= 0) {
                    free(A);
                    return -1;
                }
                A[(size_t)r * W + bw] = sqrt(sum);
            } else
                A[(size_t)r * W + (bw - (r - c))] = sum / A[(size_t)c * W + bw];
        }
    }
    s->cL = A;
    return 0;
}

static void coarse_solve(const mgo_solver *s, double *v) /* in place, v[cn] */
{
    const int n = s->cn, bw = s->cbw, W = bw + 1;
    const double *Lm = s->cL;
    for (int r = 0; r < n; ++r) {
        double sum = v[r];
        const int c0 = r - bw > 0 ? r - bw : 0;
        for (int c = c0; c < r; ++c) sum -= Lm[(size_t)r * W + (bw - (r - c))] * v[c];
        v[r] = sum / Lm[(size_t)r * W + bw];
    }
    for (int r = n - 1; r >= 0; --r) {
        double sum = v[r];
        const int c1 = r + bw < n - 1 ? r + bw : n - 1;
        for (int c = r + 1; c <= c1; ++c) sum -= Lm[(size_t)c * W + (bw - (c - r))] * v[c];
        v[r] = sum / Lm[(size_t)r * W + bw];
    }
}

void mgo_solver_destroy(mgo_solver *s)
{
    if (!s) return;
    fast_free(s);
    for (int l = 0; l < s->alloc_levels; ++l) {
        if (s->lab) free(s->lab[l]);
        if (s->x) free(s->x[l]);
        if (s->b) free(s->b[l]);
        if (s->r) free(s->r[l]);
        if (s->band) free(s->band[l]);
    }
    free(s->dims);
    free(s->lab);
    free(s->x);
    free(s->b);
    free(s->r);
    free(s->band);
    free(s->band_n);
    for (int a = 0; a < 3; ++a) free(s->w[a]);
    free(s->scratch);
    free(s->cindex);
    free(s->cL);
    free(s);
}

mgo_solver *mgo_solver_create(const int32_t *labels, const real *wx, const real *wy, const real *wz,
                              int nx, int ny, int nz, int mg_levels, int use_gs)
{
    mgo_solver *s = (mgo_solver *)calloc(1, sizeof(mgo_solver));
    s->levels = mg_levels;
    s->alloc_levels = mg_levels;
    s->use_gs = use_gs;
    s->band_width = 3; /* MG.cpp:141 */
    s->band_iters = 3; /* MG.cpp:142 */
    s->omega = 2. / 3.;
    s->pre_sweeps = s->post_sweeps = 1;
    s->dims = (dims_t *)calloc((size_t)mg_levels, sizeof(dims_t));
    s->lab = (int32_t **)calloc((size_t)mg_levels, sizeof(void *));
    s->x = (real **)calloc((size_t)mg_levels, sizeof(void *));
    s->b = (real **)calloc((size_t)mg_levels, sizeof(void *));
    s->r = (real **)calloc((size_t)mg_levels, sizeof(void *));
    s->band = (int32_t **)calloc((size_t)mg_levels, sizeof(void *));
    s->band_n = (int64_t *)calloc((size_t)mg_levels, sizeof(int64_t));
    const size_t n0 = (size_t)nx * ny * nz;
    s->dims[0].nx = nx;
    s->dims[0].ny = ny;
    s->dims[0].nz = nz;
    s->lab[0] = (int32_t *)malloc(n0 * sizeof(int32_t));
    memcpy(s->lab[0], labels, n0 * sizeof(int32_t));
    const size_t wn[3] = {(size_t)(nx + 1) * ny * nz, (size_t)nx * (ny + 1) * nz, (size_t)nx * ny * (nz + 1)};
    const real *win[3] = {wx, wy, wz};
    for (int a = 0; a < 3; ++a) {
        s->w[a] = (real *)malloc(wn[a] * sizeof(real));
        memcpy(s->w[a], win[a], wn[a] * sizeof(real));
    }
    /* coarsening with the early cap (MG.cpp:238-253): a level without solvable cells sets
     * levels = level - 1 (one more than strictly needed is dropped, as in the reference). */
    for (int l = 1; l < s->levels; ++l) {
        const dims_t f = s->dims[l - 1];
        s->dims[l].nx = f.nx / 2;
        s->dims[l].ny = f.ny / 2;
        s->dims[l].nz = f.nz / 2;
        const size_t n = (size_t)s->dims[l].nx * s->dims[l].ny * s->dims[l].nz;
        s->lab[l] = (int32_t *)malloc(n * sizeof(int32_t));
        mgo_build_coarse_labels(s->lab[l], s->lab[l - 1], f.nx, f.ny, f.nz);
        if (!has_solvable(s->lab[l], n)) {
            for (int q = l - 1 > 0 ? l - 1 : 1; q <= l; ++q) {
                free(s->lab[q]);
                s->lab[q] = NULL;
            }
            s->levels = l - 1;
            break;
        }
    }
    if (s->levels < 1) {
        mgo_solver_destroy(s);
        return NULL;
    }
    for (int l = 0; l < s->levels; ++l) {
        const dims_t d = s->dims[l];
        const size_t n = (size_t)d.nx * d.ny * d.nz;
        if (l > 0) {
            s->x[l] = (real *)calloc(n, sizeof(real));
            s->b[l] = (real *)calloc(n, sizeof(real));
        }
        s->r[l] = (real *)calloc(n, sizeof(real));
        s->band_n[l] = mgo_build_boundary_cells(s->lab[l], d.nx, d.ny, d.nz, s->band_width, &s->band[l]);
    }
    s->scratch = (real *)malloc(n0 * sizeof(real));
    /* With one level applyVCycle returns before the direct solve (MG.cpp:516-517); the reference still
     * factorises the fine matrix there (sparse Cholesky), which nothing ever uses -- skipped, a banded
     * factor of a whole fine grid would take hours. */
    if (s->levels > 1 && build_coarse_direct(s) != 0) {
        mgo_solver_destroy(s);
        return NULL;
    }
    return s;
}

int mgo_solver_levels(const mgo_solver *s) { return s->levels; }
int64_t mgo_solver_band_count(const mgo_solver *s, int level) { return s->band_n[level]; }
const int32_t *mgo_solver_band(const mgo_solver *s, int level) { return s->band[level]; }
const int32_t *mgo_solver_labels(const mgo_solver *s, int level) { return s->lab[level]; }
void mgo_solver_level_dims(const mgo_solver *s, int level, int *out)
{
    out[0] = s->dims[level].nx;
    out[1] = s->dims[level].ny;
    out[2] = s->dims[level].nz;
}
int mgo_solver_coarse_unknowns(const mgo_solver *s) { return s->cn; }

/* the direct solve of MG.cpp:669-692 alone, on grids of the coarsest level (test hook) */
void mgo_solver_coarse_solve(const mgo_solver *s, real *x, const real *b)
{
    const dims_t d = s->dims[s->levels - 1];
    const size_t n = (size_t)d.nx * d.ny * d.nz;
    double *v = (double *)calloc((size_t)(s->cn > 0 ? s->cn : 1), sizeof(double));
    for (size_t c = 0; c < n; ++c)
        if (s->cindex[c] >= 0) v[s->cindex[c]] = (double)b[c];
    coarse_solve(s, v);
    for (size_t c = 0; c < n; ++c)
        if (s->cindex[c] >= 0) x[c] = (real)v[s->cindex[c]];
    free(v);
}

/* Benchmark variants (BASELINE config 1: "2+2 damped-Jacobi sweeps"): the full-domain smoother of a stroke repeated
 * `pre` times on the way down and `post` times on the way up.  1 / 1 is the reference's schedule. */
void mgo_solver_set_sweeps(mgo_solver *s, int pre, int post)
{
    s->pre_sweeps = pre > 0 ? pre : 1;
    s->post_sweeps = post > 0 ? post : 1;
}

/* The three smoothing options the reference hard-wires (MG.cpp:141-142, Ops.h:291, 554), per solver: the band lists of
 * every level are rebuilt at `band_width`, the band stage runs `band_iters` passes (0: none) and every damped sweep uses
 * `omega`.  Returns -1 (and changes nothing) for band_width < 1, band_iters < 0 or a non-positive omega. */
int mgo_solver_set_band_options(mgo_solver *s, int band_width, int band_iters, double omega)
{
    if (band_width < 1 || band_iters < 0 || !(omega > 0)) return -1;
    if (band_width != s->band_width) {
        fast_free(s); /* its band rows follow the lists */
        for (int l = 0; l < s->levels; ++l) {
            const dims_t d = s->dims[l];
            free(s->band[l]);
            s->band[l] = NULL;
            s->band_n[l] = mgo_build_boundary_cells(s->lab[l], d.nx, d.ny, d.nz, band_width, &s->band[l]);
        }
        s->band_width = band_width;
    }
    s->band_iters = band_iters;
    s->omega = omega;
    return 0;
}

static void smooth_stroke(mgo_solver *s, int l, real *x, const real *b, int down)
{
    const dims_t d = s->dims[l];
    const real *wx = l == 0 ? s->w[0] : NULL, *wy = l == 0 ? s->w[1] : NULL, *wz = l == 0 ? s->w[2] : NULL;
    for (int it = 0; it < s->band_iters; ++it)
        mgo_boundary_jacobi_weighted(x, b, s->lab[l], s->band[l], s->band_n[l], wx, wy, wz, d.nx, d.ny, d.nz, s->omega);
    for (int rep = 0; rep < (down ? s->pre_sweeps : s->post_sweeps); ++rep) {
        if (s->use_gs) {
            if (down) { /* MG.cpp:466-479: odd fwd, even fwd */
                mgo_tiled_gs(x, b, s->lab[l], wx, wy, wz, d.nx, d.ny, d.nz, 1, 1);
                mgo_tiled_gs(x, b, s->lab[l], wx, wy, wz, d.nx, d.ny, d.nz, 0, 1);
            } else { /* MG.cpp:740-751: even bwd, odd bwd */
                mgo_tiled_gs(x, b, s->lab[l], wx, wy, wz, d.nx, d.ny, d.nz, 0, 0);
                mgo_tiled_gs(x, b, s->lab[l], wx, wy, wz, d.nx, d.ny, d.nz, 1, 0);
            }
        } else
            mgo_jacobi_weighted(x, b, s->lab[l], wx, wy, wz, d.nx, d.ny, d.nz, s->scratch, s->omega);
    }
    for (int it = 0; it < s->band_iters; ++it)
        mgo_boundary_jacobi_weighted(x, b, s->lab[l], s->band[l], s->band_n[l], wx, wy, wz, d.nx, d.ny, d.nz, s->omega);
}

/* applyVCycle (MG.cpp:420-881). */
void mgo_solver_apply_vcycle(mgo_solver *s, real *x, const real *b, int use_initial_guess)
{
    const int L = s->levels;
    const dims_t d0 = s->dims[0];
    const size_t n0 = (size_t)d0.nx * d0.ny * d0.nz;
    if (!use_initial_guess) memset(x, 0, n0 * sizeof(real)); /* MG.cpp:439-440 */
    smooth_stroke(s, 0, x, b, 1);
    if (L == 1) return; /* MG.cpp:516-517 */
    mgo_residual(s->r[0], x, b, s->lab[0], s->w[0], s->w[1], s->w[2], d0.nx, d0.ny, d0.nz);
    mgo_downsample(s->b[1], s->r[0], s->lab[1], s->dims[1].nx, s->dims[1].ny, s->dims[1].nz);
    for (int l = 1; l < L - 1; ++l) { /* MG.cpp:557-667 */
        const dims_t d = s->dims[l];
        memset(s->x[l], 0, (size_t)d.nx * d.ny * d.nz * sizeof(real));
        smooth_stroke(s, l, s->x[l], s->b[l], 1);
        mgo_residual(s->r[l], s->x[l], s->b[l], s->lab[l], NULL, NULL, NULL, d.nx, d.ny, d.nz);
        mgo_downsample(s->b[l + 1], s->r[l], s->lab[l + 1], s->dims[l + 1].nx, s->dims[l + 1].ny,
                       s->dims[l + 1].nz);
    }
    { /* direct solve, MG.cpp:669-692 */
        const dims_t d = s->dims[L - 1];
        const size_t n = (size_t)d.nx * d.ny * d.nz;
        double *v = (double *)calloc((size_t)(s->cn > 0 ? s->cn : 1), sizeof(double));
        for (size_t c = 0; c < n; ++c)
            if (s->cindex[c] >= 0) v[s->cindex[c]] = (double)s->b[L - 1][c];
        coarse_solve(s, v);
        for (size_t c = 0; c < n; ++c)
            if (s->cindex[c] >= 0) s->x[L - 1][c] = (real)v[s->cindex[c]];
        free(v);
    }
    for (int l = L - 2; l >= 1; --l) { /* MG.cpp:695-784 */
        const dims_t d = s->dims[l];
        mgo_upsample_add(s->x[l], s->x[l + 1], s->lab[l], d.nx, d.ny, d.nz);
        smooth_stroke(s, l, s->x[l], s->b[l], 0);
    }
    mgo_upsample_add(x, s->x[1], s->lab[0], d0.nx, d0.ny, d0.nz); /* MG.cpp:787-880 */
    smooth_stroke(s, 0, x, b, 0);
}

/* ------------------------------------------------------------------------------------------
 * The OPTIMISED CPU comparator ("an optimised CPU variant is reported separately so the speed-up is not
 * inflated").  Same V-cycle and the same operators as mgo_solver_apply_vcycle with the Jacobi smoother and one sweep per
 * stroke (the six neighbours of an INTERIOR cell are summed before they are subtracted: results agree to round-off, not bit
 * for bit); what changes is what the reference's structure costs and a CPU does not need:
 *   - no whole-grid copy per Jacobi sweep (Ops.h:289): the two sweeps of a level ping-pong between the iterate and one
 *     spare grid -- down x -> t, up t -> x -- so the result lands where the caller expects it with no copy at all;
 *   - the residual in ONE pass (the reference clears, applies A, adds: Ops.h:728-731);
 *   - one-byte labels for the streaming passes (the reference's are 4-byte ints); BOUNDARY cells, a few percent, still go
 *     through computeLaplacian with the int labels and the face weights;
 *   - INTERIOR runs of a row in a branch-free inner loop the compiler vectorises; OpenMP over x-rows.
 * Timed by bench.py's cpu_baseline as "optimised_variant" (build with -DMGO_REAL=float for fp32 storage).  Checked against
 * the faithful cycle in tests/test_oracle_properties.py.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    uint8_t **lab8;
    real **spare; /* one spare grid per smoothed level */
    /* band passes without look-ups: per band cell its linear index and its operator row (computeLaplacian, Ops.h:177-260,
     * evaluated once: six off-diagonal weights in the reference's visiting order -x +x -y +y -z +z, 0 for a neighbour that
     * contributes nothing, then the diagonal), SoA */
    int64_t **bcell;
    real **brow; /* 7 x band_n */
    real **btmp;
} mgo_fast;
static mgo_fast *fast_of(mgo_solver *s)
{
    if (s->fast) return (mgo_fast *)s->fast;
    mgo_fast *f = (mgo_fast *)calloc(1, sizeof(mgo_fast));
    f->lab8 = (uint8_t **)calloc((size_t)s->levels, sizeof(uint8_t *));
    f->spare = (real **)calloc((size_t)s->levels, sizeof(real *));
    f->bcell = (int64_t **)calloc((size_t)s->levels, sizeof(int64_t *));
    f->brow = (real **)calloc((size_t)s->levels, sizeof(real *));
    f->btmp = (real **)calloc((size_t)s->levels, sizeof(real *));
    for (int l = 0; l < s->levels; ++l) {
        const dims_t d = s->dims[l];
        const size_t n = (size_t)d.nx * d.ny * d.nz;
        f->lab8[l] = (uint8_t *)malloc(n);
        if (l < s->levels - 1) f->spare[l] = (real *)calloc(n, sizeof(real));
        const int32_t *lab = s->lab[l];
        uint8_t *l8 = f->lab8[l];
#pragma omp parallel for schedule(static)
        for (int64_t c = 0; c < (int64_t)n; ++c) l8[c] = (uint8_t)lab[c];
        if (l == s->levels - 1) continue;
        const int64_t nb = s->band_n[l];
        f->bcell[l] = (int64_t *)malloc((size_t)(nb > 0 ? nb : 1) * sizeof(int64_t));
        f->brow[l] = (real *)malloc((size_t)(nb > 0 ? nb : 1) * 7 * sizeof(real));
        f->btmp[l] = (real *)malloc((size_t)(nb > 0 ? nb : 1) * sizeof(real));
        const real *w[3] = {s->w[0], s->w[1], s->w[2]};
        const int weighted = l == 0;
        const ptrdiff_t stride[3] = {1, d.nx, (ptrdiff_t)d.nx * d.ny};
#pragma omp parallel for schedule(static)
        for (int64_t t = 0; t < nb; ++t) {
            const int i = s->band[l][3 * t], j = s->band[l][3 * t + 1], k = s->band[l][3 * t + 2];
            const size_t c = cidx(&d, i, j, k);
            f->bcell[l][t] = (int64_t)c;
            real diag = 0;
            for (int axis = 0; axis < 3; ++axis)
                for (int dir = 0; dir < 2; ++dir) { /* Ops.h:191-256 */
                    const int nl = lab[c + (dir ? stride[axis] : -stride[axis])];
                    real wt = 0, dg = 0;
                    if (lab[c] == MGO_INTERIOR) wt = 1, dg = 1;
                    else if (nl == MGO_INTERIOR) wt = 1, dg = 1;
                    else if (nl == MGO_BOUNDARY) wt = dg = weighted ? w[axis][fidx(&d, axis, i, j, k, dir)] : (real)1;
                    else if (nl == MGO_DIRICHLET) dg = weighted ? w[axis][fidx(&d, axis, i, j, k, dir)] : (real)1;
                    f->brow[l][(size_t)(2 * axis + dir) * nb + t] = wt;
                    diag += dg;
                }
            f->brow[l][(size_t)6 * nb + t] = diag;
        }
    }
    s->fast = f;
    return f;
}
static void fast_free(mgo_solver *s)
{
    mgo_fast *f = (mgo_fast *)s->fast;
    if (!f) return;
    for (int l = 0; l < s->levels; ++l) {
        free(f->lab8[l]);
        free(f->spare[l]);
        free(f->bcell[l]);
        free(f->brow[l]);
        free(f->btmp[l]);
    }
    free(f->lab8);
    free(f->spare);
    free(f->bcell);
    free(f->brow);
    free(f->btmp);
    free(f);
    s->fast = NULL;
}
/* one full-domain pass over level l: mode 0 out = Jacobi(x) (inactive cells: out = x), mode 1 out = b - A x (inactive: 0) */
static void fast_pass(mgo_solver *s, int l, int mode, real *out, const real *x, const real *b)
{
    const mgo_fast *f = (const mgo_fast *)s->fast;
    const dims_t d = s->dims[l];
    const uint8_t *l8 = f->lab8[l];
    const int32_t *lab = s->lab[l];
    const real *w[3] = {s->w[0], s->w[1], s->w[2]};
    const real *const *wp = l == 0 ? w : NULL;
    const ptrdiff_t sy = d.nx, sz = (ptrdiff_t)d.nx * d.ny;
    const real damped = s->omega, sixth = (real)6;
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = 0; k < d.nz; ++k)
        for (int j = 0; j < d.ny; ++j) {
            const size_t row = cidx(&d, 0, j, k);
            int i = 0;
            while (i < d.nx) {
                int e = i;
                while (e < d.nx && l8[row + e] == MGO_INTERIOR) ++e; /* a run of INTERIOR cells: Ops.h:191-207, no look-ups */
                const real *xc = x + row, *bc = b + row;
                real *oc = out + row;
#pragma omp simd
                for (int q = i; q < e; ++q) {
                    const real lap = sixth * xc[q] - (xc[q - 1] + xc[q + 1] + xc[q - sy] + xc[q + sy] + xc[q - sz] + xc[q + sz]);
                    const real res = bc[q] - lap;
                    oc[q] = mode == 0 ? xc[q] + damped * (res / sixth) : res;
                }
                if (e < d.nx) {
                    const size_t c = row + e;
                    if (l8[c] == MGO_BOUNDARY) {
                        real lap, diag;
                        laplacian(&d, x, lab, wp, e, j, k, &lap, &diag);
                        const real res = b[c] - lap;
                        out[c] = mode == 0 ? x[c] + damped * (res / diag) : res;
                    } else
                        out[c] = mode == 0 ? x[c] : (real)0;
                    ++e;
                }
                i = e;
            }
        }
}
/* boundaryJacobiPoissonSmoother x band_iters (Ops.h:524-619) over the precomputed rows: compute into a list, then scatter */
static void fast_band(mgo_solver *s, int l, real *x, const real *b)
{
    const mgo_fast *f = (const mgo_fast *)s->fast;
    const dims_t d = s->dims[l];
    const int64_t nb = s->band_n[l];
    const int64_t *cell = f->bcell[l];
    const real *row = f->brow[l];
    real *tmp = f->btmp[l];
    const ptrdiff_t sy = d.nx, sz = (ptrdiff_t)d.nx * d.ny;
    const real damped = s->omega;
    for (int it = 0; it < s->band_iters; ++it) {
#pragma omp parallel for schedule(static)
        for (int64_t t = 0; t < nb; ++t) {
            const real *xc = x + cell[t];
            real lap = 0;
            lap -= row[t] * xc[-1];
            lap -= row[nb + t] * xc[1];
            lap -= row[2 * nb + t] * xc[-sy];
            lap -= row[3 * nb + t] * xc[sy];
            lap -= row[4 * nb + t] * xc[-sz];
            lap -= row[5 * nb + t] * xc[sz];
            const real diag = row[6 * nb + t];
            lap += diag * xc[0];
            real res = b[cell[t]] - lap;
            res /= diag;
            tmp[t] = xc[0] + damped * res;
        }
#pragma omp parallel for schedule(static)
        for (int64_t t = 0; t < nb; ++t) x[cell[t]] = tmp[t];
    }
}
static void fast_downsample(real *coarse, const real *fine, const uint8_t *cl8, dims_t cd)
{
    static const real rw[4] = {1. / 8., 3. / 8., 3. / 8., 1. / 8.};
    const dims_t fd = {2 * cd.nx, 2 * cd.ny, 2 * cd.nz};
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = 0; k < cd.nz; ++k)
        for (int j = 0; j < cd.ny; ++j)
            for (int i = 0; i < cd.nx; ++i) {
                const size_t c = cidx(&cd, i, j, k);
                if (!is_active(cl8[c])) {
                    coarse[c] = 0;
                    continue;
                }
                real sum = 0;
                const real *p0 = fine + cidx(&fd, 2 * i - 1, 2 * j - 1, 2 * k - 1);
                for (int zo = 0; zo < 4; ++zo)
                    for (int yo = 0; yo < 4; ++yo) {
                        const real *p = p0 + ((size_t)zo * fd.ny + yo) * fd.nx;
                        const real wyz = rw[yo] * rw[zo];
                        sum += rw[0] * wyz * p[0];
                        sum += rw[1] * wyz * p[1];
                        sum += rw[2] * wyz * p[2];
                        sum += rw[3] * wyz * p[3];
                    }
                coarse[c] = sum;
            }
}
static void fast_upsample_add(real *fine, const real *coarse, const uint8_t *fl8, dims_t fd)
{
    const dims_t cd = {fd.nx / 2, fd.ny / 2, fd.nz / 2};
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = 1; k < fd.nz - 1; ++k)
        for (int j = 1; j < fd.ny - 1; ++j) {
            const int bj = (j - 1) >> 1, bk = (k - 1) >> 1;
            const real fy = (j & 1) ? .25 : .75, fz = (k & 1) ? .25 : .75;
            const real *r00 = coarse + cidx(&cd, 0, bj, bk), *r10 = r00 + cd.nx, *r01 = r00 + (size_t)cd.nx * cd.ny, *r11 = r01 + cd.nx;
            const size_t row = cidx(&fd, 0, j, k);
            for (int i = 1; i < fd.nx - 1; ++i) {
                if (!is_active(fl8[row + i])) continue;
                const int bi = (i - 1) >> 1;
                const real fx = (i & 1) ? .25 : .75;
                const real t = lerp(lerp(lerp(r00[bi], r00[bi + 1], fx), lerp(r10[bi], r10[bi + 1], fx), fy),
                                    lerp(lerp(r01[bi], r01[bi + 1], fx), lerp(r11[bi], r11[bi + 1], fx), fy), fz);
                fine[row + i] = fine[row + i] + 4. * t;
            }
        }
}
/* applyVCycle (MG.cpp:420-881), Jacobi smoother, one sweep per stroke.  Returns -1 where the faithful cycle must be used. */
int mgo_solver_apply_vcycle_fast(mgo_solver *s, real *x, const real *b, int use_initial_guess)
{
    if (s->use_gs || s->pre_sweeps != 1 || s->post_sweeps != 1 || s->levels < 2) return -1;
    const mgo_fast *f = fast_of(s);
    const int L = s->levels;
    real *cur[64];
    for (int l = 0; l < L - 1; ++l) {
        const dims_t d = s->dims[l];
        const size_t n = (size_t)d.nx * d.ny * d.nz;
        real *xl = l == 0 ? x : s->x[l];
        const real *bl = l == 0 ? b : s->b[l];
        if (l > 0 || !use_initial_guess) {
#pragma omp parallel for schedule(static)
            for (int k = 0; k < d.nz; ++k) memset(xl + (size_t)k * d.nx * d.ny, 0, (size_t)d.nx * d.ny * sizeof(real));
        }
        (void)n;
        fast_band(s, l, xl, bl);
        fast_pass(s, l, 0, f->spare[l], xl, bl); /* down: x -> spare */
        cur[l] = f->spare[l];
        fast_band(s, l, cur[l], bl);
        fast_pass(s, l, 1, s->r[l], cur[l], bl);
        fast_downsample(s->b[l + 1], s->r[l], f->lab8[l + 1], s->dims[l + 1]);
    }
    mgo_solver_coarse_solve(s, s->x[L - 1], s->b[L - 1]);
    for (int l = L - 2; l >= 0; --l) {
        real *xl = l == 0 ? x : s->x[l];
        const real *bl = l == 0 ? b : s->b[l];
        fast_upsample_add(cur[l], s->x[l + 1], f->lab8[l], s->dims[l]);
        fast_band(s, l, cur[l], bl);
        fast_pass(s, l, 0, xl, cur[l], bl); /* up: spare -> x */
        fast_band(s, l, xl, bl);
    }
    return 0;
}

/* solveGeometricConjugateGradient (CG.h:18-207) with A = applyPoissonMatrix and
 * M^-1 = applyVCycle (precond 1, Plug.cpp:463-483) or the diagonal (precond 0, Plug.cpp:485-618).
 * stats[0] = iterations, stats[1] = drifted relative L2 error, stats[2] = recomputed relative L2
 * error.  Returns 0 ok, 1 rhs zero, 2 already converged. */
int mgo_solve_pcg(mgo_solver *s, real *x, const real *b, double tol, int max_iter, int precond,
                  double *stats, double *rel_history)
{
    const dims_t d = s->dims[0];
    const int32_t *lab = s->lab[0];
    const size_t n = (size_t)d.nx * d.ny * d.nz;
    const int nx = d.nx, ny = d.ny, nz = d.nz;
    stats[0] = stats[1] = stats[2] = 0;
    const double rhs2 = mgo_squared_l2(b, lab, nx, ny, nz);
    if (rhs2 == 0) return 1; /* CG.h:36-40 */
    real *r = (real *)calloc(n, sizeof(real)), *p = (real *)calloc(n, sizeof(real));
    real *z = (real *)calloc(n, sizeof(real)), *t = (real *)calloc(n, sizeof(real));
    real *dinv = NULL;
    if (!precond) { /* Plug.cpp:520-548: 1/6 interior, 1/sum of the six face weights boundary */
        dinv = (real *)calloc(n, sizeof(real));
#pragma omp parallel for collapse(2) schedule(static)
        for (int k = 0; k < nz; ++k)
            for (int j = 0; j < ny; ++j)
                for (int i = 0; i < nx; ++i) {
                    const size_t c = cidx(&d, i, j, k);
                    if (lab[c] == MGO_INTERIOR) dinv[c] = 1. / 6.;
                    else if (lab[c] == MGO_BOUNDARY) {
                        real dg = 0;
                        for (int axis = 0; axis < 3; ++axis)
                            for (int dir = 0; dir < 2; ++dir) dg += s->w[axis][fidx(&d, axis, i, j, k, dir)];
                        dinv[c] = 1. / dg;
                    }
                }
    }
#define PRECOND(dst, src)                                                                          \
    do {                                                                                           \
        if (precond) mgo_solver_apply_vcycle(s, dst, src, 0);                                      \
        else {                                                                                     \
            _Pragma("omp parallel for schedule(static)") for (int64_t c = 0; c < (int64_t)n; ++c)  \
                if (is_active(lab[c])) dst[c] = src[c] * dinv[c];                                  \
        }                                                                                          \
    } while (0)
    int ret = 0, it = 0;
    mgo_apply_poisson(r, x, lab, s->w[0], s->w[1], s->w[2], nx, ny, nz); /* CG.h:50-51 */
    mgo_add_vectors(r, b, r, -1, lab, (int64_t)n);
    double res2 = mgo_squared_l2(r, lab, nx, ny, nz);
    const double thresh = tol * tol * rhs2; /* CG.h:58 */
    if (res2 < thresh) {
        ret = 2;
        stats[1] = sqrt(res2 / rhs2);
        goto done;
    }
    PRECOND(p, r);                                    /* CG.h:75 */
    double abs_new = mgo_dot(p, r, lab, nx, ny, nz);  /* CG.h:86 */
    for (; it < max_iter; ++it) {
        mgo_apply_poisson(t, p, lab, s->w[0], s->w[1], s->w[2], nx, ny, nz); /* CG.h:110 */
        const double alpha = abs_new / mgo_dot(p, t, lab, nx, ny, nz);        /* CG.h:121 */
        mgo_add_to_vector(x, p, (real)alpha, lab, (int64_t)n);                /* CG.h:132 */
        mgo_add_to_vector(r, t, (real)-alpha, lab, (int64_t)n);               /* CG.h:143 */
        res2 = mgo_squared_l2(r, lab, nx, ny, nz);                            /* CG.h:153 */
        if (rel_history) rel_history[it] = sqrt(res2 / rhs2);
        if (res2 < thresh) break; /* CG.h:161 (iteration counter not advanced, as there) */
        PRECOND(z, r);            /* CG.h:168 */
        const double abs_old = abs_new;
        abs_new = mgo_dot(z, r, lab, nx, ny, nz); /* CG.h:180 */
        const double beta = abs_new / abs_old;
        mgo_add_vectors(p, z, p, (real)beta, lab, (int64_t)n); /* CG.h:191 */
    }
    stats[0] = it;
    stats[1] = sqrt(res2 / rhs2);
    mgo_apply_poisson(r, x, lab, s->w[0], s->w[1], s->w[2], nx, ny, nz); /* CG.h:203-205 */
    mgo_add_vectors(r, b, r, -1, lab, (int64_t)n);
    stats[2] = sqrt(mgo_squared_l2(r, lab, nx, ny, nz) / rhs2);
done:
#undef PRECOND
    free(r);
    free(p);
    free(z);
    free(t);
    free(dinv);
    return ret;
}
