/*
 * ref_driver.cpp -- extern "C" entries over flat arrays that call the reference's own solver core
 * (rgoldade/GeometricMultigridPressureSolver, Source/HDK_GeometricMultigrid{Operators,PoissonSolver}.* and
 * HDK_GeometricCGPoissonSolver.h), compiled against the stand-in headers of oracle/ref_standin/ into
 * oracle/_ref/libmgref.so (`make -C oracle ref`).  TEST INFRASTRUCTURE ONLY.
 *
 * This file names the reference's headers in #include lines and holds none of their text.  The entries have
 * the shapes and argument order of the mgo_* entries of mg_oracle.c (prefix mgr_), with SolveReal = StoreReal
 * = double; grids are dense, x fastest, which is also the stand-in UT_VoxelArray's storage.  Differences:
 *   - every entry returns 0, or -1 after a reference assertion (armed in this build) or a stand-in bounds
 *     check failed: mgr_last_error() has the text.  Reductions return NaN instead;
 *   - mgr_downsample / mgr_upsample_add take the other level's labels as a last argument (the reference
 *     reads them in its assertions);
 *   - the hierarchy is not read out of the solver object (its members are private): per-level labels and
 *     band lists come from mgr_build_coarse_labels / mgr_build_boundary_cells, the functions its constructor
 *     calls.
 */
#include <cstring>
#include <limits>
#include <memory>
#include <sstream>
#include <string>

#include "HDK_GeometricMultigridOperators.h"
#include "HDK_GeometricMultigridPoissonSolver.h"
#include "HDK_GeometricCGPoissonSolver.h"

namespace
{
namespace Ops = HDK::GeometricMultigridOperators;
using Real = double;
using Grid = UT_VoxelArray<Real>;
using Labels = UT_VoxelArray<int>;
using Weights = std::array<Grid, 3>;

std::string theLastError;

// the reference reports timings on std::cout
struct MuteCout
{
    std::ostringstream sink;
    std::streambuf *old;
    MuteCout() : old(std::cout.rdbuf(sink.rdbuf())) {}
    ~MuteCout() { std::cout.rdbuf(old); }
};

template <typename Body>
int guarded(const Body &body)
{
    MuteCout mute;
    try
    {
        body();
        return 0;
    }
    catch (const std::exception &e)
    {
        theLastError = e.what();
        return -1;
    }
}

template <typename T>
void load(UT_VoxelArray<T> &grid, const T *data, int nx, int ny, int nz)
{
    grid.size(nx, ny, nz);
    if (data) std::memcpy(grid.rawData(), data, sizeof(T) * size_t(nx) * size_t(ny) * size_t(nz));
}
template <typename T>
void store(T *data, const UT_VoxelArray<T> &grid)
{
    std::memcpy(data, grid.rawData(), sizeof(T) * size_t(grid.numVoxels()));
}
void loadLabels(Labels &grid, const int32_t *data, int nx, int ny, int nz)
{
    static_assert(sizeof(int) == sizeof(int32_t), "labels are 4-byte ints");
    load(grid, reinterpret_cast<const int *>(data), nx, ny, nz);
}
// nullptr when the caller passes no weights (coarse levels)
Weights *loadWeights(Weights &w, const Real *wx, const Real *wy, const Real *wz, int nx, int ny, int nz)
{
    if (!wx) return nullptr;
    load(w[0], wx, nx + 1, ny, nz);
    load(w[1], wy, nx, ny + 1, nz);
    load(w[2], wz, nx, ny, nz + 1);
    return &w;
}
UT_Array<UT_Vector3I> loadCells(const int32_t *cells, int64_t n)
{
    UT_Array<UT_Vector3I> list;
    list.setSize(n);
    for (int64_t c = 0; c < n; ++c) list[c] = UT_Vector3I(cells[3 * c], cells[3 * c + 1], cells[3 * c + 2]);
    return list;
}

struct RefSolver
{
    Labels labels;
    Weights weights;
    std::unique_ptr<HDK::GeometricMultigridPoissonSolver> mg;
};
} // namespace

extern "C" {

const char *mgr_last_error(void) { return theLastError.c_str(); }
int mgr_real_bytes(void) { return int(sizeof(Real)); }
int mgr_cholesky_real_bytes(void) { return int(sizeof(REFSTANDIN_CHOLESKY_REAL)); }

/* ---- smoothers, operator, residual ------------------------------------------------------------------ */

int mgr_jacobi(Real *x, const Real *b, const int32_t *lab, const Real *wx, const Real *wy, const Real *wz, int nx, int ny, int nz,
               Real * /*scratch*/)
{
    return guarded([&] {
        Grid X, B;
        Labels L;
        Weights W;
        load(X, x, nx, ny, nz), load(B, b, nx, ny, nz), loadLabels(L, lab, nx, ny, nz);
        Ops::jacobiPoissonSmoother<Real>(X, B, L, loadWeights(W, wx, wy, wz, nx, ny, nz));
        store(x, X);
    });
}

int mgr_tiled_gs(Real *x, const Real *b, const int32_t *lab, const Real *wx, const Real *wy, const Real *wz, int nx, int ny, int nz,
                 int odd, int forward)
{
    return guarded([&] {
        Grid X, B;
        Labels L;
        Weights W;
        load(X, x, nx, ny, nz), load(B, b, nx, ny, nz), loadLabels(L, lab, nx, ny, nz);
        Ops::tiledGaussSeidelPoissonSmoother<Real>(X, B, L, odd != 0, forward != 0, loadWeights(W, wx, wy, wz, nx, ny, nz));
        store(x, X);
    });
}

int mgr_boundary_jacobi(Real *x, const Real *b, const int32_t *lab, const int32_t *cells, int64_t ncells, const Real *wx,
                        const Real *wy, const Real *wz, int nx, int ny, int nz)
{
    return guarded([&] {
        Grid X, B;
        Labels L;
        Weights W;
        load(X, x, nx, ny, nz), load(B, b, nx, ny, nz), loadLabels(L, lab, nx, ny, nz);
        Ops::boundaryJacobiPoissonSmoother<Real>(X, B, L, loadCells(cells, ncells), loadWeights(W, wx, wy, wz, nx, ny, nz));
        store(x, X);
    });
}

int mgr_apply_poisson(Real *y, const Real *x, const int32_t *lab, const Real *wx, const Real *wy, const Real *wz, int nx, int ny,
                      int nz)
{
    return guarded([&] {
        Grid Y, X;
        Labels L;
        Weights W;
        load(Y, y, nx, ny, nz), load(X, x, nx, ny, nz), loadLabels(L, lab, nx, ny, nz);
        Ops::applyPoissonMatrix<Real>(Y, X, L, loadWeights(W, wx, wy, wz, nx, ny, nz));
        store(y, Y);
    });
}

int mgr_residual(Real *r, const Real *x, const Real *b, const int32_t *lab, const Real *wx, const Real *wy, const Real *wz, int nx,
                 int ny, int nz)
{
    return guarded([&] {
        Grid R, X, B;
        Labels L;
        Weights W;
        load(R, r, nx, ny, nz), load(X, x, nx, ny, nz), load(B, b, nx, ny, nz), loadLabels(L, lab, nx, ny, nz);
        Ops::computePoissonResidual<Real>(R, X, B, L, loadWeights(W, wx, wy, wz, nx, ny, nz));
        store(r, R);
    });
}

/* ---- transfer ------------------------------------------------------------------------------------------ */

int mgr_downsample(Real *coarse, const Real *fine, const int32_t *coarse_lab, int cnx, int cny, int cnz, const int32_t *fine_lab)
{
    return guarded([&] {
        Grid C, F;
        Labels CL, FL;
        load(C, coarse, cnx, cny, cnz), load(F, fine, 2 * cnx, 2 * cny, 2 * cnz);
        loadLabels(CL, coarse_lab, cnx, cny, cnz), loadLabels(FL, fine_lab, 2 * cnx, 2 * cny, 2 * cnz);
        Ops::downsample<Real>(C, F, CL, FL);
        store(coarse, C);
    });
}

int mgr_upsample_add(Real *fine, const Real *coarse, const int32_t *fine_lab, int fnx, int fny, int fnz, const int32_t *coarse_lab)
{
    return guarded([&] {
        Grid F, C;
        Labels FL, CL;
        load(F, fine, fnx, fny, fnz), load(C, coarse, fnx / 2, fny / 2, fnz / 2);
        loadLabels(FL, fine_lab, fnx, fny, fnz), loadLabels(CL, coarse_lab, fnx / 2, fny / 2, fnz / 2);
        Ops::upsampleAndAdd<Real>(F, C, FL, CL);
        store(fine, F);
    });
}

/* ---- vector operations (per cell, so a flat n x 1 x 1 grid serves) and reductions ----------------------- */

int mgr_add_vectors(Real *dst, const Real *a, const Real *bs, Real s, const int32_t *lab, int64_t n)
{
    return guarded([&] {
        Grid D, A, B;
        Labels L;
        load(D, dst, int(n), 1, 1), load(A, a, int(n), 1, 1), load(B, bs, int(n), 1, 1), loadLabels(L, lab, int(n), 1, 1);
        Ops::addVectors<Real>(D, A, B, s, L);
        store(dst, D);
    });
}

int mgr_add_to_vector(Real *dst, const Real *a, Real s, const int32_t *lab, int64_t n)
{
    return guarded([&] {
        Grid D, A;
        Labels L;
        load(D, dst, int(n), 1, 1), load(A, a, int(n), 1, 1), loadLabels(L, lab, int(n), 1, 1);
        Ops::addToVector<Real>(D, A, s, L);
        store(dst, D);
    });
}

int mgr_scale_vector(Real *v, Real s, const int32_t *lab, int64_t n)
{
    return guarded([&] {
        Grid V;
        Labels L;
        load(V, v, int(n), 1, 1), loadLabels(L, lab, int(n), 1, 1);
        Ops::scaleVector<Real>(V, s, L);
        store(v, V);
    });
}

double mgr_dot(const Real *a, const Real *b, const int32_t *lab, int nx, int ny, int nz)
{
    double out = std::numeric_limits<double>::quiet_NaN();
    guarded([&] {
        Grid A, B;
        Labels L;
        load(A, a, nx, ny, nz), load(B, b, nx, ny, nz), loadLabels(L, lab, nx, ny, nz);
        out = Ops::dotProduct<Real>(A, B, L);
    });
    return out;
}

double mgr_squared_l2(const Real *a, const int32_t *lab, int nx, int ny, int nz)
{
    double out = std::numeric_limits<double>::quiet_NaN();
    guarded([&] {
        Grid A;
        Labels L;
        load(A, a, nx, ny, nz), loadLabels(L, lab, nx, ny, nz);
        out = Ops::squaredL2Norm<Real>(A, L);
    });
    return out;
}

double mgr_l2(const Real *a, const int32_t *lab, int nx, int ny, int nz)
{
    double out = std::numeric_limits<double>::quiet_NaN();
    guarded([&] {
        Grid A;
        Labels L;
        load(A, a, nx, ny, nz), loadLabels(L, lab, nx, ny, nz);
        out = Ops::l2Norm<Real>(A, L);
    });
    return out;
}

double mgr_inf_norm(const Real *a, const int32_t *lab, int nx, int ny, int nz)
{
    double out = std::numeric_limits<double>::quiet_NaN();
    guarded([&] {
        Grid A;
        Labels L;
        load(A, a, nx, ny, nz), loadLabels(L, lab, nx, ny, nz);
        out = Ops::infNorm(A, L);
    });
    return out;
}

/* ---- domain / hierarchy construction -------------------------------------------------------------------- */

/* buildExpandedCellLabels: the reference sizes the grid itself.  Base labels use the solver's codes
 * (0 interior, 1 exterior, anything else Dirichlet), as mgo_build_expanded_labels reads them.  exp_lab may be
 * null (layout only); when given it must hold out_dims cells, which the caller learns from a first call. */
int mgr_build_expanded_labels_sized(int32_t *exp_lab, const int32_t *base_lab, int bnx, int bny, int bnz, int *out_dims,
                                    int *out_offset, int *out_levels)
{
    return guarded([&] {
        Labels base, expanded;
        loadLabels(base, base_lab, bnx, bny, bnz);
        if (!base_lab) base.constant(Ops::EXTERIOR_CELL);
        auto isExterior = [](int l) { return l == Ops::EXTERIOR_CELL; };
        auto isInterior = [](int l) { return l == Ops::INTERIOR_CELL; };
        auto isDirichlet = [](int l) { return l != Ops::EXTERIOR_CELL && l != Ops::INTERIOR_CELL; };
        std::pair<UT_Vector3I, int> r = Ops::buildExpandedCellLabels(expanded, base, isExterior, isInterior, isDirichlet);
        for (int a = 0; a < 3; ++a)
        {
            out_dims[a] = int(expanded.getVoxelRes()[a]);
            out_offset[a] = int(r.first[a]);
        }
        *out_levels = r.second;
        if (exp_lab) store(reinterpret_cast<int *>(exp_lab), expanded);
    });
}

void mgr_expanded_layout(int bnx, int bny, int bnz, int *out_dims, int *out_offset, int *out_levels)
{
    if (mgr_build_expanded_labels_sized(nullptr, nullptr, bnx, bny, bnz, out_dims, out_offset, out_levels) != 0)
        out_dims[0] = out_dims[1] = out_dims[2] = *out_levels = -1;
}

int mgr_build_expanded_labels(int32_t *exp_lab, const int32_t *base_lab, int bnx, int bny, int bnz, int enx, int eny, int enz, int off)
{
    int dims[3], offset[3], levels;
    if (mgr_build_expanded_labels_sized(nullptr, base_lab, bnx, bny, bnz, dims, offset, &levels) != 0) return -1;
    if (dims[0] != enx || dims[1] != eny || dims[2] != enz || offset[0] != off || offset[1] != off || offset[2] != off)
    {
        theLastError = "the reference sizes the expanded grid differently";
        return -1;
    }
    return mgr_build_expanded_labels_sized(exp_lab, base_lab, bnx, bny, bnz, dims, offset, &levels);
}

int mgr_build_expanded_weights(Real *exp_w, const Real *base_w, int axis, int bnx, int bny, int bnz, int enx, int eny, int enz, int off,
                               const int32_t *exp_lab)
{
    return guarded([&] {
        const int b[3] = {bnx + (axis == 0), bny + (axis == 1), bnz + (axis == 2)};
        const int e[3] = {enx + (axis == 0), eny + (axis == 1), enz + (axis == 2)};
        Grid base, expanded;
        Labels L;
        load(base, base_w, b[0], b[1], b[2]);
        expanded.size(e[0], e[1], e[2]);
        loadLabels(L, exp_lab, enx, eny, enz);
        Ops::buildExpandedBoundaryWeights(expanded, base, L, UT_Vector3I(off), axis);
        store(exp_w, expanded);
    });
}

int mgr_set_boundary_labels(int32_t *lab, const Real *wx, const Real *wy, const Real *wz, int nx, int ny, int nz)
{
    return guarded([&] {
        Labels L;
        Weights W;
        loadLabels(L, lab, nx, ny, nz);
        Ops::setBoundaryCellLabels(L, *loadWeights(W, wx, wy, wz, nx, ny, nz));
        store(reinterpret_cast<int *>(lab), L);
    });
}

int mgr_build_coarse_labels(int32_t *coarse, const int32_t *fine, int fnx, int fny, int fnz)
{
    return guarded([&] {
        Labels F;
        loadLabels(F, fine, fnx, fny, fnz);
        Labels C = Ops::buildCoarseCellLabels(F);
        store(reinterpret_cast<int *>(coarse), C);
    });
}

/* the list is malloc'ed into *out (n x 3 int32, x y z); free with mgr_free.  Returns n, or -1. */
int64_t mgr_build_boundary_cells(const int32_t *lab, int nx, int ny, int nz, int width, int32_t **out)
{
    int64_t n = -1;
    guarded([&] {
        Labels L;
        loadLabels(L, lab, nx, ny, nz);
        UT_Array<UT_Vector3I> cells = Ops::buildBoundaryCells(L, width);
        int32_t *list = static_cast<int32_t *>(std::malloc(sizeof(int32_t) * 3 * size_t(cells.size() > 0 ? cells.size() : 1)));
        for (exint c = 0; c < cells.size(); ++c)
            for (int a = 0; a < 3; ++a) list[3 * c + a] = int32_t(cells[c][a]);
        *out = list;
        n = cells.size();
    });
    return n;
}

void mgr_free(void *p) { std::free(p); }

/* structural checkers: 1 pass, 0 fail, -1 error */
int mgr_unit_test_exterior(const int32_t *lab, int nx, int ny, int nz)
{
    int pass = -1;
    guarded([&] {
        Labels L;
        loadLabels(L, lab, nx, ny, nz);
        pass = Ops::unitTestExteriorCells(L) ? 1 : 0;
    });
    return pass;
}

int mgr_unit_test_boundary(const int32_t *lab, const Real *wx, const Real *wy, const Real *wz, int nx, int ny, int nz)
{
    int pass = -1;
    guarded([&] {
        Labels L;
        Weights W;
        loadLabels(L, lab, nx, ny, nz);
        pass = Ops::unitTestBoundaryCells<Real>(L, loadWeights(W, wx, wy, wz, nx, ny, nz)) ? 1 : 0;
    });
    return pass;
}

int mgr_unit_test_coarsening(const int32_t *coarse, const int32_t *fine, int fnx, int fny, int fnz)
{
    int pass = -1;
    guarded([&] {
        Labels C, F;
        loadLabels(C, coarse, fnx / 2, fny / 2, fnz / 2), loadLabels(F, fine, fnx, fny, fnz);
        pass = Ops::unitTestCoarsening(C, F) ? 1 : 0;
    });
    return pass;
}

/* ---- GeometricMultigridPoissonSolver -------------------------------------------------------------------- */

void *mgr_solver_create(const int32_t *labels, const Real *wx, const Real *wy, const Real *wz, int nx, int ny, int nz, int mg_levels,
                        int use_gs)
{
    RefSolver *s = new RefSolver;
    int rc = guarded([&] {
        loadLabels(s->labels, labels, nx, ny, nz);
        loadWeights(s->weights, wx, wy, wz, nx, ny, nz);
        s->mg.reset(new HDK::GeometricMultigridPoissonSolver(s->labels, s->weights, mg_levels, use_gs != 0));
    });
    if (rc != 0)
    {
        delete s;
        return nullptr;
    }
    return s;
}

void mgr_solver_destroy(void *h) { delete static_cast<RefSolver *>(h); }

int mgr_solver_levels(void *h) { return static_cast<RefSolver *>(h)->mg->getMGLevels(); }

int mgr_solver_apply_vcycle(void *h, Real *x, const Real *b, int use_initial_guess)
{
    RefSolver *s = static_cast<RefSolver *>(h);
    return guarded([&] {
        const UT_Vector3I res = s->labels.getVoxelRes();
        Grid X, B;
        load(X, x, int(res[0]), int(res[1]), int(res[2])), load(B, b, int(res[0]), int(res[1]), int(res[2]));
        s->mg->applyVCycle(X, B, use_initial_guess != 0);
        store(x, X);
    });
}

/* solveGeometricConjugateGradient with the reference's operators as functors, wired as the plugin wires them:
 * A = applyPoissonMatrix with the fine weights; M^-1 = the handle's V-cycle (precond 1) or the diagonal (precond 0:
 * 1/6 on interior cells, 1 / (sum of the six face weights) on boundary cells).  stats[0] = iterations, stats[1] =
 * drifted, stats[2] = recomputed relative L2 error; rel_history[i] = relative residual after iteration i.  Returns
 * 0 ok, 1 rhs zero, 2 already converged, -1 error.  The function reports only on std::cout, so iterations and residuals are
 * read off the squared-norm functor: call 0 is the rhs, call 1 the initial residual, then one per iteration, and
 * a last one for the recomputed residual. */
int mgr_solve_pcg(void *h, Real *x, const Real *b, double tol, int max_iter, int precond, double *stats, double *rel_history)
{
    RefSolver *s = static_cast<RefSolver *>(h);
    int ret = 0;
    stats[0] = stats[1] = stats[2] = 0;
    int rc = guarded([&] {
        const UT_Vector3I res = s->labels.getVoxelRes();
        const Labels &L = s->labels;
        const Weights &W = s->weights;
        Grid X, B;
        load(X, x, int(res[0]), int(res[1]), int(res[2])), load(B, b, int(res[0]), int(res[1]), int(res[2]));

        std::vector<double> norms;
        auto multiply = [&](Grid &dst, const Grid &src) { Ops::applyPoissonMatrix<Real>(dst, src, L, &W); };
        auto dot = [&](const Grid &g0, const Grid &g1) { return Ops::dotProduct<Real>(g0, g1, L); };
        auto squaredNorm = [&](const Grid &g) {
            norms.push_back(Ops::squaredL2Norm<Real>(g, L));
            return norms.back();
        };
        auto addTo = [&](Grid &dst, const Grid &src, const Real scale) { Ops::addToVector<Real>(dst, src, scale, L); };
        auto addScaled = [&](Grid &dst, const Grid &unscaled, const Grid &scaled, const Real scale) {
            Ops::addVectors<Real>(dst, unscaled, scaled, scale, L);
        };

        if (precond)
        {
            auto vcycle = [&](Grid &dst, const Grid &src) { s->mg->applyVCycle(dst, src); };
            HDK::solveGeometricConjugateGradient(X, B, multiply, vcycle, dot, squaredNorm, addTo, addScaled, Real(tol), max_iter);
        }
        else
        {
            Grid dinv;
            dinv.size(int(res[0]), int(res[1]), int(res[2]));
            UT_Vector3I cell;
            for (cell[2] = 0; cell[2] < res[2]; ++cell[2])
                for (cell[1] = 0; cell[1] < res[1]; ++cell[1])
                    for (cell[0] = 0; cell[0] < res[0]; ++cell[0])
                    {
                        if (L(cell) == Ops::INTERIOR_CELL)
                            dinv.setValue(cell, 1. / 6.);
                        else if (L(cell) == Ops::BOUNDARY_CELL)
                        {
                            Real diagonal = 0;
                            for (int axis : {0, 1, 2})
                                for (int direction : {0, 1}) diagonal += W[axis](SIM::FieldUtils::cellToFaceMap(cell, axis, direction));
                            dinv.setValue(cell, 1. / diagonal);
                        }
                    }
            auto diagonalPrecond = [&](Grid &dst, const Grid &src) {
                const exint n = src.numVoxels();
                for (exint c = 0; c < n; ++c)
                    if (L.rawData()[c] == Ops::INTERIOR_CELL || L.rawData()[c] == Ops::BOUNDARY_CELL)
                        dst.rawData()[c] = src.rawData()[c] * dinv.rawData()[c];
            };
            HDK::solveGeometricConjugateGradient(X, B, multiply, diagonalPrecond, dot, squaredNorm, addTo, addScaled, Real(tol), max_iter);
        }
        store(x, X);

        const double rhs2 = norms[0];
        if (norms.size() == 1)
        {
            ret = 1;
            return;
        }
        if (norms.size() == 2)
        {
            ret = 2;
            stats[1] = std::sqrt(norms[1] / rhs2);
            return;
        }
        const int evaluated = int(norms.size()) - 3; // per-iteration norms
        for (int i = 0; i < evaluated; ++i)
            if (rel_history) rel_history[i] = std::sqrt(norms[size_t(2 + i)] / rhs2);
        const double last = evaluated > 0 ? norms[size_t(1 + evaluated)] : norms[1];
        const double threshold = tol * tol * rhs2;
        const bool broke = evaluated > 0 && last < threshold;
        stats[0] = broke ? evaluated - 1 : evaluated;
        stats[1] = std::sqrt(last / rhs2);
        stats[2] = std::sqrt(norms.back() / rhs2);
    });
    return rc != 0 ? -1 : ret;
}

} // extern "C"
