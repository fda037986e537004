/*
 * ref_fields_driver.cpp -- extern "C" entries over flat arrays that call the reference's own plugin code
 * (rgoldade/GeometricMultigridPressureSolver, Source/HDK_GeometricFreeSurfacePressureSolver.{h,cpp} and
 * HDK_Utilities.{h,cpp}), compiled unchanged together with its solver core against the stand-in headers of
 * oracle/ref_standin/ into oracle/_ref/libmgref_fields.so (`make -C oracle ref`).  TEST INFRASTRUCTURE ONLY.
 *
 * This file names the reference's headers in #include lines and holds none of their text.  It is compiled with
 * -fno-access-control: the per-pass members of the plugin class are private, and its header stays untouched.
 *
 * One entry per reference function (prefix mgrf_), shaped like the mgf_* entries of mg_fields_oracle.c, and one
 * that runs the whole solveGasSubclass on a stand-in SIM_Object holding the named fields.  Conventions:
 *   - grids are dense, x fastest; the face grid of axis a has one more entry along a.  Whatever the reference
 *     keeps in a SIM_RawField comes in and goes out as float (fields store fpreal32), material labels as int32
 *     (0 SOLID, 1 LIQUID, 2 AIR), multigrid labels as int32, multigrid weights / rhs / solution as double
 *     (the plugin's SolveReal = StoreReal = double);
 *   - every field is built at origin 0 with the voxel size of mgrf_set_voxel_size (a power of two, default
 *     1/32), so sample positions are exact in fpreal32;
 *   - the solid SDF is a centre-sampled field aligned with the liquid SDF, the solid velocity a face-sampled
 *     field aligned with the velocity: the positions the reference interpolates them at are their own samples,
 *     and the stand-in's interpolant returns those bit for bit.  That is the one convention in which the
 *     project's API differs from the plugin's (pre-sampled solid inputs, include/mgps_fields.h);
 *   - every entry returns 0, or -1 after a reference assertion (armed in this build) or a stand-in bounds
 *     check failed, or after the plugin refused its inputs: mgrf_last_error() has the text.
 */
#include <cstring>
#include <sstream>
#include <string>

#include "HDK_GeometricFreeSurfacePressureSolver.h"
#include "HDK_GeometricMultigridOperators.h"

void initializeSIM(void *); // the plugin's registration hook (the HDK declares it for every DSO)

namespace
{
namespace Ops = HDK::GeometricMultigridOperators;
using Plugin = HDK_GeometricFreeSurfacePressureSolver;
using Real = double;
using Grid = UT_VoxelArray<Real>;
using Labels = UT_VoxelArray<int>;

std::string theLastError;
std::string theLastOutput;
float theVoxelSize = 0.03125f;

struct Dims
{
    int g[3];
    Dims(int gx, int gy, int gz) : g{gx, gy, gz} {}
    UT_Vector3 orig() const { return UT_Vector3(0, 0, 0); }
    UT_Vector3 size() const { return UT_Vector3(float(g[0]) * theVoxelSize, float(g[1]) * theVoxelSize, float(g[2]) * theVoxelSize); }
    size_t cells() const { return size_t(g[0]) * size_t(g[1]) * size_t(g[2]); }
    size_t faces(int axis) const { return cells() / size_t(g[axis]) * size_t(g[axis] + 1); }
};

const SIM_FieldSample theFaceSample[3] = {SIM_SAMPLE_FACEX, SIM_SAMPLE_FACEY, SIM_SAMPLE_FACEZ};

// the reference reports on std::cout; the text is kept for the entries that read numbers off it
template <typename Body>
int guarded(const Body &body)
{
    std::ostringstream sink;
    std::streambuf *old = std::cout.rdbuf(sink.rdbuf());
    const std::streamsize precision = std::cout.precision(17);
    int rc = 0;
    try
    {
        body();
    }
    catch (const std::exception &e)
    {
        theLastError = e.what();
        rc = -1;
    }
    std::cout.precision(precision);
    std::cout.rdbuf(old);
    theLastOutput = sink.str();
    return rc;
}

void fill(SIM_RawField &field, const float *data)
{
    if (data) std::memcpy(field.fieldNC()->rawData(), data, sizeof(float) * size_t(field.field()->numVoxels()));
}
void read(float *data, const SIM_RawField &field) { std::memcpy(data, field.field()->rawData(), sizeof(float) * size_t(field.field()->numVoxels())); }

void makeCentre(SIM_RawField &field, const Dims &d, const float *data)
{
    field.init(SIM_SAMPLE_CENTER, d.orig(), d.size(), d.g[0], d.g[1], d.g[2]);
    fill(field, data);
}
void makeFace(SIM_RawField &field, const Dims &d, int axis, const float *data)
{
    field.init(theFaceSample[axis], d.orig(), d.size(), d.g[0], d.g[1], d.g[2]);
    fill(field, data);
}
void makeVector(SIM_VectorField &field, const Dims &d, const float *const data[3])
{
    field.initStandin(true, d.orig(), d.size(), d.g[0], d.g[1], d.g[2]);
    for (int a = 0; a < 3; ++a) fill(*field.getField(a), data ? data[a] : nullptr);
}
void makeMaterial(SIM_RawIndexField &field, const Dims &d, const int32_t *data)
{
    field.init(SIM_SAMPLE_CENTER, d.orig(), d.size(), d.g[0], d.g[1], d.g[2]);
    int64 *dst = field.fieldNC()->rawData();
    for (size_t c = 0; c < d.cells(); ++c) dst[c] = data[c];
}
void loadLabels(Labels &grid, const int32_t *data, int nx, int ny, int nz)
{
    static_assert(sizeof(int) == sizeof(int32_t), "labels are 4-byte ints");
    grid.size(nx, ny, nz);
    std::memcpy(grid.rawData(), data, sizeof(int) * size_t(grid.numVoxels()));
}
void loadGrid(Grid &grid, const Real *data, int nx, int ny, int nz)
{
    grid.size(nx, ny, nz);
    if (data) std::memcpy(grid.rawData(), data, sizeof(Real) * size_t(grid.numVoxels()));
}
template <typename T>
void store(T *data, const UT_VoxelArray<T> &grid)
{
    std::memcpy(data, grid.rawData(), sizeof(T) * size_t(grid.numVoxels()));
}

struct CutWeights
{
    SIM_RawField fields[3];
    std::array<const SIM_RawField *, 3> pointers;
    CutWeights(const Dims &d, const float *wx, const float *wy, const float *wz)
    {
        const float *w[3] = {wx, wy, wz};
        for (int a = 0; a < 3; ++a)
        {
            makeFace(fields[a], d, a, w[a]);
            pointers[a] = &fields[a];
        }
    }
};

// the first number after `label` in the captured report, NaN where the label is missing
double numberAfter(const std::string &text, const std::string &label)
{
    const size_t at = text.rfind(label);
    if (at == std::string::npos) return std::nan("");
    return std::strtod(text.c_str() + at + label.size(), nullptr);
}
} // namespace

extern "C" {

const char *mgrf_last_error(void) { return theLastError.c_str(); }
const char *mgrf_last_output(void) { return theLastOutput.c_str(); }
void mgrf_set_voxel_size(float h) { theVoxelSize = h; }
int mgrf_field_real_bytes(void) { return int(sizeof(fpreal32)); }
int mgrf_cholesky_real_bytes(void) { return int(sizeof(REFSTANDIN_CHOLESKY_REAL)); }

/* initializeSIM: builds the plugin's parameter table once; returns the number of its parameters, or -1 */
int mgrf_parameter_count(void)
{
    int n = -1;
    guarded([&] {
        initializeSIM(nullptr);
        const PRM_Template *t = Plugin::dataFactoryDescriptionStandin()->getTemplates();
        for (n = 0; t[n].getType() != PRM_LIST_TERMINATOR; ++n) {}
    });
    return n;
}

/* HDK::Utilities::buildMaterialCellLabels */
int mgrf_material_labels(int32_t *material, const float *liquid_phi, const float *solid_phi, const float *cwx, const float *cwy,
                         const float *cwz, int gx, int gy, int gz)
{
    return guarded([&] {
        const Dims d(gx, gy, gz);
        SIM_RawField liquid, solid;
        makeCentre(liquid, d, liquid_phi), makeCentre(solid, d, solid_phi);
        CutWeights cw(d, cwx, cwy, cwz);
        SIM_RawIndexField labels;
        HDK::Utilities::buildMaterialCellLabels(labels, liquid, solid, cw.pointers);
        for (size_t c = 0; c < d.cells(); ++c) material[c] = int32_t(labels.field()->rawData()[c]);
    });
}

/* buildValidFaces: the three face grids as the reference stores them (fpreal32, 1 valid, 0 not) */
int mgrf_valid_faces(float *valid_x, float *valid_y, float *valid_z, const int32_t *material, const float *cwx, const float *cwy,
                     const float *cwz, int gx, int gy, int gz)
{
    return guarded([&] {
        const Dims d(gx, gy, gz);
        SIM_RawIndexField labels;
        makeMaterial(labels, d, material);
        CutWeights cw(d, cwx, cwy, cwz);
        SIM_VectorField valid;
        makeVector(valid, d, nullptr);
        Plugin plugin(nullptr);
        plugin.buildValidFaces(valid, labels, cw.pointers);
        float *out[3] = {valid_x, valid_y, valid_z};
        for (int a = 0; a < 3; ++a) read(out[a], *valid.getField(a));
    });
}

/* buildMGDomainLabels on the base grid, which the caller of the reference fills with EXTERIOR first */
int mgrf_domain_labels(int32_t *base_labels, const int32_t *material, int gx, int gy, int gz)
{
    return guarded([&] {
        const Dims d(gx, gy, gz);
        SIM_RawIndexField labels;
        makeMaterial(labels, d, material);
        Labels base;
        base.size(gx, gy, gz);
        base.constant(Ops::EXTERIOR_CELL);
        Plugin plugin(nullptr);
        plugin.buildMGDomainLabels(base, labels);
        store(reinterpret_cast<int *>(base_labels), base);
    });
}

/* buildMGBoundaryWeights of one axis on the base face grid, which the caller of the reference zeroes first */
int mgrf_boundary_weights(int axis, Real *base_w, const float *cw, const float *liquid_phi, const float *valid, const int32_t *material,
                          const int32_t *base_labels, int gx, int gy, int gz)
{
    return guarded([&] {
        const Dims d(gx, gy, gz);
        SIM_RawField weights, liquid, validFaces;
        makeFace(weights, d, axis, cw), makeCentre(liquid, d, liquid_phi), makeFace(validFaces, d, axis, valid);
        SIM_RawIndexField labels;
        makeMaterial(labels, d, material);
        Labels base;
        loadLabels(base, base_labels, gx, gy, gz);
        Grid out;
        out.size(gx + (axis == 0), gy + (axis == 1), gz + (axis == 2));
        out.constant(0);
        Plugin plugin(nullptr);
        plugin.buildMGBoundaryWeights(out, weights, liquid, validFaces, labels, base, axis);
        store(base_w, out);
    });
}

/* the sizes buildExpandedCellLabels chooses for a base grid */
int mgrf_expanded_layout(int gx, int gy, int gz, int *out_dims, int *out_offset, int *out_levels)
{
    return guarded([&] {
        Labels base, expanded;
        base.size(gx, gy, gz);
        base.constant(Ops::EXTERIOR_CELL);
        auto isExterior = [](const int v) { return v == Ops::EXTERIOR_CELL; };
        auto isInterior = [](const int v) { return v == Ops::INTERIOR_CELL; };
        auto isDirichlet = [](const int v) { return v == Ops::DIRICHLET_CELL; };
        std::pair<UT_Vector3I, int> r = Ops::buildExpandedCellLabels(expanded, base, isExterior, isInterior, isDirichlet);
        for (int a = 0; a < 3; ++a)
        {
            out_dims[a] = int(expanded.getVoxelRes()[a]);
            out_offset[a] = int(r.first[a]);
        }
        *out_levels = r.second;
    });
}

/* buildExpandedCellLabels, buildExpandedBoundaryWeights x3, setBoundaryCellLabels and the two structural
 * assertions, chained and parametrised as solveGasSubclass chains them.  The outputs hold the sizes of
 * mgrf_expanded_layout. */
int mgrf_expand(int32_t *exp_labels, Real *exp_wx, Real *exp_wy, Real *exp_wz, const int32_t *base_labels, const Real *base_wx,
                const Real *base_wy, const Real *base_wz, int gx, int gy, int gz)
{
    return guarded([&] {
        Labels base, expanded;
        loadLabels(base, base_labels, gx, gy, gz);
        const Real *bw[3] = {base_wx, base_wy, base_wz};
        Real *ew[3] = {exp_wx, exp_wy, exp_wz};
        auto isExterior = [](const int v) { return v == Ops::EXTERIOR_CELL; };
        auto isInterior = [](const int v) { return v == Ops::INTERIOR_CELL; };
        auto isDirichlet = [](const int v) { return v == Ops::DIRICHLET_CELL; };
        std::pair<UT_Vector3I, int> settings = Ops::buildExpandedCellLabels(expanded, base, isExterior, isInterior, isDirichlet);
        std::array<Grid, 3> weights;
        for (int axis : {0, 1, 2})
        {
            Grid baseWeights;
            loadGrid(baseWeights, bw[axis], gx + (axis == 0), gy + (axis == 1), gz + (axis == 2));
            UT_Vector3I size = expanded.getVoxelRes();
            ++size[axis];
            weights[axis].size(int(size[0]), int(size[1]), int(size[2]));
            weights[axis].constant(0);
            Ops::buildExpandedBoundaryWeights(weights[axis], baseWeights, expanded, settings.first, axis);
        }
        Ops::setBoundaryCellLabels(expanded, weights);
        assert(Ops::unitTestBoundaryCells<Real>(expanded, &weights));
        assert(Ops::unitTestExteriorCells(expanded));
        store(reinterpret_cast<int *>(exp_labels), expanded);
        for (int axis : {0, 1, 2}) store(ew[axis], weights[axis]);
    });
}

/* buildRHS into an expanded grid that the caller of the reference zeroes first; solid velocities may be null */
int mgrf_rhs(Real *exp_rhs, const int32_t *material, const float *vx, const float *vy, const float *vz, const float *svx, const float *svy,
             const float *svz, const float *cwx, const float *cwy, const float *cwz, const int32_t *exp_labels, int gx, int gy, int gz, int ex,
             int ey, int ez, int offset)
{
    return guarded([&] {
        const Dims d(gx, gy, gz);
        SIM_RawIndexField labels;
        makeMaterial(labels, d, material);
        const float *v[3] = {vx, vy, vz}, *sv[3] = {svx, svy, svz};
        SIM_VectorField velocity, solidVelocity;
        makeVector(velocity, d, v);
        if (svx) makeVector(solidVelocity, d, sv);
        CutWeights cw(d, cwx, cwy, cwz);
        Labels expanded;
        loadLabels(expanded, exp_labels, ex, ey, ez);
        Grid rhs;
        rhs.size(ex, ey, ez);
        rhs.constant(0);
        Plugin plugin(nullptr);
        plugin.buildRHS(rhs, labels, velocity, svx ? &solidVelocity : nullptr, cw.pointers, expanded, UT_Vector3I(offset));
        store(exp_rhs, rhs);
    });
}

/* applyOldPressure into an expanded grid that the caller of the reference zeroes first */
int mgrf_apply_old_pressure(Real *exp_x, const float *pressure, const int32_t *material, const int32_t *exp_labels, int gx, int gy, int gz,
                            int ex, int ey, int ez, int offset)
{
    return guarded([&] {
        const Dims d(gx, gy, gz);
        SIM_RawIndexField labels;
        makeMaterial(labels, d, material);
        SIM_RawField p;
        makeCentre(p, d, pressure);
        Labels expanded;
        loadLabels(expanded, exp_labels, ex, ey, ez);
        Grid x;
        x.size(ex, ey, ez);
        x.constant(0);
        Plugin plugin(nullptr);
        plugin.applyOldPressure(x, p, labels, expanded, UT_Vector3I(offset));
        store(exp_x, x);
    });
}

/* applySolutionToPressure, in place on `pressure` (the caller of the reference clears it first; this entry does not) */
int mgrf_solution_to_pressure(float *pressure, const Real *exp_x, const int32_t *material, const int32_t *exp_labels, int gx, int gy, int gz,
                              int ex, int ey, int ez, int offset)
{
    return guarded([&] {
        const Dims d(gx, gy, gz);
        SIM_RawIndexField labels;
        makeMaterial(labels, d, material);
        SIM_RawField p;
        makeCentre(p, d, pressure);
        Labels expanded;
        loadLabels(expanded, exp_labels, ex, ey, ez);
        Grid x;
        loadGrid(x, exp_x, ex, ey, ez);
        Plugin plugin(nullptr);
        plugin.applySolutionToPressure(p, labels, expanded, x, UT_Vector3I(offset));
        read(pressure, p);
    });
}

/* applyPressureGradient of one axis, in place on `velocity` */
int mgrf_pressure_gradient(int axis, float *velocity, const float *cw, const float *liquid_phi, const float *pressure, const float *valid,
                           const int32_t *material, int gx, int gy, int gz)
{
    return guarded([&] {
        const Dims d(gx, gy, gz);
        SIM_RawField v, weights, liquid, p, validFaces;
        makeFace(v, d, axis, velocity), makeFace(weights, d, axis, cw), makeCentre(liquid, d, liquid_phi), makeCentre(p, d, pressure);
        makeFace(validFaces, d, axis, valid);
        SIM_RawIndexField labels;
        makeMaterial(labels, d, material);
        Plugin plugin(nullptr);
        plugin.applyPressureGradient(v, weights, liquid, p, validFaces, labels, axis);
        read(velocity, v);
    });
}

/* computeResultingDivergence and its caller's reduction over the per-thread slots (one thread here):
 * out3 = {accumulated divergence, maximum divergence (from 0), liquid cell count} */
int mgrf_divergence(Real *out3, const int32_t *material, const float *vx, const float *vy, const float *vz, const float *svx, const float *svy,
                    const float *svz, const float *cwx, const float *cwy, const float *cwz, int gx, int gy, int gz)
{
    return guarded([&] {
        const Dims d(gx, gy, gz);
        SIM_RawIndexField labels;
        makeMaterial(labels, d, material);
        const float *v[3] = {vx, vy, vz}, *sv[3] = {svx, svy, svz};
        SIM_VectorField velocity, solidVelocity;
        makeVector(velocity, d, v);
        if (svx) makeVector(solidVelocity, d, sv);
        CutWeights cw(d, cwx, cwy, cwz);
        const int threadCount = UT_Thread::getNumProcessors();
        UT_Array<Real> sums, maxima, counts;
        for (UT_Array<Real> *list : {&sums, &maxima, &counts})
        {
            list->setSize(threadCount);
            list->constant(0);
        }
        Plugin plugin(nullptr);
        plugin.computeResultingDivergence(sums, counts, maxima, labels, velocity, svx ? &solidVelocity : nullptr, cw.pointers);
        Real sum = 0, maximum = 0, count = 0;
        for (int thread = 0; thread < threadCount; ++thread)
        {
            sum += sums[thread];
            maximum = std::max(maximum, maxima[thread]);
            count += counts[thread];
        }
        out3[0] = sum, out3[1] = maximum, out3[2] = count;
    });
}

/* The whole solveGasSubclass on a stand-in SIM_Object that holds "surface", "velocity", "cutCellWeights",
 * "validFaces", "pressure", a constant "density" and, where given, "collision" and "collisionvelocity".
 * velocity and pressure are updated in place, valid_* written.  stats[0] = CG iterations, stats[1] = drifted,
 * stats[2] = recomputed relative L2 error, stats[3 .. 5] = maximum, accumulated and average divergence: all
 * read off the plugin's own report (printed with 17 digits); NaN where the report has no such line (rhs zero,
 * or a warm start that already satisfies the tolerance). */
int mgrf_solve(const float *liquid_phi, const float *solid_phi, const float *cwx, const float *cwy, const float *cwz, float *vx, float *vy,
               float *vz, const float *svx, const float *svy, const float *svz, float *pressure, float *valid_x, float *valid_y,
               float *valid_z, int gx, int gy, int gz, double tolerance, int max_iterations, int use_mg, int use_old_pressure, double *stats)
{
    const int rc = guarded([&] {
        const Dims d(gx, gy, gz);
        SIM_Object object;
        SIM_ScalarField &surface = object.addScalarFieldStandin(GAS_NAME_SURFACE);
        surface.initStandin(SIM_SAMPLE_CENTER, d.orig(), d.size(), gx, gy, gz);
        fill(*surface.getField(), liquid_phi);
        SIM_ScalarField &p = object.addScalarFieldStandin(GAS_NAME_PRESSURE);
        p.initStandin(SIM_SAMPLE_CENTER, d.orig(), d.size(), gx, gy, gz);
        fill(*p.getField(), pressure);
        SIM_ScalarField &density = object.addScalarFieldStandin(GAS_NAME_DENSITY);
        density.initStandin(SIM_SAMPLE_CENTER, d.orig(), d.size(), gx, gy, gz);
        density.getField()->makeConstant(1000);
        if (solid_phi)
        {
            SIM_ScalarField &solid = object.addScalarFieldStandin(GAS_NAME_COLLISION);
            solid.initStandin(SIM_SAMPLE_CENTER, d.orig(), d.size(), gx, gy, gz);
            fill(*solid.getField(), solid_phi);
        }
        float *v[3] = {vx, vy, vz}, *valid[3] = {valid_x, valid_y, valid_z};
        const float *cv[3] = {vx, vy, vz}, *cw[3] = {cwx, cwy, cwz}, *sv[3] = {svx, svy, svz};
        SIM_VectorField &velocity = object.addVectorFieldStandin(GAS_NAME_VELOCITY);
        makeVector(velocity, d, cv);
        makeVector(object.addVectorFieldStandin("cutCellWeights"), d, cw);
        SIM_VectorField &validFaces = object.addVectorFieldStandin("validFaces");
        makeVector(validFaces, d, nullptr);
        if (svx) makeVector(object.addVectorFieldStandin(GAS_NAME_COLLISIONVELOCITY), d, sv);

        Plugin plugin(nullptr);
        plugin.setOptionStandin(SIM_NAME_TOLERANCE, tolerance);
        plugin.setOptionStandin("maxIterations", max_iterations);
        plugin.setOptionStandin("useMGPreconditioner", use_mg);
        plugin.setOptionStandin("useOldPressure", use_old_pressure);
        SIM_Engine engine;
        if (!plugin.solveGasSubclass(engine, &object, 0, 1. / 24.))
            throw refstandin::AssertionFailed("the plugin refused its inputs: " + (plugin.errorsStandin().empty() ? std::string("?") : plugin.errorsStandin().back()));
        if (p.modificationsStandin() != 1 || velocity.modificationsStandin() != 1 || validFaces.modificationsStandin() != 1)
            throw refstandin::AssertionFailed("the plugin did not publish pressure, velocity and valid faces once each");
        for (int a = 0; a < 3; ++a)
        {
            read(v[a], *velocity.getField(a));
            read(valid[a], *validFaces.getField(a));
        }
        read(pressure, *p.getField());
    });
    if (rc != 0) return -1;
    const char *labels[6] = {"Iterations:", "Drifted relative L2 Error:", "Recomputed relative L2 Error:", "Max divergence:",
                             "Accumulated divergence:", "Average divergence:"};
    for (int s = 0; s < 6; ++s) stats[s] = numberAfter(theLastOutput, labels[s]);
    return 0;
}

} // extern "C"
