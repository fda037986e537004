/* mgps_fields.h -- C ABI of the plugin-side field pre/post-processing around the multigrid solve, on the
 * device.  These are the per-cell / per-face passes that
 * HDK_GeometricFreeSurfacePressureSolver::solveGasSubclass runs on the host before and after the solve
 * (reference: Source/HDK_GeometricFreeSurfacePressureSolver.cpp = "Plug.cpp", Source/HDK_Utilities.* =
 * "Util.h/.cpp"); with them the label / weight / right-hand-side grids are produced where the solver
 * consumes them and the projected velocity is produced from the pressure without a round trip.
 *
 * All pointers are DEVICE pointers; grids are dense, x fastest.  Base grid g = (gx, gy, gz): the simulation
 * grid.  Expanded grid e = (ex, ey, ez): the solver grid of mgps_expanded_layout, base cell c lives at
 * c + offset.  The face grid of axis a has one more entry along a; face f of axis a lies between cells
 * f - e_a (backward) and f (forward).  Material labels (int32): 0 SOLID, 1 LIQUID, 2 AIR (Util.h:17).
 * HDK samples the solid SDF and the solid velocity by interpolation at a position (Util.cpp:25,
 * Plug.cpp:925); here the caller passes them sampled at cell centres / face centres.
 * Deviations from the reference, both pinned by tests/test_reference_fields_parity.py against the reference's
 * plugin compiled unchanged: (1) the pre-sampled solid inputs above; with solid fields
 * aligned with the samples they are read at the two agree.  (2) Arithmetic is fp32 where the reference
 * computes in double on its fpreal32 fields, theta's clamp constant included (0.01f, 2.2e-8 below 0.01):
 * labels, valid faces and both pressure copies are bit-equal, weights within 4 eps32, right-hand side,
 * gradient and report within the per-element rounding bounds stated there.
 * `stream` is a hipStream_t (NULL = the null stream).  Return values: the status codes of mgps.h. */
#ifndef MGPS_FIELDS_H
#define MGPS_FIELDS_H

#include <stdint.h>

#include "mgps.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HDK::Utilities::buildMaterialCellLabels + isCellLiquid (Util.cpp:5-45, 87-148) */
int mgps_fields_material_labels(int32_t *material, const float *liquid_phi, const float *solid_phi, const float *cwx,
                                const float *cwy, const float *cwz, int gx, int gy, int gz, void *stream);
/* buildValidFaces / classifyValidFaces (Plug.cpp:716-744, Util.h:140-195): valid[f] = 1 where the cut-cell
 * weight is positive, both cells exist and one of them is LIQUID */
int mgps_fields_valid_faces(int axis, uint8_t *valid, const int32_t *material, const float *cut_weights, int gx, int gy,
                            int gz, void *stream);
/* buildMGDomainLabels (Plug.cpp:746-793) written straight into the expanded label grid
 * (buildExpandedCellLabels copy step, Ops.h:1364-1453): LIQUID -> INTERIOR, AIR -> DIRICHLET, else EXTERIOR */
int mgps_fields_domain_labels(uint8_t *expanded_labels, const int32_t *material, int gx, int gy, int gz, int ex, int ey,
                              int ez, int offset, void *stream);
/* buildMGBoundaryWeights (Plug.cpp:795-865) written straight into the expanded face grid
 * (buildExpandedBoundaryWeights, Ops.h:1524-1571): cut-cell weight on valid faces, divided by
 * clamp(theta, 0.01, 1) (ghost fluid, Util.h:25-42) on liquid/air faces, 0 elsewhere */
int mgps_fields_boundary_weights(int axis, float *expanded_weights, const float *cut_weights, const float *liquid_phi,
                                 const uint8_t *valid, const int32_t *material, int gx, int gy, int gz, int ex, int ey,
                                 int ez, int offset, void *stream);
/* setBoundaryCellLabels (Ops.h:1574-1644) on the device: same rule as mgps_set_boundary_labels */
int mgps_fields_set_boundary_labels(uint8_t *expanded_labels, const float *wx, const float *wy, const float *wz, int ex,
                                    int ey, int ez, void *stream);
/* buildRHS (Plug.cpp:867-943): weighted velocity divergence (plus the solid-velocity flux through the closed
 * part of each face when solid velocities are given; svx/svy/svz may all be NULL) at the expanded position
 * of every LIQUID cell, 0 elsewhere */
int mgps_fields_rhs(float *expanded_rhs, const int32_t *material, const float *vx, const float *vy, const float *vz,
                    const float *svx, const float *svy, const float *svz, const float *cwx, const float *cwy,
                    const float *cwz, int gx, int gy, int gz, int ex, int ey, int ez, int offset, void *stream);
/* applyOldPressure (Plug.cpp:945-997): expanded solution grid = old pressure at LIQUID cells, 0 elsewhere */
int mgps_fields_pressure_to_solution(float *expanded_x, const float *pressure, const int32_t *material, int gx, int gy,
                                     int gz, int ex, int ey, int ez, int offset, void *stream);
/* applySolutionToPressure (Plug.cpp:999-1047): pressure at LIQUID cells = solution; other cells untouched */
int mgps_fields_solution_to_pressure(float *pressure, const float *expanded_x, const int32_t *material, int gx, int gy,
                                     int gz, int ex, int ey, int ez, int offset, void *stream);
/* applyPressureGradient (Plug.cpp:1049-1131): velocity -= grad p on valid faces, ghost-fluid scaled on
 * liquid/air faces */
int mgps_fields_pressure_gradient(int axis, float *velocity, const float *liquid_phi, const float *pressure,
                                  const uint8_t *valid, const int32_t *material, int gx, int gy, int gz, void *stream);
/* ---- surface tension: a non-zero interface pressure on liquid/air faces (ghost fluid) ---------------
 * sp is a base cell grid of surface pressure in the units of `pressure`.  On a valid liquid/air face with liquid cell L, air cell
 * A and theta = clamp(liquid fraction from L, 0.01, 1) (the theta of mgps_fields_boundary_weights), the interface pressure is
 * p_G = (1 - theta) sp[L] + theta sp[A].  No counterpart in the reference, which holds p_G at 0. */
/* sp = scale * clamp(kappa, -1, 1) at every LIQUID or AIR cell with a 6-neighbour of the other kind, 0 elsewhere; kappa is the
 * mean curvature div(grad phi / |grad phi|) of liquid_phi at the cell centre (unit-spacing central differences, indices clamped
 * into the grid; 0 where |grad phi|^2 < 1e-30).  scale = sigma dt / (density dx^2) gives the pressure of a surface tension sigma */
int mgps_fields_surface_pressure(float *sp, const float *liquid_phi, const int32_t *material, double scale, int gx, int gy, int gz,
                                 void *stream);
/* expanded_rhs[L] += w_f p_G over the liquid/air faces of every LIQUID cell, on top of the rhs mgps_fields_rhs built; w_f is the
 * expanded weight mgps_fields_boundary_weights wrote (wx/wy/wz: the expanded face grids).  p_gamma_max (device, may be NULL;
 * initialise it) is raised to the largest |p_G| */
int mgps_fields_rhs_surface(float *expanded_rhs, const float *wx, const float *wy, const float *wz, const float *liquid_phi,
                            const int32_t *material, const float *sp, float *p_gamma_max, int gx, int gy, int gz, int ex, int ey,
                            int ez, int offset, void *stream);
/* mgps_fields_pressure_gradient with the air cell's pressure replaced by p_G on liquid/air faces */
int mgps_fields_pressure_gradient_surface(int axis, float *velocity, const float *liquid_phi, const float *pressure, const float *sp,
                                          const uint8_t *valid, const int32_t *material, int gx, int gy, int gz, void *stream);
/* computeResultingDivergence (Plug.cpp:1133-1207): out_host[3] = {sum, max (starting from 0), LIQUID cell
 * count} of the weighted divergence over LIQUID cells; synchronises the stream */
int mgps_fields_divergence(double out_host[3], const int32_t *material, const float *vx, const float *vy, const float *vz,
                           const float *svx, const float *svy, const float *svz, const float *cwx, const float *cwy,
                           const float *cwz, int gx, int gy, int gz, void *stream);

/* ---- the whole of solveGasSubclass between "fields fetched" and "fields written back" in one call ------------------
 * HDK_GeometricFreeSurfacePressureSolver::solveGasSubclass (Plug.cpp:252-707) on HOST arrays: what the Houdini shim
 * (host/HDK_GeometricFreeSurfacePressureSolver.cpp) calls after flattening the SIM fields.  Uploads the inputs, runs
 * the device passes above in the reference's order -- material labels (Plug.cpp:270), valid faces (286), MG domain
 * labels + boundary weights + expansion + boundary labels (316-362), rhs (386), warm start (413) -- builds the
 * multigrid solver from the device grids, runs solveGeometricConjugateGradient (426-629), then pressure write-back,
 * pressure gradient and the divergence report (637-707), and downloads pressure, velocity and the valid-face flags.
 * Arrays are dense, x fastest, of `real_bytes` = 4 (float) or 8 (double: converted on the device); face grids have one
 * more entry along their axis.  The solid SDF and the solid velocity are passed sampled at cell / face centres. */
typedef struct mgps_projection {
    int struct_size;               /* sizeof(mgps_projection) */
    int gx, gy, gz;                /* simulation grid */
    int real_bytes;                /* 4 or 8: the type behind every `void *` real array below */
    const void *liquid_phi;        /* cell grid: liquid SDF ("surface") */
    const void *solid_phi;         /* cell grid: solid SDF ("collision") */
    const void *cut_weights[3];    /* face grids ("cutCellWeights") */
    void *velocity[3];             /* face grids, in: velocity, out: projected velocity */
    const void *solid_velocity[3]; /* face grids ("collisionvelocity"), or all NULL */
    void *pressure;                /* cell grid, in: previous pressure (read when use_old_pressure), out: pressure */
    uint8_t *valid_faces[3];       /* out, face grids: 1 = valid face (each may be NULL: not wanted) */
    int use_old_pressure;          /* "useOldPressure" */
    int use_mg_preconditioner;     /* "useMGPreconditioner" */
    int use_gauss_seidel;          /* 1 = the plugin's choice (Plug.cpp:466) */
    double tolerance;              /* SIM_NAME_TOLERANCE */
    int max_iterations;            /* "maxIterations" */
    int power_of_two;              /* 1 = the reference's expansion (Ops.h:1353-1360), 0 = tight extents */
    /* results */
    mgps_pcg_stats stats;
    int mg_levels, offset, expanded[3];
    double liquid_cells;
    double residual_inf, residual_l2;       /* of the computed solution (Plug.cpp:625-628; infNorm is the signed max) */
    double divergence_sum, divergence_max;  /* after the projection (Plug.cpp:704-706); divergence_count = liquid_cells */
    double setup_ms, solve_ms, total_ms;    /* host wall clock: everything before the solve / the solve / the whole call */
    /* options.enclosed_liquid: the liquid components that touch no air (mgps_enclosed_components) and the largest |mean| of the
       right-hand side removed on one of them (mgps_project_enclosed; rhs units).  On such a component the reported divergence
       is that mean: the part no pressure can remove.  0 / 0 with the option off */
    int enclosed_components;
    double rhs_mean_removed_max;
    /* surface tension: the liquid/air faces carry the interface pressure p_G of the surface pressure sp
       instead of 0.  sp is either sigma * curvature, from liquid_phi (surface_tension = sigma > 0: dt, dx, density are read then,
       and only then), or the caller's cell grid `surface_pressure` in the units of `pressure` (type: real_bytes).  Not both; with
       neither, the call is the plain projection */
    double surface_tension;            /* sigma, in the units of density * dx^3 / dt^2; 0 = off */
    double dt, dx, density;            /* time step, cell size, constant liquid density */
    const void *surface_pressure;      /* cell grid, or NULL */
    double surface_pressure_max;       /* result: the largest |p_G| applied (pressure units); 0 when off */
} mgps_projection;
/* status MGPS_ERR_HIERARCHY with outcome MGPS_PCG_RHS_ZERO-like early outs are reported through stats.outcome; a domain
 * without liquid returns MGPS_OK with liquid_cells = 0 and leaves velocity and pressure untouched.
 * MGPS_ERR_INTERRUPTED (opt->interrupt): the call still publishes -- pressure and velocity are those of the iterate
 * mgps_solve_pcg hands back (include/mgps.h), i.e. of the same call with max_iterations = the updates applied before the stop;
 * stats says which (outcome MGPS_PCG_MAX_ITERATIONS, iterations), residual_inf / residual_l2 are not evaluated (0) */
int mgps_project_free_surface(mgps_projection *p, const mgps_options *opt);

/* ---- the fields layer on Z-slabs -----------------------------------------------------------------------
 * One rank of a slab run (include/mgps.h, "multi-GPU") holds a z-window of every field.  With the cuts splits[0..size] of the
 * EXPANDED grid (the cuts mgps_create_slab_ranges takes), rank r owns the expanded planes [e0, e1) = [splits[r], splits[r + 1])
 * and the base planes [c0, c1), c0 = clamp(e0 - offset, 0, gz), c1 = clamp(e1 - offset, 0, gz).  Cell grids, x-face grids and
 * y-face grids hold the rank's c1 - c0 planes; z-face grids hold c1 - c0 + 1 planes, the faces c0 .. c1 (the convention of
 * wz_slab): the face plane on a cut exists on both neighbours, with the same input values, and each rank updates its own copy.
 * Expanded grids hold the e1 - e0 planes of the window (the expanded z-face grid e1 - e0 + 1).  A rank without base planes has
 * no window: c0 < c1 is required.
 * The passes do no communication.  What a pass reads of a neighbour's planes arrives as halo-plane pointers, one plane of gx * gy
 * entries each: `*_lo` is base plane c0 - 1, `*_hi` base plane c1; NULL at the ends of the grid (c0 = 0, c1 = gz), where the
 * passes behave as the whole-grid passes do at the grid boundary.  Results equal those of the whole-grid passes on the rank's
 * planes: labels and flags exactly, floats to the last place. */
typedef struct mgps_fields_slab {
    int struct_size; /* sizeof(mgps_fields_slab) */
    int gx, gy, gz;  /* the whole base grid */
    int c0, c1;      /* owned base planes */
    int ex, ey, ez;  /* the whole expanded grid */
    int offset;
    int e0, e1;      /* owned expanded planes */
} mgps_fields_slab;
/* The layout of a slab projection, on the host (no device needed): mgps_expanded_layout(gx, gy, gz, 0, power_of_two) and cuts
 * out_splits[0 .. size] that mgps_create_slab_ranges accepts (every cut even, a multiple of 16 with Gauss-Seidel, at least 16
 * planes per rank) and that divide the BASE planes as evenly as that granularity allows (an even cut of the expanded grid would
 * leave the end ranks with EXTERIOR padding only); every rank owns at least one base plane.  MGPS_ERR_INVALID_ARGUMENT with a
 * message where no such cuts exist.  Callers may pass cuts of their own to the calls below (mgps_slab_partition on the labels
 * of the previous sub-step, say). */
int mgps_projection_slab_layout(int gx, int gy, int gz, int power_of_two, int size, int use_gauss_seidel, int out_expanded[3],
                                int *out_offset, int *out_levels, int *out_splits);
/* fills `out` for rank `rank` of the cuts `splits` (size + 1 entries); MGPS_ERR_INVALID_ARGUMENT when the cuts do not run from 0
 * to ez increasing or when ANY rank owns no base plane (the verdict depends on the shared arguments only) */
int mgps_fields_slab_describe(mgps_fields_slab *out, int gx, int gy, int gz, int power_of_two, const int *splits, int size, int rank);
/* mgps_fields_material_labels on the window.  material: c1 - c0 planes */
int mgps_fields_slab_material_labels(const mgps_fields_slab *d, int32_t *material, const float *liquid_phi, const float *phi_lo,
                                     const float *phi_hi, const float *solid_phi, const float *cwx, const float *cwy, const float *cwz,
                                     void *stream);
/* One faces pass: mgps_fields_valid_faces and mgps_fields_boundary_weights of all three axes.  valid[3]: the window's base face
 * grids; expanded_weights[3]: the window's expanded face grids, written everywhere (0 outside the base box: no fill first) */
int mgps_fields_slab_faces(const mgps_fields_slab *d, uint8_t *const valid[3], float *const expanded_weights[3], const int32_t *material,
                           const int32_t *material_lo, const int32_t *material_hi, const float *liquid_phi, const float *phi_lo,
                           const float *phi_hi, const float *const cut_weights[3], void *stream);
/* One labels pass: mgps_fields_domain_labels and mgps_fields_set_boundary_labels on the window's e1 - e0 expanded planes, written
 * everywhere (EXTERIOR outside the base box).  The domain label is a function of the material label, so the material halo is
 * the label halo BOUNDARY marking needs.  expanded_weights: what mgps_fields_slab_faces wrote */
int mgps_fields_slab_labels(const mgps_fields_slab *d, uint8_t *expanded_labels, const int32_t *material, const int32_t *material_lo,
                            const int32_t *material_hi, const float *const expanded_weights[3], void *stream);
/* mgps_fields_rhs / mgps_fields_pressure_to_solution on the window's expanded planes, written everywhere (0 outside LIQUID cells) */
int mgps_fields_slab_rhs(const mgps_fields_slab *d, float *expanded_rhs, const int32_t *material, const float *const velocity[3],
                         const float *const solid_velocity[3], const float *const cut_weights[3], void *stream);
int mgps_fields_slab_pressure_to_solution(const mgps_fields_slab *d, float *expanded_x, const float *pressure, const int32_t *material,
                                          void *stream);
/* mgps_fields_solution_to_pressure; clear_others != 0 writes 0 to every cell that is not LIQUID instead of leaving it */
int mgps_fields_slab_solution_to_pressure(const mgps_fields_slab *d, float *pressure, const float *expanded_x, const int32_t *material,
                                          int clear_others, void *stream);
/* mgps_fields_pressure_gradient of all three axes in one pass (sp != NULL: mgps_fields_pressure_gradient_surface) */
int mgps_fields_slab_pressure_gradient(const mgps_fields_slab *d, float *const velocity[3], const float *liquid_phi, const float *phi_lo,
                                       const float *phi_hi, const float *pressure, const float *pressure_lo, const float *pressure_hi,
                                       const float *sp, const float *sp_lo, const float *sp_hi, const uint8_t *const valid[3],
                                       const int32_t *material, const int32_t *material_lo, const int32_t *material_hi, void *stream);
/* mgps_fields_surface_pressure / mgps_fields_rhs_surface on the window (curvature indices clamped to the whole grid) */
int mgps_fields_slab_surface_pressure(const mgps_fields_slab *d, float *sp, const float *liquid_phi, const float *phi_lo,
                                      const float *phi_hi, const int32_t *material, const int32_t *material_lo, const int32_t *material_hi,
                                      double scale, void *stream);
int mgps_fields_slab_rhs_surface(const mgps_fields_slab *d, float *expanded_rhs, const float *const expanded_weights[3],
                                 const float *liquid_phi, const float *phi_lo, const float *phi_hi, const int32_t *material,
                                 const int32_t *material_lo, const int32_t *material_hi, const float *sp, const float *sp_lo,
                                 const float *sp_hi, float *p_gamma_max, void *stream);
/* the rank's part of mgps_fields_divergence: out_host[3] = {sum, max (from 0), LIQUID cell count} over the window's cells (every
 * face of an owned cell is in the window); the caller sums / maximises over the ranks.  Synchronises the stream */
int mgps_fields_slab_divergence(const mgps_fields_slab *d, double out_host[3], const int32_t *material, const float *const velocity[3],
                                const float *const solid_velocity[3], const float *const cut_weights[3], void *stream);

/* mgps_project_free_surface on the DEVICE fields of one slab rank; a collective over `comm`: every rank calls it with the same
 * gx, gy, gz (the WHOLE grid), options, cuts and switches.  Every array is a device float32 array of the rank's window as defined
 * above; valid_faces are device uint8 outputs (each may be NULL).  With comm->size = 1 it is the device-resident projection on
 * one GPU.  Steps, in the order of mgps_project_free_surface: liquid_phi plane exchange, material labels, material plane
 * exchange, the faces pass and the labels pass; liquid cell count (all-reduce; no liquid anywhere: valid faces and zero pressure
 * are published, outcome MGPS_PCG_RHS_ZERO); mgps_create_slab_device_labels on the rank's own label planes and weights (borrowed:
 * the labels never leave the device, the constructor fetches its label halo from the neighbours; with options.host_setup or
 * MGPS_HOST_SETUP=1 the whole grid's labels go to every rank's host first -- gatherv to rank 0, scatterv with every rank's range
 * set to the whole buffer: ex * ey * ez bytes per rank, 1 GiB at 1024^3 -- for mgps_create_slab_device_weights); rhs, warm start, surface term (after an exchange of the sp plane), enclosed-liquid projection,
 * mgps_solve_pcg, residual norms; pressure write-back, pressure plane exchange, gradient on the owned faces (both copies of a
 * cut's z-face plane get the same bits), divergence report and surface_pressure_max from one all-reduce.  Every rank-local failure
 * is folded into the next all-reduce: all ranks return the same status, the failing rank with its own message, the others with
 * "rank R failed (<where>, status S)".  With comm->size = 1 no transport entry is called.  The exception is the transport itself: a rank whose
 * exchange, all-reduce, gatherv or scatterv call fails returns MGPS_ERR_COMM at once and alone (nothing can carry its status; the
 * other ranks are left in a collective of a broken transport, as on the slab solvers).  A transport without gatherv / scatterv is refused when
 * size > 1, before any device work (the collapse of uneven cuts, the enclosed-liquid merge and the host set-up's labels use them).
 * The cuts are the caller's (mgps_projection_slab_layout, or mgps_slab_partition_device on the labels of an earlier sub-step).  MGPS_ERR_INTERRUPTED: as mgps_project_free_surface. */
typedef struct mgps_projection_slab {
    int struct_size;                /* sizeof(mgps_projection_slab) */
    int gx, gy, gz;                 /* the WHOLE simulation grid */
    const float *liquid_phi, *solid_phi;
    const float *cut_weights[3];
    float *velocity[3];             /* in: velocity, out: projected velocity */
    const float *solid_velocity[3]; /* or all NULL */
    float *pressure;
    uint8_t *valid_faces[3];        /* out (each may be NULL: not wanted) */
    int use_old_pressure, use_mg_preconditioner, use_gauss_seidel;
    double tolerance;
    int max_iterations, power_of_two;
    /* results: the whole grid's numbers, the same on every rank */
    mgps_pcg_stats stats;
    int mg_levels, offset, expanded[3];
    double liquid_cells;
    double residual_inf, residual_l2;
    double divergence_sum, divergence_max;
    double setup_ms, solve_ms, total_ms; /* this rank's host wall clock */
    int enclosed_components;
    double rhs_mean_removed_max;
    double surface_tension, dt, dx, density;
    const float *surface_pressure;  /* cell grid of the window, or NULL */
    double surface_pressure_max;
    /* this rank's host wall clock per stage, ms: [0] plane exchanges + material, faces and labels passes + liquid count,
       [1] the ranks' agreement in front of the constructor (host set-up: with the whole grid's labels to every rank's host), [2] solver set-up, [3] rhs, warm start, surface term, enclosed projection, [4] solve +
       residual norms, [5] write-back, gradient, divergence report, [6] of all that: inside the plane exchanges, [7] reserved */
    double stage_ms[8];
} mgps_projection_slab;
int mgps_project_free_surface_slab(mgps_projection_slab *p, const mgps_options *opt, const mgps_comm *comm, const int *splits,
                                   void *stream);

/* ---- velocity extrapolation into the air band ------------------------------------------------------------
 * The projection leaves a velocity that is defined on valid faces only; advection needs it a few cells further out.  The passes
 * below carry it there breadth first, layer by layer, on one face grid of axis a.  No counterpart in the reference, which hands
 * its validFaces field to a downstream extrapolation (Plug.cpp:155-166, 711); the definition here is the contract.
 *   layer (uint8 face grid, out): 0 where valid == 1, 255 elsewhere, written by every call (no continuation state).
 *   For l = 1 .. layers (1 <= layers <= 254): every face f with layer[f] == 255 -- and cut_weights[f] > 0 when cut_weights is
 *   given -- that has a KNOWN neighbour gets the mean of its known neighbours' velocities and layer[f] = l.  The neighbours are
 *   the 6 faces -x, +x, -y, +y, -z, +z of the same face grid (one outside the grid does not exist); n is known when layer[n] < l.
 *   The mean is a float32 sum over the known neighbours in that order, divided by their count.
 * Every other face keeps its velocity bit for bit: valid faces, faces never reached, closed faces (never written, never known).
 * A layer reads values of layers < l only and writes faces of layer 255 only: it runs in place, without a second velocity grid
 * and without atomics on values, and the same inputs give the same bits whatever the order of execution. */
int mgps_fields_extrapolate(int axis, float *velocity, uint8_t *layer, const uint8_t *valid, const float *cut_weights /* or NULL */,
                            int layers, int gx, int gy, int gz, void *stream);
/* the three axes with one launch per layer: the bits of three mgps_fields_extrapolate calls.  cut_weights: NULL, or all three.
 * filled_dev (device, [3], may be NULL): the faces given a value per axis, ADDED to what the array holds (initialise it) */
int mgps_fields_extrapolate3(float *const velocity[3], uint8_t *const layer[3], const uint8_t *const valid[3],
                             const float *const cut_weights[3] /* or NULL */, int layers, int gx, int gy, int gz,
                             unsigned long long *filled_dev, void *stream);
/* One layer on a slab window, without communication.  l == 0 writes `layer` from `valid` (valid is read then, and only then);
 * 1 <= l <= 254 computes layer l.  velocity / layer / valid / cut_weights: the window's face grids.  Halo planes as everywhere in
 * this header for the x-face and y-face grids (base planes c0 - 1 and c1); the z-face window holds the faces c0 .. c1, so its
 * halos are the face planes c0 - 1 and c1 + 1.  All halos of a side are NULL where the grid ends, and unused with l == 0.  The
 * two copies of a cut's z-face plane see the same neighbours and come out with the same bits.  filled_dev (device, [3], may be
 * NULL) is raised by the faces filled; of the z-faces the planes c0 .. c1 - 1 count, on the last rank also plane gz, so that a sum
 * over the ranks counts every face once */
int mgps_fields_slab_extrapolate_layer(const mgps_fields_slab *d, int l, float *const velocity[3], uint8_t *const layer[3],
                                       const uint8_t *const valid[3], const float *const velocity_lo[3], const float *const velocity_hi[3],
                                       const uint8_t *const layer_lo[3], const uint8_t *const layer_hi[3],
                                       const float *const cut_weights[3] /* or NULL */, unsigned long long *filled_dev, void *stream);
/* The extrapolation on the DEVICE fields of one slab rank, a collective over `comm`: every rank calls it with the same gx, gy,
 * gz (the WHOLE grid), power_of_two, layers and cuts -- those of mgps_project_free_surface_slab, on whose velocity and valid_faces
 * it is meant to run.  Per layer one `exchange` message per neighbour carries the velocity planes and the layer planes of the
 * three axes, packed; one launch follows.  With comm->size = 1 it is the device-resident extrapolation on one GPU: no exchange and
 * no all-reduce; gatherv / scatterv are never used.  What every rank shares (struct_size, extents, layers, the cuts) is refused at
 * once; a rank-local failure (a missing array, an allocation) is carried by an all-reduce in front of the first exchange, a later
 * one by the all-reduce at the end that sums `filled`: all ranks return the same status.  A rank whose transport call fails
 * returns MGPS_ERR_COMM at once and alone, as in mgps_project_free_surface_slab. */
typedef struct mgps_extrapolation_slab {
    int struct_size;               /* sizeof(mgps_extrapolation_slab) */
    int gx, gy, gz;                /* the WHOLE simulation grid */
    int power_of_two;              /* the expansion the cuts refer to */
    int layers;                    /* 1 .. 254 */
    float *velocity[3];            /* the window's face grids, in/out */
    const uint8_t *valid_faces[3]; /* what mgps_project_free_surface_slab published */
    const float *cut_weights[3];   /* all three, or all NULL */
    uint8_t *layer[3];             /* out; each may be NULL: not wanted */
    /* results */
    unsigned long long filled[3];  /* faces given a value per axis, of the whole grid: the same on every rank */
    double total_ms, exchange_ms;  /* this rank's host wall clock: the call / inside the exchanges */
} mgps_extrapolation_slab;
int mgps_extrapolate_velocity_slab(mgps_extrapolation_slab *e, const mgps_comm *comm, const int *splits, void *stream);

/* ---- pressure feedback: net pressure force and torque on solid bodies -------------------------------------
 * The projection takes the solid velocity through the closed part 1 - w of every cut face (mgps_fields_rhs); this is the other
 * half, the operator J^T p: what the pressure pushes back with, summed per body.  No counterpart in the reference; the definition
 * here is the contract.
 *   Device inputs on the base grid: pressure (float cell grid), material (int32 cell grid), the three cut-weight face grids and
 *   body[3], int32 face grids: the id of the body that owns the closed part of a face, sampled by the caller at the face centre
 *   (as solid_velocity is).  Host inputs: bodies (1 .. 255), centres[(bodies + 1) * 3] doubles (x, y, z in cell units from the
 *   grid's corner: cell (i, j, k) has its centre at (i + 1/2, j + 1/2, k + 1/2), the x-face (i, j, k) at (i, j + 1/2, k + 1/2)) and
 *   scale.
 *   Face f of axis a with backward cell B and forward cell F (a cell outside the grid does not exist):
 *     w = cut_weights[a][f], closed fraction s = w < 1.f ? 1.f - w : 0.f in float32 (the expressions of the right-hand side);
 *     pB = pressure[B] if B exists and material[B] == LIQUID, else 0; pF likewise;
 *     the face is WET when s > 0 and B or F is LIQUID;
 *     phi = double(s) * (double(pB) - double(pF)): the push of the liquid on the solid along +a;
 *     row r = body[a][f] if 1 <= body[a][f] <= bodies, else 0.
 *   Row 0 collects every wet face no body owns (static walls, ids out of range): every wet face lands in exactly one row and the
 *   sum of the force columns over the rows does not depend on the ids.
 *   out_host[(bodies + 1) * 8] doubles, one row per r: [0..2] scale * sum of phi e_a (force), [3..5] scale * sum of
 *   (x_f - centres[r]) x (phi e_a) (torque, arm in cells), [6] sum of s (wet closed area in faces, not scaled), [7] the number of
 *   wet faces.  Sums are in fp64, in an order that is the implementation's but fixed: the same inputs give the same bits on every
 *   run (no floating-point atomics; the launch shape depends on the extents and on `bodies` only).
 * Units: the pressure is in velocity units (velocity -= p_F - p_B), so scale = density dx^3 / dt gives the force in newtons; the
 * torque then still needs a factor dx.
 * Limits: an AIR cell contributes 0 -- with surface tension on, the interface pressure p_G is not seen by this pass; 255 bodies
 * per call; the cell-centred pressure sits half a cell off the face.
 * Adjoint of the solid term of the right-hand side: with zero fluid velocity and solid velocities sv, the right-hand side is
 * rhs_c = sum_a (1 - w_back) sv_back - (1 - w_fwd) sv_fwd at LIQUID c, hence sum_c p_c rhs_c = - sum_a sum_f sv_a[f] phi_a[f]; for
 * a rigid motion sv_a[f] = (U_r + omega_r x (x_f - centres[r]))_a per row that is - sum_r (U_r . F_r + omega_r . T_r) at scale 1.
 * Every entry refuses, before any device work: a NULL array, bodies outside 1 .. 255, a non-positive extent. */
/* on whole grids; synchronises the stream */
int mgps_fields_solid_forces(double *out_host, const float *pressure, const int32_t *material, const float *cwx, const float *cwy,
                             const float *cwz, const int32_t *bx, const int32_t *by, const int32_t *bz, const double *centres_host,
                             int bodies, double scale, int gx, int gy, int gz, void *stream);
/* The rank's part on a slab window, without communication: out_host holds the sums over the window's faces, the caller adds the
 * ranks' rows.  The x- and y-faces of the owned planes count; of the z-faces the planes c0 .. c1 - 1, on the last rank also plane
 * gz (the counting rule of filled_dev above): a sum over the ranks counts every face once.  Only the lower halo is read: base
 * plane c0 - 1 of pressure and material (NULL at c0 == 0, required elsewhere).  cut_weights / body: the window's face grids;
 * positions use the plane index of the whole grid.  Synchronises the stream */
int mgps_fields_slab_solid_forces(const mgps_fields_slab *d, double *out_host, const float *pressure, const float *pressure_lo,
                                  const int32_t *material, const int32_t *material_lo, const float *const cut_weights[3],
                                  const int32_t *const body[3], const double *centres_host, int bodies, double scale, void *stream);
/* The forces on the DEVICE fields of one slab rank, a collective over `comm` on what mgps_project_free_surface_slab took
 * (liquid_phi, solid_phi, cut_weights) and published (pressure), with the same gx, gy, gz (the WHOLE grid), power_of_two and cuts.
 * Steps: the liquid_phi plane is traded with both neighbours; mgps_fields_slab_material_labels makes the projection's labels
 * again; one packed message to the upper neighbour -- the rank's last pressure plane and last material plane; nothing goes down,
 * since only the lower halo is read -- ; the window pass; one all-reduce (sum) of the rows with the ranks' statuses folded in.  With comm->size =
 * 1 it is the device-resident form: no exchange and no all-reduce; gatherv / scatterv are never used.  What every rank shares
 * (struct_size, extents, bodies, the cuts, the transport) is refused at once; a rank-local failure (a missing array, a failing
 * kernel) is carried by the all-reduce, the rank still takes part in both exchanges: all ranks return the same status, the failing
 * rank with its own message, the others with "rank R failed (rows, status S)".  A rank
 * whose transport call fails returns MGPS_ERR_COMM at once and alone, as in mgps_project_free_surface_slab; so does, with
 * MGPS_ERR_ALLOC or MGPS_ERR_NO_DEVICE, a rank that cannot get the buffers an exchange needs.
 * The struct and the call share one name, as stat does: a struct tag, not a typedef (write `struct mgps_solid_forces_slab`). */
struct mgps_solid_forces_slab {
    int struct_size;             /* sizeof(struct mgps_solid_forces_slab) */
    int gx, gy, gz;              /* the WHOLE simulation grid */
    int power_of_two;            /* the expansion the cuts refer to */
    int bodies;                  /* 1 .. 255 */
    const float *pressure;       /* the window's device arrays: what the projection published ... */
    const float *liquid_phi, *solid_phi; /* ... and took */
    const float *cut_weights[3];
    const int32_t *body[3];
    const double *centres;       /* host, (bodies + 1) * 3 */
    double scale;
    double *out;                 /* host, (bodies + 1) * 8: the whole grid's numbers, the same on every rank */
    double total_ms, exchange_ms; /* this rank's host wall clock: the call / inside the exchanges */
};
int mgps_solid_forces_slab(struct mgps_solid_forces_slab *s, const mgps_comm *comm, const int *splits, void *stream);

/* ---- two-way rigid-body coupling: body velocities solved with the pressure ---------------------------------
 * mgps_fields_rhs takes a solid velocity, mgps_fields_solid_forces returns what the pressure pushes back with; the entries below
 * close the loop for rigid bodies that the liquid moves (Batty, Bertails & Bridson 2007).  No counterpart in the reference; the
 * definition here is the contract.
 *   A body r = 1 .. bodies moves with V_r = (U_r, omega_r): sv_a[f] = (U_r + omega_r x (x_f - centres[r]))_a on the faces whose row
 *   (section "pressure feedback" above: body[a][f] if 1 <= body[a][f] <= bodies, else 0) is r.  G maps the motions to the solid
 *   part of the right-hand side: (G V)_c = sum_a s_back sv_back - s_fwd sv_fwd at a LIQUID cell c, s the closed fraction
 *   w < 1.f ? 1.f - w : 0.f of the face; faces of row 0 (walls, scripted solids, ids out of range) are not part of G.  By the
 *   adjoint identity above the rows of mgps_fields_solid_forces at scale 1 are (F, T) = - G^T p.
 *   With lengths in cells and the pressure in velocity units a body answers the pressure with V_out = V* + K (F, T)(p), K block
 *   diagonal per body: inv_mass * I_3 on the force and the symmetric 3 x 3 inv_inertia (world frame, about centres[r]) on the torque,
 *   inv_mass = density dx^3 / m, inv_inertia = density dx^5 I^-1.  inv_mass = 0 and inv_inertia = 0: a kinematic body, the one-way
 *   behaviour of mgps_fields_rhs alone.  Substituting V_out into A p = b_fluid + G V_out gives the symmetric positive definite system
 *   (A + G K G^T) p = b_fluid + G V*, which mgps_solve_pcg_coupled solves; the right-hand side is mgps_fields_rhs with the solid
 *   velocity mgps_fields_rigid_velocity writes from V*.
 * Arithmetic: fp64 from the float32 fields and the host tables; every sum over cells has one order, fixed by the extents and the
 * inputs (wave butterfly, per-workgroup tables, one sum in workgroup order; no floating-point atomics): the same inputs give the
 * same bits on every run. */
/* sv_a[f] = float((U_r + omega_r x (x_f - centres[r]))_a), formed in fp64 and rounded once, on every face with row r >= 1; every
 * other face keeps its value (walls and scripted solids stay the caller's).  motions_host[(bodies + 1) * 6]: U then omega per row
 * (row 0 is not read); centres_host[(bodies + 1) * 3] as in mgps_fields_solid_forces.  Refuses what that entry refuses. */
int mgps_fields_rigid_velocity(float *svx, float *svy, float *svz, const int32_t *bx, const int32_t *by, const int32_t *bz,
                               const double *centres_host, const double *motions_host, int bodies, int gx, int gy, int gz, void *stream);
/* The same on a slab window (no communication): sv / body are the window's face grids, face positions use the plane index of the
 * whole grid (k + c0).  The bits are those of the whole-grid pass on the rank's planes; both copies of a cut's z-face plane get
 * the same bits.  Refuses, before any device work: not a slab window, bodies outside 1 .. 255, a NULL array. */
int mgps_fields_slab_rigid_velocity(const mgps_fields_slab *d, float *const sv[3], const int32_t *const body[3], const double *centres_host,
                                    const double *motions_host, int bodies, void *stream);

/* The coupling object: the list of COUPLED cells -- LIQUID cells with at least one face of s > 0 and row >= 1 -- made on the device
 * (count, scan, compact) from the base grids; per cell its expanded index and, for its six faces, the row and the signed s (+ on
 * the backward, - on the forward face).  A cell appears once whatever the number of bodies it touches; the list is in base-cell
 * order.  The kernels of an application run over the list only.  The grids are read by mgps_coupling_create and not kept; the
 * object owns its device memory and its scratch: one call at a time per object. */
typedef struct mgps_coupling mgps_coupling;
typedef struct mgps_coupling_desc {
    int struct_size;             /* sizeof(mgps_coupling_desc) */
    int gx, gy, gz;              /* base grid */
    int ex, ey, ez, offset;      /* the expanded layout (mgps_expanded_layout): base cell c lives at c + offset */
    int bodies;                  /* 1 .. 255 */
    const int32_t *material;     /* device, base cell grid */
    const float *cut_weights[3]; /* device, base face grids */
    const int32_t *body[3];      /* device, base face grids of body ids */
    const double *centres;       /* host, (bodies + 1) * 3; row 0 is not read */
    const double *inv_mass;      /* host, bodies + 1; row 0 is not read */
    const double *inv_inertia;   /* host, (bodies + 1) * 6 in the order xx, yy, zz, xy, xz, yz; row 0 is not read */
} mgps_coupling_desc;
/* Refuses, before any device work: NULL / struct_size mismatch, a NULL array, bodies outside 1 .. 255, a non-positive extent, an
 * expanded box that does not hold the base grid at `offset` or has 2^31 cells or more, a negative or non-finite inv_mass, a
 * negative or non-finite diagonal entry of inv_inertia.  Synchronises the stream (the list's length comes to the host). */
int mgps_coupling_create(mgps_coupling **out, const mgps_coupling_desc *d, void *stream);
/* The coupling of one rank of a slab run ("on slab ranks").  desc->gx .. ez and offset are the WHOLE grid's
 * and must equal the window's; desc->material, cut_weights and body are the window's device grids (c1 - c0 planes, of the z-faces
 * c0 .. c1).  The list holds the rank's OWN coupled cells: LIQUID cells of its base planes [c0, c1) with a face of s > 0 and row
 * >= 1, each with all six faces -- a cell of the last owned plane carries its forward z-face on the cut, whoever holds the cell
 * across it.  A cell has one owner: the ranks' lists together are the whole grid's list and no face term is counted twice or
 * dropped.  The stored index is the cell's index in the rank's e1 - e0 expanded planes, the fine level of its slab solver.  No halo
 * plane is read: the cell is LIQUID, so a face of w < 1 is wet whatever lies across the cut.
 * Creation does no communication; it copies `comm` (comm->user must outlive the object) for the collectives below.  Refuses, before
 * any device work: what mgps_coupling_create refuses (the 2^31 limit applies to the window's expanded cells), a window that is not
 * one or does not match the desc, a comm without exchange and allreduce.
 * On such an object mgps_coupling_apply, mgps_coupling_impulses and mgps_coupling_velocities are COLLECTIVES: every rank calls them,
 * with its own window of x (and y), and each makes one sum all-reduce of g, (bodies + 1) * 6 doubles -- on the stream through
 * comm->allreduce_device where the transport has it, through the host otherwise.  A rank whose list is empty takes part all the
 * same.  impulses and velocities return the whole grid's numbers, the same bits on every rank; mgps_coupling_cells the rank's own
 * count; mgps_coupling_set_bodies stays local (every rank passes the same tables).  A failing transport call returns MGPS_ERR_COMM
 * at once, on that rank.  A world of one asks its transport nothing and computes the bits of the whole-grid object.  Sums stay in
 * fp64 in one fixed order per rank; for fixed inputs, cuts and transport the bits repeat. */
int mgps_coupling_create_slab(mgps_coupling **out, const mgps_coupling_desc *desc, const mgps_fields_slab *window, const mgps_comm *comm,
                              void *stream);
void mgps_coupling_destroy(mgps_coupling *c);
/* new centres and K for the same list (a sub-step that moves the bodies but not the grids' faces); checks as above */
int mgps_coupling_set_bodies(mgps_coupling *c, const double *centres_host, const double *inv_mass_host, const double *inv_inertia_host,
                             void *stream);
int mgps_coupling_cells(const mgps_coupling *c, int64_t *count);
/* x, y: expanded float32 grids.  y[c] = float(double(y[c]) + (G K G^T x)_c) on the coupled cells; nothing else is touched.  Three
 * launches: gather g = - G^T x ((bodies + 1) * 6 doubles, on the device), its sum with W = K g, scatter.  No synchronisation */
int mgps_coupling_apply(mgps_coupling *c, float *y_dev, const float *x_dev, void *stream);
/* out_host[(bodies + 1) * 6]: (F, T) = - G^T x per row at scale 1, row 0 zero: columns 0 .. 5 of mgps_fields_solid_forces on the
 * matching base-grid pressure.  Synchronises the stream */
int mgps_coupling_impulses(mgps_coupling *c, const float *x_dev, double *out_host, void *stream);
/* v_out_host = v_in_host + K (F, T)(x) per row ((bodies + 1) * 6: U then omega; row 0 is copied), the product formed on the host in
 * fp64 from the impulses; impulses_host (may be NULL) receives them.  Synchronises the stream */
int mgps_coupling_velocities(mgps_coupling *c, const float *x_dev, const double *v_in_host, double *v_out_host, double *impulses_host,
                             void *stream);
/* mgps_solve_pcg on (A + G K G^T) x = b with the coupling attached to the solver for the length of the call.  It runs the loop of
 * options.pcg_fp64_vectors = 1 whatever that option says: after t = A p, t += G K G^T p and <p, A p> gains g^T K g on the device; the
 * two true residuals lose G K G^T x (the coupled cells' float32 residual is narrowed again and |r|^2 corrected by the fp64 sum of
 * new^2 - old^2 over them); preconditioner, updates, interrupt and the iterate handed back are those of mgps_solve_pcg.  With K = 0
 * every coupling term is 0.0 and the iterates are those of mgps_solve_pcg under pcg_fp64_vectors = 1.
 * The coupled cells must be active cells of the solver (both made from the same material labels).
 * A slab solver takes the slab coupling of its own rank (mgps_coupling_create_slab: the same extents, owned expanded planes, rank and
 * size); the call is then a collective like mgps_solve_pcg on a slab solver, with one more all-reduce (g) per application of the
 * operator: iterations + 3 of them in a converged solve.  g^T K g enters the loop's <p, A p> on rank 0 alone and the residuals'
 * corrections rank by rank, both summed by the reduction the loop makes anyway.
 * Refused with a message, on the rank's own arguments and before any device work or collective (what is refused depends on what
 * the ranks share, so all refuse alike): a slab solver with a whole-grid coupling, a whole-grid solver with a slab coupling, a
 * window that is not the solver's, options.precision = 1, a solver with an enclosed component (options.enclosed_liquid: a moving body
 * changes the null space), a coupling whose expanded extents differ from the solver's.  A failing transport call: MGPS_ERR_COMM at
 * once.  The one-call on device fields is mgps_project_free_surface_rigid_slab below.  Coupling in the host-array entry
 * mgps_project_free_surface, in the default grouped fp32 loop and with enclosed_liquid: not yet. */
int mgps_solve_pcg_coupled(mgps_solver *h, mgps_coupling *coupling, float *x_dev, const float *b_dev, double tolerance,
                           int max_iterations, int use_mg_preconditioner, mgps_pcg_stats *stats);

/* The projection with rigid bodies the liquid moves, in one call on the DEVICE fields of one slab rank: a
 * collective over `comm` with the contract of mgps_project_free_surface_slab -- the same steps, plane exchanges, agreements,
 * no-liquid path, interrupt rule, surface tension and stage_ms -- around the parts above.  With comm->size = 1 it is the
 * device-resident coupled projection on one GPU and no transport entry is called.  What differs from the plain call:
 *   * the bodies' count travels in the first agreement (as a max and a min: a count that differs between the ranks is refused on
 *     every rank), with the rank's own failures -- a missing `body` grid, an allocation, a HIP error;
 *   * after the solver is built the rank makes its coupling (mgps_coupling_create_slab on its material labels, cut weights and
 *     `body`); one more agreement carries a failure of it and sums coupled_cells.  Then what mgps_solve_pcg_coupled refuses is
 *     asked, with that entry's message and on every rank alike: a solver with an enclosed component (options.enclosed_liquid = 1
 *     on a domain without one is accepted; options.precision = 1 is refused before, by the slab solver's constructor).  After
 *     either refusal pressure, velocity and solid_velocity_out hold what they held (valid_faces are written);
 *   * sv -- in solid_velocity_out when given, in buffers of the call otherwise -- is a copy of projection->solid_velocity (zeros when
 *     that is all NULL) with V* = `motions` written over the bodies' faces by mgps_fields_slab_rigid_velocity; the right-hand side
 *     is mgps_fields_slab_rhs with this sv;
 *   * the solve is mgps_solve_pcg_coupled (the loop of pcg_fp64_vectors = 1, whatever the option says); residual_inf and
 *     residual_l2 are norms of b - (A + G K G^T) x: mgps_coupling_apply into a zeroed grid, subtracted from mgps_residual's output;
 *   * mgps_coupling_velocities (a collective) gives motions_out and impulses, the same bits on every rank;
 *     mgps_fields_slab_rigid_velocity writes V_out over sv and the divergence report is taken against that sv, which
 *     solid_velocity_out publishes (both copies of a cut's z-face plane alike);
 *   * no liquid anywhere: the plain call's path with motions_out = motions, zero impulses and zero counts (solid_velocity_out, when
 *     given, holds sv of V*);
 *   * MGPS_ERR_INTERRUPTED publishes the iterate handed back as the plain call does; motions_out, impulses and solid_velocity_out
 *     are those of that iterate.
 * Refused before any collective, on what the ranks share: NULL or a struct_size mismatch of either struct, the transport checks of
 * the plain call, bodies outside 1 .. 255, a NULL table, a negative or non-finite inv_mass or diagonal entry of inv_inertia, NULL
 * motions or motions_out, solid_velocity_out partly set. */
typedef struct mgps_projection_rigid_slab {
    int struct_size;                  /* sizeof(mgps_projection_rigid_slab) */
    mgps_projection_slab *projection; /* fields, switches and results of the plain call (its struct_size is checked).  Its
                                         solid_velocity (or all NULL = 0) supplies the faces no body owns and is not written */
    int bodies;                       /* 1 .. 255 */
    const int32_t *body[3];           /* device, the window's face grids of body ids (as mgps_coupling_create_slab) */
    const double *centres, *inv_mass, *inv_inertia; /* host tables as in mgps_coupling_desc; the same on every rank */
    const double *motions;            /* host, (bodies + 1) * 6: V* = (U, omega) per row */
    float *solid_velocity_out[3];     /* device, window face grids, all three or none: the solid velocity the projected
                                         velocity is divergence free against (above) */
    double *motions_out;              /* host, (bodies + 1) * 6: V_out; required */
    double *impulses;                 /* host, (bodies + 1) * 6, or NULL */
    int64_t coupled_cells, coupled_cells_rank; /* results: the whole grid's count, this rank's */
} mgps_projection_rigid_slab;
int mgps_project_free_surface_rigid_slab(mgps_projection_rigid_slab *r, const mgps_options *opt, const mgps_comm *comm,
                                         const int *splits, void *stream);

/* ---- rigid bodies rasterised on the device: solid SDF, cut weights, body ids ------------------------------
 * The entries above take solid_phi, cut_weights and the body face grids from the caller; this pass writes them from a host table
 * of shapes and poses, for the sub-step after the bodies have moved.  No counterpart in the reference (Houdini hands it `collision`
 * and `cutCellWeights`); the definition here is the contract.
 *   Lengths are in cells from the grid's corner (section "pressure feedback"): node (i, j, k) at (i, j, k), a cell centre at + 1/2
 *   in every direction, the x-face (i, j, k) at (i, j + 1/2, k + 1/2).  All geometry is fp64 from the host tables, every output is
 *   rounded to float32 once; no atomics on values: the same inputs give the same bits on every run.
 *   x_b = R^T (x - centre) is the position in the body frame.  sdf_r(x):
 *     SPHERE  |x_b| - half[0];
 *     BOX     q = |x_b| - half, |max(q, 0)|_2 + min(max(q.x, q.y, q.z), 0);
 *     GRID    g = (x_b - origin) / spacing clamped per axis into [0, n - 1], i0 = min(floor(g), n - 2), f = g - i0, the samples
 *             interpolated along x, then y, then z as (1 - f) a + f b in fp64, plus the Euclidean distance from x_b to the sample
 *             box [origin, origin + (n - 1) spacing] (per axis max(lo - x_b, x_b - hi, 0)).
 *   The frame box of a body is [-radius, radius]^3, [-half, half] or the sample box; its reach box is the world AABB of the frame
 *   box (centre of the frame box carried to the world, +- |R| h) grown by `band` on every side, made in fp64 on the host.  At a point
 *   inside its reach box (bounds included) body r contributes min(sdf_r, band), outside it contributes band.
 *   Node field (internal): phi_n = min(band, min_r contribution_r(node)); owner_n = the lowest r that attains phi_n when
 *   phi_n < band, else 0.
 *   solid_phi[c] = min(static_solid_phi[c], float(min(band, min_r contribution_r(cell centre)))); static term +1e30f when NULL.
 *   w_b of a face: the open fraction from its four corner nodes' phi_n in cyclic order -- for axis a with in-plane axes u < v the
 *   corners (0,0), (1,0), (1,1), (0,1) in (u, v).  The polygon has, in that order, every corner with phi >= 0 and, on every edge
 *   a -> b whose ends differ in that test, the crossing at t = phi_a / (phi_a - phi_b); w_b is its shoelace area clamped into
 *   [0, 1] (two diagonal non-negative corners: one hexagon through the middle; exact for a planar SDF).  Then w_b < min_open
 *   becomes 0 and w_b > 1 - min_open becomes 1.
 *   cut_weights[a][f] = min(static_cut_weights[a][f], float(w_b)); static term 1 when the static grids are NULL.
 *   body[a][f] = owner of the corner with the smallest phi_n (ties: the first in cyclic order) when float(w_b) < 1.f, else 0:
 *   static solids land in row 0 of the sections above.
 * The static grids are inputs and never written; the outputs are separate arrays, all written everywhere. */
enum { MGPS_BODY_SPHERE = 0, MGPS_BODY_BOX = 1, MGPS_BODY_GRID = 2 };
typedef struct mgps_body_shape {
    int kind;            /* MGPS_BODY_SPHERE, MGPS_BODY_BOX, MGPS_BODY_GRID */
    double centre[3];    /* world position of the body frame's origin, cells */
    double rotation[9];  /* row-major, body -> world, orthonormal */
    double half[3];      /* BOX: half extents; SPHERE: half[0] = radius */
    const float *sdf;    /* GRID: device array, x fastest, negative inside, cells */
    int nx, ny, nz;      /* GRID: samples, each >= 2 */
    double origin[3];    /* GRID: body-frame position of sample (0,0,0) */
    double spacing;      /* GRID: cells, > 0 */
} mgps_body_shape;
typedef struct mgps_raster_desc {
    int struct_size;                     /* sizeof(mgps_raster_desc) */
    int gx, gy, gz;                      /* whole grid */
    int bodies;                          /* 1 .. 255 */
    const mgps_body_shape *shapes;       /* host, bodies + 1 rows; row 0 is not read */
    double band, min_open;               /* 2 <= band <= 16 cells; 0 <= min_open < 0.5 */
    const float *static_solid_phi;       /* device cell grid, or NULL */
    const float *static_cut_weights[3];  /* device face grids: all three, or all NULL */
    float *solid_phi;                    /* out, device cell grid */
    float *cut_weights[3];               /* out, device face grids */
    int32_t *body[3];                    /* out, device face grids */
} mgps_raster_desc;
/* One launch over tiles of 64 x 4 x 4 cells; the shape rows and reach boxes are uploaded per call.  Does not synchronise the
 * stream; the host table may be reused once the call returns.  Refuses with a message, before any device work: NULL desc or a
 * struct_size mismatch, a non-positive extent (or more than 262140 cells along y or z: launch-grid dimensions), bodies outside
 * 1 .. 255, NULL shapes, an unknown kind, a non-finite centre or rotation, |R^T R - I|_inf > 1e-6, a radius or half extent that is
 * not positive and finite, a GRID body with NULL sdf, a dimension < 2, a spacing that is not positive and finite or a non-finite
 * origin, band or min_open out of range, a NULL output, static weights only partly given. */
int mgps_fields_rasterize_bodies(const mgps_raster_desc *d, void *stream);
/* The same on a slab window, without halo and without communication: the arrays are the window's (z-face grids: the faces
 * c0 .. c1), positions use the plane index of the whole grid, the bits are those of the whole-grid pass on the rank's planes and
 * both copies of a cut's z-face plane come out alike.  Refuses also: not a slab window, or not one of the desc's extents. */
int mgps_fields_slab_rasterize_bodies(const mgps_fields_slab *w, const mgps_raster_desc *d, void *stream);

/* ---- triangle-mesh rigid bodies: signed distance sampled on the device, mass properties --------------------
 * A closed triangle mesh, given in the body frame, becomes the float32 samples a MGPS_BODY_GRID body reads; its volume, centre of
 * mass and inertia tensor give the inv_mass and inv_inertia rows of the coupling sections.  No counterpart in the reference; the
 * definition here is the contract.
 *   Sample (i, j, k) sits at s = origin + spacing (i, j, k): one product and one sum per axis, each rounded.  All geometry is fp64,
 *   the output is rounded to float32 once.
 *   d(s) = the minimum over all triangles of the exact Euclidean distance from s to the triangle (the closest point may lie on the
 *   face, an edge or a vertex).   sdf[s] = float(sigma(s) min(d(s), band)), sigma = -1 inside, +1 outside: |sdf| is exact up to band
 *   and clamped there.
 *   Inside or outside is the parity of the crossings along +x of the column (y + eps, z + eps^2), eps -> 0+.  For a projected edge
 *   a -> b: e = (b.y - a.y)(s.z - a.z) - (b.z - a.z)(s.y - a.y), every difference, both products and their difference rounded in
 *   that order, evaluated with the ends in ascending vertex index and negated when that swaps them, so both triangles on an edge see
 *   the same number.  The sign of e is the sign of the first non-zero term of (e, -(b.z - a.z), b.y - a.y), with a and b the ends as
 *   evaluated (negated with e).  A triangle is crossed when its three signs agree; one of zero projected area -- (b.y - a.y)(c.z -
 *   a.z) - (b.z - a.z)(c.y - a.y) == 0 -- or with e_a + e_b + e_c == 0 never is.  The crossing's depth is x_c = (e_a x_a + e_b x_b +
 *   e_c x_c) / (e_a + e_b + e_c), each e the edge function of the edge opposite its vertex, summed left to right.  s is inside when
 *   the number of crossed triangles with x_c > s.x is odd.  (The shift makes the parity right on a closed mesh when a column runs
 *   exactly through an edge or a vertex; "zero counts as positive" does not.)
 *   The result is a function of the mesh as a set: a triangle is first turned so that its lowest vertex index comes first, minimum
 *   and parity do not depend on the triangles' order, and nothing is summed across triangles: the same mesh gives the same bits in
 *   any triangle order, under any cyclic turn of a triangle's vertices, on every run.
 *   Band and the rasteriser: a GRID body's trilinear interpolation sees the clamp.  For a rasteriser band of B cells the samples must
 *   be exact over B plus one sample cell's diagonal: band >= B + sqrt(3) spacing, in a box that holds the mesh's bounding box grown
 *   by band + spacing, which is what the sample-box entry below returns.
 *   Slab ranks: nothing to add.  The samples live in the body frame: every rank makes its own copy from the same mesh, with no
 *   message, and gets the same bits.
 * Limits: closed, consistently oriented, manifold-edged meshes only (several shells are fine, an inward-oriented shell inside
 * another is a cavity); no open surfaces, no capsules.  (A deforming mesh's vertex velocities: the section after this one.) */
typedef struct mgps_mesh_desc {
    int struct_size;           /* sizeof(mgps_mesh_desc) */
    int vertices, triangles;   /* counts, each >= 4 */
    const double *xyz;         /* host, vertices * 3, body frame, cells */
    const int32_t *tri;        /* host, triangles * 3, vertex indices, outward orientation (counter-clockwise seen from outside) */
    int nx, ny, nz;            /* samples, each 2 .. 1024 */
    double origin[3], spacing; /* as mgps_body_shape's GRID fields */
    double band;               /* body-frame cells, > 0 */
    float *sdf;                /* out, device, nz * ny * nx, x fastest, negative inside */
} mgps_mesh_desc;
/* The mesh is uploaded per call from the host tables with the lists that bin its triangles (the tiles of 64 x 4 x 4 samples a
 * triangle's box grown by band touches, the tiles of 16 x 16 columns its y-z projection touches), then three launches: list fill,
 * parity bits, distance with sign and clamp.  Does not synchronise the stream; the host tables may be reused once the call returns.
 * Refuses with a message, before any device work: NULL desc or a struct_size mismatch, a NULL output, a dimension outside
 * 2 .. 1024, a spacing or band that is not positive and finite, a non-finite origin, and of the mesh: fewer than 4 vertices or
 * triangles, NULL tables, a non-finite coordinate, an index out of range, a triangle with a repeated index or of zero area in fp64,
 * a mesh that is not closed and consistently oriented (every directed edge must occur exactly once and its reverse exactly once:
 * the message names the first edge that does not), a signed volume that is not positive (inward orientation); lists of more than
 * 2^31 - 1 entries. */
int mgps_fields_mesh_sdf(const mgps_mesh_desc *d, void *stream);

/* Volume, centre of mass and inertia tensor about the centre of mass (row-major, symmetric) for unit density, in the body frame, in
 * cells: fp64 sums of the signed tetrahedra's polynomial integrals over the triangles, taken about the middle of the bounding box.
 * The caller multiplies volume and inertia by the density; a body's world-frame inverse inertia is R I^-1 R^T.  Host only, no
 * device call.  Refuses a NULL out and the mesh faults above. */
typedef struct mgps_mass_properties { double volume, centre[3], inertia[9]; } mgps_mass_properties;
int mgps_mesh_mass_properties(int vertices, int triangles, const double *xyz, const int32_t *tri, mgps_mass_properties *out);
/* The sample box of a mesh: out_origin = the bounding box's lower corner - (band + spacing), out_n (x, y, z) the least counts
 * (>= 2) whose last sample reaches the upper corner + (band + spacing).  Host only.  Refuses NULL pointers, no vertices, a non-finite
 * coordinate, a spacing or band that is not positive and finite, a box of more than 1024 samples along an axis. */
int mgps_mesh_sample_box(int vertices, const double *xyz, double spacing, double band, int out_n[3], double out_origin[3]);

/* ---- deforming mesh colliders: vertex velocities to the solid-velocity grids --------------------------------
 * An animated, deforming closed mesh is a scripted solid whose surface moves with per-vertex velocities.  Two device passes, split
 * as the two sections above are: mesh -> body-frame velocity samples beside the SDF samples, then samples -> the three
 * solid-velocity face grids.  No counterpart in the reference; the definition here is the contract.
 *   Samples.  For a sample s (section 19's positions) and a turned triangle T = (a, b, c), d2_T(s) is section 19's squared distance,
 *   formed by the distance pass's own expressions, so min_T d2_T is the number whose root the SDF stores.  The closest point's
 *   weights (wa, wb, wc) come from the same region tests in the same order, with d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp,
 *   d5 = ab.cp, d6 = ac.cp:
 *     vertex a (1, 0, 0); vertex b (0, 1, 0); edge ab (1 - v, v, 0), v = d1 / (d1 - d3); vertex c (0, 0, 1);
 *     edge ac (1 - w, 0, w), w = d2 / (d2 - d6); edge bc (0, 1 - w, w), w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
 *     face: va = d3 d6 - d5 d4, vb = d5 d2 - d1 d6, vc = d1 d4 - d3 d2, den = (va + vb) + vc, wb = vb / den, wc = vc / den,
 *     wa = (1 - wb) - wc.
 *   The winner is the triangle with the least (d2, v0, v1, v2) in lexicographic order, v the turned index triple: a strict order on
 *   the mesh as a set, so the triangles' order and their cyclic turns change no bit.
 *   vel[c][s] = float((wa V_a,c + wb V_b,c) + wc V_c,c) of the winner, in fp64 and rounded once, where d(s) < band; where
 *   !(d(s) < band) all three components are 0 (the SDF is clamped there and the tile's list no longer holds every triangle).
 *   sdf, when given, holds the bits mgps_fields_mesh_sdf writes for the same mesh and box.
 *   Face grids.  For a face f of axis a with r = body[a][f] in 1 .. bodies and velocities[r].vel set: x_f as in
 *   mgps_fields_rigid_velocity, x_b = R^T (x_f - centre_r) as in the rasteriser, g, i0 and f exactly section 18's GRID rule (clamped
 *   into the sample box, with no out-of-box term), u_c the trilinear interpolant of vel[c] taken along x, then y, then z as
 *   (1 - t) p + t q in fp64, and
 *     sv_a[f] = float(((R_a0 u_0 + R_a1 u_1) + R_a2 u_2) + (U + omega x (x_f - centre_r))_a),
 *   (U, omega) = velocities[r].motion, the motion of the body frame.  Every other face keeps its bits: row 0, ids out of range and
 *   bodies without samples are untouched, so a caller writes mgps_fields_rigid_velocity first and this pass after it.
 *   How it composes: deforming colliders are scripted solids.  Give them the highest ids in the rasteriser's table, pass the coupled
 *   entries (mgps_coupling_create, the rigid one-calls on one device and on slab ranks) the count of RIGID bodies only and this sv as
 *   their solid_velocity: the deforming bodies' faces then fall into row 0 ("walls and scripted solids, the caller's"), keep the
 *   sampled values and enter the right-hand side through mgps_fields_rhs.  Nothing in those entries changes.
 * Limits: vertex velocities are given, not differenced from two poses; one-way only (the liquid does not deform the collider); the
 * samples' band limits how far from the surface a face may lie (as for the SDF: band >= B + sqrt(3) spacing). */
typedef struct mgps_mesh_velocity_desc {
    int struct_size;           /* sizeof(mgps_mesh_velocity_desc) */
    int vertices, triangles;   /* as mgps_mesh_desc, down to sdf */
    const double *xyz;
    const int32_t *tri;
    int nx, ny, nz;
    double origin[3], spacing;
    double band;
    float *sdf;                /* out, device, or NULL: not written */
    const double *velocity;    /* host, vertices * 3, body frame, cells per step */
    float *vel[3];             /* out, device, each nz * ny * nx, x fastest: the (x, y, z) components in the body frame */
} mgps_mesh_velocity_desc;
/* One host pass (check, turn, bin, upload: mgps_fields_mesh_sdf's, with the vertex velocities in the same copy), the list fill and
 * the parity bits unchanged, and a third launch that walks the lists as the distance pass does and also carries the winner: per
 * sample d2 and the winner's table row stay in registers, the index triples are read only on an equal d2, and after the walk the
 * thread classifies the closest point once for the weights, gathers the three vertex velocities and stores.  No atomics on values.
 * Does not synchronise the stream.  Refuses with a message, before any device work: whatever mgps_fields_mesh_sdf refuses (but a
 * NULL sdf), a NULL velocity or a NULL vel[], a non-finite vertex velocity. */
int mgps_fields_mesh_sdf_velocity(const mgps_mesh_velocity_desc *d, void *stream);

typedef struct mgps_body_velocity {
    const float *vel[3];   /* device samples of a GRID body, all three, or all NULL: this body's faces are not written */
    double motion[6];      /* (U, omega) of the body frame, world frame, about the shape's centre */
} mgps_body_velocity;
/* The samples on the face grids (the rule above).  sv and body: the three face grids; shapes and velocities: host, bodies + 1 rows,
 * row 0 is not read; the samples of body r lie on the sample box of shapes[r].  One launch over the three axes: the ids are read
 * once, with a store only where a sampled body owns the face; the rows are uploaded per call.  Does not synchronise the stream.
 * Refuses with a message, before any device work: everything mgps_fields_rasterize_bodies refuses of a shape row, a body with
 * samples whose kind is not GRID, a partly set vel, a non-finite motion of a body with samples, a NULL grid or table, a non-positive
 * extent (or more than 262140 cells along y or z), bodies outside 1 .. 255. */
int mgps_fields_sampled_velocity(float *const sv[3], const int32_t *const body[3], int bodies, const mgps_body_shape *shapes,
                                 const mgps_body_velocity *velocities, int gx, int gy, int gz, void *stream);
/* The same on a slab window, without halo and without communication: the grids are the window's (z-face grids: the faces c0 .. c1),
 * positions use the plane index of the whole grid, the bits are those of the whole-grid pass on the rank's planes and both copies
 * of a cut's z-face plane come out alike.  Refuses also: not a slab window. */
int mgps_fields_slab_sampled_velocity(const mgps_fields_slab *w, float *const sv[3], const int32_t *const body[3], int bodies,
                                      const mgps_body_shape *shapes, const mgps_body_velocity *velocities, void *stream);

/* ---- advection: semi-Lagrangian and MacCormack field passes ------------------------------------------------
 * The step the extrapolated velocity is for: the three face grids of the velocity (self-advection) and up to four cell grids
 * (liquid_phi is the first user) carried along `velocity_in`, out of place, on the device.  With it a level-set liquid step is
 * made of this header's calls only: advect, add forces, rasterise, project, extrapolate.  No counterpart in the reference, where
 * Houdini advects; the definition here is the contract.
 *   Lengths are in cells: cell (i, j, k) has its centre at (i + 1/2, j + 1/2, k + 1/2), the x-face (i, j, k) lies at
 *   (i, j + 1/2, k + 1/2), the y- and z-faces alike.  dt is the time step over the cell size, so dt u is a displacement in cells
 *   (section 17's convention).
 *   Sampling.  A grid with n_c nodes along c whose node (0, 0, 0) lies at o -- o = (1/2, 1/2, 1/2) for cells, (0, 1/2, 1/2) for
 *   x-faces, and so on -- is sampled at a point p per axis with g = p - o, g' = clamp(g, 0, n_c - 1), i0 = min(int(floor(g')), n_c - 1),
 *   i1 = min(i0 + 1, n_c - 1), t = g' - i0; S(q, p) combines the eight values along x, then y, then z as (1 - t) a + t b in fp64
 *   (section 20's interpolant; the product t b and the sum are one fused multiply-add).  S is continuous in p; an extent of one
 *   node is allowed.  U(p) = (S(vx, p), S(vy, p), S(vz, p)) of velocity_in.
 *   Trace.  B = [0, gx] x [0, gy] x [0, gz]; clampB clamps a point into it per component.  trace_order = 1:
 *   p_dep = clampB(x - dt U(x)).  trace_order = 2, the midpoint rule and the default of the Python layer:
 *   p1 = clampB(x - (dt / 2) U(x)), p_dep = clampB(x - dt U(p1)).  The velocity traced with is always velocity_in.
 *   Targets: every cell of every scalar grid and every face of the three face grids.
 *   scheme = 0, semi-Lagrangian: out[x] = float(S(q_in, p_dep(x))), fp64 rounded once.
 *   scheme = 1, MacCormack (Selle et al. 2008): qh = the semi-Lagrangian result of all grids (float32, in the scratch grids);
 *   qt[x] = S(qh, p_fwd(x)) with p_fwd the same trace under -dt; m = qh[x] + (q_in[x] - qt[x]) / 2 in fp64;
 *   out[x] = float(clamp(m, lo, hi)), lo and hi the least and the greatest of the eight q_in values S read at p_dep(x).  With zero
 *   velocity out equals in bit for bit.
 *   Buffers.  Out of place: an array the call writes (out, and scratch under MacCormack) overlaps no other array of the call;
 *   pointer ranges are compared and an overlap is refused.  MacCormack needs caller-supplied scratch grids of the outputs' shapes
 *   for qh; its second launch forms p_dep again with the first launch's expressions instead of storing it.  No atomics on values,
 *   every target is written by its own thread: the same inputs give the same bits on every run.
 *   counts_dev (device, unsigned long long[2], may be NULL) is ADDED to, as filled_dev is (initialise it): [0] the targets for
 *   which a clampB moved a coordinate of p1 or p_dep, [1] the window form's missed planes (below).  A cell counts once per scalar grid.
 * Limits: solids are not consulted -- a departure point inside a solid reads what is there; the caller extrapolates at least
 * ceil(max |dt u|) + 2 layers first (mgps_fields_extrapolate3); transport does not keep |grad phi| = 1 (mgps_fields_redistance,
 * below, restores it); float32 grids only. */
typedef struct mgps_advect_desc {
    int struct_size;             /* sizeof(mgps_advect_desc) */
    int gx, gy, gz;              /* the WHOLE simulation grid */
    double dt;                   /* time step over cell size; finite */
    int scheme;                  /* 0 semi-Lagrangian, 1 MacCormack */
    int trace_order;             /* 1 or 2 */
    const float *velocity_in[3]; /* device face grids: the velocity traced with, and the one advected */
    float *velocity_out[3];      /* all three, or all NULL: scalars only */
    float *velocity_scratch[3];  /* scheme = 1: face grids for qh; not read otherwise */
    int scalars;                 /* 0 .. 4 */
    const float *scalar_in[4];   /* device cell grids */
    float *scalar_out[4];
    float *scalar_scratch[4];    /* scheme = 1 */
    unsigned long long *counts_dev;
} mgps_advect_desc;
/* One launch over tiles of 64 x 4 x 4 cells for scheme = 0, two for scheme = 1.  Does not synchronise the stream.  Refuses with a
 * message, before any device work: NULL desc or a struct_size mismatch, an extent < 1 (or more than 262140 cells along y or z), a
 * scheme or trace_order out of range, a non-finite dt, scalars outside 0 .. 4, velocity_out partly set, nothing to advect
 * (velocity_out NULL and scalars = 0), a NULL velocity_in / scalar_in / scalar_out of a grid in use, a NULL scratch under
 * MacCormack, overlapping buffers. */
int mgps_fields_advect(const mgps_advect_desc *d, void *stream);
/* The pass on a slab window, without communication.  The arrays in `d` are the window's, in section 14's shapes (z-face grids: the
 * faces c0 .. c1); d->gx, gy, gz are the whole grid's.  velocity_lo / scalar_lo hold the min(halo, c0) planes below the window,
 * contiguous and ascending, velocity_hi / scalar_hi the min(halo, gz - c1) planes above it; for the z-face grid these are the face
 * planes below c0 and above c1.  They are not read (may be NULL) where that count is 0.  Positions use the whole grid's plane
 * index: the window's bits are the whole grid's, and both copies of a cut's z-face plane come out alike.  A sample whose i0 or i1
 * along z is a plane inside the grid but outside window plus halo reads the nearest plane held instead, and its target is counted
 * in counts_dev[1]: the caller's test for "halo too small" is counts[1] != 0.  Of the z-face targets the planes c0 .. c1 - 1 count,
 * on the last rank also plane gz (filled_dev's rule): a sum over the ranks counts every target once.  The whole grid is the window
 * [0, gz) with no halo.
 * MacCormack on a window needs qh on the halo planes too: the window form takes scheme = 0 only and refuses scheme = 1 with a
 * message.  The collective that exchanges the halos and qh is not part of this header yet.
 * Refuses also: not a slab window, a window of other extents than the desc's, a negative halo, a NULL halo array where planes are
 * held. */
int mgps_fields_slab_advect(const mgps_fields_slab *w, const mgps_advect_desc *d, int halo, const float *const velocity_lo[3],
                            const float *const velocity_hi[3], const float *const scalar_lo[4], const float *const scalar_hi[4],
                            void *stream);

/* ---- redistancing: a fast iterative Eikonal pass -------------------------------------------------------------
 * Transport does not keep |grad phi| = 1; this pass turns liquid_phi back into a signed distance within `band` cells of the surface,
 * deterministically, out of place, on the device.  No counterpart in the reference; the definition here is the contract, and
 * tests/redistance_reference.py restates it in numpy operation by operation.
 *   Lengths are in cells; dx is the cell size in phi's units; band > 0 is in cells, B = (double)(float)band.  Inside means
 *   phi <= 0 (mgps_fields_material_labels' rule: a redistanced phi labels exactly as its input does).
 *   State.  The state of a cell is the float32 value s T: T >= 0 the distance in cells, s = - inside and + outside; an inside cell
 *   with T = 0 is -0.0f.  All arithmetic is fp64 on float32 data and EVERY operation is rounded on its own (no contraction into
 *   fused multiply-adds); a value is rounded to float32 where it is stored.
 *   Interface cells: a cell x with an in-grid 6-neighbour of the other sign.  They are fixed by the initial pass and never
 *   updated: d_cross = min over those neighbours n of phi_x / (phi_x - phi_n), in [0, 1]; g_c = (phi_+ - phi_-) / 2 where both
 *   neighbours along c exist, else the one-sided difference, else 0; d_grad = |phi_x| / sqrt((g_x^2 + g_y^2) + g_z^2) where that sum
 *   is > 0, else +inf; T0 = float(min(d_grad, d_cross, B)).  Every other cell starts at T0 = float(B).
 *   Update G, of cells that are no interface cells: a_c = the least T of the two neighbours along c, a neighbour outside the whole
 *   grid counting as +inf; sorted a1 <= a2 <= a3; t = a1 + 1; if t > a2: d = a1 - a2, t = 0.5 ((a1 + a2) + sqrt(2 - d d)); if
 *   t > a3: s = (a1 + a2) + a3, q = (a1 a1 + a2 a2) + a3 a3, disc = max(s s - 3 (q - 1), 0), t = (s + sqrt(disc)) / 3;
 *   T_new = min(T_old, float(min(t, B))).  (First-order Godunov; T only falls, and never below an interface cell's.)
 *   A round is block Jacobi on tiles of 64 x 4 x 4 cells anchored at cell (0, 0, 0) of the WHOLE grid: a tile takes its cells and
 *   a one-cell rim from the round's input, runs `inner` (1 .. 8) Jacobi iterations of G on its own cells with the rim held, and
 *   writes its cells.  inner = 1 is plain Jacobi and does not depend on the tiling.  The fixpoint does not depend on inner.
 *   Result.  After `rounds` rounds out = float(dx state); cells the front never reached hold +-B dx.
 *   counts_dev (device, unsigned long long[2], may be NULL) is ADDED to: [0] the interface cells, [1] the cells whose value the
 *   LAST round changed: the caller's test for "enough rounds" is counts[1] == 0.
 *   No atomics on values, every cell is written by its own thread: the same inputs give the same bits on every run.
 * Limits: solids are not consulted; first order; float32 grids only; the slab collective (the state's halo exchange per round) is
 * not part of this header yet. */
typedef struct mgps_redistance_desc {
    int struct_size;      /* sizeof(mgps_redistance_desc) */
    int gx, gy, gz;       /* the WHOLE simulation grid */
    double band, dx;      /* finite, > 0 */
    int rounds, inner;    /* rounds >= 0, inner 1 .. 8 */
    const float *phi_in;  /* device cell grids */
    float *phi_out;
    float *scratch;       /* of phi_out's shape; may be NULL when rounds == 0, not read by the window entries */
    unsigned long long *counts_dev;
} mgps_redistance_desc;
/* One initial launch and `rounds` launches that ping-pong between phi_out and scratch so that the last one writes phi_out.  Does
 * not synchronise the stream.  Out of place: phi_out and scratch overlap no other array of the call; pointer ranges are compared.
 * Refuses with a message, before any device work: NULL desc or a struct_size mismatch, an extent < 1 (or more than 262136 cells
 * along y or z), a band or dx that is not finite and > 0, rounds < 0, inner outside 1 .. 8, a NULL array that is in use,
 * overlapping buffers. */
int mgps_fields_redistance(const mgps_redistance_desc *d, void *stream);
/* The pass on a slab window, launch by launch and without communication.  The arrays in `d` are the window's planes c0 .. c1 - 1;
 * d->gx, gy, gz are the whole grid's; d->rounds and d->scratch are not read.  *_lo holds the min(halo, c0) planes below the window,
 * contiguous and ascending, *_hi the min(halo, gz - c1) planes above it (not read, may be NULL, where that count is 0).  Positions
 * and the tiles' anchor are the whole grid's: the window's bits are the whole grid's.
 * _init reads phi from phi_in and writes the state, unscaled, to phi_out; it reads one plane either way and adds the own planes'
 * interface cells to counts_dev[0].  _round reads a state from phi_in and writes phi_out; with `last` set it multiplies its stores
 * by dx and adds the own cells it changed to counts_dev[1], so the ranks' counts add up to the whole grid's.  A rank computes every
 * whole-grid tile that meets its window from window plus halo and writes its own planes: a round reads the planes
 * 4 floor(c0 / 4) - 1 .. 4 ceil(c1 / 4), clipped to the grid (inner = 1: c0 - 1 .. c1).  Four planes either way always suffice.
 * Fewer planes than that is refused, not counted.  The whole grid is the window [0, gz) without halo; one kernel serves both forms.
 * Refuses also: not a slab window, a window of other extents than the desc's, a negative halo, a NULL halo array where planes are
 * held, too few halo planes. */
int mgps_fields_slab_redistance_init(const mgps_fields_slab *w, const mgps_redistance_desc *d, int halo, const float *phi_lo,
                                     const float *phi_hi, void *stream);
int mgps_fields_slab_redistance_round(const mgps_fields_slab *w, const mgps_redistance_desc *d, int halo, const float *state_lo,
                                      const float *state_hi, int last, void *stream);

/* ---- FLIP particles: bin, particles -> grid, grid -> particles and move ------------------------------------------
 * A FLIP liquid's mass is its particles, so it does not lose volume as an advected level set does.  With these three calls a
 * FLIP/PIC sub-step is made of this header's calls only: bin, particles -> grid, extrapolate, (add forces), project, extrapolate,
 * grid -> particles and move.  No counterpart in the reference, where Houdini owns the particles; the definition here is the
 * contract, and tests/particles_reference.py restates it in numpy operation by operation.
 *   Conventions (those of advection, above).  Lengths are in cells; the box is B = [0, gx] x [0, gy] x [0, gz]; cell (i, j, k) has
 *   its centre at (i + 1/2, j + 1/2, k + 1/2), the x-face (i, j, k) lies at (i, j + 1/2, k + 1/2), the y- and z-faces alike; dt is
 *   the time step over the cell size.  A particle set is structure-of-arrays on the device: three float32 position arrays and three
 *   float32 velocity arrays of n entries each, 0 <= n < 2^31.  A particle is INSIDE if 0 <= x_c <= g_c for all three components
 *   (false for NaN); its cell is i_c = min(int(floor(x_c)), g_c - 1), exactly -- no arithmetic precedes the floor.  Every other
 *   particle is OUTSIDE: it takes part in nothing and is carried through unchanged.  gx gy gz + 1 must be < 2^31.
 *
 * 1. mgps_particles_bin: particles in cell order, out of place.
 *   order (int32[n]): the input index of sorted slot s.  cell_start (int32[cells + 2], cells = gx gy gz): entry c is the first slot of
 *   cell c in the linear order (k gy + j) gx + i, entry `cells` the first slot of the outside bin, entry cells + 1 is n.  The
 *   position arrays, and the velocity arrays unless velocity_out is all NULL (velocity_in is then not read), gathered into that
 *   order.  Within a cell slots ascend by input index (a stable sort): the result is a function of the inputs alone.
 *   counts_dev (device, unsigned long long[2], may be NULL) is ADDED to: [0] outside particles, [1] occupied cells.
 *   A key kernel, rocprim::radix_sort_pairs over exactly the bits cells + 1 needs, a lower-bound kernel and one gather kernel, in
 *   stream order with temporary storage from the stream's pool: no host synchronisation. */
typedef struct mgps_particles_bin_desc {
    int struct_size;               /* sizeof(mgps_particles_bin_desc) */
    int gx, gy, gz;                /* the WHOLE simulation grid */
    int n;                         /* particles, >= 0 */
    const float *position_in[3];   /* device, n entries each; not read (may be NULL) when n == 0 */
    const float *velocity_in[3];   /* not read when velocity_out is all NULL */
    float *position_out[3];
    float *velocity_out[3];        /* all three, or all NULL */
    int32_t *order;                /* n entries */
    int32_t *cell_start;           /* cells + 2 entries */
    unsigned long long *counts_dev;
} mgps_particles_bin_desc;
/* Does not synchronise the stream.  Refuses with a message, before any device work: NULL desc or a struct_size mismatch, an
 * extent < 1, gx gy gz + 1 >= 2^31, n < 0, a NULL array that is in use, velocity_out partly set, overlapping buffers (every output
 * overlaps no other array of the call). */
int mgps_particles_bin(const mgps_particles_bin_desc *d, void *stream);

/* 2. mgps_particles_to_grid: velocity, weights, known faces and liquid_phi from BINNED particles (position, velocity and cell_start
 * as mgps_particles_bin left them).
 *   All arithmetic is fp64 on float32 data and EVERY operation is rounded on its own (no contraction into fused multiply-adds); a
 *   value is rounded to float32 once, where it is stored.
 *   Hat function h(d) = max(0, 1 - |d|).  The weight of particle p at a node x: w = (h(x_p,x - x_x) h(x_p,y - x_y)) h(x_p,z - x_z).
 *   Face of axis a: num = sum w v_p,a and den = sum w, each step `num = num + w * v` and `den = den + w`, over the particles of the
 *   cells that can reach the face: for the x-face (i, j, k) the cells i - 1 .. i along x and j - 1 .. j + 1, k - 1 .. k + 1 along
 *   the other axes, the y- and z-faces alike; cells outside the grid hold nothing.  The order is ascending k, then j, then i, then
 *   slot; particles of weight 0 are included.  velocity_out = float(num / den) where den > 0, else 0; weight_out = float(den) (all
 *   three, or all NULL); known_out (uint8) = den > 0 -- the `valid` input of mgps_fields_extrapolate3.
 *   Cell centre c: m = the least (dx^2 + dy^2) + dz^2 over the particles of the 3 x 3 x 3 cells around c, +inf with none;
 *   liquid_phi_out = float(dx (min(sqrt(m), 1.5) - radius)) (may be NULL).  A particle outside those 27 cells is at least 1.5 cells
 *   from the centre, so the clamp makes the 27-cell minimum exact.  0 < radius <= 1.5; dx finite and > 0.  The result is a union
 *   of spheres, not a distance: mgps_fields_redistance makes it one.
 *   counts_dev (device, unsigned long long[2], may be NULL) is ADDED to: [0] known faces, [1] cells with phi <= 0 (counted whether
 *   or not liquid_phi_out is given).
 *   Determinism.  No floating-point atomics; every target is written by its own thread, which gathers its sources in the stated
 *   order: the same inputs give the same bits.  Safety.  Device data cannot be refused: every slot range taken from cell_start is
 *   clamped into [0, n], so a wrong cell_start gives wrong values, never an out-of-range read. */
typedef struct mgps_particles_to_grid_desc {
    int struct_size;            /* sizeof(mgps_particles_to_grid_desc) */
    int gx, gy, gz;             /* the WHOLE simulation grid */
    int n;                      /* particles, >= 0 */
    int form;                   /* the kernel: 0 the default, 1 the plain gather, 2 the staged march; all give the same bits */
    double radius, dx;          /* radius in cells, 0 < radius <= 1.5; dx the cell size in phi's units, finite and > 0 */
    const float *position[3];   /* binned; not read (may be NULL) when n == 0 */
    const float *velocity[3];
    const int32_t *cell_start;  /* cells + 2 entries */
    float *velocity_out[3];     /* device face grids */
    float *weight_out[3];       /* all three, or all NULL */
    uint8_t *known_out[3];
    float *liquid_phi_out;      /* device cell grid, may be NULL */
    unsigned long long *counts_dev;
} mgps_particles_to_grid_desc;
/* One launch over tiles of 64 x 4 x 4 cells; a thread owns its cell's phi, its three backward faces and the forward faces where the
 * grid ends.  form = 2 (and 0, the default) marches the source planes of a tile upward and takes each row's particles -- binned, so
 * one run of slots -- through LDS in chunks of 768; form = 1 gathers every target's 27 cells from global memory.  Both visit a
 * target's sources in the stated order and give the same bits (DESIGN.md section 23 has the times).  Tiles whose 6 x 6 x 66 cells
 * hold no particle stream zeros and phi = dx (1.5 - radius) through.  Does not synchronise the stream.  Refuses with a message,
 * before any device work: NULL desc or a struct_size mismatch, an extent < 1 (or more than 262140 cells along y or z),
 * gx gy gz + 1 >= 2^31, n < 0, a form outside 0 .. 2, a radius outside (0, 1.5], a dx that is not finite and > 0, a NULL array that is
 * in use, weight_out partly set, overlapping buffers. */
int mgps_particles_to_grid(const mgps_particles_to_grid_desc *d, void *stream);

/* 3. mgps_particles_update: grid -> particles, then move; one thread per particle in one launch.
 *   Per inside particle, with S and U advection's sampling rule (above), its explicit fused multiply-adds included, of grid_new
 *   (the projected, extrapolated velocity) and grid_old (the particles -> grid result before forces and projection):
 *   pic = U_new(x), old = U_old(x) (with grid_old all NULL, allowed only when flip = 0: old = pic);
 *   v_out,a = float((1 - flip) pic_a + flip (double(v_a) + (pic_a - old_a))), each operation rounded on its own: flip = 0 gives
 *   float(pic) exactly, flip = 1 with grid_old being grid_new gives v back bit for bit.
 *   Position: advection's trace with -dt in grid_new.  trace_order = 1: x_out = float(clampB(x + dt pic)); trace_order = 2:
 *   p1 = clampB(x + (dt / 2) pic), x_out = float(clampB(x + dt U_new(p1))); the product and the sum are one fused multiply-add, as
 *   in the trace of advection.  dt = 0 leaves positions bit-equal; an inside particle stays inside.
 *   Outside particles are copied through.
 *   counts_dev (device, unsigned long long[2], may be NULL) is ADDED to: [0] particles for which a clampB moved a coordinate (of p1
 *   or of the end point), [1] outside particles.
 *   Buffers.  Each output array is either exactly its input array (in place is safe: one thread per particle) or overlaps no
 *   other array of the call; a partial overlap is refused.
 * Out of scope, for all the particle entries: slab windows and particle migration between ranks; APIC / affine transfers; wiring
 * into the one-calls; continuous collision (entries 4 and 5 test a particle where it is and do not trace its path: a particle that a
 * step carries across a solid thinner than the step is not found); seeding near the surface (entry 6 seeds no cell shallower than
 * seed_depth). */
typedef struct mgps_particles_update_desc {
    int struct_size;              /* sizeof(mgps_particles_update_desc) */
    int gx, gy, gz;               /* the WHOLE simulation grid */
    int n;                        /* particles, >= 0 */
    int trace_order;              /* 1 or 2 */
    double dt;                    /* time step over cell size; finite */
    double flip;                  /* in [0, 1]: 0 is PIC, 1 is FLIP */
    const float *position_in[3];  /* device, n entries each; not read (may be NULL) when n == 0 */
    const float *velocity_in[3];
    float *position_out[3];
    float *velocity_out[3];
    const float *grid_new[3];     /* device face grids */
    const float *grid_old[3];     /* all three, or all NULL (flip = 0 only) */
    unsigned long long *counts_dev;
} mgps_particles_update_desc;
/* Does not synchronise the stream.  Refuses with a message, before any device work: NULL desc or a struct_size mismatch, an
 * extent < 1, gx gy gz + 1 >= 2^31, n < 0, a trace_order that is neither 1 nor 2, a non-finite dt, a flip outside [0, 1], a NULL
 * array that is in use, grid_old partly set, or NULL with flip > 0, overlapping buffers. */
int mgps_particles_update(const mgps_particles_update_desc *d, void *stream);

/* ---- FLIP particles next to solids: collide, and resample ------------------------------------------------------
 * With these the sub-step is: bin, RESAMPLE, particles -> grid, extrapolate, (add forces), project, extrapolate, update WITH
 * COLLISION.  Conventions, arithmetic and determinism are those of entries 1 to 3: fp64 on float32 data, every operation rounded on
 * its own, an fma only where one is written, one rounding to float32 where a value is stored, no floating-point atomics.
 * tests/particles_solids_reference.py restates both in numpy.
 *
 * 4. mgps_particles_collide: push the particles out of the solid and take the normal velocity into it away; one thread per particle.
 *   solid_phi: a device cell grid, negative inside the solid, IN CELLS, as mgps_fields_rasterize_bodies writes it.  solid_velocity:
 *   the three face grids the projection takes, all three or all NULL (the solid is at rest).  S is advection's sampling rule on the
 *   cell lattice, U on the three face lattices.  Per inside particle (x, v), x in fp64:
 *   Push-out loop, at most `iterations` times (1 .. 4):
 *     phi = S(solid_phi)(x); if phi >= margin the loop ends.
 *     g_c = S(x + e_c / 2) - S(x - e_c / 2) for c = x, y, z (the sample points are not clamped: S clamps into its lattice);
 *     m = (g_x g_x + g_y g_y) + g_z g_z.  If not m > 1e-12 (NaN as well) the particle is STUCK and the loop ends: it is not moved
 *     from where it is (a push of an earlier iteration stays, and the particle counts as pushed as well).
 *     Otherwise n_c = g_c / sqrt(m) and x_c = clampB(fma(margin - phi, n_c, x_c)): a PUSH.
 *   A particle that was not pushed leaves with its input bits, position and velocity.  A pushed one, n being that of its last push:
 *     u_s = U(solid_velocity)(x) at the fp64 end point, or 0; r_c = double(v_c) - u_s,c; vn = (r_x n_x + r_y n_y) + r_z n_z;
 *     if vn < 0: r_c = r_c - vn n_c, then r_c = (1 - friction) r_c (friction acts on a particle that moves into the solid, and on
 *     no other); v_out,c = float(r_c + u_s,c); x_out,c = float(x_c), the one rounding of the position.
 *   Outside particles are copied through.
 *   counts_dev (device, unsigned long long[3], may be NULL) is ADDED to: [0] pushed particles, [1] pushed particles with
 *   S(solid_phi)(x_out) < 0 at the float32 position, one more sample (iterations too few, or a solid thinner than a step), [2] stuck
 *   particles.
 *   Buffers: as entry 3, in place or out of place.  The pass tests a particle where it is; it does not trace through the solid. */
typedef struct mgps_particles_collide_desc {
    int struct_size;                 /* sizeof(mgps_particles_collide_desc) */
    int gx, gy, gz;                  /* the WHOLE simulation grid */
    int n;                           /* particles, >= 0 */
    int iterations;                  /* 1 .. 4 */
    double margin;                   /* cells, finite and >= 0: a particle ends at solid_phi = margin */
    double friction;                 /* in [0, 1] */
    const float *position_in[3];     /* device, n entries each; not read (may be NULL) when n == 0 */
    const float *velocity_in[3];
    float *position_out[3];
    float *velocity_out[3];
    const float *solid_phi;          /* device cell grid, cells */
    const float *solid_velocity[3];  /* device face grids: all three, or all NULL */
    unsigned long long *counts_dev;  /* 3 entries, or NULL */
} mgps_particles_collide_desc;
/* Does not synchronise the stream.  Refuses with a message, before any device work: NULL desc or a struct_size mismatch, an
 * extent < 1, gx gy gz + 1 >= 2^31, n < 0, a margin that is not finite and >= 0, iterations outside 1 .. 4, a friction outside
 * [0, 1], a NULL solid_phi, solid_velocity partly set, a NULL particle array with n > 0, overlapping buffers. */
int mgps_particles_collide(const mgps_particles_collide_desc *d, void *stream);

/* 5. mgps_particles_update_solid: entry 3 and entry 4 in ONE launch.  The update is done exactly as mgps_particles_update does it,
 * position and velocity are rounded to float32, and rule 4 is applied to those float32 values in registers: all six arrays and both
 * sets of counts (d->counts_dev[2], solid->counts_dev[3]) are BIT-EQUAL to mgps_particles_update followed by
 * mgps_particles_collide, without the second pass over six arrays.  Of `solid`, n and the particle arrays are not read; its gx, gy,
 * gz are d's.  Refuses what either entry refuses of these fields, and two descs of different extents. */
int mgps_particles_update_solid(const mgps_particles_update_desc *d, const mgps_particles_collide_desc *solid, void *stream);

/* 6. mgps_particles_resample: keep the particle count per cell in range -- thin crowded cells, seed deep empty ones.  From BINNED
 * particles (position, velocity, cell_start as mgps_particles_bin left them), out of place, into arrays of `capacity` entries; the
 * output is a binned set again (cell order, cell_start_out of cells + 2 entries, *n_out_dev), so particles -> grid follows
 * without another bin.
 *   Per cell c, with m_c = its slots, every slot range taken from cell_start clamped into [0, n] (and an end before its start: 0):
 *   Thin.  m_c <= max_per_cell: every slot is kept.  Otherwise slot t (from 0 within the cell) is kept if
 *     floor((t + 1) max / m_c) > floor(t max / m_c) in integers: exactly max slots, evenly strided, in their order.
 *   Seed.  c is DEEP if liquid_phi is given, liquid_phi[c] <= -float(seed_depth dx), and solid_phi[c] > 0 where solid_phi is given.
 *     A deep cell with k < min_per_cell kept slots gets min - k new particles behind its kept ones.  New particle q = 0 .. of cell
 *     (i_x, i_y, i_z): x_a = min(float(double(i_a) + r), the float32 just below i_a + 1), r = (h >> 8) 2^-24,
 *     h = mix(mix(mix(seed ^ 0x9e3779b9) + uint32(c)) + uint32(3 (k + q) + a)),
 *     mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 in wrapping uint32 -- so it lies in its
 *     cell.  Its velocity is float(U(grid)(x)) at that float32 position.  min_per_cell = 0: no seeding.
 *   The outside bin follows the last cell when keep_outside is 1 and is dropped otherwise: cell_start_out[cells] is its first slot,
 *   cell_start_out[cells + 1] = *n_out_dev the total.
 *   Capacity.  *n_out_dev is the total the rule asks for, whether or not it fits; no slot >= capacity is written; the outputs are a
 *   valid set only if *n_out_dev <= capacity.
 *   counts_dev (device, unsigned long long[4], may be NULL) is ADDED to: [0] particles removed by thinning, [1] particles seeded,
 *   [2] deep cells, [3] 1 when the total does not fit.
 *   The result is a function of the inputs alone.  A wrong cell_start gives wrong values (a slot that is not within the range
 *   cell_start gives for the cell of its position is dropped), never an out-of-range read or write.
 *   A count kernel over the cells, rocprim::exclusive_scan into cell_start_out, a copy kernel over the input slots (its cell from its
 *   position, its rank floor(t max / m_c) in closed form) and a seeding kernel over (cell, q), in stream order with temporary storage
 *   from the stream's pool: no host synchronisation. */
typedef struct mgps_particles_resample_desc {
    int struct_size;                 /* sizeof(mgps_particles_resample_desc) */
    int gx, gy, gz;                  /* the WHOLE simulation grid */
    int n;                           /* input particles, >= 0 */
    int capacity;                    /* entries of each output array, >= 0 */
    int min_per_cell, max_per_cell;  /* 0 <= min <= max, 1 <= max <= 64 */
    int keep_outside;                /* 0 or 1 */
    uint32_t seed;
    double dx;                       /* the cell size in liquid_phi's units, finite and > 0 */
    double seed_depth;               /* cells, finite and >= 0 */
    const float *position[3];        /* binned; not read (may be NULL) when n == 0 */
    const float *velocity[3];
    const int32_t *cell_start;       /* cells + 2 entries */
    const float *liquid_phi;         /* device cell grid; required when min_per_cell > 0 */
    const float *solid_phi;          /* device cell grid, or NULL */
    const float *grid[3];            /* device face grids, all three or all NULL; required when min_per_cell > 0 */
    float *position_out[3];          /* capacity entries each */
    float *velocity_out[3];
    int32_t *cell_start_out;         /* cells + 2 entries */
    int32_t *n_out_dev;              /* one entry */
    unsigned long long *counts_dev;  /* 4 entries, or NULL */
} mgps_particles_resample_desc;
/* Does not synchronise the stream.  Refuses with a message, before any device work: NULL desc or a struct_size mismatch, an
 * extent < 1, gx gy gz + 1 >= 2^31, n < 0, capacity < 0, max_per_cell outside 1 .. 64, min_per_cell outside 0 .. max_per_cell,
 * keep_outside neither 0 nor 1, a dx that is not finite and > 0, a seed_depth that is not finite and >= 0,
 * n + gx gy gz min_per_cell >= 2^31, grid partly set, liquid_phi or grid NULL with min_per_cell > 0, a NULL array that is in use,
 * overlapping buffers. */
int mgps_particles_resample(const mgps_particles_resample_desc *d, void *stream);

#ifdef __cplusplus
}
#endif
#endif
