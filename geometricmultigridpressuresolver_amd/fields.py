"""Python mirror of include/mgps_fields.h: the plugin-side field pre/post-processing of
HDK_GeometricFreeSurfacePressureSolver::solveGasSubclass (Plug.cpp:297-426, 631-714) on the device, with
torch CUDA tensors as device memory.  Names follow the reference's functions.

Grids are (nz, ny, nx) tensors (x fastest); face grids of axis a have one more entry along a (axis 0 = x =
last tensor dimension).  Material labels int32: 0 SOLID, 1 LIQUID, 2 AIR.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import check, lib

SOLID_CELL, LIQUID_CELL, AIR_CELL = 0, 1, 2


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _current_device():
    return torch.device("cuda", torch.cuda.current_device())


def _g(shape):
    gz, gy, gx = shape
    return gx, gy, gz


def _face_shape(shape, axis):
    s = list(shape)
    s[2 - axis] += 1
    return tuple(s)


def _chk(t, shape, dtype):
    assert t.is_cuda and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == tuple(shape), (t.shape, shape, t.dtype)
    return t


def buildMaterialCellLabels(liquid_surface, solid_surface, cut_cell_weights):
    """Util.cpp:87-148.  SDFs sampled at cell centres, cut-cell weights on the three face grids."""
    shape = tuple(liquid_surface.shape)
    cw = [_chk(cut_cell_weights[a], _face_shape(shape, a), torch.float32) for a in range(3)]
    out = torch.empty(shape, dtype=torch.int32, device=liquid_surface.device)
    check(lib().mgps_fields_material_labels(_p(out), _p(_chk(liquid_surface, shape, torch.float32)), _p(_chk(solid_surface, shape, torch.float32)),
                                            _p(cw[0]), _p(cw[1]), _p(cw[2]), *_g(shape), _stream()))
    return out


def buildValidFaces(material, cut_cell_weights):
    """Plug.cpp:716-744: one uint8 face grid per axis."""
    shape = tuple(material.shape)
    out = []
    for a in range(3):
        v = torch.empty(_face_shape(shape, a), dtype=torch.uint8, device=material.device)
        check(lib().mgps_fields_valid_faces(a, _p(v), _p(_chk(material, shape, torch.int32)),
                                            _p(_chk(cut_cell_weights[a], _face_shape(shape, a), torch.float32)), *_g(shape), _stream()))
        out.append(v)
    return out


def buildMGDomain(material, cut_cell_weights, liquid_surface, valid_faces, expanded_shape, offset):
    """buildMGDomainLabels + buildMGBoundaryWeights x3 + setBoundaryCellLabels, written straight into the
    expanded solver grid (Plug.cpp:344-362, 746-865): returns (labels uint8, [wx, wy, wz] float32)."""
    shape, eshape = tuple(material.shape), tuple(expanded_shape)
    dev = material.device
    labels = torch.empty(eshape, dtype=torch.uint8, device=dev)
    check(lib().mgps_fields_domain_labels(_p(labels), _p(material), *_g(shape), *_g(eshape), int(offset), _stream()))
    weights = []
    for a in range(3):
        w = torch.empty(_face_shape(eshape, a), dtype=torch.float32, device=dev)
        check(lib().mgps_fields_boundary_weights(a, _p(w), _p(cut_cell_weights[a]), _p(_chk(liquid_surface, shape, torch.float32)),
                                                 _p(_chk(valid_faces[a], _face_shape(shape, a), torch.uint8)), _p(material), *_g(shape),
                                                 *_g(eshape), int(offset), _stream()))
        weights.append(w)
    check(lib().mgps_fields_set_boundary_labels(_p(labels), _p(weights[0]), _p(weights[1]), _p(weights[2]), *_g(eshape), _stream()))
    return labels, weights


def buildRHS(material, velocity, cut_cell_weights, expanded_shape, offset, solid_velocity=None):
    """Plug.cpp:867-943."""
    shape, eshape = tuple(material.shape), tuple(expanded_shape)
    rhs = torch.empty(eshape, dtype=torch.float32, device=material.device)
    sv = solid_velocity if solid_velocity is not None else [None, None, None]
    check(lib().mgps_fields_rhs(_p(rhs), _p(material), *[_p(_chk(velocity[a], _face_shape(shape, a), torch.float32)) for a in range(3)],
                                *[_p(sv[a]) for a in range(3)], *[_p(cut_cell_weights[a]) for a in range(3)], *_g(shape), *_g(eshape),
                                int(offset), _stream()))
    return rhs


def applyOldPressure(pressure, material, expanded_shape, offset):
    """Plug.cpp:945-997: the warm-start solution grid."""
    shape, eshape = tuple(material.shape), tuple(expanded_shape)
    x = torch.empty(eshape, dtype=torch.float32, device=material.device)
    check(lib().mgps_fields_pressure_to_solution(_p(x), _p(_chk(pressure, shape, torch.float32)), _p(material), *_g(shape), *_g(eshape),
                                                 int(offset), _stream()))
    return x


def applySolutionToPressure(pressure, solution, material, offset):
    """Plug.cpp:999-1047 (in place on `pressure`)."""
    shape, eshape = tuple(material.shape), tuple(solution.shape)
    check(lib().mgps_fields_solution_to_pressure(_p(_chk(pressure, shape, torch.float32)), _p(solution), _p(material), *_g(shape),
                                                 *_g(eshape), int(offset), _stream()))
    return pressure


def applyPressureGradient(velocity, liquid_surface, pressure, valid_faces, material, surface_pressure=None):
    """Plug.cpp:1049-1131 (in place on the three velocity face grids).  With `surface_pressure` (a cell grid, see
    buildSurfacePressure) the air cell's pressure on a liquid/air face is the interface pressure p_G instead of 0."""
    shape = tuple(material.shape)
    for a in range(3):
        v = _p(_chk(velocity[a], _face_shape(shape, a), torch.float32))
        if surface_pressure is None:
            check(lib().mgps_fields_pressure_gradient(a, v, _p(liquid_surface), _p(pressure), _p(valid_faces[a]), _p(material), *_g(shape), _stream()))
        else:
            check(lib().mgps_fields_pressure_gradient_surface(a, v, _p(liquid_surface), _p(pressure), _p(_chk(surface_pressure, shape, torch.float32)),
                                                              _p(valid_faces[a]), _p(material), *_g(shape), _stream()))
    return velocity


def buildSurfacePressure(liquid_surface, material, scale):
    """Surface pressure scale * clamp(curvature, -1, 1) at the LIQUID / AIR cells of the free surface, 0 elsewhere (DESIGN.md
    section 13).  scale = sigma * dt / (density * dx^2) gives the pressure of a surface tension sigma."""
    shape = tuple(material.shape)
    sp = torch.empty(shape, dtype=torch.float32, device=material.device)
    check(lib().mgps_fields_surface_pressure(_p(sp), _p(_chk(liquid_surface, shape, torch.float32)), _p(_chk(material, shape, torch.int32)),
                                             C.c_double(scale), *_g(shape), _stream()))
    return sp


def addSurfacePressureToRHS(rhs, weights, liquid_surface, material, surface_pressure, offset, p_gamma_max=None):
    """rhs[L] += w_f * p_G on the liquid/air faces (in place on the expanded rhs of buildRHS; `weights` from buildMGDomain).
    `p_gamma_max` (a one-element float32 tensor, or None) is raised to the largest |p_G|."""
    shape, eshape = tuple(material.shape), tuple(rhs.shape)
    w = [_chk(weights[a], _face_shape(eshape, a), torch.float32) for a in range(3)]
    check(lib().mgps_fields_rhs_surface(_p(_chk(rhs, eshape, torch.float32)), _p(w[0]), _p(w[1]), _p(w[2]),
                                        _p(_chk(liquid_surface, shape, torch.float32)), _p(_chk(material, shape, torch.int32)),
                                        _p(_chk(surface_pressure, shape, torch.float32)), _p(p_gamma_max), *_g(shape), *_g(eshape),
                                        int(offset), _stream()))
    return rhs


def computeResultingDivergence(material, velocity, cut_cell_weights, solid_velocity=None):
    """Plug.cpp:1133-1207: (accumulated divergence, max divergence, liquid cell count)."""
    shape = tuple(material.shape)
    out = (C.c_double * 3)()
    sv = solid_velocity if solid_velocity is not None else [None, None, None]
    check(lib().mgps_fields_divergence(out, _p(material), *[_p(velocity[a]) for a in range(3)], *[_p(sv[a]) for a in range(3)],
                                       *[_p(cut_cell_weights[a]) for a in range(3)], *_g(shape), _stream()))
    return out[0], out[1], out[2]


# ---- the whole projection in one call on host arrays (what the Houdini shim calls) ---------------------------------
class Projection(C.Structure):
    """mgps_projection (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("gx", C.c_int), ("gy", C.c_int), ("gz", C.c_int), ("real_bytes", C.c_int),
        ("liquid_phi", C.c_void_p), ("solid_phi", C.c_void_p), ("cut_weights", C.c_void_p * 3), ("velocity", C.c_void_p * 3),
        ("solid_velocity", C.c_void_p * 3), ("pressure", C.c_void_p), ("valid_faces", C.c_void_p * 3),
        ("use_old_pressure", C.c_int), ("use_mg_preconditioner", C.c_int), ("use_gauss_seidel", C.c_int),
        ("tolerance", C.c_double), ("max_iterations", C.c_int), ("power_of_two", C.c_int),
        ("stats", _lib.PcgStats), ("mg_levels", C.c_int), ("offset", C.c_int), ("expanded", C.c_int * 3),
        ("liquid_cells", C.c_double), ("residual_inf", C.c_double), ("residual_l2", C.c_double),
        ("divergence_sum", C.c_double), ("divergence_max", C.c_double),
        ("setup_ms", C.c_double), ("solve_ms", C.c_double), ("total_ms", C.c_double),
        ("enclosed_components", C.c_int), ("rhs_mean_removed_max", C.c_double),
        ("surface_tension", C.c_double), ("dt", C.c_double), ("dx", C.c_double), ("density", C.c_double),
        ("surface_pressure", C.c_void_p), ("surface_pressure_max", C.c_double),
    ]


def project_free_surface(liquid_phi, solid_phi, cut_weights, velocity, pressure, solid_velocity=None, use_old_pressure=True,
                         use_mg_preconditioner=True, use_gauss_seidel=True, tolerance=1e-5, max_iterations=2500, power_of_two=True,
                         options=None, surface_tension=0.0, dt=0.0, dx=0.0, density=0.0, surface_pressure=None):
    """solveGasSubclass (Plug.cpp:252-707) on numpy host arrays of one dtype (float32 or float64): `velocity` and `pressure`
    are updated in place; returns (valid_faces[3] uint8, info dict).  Surface tension: sigma =
    `surface_tension` > 0 with the time step `dt`, the cell size `dx` and the liquid `density`, or a caller's cell grid
    `surface_pressure` in the units of `pressure`."""
    import numpy as np

    real = np.dtype(pressure.dtype)
    assert real in (np.dtype(np.float32), np.dtype(np.float64))
    shape = tuple(liquid_phi.shape)

    def chk(a, sh):
        assert a.dtype == real and a.flags.c_contiguous and tuple(a.shape) == tuple(sh), (a.dtype, a.shape, sh)
        return a.ctypes.data_as(C.c_void_p)

    pr = Projection()
    pr.struct_size = C.sizeof(Projection)
    pr.gz, pr.gy, pr.gx = shape
    pr.real_bytes = real.itemsize
    pr.liquid_phi, pr.solid_phi, pr.pressure = chk(liquid_phi, shape), chk(solid_phi, shape), chk(pressure, shape)
    valid = []
    for a in range(3):
        fs = _face_shape(shape, a)
        pr.cut_weights[a] = chk(cut_weights[a], fs)
        pr.velocity[a] = chk(velocity[a], fs)
        pr.solid_velocity[a] = chk(solid_velocity[a], fs) if solid_velocity is not None else None
        valid.append(np.zeros(fs, dtype=np.uint8))
        pr.valid_faces[a] = valid[a].ctypes.data_as(C.c_void_p)
    pr.use_old_pressure, pr.use_mg_preconditioner, pr.use_gauss_seidel = int(use_old_pressure), int(use_mg_preconditioner), int(use_gauss_seidel)
    pr.tolerance, pr.max_iterations, pr.power_of_two = float(tolerance), int(max_iterations), int(power_of_two)
    pr.surface_tension, pr.dt, pr.dx, pr.density = float(surface_tension), float(dt), float(dx), float(density)
    pr.surface_pressure = chk(surface_pressure, shape) if surface_pressure is not None else None
    status = lib().mgps_project_free_surface(C.byref(pr), C.byref(options) if options is not None else None)
    info = {
        "iterations": pr.stats.iterations, "outcome": pr.stats.outcome, "rel_residual": pr.stats.rel_residual,
        "rel_residual_recomputed": pr.stats.rel_residual_recomputed, "mg_levels": pr.mg_levels, "offset": pr.offset,
        "expanded": (pr.expanded[2], pr.expanded[1], pr.expanded[0]), "liquid_cells": pr.liquid_cells,
        "residual_inf": pr.residual_inf, "residual_l2": pr.residual_l2, "divergence_sum": pr.divergence_sum,
        "divergence_max": pr.divergence_max, "setup_ms": pr.setup_ms, "solve_ms": pr.solve_ms, "total_ms": pr.total_ms,
        "enclosed_components": pr.enclosed_components, "rhs_mean_removed_max": pr.rhs_mean_removed_max,
        "surface_pressure_max": pr.surface_pressure_max,
    }
    try:
        check(status)
    except _lib.MgpsError as e:  # (interrupted: pressure and velocity hold what the iterate reached gives, include/mgps_fields.h)
        e.info, e.valid_faces = info, valid
        raise
    return valid, info


# ---- the fields layer on Z-slabs (include/mgps_fields.h) --------------------------------------------------
class FieldsSlab(C.Structure):
    """mgps_fields_slab: one rank's window of a slab projection."""

    _fields_ = [(n, C.c_int) for n in ("struct_size", "gx", "gy", "gz", "c0", "c1", "ex", "ey", "ez", "offset", "e0", "e1")]

    @property
    def base_shape(self):
        """the window's cell grid (nz, ny, nx)"""
        return (self.c1 - self.c0, self.gy, self.gx)

    @property
    def expanded_shape(self):
        """the window's expanded cell grid (nz, ny, nx)"""
        return (self.e1 - self.e0, self.ey, self.ex)


def projection_slab_layout(shape, power_of_two, size, use_gauss_seidel):
    """mgps_projection_slab_layout (host only): the expanded layout of the WHOLE grid `shape` = (gz, gy, gx) and cuts for `size`
    ranks that divide the base planes evenly.  Returns {"expanded": (ez, ey, ex), "offset", "levels", "splits": [size + 1]}."""
    gz, gy, gx = shape
    dims, off, lev, cuts = (C.c_int * 3)(), C.c_int(), C.c_int(), (C.c_int * (int(size) + 1))()
    check(lib().mgps_projection_slab_layout(gx, gy, gz, int(bool(power_of_two)), int(size), int(bool(use_gauss_seidel)), dims, C.byref(off),
                                            C.byref(lev), cuts))
    return {"expanded": (dims[2], dims[1], dims[0]), "offset": off.value, "levels": lev.value, "splits": [int(v) for v in cuts]}


def slab_window(global_shape, power_of_two, splits, rank):
    """mgps_fields_slab_describe: the window of rank `rank` for the cuts `splits` of the expanded grid."""
    gz, gy, gx = global_shape
    d = FieldsSlab()
    cuts = (C.c_int * len(splits))(*[int(v) for v in splits])
    check(lib().mgps_fields_slab_describe(C.byref(d), gx, gy, gz, int(bool(power_of_two)), cuts, len(splits) - 1, int(rank)))
    return d


def _face3(shape):
    return [_face_shape(shape, a) for a in range(3)]


def _arr3(ts):
    return (C.c_void_p * 3)(*[t.data_ptr() if t is not None else None for t in ts])


def _halo(d, halo, dtype):
    """(lo, hi) plane tensors -> two pointers; None where the grid ends"""
    lo, hi = halo if halo is not None else (None, None)
    for t in (lo, hi):
        if t is not None:
            _chk(t, (d.gy, d.gx), dtype)
    assert (lo is not None) == (d.c0 > 0) and (hi is not None) == (d.c1 < d.gz), "halo planes: exactly where the grid goes on"
    return _p(lo), _p(hi)


def buildMaterialCellLabelsSlab(d, liquid_surface, phi_halo, solid_surface, cut_cell_weights):
    """buildMaterialCellLabels on the window `d`; phi_halo = (plane c0 - 1 or None, plane c1 or None)."""
    shape = d.base_shape
    cw = [_chk(cut_cell_weights[a], fs, torch.float32) for a, fs in enumerate(_face3(shape))]
    out = torch.empty(shape, dtype=torch.int32, device=liquid_surface.device)
    check(lib().mgps_fields_slab_material_labels(C.byref(d), _p(out), _p(_chk(liquid_surface, shape, torch.float32)), *_halo(d, phi_halo, torch.float32),
                                                 _p(_chk(solid_surface, shape, torch.float32)), _p(cw[0]), _p(cw[1]), _p(cw[2]), _stream()))
    return out


def buildFacesSlab(d, material, material_halo, liquid_surface, phi_halo, cut_cell_weights):
    """buildValidFaces + buildMGBoundaryWeights of all three axes in one pass: (valid[3] uint8 base face grids of the window,
    weights[3] float32 expanded face grids of the window, zeros outside the base box included)."""
    shape, eshape, dev = d.base_shape, d.expanded_shape, material.device
    valid = [torch.empty(fs, dtype=torch.uint8, device=dev) for fs in _face3(shape)]
    weights = [torch.empty(fs, dtype=torch.float32, device=dev) for fs in _face3(eshape)]
    cw = [_chk(cut_cell_weights[a], fs, torch.float32) for a, fs in enumerate(_face3(shape))]
    check(lib().mgps_fields_slab_faces(C.byref(d), _arr3(valid), _arr3(weights), _p(_chk(material, shape, torch.int32)), *_halo(d, material_halo, torch.int32),
                                       _p(_chk(liquid_surface, shape, torch.float32)), *_halo(d, phi_halo, torch.float32), _arr3(cw), _stream()))
    return valid, weights


def buildLabelsSlab(d, material, material_halo, weights):
    """buildMGDomainLabels + setBoundaryCellLabels on the window's expanded planes (EXTERIOR outside the base box)."""
    eshape = d.expanded_shape
    w = [_chk(weights[a], fs, torch.float32) for a, fs in enumerate(_face3(eshape))]
    labels = torch.empty(eshape, dtype=torch.uint8, device=material.device)
    check(lib().mgps_fields_slab_labels(C.byref(d), _p(labels), _p(_chk(material, d.base_shape, torch.int32)), *_halo(d, material_halo, torch.int32),
                                        _arr3(w), _stream()))
    return labels


def buildRHSSlab(d, material, velocity, cut_cell_weights, solid_velocity=None, out=None):
    """buildRHS on the window's expanded planes (`out`: a grid of a slab solver, or None for a new tensor)."""
    shape = d.base_shape
    rhs = out if out is not None else torch.empty(d.expanded_shape, dtype=torch.float32, device=material.device)
    v = [_chk(velocity[a], fs, torch.float32) for a, fs in enumerate(_face3(shape))]
    check(lib().mgps_fields_slab_rhs(C.byref(d), _p(_chk(rhs, d.expanded_shape, torch.float32)), _p(_chk(material, shape, torch.int32)), _arr3(v),
                                     _arr3(solid_velocity) if solid_velocity is not None else None, _arr3(cut_cell_weights), _stream()))
    return rhs


def applyOldPressureSlab(d, pressure, material, out=None):
    x = out if out is not None else torch.empty(d.expanded_shape, dtype=torch.float32, device=material.device)
    check(lib().mgps_fields_slab_pressure_to_solution(C.byref(d), _p(_chk(x, d.expanded_shape, torch.float32)), _p(_chk(pressure, d.base_shape, torch.float32)),
                                                      _p(_chk(material, d.base_shape, torch.int32)), _stream()))
    return x


def applySolutionToPressureSlab(d, pressure, solution, material, clear_others=False):
    check(lib().mgps_fields_slab_solution_to_pressure(C.byref(d), _p(_chk(pressure, d.base_shape, torch.float32)), _p(_chk(solution, d.expanded_shape, torch.float32)),
                                                      _p(_chk(material, d.base_shape, torch.int32)), int(bool(clear_others)), _stream()))
    return pressure


def applyPressureGradientSlab(d, velocity, liquid_surface, phi_halo, pressure, pressure_halo, valid_faces, material, material_halo,
                              surface_pressure=None, surface_pressure_halo=None):
    """applyPressureGradient of all three axes on the window (in place); with `surface_pressure` the surface-tension form."""
    shape = d.base_shape
    v = [_chk(velocity[a], fs, torch.float32) for a, fs in enumerate(_face3(shape))]
    sp = (_p(_chk(surface_pressure, shape, torch.float32)), *_halo(d, surface_pressure_halo, torch.float32)) if surface_pressure is not None else (None, None, None)
    check(lib().mgps_fields_slab_pressure_gradient(C.byref(d), _arr3(v), _p(_chk(liquid_surface, shape, torch.float32)), *_halo(d, phi_halo, torch.float32),
                                                   _p(_chk(pressure, shape, torch.float32)), *_halo(d, pressure_halo, torch.float32), *sp,
                                                   _arr3([_chk(valid_faces[a], fs, torch.uint8) for a, fs in enumerate(_face3(shape))]),
                                                   _p(_chk(material, shape, torch.int32)), *_halo(d, material_halo, torch.int32), _stream()))
    return velocity


def buildSurfacePressureSlab(d, liquid_surface, phi_halo, material, material_halo, scale):
    shape = d.base_shape
    sp = torch.empty(shape, dtype=torch.float32, device=material.device)
    check(lib().mgps_fields_slab_surface_pressure(C.byref(d), _p(sp), _p(_chk(liquid_surface, shape, torch.float32)), *_halo(d, phi_halo, torch.float32),
                                                  _p(_chk(material, shape, torch.int32)), *_halo(d, material_halo, torch.int32), C.c_double(scale), _stream()))
    return sp


def addSurfacePressureToRHSSlab(d, rhs, weights, liquid_surface, phi_halo, material, material_halo, surface_pressure, surface_pressure_halo,
                                p_gamma_max=None):
    shape, eshape = d.base_shape, d.expanded_shape
    w = [_chk(weights[a], fs, torch.float32) for a, fs in enumerate(_face3(eshape))]
    check(lib().mgps_fields_slab_rhs_surface(C.byref(d), _p(_chk(rhs, eshape, torch.float32)), _arr3(w), _p(_chk(liquid_surface, shape, torch.float32)),
                                             *_halo(d, phi_halo, torch.float32), _p(_chk(material, shape, torch.int32)), *_halo(d, material_halo, torch.int32),
                                             _p(_chk(surface_pressure, shape, torch.float32)), *_halo(d, surface_pressure_halo, torch.float32),
                                             _p(p_gamma_max), _stream()))
    return rhs


def computeResultingDivergenceSlab(d, material, velocity, cut_cell_weights, solid_velocity=None):
    """this rank's (sum, max, liquid cell count); the caller reduces over the ranks"""
    out = (C.c_double * 3)()
    check(lib().mgps_fields_slab_divergence(C.byref(d), out, _p(_chk(material, d.base_shape, torch.int32)), _arr3(velocity),
                                            _arr3(solid_velocity) if solid_velocity is not None else None, _arr3(cut_cell_weights), _stream()))
    return out[0], out[1], out[2]


class ProjectionSlab(C.Structure):
    """mgps_projection_slab (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("gx", C.c_int), ("gy", C.c_int), ("gz", C.c_int),
        ("liquid_phi", C.c_void_p), ("solid_phi", C.c_void_p), ("cut_weights", C.c_void_p * 3), ("velocity", C.c_void_p * 3),
        ("solid_velocity", C.c_void_p * 3), ("pressure", C.c_void_p), ("valid_faces", C.c_void_p * 3),
        ("use_old_pressure", C.c_int), ("use_mg_preconditioner", C.c_int), ("use_gauss_seidel", C.c_int),
        ("tolerance", C.c_double), ("max_iterations", C.c_int), ("power_of_two", C.c_int),
        ("stats", _lib.PcgStats), ("mg_levels", C.c_int), ("offset", C.c_int), ("expanded", C.c_int * 3),
        ("liquid_cells", C.c_double), ("residual_inf", C.c_double), ("residual_l2", C.c_double),
        ("divergence_sum", C.c_double), ("divergence_max", C.c_double),
        ("setup_ms", C.c_double), ("solve_ms", C.c_double), ("total_ms", C.c_double),
        ("enclosed_components", C.c_int), ("rhs_mean_removed_max", C.c_double),
        ("surface_tension", C.c_double), ("dt", C.c_double), ("dx", C.c_double), ("density", C.c_double),
        ("surface_pressure", C.c_void_p), ("surface_pressure_max", C.c_double), ("stage_ms", C.c_double * 8),
    ]


STAGES_SLAB = ("passes", "labels_to_hosts", "solver_setup", "rhs", "solve", "write_back", "plane_exchanges")


def _projection_slab(d, global_shape, liquid_phi, solid_phi, cut_weights, velocity, pressure, solid_velocity, use_old_pressure,
                     use_mg_preconditioner, use_gauss_seidel, tolerance, max_iterations, power_of_two, surface_tension, dt, dx, density,
                     surface_pressure):
    """the ProjectionSlab of one call on the window `d` and the valid-face tensors it writes"""
    shape = d.base_shape
    faces = _face3(shape)
    dev = liquid_phi.device
    pr = ProjectionSlab()
    pr.struct_size = C.sizeof(ProjectionSlab)
    pr.gz, pr.gy, pr.gx = global_shape

    def ptr(t, sh):
        return _chk(t, sh, torch.float32).data_ptr()

    pr.liquid_phi, pr.solid_phi, pr.pressure = ptr(liquid_phi, shape), ptr(solid_phi, shape), ptr(pressure, shape)
    valid = []
    for a in range(3):
        pr.cut_weights[a] = ptr(cut_weights[a], faces[a])
        pr.velocity[a] = ptr(velocity[a], faces[a])
        # (a missing entry stays NULL: the library refuses "some but not all" on every rank together)
        pr.solid_velocity[a] = ptr(solid_velocity[a], faces[a]) if solid_velocity is not None and solid_velocity[a] is not None else None
        valid.append(torch.zeros(faces[a], dtype=torch.uint8, device=dev))
        pr.valid_faces[a] = valid[a].data_ptr()
    pr.use_old_pressure, pr.use_mg_preconditioner, pr.use_gauss_seidel = int(use_old_pressure), int(use_mg_preconditioner), int(use_gauss_seidel)
    pr.tolerance, pr.max_iterations, pr.power_of_two = float(tolerance), int(max_iterations), int(bool(power_of_two))
    pr.surface_tension, pr.dt, pr.dx, pr.density = float(surface_tension), float(dt), float(dx), float(density)
    pr.surface_pressure = ptr(surface_pressure, shape) if surface_pressure is not None else None
    return pr, valid


def _projection_slab_info(pr, d):
    return {
        "iterations": pr.stats.iterations, "outcome": pr.stats.outcome, "rel_residual": pr.stats.rel_residual,
        "rel_residual_recomputed": pr.stats.rel_residual_recomputed, "mg_levels": pr.mg_levels, "offset": pr.offset,
        "expanded": (pr.expanded[2], pr.expanded[1], pr.expanded[0]), "liquid_cells": pr.liquid_cells,
        "residual_inf": pr.residual_inf, "residual_l2": pr.residual_l2, "divergence_sum": pr.divergence_sum,
        "divergence_max": pr.divergence_max, "setup_ms": pr.setup_ms, "solve_ms": pr.solve_ms, "total_ms": pr.total_ms,
        "enclosed_components": pr.enclosed_components, "rhs_mean_removed_max": pr.rhs_mean_removed_max,
        "surface_pressure_max": pr.surface_pressure_max, "window": (d.c0, d.c1),
        "stage_ms": {n: pr.stage_ms[q] for q, n in enumerate(STAGES_SLAB)},
    }


def project_free_surface_slab(comm, splits, global_shape, liquid_phi, solid_phi, cut_weights, velocity, pressure, solid_velocity=None,
                              use_old_pressure=True, use_mg_preconditioner=True, use_gauss_seidel=True, tolerance=1e-5, max_iterations=2500,
                              power_of_two=True, options=None, surface_tension=0.0, dt=0.0, dx=0.0, density=0.0, surface_pressure=None):
    """mgps_project_free_surface_slab: solveGasSubclass on the float32 CUDA tensors of this rank's window of the grid `global_shape`
    = (gz, gy, gx), a collective over the transport `comm` (RcclComm / TorchDistComm; a world of one is the device-resident
    projection on one GPU).  `splits`: the cuts of the expanded grid (projection_slab_layout, or the caller's own).  Cell, x-face
    and y-face grids hold the rank's base planes [c0, c1) (slab_window), z-face grids the faces c0 .. c1.  `velocity` and
    `pressure` are updated in place; returns (valid_faces[3] uint8 CUDA tensors, info dict of the whole grid's numbers)."""
    d = slab_window(global_shape, power_of_two, splits, comm.rank)
    pr, valid = _projection_slab(d, global_shape, liquid_phi, solid_phi, cut_weights, velocity, pressure, solid_velocity, use_old_pressure,
                                 use_mg_preconditioner, use_gauss_seidel, tolerance, max_iterations, power_of_two, surface_tension, dt, dx, density,
                                 surface_pressure)
    cuts = (C.c_int * len(splits))(*[int(v) for v in splits])
    status = lib().mgps_project_free_surface_slab(C.byref(pr), C.byref(options) if options is not None else None, C.byref(comm.struct), cuts, _stream())
    info = _projection_slab_info(pr, d)
    try:
        check(status)
    except _lib.MgpsError as e:  # (interrupted: pressure and velocity hold what the iterate reached gives)
        e.info, e.valid_faces = info, valid
        raise
    return valid, info


# ---- velocity extrapolation into the air band (include/mgps_fields.h) ------------------------------------------
def _cw3(cut_cell_weights, faces):
    """None, or the three cut-cell weight grids (a missing one stays NULL: the library refuses "some but not all")"""
    if cut_cell_weights is None:
        return None
    return [_chk(c, fs, torch.float32) if c is not None else None for c, fs in zip(cut_cell_weights, faces)]


def extrapolateVelocity(velocity, valid_faces, layers, cut_cell_weights=None):
    """mgps_fields_extrapolate3: carries the velocity of the valid faces `layers` faces out, breadth first, in place on the three
    face grids; with `cut_cell_weights` closed faces (weight <= 0) are left out.  Returns (layer_grids, filled): three uint8 face
    grids (0 valid, l = filled by layer l, 255 not reached) and the number of faces filled per axis."""
    shape = list(velocity[0].shape)
    shape[2] -= 1
    faces = _face3(tuple(shape))
    v = [_chk(velocity[a], faces[a], torch.float32) for a in range(3)]
    valid = [_chk(valid_faces[a], faces[a], torch.uint8) for a in range(3)]
    cw = _cw3(cut_cell_weights, faces)
    layer = [torch.empty(fs, dtype=torch.uint8, device=v[0].device) for fs in faces]
    filled = torch.zeros(3, dtype=torch.int64, device=v[0].device)
    check(lib().mgps_fields_extrapolate3(_arr3(v), _arr3(layer), _arr3(valid), _arr3(cw) if cw is not None else None, int(layers), *_g(shape),
                                         _p(filled), _stream()))
    return layer, [int(c) for c in filled.tolist()]


def _halo3(d, halo, dtype):
    """halo = ((lo planes[3] or None), (hi planes[3] or None)) of the three face grids -> two pointer arrays; None where the grid ends"""
    lo, hi = halo if halo is not None else (None, None)
    plane = [(d.gy, d.gx + 1), (d.gy + 1, d.gx), (d.gy, d.gx)]
    for side in (lo, hi):
        if side is not None:
            for a in range(3):
                _chk(side[a], plane[a], dtype)
    assert (lo is not None) == (d.c0 > 0) and (hi is not None) == (d.c1 < d.gz), "halo planes: exactly where the grid goes on"
    return (_arr3(lo) if lo is not None else None), (_arr3(hi) if hi is not None else None)


def extrapolateVelocityLayerSlab(d, l, velocity, layer, valid_faces=None, velocity_halo=None, layer_halo=None, cut_cell_weights=None, filled=None):
    """mgps_fields_slab_extrapolate_layer: layer `l` on the window `d`, in place on `velocity` and `layer` (the window's face grids);
    l = 0 writes `layer` from `valid_faces`.  velocity_halo / layer_halo = (planes below[3] or None, planes above[3] or None): base
    planes c0 - 1 and c1 of the x-face and y-face grids, face planes c0 - 1 and c1 + 1 of the z-face grid.  `filled`: an int64 CUDA
    tensor of 3 counts that the pass raises, or None."""
    faces = _face3(d.base_shape)
    v = [_chk(velocity[a], faces[a], torch.float32) for a in range(3)]
    lay = [_chk(layer[a], faces[a], torch.uint8) for a in range(3)]
    valid = [_chk(valid_faces[a], faces[a], torch.uint8) for a in range(3)] if valid_faces is not None else None
    cw = _cw3(cut_cell_weights, faces)
    if int(l) > 0:
        vlo, vhi = _halo3(d, velocity_halo, torch.float32)
        llo, lhi = _halo3(d, layer_halo, torch.uint8)
    else:
        vlo = vhi = llo = lhi = None
    check(lib().mgps_fields_slab_extrapolate_layer(C.byref(d), int(l), _arr3(v), _arr3(lay), _arr3(valid) if valid is not None else None, vlo, vhi, llo, lhi,
                                                   _arr3(cw) if cw is not None else None, _p(filled), _stream()))
    return layer


class ExtrapolationSlab(C.Structure):
    """mgps_extrapolation_slab (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("gx", C.c_int), ("gy", C.c_int), ("gz", C.c_int), ("power_of_two", C.c_int), ("layers", C.c_int),
        ("velocity", C.c_void_p * 3), ("valid_faces", C.c_void_p * 3), ("cut_weights", C.c_void_p * 3), ("layer", C.c_void_p * 3),
        ("filled", C.c_ulonglong * 3), ("total_ms", C.c_double), ("exchange_ms", C.c_double),
    ]


def extrapolate_velocity_slab(comm, splits, global_shape, velocity, valid_faces, layers, cut_weights=None, power_of_two=True, layer=None):
    """mgps_extrapolate_velocity_slab: the extrapolation on the CUDA tensors of this rank's window of the grid `global_shape` =
    (gz, gy, gx), a collective over the transport `comm`; meant for the velocity and the valid_faces project_free_surface_slab
    returned, with the same `splits`.  `velocity` is updated in place.  `layer`: three uint8 face grids of the window to write, or
    None for new ones.  Returns {"filled": the whole grid's counts per axis, "total_ms", "exchange_ms", "layer"}."""
    d = slab_window(global_shape, power_of_two, splits, comm.rank)
    faces = _face3(d.base_shape)
    ex = ExtrapolationSlab()
    ex.struct_size = C.sizeof(ExtrapolationSlab)
    ex.gz, ex.gy, ex.gx = global_shape
    ex.power_of_two, ex.layers = int(bool(power_of_two)), int(layers)
    if layer is None:
        layer = [torch.empty(fs, dtype=torch.uint8, device=velocity[0].device) for fs in faces]
    for a in range(3):
        ex.velocity[a] = _chk(velocity[a], faces[a], torch.float32).data_ptr()
        ex.valid_faces[a] = _chk(valid_faces[a], faces[a], torch.uint8).data_ptr()
        ex.layer[a] = _chk(layer[a], faces[a], torch.uint8).data_ptr()
        # (a missing entry stays NULL: the library refuses "some but not all" on every rank together)
        ex.cut_weights[a] = _chk(cut_weights[a], faces[a], torch.float32).data_ptr() if cut_weights is not None and cut_weights[a] is not None else None
    cuts = (C.c_int * len(splits))(*[int(v) for v in splits])
    check(lib().mgps_extrapolate_velocity_slab(C.byref(ex), C.byref(comm.struct), cuts, _stream()))
    return {"filled": [int(ex.filled[a]) for a in range(3)], "total_ms": ex.total_ms, "exchange_ms": ex.exchange_ms, "layer": layer}


# ---- pressure feedback: force and torque of the pressure on solid bodies (include/mgps_fields.h) ----------------
def _centres(centres):
    """(bodies + 1, 3) float64 host array (row 0: the point the unowned faces' torque refers to) -> (array, bodies)"""
    import numpy as np

    c = np.ascontiguousarray(centres, dtype=np.float64)
    assert c.ndim == 2 and c.shape[1] == 3 and c.shape[0] >= 2, c.shape
    return c, c.shape[0] - 1


def solidForces(pressure, material, cut_cell_weights, body, centres, scale=1.0):
    """mgps_fields_solid_forces: the net force and torque of `pressure` on the closed part of the cut faces, per body.  `body`: three
    int32 face grids of body ids (1 .. bodies; anything else counts for row 0); `centres`: (bodies + 1, 3) host array of x, y, z in
    cell units.  Returns a (bodies + 1, 8) float64 numpy array: force[3], torque[3] (both times `scale`), wet closed area, wet faces."""
    import numpy as np

    shape = tuple(material.shape)
    faces = _face3(shape)
    cw = [_chk(cut_cell_weights[a], faces[a], torch.float32) for a in range(3)]
    ids = [_chk(body[a], faces[a], torch.int32) for a in range(3)]
    c, bodies = _centres(centres)
    out = np.zeros((bodies + 1, 8), dtype=np.float64)
    check(lib().mgps_fields_solid_forces(out.ctypes.data_as(C.c_void_p), _p(_chk(pressure, shape, torch.float32)), _p(_chk(material, shape, torch.int32)),
                                         _p(cw[0]), _p(cw[1]), _p(cw[2]), _p(ids[0]), _p(ids[1]), _p(ids[2]), c.ctypes.data_as(C.c_void_p),
                                         int(bodies), C.c_double(scale), *_g(shape), _stream()))
    return out


def solidForcesSlab(d, pressure, pressure_lo, material, material_lo, cut_cell_weights, body, centres, scale=1.0):
    """mgps_fields_slab_solid_forces: this rank's rows on the window `d` (the caller adds the ranks').  pressure_lo / material_lo: base
    plane c0 - 1 (None at c0 == 0); cut_cell_weights / body: the window's face grids."""
    import numpy as np

    shape = d.base_shape
    faces = _face3(shape)
    cw = [_chk(cut_cell_weights[a], faces[a], torch.float32) for a in range(3)]
    ids = [_chk(body[a], faces[a], torch.int32) for a in range(3)]
    for t, dtype in ((pressure_lo, torch.float32), (material_lo, torch.int32)):
        if t is not None:
            _chk(t, (d.gy, d.gx), dtype)
    c, bodies = _centres(centres)
    out = np.zeros((bodies + 1, 8), dtype=np.float64)
    check(lib().mgps_fields_slab_solid_forces(C.byref(d), out.ctypes.data_as(C.c_void_p), _p(_chk(pressure, shape, torch.float32)), _p(pressure_lo),
                                              _p(_chk(material, shape, torch.int32)), _p(material_lo), _arr3(cw), _arr3(ids),
                                              c.ctypes.data_as(C.c_void_p), int(bodies), C.c_double(scale), _stream()))
    return out


class SolidForcesSlab(C.Structure):
    """struct mgps_solid_forces_slab (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("gx", C.c_int), ("gy", C.c_int), ("gz", C.c_int), ("power_of_two", C.c_int), ("bodies", C.c_int),
        ("pressure", C.c_void_p), ("liquid_phi", C.c_void_p), ("solid_phi", C.c_void_p), ("cut_weights", C.c_void_p * 3), ("body", C.c_void_p * 3),
        ("centres", C.c_void_p), ("scale", C.c_double), ("out", C.c_void_p), ("total_ms", C.c_double), ("exchange_ms", C.c_double),
    ]


def solid_forces_slab(comm, splits, global_shape, pressure, liquid_phi, solid_phi, cut_weights, body, centres, scale=1.0, power_of_two=True):
    """mgps_solid_forces_slab: the forces on the CUDA tensors of this rank's window of the grid `global_shape` = (gz, gy, gx), a
    collective over the transport `comm`; meant for the fields project_free_surface_slab took and the pressure it published, with the
    same `splits`.  Returns {"rows": (bodies + 1, 8) float64 array of the whole grid's numbers, "total_ms", "exchange_ms"}."""
    import numpy as np

    d = slab_window(global_shape, power_of_two, splits, comm.rank)
    shape = d.base_shape
    faces = _face3(shape)
    c, bodies = _centres(centres)
    out = np.zeros((bodies + 1, 8), dtype=np.float64)
    sf = SolidForcesSlab()
    sf.struct_size = C.sizeof(SolidForcesSlab)
    sf.gz, sf.gy, sf.gx = global_shape
    sf.power_of_two, sf.bodies = int(bool(power_of_two)), int(bodies)
    sf.pressure = _chk(pressure, shape, torch.float32).data_ptr()
    sf.liquid_phi, sf.solid_phi = _chk(liquid_phi, shape, torch.float32).data_ptr(), _chk(solid_phi, shape, torch.float32).data_ptr()
    for a in range(3):
        sf.cut_weights[a] = _chk(cut_weights[a], faces[a], torch.float32).data_ptr()
        # (a missing entry stays NULL: the library carries the refusal to every rank)
        sf.body[a] = _chk(body[a], faces[a], torch.int32).data_ptr() if body[a] is not None else None
    sf.centres, sf.scale, sf.out = c.ctypes.data, float(scale), out.ctypes.data
    cuts = (C.c_int * len(splits))(*[int(v) for v in splits])
    check(lib().mgps_solid_forces_slab(C.byref(sf), C.byref(comm.struct), cuts, _stream()))
    return {"rows": out, "total_ms": sf.total_ms, "exchange_ms": sf.exchange_ms}


# ---- two-way rigid-body coupling: body velocities solved with the pressure (include/mgps_fields.h) ------------
def _table(a, bodies, cols, what):
    """a host table with one row per body, row 0 included: (bodies + 1, cols) float64"""
    import numpy as np

    t = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, cols) if cols > 1 else np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    assert t.shape[0] == bodies + 1, (what, t.shape, bodies)
    return t


def rigidVelocity(solid_velocity, body, centres, motions):
    """mgps_fields_rigid_velocity (in place on the three solid-velocity face grids): (U_r + omega_r x (x_f - centres[r]))_a on the faces
    whose body id is 1 .. bodies; every other face keeps its value.  `motions`: (bodies + 1, 6) host array, U then omega per row."""
    shape = list(solid_velocity[2].shape)
    shape[0] -= 1
    faces = _face3(tuple(shape))
    sv = [_chk(solid_velocity[a], faces[a], torch.float32) for a in range(3)]
    ids = [_chk(body[a], faces[a], torch.int32) for a in range(3)]
    c, bodies = _centres(centres)
    m = _table(motions, bodies, 6, "motions")
    check(lib().mgps_fields_rigid_velocity(_p(sv[0]), _p(sv[1]), _p(sv[2]), _p(ids[0]), _p(ids[1]), _p(ids[2]), c.ctypes.data_as(C.c_void_p),
                                           m.ctypes.data_as(C.c_void_p), int(bodies), *_g(tuple(shape)), _stream()))
    return solid_velocity


def rigidVelocitySlab(d, solid_velocity, body, centres, motions):
    """mgps_fields_slab_rigid_velocity: rigidVelocity on the window `d` (in place on the window's three face grids; positions use the
    whole grid's plane index): the bits of the whole-grid pass on the rank's planes.  No communication."""
    faces = _face3(d.base_shape)
    sv = [_chk(solid_velocity[a], faces[a], torch.float32) for a in range(3)]
    ids = [_chk(body[a], faces[a], torch.int32) for a in range(3)]
    c, bodies = _centres(centres)
    m = _table(motions, bodies, 6, "motions")
    check(lib().mgps_fields_slab_rigid_velocity(C.byref(d), _arr3(sv), _arr3(ids), c.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p),
                                                int(bodies), _stream()))
    return solid_velocity


class CouplingDesc(C.Structure):
    """mgps_coupling_desc (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("gx", C.c_int), ("gy", C.c_int), ("gz", C.c_int),
        ("ex", C.c_int), ("ey", C.c_int), ("ez", C.c_int), ("offset", C.c_int), ("bodies", C.c_int),
        ("material", C.c_void_p), ("cut_weights", C.c_void_p * 3), ("body", C.c_void_p * 3),
        ("centres", C.c_void_p), ("inv_mass", C.c_void_p), ("inv_inertia", C.c_void_p),
    ]


class RigidCoupling:
    """mgps_coupling: the operator G K G^T of the bodies `body` / `centres` / `inv_mass` (bodies + 1) / `inv_inertia` (bodies + 1, 6:
    xx, yy, zz, xy, xz, yz) on the coupled cells of the base grids, for expanded grids of `expanded_shape` at `offset`.

    RigidCoupling.on_slab makes the object of one rank of a slab run: its list holds the rank's own coupled cells, its grids are the
    rank's windows, and apply, impulses and velocities are collectives (every rank calls them together)."""

    def __init__(self, material, cut_cell_weights, body, centres, inv_mass, inv_inertia, expanded_shape, offset):
        shape = tuple(material.shape)
        d, keep = self._desc(shape, shape, expanded_shape, offset, material, cut_cell_weights, body, centres, inv_mass, inv_inertia)
        self.h = C.c_void_p()
        check(lib().mgps_coupling_create(C.byref(self.h), C.byref(d), _stream()))
        self.bodies, self.expanded_shape, self.offset, self.device = d.bodies, tuple(expanded_shape), int(offset), material.device
        self.comm = None

    @staticmethod
    def _desc(grid_shape, array_shape, expanded_shape, offset, material, cut_cell_weights, body, centres, inv_mass, inv_inertia):
        """the desc of the grid `grid_shape` / `expanded_shape` over arrays of `array_shape` (the grid's, or a window's), and what
        must stay alive while the library reads it"""
        faces = _face3(array_shape)
        c, bodies = _centres(centres)
        im, ii = _table(inv_mass, bodies, 1, "inv_mass"), _table(inv_inertia, bodies, 6, "inv_inertia")
        d = CouplingDesc()
        d.struct_size = C.sizeof(CouplingDesc)
        d.gz, d.gy, d.gx = grid_shape
        d.ez, d.ey, d.ex = expanded_shape
        d.offset, d.bodies = int(offset), int(bodies)
        d.material = _chk(material, array_shape, torch.int32).data_ptr()
        for a in range(3):
            d.cut_weights[a] = _chk(cut_cell_weights[a], faces[a], torch.float32).data_ptr()
            d.body[a] = _chk(body[a], faces[a], torch.int32).data_ptr()
        d.centres, d.inv_mass, d.inv_inertia = c.ctypes.data, im.ctypes.data, ii.ctypes.data
        return d, (c, im, ii)

    @classmethod
    def on_slab(cls, d, comm, material, cut_cell_weights, body, centres, inv_mass, inv_inertia):
        """mgps_coupling_create_slab: the coupling of the rank whose window is `d` (fields.slab_window) over the transport `comm`;
        material / cut_cell_weights / body: the window's grids.  No communication here; `comm` is kept alive with the object.  Its
        expanded grids are the rank's d.expanded_shape planes: the grids of the rank's SlabSolver."""
        desc, keep = cls._desc((d.gz, d.gy, d.gx), d.base_shape, (d.ez, d.ey, d.ex), d.offset, material, cut_cell_weights, body, centres, inv_mass, inv_inertia)
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        check(lib().mgps_coupling_create_slab(C.byref(self.h), C.byref(desc), C.byref(d), C.byref(comm.struct), _stream()))
        self.bodies, self.expanded_shape, self.offset, self.device = desc.bodies, tuple(d.expanded_shape), int(d.offset), material.device
        self.comm, self.window = comm, d
        return self

    def close(self):
        if getattr(self, "h", None):
            lib().mgps_coupling_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _x(self, t):
        return _p(_chk(t, self.expanded_shape, torch.float32))

    def set_bodies(self, centres, inv_mass, inv_inertia):
        c, bodies = _centres(centres)
        assert bodies == self.bodies
        im, ii = _table(inv_mass, bodies, 1, "inv_mass"), _table(inv_inertia, bodies, 6, "inv_inertia")
        check(lib().mgps_coupling_set_bodies(self.h, c.ctypes.data_as(C.c_void_p), im.ctypes.data_as(C.c_void_p), ii.ctypes.data_as(C.c_void_p), _stream()))

    def cells(self):
        """the coupled cells of the list (on a slab: the rank's own)"""
        n = C.c_int64()
        check(lib().mgps_coupling_cells(self.h, C.byref(n)))
        return n.value

    def apply(self, y, x):
        """y += G K G^T x on the coupled cells (expanded float32 grids), in place on y.  On a slab coupling a collective: every
        rank calls it with its window of x and y, and one all-reduce sums the impulses over the ranks"""
        check(lib().mgps_coupling_apply(self.h, self._x(y), self._x(x), _stream()))
        return y

    def impulses(self, x):
        """(bodies + 1, 6) float64: (F, T) = - G^T x per row at scale 1, row 0 zero.  On a slab coupling a collective (one
        all-reduce): the whole grid's numbers, the same bits on every rank"""
        import numpy as np

        out = np.zeros((self.bodies + 1, 6), dtype=np.float64)
        check(lib().mgps_coupling_impulses(self.h, self._x(x), out.ctypes.data_as(C.c_void_p), _stream()))
        return out

    def velocities(self, x, motions):
        """(V_out, impulses): V_out = motions + K (F, T)(x), both (bodies + 1, 6) float64.  On a slab coupling a collective (one
        all-reduce): the whole grid's numbers, the same bits on every rank"""
        import numpy as np

        m = _table(motions, self.bodies, 6, "motions")
        out, imp = np.zeros_like(m), np.zeros_like(m)
        check(lib().mgps_coupling_velocities(self.h, self._x(x), m.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                             imp.ctypes.data_as(C.c_void_p), _stream()))
        return out, imp


def project_free_surface_rigid(liquid_phi, solid_phi, cut_weights, velocity, pressure, body, centres, inv_mass, inv_inertia, motions,
                               solid_velocity=None, use_old_pressure=True, use_mg_preconditioner=True, use_gauss_seidel=True, tolerance=1e-5,
                               max_iterations=2500, power_of_two=True, options=None):
    """The free-surface projection with rigid bodies the liquid moves, composed from the device passes on CUDA tensors: material
    labels, valid faces, MG domain, rigidVelocity(V*) + buildRHS, solver from the device labels, the coupled solve (A + G K G^T) p =
    b_fluid + G V*, pressure write-back and gradient.  `velocity` and `pressure` are updated in place; `solid_velocity` (or zeros)
    supplies the faces no body owns and is left untouched.  `motions` = V*: (bodies + 1, 6), U then omega per row.
    Returns {"pressure", "velocity", "motions": V_out = V* + K (F, T)(p), "impulses", "stats", "material", "valid_faces", "solid_velocity":
    the rigid velocity of V*, "offset", "expanded", "coupled_cells"}."""
    from . import solver as S

    shape = tuple(liquid_phi.shape)
    faces = _face3(shape)
    material = buildMaterialCellLabels(liquid_phi, solid_phi, cut_weights)
    valid = buildValidFaces(material, cut_weights)
    eshape, offset, levels = S.expanded_layout(shape, 0, power_of_two)
    labels, weights = buildMGDomain(material, cut_weights, liquid_phi, valid, eshape, offset)
    if solid_velocity is not None:
        sv = [_chk(solid_velocity[a], faces[a], torch.float32).clone() for a in range(3)]
    else:
        sv = [torch.zeros(faces[a], dtype=torch.float32, device=material.device) for a in range(3)]
    rigidVelocity(sv, body, centres, motions)
    rhs = buildRHS(material, velocity, cut_weights, eshape, offset, sv)
    x = applyOldPressure(pressure, material, eshape, offset) if use_old_pressure else torch.zeros(eshape, dtype=torch.float32, device=material.device)
    mg = S.GeometricMultigridPoissonSolver(labels, weights, levels, use_gauss_seidel, options=options)
    coupling = RigidCoupling(material, cut_weights, body, centres, inv_mass, inv_inertia, eshape, offset)
    try:
        stats = mg.solve_pcg_coupled(coupling, x, rhs, tolerance, max_iterations, use_mg_preconditioner)
        applySolutionToPressure(pressure, x, material, offset)
        applyPressureGradient(velocity, liquid_phi, pressure, valid, material)
        v_out, impulses = coupling.velocities(x, motions)
        cells = coupling.cells()
    finally:
        coupling.close()
        mg.close()
    return {"pressure": pressure, "velocity": velocity, "motions": v_out, "impulses": impulses, "stats": stats, "material": material,
            "valid_faces": valid, "solid_velocity": sv, "offset": offset, "expanded": eshape, "coupled_cells": cells}


class ProjectionRigidSlab(C.Structure):
    """mgps_projection_rigid_slab (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("projection", C.POINTER(ProjectionSlab)), ("bodies", C.c_int), ("body", C.c_void_p * 3),
        ("centres", C.c_void_p), ("inv_mass", C.c_void_p), ("inv_inertia", C.c_void_p), ("motions", C.c_void_p),
        ("solid_velocity_out", C.c_void_p * 3), ("motions_out", C.c_void_p), ("impulses", C.c_void_p),
        ("coupled_cells", C.c_int64), ("coupled_cells_rank", C.c_int64),
    ]


def project_free_surface_rigid_slab(comm, splits, global_shape, liquid_phi, solid_phi, cut_weights, velocity, pressure, body, centres, inv_mass,
                                    inv_inertia, motions, solid_velocity=None, solid_velocity_out=None, use_old_pressure=True,
                                    use_mg_preconditioner=True, use_gauss_seidel=True, tolerance=1e-5, max_iterations=2500, power_of_two=True,
                                    options=None, surface_tension=0.0, dt=0.0, dx=0.0, density=0.0, surface_pressure=None):
    """mgps_project_free_surface_rigid_slab: project_free_surface_slab with rigid bodies the liquid moves, a collective over `comm` (a
    world of one is the device-resident coupled projection on one GPU).  The fields are those of project_free_surface_slab; `body`:
    the window's three int32 face grids of body ids; `centres`, `inv_mass`, `inv_inertia`, `motions` (V*): the host tables of
    RigidCoupling and rigidVelocity, the same on every rank.  `solid_velocity` (or zeros) supplies the faces no body owns and is left
    untouched; `solid_velocity_out` (three float32 face grids of the window, or None) receives the solid velocity the projected
    velocity is divergence free against: `solid_velocity` with V_out on the bodies' faces.  `velocity` and `pressure` are updated in
    place.  Returns (valid_faces, info): the info of project_free_surface_slab plus "motions" (V_out) and "impulses", (bodies + 1, 6)
    float64 arrays with the same bits on every rank, "coupled_cells" (the whole grid's) and "coupled_cells_rank"."""
    import numpy as np

    d = slab_window(global_shape, power_of_two, splits, comm.rank)
    faces = _face3(d.base_shape)
    pr, valid = _projection_slab(d, global_shape, liquid_phi, solid_phi, cut_weights, velocity, pressure, solid_velocity, use_old_pressure,
                                 use_mg_preconditioner, use_gauss_seidel, tolerance, max_iterations, power_of_two, surface_tension, dt, dx, density,
                                 surface_pressure)
    c, bodies = _centres(centres)
    im, ii, m = _table(inv_mass, bodies, 1, "inv_mass"), _table(inv_inertia, bodies, 6, "inv_inertia"), _table(motions, bodies, 6, "motions")
    v_out, impulses = np.zeros_like(m), np.zeros_like(m)
    rg = ProjectionRigidSlab()
    rg.struct_size = C.sizeof(ProjectionRigidSlab)
    rg.projection = C.pointer(pr)
    rg.bodies = int(bodies)
    for a in range(3):
        # (a missing entry stays NULL: the library carries the refusal to every rank)
        rg.body[a] = _chk(body[a], faces[a], torch.int32).data_ptr() if body[a] is not None else None
        rg.solid_velocity_out[a] = _chk(solid_velocity_out[a], faces[a], torch.float32).data_ptr() if solid_velocity_out is not None else None
    rg.centres, rg.inv_mass, rg.inv_inertia, rg.motions = c.ctypes.data, im.ctypes.data, ii.ctypes.data, m.ctypes.data
    rg.motions_out, rg.impulses = v_out.ctypes.data, impulses.ctypes.data
    cuts = (C.c_int * len(splits))(*[int(v) for v in splits])
    status = lib().mgps_project_free_surface_rigid_slab(C.byref(rg), C.byref(options) if options is not None else None, C.byref(comm.struct), cuts,
                                                        _stream())
    info = _projection_slab_info(pr, d)
    info.update(motions=v_out, impulses=impulses, coupled_cells=rg.coupled_cells, coupled_cells_rank=rg.coupled_cells_rank)
    try:
        check(status)
    except _lib.MgpsError as e:  # (interrupted: pressure, velocity, motions and impulses are those of the iterate handed back)
        e.info, e.valid_faces = info, valid
        raise
    return valid, info


# ---- rigid bodies rasterised on the device (include/mgps_fields.h) ---------------------------------------------
BODY_SPHERE, BODY_BOX, BODY_GRID = 0, 1, 2


class BodyShape(C.Structure):
    """mgps_body_shape: kind, pose (centre, rotation body -> world) and extent of one rigid body; lengths in cells from the grid's
    corner, arrays in (x, y, z) order.  Make one with BodyShape.sphere, BodyShape.box, BodyShape.sdf_grid or BodyShape.mesh (below)."""

    _fields_ = [
        ("kind", C.c_int), ("centre", C.c_double * 3), ("rotation", C.c_double * 9), ("half", C.c_double * 3), ("sdf", C.c_void_p),
        ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("origin", C.c_double * 3), ("spacing", C.c_double),
    ]

    @classmethod
    def _posed(cls, kind, centre, rotation):
        s = cls()
        s.kind = kind
        s.centre[:] = [float(v) for v in centre]
        rot = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0) if rotation is None else [float(v) for row in rotation for v in row]
        s.rotation[:] = rot
        return s

    @classmethod
    def sphere(cls, centre, radius):
        s = cls._posed(BODY_SPHERE, centre, None)
        s.half[0] = float(radius)
        return s

    @classmethod
    def box(cls, centre, half, rotation=None):
        """`rotation`: 3 x 3 rows, body -> world (None: the identity)"""
        s = cls._posed(BODY_BOX, centre, rotation)
        s.half[:] = [float(v) for v in half]
        return s

    @classmethod
    def sdf_grid(cls, centre, sdf, origin, spacing, rotation=None):
        """`sdf`: a CUDA float32 tensor (nz, ny, nx) of body-frame samples, negative inside, in cells; sample (0, 0, 0) sits at the
        body-frame position `origin`, the samples are `spacing` cells apart.  The tensor is kept alive with the shape."""
        s = cls._posed(BODY_GRID, centre, rotation)
        assert sdf.is_cuda and sdf.is_contiguous() and sdf.dtype == torch.float32 and sdf.dim() == 3, (sdf.shape, sdf.dtype)
        s.nz, s.ny, s.nx = (int(v) for v in sdf.shape)
        s.sdf, s._keep = sdf.data_ptr(), sdf
        s.origin[:] = [float(v) for v in origin]
        s.spacing = float(spacing)
        return s

    @classmethod
    def mesh(cls, centre, vertices, triangles, spacing, band, rotation=None, vertex_velocities=None):
        """The GRID shape of a closed triangle mesh given in the body frame: sizes the sample box
        (meshSampleBox), samples the signed distance on the device (meshSDF) and keeps the tensor alive, as sdf_grid does.  For a
        rasteriser band of B cells give band >= B + sqrt(3) * spacing.  `.mass_properties`: (volume, centre, inertia) of
        meshMassProperties, for unit density in the body frame.
        `vertex_velocities` ((V, 3), body frame, cells per step): a deforming collider.  The samples come
        from meshSDFVelocity and `.velocity`, the (3, nz, ny, nx) velocity samples sampledVelocity reads, is kept alive with the
        shape."""
        n, origin = meshSampleBox(vertices, spacing, band)
        if vertex_velocities is None:
            s = cls.sdf_grid(centre, meshSDF(vertices, triangles, n, origin, spacing, band), origin, spacing, rotation)
        else:
            sdf, vel = meshSDFVelocity(vertices, triangles, vertex_velocities, n, origin, spacing, band)
            s = cls.sdf_grid(centre, sdf, origin, spacing, rotation)
            s.velocity = vel
        s.mass_properties = meshMassProperties(vertices, triangles)
        return s


class RasterDesc(C.Structure):
    """mgps_raster_desc (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("gx", C.c_int), ("gy", C.c_int), ("gz", C.c_int), ("bodies", C.c_int), ("shapes", C.POINTER(BodyShape)),
        ("band", C.c_double), ("min_open", C.c_double), ("static_solid_phi", C.c_void_p), ("static_cut_weights", C.c_void_p * 3),
        ("solid_phi", C.c_void_p), ("cut_weights", C.c_void_p * 3), ("body", C.c_void_p * 3),
    ]


def _raster(entry, window, grid_shape, array_shape, shapes, band, min_open, static_solid_phi, static_cut_weights):
    faces = _face3(array_shape)
    device = static_solid_phi.device if static_solid_phi is not None else _current_device()
    rows = (BodyShape * (len(shapes) + 1))(BodyShape(), *shapes)  # (row 0 is not read)
    d = RasterDesc()
    d.struct_size = C.sizeof(RasterDesc)
    d.gz, d.gy, d.gx = grid_shape
    d.bodies, d.shapes, d.band, d.min_open = len(shapes), rows, float(band), float(min_open)
    if static_solid_phi is not None:
        d.static_solid_phi = _chk(static_solid_phi, array_shape, torch.float32).data_ptr()
    if static_cut_weights is not None:
        for a in range(3):
            d.static_cut_weights[a] = _chk(static_cut_weights[a], faces[a], torch.float32).data_ptr()
    solid_phi = torch.empty(array_shape, dtype=torch.float32, device=device)
    cut_weights = [torch.empty(faces[a], dtype=torch.float32, device=device) for a in range(3)]
    body = [torch.empty(faces[a], dtype=torch.int32, device=device) for a in range(3)]
    d.solid_phi = solid_phi.data_ptr()
    for a in range(3):
        d.cut_weights[a], d.body[a] = cut_weights[a].data_ptr(), body[a].data_ptr()
    with torch.cuda.device(device):
        check(entry(C.byref(d), _stream()) if window is None else entry(C.byref(window), C.byref(d), _stream()))
    return solid_phi, cut_weights, body


def rasterizeBodies(shape, shapes, band=3.0, min_open=0.0, static_solid_phi=None, static_cut_weights=None):
    """mgps_fields_rasterize_bodies: the solid SDF, the three cut-weight face grids and the three int32 body-id face grids of the
    rigid bodies `shapes` (a list of BodyShape: body r is shapes[r - 1]) on the grid `shape` = (gz, gy, gx), merged with the static
    solids' grids where given (read, never written).  Returns (solid_phi, cut_weights, body): new CUDA tensors, what
    project_free_surface_rigid, RigidCoupling and solidForces take.  Does not synchronise."""
    return _raster(lib().mgps_fields_rasterize_bodies, None, tuple(shape), tuple(shape), shapes, band, min_open, static_solid_phi, static_cut_weights)


def rasterizeBodiesSlab(d, shapes, band=3.0, min_open=0.0, static_solid_phi=None, static_cut_weights=None):
    """mgps_fields_slab_rasterize_bodies: rasterizeBodies on the window `d` (fields.slab_window): the window's grids (z-faces
    c0 .. c1) with the bits of the whole-grid pass on the rank's planes.  No halo, no communication."""
    return _raster(lib().mgps_fields_slab_rasterize_bodies, d, (d.gz, d.gy, d.gx), d.base_shape, shapes, band, min_open, static_solid_phi,
                   static_cut_weights)


# ---- triangle-mesh rigid bodies (include/mgps_fields.h) --------------------------------------------------------
class MeshDesc(C.Structure):
    """mgps_mesh_desc (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("vertices", C.c_int), ("triangles", C.c_int), ("xyz", C.c_void_p), ("tri", C.c_void_p),
        ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("origin", C.c_double * 3), ("spacing", C.c_double), ("band", C.c_double),
        ("sdf", C.c_void_p),
    ]


class MassProperties(C.Structure):
    """mgps_mass_properties (include/mgps_fields.h)."""

    _fields_ = [("volume", C.c_double), ("centre", C.c_double * 3), ("inertia", C.c_double * 9)]


def _mesh(vertices, triangles):
    import numpy as np

    v = np.ascontiguousarray(vertices, dtype=np.float64)
    t = np.ascontiguousarray(triangles, dtype=np.int32)
    assert v.ndim == 2 and v.shape[1] == 3 and t.ndim == 2 and t.shape[1] == 3, (v.shape, t.shape)
    return v, t


def _mesh_desc(cls, v, t, n, origin, spacing, band):
    """(desc of class `cls` with the mesh and the sample box filled in, the shape (nz, ny, nx) to allocate the outputs with)"""
    d = cls()
    d.struct_size = C.sizeof(cls)
    d.vertices, d.triangles, d.xyz, d.tri = len(v), len(t), v.ctypes.data, t.ctypes.data
    d.nx, d.ny, d.nz = (int(q) for q in n)
    d.origin[:] = [float(q) for q in origin]
    d.spacing, d.band = float(spacing), float(band)
    nx, ny, nz = (min(max(int(q), 1), 1024) for q in n)  # (the library refuses a dimension outside 2 .. 1024 before it writes)
    return d, (nz, ny, nx)


def meshSDF(vertices, triangles, n, origin, spacing, band, device=None):
    """mgps_fields_mesh_sdf: the body-frame signed distance of the closed mesh (`vertices` (V, 3) float64 in (x, y, z), `triangles`
    (T, 3) vertex indices, outward orientation) at the samples origin + spacing (i, j, k), `n` = (nx, ny, nz) of them: a CUDA float32
    tensor (nz, ny, nx), negative inside, exact up to `band` and clamped there.  What BodyShape.sdf_grid takes.  Does not synchronise."""
    v, t = _mesh(vertices, triangles)
    device = _current_device() if device is None else torch.device(device)
    d, shape = _mesh_desc(MeshDesc, v, t, n, origin, spacing, band)
    sdf = torch.empty(shape, dtype=torch.float32, device=device)
    d.sdf = sdf.data_ptr()
    with torch.cuda.device(device):
        check(lib().mgps_fields_mesh_sdf(C.byref(d), _stream()))
    return sdf


def meshMassProperties(vertices, triangles):
    """mgps_mesh_mass_properties: (volume, centre (3,), inertia (3, 3) about the centre) of the closed mesh for unit density, in the
    body frame, in cells.  Host only."""
    import numpy as np

    v, t = _mesh(vertices, triangles)
    m = MassProperties()
    check(lib().mgps_mesh_mass_properties(len(v), len(t), v.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), C.byref(m)))
    return m.volume, np.array(m.centre[:]), np.array(m.inertia[:]).reshape(3, 3)


def meshSampleBox(vertices, spacing, band):
    """mgps_mesh_sample_box: ((nx, ny, nz), origin (3,)) of the samples that hold the mesh's bounding box grown by band + spacing"""
    import numpy as np

    v = np.ascontiguousarray(vertices, dtype=np.float64)
    n, origin = (C.c_int * 3)(), (C.c_double * 3)()
    check(lib().mgps_mesh_sample_box(len(v), v.ctypes.data_as(C.c_void_p), C.c_double(spacing), C.c_double(band), n, origin))
    return tuple(n[:]), np.array(origin[:])


# ---- deforming mesh colliders: vertex velocities to the solid-velocity grids (include/mgps_fields.h) ----------
class MeshVelocityDesc(C.Structure):
    """mgps_mesh_velocity_desc (include/mgps_fields.h): mgps_mesh_desc's fields, then the vertex velocities and the outputs."""

    _fields_ = MeshDesc._fields_ + [("velocity", C.c_void_p), ("vel", C.c_void_p * 3)]


class BodyVelocity(C.Structure):
    """mgps_body_velocity (include/mgps_fields.h)."""

    _fields_ = [("vel", C.c_void_p * 3), ("motion", C.c_double * 6)]


def meshSDFVelocity(vertices, triangles, vertex_velocities, n, origin, spacing, band, device=None):
    """mgps_fields_mesh_sdf_velocity: (sdf, vel) of a deforming closed mesh at the samples of meshSDF.  `sdf` holds meshSDF's bits;
    `vel` is a CUDA float32 tensor (3, nz, ny, nx): the vertex velocities (`vertex_velocities` (V, 3) float64, body frame, cells per
    step) interpolated at the closest point of the mesh, 0 where the distance is not below `band`.  Does not synchronise."""
    import numpy as np

    v, t = _mesh(vertices, triangles)
    w = np.ascontiguousarray(vertex_velocities, dtype=np.float64)
    assert w.shape == v.shape, (w.shape, v.shape)
    device = _current_device() if device is None else torch.device(device)
    d, shape = _mesh_desc(MeshVelocityDesc, v, t, n, origin, spacing, band)
    d.velocity = w.ctypes.data
    sdf = torch.empty(shape, dtype=torch.float32, device=device)
    vel = torch.empty((3,) + shape, dtype=torch.float32, device=device)
    d.sdf = sdf.data_ptr()
    for c in range(3):
        d.vel[c] = vel[c].data_ptr()
    with torch.cuda.device(device):
        check(lib().mgps_fields_mesh_sdf_velocity(C.byref(d), _stream()))
    return sdf, vel


def _sampled_rows(shapes, frame_motions):
    """(shape rows, velocity rows, what keeps them alive) of `shapes` (body r is shapes[r - 1]); row 0 is not read"""
    import numpy as np

    bodies = len(shapes)
    motions = np.zeros((bodies, 6)) if frame_motions is None else np.ascontiguousarray(frame_motions, dtype=np.float64).reshape(-1, 6)
    assert motions.shape[0] == bodies, (motions.shape, bodies)
    rows = (BodyShape * (bodies + 1))(BodyShape(), *shapes)
    vrows = (BodyVelocity * (bodies + 1))()
    for r, s in enumerate(shapes, start=1):
        vel = getattr(s, "velocity", None)
        if vel is not None:
            assert vel.is_cuda and vel.dtype == torch.float32 and tuple(vel.shape) == (3, s.nz, s.ny, s.nx), (vel.shape, vel.dtype)
            for c in range(3):
                assert vel[c].is_contiguous()
                vrows[r].vel[c] = vel[c].data_ptr()
        vrows[r].motion[:] = [float(q) for q in motions[r - 1]]
    return rows, vrows


def _sampled_velocity(d, shape, solid_velocity, body, shapes, frame_motions):
    """both forms on arrays of `shape`: the whole grid's (d None) or the window d's"""
    faces = _face3(shape)
    sv = [_chk(solid_velocity[a], faces[a], torch.float32) for a in range(3)]
    ids = [_chk(body[a], faces[a], torch.int32) for a in range(3)]
    rows, vrows = _sampled_rows(shapes, frame_motions)
    with torch.cuda.device(sv[0].device):
        if d is None:
            check(lib().mgps_fields_sampled_velocity(_arr3(sv), _arr3(ids), len(shapes), rows, vrows, *_g(shape), _stream()))
        else:
            check(lib().mgps_fields_slab_sampled_velocity(C.byref(d), _arr3(sv), _arr3(ids), len(shapes), rows, vrows, _stream()))
    return solid_velocity


def sampledVelocity(solid_velocity, body, shapes, frame_motions=None):
    """mgps_fields_sampled_velocity (in place on the three solid-velocity face grids): on the faces whose body id r is in
    1 .. len(shapes) and whose shape (shapes[r - 1], made by BodyShape.mesh with vertex_velocities) carries `.velocity`, the body's
    velocity samples interpolated at the face, turned into the world frame, plus the motion of the body frame (`frame_motions`:
    (len(shapes), 6) host array, U then omega per body, about the shape's centre; None: at rest).  Every other face keeps its
    value: call rigidVelocity first and this after it.  Does not synchronise."""
    shape = list(solid_velocity[2].shape)
    shape[0] -= 1
    return _sampled_velocity(None, tuple(shape), solid_velocity, body, shapes, frame_motions)


def sampledVelocitySlab(d, solid_velocity, body, shapes, frame_motions=None):
    """mgps_fields_slab_sampled_velocity: sampledVelocity on the window `d` (in place on the window's three face grids; positions use
    the whole grid's plane index): the bits of the whole-grid pass on the rank's planes.  No halo, no communication."""
    return _sampled_velocity(d, d.base_shape, solid_velocity, body, shapes, frame_motions)


# ---- advection: semi-Lagrangian and MacCormack passes (include/mgps_fields.h) ----------------------------------
SCHEMES = {"semi_lagrangian": 0, "maccormack": 1}


class AdvectDesc(C.Structure):
    """mgps_advect_desc (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("gx", C.c_int), ("gy", C.c_int), ("gz", C.c_int), ("dt", C.c_double), ("scheme", C.c_int),
        ("trace_order", C.c_int), ("velocity_in", C.c_void_p * 3), ("velocity_out", C.c_void_p * 3), ("velocity_scratch", C.c_void_p * 3),
        ("scalars", C.c_int), ("scalar_in", C.c_void_p * 4), ("scalar_out", C.c_void_p * 4), ("scalar_scratch", C.c_void_p * 4),
        ("counts_dev", C.c_void_p),
    ]


def _counts_ptr(counts):
    """the counts_dev of a desc: an int64 CUDA tensor of 2 that the pass adds to, or None"""
    assert counts is None or (counts.is_cuda and counts.dtype == torch.int64 and counts.numel() == 2 and counts.is_contiguous())
    return None if counts is None else counts.data_ptr()


def _held_planes(d, halo, sides, planes, array=0):
    """Halo planes -> the two pointers (below, above) of a window entry.  sides = (below, above) or None; planes: each grid's (ny, nx).
    array = 0: one grid, a side is a (count, ny, nx) tensor -> its pointer; array = n: a side is a list of one such tensor per grid ->
    a pointer array of n.  NULL where no plane is held (count = min(halo, the planes on that side) is 0) or none is given"""
    out = []
    for count, ts in zip((min(int(halo), d.c0), min(int(halo), d.gz - d.c1)), sides if sides else (None, None)):
        if count == 0 or ts is None:
            out.append(None)
            continue
        ts = ts if array else [ts]
        assert len(ts) == len(planes), "one halo tensor per grid"
        ptrs = [_chk(t, (count,) + tuple(p), torch.float32).data_ptr() for t, p in zip(ts, planes)]
        out.append((C.c_void_p * array)(*ptrs) if array else C.c_void_p(ptrs[0]))
    return out


def _advect_desc(grid_shape, array_shape, velocity, dt, scalars, scheme, trace_order, out, scratch, counts):
    """the desc of a call on arrays of `array_shape` (the whole grid's, or a window's), and what it keeps alive: (desc, velocity_out or
    None, scalars_out).  out = None: everything is advected into new tensors; out = (velocity_out or None, scalars_out): into these,
    and with velocity_out None the scalars only.  scratch: as out, read under MacCormack only"""
    faces = _face3(array_shape)
    v = [_chk(velocity[a], faces[a], torch.float32) for a in range(3)]
    s = [_chk(q, array_shape, torch.float32) for q in scalars]
    new = lambda like: [torch.empty_like(t) for t in like]  # noqa: E731
    vout, sout = (new(v), new(s)) if out is None else out
    sout = list(sout) if sout is not None else []
    assert len(sout) == len(s), "one output per scalar grid"
    d = AdvectDesc()
    d.struct_size = C.sizeof(AdvectDesc)
    d.gz, d.gy, d.gx = grid_shape
    d.dt, d.scheme, d.trace_order, d.scalars = float(dt), SCHEMES[scheme], int(trace_order), len(s)
    vscr, sscr = (None, None) if scratch is None else scratch
    if d.scheme == 1 and scratch is None:
        vscr, sscr = (new(v) if vout is not None else None), new(s)
    for a in range(3):
        d.velocity_in[a] = v[a].data_ptr()
        if vout is not None:
            d.velocity_out[a] = _chk(vout[a], faces[a], torch.float32).data_ptr()
        if vscr is not None:
            d.velocity_scratch[a] = _chk(vscr[a], faces[a], torch.float32).data_ptr()
    for q in range(len(s)):
        d.scalar_in[q], d.scalar_out[q] = s[q].data_ptr(), _chk(sout[q], array_shape, torch.float32).data_ptr()
        if sscr is not None:
            d.scalar_scratch[q] = _chk(sscr[q], array_shape, torch.float32).data_ptr()
    d.counts_dev = _counts_ptr(counts)
    return d, vout, sout, (v, s, vscr, sscr)


def advect(velocity, dt, scalars=(), scheme="maccormack", trace_order=2, out=None, counts=None, scratch=None):
    """mgps_fields_advect: the three face grids of `velocity` (self-advection) and the cell grids `scalars` (0 .. 4; liquid_phi, say)
    carried along `velocity` over `dt` (time step over cell size), out of place.  scheme: "maccormack" (two launches, limited to the
    values around the departure point) or "semi_lagrangian" (one); trace_order 2 is the midpoint rule, 1 one Euler step.  Outputs
    and MacCormack's scratch grids are allocated unless given: out = (velocity_out or None, scalars_out), where None for the
    velocity advects the scalars only; scratch likewise.  counts: an int64 CUDA tensor of 2 that the pass adds to ([0] targets
    whose trace was clamped into the grid's box), or None.  Returns (velocity_out, scalars_out).  Does not synchronise."""
    shape = list(velocity[0].shape)
    shape[2] -= 1
    shape = tuple(shape)
    d, vout, sout, keep = _advect_desc(shape, shape, velocity, dt, scalars, scheme, trace_order, out, scratch, counts)
    with torch.cuda.device(keep[0][0].device):
        check(lib().mgps_fields_advect(C.byref(d), _stream()))
    return vout, sout


def advectSlab(d, velocity, dt, halo, velocity_halo, scalars=(), scalar_halo=(), scheme="semi_lagrangian", trace_order=2, out=None,
               counts=None):
    """mgps_fields_slab_advect: advect on the window `d` (fields.slab_window), without communication; the arrays are the window's
    (z-faces c0 .. c1).  velocity_halo = (below[3] or None, above[3] or None): per face grid the min(halo, c0) planes below the window
    and the min(halo, gz - c1) planes above it as (planes, ny, nx) tensors (of the z-face grid: the face planes below c0 and above
    c1); scalar_halo likewise, one tensor per scalar grid.  None where no plane is held.  counts[1] is raised by the targets that
    asked for a plane that is not held.  The window form is semi-Lagrangian only: scheme = "maccormack" is refused by the library."""
    vlo, vhi = _held_planes(d, halo, velocity_halo, [(d.gy, d.gx + 1), (d.gy + 1, d.gx), (d.gy, d.gx)], 4)
    slo, shi = _held_planes(d, halo, scalar_halo, [(d.gy, d.gx)] * len(scalars), 4)
    desc, vout, sout, keep = _advect_desc((d.gz, d.gy, d.gx), d.base_shape, velocity, dt, scalars, "semi_lagrangian", trace_order, out, None, counts)
    desc.scheme = SCHEMES[scheme]
    with torch.cuda.device(keep[0][0].device):
        check(lib().mgps_fields_slab_advect(C.byref(d), C.byref(desc), int(halo), vlo, vhi, slo, shi, _stream()))
    return vout, sout


# ---- redistancing: a fast iterative Eikonal pass (include/mgps_fields.h) ---------------------------------------
class RedistanceDesc(C.Structure):
    """mgps_redistance_desc (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("gx", C.c_int), ("gy", C.c_int), ("gz", C.c_int), ("band", C.c_double), ("dx", C.c_double),
        ("rounds", C.c_int), ("inner", C.c_int), ("phi_in", C.c_void_p), ("phi_out", C.c_void_p), ("scratch", C.c_void_p),
        ("counts_dev", C.c_void_p),
    ]


def _redistance_desc(grid_shape, array_shape, phi_in, band, dx, rounds, inner, out, scratch, counts):
    """the desc of a call on arrays of `array_shape` (the whole grid's, or a window's); out is allocated unless given"""
    _chk(phi_in, array_shape, torch.float32)
    out = torch.empty_like(phi_in) if out is None else _chk(out, array_shape, torch.float32)
    d = RedistanceDesc()
    d.struct_size = C.sizeof(RedistanceDesc)
    d.gz, d.gy, d.gx = grid_shape
    d.band, d.dx, d.rounds, d.inner = float(band), float(dx), int(rounds), int(inner)
    d.phi_in, d.phi_out = phi_in.data_ptr(), out.data_ptr()
    if scratch is not None:
        d.scratch = _chk(scratch, array_shape, torch.float32).data_ptr()
    d.counts_dev = _counts_ptr(counts)
    return d, out


def redistanceInitSlab(d, liquid_phi, band, halo, phi_halo=None, out=None, counts=None):
    """mgps_fields_slab_redistance_init on the window `d` (fields.slab_window): the initial pass, phi -> the unscaled state s T of
    the window's planes.  phi_halo = (below or None, above or None): the min(halo, c0) planes below the window and the
    min(halo, gz - c1) planes above it as (planes, ny, nx) tensors; one plane either way is needed.  counts[0] is raised by the
    window's interface cells.  Returns the state.  Does not synchronise."""
    desc, out = _redistance_desc((d.gz, d.gy, d.gx), d.base_shape, liquid_phi, band, 1.0, 0, 1, out, None, counts)
    lo, hi = _held_planes(d, halo, phi_halo, [(d.gy, d.gx)])
    with torch.cuda.device(liquid_phi.device):
        check(lib().mgps_fields_slab_redistance_init(C.byref(d), C.byref(desc), int(halo), lo, hi, _stream()))
    return out


def redistanceRoundSlab(d, state, band, halo, state_halo=None, inner=4, last=False, dx=1.0, out=None, counts=None):
    """mgps_fields_slab_redistance_round on the window `d`: one round of `inner` block-Jacobi iterations, state -> state.
    state_halo: as phi_halo, of the neighbours' states before this round; a round of inner > 1 reads the planes
    4 floor(c0 / 4) - 1 .. 4 ceil(c1 / 4) (halo = 4 always suffices), inner = 1 one plane either way; fewer is refused.  With `last`
    the stores are multiplied by dx and counts[1] is raised by the window's cells the round changed.  Does not synchronise."""
    desc, out = _redistance_desc((d.gz, d.gy, d.gx), d.base_shape, state, band, dx, 0, inner, out, None, counts)
    lo, hi = _held_planes(d, halo, state_halo, [(d.gy, d.gx)])
    with torch.cuda.device(state.device):
        check(lib().mgps_fields_slab_redistance_round(C.byref(d), C.byref(desc), int(halo), lo, hi, int(bool(last)), _stream()))
    return out


def redistance(liquid_phi, band, dx=1.0, rounds=None, inner=4, out=None, scratch=None, counts=None):
    """mgps_fields_redistance: liquid_phi -> the signed distance (in phi's units, dx per cell) within `band` cells of its zero
    level set, +-band dx beyond; the sign of every cell (phi <= 0 is inside) is kept.  Out of place.
    rounds = an integer: the single library call -- one initial launch and `rounds` rounds of `inner` block-Jacobi iterations, no
    synchronisation; scratch (a grid like out; allocated unless given) is needed for rounds > 0; counts (an int64 CUDA tensor of 2)
    is added to: [0] interface cells, [1] the cells the last round changed.
    rounds = None, the convenience form: the initial pass, then batches of max(2, ceil(band)) rounds through the window entries on
    [0, gz) until a round changes nothing.  The last round of a batch is the one that counts, and it writes dx state to `out`; where
    it did change a cell the next batch goes on from that round's input.  One synchronisation (a read of the count) per batch.
    counts then receives [0] and, as the fixpoint's property, [1] += 0.
    Returns out."""
    shape = tuple(liquid_phi.shape)
    if rounds is not None:
        if scratch is None and int(rounds) > 0:
            scratch = torch.empty_like(liquid_phi)
        d, out = _redistance_desc(shape, shape, liquid_phi, band, dx, rounds, inner, out, scratch, counts)
        with torch.cuda.device(liquid_phi.device):
            check(lib().mgps_fields_redistance(C.byref(d), _stream()))
        return out
    from .solver import expanded_layout

    w = slab_window(shape, True, [0, expanded_layout(shape)[0][0]], 0)  # the whole grid as a window: [0, gz), no halo
    tally = torch.zeros(2, dtype=torch.int64, device=liquid_phi.device)
    out = torch.empty_like(liquid_phi) if out is None else out
    a = redistanceInitSlab(w, liquid_phi, band, 0, counts=tally)
    b = torch.empty_like(liquid_phi) if scratch is None else scratch
    batch = max(2, -int(-float(band) // 1))
    while True:
        for _ in range(batch - 1):
            a, b = redistanceRoundSlab(w, a, band, 0, inner=inner, out=b), a
        tally[1] = 0
        redistanceRoundSlab(w, a, band, 0, inner=inner, last=True, dx=dx, out=out, counts=tally)
        if int(tally[1]) == 0:
            break
    if counts is not None:
        counts += tally
    return out


# ---- FLIP particles: bin, particles -> grid, grid -> particles and move (include/mgps_fields.h) -----------------
class ParticlesBinDesc(C.Structure):
    """mgps_particles_bin_desc (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("gx", C.c_int), ("gy", C.c_int), ("gz", C.c_int), ("n", C.c_int), ("position_in", C.c_void_p * 3),
        ("velocity_in", C.c_void_p * 3), ("position_out", C.c_void_p * 3), ("velocity_out", C.c_void_p * 3), ("order", C.c_void_p),
        ("cell_start", C.c_void_p), ("counts_dev", C.c_void_p),
    ]


class ParticlesToGridDesc(C.Structure):
    """mgps_particles_to_grid_desc (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("gx", C.c_int), ("gy", C.c_int), ("gz", C.c_int), ("n", C.c_int), ("form", C.c_int), ("radius", C.c_double),
        ("dx", C.c_double), ("position", C.c_void_p * 3), ("velocity", C.c_void_p * 3), ("cell_start", C.c_void_p), ("velocity_out", C.c_void_p * 3),
        ("weight_out", C.c_void_p * 3), ("known_out", C.c_void_p * 3), ("liquid_phi_out", C.c_void_p), ("counts_dev", C.c_void_p),
    ]


class ParticlesUpdateDesc(C.Structure):
    """mgps_particles_update_desc (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("gx", C.c_int), ("gy", C.c_int), ("gz", C.c_int), ("n", C.c_int), ("trace_order", C.c_int), ("dt", C.c_double),
        ("flip", C.c_double), ("position_in", C.c_void_p * 3), ("velocity_in", C.c_void_p * 3), ("position_out", C.c_void_p * 3),
        ("velocity_out", C.c_void_p * 3), ("grid_new", C.c_void_p * 3), ("grid_old", C.c_void_p * 3), ("counts_dev", C.c_void_p),
    ]


def _particles(arrays, n=None):
    """three float32 CUDA arrays of n entries each"""
    assert len(arrays) == 3
    n = int(arrays[0].numel()) if n is None else n
    return [_chk(t, (n,), torch.float32) for t in arrays], n


def binParticles(position, velocity, shape, out=None):
    """mgps_particles_bin: the particles (three float32 CUDA arrays of positions in cells, three of velocities or None) in cell order
    on the grid `shape` = (gz, gy, gx), out of place.  Returns (position, velocity or None, order, cell_start, counts): the gathered
    arrays, order[s] = the input index of slot s (int32), cell_start (int32, cells + 2: the first slot of every cell, of the outside bin,
    and n) and counts (int64 of 2: [0] outside particles, [1] occupied cells).  out = (position[3], velocity[3] or None, order,
    cell_start) to write into given arrays.  Does not synchronise."""
    pos, n = _particles(position)
    vel = _particles(velocity, n)[0] if velocity is not None else None
    dev = pos[0].device
    d = ParticlesBinDesc()
    d.struct_size = C.sizeof(ParticlesBinDesc)
    d.gz, d.gy, d.gx = shape
    d.n = n
    cells = int(shape[0]) * int(shape[1]) * int(shape[2])
    if out is None:
        out = ([torch.empty_like(t) for t in pos], [torch.empty_like(t) for t in vel] if vel is not None else None,
               torch.empty(n, dtype=torch.int32, device=dev), torch.empty(cells + 2, dtype=torch.int32, device=dev))
    pout, vout, order, cell_start = out
    pout = _particles(pout, n)[0]
    vout = _particles(vout, n)[0] if vel is not None else None
    _chk(order, (n,), torch.int32), _chk(cell_start, (cells + 2,), torch.int32)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    for a in range(3):
        d.position_in[a], d.position_out[a] = pos[a].data_ptr(), pout[a].data_ptr()
        if vel is not None:
            d.velocity_in[a], d.velocity_out[a] = vel[a].data_ptr(), vout[a].data_ptr()
    d.order, d.cell_start, d.counts_dev = order.data_ptr(), cell_start.data_ptr(), counts.data_ptr()
    with torch.cuda.device(dev):
        check(lib().mgps_particles_bin(C.byref(d), _stream()))
    return pout, vout, order, cell_start, counts


TO_GRID_FORMS = {"default": 0, "gather": 1, "staged": 2}


def particlesToGrid(position, velocity, cell_start, shape, radius, dx=1.0, want_phi=True, out=None, form="default"):
    """mgps_particles_to_grid: BINNED particles (binParticles' position, velocity and cell_start) -> the face grids of the velocity
    (the weighted mean of the particles within one cell of a face, 0 where there is none), of the weights and of the known faces
    (uint8: the `valid_faces` of extrapolateVelocity), and liquid_phi = dx (min(distance to the nearest particle, 1.5) - radius), a
    union of spheres of `radius` cells (redistance makes it a distance).  out = (velocity[3], weight[3] or None, known[3], liquid_phi
    or None) to write into given grids.  Returns (velocity[3], weight[3], known[3], liquid_phi or None, counts): counts is int64 of
    2, [0] known faces, [1] cells with phi <= 0.  form: "gather" or "staged" picks the kernel ("default": the library's choice); the
    bits are the same.  Does not synchronise."""
    shape = tuple(int(s) for s in shape)
    pos, n = _particles(position)
    vel, _ = _particles(velocity, n)
    dev = cell_start.device
    _chk(cell_start, (shape[0] * shape[1] * shape[2] + 2,), torch.int32)
    faces = _face3(shape)
    if out is None:
        out = ([torch.empty(f, dtype=torch.float32, device=dev) for f in faces], [torch.empty(f, dtype=torch.float32, device=dev) for f in faces],
               [torch.empty(f, dtype=torch.uint8, device=dev) for f in faces], torch.empty(shape, dtype=torch.float32, device=dev) if want_phi else None)
    vout, wout, known, phi = out
    d = ParticlesToGridDesc()
    d.struct_size = C.sizeof(ParticlesToGridDesc)
    d.gz, d.gy, d.gx = shape
    d.n, d.form, d.radius, d.dx = n, TO_GRID_FORMS[form], float(radius), float(dx)
    for a in range(3):
        d.position[a], d.velocity[a] = pos[a].data_ptr(), vel[a].data_ptr()
        d.velocity_out[a] = _chk(vout[a], faces[a], torch.float32).data_ptr()
        if wout is not None:
            d.weight_out[a] = _chk(wout[a], faces[a], torch.float32).data_ptr()
        d.known_out[a] = _chk(known[a], faces[a], torch.uint8).data_ptr()
    d.cell_start = cell_start.data_ptr()
    if phi is not None:
        d.liquid_phi_out = _chk(phi, shape, torch.float32).data_ptr()
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    d.counts_dev = counts.data_ptr()
    with torch.cuda.device(dev):
        check(lib().mgps_particles_to_grid(C.byref(d), _stream()))
    return vout, wout, known, phi, counts


def _update_desc(position, velocity, grid_new, dt, grid_old, flip, trace_order, out, counts):
    """the desc of updateParticles and updateParticlesSolid, and (position_out, velocity_out)"""
    pos, n = _particles(position)
    vel, _ = _particles(velocity, n)
    shape = list(grid_new[0].shape)
    shape[2] -= 1
    faces = _face3(tuple(shape))
    pout, vout = ([torch.empty_like(t) for t in pos], [torch.empty_like(t) for t in vel]) if out is None else out
    d = ParticlesUpdateDesc()
    d.struct_size = C.sizeof(ParticlesUpdateDesc)
    d.gz, d.gy, d.gx = shape
    d.n, d.trace_order, d.dt, d.flip = n, int(trace_order), float(dt), float(flip)
    for a in range(3):
        d.position_in[a], d.velocity_in[a] = pos[a].data_ptr(), vel[a].data_ptr()
        d.position_out[a], d.velocity_out[a] = _particles(pout, n)[0][a].data_ptr(), _particles(vout, n)[0][a].data_ptr()
        d.grid_new[a] = _chk(grid_new[a], faces[a], torch.float32).data_ptr()
        if grid_old is not None:
            d.grid_old[a] = _chk(grid_old[a], faces[a], torch.float32).data_ptr()
    d.counts_dev = _counts_ptr(counts)
    return d, pout, vout


def updateParticles(position, velocity, grid_new, dt, grid_old=None, flip=0.95, trace_order=2, out=None, counts=None):
    """mgps_particles_update: grid -> particles, then move.  Every particle inside the box takes
    (1 - flip) U_new(x) + flip (v + U_new(x) - U_old(x)) as its velocity and moves along grid_new over `dt` (time step over cell size;
    trace_order 2 is the midpoint rule), clamped into the box; particles outside are copied through.  grid_new: the projected,
    extrapolated face grids; grid_old: the particlesToGrid result before forces and projection (None only with flip = 0).
    out = (position_out[3], velocity_out[3]): each array the input itself (in place) or one that overlaps nothing; None: new arrays.
    counts: an int64 CUDA tensor of 2 that the pass adds to ([0] particles a clamp moved, [1] outside particles), or None.
    Returns (position_out, velocity_out).  Does not synchronise."""
    d, pout, vout = _update_desc(position, velocity, grid_new, dt, grid_old, flip, trace_order, out, counts)
    with torch.cuda.device(position[0].device):
        check(lib().mgps_particles_update(C.byref(d), _stream()))
    return pout, vout


# ---- FLIP particles next to solids: collide, resample (include/mgps_fields.h) -----------------------------------
class ParticlesCollideDesc(C.Structure):
    """mgps_particles_collide_desc (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("gx", C.c_int), ("gy", C.c_int), ("gz", C.c_int), ("n", C.c_int), ("iterations", C.c_int), ("margin", C.c_double),
        ("friction", C.c_double), ("position_in", C.c_void_p * 3), ("velocity_in", C.c_void_p * 3), ("position_out", C.c_void_p * 3),
        ("velocity_out", C.c_void_p * 3), ("solid_phi", C.c_void_p), ("solid_velocity", C.c_void_p * 3), ("counts_dev", C.c_void_p),
    ]


class ParticlesResampleDesc(C.Structure):
    """mgps_particles_resample_desc (include/mgps_fields.h)."""

    _fields_ = [
        ("struct_size", C.c_int), ("gx", C.c_int), ("gy", C.c_int), ("gz", C.c_int), ("n", C.c_int), ("capacity", C.c_int), ("min_per_cell", C.c_int),
        ("max_per_cell", C.c_int), ("keep_outside", C.c_int), ("seed", C.c_uint32), ("dx", C.c_double), ("seed_depth", C.c_double),
        ("position", C.c_void_p * 3), ("velocity", C.c_void_p * 3), ("cell_start", C.c_void_p), ("liquid_phi", C.c_void_p), ("solid_phi", C.c_void_p),
        ("grid", C.c_void_p * 3), ("position_out", C.c_void_p * 3), ("velocity_out", C.c_void_p * 3), ("cell_start_out", C.c_void_p),
        ("n_out_dev", C.c_void_p), ("counts_dev", C.c_void_p),
    ]


def _counts_of(counts, entries):
    """an int64 CUDA tensor of `entries` that a pass adds to, or None -> its pointer"""
    assert counts is None or (counts.is_cuda and counts.dtype == torch.int64 and counts.numel() == entries and counts.is_contiguous())
    return None if counts is None else counts.data_ptr()


def _solid_desc(solid_phi, solid_velocity, margin, iterations, friction, counts):
    """the collide desc without its particle arrays"""
    shape = tuple(solid_phi.shape)
    faces = _face3(shape)
    d = ParticlesCollideDesc()
    d.struct_size = C.sizeof(ParticlesCollideDesc)
    d.gz, d.gy, d.gx = shape
    d.iterations, d.margin, d.friction = int(iterations), float(margin), float(friction)
    d.solid_phi = _chk(solid_phi, shape, torch.float32).data_ptr()
    if solid_velocity is not None:
        for a in range(3):
            d.solid_velocity[a] = _chk(solid_velocity[a], faces[a], torch.float32).data_ptr()
    d.counts_dev = _counts_of(counts, 3)
    return d


def collideParticles(position, velocity, solid_phi, solid_velocity=None, margin=0.1, iterations=2, friction=0.0, out=None, counts=None):
    """mgps_particles_collide: every particle inside the box whose solid_phi (a CUDA cell grid, negative inside the solid, in cells:
    rasterizeBodies' first result) is below `margin` is pushed along the grid's gradient to solid_phi = margin, at most `iterations`
    times (1 .. 4), and loses the velocity it has into the solid relative to solid_velocity (the three face grids the projection
    takes, or None: at rest), and the fraction `friction` of the rest.  Every other particle keeps its bits.
    out = (position_out[3], velocity_out[3]): each array the input itself (in place) or one that overlaps nothing; None: new arrays.
    counts: an int64 CUDA tensor of 3 that the pass adds to ([0] pushed, [1] pushed and still inside the solid, [2] stuck where the
    gradient vanishes), or None.  Returns (position_out, velocity_out).  Does not synchronise."""
    pos, n = _particles(position)
    vel, _ = _particles(velocity, n)
    pout, vout = ([torch.empty_like(t) for t in pos], [torch.empty_like(t) for t in vel]) if out is None else out
    d = _solid_desc(solid_phi, solid_velocity, margin, iterations, friction, counts)
    d.n = n
    for a in range(3):
        d.position_in[a], d.velocity_in[a] = pos[a].data_ptr(), vel[a].data_ptr()
        d.position_out[a], d.velocity_out[a] = _particles(pout, n)[0][a].data_ptr(), _particles(vout, n)[0][a].data_ptr()
    with torch.cuda.device(pos[0].device):
        check(lib().mgps_particles_collide(C.byref(d), _stream()))
    return pout, vout


def updateParticlesSolid(position, velocity, grid_new, dt, solid_phi, grid_old=None, flip=0.95, trace_order=2, solid_velocity=None, margin=0.1,
                         iterations=2, friction=0.0, out=None, counts=None, solid_counts=None):
    """mgps_particles_update_solid: updateParticles and collideParticles in one launch, with the bits of the two calls in a row and
    without the second pass over the six arrays.  The arguments are updateParticles' and collideParticles'; counts (int64 of 2) takes
    the update's counts, solid_counts (int64 of 3) the collision's.  Returns (position_out, velocity_out).  Does not synchronise."""
    d, pout, vout = _update_desc(position, velocity, grid_new, dt, grid_old, flip, trace_order, out, counts)
    s = _solid_desc(solid_phi, solid_velocity, margin, iterations, friction, solid_counts)
    with torch.cuda.device(position[0].device):
        check(lib().mgps_particles_update_solid(C.byref(d), C.byref(s), _stream()))
    return pout, vout


def resampleParticles(position, velocity, cell_start, shape, capacity, min_per_cell, max_per_cell, liquid_phi=None, dx=1.0, seed_depth=1.0,
                      solid_phi=None, grid=None, seed=0, keep_outside=False, out=None):
    """mgps_particles_resample: BINNED particles (binParticles' position, velocity and cell_start) -> a binned set in arrays of
    `capacity` entries in which no cell holds more than max_per_cell particles (the surplus is dropped at an even stride) and every
    deep cell -- liquid_phi <= -seed_depth dx, and solid_phi > 0 where given -- holds at least min_per_cell: the new ones lie at
    hashed places of their cell (`seed`) and take the velocity of the face grids `grid`.  min_per_cell = 0: thinning only.  The
    outside bin is kept behind the last cell, or dropped.  out = (position[3], velocity[3], cell_start, n_out) to write into given
    arrays.  Returns (position, velocity, cell_start, n_out, counts): n_out an int32 CUDA tensor of 1, the particles of the new set
    (valid only if <= capacity), counts int64 of 4: [0] thinned away, [1] seeded, [2] deep cells, [3] 1 if the set did not fit.
    Does not synchronise."""
    shape = tuple(int(s) for s in shape)
    pos, n = _particles(position)
    vel, _ = _particles(velocity, n)
    dev = cell_start.device
    cells = shape[0] * shape[1] * shape[2]
    _chk(cell_start, (cells + 2,), torch.int32)
    faces = _face3(shape)
    capacity = int(capacity)
    if out is None:
        out = ([torch.empty(capacity, dtype=torch.float32, device=dev) for _ in range(3)], [torch.empty(capacity, dtype=torch.float32, device=dev) for _ in range(3)],
               torch.empty(cells + 2, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    pout, vout, start_out, n_out = out
    pout, vout = _particles(pout, capacity)[0], _particles(vout, capacity)[0]
    d = ParticlesResampleDesc()
    d.struct_size = C.sizeof(ParticlesResampleDesc)
    d.gz, d.gy, d.gx = shape
    d.n, d.capacity, d.min_per_cell, d.max_per_cell, d.keep_outside = n, capacity, int(min_per_cell), int(max_per_cell), int(bool(keep_outside))
    d.seed, d.dx, d.seed_depth = int(seed) & 0xFFFFFFFF, float(dx), float(seed_depth)
    for a in range(3):
        d.position[a], d.velocity[a] = pos[a].data_ptr(), vel[a].data_ptr()
        d.position_out[a], d.velocity_out[a] = pout[a].data_ptr(), vout[a].data_ptr()
        if grid is not None:
            d.grid[a] = _chk(grid[a], faces[a], torch.float32).data_ptr()
    d.cell_start = cell_start.data_ptr()
    d.cell_start_out = _chk(start_out, (cells + 2,), torch.int32).data_ptr()
    d.n_out_dev = _chk(n_out, (1,), torch.int32).data_ptr()
    if liquid_phi is not None:
        d.liquid_phi = _chk(liquid_phi, shape, torch.float32).data_ptr()
    if solid_phi is not None:
        d.solid_phi = _chk(solid_phi, shape, torch.float32).data_ptr()
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    d.counts_dev = counts.data_ptr()
    with torch.cuda.device(dev):
        check(lib().mgps_particles_resample(C.byref(d), _stream()))
    return pout, vout, start_out, n_out, counts


def seedParticles(liquid_phi, per_cell=8, seed=0, jitter=1.0):
    """A helper for tests, examples and the benchmark, in plain torch (not an entry of the C ABI): per_cell = m^3 particles in every
    cell with liquid_phi < 0, on a jittered m x m x m lattice (2 x 2 x 2 by default) -- sub-cell q of a cell holds one particle at
    its centre plus jitter * uniform(-1/2, 1/2) of its size per axis.  Returns three float32 arrays of positions in cells, on
    liquid_phi's device, in cell order; the same seed gives the same particles."""
    m = round(per_cell ** (1.0 / 3.0))
    assert m >= 1 and m ** 3 == per_cell, "per_cell is a cube: 1, 8, 27, ..."
    cells = torch.nonzero(liquid_phi.detach().cpu() < 0)  # (cells, 3) as (k, j, i)
    sub = torch.stack(torch.meshgrid(*([torch.arange(m)] * 3), indexing="ij"), dim=-1).reshape(-1, 3)
    gen = torch.Generator().manual_seed(int(seed))
    u = torch.rand((cells.shape[0], per_cell, 3), generator=gen, dtype=torch.float64) - 0.5
    p = cells[:, None, :].double() + (sub[None, :, :].double() + 0.5 + float(jitter) * u) / m
    p = p.reshape(-1, 3).float()
    return [p[:, 2 - a].contiguous().to(liquid_phi.device) for a in range(3)]
