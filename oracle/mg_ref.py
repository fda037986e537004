"""ctypes front end of oracle/_ref/libmgref.so: the reference's own solver core, compiled unchanged against
the stand-in headers of oracle/ref_standin/ behind oracle/ref_driver.cpp (`make -C oracle ref`).

TEST INFRASTRUCTURE ONLY.  `Reference` offers the methods of mg_oracle.Oracle under the same names, fp64
only, so that one routine can drive either.  The library exists only where a checkout of the reference was at
hand when it was built; `available()` says so, and tests/golden/ref_*.npz hold what it computed for the
machines where it is not.  `ReferenceFields` is the same for oracle/_ref/libmgref_fields.so, the reference's
free-surface plugin behind oracle/ref_fields_driver.cpp, with tests/golden/ref_fields_*.npz as its fixtures.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
BUILD_HINT = "make -C oracle ref"


def lib_path(long_double=False):
    return os.path.join(_HERE, "_ref", "libmgref_ld.so" if long_double else "libmgref.so")


def available(long_double=False):
    return os.path.exists(lib_path(long_double))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class ReferenceError_(RuntimeError):
    """A reference assertion or a stand-in bounds check failed inside the library."""


class Reference:
    real = np.float64
    creal = C.c_double

    def __init__(self, long_double=False):
        if not available(long_double):
            raise FileNotFoundError(f"{lib_path(long_double)} is missing: build it with `{BUILD_HINT}`")
        self.lib = L = C.CDLL(lib_path(long_double))
        assert L.mgr_real_bytes() == 8
        assert L.mgr_cholesky_real_bytes() == (16 if long_double else 8)
        L.mgr_last_error.restype = C.c_char_p
        for name in ("mgr_dot", "mgr_squared_l2", "mgr_l2", "mgr_inf_norm"):
            getattr(L, name).restype = C.c_double
        L.mgr_build_boundary_cells.restype = C.c_int64
        L.mgr_solver_create.restype = C.c_void_p

    def _ok(self, rc):
        if rc != 0:
            raise ReferenceError_(self.lib.mgr_last_error().decode())

    def _num(self, v):
        if v != v:
            raise ReferenceError_(self.lib.mgr_last_error().decode())
        return v

    def arr(self, a):
        return np.ascontiguousarray(a, dtype=np.float64)

    @staticmethod
    def lab(a):
        return np.ascontiguousarray(a, dtype=np.int32)

    def _wp(self, w):
        if w is None:
            return [], (None, None, None)
        ws = [self.arr(a) for a in w]
        return ws, tuple(_ptr(a) for a in ws)

    # -- operators (in place on x / outputs) ---------------------------------------------------------------
    def jacobi(self, x, b, lab, w=None):
        nz, ny, nx = lab.shape
        keep, wp = self._wp(w)
        self._ok(self.lib.mgr_jacobi(_ptr(x), _ptr(b), _ptr(lab), *wp, nx, ny, nz, None))

    def tiled_gs(self, x, b, lab, odd, forward, w=None):
        nz, ny, nx = lab.shape
        keep, wp = self._wp(w)
        self._ok(self.lib.mgr_tiled_gs(_ptr(x), _ptr(b), _ptr(lab), *wp, nx, ny, nz, int(odd), int(forward)))

    def boundary_jacobi(self, x, b, lab, cells, w=None):
        nz, ny, nx = lab.shape
        keep, wp = self._wp(w)
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        self._ok(self.lib.mgr_boundary_jacobi(_ptr(x), _ptr(b), _ptr(lab), _ptr(cells), C.c_int64(len(cells)), *wp, nx, ny, nz))

    def apply_poisson(self, y, x, lab, w=None):
        nz, ny, nx = lab.shape
        keep, wp = self._wp(w)
        self._ok(self.lib.mgr_apply_poisson(_ptr(y), _ptr(x), _ptr(lab), *wp, nx, ny, nz))

    def residual(self, r, x, b, lab, w=None):
        nz, ny, nx = lab.shape
        keep, wp = self._wp(w)
        self._ok(self.lib.mgr_residual(_ptr(r), _ptr(x), _ptr(b), _ptr(lab), *wp, nx, ny, nz))

    def downsample(self, coarse, fine, coarse_lab, fine_lab):
        nz, ny, nx = coarse_lab.shape
        self._ok(self.lib.mgr_downsample(_ptr(coarse), _ptr(fine), _ptr(coarse_lab), nx, ny, nz, _ptr(fine_lab)))

    def upsample_add(self, fine, coarse, fine_lab, coarse_lab):
        nz, ny, nx = fine_lab.shape
        self._ok(self.lib.mgr_upsample_add(_ptr(fine), _ptr(coarse), _ptr(fine_lab), nx, ny, nz, _ptr(coarse_lab)))

    def add_vectors(self, dst, a, bs, s, lab):
        self._ok(self.lib.mgr_add_vectors(_ptr(dst), _ptr(a), _ptr(bs), C.c_double(s), _ptr(lab), C.c_int64(lab.size)))

    def add_to_vector(self, dst, a, s, lab):
        self._ok(self.lib.mgr_add_to_vector(_ptr(dst), _ptr(a), C.c_double(s), _ptr(lab), C.c_int64(lab.size)))

    def scale_vector(self, v, s, lab):
        self._ok(self.lib.mgr_scale_vector(_ptr(v), C.c_double(s), _ptr(lab), C.c_int64(lab.size)))

    def dot(self, a, b, lab):
        nz, ny, nx = lab.shape
        return self._num(self.lib.mgr_dot(_ptr(a), _ptr(b), _ptr(lab), nx, ny, nz))

    def squared_l2(self, a, lab):
        nz, ny, nx = lab.shape
        return self._num(self.lib.mgr_squared_l2(_ptr(a), _ptr(lab), nx, ny, nz))

    def l2(self, a, lab):
        nz, ny, nx = lab.shape
        return self._num(self.lib.mgr_l2(_ptr(a), _ptr(lab), nx, ny, nz))

    def inf_norm(self, a, lab):
        nz, ny, nx = lab.shape
        return self._num(self.lib.mgr_inf_norm(_ptr(a), _ptr(lab), nx, ny, nz))

    # -- domain / hierarchy ----------------------------------------------------------------------------------
    def expanded_layout(self, bnx, bny, bnz):
        dims, off, lev = (C.c_int * 3)(), (C.c_int * 3)(), C.c_int()
        self.lib.mgr_expanded_layout(bnx, bny, bnz, dims, off, C.byref(lev))
        if lev.value < 0:
            raise ReferenceError_(self.lib.mgr_last_error().decode())
        return tuple(dims), off[0], lev.value

    def build_expanded_domain(self, base_lab, base_w):
        bnz, bny, bnx = base_lab.shape
        (enx, eny, enz), off, levels = self.expanded_layout(bnx, bny, bnz)
        base_lab = self.lab(base_lab)
        lab = np.empty((enz, eny, enx), dtype=np.int32)
        self._ok(self.lib.mgr_build_expanded_labels(_ptr(lab), _ptr(base_lab), bnx, bny, bnz, enx, eny, enz, off))
        ws = []
        for axis in range(3):
            shape = [enz, eny, enx]
            shape[2 - axis] += 1
            w = np.empty(shape, dtype=np.float64)
            bw = self.arr(base_w[axis])
            self._ok(self.lib.mgr_build_expanded_weights(_ptr(w), _ptr(bw), axis, bnx, bny, bnz, enx, eny, enz, off, _ptr(lab)))
            ws.append(w)
        self._ok(self.lib.mgr_set_boundary_labels(_ptr(lab), _ptr(ws[0]), _ptr(ws[1]), _ptr(ws[2]), enx, eny, enz))
        return lab, ws, off, levels

    def set_boundary_labels(self, lab, w):
        nz, ny, nx = lab.shape
        keep, wp = self._wp(w)
        self._ok(self.lib.mgr_set_boundary_labels(_ptr(lab), *wp, nx, ny, nz))

    def build_coarse_labels(self, fine):
        nz, ny, nx = fine.shape
        coarse = np.empty((nz // 2, ny // 2, nx // 2), dtype=np.int32)
        self._ok(self.lib.mgr_build_coarse_labels(_ptr(coarse), _ptr(fine), nx, ny, nz))
        return coarse

    def build_boundary_cells(self, lab, width):
        nz, ny, nx = lab.shape
        out = C.c_void_p()
        n = self.lib.mgr_build_boundary_cells(_ptr(lab), nx, ny, nz, int(width), C.byref(out))
        if n < 0:
            raise ReferenceError_(self.lib.mgr_last_error().decode())
        cells = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int32)), shape=(max(n, 1) * 3,))[: n * 3].copy()
        self.lib.mgr_free(out)
        return cells.reshape(-1, 3)

    def _check(self, v):
        if v < 0:
            raise ReferenceError_(self.lib.mgr_last_error().decode())
        return bool(v)

    def unit_test_exterior(self, lab):
        nz, ny, nx = lab.shape
        return self._check(self.lib.mgr_unit_test_exterior(_ptr(lab), nx, ny, nz))

    def unit_test_boundary(self, lab, w=None):
        nz, ny, nx = lab.shape
        keep, wp = self._wp(w)
        return self._check(self.lib.mgr_unit_test_boundary(_ptr(lab), *wp, nx, ny, nz))

    def unit_test_coarsening(self, coarse, fine):
        nz, ny, nx = fine.shape
        return self._check(self.lib.mgr_unit_test_coarsening(_ptr(coarse), _ptr(fine), nx, ny, nz))

    def solver(self, lab, w, levels, use_gs):
        return ReferenceSolver(self, lab, w, levels, use_gs)


class ReferenceSolver:
    """The reference's GeometricMultigridPoissonSolver object (band width 3, 3 band passes, one sweep per stroke:
    its hard-wired schedule).  Its hierarchy is private; `levels` is getMGLevels()."""

    def __init__(self, ref, lab, w, levels, use_gs):
        self.o = ref
        self.labels = ref.lab(lab)
        self.w = [ref.arr(a) for a in w]
        nz, ny, nx = self.labels.shape
        h = ref.lib.mgr_solver_create(_ptr(self.labels), _ptr(self.w[0]), _ptr(self.w[1]), _ptr(self.w[2]), nx, ny, nz, int(levels), int(bool(use_gs)))
        if not h:
            raise ReferenceError_(ref.lib.mgr_last_error().decode())
        self.h = C.c_void_p(h)

    def close(self):
        if self.h:
            self.o.lib.mgr_solver_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def levels(self):
        return self.o.lib.mgr_solver_levels(self.h)

    def apply_vcycle(self, x, b, use_initial_guess=False):
        assert x.dtype == np.float64 and b.dtype == np.float64 and x.flags.c_contiguous
        self.o._ok(self.o.lib.mgr_solver_apply_vcycle(self.h, _ptr(x), _ptr(b), int(bool(use_initial_guess))))

    def solve_pcg(self, x, b, tol=1e-5, max_iter=2500, use_mg=True):
        stats = (C.c_double * 3)()
        hist = np.zeros(max_iter + 1, dtype=np.float64)
        rc = self.o.lib.mgr_solve_pcg(self.h, _ptr(x), _ptr(b), C.c_double(tol), int(max_iter), int(bool(use_mg)), stats, _ptr(hist))
        if rc < 0:
            raise ReferenceError_(self.o.lib.mgr_last_error().decode())
        it = int(stats[0])
        return {"status": rc, "iterations": it, "rel_residual": stats[1], "rel_residual_recomputed": stats[2], "history": hist[: it + 1]}


def fields_lib_path(long_double=False):
    return os.path.join(_HERE, "_ref", "libmgref_fields_ld.so" if long_double else "libmgref_fields.so")


def fields_available(long_double=False):
    return os.path.exists(fields_lib_path(long_double))


class ReferenceFields:
    """ctypes front end of oracle/_ref/libmgref_fields.so: the reference's plugin (HDK_GeometricFreeSurfacePressureSolver.cpp,
    HDK_Utilities.*), compiled unchanged behind oracle/ref_fields_driver.cpp.  The per-pass methods carry the names of
    mg_oracle.FieldsOracle where the two do the same thing.  What the reference keeps in a SIM_RawField goes in and comes out as
    float32 (raw fields store fpreal32); multigrid weights, rhs and solution are float64 (the plugin's SolveReal = StoreReal).
    Unlike the oracle, the reference builds domain labels and boundary weights on the BASE grid and expands them afterwards
    (`expand`).  Grids are numpy [k, j, i] arrays; face grids have one more entry along their axis (axis 0 = x = last dimension)."""

    def __init__(self, long_double=False, voxel_size=None):
        if not fields_available(long_double):
            raise FileNotFoundError(f"{fields_lib_path(long_double)} is missing: build it with `{BUILD_HINT}`")
        self.lib = L = C.CDLL(fields_lib_path(long_double))
        assert L.mgrf_field_real_bytes() == 4
        assert L.mgrf_cholesky_real_bytes() == (16 if long_double else 8)
        L.mgrf_last_error.restype = C.c_char_p
        L.mgrf_last_output.restype = C.c_char_p
        L.mgrf_set_voxel_size.argtypes = [C.c_float]
        if voxel_size is not None:
            L.mgrf_set_voxel_size(voxel_size)

    def _ok(self, rc):
        if rc != 0:
            raise ReferenceError_(self.lib.mgrf_last_error().decode())

    @staticmethod
    def face_shape(shape, axis):
        s = list(shape)
        s[2 - axis] += 1
        return tuple(s)

    @staticmethod
    def _f32(a):
        """a field as the reference stores it; refuses input that float32 does not hold exactly"""
        if a is None:
            return None
        f = np.ascontiguousarray(a, dtype=np.float32)
        assert (f == a).all(), "raw fields store fpreal32: pass float32 values"
        return f

    @staticmethod
    def _i32(a):
        return np.ascontiguousarray(a, dtype=np.int32)

    def _f3(self, fields):
        fs = [self._f32(a) for a in fields] if fields is not None else [None] * 3
        return fs, [_ptr(a) for a in fs]

    def parameter_count(self):
        return self.lib.mgrf_parameter_count()

    def material_labels(self, liquid_phi, solid_phi, cw):
        gz, gy, gx = liquid_phi.shape
        out = np.empty(liquid_phi.shape, dtype=np.int32)
        keep, cwp = self._f3(cw)
        self._ok(self.lib.mgrf_material_labels(_ptr(out), _ptr(self._f32(liquid_phi)), _ptr(self._f32(solid_phi)), *cwp, gx, gy, gz))
        return out

    def valid_faces(self, material, cw):
        gz, gy, gx = material.shape
        out = [np.empty(self.face_shape(material.shape, a), dtype=np.float32) for a in range(3)]
        keep, cwp = self._f3(cw)
        self._ok(self.lib.mgrf_valid_faces(*[_ptr(v) for v in out], _ptr(self._i32(material)), *cwp, gx, gy, gz))
        assert all(np.isin(v, (0.0, 1.0)).all() for v in out)
        return [v.astype(np.uint8) for v in out]

    def base_domain_labels(self, material):
        gz, gy, gx = material.shape
        out = np.empty(material.shape, dtype=np.int32)
        self._ok(self.lib.mgrf_domain_labels(_ptr(out), _ptr(self._i32(material)), gx, gy, gz))
        return out

    def base_boundary_weights(self, cw, liquid_phi, valid, material, base_labels):
        gz, gy, gx = material.shape
        out = []
        phi, mat, lab = self._f32(liquid_phi), self._i32(material), self._i32(base_labels)
        for a in range(3):
            w = np.empty(self.face_shape(material.shape, a), dtype=np.float64)
            self._ok(self.lib.mgrf_boundary_weights(a, _ptr(w), _ptr(self._f32(cw[a])), _ptr(phi), _ptr(np.ascontiguousarray(valid[a], dtype=np.float32)),
                                                    _ptr(mat), _ptr(lab), gx, gy, gz))
            out.append(w)
        return out

    def expanded_layout(self, bnx, bny, bnz):
        dims, off, lev = (C.c_int * 3)(), (C.c_int * 3)(), C.c_int()
        self._ok(self.lib.mgrf_expanded_layout(bnx, bny, bnz, dims, off, C.byref(lev)))
        assert off[0] == off[1] == off[2]
        return tuple(dims), off[0], lev.value

    def expand(self, base_labels, base_w):
        """buildExpandedCellLabels + buildExpandedBoundaryWeights x3 + setBoundaryCellLabels (+ the two structural assertions), as
        solveGasSubclass chains them: (labels int32, weights float64 [3], offset, levels)."""
        gz, gy, gx = base_labels.shape
        (ex, ey, ez), off, levels = self.expanded_layout(gx, gy, gz)
        lab = np.empty((ez, ey, ex), dtype=np.int32)
        ws = [np.empty(self.face_shape(lab.shape, a), dtype=np.float64) for a in range(3)]
        bw = [np.ascontiguousarray(a, dtype=np.float64) for a in base_w]
        self._ok(self.lib.mgrf_expand(_ptr(lab), *[_ptr(w) for w in ws], _ptr(self._i32(base_labels)), *[_ptr(w) for w in bw], gx, gy, gz))
        return lab, ws, off, levels

    def rhs(self, material, vel, cw, exp_labels, offset, solid_vel=None):
        gz, gy, gx = material.shape
        ez, ey, ex = exp_labels.shape
        out = np.empty(exp_labels.shape, dtype=np.float64)
        (kv, vp), (ks, sp), (kc, cp) = self._f3(vel), self._f3(solid_vel), self._f3(cw)
        self._ok(self.lib.mgrf_rhs(_ptr(out), _ptr(self._i32(material)), *vp, *sp, *cp, _ptr(self._i32(exp_labels)), gx, gy, gz, ex, ey, ez, int(offset)))
        return out

    def pressure_to_solution(self, pressure, material, exp_labels, offset):
        gz, gy, gx = material.shape
        ez, ey, ex = exp_labels.shape
        out = np.empty(exp_labels.shape, dtype=np.float64)
        self._ok(self.lib.mgrf_apply_old_pressure(_ptr(out), _ptr(self._f32(pressure)), _ptr(self._i32(material)), _ptr(self._i32(exp_labels)), gx, gy, gz,
                                                  ex, ey, ez, int(offset)))
        return out

    def solution_to_pressure(self, pressure, solution, material, exp_labels, offset):
        """in place on the float32 `pressure`"""
        gz, gy, gx = material.shape
        ez, ey, ex = exp_labels.shape
        assert pressure.dtype == np.float32 and pressure.flags.c_contiguous
        self._ok(self.lib.mgrf_solution_to_pressure(_ptr(pressure), _ptr(np.ascontiguousarray(solution, dtype=np.float64)), _ptr(self._i32(material)),
                                                    _ptr(self._i32(exp_labels)), gx, gy, gz, ex, ey, ez, int(offset)))
        return pressure

    def pressure_gradient(self, vel, cw, liquid_phi, pressure, valid, material):
        """in place on the three float32 velocity grids"""
        gz, gy, gx = material.shape
        phi, p, mat = self._f32(liquid_phi), self._f32(pressure), self._i32(material)
        for a in range(3):
            assert vel[a].dtype == np.float32 and vel[a].flags.c_contiguous
            self._ok(self.lib.mgrf_pressure_gradient(a, _ptr(vel[a]), _ptr(self._f32(cw[a])), _ptr(phi), _ptr(p),
                                                     _ptr(np.ascontiguousarray(valid[a], dtype=np.float32)), _ptr(mat), gx, gy, gz))
        return vel

    def divergence(self, material, vel, cw, solid_vel=None):
        gz, gy, gx = material.shape
        out = np.zeros(3)
        (kv, vp), (ks, sp), (kc, cp) = self._f3(vel), self._f3(solid_vel), self._f3(cw)
        self._ok(self.lib.mgrf_divergence(_ptr(out), _ptr(self._i32(material)), *vp, *sp, *cp, gx, gy, gz))
        return float(out[0]), float(out[1]), float(out[2])

    def solve(self, liquid_phi, solid_phi, cw, vel, pressure, solid_vel=None, tolerance=1e-5, max_iterations=2500, use_mg=True, use_old_pressure=False):
        """The whole solveGasSubclass.  Returns (velocity [3] float32, pressure float32, valid [3] uint8, info): new arrays, the
        inputs stay.  info: iterations and relative residuals as the plugin's CG reports them (None where it printed none), and
        the plugin's own divergence report."""
        gz, gy, gx = liquid_phi.shape
        v = [self._f32(a).copy() for a in vel]
        p = self._f32(pressure).copy()
        valid = [np.empty(self.face_shape(liquid_phi.shape, a), dtype=np.float32) for a in range(3)]
        (ks, sp), (kc, cp) = self._f3(solid_vel), self._f3(cw)
        stats = (C.c_double * 6)()
        self._ok(self.lib.mgrf_solve(_ptr(self._f32(liquid_phi)), _ptr(self._f32(solid_phi)), *cp, *[_ptr(a) for a in v], *sp, _ptr(p),
                                     *[_ptr(a) for a in valid], gx, gy, gz, C.c_double(tolerance), int(max_iterations), int(bool(use_mg)),
                                     int(bool(use_old_pressure)), stats))
        num = lambda x: None if x != x else float(x)  # noqa: E731
        info = {"iterations": None if stats[0] != stats[0] else int(stats[0]), "rel_residual": num(stats[1]), "rel_residual_recomputed": num(stats[2]),
                "divergence_max": num(stats[3]), "divergence_sum": num(stats[4]), "divergence_average": num(stats[5])}
        return v, p, [a.astype(np.uint8) for a in valid], info
