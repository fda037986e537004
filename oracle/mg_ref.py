"""ctypes front end of oracle/_ref/libmgref.so: the reference's own solver core, compiled unchanged against
the stand-in headers of oracle/ref_standin/ behind oracle/ref_driver.cpp (`make -C oracle ref`).

TEST INFRASTRUCTURE ONLY.  `Reference` offers the methods of mg_oracle.Oracle under the same names, fp64
only, so that one routine can drive either.  The library exists only where a checkout of the reference was at
hand when it was built; `available()` says so, and tests/golden/ref_*.npz hold what it computed for the
machines where it is not.
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
