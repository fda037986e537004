"""Cases and routines shared by tests/golden/make_ref_golden.py (which runs them on the compiled reference,
oracle/mg_ref.py) and tests/test_reference_parity.py (which runs them on the oracle, oracle/mg_oracle.py, and
on the HIP solver).  One routine drives either implementation: they offer the same methods.

Everything per cell is compared by sha256 of the fp64 / int32 bytes: both sides are fp64 with contraction off
and the oracle claims the reference's visiting and accumulation order, so "equal" means bit for bit.
"""
import hashlib

import numpy as np

from geometricmultigridpressuresolver_amd import domains as D

BAND_WIDTH, BAND_PASSES = 3, 3  # the reference's hard-wired schedule (MG.cpp:141-142)
GS_PASSES = ((True, True), (False, True), (False, False), (True, False))  # V-cycle order: down odd / even, up even / odd
PCG_TOL, PCG_MAX_ITER = 1e-5, 500

# name -> (domain kind, base grid, levels, solver shape).  The first three are the domains of make_golden.py
# (power-of-two solver grids: whole 16^3 tiles on level 0).  "ragged" is a free surface with a cut-cell solid on a
# 36 x 28 x 20 (z, y, x) base in a 56 x 40 x 40 solver grid: no extent of any level is a multiple of 16, so every
# level has partial tiles (level 1: 28 x 20 x 20, level 2: 14 x 10 x 10), and the tile colouring of the
# Gauss-Seidel smoother, the tile-major band order and the per-tile reductions all meet ragged tiles.  Extents are
# multiples of 8 because the reference demands even extents on each of its three levels.
CASES = {
    "simple16": ("simple", 16, None, None),
    "complex16": ("complex", 16, None, None),
    "solid24": ("solid", 24, None, None),
    "ragged": ("solid", (36, 28, 20), 3, (56, 40, 40)),
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def rand_active(lab, seed, scale=1.0):
    """test_gpu_parity._rand_active: U(0,1) * scale on active cells, PCG64(seed)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    v = rng.random(lab.shape) * scale
    v[~D.active_mask(lab)] = 0
    return v


def base_domain(name):
    kind, g, levels, shape = CASES[name]
    if kind == "simple":
        return D.build_simple_domain(g, 1, dtype=np.float32)
    return D.build_complex_domain(g, use_solid=(kind == "solid"), dtype=np.float32)


def solver_domain(name):
    """(labels int32, weights fp64 [3], offset, levels, dx): what every implementation is given."""
    kind, g, levels, shape = CASES[name]
    bl, bw, dx = base_domain(name)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=levels, solver_shape=shape)
    return lab.astype(np.int32), [a.astype(np.float64) for a in w], off, lev, dx


def random_solver_domain(seed, shape=(48, 32, 32), levels=3):
    """test_device_setup.random_domain: blobs of every label, fractional weights."""
    from test_device_setup import random_domain

    lab, w = random_domain(shape, levels, seed, closed_faces=False)
    return lab.astype(np.int32), [np.asarray(a, dtype=np.float64) for a in w], 0, levels, 1.0 / max(shape)


def input_hashes(lab, w, dx):
    out = {"in/labels": sha(lab), "in/wx": sha(w[0]), "in/wy": sha(w[1]), "in/wz": sha(w[2])}
    for seed, scale in ((1, 1.0), (2, dx * dx), (3, 1.0), (4, 1.0), (5, dx * dx)):
        out[f"in/rand{seed}"] = sha(rand_active(lab, seed, scale))
    return out


def hierarchy(impl, lab, levels, width=BAND_WIDTH):
    """Per-level labels and band lists through the free functions (the reference keeps its solver's own copies
    private; its constructor calls exactly these, MG.cpp:238-281)."""
    labs = [np.ascontiguousarray(lab, dtype=np.int32)]
    for _ in range(1, levels):
        labs.append(impl.build_coarse_labels(labs[-1]))
    bands = [impl.build_boundary_cells(l, width) for l in labs]
    return labs, bands


def _transfer(impl, kind, dst, src, dst_lab, src_lab):
    fn = getattr(impl, kind)
    if fn.__code__.co_argcount == 5:  # the reference's entries also take the other level's labels (it reads them in assertions)
        fn(dst, src, dst_lab, src_lab)
    else:
        fn(dst, src, dst_lab)


def per_cell(impl, lab, w, levels, dx, band_width=BAND_WIDTH, band_passes=BAND_PASSES, keep=None):
    """Every per-cell operator on every level, on the seeds test_gpu_parity.py uses -> {name: sha256}.
    `keep`, a dict, receives the arrays themselves (the GPU tests hold the kernels to them)."""
    out = {}

    def put(name, a):
        out[name] = sha(a)
        if keep is not None:
            keep[name] = np.array(a, copy=True)

    labs, bands = hierarchy(impl, lab, levels, band_width)
    for l, (ll, band) in enumerate(zip(labs, bands)):
        wl = w if l == 0 else None
        put(f"L{l}/labels", ll)
        put(f"L{l}/band", band.astype(np.int32))
        x0 = rand_active(ll, 1) if l == 0 else rand_active(ll, 10 + l)
        b0 = rand_active(ll, 2, dx * dx) if l == 0 else rand_active(ll, 20 + l)
        y = np.zeros_like(x0)
        impl.apply_poisson(y, x0, ll, wl)
        put(f"L{l}/apply", y)
        r = np.zeros_like(x0)
        impl.residual(r, x0, b0, ll, wl)
        put(f"L{l}/residual", r)
        xj = x0.copy()
        impl.jacobi(xj, b0, ll, wl)
        put(f"L{l}/jacobi", xj)
        xb = x0.copy()
        for p in range(band_passes):
            impl.boundary_jacobi(xb, b0, ll, band, wl)
            put(f"L{l}/band_pass{p + 1}", xb)
        xg = x0.copy()
        for p, (odd, fwd) in enumerate(GS_PASSES):
            impl.tiled_gs(xg, b0, ll, odd, fwd, wl)
            put(f"L{l}/gs_pass{p + 1}", xg)
        if l + 1 < len(labs):
            cl = labs[l + 1]
            coarse = np.zeros(cl.shape)
            _transfer(impl, "downsample", coarse, rand_active(ll, 30 + l), cl, ll)
            put(f"L{l}/downsample", coarse)
            fine = rand_active(ll, 50 + l)
            _transfer(impl, "upsample_add", fine, rand_active(cl, 40 + l), ll, cl)
            put(f"L{l}/upsample_add", fine)
    a, b = vector_inputs(lab)
    v = a.copy()
    impl.add_to_vector(v, b, -0.37, lab)
    put("L0/add_to_vector", v)
    v = np.zeros_like(a)
    impl.add_vectors(v, a, b, 1.7, lab)
    put("L0/add_vectors", v)
    v = a.copy()
    impl.scale_vector(v, 0.25, lab)
    put("L0/scale_vector", v)
    return out


def vector_inputs(lab):
    """test_vector_ops_and_reductions' inputs: signed entries on interior cells."""
    return rand_active(lab, 3) - 0.4 * (lab == 0), rand_active(lab, 4)


def expansion(impl, name):
    """buildExpandedCellLabels / buildExpandedBoundaryWeights / setBoundaryCellLabels on the base domain (the
    reference's own power-of-two sizing) -> {name: sha256 or number}."""
    bl, bw, dx = base_domain(name)
    lab, ws, off, levels = impl.build_expanded_domain(bl.astype(np.int32), [a.astype(np.float64) for a in bw])
    out = {"expand/labels": sha(lab.astype(np.int32)), "expand/offset": int(off), "expand/levels": int(levels),
           "expand/shape": tuple(int(n) for n in lab.shape)}
    for a, n in enumerate("xyz"):
        out["expand/w" + n] = sha(np.asarray(ws[a], dtype=np.float64))
    return out


def structure_checks(impl, lab, w, levels):
    """The three unitTest* functions on the hierarchy -> {name: bool}."""
    labs, _ = hierarchy(impl, lab, levels)
    out = {}
    for l, ll in enumerate(labs):
        out[f"L{l}/unit_test_exterior"] = bool(impl.unit_test_exterior(ll))
        out[f"L{l}/unit_test_boundary"] = bool(impl.unit_test_boundary(ll, w if l == 0 else None))
        if l > 0:
            out[f"L{l}/unit_test_coarsening"] = bool(impl.unit_test_coarsening(ll, labs[l - 1]))
    return out


def reductions(impl, lab):
    """dot, squared L2, L2, signed inf norm -> {name: float}."""
    a, b = vector_inputs(lab)
    return {"dot": impl.dot(a, b, lab), "squared_l2": impl.squared_l2(a, lab), "l2": impl.l2(a, lab), "inf_norm": impl.inf_norm(a, lab),
            "inf_norm_negative": impl.inf_norm(-np.abs(a) - 1.0 * D.active_mask(lab), lab)}


def reduction_bounds(lab):
    """|oracle - ref| <= 2 n eps sum|a_i b_i| for two summation orders of the same n products (each order's error is
    at most n eps sum|a_i b_i| to first order; Higham, Accuracy and Stability, eq. 3.5).  l2 = sqrt(S): the difference of
    the roots is the difference of the squares over 2 sqrt(S), plus one rounding of each root.  The inf norms involve
    no rounding: bound 0."""
    a, b = vector_inputs(lab)
    act = D.active_mask(lab)
    n, eps = int(act.sum()), np.finfo(np.float64).eps
    s_dot, s_sq = float(np.abs(a * b)[act].sum()), float((a * a)[act].sum())
    return {"dot": 2 * n * eps * s_dot, "squared_l2": 2 * n * eps * s_sq,
            "l2": (n + 2) * eps * np.sqrt(s_sq), "inf_norm": 0.0, "inf_norm_negative": 0.0}


def cycles(impl, lab, w, levels, dx, pcg=True):
    """One and four chained V-cycles per smoother, MG-PCG per smoother and diagonal PCG on rand_active(seed 5) ->
    {name: array or number}."""
    b = rand_active(lab, 5, dx * dx)
    out = {}
    for use_gs in (False, True):
        tag = "gs" if use_gs else "jacobi"
        s = impl.solver(lab, w, levels, use_gs)
        out["levels"] = int(s.levels)
        x = np.zeros(lab.shape)
        s.apply_vcycle(x, b, False)
        out[f"vcycle1_{tag}"] = x.copy()
        for _ in range(3):
            s.apply_vcycle(x, b, True)
        out[f"vcycle4_{tag}"] = x.copy()
        if pcg:
            xs = np.zeros(lab.shape)
            st = s.solve_pcg(xs, b, PCG_TOL, PCG_MAX_ITER, True)
            out[f"pcg_{tag}_iterations"] = int(st["iterations"])
            out[f"pcg_{tag}_history"] = np.array(st["history"])
            out[f"pcg_{tag}_solution"] = xs
            if use_gs:
                xd = np.zeros(lab.shape)
                st = s.solve_pcg(xd, b, PCG_TOL, PCG_MAX_ITER, False)
                out["pcg_diagonal_iterations"] = int(st["iterations"])
                out["pcg_diagonal_history"] = np.array(st["history"])
                out["pcg_diagonal_solution"] = xd
        s.close()
    return out


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
