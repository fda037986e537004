"""The CPU oracle (oracle/mg_oracle.c) against the reference's own solver core, compiled unchanged
(oracle/ref_driver.cpp over oracle/ref_standin/, `make -C oracle ref`), and the HIP kernels against numbers the
reference made.

Three groups:
  * fixture tests (CPU, always run): tests/golden/ref_*.npz hold what the compiled reference computed
    (tests/golden/make_ref_golden.py); the oracle must reproduce every per-cell result bit for bit;
  * live tests (CPU, skipped where oracle/_ref/libmgref.so was not built): the binary reproduces the fixtures,
    and the same comparisons on further random domains and band options;
  * GPU tests: the oracle's results are first shown to be the reference's (by hash), then the kernels are held to
    them; the V-cycles are held to the stored reference arrays.

Tolerances.  Per-cell results: none, both sides are fp64 with contraction off and the oracle claims the
reference's visiting and accumulation order.  Reductions: |oracle - ref| <= 2 n eps sum|a_i b_i|, the bound for
two summation orders of the same n products (reference_cases.reduction_bounds).  V-cycles and PCG can differ only
through the coarse direct solve (the reference uses a sparse Cholesky factorisation, its compiled stand-in a dense
one, the oracle a banded one).  The sensitivity to that solve is measured on the reference alone: the largest
relative max-norm difference, over all four cases and all V-cycle / PCG results, between its build with the
factorisation in double and in long double is 2.50e-15 (`coarse_sensitivity` in every fixture); the tolerance is
10 times that (`tolerance_factor`), 2.50e-14, because the oracle's factorisation is a third algorithm.  (As
measured, the oracle's banded factorisation performs the same operations as the dense one in the same order and
the results are equal; the tolerance is what the comparison is entitled to, not what it needs.)  PCG iteration
counts must be equal and residual histories agree to the same tolerance.
"""
import os

import numpy as np
import pytest

import reference_cases as R
from conftest import rel_err, rel_l2
from oracle import mg_ref
from test_gpu_parity import OP_TOL, VCYCLE_TOL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = list(R.CASES)
ARRAYS = ("vcycle1_jacobi", "vcycle4_jacobi", "vcycle1_gs", "vcycle4_gs")

needs_reference = pytest.mark.skipif(
    not (mg_ref.available() and mg_ref.available(long_double=True)),
    reason=f"oracle/_ref/libmgref.so and libmgref_ld.so are not built: run `{mg_ref.BUILD_HINT}` with a checkout of the reference",
)


def key(name):
    return name.replace("/", ".")


@pytest.fixture(scope="module")
def golden():
    cache = {}

    def get(name):
        if name not in cache:
            with np.load(os.path.join(GOLDEN, f"ref_{name}.npz")) as z:
                cache[name] = {k: z[k] for k in z.files}
        return cache[name]

    return get


@pytest.fixture(scope="module")
def case_domain():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = R.solver_domain(name)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def oracle_per_cell(oracle, case_domain):
    """The oracle's per-cell results of a case, computed once: (hashes, arrays)."""
    cache = {}

    def get(name):
        if name not in cache:
            lab, w, off, lev, dx = case_domain(name)
            arrays = {}
            cache[name] = (R.per_cell(oracle, lab, w, lev, dx, keep=arrays), arrays)
        return cache[name]

    return get


def tolerance(g):
    return float(g["tolerance_factor"]) * float(g["coarse_sensitivity"])


def assert_hashes(got, g):
    wrong = [k for k, v in got.items() if str(g[key(k)]) != str(v)]
    assert not wrong, f"differs from the reference: {wrong}"


def assert_cycles(got, ref, tol):
    """got / ref: results of reference_cases.cycles (ref may hold only what a fixture stores)."""
    assert got["levels"] == int(ref["levels"])
    for k, v in got.items():
        if k.endswith("_iterations"):
            assert v == int(ref[k]), k
        elif k.endswith("_history"):
            assert len(v) == len(ref[k]), k
            assert R.rel_max(v, ref[k]) <= tol, k
        elif k in ref and isinstance(v, np.ndarray):
            assert R.rel_max(v, ref[k]) <= tol, k


# ---- fixture tests: CPU, always run -----------------------------------------------------------------------------


@pytest.mark.parametrize("name", NAMES)
def test_inputs_reproduce_their_hashes(name, golden, case_domain):
    lab, w, off, lev, dx = case_domain(name)
    g = golden(name)
    assert tuple(g["shape"]) == lab.shape and int(g["offset"]) == off and int(g["levels_requested"]) == lev and float(g["dx"]) == dx
    assert_hashes(R.input_hashes(lab, w, dx), g)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_per_cell_operators_equal_reference(name, golden, oracle_per_cell):
    """Labels, band lists, apply, residual, Jacobi, each band pass, each Gauss-Seidel pass, both transfers and the vector
    operations, on every level, bit for bit."""
    hashes, _ = oracle_per_cell(name)
    g = golden(name)
    assert sum(k.endswith("/labels") for k in hashes) == int(g["levels_requested"])
    assert_hashes(hashes, g)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_expansion_and_structure_checks_equal_reference(name, golden, oracle, case_domain):
    lab, w, off, lev, dx = case_domain(name)
    g = golden(name)
    got = R.expansion(oracle, name)
    assert tuple(g["expand.shape"]) == got.pop("expand/shape")
    assert_hashes(got, g)
    checks = R.structure_checks(oracle, lab, w, lev)
    assert all(bool(g[key(k)]) for k in checks)  # the reference passes its own checks on these domains
    assert_hashes(checks, g)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_solver_hierarchy_equals_reference(name, golden, oracle, case_domain):
    """The hierarchy the oracle's solver object holds (not only its free functions), and the reference's level cap:
    "solid24" asks for 4 levels and both keep 2 (MG.cpp:243-248 drops one level more than it needs to)."""
    lab, w, off, lev, dx = case_domain(name)
    g = golden(name)
    s = oracle.solver(lab, w, lev, True)
    assert s.levels == int(g["levels"])
    for l in range(s.levels):
        assert R.sha(s.level_labels(l)) == str(g[f"L{l}.labels"]), l
        assert R.sha(s.band(l).astype(np.int32)) == str(g[f"L{l}.band"]), l
    s.close()


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reductions_within_summation_bound(name, golden, oracle, case_domain):
    lab = case_domain(name)[0]
    g = golden(name)
    got, bound = R.reductions(oracle, lab), R.reduction_bounds(lab)
    for k, v in got.items():
        assert abs(v - float(g["reduce." + k])) <= bound[k], (k, v, float(g["reduce." + k]), bound[k])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_cycles_and_pcg_within_coarse_solve_tolerance(name, golden, oracle, case_domain):
    lab, w, off, lev, dx = case_domain(name)
    g = golden(name)
    got = R.cycles(oracle, lab, w, lev, dx)
    assert all(k in g for k in ARRAYS)
    assert_cycles(got, g, tolerance(g))


def test_fixture_tolerance_is_the_measured_one(golden):
    """Every fixture carries the same measured sensitivity (the maximum over the cases) and the factor the docstring states."""
    gs = [golden(n) for n in NAMES]
    assert len({float(g["coarse_sensitivity"]) for g in gs}) == 1
    assert float(gs[0]["coarse_sensitivity"]) == max(float(g["case_sensitivity"]) for g in gs)
    assert float(gs[0]["tolerance_factor"]) == 10.0
    assert 0 < tolerance(gs[0]) < 1e-12  # a few hundred eps at the most: a direct solve of a small SPD system


# ---- live tests: CPU, need the compiled reference ----------------------------------------------------------------


@pytest.fixture(scope="module")
def reference():
    return mg_ref.Reference()


@pytest.fixture(scope="module")
def reference_ld():
    return mg_ref.Reference(long_double=True)


@needs_reference
@pytest.mark.parametrize("name", NAMES)
def test_live_reference_reproduces_fixture(name, golden, reference, reference_ld, case_domain):
    lab, w, off, lev, dx = case_domain(name)
    g = golden(name)
    assert_hashes(R.per_cell(reference, lab, w, lev, dx), g)
    got = R.expansion(reference, name)
    assert tuple(g["expand.shape"]) == got.pop("expand/shape")
    assert_hashes(got, g)
    assert_hashes(R.structure_checks(reference, lab, w, lev), g)
    for k, v in R.reductions(reference, lab).items():
        assert v == float(g["reduce." + k]), k
    cyc, cyc_ld = R.cycles(reference, lab, w, lev, dx), R.cycles(reference_ld, lab, w, lev, dx)
    assert_cycles(cyc, g, 0.0)
    for k in ARRAYS:
        assert (cyc[k] == g[k]).all(), k
    measured = max(R.rel_max(cyc_ld[k], v) for k, v in cyc.items() if isinstance(v, np.ndarray))
    assert measured == float(g["case_sensitivity"]) <= float(g["coarse_sensitivity"])


def _compare_live(oracle, reference, lab, w, lev, dx, tol, band_width=R.BAND_WIDTH, band_passes=R.BAND_PASSES, cycles=True):
    ref_hashes = R.per_cell(reference, lab, w, lev, dx, band_width, band_passes)
    got = R.per_cell(oracle, lab, w, lev, dx, band_width, band_passes)
    wrong = [k for k in ref_hashes if got[k] != ref_hashes[k]]
    assert not wrong, f"differs from the reference: {wrong}"
    assert R.structure_checks(oracle, lab, w, lev) == R.structure_checks(reference, lab, w, lev)
    r_got, r_ref, bound = R.reductions(oracle, lab), R.reductions(reference, lab), R.reduction_bounds(lab)
    for k in r_ref:
        assert abs(r_got[k] - r_ref[k]) <= bound[k], k
    if cycles:
        assert_cycles(R.cycles(oracle, lab, w, lev, dx), R.cycles(reference, lab, w, lev, dx), tol)


@needs_reference
@pytest.mark.parametrize("seed", [4, 5, 6])
def test_live_random_domains(seed, golden, oracle, reference):
    """Blobs of every label and fractional weights on a 32 x 32 x 48 grid with 3 levels: general rows everywhere."""
    lab, w, off, lev, dx = R.random_solver_domain(seed)
    _compare_live(oracle, reference, lab, w, lev, dx, tolerance(golden(NAMES[0])))


@needs_reference
@pytest.mark.parametrize("band_width,band_passes", [(2, 3), (3, 2)])
def test_live_band_options(band_width, band_passes, golden, oracle, reference, case_domain):
    """Band lists of another width and another number of band passes, per level, on the domain with partial tiles; and
    the lists the oracle's solver object rebuilds for that width.  (The reference's solver object hard-wires 3 / 3, so
    there is no reference V-cycle for other options.)"""
    lab, w, off, lev, dx = case_domain("ragged")
    _compare_live(oracle, reference, lab, w, lev, dx, 0.0, band_width, band_passes, cycles=False)
    s = oracle.solver(lab, w, lev, False, band_width=band_width, band_iterations=band_passes)
    labs, bands = R.hierarchy(reference, lab, lev, band_width)
    for l in range(s.levels):
        assert (s.band(l) == bands[l]).all(), l
    s.close()


@needs_reference
def test_live_expanded_layout_rule(oracle, reference):
    """The sizing rule of buildExpandedCellLabels (levels from the smallest extent, padding, power-of-two rounding) on
    base grids around powers of two, where ceil(log2) steps."""
    for base in [(4, 4, 4), (5, 9, 17), (8, 8, 8), (15, 16, 17), (16, 16, 16), (17, 33, 20), (31, 32, 33), (36, 28, 20), (64, 24, 40)]:
        assert oracle.expanded_layout(*base) == reference.expanded_layout(*base), base


# ---- GPU tests ------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _gpu_solver(lab, w, lev, use_gs):
    import geometricmultigridpressuresolver_amd as G

    return G.GeometricMultigridPoissonSolver(lab.astype(np.uint8), [a.astype(np.float32) for a in w], lev, use_gs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_operators_against_reference_pinned_oracle(name, golden, case_domain, oracle_per_cell, torch_cuda):
    """Every operator on every level.  The oracle's result is first shown to be the reference's, then the kernel is
    held to it: OP_TOL in rel_err, 4 OP_TOL after the four Gauss-Seidel passes (test_gpu_parity.py's constants)."""
    lab, w, off, lev, dx = case_domain(name)
    g = golden(name)
    hashes, ref = oracle_per_cell(name)
    assert_hashes(hashes, g)
    gpu = _gpu_solver(lab, w, lev, False)
    levels = gpu.getMGLevels()
    assert levels == int(g["levels"])
    H = gpu.hierarchy()
    for l in range(levels):
        ll = ref[f"L{l}/labels"]
        assert R.sha(np.ascontiguousarray(H.level_labels(l), dtype=np.int32)) == str(g[f"L{l}.labels"]), l
        assert R.sha(np.ascontiguousarray(H.band_cells(l), dtype=np.int32)) == str(g[f"L{l}.band"]), l
        x0 = R.rand_active(ll, 1) if l == 0 else R.rand_active(ll, 10 + l)
        b0 = R.rand_active(ll, 2, dx * dx) if l == 0 else R.rand_active(ll, 20 + l)
        xd, bd = gpu.to_device(x0, l), gpu.to_device(b0, l)

        yd = gpu.new_grid(l)
        gpu.applyPoissonMatrix(yd, xd, level=l)
        assert rel_err(yd.cpu().numpy(), ref[f"L{l}/apply"]) < OP_TOL, l
        rd = gpu.new_grid(l)
        gpu.computePoissonResidual(rd, xd, bd, level=l)
        assert rel_err(rd.cpu().numpy(), ref[f"L{l}/residual"]) < OP_TOL, l
        xjd = gpu.to_device(x0, l)
        gpu.jacobiPoissonSmoother(xjd, bd, level=l)
        assert rel_err(xjd.cpu().numpy(), ref[f"L{l}/jacobi"]) < OP_TOL, l
        xbd = gpu.to_device(x0, l)
        for _ in range(3):
            gpu.boundaryJacobiPoissonSmoother(xbd, bd, level=l)
        assert rel_err(xbd.cpu().numpy(), ref[f"L{l}/band_pass3"]) < OP_TOL, l
        xgd = gpu.to_device(x0, l)
        for odd, fwd in R.GS_PASSES:
            gpu.tiledGaussSeidelPoissonSmoother(xgd, bd, odd, fwd, level=l)
        assert rel_err(xgd.cpu().numpy(), ref[f"L{l}/gs_pass4"]) < 4 * OP_TOL, l
        if l + 1 < levels:
            cl = ref[f"L{l + 1}/labels"]
            cd = gpu.new_grid(l + 1)
            gpu.downsample(cd, gpu.to_device(R.rand_active(ll, 30 + l), l), fine_level=l)
            assert rel_err(cd.cpu().numpy(), ref[f"L{l}/downsample"]) < OP_TOL, l
            fd = gpu.to_device(R.rand_active(ll, 50 + l), l)
            gpu.upsampleAndAdd(fd, gpu.to_device(R.rand_active(cl, 40 + l), l + 1), fine_level=l)
            assert rel_err(fd.cpu().numpy(), ref[f"L{l}/upsample_add"]) < OP_TOL, l
    gpu.close()


@pytest.mark.gpu
@pytest.mark.parametrize("use_gs", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_gpu_vcycles_and_pcg_against_reference(name, use_gs, golden, case_domain, torch_cuda):
    """One and four chained V-cycles against the arrays the reference computed (VCYCLE_TOL k in relative L2 after k
    cycles), and MG-PCG's iteration count within 2 of the reference's."""
    lab, w, off, lev, dx = case_domain(name)
    g = golden(name)
    tag = "gs" if use_gs else "jacobi"
    gpu = _gpu_solver(lab, w, lev, use_gs)
    bd = gpu.to_device(R.rand_active(lab, 5, dx * dx))
    xd = gpu.new_grid()
    for k in range(1, 5):
        gpu.applyVCycle(xd, bd, k > 1)
        if k in (1, 4):
            assert rel_l2(xd.cpu().numpy(), g[f"vcycle{k}_{tag}"]) < VCYCLE_TOL * k, k
    xs = gpu.new_grid()
    st = gpu.solveGeometricConjugateGradient(xs, bd, R.PCG_TOL, R.PCG_MAX_ITER, True)
    assert st["outcome"] == "converged"
    assert abs(st["iterations"] - int(g[f"pcg_{tag}_iterations"])) <= 2, (st["iterations"], int(g[f"pcg_{tag}_iterations"]))
    gpu.close()
