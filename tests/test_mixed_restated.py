"""The binary16 V-cycle (options.precision = 1) against its restatement, tests/mixed_reference.py: the oracle's operators composed
in the device's order and rounded to binary16 where the device stores binary16.  The kernels behind it --
the __half instances of stencilQuadKernel / boundaryOpKernel (Jacobi, zero-start Jacobi, residual, with and without the gathered
dot), bandBoxKernel / bandBoxCopyKernel, tiledGSMixedKernel / tiledGSPureKernel, restrictKernel / restrictMarchKernel,
prolongAddBlockKernel, fromHalfKernel, zeroChunksHalfKernel, halfDotKernel, xpayHalfKernel, mixSigmaKernel -- have no
operator-level entry; the 2e-3 bound of tests/test_mixed_precision.py leaves them a factor of eight.

One cycle from zero.  The stored iterate is recovered from the fp32 result as x sigma 2^-e: every active cell must be exactly
representable in binary16 and every inactive cell 0 (fromHalfKernel and the scales).  Then, against the restatement on the fp64
oracle (R64), with the restatement on the fp32 oracle (R32) as the measure of what fp32 arithmetic alone does:
  * cells whose binary16 value differs: at most 4 n + 8, n = that count between R32 and R64.  The device's fp32 arithmetic differs
    from the oracle's fp32 build in summation order and contraction only -- the same few fp32 ulps --, and a flip of a binary16
    rounding is a rare, independent event: 4 x and the additive 8 keep a count as small as 9 more than six standard deviations
    away.  tests/test_mixed_reference.py shows on every case that one moved rounding point changes at least 5 x that cap;
  * no cell further from R64 than the largest distance between R32 and R64 plus one binary16 ulp;
  * relative L2 at most 4 x that of R32 against R64.

From a guess (x + M (b - A x), residual and sum in fp32): relative L2 of the fp32 result, same 4 x rule.
MG-PCG capped at k iterations: the iterate against the numpy PCG around R64, bound 4 x (fp32-oracle iterate against fp64-oracle
iterate) + 2e-5 (X_TOL of tests/test_pcg_exits.py, the fp32 recurrence), for the k at which that bound is below half of what the
rounding does to iterate k (PCG_KS = 1; test_mixed_reference.py asserts it), and for k = 2, the first iterate that reads the <z, r>
taken inside the loop and xpayHalfKernel's p: an error of 1e-3 in that dot moves it by more than twice the bound.

Largest values on MI355X: MEASURED at the end of this file.
"""
import numpy as np
import pytest

import mixed_reference as MR
from conftest import rel_l2
from test_mixed_reference import CYCLE_CASES, GUESS_CASE, PCG_DOMAIN, PCG_DOT_K, PCG_KS, SUBNORMALS_WANTED, case, domain, pcg_references, restatement, rhs_of, stored_references

pytestmark = pytest.mark.gpu

UNREACHABLE = 1e-12  # a tolerance nothing reaches in two iterations: the solves end on their iteration cap


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _solver(c, lab, w, lev, **more):
    import geometricmultigridpressuresolver_amd as G

    opt = G.default_options()
    opt.precision = 1
    opt.pre_sweeps = opt.post_sweeps = c["sweeps"]
    opt.band_width, opt.band_iterations, opt.jacobi_weight = c["band"]
    for k, v in more.items():
        setattr(opt, k, v)
    return G.GeometricMultigridPoissonSolver(lab, w, lev, c["use_gs"], options=opt)


@pytest.mark.parametrize("name", list(CYCLE_CASES))
def test_one_cycle_stores_what_the_restatement_stores(name, domain_factory, oracle, oracle32, torch_cuda):
    ref = stored_references(name, domain_factory, oracle, oracle32)
    c, act, r64, r32 = CYCLE_CASES[name], ref["act"], ref["R64"], ref["R32"]
    tiny = lambda v: int(np.count_nonzero((np.abs(v.astype(np.float64)[act]) > 0) & (np.abs(v.astype(np.float64)[act]) < 2.0 ** -14)))  # noqa: E731
    if c["rhs"].startswith("delta"):  # the case is about binary16 subnormals: the reference must store them
        assert tiny(r64) >= SUBNORMALS_WANTED
    s = _solver(c, ref["lab"], ref["w"], ref["lev"])
    try:
        if c["levels"] == 1:
            assert s.getMGLevels() == 1
        x = s.new_grid()
        s.applyVCycle(x, s.to_device(ref["b"]), False)
        xh = x.cpu().numpy()
    finally:
        s.close()
    assert np.isfinite(xh).all() and (xh[~act] == 0).all()
    it = xh.astype(np.float64) / ref["back"]  # the iterate's units (a power of two: exact)
    stored = it.astype(np.float16)
    off_grid = int(np.count_nonzero(stored.astype(np.float64)[act] != it[act]))
    assert off_grid == 0, f"{off_grid} active cells of x sigma 2^-e are no binary16 numbers"
    n32, ulp32, l232 = MR.compare_stored(r32, r64, act)
    n, ulp, l2 = MR.compare_stored(stored, r64, act)
    print(f"MIXED {name}: device against R64: {n} cells, {ulp} ulp, {l2:.2e}; R32 against R64: {n32} cells, {ulp32} ulp, {l232:.2e}; "
          f"cap {4 * n32 + 8}; subnormals stored {tiny(stored)} (R64 {tiny(r64)})")
    if n > 4 * n32 + 8:  # where: labels and position of the differing cells
        d = (stored != r64) & act
        where = np.argwhere(d)
        print(f"MIXED {name}: differing cells by label {np.unique(ref['lab'][d], return_counts=True)}, first {where[:12].tolist()}, "
              f"extent {where.min(0).tolist()} .. {where.max(0).tolist()}")
    assert n <= 4 * n32 + 8, (n, n32)
    assert ulp <= ulp32 + 1, (ulp, ulp32)
    assert l2 <= 4 * l232, (l2, l232)
    if c["rhs"].startswith("delta"):  # no flush: the subnormals R64 stores are stored
        assert abs(tiny(stored) - tiny(r64)) <= 4 * n32 + 8


def test_two_chained_cycles(domain_factory, oracle, oracle32, torch_cuda):
    """the second cycle starts from the first one's result: x + M (b - A x), residual and sum in fp32, only the correction in
    binary16 (launchStencil, vcycleMixed, xpayHalfKernel with beta = 1)"""
    c = GUESS_CASE
    lab, w, off, lev, dx = domain(c, domain_factory)
    b = rhs_of(c, lab, off, dx)
    xs = {}
    for key, orc in (("R64", oracle), ("R32", oracle32)):
        m = restatement(orc, c, lab, w, lev)
        xs[key] = m.apply(b, m.apply(b)).astype(np.float64)
        m.close()
    s = _solver(c, lab, w, lev)
    try:
        x, bd = s.new_grid(), s.to_device(b)
        s.applyVCycle(x, bd, False)
        x1 = x.cpu().numpy().astype(np.float64)
        s.applyVCycle(x, bd, True)
        xh = x.cpu().numpy()
    finally:
        s.close()
    l2, l232, moved = rel_l2(xh, xs["R64"]), rel_l2(xs["R32"], xs["R64"]), rel_l2(xh, x1)
    print(f"MIXED two chained cycles: device against R64 {l2:.2e}; R32 against R64 {l232:.2e}; second cycle moved x by {moved:.2e}")
    assert (xh[~MR.active(lab)] == 0).all() and moved > 100 * l232
    assert l2 <= 4 * l232, (l2, l232)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("use_gs", [False, True])
def test_capped_pcg_leaves_the_restated_iterate(use_gs, mode, domain_factory, oracle, oracle32, torch_cuda):
    """max_iterations = k: k = 1 is alpha z -- z = M b written back in fp32, <z, r> and <p, A p> -- and sees a moved rounding point
    (PCG_KS).  k = 2 is the first iterate that reads what the loop leaves in binary16: <z, r> gathered by the cycle's last stroke
    (Jacobi) or taken by halfDotKernel (Gauss-Seidel), and p = z + beta p (xpayHalfKernel).  CG has corrected half of the
    rounding away by then, so the same bound no longer separates rounding points there; it still sees an error of 1e-3 in that
    dot (test_mixed_reference.py::test_iterate_2_sees_a_wrong_dot) and is asserted for that."""
    ref = pcg_references(use_gs, domain_factory, oracle, oracle32)
    c = case(*PCG_DOMAIN, use_gs)
    s = _solver(c, ref["lab"], ref["w"], ref["lev"], pcg_fp64_vectors=mode)
    failures = []
    try:
        bd = s.to_device(ref["b"])
        for k in (1, 2):
            x = s.new_grid()
            st = s.solveGeometricConjugateGradient(x, bd, UNREACHABLE, k, True)
            xk, bound, effect, d32 = ref[k]
            err = rel_l2(x.cpu().numpy(), xk)
            print(f"MIXED pcg solid48 gs={int(use_gs)} mode={mode} k={k}: device against the restated iterate {err:.2e}; bound {bound:.2e} "
                  f"(fp32 oracle {d32:.2e}); the rounding moves iterate k by {effect:.2e}; rounding points separated: {k in PCG_KS}")
            if st["outcome"] != "max_iterations" or st["iterations"] != k:
                failures.append((k, st))
            if (k in PCG_KS or k == PCG_DOT_K) and not err <= bound:
                failures.append((k, err, bound))
    finally:
        s.close()
    assert not failures, failures


MEASURED = """
MI355X, one cycle from zero, the stored iterate against R64 -- cells that differ / largest distance in binary16 ulps / relative L2,
the device first, then R32 (the same on every machine), then the cap 4 n + 8:

  one-level-simple32      7 / 1 / 5.7e-6     3 / 1 / 5.6e-6    20        solid64-2+2          37 / 1 / 1.3e-5    37 / 1 / 1.1e-5   156
  solid64                43 / 1 / 9.5e-6    32 / 1 / 8.6e-6   136        solid64-gs           43 / 1 / 7.9e-6    33 / 1 / 1.0e-5   140
  complex64              20 / 1 / 6.5e-6    26 / 1 / 7.3e-6   112        random3-gs           97 / 1 / 1.4e-5   102 / 1 / 1.5e-5   416
  widesolid              23 / 1 / 9.1e-6    35 / 1 / 7.6e-6   148        solid64-w2d2o0.8     31 / 1 / 8.1e-6    31 / 1 / 8.9e-6   132
  wide512                62 / 1 / 7.6e-6    69 / 1 / 9.2e-6   284        solid64-w4d4o0.5     22 / 1 / 6.9e-6    24 / 1 / 7.6e-6   104
  random3                91 / 1 / 1.4e-5    94 / 1 / 1.4e-5   384        simple32-max-pow2     3 / 1 / 7.0e-6     3 / 1 / 7.0e-6    20
  random4                58 / 1 / 1.1e-5    63 / 1 / 1.2e-5   260        simple32-max-pow2-ulp 3 / 1 / 7.0e-6     3 / 1 / 7.0e-6    20
  complex32-delta         1 / 1 / 4.7e-7     1 / 1 / 4.7e-7    12   (1 370 binary16 subnormals stored, as many as R64 stores)
  complex32-delta-max-pow2  3 / 1 / 1.5e-5   5 / 1 / 1.5e-5    28   (1 352 subnormals stored, as many as R64 stores)

The largest ratio of the device's count to R32's is 2.3 (7 against 3), of its relative L2 to R32's 1.2; no cell is further than one
binary16 ulp from R64 (allowed: 2); every active cell of x sigma 2^-e was a binary16 number on every case.  On the same cases
the other choice at ONE rounding point changes 604 .. 13 842 cells and no rounding 400 .. 29 930 (tests/test_mixed_reference.py).

Two chained cycles (random3, Gauss-Seidel): 8.8e-6 against R64 (R32: 8.9e-6; bound 3.6e-5); the second cycle moved x by 0.39.

MG-PCG capped at k (solid 48), the device's iterate against the numpy PCG around R64, pcg_fp64_vectors 0 / 1:
  Jacobi        k = 1: 5.2e-6 / 5.2e-6 (bound 4.2e-5; R32 5.6e-6; the rounding moves iterate 1 by 2.2e-4)    k = 2: 4.8e-6 / 4.4e-6 (3.9e-5)
  Gauss-Seidel  k = 1: 1.0e-5 / 1.0e-5 (bound 7.2e-5; R32 1.3e-5; 2.2e-4)                                    k = 2: 1.2e-5 / 1.2e-5 (7.2e-5)

Which power of two sigma is: the simple32-max-pow2 cases run both ends of mixSigmaKernel's interval but cannot tell sigma from
sigma / 2 (a factor of two on every stored value cancels when the iterate is recovered, away from subnormals and saturation).
complex32-delta-max-pow2 can: with sigma = 1/2 for its max |b| = 1, 1 197 cells of the recovered iterate differ from R64
(tests/test_mixed_reference.py::test_the_pow2_delta_case_sees_sigma, CPU); the device differs in 3 (cap 28).
The whole file takes 10 s, the references included.
"""
