"""options.band_width / band_iterations / jacobi_weight away from their defaults (3 / 3 / 2/3) against the fp64 oracle, which
takes the same three options per solver (Oracle.solver(..., band_width=, band_iterations=, jacobi_weight=); the reference
hard-wires them: MG.cpp:141-142, Ops.h:291, 554).  The weight goes to the oracle as float(np.float32(w)): both sides damp by the
same number.

Option sets (width, depth, omega) and what a stroke of them runs -- from band_stage_form, stencil_kernel and the dispatch rules
of strokeForm (mgps_solver.hip):

  set            band stage     Jacobi stroke, quad levels / scalar + plane levels          Gauss-Seidel stroke
  (1, 1, 2/3)    boxes, H 1/2   SF_FRONT (MG-PCG's last stroke: SF_THREE_LAUNCH) / 3-launch  SF_GS_SNAPSHOT
  (2, 2, 0.8)    boxes, H 2/3   the same; 2 + 2 sweeps: SF_FIRST_FUSED;                      SF_GS_SNAPSHOT
                                fuse_band_passes = 0: pass by pass, SF_GENERIC               (fuse 0: SF_GENERIC)
  (4, 4, 0.5)    boxes, H 4/5   SF_FRONT / SF_THREE_LAUNCH                                   SF_GS_SNAPSHOT
  (8, 4, 2/3)    boxes, H 4/5   the same (band_width 8: the device builder's limit)          SF_GS_SNAPSHOT
  (3, 0, 2/3)    none           SF_GENERIC (no band stage, other ghost modes / dot sinks)    SF_GENERIC
  (3, 6, 2/3)    pass by pass   SF_GENERIC (depth > kBandMaxDepth = 4)                       SF_GENERIC
  (5, 2, 1.0)    boxes, H 2/3   SF_FRONT / SF_THREE_LAUNCH                                   SF_GS_SNAPSHOT
  (3, 3, 0.8)    boxes, H 3/4   the default forms, other weight                              SF_GS_SNAPSHOT
  (3, 3, 0.5)    boxes, H 3/4   the default forms, other weight                              SF_GS_SNAPSHOT

(H: passes of bandBoxBody in plain / closure mode.)  SF_PROLONG_FUSED at other options: tests/test_fused_upstroke.py; cut levels
of a slab run: tests/test_distributed.py::test_two_slabs_band_options.

Domains: ("solid", 48) 128^3, 5 levels asked (3 after the level cap), cut cells: width changes the band (11 342 / 21 265 /
29 907 / 37 167 / 43 010 / 53 531 cells on level 0 at widths 1 / 2 / 3 / 4 / 5 / 8) and at depth 4 the halving of the boxes bites
(121 .. 204 groups against 63 at the defaults); ("random", 4) 64 x 64 x 96, 3 levels, general rows in every box -- at depth 4 more
than kBoxMaxGeneral within reach of a single cell, so its fine level runs pass by pass there (_boxes_expected) and keeps boxes
on levels 1 and 2; ("odd", 36) level 1 with nx % 4 != 0: scalar sweep, per-cell band list; ("widesolid", 24) with
stencil_path = 2: the plane sweep, SF_THREE_LAUNCH.

Tolerances are the suite's own: OP_TOL 5e-6 per operator pass, 1e-6 fused against single, 1e-5 (it + 1) per chained V-cycle,
MG-PCG +-2 iterations and 2e-4, MIXED_VCYCLE_TOL 2e-3 (it + 1).  What fp32 alone costs on these very cases -- the oracle's fp32
build (Oracle(f32=True)) against its fp64 build, relative L2 of chained cycle `it` divided by (it + 1), largest of the three
cycles, CPU only:
  solid 48      Jacobi 7.3e-8 .. 7.2e-7 over the nine sets (the largest at depth 0), Gauss-Seidel 9.4e-8 .. 1.9e-7
  random 4      Jacobi 5.8e-8 .. 6.9e-8,  Gauss-Seidel 6.4e-8 .. 7.2e-8
  odd 36        6.2e-8 .. 1.2e-7;  solid 48 with 2 + 2 sweeps 1.1e-7
  widesolid 24  2.0e-7 at (2, 2, 0.8), 1.2e-6 at (4, 4, 0.5), 9.2e-8 at (3, 0, 2/3)
-- 8 x under the bound of 1e-5 at the least: a GPU result outside it is a logic finding.

Not vacuous: every V-cycle case first checks, from the oracle alone, that its first cycle differs from the default-option cycle by
more than 1e-3 relative L2, 100 x the tolerance (measured: solid >= 4.1e-3, random >= 1.8e-2 -- Gauss-Seidel at (4, 4, 0.5) and
(5, 2, 1.0) gives 1.7e-3 / 3.9e-3 there and runs on solid only --, odd >= 1.0e-2, widesolid >= 4.5e-3).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err, rel_l2

pytestmark = pytest.mark.gpu

OP_TOL = 5e-6
VCYCLE_TOL = 1e-5
MIXED_VCYCLE_TOL = 2e-3  # tests/test_mixed_precision.py
DISTINCT = 1e-3          # an option set must move the oracle's cycle by 100 x VCYCLE_TOL, or the case proves nothing

W23 = 2.0 / 3.0
SETS = [(1, 1, W23), (2, 2, 0.8), (4, 4, 0.5), (8, 4, W23), (3, 0, W23), (3, 6, W23), (5, 2, 1.0), (3, 3, 0.8), (3, 3, 0.5)]
# the random-label domain: depths 1, 4 and 6 and both weights (its band saturates from width 3 up: not a domain for widths)
RANDOM_JACOBI = [(1, 1, W23), (2, 2, 0.8), (4, 4, 0.5), (8, 4, W23), (3, 6, W23), (3, 3, 0.8), (3, 3, 0.5)]
RANDOM_GS = [(1, 1, W23), (3, 6, W23), (3, 3, 0.8), (3, 3, 0.5)]
DOMAIN_ARGS = {"odd": (3, (44, 44, 44)), "widesolid": (3, (32, 40, 264))}  # (levels, solver grid), as tests/test_gpu_parity.py


def _sid(s):
    return "w%dd%do%.2f" % s


def _w32(omega):
    return float(np.float32(omega))


def _rand_active(lab, seed, scale=1.0):
    from geometricmultigridpressuresolver_amd import domains as D

    rng = np.random.Generator(np.random.PCG64(seed))
    v = rng.random(lab.shape) * scale
    v[~D.active_mask(lab)] = 0
    return v


def _options(s, **kw):
    import geometricmultigridpressuresolver_amd as G

    opt = G.default_options()
    opt.band_width, opt.band_iterations, opt.jacobi_weight = s[0], s[1], s[2]
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def _band_stage_form(gpu, level):
    from geometricmultigridpressuresolver_amd._lib import check, lib

    form = C.c_int(-1)
    check(lib().mgps_band_stage_form(gpu.h, int(level), C.byref(form)), gpu.h)
    return form.value


def _boxes_expected(gpu, level, depth, labels, band):
    """The form the options imply for a level: boxes for 1 <= band_iterations <= kBandMaxDepth = 4 (with fuse_band_passes) on a
    level that has band cells -- unless a box cannot be formed: halved down to one cell, its region still reaches every band cell
    within `depth` cells of it, and the general ones among them (operator rows, kept in LDS) must number at most kBoxMaxGeneral =
    384.  (2 depth + 1)^3 is 343 at depth 3, 729 at depth 4: only depth 4 on a level crowded with general cells (the random-label
    domain's fine level) runs pass by pass instead.  General cells: band_diag == 0 in the level's set-up arrays."""
    from scipy import ndimage

    if not 1 <= depth <= 4 or len(band) == 0:
        return 0
    if (2 * depth + 1) ** 3 <= 384:
        return 1
    cells, diag = gpu.level_array(level, "band"), gpu.level_array(level, "band_diag")
    assert len(cells) == len(diag) == len(band)
    general, inband = np.zeros(labels.shape, dtype=np.int32), np.zeros(labels.shape, dtype=bool)
    general.flat[cells[diag == 0]] = 1
    inband.flat[cells] = True
    cross = ndimage.generate_binary_structure(3, 1)
    closure = inband | (np.isin(labels, (0, 3)) & ndimage.binary_dilation(inband, cross))  # what a box owns: band cells and their active face neighbours
    within = ndimage.uniform_filter(general.astype(np.float64), size=2 * depth + 1, mode="constant") * (2 * depth + 1) ** 3
    return int(np.rint(within[closure].max()) <= 384)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def cases(domain_factory, oracle, torch_cuda):
    """(kind, g, option set, smoother, sweeps, other options) -> the GPU solver, the oracle solver at the same options, the
    domain and one rhs; built once and shared by the tests of this module.  default_cycle: the oracle's first cycle on that rhs
    with the default band options (same smoother and sweep counts)."""
    import geometricmultigridpressuresolver_amd as G

    cache, defaults = {}, {}

    class Case:
        pass

    def domain(kind, g):
        lev, shape = DOMAIN_ARGS.get(kind, (None, None))
        lab, w, off, lev, dx = domain_factory(kind, g, lev, shape)
        return lab, w, lev, dx

    def get(kind, g, s, use_gs, sweeps=1, **kw):
        key = (kind, g, s, use_gs, sweeps, tuple(sorted(kw.items())))
        if key not in cache:
            c = Case()
            c.lab, c.w, c.lev, c.dx = domain(kind, g)
            c.lab32, c.w64 = c.lab.astype(np.int32), [a.astype(np.float64) for a in c.w]
            c.gpu = G.GeometricMultigridPoissonSolver(c.lab, c.w, c.lev, use_gs, options=_options(s, pre_sweeps=sweeps, post_sweeps=sweeps, **kw))
            c.orc = oracle.solver(c.lab32, c.w64, c.lev, use_gs, pre_sweeps=sweeps, post_sweeps=sweeps,
                                  band_width=s[0], band_iterations=s[1], jacobi_weight=_w32(s[2]))
            c.b32 = _rand_active(c.lab, 5, c.dx * c.dx).astype(np.float32)
            c.b64 = c.b32.astype(np.float64)
            cache[key] = c
        return cache[key]

    def default_cycle(kind, g, use_gs, sweeps=1):
        key = (kind, g, use_gs, sweeps)
        if key not in defaults:
            lab, w, lev, dx = domain(kind, g)
            orc = oracle.solver(lab.astype(np.int32), [a.astype(np.float64) for a in w], lev, use_gs, pre_sweeps=sweeps, post_sweeps=sweeps)
            b = _rand_active(lab, 5, dx * dx).astype(np.float32).astype(np.float64)
            x = np.zeros_like(b)
            orc.apply_vcycle(x, b, False)
            x.setflags(write=False)
            defaults[key] = x
        return defaults[key]

    get.default_cycle = default_cycle
    yield get
    for c in cache.values():
        c.gpu.close()
        c.orc.close()


# ---- refusals that exist ----------------------------------------------------------------------------------------------------
def test_option_refusals(domain_factory, torch_cuda):
    """band_width 0 and band_iterations -1: MGPS_ERR_INVALID_ARGUMENT from both builders; band_width 9: from the device builder
    (its band masks take up to 8); precision = 1 needs the box form of the band stage, 1 <= band_iterations <= 4."""
    import geometricmultigridpressuresolver_amd as G

    lab, w, off, lev, dx = domain_factory("simple", 32)
    for host in (0, 1):
        for s in ((0, 3, W23), (3, -1, W23)):
            with pytest.raises(G.MgpsError) as e:
                G.GeometricMultigridPoissonSolver(lab, w, lev, False, options=_options(s, host_setup=host))
            assert e.value.status == 1 and "band_width >= 1" in str(e.value), (host, s, str(e.value))
    with pytest.raises(G.MgpsError) as e:
        G.GeometricMultigridPoissonSolver(lab, w, lev, False, options=_options((9, 3, W23)))
    assert e.value.status == 1 and "<= 8" in str(e.value), str(e.value)
    for depth in (0, 5):
        with pytest.raises(G.MgpsError) as e:
            G.GeometricMultigridPoissonSolver(lab, w, lev, False, options=_options((3, depth, W23), precision=1))
        assert e.value.status == 1 and "1 <= band_iterations <= 4" in str(e.value), (depth, str(e.value))
    # depth 4 on a fine level crowded with general cells: no boxes can be formed (_boxes_expected); fp32 runs such a level pass by
    # pass, the binary16 fine level has no such stage and is refused -- by both builders
    lab, w, off, lev, dx = domain_factory("random", 4)
    for host in (0, 1):
        with pytest.raises(G.MgpsError) as e:
            G.GeometricMultigridPoissonSolver(lab, w, lev, False, options=_options((3, 4, W23), precision=1, host_setup=host))
        assert e.value.status == 1 and "band_iterations <= 3" in str(e.value), (host, str(e.value))


# ---- operators, per level ---------------------------------------------------------------------------------------------------
OPERATOR_CASES = ([("solid", 48, s) for s in SETS] + [("random", 4, s) for s in RANDOM_JACOBI]
                  + [("odd", 36, s) for s in ((1, 1, W23), (2, 2, 0.8), (4, 4, 0.5), (3, 6, W23), (5, 2, 1.0))])


@pytest.mark.parametrize("kind,g,s", OPERATOR_CASES, ids=[f"{k}{g}-{_sid(s)}" for k, g, s in OPERATOR_CASES])
def test_operators_per_level(kind, g, s, cases, oracle):
    """On every level: the band list at this width is the oracle's; the band stage runs in the form the depth implies (boxes for
    1 .. kBandMaxDepth = 4 with fuse_band_passes on a level that has band cells, pass by pass otherwise); one Jacobi sweep and one
    band pass at this weight against the oracle (_boxes_expected: the one exception at depth 4); the stage against `depth` oracle passes and against `depth` single-pass
    launches of the same library (same arithmetic per cell: a different fused-multiply-add contraction only)."""
    c = cases(kind, g, s, False)
    bw, depth, omega = s
    gpu, orc, w = c.gpu, c.orc, _w32(omega)
    assert gpu.getMGLevels() == orc.levels
    H = gpu.hierarchy()
    for l in range(orc.levels):
        ll, band = orc.level_labels(l), orc.band(l)
        assert np.array_equal(H.band_cells(l), band), l
        assert _band_stage_form(gpu, l) == _boxes_expected(gpu, l, depth, ll, band), (l, depth)
        if kind != "random" or l > 0:  # (every level but the random-label domain's fine one keeps its boxes at depth 4)
            assert _band_stage_form(gpu, l) == int(1 <= depth <= 4 and len(band) > 0), (l, depth)
        wl = c.w64 if l == 0 else None
        x0 = _rand_active(ll, 30 + l)
        b0 = _rand_active(ll, 40 + l)
        bd = gpu.to_device(b0, l)
        # jacobiPoissonSmoother at this weight
        xj, xj23 = x0.copy(), x0.copy()
        oracle.jacobi(xj, b0, ll, wl, weight=w)
        xjd = gpu.to_device(x0, l)
        gpu.jacobiPoissonSmoother(xjd, bd, level=l)
        assert rel_err(xjd.cpu().numpy(), xj) < OP_TOL, l
        if omega != W23:  # (from the oracle alone: the weight matters 100 x more than the tolerance)
            oracle.jacobi(xj23, b0, ll, wl)
            assert rel_err(xj, xj23) > 100 * OP_TOL, l
        # boundaryJacobiPoissonSmoother: one pass over this width's list
        xb = x0.copy()
        oracle.boundary_jacobi(xb, b0, ll, band, wl, weight=w)
        xbd = gpu.to_device(x0, l)
        gpu.boundaryJacobiPoissonSmoother(xbd, bd, level=l)
        assert rel_err(xbd.cpu().numpy(), xb) < OP_TOL, l
        # the stage: `depth` passes
        xb = x0.copy()
        for _ in range(depth):
            oracle.boundary_jacobi(xb, b0, ll, band, wl, weight=w)
        fused, single = gpu.to_device(x0, l), gpu.to_device(x0, l)
        gpu.boundaryJacobiStage(fused, bd, level=l)
        for _ in range(depth):
            gpu.boundaryJacobiPoissonSmoother(single, bd, level=l)
        assert rel_err(fused.cpu().numpy(), xb) < OP_TOL, l
        assert rel_err(fused.cpu().numpy(), single.cpu().numpy().astype(np.float64)) < 1e-6, l
        if (bw, depth) != (3, 3) and len(band) > 0:  # (from the oracle alone: not the default stage)
            x3, band3 = x0.copy(), oracle.build_boundary_cells(ll, 3)
            for _ in range(3):
                oracle.boundary_jacobi(x3, b0, ll, band3, wl)
            assert rel_err(xb, x3) > 100 * OP_TOL, l


# ---- V-cycle ----------------------------------------------------------------------------------------------------------------
def _vcycle_check(c, x_default):
    gpu, orc = c.gpu, c.orc
    x_ref = np.zeros_like(c.b64)
    xd, bd = gpu.new_grid(), gpu.to_device(c.b32)
    errs = []
    for it in range(3):
        orc.apply_vcycle(x_ref, c.b64, it > 0)
        if it == 0:
            distinct = rel_l2(x_ref, x_default)
            assert distinct > DISTINCT, distinct
        gpu.applyVCycle(xd, bd, it > 0)
        errs.append(rel_l2(xd.cpu().numpy(), x_ref))
        print(f"cycle {it}: rel_l2 {errs[-1]:.3e} (bound {VCYCLE_TOL * (it + 1):.0e}); first cycle against default options {distinct:.2e}")
        assert errs[-1] < VCYCLE_TOL * (it + 1), (it, errs)
    x = xd.cpu().numpy()
    assert (x[~np.isin(c.lab, (0, 3))] == 0).all()  # zero outside active cells (Ops.h:821-823)


VCYCLE_CASES = ([("solid", 48, s, gs) for s in SETS for gs in (False, True)]
                + [("random", 4, s, False) for s in RANDOM_JACOBI] + [("random", 4, s, True) for s in RANDOM_GS]
                + [("odd", 36, (2, 2, 0.8), False), ("odd", 36, (4, 4, 0.5), False), ("odd", 36, (3, 6, W23), False), ("odd", 36, (1, 1, W23), True)])


@pytest.mark.parametrize("kind,g,s,use_gs", VCYCLE_CASES, ids=[f"{k}{g}-{_sid(s)}-{'gs' if gs else 'jacobi'}" for k, g, s, gs in VCYCLE_CASES])
def test_vcycle_matches_oracle(kind, g, s, use_gs, cases):
    """Three chained cycles against the oracle at the same options, both smoothers; inactive cells exactly 0."""
    _vcycle_check(cases(kind, g, s, use_gs), cases.default_cycle(kind, g, use_gs))


def test_vcycle_two_sweeps_depth_two(cases):
    """pre_sweeps = post_sweeps = 2 with depth 2: SF_FIRST_FUSED (the first band stage and the first sweep in two launches)."""
    _vcycle_check(cases("solid", 48, (2, 2, 0.8), False, sweeps=2), cases.default_cycle("solid", 48, False, sweeps=2))


@pytest.mark.parametrize("use_gs", [False, True])
def test_vcycle_unfused_band_passes(use_gs, cases):
    """fuse_band_passes = 0 at depth 2: a launch pair per pass, SF_GENERIC with either smoother."""
    c = cases("solid", 48, (2, 2, 0.8), use_gs, fuse_band_passes=0)
    assert all(_band_stage_form(c.gpu, l) == 0 for l in range(c.gpu.getMGLevels()))
    _vcycle_check(c, cases.default_cycle("solid", 48, use_gs))


@pytest.mark.parametrize("s", [(2, 2, 0.8), (4, 4, 0.5), (3, 0, W23)], ids=_sid)
def test_vcycle_plane_sweep(s, cases):
    """options.stencil_path = 2: stencilPlaneKernel on the fine level, whose strokes run as closure launch, sweep, plain launch
    (SF_THREE_LAUNCH) -- at depth 0 as the generic stroke."""
    c = cases("widesolid", 24, s, False, stencil_path=2)
    assert c.gpu.stencil_kernel(0) == "plane" and _band_stage_form(c.gpu, 0) == int(s[1] > 0)  # (depths 2, 4, 0)
    _vcycle_check(c, cases.default_cycle("widesolid", 24, False))


# ---- MG-PCG -----------------------------------------------------------------------------------------------------------------
PCG_CASES = ([("solid", 48, s, gs) for s in SETS for gs in (False, True)]
             + [("random", 4, s, False) for s in RANDOM_JACOBI] + [("random", 4, s, True) for s in RANDOM_GS])


@pytest.mark.parametrize("kind,g,s,use_gs", PCG_CASES, ids=[f"{k}{g}-{_sid(s)}-{'gs' if gs else 'jacobi'}" for k, g, s, gs in PCG_CASES])
def test_pcg_matches_oracle(kind, g, s, use_gs, cases):
    """MG-PCG to 1e-5 (the preconditioning cycle's last stroke gathers <z, r>: other sinks at depth 0 and 6): converged, the
    oracle's iteration count +-2, the oracle's pressure to 2e-4 -- the bounds of test_sweep_counts_match_oracle."""
    c = cases(kind, g, s, use_gs)
    x_ref = np.zeros(c.lab.shape)
    ref = c.orc.solve_pcg(x_ref, c.b64, 1e-5, 200, True)
    assert ref["status"] == 0 and 5 <= ref["iterations"] <= 25, ref
    xs = c.gpu.new_grid()
    st = c.gpu.solveGeometricConjugateGradient(xs, c.gpu.to_device(c.b32), 1e-5, 200, True)
    err = rel_l2(xs.cpu().numpy(), x_ref)
    print(f"iterations {st['iterations']} (oracle {ref['iterations']}), pressure rel_l2 {err:.3e}")
    assert st["outcome"] == "converged" and abs(st["iterations"] - ref["iterations"]) <= 2, (st, ref["iterations"])
    assert err < 2e-4


def test_gathered_dot_at_band_options(torch_cuda):
    """MGPS_CHECK_FUSED_DOT=1 (read once per process, hence the child): every <z, r> gathered from the last stroke -- sweep partial
    sums + band corrections, whose sinks are counted from band_iterations -- must equal a separate reduction to 1e-9: depths 0, 1,
    4 and 6 and omega = 0.8, both smoothers, cut-cell and random-label domains."""
    import os
    import subprocess
    import sys

    from conftest import ROOT

    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests')\n"
        "import numpy as np\n"
        "import geometricmultigridpressuresolver_amd as G\n"
        "from geometricmultigridpressuresolver_amd import domains as D\n"
        "from conftest import make_domain\n"
        "for kind, g in (('solid', 48), ('random', 4)):\n"
        "    lab, w, off, lev, dx = make_domain(kind, g)\n"
        "    b = D.random_rhs(lab, dx)\n"
        "    for bw, bi, om in ((3, 0, 2 / 3), (1, 1, 2 / 3), (4, 4, 0.5), (3, 6, 2 / 3), (3, 3, 0.8)):\n"
        "        for gs in (False, True):\n"
        "            o = G.default_options()\n"
        "            o.band_width, o.band_iterations, o.jacobi_weight = bw, bi, om\n"
        "            s = G.GeometricMultigridPoissonSolver(lab, w, lev, gs, options=o)\n"
        "            x = s.new_grid()\n"
        "            st = s.solveGeometricConjugateGradient(x, s.to_device(b), 1e-6, 200, True)\n"
        "            assert st['outcome'] == 'converged', (kind, bw, bi, om, gs, st)\n"
        "            s.close()\n"
        "print('GATHER_OK')\n"
    ) % (ROOT, ROOT)
    env = dict(os.environ, MGPS_CHECK_FUSED_DOT="1")
    res = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    assert res.returncode == 0 and "GATHER_OK" in res.stdout, res.stdout[-3000:]


# ---- mixed precision --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,use_gs", [((2, 2, 0.8), False), ((4, 4, 0.5), False), ((4, 4, 0.5), True)], ids=lambda v: _sid(v) if isinstance(v, tuple) else ("gs" if v else "jacobi"))
def test_mixed_vcycle_matches_oracle(s, use_gs, cases):
    """options.precision = 1 (binary16 iterate and residual on the fine level; the mixed cycle has its own box launches and its
    own weight arguments) at other depths and weights: the bound of tests/test_mixed_precision.py, and the mixed error still
    exceeds 10 x the fp32 path's -- it is the reduced-precision path that ran."""
    mix, f32 = cases("solid", 64, s, use_gs, precision=1), cases("solid", 64, s, use_gs)
    b = (f32.b32 * 37.0).astype(np.float32)  # any magnitude: the cycle normalises by a power of two
    x_ref = np.zeros(mix.lab.shape)
    xm, xf = mix.gpu.new_grid(), f32.gpu.new_grid()
    bm, bf = mix.gpu.to_device(b), f32.gpu.to_device(b)
    for it in range(3):
        mix.orc.apply_vcycle(x_ref, b.astype(np.float64), it > 0)
        mix.gpu.applyVCycle(xm, bm, it > 0)
        f32.gpu.applyVCycle(xf, bf, it > 0)
        err, err32 = rel_l2(xm.cpu().numpy(), x_ref), rel_l2(xf.cpu().numpy(), x_ref)
        print(f"cycle {it}: mixed {err:.3e}, fp32 {err32:.3e}")
        assert err < MIXED_VCYCLE_TOL * (it + 1), (it, err)
        assert err32 < VCYCLE_TOL * (it + 1) and err > 10 * err32, (it, err, err32)
    x = xm.cpu().numpy()
    assert np.isfinite(x).all() and (x[~np.isin(mix.lab, (0, 3))] == 0).all()
