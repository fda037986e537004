"""The fields oracle (oracle/mg_fields_oracle.c) and the device field passes (csrc/mgps_fields.hip) against the reference's
own plugin, compiled unchanged (oracle/ref_fields_driver.cpp over oracle/ref_standin/, `make -C oracle ref`).

Three groups, as in test_reference_parity.py:
  * fixture tests (CPU, always run): tests/golden/ref_fields_*.npz hold what the compiled reference computed
    (tests/golden/make_ref_fields_golden.py); the oracle must reproduce every per-cell pass bit for bit;
  * live tests (CPU, skipped where oracle/_ref/libmgref_fields.so was not built): the binary reproduces the fixtures, and
    the same comparisons on three random scenes;
  * GPU tests: the oracle's arrays are first shown to be the reference's (by hash), then every device pass is held to them,
    and mgps_project_free_surface to the reference's tight run.  They read fixtures and the oracle only.

Scenes (tests/reference_fields_cases.py): `pool` and `pool_solid`, projection_scene((24, 20, 28)) without and with solid
velocity, and `edge`, 11 x 13 x 70 built by hand so that every branch of the reference's per-cell rules occurs
(test_edge_scene_has_every_configuration asserts each).

Tolerances.  Per-cell passes: none.  The oracle is fp64 on the same float32 inputs and its result is rounded to the type the
reference stores it in.  The report: count and maximum exact, the sum within 2 n eps64 sum|terms| (two summation orders).
The whole call through the oracle pipeline: iteration counts equal, valid faces equal, and the oracle's double pressure
within half a float32 ulp of the reference's float32 pressure (the rounding the reference applies where it stores) plus
`oracle_factor` (10) x `sensitivity` x max|p|; sensitivity = the largest relative max-norm difference of the reference's
solution grid between its builds with the coarse Cholesky factorisation in double and in long double, 3.83e-16 (in every
fixture).  The velocity likewise, plus what a differing float32 pressure could add across a face (2 dp / 0.01).  As
measured, pressures and velocities are equal bit for bit.

Device bounds are per element, from the kernel's own expression (eps = eps32 = 2^-23, u = eps / 2 one rounding):
  * weights: t = phi0 - phi1, theta = phi / t, w = cw / theta: three roundings, 1.5 eps, and the clamp's lower end is the
    float 0.01f where the reference has the double 0.01, 0.19 eps: |got - ref| <= 4 eps |ref| (the issue's constant);
  * rhs and the report's per-cell divergence: n terms w v and (1 - w) v_s, each with at most two roundings, added one
    after the other from 0: |got - ref| <= (n + 1) eps sum|terms| over the terms that cell adds (Higham, eq. 3.5 gives
    (n + 2) u; it holds with or without fused multiply-adds);
  * gradient: p_f - p_b is the reference's own float32 operation (Plug.cpp:1102), then theta (two roundings), the division
    by it, the clamp constant and the subtraction from v, which the reference rounds to float32 too:
    |got - ref| <= 3 eps (|v| + |grad|);
  * report: count exact; sum within the sum of the per-cell bounds (the device adds the float32 cell values in double:
    + n_cells eps64 sum|div|); maximum within the largest per-cell bound among the cells that can be the maximum.
The whole call on the device is compared with the reference's TIGHT run: relative max-norm distance of pressure and of
velocity at most `device_factor` (2) times the distance of the reference's own iterate one update short of convergence at
the device's tolerance (`short_*` in the fixture: an iterate the reference rejects; the factor because the stop test is a
residual 2-norm and the comparison an error max-norm).  MEASURED distances of the device are in the fixtures (`device.*`).
"""
import os

import numpy as np
import pytest

import reference_fields_cases as F
from oracle import mg_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LARGEST_EARLIER_FIXTURE = 466879  # golden_solid24.npz

needs_reference = pytest.mark.skipif(
    not (mg_ref.fields_available() and mg_ref.fields_available(long_double=True) and mg_ref.available() and mg_ref.available(long_double=True)),
    reason=f"oracle/_ref/libmgref_fields.so and its long-double twin are not built: run `{mg_ref.BUILD_HINT}` with a checkout of the reference",
)


def key(name):
    return name.replace("/", ".")


@pytest.fixture(scope="module")
def golden():
    cache = {}

    def get(name):
        if name not in cache:
            with np.load(os.path.join(GOLDEN, f"ref_fields_{name}.npz")) as z:
                cache[name] = {k: z[k] for k in z.files}
        return cache[name]

    return get


@pytest.fixture(scope="module")
def scenes():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = F.scene(name)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def fo():
    from oracle.mg_oracle import FieldsOracle

    return FieldsOracle()


@pytest.fixture(scope="module")
def oracle_passes(fo, oracle, scenes):
    """the oracle's per-pass arrays of a scene, computed once and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = F.oracle_passes(fo, oracle, scenes(name))
        return cache[name]

    return get


def assert_hashes(got, g):
    wrong = [k for k, v in got.items() if str(g[key(k)]) != str(v)]
    assert not wrong, f"differs from the reference: {wrong}"


def assert_passes(arrays, g, sc):
    assert_hashes(F.hashes(arrays), g)
    eshape, off, levels = arrays["layout"]
    assert eshape == tuple(g["expanded"]) and off == int(g["offset"]) and levels == int(g["levels"])
    total, mx, count = arrays["report"]
    ref_total, ref_mx, ref_count = (float(v) for v in g["report"])
    assert count == ref_count and mx == ref_mx
    assert abs(total - ref_total) <= F.report_sum_bound(sc, arrays["pass/material"]), (total, ref_total)


def assert_whole_call(got, ref, tol):
    """got: reference_fields_cases.oracle_solve; ref: a reference run (float32 arrays); tol = factor x sensitivity"""
    assert got["iterations"] == ref["iterations"]
    for a in range(3):
        assert np.array_equal(got["valid"][a], ref["valid"][a]), a
    p_ref = ref["pressure"].astype(np.float64)
    assert (np.abs(got["pressure64"] - p_ref) <= F.half_ulp32(p_ref) + tol * np.abs(p_ref).max()).all()
    dp = float(np.abs(got["pressure"].astype(np.float64) - p_ref).max())
    for a in range(3):
        v_ref = ref["velocity"][a].astype(np.float64)
        assert (np.abs(got["velocity64"][a] - v_ref) <= F.half_ulp32(v_ref) + tol * np.abs(v_ref).max() + 2 * dp / 0.01).all(), a


# ---- fixture tests: CPU, always run -----------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", F.SCENES)
def test_inputs_reproduce_their_hashes(name, golden, scenes):
    g, sc = golden(name), scenes(name)
    assert tuple(g["shape"]) == sc["liquid_phi"].shape
    assert_hashes(F.hashes(F.inputs(sc)), g)


def test_edge_scene_has_every_configuration(oracle_passes, scenes, golden):
    """Each configuration the hand-built scene exists for, on labels and valid faces that are the reference's (by hash)."""
    arrays = oracle_passes("edge")
    assert_hashes({k: v for k, v in F.hashes(arrays).items() if k in ("pass/material", "pass/validx", "pass/validy", "pass/validz")}, golden("edge"))
    F.edge_features(scenes("edge"), arrays["pass/material"], [arrays["pass/valid" + n] for n in "xyz"])
    assert {F.SOLID, F.LIQUID, F.AIR} == set(np.unique(arrays["pass/material"])) and (arrays["pass/labels"] == F.BOUNDARY).sum() > 1000


@pytest.mark.parametrize("name", F.SCENES)
def test_oracle_passes_equal_reference(name, golden, oracle_passes, scenes):
    """Material labels, valid faces, domain labels and boundary weights on the base grid and expanded after
    setBoundaryCellLabels, right-hand side, both pressure copies and the gradient: bit for bit.  The report: count and signed
    maximum exact, sum within the summation bound."""
    assert_passes(oracle_passes(name), golden(name), scenes(name))


@pytest.mark.parametrize("run", ["tight", "loose"])
@pytest.mark.parametrize("name", F.SCENES)
def test_oracle_whole_call_within_sensitivity(name, run, golden, fo, oracle, scenes):
    g, sc = golden(name), scenes(name)
    ref = F.unpack_run(g, run + ".", sc)
    tolerance = float(g[run + "_tolerance"] if run == "tight" else g["device_tolerance"])
    got = F.oracle_solve(fo, oracle, sc, tolerance)
    assert_whole_call(got, ref, float(g["oracle_factor"]) * float(g["sensitivity"]))
    assert (ref["pressure"][got["material"] != F.LIQUID] == 0).all()  # makeConstant(0), Plug.cpp:641
    if run == "loose":
        assert F.oracle_solve(fo, oracle, sc, tolerance, use_mg=False)["iterations"] == int(g["diag_iterations"])


def test_fixture_numbers_are_the_measured_ones(golden):
    gs = [golden(n) for n in F.SCENES]
    assert len({float(g["sensitivity"]) for g in gs}) == 1
    assert float(gs[0]["sensitivity"]) == max(float(g["case_sensitivity"]) for g in gs)
    assert 0 < float(gs[0]["oracle_factor"]) * float(gs[0]["sensitivity"]) < 1e-12
    for g in gs:
        assert float(g["oracle_factor"]) == F.ORACLE_FACTOR == 10.0 and float(g["device_factor"]) == F.DEVICE_FACTOR == 2.0
        assert float(g["device_tolerance"]) == F.DEVICE_TOL and float(g["tight_tolerance"]) == F.TIGHT_TOL
        assert int(g["loose.iterations"]) < int(g["tight.iterations"]) < int(g["diag_iterations"]) < F.MAX_ITER
        assert all(0 < float(g[f"short_{t}_{q}"]) < 1e-3 for t in ("mg", "diag") for q in "pv")
    for n in F.SCENES:
        assert os.path.getsize(os.path.join(GOLDEN, f"ref_fields_{n}.npz")) <= LARGEST_EARLIER_FIXTURE


# ---- live tests: CPU, need the compiled reference ------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def reference():
    return mg_ref.ReferenceFields()


@needs_reference
def test_live_plugin_registers_its_parameters(reference):
    assert reference.parameter_count() == 12  # initializeSIM builds the parameter table of getDopDescription


@needs_reference
@pytest.mark.parametrize("name", F.SCENES)
def test_live_reference_reproduces_fixture(name, golden, reference, scenes):
    g, sc = golden(name), scenes(name)
    arrays = F.reference_passes(reference, sc)
    assert_hashes(F.hashes(arrays), g)
    assert arrays["layout"] == (tuple(g["expanded"]), int(g["offset"]), int(g["levels"])) and arrays["report"] == tuple(float(v) for v in g["report"])
    for run, tol in (("tight", F.TIGHT_TOL), ("loose", F.DEVICE_TOL)):
        got, ref = F.reference_solve(reference, sc, tol), F.unpack_run(g, run + ".", sc)
        assert got["iterations"] == ref["iterations"] and np.array_equal(got["pressure"], ref["pressure"])
        for a in range(3):
            assert np.array_equal(got["velocity"][a], ref["velocity"][a]) and np.array_equal(got["valid"][a], ref["valid"][a])
        # the plugin's own report is the report pass on the velocity it leaves
        total, mx, count = reference.divergence(arrays["pass/material"], got["velocity"], sc["cut_weights"], sc["solid_velocity"])
        assert (total, mx) == (got["info"]["divergence_sum"], got["info"]["divergence_max"])
    assert F.reference_solve(reference, sc, F.DEVICE_TOL, use_mg=False)["iterations"] == int(g["diag_iterations"])


@needs_reference
@pytest.mark.parametrize("name", F.SCENES)
def test_live_sensitivity_and_short_distances(name, golden, reference, scenes):
    """Re-derives the measured numbers of the fixture: double against long double, and the iterate one update short."""
    g, sc = golden(name), scenes(name)
    core, core_ld, reference_ld = mg_ref.Reference(), mg_ref.Reference(long_double=True), mg_ref.ReferenceFields(long_double=True)
    sens = 0.0
    for run, tol in (("tight", F.TIGHT_TOL), ("loose", F.DEVICE_TOL)):
        x, it, p = F.reference_solution64(reference, core, sc, tol)
        x_ld, it_ld, _ = F.reference_solution64(reference_ld, core_ld, sc, tol)
        assert it == it_ld == int(g[run + ".iterations"]) and np.array_equal(p, F.unpack_run(g, run + ".", sc)["pressure"])
        sens = max(sens, F.rel_max(x_ld, x))
    assert sens == float(g["case_sensitivity"]) <= float(g["sensitivity"])
    tight = F.unpack_run(g, "tight.", sc)
    for tag, use_mg, its in (("mg", True, int(g["loose.iterations"])), ("diag", False, int(g["diag_iterations"]))):
        short = F.reference_solve(reference, sc, F.DEVICE_TOL, max_iterations=its, use_mg=use_mg)
        assert short["info"]["rel_residual"] >= F.DEVICE_TOL  # the reference rejects it
        assert F.rel_max(short["pressure"], tight["pressure"]) == float(g[f"short_{tag}_p"])
        assert F.rel_max(np.concatenate([v.ravel() for v in short["velocity"]]), np.concatenate([v.ravel() for v in tight["velocity"]])) == float(g[f"short_{tag}_v"])


@needs_reference
@pytest.mark.parametrize("seed", F.RANDOM_SEEDS)
def test_live_random_scenes(seed, golden, reference, fo, oracle):
    """projection_scene((20, 24, 36), randomize=True): fill level, wave, solid box drawn from the seed."""
    sc = F.random_scene(seed)
    ref, got = F.reference_passes(reference, sc), F.oracle_passes(fo, oracle, sc)
    assert (ref["pass/material"] == F.LIQUID).sum() > 1000
    hr, hg = F.hashes(ref), F.hashes(got)
    wrong = [k for k in hr if hr[k] != hg[k]]
    assert not wrong, f"differs from the reference: {wrong}"
    assert got["layout"] == ref["layout"] and got["report"][1:] == ref["report"][1:]
    assert abs(got["report"][0] - ref["report"][0]) <= F.report_sum_bound(sc, ref["pass/material"])
    tol = float(golden("edge")["oracle_factor"]) * float(golden("edge")["sensitivity"])
    for tolerance in (F.TIGHT_TOL, F.DEVICE_TOL):
        assert_whole_call(F.oracle_solve(fo, oracle, sc, tolerance), F.reference_solve(reference, sc, tolerance), tol)


@needs_reference
def test_live_results_do_not_depend_on_the_voxel_size(golden, scenes):
    """The driver builds its fields at origin 0 with a power-of-two voxel size; another one gives the same bits (positions are
    exact, and the interpolated reads of the solid inputs are the samples)."""
    coarse = mg_ref.ReferenceFields(voxel_size=0.125)
    try:
        assert_hashes(F.hashes(F.reference_passes(coarse, scenes("edge"))), golden("edge"))
    finally:
        coarse.lib.mgrf_set_voxel_size(0.03125)


# ---- GPU tests -----------------------------------------------------------------------------------------------------------------


def _dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _expanded(base_grid, eshape, off):
    out = np.zeros(eshape, dtype=base_grid.dtype)
    gz, gy, gx = base_grid.shape
    out[off:off + gz, off:off + gy, off:off + gx] = base_grid
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", F.SCENES)
def test_gpu_passes_against_reference_pinned_oracle(name, golden, oracle_passes, scenes, fo):
    """Every whole-grid device pass against the oracle's arrays, which are first shown to be the reference's.  Labels, valid
    faces, domain labels after the boundary pass and both pressure copies: exact.  Weights, rhs, gradient and report: the
    per-element bounds of the module docstring."""
    import torch

    from geometricmultigridpressuresolver_amd import fields as P

    g, sc, ref = golden(name), scenes(name), oracle_passes(name)
    assert_passes(ref, g, sc)
    eps = F.EPS32
    eshape, off, levels = ref["layout"]
    material, shape = ref["pass/material"], ref["pass/material"].shape
    cw = [_dev(a, torch) for a in sc["cut_weights"]]
    phi, sphi = _dev(sc["liquid_phi"], torch), _dev(sc["solid_phi"], torch)
    vel = [_dev(a, torch) for a in sc["velocity"]]
    sv = [_dev(a, torch) for a in sc["solid_velocity"]] if sc["solid_velocity"] is not None else None
    mat_d = P.buildMaterialCellLabels(phi, sphi, cw)
    assert np.array_equal(mat_d.cpu().numpy(), material)
    valid_d = P.buildValidFaces(mat_d, cw)
    for a, n in enumerate("xyz"):
        assert np.array_equal(valid_d[a].cpu().numpy(), ref["pass/valid" + n]), n
    lab_d, w_d = P.buildMGDomain(mat_d, cw, phi, valid_d, eshape, off)
    assert np.array_equal(lab_d.cpu().numpy().astype(np.int32), ref["pass/labels"])
    for a, n in enumerate("xyz"):
        w_ref = ref["pass/w" + n]
        err = np.abs(w_d[a].cpu().numpy().astype(np.float64) - w_ref)
        print(f"MEASURED {name} w{n}: max |got - ref| / (eps |ref|) = {(err[w_ref > 0] / (eps * w_ref[w_ref > 0])).max():.3f} (bound 4)")
        assert (err <= 4 * eps * np.abs(w_ref)).all(), n
    # rhs: the report's terms with the other sign, so the same magnitudes
    div, mag, cnt = F.cell_divergences(sc, material)
    cell_bound = (cnt + 1) * eps * mag
    rhs_err = np.abs(P.buildRHS(mat_d, vel, cw, eshape, off, sv).cpu().numpy().astype(np.float64) - ref["pass/rhs"])
    rhs_bound = _expanded(cell_bound, eshape, off)
    print(f"MEASURED {name} rhs: max |got - ref| / bound = {(rhs_err[rhs_bound > 0] / rhs_bound[rhs_bound > 0]).max():.3f}")
    assert (rhs_err <= rhs_bound).all() and np.array_equal(-_expanded(div, eshape, off), ref["pass/rhs"])
    # both pressure copies
    x_d = P.applyOldPressure(_dev(F.seeded_pressure(shape), torch), mat_d, eshape, off)
    assert np.array_equal(x_d.cpu().numpy().astype(np.float64), ref["pass/old_pressure"])
    p_back = torch.full(shape, 9.0, dtype=torch.float32, device="cuda")
    P.applySolutionToPressure(p_back, _dev(F.seeded_solution(eshape).astype(np.float32), torch), mat_d, off)
    assert np.array_equal(p_back.cpu().numpy(), ref["pass/pressure"])
    # gradient
    p_seed = F.gradient_pressure(material)
    v64 = fo.pressure_gradient([v.astype(np.float64) for v in sc["velocity"]], sc["cut_weights"], sc["liquid_phi"], p_seed,
                               [ref["pass/valid" + n] for n in "xyz"], material, raw_fields=True)
    vel_d = [v.clone() for v in vel]
    P.applyPressureGradient(vel_d, phi, _dev(p_seed, torch), valid_d, mat_d)
    for a, n in enumerate("xyz"):
        v_in, v_ref = sc["velocity"][a].astype(np.float64), ref["pass/gradient_v" + n].astype(np.float64)
        assert np.array_equal(v64[a].astype(np.float32), ref["pass/gradient_v" + n])
        bound = 3 * eps * (np.abs(v_in) + np.abs(v_in - v64[a]))
        err = np.abs(vel_d[a].cpu().numpy().astype(np.float64) - v_ref)
        on = ref["pass/valid" + n] == 1
        print(f"MEASURED {name} gradient v{n}: max |got - ref| / bound = {(err[on] / bound[on]).max():.3f}")
        assert (err[on] <= bound[on]).all() and (err[~on] == 0).all(), n
    # report
    total, mx, count = P.computeResultingDivergence(mat_d, vel, cw, sv)
    ref_total, ref_mx, ref_count = ref["report"]
    liquid = material == F.LIQUID
    sum_bound = float(cell_bound[liquid].sum()) + int(liquid.sum()) * F.EPS64 * float(np.abs(div[liquid]).sum())
    can_be_max = liquid & (div >= ref_mx - 2 * cell_bound.max())
    print(f"MEASURED {name} report: |sum - ref| / bound = {abs(total - ref_total) / sum_bound:.3f}, |max - ref| / bound = {abs(mx - ref_mx) / cell_bound[can_be_max].max():.3f}")
    assert count == ref_count and abs(total - ref_total) <= sum_bound and abs(mx - ref_mx) <= cell_bound[can_be_max].max()


@pytest.mark.gpu
@pytest.mark.parametrize("precond", ["mg", "diag"])
@pytest.mark.parametrize("name", F.SCENES)
def test_gpu_projection_against_reference_tight_run(name, precond, golden, oracle_passes, scenes):
    """mgps_project_free_surface at the device tolerance, multigrid preconditioner with the Gauss-Seidel smoother (what the
    reference hard-wires) and the diagonal one, against the reference's tight run: valid faces equal, pressure 0 outside the
    liquid, pressure and velocity within `device_factor` x the reference's own one-update-short distance."""
    from geometricmultigridpressuresolver_amd import fields as P

    g, sc, ref = golden(name), scenes(name), oracle_passes(name)
    assert_hashes({k: v for k, v in F.hashes(ref).items() if k == "pass/material"}, g)
    tight = F.unpack_run(g, "tight.", sc)
    h = lambda a: np.array(a, dtype=np.float32, order="C", copy=True)  # noqa: E731
    vel = [h(a) for a in sc["velocity"]]
    p = np.full(sc["liquid_phi"].shape, 3.0, dtype=np.float32)  # stale values everywhere: the call clears them
    valid, info = P.project_free_surface(h(sc["liquid_phi"]), h(sc["solid_phi"]), [h(a) for a in sc["cut_weights"]], vel, p,
                                         [h(a) for a in sc["solid_velocity"]] if sc["solid_velocity"] is not None else None, use_old_pressure=False,
                                         use_mg_preconditioner=precond == "mg", use_gauss_seidel=True, tolerance=F.DEVICE_TOL,
                                         max_iterations=F.MAX_ITER, power_of_two=True)
    assert info["outcome"] == 0 and info["rel_residual"] < F.DEVICE_TOL
    assert (info["expanded"], info["offset"], info["mg_levels"]) == (tuple(g["expanded"]), int(g["offset"]), int(g["levels"]))
    assert info["liquid_cells"] == float(g["report"][2])
    for a in range(3):
        assert np.array_equal(valid[a], tight["valid"][a]), a
    assert (p[ref["pass/material"] != F.LIQUID] == 0).all()
    d_p = F.rel_max(p, tight["pressure"])
    d_v = F.rel_max(np.concatenate([v.ravel() for v in vel]), np.concatenate([v.ravel() for v in tight["velocity"]]))
    factor, short_p, short_v = float(g["device_factor"]), float(g[f"short_{precond}_p"]), float(g[f"short_{precond}_v"])
    print(f"MEASURED {name} {precond}: iterations {info['iterations']}, pressure {d_p:.3e} (bound {factor * short_p:.3e}), velocity {d_v:.3e} (bound {factor * short_v:.3e})")
    assert d_p <= factor * short_p and d_v <= factor * short_v
