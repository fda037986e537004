"""tests/mixed_reference.py against the oracle alone (no GPU): the restatement of the binary16 V-cycle is the reference of
tests/test_mixed_restated.py, so it is validated first, and the criterion those tests use is shown to have the power it claims.

1. With rounding off the composition IS the oracle's cycle: bit equality with OracleSolver.apply_vcycle (the power-of-two scales
   change no bit), both smoothers, 1 and 2 sweeps, a non-default band option set, from zero and from a guess, one level and
   several, and the domain with 2^e = 8.
2. With rounding off the numpy PCG around it is mgo_solve_pcg: iterates 1, 2, 3 to 1e-12.
3. The GPU criterion on every case the GPU tests use.  n = the cells whose stored binary16 value differs between the restatement
   on the fp32 oracle (R32) and on the fp64 one (R64); the GPU may differ from R64 in cap = 4 n + 8 cells.  Moving ONE rounding
   point (the first band stage of every fine stroke rounded or not) and removing all rounding must each change at least 5 cap
   cells, or the case proves nothing.
4. The PCG bound of the GPU tests, 4 x (fp32-oracle iterate against fp64-oracle iterate) + 2e-5, must be below half the distance
   from the restated iterate k to the unrounded oracle's iterate k: only such k are in PCG_KS.  Iterate 2 is not among them; it is
   kept for the <z, r> taken inside the loop, which it is the first to read: an error of 1e-3 there must move it by twice the bound.
"""
import numpy as np
import pytest

import mixed_reference as MR
from conftest import rel_l2

W23 = 2.0 / 3.0
DOMAIN_ARGS = {"wide512": (3, (64, 64, 512)), "widesolid": (3, (32, 40, 264))}  # (levels, solver grid), as tests/test_gpu_parity.py
X_TOL = 2e-5  # tests/test_pcg_exits.py: the fp32 CG recurrence against the oracle's iterate


def _w32(omega):
    return float(np.float32(omega))


def case(kind, g, use_gs=False, sweeps=1, band=(3, 3, W23), levels=None, rhs="random"):
    return dict(kind=kind, g=g, use_gs=use_gs, sweeps=sweeps, band=band, levels=levels, rhs=rhs)


# the cases of tests/test_mixed_restated.py (one binary16 cycle from zero)
CYCLE_CASES = {
    "one-level-simple32": case("simple", 32, levels=1),                  # band boxes and the zero-start Jacobi instance, no transfers
    "solid64": case("solid", 64),                                        # 128^3, cut cells
    "complex64": case("complex", 64),                                    # 128^3, ghost-fluid weights
    "widesolid": case("widesolid", 24),                                  # 264 x 40 x 32: ragged in x and y, nx % 4 == 0
    "wide512": case("wide512", 40),                                      # two waves per row; N = 512: e = 3 (widesolid: e = 2; else 0)
    "random3": case("random", 3),                                        # general rows in every band box, rows ending anywhere
    "random4": case("random", 4),
    "solid64-2+2": case("solid", 64, sweeps=2),                          # stage-by-stage Jacobi
    "solid64-gs": case("solid", 64, use_gs=True),
    "random3-gs": case("random", 3, use_gs=True),
    "solid64-w2d2o0.8": case("solid", 64, band=(2, 2, 0.8)),
    "solid64-w4d4o0.5": case("solid", 64, band=(4, 4, 0.5)),
    # max |b| = 2^-9 and one fp32 ulp above: launchMixSigma's two ends run.  These two do NOT see which power of two sigma is -- a
    # factor of two on every stored value cancels when the iterate is recovered, away from subnormals and saturation
    "simple32-max-pow2": case("simple", 32, rhs="pow2"),
    "simple32-max-pow2-ulp": case("simple", 32, rhs="pow2+ulp"),
    "complex32-delta": case("complex", 32, rhs="delta"),                 # binary16 subnormals in the stored iterate
    # the same with max |b| = 1 exactly: sigma = 1 or 1/2 decides which bits the subnormals keep, so this case sees the closed end
    # of (1/2, 1] (test_the_pow2_delta_case_sees_sigma)
    "complex32-delta-max-pow2": case("complex", 32, rhs="delta-pow2"),
}
GUESS_CASE = case("random", 3, use_gs=True)  # two chained cycles, the second from the first one's result
PCG_DOMAIN = ("solid", 48)
# the k whose bound separates (part 4).  k = 2 does not -- Jacobi: bound 3.9e-5 against half of 7.0e-5, Gauss-Seidel: 7.2e-5 against
# half of 6.7e-5 -- and k = 3 less still (4.3e-5 / 7.2e-5 against half of 2.7e-5 / 2.1e-5): CG corrects the preconditioner away
PCG_KS = (1,)
# iterate 2 is held to the same bound for another reason: it is the first that reads a <z, r> taken inside the loop (the gathered
# dot with Jacobi, halfDotKernel with Gauss-Seidel) and p = z + beta p (xpayHalfKernel); an error of DOT_ERROR in that dot moves it
# by more than twice the bound (test_iterate_2_sees_a_wrong_dot)
PCG_DOT_K, DOT_ERROR = 2, 1e-3
SUBNORMALS_WANTED = 100


def domain(c, domain_factory):
    lev, shape = DOMAIN_ARGS.get(c["kind"], (c["levels"], None))
    lab, w, off, lev, dx = domain_factory(c["kind"], c["g"], lev, shape)
    return lab, w, off, lev, dx


def rhs_of(c, lab, off, dx):
    """fp32 rhs of a case.  random: U(0, 1) h^2 x 37 (any magnitude: the cycle normalises by a power of two)"""
    from geometricmultigridpressuresolver_amd import domains as D

    kind = c["rhs"]
    if kind == "random":
        return D.random_rhs(lab, dx, seed=5).astype(np.float32) * np.float32(37.0)
    if kind in ("pow2", "pow2+ulp"):
        b = D.random_rhs(lab, 1.0, seed=5).astype(np.float32) * np.float32(2.0 ** -10)  # below 2^-10 everywhere
        top = np.float32(2.0 ** -9)
        if kind == "pow2+ulp":
            top = np.nextafter(top, np.float32(1.0))
        cell = np.argwhere(D.active_mask(lab))[len(np.argwhere(D.active_mask(lab))) // 2]
        b[tuple(cell)] = top
        assert np.abs(b).max() == top
        return b
    if kind == "delta-pow2":  # the block at 1024 h^2 = 1 plus positive noise, cut back to 1
        b = np.minimum(D.delta_rhs(lab, c["g"], off, dx, amplitude=1.0 / (dx * dx)) + 1e-3 * D.random_rhs(lab, dx, seed=5), 1.0).astype(np.float32)
        assert np.abs(b).max() == 1.0 and np.count_nonzero(b == 1.0) >= 1
        return b
    assert kind == "delta"
    return (D.delta_rhs(lab, c["g"], off, dx) + 1e-3 * D.random_rhs(lab, dx, seed=5)).astype(np.float32)


def options_of(c):
    """keyword arguments of MixedCycle / Oracle.solver for a case (the weight as the fp32 number the device damps by)"""
    return dict(use_gs=c["use_gs"], pre_sweeps=c["sweeps"], post_sweeps=c["sweeps"], band_width=c["band"][0], band_iterations=c["band"][1],
                jacobi_weight=_w32(c["band"][2]))


def restatement(orc, c, lab, w, lev, **flags):
    real = orc.real
    return MR.MixedCycle(orc, lab.astype(np.int32), [a.astype(real) for a in w], lev, **options_of(c), **flags)


_STORED = {}


def stored_references(name, domain_factory, oracle, oracle32):
    """{"R64", "R32": the stored iterate of one cycle from zero (np.float16, read-only), "back": the factor to the caller's units,
    "act", "b"}: computed once per case and shared"""
    if name not in _STORED:
        c = CYCLE_CASES[name]
        lab, w, off, lev, dx = domain(c, domain_factory)
        b = rhs_of(c, lab, off, dx)
        out = {"b": b, "lab": lab, "w": w, "lev": lev}
        for key, orc in (("R64", oracle), ("R32", oracle32)):
            m = restatement(orc, c, lab, w, lev)
            out[key], out["back"] = m.stored(b)
            out[key].setflags(write=False)
            out["act"], out["e"] = m.act, m.e
            m.close()
        _STORED[name] = out
    return _STORED[name]


# ---- 1. the composition is the oracle's cycle ---------------------------------------------------------------------------------
UNROUNDED = [
    ("simple", 32, 1, False, 1, (3, 3, W23)), ("simple", 32, 1, True, 1, (3, 3, W23)),
    ("complex", 32, None, False, 1, (3, 3, W23)), ("complex", 32, None, False, 2, (3, 3, W23)),
    ("complex", 32, None, True, 1, (3, 3, W23)), ("random", 3, None, True, 2, (3, 3, W23)), ("random", 4, None, False, 1, (3, 3, W23)),
    ("solid", 32, None, False, 1, (2, 2, 0.8)), ("solid", 32, None, True, 1, (4, 4, 0.5)),
    ("wide512", 40, None, False, 1, (3, 3, W23)),
]


@pytest.mark.parametrize("guess", [False, True])
@pytest.mark.parametrize("kind,g,levels,use_gs,sweeps,band", UNROUNDED)
def test_unrounded_composition_is_the_oracles_cycle(kind, g, levels, use_gs, sweeps, band, guess, domain_factory, oracle):
    from geometricmultigridpressuresolver_amd import domains as D

    c = case(kind, g, use_gs, sweeps, band, levels)
    lab, w, off, lev, dx = domain(c, domain_factory)
    b = rhs_of(c, lab, off, dx).astype(np.float64)
    x0 = None
    if guess:
        rng = np.random.Generator(np.random.PCG64(21))
        x0 = np.where(D.active_mask(lab), rng.random(lab.shape) * 1e-3, 0.0)
    m = restatement(oracle, c, lab, w, lev, rounding=False)
    orc = oracle.solver(lab.astype(np.int32), [a.astype(np.float64) for a in w], lev, **options_of(c))
    assert m.levels == orc.levels == (1 if levels == 1 else m.levels)
    x_ref = np.zeros(lab.shape) if x0 is None else x0.copy()
    orc.apply_vcycle(x_ref, b, guess)
    x = m.apply(b, x0)
    assert np.abs(x_ref).max() > 0
    assert np.array_equal(x, x_ref), (int(np.count_nonzero(x != x_ref)), rel_l2(x, x_ref))
    if guess:  # the form the device takes from a guess, x0 + M (b - A x0): the same cycle up to fp64 round-off
        assert rel_l2(m.apply(b, x0, correction_form=True), x_ref) < 1e-12
    m.close()
    orc.close()


def test_scales():
    """sigma brings max |b| into (1/2, 1], both ends; e = 0 up to N = 181, 3 at 512, 5 at 1024"""
    for m, want in ((1.0, 1.0), (0.5, 2.0), (np.nextafter(np.float32(0.5), np.float32(1)), 1.0), (0.75, 1.0), (37.0, 1 / 64), (2.0 ** -9, 2.0 ** 9),
                    (np.nextafter(np.float32(2.0 ** -9), np.float32(1)), 2.0 ** 8), (0.0, 1.0)):
        s = MR.mix_sigma(m)
        assert s == want and (m == 0 or 0.5 < s * float(m) <= 1.0), (m, s)
    assert [MR.mix_exp((n, 8, 8)) for n in (32, 128, 181, 182, 256, 264, 512, 1024)] == [0, 0, 0, 1, 1, 2, 3, 5]
    h = MR.to_half(np.array([1e6, -1e6, 2.0 ** -24, 2.0 ** -25 * 1.01, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11]))
    assert h.tolist() == [65504.0, -65504.0, 2.0 ** -24, 2.0 ** -24, 1.0, 1.0 + 2.0 ** -9]  # saturation, subnormals kept, ties to even


# ---- 2. the numpy PCG is mgo_solve_pcg ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_gs", [False, True])
def test_unrounded_pcg_is_the_oracles(use_gs, domain_factory, oracle):
    from geometricmultigridpressuresolver_amd import domains as D

    c = case("complex", 32, use_gs)
    lab, w, off, lev, dx = domain(c, domain_factory)
    b = (D.delta_rhs(lab, 32, off, dx) + D.random_rhs(lab, dx)).astype(np.float32).astype(np.float64)
    m = restatement(oracle, c, lab, w, lev, rounding=False)
    orc = oracle.solver(lab.astype(np.int32), [a.astype(np.float64) for a in w], lev, **options_of(c))
    for k in (1, 2, 3):
        x_ref = np.zeros(lab.shape)
        st = orc.solve_pcg(x_ref, b, 1e-12, k, True)
        assert st["iterations"] == k
        err = rel_l2(MR.pcg(oracle, lab, m.w, b, m.apply, k), x_ref)
        print(f"gs={int(use_gs)} k={k}: numpy PCG against mgo_solve_pcg {err:.1e}")
        assert err < 1e-12
    m.close()
    orc.close()


# ---- 3. the power of the GPU criterion ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CYCLE_CASES))
def test_criterion_separates_a_moved_rounding_point(name, domain_factory, oracle, oracle32):
    ref = stored_references(name, domain_factory, oracle, oracle32)
    c, act = CYCLE_CASES[name], ref["act"]
    n, ulp, l2 = MR.compare_stored(ref["R32"], ref["R64"], act)
    cap = 4 * n + 8
    three_launch = c["sweeps"] == 1 and not c["use_gs"]
    moved = restatement(oracle, c, ref["lab"], ref["w"], ref["lev"], round_first_band=three_launch)  # the other choice than the device's
    n_moved, _, l2_moved = MR.compare_stored(moved.stored(ref["b"])[0], ref["R64"], act)
    moved.close()
    plain = restatement(oracle, c, ref["lab"], ref["w"], ref["lev"], rounding=False)
    n_plain, _, l2_plain = MR.compare_stored(MR.to_half(plain.stored(ref["b"])[0]), ref["R64"], act)
    plain.close()
    print(f"{name}: {int(act.sum())} active cells, e = {ref['e']}; R32 against R64: {n} cells, {ulp} ulp, {l2:.1e}; first band stage "
          f"{'rounded' if three_launch else 'unrounded'}: {n_moved} cells, {l2_moved:.1e}; no rounding: {n_plain} cells, {l2_plain:.1e}; cap {cap}")
    assert n_moved >= 5 * cap and n_plain >= 5 * cap, (n, cap, n_moved, n_plain)


@pytest.mark.parametrize("name", ["complex32-delta", "complex32-delta-max-pow2"])
def test_the_delta_cases_store_subnormals(name, domain_factory, oracle, oracle32):
    ref = stored_references(name, domain_factory, oracle, oracle32)
    v = np.abs(ref["R64"].astype(np.float64))[ref["act"]]
    sub = int(np.count_nonzero((v > 0) & (v < 2.0 ** -14)))
    print(f"{name}: {sub} of {v.size} active cells of the stored iterate are binary16 subnormals")
    assert sub >= SUBNORMALS_WANTED


def test_the_pow2_delta_case_sees_sigma(domain_factory, oracle, oracle32):
    """max |b| = 1 exactly: with sigma = 1/2 (the half-open interval the other way round, [1/2, 1)) every stored value is half as
    large, and the subnormals lose their last bit.  Recovered as the GPU test recovers the iterate -- with the reference's sigma --
    that must change at least 5 x the cap of cells; on simple32-max-pow2, whose stored values lie between 0.07 and 8, it changes
    none (asserted too: that case runs the end of the interval and cannot tell which sigma came out)."""
    for name, seen in (("complex32-delta-max-pow2", True), ("simple32-max-pow2", False)):
        ref = stored_references(name, domain_factory, oracle, oracle32)
        c, act = CYCLE_CASES[name], ref["act"]
        assert MR.mix_sigma(np.abs(ref["b"]).max()) == 2 * MR.mix_sigma(np.abs(ref["b"]).max(), pow2_to_half=True)
        cap = 4 * MR.compare_stored(ref["R32"], ref["R64"], act)[0] + 8
        other = restatement(oracle, c, ref["lab"], ref["w"], ref["lev"], pow2_to_half=True)
        st, back = other.stored(ref["b"])
        other.close()
        assert back == 2 * ref["back"]
        it = st.astype(np.float64) * (back / ref["back"])  # x sigma 2^-e with the reference's sigma
        n, ulp, l2 = MR.compare_stored(it.astype(np.float16), ref["R64"], act)
        off_grid = int(np.count_nonzero(it.astype(np.float16).astype(np.float64) != it))
        print(f"{name}: sigma halved: {n} cells differ, {ulp} ulp, {l2:.1e}, {off_grid} off the binary16 grid; cap {cap}")
        assert (n >= 5 * cap) if seen else (n == 0 and off_grid == 0)


# ---- 4. the PCG bound ---------------------------------------------------------------------------------------------------------
_PCG = {}


def pcg_references(use_gs, domain_factory, oracle, oracle32):
    """{k: (iterate k of the numpy PCG around R64, the GPU's bound against it, the distance to the unrounded oracle's iterate)}"""
    from geometricmultigridpressuresolver_amd import domains as D

    if use_gs not in _PCG:
        c = case(*PCG_DOMAIN, use_gs)
        lab, w, off, lev, dx = domain(c, domain_factory)
        b = (D.delta_rhs(lab, c["g"], off, dx) + D.random_rhs(lab, dx)).astype(np.float32)  # as tests/test_pcg_exits.py
        m64, m32 = restatement(oracle, c, lab, w, lev), restatement(oracle32, c, lab, w, lev)
        orc = oracle.solver(lab.astype(np.int32), [a.astype(np.float64) for a in w], lev, **options_of(c))
        out = {"b": b, "lab": lab, "w": w, "lev": lev}
        for k in (1, 2, 3):
            x64 = MR.pcg(oracle, lab, m64.w, b, m64.apply, k)
            x32 = MR.pcg(oracle32, lab, m32.w, b, m32.apply, k)
            x_plain = np.zeros(lab.shape)
            orc.solve_pcg(x_plain, b.astype(np.float64), 1e-12, k, True)
            x64.setflags(write=False)
            out[k] = (x64, 4 * rel_l2(x32, x64) + X_TOL, rel_l2(x64, x_plain), rel_l2(x32, x64))
        out["dot_move"] = rel_l2(MR.pcg(oracle, lab, m64.w, b, m64.apply, PCG_DOT_K, dot_error=DOT_ERROR), out[PCG_DOT_K][0])
        for s in (m64, m32, orc):
            s.close()
        _PCG[use_gs] = out
    return _PCG[use_gs]


@pytest.mark.parametrize("use_gs", [False, True])
def test_pcg_bound_is_below_half_the_rounding_effect(use_gs, domain_factory, oracle, oracle32):
    ref = pcg_references(use_gs, domain_factory, oracle, oracle32)
    for k in (1, 2, 3):
        x, bound, effect, d32 = ref[k]
        print(f"solid48 gs={int(use_gs)} k={k}: fp32-oracle iterate against fp64-oracle iterate {d32:.1e}; bound {bound:.1e}; "
              f"restated iterate against the unrounded oracle's {effect:.1e}")
    for k in PCG_KS:
        assert ref[k][1] < 0.5 * ref[k][2], (k, ref[k][1:])


@pytest.mark.parametrize("use_gs", [False, True])
def test_iterate_2_sees_a_wrong_dot(use_gs, domain_factory, oracle, oracle32):
    """iterate 1 reads <p, r> and <p, A p> only; the <z, r> of the loop (gathered by the cycle's last stroke, or halfDotKernel) first
    enters iterate 2 through beta: a relative error of 1e-3 in it must move that iterate by more than twice the GPU test's bound"""
    ref = pcg_references(use_gs, domain_factory, oracle, oracle32)
    print(f"solid48 gs={int(use_gs)}: <z, r> wrong by {DOT_ERROR:g} moves iterate {PCG_DOT_K} by {ref['dot_move']:.1e}; bound {ref[PCG_DOT_K][1]:.1e}")
    assert ref["dot_move"] > 2 * ref[PCG_DOT_K][1]
