"""Every way out of mgps_solve_pcg against the fp64 oracle's iterate k -- the exits the converged-end parity tests do not see.

1. max_iterations = k: the oracle's solve_pcg(x, b, tol, k, use_mg) leaves its iterate k in x, the GPU call must leave the same
   one, for pcg_fp64_vectors 0 / 1 / 2 x smoother x preconditioner, at k chosen for mode 2's flush schedule.
2. MGPS_ERR_INTERRUPTED at every poll of the first iterations: what comes back is the iterate a truncated solve returns, and the
   stats say which.
3. The same exits through the host-buffer forms, the one-call projection and (tests/test_distributed.py) a slab run.

Bounds (none of them taken from what the GPU gives):
  * x against the oracle's iterate k: 2e-5 relative L2, the bound test_pcg_fp64_vectors puts on the MG-PCG iterate.  The fp32
    build of the oracle against the fp64 one, same inputs and k, sits between 4e-8 and 6.1e-7 on the cases of part 1 from the zero
    guess and reaches 1.1e-6 from the random guess: what fp32 arithmetic alone costs leaves a factor of 18 of room.
  * residuals: 1e-3 relative (the bound test_pcg_fp64_vectors uses between recurrence and recomputed residual), at every k where
    the oracle's residual is at least 30 x what rounding its own iterate k to fp32 adds to that residual, |A (x_k - fp32(x_k))| /
    |b| (the returned x is fp32: that floor is what its true residual cannot beat; 30 x above it the rounding adds at most
    1/1800 in quadrature).  Modes 1 and 2 only: their stats come from the fp64 iterate.  In mode 0 both
    numbers are fp32 evaluations whose own error is of the order of that floor -- 1/30 of the residual at the edge of the range,
    thirty times the bound -- so mode 0 is held to the comparison of x, and its figures are printed.
  * interrupted against truncated: both narrow the same fp64 sum once (modes 1, 2) or are the same fp32 grid (mode 0): bit
    equality in mode 0, at most one fp32 ulp per cell in modes 1 and 2.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 5, 8, 9, 12)
X_TOL = 2e-5      # relative L2 of iterate k (test_pcg_fp64_vectors)
RES_TOL = 1e-3    # relative agreement of the residual figures (test_pcg_fp64_vectors)
FLOOR_FACTOR = 30.0
UNREACHABLE = 1e-12  # a tolerance no mode reaches in 12 iterations: every solve of part 1 ends on its iteration cap
INTERRUPTED = 9      # MGPS_ERR_INTERRUPTED


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


# ---- inputs and the reference ------------------------------------------------------------------------------------------------
def _inputs(kind, g, domain_factory, guess):
    """labels, weights, levels, b (fp32; delta + random as in test_pcg_fp64_vectors, random alone on the random-label domain,
    where the delta's place means nothing) and the initial guess (fp32; zero, or random on active cells)"""
    from geometricmultigridpressuresolver_amd import domains as D

    lab, w, off, lev, dx = domain_factory(kind, g)
    if kind == "random":
        b = D.random_rhs(lab, dx)
    else:
        b = (D.delta_rhs(lab, g, off, dx) + D.random_rhs(lab, dx)).astype(np.float32)
    x0 = np.zeros(lab.shape, dtype=np.float32)
    if guess:
        rng = np.random.Generator(np.random.PCG64(21))
        x0 = np.where(D.active_mask(lab), rng.random(lab.shape) * GUESS_SCALE, 0.0).astype(np.float32)
    return lab, w, lev, b, x0


GUESS_SCALE = 1.0  # (max |x| of the solutions is 1 .. 2.3 on the box domains)


def true_residual(oracle, lab32, w64, x, b64):
    """|b - A x| / |b| evaluated by the oracle in fp64"""
    r = np.zeros(lab32.shape)
    oracle.residual(r, np.ascontiguousarray(x, dtype=np.float64), b64, lab32, w64)
    return float(np.linalg.norm(r.ravel()) / np.linalg.norm(b64.ravel()))


def rounding_floor(oracle, lab32, w64, x, b64):
    """what rounding the fp64 iterate x to fp32 adds to its residual: |A (x - fp32(x))| / |b|, evaluated by the oracle in fp64
    (the residual of the rounded iterate is the root of the sum of the squares, up to the angle between the two)"""
    y = np.zeros(lab32.shape)
    oracle.apply_poisson(y, x - x.astype(np.float32).astype(np.float64), lab32, w64)
    return float(np.linalg.norm(y.ravel()) / np.linalg.norm(b64.ravel()))


_REFERENCE = {}


def reference(oracle, key, lab, w, lev, use_gs, use_mg, b, x0, ks=KS):
    """{k: the oracle's iterate k, its residual figures, the fp32 floor of that iterate and whether k is in the compared range}"""
    if key in _REFERENCE:
        return _REFERENCE[key]
    lab32, w64, b64 = lab.astype(np.int32), [a.astype(np.float64) for a in w], b.astype(np.float64)
    orc = oracle.solver(lab32, w64, lev, use_gs)
    out = {"lab32": lab32, "w64": w64, "b64": b64}
    for k in ks:
        x = x0.astype(np.float64)
        st = orc.solve_pcg(x, b64, UNREACHABLE, k, use_mg)
        assert st["status"] == 0 and st["iterations"] == k, st
        floor = rounding_floor(oracle, lab32, w64, x, b64)
        out[k] = {"x": x, "rel_residual": st["rel_residual"], "rel_residual_recomputed": st["rel_residual_recomputed"], "floor": floor,
                  "compared": st["rel_residual"] >= FLOOR_FACTOR * floor}
    orc.close()
    _REFERENCE[key] = out
    return out


def _options(mode, **more):
    import geometricmultigridpressuresolver_amd as G

    o = G.default_options()
    o.pcg_fp64_vectors = mode
    for k, v in more.items():
        setattr(o, k, v)
    return o


def _close(a, b, tol=RES_TOL):
    return abs(a - b) <= tol * abs(b)


# ---- 1. the iteration cap ----------------------------------------------------------------------------------------------------
def _truncated_against_oracle(kind, g, use_gs, use_mg, mode, guess, domain_factory, oracle, compare_iterate=True, **opts):
    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import domains as D

    lab, w, lev, b, x0 = _inputs(kind, g, domain_factory, guess)
    ref = reference(oracle, (kind, g, use_gs, use_mg, guess), lab, w, lev, use_gs, use_mg, b, x0)
    assert sum(ref[k]["compared"] for k in KS) >= 4, [(k, ref[k]["rel_residual"], ref[k]["floor"]) for k in KS]
    inactive = ~D.active_mask(lab)
    s = G.GeometricMultigridPoissonSolver(lab, w, lev, use_gs, options=_options(mode, **opts))
    worst = {"x": 0.0, "rel_residual": 0.0, "recomputed": 0.0}
    failures = []
    try:
        bd = s.to_device(b)
        for k in KS:
            x = s.to_device(x0)
            st = s.solveGeometricConjugateGradient(x, bd, UNREACHABLE, k, use_mg)
            xh = x.cpu().numpy()
            r = ref[k]
            true = true_residual(oracle, ref["lab32"], ref["w64"], xh, ref["b64"])
            ex = rel_l2(xh, r["x"])
            d_rec, d_res = abs(st["rel_residual_recomputed"] - true) / true, abs(st["rel_residual"] - r["rel_residual"]) / r["rel_residual"]
            print(f"{kind}{g} gs={int(use_gs)} mg={int(use_mg)} mode={mode} guess={int(guess)} {opts} k={k}: x {ex:.2e}; rel_residual {st['rel_residual']:.6e} "
                  f"(oracle {r['rel_residual']:.6e}, {d_res:.1e}); recomputed {st['rel_residual_recomputed']:.6e} (fp64 of the returned x {true:.6e}, "
                  f"{d_rec:.1e}); floor {r['floor']:.1e} compared={r['compared']}")
            if st["outcome"] != "max_iterations" or st["iterations"] != k:
                failures.append((k, "exit", st))
            if np.any(xh[inactive] != 0):
                failures.append((k, "non-zero outside active cells"))
            if compare_iterate:
                worst["x"] = max(worst["x"], ex)
                if not ex < X_TOL:
                    failures.append((k, "x", ex))
            if r["compared"] and mode != 0:
                worst["recomputed"] = max(worst["recomputed"], d_rec)
                if not (_close(st["rel_residual_recomputed"], true) and (not compare_iterate or _close(st["rel_residual_recomputed"], r["rel_residual_recomputed"]))):
                    failures.append((k, "rel_residual_recomputed", st["rel_residual_recomputed"], true, r["rel_residual_recomputed"]))
                if compare_iterate:
                    worst["rel_residual"] = max(worst["rel_residual"], d_res)
                    if not (_close(st["rel_residual"], r["rel_residual"]) and _close(st["rel_residual"], true)):
                        failures.append((k, "rel_residual", st["rel_residual"], r["rel_residual"], true))
    finally:
        s.close()
    print(f"WORST {kind}{g} gs={int(use_gs)} mg={int(use_mg)} mode={mode} guess={int(guess)} {opts}: {worst}")
    assert not failures, failures


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("use_mg", [True, False])
@pytest.mark.parametrize("use_gs", [False, True])
@pytest.mark.parametrize("kind,g", [("solid", 48), ("complex", 32), ("random", 4)])
def test_iteration_cap_leaves_the_oracles_iterate(kind, g, use_gs, use_mg, mode, domain_factory, oracle, torch_cuda):
    """max_iterations = k in {1, 2, 3, 5, 8, 9, 12}: outcome, iterations, x (2e-5), both residual figures (1e-3 where the oracle's
    residual is 30 x above the fp32 floor of its iterate; modes 1 and 2) and zeros outside active cells.  With the diagonal
    preconditioner mode 2 runs a group of updates to its cap of 8: k = 3 and 5 leave with updates pending, 8 right after a flush,
    9 one update into the next group; with MG the hundredfold-drop rule ends a group every three or four iterations.

    Largest values on MI355X: see MEASURED at the end of this file."""
    _truncated_against_oracle(kind, g, use_gs, use_mg, mode, False, domain_factory, oracle)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("use_mg", [True, False])
@pytest.mark.parametrize("use_gs", [False, True])
def test_iteration_cap_from_an_initial_guess(use_gs, use_mg, mode, domain_factory, oracle, torch_cuda):
    """the same from a non-zero guess, random on active cells: both sides start from r = b - A x of the x they are given"""
    _truncated_against_oracle("complex", 32, use_gs, use_mg, mode, True, domain_factory, oracle)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("use_gs", [False, True])
def test_iteration_cap_with_the_binary16_cycle(use_gs, mode, domain_factory, oracle, torch_cuda):
    """options.precision = 1: the binary16 V-cycle is another preconditioner (2e-3 from the oracle's per cycle,
    tests/test_mixed_precision.py), so iterate k has no derived bound against the UNROUNDED oracle's.  Against the cycle restated
    with the device's rounding points it has one: tests/test_mixed_restated.py::test_capped_pcg_leaves_the_restated_iterate holds
    iterate 1 to it (tests/mixed_reference.py).  Here the exit itself is checked:
    outcome, iterations, zeros outside active cells, and that the x handed back is the iterate the stats describe (its
    fp64-evaluated residual against rel_residual_recomputed)."""
    _truncated_against_oracle("solid", 48, use_gs, True, mode, False, domain_factory, oracle, compare_iterate=False, precision=1)


# ---- 2. interrupts -----------------------------------------------------------------------------------------------------------
CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p)


class Poller:
    """options.interrupt: counts the polls and answers 1 at poll `stop_at` (None: never)"""

    def __init__(self):
        self.polls, self.stop_at = 0, None
        self.cb = CALLBACK(self._poll)

    def _poll(self, user):
        n = self.polls
        self.polls += 1
        return int(self.stop_at is not None and n >= self.stop_at)

    def arm(self, stop_at):
        self.polls, self.stop_at = 0, stop_at

    def install(self, opt):
        opt.interrupt = C.cast(self.cb, C.c_void_p)
        return opt


def ulps(a, b):
    """largest distance of two fp32 arrays in units in the last place"""
    def ordered(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    return int(np.abs(ordered(a) - ordered(b)).max())


def poll_site(n, levels):
    """Where poll n of a single-device MG-PCG solve sits: (loop counter, updates applied, inside a V-cycle?).  A V-cycle of L
    levels polls L - 2 times going down (not on level 0, not at the bottom) and L - 1 times coming up; the first cycle of a solve
    runs before the loop; every iteration polls once at its top and then runs its cycle."""
    cycle = 2 * levels - 3
    if n < cycle:
        return 0, 0, True
    it, pos = divmod(n - cycle, cycle + 1)
    return it, it + (pos > 0), pos > 0


class InterruptedSolves:
    """one solver with a Poller: truncated solves (cached by the number of updates) and solves interrupted at poll n"""

    def __init__(self, lab, w, lev, use_gs, b, x0, opt):
        import geometricmultigridpressuresolver_amd as G

        self.poller = Poller()
        self.s = G.GeometricMultigridPoissonSolver(lab, w, lev, use_gs, options=self.poller.install(opt))
        self.bd, self.x0 = self.s.to_device(b), x0
        self.levels = self.s.getMGLevels()
        self.cache = {}

    def truncated(self, u):
        if u not in self.cache:
            self.poller.arm(None)
            x = self.s.to_device(self.x0)
            st = self.s.solveGeometricConjugateGradient(x, self.bd, UNREACHABLE, u, True)
            assert st["outcome"] == "max_iterations" and st["iterations"] == u, st
            self.cache[u] = (x.cpu().numpy(), st, self.poller.polls)
        return self.cache[u]

    def interrupted(self, n):
        import geometricmultigridpressuresolver_amd as G

        self.poller.arm(n)
        x = self.s.to_device(self.x0)
        with pytest.raises(G.MgpsError) as err:
            self.s.solveGeometricConjugateGradient(x, self.bd, UNREACHABLE, 200, True)
        return x.cpu().numpy(), err.value, self.poller.polls


ITERATIONS_COVERED = 9  # every poll of iterations 0 .. 8


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("use_gs", [False, True])
def test_interrupt_at_every_poll_hands_back_an_iterate(use_gs, mode, domain_factory, torch_cuda):
    """The poll schedule first: a solve capped at K iterations polls (2 L - 3) (K + 1) + K times -- a V-cycle before the loop and
    one per iteration, 2 L - 3 polls each, plus one poll at the top of every iteration.  Then the solve is interrupted at EVERY
    poll n of the first V-cycle and of iterations 0 .. 8 (rather than at a hand-picked few: the set holds the very first poll,
    polls inside the first preconditioner application, every loop-top poll and every in-cycle poll of nine iterations.  The
    oracle's residual falls 3 to 5 times per iteration on this domain, so mode 2's hundredfold-drop rule ends a group of updates
    every three or four iterations: the nine iterations hold at least two flushes, loop-top and in-cycle polls in the middle of a
    group, and the iteration right after a flush, wherever exactly the flushes fall).  Each time: MGPS_ERR_INTERRUPTED, exactly
    n + 1 polls (nothing polled, hence no cycle run, after the stop), outcome max_iterations, iterations = the loop counter at
    the stop, and x = the x of the same solver's solve capped at u iterations, u = the updates applied before poll n (the
    counter at a loop-top poll, the counter + 1 inside that iteration's V-cycle, 0 before the loop, where x is the caller's
    guess bit for bit); rel_residual is that solve's too.  Bit equality is required in mode 0, at most one fp32 ulp per cell in
    modes 1 and 2 (on MI355X: see MEASURED)."""
    lab, w, lev, b, x0 = _inputs("solid", 64, domain_factory, True)
    run = InterruptedSolves(lab, w, lev, use_gs, b, x0, _options(mode))
    try:
        L = run.levels
        assert L >= 3
        cycle = 2 * L - 3
        for K in (0, 1, 4):
            assert run.truncated(K)[2] == cycle * (K + 1) + K, (K, run.truncated(K)[2], L)
        worst, failures = 0, []
        for n in range(cycle + ITERATIONS_COVERED * (cycle + 1)):
            it, u, in_cycle = poll_site(n, L)
            xh, err, polls = run.interrupted(n)
            xt, stt, _ = run.truncated(u)
            st = err.stats
            if err.status != INTERRUPTED or polls != n + 1:
                failures.append((n, "status / polls", err.status, polls))
            if st["outcome"] != "max_iterations" or st["iterations"] != it:
                failures.append((n, "stats", it, u, in_cycle, st))
            elif not _close(st["rel_residual"], stt["rel_residual"], 1e-9):
                failures.append((n, "rel_residual", st["rel_residual"], stt["rel_residual"]))
            if u == 0 and not np.array_equal(xh, x0):
                failures.append((n, "the guess was not handed back", ulps(xh, x0)))
            d = ulps(xh, xt)
            worst = max(worst, d)
            if d > (0 if mode == 0 else 1):
                failures.append((n, "x", it, u, in_cycle, d, rel_l2(xh, xt)))
        print(f"WORST interrupt solid64 gs={int(use_gs)} mode={mode} levels={L}: {worst} ulp between interrupted and truncated")
        wrong_x = {where: [f[0] for f in failures if f[1] == "x" and f[4] == in_cycle] for where, in_cycle in (("loop-top", False), ("in-cycle", True))}
        assert not failures, (f"polls with a wrong x: {wrong_x}", failures[:8])
    finally:
        run.s.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_the_binary16_cycle_polls_at_the_loop_top_only(mode, domain_factory, torch_cuda):
    """options.precision = 1: vcycleMixed runs its coarse levels unpolled, so a solve capped at K iterations polls K times (the
    header says so); an interrupt there hands back the iterate like any loop-top one."""
    lab, w, lev, b, x0 = _inputs("solid", 64, domain_factory, True)
    run = InterruptedSolves(lab, w, lev, False, b, x0, _options(mode, precision=1))
    try:
        assert run.truncated(4)[2] == 4
        xh, err, polls = run.interrupted(2)
        assert err.status == INTERRUPTED and polls == 3 and err.stats["iterations"] == 2 and err.stats["outcome"] == "max_iterations"
        assert ulps(xh, run.truncated(2)[0]) <= (0 if mode == 0 else 1)
    finally:
        run.s.close()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("use_gs", [False, True])
def test_interrupted_enclosed_liquid_is_projected(use_gs, mode, torch_cuda):
    """options.enclosed_liquid on the sealed tank of tests/test_enclosed_liquid.py: an interrupted solve hands back the iterate
    with mean zero on the enclosed component like every other exit (the bound that file puts on converged solves: 1e-6 of
    max |x|), from a loop-top poll and from a poll inside the V-cycle."""
    from geometricmultigridpressuresolver_amd import domains as D
    from test_enclosed_liquid import tank

    n, levels = 64, 4
    lab, w = tank(n, levels)
    b = D.random_rhs(lab, 1.0 / n)
    run = InterruptedSolves(lab, w, levels, use_gs, b, np.zeros(lab.shape, dtype=np.float32), _options(mode, enclosed_liquid=1))
    try:
        assert run.s.enclosed_components()[0] == 1
        ranks = run.s.enclosed_ranks()
        cycle = 2 * run.levels - 3
        for poll in (cycle + 2 * (cycle + 1), cycle + 2 * (cycle + 1) + 2):  # the top of iteration 2, and inside its V-cycle
            it, u, in_cycle = poll_site(poll, run.levels)
            assert (it, u) == ((2, 3) if in_cycle else (2, 2))
            xh, err, polls = run.interrupted(poll)
            assert err.status == INTERRUPTED and polls == poll + 1
            assert err.stats["outcome"] == "max_iterations" and err.stats["iterations"] == it, err.stats
            d = ulps(xh, run.truncated(u)[0])
            mean = abs(xh.ravel()[ranks == 0].astype(np.float64).mean())
            print(f"enclosed tank gs={int(use_gs)} mode={mode} poll {poll} (in cycle: {in_cycle}): {d} ulp, |mean| {mean:.2e} of max |x| {np.abs(xh).max():.2e}")
            assert np.abs(xh).max() > 0 and d <= 1
            assert mean <= 1e-6 * np.abs(xh).max()
    finally:
        run.s.close()


# ---- 3. one layer out --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_forms_hand_back_the_iterate(dtype, domain_factory, torch_cuda):
    """mgps_solve_pcg_host / _host_f64 (pcg_fp64_vectors = 2) interrupted inside a V-cycle: the host buffer receives the iterate,
    as the device form's x does (include/mgps.h), and the stats say which."""
    import geometricmultigridpressuresolver_amd as G

    lab, w, lev, b, x0 = _inputs("solid", 64, domain_factory, True)
    run = InterruptedSolves(lab, w, lev, False, b, x0, _options(2))
    try:
        cycle = 2 * run.levels - 3
        poll = cycle + 2 * (cycle + 1) + 2  # inside the V-cycle of iteration 2: three updates applied
        assert poll_site(poll, run.levels) == (2, 3, True)
        xt = run.truncated(3)[0]
        run.poller.arm(poll)
        with pytest.raises(G.MgpsError) as err:
            run.s.solvePcgHost(x0.astype(dtype), b.astype(dtype), UNREACHABLE, 200, True)
        e = err.value
        assert e.status == INTERRUPTED and run.poller.polls == poll + 1
        assert e.stats["outcome"] == "max_iterations" and e.stats["iterations"] == 2, e.stats
        assert e.solution.dtype == dtype
        back = e.solution.astype(np.float32)
        assert np.array_equal(back.astype(dtype), e.solution)  # (the double form widens fp32 values)
        d = ulps(back, xt)
        print(f"host form {np.dtype(dtype).name}: {d} ulp from the truncated device solve")
        assert d <= 1
    finally:
        run.s.close()


def test_interrupted_projection_publishes_the_iterate(torch_cuda):
    """mgps_project_free_surface on the scene of test_one_call_projection_matches_the_pass_by_pass_pipeline, interrupted inside
    the V-cycle of iteration 2: status MGPS_ERR_INTERRUPTED, and the pressure (liquid cells; zero elsewhere) and velocity it
    publishes are those of the same call capped at three iterations."""
    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import domains as D
    from geometricmultigridpressuresolver_amd import fields as F

    shape = (40, 32, 48)
    sc = D.projection_scene(shape, with_solid_velocity=True)
    poller = Poller()
    opt = poller.install(G.default_options())

    def call(max_iterations):
        h = lambda a: np.array(a, dtype=np.float32, order="C", copy=True)  # noqa: E731
        vel, p = [h(a) for a in sc["velocity"]], np.zeros(shape, dtype=np.float32)
        args = (h(sc["liquid_phi"]), h(sc["solid_phi"]), [h(a) for a in sc["cut_weights"]], vel, p, [h(a) for a in sc["solid_velocity"]])
        kw = dict(use_old_pressure=False, tolerance=UNREACHABLE, max_iterations=max_iterations, options=opt)
        try:
            valid, info = F.project_free_surface(*args, **kw)
            return 0, info, p, vel
        except G.MgpsError as e:
            return e.status, e.info, p, vel

    poller.arm(None)
    status, info3, p3, vel3 = call(3)
    assert status == 0 and info3["iterations"] == 3 and info3["outcome"] == 3  # MGPS_PCG_MAX_ITERATIONS
    L = info3["mg_levels"]
    cycle = 2 * L - 3
    assert poller.polls == cycle * 4 + 3
    poll = cycle + 2 * (cycle + 1) + 2
    assert poll_site(poll, L) == (2, 3, True)
    poller.arm(poll)
    status, info, p, vel = call(200)
    assert status == INTERRUPTED and poller.polls == poll + 1
    assert info["iterations"] == 2 and info["outcome"] == 3, info
    assert np.abs(p3).max() > 0
    d = [ulps(p, p3)] + [ulps(vel[a], vel3[a]) for a in range(3)]
    print(f"one-call projection: pressure {d[0]} ulp, velocity {d[1:]} ulp from the call capped at 3 iterations")
    assert max(d) <= 1, d


MEASURED = """
MI355X, the largest value of each quantity over the cases of part 1 (zero and random guess, all three domains, both smoothers and
preconditioners), per pcg_fp64_vectors mode; residual figures over the compared k only:

  mode   x vs oracle (bound 2e-5)   rel_residual vs oracle (1e-3)   rel_residual_recomputed vs fp64 residual of the returned x (1e-3)
  0      7.6e-7                     1.4e-5 (printed, not asserted)  2.3e-4 (printed, not asserted)
  1      1.5e-7                     4.0e-6                          1.5e-4
  2      3.2e-7                     4.8e-5                          2.3e-5
  precision = 1, mode 1: rel_residual_recomputed vs the fp64 residual of the returned x 1.7e-5.

Interrupted against truncated (part 2 and 3): 0 ulp at every poll in every mode, host forms and one-call projection included --
bit equality held in modes 1 and 2 as well, where one ulp is allowed.  Sealed tank: |mean| of the interrupted x at most 3e-13
against max |x| 4e-4 (bound 1e-6 of it).  The poll counts matched 2 L - 3 per V-cycle + 1 per iteration (L = 5 on solid 64: 79
polls tried per mode and smoother); the binary16 cycle polled at the loop top only.  Mode 2 flushed its pending updates after
the updates 2 and 6 there (either smoother: with the exit made to ignore pending updates, the loop-top polls of iterations 1, 3,
4, 5, 7, 8 came back wrong, those of 0, 2 and 6 right), so the polls tried hold loop-top and in-cycle polls in the middle of a
group and right after a flush.

Before the exits were routed through one place (PcgExit, csrc/mgps_solver.hip) the following failed: every in-cycle poll left
outcome / iterations zeroed in modes 0 and 2 (70 of 70 polls) and, inside the first preconditioner application, in mode 1 (7
of 70); in mode 2 the x handed back from an in-cycle poll after the first update was the sum of the pending updates, 1.0 to 4.6
(relative L2) from the iterate at 63 of 70 polls; the sealed tank's mode-1 iterate came back unprojected from a loop-top poll
(12 410 ulp from the projected one with Jacobi, 111 208 with Gauss-Seidel); the host forms and the one-call projection, stopped
inside a cycle in mode 2, reported outcome 0 / iterations 0 (and the host forms left the buffer as passed in).
"""
