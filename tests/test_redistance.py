"""Redistancing on the device (include/mgps_fields.h, "redistancing") against tests/redistance_reference.py.

CPU: the restatement against analysis (an axis-aligned and an oblique plane), its invariants (signs, scale invariance, the bounds of
the Godunov update), the block rounds' fixpoint against plain Jacobi's, the window rule, the C ABI's refusals and the mirror's size.
GPU: the whole-grid entry against the restatement after rounds 0, 1, 2 and R* + 1 (R*: the restatement's rounds to its fixpoint) --
the fixpoint heals a wrong rim, so equality there alone would hide one --, the same bits twice, slab windows round by round against
the whole grid, and a drop in free flight with a redistance after every advection.

Tolerance.  Every operation of the definition is rounded on its own and fp64 sqrt and / are IEEE on the device, so bit-equality is
expected and printed.  The asserted bound is the derived one: G is non-expansive (its partial derivatives are >= 0 and sum to 1), so
a float32 rounding that falls the other way travels without growing: |got - want| <= (rounds inner + 2) 2^-24 B dx."""
import ctypes as C
import functools

import numpy as np
import pytest

import redistance_reference as RR
from refusals import refused as _refused

GRID = (19, 22, 37)  # section 21's grids: off every multiple of the 64 x 4 x 4 tile, rows across tile edges, a sheet one cell thick
SCENES = {"grid": (GRID, 21), "row64": ((5, 6, 64), 22), "row65": ((5, 6, 65), 23), "row131": ((5, 6, 131), 24), "sheet": ((1, 7, 70), 25)}
WINDOWS = {2: [0, 9, 19], 3: [0, 6, 13, 19]}  # base planes of the cuts: off the tile's 4 planes
BANDS, DXS, INNERS = (3.0, 6.0), (1.0, 0.37), (1, 4)


@functools.lru_cache(maxsize=None)
def scene(name):
    """phi = 3 (sin 0.3 x + cos 0.4 y + sin(0.5 z) / 2 + 0.2 + 0.3 noise) at the cell centres, five cells set to exactly 0; read-only"""
    shape, seed = SCENES[name]
    rng = np.random.default_rng(seed)
    z, y, x = np.indices(shape) + 0.5
    phi = (3.0 * (np.sin(0.3 * x) + np.cos(0.4 * y) + 0.5 * np.sin(0.5 * z) + 0.2 + 0.3 * rng.standard_normal(shape))).astype(np.float32)
    phi.ravel()[rng.choice(phi.size, 5, replace=False)] = 0.0
    phi.setflags(write=False)
    return phi


@functools.lru_cache(maxsize=None)
def restated(name, band, inner):
    """the restatement's states after 0 .. R* + 1 rounds (read-only), the interface count, the cells each round changed, R*"""
    phi = scene(name)
    state, iface = RR.init(phi, band)
    states, moved = [state], [0]
    while True:
        new = RR.round_(states[-1], band, inner)
        moved.append(RR.changed(new, states[-1]))
        states.append(new)
        if moved[-1] == 0:
            break
    for s in states:
        s.setflags(write=False)
    return {"states": states, "interfaces": int(iface.sum()), "moved": moved, "rstar": len(states) - 2}


def _signed(state):
    return state.astype(np.float64)


# ---- CPU: the restatement ------------------------------------------------------------------------------------------------------------
def test_restated_axis_aligned_plane():
    """phi = 3 (x - 10.3) on 30 x 6 x 5, band 6: clamp(x - 10.3, +-6) to 2^-23 6"""
    z, y, x = np.indices((5, 6, 30)) + 0.5
    phi = (3.0 * (x - 10.3)).astype(np.float32)
    state, rounds = RR.fixpoint(phi, 6.0, 4)
    err = np.abs(_signed(state) - np.clip(x - 10.3, -6.0, 6.0)).max()
    print(f"axis-aligned plane: worst error {err:.3e} after {rounds} rounds")
    assert err <= 2.0 ** -23 * 6.0, err


def _oblique(shape=(40, 40, 40)):
    z, y, x = np.indices(shape) + 0.5
    plane = 0.6 * x + 0.64 * y + 0.48 * z - 30.37
    away = (x > 8) & (x < 32) & (y > 8) & (y < 32) & (z > 8) & (z < 32)
    return plane, away


def test_restated_oblique_plane():
    """n = (0.6, 0.64, 0.48), phi scaled by 2.5: away from the walls the output is the plane's distance to 1e-5 of a cell (the
    gradient form of the interface cells is exact on a linear phi, and so is the Godunov update behind them)"""
    plane, away = _oblique()
    band = 6.0
    state, rounds = RR.fixpoint((2.5 * plane).astype(np.float32), band, 4)
    m = away & (np.abs(plane) < band - 1)
    err = np.abs(_signed(state) - plane)[m].max()
    print(f"oblique plane: worst error {err:.3e} on {int(m.sum())} cells after {rounds} rounds")
    assert m.sum() > 5000 and err <= 1e-5, err


def _sphere(shape=(40, 40, 40), centre=(19.3, 20.1, 20.6), radius=10.0):
    z, y, x = np.indices(shape) + 0.5
    return np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius


def test_restated_sphere_figures():
    """recorded in DESIGN.md section 22, not asserted beyond sanity: the sphere of radius 10 in 40^3, band 6, from its exact SDF"""
    exact = _sphere()
    band = 6.0
    phi = exact.astype(np.float32)
    for inner in (1, 4):
        state, rounds = RR.fixpoint(phi, band, inner)
        _, iface = RR.init(phi, band)
        err = np.abs(_signed(state) - exact)
        m = np.abs(exact) < band - 1
        print(f"sphere, inner {inner}: max {err[m].max():.4f} mean {err[m].mean():.4f} interface {err[iface].max():.4f} cells, {rounds} rounds")
        assert err[m].max() < 0.5 and err[iface].max() < 0.01


@pytest.mark.parametrize("name", list(SCENES))
def test_restated_signs_are_the_inputs(name):
    for band in BANDS:
        out = RR.scaled(restated(name, band, 4)["states"][-1], 0.37)
        assert np.array_equal(out <= 0, scene(name) <= 0) and np.array_equal(np.signbit(out), scene(name) <= 0)


def test_restated_scale_invariance():
    """redistancing 2.5 phi equals redistancing phi to 1e-5 cells"""
    for phi in (_sphere().astype(np.float32), scene("grid")):
        a, _ = RR.fixpoint(phi, 6.0, 4)
        b, _ = RR.fixpoint((np.float32(2.5) * phi).astype(np.float32), 6.0, 4)
        err = np.abs(_signed(a) - _signed(b)).max()
        print(f"scale invariance: {err:.3e}")
        assert err <= 1e-5, err


@pytest.mark.parametrize("name", list(SCENES))
def test_restated_bounds_of_the_update(name):
    """interface T <= 1; a cell behind them with T < B sits between min_nb T + 1 / sqrt 3 and min_nb T + 1 at the fixpoint"""
    for band in BANDS:
        B = RR.band_of(band)
        r = restated(name, band, 4)
        state = r["states"][-1]
        iface = RR.interface(np.signbit(state))
        T = np.abs(state).astype(np.float64)
        assert iface.sum() == r["interfaces"] and T[iface].max() <= 1.0
        least = np.full(T.shape, np.inf)
        for ax in range(3):
            for d in (1, -1):
                least = np.minimum(least, RR._shift(T, ax, d, np.inf))
        m = ~iface & (T < B)
        assert m.sum() > 50
        assert (T[m] >= least[m] + 1.0 / np.sqrt(3.0) - 1e-6).all() and (T[m] <= least[m] + 1.0 + 2.0 ** -23 * B).all()
        assert (T[~iface & ~m] == B).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_block_fixpoint_is_plain_jacobis(name):
    for band in BANDS:
        plain = restated(name, band, 1)["states"][-1]
        for inner in (2, 4, 8):
            got = restated(name, band, 4)["states"][-1] if inner == 4 else RR.fixpoint(scene(name), band, inner)[0]
            assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), (band, inner)
        assert restated(name, band, 4)["rstar"] <= restated(name, band, 1)["rstar"]
        assert restated(name, band, 1)["moved"][1] > 0 and restated(name, band, 4)["moved"][1] > 0


@pytest.mark.parametrize("size", [2, 3])
def test_restated_windows_equal_the_whole_grid(size):
    """every round from the planes a rank holds only: halo 4 for inner = 4, halo 1 for inner = 1; the counts add up; fewer planes
    than the rule asks for is refused"""
    phi, band, cuts = scene("grid"), 6.0, WINDOWS[size]
    for inner, halo in ((4, 4), (1, 1)):
        r = restated("grid", band, inner)
        parts = [RR.window_init(phi, band, (cuts[k], cuts[k + 1], 1)) for k in range(size)]
        assert np.array_equal(np.concatenate([p[0] for p in parts]).view(np.uint32), r["states"][0].view(np.uint32))
        assert sum(p[1] for p in parts) == r["interfaces"]
        for n in range(1, len(r["states"])):
            parts = [RR.window_round(r["states"][n - 1], band, inner, (cuts[k], cuts[k + 1], halo)) for k in range(size)]
            assert np.array_equal(np.concatenate([p[0] for p in parts]).view(np.uint32), r["states"][n].view(np.uint32)), (inner, n)
            assert sum(p[1] for p in parts) == r["moved"][n]
    for k in range(size):
        with pytest.raises(ValueError, match="too few"):
            RR.window_round(restated("grid", band, 4)["states"][0], band, 4, (cuts[k], cuts[k + 1], 1))
        with pytest.raises(ValueError, match="too few"):
            RR.window_init(phi, band, (cuts[k], cuts[k + 1], 0))


# ---- CPU: refusals and the mirror ------------------------------------------------------------------------------------------------------
def _desc(shape=(4, 4, 4), **kw):
    """a good desc on made-up addresses, 1 MiB apart (never dereferenced: every call below is refused on the host)"""
    from geometricmultigridpressuresolver_amd import fields as F

    d = F.RedistanceDesc()
    d.struct_size = C.sizeof(F.RedistanceDesc)
    d.gz, d.gy, d.gx = shape
    d.band, d.dx, d.rounds, d.inner = 6.0, 0.5, 3, 4
    d.phi_in, d.phi_out, d.scratch = 1 << 20, 2 << 20, 3 << 20
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_refusals_need_no_device_and_the_mirror_has_the_library_size():
    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd._lib import lib

    L = lib()
    assert C.sizeof(F.RedistanceDesc) == 72

    def checks(run, fn, make):
        d = make()
        d.struct_size -= 8
        _refused(run(d), fn, "struct_size")
        for k in ("gx", "gy", "gz"):
            _refused(run(make(**{k: 0})), fn, "extent")
        for bad in (float("nan"), float("inf"), 0.0, -1.0):
            _refused(run(make(band=bad)), fn, "band")
            _refused(run(make(dx=bad)), fn, "dx")
        _refused(run(make(rounds=-1)), fn, "rounds")
        _refused(run(make(inner=0)), fn, "inner", "1 .. 8")
        _refused(run(make(inner=9)), fn, "inner", "1 .. 8")
        _refused(run(make(phi_in=None)), fn, "phi_in")
        _refused(run(make(phi_out=None)), fn, "phi_out")
        # out of place: the ranges are compared, not the first addresses
        d = make()
        d.phi_out = d.phi_in + 4 * 4 * 4 * 4 - 4
        _refused(run(d), fn, "phi_in", "phi_out", "overlap")

    fn = "mgps_fields_redistance"
    run = lambda d: L.mgps_fields_redistance(C.byref(d), None)  # noqa: E731
    checks(run, fn, _desc)
    _refused(L.mgps_fields_redistance(None, None), fn, "struct_size")
    _refused(run(_desc(scratch=None)), fn, "scratch")
    d = _desc()
    d.scratch = d.phi_out + 16
    _refused(run(d), fn, "phi_out", "scratch", "overlap")
    d = _desc()
    d.scratch = d.phi_in
    _refused(run(d), fn, "phi_in", "scratch", "overlap")

    # the window entries
    shape = (32, 4, 4)
    splits = F.projection_slab_layout(shape, True, 2, False)["splits"]
    w0, w1 = F.slab_window(shape, True, splits, 0), F.slab_window(shape, True, splits, 1)
    assert w0.c0 == 0 and 0 < w0.c1 == w1.c0 and w1.c1 == 32
    make = lambda **kw: _desc(**{"shape": (w0.c1, 4, 4), "gz": 32, "scratch": None, **kw})  # noqa: E731  (the window's arrays, the whole grid's gz)
    entries = {
        "mgps_fields_slab_redistance_init": ("phi", lambda w, d, halo, lo, hi: L.mgps_fields_slab_redistance_init(w, d, halo, lo, hi, None)),
        "mgps_fields_slab_redistance_round": ("state", lambda w, d, halo, lo, hi: L.mgps_fields_slab_redistance_round(w, d, halo, lo, hi, 1, None)),
    }
    for fn, (what, entry) in entries.items():
        slab = lambda d, w=w0, halo=4, lo=None, hi=60 << 20: entry(C.byref(w) if w is not None else None, C.byref(d), halo, lo, hi)  # noqa: E731
        checks(slab, fn, make)
        _refused(entry(C.byref(w0), None, 4, None, 60 << 20), fn, "struct_size")
        _refused(slab(make(), w=None), "slab window")
        _refused(slab(make(gz=16)), fn, "extents")
        _refused(slab(make(), halo=-1), fn, "halo", "negative")
        _refused(slab(make(), hi=None), fn, what + "_hi", "above the window")
        _refused(slab(make(), w=w1, lo=None, hi=None), fn, what + "_lo", "below the window")
        _refused(slab(make(), halo=0, hi=None), fn, "too few halo planes")
        _refused(slab(make(), w=w1, halo=0, hi=None), fn, "too few halo planes")
        d = make()
        d.phi_out = (60 << 20) + 8
        _refused(slab(d), fn, "phi_out", what + "_hi", "overlap")
    # a cut off the tile's four planes: a round of inner = 4 reads past one plane, a round of inner = 1 does not (it gets as far as
    # the launch, which this test does not make: only the refusal is asked for)
    fn = "mgps_fields_slab_redistance_round"
    odd = F.slab_window((32, 4, 4), True, [0, splits[1] + 2, splits[2]], 0)
    assert odd.c1 == 17  # (a round of inner = 4 reads the planes up to 20)
    d = make(shape=(odd.c1, 4, 4), gz=32)
    _refused(L.mgps_fields_slab_redistance_round(C.byref(odd), C.byref(d), 1, None, 60 << 20, 0, None), fn, "too few halo planes", "inner = 4")
    _refused(L.mgps_fields_slab_redistance_round(C.byref(odd), C.byref(d), 2, None, 60 << 20, 0, None), fn, "too few halo planes", "inner = 4")


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------
PATTERN = 7777.0


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the scenes are read-only)


def _compare(got, want, rounds, inner, band, dx, what):
    """the bound of the module's docstring; prints the worst error; returns whether the bits are equal"""
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    bound = (rounds * inner + 2) * 2.0 ** -24 * RR.band_of(band) * dx
    equal = np.array_equal(got.view(np.uint32), want.view(np.uint32))
    print(f"{what}: worst |got - want| = {err:.3e} (bound {bound:.3e}){', bit-equal' if equal else ''}")
    assert err <= bound, (what, err, bound)
    return equal


CASES = [(name, band, dx, inner) for name in SCENES for band in BANDS for dx in DXS for inner in INNERS]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_device_equals_the_restatement(case):
    """rounds 0, 1, 2 and R* + 1 into outputs and scratch pre-filled with a pattern; counts[0] always equal, counts[1] equal where
    the states are bit-equal, > 0 after one round and 0 after R* + 1"""
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    name, band, dx, inner = case
    want = restated(name, band, inner)
    phi = _dev(scene(name))
    equal = True
    for rounds in sorted({0, 1, 2, want["rstar"] + 1}):
        counts = torch.zeros(2, dtype=torch.int64, device="cuda")
        out, scratch = torch.full_like(phi, PATTERN), torch.full_like(phi, PATTERN)
        got = F.redistance(phi, band, dx, rounds, inner, out=out, scratch=scratch, counts=counts)
        assert got is out
        equal &= _compare(got, RR.scaled(want["states"][rounds], dx), rounds, inner, band, dx, f"{case} rounds {rounds}")
        assert int(counts[0]) == want["interfaces"]
        if equal:
            assert int(counts[1]) == want["moved"][rounds], (rounds, counts.tolist(), want["moved"])
        if rounds == 1:
            assert int(counts[1]) > 0
        if rounds == want["rstar"] + 1:
            assert int(counts[1]) == 0
        assert np.array_equal(got.cpu().numpy() <= 0, scene(name) <= 0)


@pytest.mark.gpu
def test_two_calls_give_the_same_bits_whatever_the_scratch_holds():
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    phi = _dev(scene("grid"))
    runs = []
    for fill in (float("nan"), -3.0e7):
        for rounds in (3, 4):  # the initial launch writes the scratch, and the output
            runs.append(F.redistance(phi, 6.0, 0.37, rounds, 4, out=torch.full_like(phi, fill), scratch=torch.full_like(phi, fill)))
    assert torch.equal(runs[0], runs[2]) and torch.equal(runs[1], runs[3]) and not torch.equal(runs[0], runs[1])
    assert all(bool(torch.isfinite(r).all()) for r in runs)


@pytest.mark.gpu
def test_the_convenience_form_stops_at_the_fixpoint():
    """rounds = None: batches through the window entries on [0, gz) until a round changes nothing"""
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    for name in ("grid", "sheet"):
        for band, dx, inner in ((6.0, 0.37, 4), (3.0, 1.0, 1), (1.0, 1.0, 4)):
            state, rstar = RR.fixpoint(scene(name), band, inner)
            counts = torch.zeros(2, dtype=torch.int64, device="cuda")
            got = F.redistance(_dev(scene(name)), band, dx, inner=inner, counts=counts)
            made = rstar + 1 + max(2, int(np.ceil(band)))  # (no more rounds than that were made)
            _compare(got, RR.scaled(state, dx), made, inner, band, dx, f"{name} band {band} inner {inner}, to the fixpoint")
            assert counts.tolist() == [int(RR.init(scene(name), band)[1].sum()), 0]


def _halo_of(whole, d, halo):
    """the planes below and above the window `d` of a whole-grid tensor, as the neighbours would send them"""
    below, above = min(halo, d.c0), min(halo, d.gz - d.c1)
    return (whole[d.c0 - below:d.c0].contiguous() if below else None, whole[d.c1:d.c1 + above].contiguous() if above else None)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [2, 3])
def test_windows_equal_the_whole_grid(size):
    """cuts off the tile's four planes: init, then every round through the window entries with the halo planes sliced from the
    neighbours' states; every round's bits are the whole grid's and the ranks' counts add up.  Halo 4 with inner = 4, halo 1 with
    inner = 1; halo 1 with inner = 4 is refused"""
    import torch

    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd._lib import MgpsError

    lay = F.projection_slab_layout(GRID, True, 1, False)
    cuts = WINDOWS[size]
    splits = [0] + [lay["offset"] + c for c in cuts[1:-1]] + [lay["expanded"][0]]
    windows = [F.slab_window(GRID, True, splits, rank) for rank in range(size)]
    assert [(d.c0, d.c1) for d in windows] == list(zip(cuts[:-1], cuts[1:]))
    band, dx = 6.0, 0.37
    phi = _dev(scene("grid"))
    for inner, halo in ((4, 4), (1, 1)):
        total = torch.zeros(2, dtype=torch.int64, device="cuda")
        state = torch.cat([F.redistanceInitSlab(d, phi[d.c0:d.c1].contiguous(), band, halo, _halo_of(phi, d, halo), counts=total)
                           for d in windows])
        whole_counts = torch.zeros(2, dtype=torch.int64, device="cuda")
        assert torch.equal(state, F.redistance(phi, band, 1.0, 0, inner, counts=whole_counts))
        assert total.tolist() == whole_counts.tolist() and total[0] > 0
        rounds = restated("grid", band, inner)["rstar"] + 1
        for n in range(1, rounds + 1):
            total = torch.zeros(2, dtype=torch.int64, device="cuda")
            parts, scaled = [], []
            for d in windows:
                own, halos = state[d.c0:d.c1].contiguous(), _halo_of(state, d, halo)
                parts.append(F.redistanceRoundSlab(d, own, band, halo, halos, inner, last=False, out=torch.full_like(own, PATTERN)))
                scaled.append(F.redistanceRoundSlab(d, own, band, halo, halos, inner, last=True, dx=dx, counts=total))
            state = torch.cat(parts)
            whole_counts = torch.zeros(2, dtype=torch.int64, device="cuda")
            assert torch.equal(state, F.redistance(phi, band, 1.0, n, inner)), (inner, n)
            assert torch.equal(torch.cat(scaled), F.redistance(phi, band, dx, n, inner, counts=whole_counts)), (inner, n)
            assert int(total[1]) == int(whole_counts[1]) and int(total[0]) == 0
        assert int(total[1]) == 0
    for d in windows:
        own = state[d.c0:d.c1].contiguous()
        with pytest.raises(MgpsError, match="too few halo planes"):
            F.redistanceRoundSlab(d, own, band, 1, _halo_of(state, d, 1), 4)


def _gradient_defect(phi, width=3.0):
    """the mean of | |grad phi| - 1 | over |phi| < width, by central differences"""
    g = np.gradient(phi.astype(np.float64))
    m = np.abs(phi) < width
    return float(np.abs(np.sqrt(sum(c * c for c in g)) - 1.0)[m].mean())


@functools.lru_cache(maxsize=None)
def _free_flight(redistanced):
    """section 21's drop in free flight, twelve steps with MacCormack; with `redistanced` a redistance(phi, band=6) after every
    advection.  Returns (phi at the end, the cell counts of {phi < 0}, the centroid's offset from start + 12 dt U)"""
    from geometricmultigridpressuresolver_amd import fields as F

    import advection_reference as AR

    shape, radius, steps, dt, tolerance = (40, 40, 40), 8.0, 12, 1.7, 1e-5
    U = np.array([0.37, 0.21, -0.13], dtype=np.float32)
    start = np.array([14.0, 16.0, 22.0])
    x, s, _ = AR.targets(shape, 0)
    phi = (np.sqrt(((x - start) ** 2).sum(axis=1)) - radius).reshape(s).astype(np.float32)
    velocity = []
    for a in range(3):
        xf, sf, _ = AR.targets(shape, a + 1)
        velocity.append(np.where(np.sqrt(((xf - start) ** 2).sum(axis=1)) < radius + 1.0, U[a], np.float32(0)).reshape(sf).astype(np.float32))
    solid_phi = np.full(shape, -1.0, dtype=np.float32)
    cw = [np.ones(AR.grid_shape(shape, a + 1), dtype=np.float32) for a in range(3)]
    pressure = np.zeros(shape, dtype=np.float32)
    cells = [int((phi < 0).sum())]
    for step in range(steps):
        valid, info = F.project_free_surface(phi, solid_phi, cw, velocity, pressure, tolerance=tolerance)
        assert info["outcome"] in (0, 1, 2), (step, info)  # every projection converges
        vd = [_dev(v) for v in velocity]
        F.extrapolateVelocity(vd, [_dev(v) for v in valid], 8)
        vout, sout = F.advect(vd, dt, scalars=(_dev(phi),), scheme="maccormack")
        carried = F.redistance(sout[0], 6.0) if redistanced else sout[0]
        velocity, phi = [v.cpu().numpy() for v in vout], carried.cpu().numpy()
        cells.append(int((phi < 0).sum()))
    off = float(np.linalg.norm(x[(phi < 0).ravel()].mean(axis=0) - (start + steps * dt * U.astype(np.float64))))
    return phi, cells, off


@pytest.mark.gpu
def test_a_drop_in_free_flight_with_redistancing():
    """every projection converges, the centroid stays within section 21's 0.25 cell, and the mean of | |grad phi| - 1 | over
    |phi| < 3 is not larger than in the same run without redistancing"""
    phi, cells, off = _free_flight(True)
    plain, plain_cells, plain_off = _free_flight(False)
    with_, without = _gradient_defect(phi), _gradient_defect(plain)
    print(f"redistanced: mean | |grad phi| - 1 | = {with_:.4f}, cells {cells[0]} -> {cells[-1]}, centroid off by {off:.4f} cell")
    print(f"not redistanced: mean | |grad phi| - 1 | = {without:.4f}, cells {plain_cells[0]} -> {plain_cells[-1]}, centroid off by {plain_off:.4f} cell")
    assert off <= 0.25, off
    assert with_ <= without, (with_, without)
