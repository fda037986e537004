"""options.enclosed_liquid on the device: liquid that touches no air (a sealed tank, a pocket behind EXTERIOR walls, a pocket cut
off by zero-weight faces).  The fine level's components are labelled at set-up (union-find on the device; the host builder is the
checker), mgps_solve_pcg solves A x = P b with P = "subtract the mean on each enclosed component", and a domain without such a
component gives the bits of the option off."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import scipy.sparse.csgraph as csg  # noqa: E402

import geometricmultigridpressuresolver_amd as G  # noqa: E402
from geometricmultigridpressuresolver_amd import domains as D  # noqa: E402
from test_oracle_properties import assemble  # noqa: E402

pytestmark = pytest.mark.gpu


def tank(n, levels, open_top=False):
    """INTERIOR liquid in an EXTERIOR shell of 2^(levels-1) cells, unit weights; open_top: the top liquid layer is DIRICHLET"""
    s = 2 ** (levels - 1)
    lab = np.full((n, n, n), D.EXTERIOR, dtype=np.uint8)
    lab[s:n - s, s:n - s, s:n - s] = D.INTERIOR
    if open_top:
        lab[n - s - 1, s:n - s, s:n - s] = D.DIRICHLET
    w = [np.ones(D.face_shape(n, n, n, a), dtype=np.float32) for a in range(3)]
    D.set_boundary_labels(lab, w)
    return lab, w


def three_pockets(n=64, levels=4):
    """an open pool (x < n/2 - 4), a pocket sealed by an EXTERIOR wall (x >= n/2 + 4) and, between them, a pocket cut off from the
    pool by zero-weight x faces only"""
    s = 2 ** (levels - 1)
    lab = np.full((n, n, n), D.EXTERIOR, dtype=np.uint8)
    lab[s:n - s, s:n - s, s:n // 2 - 4] = D.INTERIOR  # pool
    lab[n - s - 1, s:n - s, s:n // 2 - 4] = D.DIRICHLET  # its air
    lab[s:n - s, s:n - s, n // 2 - 4:n // 2] = D.INTERIOR  # the weight-sealed pocket
    lab[s:n - s, s:n - s, n // 2 + 4:n - s] = D.INTERIOR  # the wall-sealed pocket
    w = [np.ones(D.face_shape(n, n, n, a), dtype=np.float32) for a in range(3)]
    w[0][:, :, n // 2 - 4] = 0.0  # the faces between the pool and the middle pocket
    D.set_boundary_labels(lab, w)
    return lab, w


def reference_ranks(lab, w):
    """rank of each cell's enclosed component (-1 elsewhere) from the SciPy assembly: components of the coupling graph, enclosed
    = no row with a DIRICHLET share, ranked by their minimum cell index"""
    A, idx, act = assemble(lab, w)
    A = A.tocsr()
    A.eliminate_zeros()
    _, comp = csg.connected_components(A, directed=False)
    cells = np.flatnonzero(act.ravel())
    dirichlet = np.asarray(A.sum(axis=1)).ravel() > 1e-6
    out = -np.ones(lab.size, dtype=np.int32)
    firsts = []
    for c in np.unique(comp):
        on = comp == c
        if not dirichlet[on].any():
            firsts.append((cells[on].min(), c))
    for r, (_, c) in enumerate(sorted(firsts)):
        out[cells[comp == c]] = r
    return out


def solver(lab, w, levels, gs, enclosed=1, **opts):
    o = G.default_options()
    o.enclosed_liquid = enclosed
    for k, v in opts.items():
        setattr(o, k, v)
    return G.GeometricMultigridPoissonSolver(lab, w, levels, gs, options=o)


def projected(b, ranks):
    pb = b.astype(np.float64).ravel().copy()
    for r in range(ranks.max() + 1):
        on = ranks == r
        pb[on] -= pb[on].mean()
    return pb


def rounding_floor(A, pb, ranks_active):
    """the true residual of the exact (fp64, mean-free on the enclosed components) solution rounded to fp32: what no fp32 x can beat"""
    import scipy.sparse.linalg as spla

    x, info = spla.cg(A, pb, rtol=1e-13, maxiter=20000)
    assert info == 0
    for r in range(ranks_active.max() + 1):
        x[ranks_active == r] -= x[ranks_active == r].mean()
    x32 = x.astype(np.float32).astype(np.float64)
    return np.linalg.norm(pb - A @ x32) / np.linalg.norm(pb)


def check_solve(lab, w, levels, gs, mode, host, ranks, tol=1e-6, res_bound=2e-6, floor=False):
    s = solver(lab, w, levels, gs, pcg_fp64_vectors=mode, host_setup=host)
    try:
        b = D.random_rhs(lab, 1.0 / lab.shape[0])
        x, bd = s.new_grid(), s.to_device(b)
        st = s.solveGeometricConjugateGradient(x, bd, tol, 400, True)
        assert st["outcome"] == "converged", st
        A, idx, act = assemble(lab, w)
        xa = x.cpu().numpy().astype(np.float64).ravel()[np.flatnonzero(act.ravel())]
        pb = projected(b, ranks)[np.flatnonzero(act.ravel())]
        res = np.linalg.norm(pb - A @ xa) / np.linalg.norm(pb)
        if floor:  # (a domain whose solution fp32 cannot hold to res_bound: the bound is 1.2 x what rounding the exact one leaves)
            res_bound = max(res_bound, 1.2 * rounding_floor(A.tocsr(), pb, ranks[np.flatnonzero(act.ravel())]))
        assert res <= res_bound, (res, res_bound, st)
        xf = x.cpu().numpy().ravel().astype(np.float64)
        for r in range(ranks.max() + 1):
            assert abs(xf[ranks == r].mean()) <= 1e-6 * np.abs(xf).max()
        return st["iterations"], res
    finally:
        s.close()


@pytest.mark.parametrize("gs", [False, True])
def test_sealed_tank_256_converges_like_the_open_one(gs):
    """Sizes where the coarse correction matters: with the pinned solve alone (no projection of the coarse rhs) the 512^3 sealed
    tank did not converge in 400 iterations.  Measured with the coarse pseudo-inverse: 256^3 Jacobi 22 (open top 36), Gauss-Seidel
    18 (33); 512^3 25-31 against 42-52 (profiles/r06_enclosed_512.json).  Residuals as the solver reports them
    (pcg_fp64_vectors = 2: the recomputed one is a true fp64 residual of P b)."""
    n, levels = 256, 5
    its = {}
    for name, open_top in (("open", True), ("sealed", False)):
        lab, w = tank(n, levels, open_top)
        s = solver(lab, w, levels, gs)
        try:
            assert s.enclosed_components()[0] == (0 if open_top else 1)
            b = D.random_rhs(lab, 1.0 / n)
            x = s.new_grid()
            st = s.solveGeometricConjugateGradient(x, s.to_device(b), 1e-6, 400, True)
            assert st["outcome"] == "converged" and st["rel_residual_recomputed"] < 1e-6, st
            its[name] = st["iterations"]
            if not open_top:
                act = D.active_mask(lab)
                mean = float(x[torch.from_numpy(act).to(x.device)].double().mean())
                assert abs(mean) <= 1e-6 * float(x.abs().max())
        finally:
            s.close()
    print(f"256^3 gs={gs}: sealed {its['sealed']} it, open top {its['open']} it")
    assert its["sealed"] <= 1.5 * its["open"] + 2, its


@pytest.mark.parametrize("n,levels", [(64, 4), (128, 5)])
@pytest.mark.parametrize("gs", [False, True])
def test_sealed_tank_pcg(n, levels, gs):
    """Measured on MI355X, tolerance 1e-6, sealed / open-top MG-PCG iterations (true residual through the SciPy matrix, x as
    returned in fp32): 64^3 Jacobi 11 / 14 (mode 0 8.8e-7, modes 1 / 2 4.4e-7), 64^3 Gauss-Seidel 9 / 13 (mode 0 9.2e-7, modes
    1 / 2 6.1e-7), 128^3 Jacobi 13 / 22 (1.0e-6), Gauss-Seidel 12 / 18 (7.6e-7; pcg_fp64_vectors 2).  Bounds: 1.5 x the open
    tank's count (+2); true residual 2e-6 for modes 1 / 2, 2e-3 for mode 0 (the fp32 loop's eps * cond floor on other domains)."""
    lab, w = tank(n, levels)
    ranks = reference_ranks(lab, w)
    assert ranks.max() == 0
    lab_o, w_o = tank(n, levels, open_top=True)
    so = solver(lab_o, w_o, levels, gs)
    try:
        assert so.enclosed_components() == (0, 0)
        b = D.random_rhs(lab_o, 1.0 / n)
        st_o = so.solveGeometricConjugateGradient(so.new_grid(), so.to_device(b), 1e-6, 400, True)
    finally:
        so.close()
    modes = [(0, 0), (1, 0), (2, 0), (2, 1)] if n == 64 else [(2, 0)]
    for mode, host in modes:
        it, res = check_solve(lab, w, levels, gs, mode, host, ranks, res_bound=2e-6 if mode else 2e-3)
        print(f"n={n} gs={gs} mode={mode} host={host}: sealed {it} it (res {res:.2e}), open top {st_o['iterations']} it")
        assert it <= 1.5 * st_o["iterations"] + 2


def test_three_pockets_labels_and_solve():
    lab, w = three_pockets()
    ranks = reference_ranks(lab, w)
    assert ranks.max() == 1
    outs = []
    for host in (1, 0):
        s = solver(lab, w, 4, False, host_setup=host)
        try:
            m, cells = s.enclosed_components()
            assert m == 2 and cells == int((ranks >= 0).sum())
            outs.append(s.enclosed_ranks())
        finally:
            s.close()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], ranks)
    # The open pool's pressure is 500 x the rhs here: the exact solution rounded to fp32 leaves a true residual of 1.09e-4 (all of it in
    # the pool; 4e-9 in either pocket), and mode 2 returns 1.093e-4.  Mode 0 (fp32 iterate, measured 5.7e-4) floors at eps * cond.
    for mode in (0, 2):
        check_solve(lab, w, 4, True, mode, 0, ranks, res_bound=2e-6 if mode else 2e-3, floor=mode != 0)


@pytest.mark.parametrize("seed", [1, 2, 5])
def test_random_domain_ranks_match(seed):
    from test_device_setup import random_domain

    lab, w = random_domain((64, 64, 96), 3, seed)
    ranks = reference_ranks(lab, w)
    outs = []
    for host in (1, 0):
        s = solver(lab, w, 3, False, host_setup=host)
        try:
            m, cells = s.enclosed_components()
            assert m == ranks.max() + 1 and cells == int((ranks >= 0).sum())
            outs.append(s.enclosed_ranks() if m > 0 else ranks)
        finally:
            s.close()
    assert np.array_equal(outs[0], ranks) and np.array_equal(outs[1], ranks)


def _domains_without_pockets():
    lab, w = D.interior_cube(64, 4)[:2]
    yield "cube64", lab, w, 4
    lab, w, _ = D.free_surface_pool(128, 5)
    yield "pool128", lab, w, 5
    from test_device_setup import random_domain

    # (with closed faces every seed has hundreds of single-cell pockets; open ones leave a domain whose liquid all meets DIRICHLET cells)
    lab, w = random_domain((64, 64, 96), 3, 4, closed_faces=False)
    assert reference_ranks(lab, w).max() < 0
    yield "random4", lab, w, 3


def test_no_enclosed_component_is_bit_identical():
    names = []
    for name, lab, w, levels in _domains_without_pockets():
        names.append(name)
        b = D.random_rhs(lab, 1.0 / lab.shape[0])
        for gs in (False, True):
            outs = []
            for enclosed in (0, 1):
                s = solver(lab, w, levels, gs, enclosed)
                try:
                    assert s.enclosed_components() == (0, 0)
                    bd, xv, xp = s.to_device(b), s.new_grid(), s.new_grid()
                    s.applyVCycle(xv, bd, False)
                    s.applyVCycle(xv, bd, True)
                    st = s.solveGeometricConjugateGradient(xp, bd, 1e-6, 200, True)
                    st.pop("solve_ms")
                    outs.append((xv.clone(), xp.clone(), st))
                finally:
                    s.close()
            assert torch.equal(outs[0][0], outs[1][0]), name
            assert torch.equal(outs[0][1], outs[1][1]), name
            assert outs[0][2] == outs[1][2], name
    assert names == ["cube64", "pool128", "random4"]


def test_projection_symmetry_and_determinism():
    lab, w = three_pockets()
    ranks = reference_ranks(lab, w)
    s = solver(lab, w, 4, True)
    try:
        rng = np.random.default_rng(4)
        act = D.active_mask(lab)
        v = np.where(act, rng.standard_normal(lab.shape), 0).astype(np.float32)
        vd = s.to_device(v)
        mx = s.project_enclosed(vd)
        out = vd.cpu().numpy().ravel()
        means = [v.ravel()[ranks == r].astype(np.float64).mean() for r in range(2)]
        assert abs(mx - max(abs(m) for m in means)) <= 1e-6 * max(abs(m) for m in means) + 1e-12
        for r in range(2):
            on = ranks == r
            assert abs(out[on].astype(np.float64).sum()) <= 1e-6 * np.abs(v.ravel()[on]).sum()
        assert np.array_equal(out[ranks < 0], v.ravel()[ranks < 0])
        # the cycle with the option on: symmetric on the range, 1_C -> 0
        u1 = np.where(act, rng.standard_normal(lab.shape), 0).astype(np.float32)
        u2 = np.where(act, rng.standard_normal(lab.shape), 0).astype(np.float32)
        p1, p2 = s.to_device(u1), s.to_device(u2)
        s.project_enclosed(p1)
        s.project_enclosed(p2)
        m1, m2 = s.new_grid(), s.new_grid()
        s.applyVCycle(m1, p1, False)
        s.applyVCycle(m2, p2, False)
        a = float((p1.double() * m2.double()).sum())
        b = float((m1.double() * p2.double()).sum())
        assert abs(a - b) <= 1e-4 * max(abs(a), abs(b)), (a, b)
        ones = np.zeros(lab.size, dtype=np.float32)
        ones[ranks == 0] = 1.0
        m3 = s.new_grid()
        s.applyVCycle(m3, s.to_device(ones.reshape(lab.shape)), False)
        assert float(m3.abs().max()) == 0.0
        # same input, same bits
        xs = []
        bd = s.to_device(D.random_rhs(lab, 1.0 / 64))
        for _ in range(2):
            x = s.new_grid()
            s.solveGeometricConjugateGradient(x, bd, 1e-6, 200, True)
            xs.append(x)
        assert torch.equal(xs[0], xs[1])
    finally:
        s.close()


def test_refusals():
    lab, w = tank(64, 4)
    for kw in ({"enclosed_liquid": 2}, {"enclosed_liquid": 1, "precision": 1}):
        o = G.default_options()
        for k, v in kw.items():
            setattr(o, k, v)
        with pytest.raises(G.MgpsError) as e:
            G.GeometricMultigridPoissonSolver(lab, w, 4, False, options=o)
        assert e.value.status == 1 and "enclosed_liquid" in str(e.value)


def test_refused_on_slab_solvers():
    import ctypes as C

    from geometricmultigridpressuresolver_amd._lib import lib

    lab, w = tank(64, 4)
    o = G.default_options()
    o.enclosed_liquid = 1
    h = C.c_void_p()
    comm = (C.c_int * 64)()  # struct_size, rank, size, ...: one rank; refused before the transport is looked at
    comm[2] = 1
    wp = [np.ascontiguousarray(a) for a in w]
    st = lib().mgps_create_slab(C.byref(h), 64, 64, 64, np.ascontiguousarray(lab).ctypes.data_as(C.c_void_p),
                                *[a.ctypes.data_as(C.c_void_p) for a in wp], 4, 0, C.byref(o), C.byref(comm))
    assert st == 1 and not h.value
    assert b"enclosed_liquid" in lib().mgps_last_error(None)


def test_fields_sealed_box():
    from geometricmultigridpressuresolver_amd import fields as F

    shape = (40, 40, 40)
    sc = D.projection_scene(shape, seed=3)
    dx = sc["dx"]
    cw = [np.where(c > 0, 1.0, 0.0).astype(np.float32) for c in sc["cut_weights"]]  # no solid box; the walls stay closed
    for a in range(3):
        sl = [slice(None)] * 3
        sl[2 - a] = slice(1, -1)
        cw[a][tuple(sl)] = 1.0
    solid = np.full(shape, -dx, dtype=np.float32)
    factors = {}
    for scene in ("full", "air"):
        phi = np.full(shape, -dx, dtype=np.float32)
        if scene == "air":
            phi[-8:] = dx
        res = {}
        for its in (0, 200):
            o = G.default_options()
            o.enclosed_liquid = 1
            vel = [a.copy() for a in sc["velocity"]]
            _, info = F.project_free_surface(phi, solid, [c.copy() for c in cw], vel, np.zeros(shape, np.float32), use_old_pressure=False,
                                             tolerance=1e-6, max_iterations=its, options=o)
            res[its] = info
        assert res[200]["outcome"] == 0, res[200]
        assert res[200]["enclosed_components"] == (1 if scene == "full" else 0)
        factors[scene] = res[0]["divergence_max"] / res[200]["divergence_max"]
    # both drop by about 1e6, to the fp32 round-off of the divergence pass (measured: air 1.28e6, full 0.93e6); without the option the
    # sealed box does not converge at all
    assert factors["full"] >= 0.5 * factors["air"] and factors["full"] > 1e4, factors
