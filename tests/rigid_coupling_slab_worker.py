"""Worker of tests/test_rigid_coupling_slabs.py: run under torch.distributed.run with 1, 2 or 4 ranks sharing the one GPU.  Two-way
rigid-body coupling on Z-slab ranks (include/mgps_fields.h, DESIGN.md section 17 "on slab ranks") against the whole-grid object,
the numpy restatement and the direct coupled solve.  The scenes are built here (numpy only) and imported by the test file.

modes: "apply" (scene A: the ranks' lists, apply, impulses and rigidVelocitySlab against the restatement and the whole-grid
passes), "one" (a world of one: the bits of the whole-grid object, no transport call), "solve" (scene B: mgps_solve_pcg_coupled on
a SlabSolver against the direct solve the test process hands over in MGPS_RC_SLAB_REF), "refusals" (one rank), "fail" (a transport
whose all-reduce fails on one rank).  Prints "WORKER_OK <rank>" on success.
"""
import ctypes as C
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rigid_coupling_reference as RC  # noqa: E402
import solid_forces_reference as R  # noqa: E402
from test_rigid_coupling import TOL, _box_tables, _motions  # noqa: E402

SHAPE_A = (48, 40, 56)  # (gz, gy, gx): the scene of the forces worker
BODIES_A = 3
CUT_PLANES = (8, 24, 40)  # the base planes the cuts of two and four ranks fall on
BASE_CUTS = {1: [], 2: [24], 4: [8, 24, 40]}
SHAPE_B = (48, 32, 40)
BOXES_B = [((4, 6, 6), (18, 26, 30)), ((22, 6, 14), (36, 26, 24))]  # (lo, hi) in (i, j, k)
SURFACE_B = 43.3


# ---- the scenes (numpy; the same on every rank and in the test process) -------------------------------------------------------------
def scene_a():
    """projection_scene with the z-face weights of the cut planes overwritten by a seeded choice among {0, 0.25, 0.6, 1}, ids drawn
    from -1 .. BODIES_A + 1, random centres and a random positive definite K per body (the draws of test_rigid_coupling.random_case).
    The material labels come from these weights: `material_of(sc)` on the device, the oracle's in the test process."""
    from geometricmultigridpressuresolver_amd import domains as D

    shape, bodies = SHAPE_A, BODIES_A
    sc = D.projection_scene(shape)
    rng = np.random.default_rng(77)
    cw = [a.copy() for a in sc["cut_weights"]]
    for k in CUT_PLANES:
        cw[2][k] = rng.choice(np.array([0.0, 0.25, 0.6, 1.0], dtype=np.float32), size=cw[2][k].shape)
    body = [rng.integers(-1, bodies + 2, size=R.face_shape(shape, a)).astype(np.int32) for a in range(3)]
    centres = rng.random((bodies + 1, 3)) * np.array([shape[2], shape[1], shape[0]])
    inv_mass = np.concatenate([[0.0], rng.uniform(0.5, 2.0, bodies) * 1e-3])
    inv_inertia = np.zeros((bodies + 1, 6))
    for r in range(1, bodies + 1):
        B = rng.standard_normal((3, 3))
        M = (B @ B.T + 0.5 * np.eye(3)) * 1e-5
        inv_inertia[r] = [M[0, 0], M[1, 1], M[2, 2], M[0, 1], M[0, 2], M[1, 2]]
    return dict(shape=shape, bodies=bodies, liquid_phi=sc["liquid_phi"], solid_phi=sc["solid_phi"], cut_weights=cw, body=body, centres=centres,
                inv_mass=inv_mass, inv_inertia=inv_inertia)


def scene_b():
    """the voxel pool of test_rigid_coupling.voxel_pool_inputs on 48 planes: a flat surface at k = 43.3, two voxel boxes (cut weights
    0 or 1) of 0.5 and 2 times the liquid's density that reach across the cuts at base planes 8 and 24, V* with spin.  `owner`: the
    body a cell belongs to (the material is SOLID exactly there)"""
    shape = SHAPE_B
    gz, gy, gx = shape
    k, j, i = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
    owner = np.zeros(shape, dtype=np.int32)
    for r, (lo, hi) in enumerate(BOXES_B, start=1):
        owner[(i >= lo[0]) & (i < hi[0]) & (j >= lo[1]) & (j < hi[1]) & (k >= lo[2]) & (k < hi[2])] = r
    liquid_phi = ((k + 0.5) - SURFACE_B).astype(np.float32) / max(shape)
    solid_phi = np.where(owner > 0, 1.0, -1.0).astype(np.float32) / max(shape)
    cw, ids = [], []
    for a in range(3):
        behind, front = R._behind_front(owner, a, 0)
        w = np.where((behind > 0) | (front > 0), 0.0, 1.0).astype(np.float32)
        ids.append(np.maximum(behind, front).astype(np.int32))
        sl = [slice(None)] * 3
        for end in (0, shape[2 - a]):  # closed walls, nobody's
            sl[2 - a] = end
            w[tuple(sl)] = 0.0
        cw.append(w)
    rng = np.random.default_rng(5)
    velocity = [(rng.random(w.shape) * 2 - 1).astype(np.float32) for w in cw]
    centres, inv_mass, inv_inertia = _box_tables(BOXES_B, [0.5, 2.0])
    return dict(shape=shape, bodies=2, owner=owner, liquid_phi=liquid_phi, solid_phi=solid_phi, cut_weights=cw, velocity=velocity, body=ids,
                centres=centres, inv_mass=inv_mass, inv_inertia=inv_inertia, motions=_motions(2, 52))


def base_cuts(splits, offset, gz):
    """the base planes the interior cuts of the expanded grid fall on"""
    return [min(max(e - offset, 0), gz) for e in splits[1:-1]]


def rank_counts(mask, splits, offset):
    """coupled cells per rank: a cell belongs to the rank that owns its base plane"""
    gz = mask.shape[0]
    edges = [0] + base_cuts(splits, offset, gz) + [gz]
    return [int(mask[a:b].sum()) for a, b in zip(edges[:-1], edges[1:])]


def fractional_liquid_faces(material, sc, k):
    """z-faces of base plane k with 0 < w < 1 that a body owns, between two LIQUID cells: a term of G on either side of a cut there"""
    cwz, rows = sc["cut_weights"][2], R.rows_of(sc["body"][2], sc["bodies"])
    return int(((material[k - 1] == R.LIQUID) & (material[k] == R.LIQUID) & (cwz[k] > 0) & (cwz[k] < 1) & (rows[k] > 0)).sum())


# ---- the device side ----------------------------------------------------------------------------------------------------------------
def _gpu():
    import torch
    import torch.distributed as dist

    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd import distributed as Dd
    import slab_slices as S

    return types.SimpleNamespace(torch=torch, dist=dist, G=G, F=F, Dd=Dd, S=S, dev=S.dev)


def window(grids, d, dev):
    return [dev(grids[0][d.c0:d.c1]), dev(grids[1][d.c0:d.c1]), dev(grids[2][d.c0:d.c1 + 1])]


def material_of(sc, g):
    return g.F.buildMaterialCellLabels(g.dev(sc["liquid_phi"]), g.dev(sc["solid_phi"]), [g.dev(a) for a in sc["cut_weights"]])


def whole_coupling(sc, material, eshape, offset, g, kinematic=False):
    z = 0.0 if kinematic else 1.0
    return g.F.RigidCoupling(material, [g.dev(a) for a in sc["cut_weights"]], [g.dev(b) for b in sc["body"]], sc["centres"], z * sc["inv_mass"],
                             z * sc["inv_inertia"], eshape, offset)


def slab_coupling(sc, material_h, d, comm, g, kinematic=False):
    z = 0.0 if kinematic else 1.0
    return g.F.RigidCoupling.on_slab(d, comm, g.dev(material_h[d.c0:d.c1]), window(sc["cut_weights"], d, g.dev), window(sc["body"], d, g.dev),
                                     sc["centres"], z * sc["inv_mass"], z * sc["inv_inertia"])


def failing_vtable(g, calls):
    """a mgps_comm of one rank whose every entry fails (and says so in `calls`)"""
    Dd = g.Dd
    silent = Dd.CommStruct()
    silent.struct_size, silent.size = C.sizeof(Dd.CommStruct), 1
    keep = [Dd._EXCH(lambda *a: calls.append("exchange") or 1), Dd._ALLR(lambda *a: calls.append("allreduce") or 1),
            Dd._ALLRD(lambda *a: calls.append("allreduce_device") or 1)]
    silent.exchange, silent.allreduce, silent.allreduce_device = keep
    return types.SimpleNamespace(struct=silent, rank=0, size=1, keep=keep)


def _base(expanded, shape, offset):
    gz, gy, gx = shape
    return expanded[offset:offset + gz, offset:offset + gy, offset:offset + gx]


def apply_mode():
    g = _gpu()
    comm = g.Dd.TorchDistComm()
    rank, size = comm.rank, comm.size
    sc = scene_a()
    shape, bodies = sc["shape"], sc["bodies"]
    material = material_of(sc, g)
    mat_h = material.cpu().numpy()
    mask = RC.coupled_mask(mat_h, sc["cut_weights"], sc["body"], bodies)
    Gm, K = RC.coupling_matrix(mat_h, sc["cut_weights"], sc["body"], sc["centres"]), RC.stiffness(sc["inv_mass"], sc["inv_inertia"])
    assert int(Gm.getnnz(axis=0).max()) < 1e5  # the premise of the apply bound (tests/test_rigid_coupling.py)
    for k in BASE_CUTS[size]:  # every interior cut that has liquid has fractional faces between two LIQUID cells
        wet = bool(((mat_h[k - 1] == R.LIQUID) | (mat_h[k] == R.LIQUID)).any())
        assert not wet or fractional_liquid_faces(mat_h, sc, k) > 0, k
    rng = np.random.default_rng(33)
    motions = np.concatenate([rng.standard_normal((bodies + 1, 3)), 0.1 * rng.standard_normal((bodies + 1, 3))], axis=1)
    before = [rng.standard_normal(R.face_shape(shape, a)).astype(np.float32) for a in range(3)]
    sv_whole = g.F.rigidVelocity([g.dev(a) for a in before], [g.dev(b) for b in sc["body"]], sc["centres"], motions)
    sv_whole = [a.cpu().numpy() for a in sv_whole]
    for p2 in (True, False):
        lay = g.F.projection_slab_layout(shape, p2, size, False)
        splits, eshape, offset = lay["splits"], lay["expanded"], lay["offset"]
        assert base_cuts(splits, offset, shape[0]) == BASE_CUTS[size], (splits, offset)
        d = g.F.slab_window(shape, p2, splits, rank)
        xr = np.random.default_rng(77)
        x = xr.standard_normal(eshape).astype(np.float32)  # (junk outside the LIQUID cells included: only coupled cells are read)
        y = xr.standard_normal(eshape).astype(np.float32)
        e = slice(d.e0, d.e1)
        cpl = slab_coupling(sc, mat_h, d, comm, g)
        whole = whole_coupling(sc, material, eshape, offset, g)
        try:
            # the lists: the rank's own cells, every cell on one rank
            want = rank_counts(mask, splits, offset)
            counts = g.S.all_ranks(cpl.cells())
            assert counts == want and sum(counts) == whole.cells() == int(mask.sum()), (counts, want, whole.cells())
            if size == 4:
                assert 0 in counts, counts  # a rank with an empty list still takes part in every all-reduce below
            before_ar = comm.device_allreduces
            xd = g.dev(x[e])
            first, second = cpl.apply(g.dev(y[e]), xd).cpu().numpy(), cpl.apply(g.dev(y[e]), xd).cpu().numpy()
            assert comm.device_allreduces - before_ar == 2  # one all-reduce per application
            got_imp = cpl.impulses(xd)
            whole_imp = whole.impulses(g.dev(x))
            host_path = None
            if not p2:  # a transport without allreduce_device: g goes through the host
                plain = g.Dd.TorchDistComm()
                plain.struct.allreduce_device = g.Dd._ALLRD()
                via_host = slab_coupling(sc, mat_h, d, plain, g)
                try:
                    host_path = via_host.apply(g.dev(y[e]), xd).cpu().numpy()
                    assert plain.device_allreduces == 0
                finally:
                    via_host.close()
        finally:
            cpl.close()
            whole.close()
        xb = np.where(mat_h == R.LIQUID, _base(x, shape, offset).astype(np.float64), 0.0)
        add, mag = RC.apply_terms(Gm, K, xb)
        yb = _base(y, shape, offset).astype(np.float64)
        ref, sizes = yb + add.reshape(shape), np.abs(yb) + mag.reshape(shape)
        full = y.copy()  # the window's result laid into the whole expanded grid
        full[e] = first
        m = mask.copy()
        m[:d.c0], m[d.c1:] = False, False  # the rank's own coupled cells
        gotb = _base(full, shape, offset).astype(np.float64)
        err, lim = np.abs(gotb - ref)[m], (2.0 ** -24 * np.abs(ref) + 1e-10 * sizes)[m]
        worst = float((err / lim).max()) if m.any() else 0.0
        assert (err <= lim).all(), (p2, worst)
        assert not m.any() or np.abs(add.reshape(shape)[m]).max() > 1e-3
        outside = np.ones(eshape, dtype=bool)
        _base(outside, shape, offset)[m] = False
        assert np.array_equal(full[outside].view(np.int32), y[outside].view(np.int32))  # every other cell keeps its bits
        assert np.array_equal(first.view(np.int32), second.view(np.int32))  # two calls, equal bits
        if host_path is not None:
            full_h = y.copy()
            full_h[e] = host_path
            assert (np.abs(_base(full_h, shape, offset).astype(np.float64) - ref)[m] <= lim).all() and np.array_equal(full_h[outside], y[outside])
        # impulses: the whole grid's numbers on every rank, the same bits
        _, fmag = R.solid_forces(np.ascontiguousarray(_base(x, shape, offset)), mat_h, sc["cut_weights"], sc["body"], sc["centres"], 1.0)
        ierr = np.abs(got_imp[1:] - whole_imp[1:]) / np.maximum(fmag[1:, :6], 1e-300)
        assert np.array_equal(got_imp[0], np.zeros(6)) and np.abs(whole_imp[1:]).max() > 1 and ierr.max() <= 1e-10, ierr.max()
        seen = g.S.all_ranks(got_imp.tobytes())
        assert all(b == seen[0] for b in seen), "the ranks hold different impulses"
        # rigidVelocitySlab: the whole-grid pass on the window, bit for bit (both copies of a cut's z-face plane included)
        sv = g.F.rigidVelocitySlab(d, window(before, d, g.dev), window(sc["body"], d, g.dev), sc["centres"], motions)
        for a, ref_a in enumerate(g.S.faces(sv_whole, d)):
            got_a = sv[a].cpu().numpy()
            assert np.array_equal(got_a.view(np.int32), ref_a.view(np.int32)), (p2, a)
            owned = R.rows_of(g.S.faces(sc["body"], d)[a], bodies) > 0
            assert owned.any() and (~owned).any()
            assert np.array_equal(got_a[~owned].view(np.int32), g.S.faces(before, d)[a][~owned].view(np.int32))  # row 0 keeps its values
            assert not np.array_equal(got_a[owned], g.S.faces(before, d)[a][owned])
        worsts = g.S.all_ranks(worst)
        if rank == 0:
            print(f"apply power_of_two={p2} cuts {splits} (base {BASE_CUTS[size]}): coupled cells per rank {counts} of {int(mask.sum())}, "
                  f"worst |error| / bound {max(worsts):.3f}, impulses against the whole-grid object {ierr.max():.2e} (bound 1e-10), "
                  f"fractional liquid z-faces on the cuts {[fractional_liquid_faces(mat_h, sc, k) for k in BASE_CUTS[size]]}", flush=True)


def one_mode():
    """a slab coupling of one rank over a vtable whose every entry fails: apply and impulses equal the whole-grid object's bit for
    bit, and nothing of the transport is called"""
    g = _gpu()
    sc = scene_a()
    shape = sc["shape"]
    material = material_of(sc, g)
    mat_h = material.cpu().numpy()
    calls = []
    silent = failing_vtable(g, calls)
    for p2 in (True, False):
        lay = g.F.projection_slab_layout(shape, p2, 1, False)
        eshape, offset = lay["expanded"], lay["offset"]
        d = g.F.slab_window(shape, p2, lay["splits"], 0)
        assert d.expanded_shape == tuple(eshape)
        rng = np.random.default_rng(78)
        x, y = rng.standard_normal(eshape).astype(np.float32), rng.standard_normal(eshape).astype(np.float32)
        cpl, whole = slab_coupling(sc, mat_h, d, silent, g), whole_coupling(sc, material, eshape, offset, g)
        try:
            assert cpl.cells() == whole.cells() > 3 * 256
            a, b = cpl.apply(g.dev(y), g.dev(x)).cpu().numpy(), whole.apply(g.dev(y), g.dev(x)).cpu().numpy()
            ia, ib = cpl.impulses(g.dev(x)), whole.impulses(g.dev(x))
            va, vb = cpl.velocities(g.dev(x), np.ones((4, 6))), whole.velocities(g.dev(x), np.ones((4, 6)))
        finally:
            cpl.close()
            whole.close()
        assert not np.array_equal(a, y) and np.array_equal(a.view(np.int32), b.view(np.int32)), "one rank differs from the whole-grid object"
        assert np.abs(ib[1:]).min() > 0 and np.array_equal(ia, ib) and np.array_equal(va[0], vb[0])
        assert not calls, calls
    cells = int(RC.coupled_mask(mat_h, sc["cut_weights"], sc["body"], sc["bodies"]).sum())
    print(f"one rank: {cells} coupled cells, equal bits with the whole-grid object, no transport call", flush=True)


def counting_comm(g):
    """a TorchDistComm that counts the all-reduces carrying more than one value (the solver's own reductions carry one)"""

    class Counting(g.Dd.TorchDistComm):
        wide = 0

        def _allreduce(self, user, values, count, op):
            self.wide += count > 1
            return super()._allreduce(user, values, count, op)

        def _allreduce_device(self, user, values_dev, count, op, stream):
            self.wide += count > 1
            return super()._allreduce_device(user, values_dev, count, op, stream)

    return Counting()


def solve_mode():
    """scene B, the tight expansion: the windows of labels, weights and right-hand side are sliced from the whole grid's; the direct
    solves (coupled p, kinematic p0, V_out) come from the test process"""
    g = _gpu()
    torch = g.torch
    comm = counting_comm(g)
    rank, size = comm.rank, comm.size
    sc = scene_b()
    shape, bodies = sc["shape"], sc["bodies"]
    ref = np.load(os.environ["MGPS_RC_SLAB_REF"])
    labels, w32, active, mat_h = ref["labels"], [ref["wx"], ref["wy"], ref["wz"]], ref["active"], ref["material"]
    lay = g.F.projection_slab_layout(shape, False, size, False)
    splits, eshape, offset, levels = lay["splits"], lay["expanded"], lay["offset"], lay["levels"]
    assert tuple(eshape) == labels.shape and offset == int(ref["offset"]) and base_cuts(splits, offset, shape[0]) == BASE_CUTS[size], (lay, labels.shape)
    d = g.F.slab_window(shape, False, splits, rank)
    e = slice(d.e0, d.e1)
    # b = buildRHS(u, sv = rigidVelocity(V*)) on the whole grid, as tests/test_rigid_coupling.py makes it
    material = g.dev(mat_h)
    cw, body, vel = [g.dev(a) for a in sc["cut_weights"]], [g.dev(b) for b in sc["body"]], [g.dev(a) for a in sc["velocity"]]
    zeros = lambda: [torch.zeros(R.face_shape(shape, a), dtype=torch.float32, device="cuda") for a in range(3)]  # noqa: E731
    sv_star = g.F.rigidVelocity(zeros(), body, sc["centres"], sc["motions"])
    rhs = g.F.buildRHS(material, vel, cw, eshape, offset, sv_star)
    opt = g.G.default_options()
    opt.min_cells_per_rank, opt.pcg_fp64_vectors = 0, 1
    slab_w = [g.dev(w32[0][e]), g.dev(w32[1][e]), g.dev(w32[2][d.e0:d.e1 + 1])]
    s = g.Dd.SlabSolver(labels, slab_w, levels, False, comm, device=0, options=opt, splits=splits)
    assert s.slab_range(0) == (d.e0, d.e1)
    kin, cpl = slab_coupling(sc, mat_h, d, comm, g, kinematic=True), slab_coupling(sc, mat_h, d, comm, g)
    try:
        counts = g.S.all_ranks(cpl.cells())
        b = s.new_grid()
        b.copy_(rhs[e])
        x0, xk, x = s.new_grid(), s.new_grid(), s.new_grid()
        st0 = s.solveGeometricConjugateGradient(x0, b, TOL, 2500, True)  # the kinematic solve: the slab mgps_solve_pcg under pcg_fp64_vectors = 1
        stk = s.solve_pcg_coupled(kin, xk, b, TOL, 2500, True)
        assert st0["outcome"] == stk["outcome"] == "converged" and st0["iterations"] == stk["iterations"] > 3, (st0, stk)
        assert st0["rel_residual"] == stk["rel_residual"] and np.array_equal(x0.cpu().numpy(), xk.cpu().numpy())  # K = 0: the same iterates
        wide0 = comm.wide
        st = s.solve_pcg_coupled(cpl, x, b, TOL, 2500, True)
        wide = comm.wide - wide0
        v_out, impulses = cpl.velocities(x, sc["motions"])
        p_all, p0_all = s.gather_global(x), s.gather_global(x0)
    finally:
        kin.close()
        cpl.close()
        s.close()
    assert st["outcome"] == "converged", st
    # the applications of a converged pcg64 solve: the first residual, one per pass of the loop (iterations + 1 passes: the pass that
    # converges leaves by `break`, before the counter moves), the recomputed residual
    assert wide == st["iterations"] + 3, (wide, st["iterations"])
    rel_l2 = lambda a, r: float(np.linalg.norm(a - r) / np.linalg.norm(r))  # noqa: E731
    e0, err = rel_l2(p0_all[active].astype(np.float64), ref["p0"]), rel_l2(p_all[active].astype(np.float64), ref["p"])
    size_v = np.abs(ref["v_out"]).sum()
    e_v = np.abs(v_out - ref["v_out"]).sum() / size_v
    Gb, K = RC.coupling_matrix(mat_h, sc["cut_weights"], sc["body"], sc["centres"]), RC.stiffness(sc["inv_mass"], sc["inv_inertia"])
    p_base = np.where(mat_h == R.LIQUID, _base(p_all, shape, offset).astype(np.float64), 0.0).reshape(-1)
    host = RC.table(RC.flat(sc["motions"]) - K @ (Gb.T @ p_base))
    e_host = np.abs(v_out - host).sum() / size_v
    seen = g.S.all_ranks(v_out.tobytes() + impulses.tobytes())
    assert all(q == seen[0] for q in seen), "the ranks hold different V_out"
    # end to end on the gathered pressure with the whole-grid passes
    phi = g.dev(sc["liquid_phi"])
    valid = g.F.buildValidFaces(material, cw)

    def divergence(x_all, motions):
        pressure, v = torch.zeros(shape, dtype=torch.float32, device="cuda"), [a.clone() for a in vel]
        g.F.applySolutionToPressure(pressure, g.dev(x_all), material, offset)
        g.F.applyPressureGradient(v, phi, pressure, valid, material)
        sv_end = g.F.rigidVelocity(zeros(), body, sc["centres"], motions)
        return g.F.computeResultingDivergence(material, v, cw, sv_end)[1], g.F.computeResultingDivergence(material, v, cw, sv_star)[1]

    kin_div = divergence(p0_all, sc["motions"])[0]
    end, star = divergence(p_all, v_out)
    if rank == 0:
        print(f"solve on {size} ranks, cuts {splits} (base {BASE_CUTS[size]}): coupled cells per rank {counts}; pressure error {err:.3e} against "
              f"e0 = {e0:.3e} (bound 4 e0), V_out error {e_v:.3e}, V_out against the host's from the gathered p {e_host:.2e} (bound 1e-10), "
              f"iterations {st['iterations']} against {st0['iterations']} kinematic (bound +{6 * bodies + 2}), {wide} all-reduces of g = iterations + 3; "
              f"max divergence {end:.3e} against rigidVelocity(V_out), {kin_div:.3e} left by the kinematic solve (bound 4 x), "
              f"{star:.3e} against rigidVelocity(V*) ({star / end:.0f} x)", flush=True)
    assert err <= 4 * e0, (err, e0)
    assert e_v <= 4 * e0 and e_host <= 1e-10, (e_v, e_host, e0)
    assert st["iterations"] <= st0["iterations"] + 6 * bodies + 2, (st["iterations"], st0["iterations"])
    assert end <= 4 * kin_div and star > 100 * end, (end, kin_div, star)


def refusals_mode():
    """one rank over a transport of one: what mgps_solve_pcg_coupled refuses on slabs, each before any device work"""
    from test_rigid_coupling import _SoloComm

    g = _gpu()
    torch = g.torch
    sc = scene_b()
    shape = sc["shape"]
    ref = np.load(os.environ["MGPS_RC_SLAB_REF"])
    labels, w32, mat_h = ref["labels"], [ref["wx"], ref["wy"], ref["wz"]], ref["material"]
    lay = g.F.projection_slab_layout(shape, False, 1, False)
    splits, eshape, offset, levels = lay["splits"], lay["expanded"], lay["offset"], lay["levels"]
    solo = _SoloComm()
    d = g.F.slab_window(shape, False, splits, 0)
    opt = g.G.default_options()
    opt.min_cells_per_rank = 0
    slab = g.Dd.SlabSolver(labels, [g.dev(a) for a in w32], levels, False, solo, device=0, options=opt, splits=splits)
    whole = g.G.GeometricMultigridPoissonSolver(labels, w32, levels, False)
    mixed_opt = g.G.default_options()
    mixed_opt.precision = 1
    mixed = g.G.GeometricMultigridPoissonSolver(labels, w32, levels, False, options=mixed_opt)
    sealed_opt = g.G.default_options()
    sealed_opt.min_cells_per_rank, sealed_opt.enclosed_liquid = 0, 1
    sealed_labels = np.where(labels == g.G.domains.DIRICHLET, g.G.domains.EXTERIOR, labels).astype(np.uint8)  # no air: nothing open
    sealed = g.Dd.SlabSolver(sealed_labels, [g.dev(a) for a in w32], levels, False, solo, device=0, options=sealed_opt, splits=splits)
    material = g.dev(mat_h)
    on_slab = slab_coupling(sc, mat_h, d, solo, g)
    on_whole = whole_coupling(sc, material, eshape, offset, g)
    lay2 = g.F.projection_slab_layout(shape, False, 2, False)
    other = slab_coupling(sc, mat_h, g.F.slab_window(shape, False, lay2["splits"], 0), solo, g)  # the lower half's window: not this solver's
    try:
        assert sealed.enclosed_components()[0] >= 1
        b = slab.new_grid()
        b.copy_(torch.rand(eshape, device="cuda"))
        cases = ((whole, on_slab, ("slab coupling",)), (slab, on_whole, ("slab solver",)), (slab, other, ("window",)), (mixed, on_slab, ("precision",)),
                 (sealed, on_slab, ("enclosed",)))
        for solver, coupling, words in cases:
            x, rhs = solver.new_grid(), solver.new_grid()
            rhs.copy_(b)
            with_error = None
            try:
                solver.solve_pcg_coupled(coupling, x, rhs, TOL, 10, True)
            except g.G.MgpsError as err:
                with_error = err
            assert with_error is not None and with_error.status == 1 and all(w in str(with_error) for w in words), (words, str(with_error))
            assert float(x.abs().max()) == 0.0  # refused before any device work
        x = slab.new_grid()
        rhs = g.F.buildRHS(material, [g.dev(a) for a in sc["velocity"]], [g.dev(a) for a in sc["cut_weights"]], eshape, offset, None)
        b.copy_(rhs)
        st = slab.solve_pcg_coupled(on_slab, x, b, 1e-3, 100, True)  # and the solver is as good as new afterwards
        assert st["outcome"] == "converged" and float(x.abs().max()) > 0, st
    finally:
        for o in (on_slab, on_whole, other, slab, whole, mixed, sealed):
            o.close()
    print("refusals: whole solver + slab coupling, slab solver + whole-grid coupling, another window, precision = 1, an enclosed component; "
          "x untouched, the solver converges afterwards", flush=True)


def fail_mode():
    """rank 1's all-reduce of g delivers and then reports a failure: MGPS_ERR_COMM there, at once; rank 0, whose all-reduce went
    through, finishes its apply"""
    g = _gpu()
    rank = g.dist.get_rank()

    class Breaking(g.Dd.TorchDistComm):
        def _allreduce_device(self, *args):
            rc = super()._allreduce_device(*args)
            return 1 if self.rank == 1 else rc

    comm = Breaking()
    assert comm.size == 2
    sc = scene_a()
    shape = sc["shape"]
    mat_h = material_of(sc, g).cpu().numpy()
    lay = g.F.projection_slab_layout(shape, True, 2, False)
    d = g.F.slab_window(shape, True, lay["splits"], rank)
    cpl = slab_coupling(sc, mat_h, d, comm, g)
    try:
        x, y = g.torch.rand(d.expanded_shape, device="cuda"), g.torch.rand(d.expanded_shape, device="cuda")
        try:
            cpl.apply(y, x)
        except g.G.MgpsError as err:
            assert rank == 1 and err.status == 8 and "all-reduce failed" in str(err), (rank, err.status, str(err))
        else:
            assert rank == 0, "rank 1: a failing transport went unnoticed"
    finally:
        cpl.close()
    assert comm.device_allreduces == 1, (rank, comm.device_allreduces)
    print(f"rank {rank}: {'MGPS_ERR_COMM' if rank == 1 else 'done'} after {comm.device_allreduces} all-reduce", flush=True)


if __name__ == "__main__":
    from slab_slices import worker_main

    worker_main({"apply": apply_mode, "one": one_mode, "solve": solve_mode, "refusals": refusals_mode, "fail": fail_mode})
