"""Two-way rigid-body coupling (include/mgps_fields.h) against tests/rigid_coupling_reference.py.

CPU: the restatement's G K G^T is symmetric positive semidefinite, G^T p is minus the rows of the forces restatement, the direct
coupled solve leaves no divergence against V_out (and a large one against V*), K = 0 is the uncoupled solve, and the masses used keep
|G K G^T|_2 under 0.05 lambda_max(A); the C ABI refuses bad arguments on the host and the mirror has the library's size.
GPU: rigidVelocity, apply and impulses against the restatement on random ids; mgps_solve_pcg_coupled in the kinematic limit (equal
to mgps_solve_pcg under pcg_fp64_vectors = 1), against the direct coupled solve, interrupted, refused; project_free_surface_rigid
end to end.

Tolerances.
  * rigidVelocity: 1 ulp of float32 (one rounding of an fp64 value whose own evaluation order is the implementation's).
  * apply: 2^-24 |y_ref| + 1e-10 sum |terms| -- one rounding to float32 plus reordered fp64 sums of fewer than 1e5 terms (asserted):
    n 2^-53 = 1.1e-11 of the magnitude, the bound of tests/test_solid_forces.py.  impulses against mgps_fields_solid_forces: 1e-10
    of the rows' magnitude, the same bound.
  * coupled solve, tolerance 1e-7: relative L2 error of the pressure against the direct solve at most 4 e0, e0 the error of
    mgps_solve_pcg under pcg_fp64_vectors = 1 with the bodies kinematic against the direct solve of A, measured in the same test: both
    are the float32 storage of x plus what the tolerance leaves, on operators of the same conditioning (the CPU test asserts
    |G K G^T|_2 <= 0.05 lambda_max(A)); the factor 4 covers the different iterates.  V_out: 4 e0 of its magnitude sum; V_out
    recomputed on the host from the device's p: 1e-10 of it.  Iterations: at most 6 bodies + 2 more than the kinematic solve.
  * end to end: max divergence against rigidVelocity(V_out) at most 4 x what the kinematic projection leaves against V*; against
    rigidVelocity(V*) more than 100 x larger."""
import ctypes as C
import functools

import numpy as np
import pytest

import rigid_coupling_reference as RC
import solid_forces_reference as R
from conftest import rel_l2
from refusals import refused as _refused

SMALL, LARGE = (24, 16, 40), (45, 113, 131)
POOL = (28, 32, 40)  # the voxel pool: room for a 24 x 20 x 12 box under the free surface
TOL = 1e-7


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def _oracles():
    from oracle.mg_oracle import FieldsOracle, Oracle

    return FieldsOracle(), Oracle()


@functools.lru_cache(maxsize=None)
def cut_scene(shape):
    """projection_scene (a pool with a wavy surface and a box that cuts cells) with the oracle's material labels"""
    from geometricmultigridpressuresolver_amd import domains as D

    sc = D.projection_scene(shape)
    material = _oracles()[0].material_labels(sc["liquid_phi"], sc["solid_phi"], sc["cut_weights"]).astype(np.int32)
    return sc, material


def _box_tables(boxes, ratios):
    """centres, inv_mass, inv_inertia of axis-aligned boxes [(lo, hi)] (x, y, z in cells) of `ratios` times the liquid's density:
    inv_mass = 1 / (ratio volume), inv_inertia = the inverse of ratio volume (b^2 + c^2) / 12 on the diagonal, plus off-diagonal
    entries of a tenth of the geometric mean of their diagonal neighbours (still positive definite: a unit diagonal with 0.1 beside
    it after scaling), so that every entry of K is in use"""
    n = len(boxes)
    centres, inv_mass, inv_inertia = np.zeros((n + 1, 3)), np.zeros(n + 1), np.zeros((n + 1, 6))
    for r, ((lo, hi), ratio) in enumerate(zip(boxes, ratios), start=1):
        lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        ext = hi - lo
        mass = ratio * ext.prod()
        centres[r] = 0.5 * (lo + hi)
        inv_mass[r] = 1.0 / mass
        d = np.array([12.0 / (mass * (ext[1] ** 2 + ext[2] ** 2)), 12.0 / (mass * (ext[0] ** 2 + ext[2] ** 2)), 12.0 / (mass * (ext[0] ** 2 + ext[1] ** 2))])
        inv_inertia[r] = [d[0], d[1], d[2], 0.1 * np.sqrt(d[0] * d[1]), -0.1 * np.sqrt(d[0] * d[2]), 0.1 * np.sqrt(d[1] * d[2])]
    return centres, inv_mass, inv_inertia


def _motions(bodies, seed):
    """V*: linear velocities of the size of the scene's, spins that move the far faces about as fast"""
    rng = np.random.default_rng(seed)
    m = np.zeros((bodies + 1, 6))
    m[1:, :3] = 0.3 * rng.standard_normal((bodies, 3))
    m[1:, 3:] = 0.03 * rng.standard_normal((bodies, 3))
    return m


def _walls_unowned(ids, shape):
    for a in range(3):
        sl = [slice(None)] * 3
        for end in (0, shape[2 - a]):
            sl[2 - a] = end
            ids[a][tuple(sl)] = 0
    return ids


@functools.lru_cache(maxsize=None)
def split_box_inputs(bodies):
    """projection_scene(SMALL) with its box cut into `bodies` bodies by planes x = const; densities 0.5, 2, 0.5 of the liquid's"""
    shape = SMALL
    sc, material = cut_scene(shape)
    gz, gy, gx = shape
    lo = np.array([0.31, 0.27, 0.18]) * np.array([gx, gy, gz])  # the box of projection_scene, in cells
    hi = np.array([0.62, 0.71, 0.44]) * np.array([gx, gy, gz])
    planes = {2: [18.25], 3: [16.25, 20.75]}[bodies]  # (off every face centre: those sit at multiples of 1/2)
    ids = []
    for a in range(3):
        x = np.broadcast_to(R.face_centres(shape, a)[0], R.face_shape(shape, a))
        ids.append((1 + sum((x > p).astype(np.int32) for p in planes)).astype(np.int32))
    ids = _walls_unowned(ids, shape)
    edges = [lo[0]] + planes + [hi[0]]
    boxes = [((edges[r], lo[1], lo[2]), (edges[r + 1], hi[1], hi[2])) for r in range(bodies)]
    centres, inv_mass, inv_inertia = _box_tables(boxes, [0.5, 2.0, 0.5][:bodies])
    return dict(shape=shape, material=material, cut_weights=sc["cut_weights"], liquid_phi=sc["liquid_phi"], solid_phi=sc["solid_phi"],
                velocity=sc["velocity"], body=ids, centres=centres, inv_mass=inv_mass, inv_inertia=inv_inertia, motions=_motions(bodies, 40 + bodies))


@functools.lru_cache(maxsize=None)
def voxel_pool_inputs(boxes):
    """a pool under a flat free surface with `boxes` voxel boxes (cut weights 0 or 1) of 0.5 and 2 times the liquid's density"""
    shape = POOL
    gz, gy, gx = shape
    spans = {1: [((8, 6, 6), (32, 26, 18))], 2: [((4, 6, 6), (18, 26, 18)), ((22, 6, 6), (36, 26, 18))]}[boxes]
    k, j, i = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
    owner = np.zeros(shape, dtype=np.int32)
    for r, (lo, hi) in enumerate(spans, start=1):
        owner[(i >= lo[0]) & (i < hi[0]) & (j >= lo[1]) & (j < hi[1]) & (k >= lo[2]) & (k < hi[2])] = r
    liquid_phi = ((k + 0.5) - 22.3).astype(np.float32) / max(shape)
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
    material = _oracles()[0].material_labels(liquid_phi, solid_phi, cw).astype(np.int32)
    assert ((material == 0) == (owner > 0)).all()
    rng = np.random.default_rng(5)
    velocity = [(rng.random(w.shape) * 2 - 1).astype(np.float32) for w in cw]
    centres, inv_mass, inv_inertia = _box_tables(spans, [0.5, 2.0][:boxes])
    return dict(shape=shape, material=material, cut_weights=cw, liquid_phi=liquid_phi, solid_phi=solid_phi, velocity=velocity, body=ids,
                centres=centres, inv_mass=inv_mass, inv_inertia=inv_inertia, motions=_motions(boxes, 50 + boxes))


SOLVE_SCENES = {"box-in-2": (split_box_inputs, 2), "box-in-3": (split_box_inputs, 3), "voxel-1": (voxel_pool_inputs, 1), "voxel-2": (voxel_pool_inputs, 2)}


@functools.lru_cache(maxsize=None)
def solve_case(name, p2):
    """the inputs of a solve scene with the oracle's expanded domain (weights rounded to float32: the operator the device holds),
    the restatement's Scene, the fluid right-hand side on the unknowns and the two direct solves (coupled, kinematic)"""
    import geometricmultigridpressuresolver_amd as G

    make, n = SOLVE_SCENES[name]
    d = dict(make(n))
    fo, orc = _oracles()
    shape = d["shape"]
    valid = fo.valid_faces(d["material"], d["cut_weights"])
    eshape, offset, levels = G.expanded_layout(shape, 0, power_of_two=p2)
    lab = fo.domain_labels(d["material"], eshape, offset)
    w = fo.boundary_weights(d["cut_weights"], d["liquid_phi"], valid, d["material"], eshape, offset)
    w32 = [a.astype(np.float32) for a in w]
    orc.set_boundary_labels(lab, [a.astype(np.float64) for a in w32])
    ref = RC.Scene(d["material"], d["cut_weights"], d["body"], d["centres"], lab, w32, offset)
    b_fluid = ref.unknowns(fo.rhs(d["material"], d["velocity"], d["cut_weights"], eshape, offset, None))
    p, v_out, b = ref.solve(b_fluid, d["inv_mass"], d["inv_inertia"], d["motions"])
    p0, v0, b0 = ref.solve(b_fluid, 0 * d["inv_mass"], 0 * d["inv_inertia"], d["motions"])
    d.update(bodies=n, valid=valid, eshape=eshape, offset=offset, levels=levels, labels=lab.astype(np.uint8), w32=w32, ref=ref, b_fluid=b_fluid,
             p=p, v_out=v_out, b=b, p0=p0)
    assert np.array_equal(b, b0) and np.array_equal(v0, d["motions"])
    return d


@functools.lru_cache(maxsize=None)
def random_case(shape, bodies):
    """ids drawn from -1 .. bodies + 1 on the cut scene, random centres, a random positive definite K per body, and the
    restatement's G (base cells) and K"""
    sc, material = cut_scene(shape)
    rng = np.random.default_rng(200 + bodies)
    body = [rng.integers(-1, bodies + 2, size=R.face_shape(shape, a)).astype(np.int32) for a in range(3)]
    centres = rng.random((bodies + 1, 3)) * np.array([shape[2], shape[1], shape[0]])
    inv_mass = np.concatenate([[0.0], rng.uniform(0.5, 2.0, bodies) * 1e-3])
    inv_inertia = np.zeros((bodies + 1, 6))
    for r in range(1, bodies + 1):
        B = rng.standard_normal((3, 3))
        M = (B @ B.T + 0.5 * np.eye(3)) * 1e-5
        inv_inertia[r] = [M[0, 0], M[1, 1], M[2, 2], M[0, 1], M[0, 2], M[1, 2]]
    G = RC.coupling_matrix(material, sc["cut_weights"], body, centres)
    return dict(shape=shape, bodies=bodies, material=material, cut_weights=sc["cut_weights"], body=body, centres=centres, inv_mass=inv_mass,
                inv_inertia=inv_inertia, G=G, K=RC.stiffness(inv_mass, inv_inertia), mask=RC.coupled_mask(material, sc["cut_weights"], body, bodies))


# ---- CPU: the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bodies", [1, 3])
def test_restatement_operator_is_symmetric_positive_semidefinite(bodies):
    c = random_case(SMALL, bodies)
    rows = np.flatnonzero(c["mask"].reshape(-1))
    M = (c["G"] @ c["K"] @ c["G"].T).tocsr()
    assert M.nnz > 0 and np.setdiff1d(np.unique(M.nonzero()[0]), rows).size == 0  # nothing outside the coupled cells
    dense = M[rows][:, rows].toarray()
    assert np.abs(dense - dense.T).max() <= 1e-14 * np.abs(dense).max()
    ev = np.linalg.eigvalsh(0.5 * (dense + dense.T))
    print(f"G K G^T on {len(rows)} coupled cells: eigenvalues {ev.min():.3e} .. {ev.max():.3e}, rank {int((ev > 1e-12 * ev.max()).sum())}")
    assert ev.max() > 0 and ev.min() >= -1e-12 * ev.max() and (ev > 1e-9 * ev.max()).sum() == 6 * bodies


@pytest.mark.parametrize("bodies", [1, 3])
def test_restatement_adjoint_is_minus_the_forces(bodies):
    c = random_case(SMALL, bodies)
    rng = np.random.default_rng(8)
    pressure = (rng.random(SMALL) * 2 - 0.5).astype(np.float32)
    rows, mag = R.solid_forces(pressure, c["material"], c["cut_weights"], c["body"], c["centres"], 1.0)
    p = np.where(c["material"] == R.LIQUID, pressure.astype(np.float64), 0.0).reshape(-1)
    got = RC.table(c["G"].T @ p)[1:]
    err = np.abs(got + rows[1:, :6]) / mag[1:, :6]
    print(f"G^T p against -rows of solid_forces: worst |difference| / magnitude {err.max():.2e} (bound 1e-12)")
    assert np.abs(rows[1:, :6]).min() > 0 and err.max() <= 1e-12


@pytest.mark.parametrize("name", list(SOLVE_SCENES))
def test_direct_coupled_solve_is_divergence_free_against_v_out(name):
    c = solve_case(name, False)
    ref, G, A = c["ref"], c["ref"].G, c["ref"].A
    scale = np.abs(c["b"]).max()
    against_out = np.abs(A @ c["p"] - (c["b_fluid"] + G @ RC.flat(c["v_out"]))).max() / scale
    against_star = np.abs(A @ c["p"] - (c["b_fluid"] + G @ RC.flat(c["motions"]))).max() / scale
    print(f"{name}: |A p - (b_fluid + G V_out)| / |b| = {against_out:.2e} (bound 1e-10), against V*: {against_star:.2e}")
    assert against_out <= 1e-10 and against_star > 1e-3
    # K = 0 is the uncoupled solve
    assert np.abs(A @ c["p0"] - c["b"]).max() <= 1e-10 * scale
    assert rel_l2(c["p"], c["p0"]) > 1e-3  # (and the coupling matters on this scene)
    cells = int(RC.coupled_mask(c["material"], c["cut_weights"], c["body"], c["bodies"]).sum())
    if name == "voxel-1":
        assert cells == 2 * (24 * 20 + 20 * 12 + 24 * 12)  # 2016: eight workgroups of 256
    assert cells > (1200 if name.startswith("voxel") else 300)


@pytest.mark.parametrize("name", list(SOLVE_SCENES))
def test_coupling_norm_is_small_against_the_operator(name):
    """the premise of the solve tolerance: |G K G^T|_2 <= 0.05 lambda_max(A) for the masses used"""
    import scipy.sparse.linalg as spla

    c = solve_case(name, False)
    G, K = c["ref"].G, RC.stiffness(c["inv_mass"], c["inv_inertia"]).toarray()
    norm = np.abs(np.linalg.eigvals(K @ (G.T @ G).toarray())).max()  # (the non-zero eigenvalues of G K G^T)
    top = float(spla.eigsh(c["ref"].A, k=1, which="LA", return_eigenvectors=False)[0])
    print(f"{name}: |G K G^T|_2 = {norm:.4f}, lambda_max(A) = {top:.3f}, ratio {norm / top:.4f} (bound 0.05)")
    assert 0 < norm <= 0.05 * top


# ---- CPU: the C ABI refuses bad arguments on the host ----------------------------------------------------------------------------------
def _desc(**kw):
    from geometricmultigridpressuresolver_amd import fields as F

    tables = [np.zeros((4, 3)), np.ones(4), np.ones((4, 6))]
    d = F.CouplingDesc()
    d.struct_size = C.sizeof(F.CouplingDesc)
    d.gx = d.gy = d.gz = 4
    d.ex = d.ey = d.ez = 8
    d.offset, d.bodies = 2, 3
    d.material = 64  # (never dereferenced: every call below is refused on the host)
    for a in range(3):
        d.cut_weights[a] = d.body[a] = 64
    d.centres, d.inv_mass, d.inv_inertia = (t.ctypes.data for t in tables)
    for k, v in kw.items():
        setattr(d, k, v)
    return d, tables


def test_argument_refusals_need_no_device_and_the_mirror_has_the_library_size():
    from geometricmultigridpressuresolver_amd._lib import lib

    L, h = lib(), C.c_void_p()
    create = lambda d: L.mgps_coupling_create(C.byref(h), C.byref(d), None)  # noqa: E731
    # the mirror's size is the library's: a good struct gets as far as the next check, one of another size is refused as such
    d, keep = _desc(bodies=0)
    _refused(create(d), "mgps_coupling_create", "bodies", "1 .. 255")
    d.struct_size -= 4
    _refused(create(d), "struct_size")
    _refused(L.mgps_coupling_create(C.byref(h), None, None), "struct_size")
    for bodies in (256, -1):
        _refused(create(_desc(bodies=bodies)[0]), "bodies")
    for k in ("gx", "gy", "gz", "ex", "ey", "ez"):
        _refused(create(_desc(**{k: 0})[0]), "extent")
    _refused(create(_desc(offset=5)[0]), "expanded box")
    _refused(create(_desc(offset=-1)[0]), "expanded box")
    _refused(create(_desc(material=None)[0]), "material")
    for name, word in (("cut_weights", "cut weights"), ("body", "body")):
        d, keep = _desc()
        getattr(d, name)[1] = None
        _refused(create(d), word)
    for name in ("centres", "inv_mass", "inv_inertia"):
        _refused(create(_desc(**{name: None})[0]), name)
    d, keep = _desc()
    keep[1][2] = -1e-3
    _refused(create(d), "inv_mass", "body 2", "negative")
    keep[1][2] = 1.0
    keep[2][3, 1] = -1.0
    _refused(create(d), "inv_inertia", "body 3")
    assert not h.value
    p, d3 = C.c_void_p(64), np.zeros(24)
    rigid = L.mgps_fields_rigid_velocity
    for bodies in (0, 256):
        _refused(rigid(p, p, p, p, p, p, _ptr(d3), _ptr(d3), bodies, 4, 4, 4, None), "mgps_fields_rigid_velocity", "bodies")
    _refused(rigid(p, p, p, p, p, p, _ptr(d3), _ptr(d3), 3, 4, 0, 4, None), "extent")
    _refused(rigid(p, None, p, p, p, p, _ptr(d3), _ptr(d3), 3, 4, 4, 4, None), "solid velocity")
    _refused(rigid(p, p, p, p, p, None, _ptr(d3), _ptr(d3), 3, 4, 4, 4, None), "body")
    _refused(rigid(p, p, p, p, p, p, None, _ptr(d3), 3, 4, 4, 4, None), "centres")
    _refused(rigid(p, p, p, p, p, p, _ptr(d3), None, 3, 4, 4, 4, None), "motions")
    for call in (L.mgps_coupling_apply(None, p, p, None), L.mgps_coupling_impulses(None, p, _ptr(d3), None),
                 L.mgps_coupling_set_bodies(None, _ptr(d3), _ptr(d3), _ptr(d3), None)):
        _refused(call, "NULL coupling")
    status = L.mgps_solve_pcg_coupled(None, None, p, p, C.c_double(1e-5), 10, 1, None)
    assert status == 1 and "NULL handle" in L.mgps_last_error(None).decode()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ulps(a, b):
    def ordered(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    return np.abs(ordered(a) - ordered(b))


def _coupling(c, eshape, offset, kinematic=False):
    from geometricmultigridpressuresolver_amd import fields as F

    z = 0.0 if kinematic else 1.0
    return F.RigidCoupling(_dev(c["material"]), [_dev(a) for a in c["cut_weights"]], [_dev(b) for b in c["body"]], c["centres"], z * c["inv_mass"],
                           z * c["inv_inertia"], eshape, offset)


def _base(expanded, shape, offset):
    gz, gy, gx = shape
    return expanded[offset:offset + gz, offset:offset + gy, offset:offset + gx]


@pytest.mark.gpu
@pytest.mark.parametrize("bodies", [3, 255])
@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=["24x16x40", "45x113x131"])
def test_rigid_velocity_matches_restatement(shape, bodies):
    from geometricmultigridpressuresolver_amd import fields as F

    c = random_case(shape, bodies) if bodies == 3 else None
    rng = np.random.default_rng(31 + bodies)
    body = c["body"] if c else [rng.integers(-1, bodies + 2, size=R.face_shape(shape, a)).astype(np.int32) for a in range(3)]
    centres = c["centres"] if c else rng.random((bodies + 1, 3)) * np.array([shape[2], shape[1], shape[0]])
    motions = np.concatenate([rng.standard_normal((bodies + 1, 3)), 0.1 * rng.standard_normal((bodies + 1, 3))], axis=1)
    before = [rng.standard_normal(R.face_shape(shape, a)).astype(np.float32) for a in range(3)]
    sv = [_dev(a) for a in before]
    F.rigidVelocity(sv, [_dev(b) for b in body], centres, motions)
    ref = R.rigid_velocity(shape, body, centres, motions[:, :3], motions[:, 3:], bodies)
    for a in range(3):
        got, owned = sv[a].cpu().numpy(), R.rows_of(body[a], bodies) > 0
        assert owned.any() and (~owned).any() and (body[a] < 0).any() and (body[a] > bodies).any()
        worst = int(_ulps(got[owned], ref[a][owned].astype(np.float32)).max())
        print(f"rigidVelocity {shape} bodies {bodies} axis {a}: worst distance {worst} ulp (bound 1) on {int(owned.sum())} faces")
        assert worst <= 1
        assert np.array_equal(got[~owned].view(np.int32), before[a][~owned].view(np.int32))  # row 0 keeps its bits


@pytest.mark.gpu
@pytest.mark.parametrize("p2", [False, True], ids=["tight", "power-of-two"])
@pytest.mark.parametrize("bodies", [1, 3])
@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=["24x16x40", "45x113x131"])
def test_apply_matches_restatement_and_touches_coupled_cells_only(shape, bodies, p2):
    import geometricmultigridpressuresolver_amd as G

    c = random_case(shape, bodies)
    eshape, offset, _ = G.expanded_layout(shape, 0, power_of_two=p2)
    rng = np.random.default_rng(77)
    x = rng.standard_normal(eshape).astype(np.float32)  # (junk outside the LIQUID cells included: only coupled cells are read)
    y = rng.standard_normal(eshape).astype(np.float32)
    cpl = _coupling(c, eshape, offset)
    try:
        count = int(c["mask"].sum())
        terms = int(c["G"].getnnz(axis=0).max())  # the longest sum of a row of g; a cell's own sum has at most 6 * 6 terms
        assert cpl.cells() == count and count > 3 * 256 and terms < 1e5, (count, terms)  # more than three workgroups; the bound's premise
        xd = _dev(x)
        first, second = cpl.apply(_dev(y), xd).cpu().numpy(), cpl.apply(_dev(y), xd).cpu().numpy()
    finally:
        cpl.close()
    xb = np.where(c["material"] == R.LIQUID, _base(x, shape, offset).astype(np.float64), 0.0)
    add, mag = RC.apply_terms(c["G"], c["K"], xb)
    yb = _base(y, shape, offset).astype(np.float64)
    ref, size = yb + add.reshape(shape), np.abs(yb) + mag.reshape(shape)
    got = _base(first, shape, offset).astype(np.float64)
    m = c["mask"]
    err, lim = np.abs(got - ref)[m], (2.0 ** -24 * np.abs(ref) + 1e-10 * size)[m]
    print(f"apply {shape} bodies {bodies} p2 {p2}: {count} coupled cells, worst |error| / bound {float((err / lim).max()):.3f}, "
          f"largest |G K G^T x| / |y| {float(np.abs(add).max() / np.abs(yb).max()):.2e}")
    assert np.abs(add.reshape(shape)[m]).max() > 1e-3 and (err <= lim).all()
    outside = np.ones(eshape, dtype=bool)
    _base(outside, shape, offset)[m] = False
    assert np.array_equal(first[outside].view(np.int32), y[outside].view(np.int32))  # every other cell keeps its bits
    assert not np.array_equal(_base(first, shape, offset)[m], _base(y, shape, offset)[m])
    assert np.array_equal(first.view(np.int32), second.view(np.int32))  # two calls, equal bits


@pytest.mark.gpu
def test_set_bodies_replaces_centres_and_k():
    """a coupling made kinematic adds exactly nothing; given the tables afterwards it is the coupling made with them, bit for bit"""
    import geometricmultigridpressuresolver_amd as G

    c = random_case(SMALL, 3)
    eshape, offset, _ = G.expanded_layout(SMALL, 0, power_of_two=False)
    rng = np.random.default_rng(79)
    x, y = rng.standard_normal(eshape).astype(np.float32), rng.standard_normal(eshape).astype(np.float32)
    made, late = _coupling(c, eshape, offset), _coupling(dict(c, centres=c["centres"] + 1.5), eshape, offset, kinematic=True)
    try:
        assert np.array_equal(late.apply(_dev(y), _dev(x)).cpu().numpy().view(np.int32), y.view(np.int32))
        late.set_bodies(c["centres"], c["inv_mass"], c["inv_inertia"])
        a, b = made.apply(_dev(y), _dev(x)).cpu().numpy(), late.apply(_dev(y), _dev(x)).cpu().numpy()
        va, vb = made.velocities(_dev(x), np.ones((4, 6))), late.velocities(_dev(x), np.ones((4, 6)))
    finally:
        made.close()
        late.close()
    assert not np.array_equal(a, y) and np.array_equal(a.view(np.int32), b.view(np.int32))
    assert np.array_equal(va[0], vb[0]) and np.array_equal(va[1], vb[1]) and np.abs(va[0][1:] - 1).min() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("bodies", [1, 3, 255])
@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=["24x16x40", "45x113x131"])
def test_impulses_are_the_rows_of_solid_forces(shape, bodies):
    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import fields as F

    sc, material = cut_scene(shape)
    if bodies == 255:
        rng = np.random.default_rng(455)
        c = dict(material=material, cut_weights=sc["cut_weights"], body=[rng.integers(-1, bodies + 2, size=R.face_shape(shape, a)).astype(np.int32) for a in range(3)],
                 centres=rng.random((bodies + 1, 3)) * np.array([shape[2], shape[1], shape[0]]), inv_mass=np.ones(bodies + 1), inv_inertia=np.ones((bodies + 1, 6)))
    else:
        c = random_case(shape, bodies)
    eshape, offset, _ = G.expanded_layout(shape, 0, power_of_two=False)
    rng = np.random.default_rng(78)
    x = rng.standard_normal(eshape).astype(np.float32)
    pressure = np.ascontiguousarray(_base(x, shape, offset))
    cpl = _coupling(c, eshape, offset)
    try:
        got, again = cpl.impulses(_dev(x)), cpl.impulses(_dev(x))
    finally:
        cpl.close()
    rows = F.solidForces(_dev(pressure), _dev(material), [_dev(a) for a in sc["cut_weights"]], [_dev(b) for b in c["body"]], c["centres"], 1.0)
    _, mag = R.solid_forces(pressure, material, sc["cut_weights"], c["body"], c["centres"], 1.0)
    err = np.abs(got[1:] - rows[1:, :6]) / np.maximum(mag[1:, :6], 1e-300)
    print(f"impulses {shape} bodies {bodies}: worst |difference| / magnitude against solidForces {err.max():.2e} (bound 1e-10)")
    assert np.array_equal(got[0], np.zeros(6)) and np.abs(rows[1:, :6]).max() > 1 and err.max() <= 1e-10
    assert np.array_equal(got, again)


def _solver(c, fp64_vectors=None, **opts):
    import geometricmultigridpressuresolver_amd as G

    opt = G.default_options()
    if fp64_vectors is not None:
        opt.pcg_fp64_vectors = fp64_vectors
    for k, v in opts.items():
        setattr(opt, k, v)
    return G.GeometricMultigridPoissonSolver(c["labels"], c["w32"], c["levels"], False, options=opt)


def _device_rhs(c):
    """b = buildRHS(u, sv = rigidVelocity(V*)) on the device: b_fluid + G V* in one pass"""
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    sv = [torch.zeros(R.face_shape(c["shape"], a), dtype=torch.float32, device="cuda") for a in range(3)]
    F.rigidVelocity(sv, [_dev(b) for b in c["body"]], c["centres"], c["motions"])
    return F.buildRHS(_dev(c["material"]), [_dev(a) for a in c["velocity"]], [_dev(a) for a in c["cut_weights"]], c["eshape"], c["offset"], sv)


@pytest.mark.gpu
@pytest.mark.parametrize("use_mg", [True, False], ids=["mg", "diagonal"])
@pytest.mark.parametrize("name", ["box-in-3", "voxel-2"])
def test_kinematic_limit_is_the_uncoupled_fp64_vector_solve(name, use_mg):
    import torch

    c = solve_case(name, True)
    b = _device_rhs(c)
    plain, coupled = _solver(c, 1), _solver(c, 0)  # (the coupled call runs the fp64-vector loop whatever the option says)
    cpl = _coupling(c, c["eshape"], c["offset"], kinematic=True)
    try:
        x0, x1 = torch.zeros_like(b), torch.zeros_like(b)
        st0 = plain.solveGeometricConjugateGradient(x0, b, TOL, 2500, use_mg)
        st1 = coupled.solve_pcg_coupled(cpl, x1, b, TOL, 2500, use_mg)
        assert cpl.cells() > 300
    finally:
        cpl.close()
        plain.close()
        coupled.close()
    print(f"kinematic {name} mg={use_mg}: {st0['iterations']} / {st1['iterations']} iterations, rel_residual {st0['rel_residual']:.3e} / {st1['rel_residual']:.3e}")
    assert st0["outcome"] == st1["outcome"] == "converged" and st0["iterations"] == st1["iterations"] > 3
    assert st0["rel_residual"] == st1["rel_residual"] and st0["rel_residual_recomputed"] == st1["rel_residual_recomputed"]
    assert np.array_equal(x0.cpu().numpy(), x1.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("use_mg", [True, False], ids=["mg", "diagonal"])
@pytest.mark.parametrize("p2", [False, True], ids=["tight", "power-of-two"])
@pytest.mark.parametrize("name", list(SOLVE_SCENES))
def test_coupled_solve_matches_the_direct_solve(name, p2, use_mg):
    import torch

    c = solve_case(name, p2)
    ref, bodies = c["ref"], c["bodies"]
    b = _device_rhs(c)
    s = _solver(c, 1)
    cpl = _coupling(c, c["eshape"], c["offset"])
    try:
        x0, x = torch.zeros_like(b), torch.zeros_like(b)
        st0 = s.solveGeometricConjugateGradient(x0, b, TOL, 2500, use_mg)  # the parent commit's path, bodies kinematic
        st = s.solve_pcg_coupled(cpl, x, b, TOL, 2500, use_mg)
        v_out, impulses = cpl.velocities(x, c["motions"])
    finally:
        cpl.close()
        s.close()
    e_b = rel_l2(ref.unknowns(b.cpu().numpy()), c["b"])
    e0, e = rel_l2(ref.unknowns(x0.cpu().numpy()), c["p0"]), rel_l2(ref.unknowns(x.cpu().numpy()), c["p"])
    size = np.abs(c["v_out"]).sum()
    e_v = np.abs(v_out - c["v_out"]).sum() / size
    p_dev = ref.unknowns(x.cpu().numpy())
    K = RC.stiffness(c["inv_mass"], c["inv_inertia"])
    host = RC.table(RC.flat(c["motions"]) - K @ (ref.G.T @ p_dev))
    e_host = np.abs(v_out - host).sum() / size
    print(f"coupled solve {name} p2={p2} mg={use_mg}: pressure error {e:.3e} against e0 = {e0:.3e} (bound 4 e0), rhs error {e_b:.2e}, "
          f"V_out error {e_v:.3e}, V_out against the host's from the device's p {e_host:.2e} (bound 1e-10), "
          f"iterations {st['iterations']} against {st0['iterations']} kinematic (bound +{6 * bodies + 2}), "
          f"|V_out - V*| / |V*| = {np.abs(c['v_out'] - c['motions']).sum() / np.abs(c['motions']).sum():.2f}")
    assert st0["outcome"] == st["outcome"] == "converged"
    assert e <= 4 * e0
    assert e_v <= 4 * e0 and e_host <= 1e-10
    assert np.abs(impulses + RC.table(ref.G.T @ p_dev)).sum() <= 1e-10 * np.abs(impulses).sum()
    assert st["iterations"] <= st0["iterations"] + 6 * bodies + 2


def _projection(c, coupled):
    """the device pipeline on the scene's fields; coupled: project_free_surface_rigid, else the same passes around mgps_solve_pcg
    under pcg_fp64_vectors = 1 with sv = rigidVelocity(V*) (the bodies kinematic).  Returns (divergence against the body motions
    the solve ends with, divergence against V*, info)"""
    import torch

    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import fields as F

    shape = c["shape"]
    phi, solid, cw = _dev(c["liquid_phi"]), _dev(c["solid_phi"]), [_dev(a) for a in c["cut_weights"]]
    vel, body = [_dev(a) for a in c["velocity"]], [_dev(b) for b in c["body"]]
    pressure = torch.zeros(shape, dtype=torch.float32, device="cuda")
    opt = G.default_options()
    opt.pcg_fp64_vectors = 1
    zeros = lambda: [torch.zeros(R.face_shape(shape, a), dtype=torch.float32, device="cuda") for a in range(3)]  # noqa: E731
    sv_star = F.rigidVelocity(zeros(), body, c["centres"], c["motions"])
    if coupled:
        out = F.project_free_surface_rigid(phi, solid, cw, vel, pressure, body, c["centres"], c["inv_mass"], c["inv_inertia"], c["motions"],
                                           use_old_pressure=False, use_gauss_seidel=False, tolerance=TOL, power_of_two=True, options=opt)
        material, motions = out["material"], out["motions"]
        for a in range(3):
            assert torch.equal(out["solid_velocity"][a], sv_star[a])
    else:
        material = F.buildMaterialCellLabels(phi, solid, cw)
        valid = F.buildValidFaces(material, cw)
        eshape, offset, levels = G.expanded_layout(shape, 0, power_of_two=True)
        labels, weights = F.buildMGDomain(material, cw, phi, valid, eshape, offset)
        rhs = F.buildRHS(material, vel, cw, eshape, offset, sv_star)
        s = G.GeometricMultigridPoissonSolver(labels, weights, levels, False, options=opt)
        try:
            x = torch.zeros_like(rhs)
            out = {"stats": s.solveGeometricConjugateGradient(x, rhs, TOL, 2500, True)}
        finally:
            s.close()
        F.applySolutionToPressure(pressure, x, material, offset)
        F.applyPressureGradient(vel, phi, pressure, valid, material)
        motions = c["motions"]
    sv_end = F.rigidVelocity(zeros(), body, c["centres"], motions)
    return F.computeResultingDivergence(material, vel, cw, sv_end)[1], F.computeResultingDivergence(material, vel, cw, sv_star)[1], out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box-in-2", "voxel-1"])
def test_projection_with_rigid_bodies_is_divergence_free_against_v_out(name):
    c = solve_case(name, True)
    kin, _, info0 = _projection(c, False)
    end, star, info = _projection(c, True)
    print(f"project_free_surface_rigid {name}: max divergence {end:.3e} against rigidVelocity(V_out), {kin:.3e} left by the kinematic projection "
          f"(bound 4 x), {star:.3e} against rigidVelocity(V*) ({star / end:.0f} x); iterations {info['stats']['iterations']} / {info0['stats']['iterations']}")
    assert info["stats"]["outcome"] == "converged" and info["coupled_cells"] > 300
    assert end <= 4 * kin
    assert star > 100 * end
    assert np.abs(info["motions"] - c["v_out"]).sum() <= 1e-4 * np.abs(c["v_out"]).sum()  # (the fields layer's own labels and weights: the same scene)


class _SoloComm:
    """a transport of one rank: nothing to exchange, reductions of one value, gathers that copy"""

    def __init__(self):
        from geometricmultigridpressuresolver_amd import distributed as Dd

        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

        def copy(dst, src, n):
            return 0 if not n or hip.hipMemcpy(dst, src, n, 4) == 0 else 1

        self.rank, self.size = 0, 1
        self._cb = (Dd._EXCH(lambda *a: 0), Dd._ALLR(lambda *a: 0), Dd._GATH(lambda u, s, r, n, root, st: copy(r, s, n)),
                    Dd._GATH(lambda u, s, r, n, root, st: copy(r, s, n)))
        self._cbv = (Dd._GATHV(lambda u, s, n, r, counts, displs, root, st: copy(r + displs[0], s, n)),
                     Dd._SCATV(lambda u, s, counts, displs, r, n, root, st: copy(r, s + displs[0], n)), Dd._ALLRD(lambda *a: 0), Dd._EXCH2(lambda *a: 0))
        self.struct = Dd.CommStruct(C.sizeof(Dd.CommStruct), 0, 1, None, *self._cb, Dd._DEST(), *self._cbv)


@pytest.mark.gpu
def test_refusals_on_the_device():
    import torch

    import geometricmultigridpressuresolver_amd as G
    from conftest import make_domain
    from geometricmultigridpressuresolver_amd.distributed import SlabSolver

    c = solve_case("box-in-2", False)
    b = _device_rhs(c)
    x = torch.zeros_like(b)
    cpl = _coupling(c, c["eshape"], c["offset"])
    other = solve_case("box-in-2", True)
    assert other["eshape"] != c["eshape"]
    wrong = _coupling(other, other["eshape"], other["offset"])
    mixed = _solver(c, None, precision=1)
    plain = _solver(c)
    lab, w, off, lev, dx = make_domain("simple", 40, 4, (64, 64, 64))
    opt = G.default_options()
    opt.min_cells_per_rank = 0
    slab = SlabSolver(lab, [_dev(a.astype(np.float32)) for a in w], lev, False, _SoloComm(), device=0, options=opt)
    try:
        for s, words in ((mixed, ("precision",)), (slab, ("slab solver",))):
            with pytest.raises(G.MgpsError) as err:
                s.solve_pcg_coupled(cpl, s.new_grid(), s.new_grid(), TOL, 10, True)
            assert err.value.status == 1 and all(wd in str(err.value) for wd in words), str(err.value)
        with pytest.raises(G.MgpsError) as err:
            plain.solve_pcg_coupled(wrong, x, b, TOL, 10, True)
        assert err.value.status == 1 and "extents" in str(err.value), str(err.value)
        assert float(x.abs().max()) == 0.0  # refused before any device work
        st = plain.solve_pcg_coupled(cpl, x, b, 1e-3, 100, True)  # and the solver is as good as new afterwards
        assert st["outcome"] == "converged"
    finally:
        for o in (cpl, wrong, mixed, plain, slab):
            o.close()


@pytest.mark.gpu
def test_enclosed_component_is_refused():
    """a sealed tank under options.enclosed_liquid: a moving body changes the null space; out of scope, so refused"""
    import torch

    import geometricmultigridpressuresolver_amd as G

    c = solve_case("box-in-2", False)
    lab = np.where(c["labels"] == G.domains.DIRICHLET, G.domains.EXTERIOR, c["labels"]).astype(np.uint8)  # no air: nothing open
    opt = G.default_options()
    opt.enclosed_liquid = 1
    s = G.GeometricMultigridPoissonSolver(lab, c["w32"], c["levels"], False, options=opt)
    cpl = _coupling(c, c["eshape"], c["offset"])
    try:
        assert s.enclosed_components()[0] >= 1
        with pytest.raises(G.MgpsError) as err:
            s.solve_pcg_coupled(cpl, s.new_grid(), s.new_grid(), TOL, 10, True)
        assert err.value.status == 1 and "enclosed" in str(err.value)
    finally:
        cpl.close()
        s.close()


@pytest.mark.gpu
def test_interrupt_inside_the_loop_hands_back_the_iterate():
    import torch

    import geometricmultigridpressuresolver_amd as G
    from test_pcg_exits import INTERRUPTED, UNREACHABLE, Poller, poll_site

    c = solve_case("box-in-3", True)
    b = _device_rhs(c)
    poller = Poller()
    opt = poller.install(G.default_options())
    s = G.GeometricMultigridPoissonSolver(c["labels"], c["w32"], c["levels"], False, options=opt)
    cpl = _coupling(c, c["eshape"], c["offset"])
    try:
        levels = s.getMGLevels()
        for poll in (2 * levels - 3 + 2 * (2 * levels - 2), 2 * levels - 3 + 3 * (2 * levels - 2) + 1):  # the top of iteration 2; inside the V-cycle of iteration 3
            it, updates, inside = poll_site(poll, levels)
            poller.arm(poll)
            x = torch.zeros_like(b)
            with pytest.raises(G.MgpsError) as err:
                s.solve_pcg_coupled(cpl, x, b, UNREACHABLE, 200, True)
            assert err.value.status == INTERRUPTED and poller.polls == poll + 1
            assert err.value.stats["outcome"] == "max_iterations" and err.value.stats["iterations"] == it, (err.value.stats, it, updates, inside)
            poller.arm(None)
            xt = torch.zeros_like(b)
            st = s.solve_pcg_coupled(cpl, xt, b, UNREACHABLE, updates, True)
            assert st["outcome"] == "max_iterations" and st["iterations"] == updates
            worst = int(_ulps(x.cpu().numpy(), xt.cpu().numpy()).max())
            print(f"interrupt at poll {poll} (iteration {it}, inside a V-cycle: {inside}): {updates} updates, {worst} ulp from the truncated solve")
            assert worst <= 1 and float(x.abs().max()) > 0
            assert err.value.stats["rel_residual"] == pytest.approx(st["rel_residual"], rel=1e-9)
    finally:
        cpl.close()
        s.close()
