"""Pressure force and torque on solid bodies (include/mgps_fields.h).

CPU: the numpy restatement (tests/solid_forces_reference.py) satisfies the adjoint identity against a restatement of the solid part of
the right-hand side, gives the buoyancy of a voxel box in hydrostatic liquid, and its force total does not depend on the ids; the C
ABI refuses bad arguments on the host.  GPU: mgps_fields_solid_forces against the restatement, twice for equal bits, the adjoint
identity through the device's own buildRHS, and the window passes summed against the whole-grid call.

Tolerances.  Columns 0-6 against the restatement: 1e-10 * sum |term| per row and column -- fewer than 1e5 terms per row at these
sizes (asserted) bound the error of a reordered fp64 sum by n * 2^-53 = 1.1e-11 of that magnitude; the margin over it is ten.  Column 7 (a
count) exactly.  The adjoint identity through buildRHS: 2e-6 * sum |p| s |sv| -- six float32 operations per cell of the rhs at 6e-8
each, with a margin of five."""
import ctypes as C
import functools

import numpy as np
import pytest

import solid_forces_reference as R
from refusals import refused as _refused

# (gz, gy, gx).  The second: a row longer than one 256-thread block, face rows of 261.  The third, odd in every extent, has 666 135
# cells, 2.5 times the 262 144 threads of the pass's fixed launch: threads take a second and a third trip through the walk, and the
# second (from plane 17.7 on) holds the top of the solid box (planes 8 .. 19, with its fractional z-faces), the walls and the free
# surface -- the stride's digits, both carries, the look-ahead weights and tables added into over several trips run under every check.
SHAPES = [(24, 16, 40), (6, 5, 260), (45, 113, 131)]
IDS = ["24x16x40", "6x5x260", "45x113x131"]
WALK_THREADS = 1024 * 256  # kForceBlocks * kForceThreads of csrc/mgps_fields.hip
# the base planes of tests/test_fields_windows.py; of the third grid the window [1, 44) alone is walked in three trips
WINDOW_CUTS = {(24, 16, 40): (1, 7, 13, 14), (6, 5, 260): (2, 3), (45, 113, 131): (1, 44)}
SCALE = 0.37


@functools.lru_cache(maxsize=None)
def scene(shape):
    """projection_scene with the oracle's material labels (the device passes are held to them in tests/test_fields.py) and a
    pressure that is random on LIQUID cells and junk elsewhere (the definition masks it)"""
    from geometricmultigridpressuresolver_amd import domains as D
    from oracle.mg_oracle import FieldsOracle

    sc = D.projection_scene(shape, with_solid_velocity=True)
    material = FieldsOracle().material_labels(sc["liquid_phi"], sc["solid_phi"], sc["cut_weights"]).astype(np.int32)
    rng = np.random.default_rng(16)
    pressure = (rng.random(shape) * 2 - 0.5).astype(np.float32)
    pressure[material != R.LIQUID] = np.float32(1e3)
    return sc, material, pressure


@functools.lru_cache(maxsize=None)
def case(shape, bodies):
    """ids drawn from -1 .. bodies + 1 (both kinds of out-of-range id), random centres inside the grid, and the restatement"""
    sc, material, pressure = scene(shape)
    rng = np.random.default_rng(100 + bodies)
    body = [rng.integers(-1, bodies + 2, size=R.face_shape(shape, a)).astype(np.int32) for a in range(3)]
    centres = rng.random((bodies + 1, 3)) * np.array([shape[2], shape[1], shape[0]])
    rows, mag = R.solid_forces(pressure, material, sc["cut_weights"], body, centres, SCALE)
    return body, centres, rows, mag


def assert_rows(what, got, rows, mag):
    err = np.abs(got[:, :7] - rows[:, :7])
    lim = 1e-10 * mag[:, :7]
    worst = float((err / np.maximum(mag[:, :7], 1e-300)).max())
    print(f"{what}: worst |error| / sum |term| = {worst:.2e} (bound 1e-10), wet faces {int(rows[:, 7].sum())}")
    assert rows[:, 7].max() < 1e5, what  # (what the bound is derived for)
    assert (err <= lim).all(), (what, worst)
    assert np.array_equal(got[:, 7], rows[:, 7]), what


# ---- CPU: the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_satisfies_the_adjoint_identity():
    shape, bodies = (24, 16, 40), 3
    sc, material, pressure = scene(shape)
    rng = np.random.default_rng(3)
    body = [rng.integers(-1, bodies + 2, size=R.face_shape(shape, a)).astype(np.int32) for a in range(3)]
    centres = rng.random((bodies + 1, 3)) * np.array([shape[2], shape[1], shape[0]])
    linear, angular = rng.standard_normal((bodies + 1, 3)), 0.1 * rng.standard_normal((bodies + 1, 3))
    sv = R.rigid_velocity(shape, body, centres, linear, angular, bodies)
    rows, _ = R.solid_forces(pressure, material, sc["cut_weights"], body, centres, 1.0)
    assert rows[:, 7].min() > 50, rows[:, 7]  # every row, row 0 included, owns wet faces
    p = np.where(material == R.LIQUID, pressure.astype(np.float64), 0.0)
    lhs = float((p * R.solid_rhs(material, sv, sc["cut_weights"])).sum())
    rhs = -float((linear * rows[:, 0:3]).sum() + (angular * rows[:, 3:6]).sum())
    size = R.power_magnitude(pressure, material, sc["cut_weights"], sv)
    print(f"adjoint identity in fp64: {lhs:.12e} against {rhs:.12e}, difference / magnitude {abs(lhs - rhs) / size:.2e}")
    assert size > 0 and abs(lhs) > 1e-3 * size and abs(lhs - rhs) <= 1e-12 * size


def test_hydrostatic_voxel_box_gets_the_buoyancy_of_its_height_plus_one():
    """weights 0 or 1, p = g (H - k - 1/2): the cell-centred pressure sits half a cell off the top and the bottom face, so a box of
    n_z cells is lifted like n_z + 1"""
    shape, g = (12, 10, 11), 0.25
    lo, n = (3, 2, 4), (4, 5, 3)  # the box: first cell and cell counts along x, y, z
    material = np.full(shape, R.LIQUID, dtype=np.int32)
    material[lo[2]:lo[2] + n[2], lo[1]:lo[1] + n[1], lo[0]:lo[0] + n[0]] = 0
    solid = material == 0
    k = np.arange(shape[0], dtype=np.float64)[:, None, None]
    pressure = np.where(solid, 7.0, g * (shape[0] - k - 0.5)).astype(np.float32)
    cw, body = [], []
    for a in range(3):
        behind, front = R._behind_front(solid, a, False)
        closed = behind | front
        cw.append(np.where(closed, 0.0, 1.0).astype(np.float32))  # (the grid's own walls stay open: only the box is closed)
        body.append(closed.astype(np.int32))
    centre = [lo[c] + n[c] / 2 for c in range(3)]
    rows, _ = R.solid_forces(pressure, material, cw, body, np.array([[0.0, 0.0, 0.0], centre]))
    wet = 2 * (n[0] * n[1] + n[1] * n[2] + n[0] * n[2])
    assert np.array_equal(rows[0], np.zeros(8))
    assert rows[1, 0] == 0 and rows[1, 1] == 0 and rows[1, 2] == g * n[0] * n[1] * (n[2] + 1), rows[1]
    assert np.abs(rows[1, 3:6]).max() <= 1e-12 * g * shape[0] * wet, rows[1]
    assert rows[1, 6] == wet and rows[1, 7] == wet, rows[1]


def test_force_total_does_not_depend_on_the_ids():
    shape, bodies = (24, 16, 40), 3
    sc, material, pressure = scene(shape)
    body, centres, rows, mag = case(shape, bodies)
    rng = np.random.default_rng(9)
    permuted = [rng.permutation(b.reshape(-1)).reshape(b.shape) for b in body]
    outside = [np.where(b == 2, 1000, b).astype(np.int32) for b in body]
    nobody = [np.zeros_like(b) for b in body]
    for what, ids in (("permuted", permuted), ("pushed out of range", outside), ("all unowned", nobody)):
        other, other_mag = R.solid_forces(pressure, material, sc["cut_weights"], ids, centres, SCALE)
        assert not np.array_equal(other[:, :3], rows[:, :3]), what
        assert np.abs(other[:, :3].sum(0) - rows[:, :3].sum(0)).max() <= 1e-12 * mag[:, :3].sum(), what
        assert other[:, 6].sum() == pytest.approx(rows[:, 6].sum(), rel=1e-13) and other[:, 7].sum() == rows[:, 7].sum(), what
    assert R.solid_forces(pressure, material, sc["cut_weights"], outside, centres, SCALE)[0][2, 7] == 0


# ---- CPU: the C ABI refuses bad arguments on the host, before any device work -------------------------------------------------------
def test_argument_refusals_need_no_device():
    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd._lib import lib

    p = C.c_void_p(64)  # (never dereferenced: every call below is refused on the host)
    one = lib().mgps_fields_solid_forces
    good, one_scale = [p] * 10, C.c_double(1.0)
    for bodies in (0, 256, -1):
        _refused(one(*good, bodies, one_scale, 4, 4, 4, None), "mgps_fields_solid_forces", "bodies", "1 .. 255")
    for g in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        _refused(one(*good, 3, one_scale, *g, None), "extent")
    for at, word in enumerate(("out_host", "pressure", "material", "cut weights", "cut weights", "cut weights", "body", "body", "body", "centres")):
        args = list(good)
        args[at] = None
        _refused(one(*args, 3, one_scale, 4, 4, 4, None), "mgps_fields_solid_forces", word)
    # the window pass: rank 1 of 2 has a plane below it
    slab = lib().mgps_fields_slab_solid_forces
    d = F.slab_window((96, 64, 64), True, [0, 64, 128], 1)
    assert d.c0 > 0
    p3, two = (C.c_void_p * 3)(64, 64, 64), (C.c_void_p * 3)(64, None, 64)

    def window(**over):
        a = dict(d=C.byref(d), out=p, pressure=p, pressure_lo=p, material=p, material_lo=p, cw=p3, body=p3, centres=p, bodies=3)
        a.update(over)
        return slab(a["d"], a["out"], a["pressure"], a["pressure_lo"], a["material"], a["material_lo"], a["cw"], a["body"], a["centres"], a["bodies"], one_scale, None)

    _refused(window(bodies=256), "mgps_fields_slab_solid_forces", "bodies")
    _refused(window(out=None), "out_host")
    _refused(window(pressure=None), "pressure")
    _refused(window(material=None), "material")
    _refused(window(cw=two), "cut_weights")
    _refused(window(cw=None), "cut_weights")
    _refused(window(body=two), "body")
    _refused(window(centres=None), "centres")
    _refused(window(pressure_lo=None), "pressure_lo", "c0 > 0")
    _refused(window(material_lo=None), "material_lo", "c0 > 0")
    bad = F.slab_window((96, 64, 64), True, [0, 64, 128], 1)
    bad.c0 += 1  # (not what mgps_fields_slab_describe produces)
    _refused(window(d=C.byref(bad)), "not a slab window")
    bad = F.slab_window((96, 64, 64), True, [0, 64, 128], 1)
    bad.struct_size -= 4
    _refused(window(d=C.byref(bad)), "struct_size")


def _comm_of_one():
    from geometricmultigridpressuresolver_amd.distributed import CommStruct

    comm = CommStruct()
    comm.struct_size, comm.size = C.sizeof(CommStruct), 1
    keep = [type(comm.exchange)(lambda *a: 1), type(comm.allreduce)(lambda *a: 1)]  # (a complete vtable; never called: a world of one)
    comm.exchange, comm.allreduce = keep
    return comm, keep


def test_collective_refuses_on_the_host_and_the_mirror_has_the_library_size():
    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd._lib import lib

    call = lib().mgps_solid_forces_slab
    comm, keep = _comm_of_one()
    cuts = (C.c_int * 2)(0, 128)
    sf = F.SolidForcesSlab()
    sf.struct_size = C.sizeof(F.SolidForcesSlab)
    sf.gx, sf.gy, sf.gz, sf.power_of_two, sf.bodies = 64, 64, 96, 1, 0
    # the mirror's size is the library's: the call gets as far as the next check; a mirror of another size is refused as such
    _refused(call(C.byref(sf), C.byref(comm), cuts, None), "mgps_solid_forces_slab", "bodies", "1 .. 255")
    sf.struct_size -= 8
    _refused(call(C.byref(sf), C.byref(comm), cuts, None), "struct_size")
    sf.struct_size += 8
    sf.bodies = 256
    _refused(call(C.byref(sf), C.byref(comm), cuts, None), "bodies")
    sf.bodies, sf.gy = 3, 0
    _refused(call(C.byref(sf), C.byref(comm), cuts, None), "extent")
    sf.gy = 64
    _refused(call(C.byref(sf), None, cuts, None), "comm")
    _refused(call(C.byref(sf), C.byref(comm), None, None), "comm")
    _refused(call(C.byref(sf), C.byref(comm), (C.c_int * 2)(0, 96), None), "mgps_fields_slab_describe")
    _refused(call(C.byref(sf), C.byref(comm), cuts, None), "pressure")  # (all NULL)
    sf.pressure = 64
    _refused(call(C.byref(sf), C.byref(comm), cuts, None), "liquid_phi")
    sf.liquid_phi = sf.solid_phi = 64
    _refused(call(C.byref(sf), C.byref(comm), cuts, None), "cut_weights")
    for a in range(3):
        sf.cut_weights[a] = 64
    sf.body[0] = sf.body[2] = 64
    _refused(call(C.byref(sf), C.byref(comm), cuts, None), "body")
    sf.body[1] = 64
    _refused(call(C.byref(sf), C.byref(comm), cuts, None), "centres")
    sf.centres = 64
    _refused(call(C.byref(sf), C.byref(comm), cuts, None), "out is NULL")


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _whole_grid(shape, bodies, scale=SCALE, body=None, centres=None):
    from geometricmultigridpressuresolver_amd import fields as F

    sc, material, pressure = scene(shape)
    if body is None:
        body, centres = case(shape, bodies)[:2]
    return F.solidForces(_dev(pressure), _dev(material), [_dev(a) for a in sc["cut_weights"]], [_dev(b) for b in body], centres, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("bodies", [1, 3, 255])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_whole_grid_matches_restatement(shape, bodies):
    body, centres, rows, mag = case(shape, bodies)
    assert rows[:, 7].sum() > 300 and (rows[:, 7] > 0).sum() >= min(bodies + 1, 100), rows[:, 7]  # non-vacuity: wet faces, spread over the rows
    if shape == SHAPES[2]:  # non-vacuity of the later trips: wet faces, cut ones among them, behind the first 262 144 cells
        sc, material, pressure = scene(shape)
        first = -(-WALK_THREADS // (shape[1] * shape[2]))  # the first plane that lies in the second trip as a whole
        later = R.solid_forces(pressure, material, sc["cut_weights"], body, centres, SCALE, planes=(first, shape[0]))[0]
        assert later[:, 7].sum() > 3000 and (later[:, 6] < later[:, 7]).any(), later[:, 6:]
    assert_rows(f"whole grid {shape} bodies {bodies}", _whole_grid(shape, bodies), rows, mag)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_two_calls_give_equal_bits(shape):
    assert (int(np.prod(shape)) > WALK_THREADS) == (shape == SHAPES[2])  # the third grid, and only it, is walked in more than one trip
    for bodies in (3, 255):
        first, second = _whole_grid(shape, bodies), _whole_grid(shape, bodies)
        assert np.abs(first[:, :6]).max() > 0 and np.array_equal(first, second), (shape, bodies)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_adjoint_identity_through_the_device_rhs(shape):
    """zero fluid velocity, a rigid motion per row: sum p rhs over the LIQUID cells of the device's buildRHS against
    -sum (U . F + omega . T) of the device's forces at scale 1"""
    import torch

    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import fields as F

    bodies = 3
    sc, material, pressure = scene(shape)
    body, centres = case(shape, bodies)[:2]
    rng = np.random.default_rng(12)
    linear, angular = rng.standard_normal((bodies + 1, 3)), 0.1 * rng.standard_normal((bodies + 1, 3))
    sv = [a.astype(np.float32) for a in R.rigid_velocity(shape, body, centres, linear, angular, bodies)]
    eshape, offset, _ = G.expanded_layout(shape, 0, power_of_two=False)
    cw = [_dev(a) for a in sc["cut_weights"]]
    zero = [torch.zeros(R.face_shape(shape, a), dtype=torch.float32, device="cuda") for a in range(3)]
    rhs = F.buildRHS(_dev(material), zero, cw, eshape, offset, [_dev(a) for a in sv]).cpu().numpy()
    rhs = rhs[offset:offset + shape[0], offset:offset + shape[1], offset:offset + shape[2]].astype(np.float64)
    p = np.where(material == R.LIQUID, pressure.astype(np.float64), 0.0)
    lhs = float((p * rhs).sum())
    rows = _whole_grid(shape, bodies, 1.0)
    power = -float((linear * rows[:, 0:3]).sum() + (angular * rows[:, 3:6]).sum())
    size = R.power_magnitude(pressure, material, sc["cut_weights"], sv)
    print(f"adjoint identity {shape}: sum p rhs = {lhs:.9e}, -sum (U.F + w.T) = {power:.9e}, difference / magnitude {abs(lhs - power) / size:.2e} (bound 2e-6)")
    assert abs(lhs) > 1e-3 * size and abs(lhs - power) <= 2e-6 * size


@pytest.mark.gpu
@pytest.mark.parametrize("p2", [False, True], ids=["tight", "power-of-two"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_windows_sum_to_the_whole_grid(shape, p2):
    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import fields as F
    from slab_slices import cell, dev, faces, halo

    bodies, cuts = 3, WINDOW_CUTS[shape]
    sc, material, pressure = scene(shape)
    body, centres, rows, mag = case(shape, bodies)
    whole = _whole_grid(shape, bodies)
    eshape, offset, _ = G.expanded_layout(shape, 0, power_of_two=p2)
    splits = [0] + [offset + c for c in cuts] + [eshape[0]]
    total = np.zeros_like(whole)
    for rank in range(len(splits) - 1):
        d = F.slab_window(shape, p2, splits, rank)
        got = F.solidForcesSlab(d, dev(cell(pressure, d)), halo(pressure, d)[0], dev(cell(material, d)), halo(material, d)[0],
                                [dev(a) for a in faces(sc["cut_weights"], d)], [dev(a) for a in faces(body, d)], centres, SCALE)
        part, part_mag = R.solid_forces(pressure, material, sc["cut_weights"], body, centres, SCALE, planes=(d.c0, d.c1))
        assert_rows(f"window [{d.c0}, {d.c1}) of {shape}", got, part, part_mag)
        total += got
    assert total[:, 7].sum() > 300
    if shape == SHAPES[2]:  # the window [1, 44) is walked in more than one trip, with wet and cut faces behind its first 262 144 cells
        first = 1 + -(-WALK_THREADS // (shape[1] * shape[2]))
        later = R.solid_forces(pressure, material, sc["cut_weights"], body, centres, SCALE, planes=(first, 44))[0]
        assert later[:, 7].sum() > 3000 and (later[:, 6] < later[:, 7]).any(), later[:, 6:]
    assert (np.abs(total[:, :7] - whole[:, :7]) <= 1e-10 * mag[:, :7]).all() and np.array_equal(total[:, 7], whole[:, 7])
