"""Deforming mesh colliders (include/mgps_fields.h) against tests/mesh_velocity_reference.py.

CPU: the restatement against analysis (linear interpolation of an affine vertex field is exact at the closest point), the condition
that the test scenes are in generic position (no in-band sample with two candidate triangles whose closest points differ), the C
ABI's refusals and the ctypes mirrors' sizes.
GPU: the velocity samples of mgps_fields_mesh_sdf_velocity against the restatement on section 19's five meshes and two grids, rows
across tile edges, an exact tie between two opposite faces, the same bits for any triangle order, turn and run, the face pass
against the restatement fed with the device's own samples, exactness on planes, slab windows against the whole grid, and the
samples as the solid velocity of the projection.

Tolerances.  A sample is one fp64 value rounded to float32: |got - want| <= 2^-24 |want| + 1e-9 max|V| (the rounding, and the
fp64 round-off of the weights with four orders of margin).  A face value is a sum formed in fp64 and rounded once:
2^-24 |want| + 1e-10 sum|terms|, section 17's bound.  Which triangle wins is a decision: the generic-position condition is asserted
on the restatement first, after which any candidate's value is the expected one."""
import ctypes as C
import functools

import numpy as np
import pytest

import mesh_reference as MR
import mesh_velocity_reference as MV
import raster_reference as RR
import test_mesh_bodies as TM
from refusals import refused as _refused

SPACING, BAND, GRIDS = TM.SPACING, TM.BAND, TM.GRIDS
NAMES = ["tetrahedron", "box", "icosphere", "l_prism", "shell"]


def vertex_velocities(mesh, seed=7):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, mesh[0].shape)


@functools.lru_cache(maxsize=None)
def restated(name, n):
    """(vel, d, details) of the restatement for section 19's scene (name, n) with seeded vertex velocities; read-only"""
    mesh = TM.meshes()[name]
    vel, d, details = MV.sample_velocity(*mesh, vertex_velocities(mesh), n, TM.grid_origin(mesh, n), SPACING, BAND)
    vel.setflags(write=False)
    return vel, d, details


# ---- CPU: the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_restated_interpolation_of_an_affine_field_is_the_field_at_the_closest_point(name):
    """V(x) = U + omega x x + S x at the vertices: the interpolated velocity is V(q) at the restatement's own closest point q, to
    1e-12 max|V|; q is a point at the restated distance; sqrt(min d2) is mesh_reference.distance"""
    mesh = TM.meshes()[name]
    v = mesh[0]
    U, omega = np.array([0.3, -0.2, 0.5]), np.array([0.11, 0.07, -0.05])
    S = np.array([[0.21, -0.04, 0.02], [0.05, -0.13, 0.03], [-0.06, 0.01, 0.08]])
    field = lambda p: U + np.cross(omega, p) + p @ S.T  # noqa: E731
    V = field(v)
    n = GRIDS[0]
    origin = TM.grid_origin(mesh, n)
    vel, d, details = MV.sample_velocity(*mesh, V, n, origin, SPACING, BAND)
    x, y, z = MR.sample_points(n, origin, SPACING)
    q = np.moveaxis(details["point"], 0, -1)
    inband = d < BAND
    want = np.moveaxis(field(q.reshape(-1, 3)).reshape(q.shape), -1, 0)
    err = np.abs(vel - want)[:, inband].max()
    gap = np.abs(np.sqrt((x - q[..., 0]) ** 2 + (y - q[..., 1]) ** 2 + (z - q[..., 2]) ** 2) - d).max()
    print(f"{name}: interpolated - V(q) {err:.2e} of max|V| = {np.abs(V).max():.2f}; | |s - q| - d | {gap:.2e}; {int(inband.sum())} samples in band")
    assert inband.sum() > 500 and (vel[:, ~inband] == 0).all()
    assert err <= 1e-12 * np.abs(V).max()
    assert gap <= 1e-12 * max(1.0, d.max())
    assert np.abs(d - MR.distance(*mesh, x, y, z)).max() <= 1e-12
    w = MV._pick(details["weights"], details["winner"])
    assert np.abs(w.sum(axis=0) - 1).max() <= 1e-12 and w.min() >= -1e-12


@pytest.mark.parametrize("n", GRIDS)
@pytest.mark.parametrize("name", NAMES)
def test_scenes_are_in_generic_position(name, n):
    """a condition, not a tolerance: no in-band sample has two candidate triangles whose closest points differ; candidates that share
    one point (a vertex's fan, an edge's pair) give one value"""
    _, d, details = restated(name, n)
    print(f"{name} {n}: {details['ambiguous']} ambiguous samples, up to {details['fan']} candidates at one point")
    assert details["ambiguous"] == 0
    assert 1 <= details["fan"] <= 6 and (d < BAND).sum() > 300


def _mesh_desc(mesh=None, velocity=True, **kw):
    from geometricmultigridpressuresolver_amd import fields as F

    v, t = MR.tetrahedron(2.0) if mesh is None else mesh
    v, t = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(t, dtype=np.int32)
    w = np.ascontiguousarray(velocity, dtype=np.float64) if isinstance(velocity, np.ndarray) else np.zeros_like(v)
    d = F.MeshVelocityDesc()
    d.struct_size = C.sizeof(F.MeshVelocityDesc)
    d.vertices, d.triangles, d.xyz, d.tri = len(v), len(t), v.ctypes.data, t.ctypes.data
    d.velocity = w.ctypes.data if velocity is not None else None
    d.nx = d.ny = d.nz = 8
    d.origin[:] = [-2.0, -2.0, -2.0]
    d.spacing, d.band = 0.5, 1.0
    d.sdf = None  # (allowed here)
    for c in range(3):
        d.vel[c] = 64  # (never dereferenced: every call below is refused on the host)
    for k, val in kw.items():
        setattr(d, k, val)
    return d, (v, t, w)


def _face_args(shapes=None, velocities=None):
    from geometricmultigridpressuresolver_amd import fields as F

    if shapes is None:
        grid = F.BodyShape.box((2, 2, 2), (1, 1, 1))
        grid.kind, grid.sdf, grid.nx, grid.ny, grid.nz, grid.spacing = F.BODY_GRID, 64, 4, 4, 4, 0.5
        shapes = [grid, F.BodyShape.sphere((2, 2, 2), 1.0)]
    rows = (F.BodyShape * (len(shapes) + 1))(F.BodyShape(), *shapes)
    vrows = (F.BodyVelocity * (len(shapes) + 1))()
    for c in range(3):
        vrows[1].vel[c] = 64
    if velocities is not None:
        velocities(vrows)
    grids = (C.c_void_p * 3)(64, 64, 64)
    return dict(sv=grids, body=(C.c_void_p * 3)(64, 64, 64), bodies=len(shapes), rows=rows, vrows=vrows)


def test_argument_refusals_need_no_device_and_the_mirrors_have_the_library_size():
    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd._lib import lib

    L = lib()
    fn = "mgps_fields_mesh_sdf_velocity"
    run = lambda d: L.mgps_fields_mesh_sdf_velocity(C.byref(d[0]), None)  # noqa: E731
    assert C.sizeof(F.MeshVelocityDesc) == C.sizeof(F.MeshDesc) + 32 == 128 and C.sizeof(F.BodyVelocity) == 72
    # the mirror's size is the library's: a good struct gets as far as the next check, one of another size is refused as such; the
    # last field is read where the library expects it
    d = _mesh_desc()
    d[0].vel[2] = None
    _refused(run(d), fn, "vel", "three")
    d = _mesh_desc()
    d[0].struct_size -= 4
    _refused(run(d), fn, "struct_size")
    _refused(L.mgps_fields_mesh_sdf_velocity(None, None), "struct_size")
    _refused(run(_mesh_desc(velocity=None)), fn, "velocity", "NULL")
    # whatever mgps_fields_mesh_sdf refuses (a NULL sdf is allowed: the band is the next thing looked at)
    for band in (0.0, float("nan")):
        _refused(run(_mesh_desc(band=band)), fn, "band")
    for name in ("nx", "ny", "nz"):
        _refused(run(_mesh_desc(**{name: 1025})), "dimension", "2 .. 1024")
    _refused(run(_mesh_desc(spacing=0.0)), "spacing")
    d = _mesh_desc()
    d[0].origin[2] = float("inf")
    _refused(run(d), "origin")
    for name in ("xyz", "tri"):
        _refused(run(_mesh_desc(**{name: None})), "NULL")
    _refused(run(_mesh_desc(triangles=3)), "at least 4")
    v, t = MR.box((0, 0, 0), (2, 3, 1))
    _refused(run(_mesh_desc((v, np.delete(t, 0, axis=0)))), fn, "not closed and consistently oriented")
    _refused(run(_mesh_desc(MR.flipped((v, t)))), "orientation")
    t2 = t.copy()
    t2[5, 1] = 8
    _refused(run(_mesh_desc((v, t2))), "triangle 5", "out of range")
    # a non-finite velocity, after the mesh's own faults
    for bad in (float("nan"), float("inf")):
        w = np.zeros_like(v)
        w[6, 1] = bad
        _refused(run(_mesh_desc((v, t), velocity=w)), fn, "non-finite", "velocity")

    # the face pass
    fn = "mgps_fields_sampled_velocity"

    def whole(a, gx=4, gy=4, gz=4):
        return L.mgps_fields_sampled_velocity(a["sv"], a["body"], a["bodies"], a["rows"], a["vrows"], gx, gy, gz, None)

    for k in ("gx", "gy", "gz"):
        _refused(whole(_face_args(), **{k: 0}), fn, "extent")
    # both mirrors have the library's row size: the second row of a good table is read where the library expects it
    bad = F.BodyShape.sphere((2, 2, 2), 1.0)
    bad.kind = 7
    _refused(whole(_face_args([_face_args()["rows"][1], bad])), fn, "body 2", "kind")

    def second_partly(vrows):
        vrows[2].vel[0] = 64

    _refused(whole(_face_args(velocities=second_partly)), "body 2", "vel", "all three")

    def sphere_sampled(vrows):
        for c in range(3):
            vrows[2].vel[c] = 64

    _refused(whole(_face_args(velocities=sphere_sampled)), "body 2", "GRID")

    def partly(vrows):
        vrows[1].vel[1] = None

    _refused(whole(_face_args(velocities=partly)), "body 1", "vel", "all three")

    def motion(vrows):
        vrows[1].motion[4] = float("nan")

    _refused(whole(_face_args(velocities=motion)), "body 1", "motion")
    for bodies in (0, 256, -1):
        a = _face_args()
        a["bodies"] = bodies
        _refused(whole(a), "bodies", "1 .. 255")
    for name in ("sv", "body"):
        a = _face_args()
        a[name][1] = None
        _refused(whole(a), "three grids")
    for name in ("rows", "vrows"):
        a = _face_args()
        a[name] = None
        _refused(whole(a), "NULL")
    # everything the rasteriser refuses of a shape row
    s = F.BodyShape.box((2, 2, 2), (1, 1, 1), [[1, 0, 0], [0, 1, 1e-5], [0, 0, 1]])
    _refused(whole(_face_args([_face_args()["rows"][1], s])), "body 2", "orthonormal")
    grid = _face_args()["rows"][1]
    for name, value, word in (("sdf", None, "sdf"), ("ny", 1, "dimension"), ("spacing", 0.0, "spacing")):
        g2 = F.BodyShape.from_buffer_copy(grid)
        setattr(g2, name, value)
        _refused(whole(_face_args([g2])), "body 1", word)
    g2 = F.BodyShape.from_buffer_copy(grid)
    g2.centre[1] = float("nan")
    _refused(whole(_face_args([g2])), "body 1", "centre")
    # the window entry: the window first, then the same refusals
    slab = lambda w, a: L.mgps_fields_slab_sampled_velocity(C.byref(w) if w is not None else None, a["sv"], a["body"], a["bodies"], a["rows"], a["vrows"], None)  # noqa: E731
    w = F.slab_window((32, 4, 4), True, F.projection_slab_layout((32, 4, 4), True, 2, False)["splits"], 0)
    _refused(slab(None, _face_args()), "mgps_fields_slab_sampled_velocity", "slab window")
    _refused(slab(w, _face_args(velocities=motion)), "mgps_fields_slab_sampled_velocity", "body 1", "motion")
    w.c1 += 1
    _refused(slab(w, _face_args()), "slab window")


# ---- GPU: the samples ------------------------------------------------------------------------------------------------------------------
def assert_samples(got, want, d, band, vmax, what):
    got = got.cpu().numpy().astype(np.float64)
    bound = 2.0 ** -24 * np.abs(want) + 1e-9 * vmax
    err = np.abs(got - want)
    print(f"{what}: worst |got - want| / bound = {(err / bound).max():.3f}, |got - want| <= {err.max():.2e}; {int((d < band).sum())} samples in band, "
          f"{int((d >= band).sum())} beyond")
    assert (got[:, d >= band] == 0).all(), what
    assert (err <= bound).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("n", GRIDS)
@pytest.mark.parametrize("name", NAMES)
def test_device_samples_equal_the_restatement(name, n):
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    mesh = TM.meshes()[name]
    want, d, details = restated(name, n)
    assert details["ambiguous"] == 0 and (n[0] < 64 or (d >= BAND).sum() > 100) and np.abs(want).max() > 0.5
    V = vertex_velocities(mesh)
    origin = TM.grid_origin(mesh, n)
    sdf, vel = F.meshSDFVelocity(*mesh, V, n, origin, SPACING, BAND)
    assert tuple(vel.shape) == (3,) + n[::-1] and vel.dtype == torch.float32
    assert torch.equal(sdf, F.meshSDF(*mesh, n, origin, SPACING, BAND))  # the bits of the distance pass
    assert_samples(vel, want, d, BAND, np.abs(V).max(), f"{name} {n}")


def _check_scene(mesh, n, origin, band, what, seed=3):
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    V = vertex_velocities(mesh, seed)
    want, d, details = MV.sample_velocity(*mesh, V, n, origin, SPACING, band)
    assert details["ambiguous"] == 0, what
    sdf, vel = F.meshSDFVelocity(*mesh, V, n, origin, SPACING, band)
    assert torch.equal(sdf, F.meshSDF(*mesh, n, origin, SPACING, band))
    assert_samples(vel, want, d, band, np.abs(V).max(), what)
    return want, d


@pytest.mark.gpu
@pytest.mark.parametrize("nx", [64, 65, 131])
def test_rows_across_tile_edges(nx):
    """section 19's rows: exactly one tile, a tile and one sample, and three tiles of which the second lies deep inside the mesh (an
    empty list: zero velocity everywhere)"""
    mesh, n, origin = TM.tile_edge_case(nx)
    want, d = _check_scene(mesh, n, origin, BAND, f"nx = {nx}")
    assert nx == 131 or (d[:, :, nx - 1] < BAND).all()
    if nx == 131:
        assert (d[:, :, 64:128] >= BAND).all() and (want[:, :, :, 64:128] == 0).all() and (d[:, :, :64] < BAND).any()


@pytest.mark.gpu
def test_a_mesh_inside_one_tile():
    mesh, n, origin, band = TM.one_tile_case()
    want, d = _check_scene(mesh, n, origin, band, "one tile")
    assert (d[:, :, 64:] >= band).all() and (d[4:] >= band).all() and (d[:, 4:] >= band).all() and (d < band).sum() >= 8


def tie_case(renumber):
    """a box [0, 2] x [0, 8] x [0, 8] sampled at half-integers: on the mid-plane x = 1 the faces x = 0 and x = 2 are equally near, and
    every number involved is exact.  renumber: the vertex numbering reversed, so that the other face holds the smaller triples"""
    v, t = MR.box((0.0, 0.0, 0.0), (2.0, 8.0, 8.0))
    if renumber:
        v, t = v[::-1].copy(), (7 - t).astype(np.int32)
    n, origin, spacing, band = (9, 21, 21), np.array([-1.0, -1.0, -1.0]), 0.5, 1.75
    V = np.random.default_rng(19).uniform(-1.0, 1.0, v.shape)
    return (v, t), V, n, origin, spacing, band


@pytest.mark.gpu
@pytest.mark.parametrize("renumber", [False, True])
def test_an_exact_tie_goes_to_the_smaller_index_triple(renumber):
    from geometricmultigridpressuresolver_amd import fields as F

    mesh, V, n, origin, spacing, band = tie_case(renumber)
    want, d, details = MV.sample_velocity(*mesh, V, n, origin, spacing, band)
    x, y, z = MR.sample_points(n, origin, spacing)
    # the samples of the mid-plane whose closest points lie strictly inside one triangle of each face: nearer to the x-faces than to
    # any other, off the faces' diagonal y = z
    tied = (x == 1.0) & (y > 1.25) & (y < 6.75) & (z > 1.25) & (z < 6.75) & (y != z)
    assert tied.sum() > 50
    tri, d2 = details["triangles"], details["d2"]
    on_face = lambda side: np.array([(mesh[0][row, 0] == side).all() for row in tri])  # noqa: E731
    lo, hi = d2[on_face(0.0)].min(axis=0), d2[on_face(2.0)].min(axis=0)
    assert np.array_equal(lo[tied], hi[tied]) and (lo[tied] == 1.0).all()  # bit-equal, and exact
    # the winner is the candidate with the smaller triple, and the other face's value differs
    win = tri[details["winner"][tied]]
    first = tri[on_face(0.0)][0] if tuple(tri[on_face(0.0)][0]) < tuple(tri[on_face(2.0)][0]) else tri[on_face(2.0)][0]
    side = mesh[0][first[0], 0]
    assert (mesh[0][win[:, 0], 0] == side).all() and side == (2.0 if renumber else 0.0)
    Vswap = V.copy()
    Vswap[mesh[0][:, 0] == side] += 1.0  # (moves the winner's value only where the winning face is the one expected)
    moved = MV.sample_velocity(*mesh, Vswap, n, origin, spacing, band)[0]
    assert np.abs(moved - want)[:, tied].min() > 0.99
    sdf, vel = F.meshSDFVelocity(*mesh, V, n, origin, spacing, band)
    got = vel.cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    print(f"tie (renumber={renumber}): {int(tied.sum())} tied samples, worst |got - want| {err[:, tied].max():.2e} there, {err.max():.2e} anywhere")
    assert (err <= 2.0 ** -24 * np.abs(want) + 1e-9).all()
    assert (sdf.cpu().numpy()[tied] == -1.0).all()


@pytest.mark.gpu
def test_triangle_order_vertex_turns_and_repeats_give_the_same_bits():
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    rng = np.random.default_rng(11)
    for name, n in (("icosphere", GRIDS[1]), ("shell", GRIDS[0])):
        v, t = TM.meshes()[name]
        V = vertex_velocities((v, t))
        origin = TM.grid_origin((v, t), n)
        run = lambda tri: F.meshSDFVelocity(v, tri, V, n, origin, SPACING, BAND)  # noqa: E731
        same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])  # noqa: E731
        first = run(t)
        assert same(first, run(t))
        assert same(first, run(t[rng.permutation(len(t))]))
        for turn in (1, 2):
            assert same(first, run(np.roll(t, turn, axis=1)))
        turns = rng.integers(0, 3, len(t))
        mixed = np.stack([t[np.arange(len(t)), (turns + q) % 3] for q in range(3)], axis=1)
        assert same(first, run(mixed[rng.permutation(len(t))]))
        assert int((first[1] != 0).sum()) > 1000
    # the tie: the order decides nothing there either
    mesh, V, n, origin, spacing, band = tie_case(False)
    first = F.meshSDFVelocity(*mesh, V, n, origin, spacing, band)
    again = F.meshSDFVelocity(mesh[0], np.roll(mesh[1][::-1], 1, axis=1), V, n, origin, spacing, band)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


# ---- GPU: the face pass ----------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pattern(shape, seed=23):
    rng = np.random.default_rng(seed)
    return [(rng.random(MV.face_positions(shape, a)[0].shape) * 2 - 1).astype(np.float32) for a in range(3)]


def assert_faces(got, pattern, ids, shape, ref_shapes, samples, motions, what, k0=0):
    """the faces the rule writes under section 17's bound, every other face with the pattern's bits"""
    want = MV.face_velocity(shape, ids, ref_shapes, samples, motions, k0)
    counts = []
    for a in range(3):
        mask, value, terms = want[a]
        g = got[a].cpu().numpy()
        assert np.array_equal(g[~mask], pattern[a][~mask]), (what, a)
        err = np.abs(g[mask].astype(np.float64) - value[mask])
        bound = 2.0 ** -24 * np.abs(value[mask]) + 1e-10 * terms[mask]
        counts.append(int(mask.sum()))
        print(f"{what} axis {a}: {counts[-1]} faces written, worst error / bound {(err / np.maximum(bound, 1e-300)).max():.3f}, worst error {err.max():.2e}")
        assert (err <= bound).all(), (what, a)
    return counts


def _mesh_body(centre, half, R, spacing=0.5, band=3.0, seed=5):
    """(device shape with .velocity, the restatement's Shape, the device's samples as a float32 array) of a box mesh with seeded
    vertex velocities"""
    from geometricmultigridpressuresolver_amd import fields as F

    mesh = MR.box(-np.asarray(half), np.asarray(half))
    V = vertex_velocities(mesh, seed)
    shape = F.BodyShape.mesh(centre, *mesh, spacing, band + np.sqrt(3.0) * spacing, R, vertex_velocities=V)
    n, origin = MR.sample_box(mesh[0], spacing, band + np.sqrt(3.0) * spacing)
    assert (shape.nx, shape.ny, shape.nz) == n and tuple(shape.velocity.shape) == (3,) + n[::-1]
    return shape, RR.sdf_grid(centre, shape._keep.cpu().numpy(), origin, spacing, R), shape.velocity.cpu().numpy()


@pytest.mark.gpu
def test_face_pass_equals_the_restatement_and_leaves_every_other_face():
    """section 18's grid with a rotated mesh box (body 1, sampled) and a sphere without samples (body 2), a moving frame, the grids
    pre-filled with a pattern; some faces are given ids out of range by hand"""
    import test_raster_bodies as TR

    from geometricmultigridpressuresolver_amd import fields as F

    shape = TR.GRID
    centre = (17.0 + np.sqrt(3.0) / 3, 11.0 + np.sqrt(5.0) / 7, 9.0 + np.sqrt(2.0) / 5)
    dev, ref, samples = _mesh_body(centre, TM.BOX_HALF, RR.rotation((1.0, 2.0, 3.0), 0.7))
    ball = F.BodyShape.sphere((5.2, 15.3, 12.1), 2.6)
    _, _, body = F.rasterizeBodies(shape, [dev, ball], 3.0, 0.0)
    ids = [b.cpu().numpy() for b in body]
    assert all((b == 1).sum() > 50 and (b == 2).sum() > 20 and (b == 0).sum() > 1000 for b in ids)
    for a in range(3):  # ids out of range, on faces the rule would otherwise write and on others
        flat = ids[a].reshape(-1)
        flat[np.flatnonzero(flat == 1)[::7]] = 3
        flat[np.flatnonzero(flat == 0)[::11]] = -1
        flat[np.flatnonzero(flat == 0)[::13]] = 300
    motions = np.array([[0.31, -0.22, 0.17, 0.021, -0.013, 0.034], [0.5, 0.5, 0.5, 0.1, 0.1, 0.1]])
    pattern = _pattern(shape)
    got = F.sampledVelocity([_dev(p) for p in pattern], [_dev(b) for b in ids], [dev, ball], motions)
    counts = assert_faces(got, pattern, ids, shape, [ref, None], [samples, None], motions, "rotated mesh box")
    assert min(counts) > 40
    # frame_motions=None is a frame at rest, and two calls give the same bits
    import torch

    rest = F.sampledVelocity([_dev(p) for p in pattern], [_dev(b) for b in ids], [dev, ball])
    assert_faces(rest, pattern, ids, shape, [ref, None], [samples, None], np.zeros((2, 6)), "frame at rest")
    again = F.sampledVelocity([_dev(p) for p in pattern], [_dev(b) for b in ids], [dev, ball], motions)
    assert all(torch.equal(got[a], again[a]) for a in range(3))


@pytest.mark.gpu
@pytest.mark.parametrize("gx", [64, 65, 131])
def test_owned_faces_across_tiles_along_x(gx):
    """the tile is 64 cells long: a mesh box across every tile boundary of a grid of one tile, of a tile and a single column, and of
    three tiles"""
    from geometricmultigridpressuresolver_amd import fields as F

    shape = (6, 9, gx)
    centre = (0.5 * gx + np.sqrt(2.0) / 7, 4.0 + np.sqrt(3.0) / 5, 3.0 + np.sqrt(5.0) / 9)
    dev, ref, samples = _mesh_body(centre, (0.5 * gx - 2.3, 1.7, 1.2), RR.rotation((0.1, 0.2, 1.0), 0.02), band=2.0)
    _, _, body = F.rasterizeBodies(shape, [dev], 2.0, 0.0)
    ids = [b.cpu().numpy() for b in body]
    assert (ids[0][:, :, 60:min(70, gx)] == 1).any() and (gx < 131 or (ids[1][:, :, 120:131] == 1).any())
    motions = np.array([[0.1, 0.2, -0.3, 0.01, 0.02, -0.01]])
    pattern = _pattern(shape)
    got = F.sampledVelocity([_dev(p) for p in pattern], body, [dev], motions)
    assert_faces(got, pattern, ids, shape, [ref], [samples], motions, f"gx = {gx}")


def stretching_box(s=0.05):
    """(mesh, vertex velocities, half) of an axis-aligned box stretching along x: V = S x, S = diag(s, 0, 0)"""
    half = np.array([5.3, 7.4, 7.2])
    mesh = MR.box(-half, half)
    V = np.zeros_like(mesh[0])
    V[:, 0] = s * mesh[0][:, 0]
    return mesh, V, half


@pytest.mark.gpu
def test_a_stretching_box_is_exact_on_its_planes():
    """x-faces owned by the body whose closest point lies on the +-x face, further than band + sqrt(3) spacing from the box's edges:
    the field is constant there (+-s h_x) and trilinear interpolation reproduces it: float(+-s h_x) within 1 ulp"""
    from geometricmultigridpressuresolver_amd import fields as F

    s, spacing, band = 0.05, 0.5, 3.0
    mesh, V, half = stretching_box(s)
    shape, centre = (24, 24, 26), np.array([13.2, 12.1, 11.7])
    sample_band = band + np.sqrt(3.0) * spacing
    dev = F.BodyShape.mesh(centre, *mesh, spacing, sample_band, vertex_velocities=V)
    _, _, body = F.rasterizeBodies(shape, [dev], band, 0.0)
    sv = [_dev(np.full(MV.face_positions(shape, a)[0].shape, 7.0, dtype=np.float32)) for a in range(3)]
    F.sampledVelocity(sv, body, [dev])
    x, y, z = MV.face_positions(shape, 0)
    xb, yb, zb = x - centre[0], y - centre[1], z - centre[2]
    margin = sample_band + np.sqrt(3.0) * spacing
    ids = body[0].cpu().numpy()
    got = sv[0].cpu().numpy()
    for sign in (1.0, -1.0):
        pick = (ids == 1) & (np.abs(sign * xb - half[0]) <= 1.0) & (np.abs(yb) < half[1] - margin) & (np.abs(zb) < half[2] - margin)
        want = np.float32(sign * s * half[0])
        ulps = np.abs(got[pick].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()
        print(f"{'+' if sign > 0 else '-'}x face: {int(pick.sum())} faces, {ulps} ulps from {want}")
        assert pick.sum() > 20 and ulps <= 1
    assert (got[ids == 0] == 7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [2, 3, "odd"])
def test_windows_equal_the_whole_grid(size):
    """section 18's cuts: 2-way and 3-way cuts of the layout and a cut of the caller's at base plane 21, through the body"""
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    shape = (48, 20, 24)
    dev, _, _ = _mesh_body((12.3, 9.6, 24.2), (4.1, 3.3, 15.2), RR.rotation((1.0, 0.3, 0.1), 0.25))
    shapes = [dev, F.BodyShape.sphere((6.1, 14.2, 40.3), 3.2)]
    _, _, body = F.rasterizeBodies(shape, shapes, 3.0, 0.03)
    motions = np.array([[0.2, -0.1, 0.3, 0.02, 0.01, -0.03], [0.0] * 6])
    pattern = [_dev(p) for p in _pattern(shape)]
    whole = F.sampledVelocity([p.clone() for p in pattern], body, shapes, motions)
    assert all(int((whole[a] != pattern[a]).sum()) > 100 for a in range(3))
    if size == "odd":
        lay = F.projection_slab_layout(shape, True, 2, False)
        size, splits = 2, [0, lay["offset"] + 21, lay["expanded"][0]]
    else:
        splits = F.projection_slab_layout(shape, True, size, False)["splits"]
    tops = []
    for rank in range(size):
        d = F.slab_window(shape, True, splits, rank)
        cut = lambda g: [g[0][d.c0:d.c1].clone(), g[1][d.c0:d.c1].clone(), g[2][d.c0:d.c1 + 1].clone()]  # noqa: E731  (copies: the pass writes in place)
        sv = F.sampledVelocitySlab(d, cut(pattern), cut(body), shapes, motions)
        for a, want in enumerate(cut(whole)):
            assert torch.equal(sv[a], want), (rank, a)
        if rank > 0:  # both copies of the cut's z-face plane; the body straddles it
            assert torch.equal(tops.pop(), sv[2][0])
            assert int((body[2][d.c0] == 1).sum()) > 0 and int((sv[2][0] != pattern[2][d.c0]).sum()) > 0
        tops.append(sv[2][-1].clone())
    assert d.c1 == shape[0]


# ---- GPU: end to end -------------------------------------------------------------------------------------------------------------------
def _pool():
    import test_raster_bodies as TR
    import test_rigid_coupling as T

    shape = T.POOL
    k = np.arange(shape[0], dtype=np.float32)[:, None, None] + np.zeros(shape, dtype=np.float32)
    liquid_phi = ((k + 0.5) - 22.3).astype(np.float32) / max(shape)
    _, scw = TR.walls(shape)
    scw[0][:] = np.where(scw[0] == np.float32(0.4), np.float32(1.0), scw[0])  # (closed walls only)
    rng = np.random.default_rng(5)
    velocity = [(rng.random(w.shape) * 2 - 1).astype(np.float32) for w in scw]
    return shape, liquid_phi, scw, velocity


def _fp64_vectors():
    """the options of test_rigid_coupling._projection: fp64 PCG vectors, so that its tolerance of 1e-7 is within reach"""
    import geometricmultigridpressuresolver_amd as G

    opt = G.default_options()
    opt.pcg_fp64_vectors = 1
    return opt


def _divergence(liquid_phi, solid_phi, cw, velocity, sv):
    """the largest divergence of `velocity` (host arrays) against the solid velocity `sv`, by the device pass"""
    from geometricmultigridpressuresolver_amd import fields as F

    cwd = [_dev(w) for w in cw]
    material = F.buildMaterialCellLabels(_dev(liquid_phi), _dev(solid_phi), cwd)
    return F.computeResultingDivergence(material, [_dev(v) for v in velocity], cwd, [_dev(a) for a in sv])[1]


@pytest.mark.gpu
def test_projection_against_the_sampled_velocity_of_a_stretching_box():
    """Section 18's pool with the stretching box as a mesh collider: project_free_surface with solid_velocity = the sampled velocity
    converges, and the divergence it leaves against that field is at most 4 x what the same scene leaves when the box instead
    translates rigidly with U = (s h_x, 0, 0) through rigidVelocity (section 17's margin; the reference run is made here).  Measured
    against sv = 0 the divergence is more than 10^3 times larger: the samples do reach the right-hand side."""
    import test_rigid_coupling as T

    from geometricmultigridpressuresolver_amd import fields as F

    shape, liquid_phi, scw, velocity = _pool()
    s = 0.05
    mesh, V, half = stretching_box(s)
    centre = np.array([20.3, 16.2, 13.1])
    dev = F.BodyShape.mesh(centre, *mesh, 0.5, 3.0 + np.sqrt(3.0) * 0.5, vertex_velocities=V)
    solid_phi, cw, body = F.rasterizeBodies(shape, [dev], 3.0, 0.05, None, [_dev(w) for w in scw])
    zeros = lambda: [_dev(np.zeros_like(w)) for w in scw]  # noqa: E731
    sv = [a.cpu().numpy() for a in F.sampledVelocity(zeros(), body, [dev])]
    centres, motions = np.zeros((2, 3)), np.zeros((2, 6))
    centres[1], motions[1, 0] = centre, s * half[0]
    sv_rigid = [a.cpu().numpy() for a in F.rigidVelocity(zeros(), body, centres, motions)]
    assert (sv[0] != 0).sum() > 300 and np.abs(sv[0]).max() <= np.float32(s * half[0]) * (1 + 1e-6)
    solid_h, cw_h = solid_phi.cpu().numpy(), [w.cpu().numpy() for w in cw]
    out = {}
    for name, field in (("sampled", sv), ("rigid", sv_rigid)):
        vel, pressure = [v.copy() for v in velocity], np.zeros(shape, dtype=np.float32)
        _, info = F.project_free_surface(liquid_phi, solid_h, cw_h, vel, pressure, field, use_old_pressure=False, use_gauss_seidel=False,
                                         tolerance=T.TOL, options=_fp64_vectors())
        assert info["outcome"] == 0, (name, info)
        out[name] = (_divergence(liquid_phi, solid_h, cw_h, vel, field), _divergence(liquid_phi, solid_h, cw_h, vel, [np.zeros_like(a) for a in field]),
                     info["iterations"])
    (end, bare, it), (kin, _, it0) = out["sampled"], out["rigid"]
    print(f"stretching box: max divergence {end:.3e} against the sampled velocity, {kin:.3e} left by the rigid translation (bound 4 x), "
          f"{bare:.3e} against sv = 0 ({bare / end:.0f} x, bound > 1000 x); iterations {it} / {it0}")
    assert end <= 4 * kin
    assert bare > 1e3 * end


@pytest.mark.gpu
def test_a_floating_rigid_box_beside_a_deforming_collider():
    """A floating rigid box (id 1, two-way) and the stretching collider (id 2) in the pool: project_free_surface_rigid is given ONE
    body and the sampled field as its solid_velocity, so the collider's faces fall into row 0.  It converges, the collider's faces in
    the returned solid_velocity keep the sampled bits, and the divergence against that field with the box at V_out is at most 4 x the
    kinematic run's."""
    import torch

    import test_rigid_coupling as T

    from geometricmultigridpressuresolver_amd import fields as F

    shape, liquid_phi, scw, velocity = _pool()
    s = 0.05
    mesh, V, half = stretching_box(s)
    collider = F.BodyShape.mesh((26.9, 16.2, 13.3), *MR.box(-half * [0.9, 1.0, 0.8], half * [0.9, 1.0, 0.8]), 0.5, 3.0 + np.sqrt(3.0) * 0.5,
                                vertex_velocities=V * 0.9)
    box_centre, box_half = np.array([8.3, 15.2, 18.1]), np.array([4.7, 8.2, 5.4])
    floating = F.BodyShape.box(box_centre, box_half, RR.rotation((0.3, 1.0, 0.2), 0.12))
    solid_phi, cw, body = F.rasterizeBodies(shape, [floating, collider], 3.0, 0.05, None, [_dev(w) for w in scw])
    assert all(int((b == 1).sum()) > 100 and int((b == 2).sum()) > 100 for b in body)
    zeros = lambda: [torch.zeros_like(w) for w in cw]  # noqa: E731
    sv = F.sampledVelocity(zeros(), body, [floating, collider])
    assert all(int(((sv[a] != 0) & (body[a] != 2)).sum()) == 0 for a in range(3)) and int((sv[0] != 0).sum()) > 100
    centres, inv_mass, inv_inertia = T._box_tables([(box_centre - box_half, box_centre + box_half)], [0.5])
    motions = T._motions(1, 51)
    phi = _dev(liquid_phi)
    out = {}
    for coupled in (False, True):
        vel, pressure = [_dev(v) for v in velocity], torch.zeros(shape, dtype=torch.float32, device="cuda")
        k = (inv_mass, inv_inertia) if coupled else (np.zeros_like(inv_mass), np.zeros_like(inv_inertia))
        res = F.project_free_surface_rigid(phi, solid_phi, cw, vel, pressure, body, centres, *k, motions, solid_velocity=sv, use_old_pressure=False,
                                           use_gauss_seidel=False, tolerance=T.TOL, options=_fp64_vectors())
        assert res["stats"]["outcome"] == "converged", res["stats"]
        for a in range(3):  # the collider's faces keep the sampled bits; the box's faces hold its rigid velocity
            mine = body[a] == 2
            assert torch.equal(res["solid_velocity"][a][mine], sv[a][mine]) and int((res["solid_velocity"][a][body[a] == 1] != 0).sum()) > 50
        end_sv = F.rigidVelocity([t.clone() for t in sv], body, centres, res["motions"])
        out[coupled] = (F.computeResultingDivergence(res["material"], vel, cw, end_sv)[1], res)
    (kin, res0), (end, res) = out[False], out[True]
    print(f"floating box + deforming collider: max divergence {end:.3e} against (rigidVelocity(V_out), sampled), {kin:.3e} left by the kinematic run "
          f"(bound 4 x); coupled cells {res['coupled_cells']}, iterations {res['stats']['iterations']} / {res0['stats']['iterations']}")
    assert res["coupled_cells"] > 100 and np.abs(res["motions"][1] - motions[1]).sum() > 0
    assert end <= 4 * kin
