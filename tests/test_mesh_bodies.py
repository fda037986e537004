"""Triangle-mesh rigid bodies (include/mgps_fields.h) against tests/mesh_reference.py.

CPU: the restatement against analysis (a sphere's distance, the membership of an L-shaped prism and of a hollow shell, columns that
run through edges, face diagonals and vertices), the mass properties of the library and of the restatement against closed forms, the
C ABI's refusals and the ctypes mirrors' sizes.
GPU: parity of mgps_fields_mesh_sdf with the restatement on five meshes and two sample grids, rows across tile edges, the ties again,
the same bits for any triangle order, any cyclic turn and on every run, a mesh body through the rasteriser, and two sub-steps of
rasterise -> coupled projection -> move with a 12-triangle box.

Tolerances.  Both sides form every value in fp64 and round to float32 once: at most 4 float32 ulps (the issue's bound, section 18's
for solid_phi; 0 or 1 is expected).  The sign is a decision: the tests first assert on the restatement that it is not round-off (no
sample within 1e-9 of the surface, no column within 1e-9 of an edge's line) or, in the tie cases, that every number involved is exact
(integer and half-integer coordinates).

The sphere.  The issue asks that the restated distance be within "the chord error r (1 - cos(half the largest edge's angle))" of
|x| - 5.  That figure is the gap between the sphere and an EDGE's middle; the gap over a FACE's middle is r (1 - cos(the face's
angular circumradius)), 1.33 x as much for a small equilateral face, and a correct distance attains it (at the sphere point over a
face's middle |x| - 5 = 0 and d is that gap).  So the test asserts 0 <= sdf_mesh - (|x| - 5) <= the face gap everywhere (the mesh is
inscribed), and the issue's edge figure where it does hold: on the rays through the edges' middles and the vertices, at the surface and
outside it."""
import ctypes as C
import functools

import numpy as np
import pytest

import mesh_reference as MR
import raster_reference as RR
from refusals import refused as _refused

SPACING, BAND = 0.37, 2.5
GRIDS = ((19, 17, 13), (70, 9, 6))  # (nx, ny, nz): the second has a row longer than one wave


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def meshes():
    s2, s3, s5 = np.sqrt(2.0), np.sqrt(3.0), np.sqrt(5.0)
    return {
        "tetrahedron": MR.moved(MR.tetrahedron(4.0), RR.rotation((1.0, 0.4, -0.3), 0.35), (s2 / 9, -s3 / 11, s5 / 13)),
        "box": MR.moved(MR.box((-1.7, -1.2, -0.9), (1.7, 1.2, 0.9)), RR.rotation((1.0, 2.0, 3.0), 0.7), (s3 / 7, s5 / 9, -s2 / 5)),
        "icosphere": MR.moved(MR.icosphere(1.9, 2), None, (s5 / 11, s2 / 7, s3 / 13)),
        "l_prism": MR.l_prism(),  # axis-aligned: ten of its triangles have no projected area
        "shell": MR.moved(MR.shell((-1.9, -1.6, -1.4), (1.9, 1.6, 1.4), (-1.0, -0.8, -0.6), (1.0, 0.8, 0.6)), RR.rotation((0.2, -1.0, 0.5), 0.2),
                          (s2 / 13, s3 / 9, s5 / 7)),
    }


def grid_origin(mesh, n, spacing=SPACING):
    """the samples centred on the mesh's bounding box, moved off it by irrational fractions of the spacing"""
    v = mesh[0]
    mid = 0.5 * (v.min(axis=0) + v.max(axis=0))
    return mid - 0.5 * spacing * (np.array(n) - 1) + spacing * np.array([np.sqrt(2.0) / 10, np.sqrt(3.0) / 10, np.sqrt(5.0) / 10])


@functools.lru_cache(maxsize=None)
def restated(name, n):
    """(sigma min(d, band), d) of the restatement, after the asserts that no sign is round-off"""
    mesh = meshes()[name]
    want, d, gap = MR.mesh_sdf(*mesh, n, grid_origin(mesh, n), SPACING, BAND, details=True)
    assert d.min() >= 1e-9 and gap >= 1e-9, (name, n, d.min(), gap)
    want.setflags(write=False)
    return want, d


def _ulps(a, b):
    def ordered(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    return int(np.abs(ordered(a) - ordered(b)).max())


# ---- CPU: the restatement against analysis -------------------------------------------------------------------------------------------
def test_restated_distance_of_an_icosphere_is_the_sphere_within_the_chord_error():
    r = 5.0
    v, t = MR.icosphere(r, 2)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    edges = np.concatenate([np.linalg.norm(p - q, axis=1) for p, q in ((a, b), (b, c), (c, a))])
    edge_gap = r * (1 - np.cos(np.arcsin(edges.max() / 2 / r)))  # r (1 - cos(half the largest edge's angle))
    la, lb, lc = (np.linalg.norm(p - q, axis=1) for p, q in ((b, c), (c, a), (a, b)))
    circumradius = la * lb * lc / (2 * np.linalg.norm(np.cross(b - a, c - a), axis=1))
    face_gap = r * (1 - np.cos(np.arcsin(circumradius.max() / r)))
    assert edge_gap < face_gap < 1.4 * edge_gap
    rng = np.random.default_rng(3)
    p = rng.uniform(-8.0, 8.0, (1500, 3))
    p = np.concatenate([p, r * rng.standard_normal((300, 3)) / 1.7, (a + b + c) / 3 * 1.2])
    sdf = np.where(MR.inside(v, t, p[:, 0], p[:, 1], p[:, 2]), -1.0, 1.0) * MR.distance(v, t, p[:, 0], p[:, 1], p[:, 2])
    off = sdf - (np.linalg.norm(p, axis=1) - r)
    print(f"icosphere of {len(t)} triangles: sdf - (|x| - r) in [{off.min():.3e}, {off.max():.3e}], face gap {face_gap:.4e}, edge gap {edge_gap:.4e}")
    assert off.min() >= -1e-12 and off.max() <= face_gap + 1e-12
    assert off.max() > edge_gap  # (why the bound over all points is the face's)
    # the issue's figure, where it holds: on the rays through the edges' middles and the vertices, at the surface and outside
    # (inside, the nearest feature is a face again)
    rays = np.concatenate([0.5 * (a + b), 0.5 * (b + c), 0.5 * (c + a), v])
    rays = rays / np.linalg.norm(rays, axis=1)[:, None]
    for scale in (1.0, 1.03, 1.1, 1.6):
        q = rays * (scale * r)
        off = MR.distance(v, t, q[:, 0], q[:, 1], q[:, 2]) - np.abs(scale * r - r)
        assert np.abs(off).max() <= edge_gap + 1e-12, (scale, np.abs(off).max(), edge_gap)


def test_restated_sign_is_the_membership_of_an_l_prism_and_of_a_hollow_shell():
    rng = np.random.default_rng(4)
    p = rng.uniform(-0.5, 3.5, (4000, 3))
    got = MR.inside(*MR.l_prism(), p[:, 0], p[:, 1], p[:, 2])
    want = MR.in_l_prism(p[:, 0], p[:, 1], p[:, 2])
    assert np.array_equal(got, want) and 500 < want.sum() < 3500
    outer, inner = ((-2.0, -1.5, -1.0), (2.0, 1.5, 1.0)), ((-1.0, -0.7, -0.4), (1.0, 0.7, 0.4))
    p = rng.uniform(-2.5, 2.5, (4000, 3))
    within = lambda b: np.all((p > np.array(b[0])) & (p < np.array(b[1])), axis=1)  # noqa: E731
    got = MR.inside(*MR.shell(*outer, *inner), p[:, 0], p[:, 1], p[:, 2])
    assert np.array_equal(got, within(outer) & ~within(inner)) and within(inner).sum() > 50


# ---- ties: columns exactly through edges, face diagonals and vertices ----------------------------------------------------------------
def tie_cases():
    """(name, mesh, n, origin, spacing, analytic membership at the samples off the surface): every coordinate is an integer or a half,
    so every edge function is exact and many are exactly zero"""
    out = []
    mesh = MR.box((1.0, 1.0, 1.0), (4.0, 5.0, 3.0))
    n, origin = (7, 8, 6), np.array([-1.0, -1.0, -1.0])
    x, y, z = MR.sample_points(n, origin, 1.0)
    out.append(("box", mesh, n, origin, 1.0, (x > 1) & (x < 4) & (y > 1) & (y < 5) & (z > 1) & (z < 3)))
    mesh = MR.octahedron(3.0)
    n, origin = (17, 17, 17), np.array([-4.0, -4.0, -4.0])
    x, y, z = MR.sample_points(n, origin, 0.5)
    out.append(("octahedron", mesh, n, origin, 0.5, np.abs(x) + np.abs(y) + np.abs(z) < 3))
    return out


def test_ties_columns_through_edges_diagonals_and_vertices_get_the_analytic_sign():
    for name, mesh, n, origin, spacing, member in tie_cases():
        x, y, z = MR.sample_points(n, origin, spacing)
        d = MR.distance(*mesh, x, y, z)
        got, gap = MR.inside(*mesh, x, y, z, gaps=True)
        assert gap == 0.0  # columns do run exactly through edges' lines
        off = d > 1e-9  # (d > 0 in exact arithmetic: a sample on an edge may get 1e-16 from the rounding of the edge's parameter)
        assert np.array_equal(got[off], member[off]), name
        assert (~off).sum() > 20 and member.sum() > 5
        # "zero counts as positive" gets some of these wrong, which is why the rule is there: a column through a vertex of the octahedron
        if name == "octahedron":
            k, j = 8, 8  # the column y = z = 0 runs through the vertices (+-3, 0, 0)
            assert np.array_equal(got[k, j][off[k, j]], (np.abs(x[k, j]) < 3)[off[k, j]]) and (~off[k, j]).sum() == 2


# ---- mass properties -----------------------------------------------------------------------------------------------------------------
def _mass_cases():
    a, b, c = 2.3, 1.7, 0.9
    edge = 1.9
    vol = edge ** 3 / (6 * np.sqrt(2.0))
    return [("box", MR.box((-a / 2, -b / 2, -c / 2), (a / 2, b / 2, c / 2)), a * b * c, a * b * c / 12 * np.diag([b * b + c * c, a * a + c * c, a * a + b * b])),
            ("tetrahedron", MR.tetrahedron(edge), vol, vol * edge ** 2 / 20 * np.eye(3))]


@pytest.mark.parametrize("which", ["library", "restatement"])
def test_mass_properties_match_the_closed_forms(which):
    from geometricmultigridpressuresolver_amd import fields as F

    mass = F.meshMassProperties if which == "library" else MR.mass_properties
    R, shift = RR.rotation((0.3, -1.0, 0.7), 0.9), np.array([3.1, -2.2, 1.7])
    for name, mesh, volume, inertia in _mass_cases():
        for rot, move in ((None, np.zeros(3)), (R, shift)):
            v, centre, tensor = mass(*MR.moved(mesh, rot, move))
            want = inertia if rot is None else rot @ inertia @ rot.T  # the inertia transforms as R I R^T
            assert abs(v - volume) <= 1e-12 * volume, (name, v, volume)
            assert np.abs(centre - move).max() <= 1e-12 * max(1.0, np.abs(move).max()), (name, centre)
            assert np.abs(tensor - want).max() <= 1e-12 * np.abs(inertia).max(), (name, tensor, want)
            assert np.abs(tensor - tensor.T).max() <= 1e-12 * np.abs(inertia).max()


def test_icosphere_inertia_converges_to_two_fifths_m_r2_from_below():
    from geometricmultigridpressuresolver_amd import fields as F

    r, last = 1.3, 0.0
    for level in range(4):
        v, centre, tensor = F.meshMassProperties(*MR.icosphere(r, level))
        ball = 0.4 * (4 / 3 * np.pi * r ** 3) * r * r
        assert np.abs(centre).max() <= 1e-12 and np.abs(tensor - tensor[0, 0] * np.eye(3)).max() <= 1e-12 * ball
        assert last < tensor[0, 0] < ball
        last = tensor[0, 0]
    assert ball - last < 0.03 * ball


# ---- CPU: the C ABI refuses bad arguments on the host --------------------------------------------------------------------------------
def _desc(mesh=None, **kw):
    from geometricmultigridpressuresolver_amd import fields as F

    v, t = MR.tetrahedron(2.0) if mesh is None else mesh
    v, t = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(t, dtype=np.int32)
    d = F.MeshDesc()
    d.struct_size = C.sizeof(F.MeshDesc)
    d.vertices, d.triangles, d.xyz, d.tri = len(v), len(t), v.ctypes.data, t.ctypes.data
    d.nx = d.ny = d.nz = 8
    d.origin[:] = [-2.0, -2.0, -2.0]
    d.spacing, d.band = 0.5, 1.0
    d.sdf = 64  # (never dereferenced: every call below is refused on the host)
    for k, val in kw.items():
        setattr(d, k, val)
    return d, (v, t)


def test_argument_refusals_need_no_device_and_the_mirrors_have_the_library_size():
    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd._lib import lib

    L = lib()
    fn = "mgps_fields_mesh_sdf"
    sdf = lambda d: L.mgps_fields_mesh_sdf(C.byref(d[0]), None)  # noqa: E731
    # the mirror's size is the library's: a good struct gets as far as the next check, one of another size is refused as such
    _refused(sdf(_desc(sdf=None)), fn, "sdf", "NULL")
    d = _desc()
    d[0].struct_size -= 4
    _refused(sdf(d), fn, "struct_size")
    _refused(L.mgps_fields_mesh_sdf(None, None), "struct_size")
    # ... and the last field is read where the library expects it: with everything else good, only a bad band is refused
    for band in (0.0, -1.0, float("inf"), float("nan")):
        _refused(sdf(_desc(band=band)), "band")
    for name in ("nx", "ny", "nz"):
        for n in (1, 1025):
            _refused(sdf(_desc(**{name: n})), "dimension", "2 .. 1024")
    for spacing in (0.0, -0.5, float("nan"), float("inf")):
        _refused(sdf(_desc(spacing=spacing)), "spacing")
    d = _desc()
    d[0].origin[1] = float("nan")
    _refused(sdf(d), "origin")
    for name in ("xyz", "tri"):
        _refused(sdf(_desc(**{name: None})), "NULL")
    _refused(sdf(_desc(vertices=3)), "at least 4")
    _refused(sdf(_desc(triangles=3)), "at least 4")

    # the mesh faults, through both entries
    mass = lambda v, t: L.mgps_mesh_mass_properties(len(v), len(t), v.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), C.byref(F.MassProperties()))  # noqa: E731

    def both(v, t, *words):
        v, t = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(t, dtype=np.int32)
        _refused(sdf(_desc((v, t))), fn, *words)
        _refused(mass(v, t), "mgps_mesh_mass_properties", *words)

    v, t = MR.box((0, 0, 0), (2, 3, 1))
    for bad in (8, -1):
        t2 = t.copy()
        t2[5, 1] = bad
        both(v, t2, "triangle 5", "out of range")
    v2 = v.copy()
    v2[3, 2] = float("inf")
    both(v2, t, "non-finite coordinate")
    t2 = t.copy()
    t2[7, 2] = t2[7, 0]
    both(v, t2, "triangle 7", "repeated index")
    v2, t2 = np.concatenate([v, [0.5 * (v[t[4, 0]] + v[t[4, 1]])]]), t.copy()
    t2[4, 2] = 8  # (the third corner on the line through the other two)
    both(v2, t2, "triangle 4", "zero area")
    # an open mesh and one with a flipped triangle name an edge
    both(v, np.delete(t, 0, axis=0), "not closed and consistently oriented", "edge (", "occurs 1 times", "reverse 0 times")
    t2 = t.copy()
    t2[1] = t2[1, ::-1]
    both(v, t2, "not closed and consistently oriented", "edge (", "occurs 2 times", "reverse 0 times")
    both(*MR.flipped((v, t)), "orientation")
    assert mass(*[np.ascontiguousarray(q) for q in (v.astype(np.float64), t.astype(np.int32))]) == 0
    assert L.mgps_mesh_mass_properties(len(v), len(t), v.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), None) == 1

    # the sample box
    n, origin = F.meshSampleBox(v, 0.5, 1.25)
    assert n == MR.sample_box(v, 0.5, 1.25)[0] == (12, 14, 10) and np.array_equal(origin, [-1.75, -1.75, -1.75])
    out_n, out_origin = (C.c_int * 3)(), (C.c_double * 3)()
    box = lambda spacing, band: L.mgps_mesh_sample_box(len(v), v.ctypes.data_as(C.c_void_p), C.c_double(spacing), C.c_double(band), out_n, out_origin)  # noqa: E731
    _refused(box(0.0, 1.0), "mgps_mesh_sample_box", "spacing")
    _refused(box(0.5, float("nan")), "band")
    _refused(box(0.001, 1.0), "1024")
    _refused(L.mgps_mesh_sample_box(len(v), None, C.c_double(0.5), C.c_double(1.0), out_n, out_origin), "NULL")
    assert C.sizeof(F.MassProperties) == 13 * 8 and C.sizeof(F.MeshDesc) == 96


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def assert_parity(got, want, d, band, what):
    got = got.cpu().numpy()
    want32 = want.astype(np.float32)
    ulps = _ulps(got, want32)
    far = d > band
    print(f"{what}: {ulps} ulps (bound 4), {int((want < 0).sum())} samples inside, {int(far.sum())} beyond band")
    assert np.array_equal(got < 0, want < 0), what
    assert ulps <= 4, what
    assert np.array_equal(got[far], np.where(want[far] < 0, -np.float32(band), np.float32(band))), what
    return ulps


@pytest.mark.gpu
@pytest.mark.parametrize("n", GRIDS)
@pytest.mark.parametrize("name", ["tetrahedron", "box", "icosphere", "l_prism", "shell"])
def test_device_samples_equal_the_restatement(name, n):
    from geometricmultigridpressuresolver_amd import fields as F

    mesh = meshes()[name]
    want, d = restated(name, n)
    assert (want < 0).sum() > 20 and (n[0] < 64 or (d > BAND).sum() > 100)
    assert len(mesh[1]) == {"tetrahedron": 4, "box": 12, "icosphere": 320, "l_prism": 20, "shell": 24}[name]
    got = F.meshSDF(*mesh, n, grid_origin(mesh, n), SPACING, BAND)
    assert tuple(got.shape) == n[::-1]
    assert_parity(got, want, d, BAND, f"{name} {n}")


def tile_edge_case(nx):
    """(mesh, n, origin): an icosphere across the tile edges of a row of nx samples.  nx = 64 and 65: a sphere of radius 10.5 in the middle
    of the row, whose last sample is still within band of it.  nx = 131: a sphere of radius 16 about the middle of the second tile (sample 95.5), which lies band and more inside it"""
    n = (nx, 9, 6)
    radius, middle = (16.0, 95.5) if nx == 131 else (10.5, 0.5 * (nx - 1))
    mesh = MR.moved(MR.icosphere(radius, 2), None, (np.sqrt(2.0) / 9, np.sqrt(3.0) / 7, np.sqrt(5.0) / 11))
    origin = grid_origin(mesh, n)
    origin[0] = mesh[0][:, 0].mean() - SPACING * middle + SPACING * np.sqrt(2.0) / 10
    return mesh, n, origin


@pytest.mark.gpu
@pytest.mark.parametrize("nx", [64, 65, 131])
def test_rows_across_tile_edges(nx):
    """the tile is 64 samples long: exactly one tile, a tile and one sample, and three tiles of which the second lies deep inside the
    mesh (an empty list: -band everywhere)"""
    from geometricmultigridpressuresolver_amd import fields as F

    mesh, n, origin = tile_edge_case(nx)
    want, d, gap = MR.mesh_sdf(*mesh, n, origin, SPACING, BAND, details=True)
    assert d.min() >= 1e-9 and gap >= 1e-9
    assert (want == -BAND).sum() > 0 and (nx == 131 or (np.abs(want[:, :, nx - 1]) < BAND).all())
    if nx == 131:
        assert (want[:, :, 64:128] == -BAND).all() and (np.abs(want[:, :, :64]) < BAND).any() and (want == BAND).sum() > 0
    assert_parity(F.meshSDF(*mesh, n, origin, SPACING, BAND), want, d, BAND, f"nx = {nx}")


def one_tile_case():
    """(mesh, n, origin, band): a bar of 6 x 1.2 x 1.2 sample cells whose reach (band = 0.8 cells) stays inside the first tile of
    64 x 4 x 4 samples"""
    h = SPACING
    mid = np.array([10 * h + 0.011, 1.5 * h + 0.007, 1.5 * h + 0.003])
    return MR.box(mid - h * np.array([3.0, 0.6, 0.6]), mid + h * np.array([3.0, 0.6, 0.6])), (70, 9, 6), np.zeros(3), 0.8 * h


@pytest.mark.gpu
def test_a_mesh_inside_one_tile():
    from geometricmultigridpressuresolver_amd import fields as F

    mesh, n, origin, band = one_tile_case()
    lo, hi = mesh[0].min(axis=0) - band, mesh[0].max(axis=0) + band
    assert (lo > 0).all() and (hi < SPACING * np.array([63, 3, 3])).all()  # its reach stays inside the tile at the origin
    want, d, gap = MR.mesh_sdf(*mesh, n, origin, SPACING, band, details=True)
    assert d.min() >= 1e-9 and gap >= 1e-9 and (want < 0).sum() >= 8
    assert (want[:, :, 64:] == band).all() and (want[4:] == band).all() and (want[:, 4:] == band).all()
    assert_parity(F.meshSDF(*mesh, n, origin, SPACING, band), want, d, band, "one tile")


@pytest.mark.gpu
def test_ties_on_the_device():
    from geometricmultigridpressuresolver_amd import fields as F

    for name, mesh, n, origin, spacing, member in tie_cases():
        x, y, z = MR.sample_points(n, origin, spacing)
        want = MR.mesh_sdf(*mesh, n, origin, spacing, 1.75)
        got = F.meshSDF(*mesh, n, origin, spacing, 1.75).cpu().numpy()
        off = np.abs(want) > 1e-9  # (as on the CPU: the samples off the surface)
        assert np.array_equal(got[off] < 0, member[off]), name
        assert _ulps(got[off], want[off].astype(np.float32)) <= 4, name
        assert np.abs(got[~off]).max() <= 1e-12 and (~off).sum() > 20


@pytest.mark.gpu
def test_triangle_order_vertex_turns_and_repeats_give_the_same_bits():
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    rng = np.random.default_rng(11)
    for name, n in (("icosphere", GRIDS[1]), ("shell", GRIDS[0])):
        v, t = meshes()[name]
        origin = grid_origin((v, t), n)
        first = F.meshSDF(v, t, n, origin, SPACING, BAND)
        assert torch.equal(first, F.meshSDF(v, t, n, origin, SPACING, BAND))
        assert torch.equal(first, F.meshSDF(v, t[rng.permutation(len(t))], n, origin, SPACING, BAND))
        for turn in (1, 2):
            assert torch.equal(first, F.meshSDF(v, np.roll(t, turn, axis=1), n, origin, SPACING, BAND))
        turns = rng.integers(0, 3, len(t))
        mixed = np.stack([t[np.arange(len(t)), (turns + q) % 3] for q in range(3)], axis=1)
        assert torch.equal(first, F.meshSDF(v, mixed[rng.permutation(len(t))], n, origin, SPACING, BAND))
        assert int((first < 0).sum()) > 20


BOX_HALF = np.array([5.0 + np.sqrt(2.0) / 4, 3.0 + np.sqrt(3.0) / 9, 2.5 + np.sqrt(5.0) / 8])


@pytest.mark.gpu
@pytest.mark.parametrize("min_open", [0.0, 0.05])
def test_a_mesh_body_through_the_rasteriser(min_open):
    """BodyShape.mesh of a rotated box on section 18's grid against raster_reference.rasterize fed with a GRID body that holds the
    device's own samples, under section 18's bounds and after its generic-position asserts"""
    import test_raster_bodies as T

    from geometricmultigridpressuresolver_amd import fields as F

    centre = (17.0 + np.sqrt(3.0) / 3, 11.0 + np.sqrt(5.0) / 7, 9.0 + np.sqrt(2.0) / 5)
    R, spacing, band = RR.rotation((1.0, 2.0, 3.0), 0.7), 0.5, 3.0
    mesh = MR.box(-BOX_HALF, BOX_HALF)
    shape = F.BodyShape.mesh(centre, *mesh, spacing, band + np.sqrt(3.0) * spacing, R)
    n, origin = MR.sample_box(mesh[0], spacing, band + np.sqrt(3.0) * spacing)
    assert (shape.nx, shape.ny, shape.nz) == n and np.array_equal(shape.origin[:], origin)
    volume, com, inertia = shape.mass_properties
    assert abs(volume - 8 * BOX_HALF.prod()) <= 1e-12 * volume and np.abs(com).max() <= 1e-12
    samples = shape._keep.cpu().numpy()
    assert samples.min() < -2.0 and samples.max() == np.float32(band + np.sqrt(3.0) * spacing)
    body = RR.sdf_grid(centre, samples, origin, spacing, R)
    T.assert_decisions_are_not_round_off(T.GRID, [body], band)
    sphi, scw = T.walls(T.GRID)
    want = RR.rasterize(T.GRID, [body], band, min_open, sphi, scw)
    assert all((b == 1).sum() > 50 for b in want[2])
    T.assert_parity(F.rasterizeBodies(T.GRID, [shape], band, min_open, T._dev(sphi), [T._dev(w) for w in scw]), want, f"mesh body min_open={min_open}")


@pytest.mark.gpu
def test_rasterise_project_move_with_a_mesh_box():
    """Section 18's pool with the floating rotated box given as a 12-triangle mesh, K from meshMassProperties at half the liquid's
    density: through project_free_surface_rigid, moved by V_out, and again.  The divergence against V_out is at most 4 x what the
    kinematic projection leaves against V* (section 17's bound).  Printed beside it, with no threshold: the difference of V_out and of
    the coupled-cell count from the same scene with BodyShape.box (what the trilinear sampling near the box's edges costs)."""
    import test_raster_bodies as TR
    import test_rigid_coupling as T

    from geometricmultigridpressuresolver_amd import fields as F

    shape = T.POOL
    gz, gy, gx = shape
    k = np.arange(gz, dtype=np.float32)[:, None, None] + np.zeros(shape, dtype=np.float32)
    liquid_phi = ((k + 0.5) - 22.3).astype(np.float32) / max(shape)
    _, scw = TR.walls(shape)
    scw[0][:] = np.where(scw[0] == np.float32(0.4), np.float32(1.0), scw[0])  # (closed walls only)
    scw_dev = [TR._dev(w) for w in scw]
    rng = np.random.default_rng(5)
    velocity = [(rng.random(w.shape) * 2 - 1).astype(np.float32) for w in scw]
    half, spacing, band = np.array([9.7, 8.2, 6.4]), 0.5, 3.0
    mesh = MR.box(-half, half)
    volume, com, inertia = F.meshMassProperties(*mesh)
    assert abs(volume - 8 * half.prod()) <= 1e-12 * volume
    motions = T._motions(1, 51)
    out = {}
    for kind in ("mesh", "box"):
        centre, R = np.array([20.3, 16.2, 17.1]), RR.rotation((0.3, 1.0, 0.2), 0.12)
        out[kind] = []
        for step in range(2):
            if kind == "mesh":
                body_shape = F.BodyShape.mesh(centre, *mesh, spacing, band + np.sqrt(3.0) * spacing, R)
            else:
                body_shape = F.BodyShape.box(centre, half, R)
            solid_phi, cw, body = F.rasterizeBodies(shape, [body_shape], band, 0.05, None, scw_dev)
            centres, inv_mass, inv_inertia = np.zeros((2, 3)), np.zeros(2), np.zeros((2, 6))
            centres[1] = centre + R @ com
            inv_mass[1] = 1.0 / (0.5 * volume)
            m = R @ np.linalg.inv(0.5 * inertia) @ R.T  # the world-frame inverse inertia R I^-1 R^T
            inv_inertia[1] = [m[0, 0], m[1, 1], m[2, 2], m[0, 1], m[0, 2], m[1, 2]]
            c = dict(shape=shape, liquid_phi=liquid_phi, solid_phi=solid_phi.cpu().numpy(), cut_weights=[t.cpu().numpy() for t in cw],
                     velocity=velocity, body=[t.cpu().numpy() for t in body], centres=centres, inv_mass=inv_mass, inv_inertia=inv_inertia, motions=motions)
            kin, _, info0 = T._projection(c, False)
            end, star, info = T._projection(c, True)
            print(f"{kind} step {step}: max divergence {end:.3e} against rigidVelocity(V_out), {kin:.3e} left by the kinematic projection (bound 4 x), "
                  f"{star:.3e} against V*; coupled cells {info['coupled_cells']}, iterations {info['stats']['iterations']} / {info0['stats']['iterations']}")
            assert info["stats"]["outcome"] == "converged" and info["coupled_cells"] > 300
            assert end <= 4 * kin
            v = info["motions"][1]
            out[kind].append((v.copy(), info["coupled_cells"]))
            centre = centre + v[:3]
            angle = float(np.linalg.norm(v[3:]))
            R = (RR.rotation(v[3:], angle) if angle > 0 else np.eye(3)) @ R
            assert np.abs(v).sum() > 0
    for step in range(2):
        (vm, cm), (vb, cb) = out["mesh"][step], out["box"][step]
        print(f"step {step}: |V_out(mesh) - V_out(box)|_inf = {np.abs(vm - vb).max():.3e} of |V_out|_inf = {np.abs(vb).max():.3e}; coupled cells {cm} (mesh) {cb} (box)")
