"""Rigid bodies rasterised on the device (include/mgps_fields.h) against tests/raster_reference.py.

CPU: the restatement gives the exact open area of a planar solid (axis-aligned and tilted) and symmetric weights for a sphere on a
node; the C ABI refuses bad arguments on the host and the ctypes mirror has the library's size.
GPU: parity with the restatement on a sphere, a rotated box and a sampled SDF (with and without static walls, min_open 0 and 0.05),
255 bodies on one tile's list, slab windows against the whole grid, determinism, and two sub-steps of rasterise -> coupled
projection -> move the body.

Tolerances (parity).  Both sides form every value in fp64 and round to float32 once, so solid_phi may differ by the rounding of two
fp64 values a few 1e-16 apart: at most 4 float32 ulps (the bound of the issue; 1 is expected), and a weight by at most two float32
ulps at 1, 2.4e-7.  body and the sign of solid_phi are decisions; the test first asserts on the restatement that they are not
round-off: no node and no cell centre with |phi| < 1e-9, no two bodies within 1e-9 of each other at a node where both are below
band.  The cell-centre condition is this file's addition: the sign of solid_phi is decided there, not at the nodes."""
import ctypes as C
import functools

import numpy as np
import pytest

import raster_reference as RR
from refusals import refused as _refused

GRID = (19, 22, 37)  # (gz, gy, gx): off every multiple of the 64 x 4 x 4 tile
TILE = (4, 4, 64)


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trio():
    """a sphere, a rotated box and a 12^3 sample of a rotated box's SDF; irrational offsets; sphere and grid body closer than band"""
    s2, s3, s5 = np.sqrt(2.0), np.sqrt(3.0), np.sqrt(5.0)
    inner = RR.rotation((1.0, -1.0, 0.5), 0.4)
    n, h = 12, 0.75
    origin = -0.5 * (n - 1) * h * np.ones(3)
    k, j, i = np.meshgrid(*(origin[0] + h * np.arange(n),) * 3, indexing="ij")
    p = [inner[0, a] * i + inner[1, a] * j + inner[2, a] * k for a in range(3)]
    samples = RR.box_sdf(p, (2.5, 2.0, 1.5)).astype(np.float32)
    return (RR.sphere((7.0 + s2, 9.0 + s3 / 2, 8.0 + s5 / 3), 3.0 + s2 / 3),
            RR.box((25.0 + s3 / 3, 11.0 + s5 / 7, 9.0 + s2 / 5), (5.0 + s2 / 4, 3.0 + s3 / 9, 2.5 + s5 / 8), RR.rotation((1.0, 2.0, 3.0), 0.7)),
            RR.sdf_grid((16.0 + s5 / 3, 8.0 + s2 / 9, 7.0 + s3 / 5), samples, origin, h, RR.rotation((-2.0, 1.0, 1.0), 1.1)))


def walls(shape):
    """static solids: closed faces on the grid's boundary, and an SDF that is positive inside (a floor slab below plane 1.5)"""
    gz, gy, gx = shape
    k = np.arange(gz, dtype=np.float32)[:, None, None] + np.zeros(shape, dtype=np.float32)
    phi = (k + 0.5 - 1.5).astype(np.float32)
    cw = []
    for a in range(3):
        s = list(shape)
        s[2 - a] += 1
        w = np.ones(s, dtype=np.float32)
        sl = [slice(None)] * 3
        for end in (0, shape[2 - a]):
            sl[2 - a] = end
            w[tuple(sl)] = 0.0
        cw.append(w)
    cw[0][:, :, 1:-1] = np.where(k[:, :, :-1] < 1, np.float32(0.4), cw[0][:, :, 1:-1])  # part-open static faces along the floor
    return phi, cw


def assert_decisions_are_not_round_off(shape, shapes, band):
    phi_n, _, every = RR.node_field(shape, shapes, band, every=True)
    assert np.abs(phi_n).min() >= 1e-9
    if len(shapes) > 1:
        two = np.sort(every, axis=0)[:2]
        both = two[1] < band
        assert (two[1] - two[0])[both].min() >= 1e-9
    phi_c, _ = RR.field(shapes, band, *RR._points(shape, 0.5, 0))
    assert np.abs(phi_c).min() >= 1e-9


def _ulps(a, b):
    def ordered(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    return np.abs(ordered(a) - ordered(b)).max()


# ---- CPU: the restatement ------------------------------------------------------------------------------------------------------------
def _clipped_area(c, normal, point, axis):
    """area of {x in the unit face at corner c: normal . (x - point) >= 0} by Sutherland-Hodgman on the square, in scalar Python"""
    u, v = [q for q in range(3) if q != axis]
    square = []
    for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
        x = np.array(c, float)
        x[u] += du
        x[v] += dv
        square.append(x)
    val = [float(normal @ (x - point)) for x in square]
    poly = []
    for e in range(4):
        n = (e + 1) % 4
        if val[e] >= 0:
            poly.append(square[e])
        if (val[e] >= 0) != (val[n] >= 0):
            poly.append(square[e] + val[e] / (val[e] - val[n]) * (square[n] - square[e]))
    if not poly:
        return 0.0
    pu, pv = np.array([x[u] for x in poly]), np.array([x[v] for x in poly])
    return 0.5 * abs(float(np.sum(pu * np.roll(pv, -1) - np.roll(pu, -1) * pv)))


@pytest.mark.parametrize("angle", [0.0, 0.31])
def test_planar_solid_gives_the_exact_open_area(angle):
    """one large BOX whose top face crosses a 12 x 10 x 8 grid at a fractional height, axis-aligned and tilted about x: every face's
    w_b is the area of the face above the plane, to 1e-12"""
    shape = (8, 10, 12)
    R = RR.rotation((1.0, 0.0, 0.0), angle)
    point, hz = np.array([6.0, 5.0, 3.37]), 50.0
    solid = RR.box(point - R @ np.array([0.0, 0.0, hz]), (100.0, 100.0, hz), R)
    normal = R @ np.array([0.0, 0.0, 1.0])  # phi = normal . (x - point) near the top face
    phi_n, owner_n = RR.node_field(shape, [solid], 3.0)
    cut = 0
    for a in range(3):
        w, w32, body = RR.faces(phi_n, owner_n, a, 0.0)
        want = np.empty_like(w)
        for idx in np.ndindex(*w.shape):
            want[idx] = _clipped_area((idx[2], idx[1], idx[0]), normal, point, a)
        assert np.abs(w - want).max() <= 1e-12
        cut += int(((w > 0) & (w < 1)).sum())
        assert ((body == 1) == (w32 < 1)).all()
    assert cut > 200
    solid_phi, _, _ = RR.rasterize(shape, [solid])
    z, y, x = np.meshgrid(np.arange(8) + 0.5, np.arange(10) + 0.5, np.arange(12) + 0.5, indexing="ij")
    plane = normal[0] * (x - point[0]) + normal[1] * (y - point[1]) + normal[2] * (z - point[2])
    assert np.abs(solid_phi - np.minimum(plane, 3.0)).max() <= 2e-6  # (float32 roundings of values below 8)


def test_sphere_on_a_node_gives_symmetric_weights():
    shape = (8, 10, 12)
    ball = RR.sphere((6.0, 5.0, 4.0), 2.6)
    solid_phi, cw, body = RR.rasterize(shape, [ball], band=2.0)
    assert (solid_phi < 0).sum() > 40
    for a in range(3):
        assert ((cw[a] > 0) & (cw[a] < 1)).sum() > 20
        for flip in range(3):
            assert np.abs(cw[a] - np.flip(cw[a], axis=flip)).max() <= 1e-6, (a, flip)
            assert np.array_equal(body[a], np.flip(body[a], axis=flip))
    for flip in range(3):
        assert np.abs(solid_phi - np.flip(solid_phi, axis=flip)).max() <= 1e-6


def test_min_open_snaps_and_ties_go_to_the_lowest_id():
    shape = (6, 6, 6)
    a = RR.box((3.0, 3.0, 0.0), (10.0, 10.0, 2.03))
    same = RR.box((3.0, 3.0, 0.0), (10.0, 10.0, 2.03))
    phi_n, owner_n = RR.node_field(shape, [a, same], 2.0)
    assert set(np.unique(owner_n)) == {0, 1}  # never 2: the lowest id wins the tie
    raw = RR.faces(phi_n, owner_n, 0, 0.0)[0]
    snapped = RR.faces(phi_n, owner_n, 0, 0.05)[0]
    assert np.abs(raw[2] - 0.97).max() <= 1e-12 and (snapped[2] == 1.0).all()
    assert (RR.faces(phi_n, owner_n, 0, 0.05)[2][2] == 0).all() and (RR.faces(phi_n, owner_n, 0, 0.0)[2][2] == 1).all()


# ---- CPU: the C ABI refuses bad arguments on the host ----------------------------------------------------------------------------------
def _desc(shapes=None, **kw):
    from geometricmultigridpressuresolver_amd import fields as F

    shapes = [F.BodyShape.sphere((2, 2, 2), 1.0), F.BodyShape.box((2, 2, 2), (1, 1, 1))] if shapes is None else shapes
    rows = (F.BodyShape * (len(shapes) + 1))(F.BodyShape(), *shapes)
    d = F.RasterDesc()
    d.struct_size = C.sizeof(F.RasterDesc)
    d.gx = d.gy = d.gz = 4
    d.bodies, d.shapes, d.band, d.min_open = len(shapes), rows, 3.0, 0.0
    d.solid_phi = 64  # (never dereferenced: every call below is refused on the host)
    for a in range(3):
        d.cut_weights[a] = d.body[a] = 64
    for k, v in kw.items():
        setattr(d, k, v)
    return d, rows


def test_argument_refusals_need_no_device_and_the_mirror_has_the_library_size():
    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd._lib import lib

    L = lib()
    whole = lambda d: L.mgps_fields_rasterize_bodies(C.byref(d), None)  # noqa: E731
    # the mirror's size is the library's: a good struct gets as far as the next check, one of another size is refused as such
    d, keep = _desc(bodies=0)
    _refused(whole(d), "mgps_fields_rasterize_bodies", "bodies", "1 .. 255")
    d.struct_size -= 4
    _refused(whole(d), "struct_size")
    _refused(L.mgps_fields_rasterize_bodies(None, None), "struct_size")
    # ... and so is the row's: the second row of a good table is read where the library expects it
    bad = F.BodyShape.box((2, 2, 2), (1, 1, 1))
    bad.kind = 7
    _refused(whole(_desc([F.BodyShape.sphere((2, 2, 2), 1.0), bad])[0]), "body 2", "kind")
    for bodies in (256, -1):
        _refused(whole(_desc(bodies=bodies)[0]), "bodies")
    for k in ("gx", "gy", "gz"):
        _refused(whole(_desc(**{k: 0})[0]), "extent")
    d, keep = _desc()
    d.shapes = C.POINTER(F.BodyShape)()
    _refused(whole(d), "shapes")
    s = F.BodyShape.sphere((2, 2, float("nan")), 1.0)
    _refused(whole(_desc([s])[0]), "body 1", "centre")
    s = F.BodyShape.box((2, 2, 2), (1, 1, 1), [[1, 0, 0], [0, float("inf"), 0], [0, 0, 1]])
    _refused(whole(_desc([s])[0]), "rotation")
    s = F.BodyShape.box((2, 2, 2), (1, 1, 1), [[1, 0, 0], [0, 1, 1e-5], [0, 0, 1]])
    _refused(whole(_desc([s])[0]), "orthonormal")
    s = F.BodyShape.box((2, 2, 2), (1, 1, 1), [[1, 0, 0], [0, 1, 1e-8], [0, 0, 1]])  # (inside the 1e-6 allowance: the next check speaks)
    _refused(whole(_desc([s], band=1.0)[0]), "band")
    _refused(whole(_desc([F.BodyShape.sphere((2, 2, 2), 0.0)])[0]), "radius")
    _refused(whole(_desc([F.BodyShape.box((2, 2, 2), (1, -1, 1))])[0]), "half extent")
    grid = F.BodyShape.box((2, 2, 2), (1, 1, 1))
    grid.kind, grid.sdf, grid.nx, grid.ny, grid.nz, grid.spacing = F.BODY_GRID, 64, 4, 4, 4, 0.5
    assert whole(_desc([grid], band=99.0)[0]) == 1 and "band" in L.mgps_last_error(None).decode()  # (a good GRID row passes)
    for name, value, word in (("sdf", None, "sdf"), ("ny", 1, "dimension"), ("spacing", 0.0, "spacing")):
        old = getattr(grid, name)
        setattr(grid, name, value)
        _refused(whole(_desc([grid])[0]), "body 1", word)
        setattr(grid, name, old)
    for band in (1.99, 16.5, float("nan")):
        _refused(whole(_desc(band=band)[0]), "band")
    for min_open in (-0.01, 0.5):
        _refused(whole(_desc(min_open=min_open)[0]), "min_open")
    _refused(whole(_desc(solid_phi=None)[0]), "solid_phi")
    for name, word in (("cut_weights", "cut_weights"), ("body", "body")):
        d, keep = _desc()
        getattr(d, name)[1] = None
        _refused(whole(d), word, "output")
    d, keep = _desc()
    d.static_cut_weights[0] = d.static_cut_weights[2] = 64
    _refused(whole(d), "static_cut_weights")
    # the window entry: the desc's refusals, then the window's
    slab = lambda w, d: L.mgps_fields_slab_rasterize_bodies(C.byref(w) if w is not None else None, C.byref(d), None)  # noqa: E731
    w = F.slab_window((32, 4, 4), True, F.projection_slab_layout((32, 4, 4), True, 2, False)["splits"], 0)
    _refused(slab(w, _desc(bodies=0)[0]), "mgps_fields_slab_rasterize_bodies", "bodies")
    _refused(slab(None, _desc(gz=32)[0]), "slab window")
    _refused(slab(w, _desc()[0]), "extents")  # (a window of 4 x 4 x 32, a desc of 4 x 4 x 4)
    w.c1 += 1
    _refused(slab(w, _desc(gz=32)[0]), "slab window")


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_shapes(shapes):
    from geometricmultigridpressuresolver_amd import fields as F

    out = []
    for s in shapes:
        if s.kind == RR.SPHERE:
            out.append(F.BodyShape.sphere(s.centre, s.half[0]))
        elif s.kind == RR.BOX:
            out.append(F.BodyShape.box(s.centre, s.half, s.rotation))
        else:
            out.append(F.BodyShape.sdf_grid(s.centre, _dev(s.sdf), s.origin, s.spacing, s.rotation))
    return out


def assert_parity(got, want, what):
    solid, cw, body = got
    solid, cw, body = solid.cpu().numpy(), [t.cpu().numpy() for t in cw], [t.cpu().numpy() for t in body]
    ulps = _ulps(solid, want[0])
    worst = max(float(np.abs(cw[a].astype(np.float64) - want[1][a]).max()) for a in range(3))
    print(f"{what}: solid_phi {ulps} ulps (bound 4), cut weights {worst:.2e} (bound 2.4e-7), owned faces {[int((b > 0).sum()) for b in body]}")
    for a in range(3):
        assert np.array_equal(body[a], want[2][a]), (what, a)
    assert np.array_equal(solid < 0, want[0] < 0)
    assert ulps <= 4
    assert worst <= 2.4e-7


@pytest.mark.gpu
@pytest.mark.parametrize("static", [False, True])
@pytest.mark.parametrize("min_open", [0.0, 0.05])
def test_device_pass_equals_the_restatement(static, min_open):
    from geometricmultigridpressuresolver_amd import fields as F

    shapes, band = trio(), 3.0
    assert_decisions_are_not_round_off(GRID, shapes, band)
    lo0, hi0 = RR.reach_box(shapes[0], 0.0)
    lo2, hi2 = RR.reach_box(shapes[2], 0.0)
    assert (np.maximum(lo0, lo2) - np.minimum(hi0, hi2)).max() < band  # two bodies closer than band
    sphi, scw = walls(GRID) if static else (None, None)
    want = RR.rasterize(GRID, shapes, band, min_open, sphi, scw)
    assert all(len(np.unique(b)) == 4 for b in want[2])  # every body owns faces of every axis
    got = F.rasterizeBodies(GRID, device_shapes(shapes), band, min_open, _dev(sphi) if static else None, [_dev(w) for w in scw] if static else None)
    assert_parity(got, want, f"trio static={static} min_open={min_open}")


@pytest.mark.gpu
@pytest.mark.parametrize("gx", [64, 65, 131])
def test_bodies_across_tiles_along_x(gx):
    """the tile is 64 cells long: a grid of exactly one tile, one of a tile and a single column (that column's cells write both their
    x-faces), and one of three tiles, with a box across every tile boundary and a sphere on the last one"""
    from geometricmultigridpressuresolver_amd import fields as F

    shape, band = (6, 9, gx), 2.0
    shapes = (RR.box((0.5 * gx + np.sqrt(2.0) / 7, 4.0 + np.sqrt(3.0) / 5, 3.0 + np.sqrt(5.0) / 9), (0.5 * gx - 2.3, 1.7, 1.2), RR.rotation((0.1, 0.2, 1.0), 0.02)),
              RR.sphere((gx - 1.0 - np.sqrt(2.0) / 3, 6.0 + np.sqrt(3.0) / 4, 2.0 + np.sqrt(5.0) / 6), 1.9))
    assert_decisions_are_not_round_off(shape, shapes, band)
    sphi, scw = walls(shape)
    want = RR.rasterize(shape, shapes, band, 0.0, sphi, scw)
    assert (want[2][0][:, :, gx - 1:] > 0).any() and (want[2][0][:, :, 60:min(70, gx)] == 1).any()
    assert_parity(F.rasterizeBodies(shape, device_shapes(shapes), band, 0.0, _dev(sphi), [_dev(w) for w in scw]), want, f"gx = {gx}")


@functools.lru_cache(maxsize=None)
def crowd():
    """255 spheres: 215 along a wavy line through the tile at the origin, 40 in a cluster at the far corner, all within band = 16 of
    the tile of cells [0, 64) x [0, 4) x [0, 4)"""
    out = []
    for r in range(215):
        out.append(RR.sphere((1.3 + 0.1741 * r, 2.0 + 0.9 * np.sin(1.1 * r + 0.3), 2.1 + 0.9 * np.cos(0.7 * r + 0.1)), 0.55 + 0.2 * np.sin(2.3 * r) ** 2))
    for r in range(40):
        out.append(RR.sphere((30.2 + 0.19 * r, 17.3 + 1.7 * np.sin(0.9 * r + 0.2), 17.9 + 1.6 * np.cos(1.3 * r + 0.5)), 0.7 + 0.25 * np.cos(1.7 * r) ** 2))
    return tuple(out)


@pytest.mark.gpu
def test_255_bodies_on_one_tile():
    from geometricmultigridpressuresolver_amd import fields as F

    shape, shapes, band = (24, 24, 40), crowd(), 16.0
    assert len(shapes) == 255
    for s in shapes:  # every reach box meets the node box of the tile at the origin
        lo, hi = RR.reach_box(s, band)
        assert (lo <= np.array([shape[2], TILE[1], TILE[0]])).all() and (hi >= 0).all()
    assert_decisions_are_not_round_off(shape, shapes, band)
    want = RR.rasterize(shape, shapes, band, 0.0)
    owners = np.unique(np.concatenate([b.reshape(-1) for b in want[2]]))
    assert owners.max() == 255 and len(owners) > 150
    assert_parity(F.rasterizeBodies(shape, device_shapes(shapes), band, 0.0), want, "255 spheres")


@pytest.mark.gpu
@pytest.mark.parametrize("size", [2, 3, "odd"])
def test_windows_equal_the_whole_grid(size):
    """2-way and 3-way cuts of the layout, and a cut of the caller's at base plane 21: a window whose tiles start off every multiple
    of the tile's 4 planes"""
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    shape = (48, 20, 24)
    shapes = device_shapes([RR.box((12.3, 9.6, 24.2), (4.1, 3.3, 15.2), RR.rotation((1.0, 0.3, 0.1), 0.25)), RR.sphere((6.1, 14.2, 40.3), 3.2)])
    sphi, scw = walls(shape)
    sphi, scw = _dev(sphi), [_dev(w) for w in scw]
    whole = F.rasterizeBodies(shape, shapes, 3.0, 0.03, sphi, scw)
    if size == "odd":
        lay = F.projection_slab_layout(shape, True, 2, False)
        size, splits = 2, [0, lay["offset"] + 21, lay["expanded"][0]]
    else:
        splits = F.projection_slab_layout(shape, True, size, False)["splits"]
    tops = []
    for rank in range(size):
        d = F.slab_window(shape, True, splits, rank)
        k = slice(d.c0, d.c1)
        solid, cw, body = F.rasterizeBodiesSlab(d, shapes, 3.0, 0.03, sphi[k].contiguous(), [scw[0][k].contiguous(), scw[1][k].contiguous(), scw[2][d.c0:d.c1 + 1].contiguous()])
        assert torch.equal(solid, whole[0][k])
        for a in range(3):
            ka = slice(d.c0, d.c1 + 1) if a == 2 else k
            assert torch.equal(cw[a], whole[1][a][ka]) and torch.equal(body[a], whole[2][a][ka])
        if rank > 0:  # both copies of the cut's z-face plane; a body straddles it
            below = tops.pop()
            assert torch.equal(below[0], cw[2][0]) and torch.equal(below[1], body[2][0])
            assert int((whole[2][0][d.c0 - 1] == 1).sum()) > 0 and int((whole[2][0][d.c0] == 1).sum()) > 0
        tops.append((cw[2][-1].clone(), body[2][-1].clone()))
    assert d.c1 == shape[0]


@pytest.mark.gpu
def test_two_calls_give_the_same_bits():
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    shapes = device_shapes(trio())
    sphi, scw = walls(GRID)
    sphi, scw = _dev(sphi), [_dev(w) for w in scw]
    first = F.rasterizeBodies(GRID, shapes, 3.0, 0.05, sphi, scw)
    second = F.rasterizeBodies(GRID, shapes, 3.0, 0.05, sphi, scw)
    assert torch.equal(first[0], second[0])
    for a in range(3):
        assert torch.equal(first[1][a], second[1][a]) and torch.equal(first[2][a], second[2][a])
    assert int((first[2][0] > 0).sum()) > 100


@pytest.mark.gpu
def test_rasterise_project_move_rasterise_project():
    """A pool with a floating box, rasterised on the device, through project_free_surface_rigid: the divergence against V_out meets the
    bound of test_projection_with_rigid_bodies_is_divergence_free_against_v_out (at most 4 x what the kinematic projection leaves
    against V*; that test's own _projection measures both).  Then the box moves by V_out (dt = 1), is rasterised again and projected
    again under the same bound."""
    import test_rigid_coupling as T

    from geometricmultigridpressuresolver_amd import fields as F

    shape = T.POOL
    gz, gy, gx = shape
    k = np.arange(gz, dtype=np.float32)[:, None, None] + np.zeros(shape, dtype=np.float32)
    liquid_phi = ((k + 0.5) - 22.3).astype(np.float32) / max(shape)
    _, scw = walls(shape)
    scw[0][:] = np.where(scw[0] == np.float32(0.4), np.float32(1.0), scw[0])  # (closed walls only)
    scw_dev = [_dev(w) for w in scw]
    rng = np.random.default_rng(5)
    velocity = [(rng.random(w.shape) * 2 - 1).astype(np.float32) for w in scw]
    centre, half, R = np.array([20.3, 16.2, 17.1]), np.array([9.7, 8.2, 6.4]), RR.rotation((0.3, 1.0, 0.2), 0.12)
    centres, inv_mass, inv_inertia = T._box_tables([(centre - half, centre + half)], [0.5])
    motions = T._motions(1, 51)
    for step in range(2):
        solid_phi, cw, body = F.rasterizeBodies(shape, [F.BodyShape.box(centre, half, R)], 3.0, 0.05, None, scw_dev)
        centres[1] = centre
        c = dict(shape=shape, liquid_phi=liquid_phi, solid_phi=solid_phi.cpu().numpy(), cut_weights=[t.cpu().numpy() for t in cw],
                 velocity=velocity, body=[t.cpu().numpy() for t in body], centres=centres, inv_mass=inv_mass, inv_inertia=inv_inertia, motions=motions)
        kin, _, info0 = T._projection(c, False)
        end, star, info = T._projection(c, True)
        print(f"step {step}: max divergence {end:.3e} against rigidVelocity(V_out), {kin:.3e} left by the kinematic projection (bound 4 x), "
              f"{star:.3e} against V*; coupled cells {info['coupled_cells']}, iterations {info['stats']['iterations']} / {info0['stats']['iterations']}")
        assert info["stats"]["outcome"] == "converged" and info["coupled_cells"] > 300
        assert end <= 4 * kin
        v = info["motions"][1]
        centre = centre + v[:3]
        angle = float(np.linalg.norm(v[3:]))
        R = (RR.rotation(v[3:], angle) if angle > 0 else np.eye(3)) @ R
        assert np.abs(v).sum() > 0
