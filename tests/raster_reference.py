"""The definition of the rigid-body rasterisation (include/mgps_fields.h, "rigid bodies rasterised") restated
in numpy fp64: the yardstick of tests/test_raster_bodies.py.  Grids are (nz, ny, nx) arrays, x fastest; positions, centres, half
extents and origins are in (x, y, z) order, in cells from the grid's corner."""
from collections import namedtuple

import numpy as np

SPHERE, BOX, GRID = 0, 1, 2

# rotation: 3 x 3, body -> world; sdf: float32 (nz, ny, nx) body-frame samples (GRID); half[0] is the radius of a SPHERE
Shape = namedtuple("Shape", "kind centre rotation half sdf origin spacing")


def sphere(centre, radius):
    return Shape(SPHERE, np.asarray(centre, float), np.eye(3), np.array([radius, 0.0, 0.0]), None, np.zeros(3), 0.0)


def box(centre, half, rotation=None):
    return Shape(BOX, np.asarray(centre, float), np.eye(3) if rotation is None else np.asarray(rotation, float), np.asarray(half, float), None,
                 np.zeros(3), 0.0)


def sdf_grid(centre, sdf, origin, spacing, rotation=None):
    return Shape(GRID, np.asarray(centre, float), np.eye(3) if rotation is None else np.asarray(rotation, float), np.zeros(3),
                 np.ascontiguousarray(sdf, dtype=np.float32), np.asarray(origin, float), float(spacing))


def rotation(axis, angle):
    """the rotation by `angle` about the unit vector along `axis` (Rodrigues)"""
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def box_sdf(p, half):
    """the BOX formula at body-frame points p = (px, py, pz)"""
    q = [np.abs(p[a]) - half[a] for a in range(3)]
    out = np.sqrt(sum(np.maximum(q[a], 0.0) ** 2 for a in range(3)))
    return out + np.minimum(np.maximum(q[0], np.maximum(q[1], q[2])), 0.0)


def reach_box(s, band):
    """(lo, hi): the world AABB of the frame box, grown by band"""
    mid = np.zeros(3)
    if s.kind == SPHERE:
        h = np.full(3, s.half[0])
    elif s.kind == BOX:
        h = np.asarray(s.half, float)
    else:
        n = np.array(s.sdf.shape[::-1], float)
        h = 0.5 * (n - 1) * s.spacing
        mid = s.origin + h
    c = s.centre + s.rotation @ mid
    e = np.abs(s.rotation) @ h + band
    return c - e, c + e


def contribution(s, band, x, y, z):
    """min(sdf, band) inside the reach box (bounds included), band outside"""
    lo, hi = reach_box(s, band)
    inside = (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (z >= lo[2]) & (z <= hi[2])
    d = [x - s.centre[0], y - s.centre[1], z - s.centre[2]]
    R = s.rotation
    p = [R[0, a] * d[0] + R[1, a] * d[1] + R[2, a] * d[2] for a in range(3)]  # R^T (x - centre)
    if s.kind == SPHERE:
        sdf = np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) - s.half[0]
    elif s.kind == BOX:
        sdf = box_sdf(p, s.half)
    else:
        n = s.sdf.shape[::-1]
        i0, f, out2 = [], [], 0.0
        for a in range(3):
            top = float(n[a] - 1)
            g = np.minimum(np.maximum((p[a] - s.origin[a]) / s.spacing, 0.0), top)
            i = np.minimum(np.floor(g).astype(np.int64), n[a] - 2)
            i0.append(i)
            f.append(g - i)
            lo_a, hi_a = s.origin[a], s.origin[a] + top * s.spacing
            e = np.maximum(np.maximum(lo_a - p[a], p[a] - hi_a), 0.0)
            out2 = out2 + e * e
        v = s.sdf.astype(np.float64)
        lerp = lambda t, u, w: (1.0 - t) * u + t * w  # noqa: E731
        at = lambda dz, dy, dx: v[i0[2] + dz, i0[1] + dy, i0[0] + dx]  # noqa: E731
        x00, x10 = lerp(f[0], at(0, 0, 0), at(0, 0, 1)), lerp(f[0], at(0, 1, 0), at(0, 1, 1))
        x01, x11 = lerp(f[0], at(1, 0, 0), at(1, 0, 1)), lerp(f[0], at(1, 1, 0), at(1, 1, 1))
        sdf = lerp(f[2], lerp(f[1], x00, x10), lerp(f[1], x01, x11)) + np.sqrt(out2)
    return np.where(inside, np.minimum(sdf, band), band)


def field(shapes, band, x, y, z, every=False):
    """(phi, owner): min(band, min_r contribution_r), and the lowest r that attains it below band (0: none).  every: also the stack of
    the contributions, (bodies, ...)"""
    phi = np.full(np.broadcast(x, y, z).shape, float(band))
    owner = np.zeros(phi.shape, dtype=np.int32)
    stack = []
    for r, s in enumerate(shapes, start=1):
        v = contribution(s, band, x, y, z)
        if every:
            stack.append(v)
        take = v < phi
        phi = np.where(take, v, phi)
        owner = np.where(take, r, owner)
    return (phi, owner, np.array(stack)) if every else (phi, owner)


def _points(gshape, offset, k0):
    gz, gy, gx = gshape
    z, y, x = np.meshgrid(np.arange(gz, dtype=float) + k0 + offset, np.arange(gy, dtype=float) + offset, np.arange(gx, dtype=float) + offset,
                          indexing="ij")
    return x, y, z


def node_field(gshape, shapes, band, k0=0, every=False):
    """the node field of the cells `gshape` = (gz, gy, gx): arrays (gz + 1, gy + 1, gx + 1); k0: the whole grid's plane of plane 0"""
    gz, gy, gx = gshape
    return field(shapes, band, *_points((gz + 1, gy + 1, gx + 1), 0.0, k0), every=every)


def open_fraction(p):
    """w_b in fp64 from the four corners' phi in cyclic order (0,0), (1,0), (1,1), (0,1), before the snap: the running shoelace sum over
    the corners with phi >= 0 and the crossings at t = phi_a / (phi_a - phi_b)"""
    cx, cy = (0.0, 1.0, 1.0, 0.0), (0.0, 0.0, 1.0, 1.0)
    shape = p[0].shape
    first_x, first_y, prev_x, prev_y, twice = (np.zeros(shape) for _ in range(5))
    nv = np.zeros(shape, dtype=np.int32)

    def vertex(on, x, y):
        nonlocal first_x, first_y, prev_x, prev_y, twice, nv
        start = on & (nv == 0)
        first_x, first_y = np.where(start, x, first_x), np.where(start, y, first_y)
        twice = np.where(on & (nv > 0), twice + (prev_x * y - x * prev_y), twice)
        prev_x, prev_y = np.where(on, x, prev_x), np.where(on, y, prev_y)
        nv = nv + on

    with np.errstate(divide="ignore", invalid="ignore"):
        for e in range(4):
            n = (e + 1) % 4
            ina, inb = p[e] >= 0.0, p[n] >= 0.0
            vertex(ina, np.full(shape, cx[e]), np.full(shape, cy[e]))
            t = p[e] / (p[e] - p[n])
            vertex(ina != inb, cx[e] + t * (cx[n] - cx[e]), cy[e] + t * (cy[n] - cy[e]))
    twice = np.where(nv > 0, twice + (prev_x * first_y - first_x * prev_y), twice)
    return np.minimum(np.maximum(0.5 * twice, 0.0), 1.0)


def face_corners(a, axis):
    """the four corner views, in cyclic order, of the faces of `axis` from a node array (gz + 1, gy + 1, gx + 1): in-plane axes u < v,
    corners (0,0), (1,0), (1,1), (0,1) in (u, v)"""
    u, v = [q for q in range(3) if q != axis]
    views = []
    for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
        sl = [slice(None)] * 3
        for q, d in ((u, du), (v, dv)):
            n = a.shape[2 - q]
            sl[2 - q] = slice(d, n - 1 + d)
        views.append(a[tuple(sl)])
    return views


def faces(phi_n, owner_n, axis, min_open):
    """(w_b after the snap in fp64, float32 weight, body id) of the faces of `axis`"""
    p, o = face_corners(phi_n, axis), face_corners(owner_n, axis)
    w = open_fraction(p)
    w = np.where(w < min_open, 0.0, w)
    w = np.where(w > 1.0 - min_open, 1.0, w)
    least, who = p[0], o[0]
    for e in range(1, 4):
        take = p[e] < least
        least, who = np.where(take, p[e], least), np.where(take, o[e], who)
    w32 = w.astype(np.float32)
    return w, w32, np.where(w32 < np.float32(1.0), who, 0).astype(np.int32)


def rasterize(gshape, shapes, band=3.0, min_open=0.0, static_solid_phi=None, static_cut_weights=None, k0=0):
    """(solid_phi, cut_weights[3], body[3]) of the planes k0 .. k0 + gz - 1 of a grid: float32, float32, int32"""
    phi_n, owner_n = node_field(gshape, shapes, band, k0)
    phi_c, _ = field(shapes, band, *_points(gshape, 0.5, k0))
    solid = phi_c.astype(np.float32)
    if static_solid_phi is not None:
        solid = np.minimum(static_solid_phi.astype(np.float32), solid)
    cw, body = [], []
    for a in range(3):
        _, w32, b = faces(phi_n, owner_n, a, min_open)
        cw.append(np.minimum(static_cut_weights[a].astype(np.float32), w32) if static_cut_weights is not None else w32)
        body.append(b)
    return solid, cw, body
