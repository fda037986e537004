"""The definition of the triangle-mesh signed distance and mass properties (include/mgps_fields.h, "triangle-mesh rigid bodies";
DESIGN.md section 19) restated in numpy fp64: the yardstick of tests/test_mesh_bodies.py.  Brute force over all triangles.  Vertices
are (V, 3) float64 arrays in (x, y, z), triangles (T, 3) integer arrays of vertex indices, outward orientation; sample grids are
(nz, ny, nx) arrays, x fastest.  Also the small mesh builders the tests use."""
import itertools

import numpy as np


# ---- builders ------------------------------------------------------------------------------------------------------------------------
def _outward(vertices, triangles):
    """the triangles of a convex body about its vertex mean, each turned to point outward"""
    v, t = np.asarray(vertices, float), np.array(triangles, dtype=np.int32)
    mid = v.mean(axis=0)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    flip = np.einsum("ij,ij->i", np.cross(b - a, c - a), (a + b + c) / 3 - mid) < 0
    t[flip] = t[flip][:, ::-1]
    return v, t


def tetrahedron(edge=1.0):
    """regular, centred on the origin"""
    s = edge / (2 * np.sqrt(2.0))
    return _outward(s * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], float), [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])


def box(lo, hi):
    """12 triangles, vertex q at (lo or hi by bit 0, 1, 2 of q for x, y, z)"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    v = np.array([[(hi if q >> a & 1 else lo)[a] for a in range(3)] for q in range(8)])
    quads = [(0, 2, 6, 4), (1, 3, 7, 5), (0, 1, 5, 4), (2, 3, 7, 6), (0, 1, 3, 2), (4, 5, 7, 6)]
    return _outward(v, [tri for q in quads for tri in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])


def octahedron(radius=1.0):
    v = radius * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], float)
    return _outward(v, [(x, y, z) for x in (0, 1) for y in (2, 3) for z in (4, 5)])


def icosphere(radius=1.0, subdivisions=0):
    """an icosahedron's 20 faces, each split in four `subdivisions` times, the vertices on the sphere: 20 * 4^subdivisions triangles"""
    g = (1 + np.sqrt(5.0)) / 2
    v = [p for a, b in itertools.product((-1.0, 1.0), (-g, g)) for p in ((0.0, a, b), (a, b, 0.0), (b, 0.0, a))]
    v = np.array(v)
    near = lambda p, q: abs(np.linalg.norm(v[p] - v[q]) - 2.0) < 1e-9  # noqa: E731  (the edges have length 2)
    v, t = _outward(v, [f for f in itertools.combinations(range(12), 3) if near(f[0], f[1]) and near(f[1], f[2]) and near(f[0], f[2])])
    assert len(t) == 20
    v = [p / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, out = {}, []

        def middle(p, q):
            key = (min(p, q), max(p, q))
            if key not in mid:
                m = v[p] + v[q]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in t:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = out
    return radius * np.array(v), np.array(t, dtype=np.int32)


L_PRISM = dict(a=3.0, b=1.2, c=1.1, d=2.6, h=1.9)  # the L is [0, a] x [0, b] joined with [0, c] x [0, d], extruded over z in [0, h]


def l_prism(a=L_PRISM["a"], b=L_PRISM["b"], c=L_PRISM["c"], d=L_PRISM["d"], h=L_PRISM["h"]):
    poly = [(0, 0), (a, 0), (a, b), (c, b), (c, d), (0, d)]  # counter-clockwise; vertex 3 is the reflex corner
    v = np.array([(x, y, z) for z in (0.0, h) for x, y in poly], float)
    fan = [(3, 4, 5), (3, 5, 0), (3, 0, 1), (3, 1, 2)]
    t = [(p + 6, q + 6, r + 6) for p, q, r in fan] + [(r, q, p) for p, q, r in fan]
    for i in range(6):
        n = (i + 1) % 6
        t += [(i, n, n + 6), (i, n + 6, i + 6)]
    return v, np.array(t, dtype=np.int32)


def in_l_prism(x, y, z, a=L_PRISM["a"], b=L_PRISM["b"], c=L_PRISM["c"], d=L_PRISM["d"], h=L_PRISM["h"]):
    return (z > 0) & (z < h) & (x > 0) & (y > 0) & (((x < a) & (y < b)) | ((x < c) & (y < d)))


def merge(*meshes):
    """several shells as one mesh"""
    v, t, base = [], [], 0
    for mv, mt in meshes:
        v.append(np.asarray(mv, float))
        t.append(np.asarray(mt, dtype=np.int32) + base)
        base += len(mv)
    return np.concatenate(v), np.concatenate(t).astype(np.int32)


def flipped(mesh):
    return mesh[0], np.ascontiguousarray(np.asarray(mesh[1])[:, ::-1])


def shell(lo, hi, inner_lo, inner_hi):
    """a box with a smaller inward-oriented box inside it: solid shell, empty core"""
    return merge(box(lo, hi), flipped(box(inner_lo, inner_hi)))


def moved(mesh, rotation=None, shift=(0.0, 0.0, 0.0)):
    v = np.asarray(mesh[0], float)
    if rotation is not None:
        v = v @ np.asarray(rotation, float).T
    return v + np.asarray(shift, float), mesh[1]


# ---- distance ------------------------------------------------------------------------------------------------------------------------
def _dot(u, w):
    return u[0] * w[0] + u[1] * w[1] + u[2] * w[2]


def point_triangle2(a, b, c, x, y, z):
    """the squared distance from the points (x, y, z) to the triangle (a, b, c): the closest point's region by the signs of the
    projections onto the edges (vertex, edge or face), then the distance to that feature"""
    ab, ac, bc = b - a, c - a, c - b
    n = np.cross(ab, ac)
    ap, bp, cp = (x - a[0], y - a[1], z - a[2]), (x - b[0], y - b[1], z - b[2]), (x - c[0], y - c[1], z - c[2])
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    h = _dot(n, ap)
    out = h * h / _dot(n, n)

    def edge(start, along, w):
        r = [start[q] - w * along[q] for q in range(3)]
        return _dot(r, r)

    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where((d3 * d6 - d5 * d4 <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), edge(bp, bc, (d4 - d3) / ((d4 - d3) + (d5 - d6))), out)
        out = np.where((d5 * d2 - d1 * d6 <= 0) & (d2 >= 0) & (d6 <= 0), edge(ap, ac, d2 / (d2 - d6)), out)
        out = np.where((d6 >= 0) & (d5 <= d6), _dot(cp, cp), out)
        out = np.where((d1 * d4 - d3 * d2 <= 0) & (d1 >= 0) & (d3 <= 0), edge(ap, ab, d1 / (d1 - d3)), out)
    out = np.where((d3 >= 0) & (d4 <= d3), _dot(bp, bp), out)
    return np.where((d1 <= 0) & (d2 <= 0), _dot(ap, ap), out)


def distance(vertices, triangles, x, y, z):
    """d: the minimum over all triangles of the distance to the triangle"""
    v = np.asarray(vertices, float)
    best = np.full(np.broadcast(x, y, z).shape, np.inf)
    for t in np.asarray(triangles):
        best = np.minimum(best, point_triangle2(v[t[0]], v[t[1]], v[t[2]], x, y, z))
    return np.sqrt(best)


# ---- inside or outside ---------------------------------------------------------------------------------------------------------------
def _first_sign(*terms):
    """the sign of the first non-zero term"""
    out = np.zeros(np.broadcast(*terms).shape, dtype=np.int64)
    for term in reversed(terms):
        s = np.sign(term).astype(np.int64)
        out = np.where(s != 0, s, out)
    return out


def edge_function(v, ia, ib, sy, sz):
    """(e, its sign under the shift (sy + eps, sz + eps^2), the column's distance from the edge's line) of the projected edge
    ia -> ib: evaluated with the ends in ascending vertex index and negated when that swaps them"""
    p, q = (v[ia], v[ib]) if ia < ib else (v[ib], v[ia])
    dy, dz = q[1] - p[1], q[2] - p[2]
    e = dy * (sz - p[2]) - dz * (sy - p[1])
    sign = _first_sign(e, -dz, dy)
    length = np.hypot(dy, dz)
    gap = np.abs(e) / length if length > 0 else np.full(np.shape(e), np.inf)
    return (e, sign, gap) if ia < ib else (-e, -sign, gap)


def turned(triangles):
    """every triangle turned cyclically so that its lowest vertex index comes first"""
    t = np.asarray(triangles)
    first = np.argmin(t, axis=1)
    return np.stack([t[np.arange(len(t)), (first + q) % 3] for q in range(3)], axis=1)


def inside(vertices, triangles, x, y, z, gaps=False):
    """the parity of the crossings along +x: True inside.  gaps: also the least distance of a column from an edge's line"""
    v = np.asarray(vertices, float)
    odd = np.zeros(np.broadcast(x, y, z).shape, dtype=bool)
    least = np.inf
    for ia, ib, ic in turned(triangles):
        a, b, c = v[ia], v[ib], v[ic]
        ea, sa, ga = edge_function(v, ib, ic, y, z)
        eb, sb, gb = edge_function(v, ic, ia, y, z)
        ec, sc, gc = edge_function(v, ia, ib, y, z)
        least = min(least, float(np.min(ga)), float(np.min(gb)), float(np.min(gc)))
        area = (b[1] - a[1]) * (c[2] - a[2]) - (b[2] - a[2]) * (c[1] - a[1])
        total = (ea + eb) + ec
        crossed = (area != 0) & (sa != 0) & (sa == sb) & (sb == sc) & (total != 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            depth = ((ea * a[0] + eb * b[0]) + ec * c[0]) / total
        odd ^= crossed & (np.where(crossed, depth, -np.inf) > x)
    return (odd, least) if gaps else odd


# ---- the samples ---------------------------------------------------------------------------------------------------------------------
def sample_points(n, origin, spacing):
    """(x, y, z) arrays (nz, ny, nx) of the samples origin + spacing (i, j, k); n = (nx, ny, nz)"""
    axes = [origin[a] + spacing * np.arange(n[a], dtype=float) for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return x, y, z


def mesh_sdf(vertices, triangles, n, origin, spacing, band, details=False):
    """sigma min(d, band) in fp64 on the samples.  details: also (d, the least distance of a column from an edge's line)"""
    x, y, z = sample_points(n, origin, spacing)
    d = distance(vertices, triangles, x, y, z)
    odd, gap = inside(vertices, triangles, x, y, z, gaps=True)
    out = np.where(odd, -1.0, 1.0) * np.minimum(d, band)
    return (out, d, gap) if details else out


def sample_box(vertices, spacing, band):
    """((nx, ny, nz), origin): the samples that hold the bounding box grown by band + spacing"""
    v = np.asarray(vertices, float)
    origin = v.min(axis=0) - (band + spacing)
    steps = np.ceil((v.max(axis=0) + (band + spacing) - origin) / spacing)
    return tuple(int(max(s + 1, 2)) for s in steps), origin


# ---- mass properties -----------------------------------------------------------------------------------------------------------------
def mass_properties(vertices, triangles):
    """(volume, centre, inertia about the centre) for unit density from the signed tetrahedra (0, a, b, c): det = a . (b x c),
    V = det / 6, int x = det / 24 (a + b + c), int x_i x_j = det / 120 (sum over the corners of p_i p_j + S_i S_j), S = a + b + c"""
    v = np.asarray(vertices, float)
    t = np.asarray(triangles)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    det = np.einsum("ij,ij->i", a, np.cross(b, c))
    s = a + b + c
    volume = det.sum() / 6
    centre = (det[:, None] * s).sum(axis=0) / 24 / volume
    second = sum(np.einsum("t,ti,tj->ij", det, p, p) for p in (a, b, c, s)) / 120
    cov = second - volume * np.outer(centre, centre)
    return volume, centre, np.trace(cov) * np.eye(3) - cov
