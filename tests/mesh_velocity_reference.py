"""The definition of the deforming-collider passes (include/mgps_fields.h, "deforming mesh colliders") restated
in numpy fp64: the yardstick of tests/test_mesh_velocity.py.  Brute force over all triangles: per triangle the squared distance
(mesh_reference.point_triangle2, section 19's), the weights of the closest point and the point itself; the winner rule; and the rule
that carries a GRID body's velocity samples to the solid-velocity face grids.  Conventions as in mesh_reference and raster_reference."""
import numpy as np

import mesh_reference as MR


# ---- the closest point of one triangle -----------------------------------------------------------------------------------------------
def closest_weights(a, b, c, x, y, z):
    """(wa, wb, wc) of the closest point of the triangle (a, b, c) to the points (x, y, z): the region tests of point_triangle2, in its
    order (vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, face)"""
    ab, ac = b - a, c - a
    ap, bp, cp = (x - a[0], y - a[1], z - a[2]), (x - b[0], y - b[1], z - b[2]), (x - c[0], y - c[1], z - c[2])
    dot = MR._dot
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    one, zero = np.ones(np.shape(d1)), np.zeros(np.shape(d1))
    with np.errstate(divide="ignore", invalid="ignore"):
        va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
        den = (va + vb) + vc
        wb, wc = vb / den, vc / den
        w = [(1.0 - wb) - wc, wb, wc]
        # (applied last to first, so that the first region that holds wins, as in the device's chain of returns)
        t = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        w = _where((d3 * d6 - d5 * d4 <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), [zero, 1.0 - t, t], w)
        t = d2 / (d2 - d6)
        w = _where((d5 * d2 - d1 * d6 <= 0) & (d2 >= 0) & (d6 <= 0), [1.0 - t, zero, t], w)
        w = _where((d6 >= 0) & (d5 <= d6), [zero, zero, one], w)
        t = d1 / (d1 - d3)
        w = _where((d1 * d4 - d3 * d2 <= 0) & (d1 >= 0) & (d3 <= 0), [1.0 - t, t, zero], w)
    w = _where((d3 >= 0) & (d4 <= d3), [zero, one, zero], w)
    return _where((d1 <= 0) & (d2 <= 0), [one, zero, zero], w)


def _where(take, new, old):
    return [np.where(take, n, o) for n, o in zip(new, old)]


def per_triangle(vertices, triangles, x, y, z):
    """(turned (T, 3), d2 (T, ...), weights (T, 3, ...), closest points (T, 3, ...)) with the triangles turned (lowest index first)
    and sorted by their index triple"""
    v = np.asarray(vertices, float)
    t = MR.turned(triangles)
    t = t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]
    d2, w, q = [], [], []
    for ia, ib, ic in t:
        a, b, c = v[ia], v[ib], v[ic]
        d2.append(MR.point_triangle2(a, b, c, x, y, z))
        wt = closest_weights(a, b, c, x, y, z)
        w.append(wt)
        q.append([wt[0] * a[m] + wt[1] * b[m] + wt[2] * c[m] for m in range(3)])
    return t, np.array(d2), np.array(w), np.array(q)


def winners(d2):
    """the index (into the sorted triangles) of the least (d2, v0, v1, v2): argmin returns the first of equal minima, and the
    triangles are in the order of their triples"""
    return np.argmin(d2, axis=0)


def _pick(a, win):
    """a[win[s], ..., s] for an array (T, m, ...) or (T, ...)"""
    idx = np.expand_dims(win, 0)
    if a.ndim == win.ndim + 2:
        return np.take_along_axis(a, np.expand_dims(idx, 1).repeat(a.shape[1], axis=1), axis=0)[0]
    return np.take_along_axis(a, idx, axis=0)[0]


def interpolate(tri, w, win, vertex_velocities):
    """(3, ...): (wa V_a + wb V_b) + wc V_c of the winner"""
    V = np.asarray(vertex_velocities, float)
    ww = _pick(w, win)
    corners = tri[win]  # (..., 3)
    return np.array([(ww[0] * V[corners[..., 0], c] + ww[1] * V[corners[..., 1], c]) + ww[2] * V[corners[..., 2], c] for c in range(3)])


def sample_velocity(vertices, triangles, vertex_velocities, n, origin, spacing, band):
    """The samples of the definition in fp64: (vel (3, nz, ny, nx), d (nz, ny, nx), details).  details: `ambiguous`, the number of
    in-band samples with a candidate triangle (d2_T <= d2_min + 1e-12 L^2, L the largest |coordinate|) whose closest point lies more
    than 0.5e-6 from the winner's (two candidates 1e-6 apart put at least one of them that far from the winner), `fan`, the largest
    number of candidates of one sample, and `point`, the winner's closest point (3, nz, ny, nx)"""
    x, y, z = MR.sample_points(n, origin, spacing)
    tri, d2, w, q = per_triangle(vertices, triangles, x, y, z)
    win = winners(d2)
    least = d2.min(axis=0)
    d = np.sqrt(least)
    vel = np.where(d < band, interpolate(tri, w, win, vertex_velocities), 0.0)
    L = np.abs(np.asarray(vertices, float)).max()
    cand = d2 <= least + 1e-12 * L * L
    point = _pick(q, win)
    apart = np.sqrt(((q - point[None]) ** 2).sum(axis=1))
    ambiguous = int(((cand & (apart > 0.5e-6)).any(axis=0) & (d < band)).sum())
    return vel, d, dict(ambiguous=ambiguous, fan=int(cand.sum(axis=0)[d < band].max()) if (d < band).any() else 0, point=point, winner=win,
                        triangles=tri, d2=d2, weights=w)


# ---- the samples on the face grids ---------------------------------------------------------------------------------------------------
def face_positions(gshape, axis, k0=0):
    """(x, y, z) of the faces of `axis` of the cells `gshape` = (gz, gy, gx): the face's own coordinate is an integer, the others + 1/2"""
    s = list(gshape)
    s[2 - axis] += 1
    off = [0.5, 0.5, 0.5]
    off[axis] = 0.0
    z, y, x = np.meshgrid(np.arange(s[0], dtype=float) + k0 + off[2], np.arange(s[1], dtype=float) + off[1], np.arange(s[2], dtype=float) + off[0],
                          indexing="ij")
    return x, y, z


def face_velocity(gshape, ids, shapes, samples, motions, k0=0):
    """The face rule in fp64.  ids: three int32 face grids; shapes: raster_reference.Shape per body (body r is shapes[r - 1]);
    samples: per body a float32 (3, nz, ny, nx) array or None; motions: (bodies, 6).  Returns per axis (mask of the faces the pass
    writes, the value in fp64 where the mask holds, the sum of the absolute values of the terms there)"""
    out = []
    for axis in range(3):
        pos = face_positions(gshape, axis, k0)
        mask = np.zeros(ids[axis].shape, dtype=bool)
        value, terms = np.zeros(ids[axis].shape), np.zeros(ids[axis].shape)
        for r, (s, vel) in enumerate(zip(shapes, samples), start=1):
            if vel is None:
                continue
            mine = ids[axis] == r
            if not mine.any():
                continue
            R = s.rotation
            d = [pos[m][mine] - s.centre[m] for m in range(3)]
            p = [R[0, m] * d[0] + R[1, m] * d[1] + R[2, m] * d[2] for m in range(3)]  # R^T (x - centre)
            n = vel.shape[:0:-1]  # (nx, ny, nz)
            i0, f = [], []
            for m in range(3):
                g = np.minimum(np.maximum((p[m] - s.origin[m]) / s.spacing, 0.0), float(n[m] - 1))
                i = np.minimum(np.floor(g).astype(np.int64), n[m] - 2)
                i0.append(i)
                f.append(g - i)
            lerp = lambda t, u, w: (1.0 - t) * u + t * w  # noqa: E731
            u = []
            for c in range(3):
                v = vel[c].astype(np.float64)
                at = lambda dz, dy, dx: v[i0[2] + dz, i0[1] + dy, i0[0] + dx]  # noqa: E731
                x00, x10 = lerp(f[0], at(0, 0, 0), at(0, 0, 1)), lerp(f[0], at(0, 1, 0), at(0, 1, 1))
                x01, x11 = lerp(f[0], at(1, 0, 0), at(1, 0, 1)), lerp(f[0], at(1, 1, 0), at(1, 1, 1))
                u.append(lerp(f[2], lerp(f[1], x00, x10), lerp(f[1], x01, x11)))
            U, w = motions[r - 1][:3], motions[r - 1][3:]
            a, b = (axis + 1) % 3, (axis + 2) % 3
            turned = [R[axis, 0] * u[0], R[axis, 1] * u[1], R[axis, 2] * u[2]]
            frame = [U[axis] + 0.0 * d[0], w[a] * d[b], w[b] * d[a]]
            value[mine] = ((turned[0] + turned[1]) + turned[2]) + (frame[0] + frame[1] - frame[2])
            terms[mine] = sum(np.abs(q) for q in turned + frame)
            mask |= mine
        out.append((mask, value, terms))
    return out
