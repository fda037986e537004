"""numpy fp64 restatement of the advection passes (include/mgps_fields.h, "advection"): sampling, trace, both
schemes, the window rule and both counters, written from the header's definition and vectorised over a grid's targets.

Arrays are (gz, gy, gx) with x fastest; points are (N, 3) in (x, y, z) order, in cells from the grid's corner.  Grid kinds: 0 cells,
1 + a the faces of axis a.  A window is (c0, c1, halo): the restatement reads the WHOLE grid's arrays and confines the plane index to
the planes the window and its halo hold, which is what a rank that holds exactly those planes reads.

Besides the values it reports what the tests' generic-position condition needs: the number of targets at which a discontinuous
decision (which eight values S reads, was a point clamped, which plane is held) is closer than EPS to going the other way."""
import numpy as np

EPS = 1e-9


def grid_shape(shape, kind):
    s = list(shape)
    if kind:
        s[3 - kind] += 1
    return tuple(s)


def nodes(shape, kind):
    gz, gy, gx = shape
    return np.array([gx + (kind == 1), gy + (kind == 2), gz + (kind == 3)], dtype=np.int64)


def offset(kind):
    o = np.full(3, 0.5)
    if kind:
        o[kind - 1] = 0.0
    return o


def held_planes(shape, kind, window):
    """[h0, h1): the planes of a grid of `kind` that the window and its halo hold, in the whole grid's plane index"""
    gz = shape[0]
    if window is None:
        return 0, gz + (kind == 3)
    c0, c1, halo = window
    return c0 - min(halo, c0), c1 + (kind == 3) + min(halo, gz - c1)


class Stencil:
    """S's indices and weights at the points p for a grid of `kind`"""

    def __init__(self, shape, kind, p, window=None):
        n = nodes(shape, kind)
        g = np.clip(p - offset(kind), 0.0, (n - 1).astype(np.float64))
        self.i0 = np.minimum(np.floor(g).astype(np.int64), n - 1)
        self.i1 = np.minimum(self.i0 + 1, n - 1)
        self.t = g - self.i0
        h0, h1 = held_planes(shape, kind, window)
        self.missed = (self.i0[:, 2] < h0) | (self.i1[:, 2] >= h1)
        self.i0[:, 2] = np.clip(self.i0[:, 2], h0, h1 - 1)
        self.i1[:, 2] = np.clip(self.i1[:, 2], h0, h1 - 1)
        # a coordinate within EPS of a node; one exactly on a face of the box B is where a clamp put it and decides nothing
        box = np.array([shape[2], shape[1], shape[0]], dtype=np.float64)
        u = p - offset(kind)
        self.near = ((np.abs(u - np.round(u)) < EPS) & (p != 0.0) & (p != box)).any(axis=1)


def lerp(t, a, b):
    return (1.0 - t) * a + t * b


def combine(q, st):
    """(S, lo, hi): the eight values of the array q along x, then y, then z; the least and the greatest of them"""
    x0, y0, z0 = st.i0.T
    x1, y1, z1 = st.i1.T
    v = [q[z, y, x].astype(np.float64) for z in (z0, z1) for y in (y0, y1) for x in (x0, x1)]
    tx, ty, tz = st.t.T
    x00, x10, x01, x11 = lerp(tx, v[0], v[1]), lerp(tx, v[2], v[3]), lerp(tx, v[4], v[5]), lerp(tx, v[6], v[7])
    return lerp(tz, lerp(ty, x00, x10), lerp(ty, x01, x11)), np.minimum.reduce(v), np.maximum.reduce(v)


def velocity_at(velocity, shape, p, window=None):
    """(U(p), missed, near)"""
    u = np.empty_like(p)
    missed, near = np.zeros(len(p), bool), np.zeros(len(p), bool)
    for c in range(3):
        st = Stencil(shape, c + 1, p, window)
        u[:, c] = combine(velocity[c], st)[0]
        missed |= st.missed
        near |= st.near
    return u, missed, near


def clamp_box(shape, q):
    """(clampB(q), a coordinate moved, a coordinate within EPS of a face without lying on it)"""
    box = np.array([shape[2], shape[1], shape[0]], dtype=np.float64)
    p = np.clip(q, 0.0, box)
    close = ((np.abs(q) < EPS) & (q != 0.0)) | ((np.abs(q - box) < EPS) & (q != box))
    return p, (p != q).any(axis=1), close.any(axis=1)


def departure(velocity, shape, x, dt, order=2, window=None):
    """(p_dep, clamped, missed, near) of the targets x; -dt gives p_fwd"""
    u, missed, _ = velocity_at(velocity, shape, x, window)  # (U(x) sits at a fixed offset from the nodes: nothing is decided there)
    clamped, near = np.zeros(len(x), bool), np.zeros(len(x), bool)
    if order == 2:
        p1, moved, close = clamp_box(shape, x - (0.5 * dt) * u)
        u, m1, n1 = velocity_at(velocity, shape, p1, window)
        clamped, missed, near = clamped | moved, missed | m1, near | n1 | close
    p, moved, close = clamp_box(shape, x - dt * u)
    return p, clamped | moved, missed, near | close


def targets(shape, kind, window=None):
    """(x, array shape, counted): the positions of the window's entries of a grid of `kind`, the shape of the window's array, and
    which entries the counters count (of the z-faces the planes c0 .. c1 - 1, and plane gz)"""
    gz = shape[0]
    c0, c1 = (0, gz) if window is None else window[:2]
    s = grid_shape((c1 - c0, shape[1], shape[2]), kind)
    k, j, i = np.meshgrid(np.arange(s[0]) + c0, np.arange(s[1]), np.arange(s[2]), indexing="ij")
    x = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(np.float64) + offset(kind)
    counted = (k.ravel() < c1) | (k.ravel() == gz) if kind == 3 else np.ones(len(x), bool)
    return x, s, counted


def advect(velocity, scalars, dt, scheme=0, order=2, window=None, advect_velocity=True):
    """The pass on whole-grid fp32 arrays.  Returns a dict: velocity (three arrays, or None), scalars (a list) -- the window's entries
    when a window is given --, counts [clamped, missed], nongeneric (targets too close to a decision), limited (MacCormack: targets
    whose m left [lo, hi])."""
    shape = (velocity[0].shape[0], velocity[0].shape[1], velocity[0].shape[2] - 1)
    assert scheme == 0 or window is None, "MacCormack on a window is not defined"
    jobs = [(0, list(scalars))] if len(scalars) else []
    if advect_velocity:
        jobs += [(a + 1, [velocity[a]]) for a in range(3)]
    out, counts, nongeneric, limited = {}, [0, 0], 0, 0
    hats = {}
    for kind, grids in jobs:
        x, s, counted = targets(shape, kind, window)
        p, clamped, missed, near = departure(velocity, shape, x, dt, order, window)
        st = Stencil(shape, kind, p, window)
        missed, near = missed | st.missed, near | st.near
        counts[0] += len(grids) * int((clamped & counted).sum())
        counts[1] += len(grids) * int((missed & counted).sum())
        hats[kind] = [combine(q, st)[0].astype(np.float32).reshape(s) for q in grids]
        out[kind] = (x, s, st, near)
    if scheme == 0:
        results = hats
        nongeneric = sum(int(out[kind][3].sum()) for kind, _ in jobs)
    else:
        results = {}
        for kind, grids in jobs:
            x, s, st, near = out[kind]
            pf, _, _, near_f = departure(velocity, shape, x, -dt, order)
            sf = Stencil(shape, kind, pf)
            near = near | near_f | sf.near
            results[kind] = []
            for q, qh in zip(grids, hats[kind]):
                _, lo, hi = combine(q, st)
                m = qh.ravel().astype(np.float64) + 0.5 * (q.ravel().astype(np.float64) - combine(qh, sf)[0])
                scale = EPS * float(np.abs(q).max())
                near = near | (np.abs(m - lo) < scale) | (np.abs(m - hi) < scale)
                limited += int(((m < lo) | (m > hi)).sum())
                results[kind].append(np.clip(m, lo, hi).astype(np.float32).reshape(s))
            nongeneric += int(near.sum())
    return {"velocity": [results[a + 1][0] for a in range(3)] if advect_velocity else None, "scalars": results.get(0, []),
            "counts": counts, "nongeneric": nongeneric, "limited": limited}


def window_of(q, kind, window):
    """the window's entries of a whole-grid array, and its halo planes (below, above; None where none is held)"""
    c0, c1, halo = window
    gz = q.shape[0] - (kind == 3)
    w1 = c1 + (kind == 3)
    below, above = min(halo, c0), min(halo, gz - c1)
    return q[c0:w1], (q[c0 - below:c0] if below else None), (q[w1:w1 + above] if above else None)
