"""numpy fp64 restatement of the FLIP particle passes (include/mgps_fields.h, "FLIP particles"): bin, particles ->
grid, grid -> particles and move, written from the header's definition operation by operation.

Grids are (gz, gy, gx) with x fastest; a particle set is three float32 arrays of positions (x, y, z, in cells from the grid's corner)
and three of velocities.  Grid kinds as in advection_reference: 0 cells, 1 + a the faces of axis a.

The face sums run as a loop over the neighbour cells in the stated order (ascending k, then j, then i), then over the slots of a cell,
vectorised over the targets: a step touches only the targets whose cell still has a slot, which leaves every other sum's bits alone.
The update samples with advection_reference's S and clamps with its clamp_box; S is not restated here."""
import numpy as np

import advection_reference as AR

EPS = AR.EPS


def inside(position, shape):
    """0 <= x_c <= g_c for all three components; false for NaN"""
    ok = np.ones(len(position[0]), bool)
    with np.errstate(invalid="ignore"):
        for c in range(3):
            ok &= (position[c] >= 0) & (position[c].astype(np.float64) <= float(shape[2 - c]))
    return ok


def keys(position, shape):
    """the linear cell (k gy + j) gx + i of every inside particle, `cells` for the others"""
    gz, gy, gx = shape
    ok = inside(position, shape)
    idx = [np.minimum(np.floor(np.where(ok, position[c], 0)).astype(np.int64), shape[2 - c] - 1) for c in range(3)]
    return np.where(ok, (idx[2] * gy + idx[1]) * gx + idx[0], gz * gy * gx)


def bin_particles(position, velocity, shape):
    """order, cell_start, the gathered arrays, counts [outside, occupied cells]"""
    cells = shape[0] * shape[1] * shape[2]
    key = keys(position, shape)
    order = np.argsort(key, kind="stable")
    cell_start = np.searchsorted(key[order], np.arange(cells + 2), side="left")
    return {"order": order.astype(np.int32), "cell_start": cell_start.astype(np.int32), "position": [q[order] for q in position],
            "velocity": [q[order] for q in velocity], "counts": [int(len(key) - cell_start[cells]), int((np.diff(cell_start[:cells + 1]) > 0).sum())]}


def hat(d):
    return np.maximum(0.0, 1.0 - np.abs(d))


def _gather(position, cell_start, shape, kind, visit):
    """walks, for every target of a grid of `kind`, the cells its definition names in ascending k, j, i and their slots in ascending
    order; visit(active targets, their node positions (M, 3), the slot of each) is called once per step"""
    gz, gy, gx = shape
    n = len(position[0])
    s = AR.grid_shape(shape, kind)
    k, j, i = [q.ravel() for q in np.meshgrid(np.arange(s[0]), np.arange(s[1]), np.arange(s[2]), indexing="ij")]
    node = np.stack([i, j, k], axis=1).astype(np.float64) + AR.offset(kind)
    reach = [(-1, 0) if kind == c + 1 else (-1, 0, 1) for c in range(3)]  # a face f of axis a: the cells f - 1 and f along a
    start = np.clip(cell_start.astype(np.int64), 0, n)  # (the device's clamp; a right cell_start is not changed by it)
    for dz in reach[2]:
        for dy in reach[1]:
            for dx in reach[0]:
                ci, cj, ck = i + dx, j + dy, k + dz
                ok = (ci >= 0) & (ci < gx) & (cj >= 0) & (cj < gy) & (ck >= 0) & (ck < gz)
                c = np.where(ok, (ck * gy + cj) * gx + ci, 0)
                first = start[c]
                count = np.where(ok, start[c + 1] - first, 0)
                r = 0
                active = np.nonzero(count > 0)[0]
                while len(active):
                    visit(active, node[active], first[active] + r)
                    r += 1
                    active = active[count[active] > r]
    return s


def to_grid(position, velocity, cell_start, shape, radius, dx=1.0):
    """velocity[3], weight[3], known[3] (uint8), phi, counts [known faces, cells with phi <= 0] from BINNED particles; num[3] and
    den[3]: the fp64 sums before they are rounded"""
    x = [q.astype(np.float64) for q in position]
    v = [q.astype(np.float64) for q in velocity]
    out = {"velocity": [], "weight": [], "known": [], "num": [], "den": [], "counts": [0, 0]}
    for a in range(3):
        total = int(np.prod(AR.grid_shape(shape, a + 1)))
        num, den = np.zeros(total), np.zeros(total)

        def visit(t, node, slot):
            w = (hat(x[0][slot] - node[:, 0]) * hat(x[1][slot] - node[:, 1])) * hat(x[2][slot] - node[:, 2])
            num[t] = num[t] + w * v[a][slot]
            den[t] = den[t] + w

        s = _gather(position, cell_start, shape, a + 1, visit)
        known = den > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            value = np.where(known, num / den, 0.0)
        out["velocity"].append(value.astype(np.float32).reshape(s))
        out["weight"].append(den.astype(np.float32).reshape(s))
        out["known"].append(known.astype(np.uint8).reshape(s))
        out["num"].append(num.reshape(s))
        out["den"].append(den.reshape(s))
        out["counts"][0] += int(known.sum())
    least = np.full(int(np.prod(shape)), np.inf)

    def nearest(t, node, slot):
        d = [x[c][slot] - node[:, c] for c in range(3)]
        least[t] = np.minimum(least[t], (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])

    _gather(position, cell_start, shape, 0, nearest)
    phi = float(dx) * (np.minimum(np.sqrt(least), 1.5) - float(radius))
    out["phi"] = phi.astype(np.float32).reshape(shape)
    out["counts"][1] = int((phi <= 0).sum())
    return out


def update(position, velocity, grid_new, grid_old, shape, dt, flip, order=2):
    """position[3], velocity[3], counts [clamped, outside], nongeneric: the particles whose p1 or end point has a coordinate within
    EPS of a face of the box without lying on it.  grid_old = None: old = pic"""
    ok = inside(position, shape)
    x = np.stack([q[ok].astype(np.float64) for q in position], axis=1)
    v = np.stack([q[ok].astype(np.float64) for q in velocity], axis=1)
    pic = AR.velocity_at(grid_new, shape, x)[0]
    old = AR.velocity_at(grid_old, shape, x)[0] if grid_old is not None else pic
    blend = (1.0 - flip) * pic + flip * (v + (pic - old))
    u, moved, close = pic, np.zeros(len(x), bool), np.zeros(len(x), bool)
    if order == 2:
        p1, moved, close = AR.clamp_box(shape, x + (0.5 * dt) * pic)
        u = AR.velocity_at(grid_new, shape, p1)[0]
    p, moved2, close2 = AR.clamp_box(shape, x + dt * u)
    out_x, out_v = [q.copy() for q in position], [q.copy() for q in velocity]
    for c in range(3):
        out_x[c][ok], out_v[c][ok] = p[:, c].astype(np.float32), blend[:, c].astype(np.float32)
    return {"position": out_x, "velocity": out_v, "counts": [int((moved | moved2).sum()), int((~ok).sum())],
            "nongeneric": int((close | close2).sum())}
