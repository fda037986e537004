"""NumPy restatement of the pressure force and torque on solid bodies (include/mgps_fields.h): the yardstick of
tests/test_solid_forces.py and tests/solid_forces_slab_worker.py.  The definition has no counterpart in the reference; it is restated
here face grid by face grid, vectorised, in float64 from the float32 inputs with the closed fraction s formed in float32.

Grids are (nz, ny, nx) arrays; the face grid of axis a (0 = x) has one more entry along numpy axis 2 - a."""
import numpy as np

LIQUID = 1


def face_shape(shape, axis):
    s = list(shape)
    s[2 - axis] += 1
    return tuple(s)


def face_centres(shape, axis):
    """x, y, z of the face centres of axis `axis`, in cell units from the grid's corner (broadcastable float64 arrays)"""
    fs = face_shape(shape, axis)
    k, j, i = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in fs], indexing="ij", sparse=True)
    pos = [i, j, k]
    return [pos[a] if a == axis else pos[a] + 0.5 for a in range(3)]


def closed_fraction(w):
    """s = w < 1.f ? 1.f - w : 0.f, in float32"""
    w = np.asarray(w, dtype=np.float32)
    return np.where(w < np.float32(1), np.float32(1) - w, np.float32(0)).astype(np.float32)


def _behind_front(cells, axis, fill):
    """the cell grid `cells` seen from the faces of `axis`: (value of the backward cell, value of the forward cell); `fill` where
    the cell does not exist"""
    ax = 2 - axis
    pad = [(0, 0)] * 3
    pad[ax] = (1, 0)
    behind = np.pad(cells, pad, constant_values=fill)
    pad[ax] = (0, 1)
    front = np.pad(cells, pad, constant_values=fill)
    return behind, front


def face_terms(pressure, material, cut_weights, axis):
    """per face of `axis`: (wet, s float32, phi float64, pB, pF)"""
    liquid = material == LIQUID
    p = np.where(liquid, pressure.astype(np.float64), 0.0)
    pb, pf = _behind_front(p, axis, 0.0)
    lb, lf = _behind_front(liquid, axis, False)
    s = closed_fraction(cut_weights[axis])
    wet = (s > 0) & (lb | lf)
    return wet, s, s.astype(np.float64) * (pb - pf), pb, pf


def rows_of(body, bodies):
    return np.where((body >= 1) & (body <= bodies), body, 0).astype(np.int64)


def counted(shape, axis, planes):
    """the faces of `axis` a slab window of base planes [c0, c1) counts: x- and y-faces of its planes, z-faces c0 .. c1 - 1 and on
    the last window plane gz (None: every face)"""
    fs = face_shape(shape, axis)
    mask = np.ones(fs, dtype=bool)
    if planes is not None:
        c0, c1 = planes
        k = np.arange(fs[0])
        keep = (k >= c0) & (k < c1)
        if axis == 2 and c1 == shape[0]:
            keep |= k == shape[0]
        mask &= keep[:, None, None]
    return mask


def solid_forces(pressure, material, cut_weights, body, centres, scale=1.0, planes=None):
    """(rows, magnitude): rows is the (bodies + 1, 8) table of the definition; magnitude holds, per row and column, the sum of
    |term| over the same faces (times |scale| on the force and torque columns) -- what the error of a reordered fp64 sum scales with.
    `planes` = (c0, c1): the part of a slab window under its counting rule, on the whole grid's arrays."""
    shape = tuple(material.shape)
    centres = np.asarray(centres, dtype=np.float64)
    bodies = centres.shape[0] - 1
    rows, mag = np.zeros((bodies + 1, 8)), np.zeros((bodies + 1, 8))
    for a in range(3):
        wet, s, phi, _, _ = face_terms(pressure, material, cut_weights, a)
        wet = wet & counted(shape, a, planes)
        r = rows_of(body[a], bodies)[wet]
        pos = [np.broadcast_to(x, wet.shape)[wet] for x in face_centres(shape, a)]
        ph = phi[wet]
        arm = [pos[c] - centres[r, c] for c in range(3)]
        u, v = (a + 1) % 3, (a + 2) % 3
        terms = {a: ph, 3 + u: arm[v] * ph, 3 + v: -arm[u] * ph, 6: s[wet].astype(np.float64), 7: np.ones(ph.shape)}
        for col, t in terms.items():
            rows[:, col] += np.bincount(r, weights=t, minlength=bodies + 1)
            mag[:, col] += np.bincount(r, weights=np.abs(t), minlength=bodies + 1)
    rows[:, :6] *= scale
    mag[:, :6] *= abs(scale)
    return rows, mag


def rigid_velocity(shape, body, centres, linear, angular, bodies):
    """sv_a[f] = (U_r + omega_r x (x_f - centres[r]))_a with r the face's row: three float64 face grids"""
    centres, linear, angular = (np.asarray(x, dtype=np.float64) for x in (centres, linear, angular))
    out = []
    for a in range(3):
        r = rows_of(body[a], bodies)
        pos = [np.broadcast_to(x, r.shape) for x in face_centres(shape, a)]
        u, v = (a + 1) % 3, (a + 2) % 3
        # (omega x d)_a = omega_u d_v - omega_v d_u
        out.append(linear[r, a] + angular[r, u] * (pos[v] - centres[r, v]) - angular[r, v] * (pos[u] - centres[r, u]))
    return out


def solid_rhs(material, solid_velocity, cut_weights):
    """the solid part of the right-hand side at LIQUID cells (cellDivergence with zero fluid velocity, signBackward = +1):
    sum_a (1 - w_back) sv_back - (1 - w_fwd) sv_fwd, 0 elsewhere; float64 from the given arrays"""
    rhs = np.zeros(material.shape)
    for a in range(3):
        flux = closed_fraction(cut_weights[a]).astype(np.float64) * np.asarray(solid_velocity[a], dtype=np.float64)
        ax = 2 - a
        n = material.shape[ax]
        rhs += np.take(flux, np.arange(n), axis=ax) - np.take(flux, np.arange(1, n + 1), axis=ax)
    return np.where(material == LIQUID, rhs, 0.0)


def power_magnitude(pressure, material, cut_weights, solid_velocity):
    """sum over the wet faces of s (|pB| + |pF|) |sv|: what both sides of the adjoint identity scale with"""
    total = 0.0
    for a in range(3):
        wet, s, _, pb, pf = face_terms(pressure, material, cut_weights, a)
        total += float((s.astype(np.float64) * (np.abs(pb) + np.abs(pf)) * np.abs(np.asarray(solid_velocity[a], dtype=np.float64)))[wet].sum())
    return total
