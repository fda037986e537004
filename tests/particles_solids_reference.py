"""numpy fp64 restatement of the particle passes next to solids (include/mgps_fields.h, "FLIP particles next to solids"; DESIGN.md
section 24): collide and resample, written from the header's definition operation by operation.  The fused update is by definition
particles_reference's update followed by collide on its float32 results; the tests compare the device's two forms bit for bit.

Grids are (gz, gy, gx) with x fastest; a particle set is three float32 arrays of positions (x, y, z, in cells from the grid's corner)
and three of velocities.  S and U are advection_reference's sampler (Stencil, combine, velocity_at) and clampB is its clamp_box; they
are not restated here.  numpy has no fused multiply-add: where the device writes one, the product is rounded here, which the tests'
tolerance covers (section 21's bound).

Generic position.  collide reports the particles at which a discrete decision sits within EPS = 1e-9 of its threshold: phi against
margin in any iteration, the final phi against 0, vn against 0 (relative to max |v|), |g| = sqrt(m) against 1e-6.  One refinement, with
its reason: a particle that HAS been pushed and then finds |phi - margin| < EPS is counted only if the normal at that point differs
from the normal of its last push by more than EPS / 10 in any component.  Where the two normals agree that closely, both ways of the
decision give the same outputs within the tolerance -- the extra push is shorter than EPS cells, and the velocity moves by at most
2 |r| |dn| <= 1e-9 max |v| / 2 with |r| <= |v| + |u_s| -- and the case cannot be avoided by a choice of seeds: the push is a Newton
step, so in an exactly planar solid_phi the second push lands on phi = margin to fp64 round-off and the third look ALWAYS sits on
the threshold."""
import numpy as np

import advection_reference as AR
import particles_reference as PR

EPS = AR.EPS
STUCK = 1e-12


def sample(q, shape, kind, p):
    """S(q)(p) for a grid of `kind`"""
    return AR.combine(q, AR.Stencil(shape, kind, p))[0]


def gradient(solid_phi, shape, x):
    """(g, m): g_c = S(x + e_c / 2) - S(x - e_c / 2), m = (g_x g_x + g_y g_y) + g_z g_z"""
    half = 0.5 * np.eye(3)
    g = np.stack([sample(solid_phi, shape, 0, x + half[c]) - sample(solid_phi, shape, 0, x - half[c]) for c in range(3)], axis=1)
    return g, (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]


def collide(position, velocity, solid_phi, solid_velocity, shape, margin=0.1, iterations=2, friction=0.0):
    """position[3], velocity[3], counts [pushed, still inside, stuck], pushed and stuck (masks over all particles), nongeneric, and in
    fp64, before anything is stored: normal (N, 3; the last push's), end (N, 3: the positions after the loop, NaN for outside
    particles), relative (N, 3: r after the rule, NaN unless pushed).  solid_velocity = None: the solid is at rest.  solid_phi may
    be fp64 (the analytic tests)"""
    ok = PR.inside(position, shape)
    where = np.nonzero(ok)[0]
    x = np.stack([q[ok].astype(np.float64) for q in position], axis=1)
    v = np.stack([q[ok].astype(np.float64) for q in velocity], axis=1)
    count = len(x)
    normal = np.zeros((count, 3))
    pushed, stuck, close, active = np.zeros(count, bool), np.zeros(count, bool), np.zeros(count, bool), np.ones(count, bool)
    for _ in range(iterations):
        a = np.nonzero(active)[0]
        if not len(a):
            break
        phi = sample(solid_phi, shape, 0, x[a])
        with np.errstate(invalid="ignore"):
            stop = phi >= margin
        near = np.abs(phi - margin) < EPS
        fresh = near & ~pushed[a]
        again = np.nonzero(near & pushed[a])[0]
        if len(again):  # (the refinement of the module's docstring)
            g, m = gradient(solid_phi, shape, x[a[again]])
            with np.errstate(invalid="ignore", divide="ignore"):
                differs = ~(np.abs(g / np.sqrt(m)[:, None] - normal[a[again]]).max(axis=1) <= EPS / 10)
            fresh[again[differs]] = True
        close[a] |= fresh
        active[a[stop]] = False
        a, phi = a[~stop], phi[~stop]
        g, m = gradient(solid_phi, shape, x[a])
        with np.errstate(invalid="ignore"):
            close[a] |= np.abs(np.sqrt(m) - np.sqrt(STUCK)) < EPS
            good = m > STUCK
        stuck[a[~good]] = True
        active[a[~good]] = False
        a, phi, g, m = a[good], phi[good], g[good], m[good]
        n = g / np.sqrt(m)[:, None]
        x[a] = AR.clamp_box(shape, x[a] + (margin - phi)[:, None] * n)[0]
        normal[a] = n
        pushed[a] = True
    us = np.zeros((count, 3))
    if solid_velocity is not None and pushed.any():
        us[pushed] = AR.velocity_at(solid_velocity, shape, x[pushed])[0]
    r = v - us
    vn = (r[:, 0] * normal[:, 0] + r[:, 1] * normal[:, 1]) + r[:, 2] * normal[:, 2]
    vmax = max(float(np.abs(v).max()), 1e-300) if count else 1.0
    close |= pushed & (np.abs(vn) < EPS * vmax)
    into = pushed & (vn < 0)
    r[into] = r[into] - vn[into, None] * normal[into]
    r[into] = (1.0 - friction) * r[into]
    out_x, out_v = [q.copy() for q in position], [q.copy() for q in velocity]
    hit = where[pushed]
    for c in range(3):
        out_x[c][hit] = x[pushed, c].astype(np.float32)
        out_v[c][hit] = (r[pushed, c] + us[pushed, c]).astype(np.float32)
    last = sample(solid_phi, shape, 0, np.stack([out_x[c][hit].astype(np.float64) for c in range(3)], axis=1))
    close[pushed] |= np.abs(last) < EPS
    mask = lambda m: np.isin(np.arange(len(position[0])), where[m])  # noqa: E731
    full, end, relative = np.zeros((len(position[0]), 3)), np.full((len(position[0]), 3), np.nan), np.full((len(position[0]), 3), np.nan)
    full[where], end[where], relative[hit] = normal, x, r[pushed]
    return {"position": out_x, "velocity": out_v, "counts": [int(pushed.sum()), int((last < 0).sum()), int(stuck.sum())], "pushed": mask(pushed),
            "stuck": mask(stuck), "normal": full, "end": end, "relative": relative, "nongeneric": int(close.sum())}


# ---- resample ------------------------------------------------------------------------------------------------------------------------
def mix(x):
    """x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 in wrapping uint32 (on uint64 arrays, masked)"""
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def kept_slots(m, most):
    """which of a cell's m slots the stride rule keeps"""
    t = np.arange(m, dtype=np.int64)
    return np.ones(m, bool) if m <= most else ((t + 1) * most // m > t * most // m)


def seeded_position(seed, cell, index, ijk):
    """the float32 position of the particle `index` (= k + q) of the linear cell `cell` with cell coordinates ijk (N, 3), x first"""
    base = mix(mix(np.uint64(seed & 0xFFFFFFFF) ^ np.uint64(0x9E3779B9)) + np.asarray(cell, dtype=np.uint64))
    out = []
    for a in range(3):
        h = mix(base + ((3 * np.asarray(index, dtype=np.uint64) + a) & 0xFFFFFFFF))
        r = (h >> 8).astype(np.float64) * 2.0 ** -24
        top = np.nextafter((ijk[:, a] + 1).astype(np.float32), np.float32(0))
        out.append(np.minimum((ijk[:, a].astype(np.float64) + r).astype(np.float32), top))
    return out


def resample(position, velocity, cell_start, shape, min_per_cell, max_per_cell, liquid_phi=None, dx=1.0, seed_depth=1.0, solid_phi=None,
             grid=None, seed=0, keep_outside=False):
    """position[3], velocity[3] (of n_out entries: the whole set, whatever the capacity), cell_start (cells + 2), n_out, counts
    [thinned, seeded, deep cells], source (the input slot of every output slot, -1 for a seeded one), per_cell (cells)"""
    gz, gy, gx = shape
    cells, n = gz * gy * gx, len(position[0])
    start = np.clip(cell_start.astype(np.int64), 0, n)
    first, m = start[:-1], np.maximum(start[1:] - start[:-1], 0)  # cells + 1 bins: the last is the outside bin
    kept = np.minimum(m[:cells], max_per_cell)
    deep = np.zeros(cells, bool)
    if liquid_phi is not None:
        with np.errstate(invalid="ignore"):
            deep = liquid_phi.ravel() <= -np.float32(seed_depth * dx)
            if solid_phi is not None:
                deep &= solid_phi.ravel() > 0
    seeds = np.where(deep & (kept < min_per_cell), min_per_cell - kept, 0)
    count = np.concatenate([kept + seeds, [m[cells] if keep_outside else 0]])
    out_start = np.concatenate([[0], np.cumsum(count)])
    n_out = int(out_start[-1])
    source = np.full(n_out, -1, dtype=np.int64)
    for c in np.nonzero(count[:cells] > 0)[0]:
        if m[c]:
            source[out_start[c]:out_start[c] + kept[c]] = first[c] + np.nonzero(kept_slots(int(m[c]), max_per_cell))[0]
    if keep_outside:
        source[out_start[cells]:n_out] = first[cells] + np.arange(m[cells])
    old = source >= 0
    out_x, out_v = [np.zeros(n_out, np.float32) for _ in range(3)], [np.zeros(n_out, np.float32) for _ in range(3)]
    for c in range(3):
        out_x[c][old], out_v[c][old] = position[c][source[old]], velocity[c][source[old]]
    c = np.repeat(np.arange(cells), seeds)
    if len(c):
        q = np.arange(len(c)) - np.repeat(np.cumsum(seeds) - seeds, seeds)
        slot = out_start[c] + kept[c] + q
        ijk = np.stack([c % gx, c // gx % gy, c // gx // gy], axis=1)
        new = seeded_position(seed, c, kept[c] + q, ijk)
        u = AR.velocity_at(grid, shape, np.stack([a.astype(np.float64) for a in new], axis=1))[0]
        for a in range(3):
            out_x[a][slot], out_v[a][slot] = new[a], u[:, a].astype(np.float32)
    return {"position": out_x, "velocity": out_v, "cell_start": out_start.astype(np.int32), "n_out": n_out,
            "counts": [int((m[:cells] - kept).sum()), int(seeds.sum()), int(deep.sum())], "source": source, "per_cell": (kept + seeds), "deep": deep}
