"""numpy restatement of the redistancing pass (include/mgps_fields.h, "redistancing"): the initial pass, the
update G, a block-Jacobi round on tiles of 64 x 4 x 4 cells anchored at cell (0, 0, 0) of the whole grid, the window rule and both
counters, written from the header's definition operation by operation: fp64 arithmetic on float32 data, every operation rounded on
its own, float32 where a value is stored.  numpy does not contract, so the device's bits are expected.

Arrays are (gz, gy, gx) with x fastest.  A state is the float32 array s T: T >= 0 the distance in cells, s = - where phi <= 0 (an
inside cell with T = 0 is -0.0).  A window is (c0, c1, halo); the window functions take the planes [h0, h1) a rank holds and never
read another: a plane inside the grid that is not held reads as NaN, which reaches an own plane only if the rule asked for too few."""
import numpy as np

f32 = np.float32
TILE = (4, 4, 64)  # (z, y, x)


def _shift(a, axis, d, fill):
    """the neighbour at +d (d = 1 or -1) along `axis`; `fill` where the array ends"""
    out = np.full_like(a, fill)
    dst, src = [slice(None)] * 3, [slice(None)] * 3
    if d > 0:
        dst[axis], src[axis] = slice(0, -1), slice(1, None)
    else:
        dst[axis], src[axis] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = a[tuple(src)]
    return out


def _z_fill(h0, h1, gz, d, inside_grid, outside_grid):
    """what a z neighbour beyond the held planes [h0, h1) reads: outside the whole grid or a plane that is not held"""
    return outside_grid if (h0 == 0 if d < 0 else h1 == gz) else inside_grid


def band_of(band):
    """B = (double)(float)band"""
    return float(f32(band))


def held(gz, window, inner=None):
    """[h0, h1): the planes a window holds.  inner given: raises ValueError where a round of `inner` needs more (the library refuses);
    inner = None: the initial pass, one plane either way"""
    c0, c1, halo = window
    h0, h1 = c0 - min(halo, c0), c1 + min(halo, gz - c1)
    if inner is None or inner == 1:
        n0, n1 = max(c0 - 1, 0), min(c1 + 1, gz)
    else:
        n0, n1 = max(4 * (c0 // 4) - 1, 0), min(4 * -(-c1 // 4) + 1, gz)
    if h0 > n0 or h1 < n1:
        raise ValueError(f"too few halo planes: [{h0}, {h1}) held, [{n0}, {n1}) needed")
    return h0, h1


def interface(neg, h0=0, gz=None):
    """a cell with an in-grid 6-neighbour of the other sign.  neg: the planes [h0, h0 + len) of a whole grid of gz planes; a z
    neighbour that is in the grid but not held counts as of the same sign (such a cell is no own cell of a window that was accepted)"""
    gz = neg.shape[0] if gz is None else gz
    s = neg.astype(np.int8)
    out = np.zeros(neg.shape, bool)
    for ax in range(3):
        for d in (1, -1):
            n = _shift(s, ax, d, -1)
            out |= (n >= 0) & (n != s)
    return out


def init(phi, band, h0=0, gz=None):
    """the initial pass on the planes [h0, h0 + len) of a grid of gz planes -> (state float32, interface mask).  On the first and last
    plane held that are not the grid's the result is wrong (their z neighbour is missing); they are no own planes"""
    B = band_of(band)
    gz = phi.shape[0] if gz is None else gz
    h1 = h0 + phi.shape[0]
    p = phi.astype(np.float64)
    neg = phi <= 0
    s = neg.astype(np.int8)
    iface = np.zeros(p.shape, bool)
    dcross = np.full(p.shape, np.inf)
    g2 = None
    with np.errstate(all="ignore"):
        for ax in (2, 1, 0):  # x, y, z: the sum of squares runs left to right
            fill = (np.nan, np.nan) if ax else (_z_fill(h0, h1, gz, 1, 0.0, np.nan), _z_fill(h0, h1, gz, -1, 0.0, np.nan))
            pp, pm = _shift(p, ax, 1, fill[0]), _shift(p, ax, -1, fill[1])
            hp, hm = ~np.isnan(pp), ~np.isnan(pm)
            for pn, d in ((pp, 1), (pm, -1)):
                sn = _shift(s, ax, d, -1)
                other = (sn >= 0) & (sn != s)
                iface |= other
                dcross = np.minimum(dcross, np.where(other, p / (p - pn), np.inf))
            g = np.where(hp & hm, 0.5 * (pp - pm), np.where(hp, pp - p, np.where(hm, p - pm, 0.0)))
            g2 = g * g if g2 is None else g2 + g * g
        dgrad = np.where(g2 > 0, np.abs(p) / np.sqrt(g2), np.inf)
    T = np.where(iface, np.minimum(np.minimum(dgrad, dcross), B), B)
    state = np.copysign(np.abs(T).astype(f32), np.where(neg, f32(-1), f32(1))).astype(f32)
    return state, iface


def G(a1, a2, a3):
    """the first-order Godunov update from the sorted neighbour minima (fp64, +inf allowed), each operation rounded on its own"""
    with np.errstate(all="ignore"):
        t = a1 + 1.0
        d = a1 - a2
        t2 = 0.5 * ((a1 + a2) + np.sqrt(2.0 - d * d))
        t = np.where(t > a2, t2, t)
        s = (a1 + a2) + a3
        q = (a1 * a1 + a2 * a2) + a3 * a3
        disc = np.maximum(s * s - 3.0 * (q - 1.0), 0.0)
        t3 = (s + np.sqrt(disc)) / 3.0
        t = np.where(t > a3, t3, t)
    return t


def _update(nb, T, fixed, B):
    """nb: the six neighbour T arrays as (x+, x-, y+, y-, z+, z-)"""
    with np.errstate(all="ignore"):
        a = np.sort(np.stack([np.minimum(nb[2 * c], nb[2 * c + 1]) for c in range(3)]).astype(np.float64), axis=0)
        t = np.minimum(G(a[0], a[1], a[2]), B).astype(f32)
        return np.where(fixed, T, np.minimum(T, t))


def round_(state, band, inner, h0=0, gz=None):
    """one round on the planes [h0, h0 + len) of a grid of gz planes -> the new state.  Tiles are anchored at plane 0 of the WHOLE
    grid.  A z neighbour in the grid that is not held reads NaN"""
    B = band_of(band)
    gz = state.shape[0] if gz is None else gz
    h1 = h0 + state.shape[0]
    neg = np.signbit(state)
    fixed = interface(neg, h0, gz)
    T0 = np.abs(state)
    idx = np.indices(state.shape)
    idx[0] += h0
    edge = {}
    for ax in range(3):
        edge[(ax, 1)] = idx[ax] % TILE[ax] == TILE[ax] - 1
        edge[(ax, -1)] = idx[ax] % TILE[ax] == 0

    def fill(ax, d):
        return np.inf if ax else _z_fill(h0, h1, gz, d, np.nan, np.inf)

    pairs = [(ax, d) for ax in (2, 1, 0) for d in (1, -1)]
    rim = {k: _shift(T0, k[0], k[1], fill(*k)) for k in pairs}
    cur = T0
    for _ in range(int(inner)):
        nb = [np.where(edge[k], rim[k], _shift(cur, k[0], k[1], fill(*k))) for k in pairs]
        cur = _update(nb, cur, fixed, B)
    return np.where(neg, -cur, cur).astype(f32)


def changed(new, old):
    return int((np.abs(new) != np.abs(old)).sum())


def scaled(state, dx):
    """out = float(dx state)"""
    return (float(dx) * state.astype(np.float64)).astype(f32)


def redistance(phi, band, dx=1.0, rounds=0, inner=4):
    """mgps_fields_redistance -> {"out", "state" (unscaled), "counts": [interface cells, cells the last round changed]}"""
    state, iface = init(phi, band)
    counts = [int(iface.sum()), 0]
    for _ in range(int(rounds)):
        new = round_(state, band, inner)
        counts[1] = changed(new, state)
        state = new
    return {"out": scaled(state, dx), "state": state, "counts": counts}


def fixpoint(phi, band, inner, limit=1000):
    """(the state at the fixpoint, R*: the number of rounds that changed a cell)"""
    state, _ = init(phi, band)
    for r in range(limit):
        new = round_(state, band, inner)
        if changed(new, state) == 0:
            return state, r
        state = new
    raise RuntimeError("no fixpoint")


def window_init(phi, band, window):
    """mgps_fields_slab_redistance_init from the planes the window holds -> (the own planes' state, interface cells on them)"""
    gz = phi.shape[0]
    c0, c1, _ = window
    h0, h1 = held(gz, window)
    state, iface = init(phi[h0:h1], band, h0, gz)
    own = slice(c0 - h0, c1 - h0)
    assert not np.isnan(state[own]).any()
    return state[own], int(iface[own].sum())


def window_round(state, band, inner, window):
    """mgps_fields_slab_redistance_round from the planes the window holds of the WHOLE grid's state -> (the own planes' new state,
    the number of own cells it changed)"""
    gz = state.shape[0]
    c0, c1, _ = window
    h0, h1 = held(gz, window, inner)
    new = round_(state[h0:h1], band, inner, h0, gz)
    own = slice(c0 - h0, c1 - h0)
    assert not np.isnan(new[own]).any()
    return new[own], changed(new[own], state[c0:c1])
