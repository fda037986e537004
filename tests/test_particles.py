"""FLIP particles on the device (include/mgps_fields.h, "FLIP particles") against tests/particles_reference.py.

CPU: the restatement against analysis (a constant particle velocity is the grid's; partition of unity and momentum; one particle's
phi; the FLIP and PIC ends of the blend; particles on cell boundaries and walls; NaN and out-of-box particles), the condition that the
seeded scenes are in generic position, the C ABI's refusals and the ctypes mirrors' sizes.
GPU: the three entries against the restatement on section 18's grid, rows across tile edges and a sheet one cell thick; both trace
orders, in place and out of place; the same bits twice; shuffled input; a wrong cell_start; a drop in free flight carried by particles.

Tolerance.  order, cell_start, the gathered arrays, known, the counts and liquid_phi are EQUAL to the restatement's: integers, a min,
an exactly rounded sqrt and operations rounded one by one.  Grid velocities and weights, and the updated particles:
|got - want| <= 2^-24 |want| + 1e-9 max|v| (max g_c for positions) -- the one float32 rounding, and for the update the fp64 round-off
of positions and weights where the device fuses a product into a sum, with orders of margin (section 21's bound).  Whether a clamp
moved a coordinate is not continuous: the restatement counts the particles closer than 1e-9 to that decision and a CPU test asserts
that count is 0 for every seeded scene used here."""
import ctypes as C
import functools

import numpy as np
import pytest

import advection_reference as AR
import particles_reference as PR
from refusals import refused as _refused

DT = 0.7
RADIUS = 1.0
GRID = (19, 22, 37)  # section 18's grid: off every multiple of the 64 x 4 x 4 tile
# The staged to-grid kernel takes a row's particles through LDS in chunks of kChunk = 768 (csrc/mgps_particles.hip; DESIGN.md section
# 23): the crowded cell holds more than that, its x-neighbour half as many, so a thread's three cells span three chunks
CROWD = 800
FORMS = ["gather", "staged"]
SCENES = {  # name -> (shape, seed, crowded row)
    "grid": (GRID, 31, True),
    "row64": ((5, 6, 64), 32, False),
    "row65": ((5, 6, 65), 33, False),
    "row131": ((5, 6, 131), 34, False),
    "sheet": ((1, 7, 70), 35, False),  # an extent of one cell
}


def _box(shape):
    return np.array([shape[2], shape[1], shape[0]], dtype=np.float64)


def _face_grids(shape, rng, phase):
    """three face grids: a smooth field plus noise, scaled to max |DT u| = 2.5"""
    grids = []
    for a in range(3):
        x, s, _ = AR.targets(shape, a + 1)
        smooth = np.sin(0.31 * x[:, 0] + 0.17 * x[:, 1] + 0.23 * x[:, 2] + 1.3 * a + phase)
        grids.append((smooth + 0.3 * rng.uniform(-1.0, 1.0, len(x))).reshape(s))
    scale = 2.5 / (DT * max(float(np.abs(g).max()) for g in grids))
    return [(scale * g).astype(np.float32) for g in grids]


def empty_region(shape, i, j, k, margin):
    """the cells without particles: y >= gy / 2 - 1 and z >= gz / 2 (the sheet: x >= gx / 2 - 1).  margin = 1: without its first rows,
    onto which a float32 position can round -- the tiles whose cells and rims lie in there hold nothing"""
    gz, gy, gx = shape
    return (j >= gy // 2 - 1 + margin) & ((k >= gz // 2 + margin) if gz > 1 else (i >= gx // 2 - 1 + margin))


@functools.lru_cache(maxsize=None)
def scene(name):
    """position[3], velocity[3] (unbinned particles), grid_new[3], grid_old[3]; float32, read-only.
    A mean of four particles per liquid cell; empty_region holds none, so the tiles there and their rims hold nothing; particles
    exactly on cell boundaries and on all six walls; a few outside and NaN"""
    shape, seed, crowded = SCENES[name]
    gz, gy, gx = shape
    rng = np.random.default_rng(seed)
    box = _box(shape)
    k, j, i = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
    liquid = ~empty_region(shape, i, j, k, 0)
    cells = np.stack([i[liquid], j[liquid], k[liquid]], axis=1)
    pick = cells[rng.integers(0, len(cells), 4 * len(cells))]
    parts = [pick + rng.uniform(0.0, 1.0, pick.shape)]
    # on cell boundaries: one, two or all three coordinates whole numbers
    edge = cells[rng.integers(0, len(cells), 60)] + rng.uniform(0.0, 1.0, (60, 3))
    for q in range(60):
        for c in range(3):
            if (q >> c) & 1 or q % 7 == 0:
                edge[q, c] = np.floor(edge[q, c])
    parts.append(edge)
    # on all six walls; one that falls into the empty region is moved out of it along an axis that is not its wall's
    wall = rng.uniform(0.0, 1.0, (36, 3)) * box
    for q in range(36):
        w = q % 3
        wall[q, w] = 0.0 if (q // 3) % 2 else box[w]
        if empty_region(shape, *np.floor(wall[q]), 0):
            free = 1 if w != 1 else (2 if gz > 1 else 0)
            wall[q, free] = rng.uniform(0.0, 1.0) * ((gy // 2 - 2) if free == 1 else (gz // 2 - 1) if free == 2 else (gx // 2 - 2))
    parts.append(wall)
    parts.append(np.array([[0.0, 0.0, 0.0], [box[0], 0.0, box[2]], [0.0, box[1], 0.0]]))
    if crowded:  # the crowded row: cell (20, 5, 4) and its x-neighbour (21, 5, 4)
        parts.append(np.array([20.0, 5.0, 4.0]) + rng.uniform(0.0, 1.0, (CROWD, 3)))
        parts.append(np.array([21.0, 5.0, 4.0]) + rng.uniform(0.0, 1.0, (CROWD // 2, 3)))
    outside = np.array([[-0.5, 1.0, 0.5], [box[0] + 1.0, 1.0, 0.5], [1.0, -1e-3, 0.5], [1.0, box[1] * (1 + 1e-6), 0.5], [1.0, 1.0, -2.0],
                        [1.0, 1.0, box[2] + 0.25], [np.nan, 1.0, 0.5], [1.0, np.nan, 0.5], [1.0, 1.0, np.nan], [np.inf, 1.0, 0.5],
                        [-np.inf, np.nan, 0.5]])
    parts.append(outside)
    x = np.concatenate(parts)
    x = x[rng.permutation(len(x))]
    position = [x[:, c].astype(np.float32) for c in range(3)]
    xs = np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)
    velocity = [np.sin(0.29 * xs[:, 0] - 0.21 * xs[:, 1] + 0.19 * xs[:, 2] + 0.9 * a) + 0.3 * rng.uniform(-1.0, 1.0, len(x)) for a in range(3)]
    scale = 2.5 / (DT * max(float(np.abs(v).max()) for v in velocity))
    velocity = [(scale * v).astype(np.float32) for v in velocity]
    out = {"shape": shape, "position": position, "velocity": velocity, "grid_new": _face_grids(shape, rng, 0.0), "grid_old": _face_grids(shape, rng, 0.4)}
    for key in ("position", "velocity", "grid_new", "grid_old"):
        for q in out[key]:
            q.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def binned(name):
    s = scene(name)
    return PR.bin_particles(s["position"], s["velocity"], s["shape"])


@functools.lru_cache(maxsize=None)
def gridded(name):
    b = binned(name)
    return PR.to_grid(b["position"], b["velocity"], b["cell_start"], scene(name)["shape"], RADIUS, 0.5)


@functools.lru_cache(maxsize=None)
def updated(name, order):
    s, b = scene(name), binned(name)
    return PR.update(b["position"], b["velocity"], s["grid_new"], s["grid_old"], s["shape"], DT, 0.95, order)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype.itemsize == 4 else np.uint8)


# ---- CPU: the restatement against analysis -------------------------------------------------------------------------------------------
def _cloud(shape, count, margin, seed):
    rng = np.random.default_rng(seed)
    box = _box(shape)
    x = margin + rng.uniform(0.0, 1.0, (count, 3)) * (box - 2 * margin)
    return [x[:, c].astype(np.float32) for c in range(3)], rng


def test_restated_constant_particle_velocity_is_the_grid_velocity():
    shape = (7, 8, 9)
    position, _ = _cloud(shape, 900, 0.0, 1)
    U = np.array([0.625, -0.375, 0.25], dtype=np.float32)
    b = PR.bin_particles(position, [np.full(900, U[a], np.float32) for a in range(3)], shape)
    g = PR.to_grid(b["position"], b["velocity"], b["cell_start"], shape, RADIUS)
    for a in range(3):
        known = g["known"][a] == 1
        assert known.sum() > 300
        assert np.abs(g["num"][a][known] / g["den"][a][known] - float(U[a])).max() <= 1e-12
        assert np.array_equal(g["velocity"][a][known], np.full(int(known.sum()), U[a])) and not g["velocity"][a][~known].any()


def test_restated_partition_of_unity_and_momentum():
    """particles at least one cell from every wall: every particle's weights add up to 1 per axis"""
    shape = (8, 9, 10)
    position, rng = _cloud(shape, 700, 1.0, 2)
    velocity = [rng.uniform(-1.0, 1.0, 700).astype(np.float32) for _ in range(3)]
    b = PR.bin_particles(position, velocity, shape)
    assert b["counts"][0] == 0
    g = PR.to_grid(b["position"], b["velocity"], b["cell_start"], shape, RADIUS)
    for a in range(3):
        assert abs(g["den"][a].sum() - 700.0) <= 1e-9 * 700.0
        known = g["den"][a] > 0
        momentum = (g["den"][a][known] * (g["num"][a][known] / g["den"][a][known])).sum()
        want = velocity[a].astype(np.float64).sum()
        assert abs(momentum - want) <= 1e-9 * np.abs(velocity[a]).astype(np.float64).sum()


def test_restated_phi_of_one_particle():
    shape, radius, dx = (6, 7, 8), 0.75, 0.25
    p = np.array([3.3, 2.6, 3.1], dtype=np.float32)
    b = PR.bin_particles([p[c:c + 1] for c in range(3)], [np.zeros(1, np.float32)] * 3, shape)
    g = PR.to_grid(b["position"], b["velocity"], b["cell_start"], shape, radius, dx)
    x, s, _ = AR.targets(shape, 0)
    dist = np.sqrt(((x - p.astype(np.float64)) ** 2).sum(axis=1))
    want = dx * (np.minimum(dist, 1.5) - radius)
    assert np.abs(g["phi"].ravel() - want).max() <= 1e-6 and (dist < 1.5).sum() > 8
    assert np.array_equal(g["phi"].ravel()[dist > 1.5], np.full(int((dist > 1.5).sum()), np.float32(dx * (1.5 - radius))))
    assert g["counts"][1] == int((dist <= radius).sum())


@pytest.mark.parametrize("order", [1, 2])
def test_restated_blend_ends(order):
    s, b = scene("row65"), binned("row65")
    ok = PR.inside(b["position"], s["shape"])
    r = PR.update(b["position"], b["velocity"], s["grid_new"], s["grid_new"], s["shape"], DT, 1.0, order)
    assert all(np.array_equal(_bits(r["velocity"][c]), _bits(b["velocity"][c])) for c in range(3))
    r = PR.update(b["position"], b["velocity"], s["grid_new"], None, s["shape"], DT, 0.0, order)
    x = np.stack([q[ok].astype(np.float64) for q in b["position"]], axis=1)
    pic = AR.velocity_at(s["grid_new"], s["shape"], x)[0]
    assert all(np.array_equal(r["velocity"][c][ok], pic[:, c].astype(np.float32)) for c in range(3))
    r0 = PR.update(b["position"], b["velocity"], s["grid_new"], s["grid_old"], s["shape"], 0.0, 0.95, order)
    assert all(np.array_equal(_bits(r0["position"][c]), _bits(b["position"][c])) for c in range(3)) and r0["counts"][0] == 0


def test_restated_cells_of_particles_on_boundaries_and_outside():
    shape = (3, 4, 5)
    cells = 60
    cases = [((0.0, 0.0, 0.0), 0), ((5.0, 4.0, 3.0), cells - 1), ((2.0, 1.0, 1.0), (1 * 4 + 1) * 5 + 2), ((5.0, 0.5, 0.5), 4),
             ((4.999999, 3.9999998, 2.9999998), cells - 1), ((1.0, 4.0, 0.0), 3 * 5 + 1), ((-0.0, 0.0, 0.0), 0),
             ((-1e-6, 1.0, 1.0), cells), ((5.0000005, 1.0, 1.0), cells), ((1.0, np.nan, 1.0), cells), ((np.inf, 1.0, 1.0), cells),
             ((1.0, 1.0, 3.5), cells)]
    position = [np.array([c[0][a] for c in cases], dtype=np.float32) for a in range(3)]
    assert PR.keys(position, shape).tolist() == [c[1] for c in cases]
    b = PR.bin_particles(position, position, shape)
    assert b["counts"] == [5, 5] and b["cell_start"][cells] == 7 and b["cell_start"][cells + 1] == 12
    assert b["order"][:3].tolist() == [0, 6, 3]  # (within a cell the slots ascend by input index)


@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_are_in_generic_position_and_hold_what_they_should(name):
    s, b, g = scene(name), binned(name), gridded(name)
    gz, gy, gx = s["shape"]
    for order in (1, 2):
        r = updated(name, order)
        assert r["nongeneric"] == 0 and r["counts"][0] > 100 and r["counts"][1] == 11
    assert b["counts"][0] == 11
    count = np.diff(b["cell_start"][:gz * gy * gx + 1]).reshape(s["shape"])
    assert 3.0 < count[count > 0].mean() < 6.0
    k, j, i = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
    hollow = empty_region(s["shape"], i, j, k, 1)
    assert hollow.sum() >= 6 * 6 * 7 or gz == 1 and not count[hollow].any()
    assert not count[hollow].any()
    if SCENES[name][2]:
        assert count[4, 5, 20] >= CROWD and count[4, 5, 21] >= CROWD // 2
    assert all(0 < int(g["known"][a].sum()) < g["known"][a].size for a in range(3)) and 0 < g["counts"][1] < gz * gy * gx


# ---- CPU: refusals and the mirrors -----------------------------------------------------------------------------------------------------
def _fill(d, fields, slot):
    for name in fields:
        arr = getattr(d, name)
        if isinstance(arr, C.Array):
            for a in range(3):
                arr[a] = next(slot) << 24
        else:
            setattr(d, name, next(slot) << 24)


def _desc(kind, **kw):
    """a good desc on made-up addresses, 16 MiB apart (never dereferenced: every call below is refused on the host)"""
    from geometricmultigridpressuresolver_amd import fields as F

    cls, names = {
        "bin": (F.ParticlesBinDesc, ("position_in", "velocity_in", "position_out", "velocity_out", "order", "cell_start")),
        "to_grid": (F.ParticlesToGridDesc, ("position", "velocity", "cell_start", "velocity_out", "weight_out", "known_out", "liquid_phi_out")),
        "update": (F.ParticlesUpdateDesc, ("position_in", "velocity_in", "position_out", "velocity_out", "grid_new", "grid_old")),
    }[kind]
    d = cls()
    d.struct_size = C.sizeof(cls)
    d.gx, d.gy, d.gz, d.n = 6, 5, 4, 100
    if kind == "to_grid":
        d.radius, d.dx = 1.0, 0.5
    if kind == "update":
        d.dt, d.flip, d.trace_order = 0.5, 0.95, 2
    _fill(d, names, iter(range(1, 64)))
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_refusals_need_no_device_and_the_mirrors_have_the_library_sizes():
    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd._lib import lib

    L = lib()
    assert (C.sizeof(F.ParticlesBinDesc), C.sizeof(F.ParticlesToGridDesc), C.sizeof(F.ParticlesUpdateDesc)) == (144, 184, 192)
    entries = {"bin": L.mgps_particles_bin, "to_grid": L.mgps_particles_to_grid, "update": L.mgps_particles_update}
    nan, inf = float("nan"), float("inf")
    for kind, entry in entries.items():
        fn = "mgps_particles_" + kind
        run = lambda d: entry(C.byref(d), None)  # noqa: E731
        make = functools.partial(_desc, kind)
        _refused(entry(None, None), fn, "struct_size")
        d = make()
        d.struct_size -= 8
        _refused(run(d), fn, "struct_size")
        for k in ("gx", "gy", "gz"):
            _refused(run(make(**{k: 0})), fn, "extent")
        _refused(run(make(gx=2048, gy=1024, gz=1024)), fn, "too many cells", "int32")
        _refused(run(make(gx=2047, gy=1024, gz=1024, n=-1)), fn, "n = -1", "negative")
        _refused(run(make(n=-1)), fn, "negative")
    # bin
    fn, run, make = "mgps_particles_bin", lambda d: entries["bin"](C.byref(d), None), functools.partial(_desc, "bin")  # noqa: E731
    for name, idx in (("position_in", 0), ("position_out", 2), ("velocity_in", 1)):
        d = make()
        getattr(d, name)[idx] = None
        _refused(run(d), fn, name + f"[{idx}]", "NULL")
    for name in ("order", "cell_start"):
        _refused(run(make(**{name: None})), fn, name, "NULL")
    d = make()
    d.velocity_out[1] = None
    _refused(run(d), fn, "velocity_out", "all three")
    d = make()
    d.position_out[0] = d.position_in[0]
    _refused(run(d), fn, "position_in[0]", "position_out[0]", "overlap")
    d = make()
    d.order = d.velocity_out[2] + 396
    _refused(run(d), fn, "velocity_out[2]", "order", "overlap")
    d = make()
    d.cell_start = d.position_in[1] - (6 * 5 * 4 + 2) * 4 + 4
    _refused(run(d), fn, "position_in[1]", "cell_start", "overlap")
    # to grid
    fn, run, make = "mgps_particles_to_grid", lambda d: entries["to_grid"](C.byref(d), None), functools.partial(_desc, "to_grid")  # noqa: E731
    for bad in (0.0, -1.0, 1.5000001, nan, inf):
        _refused(run(make(radius=bad)), fn, "radius")
    for bad in (-1, 3):
        _refused(run(make(form=bad)), fn, "form")
    for bad in (0.0, -1.0, nan, inf):
        _refused(run(make(dx=bad)), fn, "dx")
    _refused(run(make(gy=4 * 65535 + 1, gx=1, gz=1)), fn, "along y or z")
    for name, idx in (("position", 0), ("velocity", 2), ("velocity_out", 1), ("known_out", 0)):
        d = make()
        getattr(d, name)[idx] = None
        _refused(run(d), fn, name + f"[{idx}]", "NULL")
    _refused(run(make(cell_start=None)), fn, "cell_start", "NULL")
    d = make()
    d.weight_out[2] = None
    _refused(run(d), fn, "weight_out", "all three")
    d = make()
    d.known_out[1] = d.velocity_out[0] + 7 * 5 * 4 * 4 - 1
    _refused(run(d), fn, "velocity_out[0]", "known_out[1]", "overlap")
    d = make()
    d.liquid_phi_out = d.velocity[1] + 4
    _refused(run(d), fn, "velocity[1]", "liquid_phi_out", "overlap")
    d = make()
    d.weight_out[0] = d.cell_start
    _refused(run(d), fn, "cell_start", "weight_out[0]", "overlap")
    # update
    fn, run, make = "mgps_particles_update", lambda d: entries["update"](C.byref(d), None), functools.partial(_desc, "update")  # noqa: E731
    for bad in (0, 3):
        _refused(run(make(trace_order=bad)), fn, "trace_order")
    for bad in (nan, inf, -inf):
        _refused(run(make(dt=bad)), fn, "dt", "finite")
    for bad in (-0.01, 1.01, nan, inf):
        _refused(run(make(flip=bad)), fn, "flip")
    for name, idx in (("position_in", 1), ("velocity_in", 0), ("position_out", 2), ("velocity_out", 1), ("grid_new", 0)):
        d = make()
        getattr(d, name)[idx] = None
        _refused(run(d), fn, name + f"[{idx}]", "NULL")
    d = make()
    d.grid_old[1] = None
    _refused(run(d), fn, "grid_old", "all three")
    d = make()
    for a in range(3):
        d.grid_old[a] = None
    _refused(run(d), fn, "grid_old", "flip > 0")
    d = make()
    d.position_out[0] = d.position_in[0] + 4  # a partial overlap; the array itself (in place) is allowed
    _refused(run(d), fn, "position_in[0]", "position_out[0]", "overlap")
    d = make()
    d.velocity_out[1] = d.position_in[1]
    _refused(run(d), fn, "position_in[1]", "velocity_out[1]", "overlap")
    d = make()
    d.velocity_out[0] = d.velocity_in[0]
    d.position_out[2] = d.grid_new[2] + 64
    _refused(run(d), fn, "grid_new[2]", "position_out[2]", "overlap")


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the scenes are read-only)


def _dev3(arrays):
    return [_dev(q) for q in arrays]


def _host(t):
    return t.cpu().numpy()


def _equal(got, want, what):
    got = _host(got)
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))


def _close(got, want, scale, what, where=None):
    """the tolerance of the module's docstring on the entries `where`, equal bits elsewhere; prints the worst error in units of it"""
    got = _host(got)
    assert got.shape == want.shape
    where = np.ones(want.shape, bool) if where is None else where
    assert np.array_equal(_bits(got)[~where], _bits(want)[~where]), what
    g, w = got[where].astype(np.float64), want[where].astype(np.float64)
    bound = 2.0 ** -24 * np.abs(w) + 1e-9 * scale
    err = np.abs(g - w)
    print(f"{what}: worst |got - want| = {err.max():.3e}, worst error / bound = {(err / bound).max():.3f}, unequal {int((g != w).sum())}")
    assert (err <= bound).all(), (what, float((err / bound).max()), int((~(err <= bound)).sum()))


def _vmax(name):
    return max(float(np.abs(v).max()) for v in scene(name)["velocity"])


def _bin_on_device(name, fill=7777.0, permutation=None):
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    s = scene(name)
    pick = (lambda q: q) if permutation is None else (lambda q: q[permutation])  # noqa: E731
    pos, vel = _dev3([pick(q) for q in s["position"]]), _dev3([pick(q) for q in s["velocity"]])
    n, cells = len(s["position"][0]), int(np.prod(s["shape"]))
    out = ([torch.full_like(q, fill) for q in pos], [torch.full_like(q, fill) for q in vel],
           torch.full((n,), -5, dtype=torch.int32, device="cuda"), torch.full((cells + 2,), -5, dtype=torch.int32, device="cuda"))
    return F.binParticles(pos, vel, s["shape"], out=out)


def _to_grid_on_device(name, position, velocity, cell_start, fill=7777.0, form="default"):
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    shape = scene(name)["shape"]
    new = lambda dtype, value: [torch.full(AR.grid_shape(shape, a + 1), value, dtype=dtype, device="cuda") for a in range(3)]  # noqa: E731
    out = (new(torch.float32, fill), new(torch.float32, fill), new(torch.uint8, 77), torch.full(shape, fill, dtype=torch.float32, device="cuda"))
    return F.particlesToGrid(position, velocity, cell_start, shape, RADIUS, 0.5, out=out, form=form)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_bin_equals_the_restatement(name):
    pos, vel, order, cell_start, counts = _bin_on_device(name)
    want = binned(name)
    _equal(order, want["order"], "order")
    _equal(cell_start, want["cell_start"], "cell_start")
    for c in range(3):
        _equal(pos[c], want["position"][c], f"position[{c}]")
        _equal(vel[c], want["velocity"][c], f"velocity[{c}]")
    assert counts.tolist() == want["counts"]


@pytest.mark.gpu
def test_bin_without_velocities_and_without_particles():
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    s, want = scene("row65"), binned("row65")
    pos, vel, order, cell_start, counts = F.binParticles(_dev3(s["position"]), None, s["shape"])
    assert vel is None and counts.tolist() == want["counts"]
    _equal(order, want["order"], "order")
    _equal(pos[1], want["position"][1], "position[1]")
    none = [torch.empty(0, device="cuda")] * 3
    pos, vel, order, cell_start, counts = F.binParticles(none, none, (3, 4, 5))
    assert counts.tolist() == [0, 0] and not cell_start.any() and cell_start.numel() == 62
    vout, wout, known, phi, counts = F.particlesToGrid(pos, vel, cell_start, (3, 4, 5), 0.5, 2.0)
    assert counts.tolist() == [0, 0] and not any(bool(q.any()) for q in vout + wout + known) and bool((phi == 2.0).all())
    pos, vel = F.updateParticles(pos, vel, vout, DT, vout)
    assert pos[0].numel() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("form", FORMS)
def test_to_grid_equals_the_restatement(form, name):
    b, want = binned(name), gridded(name)
    vout, wout, known, phi, counts = _to_grid_on_device(name, _dev3(b["position"]), _dev3(b["velocity"]), _dev(b["cell_start"]), form=form)
    for a in range(3):
        _equal(known[a], want["known"][a], f"known[{a}]")
        _close(vout[a], want["velocity"][a], _vmax(name), f"{name} {form} velocity[{a}]")
        _close(wout[a], want["weight"][a], _vmax(name), f"{name} {form} weight[{a}]")
    _equal(phi, want["phi"], "liquid_phi")
    assert counts.tolist() == want["counts"]


@pytest.mark.gpu
def test_to_grid_without_phi_and_weights_writes_the_same_velocity():
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    b, shape = binned("row131"), scene("row131")["shape"]
    args = (_dev3(b["position"]), _dev3(b["velocity"]), _dev(b["cell_start"]), shape, RADIUS, 0.5)
    full = F.particlesToGrid(*args)
    faces = [AR.grid_shape(shape, a + 1) for a in range(3)]
    out = ([torch.empty(f, device="cuda") for f in faces], None, [torch.empty(f, dtype=torch.uint8, device="cuda") for f in faces], None)
    vout, wout, known, phi, counts = F.particlesToGrid(*args, out=out)
    assert phi is None and wout is None and counts.tolist() == full[4].tolist()
    assert all(torch.equal(vout[a], full[0][a]) and torch.equal(known[a], full[2][a]) for a in range(3))
    assert F.particlesToGrid(*args, want_phi=False)[3] is None


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("order", [1, 2])
def test_update_equals_the_restatement_in_place_and_out_of_place(name, order):
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    s, b, want = scene(name), binned(name), updated(name, order)
    ok = PR.inside(b["position"], s["shape"])
    grid_new, grid_old = _dev3(s["grid_new"]), _dev3(s["grid_old"])
    pos, vel = _dev3(b["position"]), _dev3(b["velocity"])
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = ([torch.full_like(q, 7777.0) for q in pos], [torch.full_like(q, 7777.0) for q in vel])
    pout, vout = F.updateParticles(pos, vel, grid_new, DT, grid_old, 0.95, order, out=out, counts=counts)
    vscale = max(_vmax(name), max(float(np.abs(g).max()) for g in s["grid_new"] + s["grid_old"]))
    for c in range(3):
        _close(pout[c], want["position"][c], float(max(s["shape"])), f"{name} order {order} position[{c}]", ok)
        _close(vout[c], want["velocity"][c], vscale, f"{name} order {order} velocity[{c}]", ok)
        assert bool((pout[c][torch.from_numpy(ok).cuda()] >= 0).all()) and bool((pout[c][torch.from_numpy(ok).cuda()] <= s["shape"][2 - c]).all())
    assert counts.tolist() == want["counts"]
    # in place: the same bits (positions and velocities both, then the positions alone)
    F.updateParticles(pos, vel, grid_new, DT, grid_old, 0.95, order, out=(pos, vel))
    assert all(np.array_equal(_bits(_host(a)), _bits(_host(b_))) for a, b_ in zip(pos + vel, pout + vout))
    pos = _dev3(b["position"])
    _, v2 = F.updateParticles(pos, _dev3(b["velocity"]), grid_new, DT, grid_old, 0.95, order, out=(pos, [torch.empty_like(q) for q in pos]))
    assert all(np.array_equal(_bits(_host(a)), _bits(_host(b_))) for a, b_ in zip(pos + v2, pout + vout))


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 2])
def test_update_exact_cases(order):
    """dt = 0 leaves positions as they are; flip = 1 with old = new leaves velocities as they are; flip = 0 is float(U_new(x))"""
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    s, b = scene("grid"), binned("grid")
    grid_new, grid_old = _dev3(s["grid_new"]), _dev3(s["grid_old"])
    pos, vel = _dev3(b["position"]), _dev3(b["velocity"])
    finite = lambda ts: [torch.nan_to_num(t, nan=-1.0, posinf=-2.0, neginf=-3.0) for t in ts]  # noqa: E731  (torch.equal: NaN != NaN)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    pout, _ = F.updateParticles(pos, vel, grid_new, 0.0, grid_old, 0.95, order, counts=counts)
    assert all(torch.equal(a, b_) for a, b_ in zip(finite(pout), finite(pos))) and counts.tolist() == [0, 11]
    _, vout = F.updateParticles(pos, vel, grid_new, DT, grid_new, 1.0, order)
    assert all(torch.equal(a, b_) for a, b_ in zip(vout, vel))
    _, vout = F.updateParticles(pos, vel, grid_new, DT, None, 0.0, order)
    want = PR.update(b["position"], b["velocity"], s["grid_new"], None, s["shape"], DT, 0.0, order)
    ok = PR.inside(b["position"], s["shape"])
    for c in range(3):
        _close(vout[c], want["velocity"][c], max(float(np.abs(g).max()) for g in s["grid_new"]), f"flip = 0, velocity[{c}]", ok)


@pytest.mark.gpu
def test_two_runs_give_the_same_bits_whatever_the_outputs_held():
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    s = scene("grid")
    grid_new, grid_old = _dev3(s["grid_new"]), _dev3(s["grid_old"])
    runs = []
    for fill, form in ((float("nan"), "gather"), (-3.0e7, "staged")):  # (the two kernels give the same bits as well)
        pos, vel, order, cell_start, counts = _bin_on_device("grid", fill)
        vout, wout, known, phi, gcounts = _to_grid_on_device("grid", pos, vel, cell_start, fill, form)
        out = ([torch.full_like(q, fill) for q in pos], [torch.full_like(q, fill) for q in vel])
        pout, uout = F.updateParticles(pos, vel, grid_new, DT, grid_old, 0.95, 2, out=out)
        runs.append(pos + vel + [order, cell_start, counts] + vout + wout + known + [phi, gcounts] + pout + uout)
    assert len(runs[0]) == 26
    for a, b in zip(*runs):
        a, b = _host(a), _host(b)
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float32 else np.array_equal(a, b)
    assert all(bool(torch.isfinite(q).all()) for q in runs[0][9:19])  # (the ten grids; the particles hold the scene's NaN)


@pytest.mark.gpu
def test_shuffled_input_gives_the_same_grids():
    import torch

    name = "grid"
    n = len(scene(name)["position"][0])
    results = []
    for permutation in (None, np.random.default_rng(5).permutation(n)):
        pos, vel, order, cell_start, counts = _bin_on_device(name, permutation=permutation)
        results.append((cell_start, counts) + _to_grid_on_device(name, pos, vel, cell_start))
    a, b = results
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[6], b[6])
    assert torch.equal(a[5], b[5])  # liquid_phi: a min does not care about the order
    for c in range(3):
        assert torch.equal(a[4][c], b[4][c])
        _close(b[2][c], _host(a[2][c]), _vmax(name), f"shuffled velocity[{c}]")
        _close(b[3][c], _host(a[3][c]), _vmax(name), f"shuffled weight[{c}]")


@pytest.mark.gpu
def test_a_wrong_cell_start_gives_finite_values():
    """entries beyond n and negative ones, on a tiny grid: the call returns and every output is finite -- only that"""
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    shape = (3, 5, 6)
    position, rng = _cloud(shape, 200, 0.0, 9)
    velocity = [rng.uniform(-1.0, 1.0, 200).astype(np.float32) for _ in range(3)]
    b = PR.bin_particles(position, velocity, shape)
    wrong = rng.integers(-300, 500, len(b["cell_start"])).astype(np.int32)
    for form in FORMS:
        vout, wout, known, phi, counts = F.particlesToGrid(_dev3(b["position"]), _dev3(b["velocity"]), _dev(wrong), shape, RADIUS, form=form)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(q).all()) for q in vout + wout + [phi]) and all(bool((q <= 1).all()) for q in known)


@pytest.mark.gpu
def test_a_drop_in_free_flight_carried_by_particles():
    """Section 21's drop with particles: a ball of radius 8 cells in 40^3 without solids, seedParticles at 8 per cell, every particle
    at U with dt U = 1.7 (0.37, 0.21, -0.13); twelve sub-steps of binParticles, particlesToGrid, redistance, extrapolateVelocity (known,
    8 layers), project_free_surface, extrapolateVelocity, updateParticles (flip = 0.95).  Every projection converges; no particle is
    lost or leaves the box; particle velocities stay within 1e-5 |U| of U; the particles' centroid lands within 0.25 cell of the start
    plus 12 dt U.  The cells with phi < 0 are printed, not asserted."""
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    shape, radius, steps, dt, tolerance = (40, 40, 40), 8.0, 12, 1.7, 1e-5
    U = np.array([0.37, 0.21, -0.13], dtype=np.float32)
    start = np.array([14.0, 16.0, 22.0])
    x, s, _ = AR.targets(shape, 0)
    ball = (np.sqrt(((x - start) ** 2).sum(axis=1)) - radius).reshape(s).astype(np.float32)
    pos = F.seedParticles(torch.from_numpy(ball).cuda(), per_cell=8, seed=7)
    n = pos[0].numel()
    assert n == 8 * int((ball < 0).sum())
    vel = [torch.full((n,), float(U[a]), device="cuda") for a in range(3)]
    centroid = lambda p: np.array([float(q.double().mean()) for q in p])  # noqa: E731
    first = centroid(pos)
    solid_phi = np.full(shape, -1.0, dtype=np.float32)  # (a cell that is not liquid is solid where solid_phi >= 0: none is)
    cw = [np.ones(AR.grid_shape(shape, a + 1), dtype=np.float32) for a in range(3)]
    pressure = np.zeros(shape, dtype=np.float32)
    lost = torch.zeros(2, dtype=torch.int64, device="cuda")
    cells = []
    for step in range(steps):
        pos, vel, _, cell_start, counts = F.binParticles(pos, vel, shape)
        assert counts[0] == 0
        grid, _, known, phi, gcounts = F.particlesToGrid(pos, vel, cell_start, shape, RADIUS)
        phi = F.redistance(phi, 3.0)
        cells.append(int((phi < 0).sum()))
        F.extrapolateVelocity(grid, known, 8)
        velocity = [_host(g) for g in grid]  # grid_old: the particles' velocity on the grid, before the projection
        valid, info = F.project_free_surface(_host(phi), solid_phi, cw, velocity, pressure, tolerance=tolerance)
        assert info["outcome"] in (0, 1, 2), (step, info)  # converged, zero right-hand side, converged at the start
        projected = _dev3(velocity)
        F.extrapolateVelocity(projected, _dev3(valid), 8)
        pos, vel = F.updateParticles(pos, vel, projected, dt, grid, 0.95, 2, out=(pos, vel), counts=lost)
        off = max(float((vel[a] - float(U[a])).abs().max()) for a in range(3))
        assert off <= tolerance * float(np.abs(U).max()), (step, off)
    assert pos[0].numel() == n and lost.tolist() == [0, 0]
    off = float(np.linalg.norm(centroid(pos) - (first + steps * dt * U.astype(np.float64))))
    print(f"particles: cells of phi < 0 {cells[0]} -> {cells[-1]} (the ball: {int((ball < 0).sum())}), centroid off by {off:.4f} cell")
    assert off <= 0.25, off
