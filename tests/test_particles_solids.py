"""FLIP particles next to solids (include/mgps_fields.h, "FLIP particles next to solids") against
tests/particles_solids_reference.py: collide, the fused update, resample.

CPU: the restatement against analysis (an exact plane, untouched bits, friction 0 and 1, the stride rule, the seeded cell, the hash),
the condition that the scenes are in generic position, the C ABI's refusals and the ctypes mirrors' sizes.
GPU: collide against the restatement; the fused update bit-equal to update then collide; resample against the restatement, at a
capacity too small and with a wrong cell_start; a liquid ball that falls onto a rasterised sphere, carried by particles.

Scenes.  Section 23's five (test_particles.scene: shapes, particles, face grids), each with an analytic float32 solid_phi in cells --
the union of a small tilted half-space at the corner (0, 0, 0) and a sphere whose centre is a cell centre and which reaches through the
wall y = 0 --, smooth solid-velocity face grids, and 200 particles put into the sphere at depths of 0 .. 3 cells, a dozen into the
half-space and three at the sphere's centre, where the gradient vanishes (the stuck path); pushes out of the sphere towards y < 0 take
the clampB path.

Tolerance (section 23's).  Counts, cell_start_out, n_out and which particles were pushed, kept or seeded are EQUAL; seeded positions
and every copied value are BIT-EQUAL; positions and velocities that the device computes: |got - want| <= 2^-24 |want| + 1e-9 scale,
scale = max g_c for positions and max |v| for velocities.  Generic position is a condition: the restatement counts the particles with
a decision closer than 1e-9 to its threshold (its docstring has the list), and a CPU test asserts 0 for every configuration used."""
import ctypes as C
import functools

import numpy as np
import pytest

import advection_reference as AR
import particles_reference as PR
import particles_solids_reference as SR
import test_particles as TP
from refusals import refused as _refused

DT = TP.DT
MARGIN, FRICTION = 0.1, 0.25
SOLID_SEEDS = {"grid": 1, "row64": 1, "row65": 1, "row131": 1, "sheet": 1}  # chosen so that the scenes are in generic position (a CPU test)
CONFIGS = [(iterations, moving) for iterations in (1, 3) for moving in (False, True)]
RESAMPLE_SEED = 2024


def _solid_grids(shape, rng):
    """solid_phi (float32, cells): min(tilted half-space at the corner, sphere), the sphere's centre and radius, the plane (n, D)"""
    gz, gy, gx = shape
    x, s, _ = AR.targets(shape, 0)
    n = np.array([1.0, 0.8, 0.6 if gz > 1 else 0.0])
    n /= np.linalg.norm(n)
    D = 1.2 + 0.3 * rng.uniform()
    radius = 4.1 if gz > 8 else 3.3  # (no cell centre lies on the sphere: no solid_phi value is 0)
    centre = np.array([gx - 11.5, 2.5, 5.5 if gz > 8 else (2.5 if gz > 1 else 0.5)])
    d = x - centre
    sphere = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) - radius
    phi = np.minimum(x @ n - D, sphere).astype(np.float32).reshape(s)
    return phi, centre, radius, n, D


@functools.lru_cache(maxsize=None)
def solid_scene(name):
    """section 23's scene `name` with the solid's grids and the particles in the solid added; float32, read-only"""
    base = TP.scene(name)
    shape = base["shape"]
    gz, gy, gx = shape
    rng = np.random.default_rng(1000 + SOLID_SEEDS[name])
    box = TP._box(shape)
    phi, centre, radius, n, D = _solid_grids(shape, rng)
    extra = []
    while len(extra) < 12:  # in the half-space, which is exactly planar (see the restatement's docstring): a few
        p = rng.uniform(0.0, 1.0, 3) * np.minimum(box, 3.0)
        if p @ n - D <= 0.0:
            extra.append(p)
    while len(extra) < 12 + 200:  # in the sphere, at depths 0 .. 3, inside the box
        u = rng.normal(size=3)
        if gz == 1:
            u[2] = 0.0
        p = centre + (radius - rng.uniform(0.0, 3.0)) * u / np.linalg.norm(u)
        if (p >= 0).all() and (p <= box).all():
            extra.append(p)
    extra += [centre.copy()] * 3
    extra = np.array(extra)
    position = [np.concatenate([base["position"][c], extra[:, c].astype(np.float32)]) for c in range(3)]
    velocity = [np.concatenate([base["velocity"][c], (1.5 * rng.uniform(-1.0, 1.0, len(extra))).astype(np.float32)]) for c in range(3)]
    sv = [(0.4 * g).astype(np.float32) for g in TP._face_grids(shape, rng, 2.1)]
    out = {"shape": shape, "position": position, "velocity": velocity, "solid_phi": phi, "solid_velocity": sv,
           "grid_new": base["grid_new"], "grid_old": base["grid_old"]}
    for key in ("position", "velocity", "solid_velocity"):
        for q in out[key]:
            q.setflags(write=False)
    phi.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def collided(name, iterations, moving):
    s = solid_scene(name)
    return SR.collide(s["position"], s["velocity"], s["solid_phi"], s["solid_velocity"] if moving else None, s["shape"], MARGIN, iterations, FRICTION)


def _liquid_phi(shape, dx):
    """a liquid below y = 0.62 gy with a ripple, in phi's units; no value is a threshold of the tests (a CPU test)"""
    x, s, _ = AR.targets(shape, 0)
    return (dx * (x[:, 1] - 0.62 * shape[1] + 0.3 * np.sin(0.7 * x[:, 0] + 0.4 * x[:, 2]))).astype(np.float32).reshape(s)


RESAMPLE_DX, RESAMPLE_DEPTH = 0.5, 1.0


@functools.lru_cache(maxsize=None)
def resampled(name, least, most, keep_outside, empty=False):
    s, b = solid_scene(name), TP.binned(name)
    shape = s["shape"]
    pos, vel, start = b["position"], b["velocity"], b["cell_start"]
    if empty:
        pos, vel, start = [q[:0] for q in pos], [q[:0] for q in vel], np.zeros_like(start)
    return SR.resample(pos, vel, start, shape, least, most, _liquid_phi(shape, RESAMPLE_DX), RESAMPLE_DX, RESAMPLE_DEPTH, s["solid_phi"], s["grid_new"],
                       RESAMPLE_SEED, keep_outside)


_bits = TP._bits


# ---- CPU: the restatement against analysis -------------------------------------------------------------------------------------------
def _plane(shape, n, D):
    x, s, _ = AR.targets(shape, 0)
    return (x @ n - D).reshape(s)  # fp64: an exactly planar grid, which S reproduces to round-off


def test_restated_push_out_of_an_exact_plane_lands_on_the_margin():
    shape = (12, 12, 12)
    n = np.array([0.48, -0.6, 0.64])
    D = n @ np.array([6.0, 6.0, 6.0])
    rng = np.random.default_rng(3)
    foot = np.array([6.0, 6.0, 6.0]) + rng.uniform(-1.0, 1.0, (300, 3))
    foot -= ((foot @ n - D))[:, None] * n  # on the plane
    depth = rng.uniform(0.0, 3.0, 300)
    x = foot - depth[:, None] * n
    assert (x >= 1.0).all() and (x <= 11.0).all()  # (a cell from every wall: S sees the plane, not its clamp)
    position = [x[:, c].astype(np.float32) for c in range(3)]
    velocity = [rng.uniform(-1.0, 1.0, 300).astype(np.float32) for _ in range(3)]
    r = SR.collide(position, velocity, _plane(shape, n, D), None, shape, 0.1, 1, 0.0)
    assert r["counts"] == [300, 0, 0] and r["pushed"].all()
    assert np.abs(r["end"] @ n - D - 0.1).max() <= 1e-12 and np.abs(r["normal"] - n).max() <= 1e-12  # the fp64 end point, before the store
    assert all(np.array_equal(r["position"][c], r["end"][:, c].astype(np.float32)) for c in range(3))
    p = np.stack([q.astype(np.float64) for q in position], axis=1)
    assert np.abs(np.cross(r["end"] - p, n)).max() <= 1e-12  # along the normal
    # friction 0: the tangential velocity stays, the normal velocity does not point into the solid
    v = np.stack([q.astype(np.float64) for q in velocity], axis=1)
    w = np.stack([q.astype(np.float64) for q in r["velocity"]], axis=1)
    vn, wn = v @ n, w @ n
    assert np.abs((w - wn[:, None] * n) - (v - vn[:, None] * n)).max() <= 1e-6 and wn.min() >= -1e-6
    assert (vn < 0).sum() > 100 and np.abs(wn[vn < 0]).max() <= 1e-6 and np.abs(w[vn >= 0] - v[vn >= 0]).max() <= 1e-7


def test_restated_friction_ends_and_untouched_bits():
    s = solid_scene("row65")
    shape = s["shape"]
    ok = PR.inside(s["position"], shape)
    for moving in (False, True):
        sv = s["solid_velocity"] if moving else None
        free = SR.collide(s["position"], s["velocity"], s["solid_phi"], sv, shape, MARGIN, 2, 0.0)
        full = SR.collide(s["position"], s["velocity"], s["solid_phi"], sv, shape, MARGIN, 2, 1.0)
        pushed = free["pushed"]
        assert pushed.sum() > 200 and np.array_equal(pushed, full["pushed"]) and not pushed[~ok].any()
        for r in (free, full):  # untouched particles keep their bits (the NaN ones too)
            for c in range(3):
                assert np.array_equal(_bits(r["position"][c])[~pushed], _bits(s["position"][c])[~pushed])
                assert np.array_equal(_bits(r["velocity"][c])[~pushed], _bits(s["velocity"][c])[~pushed])
        us = AR.velocity_at(sv, shape, free["end"][pushed])[0] if moving else np.zeros((int(pushed.sum()), 3))
        n = free["normal"][pushed]
        v = np.stack([q[pushed].astype(np.float64) for q in s["velocity"]], axis=1) - us
        w = free["relative"][pushed]  # fp64, before the store
        vn, wn = (v * n).sum(axis=1), (w * n).sum(axis=1)
        # friction 0: the tangential relative velocity is unchanged, vn_out >= 0
        assert np.abs((w - wn[:, None] * n) - (v - vn[:, None] * n)).max() <= 1e-12 and wn.min() >= -1e-12
        assert np.array_equal(w[vn >= 0], v[vn >= 0])
        # friction 1: a particle that moved into the solid leaves with the solid's velocity
        into = vn < 0
        assert into.sum() > 50 and not full["relative"][pushed][into].any()
        for c in range(3):
            assert np.array_equal(full["velocity"][c][pushed][into], us[into, c].astype(np.float32))


def test_restated_stride_rule_keeps_exactly_max_slots_in_order():
    for most in range(1, 65):
        for m in range(1, 201):
            keep = SR.kept_slots(m, most)
            assert int(keep.sum()) == min(m, most), (m, most)
            if m > most:  # evenly strided: the gaps between kept slots differ by one at the most
                gaps = np.diff(np.nonzero(keep)[0])
                assert len(gaps) == 0 or gaps.max() - gaps.min() <= 1
                # the closed form of the rank that the copy kernel uses
                t = np.arange(m)
                assert np.array_equal(np.cumsum(keep) - keep, t * most // m)


def test_restated_seeded_particles_lie_in_their_cell_and_the_hash_is_pinned():
    assert [int(v) for v in SR.mix(np.array([0, 1, 2, 0x9E3779B9, 0xFFFFFFFF]))] == PINNED_MIX
    index = np.arange(4000)
    for i in (0, 1, 1023, 262143):
        ijk = np.full((4000, 3), i)
        for seed in (0, 7, 0xFFFFFFFF):
            x = SR.seeded_position(seed, np.full(4000, 12345), index, ijk)
            for a in range(3):
                assert x[a].dtype == np.float32 and np.array_equal(np.floor(x[a]).astype(np.int64), ijk[:, a])
    x = SR.seeded_position(5, np.array([3, 3, 4]), np.array([0, 1, 0]), np.array([[3, 0, 0], [3, 0, 0], [4, 0, 0]]))
    assert [[float(v) for v in q] for q in x] == PINNED_SEEDED
    r = (SR.mix(np.arange(100000)) >> 8).astype(np.float64) * 2.0 ** -24
    assert 0.0 <= r.min() and r.max() < 1.0 and abs(r.mean() - 0.5) < 0.01


# mix of 0, 1, 2, 0x9e3779b9, 0xffffffff; the particles (seed 5: cell 3 index 0, cell 3 index 1, cell 4 index 0) per axis
PINNED_MIX = [0, 1753845952, 3507691905, 33350994, 1734902346]
PINNED_SEEDED = [[3.584669828414917, 3.7243216037750244, 4.083748817443848], [0.7486441731452942, 0.09757953882217407, 0.8125662803649902],
                 [0.7178364992141724, 0.5989094972610474, 0.6816464066505432]]


@pytest.mark.parametrize("name", list(TP.SCENES))
def test_scenes_are_in_generic_position_and_hold_what_they_should(name):
    s = solid_scene(name)
    ok = PR.inside(s["position"], s["shape"])
    for iterations, moving in CONFIGS:
        r = collided(name, iterations, moving)
        assert r["nongeneric"] == 0, (iterations, moving, r["nongeneric"])
        assert r["counts"][0] >= 200 and r["counts"][2] >= 3 and not r["pushed"][~ok].any()
    one, three = collided(name, 1, True), collided(name, 3, True)
    assert one["counts"][1] >= three["counts"][1]
    # the clampB path: a pushed particle ends on the wall y = 0
    assert (three["position"][1][three["pushed"]] == 0).sum() >= 1
    # the update of section 23 followed by collide, as the fused kernel runs it, is not asserted generic: that test is bit-equality


def test_resample_restated_counts_and_cells():
    name = "grid"
    s, b = solid_scene(name), TP.binned(name)
    shape = s["shape"]
    cells = int(np.prod(shape))
    phi = _liquid_phi(shape, RESAMPLE_DX)
    assert not (phi == -np.float32(RESAMPLE_DEPTH * RESAMPLE_DX)).any() and not (s["solid_phi"] == 0).any()
    m = np.diff(b["cell_start"][:cells + 1])
    outside = int(b["cell_start"][cells + 1] - b["cell_start"][cells])
    assert m.max() >= TP.CROWD and outside == 11
    for keep in (False, True):
        r = resampled(name, 4, 16, keep)
        per = np.diff(r["cell_start"][:cells + 1])
        assert np.array_equal(per, r["per_cell"]) and per.max() == 16 and (per[r["deep"]] >= 4).all()
        assert r["counts"][0] == int(np.maximum(m - 16, 0).sum()) > 1000 and r["counts"][1] > 1000 and 0 < r["counts"][2] < cells
        assert r["n_out"] == int(np.minimum(m, 16).sum()) + r["counts"][1] + (outside if keep else 0)
        assert r["cell_start"][cells] == r["n_out"] - (outside if keep else 0) and r["cell_start"][cells + 1] == r["n_out"]
        # binned: the keys of the output ascend, every particle lies in the cell that holds its slot
        key = PR.keys(r["position"], shape)
        assert (np.diff(key) >= 0).all() and np.array_equal(np.searchsorted(key, np.arange(cells + 2), side="left"), r["cell_start"])
        kept = r["source"][r["source"] >= 0]
        assert (np.diff(kept) > 0).all()  # kept particles hold their order
    thin = resampled(name, 0, 16, False)
    assert thin["counts"][1] == 0 and thin["n_out"] == int(np.minimum(m, 16).sum())
    allnew = resampled(name, 4, 16, False, True)
    assert allnew["counts"] == [0, 4 * allnew["counts"][2], allnew["counts"][2]] and allnew["n_out"] == allnew["counts"][1] > 0


# ---- CPU: refusals and the mirrors -----------------------------------------------------------------------------------------------------
def _desc(kind, **kw):
    """a good desc on made-up addresses, 16 MiB apart (never dereferenced: every call below is refused on the host)"""
    from geometricmultigridpressuresolver_amd import fields as F

    cls, names = {
        "collide": (F.ParticlesCollideDesc, ("position_in", "velocity_in", "position_out", "velocity_out", "solid_phi", "solid_velocity", "counts_dev")),
        "update": (F.ParticlesUpdateDesc, ("position_in", "velocity_in", "position_out", "velocity_out", "grid_new", "grid_old")),
        "resample": (F.ParticlesResampleDesc, ("position", "velocity", "cell_start", "liquid_phi", "solid_phi", "grid", "position_out", "velocity_out",
                                               "cell_start_out", "n_out_dev", "counts_dev")),
    }[kind]
    d = cls()
    d.struct_size = C.sizeof(cls)
    d.gx, d.gy, d.gz, d.n = 6, 5, 4, 100
    if kind == "collide":
        d.margin, d.iterations, d.friction = 0.1, 2, 0.5
    if kind == "update":
        d.dt, d.flip, d.trace_order = 0.5, 0.95, 2
    if kind == "resample":
        d.capacity, d.min_per_cell, d.max_per_cell, d.dx, d.seed_depth = 500, 4, 16, 0.5, 1.0
    TP._fill(d, names, iter(range(64 if kind == "update" else 1, 128)))
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_refusals_need_no_device_and_the_mirrors_have_the_library_sizes():
    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd._lib import lib

    L = lib()
    assert (C.sizeof(F.ParticlesCollideDesc), C.sizeof(F.ParticlesResampleDesc), C.sizeof(F.ParticlesUpdateDesc)) == (176, 224, 192)
    nan, inf = float("nan"), float("inf")
    collide = lambda d: L.mgps_particles_collide(C.byref(d), None)  # noqa: E731
    fused = lambda d: L.mgps_particles_update_solid(C.byref(_desc("update")), C.byref(d), None)  # noqa: E731
    resample = lambda d: L.mgps_particles_resample(C.byref(d), None)  # noqa: E731
    # what the collide desc is refused for, by both entries that take it
    for fn, run in (("mgps_particles_collide", collide), ("mgps_particles_update_solid", fused)):
        make = functools.partial(_desc, "collide")
        d = make()
        d.struct_size -= 8
        _refused(run(d), fn, "struct_size", "mgps_particles_collide_desc")
        for k in ("gx", "gy", "gz"):
            _refused(run(make(**{k: 0})), fn, "extent")
        _refused(run(make(gx=2048, gy=1024, gz=1024)), fn, "too many cells", "int32")
        for bad in (-0.01, nan, inf):
            _refused(run(make(margin=bad)), fn, "margin")
        for bad in (0, 5, -1):
            _refused(run(make(iterations=bad)), fn, "iterations", "1 .. 4")
        for bad in (-0.01, 1.01, nan):
            _refused(run(make(friction=bad)), fn, "friction")
        _refused(run(make(solid_phi=None)), fn, "solid_phi", "NULL")
        d = make()
        d.solid_velocity[1] = None
        _refused(run(d), fn, "solid_velocity", "all three")
    fn, make = "mgps_particles_collide", functools.partial(_desc, "collide")
    _refused(L.mgps_particles_collide(None, None), fn, "struct_size")
    _refused(collide(make(n=-1)), fn, "negative")
    for name, idx in (("position_in", 1), ("velocity_in", 0), ("position_out", 2), ("velocity_out", 1)):
        d = make()
        getattr(d, name)[idx] = None
        _refused(collide(d), fn, name + f"[{idx}]", "NULL")
    d = make()
    d.position_out[0] = d.position_in[0] + 4  # a partial overlap; the array itself (in place) is allowed
    _refused(collide(d), fn, "position_in[0]", "position_out[0]", "overlap")
    d = make()
    d.velocity_out[2] = d.solid_phi + 8
    _refused(collide(d), fn, "solid_phi", "velocity_out[2]", "overlap")
    d = make()
    d.position_out[1] = d.solid_velocity[0]
    _refused(collide(d), fn, "solid_velocity[0]", "position_out[1]", "overlap")
    d = make()
    d.counts_dev = d.velocity_in[1] + 8
    _refused(collide(d), fn, "velocity_in[1]", "counts_dev", "overlap")
    # the fused entry: the update desc's refusals under its name, the two descs of one grid, overlaps across the descs
    fn = "mgps_particles_update_solid"
    both = lambda u, s: L.mgps_particles_update_solid(C.byref(u), C.byref(s), None)  # noqa: E731
    _refused(L.mgps_particles_update_solid(None, C.byref(make()), None), fn, "struct_size", "mgps_particles_update_desc")
    _refused(L.mgps_particles_update_solid(C.byref(_desc("update")), None, None), fn, "struct_size", "mgps_particles_collide_desc")
    _refused(both(_desc("update", trace_order=3), make()), fn, "trace_order")
    _refused(both(_desc("update", flip=1.5), make()), fn, "flip")
    _refused(both(_desc("update", dt=nan), make()), fn, "dt", "finite")
    _refused(both(_desc("update", n=-1), make()), fn, "negative")
    u = _desc("update")
    u.grid_new[2] = None
    _refused(both(u, make()), fn, "grid_new[2]", "NULL")
    _refused(both(_desc("update"), make(gy=6)), fn, "one grid")
    u, s = _desc("update"), make()
    u.position_out[0] = s.solid_phi
    _refused(both(u, s), fn, "position_out[0]", "solid_phi", "overlap")
    u, s = _desc("update"), make()
    u.velocity_out[1] = s.solid_velocity[2] + 16
    _refused(both(u, s), fn, "velocity_out[1]", "solid_velocity[2]", "overlap")
    # resample
    fn, make = "mgps_particles_resample", functools.partial(_desc, "resample")
    _refused(L.mgps_particles_resample(None, None), fn, "struct_size")
    d = make()
    d.struct_size += 8
    _refused(resample(d), fn, "struct_size")
    for k in ("gx", "gy", "gz"):
        _refused(resample(make(**{k: 0})), fn, "extent")
    _refused(resample(make(gx=2048, gy=1024, gz=1024)), fn, "too many cells", "int32")
    _refused(resample(make(n=-1)), fn, "negative")
    _refused(resample(make(capacity=-1)), fn, "capacity")
    for bad in (0, 65, -3):
        _refused(resample(make(max_per_cell=bad, min_per_cell=0)), fn, "max_per_cell", "1 .. 64")
    for bad in (-1, 17):
        _refused(resample(make(min_per_cell=bad)), fn, "min_per_cell")
    for bad in (-1, 2):
        _refused(resample(make(keep_outside=bad)), fn, "keep_outside")
    for bad in (0.0, -1.0, nan, inf):
        _refused(resample(make(dx=bad)), fn, "dx")
    for bad in (-0.5, nan, inf):
        _refused(resample(make(seed_depth=bad)), fn, "seed_depth")
    _refused(resample(make(gx=1024, gy=1024, gz=512, min_per_cell=4)), fn, "2^31", "min_per_cell")
    d = make()
    d.grid[0] = None
    _refused(resample(d), fn, "grid", "all three")
    _refused(resample(make(liquid_phi=None)), fn, "liquid_phi", "min_per_cell > 0")
    d = make()
    for a in range(3):
        d.grid[a] = None
    _refused(resample(d), fn, "grid", "min_per_cell > 0")
    for name, idx in (("position", 0), ("velocity", 2), ("position_out", 1), ("velocity_out", 0)):
        d = make()
        getattr(d, name)[idx] = None
        _refused(resample(d), fn, name + f"[{idx}]", "NULL")
    for name in ("cell_start", "cell_start_out", "n_out_dev"):
        _refused(resample(make(**{name: None})), fn, name, "NULL")
    d = make()
    d.position_out[0] = d.position[0]  # out of place only
    _refused(resample(d), fn, "position[0]", "position_out[0]", "overlap")
    d = make()
    d.velocity_out[1] = d.position_out[1] + 4 * 499  # the outputs have `capacity` entries
    _refused(resample(d), fn, "position_out[1]", "velocity_out[1]", "overlap")
    d = make()
    d.cell_start_out = d.cell_start + 4
    _refused(resample(d), fn, "cell_start", "cell_start_out", "overlap")
    d = make()
    d.n_out_dev = d.grid[2] + 4
    _refused(resample(d), fn, "grid[2]", "n_out_dev", "overlap")
    d = make()
    d.counts_dev = d.liquid_phi + 8
    _refused(resample(d), fn, "liquid_phi", "counts_dev", "overlap")


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------
_dev, _dev3, _host, _equal, _close = TP._dev, TP._dev3, TP._host, TP._equal, TP._close


def _scales(s):
    vmax = max(float(np.nanmax(np.abs(q))) for q in s["velocity"] + s["solid_velocity"] + s["grid_new"] + s["grid_old"])
    return float(max(s["shape"])), vmax


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TP.SCENES))
@pytest.mark.parametrize("iterations,moving", CONFIGS)
def test_collide_equals_the_restatement_in_place_and_out_of_place(name, iterations, moving):
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    s, want = solid_scene(name), collided(name, iterations, moving)
    pos, vel = _dev3(s["position"]), _dev3(s["velocity"])
    phi, sv = _dev(s["solid_phi"]), _dev3(s["solid_velocity"]) if moving else None
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    out = ([torch.full_like(q, 7777.0) for q in pos], [torch.full_like(q, 7777.0) for q in vel])
    pout, vout = F.collideParticles(pos, vel, phi, sv, MARGIN, iterations, FRICTION, out=out, counts=counts)
    print(f"{name} iterations {iterations} moving {moving}: counts {counts.tolist()}")
    assert counts.tolist() == want["counts"]
    xscale, vscale = _scales(s)
    pushed = want["pushed"]
    for c in range(3):  # (_close: equal bits wherever the restatement did not push -- which particles were pushed is EQUAL)
        _close(pout[c], want["position"][c], xscale, f"{name} position[{c}]", pushed)
        _close(vout[c], want["velocity"][c], vscale, f"{name} velocity[{c}]", pushed)
        changed = _bits(_host(pout[c])) != _bits(s["position"][c])
        assert not changed[~pushed].any()
    F.collideParticles(pos, vel, phi, sv, MARGIN, iterations, FRICTION, out=(pos, vel), counts=counts)  # in place: the same bits
    assert all(np.array_equal(_bits(_host(a)), _bits(_host(b))) for a, b in zip(pos + vel, pout + vout))
    assert counts.tolist() == [2 * v for v in want["counts"]]  # (the counts are added to)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TP.SCENES))
@pytest.mark.parametrize("order", [1, 2])
def test_fused_update_is_bit_equal_to_update_then_collide(name, order):
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    s = solid_scene(name)
    pos, vel = _dev3(s["position"]), _dev3(s["velocity"])
    grid_new, grid_old, phi, sv = _dev3(s["grid_new"]), _dev3(s["grid_old"]), _dev(s["solid_phi"]), _dev3(s["solid_velocity"])
    moved = torch.zeros(2, dtype=torch.int64, device="cuda")
    hit = torch.zeros(3, dtype=torch.int64, device="cuda")
    mid = F.updateParticles(pos, vel, grid_new, DT, grid_old, 0.95, order, counts=moved)
    two = F.collideParticles(mid[0], mid[1], phi, sv, MARGIN, 3, FRICTION, counts=hit)
    assert hit[0] > 50 and moved[1] == 11
    finite = lambda ts: [torch.nan_to_num(t, nan=-1.0, posinf=-2.0, neginf=-3.0) for t in ts]  # noqa: E731  (torch.equal: NaN != NaN)
    for fill in (float("nan"), -3.0e7):
        moved1, hit1 = torch.zeros_like(moved), torch.zeros_like(hit)
        out = ([torch.full_like(q, fill) for q in pos], [torch.full_like(q, fill) for q in vel])
        one = F.updateParticlesSolid(pos, vel, grid_new, DT, phi, grid_old, 0.95, order, sv, MARGIN, 3, FRICTION, out=out, counts=moved1, solid_counts=hit1)
        for a, b in zip(one[0] + one[1], two[0] + two[1]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(finite([a])[0], finite([b])[0])
        assert torch.equal(moved1, moved) and torch.equal(hit1, hit)
    # a solid at rest, two iterations, in place
    two = F.collideParticles(mid[0], mid[1], phi, None, MARGIN, 2, 0.0)
    F.updateParticlesSolid(pos, vel, grid_new, DT, phi, grid_old, 0.95, order, None, MARGIN, 2, 0.0, out=(pos, vel))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(pos + vel, two[0] + two[1]))


def _resample_on_device(name, least, most, keep_outside, empty=False, capacity=None, guard=64, fill=7777.0):
    """(the call's results, the whole arrays with their guard regions)"""
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    s, b, want = solid_scene(name), TP.binned(name), resampled(name, least, most, keep_outside, empty)
    shape = s["shape"]
    cells = int(np.prod(shape))
    capacity = want["n_out"] + 100 if capacity is None else capacity
    pos, vel, start = b["position"], b["velocity"], b["cell_start"]
    if empty:
        pos, vel, start = [q[:0] for q in pos], [q[:0] for q in vel], np.zeros_like(start)
    whole = [torch.full((capacity + guard,), fill, device="cuda") for _ in range(6)]
    ints = torch.full((cells + 2 + guard + 1 + guard,), -5, dtype=torch.int32, device="cuda")
    out = ([w[:capacity] for w in whole[:3]], [w[:capacity] for w in whole[3:]], ints[:cells + 2], ints[cells + 2 + guard:cells + 3 + guard])
    got = F.resampleParticles(_dev3(pos), _dev3(vel), _dev(start), shape, capacity, least, most, _dev(_liquid_phi(shape, RESAMPLE_DX)),
                              RESAMPLE_DX, RESAMPLE_DEPTH, _dev(s["solid_phi"]), _dev3(s["grid_new"]), RESAMPLE_SEED, keep_outside, out=out)
    return got, whole, ints, capacity


def _check_resampled(name, got, want, capacity):
    pout, vout, start, n_out, counts = got
    s = solid_scene(name)
    _equal(start, want["cell_start"], "cell_start_out")
    assert int(n_out) == want["n_out"] and counts.tolist() == want["counts"] + [int(want["n_out"] > capacity)]
    n = min(want["n_out"], capacity)
    seeded = want["source"][:n] < 0
    vscale = max(float(np.abs(g).max()) for g in s["grid_new"])
    for c in range(3):
        _equal(pout[c][:n], want["position"][c][:n], f"position[{c}]")  # kept: copies; seeded: the hash and one rounding
        if seeded.any():
            _close(vout[c][:n], want["velocity"][c][:n], vscale, f"{name} resampled velocity[{c}]", seeded)  # (kept: equal bits)
        else:
            _equal(vout[c][:n], want["velocity"][c][:n], f"velocity[{c}]")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["seed", "seed_keep_outside", "thin_only", "all_new", "row64", "row65", "row131"])
def test_resample_equals_the_restatement_and_its_output_is_binned(case):
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    name = case if case.startswith("row") else "grid"
    least, keep, empty = (0 if case == "thin_only" else 4), case == "seed_keep_outside", case == "all_new"
    most = 16 if name == "grid" else 5  # (the rows hold a mean of four per cell: a bound of 5 thins some of them)
    want = resampled(name, least, most, keep, empty)
    got, whole, ints, capacity = _resample_on_device(name, least, most, keep, empty)
    print(f"{case}: n_out {int(got[3])}, counts {got[4].tolist()}")
    _check_resampled(name, got, want, capacity)
    assert want["counts"][0] > 0 or empty
    assert all(bool((w[capacity:] == 7777.0).all()) for w in whole)
    n = want["n_out"]
    shape = solid_scene(name)["shape"]
    _, _, order, start, _ = F.binParticles([q[:n] for q in got[0]], [q[:n] for q in got[1]], shape)
    assert torch.equal(order, torch.arange(n, dtype=torch.int32, device="cuda")) and torch.equal(start, got[2])


@pytest.mark.gpu
def test_resample_into_a_capacity_too_small_writes_nothing_past_it():
    name = "grid"
    want = resampled(name, 4, 16, True)
    got, whole, ints, capacity = _resample_on_device(name, 4, 16, True, capacity=want["n_out"] - 1)
    assert got[4][3] == 1 and int(got[3]) == want["n_out"]
    _check_resampled(name, got, want, capacity)
    cells = int(np.prod(solid_scene(name)["shape"]))
    assert all(bool((w[capacity:] == 7777.0).all()) for w in whole)
    assert bool((ints[cells + 2:cells + 2 + 64] == -5).all()) and bool((ints[cells + 3 + 64:] == -5).all())


@pytest.mark.gpu
def test_resample_with_a_wrong_cell_start_stays_in_its_arrays():
    """entries beyond n and negative ones, on a tiny grid: the call returns, the guard regions are intact and the outputs are finite --
    only that"""
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    shape = (3, 5, 6)
    position, rng = TP._cloud(shape, 200, 0.0, 9)
    velocity = [rng.uniform(-1.0, 1.0, 200).astype(np.float32) for _ in range(3)]
    b = PR.bin_particles(position, velocity, shape)
    grid = [rng.uniform(-1.0, 1.0, AR.grid_shape(shape, a + 1)).astype(np.float32) for a in range(3)]
    phi = np.full(shape, -3.0, dtype=np.float32)
    for trial in range(3):
        wrong = rng.integers(-300, 500, len(b["cell_start"])).astype(np.int32)
        capacity, guard = 700, 64
        whole = [torch.full((capacity + guard,), 7777.0, device="cuda") for _ in range(6)]
        ints = torch.full((92 + guard + 1 + guard,), -5, dtype=torch.int32, device="cuda")
        out = ([w[:capacity] for w in whole[:3]], [w[:capacity] for w in whole[3:]], ints[:92], ints[92 + guard:93 + guard])
        F.resampleParticles(_dev3(b["position"]), _dev3(b["velocity"]), _dev(wrong), shape, capacity, 4, 8, _dev(phi), 1.0, 1.0, None, _dev3(grid), trial,
                            bool(trial % 2), out=out)
        torch.cuda.synchronize()
        assert all(bool((w[capacity:] == 7777.0).all()) and bool(torch.isfinite(w).all()) for w in whole)
        assert bool((ints[92:92 + guard] == -5).all()) and bool((ints[93 + guard:] == -5).all())


def _sample_cells(grid, pos):
    """S(grid)(x) of device particles, in torch fp64 (section 21's rule on the cell lattice)"""
    import torch

    gz, gy, gx = grid.shape
    g = grid.double()
    idx, t = [], []
    for c, size in enumerate((gx, gy, gz)):
        u = (pos[c].double() - 0.5).clamp(0.0, size - 1.0)
        i0 = u.floor().long().clamp(max=size - 1)
        idx.append((i0, (i0 + 1).clamp(max=size - 1)))
        t.append(u - i0)
    value = 0.0
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (t[0] if dx else 1 - t[0]) * (t[1] if dy else 1 - t[1]) * (t[2] if dz else 1 - t[2])
                value = value + w * g[idx[2][dz], idx[1][dy], idx[0][dx]]
    return value


@pytest.mark.gpu
def test_a_liquid_ball_falls_onto_a_rasterised_sphere_and_stays_out_of_it():
    """40^3; rasterizeBodies puts a sphere of radius 7 on the floor's centre; a liquid ball of radius 8 above it, seedParticles at 8 per
    cell, falls under gravity (added to the grid velocity by a torch op).  30 sub-steps of binParticles, resampleParticles (min 4,
    max 16), particlesToGrid, redistance, extrapolateVelocity, project_free_surface with the rasterised solid_phi and weights,
    extrapolateVelocity, updateParticlesSolid (margin 0.1, 2 iterations).  Every projection converges; after every sub-step no pushed
    particle is left inside the solid (counts[1] = 0) and no inside particle has S(solid_phi)(x) < -1e-6; after every resample every
    deep cell holds min .. max particles and n_out <= capacity.  The same run with updateParticles and without resample leaves
    particles deeper than half a cell in the solid: the scene tests something.  The curves are printed, not asserted (section 24)."""
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    shape, steps, dt, gravity, tolerance = (40, 40, 40), 30, 1.0, 0.06, 1e-5
    least, most, depth = 4, 16, 1.0
    solid_phi, cw, _ = F.rasterizeBodies(shape, [F.BodyShape.sphere((20.0, 20.0, 7.0), 7.0)], 3.0, 0.0)
    solid_host, cw_host = _host(solid_phi), [_host(w) for w in cw]
    x, s, _ = AR.targets(shape, 0)
    ball = (np.sqrt(((x - np.array([20.0, 20.0, 24.0])) ** 2).sum(axis=1)) - 8.0).reshape(s).astype(np.float32)
    curves = {}
    for solids in (True, False):
        pos = F.seedParticles(torch.from_numpy(ball).cuda(), per_cell=8, seed=7)
        n0 = pos[0].numel()
        capacity = 2 * n0
        vel = [torch.zeros(n0, device="cuda") for _ in range(3)]
        pressure = np.zeros(shape, dtype=np.float32)
        hit = torch.zeros(3, dtype=torch.int64, device="cuda")
        curve = []
        for step in range(steps):
            pos, vel, _, cell_start, counts = F.binParticles(pos, vel, shape)
            assert counts[0] == 0
            if solids:
                guess = F.particlesToGrid(pos, vel, cell_start, shape, 1.0)  # the liquid_phi and the velocity the new particles take
                liquid = F.redistance(guess[3], 3.0)
                F.extrapolateVelocity(guess[0], guess[2], 4)
                pos, vel, cell_start, n_out, rcounts = F.resampleParticles(pos, vel, cell_start, shape, capacity, least, most, liquid, 1.0, depth, solid_phi,
                                                                           guess[0], seed=step)
                n = int(n_out)
                assert n <= capacity and rcounts[3] == 0
                per = (cell_start[1:-1] - cell_start[:-2]).reshape(shape)
                deep = (liquid <= -depth) & (solid_phi > 0)
                assert int(deep.sum()) == rcounts[2] and bool((per[deep] >= least).all()) and bool((per <= most).all())
                pos, vel = [q[:n] for q in pos], [q[:n] for q in vel]
            grid, _, known, phi, _ = F.particlesToGrid(pos, vel, cell_start, shape, 1.0)
            phi = F.redistance(phi, 3.0)
            F.extrapolateVelocity(grid, known, 8)
            forced = [g.clone() for g in grid]
            forced[2] -= gravity
            velocity = [_host(g) for g in forced]
            valid, info = F.project_free_surface(_host(phi), solid_host, cw_host, velocity, pressure, tolerance=tolerance)
            assert info["outcome"] in (0, 1, 2), (step, info)
            projected = _dev3(velocity)
            F.extrapolateVelocity(projected, _dev3(valid), 8)
            if solids:
                hit.zero_()
                pos, vel = F.updateParticlesSolid(pos, vel, projected, dt, solid_phi, grid, 0.95, 2, None, 0.1, 2, 0.0, solid_counts=hit)
                assert hit[1] == 0, (step, hit.tolist())
            else:
                pos, vel = F.updateParticles(pos, vel, projected, dt, grid, 0.95, 2)
            at = _sample_cells(solid_phi, pos)
            curve.append((pos[0].numel(), int(hit[0]), int((at < 0).sum()), float(at.min())))
            if solids:
                assert float(at.min()) >= -1e-6, (step, float(at.min()))
        curves[solids] = curve
    print("with collision and resampling (particles, pushed, S(solid_phi) < 0, least S):", curves[True])
    print("with neither:", curves[False])
    assert max(c[1] for c in curves[True]) > 100  # the ball reached the sphere
    assert int((_sample_cells(solid_phi, pos) < -0.5).sum()) > 0  # (pos: the run with neither)
