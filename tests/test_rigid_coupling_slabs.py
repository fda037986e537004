"""Two-way rigid-body coupling on Z-slab ranks (include/mgps_fields.h, DESIGN.md section 17 "on slab ranks"): 1, 2 and 4 ranks share
the one device over TorchDistComm/gloo (tests/rigid_coupling_slab_worker.py, one process per rank, every launch with a timeout of
its own).

CPU: the two new entries refuse bad arguments on the host and the Python mirrors have the library's sizes; the premises of the solve
scene (the coupling's norm against the operator's, an empty rank at four ranks, wet faces whose liquid cell and body lie on
different ranks, a pressure the coupling changes).
GPU: the ranks' lists, apply, impulses and rigidVelocitySlab against the restatement and the whole-grid passes; a world of one
against the whole-grid object bit for bit, without a transport call; mgps_solve_pcg_coupled on slab solvers in the kinematic limit
and against the direct coupled solve; what it refuses; a transport whose all-reduce fails.

Tolerances: those of tests/test_rigid_coupling.py (stated there), on the same quantities.
  * apply: 2^-24 |y_ref| + 1e-10 sum |terms|; impulses against the whole-grid mgps_coupling_impulses: 1e-10 of the rows' magnitude (the
    sums of the ranks are added in another order than the workgroups of one device: the reordering bound of an fp64 sum).
  * rigidVelocitySlab: the bits of the whole-grid pass (the same fp64 expression on the same integers).
  * solve, tolerance 1e-7: pressure and V_out within 4 e0, e0 the error of the kinematic slab solve against the direct solve of A
    measured in the same run; V_out recomputed on the host from the gathered p: 1e-10; iterations at most 6 bodies + 2 more than
    kinematic; the all-reduces that carry more than one value number iterations + 3, the applications of the operator in a
    converged pcg64 solve (first residual, iterations + 1 passes of the loop, recomputed residual)."""
import ctypes as C
import functools
from functools import partial

import numpy as np
import pytest

import rigid_coupling_reference as RC
import rigid_coupling_slab_worker as W
import solid_forces_reference as R
from conftest import rel_l2
from slab_launch import run_workers as launch
from test_rigid_coupling import _desc, _oracles, _ptr, _refused

run_workers = partial(launch, "rigid_coupling_slab_worker.py")


# ---- CPU: the new entries refuse bad arguments on the host --------------------------------------------------------------------------
def _window(F, **kw):
    """rank 0 of two of a 4 x 4 x 32 grid (power-of-two expansion) and the desc that matches it"""
    lay = F.projection_slab_layout((32, 4, 4), True, 2, False)
    w = F.slab_window((32, 4, 4), True, lay["splits"], 0)
    ez, ey, ex = lay["expanded"]
    d, keep = _desc(gx=4, gy=4, gz=32, ex=ex, ey=ey, ez=ez, offset=lay["offset"], **kw)
    return w, d, keep


def _comm(Dd, **kw):
    cm = Dd.CommStruct()
    cm.struct_size, cm.rank, cm.size = C.sizeof(Dd.CommStruct), 0, 2
    keep = [Dd._EXCH(lambda *a: 1), Dd._ALLR(lambda *a: 1)]
    cm.exchange, cm.allreduce = keep
    for k, v in kw.items():
        setattr(cm, k, v)
    return cm, keep


def test_new_entries_refuse_on_the_host_and_the_mirrors_have_the_library_sizes():
    from geometricmultigridpressuresolver_amd import distributed as Dd
    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd._lib import lib

    L, h = lib(), C.c_void_p()
    assert hasattr(L, "mgps_coupling_create_slab") and hasattr(L, "mgps_fields_slab_rigid_velocity")
    cm, keep_cm = _comm(Dd)
    create = lambda d, w, c=cm: L.mgps_coupling_create_slab(C.byref(h), C.byref(d), C.byref(w) if w is not None else None,  # noqa: E731
                                                             C.byref(c) if c is not None else None, None)
    fn = "mgps_coupling_create_slab"
    # the mirrors' sizes are the library's: good structs get as far as the next check, one of another size is refused as such
    w, d, keep = _window(F, bodies=0)
    _refused(create(d, w), fn, "bodies", "1 .. 255")
    d.struct_size -= 4
    _refused(create(d, w), fn, "struct_size")
    _refused(L.mgps_coupling_create_slab(C.byref(h), None, C.byref(w), C.byref(cm), None), fn, "struct_size")
    w, d, keep = _window(F)
    w.struct_size -= 4
    _refused(create(d, w), fn, "not a slab window")
    _refused(create(d, None), fn, "not a slab window")
    w, d, keep = _window(F)
    short, keep_short = _comm(Dd, struct_size=8)
    _refused(create(d, w, short), fn, "comm", "exchange and allreduce")
    long, keep_long = _comm(Dd, struct_size=C.sizeof(Dd.CommStruct) + 8)
    _refused(create(d, w, long), fn, "comm")
    # what mgps_coupling_create refuses
    for bodies in (256, -1):
        _refused(create(_window(F, bodies=bodies)[1], w), fn, "bodies")
    _refused(create(_window(F, material=None)[1], w), fn, "material")
    for name, word in (("cut_weights", "cut weights"), ("body", "body")):
        d1 = _window(F)[1]
        getattr(d1, name)[2] = None
        _refused(create(d1, w), fn, word)
    for name in ("centres", "inv_mass", "inv_inertia"):
        _refused(create(_window(F, **{name: None})[1], w), fn, name)
    w, d, keep = _window(F)
    keep[1][2] = -1e-3
    _refused(create(d, w), fn, "inv_mass", "body 2", "negative")
    keep[1][2] = 1.0
    # a window that does not match the desc
    for k in ("gx", "gz", "ex", "ez", "offset"):
        w1, d1, keep1 = _window(F)
        setattr(d1, k, getattr(d1, k) + (2 if k in ("ex", "ez") else 1 if k != "offset" else -1))
        _refused(create(d1, w1), fn, "window does not match the desc")
    w1 = _window(F)[0]
    w1.c1 += 1  # not the base planes of [e0, e1)
    _refused(create(d, w1), fn, "not a slab window")
    # a comm without exchange / allreduce, or none
    _refused(create(d, w, None), fn, "comm")
    _refused(create(d, w, _comm(Dd, exchange=Dd._EXCH())[0]), fn, "exchange and allreduce")
    _refused(create(d, w, _comm(Dd, allreduce=Dd._ALLR())[0]), fn, "exchange and allreduce")
    _refused(create(d, w, _comm(Dd, rank=2)[0]), fn, "comm")
    assert not h.value
    # mgps_fields_slab_rigid_velocity
    fn = "mgps_fields_slab_rigid_velocity"
    rigid = L.mgps_fields_slab_rigid_velocity
    p3, t = (C.c_void_p * 3)(64, 64, 64), np.zeros(24)
    hole = (C.c_void_p * 3)(64, None, 64)
    for bodies in (0, 256):
        _refused(rigid(C.byref(w), p3, p3, _ptr(t), _ptr(t), bodies, None), fn, "bodies")
    _refused(rigid(None, p3, p3, _ptr(t), _ptr(t), 3, None), fn, "not a slab window")
    _refused(rigid(C.byref(w1), p3, p3, _ptr(t), _ptr(t), 3, None), fn, "not a slab window")
    _refused(rigid(C.byref(w), hole, p3, _ptr(t), _ptr(t), 3, None), fn, "solid velocity")
    _refused(rigid(C.byref(w), None, p3, _ptr(t), _ptr(t), 3, None), fn, "solid velocity")
    _refused(rigid(C.byref(w), p3, hole, _ptr(t), _ptr(t), 3, None), fn, "body")
    _refused(rigid(C.byref(w), p3, p3, None, _ptr(t), 3, None), fn, "centres")
    _refused(rigid(C.byref(w), p3, p3, _ptr(t), None, 3, None), fn, "motions")
    del keep_cm, keep_short, keep_long


# ---- scene B: the direct solves, once per test process ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_b_case():
    """scene B with the oracle's expanded domain of the tight expansion (weights rounded to float32: the operator the device holds)
    and the two direct solves (coupled, kinematic): tests/test_rigid_coupling.py::solve_case on this scene"""
    from geometricmultigridpressuresolver_amd import fields as F

    d = dict(W.scene_b())
    fo, orc = _oracles()
    shape = d["shape"]
    d["material"] = fo.material_labels(d["liquid_phi"], d["solid_phi"], d["cut_weights"]).astype(np.int32)
    assert ((d["material"] == 0) == (d["owner"] > 0)).all()
    lay = F.projection_slab_layout(shape, False, 1, False)
    eshape, offset = lay["expanded"], lay["offset"]
    valid = fo.valid_faces(d["material"], d["cut_weights"])
    lab = fo.domain_labels(d["material"], eshape, offset)
    w = fo.boundary_weights(d["cut_weights"], d["liquid_phi"], valid, d["material"], eshape, offset)
    w32 = [a.astype(np.float32) for a in w]
    orc.set_boundary_labels(lab, [a.astype(np.float64) for a in w32])
    ref = RC.Scene(d["material"], d["cut_weights"], d["body"], d["centres"], lab, w32, offset)
    b_fluid = ref.unknowns(fo.rhs(d["material"], d["velocity"], d["cut_weights"], eshape, offset, None))
    p, v_out, b = ref.solve(b_fluid, d["inv_mass"], d["inv_inertia"], d["motions"])
    p0, v0, b0 = ref.solve(b_fluid, 0 * d["inv_mass"], 0 * d["inv_inertia"], d["motions"])
    assert np.array_equal(b, b0) and np.array_equal(v0, d["motions"])
    d.update(eshape=eshape, offset=offset, levels=lay["levels"], labels=lab.astype(np.uint8), w32=w32, ref=ref, p=p, p0=p0, v_out=v_out,
             mask=RC.coupled_mask(d["material"], d["cut_weights"], d["body"], d["bodies"]))
    return d


@pytest.fixture(scope="module")
def reference_file(tmp_path_factory):
    """what the solve and refusal workers load: the domain and the direct solves of scene B"""
    c = scene_b_case()
    path = str(tmp_path_factory.mktemp("rigid_slabs") / "scene_b.npz")
    np.savez(path, labels=c["labels"], wx=c["w32"][0], wy=c["w32"][1], wz=c["w32"][2], active=c["ref"].active, material=c["material"],
             offset=c["offset"], p=c["p"], p0=c["p0"], v_out=c["v_out"])
    return {"MGPS_RC_SLAB_REF": path}


def test_solve_scene_premises():
    """scene B: |G K G^T|_2 <= 0.05 lambda_max(A) (the premise of the 4 e0 bound), an empty rank at four ranks, wet z-faces on a cut
    whose liquid cell and body lie on different ranks, and a pressure the coupling changes"""
    import scipy.sparse.linalg as spla

    from geometricmultigridpressuresolver_amd import fields as F

    c = scene_b_case()
    shape, mat, mask = c["shape"], c["material"], c["mask"]
    G, K = c["ref"].G, RC.stiffness(c["inv_mass"], c["inv_inertia"]).toarray()
    norm = np.abs(np.linalg.eigvals(K @ (G.T @ G).toarray())).max()
    top = float(spla.eigsh(c["ref"].A, k=1, which="LA", return_eigenvectors=False)[0])
    counts = {}
    for size in (2, 4):
        lay = F.projection_slab_layout(shape, False, size, False)
        assert lay["expanded"] == c["eshape"] and lay["offset"] == c["offset"] and W.base_cuts(lay["splits"], lay["offset"], shape[0]) == W.BASE_CUTS[size], lay
        counts[size] = W.rank_counts(mask, lay["splits"], lay["offset"])
    # wet z-faces of a body exactly on cut 24: the body's cell lies below the cut, the LIQUID cell that owns the face above it
    on_cut = (c["cut_weights"][2][24] < 1) & (c["body"][2][24] > 0) & (mat[24] == R.LIQUID) & (c["owner"][23] > 0)
    change = rel_l2(c["p"], c["p0"])
    print(f"scene B: {int(mask.sum())} coupled cells, per rank {counts}; {int(on_cut.sum())} wet z-faces on cut 24 with the body below and the liquid "
          f"cell above; |G K G^T|_2 = {norm:.4f}, lambda_max(A) = {top:.3f}, ratio {norm / top:.4f} (bound 0.05); coupled against kinematic "
          f"pressure {change:.2f} relative")
    assert 0 < norm <= 0.05 * top
    assert sum(counts[4]) == sum(counts[2]) == int(mask.sum()) > 1200
    assert 0 in counts[4] and sum(n > 0 for n in counts[4]) >= 3 and min(counts[2]) > 0
    assert int(on_cut.sum()) > 0
    assert change > 1e-3


def test_apply_scene_premises():
    """scene A: a cell belongs to one rank, four ranks leave one list empty, and every interior cut that has liquid carries
    fractional z-faces between two LIQUID cells"""
    from geometricmultigridpressuresolver_amd import fields as F

    sc = W.scene_a()
    shape = sc["shape"]
    mat = _oracles()[0].material_labels(sc["liquid_phi"], sc["solid_phi"], sc["cut_weights"]).astype(np.int32)
    mask = RC.coupled_mask(mat, sc["cut_weights"], sc["body"], sc["bodies"])
    out = {}
    for size in (2, 4):
        for p2 in (True, False):
            lay = F.projection_slab_layout(shape, p2, size, False)
            assert W.base_cuts(lay["splits"], lay["offset"], shape[0]) == W.BASE_CUTS[size], (size, p2, lay)
            out[size] = W.rank_counts(mask, lay["splits"], lay["offset"])
    frac = {k: W.fractional_liquid_faces(mat, sc, k) for k in W.CUT_PLANES}
    print(f"scene A: {int(mask.sum())} coupled cells, per rank {out}; fractional owned z-faces between two LIQUID cells on the cut planes {frac}")
    assert sum(out[4]) == sum(out[2]) == int(mask.sum()) > 3 * 256 and 0 in out[4] and min(out[2]) > 0
    for k in W.CUT_PLANES:
        assert frac[k] > 0 or not ((mat[k - 1] == R.LIQUID) | (mat[k] == R.LIQUID)).any(), k
    assert frac[8] > 0 and frac[24] > 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 4])
def test_slab_apply_impulses_and_rigid_velocity_match_the_whole_grid(nproc):
    print(run_workers("apply", nproc, 300)[-4000:])


@pytest.mark.gpu
def test_one_rank_is_bit_equal_to_the_whole_grid_object_without_a_transport_call():
    print(run_workers("one", 1, 300)[-2000:])


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 4])
def test_slab_coupled_solve_matches_the_direct_solve(nproc, reference_file):
    print(run_workers("solve", nproc, 300, extra_env=reference_file)[-4000:])


@pytest.mark.gpu
def test_refusals_on_the_device(reference_file):
    print(run_workers("refusals", 1, 300, extra_env=reference_file)[-2000:])


@pytest.mark.gpu
def test_failing_allreduce_returns_comm_error_without_hanging():
    print(run_workers("fail", 2, 120)[-2000:])
