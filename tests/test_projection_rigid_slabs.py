"""The one-call projection with rigid bodies on slab ranks and on one device: mgps_project_free_surface_rigid_slab
(include/mgps_fields.h).  1, 2 and 4 ranks share the one device over TorchDistComm/gloo
(tests/projection_rigid_slab_worker.py, one process per rank, every launch with a timeout of its own).

CPU: what the entry refuses before any collective, on the host (pointer values of 64 are never dereferenced); the Python mirror has
the library's size; the structs of the entries this one leaves alone keep theirs.
GPU, one rank over a transport whose every entry fails: the kinematic anchor (K = 0 is the plain one-call on rigidVelocitySlab(V*),
bit for bit, with and without surface tension), real K against project_free_surface_rigid, a warm start, an interrupt.
GPU, two and four ranks: the anchor and real K on every rank's window, one report on every rank, equal copies of the cuts' z-face
planes, the ranks' counts; scene A (fractional z-face weights on the cuts) at two ranks; failures at two ranks.

Tolerances (the project's rules for the same quantities, stated with the tests that introduced them):
  * against project_free_surface_rigid: tests/projection_slab_worker.py::check_against_single -- flags equal, iterations +- 1,
    pressure 1e-4 relative L2, velocity 1e-6 max(1, max |u|);
  * motions_out against V* - K G^T p formed on the host in fp64 from the published pressure, impulses against solidForces on it:
    1e-10 (tests/test_rigid_coupling_slabs.py: the reordering bound of an fp64 sum);
  * solid_velocity_out: the bits of rigidVelocity(base, motions_out); divergence_max against computeResultingDivergence on the
    published fields: 1e-5 relative (tests/projection_slab_worker.py::passes_mode);
  * divergence_max at most 4 x what the plain one-call leaves with the bodies kinematic, and more than 100 x smaller than the
    divergence against rigidVelocity(V*) (tests/test_rigid_coupling.py, end to end);
  * interrupt: the pressure within 1 ulp of the call truncated at stats.iterations (tests/test_pcg_exits.py)."""
import ctypes as C
from functools import partial

import numpy as np
import pytest

from slab_launch import run_workers as launch
from test_rigid_coupling import _refused

run_workers = partial(launch, "projection_rigid_slab_worker.py")
FN = "mgps_project_free_surface_rigid_slab"
SHAPE = (32, 4, 4)  # (gz, gy, gx) of the host-side refusals


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def _comm(Dd, size=2, **kw):
    cm = Dd.CommStruct()
    cm.struct_size, cm.rank, cm.size = C.sizeof(Dd.CommStruct), 0, size
    keep = [Dd._EXCH(lambda *a: 1), Dd._ALLR(lambda *a: 1), Dd._GATHV(lambda *a: 1), Dd._SCATV(lambda *a: 1)]
    cm.exchange, cm.allreduce, cm.gatherv, cm.scatterv = keep
    for k, v in kw.items():
        setattr(cm, k, v)
    return cm, keep


def _call(F, L, cm, splits=None, edit=None, tables=None):
    """one call on structs that are good but for what `edit(rigid, projection, tables)` changes; nothing is dereferenced"""
    lay = F.projection_slab_layout(SHAPE, True, cm.size, False)
    pr = F.ProjectionSlab()
    pr.struct_size = C.sizeof(F.ProjectionSlab)
    pr.gz, pr.gy, pr.gx = SHAPE
    pr.power_of_two = 1
    pr.liquid_phi = pr.solid_phi = pr.pressure = 64
    for a in range(3):
        pr.cut_weights[a] = pr.velocity[a] = 64
    t = tables or dict(centres=np.zeros((4, 3)), inv_mass=np.ones(4), inv_inertia=np.ones((4, 6)), motions=np.zeros((4, 6)), motions_out=np.zeros((4, 6)))
    rg = F.ProjectionRigidSlab()
    rg.struct_size = C.sizeof(F.ProjectionRigidSlab)
    rg.projection = C.pointer(pr)
    rg.bodies = 3
    for a in range(3):
        rg.body[a] = 64
    for k, v in t.items():
        setattr(rg, k, v.ctypes.data)
    if edit is not None:
        edit(rg, pr, t)
    cuts = splits if splits is not None else lay["splits"]
    return L.mgps_project_free_surface_rigid_slab(C.byref(rg), None, C.byref(cm) if cm is not None else None, (C.c_int * len(cuts))(*cuts), None)


def test_entry_refuses_on_the_host_before_any_collective():
    from geometricmultigridpressuresolver_amd import distributed as Dd
    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd._lib import lib

    L = lib()
    assert hasattr(L, FN)
    cm, keep = _comm(Dd)
    call = partial(_call, F, L, cm)
    # NULL or a struct_size mismatch, of either struct
    _refused(L.mgps_project_free_surface_rigid_slab(None, None, C.byref(cm), (C.c_int * 3)(0, 32, 64), None), FN, "struct_size")
    _refused(call(edit=lambda rg, pr, t: setattr(rg, "struct_size", rg.struct_size - 8)), FN, "struct_size")
    _refused(call(edit=lambda rg, pr, t: setattr(rg, "projection", None)), FN, "struct_size")
    _refused(call(edit=lambda rg, pr, t: setattr(pr, "struct_size", pr.struct_size - 8)), FN, "struct_size")
    # the transport checks of the plain call
    lay = F.projection_slab_layout(SHAPE, True, 2, False)
    rigid = L.mgps_project_free_surface_rigid_slab
    _refused(_call(F, L, _comm(Dd, exchange=Dd._EXCH())[0]), FN, "comm / splits")
    _refused(_call(F, L, _comm(Dd, allreduce=Dd._ALLR())[0]), FN, "comm / splits")
    _refused(_call(F, L, _comm(Dd, rank=2)[0]), FN, "comm / splits")
    _refused(_call(F, L, _comm(Dd, struct_size=8)[0]), FN, "comm / splits")
    _refused(_call(F, L, _comm(Dd, gatherv=Dd._GATHV())[0]), FN, "gatherv")
    good = F.ProjectionRigidSlab()
    good.struct_size = C.sizeof(F.ProjectionRigidSlab)
    pr = F.ProjectionSlab()
    pr.struct_size = C.sizeof(F.ProjectionSlab)
    good.projection = C.pointer(pr)
    _refused(rigid(C.byref(good), None, None, (C.c_int * 3)(*lay["splits"]), None), FN, "comm / splits")
    _refused(rigid(C.byref(good), None, C.byref(cm), None, None), FN, "comm / splits")
    # bodies outside 1 .. 255
    for bodies in (0, 256, -1):
        _refused(call(edit=lambda rg, pr, t, b=bodies: setattr(rg, "bodies", b)), FN, "bodies", "1 .. 255")
    # a NULL table
    for name in ("centres", "inv_mass", "inv_inertia"):
        _refused(call(edit=lambda rg, pr, t, n=name: setattr(rg, n, None)), FN, name, "NULL")

    # a negative or non-finite inv_mass, a bad diagonal entry of inv_inertia: the texts of the coupling's constructor
    def spoil(name, index, value):
        def edit(rg, pr, t):
            t[name][index] = value
        return edit

    _refused(call(edit=spoil("inv_mass", 2, -1e-3)), FN, "inv_mass", "body 2", "negative")
    _refused(call(edit=spoil("inv_mass", 1, np.inf)), FN, "inv_mass", "body 1", "not finite")
    _refused(call(edit=spoil("inv_inertia", (3, 1), -1.0)), FN, "inv_inertia", "body 3", "negative diagonal")
    _refused(call(edit=spoil("inv_inertia", (2, 4), np.nan)), FN, "inv_inertia", "body 2", "not finite")
    # NULL motions or motions_out, solid_velocity_out partly set
    _refused(call(edit=lambda rg, pr, t: setattr(rg, "motions", None)), FN, "motions is NULL")
    _refused(call(edit=lambda rg, pr, t: setattr(rg, "motions_out", None)), FN, "motions_out is NULL")

    def partly(rg, pr, t):
        rg.solid_velocity_out[0] = rg.solid_velocity_out[2] = 64

    _refused(call(edit=partly), FN, "solid_velocity_out", "all three or none")
    del keep


def test_mirror_has_the_library_size_and_the_other_structs_keep_theirs():
    from geometricmultigridpressuresolver_amd import _lib
    from geometricmultigridpressuresolver_amd import distributed as Dd
    from geometricmultigridpressuresolver_amd import fields as F

    L = _lib.lib()
    cm, keep = _comm(Dd)
    # a good struct gets as far as the layout check; one 8 bytes short is refused as such
    _refused(_call(F, L, cm, splits=[0, 16, 40]), "mgps_fields_slab_describe", "the cuts must run from 0")
    _refused(_call(F, L, cm, edit=lambda rg, pr, t: setattr(rg, "struct_size", rg.struct_size - 8)), FN, "struct_size", "mgps_projection_rigid_slab")
    assert C.sizeof(F.ProjectionRigidSlab) == 136
    # the entries this one leaves alone: the sizes before it
    sizes = (C.sizeof(_lib.Options), C.sizeof(F.Projection), C.sizeof(Dd.CommStruct), C.sizeof(F.ProjectionSlab), C.sizeof(F.CouplingDesc))
    assert sizes == (96, 368, 96, 424, 120), sizes
    del keep


# ---- GPU, one rank: a transport whose every entry fails -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_rank_kinematic_anchor_is_the_plain_one_call_bit_for_bit():
    print(run_workers("one_anchor", 1, 240)[-3000:])


@pytest.mark.gpu
def test_one_rank_real_k_matches_the_composed_projection_and_warm_starts():
    print(run_workers("one_real", 1, 240)[-3000:])


@pytest.mark.gpu
def test_one_rank_interrupt_publishes_the_iterate_handed_back():
    print(run_workers("one_interrupt", 1, 240)[-3000:])


# ---- GPU, two and four ranks over gloo -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 4])
def test_ranks_anchor_and_real_k_on_every_window(nproc):
    print(run_workers("ranks", nproc, 300)[-4000:])


@pytest.mark.gpu
def test_scene_a_fractional_cut_faces_at_two_ranks():
    print(run_workers("scene_a", 2, 300)[-3000:])


@pytest.mark.gpu
def test_failures_at_two_ranks():
    print(run_workers("fail", 2, 240)[-3000:])
